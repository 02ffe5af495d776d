"""The cases of the NLSPN refinement stage and the DCNv2 operator under it (include/ddepth_dcn.h, csrc/dd_dcn.hip) AT THE PLACES WHERE THE KERNELS
BRANCH, shared by tests/test_nlspn_cases_host_emulation.py (the kernels' source on the CPU) and tests/test_zz_gpu_nlspn_cases.py (the built
library): shapes, seeded NumPy inputs, the fp64 oracle (oracle/dcn_oracle.py), pure index-arithmetic expectations for the exact cases, the
conditions a case must meet to reach the branch it is for (computed here from index arithmetic, never through a kernel), and the checks, which
take ``run_*`` callables on NumPy arrays.  Nothing is imported from diffusiondepth_amd.

What the shapes are for (csrc/dd_dcn.hip: launch_prop, nlspn_prop_lds_kernel): the default propagation kernel stages a 16 x 64 tile plus an
8-pixel halo in LDS and hands every sample whose 2 x 2 cell leaves that window to another sampler (sample_pair; sample_plane when W < 2).
MAIN = (2, 37, 150) has three tile columns and three tile rows with last tiles 22 wide and 5 high; offsets of 6 N(0, 1) put a few per cent of
the in-image samples outside the window and carry samples over every tile seam in both directions; the edge shapes are one pixel, one row, one
column (W = 1: the only default route to the four-load sampler), a last tile one column and one row wide, and exactly one tile.

Bounds.  Propagation: every iteration's map within 1e-5 x max|oracle's map of that iteration| (the TOL of tests/test_zz_gpu_nlspn.py; the
operation and the arithmetic are the same and the oracle forms the sampling positions in fp32 exactly as the kernels do, so floor() picks the
same cell).  Exact cases: bit-equal.  Affinity stage: offset 2e-5 / aff 1e-5 absolute, guided 5e-5 / 2e-5 (the golden and oracle tests of
tests/test_library_host_emulation.py).  DCNv2: 1e-5 of the largest magnitude of the compared tensor."""
import functools

import numpy as np

from oracle import dcn_oracle as O

TOL = 1e-5
T = 3                                   # both workspace halves and the final no-blend branch of dd_nlspn_propagate
SENTINEL = np.float32(-12345.678)
GUARD = 16                              # sentinel elements in front of and behind every output (64 bytes: 16-byte alignment stays)
MAIN = (2, 37, 150)
EDGES = ((1, 1, 1), (1, 1, 2), (1, 3, 1), (1, 17, 65), (2, 16, 64))
KFS = (3, 5, 7)
PROP_BIAS = np.float32(0.37)
VARIANT_SHAPE = (1, 37, 152)            # W % 4 == 0: the four-pixels-per-lane kernel (g4) is eligible
VARIANTS = ("g1", "g1p", "g4", "g4p", "l8", "l8p", "l16", "l16p", "l32", "l32p", "l16q", "l16pq", "l8pq", "l32q")
VARIANTS_K57 = ("g1p", "l8p", "l32")
MODES = {"AS": 0, "ASS": 1, "TC": 2, "TGASS": 3}
AFF_SHAPES = ((2, 9, 70), (1, 1, 1))
GUIDED_SHAPES = ((2, 9, 70), (1, 1, 1), (1, 8, 64), (1, 17, 65))
W_CONF, B_CONF = np.float32(0.7), np.float32(0.25)
# the default kernel's LDS window (nlspn_prop_lds_kernel<KF, 16, PAIR>): tile rows, tile columns, halo
LDS_TH, LDS_TW, LDS_R = 16, 64, 8


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def sid(shape):
    return "x".join(str(v) for v in shape)


def prop_shapes(k_f):
    return (MAIN,) + EDGES if k_f == 3 else ((1,) + MAIN[1:], (1, 1, 1), (1, 17, 65))


def prop_cases():
    return [(k_f, s, p) for k_f in KFS for s in prop_shapes(k_f) for p in (0, 1)]


def exact_cases():
    return [(k_f, s, p) for k_f in KFS for s in (MAIN, (1, 17, 65)) for p in (0, 1)]


def variant_cases():
    return [(v, 3) for v in VARIANTS] + [(v, k) for k in (5, 7) for v in VARIANTS_K57]


def case_id(c):
    return "-".join(sid(v) if isinstance(v, tuple) else str(v) for v in c)


def _seed(tag, k_f, shape):
    B, H, W = shape
    return 100000 * tag + 10000 * k_f + 3001 * B + 101 * H + W


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- index arithmetic: where every tap of every pixel samples, and what the default kernel's window holds of it ---------------------------------
def tap_geometry(offset, k_f):
    """offset [B, 2 K, H, W] -> hs, ws (fp32 sampling positions, formed as the kernels form them: the integer base converted to float plus the
    fp32 offset), fh, fw (floor cell, int64), inside (the range test -1 < h < H, -1 < w < W), each [B, K, H, W]."""
    B, K2, H, W = offset.shape
    K, pad = k_f * k_f, (k_f - 1) // 2
    assert K2 == 2 * K
    k = np.arange(K)
    hb = (np.arange(H)[None, :, None] - pad + (k // k_f)[:, None, None]).astype(np.float32)
    wb = (np.arange(W)[None, None, :] - pad + (k % k_f)[:, None, None]).astype(np.float32)
    hs = (hb[None] + offset[:, 0::2]).astype(np.float32)
    ws = (wb[None] + offset[:, 1::2]).astype(np.float32)
    inside = (hs > -1) & (ws > -1) & (hs < H) & (ws < W)
    return hs, ws, np.floor(hs).astype(np.int64), np.floor(ws).astype(np.int64), inside


def window_stats(offset, k_f, th=LDS_TH, tw=LDS_TW, r=LDS_R):
    """-> dict: ``fallback_share`` = share of all taps whose 2 x 2 cell is not inside the (th + 2 r) x (tw + 2 r) LDS window of the pixel's tile
    while the sample is inside the image (those take the fallback sampler and contribute a value); ``seams`` = {(axis, seam, direction):
    (taps served from the window, taps served by the fallback)} counting in-image samples of a pixel on one side of the tile seam whose whole
    cell lies on the other side."""
    B, _, H, W = offset.shape
    hs, ws, fh, fw, inside = tap_geometry(offset, k_f)
    ph, pw = np.arange(H)[None, None, :, None], np.arange(W)[None, None, None, :]
    ly, lx = fh - (ph // th * th - r), fw - (pw // tw * tw - r)
    in_win = (ly >= 0) & (ly < th + 2 * r - 1) & (lx >= 0) & (lx < tw + 2 * r - 1)
    seams = {}
    for s in range(tw, W, tw):
        seams[("x", s, "+")] = inside & (pw < s) & (fw >= s)
        seams[("x", s, "-")] = inside & (pw >= s) & (fw + 1 < s)
    for s in range(th, H, th):
        seams[("y", s, "+")] = inside & (ph < s) & (fh >= s)
        seams[("y", s, "-")] = inside & (ph >= s) & (fh + 1 < s)
    return dict(fallback_share=float((~in_win & inside).mean()), in_image_share=float(inside.mean()),
                seams={k: (int((v & in_win).sum()), int((v & ~in_win).sum())) for k, v in seams.items()})


def check_prop_conditions(k_f):
    """The main shape reaches what it is for: at least 1 % of all taps take the fallback sampler with a sample inside the image, and every tile
    seam is crossed in both directions, through the halo of the window and through the fallback."""
    shape = prop_shapes(k_f)[0]
    st = window_stats(prop_inputs(k_f, shape)[1], k_f)
    print(f"k_f {k_f} {sid(shape)}: fallback share {st['fallback_share']:.4f}, in-image share {st['in_image_share']:.4f}, seams {st['seams']}")
    assert st["fallback_share"] >= 0.01, st
    assert set(st["seams"]) == {(a, s, d) for a, ss in (("x", (64, 128)), ("y", (16, 32))) for s in ss for d in "+-"}
    for key, (halo, fallback) in st["seams"].items():
        assert halo > 0 and fallback > 0, (key, halo, fallback)
    # ... which a 3x3 case of at most 20 x 28 with |offset| < 5.7 (the largest of the golden and oracle cases) cannot do: one tile column, and
    # the second tile row's window still covers every cell such an offset reaches
    small = np.random.RandomState(1).uniform(-5.7, 5.7, (1, 18, 20, 28)).astype(np.float32)
    assert window_stats(small, 3)["fallback_share"] == 0.0


# ---- propagation: real-valued cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prop_inputs(k_f, shape):
    """feat U(0, 10); offsets 6 N(0, 1); affinities 0.1 N(0, 1) with the centre tap 1 - sum(others); w N(0, 1), not symmetric; b 0.37; feat_fix
    positive on 5 % of the pixels.  -> (feat, offset, aff, fix, w, b), read-only."""
    B, H, W = shape
    K = k_f * k_f
    rs = np.random.RandomState(_seed(1, k_f, shape))
    feat = rs.uniform(0, 10, (B, 1, H, W)).astype(np.float32)
    offset = (6.0 * rs.standard_normal((B, 2 * K, H, W))).astype(np.float32)
    aff = (0.1 * rs.standard_normal((B, K, H, W))).astype(np.float32)
    aff[:, K // 2] = 1.0 - (aff.sum(axis=1) - aff[:, K // 2])
    w = rs.standard_normal(K).astype(np.float32)
    assert np.abs(w.reshape(k_f, k_f) - w.reshape(k_f, k_f).T).max() > 0.1
    fix = np.where(rs.uniform(size=(B, 1, H, W)) < 0.05, rs.uniform(1, 20, (B, 1, H, W)), 0.0).astype(np.float32)
    return _ro(feat, offset, aff, fix, w, np.full(1, PROP_BIAS, np.float32))


@functools.lru_cache(maxsize=None)
def prop_oracle(k_f, shape, preserve):
    feat, offset, aff, fix, w, b = prop_inputs(k_f, shape)
    _, feats = O.nlspn_propagate(feat, offset, aff, fix if preserve else None, T, bool(preserve), k_f, w=w, b=b[0])
    return _ro(np.stack(feats))[0]


def check_prop_real(run_prop, k_f, shape, preserve, record=None, where="", tag="default"):
    """run_prop(feat, offset, aff, fix or None, w, b, k_f, prop_time, preserve) -> [T, B, 1, H, W] fp32.  -> what it returned."""
    feat, offset, aff, fix, w, b = prop_inputs(k_f, shape)
    want = prop_oracle(k_f, shape, preserve)
    got = run_prop(feat, offset, aff, fix if preserve else None, w, b, k_f, T, preserve)
    assert got.shape == want.shape and got.dtype == np.float32
    errs = [float(np.abs(got[it].astype(np.float64) - want[it]).max() / np.abs(want[it]).max()) for it in range(T)]
    print(f"{where} propagate {tag} k_f {k_f} {sid(shape)} preserve {preserve}: rel err per iteration {['%.2e' % e for e in errs]}")
    if record is not None:
        record("nlspn_cases_propagate", where=where, kernel=tag, k_f=k_f, shape=sid(shape), preserve=preserve, err=max(errs))
    assert np.isfinite(got).all()
    assert max(errs) <= TOL, (k_f, shape, preserve, errs)
    return got


# ---- propagation: exact cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_inputs(k_f, shape):
    """Integer offsets in [-12, 12] (beyond the 8-pixel halo), affinities one-hot per pixel on a seeded tap, w = 1, b = 0, feat and the 5 % of
    positive feat_fix integers in 1..15: every product and sum is exact, so the result is a gather.  -> (feat, offset, aff, fix, w, b, tap)."""
    B, H, W = shape
    K = k_f * k_f
    rs = np.random.RandomState(_seed(2, k_f, shape))
    feat = rs.randint(1, 16, (B, 1, H, W)).astype(np.float32)
    offset = rs.randint(-12, 13, (B, 2 * K, H, W)).astype(np.float32)
    tap = rs.randint(0, K, (B, H, W))
    aff = (np.arange(K)[None, :, None, None] == tap[:, None]).astype(np.float32)
    fix = np.where(rs.uniform(size=(B, 1, H, W)) < 0.05, rs.randint(1, 16, (B, 1, H, W)), 0).astype(np.float32)
    return _ro(feat, offset, aff, fix, np.ones(K, np.float32), np.zeros(1, np.float32), tap)


def exact_expected(k_f, shape, preserve):
    """Index arithmetic only: out[b, y, x] = in[b, y + i - pad + offset_h, x + j - pad + offset_w] for the pixel's tap (i, j) where that lies in
    the image, +0 elsewhere; ``in`` is the previous map with feat_fix written over it where that is positive (preserve_input)."""
    feat, offset, aff, fix, _, _, tap = exact_inputs(k_f, shape)
    B, H, W = shape
    pad = (k_f - 1) // 2
    bb, yy, xx = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    sy = yy + tap // k_f - pad + offset[bb, 2 * tap, yy, xx].astype(np.int64)
    sx = xx + tap % k_f - pad + offset[bb, 2 * tap + 1, yy, xx].astype(np.int64)
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    cur, maps = feat[:, 0], []
    for _ in range(T):
        if preserve:
            cur = np.where(fix[:, 0] > 0, fix[:, 0], cur)
        cur = np.where(ok, cur[bb, sy.clip(0, H - 1), sx.clip(0, W - 1)], np.float32(0.0)).astype(np.float32)
        maps.append(cur[:, None])
    return np.stack(maps)


def check_prop_exact(run_prop, k_f, shape, preserve, tag="default"):
    feat, offset, aff, fix, w, b, _ = exact_inputs(k_f, shape)
    want = exact_expected(k_f, shape, preserve)
    assert len(np.unique(want[-1])) > 8 and (want == 0).any()          # a gather of many values, some from outside the image
    got = run_prop(feat, offset, aff, fix if preserve else None, w, b, k_f, T, preserve)
    assert got.shape == want.shape
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{tag} k_f {k_f} {sid(shape)} preserve {preserve}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"
    return got


def check_variant(run_prop, set_variant, variant, k_f, record=None, where=""):
    """set_variant(name or None) selects the kernel for the following calls (DD_NLSPN_KERNEL, read per call).  The variant is held to the oracle
    and to the exact expectation like the default; its largest difference from the default is recorded, not asserted."""
    feat, offset, aff, fix, w, b = prop_inputs(k_f, VARIANT_SHAPE)
    set_variant(None)
    base = run_prop(feat, offset, aff, fix, w, b, k_f, T, 1)          # the default is held to the oracle by its own tests, not here
    set_variant(variant)
    got = check_prop_real(run_prop, k_f, VARIANT_SHAPE, 1, record=record, where=where, tag=variant)
    diff = float(np.abs(got.astype(np.float64) - base).max())
    print(f"{where} {variant} k_f {k_f}: max |variant - default| {diff:.3e}")
    if record is not None:
        record("nlspn_cases_variant_vs_default", where=where, kernel=variant, k_f=k_f, max_abs_diff=diff)
    if k_f == 3:
        for preserve in (0, 1):
            check_prop_exact(run_prop, k_f, VARIANT_SHAPE, preserve, tag=variant)


# ---- the affinity stage -----------------------------------------------------------------------------------------------------------------------------
def affinity_grid(kfs=KFS):
    return [(k_f, m, c, l) for k_f in kfs for m in MODES for c in (0, 1) for l in (0, 1)]


@functools.lru_cache(maxsize=None)
def affinity_inputs(k_f, shape):
    """raw: offsets 3 N(0, 1) (confidence samples leave the image), affinity logits N(0, 1); confidence U(0, 1); gamma = 0.5 num."""
    B, H, W = shape
    num = k_f * k_f - 1
    rs = np.random.RandomState(_seed(3, k_f, shape))
    raw = rs.standard_normal((B, 3 * num, H, W))
    raw[:, :2 * num] *= 3.0
    conf = rs.uniform(0, 1, (B, 1, H, W)).astype(np.float32)
    return _ro(raw.astype(np.float32), conf, np.full(1, 0.5 * num, np.float32), np.full(1, W_CONF, np.float32), np.full(1, B_CONF, np.float32))


@functools.lru_cache(maxsize=None)
def affinity_oracle(k_f, shape, mode, conf_prop, legacy):
    raw, conf, gamma, w_conf, b_conf = affinity_inputs(k_f, shape)
    return _ro(*O.nlspn_offset_affinity(raw, conf if conf_prop else None, gamma[0], mode, k_f, bool(conf_prop), bool(legacy), w_conf=w_conf[0],
                                        b=b_conf[0]))


def check_affinity(run_affinity, k_f, mode, conf_prop, legacy, record=None, where=""):
    """run_affinity(raw, conf or None, gamma, w_conf, b_conf, k_f, mode id, conf_prop, legacy) -> offset, aff."""
    for shape in AFF_SHAPES:
        raw, conf, gamma, w_conf, b_conf = affinity_inputs(k_f, shape)
        want_o, want_a = affinity_oracle(k_f, shape, mode, conf_prop, legacy)
        if conf_prop and shape == AFF_SHAPES[0]:
            H, W = shape[1:]
            ys, xs = np.arange(H)[:, None] + want_o[:, 0::2], np.arange(W)[None, :] + want_o[:, 1::2]
            assert ((ys <= -1) | (ys >= H) | (xs <= -1) | (xs >= W)).mean() > 0.05      # confidence samples leave the image
        got_o, got_a = run_affinity(raw, conf if conf_prop else None, gamma, w_conf, b_conf, k_f, MODES[mode], conf_prop, legacy)
        eo, ea = float(np.abs(got_o - want_o).max()), float(np.abs(got_a - want_a).max())
        print(f"{where} affinity k_f {k_f} {mode} conf {conf_prop} legacy {legacy} {sid(shape)}: offset {eo:.2e} aff {ea:.2e}")
        if record is not None:
            record("nlspn_cases_affinity", where=where, k_f=k_f, mode=mode, conf_prop=conf_prop, legacy=legacy, shape=sid(shape), offset_abs=eo, aff_abs=ea)
        assert got_o.shape == want_o.shape and got_a.shape == want_a.shape
        assert eo <= 2e-5 and ea <= 1e-5, (k_f, mode, conf_prop, legacy, shape, eo, ea)


def conv3x3_fp64(x, w, b):
    """Conv2d(kernel 3, padding 1, bias) in fp64 as nine shifted matrix products."""
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2), np.float64)
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((B, w.shape[0], H, W), np.float64) + b.astype(np.float64)[None, :, None, None]
    for i in range(3):
        for j in range(3):
            y += np.einsum("oc,bchw->bohw", w[:, :, i, j].astype(np.float64), xp[:, :, i:i + H, j:j + W])
    return y


@functools.lru_cache(maxsize=None)
def guided_inputs(shape):
    """guidance N(0, 1), conv weight 0.2 N(0, 1), conv bias 0.1 N(0, 1) (the law of test_nlspn_guided_affinity_kernel_vs_oracle, which its bounds
    were set for: 72 products of mean magnitude 0.13 per output, offsets of deviation 1.7), confidence U(0, 1), gamma 4."""
    B, H, W = shape
    rs = np.random.RandomState(_seed(4, 3, shape))
    guide = rs.standard_normal((B, 8, H, W)).astype(np.float32)
    cw = (0.2 * rs.standard_normal((24, 8, 3, 3))).astype(np.float32)
    cb = (0.1 * rs.standard_normal(24)).astype(np.float32)
    conf = rs.uniform(0, 1, (B, 1, H, W)).astype(np.float32)
    return _ro(guide, cw, cb, conf, np.full(1, 4.0, np.float32), np.full(1, W_CONF, np.float32), np.full(1, B_CONF, np.float32))


@functools.lru_cache(maxsize=None)
def guided_oracle(shape, mode, conf_prop, legacy):
    guide, cw, cb, conf, gamma, w_conf, b_conf = guided_inputs(shape)
    return _ro(*O.nlspn_offset_affinity(conv3x3_fp64(guide, cw, cb), conf if conf_prop else None, gamma[0], mode, 3, bool(conf_prop), bool(legacy),
                                        w_conf=w_conf[0], b=b_conf[0]))


def check_guided(run_guided, mode, conf_prop, legacy, record=None, where=""):
    """run_guided(guide, conv_weight, conv_bias, conf or None, gamma, w_conf, b_conf, mode id, conf_prop, legacy) -> offset, aff."""
    for shape in GUIDED_SHAPES:
        guide, cw, cb, conf, gamma, w_conf, b_conf = guided_inputs(shape)
        want_o, want_a = guided_oracle(shape, mode, conf_prop, legacy)
        got_o, got_a = run_guided(guide, cw, cb, conf if conf_prop else None, gamma, w_conf, b_conf, MODES[mode], conf_prop, legacy)
        eo, ea = float(np.abs(got_o - want_o).max()), float(np.abs(got_a - want_a).max())
        print(f"{where} guided affinity {mode} conf {conf_prop} legacy {legacy} {sid(shape)}: offset {eo:.2e} aff {ea:.2e}")
        if record is not None:
            record("nlspn_cases_guided", where=where, mode=mode, conf_prop=conf_prop, legacy=legacy, shape=sid(shape), offset_abs=eo, aff_abs=ea)
        assert got_o.shape == want_o.shape and got_a.shape == want_a.shape
        assert eo <= 5e-5 and ea <= 2e-5, (mode, conf_prop, legacy, shape, eo, ea)


# ---- the DCNv2 operator -----------------------------------------------------------------------------------------------------------------------------
# name -> (B, C, Co, H, W, kh, kw, stride, pad, dil, group, dg)
DCN_CASES = {
    "slabs": (3, 2, 2, 56, 56, 3, 3, (1, 1), (1, 1), (1, 1), 1, 1),          # 9408 positions = two slabs of 4704, the slab edge inside image 1
    "slabs_g2_dg2": (3, 2, 2, 56, 56, 3, 3, (1, 1), (1, 1), (1, 1), 2, 2),
    "integer": (2, 2, 2, 9, 11, 3, 3, (1, 1), (1, 1), (1, 1), 1, 1),
}
DCN_SLAB = 8192                         # dd_dcn_backward: ceil(npos / 8192) slabs of ceil(npos / nslab) positions
GRAD_NAMES = ("input", "offset", "mask", "weight", "bias")


@functools.lru_cache(maxsize=None)
def dcn_inputs(name):
    """x, w, b, go N(0, 1), mask U(0, 2) (the law of tests/test_oracle_dcn.py); offsets 2.5 N(0, 1), or -- "integer" -- zero on image 0 and drawn
    from {-2, -1, -0.5, 0, 0.5, 1, 2} on image 1, so that samples fall exactly on -1, 0, H - 1 and H (and W likewise): the positions a
    zero-initialised conv_offset_aff produces in the first training step."""
    B, C, Co, H, W, kh, kw, st, pd, dl, grp, dg = DCN_CASES[name]
    Ho, Wo = O.out_size(H, W, kh, kw, st, pd, dl)
    rs = np.random.RandomState(900 + list(DCN_CASES).index(name))
    x = rs.standard_normal((B, C, H, W)).astype(np.float32)
    w = rs.standard_normal((Co, C // grp, kh, kw)).astype(np.float32)
    b = rs.standard_normal(Co).astype(np.float32)
    if name == "integer":
        off = rs.choice(np.array([-2, -1, -0.5, 0, 0.5, 1, 2], np.float32), size=(B, dg * 2 * kh * kw, Ho, Wo))
        off[0] = 0.0
    else:
        off = (2.5 * rs.standard_normal((B, dg * 2 * kh * kw, Ho, Wo))).astype(np.float32)
    m = rs.uniform(0, 2, (B, dg * kh * kw, Ho, Wo)).astype(np.float32)
    go = rs.standard_normal((B, Co, Ho, Wo)).astype(np.float32)
    return _ro(x, w, b, off, m, go)


@functools.lru_cache(maxsize=None)
def dcn_oracle(name):
    B, C, Co, H, W, kh, kw, st, pd, dl, grp, dg = DCN_CASES[name]
    x, w, b, off, m, go = dcn_inputs(name)
    return _ro(O.mdcn_forward(x, w, b, off, m, st, pd, dl, grp, dg), *O.mdcn_backward(x, w, b, off, m, go, st, pd, dl, grp, dg))


def check_dcn_conditions():
    """What the DCNv2 cases are for, from index arithmetic."""
    for name in ("slabs", "slabs_g2_dg2"):
        B, C, Co, H, W, kh, kw, st, pd, dl, grp, dg = DCN_CASES[name]
        Ho, Wo = O.out_size(H, W, kh, kw, st, pd, dl)
        npos = B * Ho * Wo
        nslab = -(-npos // DCN_SLAB)
        slab = -(-npos // nslab)
        assert (npos, nslab, slab) == (9408, 2, 4704) and Ho * Wo < slab < 2 * Ho * Wo      # the slab edge lies inside image 1
    B, C, Co, H, W, kh, kw, st, pd, dl, grp, dg = DCN_CASES["integer"]
    off = dcn_inputs("integer")[3]
    assert not off[0].any() and len(np.unique(off[1])) == 7
    hs, ws, _, _, _ = tap_geometry(off, 3)
    for pos, n in ((hs, H), (ws, W)):
        other_in = ((ws if pos is hs else hs) > -1) & ((ws if pos is hs else hs) < (W if pos is hs else H))
        for b in range(B):
            for v in (-1, 0, n - 1, n):
                assert ((pos[b] == v) & other_in[b]).sum() >= 4, (b, v)


def check_dcn(run_dcn, name, record=None, where=""):
    """run_dcn(x, w, b, off, m, go, (B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, group, dg, im2col_step)) -> out, [five gradients]."""
    B, C, Co, H, W, kh, kw, st, pd, dl, grp, dg = DCN_CASES[name]
    x, w, b, off, m, go = dcn_inputs(name)
    want = dcn_oracle(name)
    out, grads = run_dcn(x, w, b, off, m, go, (B, C, H, W, Co, kh, kw, st[0], st[1], pd[0], pd[1], dl[0], dl[1], grp, dg, 64))
    errs = {}
    for key, g, r in zip(("out",) + tuple("g_" + n for n in GRAD_NAMES), [out] + list(grads), want):
        assert g.shape == r.shape, key
        errs[key] = float(np.abs(g.astype(np.float64) - r).max() / max(np.abs(r).max(), 1e-12))
    print(f"{where} dcn {name}: {', '.join('%s %.2e' % kv for kv in errs.items())}")
    if record is not None:
        record("nlspn_cases_dcn_" + name, where=where, **errs)
    assert max(errs.values()) <= TOL, errs


# ---- guards for the NumPy side (the host emulation; the GPU consumer does the same with device tensors) --------------------------------------------
class Guarded:
    """Arrays with GUARD sentinel values in front of and behind them, 16-byte aligned like a device allocation; inputs keep a copy of their bits."""

    def __init__(self):
        self.bufs, self.inputs = [], []

    def _place(self, n):
        raw = np.full(n + 2 * GUARD + 4, SENTINEL, dtype=np.float32)
        off = ((-raw.ctypes.data) % 16) // 4
        buf = raw[off:off + n + 2 * GUARD]
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n]

    def out(self, shape, fill=np.nan):
        v = self._place(int(np.prod(shape))).reshape(shape)
        v[...] = fill
        return v

    def inp(self, a):
        if a is None:
            return None
        v = self._place(a.size).reshape(a.shape)
        v[...] = a
        self.inputs.append((v, np.array(a, dtype=np.float32)))
        return v

    def check(self):
        for buf, n in self.bufs:
            assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), "the library wrote outside a tensor"
        for v, a in self.inputs:
            assert np.array_equal(bits(v), bits(a)), "the library wrote to an input"
