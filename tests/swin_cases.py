"""The cases of the shifted-window attention operator (include/ddepth_swin.h), shared by tests/test_swin_host_emulation.py (the kernel's source on
the CPU) and tests/test_zz_gpu_swin_attention.py (the built library): the shapes, an fp64 oracle written from the header's semantics as index
arithmetic (no pad, roll or partition op, nothing imported from the reference or from diffusiondepth_amd.swin), a pure index-arithmetic oracle
for the exact cases, and the checks themselves, which take a ``run(qkv, qkv_pad, rel_bias, heads, shift, prec) -> out`` callable on numpy arrays.

Bounds.  Exact cases: bit-equal.  Real-valued cases: the library's max-abs error against the fp64 oracle is at most 4 x max(the baseline's own
error against the same oracle, 1e-6) -- the codec's rule -- where the baseline is the torch composition in fp32 (fp32 mode) or ``attend`` in fp32
with q * scale, k, the probabilities and v rounded to the operand type (bf16 / f16 modes)."""
import functools

import numpy as np
import torch

WINDOW, N, HD = 7, 49, 32
# name -> (B, H, W, heads)
SHAPES = {
    "one": (1, 7, 7, 1),            # one window
    "whole": (2, 14, 21, 3),        # whole windows
    "ragged": (2, 10, 17, 3),       # ragged both ways, pad 4 / 4
    "sub": (1, 4, 5, 1),            # smaller than a window
    "last": (1, 11, 38, 6),         # the Swin-L last-stage map with fewer heads
    "big": (2, 70, 70, 6),          # 1 200 tasks: more than one pass of the persistent grid
}
SHIFTS = (0, 3)
PRECISIONS = {"fp32": 1, "bf16": 2, "f16": 3}
ROUND = {"fp32": None, "bf16": torch.bfloat16, "f16": torch.float16}
BIAS_SCALES = (1.0, 50.0)
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4


def case_id(c):
    return "-".join(str(v) for v in c)


def cases(names=tuple(SHAPES)):
    return [(n, s, p) for n in names for s in SHIFTS for p in PRECISIONS]


# ---- index arithmetic: where slot s of window (wy, wx) lives ------------------------------------------------------------------------------------
def slot_map(H, W, shift):
    """-> y, x, inside, label, each [nwy, nwx, 49].  Slot s of window (wy, wx) is position (r, c) = (7 wy + s // 7, 7 wx + s % 7) of the rolled
    padded frame, i.e. token ((r + shift) mod Hp, (c + shift) mod Wp) of the padded frame; ``inside`` where that is a token of the image; the
    label is 3 * band(r) + band(c) with the bands [0, n - 7), [n - 7, n - shift), [n - shift, n) on the ROLLED frame (0 without a shift)."""
    nwy, nwx = -(-H // WINDOW), -(-W // WINDOW)
    Hp, Wp = nwy * WINDOW, nwx * WINDOW
    s = np.arange(N)
    r = (np.arange(nwy) * WINDOW)[:, None, None] + (s // WINDOW)[None, None, :] + np.zeros((1, nwx, 1), dtype=np.int64)
    c = (np.arange(nwx) * WINDOW)[None, :, None] + (s % WINDOW)[None, None, :] + np.zeros((nwy, 1, 1), dtype=np.int64)
    y, x = (r + shift) % Hp, (c + shift) % Wp
    if shift:
        band = lambda v, n: np.where(v < n - WINDOW, 0, np.where(v < n - shift, 1, 2))
        label = 3 * band(r, Hp) + band(c, Wp)
    else:
        label = np.zeros_like(r)
    return y, x, (y < H) & (x < W), label


def gather(qkv, qkv_pad, shift):
    """qkv [B, H, W, K] -> [B, nwy, nwx, 49, K]: every window's slots, padded positions holding qkv_pad (zeros when None)."""
    B, H, W, K = qkv.shape
    y, x, inside, _ = slot_map(H, W, shift)
    Hp, Wp = -(-H // WINDOW) * WINDOW, -(-W // WINDOW) * WINDOW
    frame = np.zeros((B, Hp, Wp, K), dtype=qkv.dtype)
    if qkv_pad is not None:
        frame[...] = qkv_pad
    frame[:, :H, :W] = qkv
    return frame[:, y, x]


def scatter(win_out, H, W, shift):
    """[B, nwy, nwx, 49, C] -> [B, H, W, C]: every in-image slot back at its token (each token is the slot of exactly one window)."""
    y, x, inside, _ = slot_map(H, W, shift)
    out = np.full((win_out.shape[0], H, W, win_out.shape[-1]), np.nan, dtype=win_out.dtype)
    out[:, y[inside], x[inside]] = win_out[:, inside]
    assert not np.isnan(out).any() or np.isnan(win_out).any()
    return out


def attend(qkv, qkv_pad, rel_bias, heads, shift, dtype=torch.float64, round_to=None):
    """softmax(q * 32^-0.5 . k^T + rel_bias + mask) . v per window and head in ``dtype``; ``round_to`` rounds q * scale, k, the probabilities and v
    once each (the 16-bit modes' emulation, with dtype = float32).  -> numpy [B, H, W, C] in ``dtype``."""
    B, H, W, K = qkv.shape
    C = K // 3
    y, x, inside, label = slot_map(H, W, shift)
    win = torch.from_numpy(gather(qkv, qkv_pad, shift)).to(dtype)
    win = win.view(B, *y.shape[:2], N, 3, heads, HD).permute(4, 0, 1, 2, 5, 3, 6)      # [3, B, nwy, nwx, heads, 49, 32]
    rnd = (lambda t: t.to(round_to).to(dtype)) if round_to is not None else (lambda t: t)
    q, k, v = rnd(win[0] * (HD ** -0.5)), rnd(win[1]), rnd(win[2])
    s = q @ k.transpose(-1, -2) + torch.tensor(rel_bias, dtype=dtype)
    if shift:
        lab = torch.from_numpy(label)
        s = s + torch.where(lab[:, :, :, None] != lab[:, :, None, :], -100.0, 0.0).to(dtype)[None, :, :, None]
    o = rnd(torch.softmax(s, dim=-1)) @ v                                                # [B, nwy, nwx, heads, 49, 32]
    o = o.permute(0, 1, 2, 4, 3, 5).reshape(B, *y.shape[:2], N, C)
    return scatter(o.numpy(), H, W, shift)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def rel_index():
    i = np.arange(N)
    yy, xx = i // WINDOW, i % WINDOW
    return (yy[:, None] - yy[None, :] + WINDOW - 1) * (2 * WINDOW - 1) + (xx[:, None] - xx[None, :] + WINDOW - 1)


def real_pad_is_null(name, shift):
    """qkv_pad is NULL in half of the real-valued cases: ragged and last without a shift, sub with one."""
    return (list(SHAPES).index(name) + (shift > 0)) % 2 == 0


@functools.lru_cache(maxsize=None)
def real_inputs(name, shift, bias_scale):
    """N(0, 1) qkv with q and k times 1.5 (scores q . k / sqrt(32) then have a deviation of 2.25: about +-8 over a window), a bias table from
    trunc_normal(std 0.02) times ``bias_scale``, a qkv_pad of the same law or None.  -> (qkv, qkv_pad, rel_bias), read-only."""
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    g = torch.Generator().manual_seed(1000 * list(SHAPES).index(name) + 10 * shift + int(bias_scale))
    gain = torch.cat([torch.full((2 * C,), 1.5), torch.ones(C)])
    qkv = (torch.randn(B, H, W, 3 * C, generator=g) * gain).numpy()
    pad = None if real_pad_is_null(name, shift) else (torch.randn(3 * C, generator=g) * gain).numpy()
    table = torch.nn.init.trunc_normal_(torch.empty(169, heads), std=0.02, generator=g).numpy() * np.float32(bias_scale)
    bias = np.ascontiguousarray(table[rel_index().reshape(-1)].reshape(N, N, heads).transpose(2, 0, 1))
    for a in (qkv, pad, bias):
        if a is not None:
            a.setflags(write=False)
    return qkv, pad, bias


@functools.lru_cache(maxsize=None)
def real_oracle(name, shift, bias_scale):
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    out = attend(qkv, pad, bias, SHAPES[name][3], shift)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def real_emulation(name, shift, bias_scale, prec):
    """The 16-bit modes' baseline: fp32 sums, operands rounded once."""
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    out = attend(qkv, pad, bias, SHAPES[name][3], shift, dtype=torch.float32, round_to=ROUND[prec])
    out.setflags(write=False)
    return out


def permutation(kind, h):
    i = np.arange(N)
    if kind == "identity":
        return i
    return ((3, 5, 2, 4, 6, 8)[h % 6] * i + 11 + 5 * h) % N      # the multipliers are coprime to 49


def exact_pad_is_null(name, shift):
    """NULL wherever that keeps the expectation exact: without a shift and on whole-window shapes.  With a shift AND padding a selection that
    crosses mask regions has row maximum 100, the unmasked other keys keep exp(-100) ~ 4e-44 (a denormal, not 0), and a selected v of exactly
    0 (a NULL pad) would leave their sum in the output; with |v| >= 1 everywhere it is below half an ulp and the output is v."""
    _, H, W, _ = SHAPES[name]
    return shift == 0 or (H % WINDOW == 0 and W % WINDOW == 0)


@functools.lru_cache(maxsize=None)
def exact_inputs(name, shift, kind):
    """q = 0 (scores = bias exactly), k small integers, v integers with 1 <= |v| <= 15 (exact in bf16 and f16); rel_bias[h, i, pi_h(i)] = 200, 0
    elsewhere: softmax is exactly one-hot (exp(-100) and less against 1 vanishes in the fp32 sum), so out at slot i is v at slot pi_h(i)."""
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    g = torch.Generator().manual_seed(77 + list(SHAPES).index(name) + 10 * shift)

    def ints(*shape):
        q = torch.zeros(*shape, C)
        k = torch.randint(-3, 4, (*shape, C), generator=g).float()
        v = torch.randint(1, 16, (*shape, C), generator=g).float() * (2 * torch.randint(0, 2, (*shape, C), generator=g) - 1)
        return torch.cat([q, k, v], dim=-1).numpy()

    qkv = ints(B, H, W)
    pad = None if exact_pad_is_null(name, shift) else ints()
    bias = np.zeros((heads, N, N), dtype=np.float32)
    for h in range(heads):
        bias[h, np.arange(N), permutation(kind, h)] = 200.0
    for a in (qkv, pad, bias):
        if a is not None:
            a.setflags(write=False)
    return qkv, pad, bias


def exact_expected(name, shift, kind):
    """Index arithmetic only: out[token of slot i, head h] = v[slot pi_h(i) of the same rolled, padded window, head h]."""
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    qkv, pad, _ = exact_inputs(name, shift, kind)
    v = gather(qkv[..., 2 * C:], None if pad is None else pad[2 * C:], shift)      # [B, nwy, nwx, 49, C]
    sel = np.empty_like(v)
    for h in range(heads):
        sel[..., h * HD:(h + 1) * HD] = v[:, :, :, permutation(kind, h), h * HD:(h + 1) * HD]
    return scatter(sel, H, W, shift)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the checks: run(qkv, qkv_pad, rel_bias, heads, shift, prec) -> out [B, H, W, C] fp32 numpy ---------------------------------------------------
def check_exact(run, name, shift, prec, kind):
    qkv, pad, bias = exact_inputs(name, shift, kind)
    got = run(qkv, pad, bias, SHAPES[name][3], shift, prec)
    want = exact_expected(name, shift, kind)
    assert got.shape == want.shape
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{name} shift {shift} {prec} {kind}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def check_real(run, baseline_fp32, name, shift, prec, bias_scale, record=None, where=""):
    """baseline_fp32(qkv, qkv_pad, rel_bias, heads, shift) -> the torch composition's fp32 output (the fp32 mode's yardstick)."""
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    heads = SHAPES[name][3]
    oracle = real_oracle(name, shift, bias_scale)
    got = run(qkv, pad, bias, heads, shift, prec)
    base = baseline_fp32(qkv, pad, bias, heads, shift) if prec == "fp32" else real_emulation(name, shift, bias_scale, prec)
    err = float(np.abs(got.astype(np.float64) - oracle).max())
    base_err = float(np.abs(np.asarray(base, dtype=np.float64) - oracle).max())
    print(f"{where} {name} shift {shift} {prec} bias x{bias_scale:g}: library {err:.3e} baseline {base_err:.3e}")
    if record is not None:
        record("swin_window_attention", where=where, shape=name, shift=shift, precision=prec, bias_scale=bias_scale, err=err, baseline_err=base_err)
    assert np.isfinite(got).all()
    assert err <= 4.0 * max(base_err, 1e-6), (name, shift, prec, bias_scale, err, base_err)


def check_batch_and_repeat(run, prec, shift=3, name="ragged"):
    """Image b of a B = 2 call equals the B = 1 call on it; two calls are equal to each other.  Bit-equal."""
    qkv, pad, bias = real_inputs(name, shift, 1.0)
    heads = SHAPES[name][3]
    both = run(qkv, pad, bias, heads, shift, prec)
    again = run(qkv, pad, bias, heads, shift, prec)
    assert np.array_equal(bits(both), bits(again)), "two calls differ"
    for b in range(qkv.shape[0]):
        one = run(np.ascontiguousarray(qkv[b:b + 1]), pad, bias, heads, shift, prec)
        assert np.array_equal(bits(one[0]), bits(both[b])), f"image {b} of the batched call differs from the single call"


NAN_AT = dict(b=1, y=4, x=9, head=1, d=5)


def check_nan(run, prec, shift=3, name="ragged"):
    """A NaN in one in-image token's k of one head: every in-image output of that (window, head) is NaN, every other output is bit-identical to
    the clean run."""
    qkv, pad, bias = real_inputs(name, shift, 1.0)
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    clean = run(qkv, pad, bias, heads, shift, prec)
    dirty = qkv.copy()
    a = NAN_AT
    dirty[a["b"], a["y"], a["x"], C + a["head"] * HD + a["d"]] = np.nan
    got = run(dirty, pad, bias, heads, shift, prec)
    y, x, inside, _ = slot_map(H, W, shift)
    hit = ((y == a["y"]) & (x == a["x"])).any(axis=-1)      # the one window that holds the token
    assert hit.sum() == 1
    wy, wx = np.argwhere(hit)[0]
    want_nan = np.zeros((B, H, W, C), dtype=bool)
    m = inside[wy, wx]
    want_nan[a["b"], y[wy, wx][m], x[wy, wx][m], a["head"] * HD:(a["head"] + 1) * HD] = True
    assert 1 < want_nan.sum() < want_nan.size
    assert np.isnan(got[want_nan]).all(), "the NaN did not reach every output of its window and head"
    assert np.array_equal(bits(got)[~want_nan], bits(clean)[~want_nan]), "the NaN left its window or head"


# ---- a tiny Swin-like backbone for the facade tests: a patch-embedding conv, one plain and one shifted block, four maps at the Swin head's widths --
def tiny_backbone(seed=0):
    """Built from duck-typed attention modules that are NOT HipShiftWindowMSA (``window_size``, ``shift_size``, ``w_msa``, ``drop`` and the torch
    sequence as forward), so that convert_hip_window_attention has something to replace.  Maps: 192 channels at stride 4 out of the two blocks,
    then 384 / 768 / 1536 at strides 8 / 16 / 32 through average pooling and 1x1 convolutions."""
    from torch import nn

    from diffusiondepth_amd import swin as SW

    class DuckShiftWindowMSA(nn.Module):
        def __init__(self, dims, heads, shift):
            super().__init__()
            self.window_size, self.shift_size = WINDOW, shift
            self.w_msa = SW.WindowMSA(dims, heads, (WINDOW, WINDOW))
            self.drop = nn.Identity()

        def forward(self, query, hw_shape):
            return SW.HipShiftWindowMSA._forward_torch(self, query, *hw_shape)

    class Block(nn.Module):
        def __init__(self, dims, heads, shift):
            super().__init__()
            self.norm1 = nn.LayerNorm(dims)
            self.attn = DuckShiftWindowMSA(dims, heads, shift)

        def forward(self, x, hw):
            return x + self.attn(self.norm1(x), hw)

    class TinySwin(nn.Module):
        def __init__(self):
            super().__init__()
            self.patch_embed = nn.Conv2d(3, 192, 4, 4)
            self.blocks = nn.ModuleList([Block(192, 6, 0), Block(192, 6, 3)])
            self.down = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in ((192, 384), (384, 768), (768, 1536))])

        def forward(self, img):
            x = self.patch_embed(img)
            B, C, H, W = x.shape
            t = x.flatten(2).transpose(1, 2)
            for blk in self.blocks:
                t = blk(t, (H, W))
            maps = [t.transpose(1, 2).reshape(B, C, H, W)]
            for conv in self.down:
                maps.append(conv(torch.nn.functional.avg_pool2d(maps[-1], 2)))
            return maps

    torch.manual_seed(seed)
    net = TinySwin()
    for m in net.modules():
        if isinstance(m, SW.WindowMSA):
            m.init_weights()
    return net
