"""The cases of the token Linear operator (include/swin/ddepth_linear.h), shared by tests/test_linear_host_emulation.py (the kernel's source on
the CPU) and tests/test_zz_gpu_linear.py (the built library): the shapes, the oracles written from the header's semantics (nothing imported from
the reference or from diffusiondepth_amd.linear) and the checks themselves, which take a ``run(x, w, bias, addend, act, prec) -> y`` callable on
numpy arrays (``w`` is the fp32 [N, K] weight: run packs it).

Bounds.  Exact families (small integers; a one-hot selection): bit-equal at every precision.  Real-valued cases: the library's max-abs error
against the fp64 oracle is at most 4 x max(the baseline's own error against the same oracle, 1e-6) -- the project's rule -- where the baseline
is torch fp32 on the CPU (F.linear, F.gelu, add), in the 16-bit modes with x and w rounded once to the operand type.  Identities (repeat, row
prefix, NaN containment): bitwise."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# name -> (M, K, N).  The kernel's tiles are 64 x 128 and, in the 16-bit modes where at least 256 of them fit, 128 x 128.
SHAPES = {
    "one": (1, 32, 32),              # a single row
    "tile": (64, 64, 128),           # one workgroup tile exactly in M and N
    "tile-1": (63, 64, 128),
    "tile+1": (65, 64, 128),
    "ragged": (340, 96, 288),        # Swin-T qkv on a 2 x 10 x 17 map; M and N ragged against 64 and 128
    "deep": (40, 6144, 64),          # the longest K; many pipeline stages
    "wide": (77, 64, 1024),          # many column tiles
    "many": (4100, 64, 256),         # many row tiles
    "merge": (50, 768, 384),         # PatchMerging's reduction: bias NULL
    "big-1": (511, 32, 8192),        # 4 x 64 = 256 tiles of 128 x 128: the big-tile instantiation (16-bit modes), ragged last row tile
    "big": (512, 32, 8192),          # ... exactly four row tiles
    "big+1": (513, 32, 8192),        # ... a fifth row tile of one row
}
PRECISIONS = {"fp32": 1, "bf16": 2, "f16": 3}
ROUND = {"fp32": None, "bf16": torch.bfloat16, "f16": torch.float16}
VARIANTS = ("plain", "full")      # real-valued: no bias / addend / activation, or all three
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4
TILE_EDGES = {"tile": (63, 64, 65), "big": (127, 128, 129, 511)}      # row counts on both sides of a tile edge, per instantiation


def case_id(c):
    return "-".join(str(v) for v in c)


def cases(names=tuple(SHAPES)):
    return [(n, p) for n in names for p in PRECISIONS]


def has_bias(name):
    return name != "merge"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _seed(name, salt):
    return 100 * list(SHAPES).index(name) + salt


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- exact family 1: small integers, an int64 oracle ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_inputs(name):
    """x, w, bias, addend integers with |v| <= 8: every product and partial sum is exact in fp32 (K * 64 < 2^24) and every operand exact in bf16
    and f16.  -> (x, w, bias or None, addend, expected)."""
    M, K, N = SHAPES[name]
    g = torch.Generator().manual_seed(_seed(name, 1))
    ints = lambda *s: torch.randint(-8, 9, s, generator=g).numpy().astype(np.int64)
    x, w, addend = ints(M, K), ints(N, K), ints(M, N)
    bias = ints(N) if has_bias(name) else None
    want = x @ w.T + addend + (0 if bias is None else bias[None, :])
    assert np.abs(want).max() < 2 ** 24
    f = lambda a: None if a is None else a.astype(np.float32)
    return _frozen(f(x), f(w), f(bias), f(addend), want.astype(np.float32))


def check_ints(run, name, prec):
    x, w, bias, addend, want = int_inputs(name)
    got = run(x, w, bias, addend, 0, prec)
    assert got.shape == want.shape
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{name} {prec}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


# ---- exact family 2: a selection ------------------------------------------------------------------------------------------------------------------
def selection(name):
    M, K, N = SHAPES[name]
    return (7 * np.arange(N) + 3) % K      # (a k that changes with every column and wraps around K several times where N > K)


@functools.lru_cache(maxsize=None)
def select_inputs(name):
    """w one-hot rows, y[m, n] = x[m, pi(n)]; x = +-(1 + j / 128) 2^e with e in -3 .. 3: 8 significant bits, exact in bf16 and f16, never 0 (so
    the zeros the other products add cannot change a sign).  -> (x, w, expected)."""
    M, K, N = SHAPES[name]
    g = torch.Generator().manual_seed(_seed(name, 2))
    mant = 1.0 + torch.randint(0, 128, (M, K), generator=g).double() / 128.0
    x = (mant * 2.0 ** torch.randint(-3, 4, (M, K), generator=g).double() * (2 * torch.randint(0, 2, (M, K), generator=g) - 1)).float().numpy()
    pi = selection(name)
    w = np.zeros((N, K), dtype=np.float32)
    w[np.arange(N), pi] = 1.0
    return _frozen(x, w, np.ascontiguousarray(x[:, pi]))


def check_selection(run, name, prec):
    x, w, want = select_inputs(name)
    got = run(x, w, None, None, 0, prec)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{name} {prec}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


# ---- real-valued cases against the fp64 oracle ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_inputs(name):
    """N(0, 1) x, w ~ N(0, 1 / K), N(0, 1) bias (None for "merge") and addend.  -> (x, w, bias, addend), read-only."""
    M, K, N = SHAPES[name]
    g = torch.Generator().manual_seed(_seed(name, 3))
    x = torch.randn(M, K, generator=g).numpy()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).numpy()
    bias = torch.randn(N, generator=g).numpy() if has_bias(name) else None
    addend = torch.randn(M, N, generator=g).numpy()
    return _frozen(x, w, bias, addend)


def variant_inputs(name, variant):
    x, w, bias, addend = real_inputs(name)
    return (x, w, None, None, 0) if variant == "plain" else (x, w, bias, addend, 1)


def compose(x, w, bias, addend, act, dtype, round_to=None):
    """act(x . w^T + bias) + addend in ``dtype`` on the CPU; ``round_to`` rounds x and w once (the 16-bit modes' baseline, with dtype float32)."""
    t = lambda a: None if a is None else torch.tensor(a).to(dtype)      # (a copy: the inputs are read-only)
    rnd = (lambda a: a.to(round_to).to(dtype)) if round_to is not None else (lambda a: a)
    y = F.linear(rnd(t(x)), rnd(t(w)), t(bias))
    if act == 1:
        y = F.gelu(y)      # (the exact erf form: the default)
    if addend is not None:
        y = y + t(addend)
    return y.numpy()


@functools.lru_cache(maxsize=None)
def real_oracle(name, variant):
    out = compose(*variant_inputs(name, variant), torch.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def real_baseline(name, variant, prec):
    out = compose(*variant_inputs(name, variant), torch.float32, ROUND[prec])
    out.setflags(write=False)
    return out


def check_real(run, name, prec, variant, record=None, where=""):
    x, w, bias, addend, act = variant_inputs(name, variant)
    oracle = real_oracle(name, variant)
    got = run(x, w, bias, addend, act, prec)
    err = float(np.abs(got.astype(np.float64) - oracle).max())
    base_err = float(np.abs(real_baseline(name, variant, prec).astype(np.float64) - oracle).max())
    print(f"{where} {name} {prec} {variant}: library {err:.3e} baseline {base_err:.3e}")
    if record is not None:
        record("swin_linear", where=where, shape=name, precision=prec, variant=variant, err=err, baseline_err=base_err)
    assert np.isfinite(got).all()
    assert err <= 4.0 * max(base_err, 1e-6), (name, prec, variant, err, base_err)


# ---- bitwise identities -------------------------------------------------------------------------------------------------------------------------------
def check_repeat_and_rows(run, prec, name="ragged", edges=TILE_EDGES["tile"]):
    """Two calls give the same bits; the first m0 rows of y(x) are y(x[:m0]) for m0 on both sides of a tile edge."""
    x, w, bias, addend, act = variant_inputs(name, "full")
    whole = run(x, w, bias, addend, act, prec)
    again = run(x, w, bias, addend, act, prec)
    assert np.array_equal(bits(whole), bits(again)), "two calls differ"
    for m0 in (1,) + tuple(edges):
        assert m0 < x.shape[0]
        part = run(np.ascontiguousarray(x[:m0]), w, bias, np.ascontiguousarray(addend[:m0]), act, prec)
        assert np.array_equal(bits(part), bits(whole[:m0])), f"the first {m0} rows differ from the call on {m0} rows"


NAN_ROW, NAN_K, NAN_ADD = 70, 41, (3, 130)


def check_nan(run, prec, name="ragged"):
    """A NaN in one element of x: that whole row of y is NaN and every other row has the clean run's bits (a guard that multiplies garbage by
    zero fails here).  A NaN in one addend element reaches that element only."""
    x, w, bias, addend, act = variant_inputs(name, "full")
    clean = run(x, w, bias, addend, act, prec)
    dirty = x.copy()
    dirty[NAN_ROW, NAN_K] = np.nan
    got = run(dirty, w, bias, addend, act, prec)
    assert np.isnan(got[NAN_ROW]).all(), "the NaN did not reach every output of its row"
    rest = np.arange(x.shape[0]) != NAN_ROW
    assert np.array_equal(bits(got[rest]), bits(clean[rest])), "the NaN left its row"
    add = addend.copy()
    add[NAN_ADD] = np.nan
    got = run(x, w, bias, add, act, prec)
    hit = np.zeros(got.shape, dtype=bool)
    hit[NAN_ADD] = True
    assert np.isnan(got[hit]).all() and np.array_equal(bits(got[~hit]), bits(clean[~hit])), "the addend's NaN is not where it was put"


# ---- a tiny Swin-like backbone of WHOLE blocks for the facade tests: a patch-embedding conv, one plain and one shifted block, four maps ----------------
class DuckFFN(torch.nn.Module):
    """The interface of mmcv's FFN: layers = Sequential(Sequential(Linear, GELU, Dropout), Linear, Dropout), dropout_layer, add_identity,
    forward(x, identity=None).  NOT a HipFFN, so that convert_hip_swin_linears has something to replace."""

    def __init__(self, dims, hidden, add_identity=True, act=None, bias=True):
        from torch import nn
        super().__init__()
        self.embed_dims, self.feedforward_channels, self.add_identity = dims, hidden, add_identity
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(dims, hidden, bias=bias), act if act is not None else nn.GELU(), nn.Dropout(0.0)),
                                    nn.Linear(hidden, dims, bias=bias), nn.Dropout(0.0))
        self.dropout_layer = nn.Identity()

    def forward(self, x, identity=None):
        out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        if identity is None:
            identity = x
        return identity + self.dropout_layer(out)


def tiny_backbone(seed=0):
    """Duck-typed attention (``window_size``, ``shift_size``, ``w_msa``, ``drop``; the torch sequence as forward) and duck-typed FFNs in two whole
    blocks of 192 channels (norm1, attn, norm2, ffn with add_identity), the second shifted; maps of 192 / 384 / 768 / 1536 channels at strides
    4 / 8 / 16 / 32 through average pooling and 1x1 convolutions, as swin_cases.tiny_backbone builds them."""
    from torch import nn

    from diffusiondepth_amd import swin as SW

    class DuckShiftWindowMSA(nn.Module):
        def __init__(self, dims, heads, shift):
            super().__init__()
            self.window_size, self.shift_size = 7, shift
            self.w_msa = SW.WindowMSA(dims, heads, (7, 7))
            self.drop = nn.Identity()

        def forward(self, query, hw_shape):
            return SW.HipShiftWindowMSA._forward_torch(self, query, *hw_shape)

    class Block(nn.Module):
        def __init__(self, dims, heads, shift):
            super().__init__()
            self.norm1 = nn.LayerNorm(dims)
            self.attn = DuckShiftWindowMSA(dims, heads, shift)
            self.norm2 = nn.LayerNorm(dims)
            self.ffn = DuckFFN(dims, 4 * dims)

        def forward(self, x, hw):
            x = x + self.attn(self.norm1(x), hw)
            return self.ffn(self.norm2(x), identity=x)

    class TinySwin(nn.Module):
        def __init__(self):
            super().__init__()
            self.patch_embed = nn.Conv2d(3, 192, 4, 4)
            self.blocks = nn.ModuleList([Block(192, 6, 0), Block(192, 6, 3)])
            self.down = nn.ModuleList([nn.Conv2d(a, b, 1) for a, b in ((192, 384), (384, 768), (768, 1536))])

        def forward(self, img):
            x = self.patch_embed(img)
            B, C, H, W = x.shape
            t = x.flatten(2).transpose(1, 2).contiguous()      # (as behind the reference's patch-embedding norm: contiguous tokens)
            for blk in self.blocks:
                t = blk(t, (H, W))
            maps = [t.transpose(1, 2).reshape(B, C, H, W)]
            for conv in self.down:
                maps.append(conv(F.avg_pool2d(maps[-1], 2)))
            return maps

    torch.manual_seed(seed)
    net = TinySwin()
    for m in net.modules():
        if isinstance(m, SW.WindowMSA):
            m.init_weights()
    return net
