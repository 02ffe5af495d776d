"""Shared cases of the tests of include/ddepth_conv_fused.h (the folded eval-mode forward: a 3x3 pad-1 convolution of stride 1 or 2 with
BatchNorm, residual add and ReLU in its epilogue; tests/test_conv_fused_host_emulation.py and tests/test_conv_fused_cpu.py on the CPU,
tests/test_zz_gpu_conv_fused.py on the GPU): shapes, seeded inputs, the fp64 references and the rules a result is held to.

    y = relu(conv(x, w) * scale[co] + shift[co] + addend)            addend and relu optional

Exact data.  x, w and addend are integers in {-1, 0, 1}, scale is in {-1, 1/2, 1, 2}, shift an integer in -3 .. 3.  The accumulator is an integer
of magnitude <= 9 Cin <= 648 (asserted below), so acc * scale + shift + addend is a multiple of 1/2 below 2^11: exact in fp32 at every step,
in every precision.  The rule is np.array_equal against the fp64 reference.

Real-valued data (N(0, 1) everywhere, scale in +-[0.5, 2]), per element |got - ref64| <= tol, the reference taken on x and w rounded to the
precision (bf16 / f16; f16x3: unrounded), scale, shift and addend never rounded:
    tol = (K + 1 + E) * 2^-23 * S   (+ 2^-18 * S in f16x3),   K = 9 Cin,   S = the same expression on absolute values in fp64.
E is the number of fp32 roundings the epilogue makes behind the accumulation.  From the kernel text (csrc/dd_conv_kernels.h, the DD_CONV_AFFINE pass,
and affine_tail in csrc/dd_conv.hip):  v = fmaf(acc, scale[n], shift[n]) rounds once;  v += addend[o] rounds once more;  the ReLU is a select and
rounds nothing.  So E = 2 with an addend and E = 1 without one.

The stride-1 shapes are those of tests/conv_cases.py (S1, S3) and tests/conv_ragged_cases.py (R1, R5); the stride-2 ones those of
tests/conv_strided_cases.py (Z1, Z4, Z5, Z6).  The rounding rule, ULP and the precision ids are imported from those files."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as CC
import conv_ragged_cases as RC
import conv_strided_cases as ZC
from conv_cases import PRECISIONS, ULP, _rounded  # noqa: F401  (re-exported to the tests)

# name -> (stride, (B, Cin, Cout, H, W)); H, W = input size
SHAPES = {
    "S1": (1, CC.SHAPES["S1"][1]),      # (2, 64, 256, 9, 35): four cout tiles, ragged pixel tiles, batch offset of the addend
    "S3": (1, CC.SHAPES["S3"][1]),      # (1, 64, 64, 3, 5): sub-tile
    "R1": (1, RC.SHAPES["R1"][1]),      # (1, 72, 72, 5, 35): N tail of 8 -- guarded reads of scale_shift
    "R5": (1, RC.SHAPES["R5"][1]),      # (1, 8, 24, 3, 5): the lower end
    "Z1": (2, ZC.SHAPES["Z1"]),         # (2, 64, 128, 9, 67)
    "Z4": (2, ZC.SHAPES["Z4"]),         # (1, 8, 8, 1, 2)
    "Z5": (2, ZC.SHAPES["Z5"]),         # (2, 3, 64, 10, 37): RGB
    "Z6": (2, ZC.SHAPES["Z6"]),         # (1, 72, 216, 7, 12)
}
assert SHAPES["S1"][1] == (2, 64, 256, 9, 35) and SHAPES["S3"][1] == (1, 64, 64, 3, 5) and SHAPES["R1"][1] == (1, 72, 72, 5, 35)
assert SHAPES["R5"][1] == (1, 8, 24, 3, 5) and SHAPES["Z1"][1] == (2, 64, 128, 9, 67) and SHAPES["Z4"][1] == (1, 8, 8, 1, 2)
assert SHAPES["Z5"][1] == (2, 3, 64, 10, 37) and SHAPES["Z6"][1] == (1, 72, 216, 7, 12)

ADDEND = (True, False)
RELU = (True, False)
VARIANTS = [(a, r) for a in ADDEND for r in RELU]
CASES = [(n, p) for n in SHAPES for p in PRECISIONS]
PAD_RAGGED = ("R1", "Z6")      # a ragged shape equals the block-64 instantiation on zero-padded tensors
NAN_CASE = "S1"
E_ADDEND, E_PLAIN = 2, 1       # fp32 roundings of the epilogue (module docstring)

FOLD_C = (8, 72, 2048)
FOLD_EPS = 1e-5


def case_id(c):
    return "-".join(str(v) for v in c)


def variant_id(v):
    return ("add" if v[0] else "noadd") + "-" + ("relu" if v[1] else "lin")


def out_size(n, stride):
    return (n - 1) // 2 + 1 if stride == 2 else n


def shapes_for(stride, dims):
    """(x, w, scale_shift, y) shapes."""
    B, Cin, Cout, H, W = dims
    return (B, Cin, H, W), (Cout, Cin, 3, 3), (2, Cout), (B, Cout, out_size(H, stride), out_size(W, stride))


def shapes_of(name):
    return shapes_for(*SHAPES[name])


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, scale_shift ([2, Cout]: scale, shift), addend.  kind: "int" or "normal".  Treat as read-only (cached)."""
    xs, ws, ss, ys = shapes_of(name)
    g = torch.Generator().manual_seed(49979687 * (list(SHAPES).index(name) + 1) + len(kind))
    out = {}
    if kind == "normal":
        out["x"], out["w"] = torch.randn(xs, generator=g), torch.randn(ws, generator=g)
        mag = 0.5 + 1.5 * torch.rand(ss[1], generator=g)
        sign = torch.randint(0, 2, (ss[1],), generator=g).float() * 2 - 1
        out["scale_shift"] = torch.stack([mag * sign, torch.randn(ss[1], generator=g)]).contiguous()
        out["addend"] = torch.randn(ys, generator=g)
        assert ((out["scale_shift"][0].abs() >= 0.5) & (out["scale_shift"][0].abs() <= 2.0)).all()
        return out
    out["x"] = torch.randint(-1, 2, xs, generator=g).float()
    out["w"] = torch.randint(-1, 2, ws, generator=g).float()
    scale = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (ss[1],), generator=g)]
    shift = torch.randint(-3, 4, (ss[1],), generator=g).float()
    out["scale_shift"] = torch.stack([scale, shift]).contiguous()
    out["addend"] = torch.randint(-1, 2, ys, generator=g).float()
    # the exactness preconditions (module docstring): every operand exact in bf16 and f16, every intermediate a multiple of 1/2 below 2^11
    for k in ("x", "w", "addend"):
        assert torch.equal(out[k], out[k].round()) and out[k].abs().max() <= 1
    assert all(float(s) in (-1.0, 0.5, 1.0, 2.0) for s in scale) and torch.equal(shift, shift.round()) and shift.abs().max() <= 3
    Cin = SHAPES[name][1][1]
    assert 9 * Cin * 2 + 3 + 1 < 2 ** 11, "acc * scale + shift + addend stays a multiple of 1/2 below 2^11: exact in fp32"
    return out


def _reference(stride, x, w, ss, addend, relu):
    y = F.conv2d(x, w, None, stride, 1) * ss[0].view(1, -1, 1, 1) + ss[1].view(1, -1, 1, 1)
    if addend is not None:
        y = y + addend
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)      # (keeps a NaN, as torch.relu does)
    return y.numpy()


def reference_of(stride, inp, addend, relu, operands="exact"):
    """fp64 reference on the tensors `inp`.  operands: "exact", "bf16" / "f16" (x and w rounded to that type first; scale, shift and addend
    never), "abs" / "abs_bf16" / "abs_f16" (absolute values of everything, no ReLU: the S of the tolerance)."""
    prec = operands.replace("abs_", "").replace("abs", "exact")
    x, w = _rounded(inp["x"], prec), _rounded(inp["w"], prec)
    ss, a = inp["scale_shift"].double(), inp["addend"].double() if addend else None
    if operands.startswith("abs"):
        return _reference(stride, x.abs(), w.abs(), ss.abs(), a.abs() if a is not None else None, False)
    return _reference(stride, x, w, ss, a, relu)


@functools.lru_cache(maxsize=None)
def reference(name, kind, addend, relu, operands="exact"):
    """Computed once per (case, kind, addend, relu, operands) and shared; treat as read-only."""
    return reference_of(SHAPES[name][0], make_inputs(name, kind), addend, relu, operands)


def check_exact(y, name, addend, relu, label=""):
    want = reference(name, "int", addend, relu)
    got = np.asarray(y, dtype=np.float64).reshape(want.shape)
    print(f"{label} {name} int addend={addend} relu={relu}: max|ref| {np.abs(want).max():.6g} differing {int((got != want).sum())} of {got.size}")
    assert np.array_equal(got, want)


def tolerance(name, prec, addend):
    rounded = prec in ("bf16", "f16")
    S = reference(name, "normal", addend, False, "abs_" + prec if rounded else "abs")
    K = 9 * SHAPES[name][1][1]
    E = E_ADDEND if addend else E_PLAIN
    return ((0.0 if rounded else 2.0 ** -18) + (K + 1 + E) * ULP) * S


def check_real(y, name, prec, addend, relu, label=""):
    """Asserts the cap; returns the worst err / tol."""
    rounded = prec in ("bf16", "f16")
    ref = reference(name, "normal", addend, relu, prec if rounded else "exact")
    tol = tolerance(name, prec, addend)
    got = np.asarray(y, dtype=np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{label} {name} {prec} addend={addend} relu={relu}: max err {err.max():.3e} worst err/tol {worst:.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), worst
    return worst


# ---- the zero-padding identity --------------------------------------------------------------------------------------------------------------------
def _pad(t, shape):
    out = torch.zeros(shape, dtype=t.dtype)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out


def zero_padded(name):
    """(dims, inputs) of case `name` (real-valued data) with both channel counts zero-padded to the next multiple of 64."""
    stride, (B, Cin, Cout, H, W) = SHAPES[name]
    up = lambda n: -(-n // 64) * 64
    dims = (B, up(Cin), up(Cout), H, W)
    inp = make_inputs(name, "normal")
    return dims, {k: _pad(inp[k], s) for k, s in zip(("x", "w", "scale_shift", "addend"), shapes_for(stride, dims))}


def cut(name, y):
    ys = shapes_of(name)[3]
    return np.ascontiguousarray(np.asarray(y)[tuple(slice(0, s) for s in ys)])


# ---- NaN --------------------------------------------------------------------------------------------------------------------------------------------
NAN_SHIFT_CHANNEL = 3


@functools.lru_cache(maxsize=None)
def nan_inputs(in_shift):
    """S1 (real-valued) with one NaN pixel in x of image 1 -- image 0 stays clean -- and, with `in_shift`, one NaN in shift as well: then channel
    NAN_SHIFT_CHANNEL of both images is NaN and the rest of image 0 stays clean."""
    inp = {k: v.clone() for k, v in make_inputs(NAN_CASE, "normal").items()}
    inp["x"][1, 5, 4, 17] = float("nan")
    if in_shift:
        inp["scale_shift"][1, NAN_SHIFT_CHANNEL] = float("nan")
    return inp


def check_nan(y, in_shift, addend, label=""):
    """The NaN mask of y equals the fp64 reference's (ReLU on), and image 0 is clean (but for the NaN shift's channel)."""
    want = reference_of(SHAPES[NAN_CASE][0], nan_inputs(in_shift), addend, True)
    got = np.asarray(y).reshape(want.shape)
    print(f"{label} NaN in_shift={in_shift} addend={addend}: {int(np.isnan(want).sum())} NaN expected, {int(np.isnan(got).sum())} got")
    assert np.isnan(want[1]).any() and np.isnan(want[0]).any() == in_shift
    assert np.array_equal(np.isnan(got), np.isnan(want))
    clean = np.delete(got[0], NAN_SHIFT_CHANNEL, axis=0) if in_shift else got[0]
    assert np.isfinite(clean).all(), "image 0 is clean"


# ---- dd_bn_fold -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fold_inputs(C):
    """fp32 numpy vectors gamma, beta, mean, var (in [1e-3, 4]), conv_bias."""
    r = np.random.RandomState(1000 + C)
    return {"gamma": r.uniform(0.5, 1.5, C).astype(np.float32), "beta": (0.3 * r.standard_normal(C)).astype(np.float32),
            "mean": (0.3 * r.standard_normal(C)).astype(np.float32), "var": r.uniform(1e-3, 4.0, C).astype(np.float32),
            "conv_bias": r.standard_normal(C).astype(np.float32)}


FOLD_ABSENT = (None, "gamma", "beta", "conv_bias")


def fold_reference(v, absent, eps=FOLD_EPS):
    """[2, C] fp32: the numpy fp64 evaluation rounded to fp32."""
    C = v["mean"].size
    g = np.ones(C) if absent == "gamma" else v["gamma"].astype(np.float64)
    b = np.zeros(C) if absent == "beta" else v["beta"].astype(np.float64)
    cb = np.zeros(C) if absent == "conv_bias" else v["conv_bias"].astype(np.float64)
    scale = g / np.sqrt(v["var"].astype(np.float64) + eps)
    shift = b + (cb - v["mean"].astype(np.float64)) * scale
    return np.stack([scale, shift]).astype(np.float32)


def check_fold(got, v, absent, label=""):
    """Within 1 fp32 ulp of the reference."""
    want = fold_reference(v, absent)
    got = np.asarray(got, dtype=np.float32).reshape(want.shape)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{label} C={want.shape[1]} absent={absent}: worst err {float((err / ulp).max()):.3g} ulp")
    assert np.isfinite(got).all() and (err <= ulp).all()


# ---- the network case F1 ----------------------------------------------------------------------------------------------------------------------------
# ResNetForMMBEV([1, 1], channels=(64, 128)) on a (2, 3, 40, 72) input, in .eval() under no_grad, with seeded non-trivial BatchNorm state.  Per feature
# map, relative L2 against the unconverted net in fp64 on the CPU; the rule of the GPU test:
#     err(fold) <= err(un-fused "hip", same precision) + 4 * max(err(fp32 torch eval), 1e-6)
# The fold differs from the un-fused path only by fp32 epilogue roundings; the factor 4 is the project's rule for the codec.
F1_LAYERS, F1_CHANNELS, F1_INPUT = [1, 1], (64, 128), (2, 3, 40, 72)
F1_ASSERTED = ("bf16", "f16x3")      # f16 is recorded only


def f1_net():
    """The fp32 CPU net in .eval(): seeded weights, and BatchNorm state gamma in [0.5, 1.5], beta ~ N(0, 0.3), mean ~ N(0, 0.3), var in [0.5, 2]."""
    from diffusiondepth_amd.model import ResNetForMMBEV
    torch.manual_seed(0)
    net = ResNetForMMBEV(F1_LAYERS, channels=F1_CHANNELS)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.3 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net.eval()


@functools.lru_cache(maxsize=None)
def f1_input():
    return torch.randn(F1_INPUT, generator=torch.Generator().manual_seed(12))


@functools.lru_cache(maxsize=None)
def f1_reference():
    """The unconverted net in fp64 on the CPU: one fp64 numpy array per feature map."""
    with torch.no_grad():
        return [f.numpy() for f in f1_net().double()(f1_input().double())]


def rel_l2(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def f1_errors(feats):
    return [rel_l2(f.detach().double().cpu().numpy(), r) for f, r in zip(feats, f1_reference())]
