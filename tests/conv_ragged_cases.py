"""Shared cases of the extended-channel-range convolution tests (dd_convx_* of include/ddepth_conv.h; tests/test_conv_ragged_host_emulation.py on
the CPU, tests/test_zz_gpu_conv_ragged.py on the GPU): channel counts that are multiples of 8 but not of 64, or beyond 1536, for the 3x3, the
transpose 2x2 and the 1x1 operator.  The rules are those of tests/conv_cases.py, unchanged:

Exact data.  x, w and grad_y are integers in {-1, 0, 1}; an fp32 accumulation in any order gives the fp64 result bit for bit in every precision,
the rule is np.array_equal.  The WIDE cases (f16x3 only) give one operand the values a + b * 2^-12, a in {-1, 0, 1}, b in {-7 .. 7}; the builder
keeps the asserts of conv_cases.make_inputs: K * max|term| < 2^11 for the forward's K, < 2^12 for the K of each gradient.  For the shapes used:
R1 forward 9 * 72 = 648, R2 forward 9 * 216 * (1 + 7 * 2^-12) = 1947.3 < 2^11, R2 gradients 2304 and 594 terms, T2 216 / 352 / 90.

Real-valued data (N(0, 1)), per element |got - ref64| <= tol, S the same convolution of the absolute values in fp64, K the accumulated terms:
    bf16 / f16   ref64 on operands rounded to that type     tol = (K + 1) * 2^-23 * S
    f16x3        ref64 on the unrounded operands            tol = (2^-18 + (K + 1) * 2^-23) * S

Zero padding.  A guarded kernel treats the channels beyond the count as zeros and keeps the accumulation order of the block-64 kernel, so a
ragged shape through dd_convx_* must EQUAL (float values) the block-64 operator on the same tensors zero-padded to 128 channels, cut back to the
real channels: ``zero_padded`` builds those tensors, ``cut`` takes the real part of the results."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import KEYS, PRECISIONS, ULP, _rounded, case_id  # noqa: F401  (re-exported to the tests)

CONV, DECONV, CONV1X1 = 0, 1, 2          # dd_conv_op

# name -> (op, (B, Cin, Cout, H, W)); H, W = input size
SHAPES = {
    "R1": (CONV, (1, 72, 72, 5, 35)),         # K tail of 8 (half an MFMA k-step), N tail of 8, ragged tiles both ways
    "R2": (CONV, (2, 216, 256, 9, 33)),       # the MPViT lateral: six 32-chunks + 24; the data gradient has N = 216
    "R3": (CONV, (1, 88, 216, 3, 5)),         # N = 216 forward, K = 216 in the data gradient, image smaller than a tile
    "R4": (CONV, (1, 2048, 64, 3, 5)),        # beyond 1536: K = 2048 forward, N = 2048 data gradient, 32 x 1 weight-gradient grid
    "R5": (CONV, (1, 8, 24, 3, 5)),           # the lower end: K < one chunk, N < one block
    "R6": (CONV, (1, 728, 216, 2, 3)),        # MPViT trans_fusion.0
    "T1": (DECONV, (1, 72, 72, 3, 5)),        # N = 288: t4 segments start inside 32-row blocks; the data gradient has K = 72 at chunk 16
    "T2": (DECONV, (2, 216, 88, 5, 9)),       # both tails, more than one tile
    "P1": (CONV1X1, (2, 72, 72, 5, 27)),      # 135 pixels = one tile + 7; K tail of 8; two channel blocks per wave with a tail block
    "P2": (CONV1X1, (1, 216, 512, 3, 11)),    # MPViT trans_proj; four channel blocks per wave forward, N = 216 backward
    "P3": (CONV1X1, (1, 2048, 72, 2, 3)),     # beyond 1536
}
EXACT = [(n, p, "int") for n in SHAPES for p in PRECISIONS]
WIDE = [(n, "f16x3", "wide_" + role) for n in ("R1", "R2", "T2") for role in ("x", "w", "grad_y")]
REAL = [(n, p, "normal") for n in ("R2", "T2", "P2") for p in PRECISIONS]
PADDED = ("R1", "T1", "P1")              # the zero-padding identity
PAD_TO = 128


def shapes_for(op, dims):
    """(x, w, y) shapes."""
    B, Cin, Cout, H, W = dims
    if op == CONV:
        return (B, Cin, H, W), (Cout, Cin, 3, 3), (B, Cout, H, W)
    if op == DECONV:
        return (B, Cin, H, W), (Cin, Cout, 2, 2), (B, Cout, 2 * H, 2 * W)
    return (B, Cin, H, W), (Cout, Cin, 1, 1), (B, Cout, H, W)


def shapes_of(name):
    return shapes_for(*SHAPES[name])


def terms(name):
    """Accumulated terms K of (y, grad_x, grad_w)."""
    op, (B, Cin, Cout, H, W) = SHAPES[name]
    taps_f, taps_b = {CONV: (9, 9), DECONV: (1, 4), CONV1X1: (1, 1)}[op]
    return {"y": taps_f * Cin, "grad_x": taps_b * Cout, "grad_w": B * H * W}


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, grad_y.  Treat as read-only (cached)."""
    xs, ws, ys = shapes_of(name)
    g = torch.Generator().manual_seed(15485863 * (list(SHAPES).index(name) + 1) + len(kind))
    out = {}
    for key, shape in (("x", xs), ("w", ws), ("grad_y", ys)):
        if kind == "normal":
            out[key] = torch.randn(shape, generator=g)
            continue
        a = torch.randint(-1, 2, shape, generator=g).double()
        if kind == "wide_" + key:
            a = a + torch.randint(-7, 8, shape, generator=g).double() * 2.0 ** -12
        out[key] = a.float()
        assert torch.equal(out[key].double(), a)
    if kind != "normal":
        for t in out.values():      # the exactness conditions (conv_cases' module docstring)
            assert torch.equal(t.double() * 4096, (t.double() * 4096).round()), "every value is a multiple of 2^-12"
        if kind.startswith("wide_"):
            big = 1.0 + 7 * 2.0 ** -12
            op, (B, Cin, Cout, H, W) = SHAPES[name]
            assert (Cin if op == CONV1X1 else 9 * Cin) * big < 2 ** 11
            assert all(k * (big + 2.0 ** -11) < 2 ** 12 for k in terms(name).values())
    return out


def _reference(op, x, w, gy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = F.conv2d(x, w, None, 1, 1) if op == CONV else F.conv_transpose2d(x, w, None, 2) if op == DECONV else F.conv2d(x, w)
    y.backward(gy)
    return {"y": y.detach().double().numpy(), "grad_x": x.grad.double().numpy(), "grad_w": w.grad.double().numpy()}


@functools.lru_cache(maxsize=None)
def reference(name, kind, operands="exact"):
    """fp64 torch CPU reference: dict KEYS -> fp64 numpy; `operands` as in conv_cases.reference."""
    inp = make_inputs(name, kind)
    op = SHAPES[name][0]
    ts = [inp["x"], inp["w"], inp["grad_y"]]
    if operands == "fp32":
        return _reference(op, *ts)
    prec = operands.replace("abs_", "").replace("abs", "exact")
    ts = [_rounded(t, prec) for t in ts]
    if operands.startswith("abs"):
        ts = [t.abs() for t in ts]
    return _reference(op, *ts)


def check_exact(result, name, kind, label=""):
    ref = reference(name, kind)
    bad = []
    for k in KEYS:
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        print(f"{label} {name} {kind} {k}: max|ref| {np.abs(ref[k]).max():.6g} differing {int((got != ref[k]).sum())} of {got.size}")
        if not np.array_equal(got, ref[k]):
            bad.append(k)
    assert not bad, bad


def check_real(result, name, prec, label=""):
    """Asserts the cap; returns {key: err / usual bound} (recorded by the GPU test, not asserted)."""
    rounded = prec in ("bf16", "f16")
    ref = reference(name, "normal", prec if rounded else "exact")
    S = reference(name, "normal", "abs_" + prec if rounded else "abs")
    r64, r32 = reference(name, "normal"), reference(name, "normal", "fp32")
    K = terms(name)
    bad, ratios = [], {}
    for k in KEYS:
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        tol = ((0.0 if rounded else 2.0 ** -18) + (K[k] + 1) * ULP) * S[k]
        err = np.abs(got - ref[k])
        worst = float(np.max(err / np.maximum(tol, 1e-300)))
        usual = 4.0 * max(float(np.abs(r32[k] - r64[k]).max()), ULP * float(np.abs(r64[k]).max()))
        ratios[k] = float(np.abs(got - r64[k]).max()) / usual
        print(f"{label} {name} {prec} {k}: max err {err.max():.3e} worst err/tol {worst:.3e} ratio to the usual bound {ratios[k]:.3g}")
        if not np.isfinite(got).all() or not (err <= tol).all():
            bad.append((k, worst))
    assert not bad, bad
    return ratios


# ---- the zero-padding identity ------------------------------------------------------------------------------------------------------------
def _pad(t, dims_to):
    out = torch.zeros(dims_to, dtype=t.dtype)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out


def zero_padded(name):
    """(dims, inputs) of PADDED case `name` with both channel counts zero-padded to PAD_TO (real-valued data)."""
    op, (B, Cin, Cout, H, W) = SHAPES[name]
    assert Cin <= PAD_TO and Cout <= PAD_TO
    dims = (B, PAD_TO, PAD_TO, H, W)
    inp = make_inputs(name, "normal")
    xs, ws, ys = shapes_for(op, dims)
    return dims, {"x": _pad(inp["x"], xs), "w": _pad(inp["w"], ws), "grad_y": _pad(inp["grad_y"], ys)}


def cut(name, result):
    """The real channels of a zero-padded result."""
    xs, ws, ys = shapes_of(name)
    take = lambda a, shape: np.ascontiguousarray(np.asarray(a)[tuple(slice(0, s) for s in shape)])
    return {"y": take(result["y"], ys), "grad_x": take(result["grad_x"], xs), "grad_w": take(result["grad_w"], ws)}
