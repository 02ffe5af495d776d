"""Shared cases of the convolution tests (tests/test_conv_host_emulation.py on the CPU, tests/test_zz_gpu_conv.py on the GPU): shapes, seeded
inputs, the fp64 torch CPU references and the two rules a result is held to.

Exact data.  x, w and grad_y are integers in {-1, 0, 1}: every product and every partial sum is an integer far below 2^24, so an fp32
accumulation in ANY order gives the fp64 result bit for bit, in every precision (the values are exact in bf16 and f16).  The rule is
np.array_equal.  The WIDE cases (f16x3 only, S1 and S2) give one operand the values a + b * 2^-12, a in {-1, 0, 1}, b in {-7 .. 7}: more than
f16's 11 bits, split exactly into hi = f16(v) and lo = v - hi (both multiples of 2^-12), the other operands stay integers (their lo is 0, so
the dropped lo.lo term is 0).  Every term and partial sum is then a multiple of 2^-12, exact in fp32 while its magnitude stays below 2^12; the
builder asserts K * max|term| < 2^11 for the forward's K = 9 Cin, and < 2^12 -- still 24 bits -- for the K of each gradient (the data gradient of
a 256-channel output adds 2304 terms).  A kernel that silently runs ONE f16 MFMA on such data is wrong on nearly every output.

Real-valued data (N(0, 1), unscaled, on S2 and D1), per element |got - ref64| <= tol with S the same convolution of the absolute values in fp64
and K the number of accumulated terms:
    bf16 / f16   ref64 on operands rounded to that type     tol = (K + 1) * 2^-23 * S              (worst case of any fp32 summation order)
    f16x3        ref64 on the unrounded operands            tol = (2^-18 + (K + 1) * 2^-23) * S
These are caps, not precision claims; check_real also returns the ratio to the project's usual 4 * max(|ref32 - ref64|, 2^-23 |ref64|)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
CONV, DECONV = 0, 1                      # dd_conv_op
PRECISIONS = {"bf16": 2, "f16": 3, "f16x3": 4}      # name -> dd_precision
KEYS = ("y", "grad_x", "grad_w")

# name -> (op, (B, Cin, Cout, H, W)); H, W = input size
SHAPES = {
    "S1": (CONV, (2, 64, 256, 9, 35)),        # ragged both ways, more than one tile each way; the data gradient has N = 64
    "S2": (CONV, (1, 192, 256, 17, 33)),      # six K-chunks of 32; the data gradient has N = 192
    "S3": (CONV, (1, 64, 64, 3, 5)),          # smaller than any tile, halo on every side
    "S4": (CONV, (3, 64, 256, 40, 70)),       # 8400 pixels = 180 pixel tiles of the weight gradient: 23 splits of 8, the last one partial (4)
    "D1": (DECONV, (2, 256, 256, 5, 9)),
    "D2": (DECONV, (1, 64, 128, 11, 19)),
}
EXACT = [(n, p, "int") for n in SHAPES for p in PRECISIONS]
WIDE = [(n, "f16x3", "wide_" + role) for n in ("S1", "S2") for role in ("x", "w", "grad_y")]
REAL = [(n, p, "normal") for n in ("S2", "D1") for p in PRECISIONS]


def case_id(c):
    return "-".join(c)


def shapes_of(name):
    """(x, w, y) shapes."""
    op, (B, Cin, Cout, H, W) = SHAPES[name]
    if op == CONV:
        return (B, Cin, H, W), (Cout, Cin, 3, 3), (B, Cout, H, W)
    return (B, Cin, H, W), (Cin, Cout, 2, 2), (B, Cout, 2 * H, 2 * W)


def terms(name):
    """Accumulated terms K of (y, grad_x, grad_w)."""
    op, (B, Cin, Cout, H, W) = SHAPES[name]
    if op == CONV:
        return {"y": 9 * Cin, "grad_x": 9 * Cout, "grad_w": B * H * W}
    return {"y": Cin, "grad_x": 4 * Cout, "grad_w": B * H * W}


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, grad_y.  Treat as read-only (cached)."""
    xs, ws, ys = shapes_of(name)
    g = torch.Generator().manual_seed(7919 * (list(SHAPES).index(name) + 1) + len(kind))
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
        for t in out.values():      # the exactness conditions (module docstring)
            assert torch.equal(t.double() * 4096, (t.double() * 4096).round()), "every value is a multiple of 2^-12"
        if kind.startswith("wide_"):
            big = 1.0 + 7 * 2.0 ** -12
            op, (B, Cin, Cout, H, W) = SHAPES[name]
            assert 9 * Cin * big < 2 ** 11
            assert all(k * (big + 2.0 ** -11) < 2 ** 12 for k in terms(name).values())
    return out


def _reference(op, x, w, gy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = F.conv2d(x, w, None, 1, 1) if op == CONV else F.conv_transpose2d(x, w, None, 2)
    y.backward(gy)
    return {"y": y.detach().double().numpy(), "grad_x": x.grad.double().numpy(), "grad_w": w.grad.double().numpy()}


def _rounded(t, prec):
    if prec == "bf16":
        return t.to(torch.bfloat16).double()
    if prec == "f16":
        return t.to(torch.float16).double()
    return t.double()


@functools.lru_cache(maxsize=None)
def reference(name, kind, operands="exact"):
    """fp64 torch CPU reference: dict KEYS -> fp64 numpy.  operands: "exact" (fp64 of the fp32 inputs), "bf16" / "f16" (operands rounded to that
    type first), "abs" / "abs_bf16" / "abs_f16" (absolute values: the S of the tolerance), "fp32" (evaluated in fp32)."""
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
        same = np.array_equal(got, ref[k])
        print(f"{label} {name} {kind} {k}: max|ref| {np.abs(ref[k]).max():.6g} differing {int((got != ref[k]).sum())} of {got.size}")
        if not same:
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
