"""Shared cases of the pointwise (1x1) convolution tests (tests/test_conv_pw_host_emulation.py on the CPU, tests/test_zz_gpu_conv_neck.py on the
GPU): shapes, seeded inputs, the fp64 torch CPU references of F.conv2d(x, w) with a 1x1 weight, and the two rules of tests/conv_cases.py.

Exact data.  x, w and grad_y are integers in {-1, 0, 1}: an fp32 accumulation in any order gives the fp64 result bit for bit in every precision;
the rule is np.array_equal.  The WIDE cases (f16x3 only; P1 and P2, where B * H * W < 4090 and Cin, Cout <= 1024) give one operand the values
a + b * 2^-12, a in {-1, 0, 1}, b in {-7 .. 7}, which one f16 cannot carry; the builder asserts the exactness conditions of
conv_cases.make_inputs with the K of a 1x1: Cin terms forward, Cout for the data gradient, B * H * W for the weight gradient.

Real-valued data (N(0, 1), on P2), per element |got - ref64| <= tol, S the same convolution of the absolute values in fp64, K the terms:
    bf16 / f16   ref64 on operands rounded to that type     tol = (K + 1) * 2^-23 * S
    f16x3        ref64 on the unrounded operands            tol = (2^-18 + (K + 1) * 2^-23) * S

Shapes: the smallest at which the kernels can still go wrong (kPwTile = 128 consecutive pixels of a plane per workgroup, 32 per wave)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import KEYS, PRECISIONS, ULP, _rounded, case_id  # noqa: F401  (re-exported to the tests)

CONV1X1 = 2                              # dd_conv_op
PW_TILE = 128                            # kPwTile of csrc/dd_conv.h

# name -> (B, Cin, Cout, H, W)
SHAPES = {
    "P1": (2, 64, 192, 9, 35),           # P = 315: odd (planes start off 16 bytes), ragged against any tile; the data gradient has N = 64
    "P2": (1, 192, 512, 11, 38),         # the deepest level's real plane, P = 418; twelve K steps; four channel blocks per wave forward, two backward
    "P3": (1, 64, 64, 1, 3),             # smaller than any tile
    "P4": (3, 64, 128, 40, 70),          # 8400 pixels = 66 pixel tiles of the weight gradient: 9 splits of 8, the last one partial (2)
    "P5": (2, 128, 64, 4, 32),           # P = 128: exactly one tile per image, an image boundary on a tile boundary
}
EXACT = [(n, p, "int") for n in SHAPES for p in PRECISIONS]
WIDE = [(n, "f16x3", "wide_" + role) for n in ("P1", "P2") for role in ("x", "w", "grad_y")]
REAL = [("P2", p, "normal") for p in PRECISIONS]


def shapes_of(name):
    """(x, w, y) shapes."""
    B, Cin, Cout, H, W = SHAPES[name]
    return (B, Cin, H, W), (Cout, Cin, 1, 1), (B, Cout, H, W)


def terms(name):
    """Accumulated terms K of (y, grad_x, grad_w)."""
    B, Cin, Cout, H, W = SHAPES[name]
    return {"y": Cin, "grad_x": Cout, "grad_w": B * H * W}


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, grad_y.  Treat as read-only (cached)."""
    xs, ws, ys = shapes_of(name)
    g = torch.Generator().manual_seed(104729 * (list(SHAPES).index(name) + 1) + len(kind))
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
            B, Cin, Cout, H, W = SHAPES[name]
            assert B * H * W < 4090 and Cin <= 1024 and Cout <= 1024
            assert Cin * big < 2 ** 11
            assert all(k * (big + 2.0 ** -11) < 2 ** 12 for k in terms(name).values())
    return out


def _reference(x, w, gy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = F.conv2d(x, w)
    y.backward(gy)
    return {"y": y.detach().double().numpy(), "grad_x": x.grad.double().numpy(), "grad_w": w.grad.double().numpy()}


@functools.lru_cache(maxsize=None)
def reference(name, kind, operands="exact"):
    """fp64 torch CPU reference: dict KEYS -> fp64 numpy; `operands` as in conv_cases.reference."""
    inp = make_inputs(name, kind)
    ts = [inp["x"], inp["w"], inp["grad_y"]]
    if operands == "fp32":
        return _reference(*ts)
    prec = operands.replace("abs_", "").replace("abs", "exact")
    ts = [_rounded(t, prec) for t in ts]
    if operands.startswith("abs"):
        ts = [t.abs() for t in ts]
    return _reference(*ts)


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
