"""Shared cases of the tests of include/ddepth_conv_scaled.h (the two gradients of the training convolutions on a grad_y rescaled by a power of
two; tests/test_conv_scaled_host_emulation.py on the CPU, tests/test_zz_gpu_conv_scaled.py on the GPU).  Shapes, seeded inputs and the fp64
references come from tests/conv_cases.py ("cc"), tests/conv_pw_cases.py ("pw") and tests/conv_ragged_cases.py ("rg"); a case is named
"cc:S2", "pw:P2", "rg:P2".

The rule (``scale_of``, computed here in numpy, never taken from the code under test):
    amax = the largest finite |grad_y|;  s = 2^(14 - floor(log2 amax)) from amax's exponent field, the shift held to +-126;  amax == 0: s = 1.

What a result is held to:
  equivariance   run(2^k grad_y) == 2^k run(grad_y), np.array_equal, k in K_SMALL: both factors are powers of two, so the operands are the same bits.
  caps           grad_y 2^-20 ("small") and grad_y 2^-20 with the middle element set to 4096 * 2^-20 ("spike"), N(0, 1) data.  Per element
                 |got - ref64| <= tol, S the same gradient of the absolute values in fp64, K the accumulated terms (those of conv_cases.check_real):
                     f16     ref64 on x and w rounded to f16 and grad_y rounded as the rule says, f16(grad_y s) / s;   tol = (K + 1) 2^-23 S
                     f16x3   ref64 on the unrounded tensors;                                                          tol = (2^-18 + (K + 1) 2^-23) S
                 Derived, not tuned: (K + 1) 2^-23 S is the worst case of any fp32 summation order, 2^-18 the split pair's 2 x 2^-22 for two
                 operands with room for the dropped lo.lo term and the lo halves that go subnormal below |s v| = 2^-3.
  exact          integer data {-1, 0, 1} times 2^-20: the result equals 2^-20 times the fp64 integer reference exactly.
"""
import functools

import numpy as np
import torch

import conv_cases as CC
import conv_pw_cases as PC
import conv_ragged_cases as RC

ULP = 2.0 ** -23
CONV, DECONV, CONV1X1 = 0, 1, 2
PRECISIONS = {"bf16": 2, "f16": 3, "f16x3": 4}      # name -> dd_precision
F16_MODES = ("f16", "f16x3")
KEYS = ("grad_x", "grad_w")
AMAX_EXP = 14
K_SMALL = (-24, -20, -14, 16)
_SRC = {"cc": CC, "pw": PC, "rg": RC}

EQUIVARIANCE = ("cc:S3", "rg:R1", "rg:T1", "rg:P1", "pw:P3")
CAPS = ("cc:S2", "rg:R2", "cc:D1", "rg:T2", "pw:P2", "rg:P2")
EXACT = ("cc:S1", "cc:S4", "cc:D2", "pw:P4", "pw:P5")      # S4: 23 splits, P4: 9 -- the reduce twin adds more than one partial
BF16_IDENTITY = ("rg:R1", "rg:T1", "rg:P1")
BLOCK64_IDENTITY = ("cc:S1", "cc:D1")
EDGE = ("rg:R1", "rg:T1", "rg:P1")


def geometry(case):
    """(op, (B, Cin, Cout, H, W))."""
    src, name = case.split(":")
    return (CONV1X1, PC.SHAPES[name]) if src == "pw" else _SRC[src].SHAPES[name]


def shapes(case):
    """(x, w, y) shapes."""
    return RC.shapes_for(*geometry(case))


def terms(case):
    src, name = case.split(":")
    return _SRC[src].terms(name)


def inputs(case, kind="normal"):
    """dict of fp32 numpy arrays x, w, grad_y at unit scale (copies: free to change)."""
    src, name = case.split(":")
    return {k: v.numpy().copy() for k, v in _SRC[src].make_inputs(name, kind).items()}


def scale_of(grad_y):
    """s of the rule, a Python float (a power of two)."""
    a = np.abs(np.asarray(grad_y, dtype=np.float32)).ravel()
    a = a[np.isfinite(a)]
    amax = np.float32(a.max()) if a.size else np.float32(0)
    if amax == 0:
        return 1.0
    e = int(amax.view(np.uint32) >> 23) - 127      # floor(log2 amax); -127 for a subnormal, whose shift is at its limit anyway
    return 2.0 ** int(np.clip(AMAX_EXP - e, -126, 126))


def scale_words(grad_y):
    """The four floats dd_conv_grad_scale writes, as uint32: {s, 1 / s, bits of amax, 0}."""
    a = np.abs(np.asarray(grad_y, dtype=np.float32)).ravel()
    a = a[np.isfinite(a)]
    amax = np.float32(a.max()) if a.size else np.float32(0)
    s = scale_of(grad_y)
    return np.array([np.float32(s).view(np.uint32), np.float32(1.0 / s).view(np.uint32), amax.view(np.uint32), 0], dtype=np.uint32)


def small(grad_y, k):
    return (grad_y.astype(np.float64) * 2.0 ** k).astype(np.float32)      # exact: a power of two, far inside fp32's range


def spike(grad_y):
    g = small(grad_y, -20)
    g.reshape(-1)[g.size // 2] = np.float32(4096 * 2.0 ** -20)
    return g


def variant(case, which):
    """grad_y of the cap cases: "small" (k = -20) or "spike"."""
    gy = inputs(case)["grad_y"]
    return small(gy, -20) if which == "small" else spike(gy)


def _ref64(op, x, w, gy):
    r = RC._reference(op, torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(w)),
                      torch.from_numpy(np.ascontiguousarray(gy)))
    return {k: r[k] for k in KEYS}


def _f16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float16).double().numpy()


@functools.lru_cache(maxsize=None)
def cap_reference(case, which, prec):
    """(ref, tol): dicts KEYS -> fp64 numpy, as the module docstring says."""
    op, _ = geometry(case)
    inp = inputs(case)
    gy = variant(case, which)
    x, w, g = inp["x"].astype(np.float64), inp["w"].astype(np.float64), gy.astype(np.float64)
    if prec == "f16":
        s = scale_of(gy)
        gs = gy * np.float32(s)      # exact in fp32: a power of two
        assert np.array_equal(gs.astype(np.float64), gy.astype(np.float64) * s)
        x, w, g = _f16(inp["x"]), _f16(inp["w"]), _f16(gs) / s
    ref = _ref64(op, x, w, g)
    S = _ref64(op, np.abs(x), np.abs(w), np.abs(g))
    K = terms(case)
    tol = {k: ((0.0 if prec == "f16" else 2.0 ** -18) + (K[k] + 1) * ULP) * S[k] for k in KEYS}
    return ref, tol


def check_caps(result, case, which, prec, label=""):
    ref, tol = cap_reference(case, which, prec)
    bad = []
    for k in KEYS:
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        err = np.abs(got - ref[k])
        worst = float(np.max(err / np.maximum(tol[k], 1e-300)))
        print(f"{label} {case} {which} {prec} {k}: max|ref| {np.abs(ref[k]).max():.3e} max err {err.max():.3e} worst err/tol {worst:.3e}")
        if not np.isfinite(got).all() or not (err <= tol[k]).all():
            bad.append((k, worst))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def exact_reference(case):
    """fp64 reference of the integer data at unit scale."""
    op, _ = geometry(case)
    inp = inputs(case, "int")
    return _ref64(op, *(inp[k].astype(np.float64) for k in ("x", "w", "grad_y")))


def check_exact(result, case, k=-20, label=""):
    ref = exact_reference(case)
    bad = []
    for key in KEYS:
        got = np.asarray(result[key], dtype=np.float64).reshape(ref[key].shape)
        want = ref[key] * 2.0 ** k
        print(f"{label} {case} int * 2^{k} {key}: max|ref| {np.abs(want).max():.6g} differing {int((got != want).sum())} of {got.size}")
        if not np.array_equal(got, want):
            bad.append(key)
    assert not bad, bad


def check_equivariant(scaled_result, base_result, k, label=""):
    """run(2^k grad_y) == 2^k run(grad_y)."""
    bad = []
    for key in KEYS:
        want = base_result[key].astype(np.float64) * 2.0 ** k
        assert np.isfinite(base_result[key]).all() and (np.abs(want[want != 0]) > 2.0 ** -120).all() and (np.abs(want) < 2.0 ** 120).all(), \
            "the comparison itself must stay inside fp32's normal range"
        n = int((scaled_result[key].astype(np.float64) != want).sum())
        print(f"{label} k = {k} {key}: differing {n} of {want.size}")
        if n:
            bad.append((key, n))
    return bad


def power_of_two_into_top_binade(grad_y):
    """grad_y times the power of two that puts amax into [2^14, 2^15): the rule then gives s = 1."""
    g = (grad_y.astype(np.float64) * scale_of(grad_y)).astype(np.float32)
    assert scale_of(g) == 1.0
    return g


def edge_element(case):
    """Index (b, co, y, x) of the grad_y element the Inf / NaN cases replace: inside the image, away from the first channel and pixel."""
    _, _, ys = shapes(case)
    return tuple(s // 2 for s in ys)


def footprint(case, idx):
    """Boolean masks KEYS -> the outputs element `idx` of grad_y takes part in."""
    op, _ = geometry(case)
    xs, ws, _ = shapes(case)
    b, co, y, x = idx
    mx, mw = np.zeros(xs, dtype=bool), np.zeros(ws, dtype=bool)
    if op == CONV:
        mx[b, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        mw[co] = True
    elif op == DECONV:
        mx[b, :, y // 2, x // 2] = True
        mw[:, co] = True
    else:
        mx[b, :, y, x] = True
        mw[co] = True
    return {"grad_x": mx, "grad_w": mw}
