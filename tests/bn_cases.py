"""Shared cases of the BatchNorm tests (tests/test_bn_host_emulation.py on the CPU, tests/test_zz_gpu_bn.py on the GPU): shapes, inputs, the torch
CPU references and the tolerance rule.

Tolerance (the project's rule for every compared tensor): with ref64 the torch CPU evaluation in fp64 of F.batch_norm(training=True) + activation
and its autograd, and ref32 the same evaluation in fp32,
    max|v - ref64| <= 4 * max(max|ref32 - ref64|, 2^-23 * max|ref64|).
The first term is what an fp32 evaluation in another order legitimately differs by, the second one ulp of an fp32 result; the factor covers a
different order of the same roundings.  NaN must sit exactly where ref64 has it.

A flipped activation mask is not a rounding error, so the inputs of the activation cases are built with min|z64| >= 1e-4 over the pre-activation z
(offending values of x are nudged on the CPU until the guard holds; it is asserted) and then EVERY element is compared."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
EPS, MOMENTUM = 1e-5, 0.1
GUARD = 1e-4

# (B, C, H, W): HW = 35, unaligned planes smaller than one workgroup | ragged | a plane of several workgroups | many channels, tiny planes
SHAPES = [(2, 3, 5, 7), (3, 16, 11, 19), (2, 4, 67, 131), (1, 256, 6, 10)]
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "leaky": (2, 0.2)}      # name -> (dd_bn_act, slope)
KEYS = ("y", "grad_x", "grad_weight", "grad_bias", "running_mean", "running_var")

# (act, affine, kind) of every shape: the six act x affine combinations, the cancellation case x = 1000 + N(0, 1) and the one-channel NaN
VARIANTS = [(a, aff, "normal") for a in ACTS for aff in (True, False)] + [("relu", True, "offset"), ("relu", True, "nan")]


def variant_id(v):
    return f"{v[0]}-{'affine' if v[1] else 'plain'}-{v[2]}"


def _act(z, act):
    if act == "relu":
        return F.relu(z)
    if act == "leaky":
        return F.leaky_relu(z, ACTS[act][1])
    return z


def nan_channel(C):
    return C // 2


@functools.lru_cache(maxsize=None)
def make_inputs(shape, act, affine, kind):
    """dict of fp32 CPU tensors x, grad_y, weight / bias (None without affine), running_mean, running_var.  Treat as read-only (cached)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * sum(shape) + 10 * list(ACTS).index(act) + int(affine) + 100 * len(kind))
    x = torch.randn(shape, generator=g)
    if kind == "offset":
        x = x + 1000.0
    gy = torch.randn(shape, generator=g)
    w = (0.5 + torch.rand(C, generator=g)) if affine else None
    b = (0.5 * torch.randn(C, generator=g)) if affine else None
    rm, rv = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if act != "none":
        for _ in range(20):      # nudge what sits within the guard of the activation's kink (moves the statistics a little: repeat)
            bad = _preact64(x, w, b).abs() < GUARD
            if not bad.any():
                break
            x = torch.where(bad, x + 0.01, x)
        assert float(_preact64(x, w, b).abs().min()) >= GUARD, "guard: min|z64| >= 1e-4"
    if kind == "nan":
        x = x.clone()
        x[0, nan_channel(C), 0, 0] = float("nan")
    return {"x": x.contiguous(), "grad_y": gy.contiguous(), "weight": w, "bias": b, "running_mean": rm, "running_var": rv}


def _preact64(x, w, b):
    x = x.double()
    z = F.batch_norm(x, None, None, w.double() if w is not None else None, b.double() if b is not None else None, True, 0.0, EPS)
    return z


@functools.lru_cache(maxsize=None)
def reference(shape, act, affine, kind, dtype):
    """torch CPU: F.batch_norm(training=True) + activation and its autograd in `dtype`; dict of KEYS -> fp64 numpy arrays (None without affine)."""
    inp = make_inputs(shape, act, affine, kind)
    x = inp["x"].detach().to(dtype).clone().requires_grad_(True)
    w = inp["weight"].detach().to(dtype).clone().requires_grad_(True) if affine else None
    b = inp["bias"].detach().to(dtype).clone().requires_grad_(True) if affine else None
    rm, rv = inp["running_mean"].to(dtype).clone(), inp["running_var"].to(dtype).clone()
    y = _act(F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS), act)
    y.backward(inp["grad_y"].to(dtype))
    out = {"y": y.detach(), "grad_x": x.grad, "grad_weight": w.grad if affine else None, "grad_bias": b.grad if affine else None,
           "running_mean": rm, "running_var": rv}
    return {k: (v.double().numpy() if v is not None else None) for k, v in out.items()}


def bound(ref32, ref64):
    ok = np.isfinite(ref64) & np.isfinite(ref32)
    if not ok.any():
        return 0.0
    return 4.0 * max(float(np.max(np.abs(ref32[ok] - ref64[ok]))), ULP * float(np.max(np.abs(ref64[ok]))))


def check(result, shape, act, affine, kind, label=""):
    """result: dict KEYS -> array-like (grad_weight / grad_bias ignored without affine).  Prints every figure, then asserts."""
    r32, r64 = reference(shape, act, affine, kind, torch.float32), reference(shape, act, affine, kind, torch.float64)
    failures = []
    for k in KEYS:
        if r64[k] is None:
            continue
        v = np.asarray(result[k], dtype=np.float64).reshape(r64[k].shape)
        nan_ok = np.array_equal(np.isnan(v), np.isnan(r64[k]))
        fin = ~np.isnan(r64[k])
        err = float(np.max(np.abs(v[fin] - r64[k][fin]))) if fin.any() and nan_ok else float("inf")
        bnd = bound(r32[k], r64[k])
        print(f"{label} {shape} {act} affine={affine} {kind} {k}: err {err:.3e} bound {bnd:.3e} nan_ok {nan_ok}")
        if not nan_ok or not err <= bnd:
            failures.append((k, err, bnd, nan_ok))
    if kind == "nan":      # the NaN stays in its channel
        c = nan_channel(shape[1])
        y = np.asarray(result["y"], dtype=np.float64).reshape(shape)
        gx = np.asarray(result["grad_x"], dtype=np.float64).reshape(shape)
        others = [i for i in range(shape[1]) if i != c]
        assert np.isnan(y[:, c]).all() and np.isfinite(y[:, others]).all()
        assert np.isnan(gx[:, c]).all() and np.isfinite(gx[:, others]).all()
    assert not failures, failures
