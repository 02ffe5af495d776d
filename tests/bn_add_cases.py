"""Shared cases of the BatchNorm-with-addend tests (tests/test_bn_add_host_emulation.py on the CPU, tests/test_zz_gpu_bn_add.py on the GPU): the
shapes of tests/bn_cases.py, inputs with an addend r ~ N(0, 1), the torch CPU references and the tolerance rule.

    pre    y = act(bn(x) + r)     a BasicBlock's tail
    post   y = act(bn(x)) + r     the FPN's top-down add

Tolerance: bn_cases.bound, reused -- max|v - ref64| <= 4 * max(max|ref32 - ref64|, 2^-23 * max|ref64|) with ref32 / ref64 the torch CPU evaluation
of the expression above and its autograd in fp32 / fp64.  NaN must sit exactly where ref64 has it.

A flipped activation mask is not a rounding error, so the activation cases are built with min|kink64| >= 1e-4 (asserted) and then EVERY element is
compared.  The kink is z + r in "pre" mode: r is nudged by +0.01 where |z64 + r| < 1e-4, in one pass, because r does not move the statistics.
In "post" mode the kink is z, and x carries the nudge of bn_cases.make_inputs."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import bn_cases as BC

SHAPES = BC.SHAPES
ACTS = BC.ACTS
MODES = {"pre": 0, "post": 1}      # name -> dd_bn_add_mode
KEYS = ("y", "grad_x", "grad_addend", "grad_weight", "grad_bias", "running_mean", "running_var")
GUARD = BC.GUARD

# (mode, act, affine, kind) of every shape
VARIANTS = [(m, a, aff, "normal") for m in MODES for a in ACTS for aff in (True, False)] + [("pre", "relu", True, "offset"), ("pre", "relu", True, "nan")]


def variant_id(v):
    return f"{v[0]}-{v[1]}-{'affine' if v[2] else 'plain'}-{v[3]}"


@functools.lru_cache(maxsize=None)
def make_inputs(shape, mode, act, affine, kind):
    """bn_cases.make_inputs (x, grad_y, weight, bias, running_mean, running_var) plus "addend".  Treat as read-only (cached)."""
    inp = dict(BC.make_inputs(shape, act, affine, kind))
    g = torch.Generator().manual_seed(77 + 1000 * sum(shape) + 10 * list(ACTS).index(act) + int(affine) + 100 * len(kind) + 5 * MODES[mode])
    r = torch.randn(shape, generator=g)
    if act != "none":
        z = BC._preact64(inp["x"], inp["weight"], inp["bias"])
        if mode == "pre":
            r = torch.where((z + r.double()).abs() < GUARD, r + 0.01, r)      # (a NaN z compares false: nothing to guard there)
            kink = z + r.double()
        else:
            kink = z
        kink = kink[~torch.isnan(kink)]
        assert float(kink.abs().min()) >= GUARD, "guard: min|kink64| >= 1e-4"
    inp["addend"] = r.contiguous()
    return inp


def _act(z, act):
    return BC._act(z, act)


@functools.lru_cache(maxsize=None)
def reference(shape, mode, act, affine, kind, dtype):
    """torch CPU: act(bn(x) + r) / act(bn(x)) + r and its autograd in `dtype`; dict of KEYS -> fp64 numpy arrays (None without affine)."""
    inp = make_inputs(shape, mode, act, affine, kind)
    x = inp["x"].detach().to(dtype).clone().requires_grad_(True)
    r = inp["addend"].detach().to(dtype).clone().requires_grad_(True)
    w = inp["weight"].detach().to(dtype).clone().requires_grad_(True) if affine else None
    b = inp["bias"].detach().to(dtype).clone().requires_grad_(True) if affine else None
    rm, rv = inp["running_mean"].to(dtype).clone(), inp["running_var"].to(dtype).clone()
    z = F.batch_norm(x, rm, rv, w, b, True, BC.MOMENTUM, BC.EPS)
    y = _act(z + r, act) if mode == "pre" else _act(z, act) + r
    y.backward(inp["grad_y"].to(dtype))
    out = {"y": y.detach(), "grad_x": x.grad, "grad_addend": r.grad, "grad_weight": w.grad if affine else None,
           "grad_bias": b.grad if affine else None, "running_mean": rm, "running_var": rv}
    return {k: (v.double().numpy() if v is not None else None) for k, v in out.items()}


def check(result, shape, mode, act, affine, kind, label=""):
    """result: dict KEYS -> array-like (grad_weight / grad_bias ignored without affine).  Prints every figure, then asserts."""
    r32, r64 = reference(shape, mode, act, affine, kind, torch.float32), reference(shape, mode, act, affine, kind, torch.float64)
    failures = []
    for k in KEYS:
        if r64[k] is None:
            continue
        v = np.asarray(result[k], dtype=np.float64).reshape(r64[k].shape)
        nan_ok = np.array_equal(np.isnan(v), np.isnan(r64[k]))
        fin = ~np.isnan(r64[k])
        err = float(np.max(np.abs(v[fin] - r64[k][fin]))) if fin.any() and nan_ok else float("inf")
        bnd = BC.bound(r32[k], r64[k])
        print(f"{label} {shape} {mode} {act} affine={affine} {kind} {k}: err {err:.3e} bound {bnd:.3e} nan_ok {nan_ok}")
        if not nan_ok or not err <= bnd:
            failures.append((k, err, bnd, nan_ok))
    if kind == "nan":      # the NaN stays in its channel; the addend's gradient has none (a NaN y passes grad_y through the ReLU)
        c = BC.nan_channel(shape[1])
        others = [i for i in range(shape[1]) if i != c]
        for k in ("y", "grad_x"):
            v = np.asarray(result[k], dtype=np.float64).reshape(shape)
            assert np.isnan(v[:, c]).all() and np.isfinite(v[:, others]).all(), k
        assert np.isfinite(np.asarray(result["grad_addend"], dtype=np.float64)).all()
    assert not failures, failures
