"""Shared cases of the tests of include/ddepth_conv_strided.h (the 3x3 stride-2 pad-1 convolution with an optional bias;
tests/test_conv_strided_host_emulation.py and tests/test_conv_strided_cpu.py on the CPU, tests/test_zz_gpu_conv_strided.py on the GPU): shapes,
seeded inputs, the fp64 torch CPU references ``F.conv2d(x, w, b, 2, 1)`` with autograd, and the rules a result is held to.  The rules are those
of tests/conv_cases.py, unchanged:

Exact data.  x, w, bias and grad_y are integers in {-1, 0, 1}: the rule is np.array_equal in every precision.  The WIDE cases (f16x3 only, Z1 and
Z2) give one of x, w, grad_y the values a + b * 2^-12; the builder keeps the assertions of conv_cases.make_inputs (K * max|term| < 2^11 for the
forward's 9 Cin, < 2^12 for the K of every result).

Real-valued data (N(0, 1)), per element |got - ref64| <= tol with S the same quantity on absolute values in fp64 and K the accumulated terms:
    bf16 / f16   ref64 on x, w and grad_y rounded to that type (the bias is added in fp32: unrounded)    tol = (K + 1) * 2^-23 * S
    f16x3        ref64 on the unrounded operands                                                          tol = (2^-18 + (K + 1) * 2^-23) * S
    K = 9 Cin + 1 for y, 4 Cout for grad_x (the most taps any input pixel has), B Ho Wo for grad_w and grad_bias.
grad_bias is the weight gradient of an all-ones plane: the library sums grad_y as the weight gradient's operand holds it, which is what the
reference on rounded operands does.

Scaled runs (the rules of tests/conv_scaled_cases.py; the scale pair is built here in numpy by its ``scale_words``, never taken from the library):
equivariance run(2^k grad_y) == 2^k run(grad_y), and integer data times 2^-20 exact.

The network case N1 and its precondition are at the end of the file."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import PRECISIONS, ULP, _rounded, case_id  # noqa: F401  (re-exported to the tests)
from conv_scaled_cases import K_SMALL, scale_of, scale_words, small  # noqa: F401

KEYS = ("y", "grad_x", "grad_w", "grad_bias")
GRAD_KEYS = ("grad_x", "grad_w", "grad_bias")

# name -> (B, Cin, Cout, H, W); H, W = input size
SHAPES = {
    "Z1": (2, 64, 128, 9, 67),        # odd x odd -> 5 x 34, more than one tile each way
    "Z2": (1, 192, 64, 16, 34),       # even x even (the absent tap at the last row and column), six K chunks
    "Z3": (1, 64, 64, 3, 5),          # smaller than a tile
    "Z4": (1, 8, 8, 1, 2),            # one output pixel, centre row only, ragged
    "Z5": (2, 3, 64, 10, 37),         # RGB, even x odd
    "Z6": (1, 72, 216, 7, 12),        # ragged both counts, odd x even
    "Z7": (3, 64, 64, 79, 139),       # 40 x 70 outputs: the weight gradient runs many splits with a partial last one
}
BIAS = (True, False)
EXACT = [(n, p, "int") for n in SHAPES for p in PRECISIONS]
WIDE = [(n, "f16x3", "wide_" + role) for n in ("Z1", "Z2") for role in ("x", "w", "grad_y")]
REAL = [(n, p, "normal") for n in ("Z2", "Z5", "Z6") for p in PRECISIONS]
EQUIVARIANCE = ("Z3", "Z4", "Z5")
SCALED_EXACT = ("Z1", "Z7")
PAD64 = "Z1"          # a block-64 shape: equals the same call on tensors zero-padded to the next multiple of 64 (+64 here: 128 / 192)
PAD_RAGGED = "Z6"     # a ragged shape: equals the block-64 instantiation on tensors zero-padded to 128 / 256 channels


def out_size(n):
    return (n - 1) // 2 + 1


def shapes_for(dims):
    """(x, w, bias, y) shapes."""
    B, Cin, Cout, H, W = dims
    return (B, Cin, H, W), (Cout, Cin, 3, 3), (Cout,), (B, Cout, out_size(H), out_size(W))


def shapes_of(name):
    return shapes_for(SHAPES[name])


def terms(name):
    B, Cin, Cout, H, W = SHAPES[name]
    n = B * out_size(H) * out_size(W)
    return {"y": 9 * Cin + 1, "grad_x": 4 * Cout, "grad_w": n, "grad_bias": n}


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, bias, grad_y.  Treat as read-only (cached)."""
    xs, ws, bs, ys = shapes_of(name)
    g = torch.Generator().manual_seed(32452843 * (list(SHAPES).index(name) + 1) + len(kind))
    out = {}
    for key, shape in (("x", xs), ("w", ws), ("bias", bs), ("grad_y", ys)):
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
            assert (9 * SHAPES[name][1] + 1) * big < 2 ** 11
            assert all(k * (big + 2.0 ** -11) < 2 ** 12 for k in terms(name).values())
    return out


def _reference(x, w, b, gy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True) if b is not None else None
    y = F.conv2d(x, w, b, 2, 1)
    y.backward(gy)
    out = {"y": y.detach().double().numpy(), "grad_x": x.grad.double().numpy(), "grad_w": w.grad.double().numpy()}
    # (without a bias the library is handed no grad_bias; the reference keeps the key so that both runs share one comparison)
    out["grad_bias"] = b.grad.double().numpy() if b is not None else gy.double().sum((0, 2, 3)).numpy()
    return out


def reference_of(inp, bias, operands="exact"):
    """fp64 reference of the tensors `inp` (dict of fp32 tensors).  operands: "exact", "bf16" / "f16" (x, w, grad_y rounded to that type first; the
    bias never), "abs" / "abs_bf16" / "abs_f16" (absolute values: the S of the tolerance), "fp32" (evaluated in fp32)."""
    ts = [inp["x"], inp["w"], inp["grad_y"]]
    b = inp["bias"] if bias else None
    if operands == "fp32":
        return _reference(ts[0], ts[1], b, ts[2])
    prec = operands.replace("abs_", "").replace("abs", "exact")
    ts = [_rounded(t, prec) for t in ts]
    b = b.double() if b is not None else None
    if operands.startswith("abs"):
        ts = [t.abs() for t in ts]
        b = b.abs() if b is not None else None
    return _reference(ts[0], ts[1], b, ts[2])


@functools.lru_cache(maxsize=None)
def reference(name, kind, bias, operands="exact"):
    """Computed once per (case, kind, bias, operands) and shared; treat as read-only."""
    return reference_of(make_inputs(name, kind), bias, operands)


def _keys(result):
    return [k for k in KEYS if result.get(k) is not None]


def check_exact(result, name, kind, bias, label="", scale_exp=0):
    """np.array_equal against the fp64 reference (of the gradients: times 2^scale_exp, the scaled runs' integer . 2^-20 rule)."""
    ref = reference(name, kind, bias)
    bad = []
    for k in _keys(result):
        want = ref[k] * 2.0 ** scale_exp if k in GRAD_KEYS else ref[k]
        got = np.asarray(result[k], dtype=np.float64).reshape(want.shape)
        print(f"{label} {name} {kind} bias={bias} {k}: max|ref| {np.abs(want).max():.6g} differing {int((got != want).sum())} of {got.size}")
        if not np.array_equal(got, want):
            bad.append(k)
    assert not bad, bad


def check_real(result, name, prec, bias, label=""):
    """Asserts the cap; returns {key: worst err / tol}."""
    rounded = prec in ("bf16", "f16")
    ref = reference(name, "normal", bias, prec if rounded else "exact")
    S = reference(name, "normal", bias, "abs_" + prec if rounded else "abs")
    K = terms(name)
    bad, ratios = [], {}
    for k in _keys(result):
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        tol = ((0.0 if rounded else 2.0 ** -18) + (K[k] + 1) * ULP) * S[k]
        err = np.abs(got - ref[k])
        ratios[k] = float(np.max(err / np.maximum(tol, 1e-300)))
        print(f"{label} {name} {prec} bias={bias} {k}: max err {err.max():.3e} worst err/tol {ratios[k]:.3e}")
        if not np.isfinite(got).all() or not (err <= tol).all():
            bad.append((k, ratios[k]))
    assert not bad, bad
    return ratios


def check_equivariant(scaled_result, base_result, k, label=""):
    """run(2^k grad_y) == 2^k run(grad_y) for every gradient present; returns the list of failures."""
    bad = []
    for key in GRAD_KEYS:
        if base_result.get(key) is None:
            continue
        want = base_result[key].astype(np.float64) * 2.0 ** k
        assert np.isfinite(base_result[key]).all() and (np.abs(want[want != 0]) > 2.0 ** -120).all() and (np.abs(want) < 2.0 ** 120).all(), \
            "the comparison itself must stay inside fp32's normal range"
        n = int((scaled_result[key].astype(np.float64) != want).sum())
        print(f"{label} k = {k} {key}: differing {n} of {want.size}")
        if n:
            bad.append((key, n))
    return bad


# ---- the zero-padding identities ----------------------------------------------------------------------------------------------------------------
def _pad(t, shape):
    out = torch.zeros(shape, dtype=t.dtype)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out


def zero_padded(name, cin_to, cout_to):
    """(dims, inputs) of case `name` (real-valued data) with its channel counts zero-padded to cin_to / cout_to."""
    B, Cin, Cout, H, W = SHAPES[name]
    assert Cin <= cin_to and Cout <= cout_to
    dims = (B, cin_to, cout_to, H, W)
    inp = make_inputs(name, "normal")
    return dims, {k: _pad(inp[k], s) for k, s in zip(("x", "w", "bias", "grad_y"), shapes_for(dims))}


def cut(name, result):
    """The real channels of a zero-padded result."""
    xs, ws, bs, ys = shapes_of(name)
    take = lambda a, shape: None if a is None else np.ascontiguousarray(np.asarray(a)[tuple(slice(0, s) for s in shape)])
    return {"y": take(result["y"], ys), "grad_x": take(result["grad_x"], xs), "grad_w": take(result["grad_w"], ws),
            "grad_bias": take(result.get("grad_bias"), bs)}


# ---- the network case N1 ------------------------------------------------------------------------------------------------------------------------
# ResNetForMMBEV([1, 1], channels=(64, 128), strides=(2, 2)) in .train(): six convolutions (per stage conv1 s2, conv2 s1 and the biased downsample
# s2), four BatchNorms, two feature maps.  The loss is sum_i (f_i . u_i).sum() with fixed upstream gradients u_i.  The GPU test asserts, per
# gradient tensor and per feature map, relative L2 against the fp64 CPU reference:  f16x3 <= 5e-3, bf16 <= 2e-1 (the project's bounds,
# tests/test_zz_gpu_conv.py).  The precondition -- checked on the CPU by tests/test_conv_strided_cpu.py -- is what the arithmetic alone does: the
# same net in fp64 with the operands of every convolution (x, w, grad_y) rounded ONCE to the operand type, must stay within HALF of each bound.
N1_LAYERS, N1_CHANNELS, N1_STRIDES = [1, 1], (64, 128), (2, 2)
N1_INPUT = (2, 3, 40, 72)
N1_BOUNDS = {"f16x3": 5e-3, "bf16": 2e-1}


def n1_net():
    """The fp32 CPU net, seeded, in .train()."""
    from diffusiondepth_amd.model import ResNetForMMBEV
    torch.manual_seed(0)
    return ResNetForMMBEV(N1_LAYERS, channels=N1_CHANNELS, strides=N1_STRIDES).train()


@functools.lru_cache(maxsize=None)
def n1_data():
    """(x, [u_0, u_1]) fp32 CPU tensors: x first, then one upstream gradient per feature map, from one generator in that order."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N1_INPUT, generator=g)
    B, _, H, W = N1_INPUT
    ups = []
    for c, s in zip(N1_CHANNELS, N1_STRIDES):
        H, W = out_size(H) if s == 2 else H, out_size(W) if s == 2 else W
        ups.append(torch.randn((B, c, H, W), generator=g))
    return x, ups


def n1_run(net, x, ups):
    """One training step of `net` on (x, ups) -> (features, {parameter name: gradient}) as fp64 numpy."""
    net.zero_grad(set_to_none=True)
    feats = net(x)
    sum((f * u).sum() for f, u in zip(feats, ups)).backward()
    return [f.detach().double().cpu().numpy() for f in feats], {n: p.grad.detach().double().cpu().numpy() for n, p in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def n1_reference():
    """The unconverted net in fp64 on the CPU."""
    x, ups = n1_data()
    return n1_run(n1_net().double(), x.double(), [u.double() for u in ups])


def _round_operand(t, prec):
    """fp64 tensor of what the kernels hold of the fp32 value t: bf16(t), f16(t), or the pair f16(t) + f16(t - f16(t))."""
    t32 = t.float()
    if prec == "bf16":
        return t32.to(torch.bfloat16).double()
    hi = t32.to(torch.float16)
    if prec == "f16":
        return hi.double()
    lo = (t32 - hi.float()).to(torch.float16)
    return hi.double() + lo.double()


class _RoundedConv(torch.autograd.Function):
    """F.conv2d in fp64 on operands rounded once: x and w in the forward, grad_y (and again x, w) in the backward.  The bias is not an operand."""

    @staticmethod
    def forward(ctx, x, w, b, stride, prec):
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, prec, b is not None)
        return F.conv2d(_round_operand(x, prec), _round_operand(w, prec), b, stride, 1)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, prec, has_bias = ctx.conf
        g = _round_operand(gy, prec)
        gx = torch.nn.grad.conv2d_input(x.shape, _round_operand(w, prec), g, stride, 1)
        gw = torch.nn.grad.conv2d_weight(_round_operand(x, prec), w.shape, g, stride, 1)
        return gx, gw, g.sum((0, 2, 3)) if has_bias else None, None, None


class _RoundedConvModule(torch.nn.Module):
    def __init__(self, conv, prec):
        super().__init__()
        self.weight, self.bias, self.stride, self.prec = conv.weight, conv.bias, conv.stride, prec

    def forward(self, x):
        return _RoundedConv.apply(x, self.weight, self.bias, self.stride, self.prec)


def _swap_convs(module, prec):
    for name, child in list(module.named_children()):
        if isinstance(child, torch.nn.Conv2d):
            setattr(module, name, _RoundedConvModule(child, prec))      # (same parameter tensors, same names)
        else:
            _swap_convs(child, prec)
    return module


@functools.lru_cache(maxsize=None)
def n1_emulation(prec):
    """N1 in fp64 with every convolution's operands rounded once to `prec`: what the arithmetic alone does."""
    x, ups = n1_data()
    net = _swap_convs(copy.deepcopy(n1_net().double()), prec)
    return n1_run(net, x.double(), [u.double() for u in ups])


def rel_l2(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def n1_errors(result, reference=None):
    """({parameter name: relative L2 of its gradient}, [relative L2 per feature map]) of an n1_run result against the fp64 reference."""
    ref_f, ref_g = reference if reference is not None else n1_reference()
    feats, grads = result
    return {n: rel_l2(grads[n], ref_g[n]) for n in ref_g}, [rel_l2(f, r) for f, r in zip(feats, ref_f)]
