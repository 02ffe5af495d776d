"""Shared cases of the latent-codec convolution tests (tests/test_codec_host_emulation.py on the CPU, tests/test_zz_gpu_codec.py on the GPU):
shapes, seeded inputs, the fp64 torch CPU references (through autograd) and the rules a result is held to.  Sizes are the op's INPUT size.

Exact data.  x, w, bias and grad_y are integers in {-1, 0, 1}: every product and every partial sum is an integer far below 2^24 (the longest sum,
a weight or bias gradient of T4, has fewer than 2^13 terms), so fp32 in ANY order equals fp64 bit for bit.  The rule is np.array_equal on y,
grad_x, grad_w and grad_bias.

Real-valued data (N(0, 1), on T2 and T4), per element |got - ref64| <= (K + 1) * 2^-23 * S, S the same operation on the absolute values in fp64,
K the number of accumulated terms (+ 1 with a bias): the worst case of any fp32 summation order, the cap of tests/conv_cases.py.  check_real
also prints the ratio to the project's usual 4 * max(|ref32 - ref64|, 2^-23 |ref64|); that ratio is recorded, not asserted.

Tail.  z ~ N(0, 3) plus planted -20, -14, 0, 14 and NaN; no other element has sigmoid(z) within 1e-3 (relative) of eps, so fp32 and fp64 agree
on which side of the clamp every element lies.  Forward |got - ref64| <= 8 * 2^-23 * (1 + |ref64|): at most 4 ulp of 1 / s from the exponential, the
addition, two divisions and the subtraction, with a margin of 2.  Backward |got - ref64| <= 8 * 2^-23 * |ref64|, an exact 0 where the clamp is
active and NaN at the NaN."""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
ENC0, ENC1, DEC0, DEC1 = 0, 1, 2, 3      # dd_codec_op
OP_NAMES = {ENC0: "enc0", ENC1: "enc1", DEC0: "dec0", DEC1: "dec1"}
KEYS = ("y", "grad_x", "grad_w", "grad_bias")
EPS = 1e-6

# name -> (op, (B, H, W))
SHAPES = {}
for _op in (ENC0, ENC1, DEC0, DEC1):
    SHAPES["T1-" + OP_NAMES[_op]] = (_op, (2, 3, 5))        # smaller than any tile, halo on every side
    SHAPES["T2-" + OP_NAMES[_op]] = (_op, (1, 17, 35))      # ragged both ways, more than one tile each way
    SHAPES["T5-" + OP_NAMES[_op]] = (_op, (3, 5, 7))        # H * W = 35: no plane but the first starts on a 16-byte boundary
SHAPES["T3-enc0-odd"] = (ENC0, (1, 7, 11))                  # the last tap row / column falls off the image ...
SHAPES["T3-enc0-even"] = (ENC0, (1, 8, 11))                 # ... and does not
SHAPES["T3-dec0"] = (DEC0, (1, 5, 9))
# T4: 20 pixel tiles of the weight gradient (10 rows of the unshifted operand, 70 pixels = two tiles of 64 per row): at kSplitTiles = 8 two full
# splits and one of 4 (asserted from csrc/dd_codec.h by the host-emulation test)
SHAPES["T4-enc0"] = (ENC0, (1, 20, 139))                    # grad_y is 10 x 70
SHAPES["T4-enc1"] = (ENC1, (1, 10, 70))
SHAPES["T4-dec0"] = (DEC0, (1, 10, 70))
SHAPES["T4-dec1"] = (DEC1, (1, 10, 70))
EXACT = [(n, "int") for n in SHAPES]
REAL = [(n, "normal") for n in SHAPES if n.startswith(("T2", "T4"))]


def case_id(c):
    return "-".join(c)


def has_bias(op):
    return op in (DEC0, DEC1)


def out_hw(op, H, W):
    if op == ENC0:
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if op == DEC0:
        return 2 * H, 2 * W
    return H, W


def shapes_of(name):
    """(x, w, bias or None, y) shapes."""
    op, (B, H, W) = SHAPES[name]
    Ho, Wo = out_hw(op, H, W)
    cin, cout = (1, 16) if op == ENC0 else (16, 1) if op == DEC1 else (16, 16)
    wshape = (16, 16, 4, 4) if op == DEC0 else (cout, cin, 3, 3)
    return (B, cin, H, W), wshape, ((cout,) if has_bias(op) else None), (B, cout, Ho, Wo)


def wgrad_tiles(name, tile_w=64):
    """Pixel tiles of the weight gradient: rows of the unshifted operand (grad_y of ENC0, x of DEC0) times the 64-pixel tiles per row."""
    op, (B, H, W) = SHAPES[name]
    Hp, Wp = out_hw(op, H, W) if op == ENC0 else (H, W)
    return B * Hp * (-(-Wp // tile_w))


def header_constants():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusiondepth_amd", "csrc", "dd_codec.h")).read()
    return {k: int(re.search(r"%s = (\d+);" % k, hdr).group(1)) for k in ("kWgTileW", "kSplitTiles", "kMaxSplits")}


def terms(name):
    """Accumulated terms K of every result (the bias counts as one)."""
    op, (B, H, W) = SHAPES[name]
    Ho, Wo = out_hw(op, H, W)
    if op == ENC0:
        return {"y": 9, "grad_x": 4 * 16, "grad_w": B * Ho * Wo}
    if op == ENC1:
        return {"y": 144, "grad_x": 144, "grad_w": B * H * W}
    if op == DEC0:
        return {"y": 4 * 16 + 1, "grad_x": 16 * 16, "grad_w": B * H * W, "grad_bias": B * Ho * Wo}
    return {"y": 144 + 1, "grad_x": 9, "grad_w": B * H * W, "grad_bias": B * H * W}


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """dict of fp32 CPU tensors x, w, bias (None without one), grad_y.  Treat as read-only (cached)."""
    xs, ws, bs, ys = shapes_of(name)
    g = torch.Generator().manual_seed(104729 * (list(SHAPES).index(name) + 1) + len(kind))
    out = {}
    for key, shape in (("x", xs), ("w", ws), ("bias", bs), ("grad_y", ys)):
        if shape is None:
            out[key] = None
        elif kind == "normal":
            out[key] = torch.randn(shape, generator=g)
        else:
            out[key] = torch.randint(-1, 2, shape, generator=g).float()
    if kind != "normal":
        assert max(terms(name).values()) + 1 < 2 ** 13
    return out


def forward(op, x, w, bias):
    if op == ENC0:
        return F.conv2d(x, w, None, 2, 1)
    if op == DEC0:
        return F.conv_transpose2d(x, w, bias, 2, 1)
    return F.conv2d(x, w, bias, 1, 1)


def _reference(op, x, w, bias, gy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    bias = bias.detach().clone().requires_grad_(True) if bias is not None else None
    y = forward(op, x, w, bias)
    y.backward(gy)
    out = {"y": y.detach().double().numpy(), "grad_x": x.grad.double().numpy(), "grad_w": w.grad.double().numpy()}
    if bias is not None:
        out["grad_bias"] = bias.grad.double().numpy()
    return out


@functools.lru_cache(maxsize=None)
def reference(name, kind, operands="exact"):
    """fp64 torch CPU reference: dict KEYS -> fp64 numpy.  operands: "exact" (fp64 of the fp32 inputs), "abs" (absolute values: the S of the
    tolerance), "fp32" (evaluated in fp32)."""
    inp = make_inputs(name, kind)
    op = SHAPES[name][0]
    ts = [inp["x"], inp["w"], inp["bias"], inp["grad_y"]]
    if operands != "fp32":
        ts = [None if t is None else t.double() for t in ts]
    if operands == "abs":
        ts = [None if t is None else t.abs() for t in ts]
    return _reference(op, *ts)


def keys_of(name):
    return KEYS if has_bias(SHAPES[name][0]) else KEYS[:3]


def check_exact(result, name, kind, label=""):
    ref = reference(name, kind)
    bad = []
    for k in keys_of(name):
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        same = np.array_equal(got, ref[k])
        print(f"{label} {name} {kind} {k}: max|ref| {np.abs(ref[k]).max():.6g} differing {int((got != ref[k]).sum())} of {got.size}")
        if not same:
            bad.append(k)
    assert not bad, bad


def check_real(result, name, label=""):
    """Asserts the cap; returns {key: err / usual bound} (recorded, not asserted)."""
    ref, S, r32 = reference(name, "normal"), reference(name, "normal", "abs"), reference(name, "normal", "fp32")
    K = terms(name)
    bad, ratios = [], {}
    for k in keys_of(name):
        got = np.asarray(result[k], dtype=np.float64).reshape(ref[k].shape)
        tol = (K[k] + 1) * ULP * S[k]
        err = np.abs(got - ref[k])
        worst = float(np.max(err / np.maximum(tol, 1e-300)))
        usual = 4.0 * max(float(np.abs(r32[k] - ref[k]).max()), ULP * float(np.abs(ref[k]).max()))
        ratios[k] = float(err.max()) / usual
        print(f"{label} {name} {k}: max err {err.max():.3e} worst err/tol {worst:.3e} ratio to the usual bound {ratios[k]:.3g}")
        if not np.isfinite(got).all() or not (err <= tol).all():
            bad.append((k, worst))
    assert not bad, bad
    return ratios


# ---- the decoder's tail -------------------------------------------------------------------------------------------------------------------------
PLANTED = (-20.0, -14.0, 0.0, 14.0, float("nan"))
TAIL_N = 4099      # more than one workgroup, no multiple of 4


@functools.lru_cache(maxsize=None)
def tail_inputs():
    """(z, grad_depth) fp32 CPU tensors; the planted values are z[0 .. 4].  Read-only."""
    g = torch.Generator().manual_seed(6151)
    z = torch.randn(TAIL_N, generator=g) * 3.0
    gd = torch.randn(TAIL_N, generator=g)
    z[:len(PLANTED)] = torch.tensor(PLANTED)
    s = torch.sigmoid(z[len(PLANTED):].double())
    assert bool(((s / EPS - 1.0).abs() > 1e-3).all()), "an element sits on the clamp"
    return z, gd


@functools.lru_cache(maxsize=None)
def tail_reference():
    """fp64: (depth, grad_z) numpy, through autograd of 1 / sigmoid(z).clamp(eps) - 1."""
    z, gd = tail_inputs()
    z64 = z.double().requires_grad_(True)
    depth = 1.0 / torch.sigmoid(z64).clamp(EPS) - 1
    depth.backward(gd.double())
    return depth.detach().numpy(), z64.grad.numpy()


def check_tail(depth, grad_z, label=""):
    z, _ = tail_inputs()
    rd, rg = tail_reference()
    depth, grad_z = np.asarray(depth, dtype=np.float64), np.asarray(grad_z, dtype=np.float64)
    nan = np.isnan(z.numpy())
    assert nan.sum() == 1 and np.isnan(rd[nan]).all()
    assert np.isnan(depth[nan]).all() and np.isnan(grad_z[nan]).all(), "a NaN in z gives NaN out and a NaN gradient"
    ok = ~nan
    ef, eb = np.abs(depth[ok] - rd[ok]), np.abs(grad_z[ok] - rg[ok])
    tf, tb = 8 * ULP * (1 + np.abs(rd[ok])), 8 * ULP * np.abs(rg[ok])
    print(f"{label} tail forward: worst err/tol {np.max(ef / tf):.3e}; backward: worst err/tol {np.max(eb / np.maximum(tb, 1e-300)):.3e}")
    assert np.isfinite(depth[ok]).all() and (ef <= tf).all()
    assert np.isfinite(grad_z[ok]).all() and (eb <= tb).all()
    assert rg[0] == 0.0 and grad_z[0] == 0.0 and grad_z[1] == 0.0, "an exact 0 where the clamp is active (z = -20, -14)"


# ---- the whole codec in .train() ------------------------------------------------------------------------------------------------------------------
def init_codec(dt, seed=2024):
    """N(0, 1) weights scaled by 1 / sqrt(fan-in) (the last convolution by 0.6 more, bias -2: z stays near -2, the depth e^-z inside 0.5 .. 80 m);
    BatchNorm weight 1 + 0.1 N(0, 1), bias 0.1 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in dt.named_parameters():
            if p.dim() == 4:
                fan = p.shape[0] * 4 if n.startswith("conv_inv_transform.0.") else p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g) / fan ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if n.endswith("weight") else 0.0))
        dt.conv_inv_transform[3][0].weight.mul_(0.6)
        dt.conv_inv_transform[3][0].bias.fill_(-2.0)
    return dt


@functools.lru_cache(maxsize=None)
def whole_codec_inputs():
    """B = 2, a 34 x 70 depth map (latent 17 x 35): (depth, latent, grad of t(depth), grad of inv_t(latent)), fp32 CPU.  Read-only."""
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 16, 17, 35, generator=g)
    depth = torch.rand(2, 1, 34, 70, generator=g) * 60.0 + 1.0
    return depth, lat, torch.randn(2, 16, 17, 35, generator=g), torch.randn(2, 1, 34, 70, generator=g)


ZERO_GRADIENT = "grad:conv_inv_transform.0.bias"


def whole_codec_step(dt, dev, dtype):
    """t(depth) and inv_t(latent) of a .train() codec, each with its upstream gradient; -> dict name -> fp64 numpy."""
    depth, lat, g_t, g_inv = (t.to(dev, dtype) for t in whole_codec_inputs())
    dt = dt.to(dev).train()
    dt.zero_grad()
    lat = lat.clone().requires_grad_(True)
    seen = {}
    # the transpose convolution's bias is followed by batch-statistics BatchNorm: its exact gradient, the sum of grad_y per channel, is ZERO.  Its
    # natural scale is the sum of |grad_y| (the S of the real-valued rule); check_whole_codec measures that one tensor against it.
    hook = dt.conv_inv_transform[0].register_forward_hook(lambda m, i, o: o.register_hook(lambda g: seen.__setitem__("s", g.detach().abs().sum((0, 2, 3)))) and None)
    try:
        enc, dec = dt.t(depth), dt.inv_t(lat)
        torch.autograd.backward([enc, dec], [g_t, g_inv])
    finally:
        hook.remove()
    out = {"t(depth)": enc, "inv_t(latent)": dec, "grad_latent": lat.grad, "scale:" + ZERO_GRADIENT: seen["s"]}
    out.update({"grad:" + k: p.grad for k, p in dt.named_parameters()})
    assert all(v is not None for v in out.values())
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def rel_l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-30, np.sqrt((b ** 2).sum())))
