"""The condition FPN's and the HAHI neck's training convolutions, forward and backward, over the C ABI of include/ddepth_conv.h.

What it is for: in .train() the condition FPN's ``conv_lateral[i]`` (Conv3x3 C_i -> 256, no bias) and ``conv_up[j]`` (ConvTranspose2d 256 -> 256,
k2 s2, no bias) and their autograd run as fp32 MIOpen kernels, whatever the precision of the rest of the step.  ``HipConv2d`` and
``HipConvTranspose2d`` run them through csrc/dd_conv.hip on the head's 16-bit MFMA operands (bf16, f16, or the split-f16 pair of "f16x3") with
fp32 accumulation; only ``x`` and the weight are kept for the backward, and a gradient nobody needs is not computed.

    convert_hip_conv(head.conv_lateral, "bf16")      # or: DDIMDepthEstimate_Res(..., conv_backend="hip") / DDEPTH_CONV_BACKEND=hip

The HAHI neck (necks.HAHIHeteroNeck) has twelve more convolutions, eight of them 1x1 (``lateral_convs``, ``conv_proj``, ``trans_proj``; no bias,
a BatchNorm follows).  ``HipConv2d`` serves ``nn.Conv2d(cin, cout, 1, bias=False)`` too, through the pointwise kernels of the library
(dd_conv1x1_*), but the converter replaces a 1x1 only when asked to:

    convert_hip_conv(head.hahineck, "bf16", pointwise=True)      # or: conv_backend="hip+neck" / DDEPTH_CONV_BACKEND=hip+neck

The library route is decided BEFORE the call and taken only when the input and the weight are contiguous fp32 tensors on a HIP device, the
module's precision is "bf16", "f16" or "f16x3", and the channel counts are supported: multiples of 64 in 64..1536, or, for a module converted
with ``channels="any"`` (``conv_backend="hip+all"``), multiples of 8 in 8..2048 through dd_convx_*.  Everything else -- CPU
tensors, the "fp32" / "f16r" / "naive_fp32" precisions, other dtypes or layouts -- calls the torch forward the module inherits.  It is never a
fallback after an error, nothing is copied or converted silently, and there is no CPU library path.

Scale of the incoming gradient (opt-in, ``grad_autoscale``).  The kernels round ``grad_y`` to f16 as it arrives; a training step's gradients are
about 3e-7 (the loss is a mean over millions of pixels), below f16's normal range.  With ``grad_autoscale=True`` the backward of "f16" / "f16x3"
multiplies ``grad_y`` by a power of two taken from its largest finite magnitude on the device, and the result by the inverse
(include/ddepth_conv_scaled.h): nothing else changes, and "bf16" is left as it is.  Off by default -- today's calls and today's bits:

    convert_hip_conv(head.conv_lateral, "f16x3", grad_autoscale=True)      # or: conv_grad_autoscale=True / DDEPTH_CONV_GRAD_AUTOSCALE=1

The backbone (opt-in, ``strided``).  model.ResNetForMMBEV opens every stage with two 3x3 stride-2 pad-1 convolutions, ``conv1`` and the biased
``downsample``, the first of them on the three RGB planes.  ``HipConv2d`` marked ``strided = True`` runs them through include/ddepth_conv_strided.h
(dd_conv3x3s2_*: bias in the epilogue, its gradient from the weight gradient's call, Cin 3 or a multiple of 8); the converter marks a module only
when asked to, and the default replaces exactly what it always replaced:

    convert_hip_conv(backbone, "bf16", channels="any", strided=True)       # or: args.backbone_backend="hip" / DDEPTH_BACKBONE_BACKEND=hip

The backbone in .eval() (opt-in, include/ddepth_conv_fused.h).  There a BatchNorm is a per-channel scale and shift: ``conv_bn_act(conv, bn, x, addend, relu)``
folds it on the device (``bn_fold``) and runs the 3x3 convolution, stride 1 or 2, with scale, shift, the residual add and the ReLU where the accumulator is
stored (``conv_affine_forward``) -- no torch BatchNorm, add or ReLU.  It keeps nothing for a backward and returns None where the call is not native, so the
caller falls back; model.fold_eval_basic_blocks / ``backbone_backend="hip+fold"`` use it for every BasicBlock under no_grad.

A training conv -> BatchNorm pair (opt-in, include/ddepth_conv_stats.h).  In .train() a BatchNorm starts with a pass over the tensor its convolution
has just written; ``conv_bn_train(conv, bn, x, addend)`` runs the 3x3 convolution, stride 1 or 2, with the per-channel fp64 sums taken in its epilogue
(``conv_stats_forward`` / ``ConvStatsFunction``) and hands them to ``HipBatchNorm2d.forward_sums``: no dd_bn_stats.  The backward is the un-fused pair's.
It returns None where one half is not native; model.fuse_conv_bn_stats / ``backbone_backend="hip+stats"`` and the heads' ``conv_bn_stats=True`` use it.
Not covered: the transpose, pointwise and codec convolutions, and statistics in the backward.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import backend

# every symbol include/ddepth_conv.h declares (checked by tests/test_conv_cpu.py)
ABI_SYMBOLS = ["dd_conv_last_error", "dd_conv_supported", "dd_conv_workspace_bytes", "dd_conv3x3_forward", "dd_conv3x3_backward_data",
               "dd_conv3x3_backward_weight", "dd_deconv2x2_forward", "dd_deconv2x2_backward_data", "dd_deconv2x2_backward_weight",
               "dd_conv1x1_forward", "dd_conv1x1_backward_data", "dd_conv1x1_backward_weight",
               "dd_convx_supported", "dd_convx_workspace_bytes", "dd_convx_forward", "dd_convx_backward_data", "dd_convx_backward_weight"]

# every symbol include/ddepth_conv_scaled.h declares (tests/test_conv_scaled_cpu.py); bound on first use, so ABI_SYMBOLS and _lib() stay what they were
ABI_SYMBOLS_SCALED = ["dd_conv_grad_scale", "dd_convx_backward_data_scaled", "dd_convx_backward_weight_scaled"]

# every symbol include/ddepth_conv_strided.h declares (tests/test_conv_strided_cpu.py): the 3x3 stride-2 operator; bound on first use as well
ABI_SYMBOLS_STRIDED = ["dd_conv3x3s2_supported", "dd_conv3x3s2_workspace_bytes", "dd_conv3x3s2_forward", "dd_conv3x3s2_backward_data",
                       "dd_conv3x3s2_backward_weight"]

# every symbol include/ddepth_conv_fused.h declares (tests/test_conv_fused_cpu.py): the folded eval-mode forward; bound on first use as well
ABI_SYMBOLS_FUSED = ["dd_bn_fold", "dd_conv3x3_affine_supported", "dd_conv3x3_affine_workspace_bytes", "dd_conv3x3_affine_forward"]

# every symbol include/ddepth_conv_stats.h declares (tests/test_conv_stats_cpu.py): the training forward that emits the BatchNorm statistics; bound on
# first use as well
ABI_SYMBOLS_STATS = ["dd_conv3x3_stats_supported", "dd_conv3x3_stats_workspace_bytes", "dd_conv3x3_stats_forward"]

OP_CONV3X3, OP_DECONV2X2, OP_CONV1X1 = 0, 1, 2      # dd_conv_op
LIBRARY_PRECISIONS = ("bf16", "f16", "f16x3")
_LIBRARY_PRECISION_IDS = tuple(backend.PRECISIONS[p] for p in LIBRARY_PRECISIONS)
_ENTRY = {OP_CONV3X3: ("dd_conv3x3_forward", "dd_conv3x3_backward_data", "dd_conv3x3_backward_weight"),
          OP_DECONV2X2: ("dd_deconv2x2_forward", "dd_deconv2x2_backward_data", "dd_deconv2x2_backward_weight"),
          OP_CONV1X1: ("dd_conv1x1_forward", "dd_conv1x1_backward_data", "dd_conv1x1_backward_weight")}
_ENTRY_ANY = ("dd_convx_forward", "dd_convx_backward_data", "dd_convx_backward_weight")      # (op, ...): the extended channel range
# the channel contracts: "block64" = multiples of 64 in 64..1536 (dd_conv_*), "any" = multiples of 8 in 8..2048 (dd_convx_*, a superset that
# runs a block-64 shape through the same kernels)
CHANNELS = ("block64", "any")

_ENTRY_SCALED = (None, "dd_convx_backward_data_scaled", "dd_convx_backward_weight_scaled")      # (op, ..., scale, ...): always the extended range

_bound = None
_bound_scaled = None
_bound_strided = None
_bound_fused = None
_bound_stats = None
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_conv_last_error.restype, lib.dd_conv_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_conv_supported.restype, lib.dd_conv_supported.argtypes = c_int, [c_int] * 4
        lib.dd_conv_workspace_bytes.restype = c_int
        lib.dd_conv_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
        for names in _ENTRY.values():
            for n in names:
                f = getattr(lib, n)
                f.restype, f.argtypes = c_int, [c_vp] * 4 + [c_int] * 6 + [c_vp]
        lib.dd_convx_supported.restype, lib.dd_convx_supported.argtypes = c_int, [c_int] * 4
        lib.dd_convx_workspace_bytes.restype = c_int
        lib.dd_convx_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
        for n in _ENTRY_ANY:
            f = getattr(lib, n)
            f.restype, f.argtypes = c_int, [c_int] + [c_vp] * 4 + [c_int] * 6 + [c_vp]
        _bound = lib
    return _bound


def _lib_scaled():
    global _bound_scaled
    if _bound_scaled is None:
        lib = _lib()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_conv_grad_scale.restype, lib.dd_conv_grad_scale.argtypes = c_int, [c_vp, ctypes.c_int64, c_int, c_vp, c_vp]
        for n in _ENTRY_SCALED[1:]:
            f = getattr(lib, n)
            f.restype, f.argtypes = c_int, [c_int] + [c_vp] * 5 + [c_int] * 6 + [c_vp]
        _bound_scaled = lib
    return _bound_scaled


def _lib_strided():
    global _bound_strided
    if _bound_strided is None:
        lib = _lib()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_conv3x3s2_supported.restype, lib.dd_conv3x3s2_supported.argtypes = c_int, [c_int] * 3
        lib.dd_conv3x3s2_workspace_bytes.restype = c_int
        lib.dd_conv3x3s2_workspace_bytes.argtypes = [c_int] * 6 + [ctypes.POINTER(ctypes.c_int64)]
        lib.dd_conv3x3s2_forward.restype, lib.dd_conv3x3s2_forward.argtypes = c_int, [c_vp] * 5 + [c_int] * 6 + [c_vp]
        lib.dd_conv3x3s2_backward_data.restype, lib.dd_conv3x3s2_backward_data.argtypes = c_int, [c_vp] * 5 + [c_int] * 6 + [c_vp]
        lib.dd_conv3x3s2_backward_weight.restype, lib.dd_conv3x3s2_backward_weight.argtypes = c_int, [c_vp] * 6 + [c_int] * 6 + [c_vp]
        _bound_strided = lib
    return _bound_strided


def _lib_fused():
    global _bound_fused
    if _bound_fused is None:
        lib = _lib()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_bn_fold.restype, lib.dd_bn_fold.argtypes = c_int, [c_vp] * 4 + [ctypes.c_double] + [c_vp] * 2 + [c_int, c_vp]
        lib.dd_conv3x3_affine_supported.restype, lib.dd_conv3x3_affine_supported.argtypes = c_int, [c_int] * 4
        lib.dd_conv3x3_affine_workspace_bytes.restype = c_int
        lib.dd_conv3x3_affine_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
        lib.dd_conv3x3_affine_forward.restype, lib.dd_conv3x3_affine_forward.argtypes = c_int, [c_vp] * 6 + [c_int] * 8 + [c_vp]
        _bound_fused = lib
    return _bound_fused


def _lib_stats():
    global _bound_stats
    if _bound_stats is None:
        lib = _lib()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_conv3x3_stats_supported.restype, lib.dd_conv3x3_stats_supported.argtypes = c_int, [c_int] * 4
        lib.dd_conv3x3_stats_workspace_bytes.restype = c_int
        lib.dd_conv3x3_stats_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
        lib.dd_conv3x3_stats_forward.restype, lib.dd_conv3x3_stats_forward.argtypes = c_int, [c_vp] * 6 + [c_int] * 7 + [c_vp]
        _bound_stats = lib
    return _bound_stats


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib().dd_conv_last_error().decode()}")


def _stream(t):
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def precision_id(precision) -> Optional[int]:
    """dd_precision of a precision name the library route runs, else None."""
    pid = backend.PRECISIONS.get(str(precision).lower())      # (the aliases of backend.PRECISIONS count: "fp16", "split_f16")
    return pid if pid in _LIBRARY_PRECISION_IDS else None


def _any(channels) -> bool:
    if channels not in CHANNELS:
        raise ValueError(f"channels must be 'block64' or 'any' (got {channels!r})")
    return channels == "any"


def supported(op: int, cin: int, cout: int, precision, channels="block64") -> bool:
    """dd_conv_supported, or with ``channels="any"`` dd_convx_supported: no device needed, no side effects."""
    p = precision_id(precision)
    query = _lib().dd_convx_supported if _any(channels) else _lib().dd_conv_supported
    return p is not None and bool(query(int(op), int(cin), int(cout), p))


def workspace_for(t: torch.Tensor, op: int, B: int, cin: int, cout: int, H: int, W: int, prec: int, channels="block64") -> torch.Tensor:
    """The device scratch of one call (packed 16-bit weights, or the weight gradient's partial sums), cached per (device, bytes): a shape that
    returns finds its buffer again, and the steady state allocates nothing.  Calls on one stream are ordered, so sites of equal size share a
    buffer.  A first call inside a graph capture would allocate from the capture's pool: call once eagerly before capturing."""
    need = ctypes.c_int64(0)
    if _any(channels):
        _ck(_lib().dd_convx_workspace_bytes(op, B, cin, cout, H, W, prec, ctypes.byref(need)), "dd_convx_workspace_bytes")
    else:
        _ck(_lib().dd_conv_workspace_bytes(op, B, cin, cout, H, W, prec, ctypes.byref(need)), "dd_conv_workspace_bytes")
    key = (t.device.index if t.device.index is not None else torch.cuda.current_device(), int(need.value))
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=t.device)
        _workspaces[key] = ws
    return ws


def _check_native(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the HIP convolution runs only on a HIP device (there is no CPU library path)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")


def _geometry(op: int, x: torch.Tensor, w: torch.Tensor):
    """(B, Cin, Cout, H, W) of the forward, H, W = input size; checks that x and w belong together."""
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(f"expected 4D input and weight (got {x.dim()}D, {w.dim()}D)")
    B, cin, H, W = (int(s) for s in x.shape)
    if op == OP_DECONV2X2:
        wcin, cout, k = int(w.shape[0]), int(w.shape[1]), 2
    else:
        cout, wcin, k = int(w.shape[0]), int(w.shape[1]), 3 if op == OP_CONV3X3 else 1
    if wcin != cin or tuple(w.shape[2:]) != (k, k):
        raise ValueError(f"weight {tuple(w.shape)} does not fit input {tuple(x.shape)}")
    return B, cin, cout, H, W


def _call(op, which, a, b, out, dims, prec, channels, scale=None):
    B, cin, cout, H, W = dims
    with torch.cuda.device(a.device):
        if scale is not None:      # dd_convx_*_scaled: the extended contract (a superset) and its workspace, whichever contract the module has
            ws = workspace_for(a, op, B, cin, cout, H, W, prec, "any")
            name = _ENTRY_SCALED[which]
            _ck(getattr(_lib_scaled(), name)(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), scale.data_ptr(), B, cin, cout, H, W,
                                             prec, _stream(a)), name)
            return out
        ws = workspace_for(a, op, B, cin, cout, H, W, prec, channels)
        args = (a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), B, cin, cout, H, W, prec, _stream(a))
        if _any(channels):
            name = _ENTRY_ANY[which]
            _ck(getattr(_lib(), name)(op, *args), name)
        else:
            name = _ENTRY[op][which]
            _ck(getattr(_lib(), name)(*args), name)
    return out


# ---- the three directions, one function each (what the tests and tools drive; the autograd Function below is built from them) -----------------
def conv_forward(op: int, x: torch.Tensor, w: torch.Tensor, prec: int, channels="block64") -> torch.Tensor:
    _any(channels)      # (a wrong value is an error before anything else)
    _check_native(x, "x")
    _check_native(w, "weight")
    dims = _geometry(op, x, w)
    B, _, cout, H, W = dims
    s = 2 if op == OP_DECONV2X2 else 1
    return _call(op, 0, x, w, torch.empty((B, cout, s * H, s * W), dtype=torch.float32, device=x.device), dims, prec, channels)


def _check_scale(scale, like: torch.Tensor):
    if scale is not None and not (scale.is_cuda and scale.device == like.device and scale.dtype == torch.float32 and scale.is_contiguous()
                                  and scale.numel() >= 4):
        raise RuntimeError("scale must be the 4-float device tensor grad_scale returns, on grad_y's device")


def grad_scale(grad_y: torch.Tensor, prec: int) -> torch.Tensor:
    """dd_conv_grad_scale: a fresh 4-float device tensor {s, 1 / s, bits of amax, 0} with s = 2^(14 - floor(log2 amax)) for the largest finite
    |grad_y| (include/ddepth_conv_scaled.h; "bf16": {1, 1}, no pass over grad_y).  From the caching allocator; nothing synchronises the host.
    Compute it once per backward and pass it to both ``conv_backward_data`` and ``conv_backward_weight``."""
    _check_native(grad_y, "grad_y")
    scale = torch.empty(4, dtype=torch.float32, device=grad_y.device)
    with torch.cuda.device(grad_y.device):
        _ck(_lib_scaled().dd_conv_grad_scale(grad_y.data_ptr(), grad_y.numel(), int(prec), scale.data_ptr(), _stream(grad_y)), "dd_conv_grad_scale")
    return scale


def conv_backward_data(op: int, grad_y: torch.Tensor, w: torch.Tensor, x_shape, prec: int, channels="block64", *, scale=None) -> torch.Tensor:
    """``scale`` (a ``grad_scale`` tensor; None: none): run dd_convx_backward_data_scaled, whichever ``channels`` says."""
    _any(channels)      # (a wrong value is an error before anything else)
    _check_native(grad_y, "grad_y")
    _check_native(w, "weight")
    _check_scale(scale, grad_y)
    grad_x = torch.empty(tuple(x_shape), dtype=torch.float32, device=grad_y.device)
    return _call(op, 1, grad_y, w, grad_x, _geometry(op, grad_x, w), prec, channels, scale)


def conv_backward_weight(op: int, x: torch.Tensor, grad_y: torch.Tensor, w_shape, prec: int, channels="block64", *, scale=None) -> torch.Tensor:
    """``scale``: as in ``conv_backward_data`` (dd_convx_backward_weight_scaled)."""
    _any(channels)      # (a wrong value is an error before anything else)
    _check_native(x, "x")
    _check_native(grad_y, "grad_y")
    _check_scale(scale, grad_y)
    grad_w = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    return _call(op, 2, x, grad_y, grad_w, _geometry(op, x, grad_w), prec, channels, scale)


def _forward(ctx, op, x, weight, prec, channels, grad_autoscale=False):
    ctx.save_for_backward(x, weight)
    ctx.conf = (int(op), int(prec), channels)
    ctx.grad_autoscale = bool(grad_autoscale)
    # (positional, and the default contract with exactly the arguments it always had: callers wrap these three functions)
    extra = (channels,) if _any(channels) else ()
    return conv_forward(op, x, weight.detach(), int(prec), *extra)


def _backward(ctx, grad_y):
    x, weight = ctx.saved_tensors
    op, prec, channels = ctx.conf
    extra = (channels,) if _any(channels) else ()
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_x or need_w):
        return None, None, None, None, None
    gy = grad_y.detach()
    if gy.dtype != torch.float32 or not gy.is_contiguous():
        gy = gy.float().contiguous()
    # (without the rescale: exactly the calls there always were)
    scaled = {"scale": grad_scale(gy, prec)} if ctx.grad_autoscale else {}      # once: grad_y is reduced once for both directions
    gx = conv_backward_data(op, gy, weight.detach(), x.shape, prec, *extra, **scaled) if need_x else None      # not for a detached input
    gw = conv_backward_weight(op, x, gy, weight.shape, prec, *extra, **scaled) if need_w else None             # not for a frozen weight
    return gx, gw, None, None, None


class Conv3x3Function(Function):
    """(x, weight, dd_precision[, channels]) -> F.conv2d(x, weight, None, 1, 1) over the three dd_conv3x3_* calls (``channels="any"``: over
    dd_convx_*; the choice travels in ``ctx.conf``).  Kept for the backward: x and weight.  A gradient ``ctx.needs_input_grad`` does not ask for
    is not computed.  ``grad_autoscale``: the backward rescales grad_y by a power of two (module docstring).  Nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, weight, prec, channels="block64", grad_autoscale=False):
        return _forward(ctx, OP_CONV3X3, x, weight, prec, channels, grad_autoscale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class Conv1x1Function(Function):
    """(x, weight, dd_precision) -> F.conv2d(x, weight) with a [Cout, Cin, 1, 1] weight over the three dd_conv1x1_* calls; as Conv3x3Function."""

    @staticmethod
    def forward(ctx, x, weight, prec, channels="block64", grad_autoscale=False):
        return _forward(ctx, OP_CONV1X1, x, weight, prec, channels, grad_autoscale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class ConvTranspose2x2Function(Function):
    """(x, weight, dd_precision) -> F.conv_transpose2d(x, weight, None, 2) over the three dd_deconv2x2_* calls; as Conv3x3Function."""

    @staticmethod
    def forward(ctx, x, weight, prec, channels="block64", grad_autoscale=False):
        return _forward(ctx, OP_DECONV2X2, x, weight, prec, channels, grad_autoscale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


# ---- 3x3 stride 2 pad 1, with or without a bias (include/ddepth_conv_strided.h): the opening convolutions of a ResNet stage ------------------------
def supported_s2(cin: int, cout: int, precision, channels="any") -> bool:
    """dd_conv3x3s2_supported (Cout a multiple of 8 in 8..2048, Cin 3 or such a multiple); ``channels="block64"`` narrows it to the block-64
    shapes.  No device needed, no side effects."""
    p = precision_id(precision)
    if p is None or not bool(_lib_strided().dd_conv3x3s2_supported(int(cin), int(cout), p)):
        return False
    return _any(channels) or all(c % 64 == 0 and 64 <= c <= 1536 for c in (int(cin), int(cout)))


def strided_out(n: int) -> int:
    """Output rows (columns) of k3 s2 p1 on n input rows (columns)."""
    return (int(n) - 1) // 2 + 1


def _s2_geometry(x: torch.Tensor, w: torch.Tensor):
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(f"expected 4D input and weight (got {x.dim()}D, {w.dim()}D)")
    B, cin, H, W = (int(s) for s in x.shape)
    if int(w.shape[1]) != cin or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"weight {tuple(w.shape)} does not fit input {tuple(x.shape)}")
    return B, cin, int(w.shape[0]), H, W


def _s2_workspace(t, dims, prec):
    need = ctypes.c_int64(0)
    _ck(_lib_strided().dd_conv3x3s2_workspace_bytes(*dims, prec, ctypes.byref(need)), "dd_conv3x3s2_workspace_bytes")
    key = (t.device.index if t.device.index is not None else torch.cuda.current_device(), int(need.value))
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=t.device)
        _workspaces[key] = ws
    return ws


def _check_vector(t, name, n, like):
    if t is not None:
        _check_native(t, name)
        if t.dim() != 1 or t.numel() != n or t.device != like.device:
            raise ValueError(f"{name} must have {n} elements on {like.device} (got {tuple(t.shape)} on {t.device})")


def conv_s2_forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], prec: int) -> torch.Tensor:
    """F.conv2d(x, w, bias, 2, 1) through dd_conv3x3s2_forward; ``bias`` may be None."""
    _check_native(x, "x")
    _check_native(w, "weight")
    dims = _s2_geometry(x, w)
    B, _, cout, H, W = dims
    _check_vector(bias, "bias", cout, x)
    y = torch.empty((B, cout, strided_out(H), strided_out(W)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = _s2_workspace(x, dims, int(prec))
        _ck(_lib_strided().dd_conv3x3s2_forward(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                                ws.data_ptr(), *dims, int(prec), _stream(x)), "dd_conv3x3s2_forward")
    return y


def conv_s2_backward_data(grad_y: torch.Tensor, w: torch.Tensor, x_shape, prec: int, *, scale=None) -> torch.Tensor:
    """The data gradient; ``scale``: a ``grad_scale`` tensor or None, as in ``conv_backward_data``."""
    _check_native(grad_y, "grad_y")
    _check_native(w, "weight")
    _check_scale(scale, grad_y)
    grad_x = torch.empty(tuple(x_shape), dtype=torch.float32, device=grad_y.device)
    dims = _s2_geometry(grad_x, w)
    if tuple(grad_y.shape) != (dims[0], dims[2], strided_out(dims[3]), strided_out(dims[4])):
        raise ValueError(f"grad_y {tuple(grad_y.shape)} does not fit input {tuple(x_shape)} and weight {tuple(w.shape)}")
    with torch.cuda.device(grad_y.device):
        ws = _s2_workspace(grad_y, dims, int(prec))
        _ck(_lib_strided().dd_conv3x3s2_backward_data(grad_y.data_ptr(), w.data_ptr(), grad_x.data_ptr(), ws.data_ptr(),
                                                      scale.data_ptr() if scale is not None else None, *dims, int(prec), _stream(grad_y)),
            "dd_conv3x3s2_backward_data")
    return grad_x


def conv_s2_backward_weight(x: torch.Tensor, grad_y: torch.Tensor, w_shape, prec: int, *, with_bias: bool = False, scale=None):
    """(grad_w, grad_bias) from ONE call; grad_bias is None unless ``with_bias``."""
    _check_native(x, "x")
    _check_native(grad_y, "grad_y")
    _check_scale(scale, grad_y)
    grad_w = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    dims = _s2_geometry(x, grad_w)
    if tuple(grad_y.shape) != (dims[0], dims[2], strided_out(dims[3]), strided_out(dims[4])):
        raise ValueError(f"grad_y {tuple(grad_y.shape)} does not fit input {tuple(x.shape)} and weight {tuple(w_shape)}")
    grad_b = torch.empty(dims[2], dtype=torch.float32, device=x.device) if with_bias else None
    with torch.cuda.device(x.device):
        ws = _s2_workspace(x, dims, int(prec))
        _ck(_lib_strided().dd_conv3x3s2_backward_weight(x.data_ptr(), grad_y.data_ptr(), grad_w.data_ptr(),
                                                        grad_b.data_ptr() if grad_b is not None else None, ws.data_ptr(),
                                                        scale.data_ptr() if scale is not None else None, *dims, int(prec), _stream(x)),
            "dd_conv3x3s2_backward_weight")
    return grad_w, grad_b


class Conv3x3S2Function(Function):
    """(x, weight, bias or None, dd_precision[, grad_autoscale]) -> F.conv2d(x, weight, bias, 2, 1) over the three dd_conv3x3s2_* calls.  Kept for
    the backward: x and weight only.  A gradient ``ctx.needs_input_grad`` does not ask for is not computed (the RGB image needs no data
    gradient); the bias gradient comes from the same call as the weight gradient.  Nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, weight, bias, prec, grad_autoscale=False):
        ctx.save_for_backward(x, weight)
        ctx.prec = int(prec)
        ctx.grad_autoscale = bool(grad_autoscale)
        return conv_s2_forward(x, weight.detach(), bias.detach() if bias is not None else None, int(prec))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None, None
        gy = grad_y.detach()
        if gy.dtype != torch.float32 or not gy.is_contiguous():
            gy = gy.float().contiguous()
        scaled = {"scale": grad_scale(gy, ctx.prec)} if ctx.grad_autoscale else {}      # once per backward
        gx = conv_s2_backward_data(gy, weight.detach(), x.shape, ctx.prec, **scaled) if need_x else None
        gw = gb = None
        if need_w or need_b:      # (one call serves both; a frozen weight with a live bias still runs it)
            gw, gb = conv_s2_backward_weight(x, gy, weight.shape, ctx.prec, with_bias=need_b, **scaled)
        return gx, gw if need_w else None, gb, None, None


def _tensors_native(x: torch.Tensor, w: torch.Tensor) -> bool:
    return bool(x.is_cuda and w.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_contiguous()
                and w.is_contiguous() and x.numel() > 0)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _plain(m) -> bool:
    """No bias, groups 1, dilation 1, zero padding mode: what both operators of the library assume."""
    return m.bias is None and m.groups == 1 and _pair(m.dilation) == (1, 1) and getattr(m, "padding_mode", "zeros") == "zeros"


def _is_conv3x3(m) -> bool:
    return (isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d) and _plain(m) and _pair(m.kernel_size) == (3, 3)
            and _pair(m.stride) == (1, 1) and m.padding != "same" and _pair(m.padding) == (1, 1))


def _is_conv3x3s2(m) -> bool:
    """3x3, stride 2, pad 1, dilation 1, groups 1, zero padding; a bias is allowed."""
    return (isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d) and m.groups == 1 and _pair(m.dilation) == (1, 1)
            and getattr(m, "padding_mode", "zeros") == "zeros" and _pair(m.kernel_size) == (3, 3) and _pair(m.stride) == (2, 2)
            and m.padding != "same" and _pair(m.padding) == (1, 1))


def _is_conv1x1(m) -> bool:
    return (isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d) and _plain(m) and _pair(m.kernel_size) == (1, 1)
            and _pair(m.stride) == (1, 1) and m.padding != "same" and _pair(m.padding) == (0, 0))


def _is_deconv2x2(m) -> bool:
    return (isinstance(m, nn.ConvTranspose2d) and _plain(m) and _pair(m.kernel_size) == (2, 2) and _pair(m.stride) == (2, 2)
            and _pair(m.padding) == (0, 0) and _pair(m.output_padding) == (0, 0))


def _channels_repr(channels) -> str:
    return "" if channels == "block64" else f", channels={channels}"


def _autoscale_repr(on) -> str:
    return ", grad_autoscale=True" if on else ""


def _apply(fn, x, weight, prec, channels, grad_autoscale):
    # (off: the call with exactly the arguments it always had)
    return fn.apply(x, weight, prec, channels, True) if grad_autoscale else fn.apply(x, weight, prec, channels)


class HipConv2d(nn.Conv2d):
    """``nn.Conv2d(cin, cout, 3, 1, 1, bias=False)`` or ``nn.Conv2d(cin, cout, 1, bias=False)`` (same parameter, same state-dict key) whose
    forward and backward on a HIP device run in csrc/dd_conv.hip on ``precision`` operands ("bf16", "f16", "f16x3"); the operator (3x3 or
    pointwise) follows from the module's own geometry.  Every other geometry or precision and every tensor the library does not take (module
    docstring) runs the inherited torch forward."""

    channels = "block64"      # the channel contract (CHANNELS); a class attribute, so modules made before it existed behave as they did
    grad_autoscale = False    # rescale grad_y by a power of two in the "f16" / "f16x3" backward (module docstring); likewise a class attribute
    strided = False           # True: a 3x3 stride-2 pad-1 geometry, with or without a bias, runs dd_conv3x3s2_* (convert_hip_conv(..., strided=True))

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False, precision="fp32", **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias=bias, **kwargs)
        self.precision = precision

    def extra_repr(self):
        return (super().extra_repr() + f", precision={self.precision}" + _channels_repr(self.channels) + _autoscale_repr(self.grad_autoscale)
                + (", strided=True" if self.strided else ""))

    def _native_s2(self, x) -> bool:
        """Whether this call runs the stride-2 operator of the library."""
        if not (self.strided and _is_conv3x3s2(self) and _tensors_native(x, self.weight) and x.shape[1] == self.in_channels):
            return False
        b = self.bias
        if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()):
            return False
        return supported_s2(self.in_channels, self.out_channels, self.precision, self.channels)

    def _native(self, x) -> Optional[int]:
        """The dd_conv_op this call runs in the library, or None for the torch forward."""
        op = OP_CONV3X3 if _is_conv3x3(self) else OP_CONV1X1 if _is_conv1x1(self) else None
        if op is None or not (_tensors_native(x, self.weight) and x.shape[1] == self.in_channels
                              and supported(op, self.in_channels, self.out_channels, self.precision, self.channels)):
            return None
        return op

    def forward(self, x):
        if self.strided and self._native_s2(x):
            return Conv3x3S2Function.apply(x, self.weight, self.bias, precision_id(self.precision), self.grad_autoscale)
        op = self._native(x)
        if op is None:
            return super().forward(x)
        return _apply(Conv3x3Function if op == OP_CONV3X3 else Conv1x1Function, x, self.weight, precision_id(self.precision), self.channels,
                      self.grad_autoscale)


class HipConvTranspose2d(nn.ConvTranspose2d):
    """``nn.ConvTranspose2d(cin, cout, 2, 2, bias=False)``; as HipConv2d."""

    channels = "block64"
    grad_autoscale = False

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2, padding=0, output_padding=0, bias=False, precision="fp32", **kwargs):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, output_padding, bias=bias, **kwargs)
        self.precision = precision

    def extra_repr(self):
        return super().extra_repr() + f", precision={self.precision}" + _channels_repr(self.channels) + _autoscale_repr(self.grad_autoscale)

    def _native(self, x, output_size) -> bool:
        return bool(output_size is None and _is_deconv2x2(self) and _tensors_native(x, self.weight) and x.shape[1] == self.in_channels
                    and supported(OP_DECONV2X2, self.in_channels, self.out_channels, self.precision, self.channels))

    def forward(self, x, output_size=None):
        if not self._native(x, output_size):
            return super().forward(x, output_size)
        return _apply(ConvTranspose2x2Function, x, self.weight, precision_id(self.precision), self.channels, self.grad_autoscale)


# ---- the folded eval-mode forward (include/ddepth_conv_fused.h): convolution + BatchNorm + residual + ReLU in one kernel -------------------------------
def supported_affine(stride: int, cin: int, cout: int, precision) -> bool:
    """dd_conv3x3_affine_supported: stride 1 takes the range of dd_convx_supported(3x3), stride 2 that of dd_conv3x3s2_supported.  No device needed."""
    p = precision_id(precision)
    return p is not None and bool(_lib_fused().dd_conv3x3_affine_supported(int(stride), int(cin), int(cout), p))


def _vector_native(t, n, device) -> bool:
    return t is None or bool(t.is_cuda and t.device == device and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and t.numel() == n)


def _fold(bn, conv_bias, C: int, device) -> torch.Tensor:
    vecs = [None] * 4 if bn is None else [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    vecs = [v.detach() if v is not None else None for v in vecs + [conv_bias]]
    for name, v in zip(("weight", "bias", "running_mean", "running_var", "conv_bias"), vecs):
        if not _vector_native(v, C, torch.device(device)):
            raise RuntimeError(f"{name} must be a contiguous fp32 vector of {C} elements on {device} (got {tuple(v.shape)} {v.dtype} on {v.device})")
    if bn is not None and (vecs[2] is None or vecs[3] is None):
        raise RuntimeError("the BatchNorm has no running statistics to fold")
    scale_shift = torch.empty((2, C), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _ck(_lib_fused().dd_bn_fold(*[v.data_ptr() if v is not None else None for v in vecs[:4]], float(bn.eps) if bn is not None else 0.0,
                                    vecs[4].data_ptr() if vecs[4] is not None else None, scale_shift.data_ptr(), C, _stream(scale_shift)),
            "dd_bn_fold")
    return scale_shift


def bn_fold(bn, conv_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dd_bn_fold: the fp32 device tensor [2, C] = [scale | shift] of an eval-mode BatchNorm ``bn`` (``nn.BatchNorm2d`` or ``HipBatchNorm2d``; its
    running statistics, eps and affine parameters) behind a convolution with the bias ``conv_bias``:
    scale = weight / sqrt(running_var + eps), shift = bias + (conv_bias - running_mean) * scale, in fp64 on the device, rounded once.
    ``bn=None``: the identity scale with ``conv_bias`` as the shift.  One tiny launch; nothing is cached, nothing synchronises the host."""
    if bn is None:
        if conv_bias is None:
            raise ValueError("bn_fold needs a BatchNorm or a bias")
        return _fold(None, conv_bias, int(conv_bias.numel()), conv_bias.device)
    if bn.running_mean is None or bn.running_var is None:
        raise RuntimeError("the BatchNorm has no running statistics to fold")
    return _fold(bn, conv_bias, int(bn.num_features), bn.running_mean.device)


def conv_affine_forward(x: torch.Tensor, w: torch.Tensor, scale_shift: torch.Tensor, addend: Optional[torch.Tensor], relu: bool, prec: int,
                        stride: int = 1) -> torch.Tensor:
    """relu(F.conv2d(x, w, None, stride, 1) * scale + shift + addend) through dd_conv3x3_affine_forward; ``scale_shift`` is [2, Cout] as ``bn_fold``
    returns it, ``addend`` (the output's shape) may be None."""
    _check_native(x, "x")
    _check_native(w, "weight")
    _check_native(scale_shift, "scale_shift")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2 (got {stride!r})")
    dims = _s2_geometry(x, w)
    B, _, cout, H, W = dims
    if tuple(scale_shift.shape) != (2, cout) or scale_shift.device != x.device:
        raise ValueError(f"scale_shift must be [2, {cout}] on {x.device} (got {tuple(scale_shift.shape)} on {scale_shift.device})")
    shape = (B, cout, strided_out(H), strided_out(W)) if stride == 2 else (B, cout, H, W)
    if addend is not None:
        _check_native(addend, "addend")
        if tuple(addend.shape) != shape or addend.device != x.device:
            raise ValueError(f"addend must be {shape} on {x.device} (got {tuple(addend.shape)} on {addend.device})")
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        need = ctypes.c_int64(0)
        _ck(_lib_fused().dd_conv3x3_affine_workspace_bytes(int(stride), *dims, int(prec), ctypes.byref(need)), "dd_conv3x3_affine_workspace_bytes")
        key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), int(need.value))
        ws = _workspaces.get(key)
        if ws is None:
            ws = torch.empty(int(need.value), dtype=torch.uint8, device=x.device)
            _workspaces[key] = ws
        _ck(_lib_fused().dd_conv3x3_affine_forward(x.data_ptr(), w.data_ptr(), scale_shift.data_ptr(), addend.data_ptr() if addend is not None else None,
                                                   y.data_ptr(), ws.data_ptr(), int(stride), int(bool(relu)), *dims, int(prec), _stream(x)),
            "dd_conv3x3_affine_forward")
    return y


def conv_bn_act(conv, bn, x: torch.Tensor, addend: Optional[torch.Tensor] = None, relu: bool = True) -> Optional[torch.Tensor]:
    """relu(bn(conv(x)) + addend) of an eval-mode block in two library launches behind the weight pack, or None where the call is not native
    (the caller then takes its own path): ``conv`` must be a ``HipConv2d`` of the 3x3 pad-1 geometry, stride 1 (no bias) or 2 (a bias allowed),
    of a precision and channel counts the operator runs; ``bn`` an ``nn.BatchNorm2d`` / ``HipBatchNorm2d`` with running statistics, or None
    (identity scale, the conv's bias as the shift); every tensor a contiguous fp32 tensor on one HIP device.  Uses the RUNNING statistics and
    keeps nothing for a backward: for .eval() under no_grad.  The fold runs on every call (one tiny launch), so it is never stale."""
    if not isinstance(conv, HipConv2d):
        return None
    stride = 2 if _is_conv3x3s2(conv) else 1 if _is_conv3x3(conv) else None
    if stride is None or not (_tensors_native(x, conv.weight) and x.shape[1] == conv.in_channels):
        return None
    cout, dev = conv.out_channels, x.device
    if conv.weight.device != dev or not supported_affine(stride, conv.in_channels, cout, conv.precision):
        return None
    if not _vector_native(conv.bias, cout, dev):
        return None
    if bn is not None:
        if (not isinstance(bn, nn.modules.batchnorm._BatchNorm) or bn.training or bn.num_features != cout or bn.running_mean is None
                or bn.running_var is None):
            return None
        if not all(_vector_native(v, cout, dev) for v in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
            return None
    shape = (x.shape[0], cout) + ((strided_out(x.shape[2]), strided_out(x.shape[3])) if stride == 2 else tuple(x.shape[2:]))
    if addend is not None and not (addend.is_cuda and addend.device == dev and addend.dtype == torch.float32 and addend.is_contiguous()
                                   and tuple(addend.shape) == shape):
        return None
    scale_shift = _fold(bn, conv.bias, cout, dev)
    return conv_affine_forward(x.detach(), conv.weight.detach(), scale_shift, addend.detach() if addend is not None else None, relu,
                               precision_id(conv.precision), stride)


# ---- the statistics-emitting training forward (include/ddepth_conv_stats.h): the convolution writes the BatchNorm's sums from its epilogue ------------
def supported_stats(stride: int, cin: int, cout: int, precision) -> bool:
    """dd_conv3x3_stats_supported: the ranges of ``supported_affine``.  No device needed."""
    p = precision_id(precision)
    return p is not None and bool(_lib_stats().dd_conv3x3_stats_supported(int(stride), int(cin), int(cout), p))


def conv_stats_forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, prec: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, sums) through dd_conv3x3_stats_forward: y = F.conv2d(x, w, bias, stride, 1), the bits ``conv_forward(OP_CONV3X3, ..., "any")`` /
    ``conv_s2_forward`` give, and sums = the (2 Cout + 1) fp64 vector [sum y | sum y^2 | n] that ``batchnorm.bn_stats(y)`` would compute with a
    pass over y (equal bit for bit where the sums are exact in fp64; elsewhere within the rounding of an fp64 sum)."""
    _check_native(x, "x")
    _check_native(w, "weight")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2 (got {stride!r})")
    dims = _s2_geometry(x, w)
    B, _, cout, H, W = dims
    _check_vector(bias, "bias", cout, x)
    y = torch.empty((B, cout, strided_out(H), strided_out(W)) if stride == 2 else (B, cout, H, W), dtype=torch.float32, device=x.device)
    sums = torch.empty(2 * cout + 1, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        need = ctypes.c_int64(0)
        _ck(_lib_stats().dd_conv3x3_stats_workspace_bytes(int(stride), *dims, int(prec), ctypes.byref(need)), "dd_conv3x3_stats_workspace_bytes")
        key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), int(need.value))
        ws = _workspaces.get(key)
        if ws is None:
            ws = torch.empty(int(need.value), dtype=torch.uint8, device=x.device)
            _workspaces[key] = ws
        _ck(_lib_stats().dd_conv3x3_stats_forward(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                                  sums.data_ptr(), ws.data_ptr(), int(stride), *dims, int(prec), _stream(x)),
            "dd_conv3x3_stats_forward")
    return y, sums


class ConvStatsFunction(Function):
    """(x, weight, bias or None, dd_precision, stride, channels, grad_autoscale) -> (y, sums) of ``conv_stats_forward``; ``sums`` is not
    differentiable.  A bias is taken at stride 2 only (ValueError at stride 1).  The backward is the un-fused operator's: at stride 1 the calls of Conv3x3Function under the module's channel contract, at
    stride 2 those of Conv3x3S2Function (the bias gradient from the weight gradient's call), ``grad_autoscale`` as there.  Kept: x and weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, prec, stride, channels="any", grad_autoscale=False):
        if int(stride) == 1 and bias is not None:
            # (the C ABI adds a bias at either stride, but the stride-1 backward is Conv3x3Function's, which has no bias gradient to give)
            raise ValueError("ConvStatsFunction takes a bias at stride 2 only: the stride-1 operator of HipConv2d has none, and its backward "
                             "computes no bias gradient (conv_stats_forward runs the biased stride-1 forward)")
        ctx.save_for_backward(x, weight)
        ctx.stride = int(stride)
        ctx.prec = int(prec)                                  # (what Conv3x3S2Function.backward reads ...
        ctx.conf = (OP_CONV3X3, int(prec), channels)          # ... and what _backward reads)
        ctx.grad_autoscale = bool(grad_autoscale)
        y, sums = conv_stats_forward(x, weight.detach(), bias.detach() if bias is not None else None, int(stride), int(prec))
        ctx.mark_non_differentiable(sums)
        return y, sums

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y, _grad_sums):
        if ctx.stride == 2:
            return tuple(Conv3x3S2Function.backward(ctx, grad_y)) + (None, None)      # (gx, gw, gb, None, None)
        gx, gw = _backward(ctx, grad_y)[:2]
        return gx, gw, None, None, None, None, None


def conv_bn_train(conv, bn, x: torch.Tensor, addend: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """``bn(conv(x), addend)`` of a training conv -> BatchNorm pair with the BatchNorm's statistics taken from the convolution's epilogue (no
    dd_bn_stats pass over conv's output), or None -- with nothing touched -- where one half is not native, so that the caller runs what it ran:
    ``conv`` a ``HipConv2d`` that would run its 3x3 operator on x (stride 1, or ``strided`` stride 2 with or without a bias) at a shape and
    precision dd_conv3x3_stats_supported takes; ``bn`` a ``batchnorm.HipBatchNorm2d`` in .train() that would run its library path (tracked
    running statistics, a fixed momentum, fp32 parameters); ``addend`` None or a contiguous fp32 tensor of the output's shape on x's device that
    the BatchNorm's ``add_mode`` takes; more than one value per channel unless the statistics are exchanged.  Everything behind the statistics
    -- the SyncBN all-reduce of ``sums``, finalize and the running buffers, apply, the saved tensors, both backwards -- is what the un-fused pair
    runs."""
    from .batchnorm import HipBatchNorm2d
    if not (isinstance(conv, HipConv2d) and isinstance(bn, HipBatchNorm2d) and bn.training and bn.num_features == conv.out_channels):
        return None
    if conv.strided and conv._native_s2(x):
        stride = 2
    elif conv._native(x) == OP_CONV3X3:
        stride = 1
    else:
        return None
    # bn._native is asked about x, the convolution's INPUT: of a tensor it reads only device kind, dtype and contiguity, and the BatchNorm's own input
    # y is a fresh contiguous fp32 tensor that conv_stats_forward allocates on x's device, so the answer is y's.  (forward_sums asks again on y itself
    # and raises where it does not hold: a mismatch cannot pass silently.)
    if not (supported_stats(stride, conv.in_channels, conv.out_channels, conv.precision) and bn._native(x)):
        return None
    shape = (x.shape[0], conv.out_channels) + ((strided_out(x.shape[2]), strided_out(x.shape[3])) if stride == 2 else tuple(x.shape[2:]))
    if addend is not None and not (tuple(addend.shape) == shape and bn.add_mode in ("pre", "post") and addend.device == x.device
                                   and bn._native_addend(addend, addend)):      # (the output has the addend's shape: checked above)
        return None
    if shape[0] * shape[2] * shape[3] == 1 and not bn._exchanges():
        return None
    y, sums = ConvStatsFunction.apply(x, conv.weight, conv.bias, precision_id(conv.precision), stride, conv.channels, conv.grad_autoscale)
    return bn.forward_sums(y, sums, addend)


def eligible(m: nn.Module, precision, pointwise: bool = False, channels="block64", strided: bool = False) -> bool:
    """3x3 s1 p1 or transpose k2 s2 (with ``pointwise``: or 1x1 s1 p0), no bias, groups 1, dilation 1, and channel counts and a precision
    dd_conv_supported (``channels="any"``: dd_convx_supported) accepts.  With ``strided``: also 3x3 s2 p1, with or without a bias, that
    dd_conv3x3s2_supported accepts (``channels="block64"``: its block-64 shapes only)."""
    if isinstance(m, (HipConv2d, HipConvTranspose2d)):
        return False
    if strided and _is_conv3x3s2(m):
        return supported_s2(m.in_channels, m.out_channels, precision, channels)
    if pointwise and _is_conv1x1(m):
        return supported(OP_CONV1X1, m.in_channels, m.out_channels, precision, channels)
    if _is_conv3x3(m):
        return supported(OP_CONV3X3, m.in_channels, m.out_channels, precision, channels)
    if _is_deconv2x2(m):
        return supported(OP_DECONV2X2, m.in_channels, m.out_channels, precision, channels)
    return False


def _from_conv(m, precision, channels="block64", grad_autoscale=False):
    cls = HipConvTranspose2d if isinstance(m, nn.ConvTranspose2d) else HipConv2d
    out = cls.__new__(cls)
    nn.Module.__init__(out)
    out.__dict__.update({k: v for k, v in m.__dict__.items() if k not in ("_parameters", "_buffers", "_modules")})
    out._parameters.update(m._parameters)      # the SAME tensors: optimizers built before the conversion stay valid
    out._buffers.update(m._buffers)
    out.precision = precision
    if channels != "block64":      # (the default stays the class attribute)
        out.channels = channels
    if grad_autoscale:
        out.grad_autoscale = True
    if cls is HipConv2d and _is_conv3x3s2(m):      # (only convert_hip_conv(..., strided=True) finds such a module eligible)
        out.strided = True
    return out


def convert_hip_conv(module: nn.Module, precision, pointwise: bool = False, channels="block64", grad_autoscale: bool = False,
                     strided: bool = False) -> nn.Module:
    """Every eligible convolution of ``module`` (see ``eligible``) becomes a ``HipConv2d`` / ``HipConvTranspose2d`` holding the SAME parameter
    tensor under the same name: state-dict keys and the indices inside an ``nn.Sequential`` do not change.  With a precision the library does
    not run ("fp32", "f16r", "naive_fp32") or channel counts it does not support nothing is eligible and nothing is replaced.  A 1x1
    convolution is replaced only with ``pointwise=True`` (the HAHI neck); the default leaves every 1x1 an ``nn.Conv2d``.  ``channels="any"``
    takes every multiple of 8 in 8..2048 (MPViT's 216 / 288, Swin-L's 2048 -> 1536) and marks the new modules with it; the default keeps
    the block-64 contract, multiples of 64 in 64..1536.  ``grad_autoscale=True`` marks the new modules so that their "f16" / "f16x3" backward
    rescales the incoming gradient by a power of two (module docstring); the default leaves the backward as it is.  ``strided=True`` also takes
    the 3x3 stride-2 pad-1 convolutions, biased ones included (the openings of a ResNet stage: ``conv1`` and ``downsample`` of
    model.ResNetForMMBEV), and marks them ``strided``; the default leaves every one of them an ``nn.Conv2d``."""
    out = _from_conv(module, precision, channels, grad_autoscale) if eligible(module, precision, pointwise, channels, strided) else module
    for name, child in list(module.named_children()):
        new = convert_hip_conv(child, precision, pointwise, channels, grad_autoscale, strided)
        if new is not child:
            setattr(out, name, new)
    return out


def resolve_conv_backend(conv_backend: Optional[str] = None) -> str:
    """The head keyword ``conv_backend`` / the environment variable DDEPTH_CONV_BACKEND: "torch" (default; empty or absent), "hip" (the FPN's
    convolutions), "hip+neck" (those and, on a head that has one, the HAHI neck's, its 1x1 included) or "hip+all" (as "hip+neck", with the
    extended channel range: every FPN and neck convolution of every registered head)."""
    choice = conv_backend or os.environ.get("DDEPTH_CONV_BACKEND") or "torch"
    if choice not in ("torch", "hip", "hip+neck", "hip+all"):
        raise ValueError(f"conv_backend must be 'torch', 'hip', 'hip+neck' or 'hip+all' (got {choice!r})")
    return choice


def resolve_conv_grad_autoscale(conv_grad_autoscale: Optional[bool] = None) -> bool:
    """The head keyword ``conv_grad_autoscale`` / the environment variable DDEPTH_CONV_GRAD_AUTOSCALE ("1" is on; "0", empty or absent is off, the
    default): whether the converted convolutions rescale the incoming gradient in the "f16" / "f16x3" backward."""
    if conv_grad_autoscale is not None:
        return bool(conv_grad_autoscale)
    choice = os.environ.get("DDEPTH_CONV_GRAD_AUTOSCALE") or "0"
    if choice not in ("0", "1"):
        raise ValueError(f"DDEPTH_CONV_GRAD_AUTOSCALE must be '0' or '1' (got {choice!r})")
    return choice == "1"


def resolve_conv_bn_stats(conv_bn_stats: Optional[bool] = None) -> bool:
    """The head keyword ``conv_bn_stats`` / the environment variable DDEPTH_CONV_BN_STATS ("1" is on; "0", empty or absent is off, the default):
    whether a converted conv_lateral in front of a ``HipBatchNorm2d`` emits that BatchNorm's statistics from its epilogue (``conv_bn_train``)."""
    if conv_bn_stats is not None:
        return bool(conv_bn_stats)
    choice = os.environ.get("DDEPTH_CONV_BN_STATS") or "0"
    if choice not in ("0", "1"):
        raise ValueError(f"DDEPTH_CONV_BN_STATS must be '0' or '1' (got {choice!r})")
    return choice == "1"
