"""Batch-statistics BatchNorm2d with a fused activation, forward and backward, over the C ABI of include/ddepth_bn.h.

What it is for: in .train() the part of a head that runs once per image (condition FPN, latent codec, HAHI neck) normalises with batch
statistics.  As torch modules that is one MIOpen batch-norm kernel pair plus an activation pass per layer on a single rank, and on a
data-parallel rank -- where every BatchNorm is a ``dist.SyncBatchNorm`` -- a composition of about a dozen elementwise launches per layer and
direction with a saved ``xhat`` as large as the activation.  ``HipBatchNorm2d`` runs the same arithmetic through csrc/dd_bn.hip: four
streaming kernels (statistics, apply, backward reduce, backward apply), the activation fused, and only ``x`` kept for the backward.

The exchange between ranks sits between the reduce and the apply of each direction (one fp64 all-reduce each way), so one module serves
both the single-rank and the data-parallel case.

    convert_hip_batchnorm(head)            # or: DDIMDepthEstimate_Res(..., bn_backend="hip") / DDEPTH_BN_BACKEND=hip

Where a residual joins, ``HipBatchNorm2d.forward(x, addend)`` runs the add inside the apply kernel (include/ddepth_bn_add.h): ``add_mode="pre"``
is act(bn(x) + addend), the tail of a ResNet BasicBlock (model.fuse_basic_block_tails), ``"post"`` is act(bn(x)) + addend, the top-down add of the
FPN (``bn_backend="hip+add"``).  The statistics are those of x alone, so the exchange is unchanged; the "pre" backward reads its mask from the
output it kept and writes the addend's gradient in the pass that forms the sums.

The library path needs contiguous fp32 tensors on a HIP device in .train() with tracked running statistics and a fixed momentum; anything
else (eval mode, CPU tensors, other dtypes or layouts, ``momentum=None``, ``track_running_stats=False``) takes the torch path the module
inherits and applies the activation behind it.  Nothing is copied or converted silently, and there is no CPU library path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch
import torch.distributed as tdist
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import backend
from . import dist as ddist

# every symbol include/ddepth_bn.h declares (checked by tests/test_bn_cpu.py)
ABI_SYMBOLS = ["dd_bn_last_error", "dd_bn_workspace_bytes", "dd_bn_stats", "dd_bn_finalize", "dd_bn_apply", "dd_bn_backward_reduce",
               "dd_bn_backward_apply"]

# every symbol include/ddepth_bn_add.h declares (checked by tests/test_bn_add_cpu.py)
ADD_ABI_SYMBOLS = ["dd_bn_apply_add", "dd_bn_backward_reduce_add"]

ACT_NONE, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2      # dd_bn_act
ACTIVATIONS = {None: ACT_NONE, "relu": ACT_RELU, "leaky_relu": ACT_LEAKY_RELU}
ADD_PRE, ADD_POST = 0, 1                          # dd_bn_add_mode
ADD_MODES = {"pre": ADD_PRE, "post": ADD_POST}

_bound = None
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp, c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
        lib.dd_bn_last_error.restype, lib.dd_bn_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_bn_workspace_bytes.restype = c_int
        lib.dd_bn_workspace_bytes.argtypes = [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]
        lib.dd_bn_stats.restype, lib.dd_bn_stats.argtypes = c_int, [c_vp] * 3 + [c_int] * 3 + [c_vp]
        lib.dd_bn_finalize.restype, lib.dd_bn_finalize.argtypes = c_int, [c_vp, c_f, c_f, c_vp, c_vp, c_vp, c_int, c_vp]
        lib.dd_bn_apply.restype, lib.dd_bn_apply.argtypes = c_int, [c_vp] * 5 + [c_int, c_f] + [c_int] * 3 + [c_vp]
        lib.dd_bn_backward_reduce.restype = c_int
        lib.dd_bn_backward_reduce.argtypes = [c_vp] * 5 + [c_int, c_f, c_vp, c_vp] + [c_int] * 3 + [c_vp]
        lib.dd_bn_backward_apply.restype = c_int
        lib.dd_bn_backward_apply.argtypes = [c_vp] * 8 + [c_int, c_f] + [c_int] * 3 + [c_vp]
        lib.dd_bn_apply_add.restype, lib.dd_bn_apply_add.argtypes = c_int, [c_vp] * 6 + [c_int, c_f, c_int] + [c_int] * 3 + [c_vp]
        lib.dd_bn_backward_reduce_add.restype = c_int
        lib.dd_bn_backward_reduce_add.argtypes = [c_vp] * 4 + [c_int, c_f, c_vp, c_vp, c_vp] + [c_int] * 3 + [c_vp]
        _bound = lib
    return _bound


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib().dd_bn_last_error().decode()}")


def _stream(t):
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def workspace_for(t: torch.Tensor, B: int, C: int, HW: int) -> torch.Tensor:
    """The device scratch of the two reductions: one buffer per (device, stream), zeroed ONCE when it is allocated and grown when a larger
    shape arrives.  Steady state allocates nothing.  A first call inside a graph capture would allocate from the capture's pool: call once
    eagerly before capturing, as for any torch graph."""
    need = ctypes.c_int64(0)
    _ck(_lib().dd_bn_workspace_bytes(B, C, HW, ctypes.byref(need)), "dd_bn_workspace_bytes")
    key = (t.device.index if t.device.index is not None else torch.cuda.current_device(), _stream(t))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need.value:
        ws = torch.zeros(int(need.value), dtype=torch.uint8, device=t.device)
        _workspaces[key] = ws
    return ws


def _geometry(x: torch.Tensor) -> Tuple[int, int, int]:
    B, C = int(x.shape[0]), int(x.shape[1])
    return B, C, int(x.numel() // max(B * C, 1))


def _check_native(x: torch.Tensor, name: str):
    if not x.is_cuda:
        raise RuntimeError(f"{name} is on {x.device}: the HIP BatchNorm runs only on a HIP device (there is no CPU library path)")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor (got {x.dtype}, contiguous={x.is_contiguous()})")


# ---- the six calls, one function each (what the tests and tools drive; the autograd Function below is built from them) ---------------------
def bn_stats(x: torch.Tensor) -> torch.Tensor:
    """(2C + 1) fp64 [sum x | sum x^2 | n] of a contiguous fp32 (B, C, ...) HIP tensor (dd_bn_stats): the payload of the forward exchange."""
    _check_native(x, "x")
    B, C, HW = _geometry(x)
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = workspace_for(x, B, C, HW)
        _ck(_lib().dd_bn_stats(x.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, C, HW, _stream(x)), "dd_bn_stats")
    return sums


def bn_finalize(sums: torch.Tensor, eps: float, momentum: float = 0.0, running_mean: Optional[torch.Tensor] = None,
                running_var: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(2C) fp32 [mean | invstd] from sums (dd_bn_finalize); the running buffers, where given, are updated in place."""
    C = (int(sums.numel()) - 1) // 2
    mean_invstd = torch.empty(2 * C, dtype=torch.float32, device=sums.device)
    with torch.cuda.device(sums.device):
        _ck(_lib().dd_bn_finalize(sums.data_ptr(), float(eps), float(momentum), mean_invstd.data_ptr(), _ptr(running_mean), _ptr(running_var),
                                  C, _stream(sums)), "dd_bn_finalize")
    return mean_invstd


def bn_apply(x, mean_invstd, weight=None, bias=None, act: int = ACT_NONE, slope: float = 0.0) -> torch.Tensor:
    """y = act((x - mean) * invstd * weight + bias) (dd_bn_apply)."""
    _check_native(x, "x")
    B, C, HW = _geometry(x)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _ck(_lib().dd_bn_apply(x.data_ptr(), mean_invstd.data_ptr(), _ptr(weight), _ptr(bias), y.data_ptr(), int(act), float(slope), B, C, HW,
                               _stream(x)), "dd_bn_apply")
    return y


def bn_backward_reduce(x, grad_y, mean_invstd, weight=None, bias=None, act: int = ACT_NONE, slope: float = 0.0) -> torch.Tensor:
    """(2C) fp64 [sum g | sum g * xhat] (dd_bn_backward_reduce): locally the bias and weight gradients, and the payload of the backward exchange."""
    _check_native(x, "x")
    _check_native(grad_y, "grad_y")
    B, C, HW = _geometry(x)
    sums2 = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = workspace_for(x, B, C, HW)
        _ck(_lib().dd_bn_backward_reduce(x.data_ptr(), grad_y.data_ptr(), mean_invstd.data_ptr(), _ptr(weight), _ptr(bias), int(act), float(slope),
                                         sums2.data_ptr(), ws.data_ptr(), B, C, HW, _stream(x)), "dd_bn_backward_reduce")
    return sums2


def bn_backward_apply(x, grad_y, mean_invstd, sums2, sums, weight=None, bias=None, act: int = ACT_NONE, slope: float = 0.0) -> torch.Tensor:
    """grad_x = weight * invstd * (g - sum g / N - xhat * sum(g * xhat) / N) (dd_bn_backward_apply); N is read from sums on the device."""
    _check_native(x, "x")
    _check_native(grad_y, "grad_y")
    B, C, HW = _geometry(x)
    grad_x = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _ck(_lib().dd_bn_backward_apply(x.data_ptr(), grad_y.data_ptr(), mean_invstd.data_ptr(), _ptr(weight), _ptr(bias), sums2.data_ptr(),
                                        sums.data_ptr(), grad_x.data_ptr(), int(act), float(slope), B, C, HW, _stream(x)), "dd_bn_backward_apply")
    return grad_x


def bn_apply_add(x, mean_invstd, addend, weight=None, bias=None, act: int = ACT_NONE, slope: float = 0.0, add_mode: int = ADD_PRE) -> torch.Tensor:
    """y = act(z + addend) (ADD_PRE) or act(z) + addend (ADD_POST), z = (x - mean) * invstd * weight + bias (dd_bn_apply_add)."""
    _check_native(x, "x")
    _check_native(addend, "addend")
    if addend.shape != x.shape or addend.device != x.device:
        raise RuntimeError(f"addend must have x's shape and device (got {tuple(addend.shape)} on {addend.device}, x {tuple(x.shape)} on {x.device})")
    B, C, HW = _geometry(x)
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _ck(_lib().dd_bn_apply_add(x.data_ptr(), mean_invstd.data_ptr(), _ptr(weight), _ptr(bias), addend.data_ptr(), y.data_ptr(), int(act),
                                   float(slope), int(add_mode), B, C, HW, _stream(x)), "dd_bn_apply_add")
    return y


def bn_backward_reduce_add(x, grad_y, y, mean_invstd, act: int = ACT_NONE, slope: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(g, sums2) of the ADD_PRE backward in one pass (dd_bn_backward_reduce_add): g = grad_y * act'(y), masked by the forward's output -- the
    addend's gradient and the ``grad_y`` of ``bn_backward_apply(x, g, ..., act=ACT_NONE)`` -- and (2C) fp64 [sum g | sum g * xhat]."""
    for name, t in (("x", x), ("grad_y", grad_y), ("y", y)):
        _check_native(t, name)
        if t.shape != x.shape:
            raise RuntimeError(f"{name} must have x's shape (got {tuple(t.shape)}, x {tuple(x.shape)})")
    B, C, HW = _geometry(x)
    g = torch.empty_like(x)
    sums2 = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = workspace_for(x, B, C, HW)
        _ck(_lib().dd_bn_backward_reduce_add(x.data_ptr(), grad_y.data_ptr(), y.data_ptr(), mean_invstd.data_ptr(), int(act), float(slope),
                                             g.data_ptr(), sums2.data_ptr(), ws.data_ptr(), B, C, HW, _stream(x)), "dd_bn_backward_reduce_add")
    return g, sums2


def _touch(t: Optional[torch.Tensor]):
    """The library wrote through the raw pointer: tell torch (the version counter is what HipBound's staleness check reads)."""
    if t is not None:
        torch.autograd.graph.increment_version(t)


class BatchNormTrainFunction(Function):
    """(x, weight, bias) -> act(batch_norm(x)) with batch statistics, over the six calls of include/ddepth_bn.h.  ``exchange`` is None or a
    process group handle wrapped in a 1-tuple: then ``sums`` (forward) and ``sums2`` (backward) are all-reduced, one fp64 collective each way.
    Kept for the backward: x, mean_invstd (2C fp32) and sums (for N).  Nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, act, slope, exchange):
        _check_native(x, "x")
        for name, p in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if p is not None:
                _check_native(p, name)
        w = weight.detach() if weight is not None else None
        b = bias.detach() if bias is not None else None
        sums = bn_stats(x)
        if exchange is not None:
            tdist.all_reduce(sums, group=exchange[0])
        mean_invstd = bn_finalize(sums, eps, momentum, running_mean, running_var)
        _touch(running_mean)
        _touch(running_var)
        y = bn_apply(x, mean_invstd, w, b, act, slope)
        ctx.save_for_backward(x, mean_invstd, sums, weight, bias)
        ctx.conf = (int(act), float(slope), exchange)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, mean_invstd, sums, weight, bias = ctx.saved_tensors
        act, slope, exchange = ctx.conf
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return (None,) * 10
        gy = grad_y.detach()
        if gy.dtype != torch.float32 or not gy.is_contiguous():
            gy = gy.float().contiguous()
        sums2 = bn_backward_reduce(x, gy, mean_invstd, weight, bias, act, slope)
        C = mean_invstd.numel() // 2
        # the LOCAL sums are the parameter gradients (the gradient exchange of data-parallel training averages those), taken before the exchange
        gb = sums2[:C].to(bias.dtype) if need_b else None
        gw = sums2[C:].to(weight.dtype) if need_w else None
        gx = None
        if need_x:
            if exchange is not None:
                tdist.all_reduce(sums2, group=exchange[0])
            gx = bn_backward_apply(x, gy, mean_invstd, sums2, sums, weight, bias, act, slope)
        return gx, gw, gb, None, None, None, None, None, None, None


class BatchNormAddTrainFunction(Function):
    """(x, addend, weight, bias) -> act(batch_norm(x) + addend) (``add_mode`` ADD_PRE: a BasicBlock's tail) or act(batch_norm(x)) + addend
    (ADD_POST: the FPN's top-down add), over include/ddepth_bn.h and include/ddepth_bn_add.h.  The statistics are those of x alone, so
    ``exchange`` works as in BatchNormTrainFunction.  Kept for the backward: ADD_PRE x, the output y (its sign is the activation's mask),
    mean_invstd, sums and weight; ADD_POST what BatchNormTrainFunction keeps.  The addend is never kept.  Nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, running_mean, running_var, eps, momentum, act, slope, add_mode, exchange):
        _check_native(x, "x")
        _check_native(addend, "addend")
        for name, p in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if p is not None:
                _check_native(p, name)
        if add_mode not in (ADD_PRE, ADD_POST):
            raise ValueError(f"add_mode must be ADD_PRE or ADD_POST (got {add_mode!r})")
        if add_mode == ADD_PRE and act == ACT_LEAKY_RELU and slope < 0:
            raise RuntimeError("ADD_PRE with a LeakyReLU of negative slope: the output's sign is not the mask (HipBatchNorm2d takes the torch path)")
        w = weight.detach() if weight is not None else None
        b = bias.detach() if bias is not None else None
        sums = bn_stats(x)
        if exchange is not None:
            tdist.all_reduce(sums, group=exchange[0])
        mean_invstd = bn_finalize(sums, eps, momentum, running_mean, running_var)
        _touch(running_mean)
        _touch(running_var)
        y = bn_apply_add(x, mean_invstd, addend.detach(), w, b, act, slope, add_mode)
        if add_mode == ADD_PRE:
            ctx.save_for_backward(x, y, mean_invstd, sums, weight)
        else:
            ctx.save_for_backward(x, mean_invstd, sums, weight, bias)
        ctx.conf = (int(act), float(slope), int(add_mode), exchange)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        act, slope, add_mode, exchange = ctx.conf
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        none8 = (None,) * 8
        if not (need_x or need_r or need_w or need_b):
            return (None,) * 12
        gy = grad_y.detach()
        if gy.dtype != torch.float32 or not gy.is_contiguous():
            gy = gy.float().contiguous()
        if add_mode == ADD_PRE:
            x, y, mean_invstd, sums, weight = ctx.saved_tensors
            g, sums2 = bn_backward_reduce_add(x, gy, y, mean_invstd, act, slope)
            gr, bias, act = g, None, ACT_NONE      # the data gradient is the plain BatchNorm backward of g
        else:
            x, mean_invstd, sums, weight, bias = ctx.saved_tensors
            g, gr = gy, grad_y                     # the add sits behind the activation: its gradient is grad_y itself
            if not (need_x or need_w or need_b):
                return (None, gr) + (None,) * 10
            sums2 = bn_backward_reduce(x, gy, mean_invstd, weight, bias, act, slope)
        C = mean_invstd.numel() // 2
        # the LOCAL sums are the parameter gradients, taken before the exchange (as in BatchNormTrainFunction)
        gb = sums2[:C].to(torch.float32) if need_b else None
        gw = sums2[C:].to(weight.dtype) if need_w else None
        gx = None
        if need_x:
            if exchange is not None:
                tdist.all_reduce(sums2, group=exchange[0])
            gx = bn_backward_apply(x, g, mean_invstd, sums2, sums, weight, bias, act, slope)
        return (gx, gr if need_r else None, gw, gb) + none8


def _check_sums(sums: torch.Tensor, x: torch.Tensor):
    C = int(x.shape[1])
    if not (sums.is_cuda and sums.device == x.device and sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == 2 * C + 1):
        raise RuntimeError(f"sums must be the contiguous fp64 vector of {2 * C + 1} elements bn_stats returns, on x's device "
                           f"(got {tuple(sums.shape)} {sums.dtype} on {sums.device})")


class BatchNormSumsTrainFunction(Function):
    """BatchNormTrainFunction with the statistics ready: ``sums`` (last argument, not differentiable) is the (2C + 1) fp64 vector ``bn_stats(x)``
    would compute -- conv.ConvStatsFunction writes it from the convolution's epilogue -- so dd_bn_stats does not run.  Everything behind it is
    BatchNormTrainFunction's: the all-reduce of ``sums`` (in place) under ``exchange``, finalize and the running buffers, apply, the saved
    tensors, and the backward itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, act, slope, exchange, sums):
        _check_native(x, "x")
        for name, p in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if p is not None:
                _check_native(p, name)
        sums = sums.detach()
        _check_sums(sums, x)
        w = weight.detach() if weight is not None else None
        b = bias.detach() if bias is not None else None
        if exchange is not None:
            tdist.all_reduce(sums, group=exchange[0])
        mean_invstd = bn_finalize(sums, eps, momentum, running_mean, running_var)
        _touch(running_mean)
        _touch(running_var)
        y = bn_apply(x, mean_invstd, w, b, act, slope)
        ctx.save_for_backward(x, mean_invstd, sums, weight, bias)
        ctx.conf = (int(act), float(slope), exchange)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return tuple(BatchNormTrainFunction.backward(ctx, grad_y)) + (None,)      # (the same saved tensors, the same first three inputs)


class BatchNormAddSumsTrainFunction(Function):
    """BatchNormAddTrainFunction with the statistics ready in ``sums`` (last argument), as BatchNormSumsTrainFunction: the statistics are those
    of x alone in either ``add_mode``, so the convolution that wrote x can supply them."""

    @staticmethod
    def forward(ctx, x, addend, weight, bias, running_mean, running_var, eps, momentum, act, slope, add_mode, exchange, sums):
        _check_native(x, "x")
        _check_native(addend, "addend")
        for name, p in (("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var)):
            if p is not None:
                _check_native(p, name)
        if add_mode not in (ADD_PRE, ADD_POST):
            raise ValueError(f"add_mode must be ADD_PRE or ADD_POST (got {add_mode!r})")
        if add_mode == ADD_PRE and act == ACT_LEAKY_RELU and slope < 0:
            raise RuntimeError("ADD_PRE with a LeakyReLU of negative slope: the output's sign is not the mask (HipBatchNorm2d takes the torch path)")
        sums = sums.detach()
        _check_sums(sums, x)
        w = weight.detach() if weight is not None else None
        b = bias.detach() if bias is not None else None
        if exchange is not None:
            tdist.all_reduce(sums, group=exchange[0])
        mean_invstd = bn_finalize(sums, eps, momentum, running_mean, running_var)
        _touch(running_mean)
        _touch(running_var)
        y = bn_apply_add(x, mean_invstd, addend.detach(), w, b, act, slope, add_mode)
        if add_mode == ADD_PRE:
            ctx.save_for_backward(x, y, mean_invstd, sums, weight)
        else:
            ctx.save_for_backward(x, mean_invstd, sums, weight, bias)
        ctx.conf = (int(act), float(slope), int(add_mode), exchange)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return tuple(BatchNormAddTrainFunction.backward(ctx, grad_y)) + (None,)      # (the same saved tensors, the same first four inputs)


class HipBatchNorm2d(ddist.SyncBatchNorm):
    """``nn.BatchNorm2d`` (same parameters, buffers and state-dict keys) whose .train() forward and backward on a HIP device run in
    csrc/dd_bn.hip, with ``activation`` (None, "relu" or "leaky_relu" with ``negative_slope``) fused behind it.

    A subclass of ``dist.SyncBatchNorm``: ``dist.convert_sync_batchnorm`` leaves it alone, and it exchanges statistics under the same
    rule -- .train(), an initialised process group, and more than one rank (or ``force_sync``).  When it exchanges, the fp64 sums travel:
    one all-reduce in the forward, one in the backward."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, process_group=None, activation=None,
                 negative_slope=0.01):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, process_group)
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {list(ACTIVATIONS)} (got {activation!r})")
        self.activation = activation
        self.negative_slope = float(negative_slope)
        self.add_mode = "pre"      # where forward(x, addend) adds: "pre" act(bn(x) + addend), "post" act(bn(x)) + addend

    def extra_repr(self):
        s = super().extra_repr()
        if self.activation is not None:
            s += f", activation={self.activation}" + (f"({self.negative_slope})" if self.activation == "leaky_relu" else "")
        return s

    def _check_input_dim(self, input):
        if input.dim() != 4:
            raise ValueError(f"expected 4D input (got {input.dim()}D input)")

    def _activate(self, y):
        if self.activation == "relu":
            return F.relu(y)
        if self.activation == "leaky_relu":
            return F.leaky_relu(y, self.negative_slope)
        return y

    def _native(self, x) -> bool:
        return bool(self.training and self.track_running_stats and self.momentum is not None and x.is_cuda and x.dtype == torch.float32
                    and x.is_contiguous() and (self.weight is None or self.weight.dtype == torch.float32))

    def _native_addend(self, x, addend) -> bool:
        """The library's apply takes this addend: a contiguous fp32 tensor of x's shape on x's device, and in "pre" mode an activation whose
        output carries its own mask (any but a LeakyReLU of negative slope)."""
        return bool(addend.is_cuda and addend.device == x.device and addend.dtype == torch.float32 and addend.is_contiguous()
                    and addend.shape == x.shape
                    and not (self.add_mode == "pre" and self.activation == "leaky_relu" and self.negative_slope < 0))

    def forward(self, x, addend=None):
        self._check_input_dim(x)
        if addend is not None and self.add_mode not in ADD_MODES:
            raise ValueError(f"add_mode must be one of {list(ADD_MODES)} (got {self.add_mode!r})")
        if not self._native(x) or (addend is not None and not self._native_addend(x, addend)):
            if addend is None:
                return self._activate(super().forward(x))
            z = super().forward(x)
            return self._activate(z) + addend if self.add_mode == "post" else self._activate(z + addend)
        exchange = (self.process_group,) if self._exchanges() else None
        if exchange is None and x.numel() // x.shape[1] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
        if self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        if addend is not None:
            return BatchNormAddTrainFunction.apply(x, addend, self.weight, self.bias, self.running_mean, self.running_var, self.eps,
                                                   self.momentum, ACTIVATIONS[self.activation], self.negative_slope, ADD_MODES[self.add_mode],
                                                   exchange)
        return BatchNormTrainFunction.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, self.momentum,
                                            ACTIVATIONS[self.activation], self.negative_slope, exchange)


    def forward_sums(self, x, sums, addend=None):
        """``forward(x, addend)`` on the library path with the statistics of x ready: ``sums`` is the (2C + 1) fp64 vector ``bn_stats(x)`` would
        compute, written by whoever wrote x (conv.conv_bn_train: the convolution's epilogue), so no dd_bn_stats runs.  The caller has checked
        what ``forward`` checks before it takes the library path (``_native``, ``_native_addend``); a tensor that is not native is an error
        here, never a silent torch path, because ``sums`` would be dropped."""
        self._check_input_dim(x)
        if addend is not None and self.add_mode not in ADD_MODES:
            raise ValueError(f"add_mode must be one of {list(ADD_MODES)} (got {self.add_mode!r})")
        if not self._native(x) or (addend is not None and not self._native_addend(x, addend)):
            raise RuntimeError("forward_sums needs what the library path needs: .train(), tracked running statistics, a fixed momentum and "
                               "contiguous fp32 HIP tensors (an addend of x's shape)")
        exchange = (self.process_group,) if self._exchanges() else None
        if exchange is None and x.numel() // x.shape[1] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
        if self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        if addend is not None:
            return BatchNormAddSumsTrainFunction.apply(x, addend, self.weight, self.bias, self.running_mean, self.running_var, self.eps,
                                                       self.momentum, ACTIVATIONS[self.activation], self.negative_slope,
                                                       ADD_MODES[self.add_mode], exchange, sums)
        return BatchNormSumsTrainFunction.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, self.momentum,
                                                ACTIVATIONS[self.activation], self.negative_slope, exchange, sums)


def _from_batchnorm(m: nn.modules.batchnorm._BatchNorm, process_group) -> HipBatchNorm2d:
    group = process_group if process_group is not None else getattr(m, "process_group", None)
    out = HipBatchNorm2d(m.num_features, m.eps, m.momentum, m.affine, m.track_running_stats, group)
    if m.affine:
        out.weight, out.bias = m.weight, m.bias
    out.running_mean, out.running_var, out.num_batches_tracked = m.running_mean, m.running_var, m.num_batches_tracked
    out.training = m.training
    return out


def convert_hip_batchnorm(module: nn.Module, process_group=None, fuse_activation: bool = True) -> nn.Module:
    """Every ``nn.BatchNorm2d`` and ``dist.SyncBatchNorm`` of ``module`` becomes a ``HipBatchNorm2d`` holding the SAME parameter and buffer
    tensors (optimizers built before the conversion stay valid; state-dict keys unchanged).  With ``fuse_activation``, where the next
    sibling inside an ``nn.Sequential`` is an ``nn.ReLU`` or ``nn.LeakyReLU``, the BatchNorm takes that activation over and an
    ``nn.Identity`` takes its place: indices, and with them the keys of everything behind, do not move."""
    out = module
    if isinstance(module, (nn.BatchNorm2d, ddist.SyncBatchNorm)) and not isinstance(module, HipBatchNorm2d):
        out = _from_batchnorm(module, process_group)
    for name, child in list(module.named_children()):
        new = convert_hip_batchnorm(child, process_group, fuse_activation)
        if new is not child:
            setattr(out, name, new)
    if fuse_activation and isinstance(out, nn.Sequential):
        kids = list(out._modules.items())
        for (_, bn), (key, nxt) in zip(kids, kids[1:]):
            if not (isinstance(bn, HipBatchNorm2d) and bn.activation is None):
                continue
            if type(nxt) is nn.ReLU:
                bn.activation = "relu"
            elif type(nxt) is nn.LeakyReLU:
                bn.activation, bn.negative_slope = "leaky_relu", float(nxt.negative_slope)
            else:
                continue
            out._modules[key] = nn.Identity()
    return out


def resolve_bn_backend(bn_backend: Optional[str] = None) -> str:
    """The head keyword ``bn_backend`` / the environment variable DDEPTH_BN_BACKEND: "torch" (default; empty or absent), "hip", or "hip+add"
    ("hip", and the FPN's top-down add runs inside the lateral BatchNorm's apply)."""
    import os
    choice = bn_backend or os.environ.get("DDEPTH_BN_BACKEND") or "torch"
    if choice not in ("torch", "hip", "hip+add"):
        raise ValueError(f"bn_backend must be 'torch', 'hip' or 'hip+add' (got {choice!r})")
    return choice
