"""The latent depth codec's training convolutions and its decoder tail, forward and backward, over the C ABI of include/ddepth_codec.h.

What it is for: in .train() the four convolutions of ``modules.DeepDepthTransformWithUpsampling`` -- Conv 1 -> 16 k3 s2 p1 and Conv 16 -> 16 k3 s1
p1 (encoder, no bias), ConvTranspose2d 16 -> 16 k4 s2 p1 and Conv 16 -> 1 k3 s1 p1 (decoder, with bias) -- and their autograd run as fp32 MIOpen
kernels, and ``1 / sigmoid(z).clamp(eps) - 1`` behind the decoder as four elementwise launches.  ``HipCodecConv2d``, ``HipCodecConvTranspose2d``
and ``HipCodecTail`` run them through csrc/dd_codec.hip in fp32; only ``x`` and the weight (the tail: ``z``) are kept for the backward, and a
gradient nobody needs is not computed.

    convert_hip_codec(head.depth_transform)      # or: DDIMDepthEstimate_Res(..., codec_backend="hip") / DDEPTH_CODEC_BACKEND=hip

The library route is decided BEFORE the call and taken only when the input and the parameters are contiguous fp32 tensors on a HIP device and the
module has exactly one of the four geometries.  Everything else -- CPU tensors, other dtypes, layouts or geometries -- calls the torch forward the
module inherits.  It is never a fallback after an error, nothing is copied or converted silently, and there is no CPU library path.  The eval-mode
inference kernels of the codec (dd_encode / dd_decode) are untouched: ``DeepDepthTransformWithUpsampling._torch_path`` decides as before.
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

# every symbol include/ddepth_codec.h declares (checked by tests/test_codec_cpu.py)
ABI_SYMBOLS = ["dd_codec_last_error", "dd_codec_workspace_bytes", "dd_codec_conv_forward", "dd_codec_conv_backward_data",
               "dd_codec_conv_backward_weight", "dd_codec_tail_forward", "dd_codec_tail_backward"]

OP_ENC0, OP_ENC1, OP_DEC0, OP_DEC1 = 0, 1, 2, 3      # dd_codec_op
# op -> (Cin, Cout, kernel, stride, padding, has bias, transposed)
GEOMETRY = {OP_ENC0: (1, 16, 3, 2, 1, False, False), OP_ENC1: (16, 16, 3, 1, 1, False, False),
            OP_DEC0: (16, 16, 4, 2, 1, True, True), OP_DEC1: (16, 1, 3, 1, 1, True, False)}

_bound = None
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp, c_i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
        lib.dd_codec_last_error.restype, lib.dd_codec_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_codec_workspace_bytes.restype, lib.dd_codec_workspace_bytes.argtypes = c_int, [c_int] * 4 + [ctypes.POINTER(c_i64)]
        lib.dd_codec_conv_forward.restype, lib.dd_codec_conv_forward.argtypes = c_int, [c_int] + [c_vp] * 5 + [c_int] * 3 + [c_vp]
        lib.dd_codec_conv_backward_data.restype, lib.dd_codec_conv_backward_data.argtypes = c_int, [c_int] + [c_vp] * 4 + [c_int] * 3 + [c_vp]
        lib.dd_codec_conv_backward_weight.restype, lib.dd_codec_conv_backward_weight.argtypes = c_int, [c_int] + [c_vp] * 5 + [c_int] * 3 + [c_vp]
        lib.dd_codec_tail_forward.restype, lib.dd_codec_tail_forward.argtypes = c_int, [c_vp, c_vp, c_i64, ctypes.c_float, c_vp]
        lib.dd_codec_tail_backward.restype, lib.dd_codec_tail_backward.argtypes = c_int, [c_vp, c_vp, c_vp, c_i64, ctypes.c_float, c_vp]
        _bound = lib
    return _bound


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib().dd_codec_last_error().decode()}")


def _stream(t):
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def workspace_for(t: torch.Tensor, op: int, B: int, H: int, W: int) -> torch.Tensor:
    """The device scratch of one call (the repacked weights, or the weight gradient's partial sums), cached per (device, bytes): a shape that returns finds its buffer
    again, and the steady state allocates nothing.  Calls on one stream are ordered, so sites of equal size share a buffer.  A first call
    inside a graph capture would allocate from the capture's pool: call once eagerly before capturing."""
    need = ctypes.c_int64(0)
    _ck(_lib().dd_codec_workspace_bytes(op, B, H, W, ctypes.byref(need)), "dd_codec_workspace_bytes")
    key = (t.device.index if t.device.index is not None else torch.cuda.current_device(), int(need.value))
    ws = _workspaces.get(key)
    if ws is None:
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=t.device)
        _workspaces[key] = ws
    return ws


def _check_native(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the HIP codec runs only on a HIP device (there is no CPU library path)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")


def weight_shape(op: int):
    cin, cout, k, _, _, _, transposed = GEOMETRY[op]
    return (cin, cout, k, k) if transposed else (cout, cin, k, k)


def output_hw(op: int, H: int, W: int):
    if op == OP_ENC0:
        return (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if op == OP_DEC0:
        return 2 * H, 2 * W
    return H, W


def _dims(op: int, x_shape, w: torch.Tensor):
    """(B, H, W) of the forward's input; checks that the shapes are the op's."""
    if len(x_shape) != 4 or int(x_shape[1]) != GEOMETRY[op][0] or tuple(w.shape) != weight_shape(op):
        raise ValueError(f"input {tuple(x_shape)} / weight {tuple(w.shape)} are not those of dd_codec_op {op}")
    return int(x_shape[0]), int(x_shape[2]), int(x_shape[3])


def _check_grad_y(op: int, grad_y: torch.Tensor, B: int, H: int, W: int):
    want = (B, GEOMETRY[op][1], *output_hw(op, H, W))
    if tuple(grad_y.shape) != want:
        raise ValueError(f"grad_y {tuple(grad_y.shape)} is not the output shape {want} of dd_codec_op {op}")


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- the three directions and the tail, one function each (what the tests and tools drive; the autograd Functions below are built from them) ----
def conv_forward(op: int, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    _check_native(x, "x")
    _check_native(w, "weight")
    if bias is not None:
        _check_native(bias, "bias")
        if not GEOMETRY[op][5] or tuple(bias.shape) != (GEOMETRY[op][1],):
            raise ValueError(f"bias {tuple(bias.shape)} does not belong to dd_codec_op {op}")
    B, H, W = _dims(op, x.shape, w)
    y = torch.empty((B, GEOMETRY[op][1], *output_hw(op, H, W)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = workspace_for(x, op, B, H, W)
        _ck(_lib().dd_codec_conv_forward(op, x.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), ws.data_ptr(), B, H, W, _stream(x)),
            "dd_codec_conv_forward")
    return y


def conv_backward_data(op: int, grad_y: torch.Tensor, w: torch.Tensor, x_shape) -> torch.Tensor:
    _check_native(grad_y, "grad_y")
    _check_native(w, "weight")
    B, H, W = _dims(op, x_shape, w)
    _check_grad_y(op, grad_y, B, H, W)
    grad_x = torch.empty(tuple(x_shape), dtype=torch.float32, device=grad_y.device)
    with torch.cuda.device(grad_y.device):
        ws = workspace_for(grad_y, op, B, H, W)
        _ck(_lib().dd_codec_conv_backward_data(op, grad_y.data_ptr(), w.data_ptr(), grad_x.data_ptr(), ws.data_ptr(), B, H, W, _stream(grad_y)),
            "dd_codec_conv_backward_data")
    return grad_x


def conv_backward_weight(op: int, x: torch.Tensor, grad_y: torch.Tensor, need_bias: bool = False):
    """-> (grad_w, grad_bias or None)."""
    _check_native(x, "x")
    _check_native(grad_y, "grad_y")
    grad_w = torch.empty(weight_shape(op), dtype=torch.float32, device=x.device)
    B, H, W = _dims(op, x.shape, grad_w)
    _check_grad_y(op, grad_y, B, H, W)
    grad_b = torch.empty((GEOMETRY[op][1],), dtype=torch.float32, device=x.device) if need_bias else None
    with torch.cuda.device(x.device):
        ws = workspace_for(x, op, B, H, W)
        _ck(_lib().dd_codec_conv_backward_weight(op, x.data_ptr(), grad_y.data_ptr(), grad_w.data_ptr(), _ptr(grad_b), ws.data_ptr(), B, H, W,
                                                 _stream(x)), "dd_codec_conv_backward_weight")
    return grad_w, grad_b


def tail_forward(z: torch.Tensor, eps: float) -> torch.Tensor:
    _check_native(z, "z")
    depth = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _ck(_lib().dd_codec_tail_forward(z.data_ptr(), depth.data_ptr(), z.numel(), float(eps), _stream(z)), "dd_codec_tail_forward")
    return depth


def tail_backward(z: torch.Tensor, grad_depth: torch.Tensor, eps: float) -> torch.Tensor:
    _check_native(z, "z")
    _check_native(grad_depth, "grad_depth")
    if grad_depth.shape != z.shape:
        raise ValueError(f"grad_depth {tuple(grad_depth.shape)} does not have the shape {tuple(z.shape)} of z")
    grad_z = torch.empty_like(z)
    with torch.cuda.device(z.device):
        _ck(_lib().dd_codec_tail_backward(z.data_ptr(), grad_depth.data_ptr(), grad_z.data_ptr(), z.numel(), float(eps), _stream(z)),
            "dd_codec_tail_backward")
    return grad_z


def _plain(g: torch.Tensor) -> torch.Tensor:
    g = g.detach()
    return g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()


def _forward(ctx, op, x, weight, bias):
    ctx.save_for_backward(x, weight)
    ctx.op = int(op)
    return conv_forward(op, x, weight.detach(), bias.detach() if bias is not None else None)


def _backward(ctx, grad_y):
    x, weight = ctx.saved_tensors
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    need_b = len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2]
    if not (need_x or need_w or need_b):
        return (None,) * len(ctx.needs_input_grad)
    gy = _plain(grad_y)
    gx = conv_backward_data(ctx.op, gy, weight.detach(), x.shape) if need_x else None      # not for a detached input (ENC0 in a head)
    gw = gb = None
    if need_w or need_b:                                                                 # not for frozen parameters
        gw, gb = conv_backward_weight(ctx.op, x, gy, need_bias=need_b)
    return (gx, gw if need_w else None, gb)[:len(ctx.needs_input_grad)]


class Enc0Function(Function):
    """(x, weight) -> F.conv2d(x, weight, None, 2, 1), 1 -> 16 channels, over the three dd_codec_conv_* calls.  Kept for the backward: x and
    weight.  A gradient ``ctx.needs_input_grad`` does not ask for is not computed.  Nothing synchronises the host."""

    @staticmethod
    def forward(ctx, x, weight):
        return _forward(ctx, OP_ENC0, x, weight, None)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class Enc1Function(Function):
    """(x, weight) -> F.conv2d(x, weight, None, 1, 1), 16 -> 16 channels; as Enc0Function."""

    @staticmethod
    def forward(ctx, x, weight):
        return _forward(ctx, OP_ENC1, x, weight, None)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class Dec0Function(Function):
    """(x, weight, bias) -> F.conv_transpose2d(x, weight, bias, 2, 1) with a [16, 16, 4, 4] weight; as Enc0Function."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        return _forward(ctx, OP_DEC0, x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class Dec1Function(Function):
    """(x, weight, bias) -> F.conv2d(x, weight, bias, 1, 1), 16 -> 1 channels; as Enc0Function."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        return _forward(ctx, OP_DEC1, x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        return _backward(ctx, grad_y)


class TailFunction(Function):
    """(z, eps) -> 1 / sigmoid(z).clamp(eps) - 1 in one launch each way.  Kept for the backward: z."""

    @staticmethod
    def forward(ctx, z, eps):
        ctx.save_for_backward(z)
        ctx.eps = float(eps)
        return tail_forward(z, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_depth):
        if not ctx.needs_input_grad[0]:
            return None, None
        (z,) = ctx.saved_tensors
        return tail_backward(z, _plain(grad_depth), ctx.eps), None


_FUNCTIONS = {OP_ENC0: Enc0Function, OP_ENC1: Enc1Function, OP_DEC0: Dec0Function, OP_DEC1: Dec1Function}


def _tensor_native(t: Optional[torch.Tensor]) -> bool:
    return bool(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def codec_op(m) -> Optional[int]:
    """The dd_codec_op whose geometry the convolution module ``m`` has, else None."""
    if not isinstance(m, nn.Conv2d) and not isinstance(m, nn.ConvTranspose2d):
        return None
    if m.groups != 1 or _pair(m.dilation) != (1, 1) or getattr(m, "padding_mode", "zeros") != "zeros" or isinstance(m.padding, str):
        return None
    transposed = isinstance(m, nn.ConvTranspose2d)
    if transposed and _pair(m.output_padding) != (0, 0):
        return None
    have = (m.in_channels, m.out_channels, _pair(m.kernel_size), _pair(m.stride), _pair(m.padding), m.bias is not None, transposed)
    for op, (cin, cout, k, s, p, bias, tr) in GEOMETRY.items():
        if have == (cin, cout, (k, k), (s, s), (p, p), bias, tr):
            return op
    return None


def _module_native(m, x) -> Optional[int]:
    op = codec_op(m)
    if op is None or not (_tensor_native(x) and x.dim() == 4 and x.shape[1] == m.in_channels and _tensor_native(m.weight)):
        return None
    if m.bias is not None and not _tensor_native(m.bias):
        return None
    return op


class HipCodecConv2d(nn.Conv2d):
    """``nn.Conv2d`` (same parameters, same state-dict keys) whose forward and backward on a HIP device run in csrc/dd_codec.hip when its
    geometry is the codec's ENC0 (1 -> 16 k3 s2 p1, no bias), ENC1 (16 -> 16 k3 s1 p1, no bias) or DEC1 (16 -> 1 k3 s1 p1, bias).  Every other
    geometry and every tensor the library does not take (module docstring) runs the inherited torch forward."""

    def forward(self, x):
        op = _module_native(self, x)
        if op is None:
            return super().forward(x)
        if self.bias is None:
            return _FUNCTIONS[op].apply(x, self.weight)
        return _FUNCTIONS[op].apply(x, self.weight, self.bias)


class HipCodecConvTranspose2d(nn.ConvTranspose2d):
    """``nn.ConvTranspose2d(16, 16, 4, 2, 1)`` with bias (DEC0); as HipCodecConv2d."""

    def forward(self, x, output_size=None):
        op = _module_native(self, x) if output_size is None else None
        if op is None:
            return super().forward(x, output_size)
        return _FUNCTIONS[op].apply(x, self.weight, self.bias)


class HipCodecTail(nn.Sigmoid):
    """The ``nn.Sigmoid`` that ends the decoder.  On the library route -- ``returns_depth(z)``: a contiguous fp32 tensor on a HIP device -- its
    forward returns the DEPTH ``1 / sigmoid(z).clamp(eps) - 1`` from one fused launch (one more in the backward), and
    ``DeepDepthTransformWithUpsampling.inv_t`` skips its own ``1 / clamp - 1``; everywhere else it is the sigmoid it inherits."""

    def __init__(self, eps: float = 1e-6):
        super().__init__()
        self.eps = float(eps)

    def extra_repr(self):
        return f"eps={self.eps}"

    def returns_depth(self, z) -> bool:
        return _tensor_native(z)

    def forward(self, z):
        if not self.returns_depth(z):
            return super().forward(z)
        return TailFunction.apply(z, self.eps)


def _from_conv(m):
    cls = HipCodecConvTranspose2d if isinstance(m, nn.ConvTranspose2d) else HipCodecConv2d
    out = cls.__new__(cls)
    nn.Module.__init__(out)
    out.__dict__.update({k: v for k, v in m.__dict__.items() if k not in ("_parameters", "_buffers", "_modules")})
    out._parameters.update(m._parameters)      # the SAME tensors: optimizers built before the conversion stay valid
    out._buffers.update(m._buffers)
    return out


def _convert_convs(module: nn.Module) -> nn.Module:
    out = module
    if type(module) in (nn.Conv2d, nn.ConvTranspose2d) and codec_op(module) is not None:
        out = _from_conv(module)
    for name, child in list(module.named_children()):
        new = _convert_convs(child)
        if new is not child:
            setattr(out, name, new)
    return out


def convert_hip_codec(depth_transform: nn.Module) -> nn.Module:
    """In place, on a ``modules.DeepDepthTransformWithUpsampling``: its four convolutions become ``HipCodecConv2d`` /
    ``HipCodecConvTranspose2d`` holding the SAME parameter tensors under the same names, and the ``nn.Sigmoid`` that ends
    ``conv_inv_transform`` becomes a ``HipCodecTail`` with the module's ``eps``.  State-dict keys and the indices inside every
    ``nn.Sequential`` do not change; BatchNorm layers are not touched, so ``convert_hip_batchnorm`` may run before or after.  Idempotent.
    Returns ``depth_transform``."""
    if not (isinstance(getattr(depth_transform, "conv_transform", None), nn.Sequential)
            and isinstance(getattr(depth_transform, "conv_inv_transform", None), nn.Sequential)):
        raise TypeError("convert_hip_codec expects a DeepDepthTransformWithUpsampling (conv_transform / conv_inv_transform)")
    for name in ("conv_transform", "conv_inv_transform"):
        _convert_convs(getattr(depth_transform, name))      # (an nn.Sequential is never replaced itself)
    dec = depth_transform.conv_inv_transform
    last = list(dec._modules)[-1]
    if type(dec._modules[last]) is nn.Sigmoid:
        dec._modules[last] = HipCodecTail(getattr(depth_transform, "eps", 1e-6))
    return depth_transform


def resolve_codec_backend(codec_backend: Optional[str] = None) -> str:
    """The head keyword ``codec_backend`` / the environment variable DDEPTH_CODEC_BACKEND: "torch" (default; empty or absent) or "hip"."""
    choice = codec_backend or os.environ.get("DDEPTH_CODEC_BACKEND") or "torch"
    if choice not in ("torch", "hip"):
        raise ValueError(f"codec_backend must be 'torch' or 'hip' (got {choice!r})")
    return choice
