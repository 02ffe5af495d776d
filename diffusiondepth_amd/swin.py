"""The Swin backbone's shifted-window attention over the C ABIs of include/ddepth_swin.h (forward) and include/train/ddepth_swin_backward.h
(backward): window 7, head dimension 32.

What it is for: the reference's ``ShiftWindowMSA`` (src/model/backbone/swin.py) runs pad -> roll -> mask build -> window partition -> ``qkv`` ->
reshape / permute -> scale -> QK^T -> + relative-position bias -> + mask -> softmax -> .V -> transpose / reshape -> ``proj`` -> window reverse ->
roll -> crop: about a dozen full-tensor passes, six of them copies.  ``HipShiftWindowMSA`` runs the ``qkv`` Linear on the tokens as they are, ONE
library call that does the rest in its addressing (csrc/dd_swin.hip), and the ``proj`` Linear.

    convert_hip_window_attention(backbone, precision="fp32")    # or: args.backbone_attention = "hip" / DDEPTH_BACKBONE_ATTENTION=hip

The library route is decided BEFORE the call and taken only without autograd, for contiguous fp32 tensors on a HIP device, window 7,
``embed_dims == 32 * num_heads`` and no active dropout.  Everything else -- training, a tensor that needs a gradient, CPU tensors, other windows --
runs the reference's sequence in torch (``window_attention_torch``, differentiable).  It is never a fallback after an error.

Training, opt-in: ``backward="hip"`` (``convert_hip_window_attention(backbone, precision, backward="hip")``, ``args.backbone_attention =
"hip+train"``) sends the differentiable case through ``WindowAttentionFunction``: the same forward call, and ONE backward call that recomputes
the probabilities (csrc/dd_swin_bwd.hip) -- nothing of size [windows, heads, 49, 49] is saved.  The bias table's gradient is a fixed gather of
the dense one (``fold_bias_grad``), so the whole route is bitwise reproducible.  The default ``backward="torch"`` changes nothing.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import backend
from . import linear as _linear

# every symbol include/ddepth_swin.h declares (checked by tests/test_swin_cpu.py)
ABI_SYMBOLS = ["dd_swin_last_error", "dd_window_attention_supported", "dd_window_attention_forward"]
PRECISIONS = {"fp32": 1, "bf16": 2, "f16": 3}      # dd_precision
WINDOW, HEAD_DIM = 7, 32
# every symbol include/train/ddepth_swin_backward.h declares (checked by tests/test_swin_backward_cpu.py)
BACKWARD_ABI_SYMBOLS = ["dd_window_attention_backward_supported", "dd_window_attention_backward_workspace_bytes", "dd_window_attention_backward"]
ATTENTION_BACKENDS = ("torch", "hip", "hip+train")
BACKWARDS = ("torch", "hip")

_bound = None


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_swin_last_error.restype, lib.dd_swin_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_window_attention_supported.restype, lib.dd_window_attention_supported.argtypes = c_int, [c_int] * 4
        lib.dd_window_attention_forward.restype, lib.dd_window_attention_forward.argtypes = c_int, [c_vp] * 4 + [c_int] * 8 + [c_vp]
        lib.dd_window_attention_backward_supported.restype, lib.dd_window_attention_backward_supported.argtypes = c_int, [c_int] * 4
        lib.dd_window_attention_backward_workspace_bytes.restype = c_int
        lib.dd_window_attention_backward_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
        lib.dd_window_attention_backward.restype, lib.dd_window_attention_backward.argtypes = c_int, [c_vp] * 9 + [c_int] * 8 + [c_vp]
        _bound = lib
    return _bound


def _precision_id(precision: str) -> int:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {list(PRECISIONS)} (got {precision!r})")
    return PRECISIONS[precision]


def supported(C: int, heads: int, window: int, precision: str = "fp32") -> bool:
    """What dd_window_attention_supported answers (no device needed)."""
    return bool(_lib().dd_window_attention_supported(int(C), int(heads), int(window), _precision_id(precision)))


# ---- the relative-position bias ----------------------------------------------------------------------------------------------------------------
def relative_position_index(window: int = WINDOW) -> torch.Tensor:
    """[N, N] rows of the (2 window - 1)^2 bias table: query i at (yi, xi), key j at (yj, xj) -> (yi - yj + window - 1) (2 window - 1) +
    (xi - xj + window - 1).  The reference builds the same numbers with double_step_seq and a flip."""
    pos = torch.arange(window * window)
    y, x = pos // window, pos % window
    return ((y[:, None] - y[None, :] + window - 1) * (2 * window - 1) + (x[:, None] - x[None, :] + window - 1)).contiguous()


def dense_bias(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """relative_position_bias_table[relative_position_index] permuted to the dense [heads, N, N] the operator reads."""
    n = index.shape[0]
    return table[index.reshape(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()


# ---- the torch composition: the reference's op sequence, from qkv on ------------------------------------------------------------------------------
def _partition(x: torch.Tensor, window: int) -> torch.Tensor:
    B, H, W, C = x.shape
    x = x.view(B, H // window, window, W // window, window, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, window, window, C)


def _reverse(windows: torch.Tensor, H: int, W: int, window: int) -> torch.Tensor:
    B = windows.shape[0] // ((H // window) * (W // window))
    x = windows.view(B, H // window, W // window, window, window, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def _shift_mask(Hp: int, Wp: int, window: int, shift: int, device, dtype) -> torch.Tensor:
    """[nW, N, N]: 0 where query and key of a window carry the same band label, -100 elsewhere (labels on the rolled padded frame)."""
    img = torch.zeros((1, Hp, Wp, 1), device=device, dtype=dtype)
    bands = (slice(0, -window), slice(-window, -shift), slice(-shift, None))
    cnt = 0
    for h in bands:
        for w in bands:
            img[:, h, w, :] = cnt
            cnt += 1
    lab = _partition(img, window).view(-1, window * window)
    diff = lab.unsqueeze(1) - lab.unsqueeze(2)
    return diff.masked_fill(diff != 0, -100.0).masked_fill(diff == 0, 0.0)


def _attend(qkv_windows: torch.Tensor, rel_bias: torch.Tensor, mask: Optional[torch.Tensor], heads: int, scale: float, attn_drop=None,
            round_to: Optional[torch.dtype] = None) -> torch.Tensor:
    """[Bw, N, 3 C] -> [Bw, N, C]: the body of the reference's WindowMSA between its two Linears.  ``round_to`` (bf16 / f16) rounds q * scale, k,
    the probabilities and v once each and keeps every sum in the input's type: what the library's 16-bit modes compute."""
    Bw, N, C3 = qkv_windows.shape
    C = C3 // 3
    qkv = qkv_windows.reshape(Bw, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    rnd = (lambda t: t.to(round_to).to(t.dtype)) if round_to is not None else (lambda t: t)
    q = rnd(q * scale)
    attn = q @ rnd(k).transpose(-2, -1)
    attn = attn + rel_bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = attn.view(Bw // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, N, N)
    attn = rnd(attn.softmax(dim=-1))
    if attn_drop is not None:
        attn = attn_drop(attn)
    return (attn @ rnd(v)).transpose(1, 2).reshape(Bw, N, C)


def window_attention_torch(qkv: torch.Tensor, qkv_pad: Optional[torch.Tensor], rel_bias: torch.Tensor, heads: int, window: int, shift: int,
                           round_to: Optional[torch.dtype] = None) -> torch.Tensor:
    """What dd_window_attention_forward computes, as the reference's sequence of torch ops on ``qkv`` [B, H, W, 3 C]: pad (padded tokens hold
    ``qkv_pad``, or zeros), roll, mask, partition, attention, reverse, roll, crop -> [B, H, W, C].  Differentiable; any device and float type."""
    B, H, W, C3 = qkv.shape
    if not 0 <= shift < window:
        raise ValueError(f"shift must be in 0 .. window - 1 (got {shift}, window {window})")
    pad_r, pad_b = (window - W % window) % window, (window - H % window) % window
    x = F.pad(qkv, (0, 0, 0, pad_r, 0, pad_b))
    if qkv_pad is not None and (pad_r or pad_b):
        inside = F.pad(torch.ones((1, H, W, 1), dtype=torch.bool, device=qkv.device), (0, 0, 0, pad_r, 0, pad_b))
        x = torch.where(inside, x, qkv_pad.to(x.dtype).view(1, 1, 1, -1))
    Hp, Wp = H + pad_b, W + pad_r
    mask = None
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        mask = _shift_mask(Hp, Wp, window, shift, qkv.device, qkv.dtype)
    windows = _partition(x, window).view(-1, window * window, C3)
    y = _attend(windows, rel_bias, mask, heads, float(C3 // 3 // heads) ** -0.5, round_to=round_to)
    y = _reverse(y.view(-1, window, window, C3 // 3), Hp, Wp, window)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y[:, :H, :W, :].contiguous()


# ---- the library call ------------------------------------------------------------------------------------------------------------------------------
def _native(t: Optional[torch.Tensor]) -> bool:
    return t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not (t.requires_grad and torch.is_grad_enabled()))


def window_attention_forward(qkv: torch.Tensor, qkv_pad: Optional[torch.Tensor], rel_bias: torch.Tensor, heads: int, window: int, shift: int,
                             precision: str = "fp32") -> torch.Tensor:
    """One dd_window_attention_forward on contiguous fp32 HIP tensors; anything the library does not take is an error here."""
    for name, t in (("qkv", qkv), ("qkv_pad", qkv_pad), ("rel_bias", rel_bias)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous fp32 tensor on a HIP device (got {t.dtype} on {t.device}); there is no CPU library path")
    if qkv.dim() != 4 or qkv.shape[3] % 3:
        raise ValueError(f"qkv must be [B, H, W, 3 C] (got {tuple(qkv.shape)})")
    B, H, W, C = int(qkv.shape[0]), int(qkv.shape[1]), int(qkv.shape[2]), int(qkv.shape[3]) // 3
    n = window * window
    if tuple(rel_bias.shape) != (heads, n, n):
        raise ValueError(f"rel_bias must be [{heads}, {n}, {n}] (got {tuple(rel_bias.shape)})")
    if qkv_pad is not None and qkv_pad.numel() != 3 * C:
        raise ValueError(f"qkv_pad must hold {3 * C} values (got {qkv_pad.numel()})")
    if qkv_pad is not None and qkv_pad.data_ptr() % 16:
        qkv_pad = qkv_pad.clone()      # (a view into a larger buffer: the kernel reads it in 16-byte pieces)
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = _lib().dd_window_attention_forward(qkv.data_ptr(), qkv_pad.data_ptr() if qkv_pad is not None else None, rel_bias.data_ptr(),
                                                out.data_ptr(), B, H, W, C, heads, window, shift, _precision_id(precision),
                                                int(torch.cuda.current_stream(qkv.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"dd_window_attention_forward failed ({rc}): {_lib().dd_swin_last_error().decode()}")
    return out


def window_attention(qkv: torch.Tensor, qkv_pad: Optional[torch.Tensor], rel_bias: torch.Tensor, heads: int, window: int, shift: int,
                     precision: str = "fp32") -> torch.Tensor:
    """[B, H, W, 3 C] -> [B, H, W, C].  Contiguous fp32 HIP tensors that need no gradient, at a shape the operator runs, go through the library;
    everything else runs ``window_attention_torch`` (in the tensors' own type; ``precision`` is the library's operand type)."""
    _precision_id(precision)
    if qkv.dim() == 4 and qkv.is_cuda and all(_native(t) for t in (qkv, qkv_pad, rel_bias)) and \
            supported(qkv.shape[3] // 3, heads, window, precision) and qkv.shape[3] == 3 * HEAD_DIM * heads:
        return window_attention_forward(qkv, qkv_pad, rel_bias, heads, window, shift, precision)
    return window_attention_torch(qkv, qkv_pad, rel_bias, heads, window, shift)


# ---- the backward ------------------------------------------------------------------------------------------------------------------------------------
def backward_workspace_bytes(B: int, H: int, W: int, C: int, heads: int, window: int = WINDOW, precision: str = "fp32") -> int:
    """What dd_window_attention_backward_workspace_bytes answers (no device needed): a function of the shape alone."""
    n = ctypes.c_int64(0)
    rc = _lib().dd_window_attention_backward_workspace_bytes(int(B), int(H), int(W), int(C), int(heads), int(window), _precision_id(precision),
                                                             ctypes.byref(n))
    if rc != 0:
        raise RuntimeError(f"dd_window_attention_backward_workspace_bytes failed ({rc}): {_lib().dd_swin_last_error().decode()}")
    return int(n.value)


_workspaces = {}      # (device, stream) -> a float tensor that only grows: calls on one stream are ordered, so they can share it


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    key = (device, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _workspaces[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return ws


def window_attention_backward(qkv: torch.Tensor, qkv_pad: Optional[torch.Tensor], rel_bias: torch.Tensor, grad_out: torch.Tensor, heads: int,
                              window: int, shift: int, precision: str = "fp32", scale: Optional[torch.Tensor] = None, need_pad: bool = True,
                              need_bias: bool = True):
    """One dd_window_attention_backward on contiguous fp32 HIP tensors -> (grad_qkv, grad_qkv_pad or None, grad_rel_bias [heads, 49, 49] or
    None).  ``scale``: the 4-float tensor of ``conv.grad_scale`` for grad_out (read at "f16" only) or None.  The workspace is cached per device
    and stream; nothing synchronises the host."""
    for name, t in (("qkv", qkv), ("qkv_pad", qkv_pad), ("rel_bias", rel_bias), ("grad_out", grad_out), ("scale", scale)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"{name} must be a contiguous fp32 tensor on a HIP device (got {t.dtype} on {t.device}); there is no CPU library path")
    if qkv.dim() != 4 or qkv.shape[3] % 3:
        raise ValueError(f"qkv must be [B, H, W, 3 C] (got {tuple(qkv.shape)})")
    B, H, W, C = int(qkv.shape[0]), int(qkv.shape[1]), int(qkv.shape[2]), int(qkv.shape[3]) // 3
    n = window * window
    if tuple(rel_bias.shape) != (heads, n, n):
        raise ValueError(f"rel_bias must be [{heads}, {n}, {n}] (got {tuple(rel_bias.shape)})")
    if tuple(grad_out.shape) != (B, H, W, C):
        raise ValueError(f"grad_out must be [{B}, {H}, {W}, {C}] (got {tuple(grad_out.shape)})")
    if qkv_pad is not None and qkv_pad.numel() != 3 * C:
        raise ValueError(f"qkv_pad must hold {3 * C} values (got {qkv_pad.numel()})")
    if scale is not None and scale.numel() < 4:
        raise ValueError("scale must be the 4-float tensor conv.grad_scale returns")
    if qkv_pad is not None and qkv_pad.data_ptr() % 16:
        qkv_pad = qkv_pad.clone()
    if grad_out.data_ptr() % 16:
        grad_out = grad_out.clone()
    dev = qkv.device
    grad_qkv = torch.empty_like(qkv)
    grad_pad = torch.empty(3 * C, dtype=torch.float32, device=dev) if need_pad else None
    grad_bias = torch.empty((heads, n, n), dtype=torch.float32, device=dev) if need_bias else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        ws = _workspace(backward_workspace_bytes(B, H, W, C, heads, window, precision), dev)
        rc = _lib().dd_window_attention_backward(qkv.data_ptr(), ptr(qkv_pad), rel_bias.data_ptr(), grad_out.data_ptr(), grad_qkv.data_ptr(),
                                                 ptr(grad_pad), ptr(grad_bias), ws.data_ptr(), ptr(scale), B, H, W, C, heads, window, shift,
                                                 _precision_id(precision), int(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"dd_window_attention_backward failed ({rc}): {_lib().dd_swin_last_error().decode()}")
    return grad_qkv, grad_pad, grad_bias


class WindowAttentionFunction(torch.autograd.Function):
    """``apply(qkv, qkv_pad, rel_bias, heads, window, shift, precision="fp32", grad_autoscale=True)``: dd_window_attention_forward (the bits of
    ``window_attention_forward``) with dd_window_attention_backward as its gradient.  Saves qkv, qkv_pad and rel_bias only.  With
    ``grad_autoscale`` the "f16" backward is preceded by dd_conv_grad_scale on grad_out (include/ddepth_conv_scaled.h).  Gradients: qkv, qkv_pad
    and the DENSE bias; ``dense_bias_folded`` makes the table's gradient a fixed gather of the latter."""

    @staticmethod
    def forward(ctx, qkv, qkv_pad, rel_bias, heads, window, shift, precision="fp32", grad_autoscale=True):
        out = window_attention_forward(qkv, qkv_pad, rel_bias, heads, window, shift, precision)
        ctx.save_for_backward(qkv, qkv_pad, rel_bias)
        ctx.cfg = (int(heads), int(window), int(shift), precision, bool(grad_autoscale))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, qkv_pad, rel_bias = ctx.saved_tensors
        heads, window, shift, precision, autoscale = ctx.cfg
        grad_out = grad_out.contiguous()
        scale = None
        if precision == "f16" and autoscale:
            from . import conv
            scale = conv.grad_scale(grad_out, PRECISIONS["f16"])      # (dd_precision: the same enum)
        need = ctx.needs_input_grad
        gq, gp, gb = window_attention_backward(qkv, qkv_pad, rel_bias, grad_out, heads, window, shift, precision, scale,
                                               need_pad=qkv_pad is not None and need[1], need_bias=need[2])
        return (gq if need[0] else None), gp, gb, None, None, None, None, None


_fold_cache = {}


def bias_fold_index(window: int = WINDOW) -> torch.Tensor:
    """[(2 window - 1)^2, window^2] (CPU, int64): for every row of the bias table the flat positions query * N + key of the dense [N, N] bias that
    read it, in ascending order, padded with N * N -- the index of one appended zero."""
    if window not in _fold_cache:
        n = window * window
        flat = relative_position_index(window).reshape(-1)
        rows = torch.full(((2 * window - 1) ** 2, n), n * n, dtype=torch.int64)
        for t in range(rows.shape[0]):
            pos = torch.nonzero(flat == t).reshape(-1)
            rows[t, :pos.numel()] = pos
        _fold_cache[window] = rows
    return _fold_cache[window]


def fold_bias_grad(grad_dense: torch.Tensor, fold: torch.Tensor) -> torch.Tensor:
    """The table's gradient [(2 window - 1)^2, heads] from the dense one [heads, N, N]: a gather and a sum in a fixed order, no scatter-add (whose
    atomics would make the sum's order, and its bits, vary from run to run)."""
    heads = grad_dense.shape[0]
    padded = torch.cat([grad_dense.reshape(heads, -1), grad_dense.new_zeros(heads, 1)], dim=1)
    return padded[:, fold].sum(-1).t().contiguous()


class _DenseBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, index, fold):
        ctx.fold = fold      # (a constant index, kept by the module: not a tensor saved for this backward)
        return dense_bias(table, index)

    @staticmethod
    def backward(ctx, grad_dense):
        return fold_bias_grad(grad_dense.contiguous(), ctx.fold), None, None


def dense_bias_folded(table: torch.Tensor, index: torch.Tensor, fold: torch.Tensor) -> torch.Tensor:
    """``dense_bias`` (the same bits) whose backward is ``fold_bias_grad``; ``fold``: ``bias_fold_index`` on the table's device."""
    return _DenseBias.apply(table, index, fold)


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """Stochastic depth per sample (the reference's default dropout_layer); the identity at drop_prob 0 or in .eval()."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x.div(keep) * mask


def _build_dropout(cfg) -> nn.Module:
    if cfg is None:
        return nn.Identity()
    cfg = dict(cfg)
    kind = cfg.pop("type", "DropPath")
    if kind == "DropPath":
        return DropPath(cfg.get("drop_prob", 0.0))
    if kind == "Dropout":
        return nn.Dropout(cfg.get("p", cfg.get("drop_prob", 0.5)))
    raise ValueError(f"dropout_layer type {kind!r}: DropPath or Dropout")


class WindowMSA(nn.Module):
    """The parameters of the reference's WindowMSA under the same names; HipShiftWindowMSA.forward drives them."""

    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_drop_rate=0., proj_drop_rate=0., init_cfg=None):
        super().__init__()
        self.embed_dims = embed_dims
        self.window_size = tuple(window_size)
        self.num_heads = num_heads
        self.scale = qk_scale or (embed_dims // num_heads) ** -0.5
        self.init_cfg = init_cfg
        Wh, Ww = self.window_size
        if Wh != Ww:
            raise ValueError("square windows only")
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * Wh - 1) * (2 * Ww - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(Wh))
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.proj = nn.Linear(embed_dims, embed_dims)
        self.proj_drop = nn.Dropout(proj_drop_rate)
        self.softmax = nn.Softmax(dim=-1)

    def init_weights(self):
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


def _active(drop: Optional[nn.Module], training: bool) -> bool:
    if drop is None or not training:
        return False
    p = getattr(drop, "p", None)
    if p is None:
        p = getattr(drop, "drop_prob", None)
    return p is None and not isinstance(drop, nn.Identity) or bool(p)


class HipShiftWindowMSA(nn.Module):
    """The reference's ShiftWindowMSA: same constructor keywords, attributes and state-dict keys (``w_msa.qkv.*``, ``w_msa.proj.*``,
    ``w_msa.relative_position_bias_table``, ``w_msa.relative_position_index``).  Without autograd on HIP fp32 tensors ``forward`` is the ``qkv``
    Linear on the tokens as they are, one library call, the ``proj`` Linear and ``drop``; otherwise the reference's sequence in torch.
    ``linear="hip"`` (``linear.convert_hip_swin_linears``) runs the two Linears of that inference branch in the library too, at
    ``linear_precision``; the default ``linear="torch"`` changes nothing."""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_drop_rate=0, proj_drop_rate=0,
                 dropout_layer=dict(type="DropPath", drop_prob=0.), init_cfg=None, precision="fp32", backward="torch", grad_autoscale=True,
                 linear="torch", linear_precision=None):
        super().__init__()
        self.window_size = window_size
        self.shift_size = shift_size
        assert 0 <= self.shift_size < self.window_size
        self.w_msa = WindowMSA(embed_dims=embed_dims, num_heads=num_heads, window_size=(window_size, window_size), qkv_bias=qkv_bias,
                               qk_scale=qk_scale, attn_drop_rate=attn_drop_rate, proj_drop_rate=proj_drop_rate, init_cfg=None)
        self.drop = _build_dropout(dropout_layer)
        self.init_cfg = init_cfg
        _precision_id(precision)
        self.precision = precision
        self.backward = _backward_choice(backward)
        self.grad_autoscale = bool(grad_autoscale)
        self.linear = _linear_choice(linear)
        self.linear_precision = linear_precision      # (None: the attention's)
        if linear_precision is not None:
            _precision_id(linear_precision)
        self._bias_cache = None
        self._fold = None

    @classmethod
    def from_module(cls, m: nn.Module, precision: str = "fp32", backward: str = "torch", grad_autoscale: bool = True) -> "HipShiftWindowMSA":
        """A HipShiftWindowMSA around the SAME ``w_msa`` and ``drop`` modules as the duck-typed ``m``: same tensors, same keys."""
        _precision_id(precision)
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        new.window_size = int(m.window_size)
        new.shift_size = int(m.shift_size)
        new.w_msa = m.w_msa
        new.drop = m.drop if isinstance(getattr(m, "drop", None), nn.Module) else nn.Identity()
        new.init_cfg = getattr(m, "init_cfg", None)
        new.precision = precision
        new.backward = _backward_choice(backward)
        new.grad_autoscale = bool(grad_autoscale)
        new.linear, new.linear_precision = "torch", None
        new._bias_cache = None
        new._fold = None
        new.train(m.training)
        return new

    # -- what decides the route ------------------------------------------------------------------------------------------------------------------
    def _dense_bias(self) -> torch.Tensor:
        """The dense [heads, 49, 49] bias, rebuilt when the table was written (its _version) or moved (its device)."""
        table = self.w_msa.relative_position_bias_table
        key = (table._version, table.device, table.data_ptr())
        if self._bias_cache is None or self._bias_cache[0] != key:
            with torch.no_grad():
                self._bias_cache = (key, dense_bias(table.detach(), self.w_msa.relative_position_index))
        return self._bias_cache[1]

    def _library_route(self, query: torch.Tensor) -> bool:
        w = self.w_msa
        if torch.is_grad_enabled() and (self.training or query.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if not (query.is_cuda and query.dtype == torch.float32 and w.qkv.weight.is_cuda and w.qkv.weight.dtype == torch.float32):
            return False
        if torch.is_autocast_enabled():
            return False
        if any(_active(getattr(o, n, None), self.training) for o, n in ((w, "attn_drop"), (w, "proj_drop"), (self, "drop"))):
            return False
        heads = int(w.num_heads)
        if abs(float(w.scale) - HEAD_DIM ** -0.5) > 1e-12 or query.shape[-1] != HEAD_DIM * heads:
            return False
        return supported(query.shape[-1], heads, self.window_size, self.precision)

    def _linear_route(self, query: torch.Tensor) -> bool:
        """On the library route (``_library_route`` holds): ``linear="hip"``, a contiguous query, and ``qkv`` and ``proj`` plain Linears the
        operator runs.  Otherwise they stay torch calls, as with ``linear="torch"``."""
        if getattr(self, "linear", "torch") != "hip":
            return False
        w = self.w_msa
        lp = self.linear_precision or self.precision
        C = query.shape[-1]
        if not _linear.linear_native(w.qkv, query, _linear.ACT_NONE, lp) or w.qkv.out_features != 3 * C:
            return False
        p = w.proj
        return type(p) is nn.Linear and p.in_features == C and p.weight.is_cuda and p.weight.dtype == torch.float32 and \
            p.weight.is_contiguous() and (p.bias is None or p.bias.is_contiguous()) and _linear.supported(C, p.out_features, _linear.ACT_NONE, lp)

    def _train_route(self, query: torch.Tensor) -> bool:
        """``backward="hip"`` and something needs a gradient: HIP fp32 tensors, window 7, head dimension 32, no autocast, an inactive attn_drop.
        ``proj_drop`` and ``drop`` sit behind ``proj`` as torch modules and do not matter."""
        w = self.w_msa
        if self.backward != "hip" or not torch.is_grad_enabled():
            return False
        if not (query.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if not (query.is_cuda and query.dtype == torch.float32 and w.qkv.weight.is_cuda and w.qkv.weight.dtype == torch.float32):
            return False
        if torch.is_autocast_enabled() or _active(getattr(w, "attn_drop", None), self.training):
            return False
        heads = int(w.num_heads)
        if abs(float(w.scale) - HEAD_DIM ** -0.5) > 1e-12 or query.shape[-1] != HEAD_DIM * heads:
            return False
        return supported(query.shape[-1], heads, self.window_size, self.precision)

    def _fold_index(self, device) -> torch.Tensor:
        if self._fold is None or self._fold.device != device:
            self._fold = bias_fold_index(self.window_size).to(device)
        return self._fold

    def forward(self, query, hw_shape):
        B, L, C = query.shape
        H, W = hw_shape
        assert L == H * W, "input feature has wrong size"
        w = self.w_msa
        if self._train_route(query):
            qkv = w.qkv(query).view(B, H, W, 3 * C).contiguous()
            table = w.relative_position_bias_table
            bias = dense_bias_folded(table, w.relative_position_index, self._fold_index(table.device))
            x = WindowAttentionFunction.apply(qkv, w.qkv.bias, bias, int(w.num_heads), self.window_size, self.shift_size, self.precision,
                                              self.grad_autoscale)
            x = w.proj(x.view(B, L, C))
            proj_drop = getattr(w, "proj_drop", None)
            return self.drop(proj_drop(x) if proj_drop is not None else x)
        if self._library_route(query):
            if self._linear_route(query):
                # linear="hip": qkv and proj in the library as well (include/swin/ddepth_linear.h), their weights packed once
                lp = self.linear_precision or self.precision
                qkv = _linear.linear_forward(query, _linear.packed_for(self, "qkv", w.qkv, lp), w.qkv.bias, None, _linear.ACT_NONE, lp)
                x = window_attention_forward(qkv.view(B, H, W, 3 * C), w.qkv.bias, self._dense_bias(), int(w.num_heads), self.window_size,
                                             self.shift_size, self.precision)
                x = _linear.linear_forward(x.view(B, L, C), _linear.packed_for(self, "proj", w.proj, lp), w.proj.bias, None, _linear.ACT_NONE, lp)
                proj_drop = getattr(w, "proj_drop", None)
                return self.drop(proj_drop(x) if proj_drop is not None else x)
            qkv = w.qkv(query).view(B, H, W, 3 * C)
            x = window_attention_forward(qkv.contiguous(), w.qkv.bias, self._dense_bias(), int(w.num_heads), self.window_size, self.shift_size,
                                         self.precision)
            x = w.proj(x.view(B, L, C))
            proj_drop = getattr(w, "proj_drop", None)
            return self.drop(proj_drop(x) if proj_drop is not None else x)
        return self._forward_torch(query, H, W)

    def _forward_torch(self, query, H, W):
        """The reference's sequence: pad the tokens, roll, build the mask, partition, WindowMSA on the windows, reverse, roll, crop, drop."""
        B, L, C = query.shape
        ws, shift, w = self.window_size, self.shift_size, self.w_msa
        x = query.view(B, H, W, C)
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        Hp, Wp = x.shape[1], x.shape[2]
        mask = None
        if shift > 0:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
            mask = _shift_mask(Hp, Wp, ws, shift, query.device, torch.float32)
        windows = _partition(x, ws).view(-1, ws * ws, C)
        bias = dense_bias(w.relative_position_bias_table, w.relative_position_index)
        y = _attend(w.qkv(windows), bias, mask, int(w.num_heads), float(w.scale), attn_drop=getattr(w, "attn_drop", None))
        y = w.proj(y)
        proj_drop = getattr(w, "proj_drop", None)
        if proj_drop is not None:
            y = proj_drop(y)
        y = _reverse(y.view(-1, ws, ws, C), Hp, Wp, ws)
        if shift > 0:
            y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
        if pad_r > 0 or pad_b:
            y = y[:, :H, :W, :].contiguous()
        return self.drop(y.view(B, H * W, C))


def _linear_choice(linear: str) -> str:
    if linear not in _linear.LINEAR_BACKENDS:
        raise ValueError(f"linear must be one of {list(_linear.LINEAR_BACKENDS)} (got {linear!r})")
    return linear


def _backward_choice(backward: str) -> str:
    if backward not in BACKWARDS:
        raise ValueError(f"backward must be one of {list(BACKWARDS)} (got {backward!r})")
    return backward


def _matches(m: nn.Module) -> bool:
    w = getattr(m, "w_msa", None)
    return hasattr(m, "window_size") and hasattr(m, "shift_size") and w is not None and \
        all(hasattr(w, a) for a in ("qkv", "proj", "num_heads", "relative_position_bias_table", "relative_position_index"))


def _convertible(m: nn.Module, precision: str) -> bool:
    w = m.w_msa
    if not isinstance(m.window_size, int) or not isinstance(w.qkv, nn.Linear) or not isinstance(w.proj, nn.Linear):
        return False
    if abs(float(getattr(w, "scale", HEAD_DIM ** -0.5)) - HEAD_DIM ** -0.5) > 1e-12:
        return False
    return w.qkv.out_features == 3 * w.qkv.in_features and supported(w.qkv.in_features, int(w.num_heads), m.window_size, precision)


def convert_hip_window_attention(module: nn.Module, precision: str = "fp32", backward: str = "torch", grad_autoscale: bool = True) -> nn.Module:
    """Replaces every duck-typed shifted-window attention of ``module`` (``window_size``, ``shift_size`` and a ``w_msa`` with ``qkv``, ``proj``,
    ``num_heads``, ``relative_position_bias_table``, ``relative_position_index`` -- the reference's own class included) that the operator runs by
    a ``HipShiftWindowMSA`` holding the SAME parameter and buffer tensors under the same keys.  Modules it does not run (another window, a head
    dimension other than 32, a custom qk_scale) are left alone; calling it again changes nothing.  ``backward="hip"``: the converted modules
    also run what needs a gradient in the library (``WindowAttentionFunction``), at "f16" with ``grad_autoscale``."""
    _precision_id(precision)
    _backward_choice(backward)
    if isinstance(module, HipShiftWindowMSA):
        return module
    if _matches(module):
        return HipShiftWindowMSA.from_module(module, precision, backward, grad_autoscale) if _convertible(module, precision) else module
    for name, child in list(module.named_children()):
        new = convert_hip_window_attention(child, precision, backward, grad_autoscale)
        if new is not child:
            setattr(module, name, new)
    return module


def resolve_attention_backend(choice=None) -> str:
    """``args.backbone_attention`` / DDEPTH_BACKBONE_ATTENTION: "torch" (default; empty or absent), "hip" (inference) or "hip+train" ("hip" plus
    ``backward="hip"``)."""
    choice = choice or os.environ.get("DDEPTH_BACKBONE_ATTENTION") or "torch"
    if choice not in ATTENTION_BACKENDS:
        raise ValueError(f"backbone_attention must be one of {list(ATTENTION_BACKENDS)} (got {choice!r})")
    return choice


def resolve_attention_precision(choice=None) -> str:
    """``args.backbone_attention_precision`` / DDEPTH_BACKBONE_ATTENTION_PRECISION: "fp32" (default), "bf16" or "f16"."""
    choice = choice or os.environ.get("DDEPTH_BACKBONE_ATTENTION_PRECISION") or "fp32"
    if choice not in PRECISIONS:
        raise ValueError(f"backbone_attention_precision must be one of {list(PRECISIONS)} (got {choice!r})")
    return choice


def resolve_attention_grad_autoscale(choice=None) -> bool:
    """``args.backbone_attention_grad_autoscale`` / DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE: on by default; "0" / "false" / "off" / "no" or a
    false value switch the f16 backward's rescale of grad_out off."""
    if choice is None:
        choice = os.environ.get("DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE")
    if choice is None or choice == "":
        return True
    if isinstance(choice, str):
        if choice.lower() in ("1", "true", "on", "yes"):
            return True
        if choice.lower() in ("0", "false", "off", "no"):
            return False
        raise ValueError(f"backbone_attention_grad_autoscale must be a boolean (got {choice!r})")
    return bool(choice)
