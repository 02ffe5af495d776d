"""The Swin backbone's shifted-window attention over the C ABI of include/ddepth_swin.h: inference, window 7, head dimension 32.

What it is for: the reference's ``ShiftWindowMSA`` (src/model/backbone/swin.py) runs pad -> roll -> mask build -> window partition -> ``qkv`` ->
reshape / permute -> scale -> QK^T -> + relative-position bias -> + mask -> softmax -> .V -> transpose / reshape -> ``proj`` -> window reverse ->
roll -> crop: about a dozen full-tensor passes, six of them copies.  ``HipShiftWindowMSA`` runs the ``qkv`` Linear on the tokens as they are, ONE
library call that does the rest in its addressing (csrc/dd_swin.hip), and the ``proj`` Linear.

    convert_hip_window_attention(backbone, precision="fp32")    # or: args.backbone_attention = "hip" / DDEPTH_BACKBONE_ATTENTION=hip

The library route is decided BEFORE the call and taken only without autograd, for contiguous fp32 tensors on a HIP device, window 7,
``embed_dims == 32 * num_heads`` and no active dropout.  Everything else -- training, a tensor that needs a gradient, CPU tensors, other windows --
runs the reference's sequence in torch (``window_attention_torch``, differentiable).  It is never a fallback after an error.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import backend

# every symbol include/ddepth_swin.h declares (checked by tests/test_swin_cpu.py)
ABI_SYMBOLS = ["dd_swin_last_error", "dd_window_attention_supported", "dd_window_attention_forward"]
PRECISIONS = {"fp32": 1, "bf16": 2, "f16": 3}      # dd_precision
WINDOW, HEAD_DIM = 7, 32
ATTENTION_BACKENDS = ("torch", "hip")

_bound = None


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_swin_last_error.restype, lib.dd_swin_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_window_attention_supported.restype, lib.dd_window_attention_supported.argtypes = c_int, [c_int] * 4
        lib.dd_window_attention_forward.restype, lib.dd_window_attention_forward.argtypes = c_int, [c_vp] * 4 + [c_int] * 8 + [c_vp]
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
    Linear on the tokens as they are, one library call, the ``proj`` Linear and ``drop``; otherwise the reference's sequence in torch."""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_drop_rate=0, proj_drop_rate=0,
                 dropout_layer=dict(type="DropPath", drop_prob=0.), init_cfg=None, precision="fp32"):
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
        self._bias_cache = None

    @classmethod
    def from_module(cls, m: nn.Module, precision: str = "fp32") -> "HipShiftWindowMSA":
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
        new._bias_cache = None
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

    def forward(self, query, hw_shape):
        B, L, C = query.shape
        H, W = hw_shape
        assert L == H * W, "input feature has wrong size"
        w = self.w_msa
        if self._library_route(query):
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


def convert_hip_window_attention(module: nn.Module, precision: str = "fp32") -> nn.Module:
    """Replaces every duck-typed shifted-window attention of ``module`` (``window_size``, ``shift_size`` and a ``w_msa`` with ``qkv``, ``proj``,
    ``num_heads``, ``relative_position_bias_table``, ``relative_position_index`` -- the reference's own class included) that the operator runs by
    a ``HipShiftWindowMSA`` holding the SAME parameter and buffer tensors under the same keys.  Modules it does not run (another window, a head
    dimension other than 32, a custom qk_scale) are left alone; calling it again changes nothing."""
    _precision_id(precision)
    if isinstance(module, HipShiftWindowMSA):
        return module
    if _matches(module):
        return HipShiftWindowMSA.from_module(module, precision) if _convertible(module, precision) else module
    for name, child in list(module.named_children()):
        new = convert_hip_window_attention(child, precision)
        if new is not child:
            setattr(module, name, new)
    return module


def resolve_attention_backend(choice=None) -> str:
    """``args.backbone_attention`` / DDEPTH_BACKBONE_ATTENTION: "torch" (default; empty or absent) or "hip"."""
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
