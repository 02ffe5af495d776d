"""The token Linears of a Swin block over the C ABI of include/swin/ddepth_linear.h: ``qkv`` and ``proj`` around the shifted-window attention, and the
MLP (``fc1`` with GELU in its epilogue, ``fc2`` with the block's residual in its epilogue), for inference.

    convert_hip_swin_linears(backbone, precision="bf16")      # or: args.backbone_linear = "hip" / DDEPTH_BACKBONE_LINEAR=hip

``y = act(x . w^T + bias) + addend`` on fp32 token tensors as torch holds them (csrc/dd_linear.hip); ``precision`` is the MFMA operand type
("fp32" is the parity mode; "bf16" / "f16" round x and w once), accumulation and epilogue are fp32.  The weight is packed once per
(weight version, device, storage, precision) and the image kept beside the module (``packed_for``): a plain attribute, never in a state dict.

The library route is decided BEFORE the call and taken only without autograd, for contiguous fp32 tensors on a HIP device, outside autocast,
with no active dropout, at widths the operator runs.  Everything else -- training, a tensor that needs a gradient, CPU tensors, other
activations -- runs the module's own torch sequence.  It is never a fallback after an error.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch
import torch.nn as nn

from . import backend

# every symbol include/swin/ddepth_linear.h declares (checked by tests/test_linear_cpu.py)
ABI_SYMBOLS = ["dd_linear_last_error", "dd_linear_supported", "dd_linear_packed_bytes", "dd_linear_pack", "dd_linear_forward"]
PRECISIONS = {"fp32": 1, "bf16": 2, "f16": 3}      # dd_precision
ACT_NONE, ACT_GELU = 0, 1
LINEAR_BACKENDS = ("torch", "hip")
PACK_COUNT = 0      # dd_linear_pack calls so far: tests assert that a second forward packs nothing

_bound = None


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp = ctypes.c_int, ctypes.c_void_p
        lib.dd_linear_last_error.restype, lib.dd_linear_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_linear_supported.restype, lib.dd_linear_supported.argtypes = c_int, [c_int] * 4
        lib.dd_linear_packed_bytes.restype, lib.dd_linear_packed_bytes.argtypes = c_int, [c_int] * 3 + [ctypes.POINTER(ctypes.c_int64)]
        lib.dd_linear_pack.restype, lib.dd_linear_pack.argtypes = c_int, [c_vp, c_vp] + [c_int] * 3 + [c_vp]
        lib.dd_linear_forward.restype, lib.dd_linear_forward.argtypes = c_int, [c_vp] * 5 + [ctypes.c_longlong] + [c_int] * 4 + [c_vp]
        _bound = lib
    return _bound


def _precision_id(precision: str) -> int:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {list(PRECISIONS)} (got {precision!r})")
    return PRECISIONS[precision]


def supported(K: int, N: int, act: int = ACT_NONE, precision: str = "bf16") -> bool:
    """What dd_linear_supported answers (no device needed)."""
    return bool(_lib().dd_linear_supported(int(K), int(N), int(act), _precision_id(precision)))


def packed_bytes(K: int, N: int, precision: str = "bf16") -> int:
    """What dd_linear_packed_bytes answers (no device needed)."""
    n = ctypes.c_int64(0)
    rc = _lib().dd_linear_packed_bytes(int(K), int(N), _precision_id(precision), ctypes.byref(n))
    if rc != 0:
        raise RuntimeError(f"dd_linear_packed_bytes failed ({rc}): {_lib().dd_linear_last_error().decode()}")
    return int(n.value)


class PackedWeight:
    """The operand image of one [N, K] weight at one precision: ``data`` is a uint8 tensor of ``packed_bytes(K, N, precision)``."""
    __slots__ = ("data", "K", "N", "precision")

    def __init__(self, data, K, N, precision):
        self.data, self.K, self.N, self.precision = data, K, N, precision


def _check(name: str, t: Optional[torch.Tensor]) -> None:
    if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous fp32 tensor on a HIP device (got {t.dtype} on {t.device}); there is no CPU library path")


def pack_weight(weight: torch.Tensor, precision: str = "bf16") -> PackedWeight:
    """One dd_linear_pack of an ``nn.Linear.weight`` [N, K]; anything the library does not take is an error here."""
    global PACK_COUNT
    pid = _precision_id(precision)
    weight = weight.detach()
    _check("weight", weight)
    if weight.dim() != 2:
        raise ValueError(f"weight must be [N, K] (got {tuple(weight.shape)})")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    if not supported(K, N, ACT_NONE, precision):
        raise RuntimeError(f"a Linear {K} -> {N} does not run in the library (multiples of 32 in 32 .. 8192)")
    if weight.data_ptr() % 16:
        weight = weight.clone()
    data = torch.empty(packed_bytes(K, N, precision), dtype=torch.uint8, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = _lib().dd_linear_pack(weight.data_ptr(), data.data_ptr(), K, N, pid, int(torch.cuda.current_stream(weight.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"dd_linear_pack failed ({rc}): {_lib().dd_linear_last_error().decode()}")
    PACK_COUNT += 1
    return PackedWeight(data, K, N, precision)


def linear_forward(x: torch.Tensor, packed: PackedWeight, bias: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None,
                   act: int = ACT_NONE, precision: str = "bf16") -> torch.Tensor:
    """One dd_linear_forward: ``x`` [..., K] -> [..., N] = act(x . w^T + bias) + addend on contiguous fp32 HIP tensors; anything the library
    does not take is an error here."""
    pid = _precision_id(precision)
    if bias is not None:
        bias = bias.detach()
    for name, t in (("x", x), ("bias", bias), ("addend", addend)):
        _check(name, t)
    if packed.precision != precision:
        raise ValueError(f"the weight was packed for {packed.precision!r}, not {precision!r}")
    K, N = packed.K, packed.N
    if x.dim() < 1 or x.shape[-1] != K or x.numel() == 0:
        raise ValueError(f"x must be [..., {K}] and not empty (got {tuple(x.shape)})")
    if packed.data.device != x.device:
        raise RuntimeError(f"the packed weight is on {packed.data.device}, x on {x.device}")
    shape = tuple(x.shape[:-1]) + (N,)
    if bias is not None and bias.numel() != N:
        raise ValueError(f"bias must hold {N} values (got {bias.numel()})")
    if addend is not None and tuple(addend.shape) != shape:
        raise ValueError(f"addend must be {list(shape)} (got {list(addend.shape)})")
    if not supported(K, N, act, precision):
        raise RuntimeError(f"a Linear {K} -> {N} with act {act} does not run in the library")
    if x.data_ptr() % 16:      # (a view into a larger buffer: the kernel reads 16-byte pieces)
        x = x.clone()
    if addend is not None and addend.data_ptr() % 16:
        addend = addend.clone()
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = _lib().dd_linear_forward(x.data_ptr(), packed.data.data_ptr(), bias.data_ptr() if bias is not None else None,
                                      addend.data_ptr() if addend is not None else None, y.data_ptr(), x.numel() // K, K, N, int(act), pid,
                                      int(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"dd_linear_forward failed ({rc}): {_lib().dd_linear_last_error().decode()}")
    return y


# ---- the pack cache: one image per Linear, kept on the module that drives it -------------------------------------------------------------------------
def packed_for(owner: nn.Module, name: str, lin: nn.Linear, precision: str) -> PackedWeight:
    """The packed image of ``lin.weight``, rebuilt when the weight was written (its _version), moved (device, storage) or the precision
    changed.  Kept in ``owner._linear_packs[name]``: a plain attribute, never a buffer or a parameter."""
    w = lin.weight
    key = (w._version, w.device, w.data_ptr(), precision)
    packs = owner.__dict__.setdefault("_linear_packs", {})
    hit = packs.get(name)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = packs[name] = (key, pack_weight(w, precision))
    return hit[1]


def _active(drop: Optional[nn.Module], training: bool) -> bool:
    if drop is None or not training or isinstance(drop, nn.Identity):
        return False
    p = getattr(drop, "p", None)
    if p is None:
        p = getattr(drop, "drop_prob", None)
    return p is None or bool(p)


def linear_native(lin: nn.Module, x: torch.Tensor, act: int, precision: str) -> bool:
    """Does ``lin(x)`` take the library route as far as the tensors go: a plain nn.Linear with fp32 HIP parameters, a contiguous fp32 HIP ``x``
    of its width, a width pair the operator runs?  (Autograd, autocast and dropout are the caller's part of the rule.)"""
    if type(lin) is not nn.Linear or not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0):
        return False
    w, b = lin.weight, lin.bias
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.device == x.device):
        return False
    if b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous()):
        return False
    return x.shape[-1] == lin.in_features and supported(lin.in_features, lin.out_features, act, precision)


# ---- the MLP -----------------------------------------------------------------------------------------------------------------------------------------
def _build_dropout(cfg) -> nn.Module:
    from .swin import _build_dropout as build
    return build(cfg)


def _build_act(cfg) -> nn.Module:
    cfg = dict(cfg or dict(type="GELU"))
    kind = cfg.pop("type")
    if kind == "GELU":
        return nn.GELU()
    if kind == "ReLU":
        return nn.ReLU(inplace=bool(cfg.get("inplace", False)))
    raise ValueError(f"act_cfg type {kind!r}: GELU or ReLU")


def _ffn_parts(m: nn.Module):
    """(fc1, act, drop1, fc2, drop2) of ``layers = Sequential(Sequential(Linear, act, Dropout), Linear, Dropout)``, or None for any other shape."""
    layers = getattr(m, "layers", None)
    if not isinstance(layers, nn.Sequential) or len(layers) != 3 or not isinstance(layers[0], nn.Sequential) or len(layers[0]) != 3:
        return None
    fc1, act, drop1 = layers[0]
    fc2, drop2 = layers[1], layers[2]
    if type(fc1) is not nn.Linear or type(fc2) is not nn.Linear or fc1.out_features != fc2.in_features:
        return None
    return fc1, act, drop1, fc2, drop2


def _gelu_erf(act: nn.Module) -> bool:
    return type(act) is nn.GELU and getattr(act, "approximate", "none") == "none"


class HipFFN(nn.Module):
    """mmcv's FFN (the reference's Swin MLP): same constructor keywords, attributes and state-dict keys (``layers.0.0.*``, ``layers.1.*``).
    Without autograd on contiguous fp32 HIP tensors ``forward`` is two library calls -- fc1 with GELU, fc2 with the identity as its addend --
    otherwise the module's own torch sequence."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="GELU"), ffn_drop=0., dropout_layer=None,
                 add_identity=True, init_cfg=None, precision="bf16"):
        super().__init__()
        assert num_fcs >= 2, f"num_fcs should be no less than 2. got {num_fcs}."
        self.embed_dims, self.feedforward_channels, self.num_fcs, self.act_cfg = embed_dims, feedforward_channels, num_fcs, act_cfg
        layers, width = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(nn.Linear(width, feedforward_channels), _build_act(act_cfg), nn.Dropout(ffn_drop)))
            width = feedforward_channels
        layers.append(nn.Linear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = _build_dropout(dropout_layer) if dropout_layer else nn.Identity()
        self.add_identity = add_identity
        self.init_cfg = init_cfg
        _precision_id(precision)
        self.precision = precision

    @classmethod
    def from_module(cls, m: nn.Module, precision: str = "bf16") -> "HipFFN":
        """A HipFFN around the SAME ``layers`` and ``dropout_layer`` modules as the duck-typed ``m``: same tensors, same keys."""
        _precision_id(precision)
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        for a in ("embed_dims", "feedforward_channels", "num_fcs", "act_cfg", "init_cfg"):
            setattr(new, a, getattr(m, a, None))
        new.layers = m.layers
        new.dropout_layer = m.dropout_layer if isinstance(getattr(m, "dropout_layer", None), nn.Module) else nn.Identity()
        new.add_identity = bool(m.add_identity)
        new.precision = precision
        new.train(m.training)
        return new

    def _library_route(self, x: torch.Tensor, identity: Optional[torch.Tensor] = None) -> bool:
        parts = _ffn_parts(self)
        if parts is None or not _gelu_erf(parts[1]):
            return False
        fc1, _, drop1, fc2, drop2 = parts
        needs_grad = x.requires_grad or (identity is not None and identity.requires_grad) or any(p.requires_grad for p in self.parameters())
        if torch.is_grad_enabled() and (self.training or needs_grad):
            return False
        if torch.is_autocast_enabled():
            return False
        if any(_active(d, self.training) for d in (drop1, drop2, self.dropout_layer)):
            return False
        if identity is not None and not (identity.is_cuda and identity.dtype == torch.float32 and identity.is_contiguous() and
                                         identity.shape == x.shape and identity.device == x.device):
            return False
        if not linear_native(fc1, x, ACT_GELU, self.precision):
            return False
        w2 = fc2.weight
        return w2.is_cuda and w2.dtype == torch.float32 and w2.is_contiguous() and w2.device == x.device and \
            (fc2.bias is None or fc2.bias.is_contiguous()) and fc2.out_features == x.shape[-1] and \
            supported(fc2.in_features, fc2.out_features, ACT_NONE, self.precision)

    def forward(self, x, identity=None):
        if self._library_route(x, identity):
            fc1, _, _, fc2, _ = _ffn_parts(self)
            hidden = linear_forward(x, packed_for(self, "fc1", fc1, self.precision), fc1.bias, None, ACT_GELU, self.precision)
            addend = (x if identity is None else identity) if self.add_identity else None
            return linear_forward(hidden, packed_for(self, "fc2", fc2, self.precision), fc2.bias, addend, ACT_NONE, self.precision)
        out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        if identity is None:
            identity = x
        return identity + self.dropout_layer(out)


def _ffn_matches(m: nn.Module) -> bool:
    return not isinstance(m, HipFFN) and hasattr(m, "add_identity") and isinstance(getattr(m, "layers", None), nn.Sequential)


def _ffn_convertible(m: nn.Module, precision: str) -> bool:
    parts = _ffn_parts(m)
    if parts is None or not _gelu_erf(parts[1]):
        return False
    fc1, _, _, fc2, _ = parts
    return fc2.out_features == fc1.in_features and supported(fc1.in_features, fc1.out_features, ACT_GELU, precision) and \
        supported(fc2.in_features, fc2.out_features, ACT_NONE, precision)


def convert_hip_swin_linears(module: nn.Module, precision: str = "bf16") -> nn.Module:
    """Sets ``linear="hip"`` (at ``precision``) on every ``swin.HipShiftWindowMSA`` of ``module`` whose ``qkv`` and ``proj`` the operator runs,
    and replaces every duck-typed FFN (``layers = Sequential(Sequential(Linear, GELU, Dropout), Linear, Dropout)``, ``add_identity`` -- mmcv's
    class included) the operator runs by a ``HipFFN`` holding the SAME modules under the same keys.  Everything else (another activation, a
    width that is no multiple of 32, three fcs) is left alone; calling it again changes nothing.  Attention modules that are not
    HipShiftWindowMSA keep their torch Linears: convert them first (``swin.convert_hip_window_attention``)."""
    from .swin import HipShiftWindowMSA
    _precision_id(precision)
    if isinstance(module, HipFFN):
        return module
    if isinstance(module, HipShiftWindowMSA):
        w = module.w_msa
        if module.linear != "hip" and type(w.qkv) is nn.Linear and type(w.proj) is nn.Linear and \
                supported(w.qkv.in_features, w.qkv.out_features, ACT_NONE, precision) and \
                supported(w.proj.in_features, w.proj.out_features, ACT_NONE, precision):
            module.linear, module.linear_precision = "hip", precision
        return module
    if _ffn_matches(module):
        return HipFFN.from_module(module, precision) if _ffn_convertible(module, precision) else module
    for name, child in list(module.named_children()):
        new = convert_hip_swin_linears(child, precision)
        if new is not child:
            setattr(module, name, new)
    return module


def resolve_linear_backend(choice=None) -> str:
    """``args.backbone_linear`` / DDEPTH_BACKBONE_LINEAR: "torch" (default; empty or absent) or "hip"."""
    choice = choice or os.environ.get("DDEPTH_BACKBONE_LINEAR") or "torch"
    if choice not in LINEAR_BACKENDS:
        raise ValueError(f"backbone_linear must be one of {list(LINEAR_BACKENDS)} (got {choice!r})")
    return choice


def resolve_linear_precision(choice=None) -> str:
    """``args.backbone_linear_precision`` / DDEPTH_BACKBONE_LINEAR_PRECISION: "bf16" (default), "fp32" or "f16"."""
    choice = choice or os.environ.get("DDEPTH_BACKBONE_LINEAR_PRECISION") or "bf16"
    if choice not in PRECISIONS:
        raise ValueError(f"backbone_linear_precision must be one of {list(PRECISIONS)} (got {choice!r})")
    return choice
