"""Diffusion_DCbase_Model facade (reference src/model/diffusion_dcbase_model.py:26-224): same
``forward(sample) -> dict`` contract, same ``args`` attributes (backbone_module/backbone_name/
head_specify/inference_steps/num_train_timesteps).  The visual backbone stays in PyTorch-ROCm; a
stem-less BasicBlock ResNet equivalent of the reference's mmbev_res18/50/101
(reference src/model/backbone/mmbev_resnet.py:101-194, which needs mmdet) is provided so the whole
model can run offline with random-init weights.  Opt-in (``args.backbone_backend="hip"`` /
DDEPTH_BACKBONE_BACKEND=hip): the backbone's convolutions run in the library (conv.convert_hip_conv
with ``channels="any", strided=True``); the default leaves the backbone as it is.  ``"hip+bn"`` adds the
BatchNorms with the block tails fused for .train(), ``"hip+fold"`` also runs every BasicBlock in .eval() under
no_grad as convolutions with BatchNorm, add and ReLU in their epilogues, ``"hip+stats"`` also takes the training
BatchNorms' statistics from the convolutions' epilogues; ``args.backbone_precision`` /
DDEPTH_BACKBONE_PRECISION gives the backbone a precision of its own.  Independent of it, ``args.backbone_attention="hip"`` /
DDEPTH_BACKBONE_ATTENTION=hip runs every shifted-window attention of a Swin backbone (resolved or injected) as one library call in
inference (swin.convert_hip_window_attention), at ``args.backbone_attention_precision`` / DDEPTH_BACKBONE_ATTENTION_PRECISION
("fp32" by default, "bf16", "f16"); ``"hip+train"`` also runs its backward in the library (``backward="hip"``), at "f16" with
``args.backbone_attention_grad_autoscale`` / DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE (on by default).  ``args.backbone_linear="hip"`` /
DDEPTH_BACKBONE_LINEAR=hip runs the Swin blocks' token Linears in the library for inference (linear.convert_hip_swin_linears: the FFNs, and
qkv / proj of the converted attention modules), at ``args.backbone_linear_precision`` / DDEPTH_BACKBONE_LINEAR_PRECISION ("bf16" by default,
"fp32", "f16").
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch
from torch import nn

from .batchnorm import HipBatchNorm2d, convert_hip_batchnorm
from .conv import conv_bn_act, conv_bn_train, convert_hip_conv
from .head import build_head
from .linear import convert_hip_swin_linears, resolve_linear_backend, resolve_linear_precision
from .swin import convert_hip_window_attention, resolve_attention_backend, resolve_attention_grad_autoscale, resolve_attention_precision


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride, first=False):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        # the reference passes a bare 3x3 conv (with bias) as the first block's downsample (mmbev_resnet.py:128-129)
        self.downsample = nn.Conv2d(cin, cout, 3, stride, 1) if first else None
        # set by fuse_basic_block_tails: both BatchNorms are batchnorm.HipBatchNorm2d carrying their ReLU, and bn2 takes the residual as its addend
        self.fused_tail = False
        # set by fold_eval_basic_blocks: in .eval() without grad the block is two or three library calls (conv.conv_bn_act), each a convolution with the
        # folded BatchNorm, the residual add and the ReLU in its epilogue
        self.folded_eval = False
        # set by fuse_conv_bn_stats: with fused_tail, in .train() each conv -> BatchNorm pair runs through conv.conv_bn_train -- the convolution's
        # epilogue emits the BatchNorm's statistics, so no pass over its output starts the BatchNorm
        self.conv_bn_stats = False

    def _forward_folded(self, x):
        """The eval-mode block in the library, or None where one of its calls is not native (nothing has been changed then)."""
        out = conv_bn_act(self.conv1, self.bn1, x, relu=True)
        if out is None:
            return None
        idt = x if self.downsample is None else conv_bn_act(self.downsample, None, x, relu=False)
        if idt is None:
            return None
        return conv_bn_act(self.conv2, self.bn2, out, addend=idt, relu=True)

    def forward(self, x):
        if self.folded_eval and not self.training and not torch.is_grad_enabled():
            out = self._forward_folded(x)
            if out is not None:
                return out
        idt = x if self.downsample is None else self.downsample(x)
        if self.fused_tail and self.conv_bn_stats and self.training:
            # (a pair that is not native -- CPU tensors, another module, an unsupported shape -- returns None untouched and runs as below)
            out = conv_bn_train(self.conv1, self.bn1, x)
            if out is None:
                out = self.bn1(self.conv1(x))
            res = conv_bn_train(self.conv2, self.bn2, out, addend=idt)
            return res if res is not None else self.bn2(self.conv2(out), addend=idt)
        if self.fused_tail:
            out = self.bn1(self.conv1(x))
            return self.bn2(self.conv2(out), addend=idt)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + idt)


class ResNetForMMBEV(nn.Module):
    """Stem-less BasicBlock stacks emitting [64,128,256,512] channels at strides 2/4/8/16
    (reference mmbev_resnet.py:101-160)."""

    def __init__(self, num_layer, in_channels=3, channels=(64, 128, 256, 512), strides=(2, 2, 2, 2)):
        super().__init__()
        layers = []
        cin = in_channels
        for n, c, s in zip(num_layer, channels, strides):
            blocks = [_BasicBlock(cin, c, s, first=True)] + [_BasicBlock(c, c, 1) for _ in range(n - 1)]
            layers.append(nn.Sequential(*blocks))
            cin = c
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        feats = []
        for layer in self.layers:
            x = layer(x)
            feats.append(x)
        return feats


BACKBONES = {                                       # reference mmbev_resnet.py:176-194
    "mmbev_res18": lambda: ResNetForMMBEV([2, 2, 2, 2]),
    "mmbev_res50": lambda: ResNetForMMBEV([3, 4, 6, 3]),      # BasicBlock [3,4,6,3]: the ResNet-34 layout
    "mmbev_res101": lambda: ResNetForMMBEV([3, 4, 23, 3]),
}


def default_args(**over):
    """The subset of reference src/config.py flags the model reads."""
    a = dict(backbone_module="mmbev_resnet", backbone_name="mmbev_res50", head_specify="DDIMDepthEstimate_Res",
             inference_steps=20, num_train_timesteps=1000, model_name="Diffusion_DCbase_", precision=None)
    a.update(over)
    return SimpleNamespace(**a)


def resolve_backbone(args):
    """The reference's rule (src/model/backbone/__init__.py:5-11): ``getattr(import_module('model.backbone.' +
    args.backbone_module.lower()), args.backbone_name)`` -- a zero-argument factory.  The bundled mmbev_res* family is served from
    BACKBONES (no mmdet needed); any other name is imported from ``args.backbone_package`` (default 'model.backbone', i.e. the
    reference tree this package is dropped into: swin.py / depthformerswin.py / mpvit.py stay upstream PyTorch per the north star)."""
    from importlib import import_module
    name = args.backbone_name
    if name in BACKBONES:
        return BACKBONES[name]
    pkg = getattr(args, "backbone_package", None) or "model.backbone"
    modname = f"{pkg}.{str(args.backbone_module).lower()}"
    try:
        module = import_module(modname)
    except ImportError as e:
        raise ImportError(f"backbone {name!r}: cannot import {modname!r} ({e}); only the mmbev_res* family is bundled -- run inside the "
                          "reference tree (its src/ on sys.path), set args.backbone_package, or pass depth_backbone=<nn.Module>") from e
    return getattr(module, name)


def fuse_basic_block_tails(backbone: nn.Module) -> nn.Module:
    """Every ``_BasicBlock`` of ``backbone`` whose bn1 and bn2 are ``HipBatchNorm2d`` (after ``convert_hip_batchnorm``) runs
    ``bn1 = BatchNorm + ReLU`` and ``bn2 = ReLU(BatchNorm + identity)`` as one library call each (include/ddepth_bn_add.h): no torch add, no
    torch ReLU.  Same parameter tensors and state-dict keys; ``relu`` stays an attribute.  Blocks on other BatchNorms are left alone;
    calling it again changes nothing.  On CPU tensors, in .eval() and for other dtypes the BatchNorms take their torch path and the block
    computes what it computed."""
    for m in backbone.modules():
        if isinstance(m, _BasicBlock) and isinstance(m.bn1, HipBatchNorm2d) and isinstance(m.bn2, HipBatchNorm2d):
            m.bn1.activation = "relu"
            m.bn2.activation = "relu"
            m.bn2.add_mode = "pre"
            m.fused_tail = True
    return backbone


def fold_eval_basic_blocks(backbone: nn.Module) -> nn.Module:
    """Marks every ``_BasicBlock`` of ``backbone`` ``folded_eval``: in .eval() with grad disabled, on tensors and modules the library takes
    (``HipConv2d`` convolutions after ``convert_hip_conv(..., channels="any", strided=True)``, BatchNorms with running statistics, contiguous fp32
    HIP tensors), the block runs as two or three calls of include/ddepth_conv_fused.h -- no torch BatchNorm, add or ReLU.  Everywhere else
    (.train(), grad enabled, CPU tensors, a convolution or precision the operator does not run) the block computes exactly what it computed.
    Parameter tensors and state-dict keys are untouched; calling it again changes nothing."""
    for m in backbone.modules():
        if isinstance(m, _BasicBlock):
            m.folded_eval = True
    return backbone


def fuse_conv_bn_stats(backbone: nn.Module) -> nn.Module:
    """Marks every ``_BasicBlock`` of ``backbone`` ``conv_bn_stats``: in .train(), where the block has a fused tail (``fuse_basic_block_tails``),
    ``conv1 + bn1`` and ``conv2 + bn2(+ identity)`` run through conv.conv_bn_train -- the convolutions of include/ddepth_conv_stats.h, whose
    epilogues emit the BatchNorms' statistics, so that neither BatchNorm starts with a pass over its input.  A pair that is not native (CPU
    tensors, a convolution or BatchNorm that is not the library's, an unsupported shape or precision) and everything in .eval() run exactly
    what they ran.  The ``downsample`` convolution has no BatchNorm and is not touched.  Parameter tensors and state-dict keys are untouched;
    calling it again changes nothing."""
    for m in backbone.modules():
        if isinstance(m, _BasicBlock):
            m.conv_bn_stats = True
    return backbone


BACKBONE_BACKENDS = ("torch", "hip", "hip+bn", "hip+fold", "hip+stats")
BACKBONE_PRECISIONS = ("bf16", "f16", "f16x3")


def resolve_backbone_backend(backbone_backend=None) -> str:
    """``args.backbone_backend`` / the environment variable DDEPTH_BACKBONE_BACKEND: "torch" (default; empty or absent), "hip" (the backbone's
    convolutions run in the library, the stride-2 openings of every stage included), "hip+bn" ("hip", and at every precision the backbone's
    BatchNorms run in the library with each BasicBlock's ReLUs and residual add fused: convert_hip_batchnorm + fuse_basic_block_tails) or
    "hip+fold" ("hip+bn", and in .eval() without grad every BasicBlock runs its convolutions with BatchNorm, residual add and ReLU folded into
    their epilogues: fold_eval_basic_blocks -- one value for training and inference) or "hip+stats" ("hip+fold", and in .train() every
    convolution of a BasicBlock that a BatchNorm follows emits that BatchNorm's statistics from its epilogue: fuse_conv_bn_stats)."""
    choice = backbone_backend or os.environ.get("DDEPTH_BACKBONE_BACKEND") or "torch"
    if choice not in BACKBONE_BACKENDS:
        raise ValueError(f"backbone_backend must be one of {list(BACKBONE_BACKENDS)} (got {choice!r})")
    return choice


def resolve_backbone_precision(backbone_precision=None):
    """``args.backbone_precision`` / the environment variable DDEPTH_BACKBONE_PRECISION: "bf16", "f16" or "f16x3" -- the operand precision of the
    backbone's library convolutions, whatever the head's (a fast-profile "f16r" head can run an "f16x3" or "bf16" backbone) -- or None (empty or
    absent: the backbone takes the head's precision, and is converted only where the library runs that one)."""
    choice = backbone_precision or os.environ.get("DDEPTH_BACKBONE_PRECISION") or None
    if choice is not None and choice not in BACKBONE_PRECISIONS:
        raise ValueError(f"backbone_precision must be one of {list(BACKBONE_PRECISIONS)} (got {choice!r})")
    return choice


class Diffusion_DCbase_Model(nn.Module):
    def __init__(self, args=None, depth_backbone=None, depth_head=None, **kwargs):
        """As the reference (diffusion_dcbase_model.py:28-91): ``depth_backbone`` / ``depth_head`` may be injected as built modules;
        otherwise the backbone is resolved from args.backbone_module / args.backbone_name and the head from args.head_specify.  The
        head classes fix their own pyramid widths (the reference passes in_channels=[64,128,256,512] to every head and each head
        overrides it, ...res.py:31, ...res_swin_add.py:31), so any backbone emitting that head's 4 maps composes."""
        super().__init__()
        self.args = args if args is not None else default_args()
        self.depth_backbone = depth_backbone if depth_backbone is not None else resolve_backbone(self.args)()
        if depth_head is not None:
            self.depth_head = depth_head
        else:
            self.depth_head = build_head(dict(type=self.args.head_specify, in_channels=[64, 128, 256, 512],
                                              inference_steps=getattr(self.args, "inference_steps", 20),
                                              num_train_timesteps=getattr(self.args, "num_train_timesteps", 1000), depth_feature_dim=16,
                                              loss_cfgs=[], init_cfg=None, precision=getattr(self.args, "precision", None)))
        # Opt-in: the (resolved or injected) backbone's convolutions in the library -- 3x3 s1 through dd_convx_*, the 3x3 s2 openings of every
        # stage (conv1, the biased downsample, the RGB one included) through dd_conv3x3s2_*.  Same parameter tensors, same state-dict keys.  With
        # a precision the library does not run (fp32, f16r, None) nothing is converted, as in the heads.  "hip+bn" adds the backbone's BatchNorms
        # (below); with "hip" they stay torch modules.
        self.backbone_backend = resolve_backbone_backend(getattr(self.args, "backbone_backend", None))
        # args.backbone_precision / DDEPTH_BACKBONE_PRECISION gives the backbone a precision of its own; absent, it takes the head's.
        self.backbone_precision = resolve_backbone_precision(getattr(self.args, "backbone_precision", None))
        if self.backbone_backend != "torch":
            precision = self.backbone_precision
            if precision is None:
                precision = getattr(self.args, "precision", None)
            if precision is None:      # (the head resolved its own: profile / DDEPTH_PRECISION)
                precision = getattr(getattr(self.depth_head, "model", None), "precision", None)
            self.depth_backbone = convert_hip_conv(self.depth_backbone, precision, channels="any", strided=True,
                                                   grad_autoscale=bool(getattr(self.depth_head, "conv_grad_autoscale", False)))
        if self.backbone_backend in ("hip+bn", "hip+fold", "hip+stats"):
            # BatchNorm is fp32 whatever the convolutions' precision: every BatchNorm of the backbone in the library, and in the bundled BasicBlock
            # stacks the two ReLUs and the residual add of each block inside those calls
            self.depth_backbone = fuse_basic_block_tails(convert_hip_batchnorm(self.depth_backbone))
        if self.backbone_backend in ("hip+fold", "hip+stats"):
            # ... and in .eval() without grad each block's BatchNorms, add and ReLUs inside its convolutions' epilogues (include/ddepth_conv_fused.h)
            self.depth_backbone = fold_eval_basic_blocks(self.depth_backbone)
        if self.backbone_backend == "hip+stats":
            # ... and in .train() the BatchNorms' statistics out of the convolutions' epilogues (include/ddepth_conv_stats.h)
            self.depth_backbone = fuse_conv_bn_stats(self.depth_backbone)
        # Opt-in, independent of backbone_backend: the shifted-window attentions of a Swin backbone in the library (include/ddepth_swin.h) for
        # inference.  Same parameter tensors, same state-dict keys; training and anything that needs a gradient keep the torch sequence, unless
        # "hip+train" asks for the library's backward (include/train/ddepth_swin_backward.h) as well.
        self.backbone_attention = resolve_attention_backend(getattr(self.args, "backbone_attention", None))
        self.backbone_attention_precision = resolve_attention_precision(getattr(self.args, "backbone_attention_precision", None))
        self.backbone_attention_grad_autoscale = resolve_attention_grad_autoscale(getattr(self.args, "backbone_attention_grad_autoscale", None))
        if self.backbone_attention in ("hip", "hip+train"):
            self.depth_backbone = convert_hip_window_attention(self.depth_backbone, self.backbone_attention_precision,
                                                               backward="hip" if self.backbone_attention == "hip+train" else "torch",
                                                               grad_autoscale=self.backbone_attention_grad_autoscale)
        # Opt-in, after the attention conversion: the token Linears of a Swin backbone in the library (include/swin/ddepth_linear.h) for inference --
        # every duck-typed FFN (fc1 + GELU, fc2 + residual) and, in the attention modules converted above, qkv and proj.  With
        # backbone_attention="torch" only the FFNs convert: the attention's Linears need the library attention module.
        self.backbone_linear = resolve_linear_backend(getattr(self.args, "backbone_linear", None))
        self.backbone_linear_precision = resolve_linear_precision(getattr(self.args, "backbone_linear_precision", None))
        if self.backbone_linear == "hip":
            self.depth_backbone = convert_hip_swin_linears(self.depth_backbone, self.backbone_linear_precision)

    def extract_depth(self, img, depth_map, depth_mask, gt_depth_map=None, return_loss=False, **kw):
        fp = self.depth_backbone(img)                                                   # :125
        return self.depth_head(fp, depth_map, depth_mask, gt_depth_map=gt_depth_map, return_loss=return_loss, image=img, **kw)

    def forward(self, sample):
        """sample keys rgb (B,3,H,W), gt (B,1,H,W), dep, depth_map, depth_mask (reference :186-224)."""
        rgb, gt = sample["rgb"], sample["gt"]
        depth_map = sample.get("depth_map", sample.get("dep"))
        depth_mask = sample.get("depth_mask")
        return self.extract_depth(rgb, depth_map, depth_mask, gt_depth_map=gt, return_loss=self.training,
                                  sparse_depth=sample.get("dep"))
