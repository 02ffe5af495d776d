"""Drop-in for the reference's training loss, over the C ABI of include/ddepth_eval.h.

Reference interfaces mirrored here (same names, attributes, argument order and result shapes):
  BaseLoss / Diffusion_DCbase_Loss   src/loss/__init__.py:32-58, src/loss/diffusion_dcbase_loss.py:5-49
  L1Loss, L2Loss                     src/loss/submodule/l1loss.py, l2loss.py
  SigLoss                            src/loss/submodule/sigloss.py (the scale-invariant log loss of AdaBins)
so a reference checkout switches over with ``from diffusiondepth_amd.loss import Diffusion_DCbase_Loss``.

``--loss 1.0*L1+1.0*L2+1.0*DDIM`` (the default, src/config.py:147) costs ONE fused forward pass over pred and gt for L1 and L2 together and ONE
elementwise backward pass (csrc/dd_eval.hip through ``SupervisedLossFunction``) where the reference runs two chains of about ten torch ops
each, forward and again backward.  HIP tensors go through the library; tensors that are not on a HIP device run the eager torch composition
below (the package's usual "plumbing, no GPU" rule).  DDIM and BIN only read what the head already computed; Sig stays a torch composition.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import metric as _m

T_VALID = 0.0001
SUPERVISED = ("L1", "L2")
KNOWN = ("L1", "L2", "Sig", "DDIM", "BIN")


class SupervisedLossFunction(Function):
    """(pred, gt) -> tensor [L1, L2] of the reference's L1Loss and L2Loss, one kernel pass each way (dd_sup_loss_forward / _backward).
    The upstream gradient reaches the backward kernel as a device pointer; nothing is read on the host."""

    @staticmethod
    def forward(ctx, pred, gt, max_depth, t_valid, reduce):
        p, g = _m._pair(pred, gt)
        B, H, W = _m._image_shape(p)
        loss = torch.empty(2, dtype=torch.float32, device=p.device)
        sums = torch.empty((B, 3), dtype=torch.float64, device=p.device)
        with torch.cuda.device(p.device):
            ws = _m.workspace_for(p, B, H, W)
            _m._ck(_m._lib().dd_sup_loss_forward(p.data_ptr(), g.data_ptr(), loss.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W,
                                                 float(max_depth), float(t_valid), int(reduce), _m._stream(p)), "dd_sup_loss_forward")
        ctx.save_for_backward(p, g, sums)
        ctx.geom = (B, H, W, float(max_depth), float(t_valid), pred.shape, pred.dtype)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        p, g, sums = ctx.saved_tensors
        B, H, W, max_depth, t_valid, shape, dtype = ctx.geom
        go = grad_loss.detach().float().contiguous()
        grad = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _m._ck(_m._lib().dd_sup_loss_backward(p.data_ptr(), g.data_ptr(), sums.data_ptr(), go.data_ptr(), go.data_ptr() + 4, grad.data_ptr(),
                                                  B, H, W, max_depth, t_valid, _m._stream(p)), "dd_sup_loss_backward")
        return grad.view(shape).to(dtype), None, None, None, None


def eager_supervised_loss(pred: torch.Tensor, gt: torch.Tensor, max_depth: float, t_valid: float = T_VALID) -> torch.Tensor:
    """[L1, L2] as a torch composition (differentiable by autograd): clamp both to [0, max_depth], mask = gt > t_valid multiplied in, per image
    sum / (count + 1e-8), summed over the batch."""
    g = torch.clamp(gt, min=0, max=max_depth)
    p = torch.clamp(pred, min=0, max=max_depth)
    mask = (g > t_valid).type_as(p).detach()
    dims = list(range(1, p.dim()))
    den = torch.sum(mask, dim=dims) + 1e-8
    d = p - g
    l1 = (torch.sum(torch.abs(d) * mask, dim=dims) / den).sum()
    l2 = (torch.sum(torch.pow(d, 2) * mask, dim=dims) / den).sum()
    return torch.stack([l1, l2])


def supervised_loss(pred: torch.Tensor, gt: torch.Tensor, max_depth: float, t_valid: float = T_VALID, reduce: int = _m.REDUCE_DEFAULT) -> torch.Tensor:
    """Tensor [L1, L2]: the library for HIP tensors, the eager composition otherwise."""
    if pred.is_cuda:
        return SupervisedLossFunction.apply(pred, gt, max_depth, t_valid, reduce)
    return eager_supervised_loss(pred, gt, max_depth, t_valid)


class _Supervised(nn.Module):
    def __init__(self, args, index):
        super().__init__()
        self.args = args
        self.t_valid = T_VALID
        self.index = index

    def forward(self, pred, gt):
        return supervised_loss(pred, gt, self.args.max_depth, self.t_valid)[self.index]


class L1Loss(_Supervised):
    """sum_b sum|clamp(pred) - clamp(gt)| mask / (sum mask + 1e-8)."""

    def __init__(self, args):
        super().__init__(args, 0)


class L2Loss(_Supervised):
    """sum_b sum (clamp(pred) - clamp(gt))^2 mask / (sum mask + 1e-8)."""

    def __init__(self, args):
        super().__init__(args, 1)


class SigLoss(nn.Module):
    """Scale-invariant log loss over the pixels with gt > 0: g = log(pred + eps) - log(gt + eps), loss_weight * sqrt(var(g) + 0.15 mean(g)^2).
    A plain torch composition (its boolean gather synchronises the host; it is not on by default)."""

    def __init__(self, args=None, valid_mask=True, loss_weight=2.0, max_depth=None, warm_up=False, warm_iter=100):
        super().__init__()
        self.valid_mask, self.loss_weight, self.max_depth = valid_mask, loss_weight, max_depth
        self.eps = 0.001
        self.warm_up, self.warm_iter, self.warm_up_counter = warm_up, warm_iter, 0

    def forward(self, depth_pred, depth_gt):
        if self.valid_mask:
            keep = depth_gt > 0
            if self.max_depth is not None:
                keep = torch.logical_and(keep, depth_gt <= self.max_depth)
            depth_pred, depth_gt = depth_pred[keep], depth_gt[keep]
        g = torch.log(depth_pred + self.eps) - torch.log(depth_gt + self.eps)
        if self.warm_up and self.warm_up_counter < self.warm_iter:
            self.warm_up_counter += 1
            return self.loss_weight * torch.sqrt(0.15 * torch.pow(torch.mean(g), 2))
        return self.loss_weight * torch.sqrt(torch.var(g) + 0.15 * torch.pow(torch.mean(g), 2))


_FUNCS = {"L1": L1Loss, "L2": L2Loss, "Sig": SigLoss}


def parse_loss(spec: str) -> "OrderedDict[str, float]":
    """``"1.0*L1+0.5*L2+1.0*DDIM"`` -> {"L1": 1.0, "L2": 0.5, "DDIM": 1.0} in the order written (a repeated name keeps its first position and
    its last weight, as the reference's dict does).  A name outside L1 / L2 / Sig / DDIM / BIN raises NotImplementedError."""
    out: "OrderedDict[str, float]" = OrderedDict()
    for item in spec.split("+"):
        weight, name = item.split("*")
        if name not in KNOWN:
            raise NotImplementedError(f"loss '{name}' in '{spec}': known names are {', '.join(KNOWN)}")
        out[name] = float(weight)
    return out


class Diffusion_DCbase_Loss:
    """``Diffusion_DCbase_Loss(args)(sample, output)`` -> (loss_sum of shape (1,), loss_val of shape (1, K + 1), detached: the K weighted terms in
    the order of ``args.loss`` and their total), as the reference's class; ``loss_name`` lists the K names and 'Total'."""

    def __init__(self, args):
        self.args = args
        self.loss_dict = OrderedDict()
        self.loss_module = nn.ModuleList()
        for name, weight in parse_loss(args.loss).items():
            func = _FUNCS[name](args) if name in _FUNCS else name      # DDIM / BIN: read from the head's output, nothing to call
            self.loss_dict[name] = {"weight": weight, "func": func}
            if isinstance(func, nn.Module):
                self.loss_module.append(func)
        self.loss_dict["Total"] = {"weight": 1.0, "func": None}
        self.loss_name = list(self.loss_dict)

    def __call__(self, sample, output):
        return self.compute(sample, output)

    def cuda(self, gpu=None):
        self.loss_module.cuda(gpu)

    def compute(self, sample, output):
        pred, gt = output["pred"], sample["gt"]
        fused = None
        loss_val = []
        for name, entry in self.loss_dict.items():
            if entry["func"] is None:
                continue
            if name in SUPERVISED:
                if fused is None:          # L1 and L2 together: one pass forward, one backward
                    fused = supervised_loss(pred, gt, self.args.max_depth, T_VALID)
                term = fused[SUPERVISED.index(name)]
            elif name == "Sig":
                term = entry["func"](pred, gt)
            elif name == "DDIM":
                term = output["ddim_loss"]
            elif name == "BIN":
                term = 0
                for value in output["bin_losses"].values():
                    term = term + value
            else:
                raise NotImplementedError(name)
            loss_val.append(entry["weight"] * term)
        loss_val = torch.stack(loss_val)
        loss_sum = torch.sum(loss_val, dim=0, keepdim=True)
        loss_val = torch.unsqueeze(torch.cat((loss_val, loss_sum)), dim=0).detach()
        return loss_sum, loss_val
