#!/usr/bin/env python3
"""The .eval() forward of the bundled ``mmbev_res18`` and ``mmbev_res50`` backbones under ``torch.no_grad()`` at KITTI (352 x 1216) and NYU
(228 x 304) size, B = 1 and 4, on the MI355X, five ways in one process on the same parameters:

    (a) torch fp32                                          (MIOpen: what runs today)
    (b) the same under torch.autocast(bfloat16)             (MIOpen's own 16-bit path)
    (c) backbone_backend "hip", bf16                        (library convolutions, torch BatchNorm / add / ReLU: the un-fused path)
    (d) backbone_backend "hip+fold", bf16                   (include/ddepth_conv_fused.h: BatchNorm, add and ReLU in the convolution's epilogue)
    (e) the same, f16x3

and one block tail per stage (conv2 -> bn2 -> + identity -> ReLU of a stride-1 block, B = 4) the same five ways, and the depth difference of a
whole ``Diffusion_DCbase_Model`` forward (mmbev_res18, fast profile) with a bf16 / f16x3 folded backbone against the fp32 torch backbone on the
same weights and the same noise.

    python tools/backbone_eval_timing.py [--out profiles/backbone_eval_timing.json] [--windows 7] [--sizes kitti,nyu] [--batches 1,4]

Method: that of tools/conv_timing.py -- every variant is warmed up; a timed window is CALLS forwards between two device events; inside one
repeat the variants are timed one after another, and the median over the repeats is reported with min and max.  Nothing is asserted: where the
folded path is slower it is reported as measured (``fold_not_slower_than_*`` false).  A measurement path that finds no GPU fails.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_timing import spread, window  # noqa: E402
from diffusiondepth_amd import conv as CV  # noqa: E402
from diffusiondepth_amd import model as M  # noqa: E402
from diffusiondepth_amd.batchnorm import convert_hip_batchnorm  # noqa: E402

SIZES = {"kitti": (352, 1216), "nyu": (228, 304)}
WIDTHS = (64, 128, 256, 512)
VARIANTS = ("a_fp32", "b_autocast_bf16", "c_hip_bf16", "d_fold_bf16", "e_fold_f16x3")


def randomise_batchnorm(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.3 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return net


def variants_of(make):
    """{variant: (module on the GPU in .eval(), autocast?)}; `make()` builds the fp32 torch module with the same parameters every time."""
    def conv(prec, fold):
        net = CV.convert_hip_conv(make(), prec, channels="any", strided=True)
        if any(isinstance(m, torch.nn.Conv2d) and not isinstance(m, CV.HipConv2d) for m in net.modules()):
            sys.exit("backbone_eval_timing: a convolution was not converted: it would time torch's")
        if fold:
            net = M.fold_eval_basic_blocks(M.fuse_basic_block_tails(convert_hip_batchnorm(net)))
        return net
    nets = {"a_fp32": make(), "b_autocast_bf16": make(), "c_hip_bf16": conv("bf16", False), "d_fold_bf16": conv("bf16", True),
            "e_fold_f16x3": conv("f16x3", True)}
    return {k: v.cuda().eval() for k, v in nets.items()}


def time_variants(nets, x, windows, calls):
    def run(key):
        with torch.no_grad():
            if key == "b_autocast_bf16":
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return nets[key](x)
            return nets[key](x)
    for key in nets:
        for _ in range(3):
            run(key)
    torch.cuda.synchronize()
    times = {k: [] for k in nets}
    for _ in range(windows):
        for key in nets:
            times[key].append(window(lambda: run(key), calls))
    out = {k: spread(v) for k, v in times.items()}
    d = out["d_fold_bf16"]
    for key in ("a_fp32", "b_autocast_bf16", "c_hip_bf16"):
        o = out[key]
        out["fold_not_slower_than_" + key] = bool(d["median_ms"] <= o["median_ms"] + max(o["max_ms"] - o["min_ms"], d["max_ms"] - d["min_ms"]))
    return out


def time_backbone(name, B, H, W, windows):
    torch.manual_seed(0)
    sd = randomise_batchnorm(M.BACKBONES[name](), 1).state_dict()

    def make():
        net = M.BACKBONES[name]()
        net.load_state_dict(sd)
        return net
    x = torch.randn(B, 3, H, W, device="cuda")
    return {"backbone": name, "shape": [B, 3, H, W], "windows": windows, "calls_per_window": 3, **time_variants(variants_of(make), x, windows, 3)}


class _Tail(torch.nn.Module):
    """A stride-1 BasicBlock: timed on (x, identity = x), so conv1 + bn1 + ReLU and the tail conv2 + bn2 + add + ReLU."""

    def __init__(self, c):
        super().__init__()
        self.block = M._BasicBlock(c, c, 1)

    def forward(self, x):
        return self.block(x)


def time_block(stage, B, H, W, windows):
    c = WIDTHS[stage]
    h, w = H, W
    for _ in range(stage + 1):
        h, w = CV.strided_out(h), CV.strided_out(w)
    torch.manual_seed(stage)
    sd = randomise_batchnorm(_Tail(c), 2).state_dict()

    def make():
        net = _Tail(c)
        net.load_state_dict(sd)
        return net
    x = torch.randn(B, c, h, w, device="cuda")
    calls = 10
    return {"stage": stage, "shape": [B, c, h, w], "windows": windows, "calls_per_window": calls, **time_variants(variants_of(make), x, windows, calls)}


def depth_difference(H, W):
    """max and mean |depth| difference of the whole model (mmbev_res18, fast profile, 2 steps) with a folded backbone against the fp32 torch backbone."""
    from diffusiondepth_amd import synth
    rgb = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    gt = torch.from_numpy(synth.make_gt_depth(6, 1, H, W)).cuda()
    sample = {"rgb": rgb, "gt": gt, "dep": gt, "depth_map": gt, "depth_mask": gt > 0}
    preds, sd = {}, None
    for key, extra in (("torch", {}), ("fold_bf16", {"backbone_backend": "hip+fold", "backbone_precision": "bf16"}),
                       ("fold_f16x3", {"backbone_backend": "hip+fold", "backbone_precision": "f16x3"})):
        torch.manual_seed(0)
        model = M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, precision="f16r", **extra))
        if sd is None:
            randomise_batchnorm(model.depth_backbone, 4)
            sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(sd)
        model = model.cuda().eval()
        torch.manual_seed(7)      # the same x_T
        with torch.no_grad():
            preds[key] = model(sample)["pred"].float()
    ref = preds["torch"]
    return {"shape": [1, 3, H, W], "pred_max": float(ref.abs().max()),
            **{k: {"max_abs": float((v - ref).abs().max()), "mean_abs": float((v - ref).abs().mean())} for k, v in preds.items() if k != "torch"}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="kitti,nyu")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--backbones", default="mmbev_res18,mmbev_res50")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("backbone_eval_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("backbone_eval_timing: at least five windows")
    torch.cuda.set_device(0)
    rows, blocks = [], []
    for size in filter(None, args.sizes.split(",")):
        H, W = SIZES[size]
        for B in (int(b) for b in args.batches.split(",")):
            for name in filter(None, args.backbones.split(",")):
                row = {"size": size, **time_backbone(name, B, H, W, args.windows)}
                rows.append(row)
                print(f"{size:5s} B={B} {name:12s} eval forward ms  " +
                      "  ".join(f"({k[0]}) {row[k]['median_ms']:7.3f} [{row[k]['min_ms']:.3f}..{row[k]['max_ms']:.3f}]" for k in VARIANTS), flush=True)
                torch.cuda.empty_cache()
        for stage in range(4):
            row = {"size": size, **time_block(stage, 4, H, W, args.windows)}
            blocks.append(row)
            print(f"{size:5s} B=4 block of stage {stage} {str(tuple(row['shape'])):22s} ms  " +
                  "  ".join(f"({k[0]}) {row[k]['median_ms']:7.3f} [{row[k]['min_ms']:.3f}..{row[k]['max_ms']:.3f}]" for k in VARIANTS), flush=True)
            torch.cuda.empty_cache()
    depth = [{"size": size, **depth_difference(*SIZES[size])} for size in filter(None, args.sizes.split(","))]
    for d in depth:
        print(f"{d['size']:5s} depth difference against the fp32 torch backbone (pred max {d['pred_max']:.3f}): " +
              "  ".join(f"{k} max {d[k]['max_abs']:.3e} mean {d[k]['mean_abs']:.3e}" for k in ("fold_bf16", "fold_f16x3")), flush=True)
    result = {"tool": "backbone_eval_timing", "device": torch.cuda.get_device_name(0), "variants": list(VARIANTS), "backbones": rows, "blocks": blocks,
              "depth_difference": depth}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
