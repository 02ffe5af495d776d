#!/usr/bin/env python3
"""What the statistics epilogue of include/ddepth_conv_stats.h costs and saves on the MI355X, per site and for a whole training step, in bf16 and
f16x3 at B = 4, KITTI (352 x 1216) and NYU (228 x 304) size, all variants alternating in one process.

Per site -- the four ``conv_lateral`` of the condition FPN (C_i -> 256, stride 1) and, per backbone stage, one stride-1 site (``conv2``, C -> C) and
one stride-2 site (``conv1`` of the opening block, C_prev -> C on the previous stage's map; stage 0 reads the RGB image):

    parent      conv.conv_forward / conv.conv_s2_forward followed by batchnorm.bn_stats(y)      (what a training conv -> BatchNorm runs today)
    fused       conv.conv_stats_forward                                                        (one call: y and sums)
    conv_only   the convolution call of `parent` alone                                         (weight pack + plain implicit GEMM)
    stats_only  batchnorm.bn_stats(y) alone                                                    (the pass the epilogue replaces)

``fused - conv_only`` is what the epilogue and the combine launch add to the convolution; ``parent - fused`` is what the site saves.  These are
call-level device times between two events (the weight pack launch is inside both convolution calls), not single-kernel times.

Whole step: forward + backward of the ``mmbev_res50`` backbone in .train() under "hip+bn" (library convolutions and BatchNorms, fused block
tails) against "hip+stats" (the same plus ``fuse_conv_bn_stats``), on the same parameters.

    python tools/conv_stats_timing.py [--out profiles/conv_stats_timing.json] [--windows 7] [--sizes kitti,nyu]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/conv_stats_timing.py --sizes kitti --sites lateral0 --no-step
        # the kernels one by one: one site per run, since sites of one stride, precision and contract share an instantiation's name

Method: that of tools/conv_timing.py -- every variant is warmed up; a timed window is CALLS calls between two device events; inside one repeat
the variants are timed one after another, and the median over the repeats is reported with min and max.  Nothing is asserted: a site where the
fused call is slower is reported as measured (``pays`` false).  A measurement path that finds no GPU fails.
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
from diffusiondepth_amd import batchnorm as BN  # noqa: E402
from diffusiondepth_amd import conv as CV  # noqa: E402
from diffusiondepth_amd import model as M  # noqa: E402

SIZES = {"kitti": (352, 1216), "nyu": (228, 304)}
WIDTHS = (64, 128, 256, 512)
PRECISIONS = ("bf16", "f16x3")
VARIANTS = ("parent", "fused", "conv_only", "stats_only")
B = 4


def sites(H, W):
    """(name, stride, Cin, Cout, input H, input W) of every timed site at image size H x W."""
    out, maps = [], []
    h, w = H, W
    for _ in WIDTHS:
        h, w = CV.strided_out(h), CV.strided_out(w)
        maps.append((h, w))
    for i, c in enumerate(WIDTHS):
        out.append((f"lateral{i}", 1, c, 256) + maps[i])
    for i, c in enumerate(WIDTHS):
        out.append((f"stage{i}.conv2", 1, c, c) + maps[i])
        out.append((f"stage{i}.conv1", 2, 3 if i == 0 else WIDTHS[i - 1], c) + ((H, W) if i == 0 else maps[i - 1]))
    return out


def time_site(name, stride, cin, cout, h, w, windows):
    g = torch.Generator().manual_seed(len(name) + cin + h)
    x = torch.randn(B, cin, h, w, generator=g).cuda()
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).cuda()
    row = {"site": name, "stride": stride, "shape": [B, cin, cout, h, w], "windows": windows}
    for prec in PRECISIONS:
        pid = CV.precision_id(prec)
        conv = (lambda: CV.conv_s2_forward(x, wt, None, pid)) if stride == 2 else (lambda: CV.conv_forward(CV.OP_CONV3X3, x, wt, pid, "any"))
        y = conv()
        calls = 20 if y.numel() < (1 << 24) else 5
        fns = {"parent": lambda: BN.bn_stats(conv()), "fused": lambda: CV.conv_stats_forward(x, wt, None, stride, pid), "conv_only": conv,
               "stats_only": lambda: BN.bn_stats(y)}
        for k in VARIANTS:
            for _ in range(3):
                fns[k]()
        torch.cuda.synchronize()
        times = {k: [] for k in VARIANTS}
        for _ in range(windows):
            for k in VARIANTS:
                times[k].append(window(fns[k], calls))
        res = {k: spread(v) for k, v in times.items()}
        res["calls_per_window"] = calls
        res["saved_ms"] = res["parent"]["median_ms"] - res["fused"]["median_ms"]
        res["epilogue_and_combine_ms"] = res["fused"]["median_ms"] - res["conv_only"]["median_ms"]
        res["pays"] = bool(res["fused"]["median_ms"] < res["parent"]["median_ms"])
        row[prec] = res
    return row


def time_step(H, W, windows):
    """Forward + backward of mmbev_res50 in .train(): "hip+bn" against "hip+stats", per precision, on the same parameters."""
    torch.manual_seed(0)
    sd = M.BACKBONES["mmbev_res50"]().state_dict()
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    out = {"backbone": "mmbev_res50", "shape": [B, 3, H, W], "windows": windows, "calls_per_window": 3}
    for prec in PRECISIONS:
        nets = {}
        for key in ("hip+bn", "hip+stats"):
            net = M.BACKBONES["mmbev_res50"]()
            net.load_state_dict(sd)
            net = M.fuse_basic_block_tails(BN.convert_hip_batchnorm(CV.convert_hip_conv(net, prec, channels="any", strided=True)))
            if key == "hip+stats":
                net = M.fuse_conv_bn_stats(net)
            nets[key] = net.cuda().train()

        def step(net):
            net.zero_grad(set_to_none=True)
            sum((f ** 2).mean() for f in net(x)).backward()
        for net in nets.values():
            for _ in range(3):
                step(net)
        torch.cuda.synchronize()
        times = {k: [] for k in nets}
        for _ in range(windows):
            for k, net in nets.items():
                times[k].append(window(lambda: step(net), 3))
        res = {k: spread(v) for k, v in times.items()}
        res["saved_ms"] = res["hip+bn"]["median_ms"] - res["hip+stats"]["median_ms"]
        res["pays"] = bool(res["hip+stats"]["median_ms"] < res["hip+bn"]["median_ms"])
        out[prec] = res
        del nets
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="kitti,nyu")
    ap.add_argument("--sites", default="", help="comma-separated site names (default: all); one site, for a run under a kernel trace")
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_stats_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("conv_stats_timing: at least five windows")
    torch.cuda.set_device(0)
    rows, steps = [], []
    for size in filter(None, args.sizes.split(",")):
        H, W = SIZES[size]
        for site in sites(H, W):
            if args.sites and site[0] not in args.sites.split(","):
                continue
            row = {"size": size, **time_site(*site, args.windows)}
            rows.append(row)
            for prec in PRECISIONS:
                r = row[prec]
                print(f"{size:5s} {row['site']:14s} {str(tuple(row['shape'])):26s} {prec:5s} ms  " +
                      "  ".join(f"{k} {r[k]['median_ms']:.4f}" for k in VARIANTS) +
                      f"  saved {r['saved_ms']:+.4f}  epilogue+combine {r['epilogue_and_combine_ms']:+.4f}  pays {r['pays']}", flush=True)
            torch.cuda.empty_cache()
        if args.no_step:
            continue
        step = {"size": size, **time_step(H, W, args.windows)}
        steps.append(step)
        for prec in PRECISIONS:
            r = step[prec]
            print(f"{size:5s} mmbev_res50 training step {prec:5s} ms  hip+bn {r['hip+bn']['median_ms']:.3f} [{r['hip+bn']['min_ms']:.3f}.."
                  f"{r['hip+bn']['max_ms']:.3f}]  hip+stats {r['hip+stats']['median_ms']:.3f} [{r['hip+stats']['min_ms']:.3f}.."
                  f"{r['hip+stats']['max_ms']:.3f}]  saved {r['saved_ms']:+.3f}", flush=True)
    result = {"tool": "conv_stats_timing", "device": torch.cuda.get_device_name(0), "batch": B, "precisions": list(PRECISIONS),
              "variants": list(VARIANTS), "sites": rows, "steps": steps}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
