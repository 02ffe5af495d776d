#!/usr/bin/env python3
"""Forward + backward time of the seven convolution sites of the condition FPN (lateral0-3, up0-2) of a Res and of a Swin head at KITTI size
(B = 4) on the MI355X, four ways in one process:

    (a) nn.Conv2d / nn.ConvTranspose2d in fp32                    (MIOpen: what runs today)
    (b) the same under torch.autocast(bfloat16)                   (MIOpen's own 16-bit path: the fair comparator)
    (c) conv.HipConv2d / conv.HipConvTranspose2d, precision bf16  (csrc/dd_conv.hip)
    (d) the same, precision f16x3

    python tools/conv_timing.py [--out profiles/conv_timing.json] [--windows 7] [--heads res,swin] [--sites lateral0,up1]
    python tools/conv_timing.py --channels any --heads mpvit      # the MPViT-small laterals through the extended channel range (dd_convx_*)

Method: every variant of a site is warmed up; a timed window is CALLS forward + backward passes (input and weight gradient) between two device
events; inside one repeat the variants are timed one after another (so drift hits all alike), and the median over the repeats is reported with
min and max.  The three library calls of (c) are also timed one by one (a call = its pack or reduce launch plus the MFMA kernel) and set against
both roofs: the bf16 MFMA peak from 2 * taps * Cin * Cout * B * H * W flops (taps = 9, or 4 for the transpose convolution), and the HBM peak from
the bytes the algorithm needs (each tensor of the call once, fp32).  A measurement path that finds no GPU fails.

The whole training step is a command set, not part of this tool (bench.py decides how a step is measured):
    python bench.py --mode train-dp --variant res --batch 4              (also --variant swin)
    DDEPTH_CONV_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4
    DDEPTH_CONV_BACKEND=hip DDEPTH_BN_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # before torch: as bench.py and the tests do

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffusiondepth_amd import conv as CV  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
MFMA_PEAK = 2.5168e15      # flop/s, bf16 / f16 dense MFMA, MI355X spec (16 x the 157.3 TF fp32 matrix rate)
B, H, W = 4, 352, 1216     # KITTI crop
# pyramid widths, stride of the first level.  "mpvit" (MPViT-small: 216 and 288 are no multiples of 64) needs --channels any
HEADS = {"res": ((64, 128, 256, 512), 2), "swin": ((192, 384, 768, 1536), 4), "mpvit": ((128, 216, 288, 288), 4)}
STEP_COMMANDS = ["python bench.py --mode train-dp --variant res --batch 4",
                 "DDEPTH_CONV_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4",
                 "DDEPTH_CONV_BACKEND=hip DDEPTH_BN_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4"]
VARIANTS = ("a_fp32", "b_autocast_bf16", "c_hip_bf16", "d_hip_f16x3")


def sites(head):
    """(name, op, Cin, Cout, h, w) with h, w the INPUT size: conv_lateral.i reads level i, conv_up.j reads level j + 1 and writes level j."""
    chans, s0 = HEADS[head]
    lv = [(-(-H // (s0 * 2 ** i)), -(-W // (s0 * 2 ** i))) for i in range(4)]
    out = [(f"lateral{i}", CV.OP_CONV3X3, c, 256, lv[i][0], lv[i][1]) for i, c in enumerate(chans)]
    out += [(f"up{j}", CV.OP_DECONV2X2, 256, 256, lv[j + 1][0], lv[j + 1][1]) for j in range(3)]
    return out


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--heads", default="res,swin")
    ap.add_argument("--sites", default="")
    ap.add_argument("--channels", default="block64", choices=CV.CHANNELS, help="the channel contract of the HipConv* modules (conv.CHANNELS)")
    args = ap.parse_args()
    extra = (args.channels,) if args.channels != "block64" else ()
    if not torch.cuda.is_available():
        sys.exit("conv_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("conv_timing: at least five windows")
    torch.cuda.set_device(0)
    want = set(filter(None, args.sites.split(",")))
    rows = []
    for head in filter(None, args.heads.split(",")):
        for name, op, cin, cout, h, w in sites(head):
            if want and name not in want:
                continue
            s = 1 if op == CV.OP_CONV3X3 else 2
            taps = 9 if op == CV.OP_CONV3X3 else 4
            x = torch.randn(B, cin, h, w, device="cuda").requires_grad_(True)
            gy = torch.randn(B, cout, s * h, s * w, device="cuda")
            gy16 = gy.bfloat16()

            def make(prec):
                if prec is None:
                    return (nn.Conv2d(cin, cout, 3, 1, 1, bias=False) if op == CV.OP_CONV3X3 else nn.ConvTranspose2d(cin, cout, 2, 2, bias=False)).cuda()
                m = (CV.HipConv2d(cin, cout, precision=prec) if op == CV.OP_CONV3X3 else CV.HipConvTranspose2d(cin, cout, precision=prec)).cuda()
                m.channels = args.channels
                if not CV.supported(op, cin, cout, prec, args.channels):
                    sys.exit(f"conv_timing: {name} {cin} -> {cout} is not supported with --channels {args.channels}: it would time torch's convolution")
                return m

            mods = {"a_fp32": make(None), "b_autocast_bf16": make(None), "c_hip_bf16": make("bf16"), "d_hip_f16x3": make("f16x3")}

            def step(key):
                x.grad = None
                mods[key].weight.grad = None
                if key == "b_autocast_bf16":
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        y = mods[key](x)
                    y.backward(gy16)
                else:
                    mods[key](x).backward(gy)

            flops = 2.0 * taps * cin * cout * B * h * w
            calls = max(2, min(20, int(4e11 // flops)))
            for key in mods:
                for _ in range(2):
                    step(key)
            torch.cuda.synchronize()
            times = {k: [] for k in mods}
            for _ in range(args.windows):
                for key in mods:
                    times[key].append(window(lambda: step(key), calls))
            # the three library calls of (c), one call per window
            xd, wd, pid = x.detach(), mods["c_hip_bf16"].weight.detach(), CV.precision_id("bf16")
            kern = {"forward": lambda: CV.conv_forward(op, xd, wd, pid, *extra),
                    "backward_data": lambda: CV.conv_backward_data(op, gy, wd, xd.shape, pid, *extra),
                    "backward_weight": lambda: CV.conv_backward_weight(op, xd, gy, wd.shape, pid, *extra)}
            nbytes = {"forward": 4 * (xd.numel() + wd.numel() + gy.numel()), "backward_data": 4 * (xd.numel() + wd.numel() + gy.numel()),
                      "backward_weight": 4 * (xd.numel() + wd.numel() + gy.numel())}
            ktimes = {k: [] for k in kern}
            for fn in kern.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(args.windows):
                for k, fn in kern.items():
                    ktimes[k].append(window(fn, calls))
            row = {"head": head, "site": name, "op": "conv3x3" if op == CV.OP_CONV3X3 else "deconv2x2", "shape": [B, cin, cout, h, w],
                   "calls_per_window": calls, "windows": args.windows, "flops_per_direction": flops,
                   "fwd_bwd": {k: spread(v) for k, v in times.items()}, "kernels_c": {}}
            for k, v in ktimes.items():
                sp = spread(v)
                sp["mfma_share"] = flops / (sp["median_ms"] * 1e-3) / MFMA_PEAK
                sp["bytes"] = nbytes[k]
                sp["hbm_share"] = nbytes[k] / (sp["median_ms"] * 1e-3) / HBM_PEAK
                sp["nearer_roof"] = "mfma" if sp["mfma_share"] >= sp["hbm_share"] else "hbm"      # (the roof the call is closer to: what would bound it)
                row["kernels_c"][k] = sp
            f = row["fwd_bwd"]
            a, c = f["a_fp32"], f["c_hip_bf16"]
            row["c_not_slower_than_a_beyond_spread"] = bool(c["median_ms"] <= a["median_ms"] + max(a["max_ms"] - a["min_ms"], c["max_ms"] - c["min_ms"]))
            rows.append(row)
            print(f"{head:4s} {name:9s} {str((B, cin, cout, h, w)):26s} fwd+bwd ms  " +
                  "  ".join(f"({k[0]}) {f[k]['median_ms']:7.3f} [{f[k]['min_ms']:.3f}..{f[k]['max_ms']:.3f}]" for k in VARIANTS), flush=True)
            print("               " + "  ".join(f"{k} {sp['median_ms']:.3f} ms = {100 * sp['mfma_share']:.1f} % MFMA, {100 * sp['hbm_share']:.1f} % HBM"
                                               for k, sp in row["kernels_c"].items()), flush=True)
            del x, gy, gy16, mods, kern, xd, wd
            torch.cuda.empty_cache()
    total = {hd: {k: sum(r["fwd_bwd"][k]["median_ms"] for r in rows if r["head"] == hd) for k in VARIANTS} for hd in sorted({r["head"] for r in rows})}
    for hd, t in total.items():
        print(f"{hd}: sum over the sites, ms: " + "  ".join(f"{k} {v:.3f}" for k, v in t.items()))
    print("the whole step (not run here):")
    for c in STEP_COMMANDS:
        print("    " + c)
    result = {"tool": "conv_timing", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "mfma_peak_flops_per_s": MFMA_PEAK,
              "channels": args.channels, "sites": rows, "sum_ms": total, "step_commands": STEP_COMMANDS}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
