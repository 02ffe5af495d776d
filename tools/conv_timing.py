#!/usr/bin/env python3
"""Forward + backward time of the seven convolution sites of the condition FPN (lateral0-3, up0-2) of a Res and of a Swin head at KITTI size
(B = 4) on the MI355X, four ways in one process:

    (a) nn.Conv2d / nn.ConvTranspose2d in fp32                    (MIOpen: what runs today)
    (b) the same under torch.autocast(bfloat16)                   (MIOpen's own 16-bit path: the fair comparator)
    (c) conv.HipConv2d / conv.HipConvTranspose2d, precision bf16  (csrc/dd_conv.hip)
    (d) the same, precision f16x3

    python tools/conv_timing.py [--out profiles/conv_timing.json] [--windows 7] [--heads res,swin] [--sites lateral0,up1]
    python tools/conv_timing.py --channels any --heads mpvit      # the MPViT-small laterals through the extended channel range (dd_convx_*)
    python tools/conv_timing.py --grad-autoscale                  # instead: each site's f16 / f16x3 backward with and without the rescale of grad_y

Method: every variant of a site is warmed up; a timed window is CALLS forward + backward passes (input and weight gradient) between two device
events; inside one repeat the variants are timed one after another (so drift hits all alike), and the median over the repeats is reported with
min and max.  The three library calls of (c) are also timed one by one (a call = its pack or reduce launch plus the MFMA kernel) and set against
both roofs: the bf16 MFMA peak from 2 * taps * Cin * Cout * B * H * W flops (taps = 9, or 4 for the transpose convolution), and the HBM peak from
the bytes the algorithm needs (each tensor of the call once, fp32).  A measurement path that finds no GPU fails.

--grad-autoscale (include/ddepth_conv_scaled.h; ``time_grad_autoscale`` below, shared with tools/neck_conv_timing.py) times, per site and for "f16"
and "f16x3", in the same windows: the two gradient calls as they are; ``conv.grad_scale`` plus the two scaled calls (what ``grad_autoscale=True``
runs); the amax pass alone; and each GEMM call against its scaled twin with a precomputed scale.  The comparison is the site's own unscaled
backward from the same run; a twin is named slower only where its median exceeds the unscaled call's by more than the larger min-max spread.

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


AUTOSCALE_PRECISIONS = ("f16", "f16x3")


def time_grad_autoscale(op, xd, wd, gy, calls, windows, extra=()):
    """{precision: {variant: spread, ...}} for one site: the backward (data + weight gradient) without and with the power-of-two rescale of
    grad_y, the amax pass (conv.grad_scale) alone, and each GEMM call beside its scaled twin (scale computed beforehand)."""
    out = {}
    for prec in AUTOSCALE_PRECISIONS:
        pid = CV.precision_id(prec)
        s0 = CV.grad_scale(gy, pid)

        def both(scale=None):
            kw = {} if scale is None else {"scale": scale}
            CV.conv_backward_data(op, gy, wd, xd.shape, pid, *extra, **kw)
            CV.conv_backward_weight(op, xd, gy, wd.shape, pid, *extra, **kw)

        fns = {"backward_unscaled": both, "backward_scaled": lambda: both(CV.grad_scale(gy, pid)), "grad_scale": lambda: CV.grad_scale(gy, pid),
               "data_unscaled": lambda: CV.conv_backward_data(op, gy, wd, xd.shape, pid, *extra),
               "data_scaled": lambda: CV.conv_backward_data(op, gy, wd, xd.shape, pid, *extra, scale=s0),
               "weight_unscaled": lambda: CV.conv_backward_weight(op, xd, gy, wd.shape, pid, *extra),
               "weight_scaled": lambda: CV.conv_backward_weight(op, xd, gy, wd.shape, pid, *extra, scale=s0)}
        for fn in fns.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(windows):
            for k, fn in fns.items():
                times[k].append(window(fn, calls))
        row = {k: spread(v) for k, v in times.items()}
        width = lambda a, b: max(row[a]["max_ms"] - row[a]["min_ms"], row[b]["max_ms"] - row[b]["min_ms"])
        row["grad_y_bytes"] = 4 * gy.numel()
        row["grad_scale_hbm_share"] = row["grad_y_bytes"] / (row["grad_scale"]["median_ms"] * 1e-3) / HBM_PEAK
        row["backward_extra_ms"] = row["backward_scaled"]["median_ms"] - row["backward_unscaled"]["median_ms"]
        for g in ("data", "weight"):      # the scaled GEMM itself against its twin, beyond the run's own spread
            row[g + "_twin_slower_beyond_spread"] = bool(row[g + "_scaled"]["median_ms"] > row[g + "_unscaled"]["median_ms"] + width(g + "_scaled", g + "_unscaled"))
        out[prec] = row
    return out


def print_grad_autoscale(label, shape, res):
    for prec, r in res.items():
        print(f"{label:18s} {str(shape):28s} {prec:5s} backward ms  unscaled {r['backward_unscaled']['median_ms']:.3f}  scaled {r['backward_scaled']['median_ms']:.3f}"
              f"  (amax pass {r['grad_scale']['median_ms']:.3f} = {100 * r['grad_scale_hbm_share']:.1f} % HBM)   data {r['data_unscaled']['median_ms']:.3f} -> "
              f"{r['data_scaled']['median_ms']:.3f}   weight {r['weight_unscaled']['median_ms']:.3f} -> {r['weight_scaled']['median_ms']:.3f}"
              + ("   TWIN SLOWER: " + ", ".join(g for g in ("data", "weight") if r[g + "_twin_slower_beyond_spread"])
                 if r["data_twin_slower_beyond_spread"] or r["weight_twin_slower_beyond_spread"] else ""), flush=True)


def main_grad_autoscale(args, extra):
    want = set(filter(None, args.sites.split(",")))
    rows = []
    for head in filter(None, args.heads.split(",")):
        for name, op, cin, cout, h, w in sites(head):
            if want and name not in want:
                continue
            if not CV.supported(op, cin, cout, "f16", args.channels):
                sys.exit(f"conv_timing: {name} {cin} -> {cout} is not supported with --channels {args.channels}")
            s = 1 if op == CV.OP_CONV3X3 else 2
            taps = 9 if op == CV.OP_CONV3X3 else 4
            xd = torch.randn(B, cin, h, w, device="cuda")
            wd = torch.randn((cout, cin, 3, 3) if op == CV.OP_CONV3X3 else (cin, cout, 2, 2), device="cuda") * 0.05
            gy = torch.randn(B, cout, s * h, s * w, device="cuda") * 2.0 ** -20      # (a training step's magnitude: unscaled, the f16 operands of grad_y are subnormals)
            calls = max(2, min(20, int(4e11 // (2.0 * taps * cin * cout * B * h * w))))
            res = time_grad_autoscale(op, xd, wd, gy, calls, args.windows, extra)
            print_grad_autoscale(f"{head} {name}", (B, cin, cout, h, w), res)
            rows.append({"head": head, "site": name, "op": "conv3x3" if op == CV.OP_CONV3X3 else "deconv2x2", "shape": [B, cin, cout, h, w],
                         "calls_per_window": calls, "windows": args.windows, "grad_autoscale": res})
            del xd, wd, gy
            torch.cuda.empty_cache()
    result = {"tool": "conv_timing --grad-autoscale", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "channels": args.channels,
              "sites": rows}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--grad-autoscale", action="store_true", help="time each site's f16 / f16x3 backward with and without the rescale of grad_y instead")
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
    if args.grad_autoscale:
        return main_grad_autoscale(args, extra)
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
