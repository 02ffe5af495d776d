#!/usr/bin/env python3
"""Forward + backward time of the eleven convolution sites of the HAHI neck that the library covers (Swin-L widths, KITTI size, B = 4: eight 1x1 and
three 3x3; trans_fusion.2 with its 2048 input channels stays MIOpen and is not timed) on the MI355X, four ways in one process -- the protocol of
tools/conv_timing.py:

    (a) nn.Conv2d in fp32                                (MIOpen: what runs by default)
    (b) the same under torch.autocast(bfloat16)          (MIOpen's own 16-bit path: the fair comparator)
    (c) conv.HipConv2d, precision bf16                   (csrc/dd_conv.hip)
    (d) the same, precision f16x3

and one more row: the whole neck (necks.HAHIHeteroNeck, .train(), forward + backward) with default convolutions against the neck converted with
convert_hip_conv(neck, "bf16", pointwise=True).

    python tools/neck_conv_timing.py [--out profiles/neck_conv_timing.json] [--windows 7] [--sites lateral0,conv_proj] [--no-neck]
    python tools/neck_conv_timing.py --channels any      # the extended channel range (dd_convx_*): Swin-L trans_fusion.2 (2048 -> 1536) and the twelve
                                                         # neck sites of MPViT-small (128 / 216 / 288 / 288), plus the block-64 Swin-L sites again through
                                                         # channels="any" (same kernels: they should agree with the default run within its spread)
    python tools/neck_conv_timing.py --grad-autoscale    # instead: each site's f16 / f16x3 backward with and without the rescale of grad_y
                                                         # (include/ddepth_conv_scaled.h; the protocol of tools/conv_timing.py --grad-autoscale)

Method: every variant of a site is warmed up; a timed window is CALLS forward + backward passes (input and weight gradient) between two device
events; inside one repeat the variants are timed one after another (so drift hits all alike), and the median over the repeats is reported with
min and max.  The three library calls of (c) are also timed one by one (a call = its pack or reduce launch plus the MFMA kernel) and set against
both roofs: the bf16 MFMA peak from 2 * taps * Cin * Cout * B * H * W flops, and the HBM peak from the bytes the algorithm needs (each tensor of
the call once, fp32).  A measurement path that finds no GPU fails."""
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
from diffusiondepth_amd.necks import HAHIHeteroNeck  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
MFMA_PEAK = 2.5168e15      # flop/s, bf16 / f16 dense MFMA, MI355X spec
B, H, W = 4, 352, 1216     # KITTI crop
CHANS, EMBED, STRIDE0 = (192, 384, 768, 1536), 512, 4
VARIANTS = ("a_fp32", "b_autocast_bf16", "c_hip_bf16", "d_hip_f16x3")


def levels():
    return [(-(-H // (STRIDE0 * 2 ** i)), -(-W // (STRIDE0 * 2 ** i))) for i in range(4)]


def sites():
    """(name, kernel size, Cin, Cout, h, w): the neck's convolutions in forward order, without trans_fusion.2 (2048 -> 1536: not supported)."""
    lv = levels()
    out = [(f"lateral{i}", 1, c, c, *lv[i]) for i, c in enumerate(CHANS)]
    out.append(("conv_proj", 1, CHANS[0], EMBED, *lv[0]))
    out += [(f"trans_proj{j}", 1, CHANS[j + 1], EMBED, *lv[j + 1]) for j in range(3)]
    out.append(("conv_fusion", 3, CHANS[0] + EMBED, CHANS[0], *lv[0]))
    out += [(f"trans_fusion{j}", 3, CHANS[j + 1] + EMBED, CHANS[j + 1], *lv[j + 1]) for j in range(2)]
    return out


def sites_any():
    """--channels any: what only the extended range takes -- Swin-L trans_fusion.2 and the MPViT-small neck (names prefixed) -- then the block-64
    Swin-L sites once more, which run the same kernels through the other entry points."""
    lv = levels()
    out = [("swin_trans_fusion2", 3, CHANS[3] + EMBED, CHANS[3], *lv[3])]
    mp = (128, 216, 288, 288)
    out += [(f"mpvit_lateral{i}", 1, c, c, *lv[i]) for i, c in enumerate(mp)]
    out.append(("mpvit_conv_proj", 1, mp[0], EMBED, *lv[0]))
    out += [(f"mpvit_trans_proj{j}", 1, mp[j + 1], EMBED, *lv[j + 1]) for j in range(3)]
    out.append(("mpvit_conv_fusion", 3, mp[0] + EMBED, mp[0], *lv[0]))
    out += [(f"mpvit_trans_fusion{j}", 3, mp[j + 1] + EMBED, mp[j + 1], *lv[j + 1]) for j in range(3)]
    return out + sites()


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


def not_slower(c, a):
    """`c` is not slower than `a` beyond the run's own spread."""
    return bool(c["median_ms"] <= a["median_ms"] + max(a["max_ms"] - a["min_ms"], c["max_ms"] - c["min_ms"]))


def time_site(name, k, cin, cout, h, w, windows, channels="block64"):
    op = CV.OP_CONV3X3 if k == 3 else CV.OP_CONV1X1
    extra = (channels,) if channels != "block64" else ()
    if not CV.supported(op, cin, cout, "bf16", channels):
        sys.exit(f"neck_conv_timing: {name} {cin} -> {cout} is not supported with --channels {channels}: it would time torch's convolution")
    x = torch.randn(B, cin, h, w, device="cuda").requires_grad_(True)
    gy = torch.randn(B, cout, h, w, device="cuda")
    gy16 = gy.bfloat16()

    def make(prec):
        if prec is None:
            return nn.Conv2d(cin, cout, k, 1, k // 2, bias=False).cuda()
        m = CV.HipConv2d(cin, cout, k, 1, k // 2, precision=prec).cuda()
        m.channels = channels
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

    flops = 2.0 * k * k * cin * cout * B * h * w
    calls = max(2, min(20, int(4e11 // flops)))
    for key in mods:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {key: [] for key in mods}
    for _ in range(windows):
        for key in mods:
            times[key].append(window(lambda: step(key), calls))
    # the three library calls of (c), one call per window
    xd, wd, pid = x.detach(), mods["c_hip_bf16"].weight.detach(), CV.precision_id("bf16")
    kern = {"forward": lambda: CV.conv_forward(op, xd, wd, pid, *extra), "backward_data": lambda: CV.conv_backward_data(op, gy, wd, xd.shape, pid, *extra),
            "backward_weight": lambda: CV.conv_backward_weight(op, xd, gy, wd.shape, pid, *extra)}
    nbytes = 4 * (xd.numel() + wd.numel() + gy.numel())
    ktimes = {kk: [] for kk in kern}
    for fn in kern.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for kk, fn in kern.items():
            ktimes[kk].append(window(fn, calls))
    row = {"site": name, "op": "conv3x3" if k == 3 else "conv1x1", "shape": [B, cin, cout, h, w], "calls_per_window": calls, "windows": windows,
           "flops_per_direction": flops, "flops_per_input_byte": flops / (4.0 * xd.numel()), "fwd_bwd": {kk: spread(v) for kk, v in times.items()},
           "kernels_c": {}}
    for kk, v in ktimes.items():
        sp = spread(v)
        sp["mfma_share"] = flops / (sp["median_ms"] * 1e-3) / MFMA_PEAK
        sp["bytes"] = nbytes
        sp["hbm_share"] = nbytes / (sp["median_ms"] * 1e-3) / HBM_PEAK
        sp["nearer_roof"] = "mfma" if sp["mfma_share"] >= sp["hbm_share"] else "hbm"      # (the roof the call is closer to: what would bound it)
        row["kernels_c"][kk] = sp
    f = row["fwd_bwd"]
    row["c_not_slower_than_a_beyond_spread"] = not_slower(f["c_hip_bf16"], f["a_fp32"])
    row["c_not_slower_than_b_beyond_spread"] = not_slower(f["c_hip_bf16"], f["b_autocast_bf16"])
    print(f"{name:13s} {str((B, cin, cout, h, w)):28s} fwd+bwd ms  " +
          "  ".join(f"({kk[0]}) {f[kk]['median_ms']:7.3f} [{f[kk]['min_ms']:.3f}..{f[kk]['max_ms']:.3f}]" for kk in VARIANTS), flush=True)
    print("               " + "  ".join(f"{kk} {sp['median_ms']:.3f} ms = {100 * sp['mfma_share']:.1f} % MFMA, {100 * sp['hbm_share']:.1f} % HBM"
                                       for kk, sp in row["kernels_c"].items()), flush=True)
    return row


def time_neck(windows):
    """The whole neck in .train(), forward + backward: default convolutions against convert_hip_conv(neck, "bf16", pointwise=True)."""
    def build(convert):
        torch.manual_seed(0)
        neck = HAHIHeteroNeck(list(CHANS), list(CHANS), embedding_dim=EMBED, cross_att=False, self_att=False).cuda().train()
        return CV.convert_hip_conv(neck, "bf16", pointwise=True) if convert else neck

    necks = {"default": build(False), "pointwise_bf16": build(True)}
    converted = sum(isinstance(m, CV.HipConv2d) for m in necks["pointwise_bf16"].modules())
    xs = [torch.randn(B, c, h, w, device="cuda").requires_grad_(True) for c, (h, w) in zip(CHANS, levels())]
    ups = [torch.randn(B, c, h, w, device="cuda") for c, (h, w) in zip(CHANS, levels())]

    def step(key):
        for t in xs:
            t.grad = None
        necks[key].zero_grad(set_to_none=True)
        torch.autograd.backward(necks[key](xs), ups)

    for key in necks:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {key: [] for key in necks}
    for _ in range(windows):
        for key in necks:
            times[key].append(window(lambda: step(key), 2))
    row = {"site": "whole_neck", "converted_convolutions": converted, "windows": windows, "fwd_bwd": {k: spread(v) for k, v in times.items()}}
    row["converted_not_slower_beyond_spread"] = not_slower(row["fwd_bwd"]["pointwise_bf16"], row["fwd_bwd"]["default"])
    print("whole neck (train, fwd+bwd) ms  " + "  ".join(f"{k} {v['median_ms']:.3f} [{v['min_ms']:.3f}..{v['max_ms']:.3f}]" for k, v in row["fwd_bwd"].items()),
          flush=True)
    return row


def main_grad_autoscale(args):
    from conv_timing import print_grad_autoscale, time_grad_autoscale      # (tools/ is this script's directory)
    extra = (args.channels,) if args.channels != "block64" else ()
    want = set(filter(None, args.sites.split(",")))
    rows = []
    for name, k, cin, cout, h, w in (sites_any() if args.channels == "any" else sites()):
        if want and name not in want:
            continue
        op = CV.OP_CONV3X3 if k == 3 else CV.OP_CONV1X1
        if not CV.supported(op, cin, cout, "f16", args.channels):
            sys.exit(f"neck_conv_timing: {name} {cin} -> {cout} is not supported with --channels {args.channels}")
        xd = torch.randn(B, cin, h, w, device="cuda")
        wd = torch.randn(cout, cin, k, k, device="cuda") * 0.05
        gy = torch.randn(B, cout, h, w, device="cuda") * 2.0 ** -20      # (a training step's magnitude: unscaled, the f16 operands of grad_y are subnormals)
        calls = max(2, min(20, int(4e11 // (2.0 * k * k * cin * cout * B * h * w))))
        res = time_grad_autoscale(op, xd, wd, gy, calls, args.windows, extra)
        print_grad_autoscale(name, (B, cin, cout, h, w), res)
        rows.append({"site": name, "op": "conv3x3" if k == 3 else "conv1x1", "shape": [B, cin, cout, h, w], "calls_per_window": calls,
                     "windows": args.windows, "grad_autoscale": res})
        del xd, wd, gy
        torch.cuda.empty_cache()
    result = {"tool": "neck_conv_timing --grad-autoscale", "channels": args.channels, "device": torch.cuda.get_device_name(0),
              "hbm_peak_bytes_per_s": HBM_PEAK, "sites": rows}
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
    ap.add_argument("--sites", default="")
    ap.add_argument("--no-neck", action="store_true")
    ap.add_argument("--channels", default="block64", choices=CV.CHANNELS, help="the channel contract of the HipConv2d modules; 'any' times sites_any()")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neck_conv_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("neck_conv_timing: at least five windows")
    torch.cuda.set_device(0)
    if args.grad_autoscale:
        return main_grad_autoscale(args)
    want = set(filter(None, args.sites.split(",")))
    rows = []
    for site in (sites_any() if args.channels == "any" else sites()):
        if want and site[0] not in want:
            continue
        rows.append(time_site(*site, args.windows, args.channels))
        torch.cuda.empty_cache()
    total = {k: sum(r["fwd_bwd"][k]["median_ms"] for r in rows) for k in VARIANTS}
    print("sum over the sites, ms: " + "  ".join(f"{k} {v:.3f}" for k, v in total.items()))
    neck = None if (args.no_neck or args.channels == "any") else time_neck(args.windows)
    result = {"tool": "neck_conv_timing", "channels": args.channels, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "mfma_peak_flops_per_s": MFMA_PEAK,
              "sites": rows, "sum_ms": total, "whole_neck": neck}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
