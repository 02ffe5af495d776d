#!/usr/bin/env python3
"""Forward + backward time of the eight stride-2 3x3 convolutions of the bundled ``mmbev_res50`` backbone (``conv1`` and the biased ``downsample`` of the
first block of each stage: 3 -> 64, 64 -> 128, 128 -> 256, 256 -> 512) at KITTI (352 x 1216) and NYU (228 x 304) size, B = 4, on the MI355X, four
ways in one process:

    (a) nn.Conv2d in fp32                                  (MIOpen: what runs today)
    (b) the same under torch.autocast(bfloat16)            (MIOpen's own 16-bit path: the fair comparator)
    (c) conv.HipConv2d marked ``strided``, precision bf16  (csrc/dd_conv.hip, include/ddepth_conv_strided.h)
    (d) the same, precision f16x3

and one training step of the whole backbone (forward, a fixed upstream gradient per feature map, backward) with ``backbone_backend`` "torch" and
"hip" (bf16 and f16x3; BatchNorm stays torch's in both).

    python tools/backbone_conv_timing.py [--out profiles/backbone_conv_timing.json] [--windows 7] [--sizes kitti,nyu] [--no-step]

Method: that of tools/conv_timing.py -- every variant is warmed up; a timed window is CALLS forward + backward passes between two device events;
inside one repeat the variants are timed one after another, and the median over the repeats is reported with min and max.  The input of a site
requires a gradient except the RGB image's (a backbone never asks for it).  The three library calls of (c) are also timed one by one.  Nothing
is asserted: a site where the library is slower than MIOpen is reported as it is measured (``c_not_slower_than_a_beyond_spread`` false).  A
measurement path that finds no GPU fails.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # before torch: as bench.py and the tests do

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from conv_timing import HBM_PEAK, MFMA_PEAK, spread, window  # noqa: E402
from diffusiondepth_amd import conv as CV  # noqa: E402
from diffusiondepth_amd import model as M  # noqa: E402

B = 4
SIZES = {"kitti": (352, 1216), "nyu": (228, 304)}
WIDTHS = (3, 64, 128, 256, 512)
VARIANTS = ("a_fp32", "b_autocast_bf16", "c_hip_bf16", "d_hip_f16x3")
STEP_VARIANTS = (("torch", None), ("hip_bf16", "bf16"), ("hip_f16x3", "f16x3"))


def sites(H, W):
    """(name, Cin, Cout, h, w, bias) with h, w the INPUT size of the stage."""
    out = []
    for s in range(4):
        for name, bias in (("conv1", False), ("downsample", True)):
            out.append((f"layer{s}.{name}", WIDTHS[s], WIDTHS[s + 1], H, W, bias))
        H, W = CV.strided_out(H), CV.strided_out(W)
    return out


def time_site(cin, cout, h, w, bias, windows):
    x = torch.randn(B, cin, h, w, device="cuda").requires_grad_(cin != 3)
    gy = torch.randn(B, cout, CV.strided_out(h), CV.strided_out(w), device="cuda")
    gy16 = gy.bfloat16()

    def make(prec):
        if prec is None:
            return nn.Conv2d(cin, cout, 3, 2, 1, bias=bias).cuda()
        m = CV.HipConv2d(cin, cout, 3, 2, 1, bias=bias, precision=prec).cuda()
        m.strided, m.channels = True, "any"
        if not m._native_s2(x):
            sys.exit(f"backbone_conv_timing: {cin} -> {cout} does not take the library route: it would time torch's convolution")
        return m

    mods = {"a_fp32": make(None), "b_autocast_bf16": make(None), "c_hip_bf16": make("bf16"), "d_hip_f16x3": make("f16x3")}

    def step(key):
        x.grad = None
        mods[key].zero_grad(set_to_none=True)
        if key == "b_autocast_bf16":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = mods[key](x)
            y.backward(gy16)
        else:
            mods[key](x).backward(gy)

    flops = 2.0 * 9 * cin * cout * B * gy.shape[2] * gy.shape[3]
    calls = max(2, min(20, int(4e11 // flops)))
    for key in mods:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {k: [] for k in mods}
    for _ in range(windows):
        for key in mods:
            times[key].append(window(lambda: step(key), calls))
    xd, wd, pid = x.detach(), mods["c_hip_bf16"].weight.detach(), CV.precision_id("bf16")
    bd = mods["c_hip_bf16"].bias.detach() if bias else None
    kern = {"forward": lambda: CV.conv_s2_forward(xd, wd, bd, pid),
            "backward_data": lambda: CV.conv_s2_backward_data(gy, wd, xd.shape, pid),
            "backward_weight": lambda: CV.conv_s2_backward_weight(xd, gy, wd.shape, pid, with_bias=bias)}
    nbytes = 4 * (xd.numel() + wd.numel() + gy.numel())
    ktimes = {k: [] for k in kern}
    for fn in kern.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, fn in kern.items():
            ktimes[k].append(window(fn, calls))
    row = {"shape": [B, cin, cout, h, w], "bias": bias, "calls_per_window": calls, "windows": windows, "flops_per_direction": flops,
           "data_gradient_in_fwd_bwd": cin != 3, "fwd_bwd": {k: spread(v) for k, v in times.items()}, "kernels_c": {}}
    for k, v in ktimes.items():
        sp = spread(v)
        sp["mfma_share"] = flops / (sp["median_ms"] * 1e-3) / MFMA_PEAK
        sp["hbm_share"] = nbytes / (sp["median_ms"] * 1e-3) / HBM_PEAK
        row["kernels_c"][k] = sp
    f = row["fwd_bwd"]
    for key in ("c_hip_bf16", "d_hip_f16x3"):
        a, c = f["a_fp32"], f[key]
        row[key[0] + "_not_slower_than_a_beyond_spread"] = bool(c["median_ms"] <= a["median_ms"] + max(a["max_ms"] - a["min_ms"], c["max_ms"] - c["min_ms"]))
    return row


def time_backbone_step(H, W, windows):
    """One training step of mmbev_res50 alone per STEP_VARIANTS entry, same parameters in all of them."""
    torch.manual_seed(0)
    base = M.BACKBONES["mmbev_res50"]()
    sd = base.state_dict()
    x = torch.randn(B, 3, H, W, device="cuda")
    nets, ups = {}, None
    for key, prec in STEP_VARIANTS:
        net = M.BACKBONES["mmbev_res50"]()
        net.load_state_dict(sd)
        if prec is not None:
            net = CV.convert_hip_conv(net, prec, channels="any", strided=True)
            if any(isinstance(m, nn.Conv2d) and not isinstance(m, CV.HipConv2d) for m in net.modules()):
                sys.exit("backbone_conv_timing: a convolution of the backbone was not converted")
        nets[key] = net.cuda().train()
    with torch.no_grad():
        ups = [torch.randn_like(f) for f in nets["torch"](x)]

    def step(key):
        nets[key].zero_grad(set_to_none=True)
        feats = nets[key](x)
        torch.autograd.backward(feats, ups)

    for key in nets:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {k: [] for k in nets}
    for _ in range(windows):
        for key in nets:
            times[key].append(window(lambda: step(key), 2))
    return {"backbone": "mmbev_res50", "shape": [B, 3, H, W], "calls_per_window": 2, "windows": windows, "batchnorm": "torch",
            "step": {k: spread(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="kitti,nyu")
    ap.add_argument("--no-step", action="store_true", help="skip the whole-backbone step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("backbone_conv_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("backbone_conv_timing: at least five windows")
    torch.cuda.set_device(0)
    rows, steps = [], []
    for size in filter(None, args.sizes.split(",")):
        H, W = SIZES[size]
        for name, cin, cout, h, w, bias in sites(H, W):
            row = {"size": size, "site": name, **time_site(cin, cout, h, w, bias, args.windows)}
            rows.append(row)
            f = row["fwd_bwd"]
            print(f"{size:5s} {name:18s} {str(tuple(row['shape'])):26s} fwd+bwd ms  " +
                  "  ".join(f"({k[0]}) {f[k]['median_ms']:7.3f} [{f[k]['min_ms']:.3f}..{f[k]['max_ms']:.3f}]" for k in VARIANTS), flush=True)
            print("                         " + "  ".join(f"{k} {sp['median_ms']:.3f} ms = {100 * sp['mfma_share']:.1f} % MFMA, {100 * sp['hbm_share']:.1f} % HBM"
                                                         for k, sp in row["kernels_c"].items()), flush=True)
            torch.cuda.empty_cache()
        if not args.no_step:
            st = {"size": size, **time_backbone_step(H, W, args.windows)}
            steps.append(st)
            print(f"{size:5s} mmbev_res50 step ms  " + "  ".join(f"{k} {v['median_ms']:.3f} [{v['min_ms']:.3f}..{v['max_ms']:.3f}]" for k, v in st["step"].items()),
                  flush=True)
            torch.cuda.empty_cache()
    total = {sz: {k: sum(r["fwd_bwd"][k]["median_ms"] for r in rows if r["size"] == sz) for k in VARIANTS} for sz in sorted({r["size"] for r in rows})}
    for sz, t in total.items():
        print(f"{sz}: sum over the eight sites, ms: " + "  ".join(f"{k} {v:.3f}" for k, v in t.items()))
    result = {"tool": "backbone_conv_timing", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "mfma_peak_flops_per_s": MFMA_PEAK,
              "sites": rows, "sum_ms": total, "backbone_step": steps}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
