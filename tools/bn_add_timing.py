#!/usr/bin/env python3
"""Forward + backward time of a BasicBlock's tail -- relu(bn2(z) + identity) -- per stage of mmbev_res50 at KITTI and NYU size (B = 4) on the
MI355X, three ways in one process, and of the whole backbone step under the three ``backbone_backend`` values:

    (a) nn.BatchNorm2d, torch add, in-place torch ReLU                          (what "torch" and "hip" run)
    (b) batchnorm.HipBatchNorm2d without an activation, torch add, torch ReLU   (convert_hip_batchnorm alone)
    (c) batchnorm.HipBatchNorm2d with the add and the ReLU inside its kernels   (fuse_basic_block_tails; include/ddepth_bn_add.h)

    python tools/bn_add_timing.py [--out profiles/bn_add_timing.json] [--windows 7] [--sizes kitti,nyu] [--no-backbone]

Method (that of tools/bn_timing.py): every variant is warmed up; a timed window is CALLS forward + backward passes between two device events;
inside one repeat the variants are timed one after another (so drift hits all alike), and the median over the repeats is reported with min and
max.  The four kernels of (c) are also timed one by one (the two reductions include their small combine launch) and set against the bytes the
algorithm needs -- 4n stats, 12n apply_add, 16n backward_reduce_add, 12n backward_apply for n fp32 values -- over the 8 TB/s HBM peak.  The
comparison point of every figure is the torch variant measured in the same run.  A measurement path that finds no GPU fails.
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

from diffusiondepth_amd import batchnorm as BN  # noqa: E402
from diffusiondepth_amd import model as M  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
B = 4
SIZES = {"kitti": (352, 1216), "nyu": (228, 304)}
CHANNELS = (64, 128, 256, 512)
KERNEL_BYTES_PER_VALUE = {"stats": 4, "apply_add": 12, "backward_reduce_add": 16, "backward_apply": 12}
BACKENDS = ("torch", "hip", "hip+bn")


def stages(size):
    """(name, C, h, w) of the four stages: each opens with a 3x3 stride-2 convolution (padding 1)."""
    h, w = SIZES[size]
    out = []
    for i, c in enumerate(CHANNELS):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((f"stage{i + 1}", c, h, w))
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


def fmt(s):
    return f"{s['median_ms']:8.3f} [{s['min_ms']:.3f}..{s['max_ms']:.3f}]"


def time_tail(size, name, C, h, w, windows):
    n = B * C * h * w
    z = torch.randn(B, C, h, w, device="cuda").requires_grad_(True)
    idt = torch.randn(B, C, h, w, device="cuda").requires_grad_(True)
    gy = torch.randn(B, C, h, w, device="cuda")
    bn_a, bn_b, bn_c = nn.BatchNorm2d(C), BN.HipBatchNorm2d(C), BN.HipBatchNorm2d(C, activation="relu")
    bn_c.add_mode = "pre"
    for m in (bn_a, bn_b, bn_c):
        m.cuda().train()
    relu = nn.ReLU(inplace=True)
    tails = {"a_torch": lambda: relu(bn_a(z) + idt), "b_hip_unfused": lambda: relu(bn_b(z) + idt), "c_hip_fused": lambda: bn_c(z, addend=idt)}

    def step(key):
        z.grad = idt.grad = None
        tails[key]().backward(gy)

    calls = max(2, min(20, int(2e8 // n)))
    for key in tails:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {k: [] for k in tails}
    for _ in range(windows):
        for key in tails:
            times[key].append(window(lambda: step(key), calls))
    # the four kernels of (c), one library call per window
    zd, rd, w_, b_ = z.detach(), idt.detach(), bn_c.weight.detach(), bn_c.bias.detach()
    sums = BN.bn_stats(zd)
    mi = BN.bn_finalize(sums, 1e-5)
    y = BN.bn_apply_add(zd, mi, rd, w_, b_, BN.ACT_RELU, 0.0, BN.ADD_PRE)
    g, sums2 = BN.bn_backward_reduce_add(zd, gy, y, mi, BN.ACT_RELU, 0.0)
    kern = {"stats": lambda: BN.bn_stats(zd), "apply_add": lambda: BN.bn_apply_add(zd, mi, rd, w_, b_, BN.ACT_RELU, 0.0, BN.ADD_PRE),
            "backward_reduce_add": lambda: BN.bn_backward_reduce_add(zd, gy, y, mi, BN.ACT_RELU, 0.0),
            "backward_apply": lambda: BN.bn_backward_apply(zd, g, mi, sums2, sums, w_, None, BN.ACT_NONE, 0.0)}
    ktimes = {k: [] for k in kern}
    for fn in kern.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, fn in kern.items():
            ktimes[k].append(window(fn, calls))
    row = {"size": size, "site": name, "shape": [B, C, h, w], "calls_per_window": calls, "windows": windows,
           "fwd_bwd": {k: spread(v) for k, v in times.items()}, "kernels": {}}
    for k, v in ktimes.items():
        s = spread(v)
        s["bytes"] = KERNEL_BYTES_PER_VALUE[k] * n
        s["hbm_share"] = s["bytes"] / (s["median_ms"] * 1e-3) / HBM_PEAK
        row["kernels"][k] = s
    f = row["fwd_bwd"]
    print(f"{size:5s} {name:7s} {str((B, C, h, w)):20s} tail fwd+bwd ms  (a) {fmt(f['a_torch'])}  (b) {fmt(f['b_hip_unfused'])}  (c) {fmt(f['c_hip_fused'])}",
          flush=True)
    print("              " + "  ".join(f"{k} {s['median_ms']:.3f} ms = {100 * s['hbm_share']:.1f} % of HBM peak" for k, s in row["kernels"].items()),
          flush=True)
    return row


def time_backbone(size, windows, precision):
    """One forward + backward of mmbev_res50 in .train() under each backbone_backend (built through the facade, as a user gets it)."""
    h, w = SIZES[size]
    img = torch.randn(B, 3, h, w, device="cuda")
    nets = {}
    for be in BACKENDS:
        torch.manual_seed(0)
        model = M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res50", inference_steps=2, precision=precision, backbone_backend=be))
        nets[be] = model.depth_backbone.cuda().train()
        del model
    ups = None

    def step(key):
        nonlocal ups
        net = nets[key]
        for p in net.parameters():
            p.grad = None
        feats = net(img)
        if ups is None:
            ups = [torch.randn_like(f) for f in feats]
        torch.autograd.backward(feats, ups)

    for key in nets:
        for _ in range(2):
            step(key)
    torch.cuda.synchronize()
    times = {k: [] for k in nets}
    for _ in range(windows):
        for key in nets:
            times[key].append(window(lambda: step(key), 2))
    row = {"size": size, "backbone": "mmbev_res50", "batch": B, "precision": precision, "calls_per_window": 2, "windows": windows,
           "fwd_bwd": {k: spread(v) for k, v in times.items()}}
    print(f"{size:5s} mmbev_res50 step (B = {B}, convolutions {precision}) fwd+bwd ms  " + "  ".join(f"{k!r} {fmt(s)}" for k, s in row["fwd_bwd"].items()),
          flush=True)
    del nets
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="kitti,nyu")
    ap.add_argument("--precision", default="bf16", help="operand mode of the backbone's library convolutions under 'hip' and 'hip+bn'")
    ap.add_argument("--no-backbone", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bn_add_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("bn_add_timing: at least five windows")
    torch.cuda.set_device(0)
    sizes = [s for s in args.sizes.split(",") if s]
    tails, steps = [], []
    for size in sizes:
        for name, C, h, w in stages(size):
            tails.append(time_tail(size, name, C, h, w, args.windows))
            torch.cuda.empty_cache()
    if not args.no_backbone:
        for size in sizes:
            steps.append(time_backbone(size, args.windows, args.precision))
    result = {"tool": "bn_add_timing", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "tails": tails, "backbone_steps": steps}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
