#!/usr/bin/env python3
"""Forward + backward time of the ten BatchNorm sites of a Res head at KITTI size (B = 4) on the MI355X, three ways in one process:

    (a) nn.BatchNorm2d + activation                                   (MIOpen: what a single rank runs today)
    (b) dist.SyncBatchNorm + activation, force_sync on a one-rank group (the torch composition a data-parallel rank runs today)
    (c) batchnorm.HipBatchNorm2d with the activation fused             (csrc/dd_bn.hip), without a group and exchanging like (b)

    python tools/bn_timing.py [--out FILE] [--windows 7] [--sites lateral0,dec]      # table, then one JSON object on the last line

Method: every variant of a site is warmed up; a timed window is CALLS forward + backward passes between two device events; inside one repeat the
variants are timed one after another (so drift hits all alike), and the median over the repeats is reported with min and max.  The four kernels
of (c) are also timed one by one (windows of back-to-back calls of one library call; the two reductions include their small combine launch) and
set against the bytes the algorithm needs -- 4n stats, 8n apply, 8n backward reduce, 12n backward apply for n fp32 values -- over the 8 TB/s HBM
peak.  A measurement path that finds no GPU fails.

The whole training step is a command pair, not part of this tool (bench.py decides how a step is measured):
    python bench.py --mode train-dp --variant res --batch 4
    DDEPTH_BN_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # before torch: as bench.py and the tests do

import torch
import torch.distributed as dist
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffusiondepth_amd import batchnorm as BN  # noqa: E402
from diffusiondepth_amd import dist as ddist  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
B, H, W = 4, 352, 1216     # KITTI crop; the pyramid is at strides 2 / 4 / 8 / 16
KERNEL_BYTES_PER_VALUE = {"stats": 4, "apply": 8, "backward_reduce": 8, "backward_apply": 12}
STEP_COMMANDS = ["python bench.py --mode train-dp --variant res --batch 4",
                 "DDEPTH_BN_BACKEND=hip python bench.py --mode train-dp --variant res --batch 4"]


def sites():
    """(name, C, h, w, activation, slope): conv_lateral.0-3, conv_up.0-2 (each writes the level above its input), the two encoder BatchNorms and
    the decoder's."""
    lv = [(H // 2 ** (i + 1), W // 2 ** (i + 1)) for i in range(4)]
    out = [(f"lateral{i}", 256, h, w, "relu", 0.0) for i, (h, w) in enumerate(lv)]
    out += [(f"up{i}", 256, lv[i][0], lv[i][1], "relu", 0.0) for i in range(3)]
    out += [("enc0", 16, lv[0][0], lv[0][1], "leaky_relu", 0.2), ("enc1", 16, lv[0][0], lv[0][1], None, 0.0), ("dec", 16, H, W, "relu", 0.0)]
    return out


def activation(act, slope):
    return nn.ReLU(True) if act == "relu" else nn.LeakyReLU(slope, inplace=True) if act == "leaky_relu" else nn.Identity()


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
    ap.add_argument("--sites", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bn_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.windows < 5:
        sys.exit("bn_timing: at least five windows")
    torch.cuda.set_device(0)
    if not dist.is_initialized():      # the one-rank RCCL group of (b) and of (c)'s exchanging mode
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(s.getsockname()[1])
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    want = set(filter(None, args.sites.split(",")))
    rows = []
    for name, C, h, w, act, slope in sites():
        if want and name not in want:
            continue
        n = B * C * h * w
        x = torch.randn(B, C, h, w, device="cuda").requires_grad_(True)
        gy = torch.randn(B, C, h, w, device="cuda")
        mods = {
            "a_bn2d": nn.Sequential(nn.BatchNorm2d(C), activation(act, slope)),
            "b_syncbn": nn.Sequential(ddist.SyncBatchNorm(C), activation(act, slope)),
            "c_hip": BN.HipBatchNorm2d(C, activation=act, negative_slope=slope),
            "c_hip_sync": BN.HipBatchNorm2d(C, activation=act, negative_slope=slope),
        }
        forced = {"b_syncbn": mods["b_syncbn"][0], "c_hip_sync": mods["c_hip_sync"]}
        for m in mods.values():
            m.cuda().train()

        def step(key):
            for k, m in forced.items():      # an instance attribute shadows the class-wide switch: only the variant under the clock exchanges
                m.force_sync = k == key
            x.grad = None
            mods[key](x).backward(gy)

        calls = max(2, min(20, int(2e8 // n)))
        for key in mods:
            for _ in range(2):
                step(key)
        torch.cuda.synchronize()
        times = {k: [] for k in mods}
        for _ in range(args.windows):
            for key in mods:
                times[key].append(window(lambda: step(key), calls))
        # the four kernels of (c), one library call per window
        xd, w_, b_ = x.detach(), mods["c_hip"].weight.detach(), mods["c_hip"].bias.detach()
        a_id = BN.ACTIVATIONS[act]
        sums = BN.bn_stats(xd)
        mi = BN.bn_finalize(sums, 1e-5)
        sums2 = BN.bn_backward_reduce(xd, gy, mi, w_, b_, a_id, slope)
        kern = {"stats": lambda: BN.bn_stats(xd), "apply": lambda: BN.bn_apply(xd, mi, w_, b_, a_id, slope),
                "backward_reduce": lambda: BN.bn_backward_reduce(xd, gy, mi, w_, b_, a_id, slope),
                "backward_apply": lambda: BN.bn_backward_apply(xd, gy, mi, sums2, sums, w_, b_, a_id, slope)}
        ktimes = {k: [] for k in kern}
        for fn in kern.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(args.windows):
            for k, fn in kern.items():
                ktimes[k].append(window(fn, calls))
        row = {"site": name, "shape": [B, C, h, w], "activation": act, "calls_per_window": calls, "windows": args.windows,
               "fwd_bwd": {k: spread(v) for k, v in times.items()}, "kernels": {}}
        for k, v in ktimes.items():
            s = spread(v)
            s["bytes"] = KERNEL_BYTES_PER_VALUE[k] * n
            s["hbm_share"] = s["bytes"] / (s["median_ms"] * 1e-3) / HBM_PEAK
            row["kernels"][k] = s
        rows.append(row)
        f = row["fwd_bwd"]
        print(f"{name:9s} {str((B, C, h, w)):22s} fwd+bwd ms  (a) {f['a_bn2d']['median_ms']:8.3f} [{f['a_bn2d']['min_ms']:.3f}..{f['a_bn2d']['max_ms']:.3f}]"
              f"  (b) {f['b_syncbn']['median_ms']:8.3f} [{f['b_syncbn']['min_ms']:.3f}..{f['b_syncbn']['max_ms']:.3f}]"
              f"  (c) {f['c_hip']['median_ms']:8.3f} [{f['c_hip']['min_ms']:.3f}..{f['c_hip']['max_ms']:.3f}]"
              f"  (c, exchanging) {f['c_hip_sync']['median_ms']:8.3f} [{f['c_hip_sync']['min_ms']:.3f}..{f['c_hip_sync']['max_ms']:.3f}]", flush=True)
        print("          " + "  ".join(f"{k} {s['median_ms']:.3f} ms = {100 * s['hbm_share']:.1f} % of HBM peak" for k, s in row["kernels"].items()), flush=True)
        del x, gy, mods, forced, kern, xd, sums, mi, sums2
        torch.cuda.empty_cache()
    total = {k: sum(r["fwd_bwd"][k]["median_ms"] for r in rows) for k in ("a_bn2d", "b_syncbn", "c_hip", "c_hip_sync")}
    print("sum over the sites, ms: " + "  ".join(f"{k} {v:.3f}" for k, v in total.items()))
    print("the whole step (not run here):")
    for c in STEP_COMMANDS:
        print("    " + c)
    result = {"tool": "bn_timing", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "sites": rows, "sum_ms": total,
              "step_commands": STEP_COMMANDS}
    dist.destroy_process_group()
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
