#!/usr/bin/env python3
"""Per-call time of the depth metric and of the supervised loss (forward + backward) on the MI355X: the library path (csrc/dd_eval.hip, both ways of
combining the workgroup partials) against this package's own eager torch path on the same tensors, in the same process.

    python tools/eval_timing.py                       # per-call table + the 200-image eval loop; one JSON object on the last line
    python tools/eval_timing.py --out FILE            # ... also written to FILE
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/eval_timing.py --kernels-only      # kernel times, a run of its own (tracing slows the host)
    python tools/eval_timing.py --trace-csv DIR/.../*_kernel_trace.csv                          # ... kernel time per shape -> achieved bytes/s over the HBM peak

Method: every shape is warmed up; a timed window is CALLS back-to-back calls between two device events (one call is microseconds: a one-call window
would measure the clock); inside one repeat the versions are timed one after another, and the repeats give the spread (min / median / max).
The eval loop is wall time ending in a device synchronise: IMAGES forwards of the Res head in the fast profile at KITTI size, B = 1, each followed by
``MetricAccumulator.update`` -- with the eager metric and with the library's, alternating.

Bytes are counted from shapes: the metric reads pred and gt once (8 B per pixel); the loss forward the same; the loss backward reads both and writes
grad_pred (12 B per pixel).  A measurement path that finds no GPU fails."""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys
import time
import types

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # before torch: as bench.py and the tests do

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import diffusiondepth_amd as dda  # noqa: E402
from diffusiondepth_amd import loss as L  # noqa: E402
from diffusiondepth_amd import metric as M  # noqa: E402
from diffusiondepth_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
SHAPES = [("kitti_b1", 1, 352, 1216, 0.16, 88.0), ("kitti_b4", 4, 352, 1216, 0.16, 88.0), ("nyu_b1", 1, 228, 304, 1.0, 10.0)]
KERNEL_BYTES_PER_PIXEL = {"dd_metric_sums_kernel": 8, "dd_sup_loss_sums_kernel": 8, "dd_sup_loss_backward_kernel": 12}


def make(B, H, W, valid, max_depth, seed=0):
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.5, 0.9 * max_depth, size=(B, 1, H, W))
    gt = np.where(rs.uniform(size=depth.shape) < valid, depth, 0.0).astype(np.float32)
    pred = (depth * np.exp(0.3 * rs.standard_normal(depth.shape))).astype(np.float32)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()


class EagerMetric(M.Diffusion_DCbase_Metric):
    """The package's eager torch path, forced for HIP tensors too (what a run without the library's kernels would execute)."""

    def sums(self, sample, output):
        return M.eager_metric_sums(output["pred"], sample["gt"], self.t_valid)

    def finalize(self, sums):
        return M.eager_metrics_from_sums(sums)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def per_call(calls, repeats):
    rows = []
    for name, B, H, W, valid, max_depth in SHAPES:
        pred, gt = make(B, H, W, valid, max_depth)
        sample, output = {"gt": gt}, {"pred": pred}
        eager, hip = EagerMetric(), M.Diffusion_DCbase_Metric()
        go = torch.tensor([1.0, 1.0], device="cuda")

        def metric_hip(mode):
            return lambda: M.metrics_from_sums(M.metric_sums(pred, gt, 1e-4, reduce=mode))

        def loss_hip(mode):
            def f():
                p = pred.detach().requires_grad_(True)
                torch.autograd.grad(L.supervised_loss(p, gt, max_depth, reduce=mode), p, go)
            return f

        def loss_eager():
            p = pred.detach().requires_grad_(True)
            torch.autograd.grad(L.eager_supervised_loss(p, gt, max_depth), p, go)

        arms = {"metric": {"eager": lambda: eager.evaluate(sample, output), "hip_default": lambda: hip.evaluate(sample, output),
                           "hip_two_launch": metric_hip(M.REDUCE_TWO_LAUNCH), "hip_ticket": metric_hip(M.REDUCE_TICKET)},
                "loss_fwd_bwd": {"eager": loss_eager, "hip_default": loss_hip(M.REDUCE_DEFAULT),
                                 "hip_two_launch": loss_hip(M.REDUCE_TWO_LAUNCH), "hip_ticket": loss_hip(M.REDUCE_TICKET)}}
        for what, versions in arms.items():
            for fn in versions.values():          # warm up every version of every shape
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in versions}
            for _ in range(repeats):              # the versions alternate inside a repeat
                for k, fn in versions.items():
                    times[k].append(window(fn, calls))
            row = {"shape": name, "B": B, "H": H, "W": W, "what": what, "calls_per_window": calls, "repeats": repeats,
                   "us_per_call": {k: spread(v) for k, v in times.items()}}
            e = row["us_per_call"]["eager"]["median"]
            row["eager_over_hip"] = {k: e / v["median"] for k, v in row["us_per_call"].items() if k != "eager"}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def eval_loop(images, repeats):
    B, H, W = 1, 352, 1216
    sd = synth.make_state_dict(7240, "res", 0.05, 0.0)
    sd.update(synth.make_fpn_state_dict(7241))
    head = dda.DDIMDepthEstimate_Res(in_channels=[64, 128, 256, 512], inference_steps=20, num_train_timesteps=1000, depth_feature_dim=16,
                                     loss_cfgs=[], profile="fast").eval()
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    head = head.cuda()
    fp = [torch.from_numpy(f).cuda() for f in synth.make_backbone_features(11, B, H, W)]
    gt = torch.from_numpy(synth.make_gt_depth(12, B, H, W)).cuda()
    sample = {"gt": gt}

    def loop(metric, n):
        acc = M.MetricAccumulator(metric) if metric is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(n):
                out = head(fp, gt, gt > 0, gt_depth_map=gt, return_loss=False)
                if acc is not None:
                    acc.update(sample, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, (acc.result() if acc is not None else None)

    arms = {"no_metric": None, "eager": EagerMetric(), "hip": M.Diffusion_DCbase_Metric()}
    for m in arms.values():
        loop(m, 10)
    times = {k: [] for k in arms}
    res = {}
    for _ in range(repeats):
        for k, m in arms.items():
            dt, r = loop(m, images)
            times[k].append(dt * 1e3)
            res[k] = r
    row = {"what": "eval_loop", "head": "DDIMDepthEstimate_Res fast profile", "images": images, "B": B, "H": H, "W": W, "repeats": repeats,
           "wall_ms": {k: spread(v) for k, v in times.items()},
           "exact_rmse_mae": {k: [float(r["exact"][0]), float(r["exact"][1])] for k, r in res.items() if r is not None}}
    row["eager_over_hip"] = row["wall_ms"]["eager"]["median"] / row["wall_ms"]["hip"]["median"]
    row["metric_ms_per_image"] = {k: (row["wall_ms"][k]["median"] - row["wall_ms"]["no_metric"]["median"]) / images for k in ("eager", "hip")}
    print(json.dumps(row), flush=True)
    return row


def kernels_only(calls):
    """What the rocprofv3 run executes: CALLS launches of every kernel per shape and combine step, nothing else of weight."""
    for name, B, H, W, valid, max_depth in SHAPES:
        pred, gt = make(B, H, W, valid, max_depth)
        go = torch.tensor([1.0, 1.0], device="cuda")
        for mode in (M.REDUCE_TWO_LAUNCH, M.REDUCE_TICKET):
            for _ in range(calls):
                M.metrics_from_sums(M.metric_sums(pred, gt, 1e-4, reduce=mode))
                p = pred.detach().requires_grad_(True)
                torch.autograd.grad(L.supervised_loss(p, gt, max_depth, reduce=mode), p, go)
        torch.cuda.synchronize()
    print(json.dumps({"what": "kernels_only", "calls_per_shape_and_mode": calls, "shapes": [s[0] for s in SHAPES]}))


def trace_csv(path):
    """rocprofv3's kernel_trace.csv -> time per launch of every kernel of csrc/dd_eval.hip PER SHAPE (the shapes share kernel names; a launch's grid
    tells which shape it served: workgroups per image x images), and from the bytes the shape needs the achieved bytes/s over the HBM peak."""
    def groups(n, cap):
        return max(1, min(cap, -(-n // 4096)))
    by = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            kname = r.get("Kernel_Name", "")
            if "ddeval" not in kname:
                continue
            m = re.search(r"(dd_\w+_kernel)", kname)
            short = m.group(1) if m else kname
            wg = max(int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256), 1)
            key = (short, "ticket" if "<true>" in kname else ("two_launch" if "<false>" in kname else ""), int(r["Grid_Size_X"]) // wg, int(r.get("Grid_Size_Y") or 1))
            by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    rows = []
    for (short, mode, gx, gy), us in sorted(by.items()):
        row = {"kernel": short, "combine": mode, "workgroups_x": gx, "grid_y": gy, "launches": len(us), "us": spread(us)}
        bpp = KERNEL_BYTES_PER_PIXEL.get(short)
        for name, B, H, W, _, _ in SHAPES:
            cap = 1024 if short == "dd_sup_loss_backward_kernel" else 128
            if bpp and gx == groups(H * W, cap) and gy == B:
                row["shape"], row["bytes"] = name, bpp * B * H * W
                row["bytes_per_s"] = row["bytes"] / (row["us"]["median"] * 1e-6)
                row["frac_of_hbm_peak"] = row["bytes_per_s"] / HBM_PEAK
        rows.append(row)
        print(json.dumps(row))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace-csv")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.trace_csv:
        out = {"kernel_times": trace_csv(a.trace_csv)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("eval_timing.py measures on a HIP device; none found")
        if a.kernels_only:
            kernels_only(a.calls)
            return
        out = {"device": torch.cuda.get_device_name(0), "per_call": per_call(a.calls, a.repeats)}
        if not a.no_loop:
            out["eval_loop"] = eval_loop(a.images, a.loop_repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
