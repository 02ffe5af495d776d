#!/usr/bin/env python3
"""Time of the Swin backbone's shifted-window attention at the four Swin-L sites of a KITTI-size image (the stride-4 map is 88 x 304) on the MI355X:

    site   map        C     heads
    s1     88 x 304   192   6
    s2     44 x 152   384   12
    s3     22 x 76    768   24
    s4     11 x 38    1536  48

for B = 1 and 4 and shift 0 and 3, the whole module (``qkv`` Linear -> attention -> ``proj`` Linear) five ways in one process:

    torch_fp32   the reference's sequence in torch, fp32                      (HipShiftWindowMSA._forward_torch: what "torch" runs)
    torch_bf16   the same under torch.autocast(bfloat16)
    hip_fp32 / hip_bf16 / hip_f16   HipShiftWindowMSA, one library call between the two fp32 Linears

and the kernel alone (dd_window_attention_forward on a ready qkv tensor) at the three precisions, with its achieved bytes/s against the
operator's floor of one read of qkv and one write of out: 16 C bytes per token.

    python tools/window_attention_timing.py --out profiles/window_attention_timing.json [--windows 7] [--step-timeout 300]

``--backward`` times training instead: the module's forward + backward (input and parameters need gradients) as torch fp32, torch under bf16
autocast and ``backward="hip"`` at fp32 / bf16 / f16; the backward kernel alone (dd_window_attention_backward on ready tensors, all three
gradients) against its floor of one read of qkv and grad_out and one write of grad_qkv, 28 C bytes per token; and the peak device memory of one
module forward + backward on the torch fp32 and the hip fp32 route (torch.cuda.max_memory_allocated above what is allocated before the step).

    python tools/window_attention_timing.py --backward --out profiles/window_attention_backward_timing.json

Method: the parent process never opens the GPU; every (site, batch) is a child process of this file (``--site``) under its own time limit, one at
a time, and the first child that fails ends the run.  In a child every variant is warmed up, a timed window is CALLS calls between two device
events, inside one repeat the variants are timed one after another (so drift hits all alike), and the median over the windows is reported with
min and max.  A measurement path that finds no GPU fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # before torch: as bench.py and the tests do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec
SITES = {"s1": (88, 304, 192, 6), "s2": (44, 152, 384, 12), "s3": (22, 76, 768, 24), "s4": (11, 38, 1536, 48)}
BATCHES = (1, 4)
SHIFTS = (0, 3)


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def time_site(site, B, windows):
    import torch

    from diffusiondepth_amd import swin as SW
    if not torch.cuda.is_available():
        sys.exit("window_attention_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    torch.cuda.set_device(0)
    H, W, C, heads = SITES[site]
    tokens = B * H * W
    rows = []

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    for shift in SHIFTS:
        torch.manual_seed(0)
        mods = {p: SW.HipShiftWindowMSA(C, heads, 7, shift_size=shift, precision=p) for p in SW.PRECISIONS}
        mods["fp32"].w_msa.init_weights()
        for m in mods.values():
            m.load_state_dict(mods["fp32"].state_dict())
            for p in m.parameters():
                p.requires_grad_(False)
            m.cuda().eval()
        ref = mods["fp32"]
        x = torch.randn(B, H * W, C, device="cuda")
        qkv = ref.w_msa.qkv(x).view(B, H, W, 3 * C).contiguous()
        bias, pad = ref._dense_bias(), ref.w_msa.qkv.bias

        def autocast():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return ref._forward_torch(x, H, W)

        variants = {"torch_fp32": lambda: ref._forward_torch(x, H, W), "torch_bf16": autocast}
        variants.update({f"hip_{p}": (lambda m=m: m(x, (H, W))) for p, m in mods.items()})
        kernels = {p: (lambda p=p: SW.window_attention_forward(qkv, pad, bias, heads, 7, shift, p)) for p in SW.PRECISIONS}
        calls = max(5, min(200, int(4e6 // tokens)))
        with torch.no_grad():
            want = variants["torch_fp32"]()
            diff = {k: float((fn().float() - want).abs().max()) for k, fn in variants.items()}      # (also the warm-up of every variant)
            for fn in list(variants.values()) + list(kernels.values()):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            ktimes = {k: [] for k in kernels}
            for _ in range(windows):
                for k, fn in variants.items():
                    times[k].append(window(fn, calls))
                for k, fn in kernels.items():
                    ktimes[k].append(window(fn, calls))
        row = {"site": site, "shape": [B, H, W, C], "heads": heads, "shift": shift, "calls_per_window": calls, "windows": windows,
               "module": {k: spread(v) for k, v in times.items()}, "module_maxabs_vs_torch_fp32": diff, "kernel": {}}
        for k, v in ktimes.items():
            s = spread(v)
            s["bytes"] = 16 * C * tokens
            s["bytes_per_s"] = s["bytes"] / (s["median_ms"] * 1e-3)
            s["hbm_share"] = s["bytes_per_s"] / HBM_PEAK
            row["kernel"][k] = s
        print(f"{site} B={B} shift={shift} module ms  " + "  ".join(f"{k} {s['median_ms']:.3f}" for k, s in row["module"].items()), flush=True)
        print("      kernel  " + "  ".join(f"{k} {s['median_ms']:.4f} ms = {s['bytes_per_s'] / 1e9:.0f} GB/s ({100 * s['hbm_share']:.1f} % of HBM peak)"
                                           for k, s in row["kernel"].items()), flush=True)
        rows.append(row)
        del mods, variants, kernels
        torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "rows": rows}


def time_site_backward(site, B, windows):
    import torch

    from diffusiondepth_amd import swin as SW
    if not torch.cuda.is_available():
        sys.exit("window_attention_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    torch.cuda.set_device(0)
    H, W, C, heads = SITES[site]
    tokens = B * H * W
    rows = []

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    for shift in SHIFTS:
        torch.manual_seed(0)
        mods = {p: SW.HipShiftWindowMSA(C, heads, 7, shift_size=shift, precision=p, backward="hip") for p in SW.PRECISIONS}
        mods["torch"] = SW.HipShiftWindowMSA(C, heads, 7, shift_size=shift)
        mods["fp32"].w_msa.init_weights()
        for m in mods.values():
            m.load_state_dict(mods["fp32"].state_dict())
            m.cuda().train()
        ref = mods["torch"]
        x = torch.randn(B, H * W, C, device="cuda", requires_grad=True)
        g = torch.randn(B, H * W, C, device="cuda")
        with torch.no_grad():
            qkv = ref.w_msa.qkv(x).view(B, H, W, 3 * C).contiguous()
            bias, pad = ref._dense_bias().clone(), ref.w_msa.qkv.bias.detach().clone()
        gout = torch.randn(B, H, W, C, device="cuda")

        def step(m, autocast=False):
            def fn():
                x.grad = None
                m.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    y = m(x, (H, W))
                y.backward(g)
                return x.grad
            return fn

        variants = {"torch_fp32": step(ref), "torch_bf16": step(ref, True)}
        variants.update({f"hip_{p}": step(mods[p]) for p in SW.PRECISIONS})
        kernels = {p: (lambda p=p: SW.window_attention_backward(qkv, pad, bias, gout, heads, 7, shift, p)) for p in SW.PRECISIONS}
        calls = max(3, min(100, int(2e6 // tokens)))
        want = variants["torch_fp32"]().clone()
        diff = {k: float((fn().float() - want).abs().max()) for k, fn in variants.items()}      # (also the warm-up of every variant)
        for fn in list(variants.values()) + list(kernels.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        peak = {}
        for k in ("torch_fp32", "hip_fp32"):
            x.grad = None
            for m in mods.values():
                m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            variants[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - before
        times = {k: [] for k in variants}
        ktimes = {k: [] for k in kernels}
        for _ in range(windows):
            for k, fn in variants.items():
                times[k].append(window(fn, calls))
            for k, fn in kernels.items():
                ktimes[k].append(window(fn, calls))
        row = {"site": site, "shape": [B, H, W, C], "heads": heads, "shift": shift, "calls_per_window": calls, "windows": windows,
               "module_forward_backward": {k: spread(v) for k, v in times.items()}, "input_grad_maxabs_vs_torch_fp32": diff,
               "peak_bytes_forward_backward": peak, "workspace_bytes": SW.backward_workspace_bytes(B, H, W, C, heads), "backward_kernel": {}}
        for k, v in ktimes.items():
            s = spread(v)
            s["bytes"] = 28 * C * tokens
            s["bytes_per_s"] = s["bytes"] / (s["median_ms"] * 1e-3)
            s["hbm_share"] = s["bytes_per_s"] / HBM_PEAK
            row["backward_kernel"][k] = s
        print(f"{site} B={B} shift={shift} module fwd+bwd ms  " + "  ".join(f"{k} {s['median_ms']:.3f}" for k, s in row["module_forward_backward"].items()),
              flush=True)
        print("      backward kernel  " + "  ".join(f"{k} {s['median_ms']:.4f} ms = {s['bytes_per_s'] / 1e9:.0f} GB/s" for k, s in row["backward_kernel"].items())
              + f"   peak MB torch {peak['torch_fp32'] / 1e6:.1f} hip {peak['hip_fp32'] / 1e6:.1f}", flush=True)
        rows.append(row)
        del mods, variants, kernels
        torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sites", default=",".join(SITES))
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for one (site, batch) child process")
    ap.add_argument("--site", help="(child) time this one site and write the rows to --out")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--backward", action="store_true", help="time the module's forward + backward and the backward kernel instead")
    args = ap.parse_args()
    if args.windows < 5:
        sys.exit("window_attention_timing: at least five windows")
    if args.site:
        res = (time_site_backward if args.backward else time_site)(args.site, args.batch, args.windows)
        with open(args.out, "w") as fh:
            json.dump(res, fh)
        return
    rows, device = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for site in [s for s in args.sites.split(",") if s]:
            for B in BATCHES:
                part = os.path.join(tmp, f"{site}_{B}.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--site", site, "--batch", str(B), "--windows", str(args.windows), "--out", part] + \
                    (["--backward"] if args.backward else [])
                try:
                    r = subprocess.run(cmd, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    sys.exit(f"window_attention_timing: {site} B={B} ran into its time limit of {args.step_timeout} s; nothing more is started")
                if r.returncode != 0:
                    sys.exit(f"window_attention_timing: {site} B={B} failed with status {r.returncode}; nothing more is started")
                with open(part) as fh:
                    res = json.load(fh)
                device = res["device"]
                rows += res["rows"]
    result = {"tool": "window_attention_timing" + (" --backward" if args.backward else ""), "device": device, "hbm_peak_bytes_per_s": HBM_PEAK,
              "floor_bytes_per_token": "28 * C" if args.backward else "16 * C", "rows": rows}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
