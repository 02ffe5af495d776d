#!/usr/bin/env python3
"""Time of a Swin block's token Linears (include/swin/ddepth_linear.h) at the four Swin-L sites of a KITTI-size image (the stride-4 map is 88 x 304) on
the MI355X:

    site   map        C     heads
    s1     88 x 304   192   6
    s2     44 x 152   384   12
    s3     22 x 76    768   24
    s4     11 x 38    1536  48

for B = 1 and 4, in one process per (site, batch):

    linears   qkv (C -> 3 C), proj (C -> C), fc1 (C -> 4 C, + GELU), fc2 (4 C -> C, + residual), each alone: torch fp32, torch under
              torch.autocast(bfloat16) (with its casts), the library at fp32 / bf16 / f16 on a packed weight -- with the library's bytes/s against
              the call's floor (one read of x, the packed weight and the addend, one write of y) and its share of the f16 MFMA peak
    attention HipShiftWindowMSA(precision=p) with linear="torch" (what the module ran before the Linears existed) against linear="hip",
              p = fp32 / bf16 / f16, shift 0, and the torch sequence under bf16 autocast
    ffn       identity + fc2(GELU(fc1(x))): torch fp32, torch under bf16 autocast, HipFFN at fp32 / bf16 / f16
    block     x + attn(norm1(x)), then ffn(norm2(.), identity): the library attention with torch Linears and a torch FFN, against library
              Linears everywhere, at the three precisions, and the all-torch block under bf16 autocast

    python tools/swin_linear_timing.py --out profiles/swin_linear_timing.json [--windows 7] [--step-timeout 300]

Method (tools/window_attention_timing.py's): the parent process never opens the GPU; every (site, batch) is a child process of this file
(``--site``) under its own time limit, one at a time, and the first child that fails ends the run.  In a child every variant is warmed up, a
timed window is CALLS calls between two device events, inside one repeat the variants are timed one after another (so drift hits all alike),
and the median over the windows is reported with min and max.  A measurement path that finds no GPU fails.
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
F16_MFMA_PEAK = 2.5e15     # FLOP/s, MI355X spec (dense f16 / bf16)
SITES = {"s1": (88, 304, 192, 6), "s2": (44, 152, 384, 12), "s3": (22, 76, 768, 24), "s4": (11, 38, 1536, 48)}
BATCHES = (1, 4)
PRECS = ("fp32", "bf16", "f16")


def spread(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def time_site(site, B, windows):
    import torch
    import torch.nn.functional as F
    from torch import nn

    from diffusiondepth_amd import linear as LN
    from diffusiondepth_amd import swin as SW
    if not torch.cuda.is_available():
        sys.exit("swin_linear_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    torch.cuda.set_device(0)
    H, W, C, heads = SITES[site]
    tokens = B * H * W

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def measure(variants, calls):
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(windows):
            for k, fn in variants.items():
                times[k].append(window(fn, calls))
        return {k: spread(v) for k, v in times.items()}

    def autocast(fn):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return fn()
        return run

    torch.manual_seed(0)
    calls = max(5, min(200, int(2e6 // tokens)))
    out = {"site": site, "shape": [B, H, W, C], "tokens": tokens, "heads": heads, "calls_per_window": calls, "windows": windows, "linears": {}}
    x = torch.randn(B, H * W, C, device="cuda")
    with torch.no_grad():
        # ---- the four Linears alone ------------------------------------------------------------------------------------------------------------
        for name, K, N, act, add in (("qkv", C, 3 * C, 0, False), ("proj", C, C, 0, False), ("fc1", C, 4 * C, 1, False), ("fc2", 4 * C, C, 0, True)):
            lin = nn.Linear(K, N).cuda().requires_grad_(False)
            xin = torch.randn(B, H * W, K, device="cuda")
            addend = torch.randn(B, H * W, N, device="cuda") if add else None

            def torch_fn(lin=lin, xin=xin, addend=addend, act=act):
                y = lin(xin)
                if act:
                    y = F.gelu(y)
                return y if addend is None else addend + y

            variants = {"torch_fp32": torch_fn, "torch_bf16": autocast(torch_fn)}
            for p in PRECS:
                packed = LN.pack_weight(lin.weight, p)
                variants[f"hip_{p}"] = lambda packed=packed, p=p, lin=lin, xin=xin, addend=addend, act=act: \
                    LN.linear_forward(xin, packed, lin.bias, addend, act, p)
            want = torch_fn()
            diff = {k: float((fn().float() - want).abs().max()) for k, fn in variants.items()}
            row = {"K": K, "N": N, "act": act, "addend": add, "flop": 2.0 * tokens * K * N, "maxabs_vs_torch_fp32": diff, "times": measure(variants, calls)}
            for p in PRECS:
                s = row["times"][f"hip_{p}"]
                s["floor_bytes"] = 4 * tokens * K + N * K * (4 if p == "fp32" else 2) + 4 * tokens * N * (2 if add else 1)
                s["bytes_per_s"] = s["floor_bytes"] / (s["median_ms"] * 1e-3)
                s["hbm_share"] = s["bytes_per_s"] / HBM_PEAK
                s["f16_mfma_peak_share"] = row["flop"] / (s["median_ms"] * 1e-3) / F16_MFMA_PEAK
            out["linears"][name] = row
            print(f"{site} B={B} {name:4s} {K:5d} -> {N:5d} ms  " + "  ".join(f"{k} {s['median_ms']:.4f}" for k, s in row["times"].items()) +
                  "   hip GB/s " + " ".join(f"{row['times'][f'hip_{p}']['bytes_per_s'] / 1e9:.0f}" for p in PRECS), flush=True)

        # ---- the attention module, the FFN and a whole block --------------------------------------------------------------------------------------
        att = {p: SW.HipShiftWindowMSA(C, heads, 7, shift_size=0, precision=p) for p in PRECS}
        att["fp32"].w_msa.init_weights()
        ffn = {p: LN.HipFFN(C, 4 * C, precision=p) for p in PRECS}
        for group in (att, ffn):
            for m in group.values():
                m.load_state_dict(group["fp32"].state_dict())
                m.requires_grad_(False).cuda().eval()
        norm1, norm2 = nn.LayerNorm(C).cuda().requires_grad_(False), nn.LayerNorm(C).cuda().requires_grad_(False)

        def att_fn(p, linear):
            def run():
                att[p].linear = linear
                return att[p](x, (H, W))
            return run

        variants = {"torch_seq_bf16_autocast": autocast(lambda: att["fp32"]._forward_torch(x, H, W))}
        for p in PRECS:
            variants[f"linear_torch_{p}"], variants[f"linear_hip_{p}"] = att_fn(p, "torch"), att_fn(p, "hip")
        out["attention"] = measure(variants, calls)

        torch_ffn = lambda: x + ffn["fp32"].layers(x)
        variants = {"torch_fp32": torch_ffn, "torch_bf16": autocast(torch_ffn)}
        variants.update({f"hip_{p}": (lambda p=p: ffn[p](x)) for p in PRECS})
        want = torch_ffn()
        out["ffn_maxabs_vs_torch_fp32"] = {k: float((fn().float() - want).abs().max()) for k, fn in variants.items()}
        out["ffn"] = measure(variants, calls)

        def block(p, linear):
            def run():
                att[p].linear = linear
                t = x + att[p](norm1(x), (H, W))
                h = norm2(t)
                return ffn[p](h, identity=t) if linear == "hip" else t + ffn[p].layers(h)
            return run

        def torch_block():
            t = x + att["fp32"]._forward_torch(norm1(x), H, W)
            return t + ffn["fp32"].layers(norm2(t))

        variants = {"torch_seq_bf16_autocast": autocast(torch_block)}
        for p in PRECS:
            variants[f"linear_torch_{p}"], variants[f"linear_hip_{p}"] = block(p, "torch"), block(p, "hip")
        out["block"] = measure(variants, calls)
    for part in ("attention", "ffn", "block"):
        print(f"{site} B={B} {part:9s} ms  " + "  ".join(f"{k} {s['median_ms']:.4f}" for k, s in out[part].items()), flush=True)
    return {"device": torch.cuda.get_device_name(0), "rows": [out]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sites", default=",".join(SITES))
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for one (site, batch) child process")
    ap.add_argument("--site", help="(child) time this one site and write the rows to --out")
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    if args.windows < 5:
        sys.exit("swin_linear_timing: at least five windows")
    if args.site:
        res = time_site(args.site, args.batch, args.windows)
        with open(args.out, "w") as fh:
            json.dump(res, fh)
        return
    rows, device = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for site in [s for s in args.sites.split(",") if s]:
            for B in BATCHES:
                part = os.path.join(tmp, f"{site}_{B}.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--site", site, "--batch", str(B), "--windows", str(args.windows), "--out", part]
                try:
                    r = subprocess.run(cmd, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    sys.exit(f"swin_linear_timing: {site} B={B} ran into its time limit of {args.step_timeout} s; nothing more is started")
                if r.returncode != 0:
                    sys.exit(f"swin_linear_timing: {site} B={B} failed with status {r.returncode}; nothing more is started")
                with open(part) as fh:
                    res = json.load(fh)
                device = res["device"]
                rows += res["rows"]
    result = {"tool": "swin_linear_timing", "device": device, "hbm_peak_bytes_per_s": HBM_PEAK, "f16_mfma_peak_flop_per_s": F16_MFMA_PEAK,
              "rows": rows}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
