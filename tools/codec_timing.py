#!/usr/bin/env python3
"""Forward + backward time of the latent codec's four convolution sites, its decoder tail, and the whole encoder and decoder in .train() on the
MI355X, at KITTI (352 x 1216) and NYU (228 x 304) size, B = 4, in one process:

    sites     (a) nn.Conv2d / nn.ConvTranspose2d in fp32       (MIOpen: what runs by default, the parent's path)
              (b) codec.HipCodecConv2d / HipCodecConvTranspose2d  (csrc/dd_codec.hip)
    tail      (a) 1 / sigmoid(z).clamp(eps) - 1 as torch writes it (four launches forward)      (b) codec.HipCodecTail
    encoder, decoder: DeepDepthTransformWithUpsampling.t / .inv_t, .train(), forward + backward, the four combinations of
              codec_backend torch | hip and bn_backend torch | hip

    python tools/codec_timing.py [--out profiles/codec_timing.json] [--windows 7] [--sizes kitti,nyu]
    python tools/codec_timing.py --eval-kernels      # the eval-mode inference kernels dd_encode / dd_decode instead (KITTI, B = 4 and 1)

Method: every variant is warmed up; a timed window is CALLS forward + backward passes (every gradient the head asks for: ENC0 has no data gradient)
between two device events on the caller's stream; inside one repeat the variants are timed one after another (so drift hits all alike), and the
median over the repeats is reported with min and max.  Each library call of (b) is also timed alone and set against the HBM peak from the bytes the
call must move (each tensor of the call once, fp32).  No speed-up is assumed: every row is reported, slower ones included.  A measurement path that
finds no GPU fails."""
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
from diffusiondepth_amd import codec as CD  # noqa: E402
from diffusiondepth_amd.modules import DeepDepthTransformWithUpsampling  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec
B = 4
SIZES = {"kitti": (352, 1216), "nyu": (228, 304)}
SITES = (("enc0", CD.OP_ENC0), ("enc1", CD.OP_ENC1), ("dec0", CD.OP_DEC0), ("dec1", CD.OP_DEC1))


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


def timed(variants, windows, calls):
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, calls))
    return {k: spread(v) for k, v in times.items()}


def input_hw(op, H, W):
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (H, W) if op in (CD.OP_ENC0, CD.OP_DEC1) else (h, w)


def time_site(size, name, op, H, W, windows):
    cin, cout, k, s, p, bias, transposed = CD.GEOMETRY[op]
    h, w = input_hw(op, H, W)
    need_x = op != CD.OP_ENC0      # the ground-truth depth carries no gradient
    x = torch.randn(B, cin, h, w, device="cuda").requires_grad_(need_x)
    gy = torch.randn(B, cout, *CD.output_hw(op, h, w), device="cuda")

    def make(hip):
        if transposed:
            return (CD.HipCodecConvTranspose2d if hip else nn.ConvTranspose2d)(cin, cout, k, s, p).cuda()
        return (CD.HipCodecConv2d if hip else nn.Conv2d)(cin, cout, k, s, p, bias=bias).cuda()

    mods = {"a_miopen_fp32": make(False), "b_hip": make(True)}

    def step(key):
        x.grad = None
        mods[key].zero_grad(set_to_none=True)
        mods[key](x).backward(gy)

    calls = 10
    row = {"size": size, "site": name, "input": [B, cin, h, w], "calls_per_window": calls, "windows": windows,
           "fwd_bwd": timed({key: (lambda key=key: step(key)) for key in mods}, windows, calls), "kernels_b": {}}
    m = mods["b_hip"]
    xd, wd, bd = x.detach(), m.weight.detach(), (m.bias.detach() if bias else None)
    kern = {"forward": (lambda: CD.conv_forward(op, xd, wd, bd), 4 * (xd.numel() + gy.numel())),
            "backward_weight": (lambda: CD.conv_backward_weight(op, xd, gy, need_bias=bias), 4 * (xd.numel() + gy.numel()))}
    if need_x:
        kern["backward_data"] = (lambda: CD.conv_backward_data(op, gy, wd, xd.shape), 4 * (xd.numel() + gy.numel()))
    kt = timed({kk: fn for kk, (fn, _) in kern.items()}, windows, calls)
    for kk, sp in kt.items():
        sp["bytes"] = kern[kk][1]
        sp["hbm_share"] = sp["bytes"] / (sp["median_ms"] * 1e-3) / HBM_PEAK
        row["kernels_b"][kk] = sp
    f = row["fwd_bwd"]
    row["b_not_slower_than_a_beyond_spread"] = not_slower(f["b_hip"], f["a_miopen_fp32"])
    print(f"{size:5s} {name:5s} {str((B, cin, h, w)):20s} fwd+bwd ms  " +
          "  ".join(f"{kk} {v['median_ms']:7.3f} [{v['min_ms']:.3f}..{v['max_ms']:.3f}]" for kk, v in f.items()), flush=True)
    print("            " + "  ".join(f"{kk} {sp['median_ms']:.3f} ms = {100 * sp['hbm_share']:.1f} % HBM" for kk, sp in row["kernels_b"].items()), flush=True)
    return row


def time_tail(size, H, W, windows):
    z = (torch.randn(B, 1, H, W, device="cuda") * 2 - 2).requires_grad_(True)
    gd = torch.randn(B, 1, H, W, device="cuda")
    tail, eps = CD.HipCodecTail(1e-6), 1e-6

    def step(hip):
        z.grad = None
        (tail(z) if hip else 1.0 / torch.sigmoid(z).clamp(eps) - 1).backward(gd)

    calls = 10
    row = {"size": size, "site": "tail", "input": [B, 1, H, W], "calls_per_window": calls, "windows": windows,
           "fwd_bwd": timed({"a_torch": lambda: step(False), "b_hip": lambda: step(True)}, windows, calls), "kernels_b": {}}
    zd = z.detach()
    kern = {"forward": (lambda: CD.tail_forward(zd, eps), 8 * zd.numel()), "backward": (lambda: CD.tail_backward(zd, gd, eps), 12 * zd.numel())}
    kt = timed({kk: fn for kk, (fn, _) in kern.items()}, windows, calls)
    for kk, sp in kt.items():
        sp["bytes"] = kern[kk][1]
        sp["hbm_share"] = sp["bytes"] / (sp["median_ms"] * 1e-3) / HBM_PEAK
        row["kernels_b"][kk] = sp
    f = row["fwd_bwd"]
    row["b_not_slower_than_a_beyond_spread"] = not_slower(f["b_hip"], f["a_torch"])
    print(f"{size:5s} tail  {str((B, 1, H, W)):20s} fwd+bwd ms  " +
          "  ".join(f"{kk} {v['median_ms']:7.3f} [{v['min_ms']:.3f}..{v['max_ms']:.3f}]" for kk, v in f.items()), flush=True)
    print("            " + "  ".join(f"{kk} {sp['median_ms']:.3f} ms = {100 * sp['hbm_share']:.1f} % HBM" for kk, sp in row["kernels_b"].items()), flush=True)
    return row


def time_codec(size, H, W, windows):
    """The whole encoder (t) and decoder (inv_t) in .train(), forward + backward, codec_backend x bn_backend."""
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    depth = torch.rand(B, 1, H, W, device="cuda") * 60 + 1
    lat = torch.randn(B, 16, h, w, device="cuda").requires_grad_(True)
    g_t, g_inv = torch.randn(B, 16, h, w, device="cuda"), torch.randn(B, 1, 2 * h, 2 * w, device="cuda")

    def build(codec, bn):
        torch.manual_seed(0)
        dt = DeepDepthTransformWithUpsampling()
        if codec == "hip":
            CD.convert_hip_codec(dt)
        if bn == "hip":
            BN.convert_hip_batchnorm(dt)
        return dt.cuda().train()

    mods = {f"codec_{c}_bn_{b}": build(c, b) for c in ("torch", "hip") for b in ("torch", "hip")}

    def enc(key):
        mods[key].zero_grad(set_to_none=True)
        mods[key].t(depth).backward(g_t)

    def dec(key):
        lat.grad = None
        mods[key].zero_grad(set_to_none=True)
        mods[key].inv_t(lat).backward(g_inv)

    rows = []
    for part, fn in (("encoder", enc), ("decoder", dec)):
        row = {"size": size, "site": part, "windows": windows, "calls_per_window": 5,
               "fwd_bwd": timed({key: (lambda key=key, fn=fn: fn(key)) for key in mods}, windows, 5)}
        f = row["fwd_bwd"]
        row["hip_not_slower_beyond_spread"] = {b: not_slower(f[f"codec_hip_bn_{b}"], f[f"codec_torch_bn_{b}"]) for b in ("torch", "hip")}
        print(f"{size:5s} whole {part} (train, fwd+bwd) ms  " + "  ".join(f"{k} {v['median_ms']:.3f} [{v['min_ms']:.3f}..{v['max_ms']:.3f}]" for k, v in f.items()),
              flush=True)
        rows.append(row)
    return rows


def eval_kernels():
    """--eval-kernels: the eval-mode inference kernels (dd_encode / dd_decode) at KITTI size, B = 4 and 1, and the decoder's parity against the
    torch-CPU port (what this tool measured before the training operators existed)."""
    import numpy as np
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    from oracle import torch_cpu_port as P
    sd = synth.make_state_dict(7240)
    be = dda.HipDenoiser()
    be.load_state_dict(sd)
    H, W = SIZES["kitti"]
    h, w = synth.latent_hw(H, W)
    for batch in (4, 1):
        gt = torch.from_numpy(synth.make_gt_depth(3, batch, H, W)).cuda()
        z = (torch.randn(batch, 16, h, w, generator=torch.Generator().manual_seed(1)) * 3).cuda()
        for name, fn in (("encode", lambda: be.encode(gt)), ("decode", lambda: be.decode(z))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            print(f"B={batch} {name}: {window(fn, 20) * 1e3:.1f} us", flush=True)
        d_ref = P.decode(P.to_torch_sd(sd), z[:1].cpu()).numpy()
        d = be.decode(z[:1]).cpu().numpy()
        print(f"B={batch} decode max rel err vs torch-CPU port: {float((np.abs(d - d_ref) / np.maximum(np.abs(d_ref), 1e-2)).max()):.2e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sizes", default="kitti,nyu")
    ap.add_argument("--eval-kernels", action="store_true", help="time dd_encode / dd_decode (eval-mode inference kernels) instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("codec_timing: no GPU visible to PyTorch -- this tool measures, it has no CPU path")
    if args.eval_kernels:
        return eval_kernels()
    if args.windows < 5:
        sys.exit("codec_timing: at least five windows")
    torch.cuda.set_device(0)
    rows = []
    for size in filter(None, args.sizes.split(",")):
        H, W = SIZES[size]
        for name, op in SITES:
            rows.append(time_site(size, name, op, H, W, args.windows))
        rows.append(time_tail(size, 2 * ((H - 1) // 2 + 1), 2 * ((W - 1) // 2 + 1), args.windows))
        rows += time_codec(size, H, W, args.windows)
        torch.cuda.empty_cache()
    result = {"tool": "codec_timing", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "batch": B, "rows": rows}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
