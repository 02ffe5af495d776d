#!/usr/bin/env python3
"""Where should a rescaled grad_y sit in f16?  CPU-only emulation of the operand rounding of the training convolutions' two gradients
(csrc/dd_conv.hip: ``to_operand`` rounds grad_y to f16, in "f16x3" to the pair hi = f16(v), lo = f16(v - hi)); the recorded evidence for the
exponent 14 of include/ddepth_conv_scaled.h.  No GPU, no library: torch's CPU convolutions in fp64.

    python tools/conv_grad_scale_sweep.py [--out profiles/conv_grad_scale_sweep.json] [--exponents -10:15] [--scales -30:16:2]

For each REAL shape of tests/conv_cases.py (S2, D1; N(0, 1) tensors), each mode, each incoming scale 2^k and each target exponent E -- or no
rescale at all ("none": grad_y is rounded as it arrives, what the unscaled entry points do) -- grad_y 2^k is multiplied by
s = 2^(E - floor(log2 amax)), rounded to the operand the kernel would hold (f16, or hi + lo; overflow to Inf and the subnormal grid included),
divided by s again, and sent through the fp64 gradient with x and w as the mode rounds them (f16: rounded; f16x3: their own hi + lo).  What is
recorded is the error this ROUNDING OF grad_y ALONE adds, against the same fp64 gradient on the unrounded grad_y, as a multiple of the tests'
cap (conv_cases.check_real: (K + 1) 2^-23 S, plus 2^-18 S for f16x3), maximum over the elements of grad_x and grad_w.  "spike": the same with
one element of grad_y set to 4096 times the unit scale, the heavy tail that decides how much headroom a lower exponent buys.

Reading it: an exponent is good where the share stays small for EVERY scale, with and without the spike.  Every E <= 15 keeps s amax below
65504, so the top never overflows; what E decides is the bottom: each bit of headroom given away at the top pushes the small elements of a
heavy-tailed gradient towards f16's subnormals (f16x3: lo goes subnormal below |s v| = 2^-3)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_cases as CC  # noqa: E402

ULP = 2.0 ** -23
KEYS = ("grad_x", "grad_w")


def f16(t):
    return t.float().to(torch.float16).double()      # (fp32 first: the kernel multiplies and rounds an fp32 value)


def operand(t, mode):
    """What the MFMA operand(s) of fp64 tensor `t` add up to: f16(t), or f16(t) + f16(t - f16(t))."""
    hi = f16(t)
    if mode == "f16":
        return hi
    lo = f16((t.float() - hi.float()).double())
    return hi + lo


def floor_log2(a):
    return int(np.float32(a).view(np.uint32) >> 23) - 127


def grads(op, x, w, gy):
    r = CC._reference(op, x, w, gy)
    return {k: r[k] for k in KEYS}


def sweep_case(name, mode, scales, exponents, spike):
    op = CC.SHAPES[name][0]
    inp = CC.make_inputs(name, "normal")
    x, w = operand(inp["x"].double(), mode), operand(inp["w"].double(), mode)
    gy1 = inp["grad_y"].double().clone()
    if spike:
        gy1.view(-1)[gy1.numel() // 2] = 4096.0
    K = CC.terms(name)
    ref1 = grads(op, x, w, gy1)                                  # linear in grad_y: the reference and S at scale 2^k are 2^k times these
    S1 = grads(op, x.abs(), w.abs(), gy1.abs())
    cap1 = {k: ((2.0 ** -18 if mode == "f16x3" else 0.0) + (K[k] + 1) * ULP) * S1[k] for k in KEYS}
    amax1 = float(gy1.abs().max())
    out = {}
    for k2 in scales:
        gy = (gy1 * 2.0 ** k2).float().double()                  # fp32, as it arrives
        e_amax = floor_log2(amax1 * 2.0 ** k2)
        row = {}
        for E in ["none"] + list(exponents):
            s = 1.0 if E == "none" else 2.0 ** int(np.clip(E - e_amax, -126, 126))
            rounded = operand(gy * s, mode) / s
            got = grads(op, x, w, rounded)
            worst = 0.0
            for key in KEYS:
                err = np.abs(got[key] - ref1[key] * 2.0 ** k2) / (cap1[key] * 2.0 ** k2)
                worst = max(worst, float(np.nanmax(err)) if np.isfinite(got[key]).all() else float("inf"))
            row[str(E)] = worst
        out[str(k2)] = row
    return out


def span(text):
    parts = [int(p) for p in text.split(":")]
    return list(range(parts[0], parts[1] + 1, parts[2] if len(parts) > 2 else 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--exponents", default="-10:15", help="target exponents E, first:last[:step]")
    ap.add_argument("--scales", default="-30:16:2", help="incoming scales k of grad_y 2^k, first:last[:step]")
    args = ap.parse_args()
    exponents, scales = span(args.exponents), span(args.scales)
    cases = {}
    for name in sorted({n for n, _, _ in CC.REAL}):
        for mode in ("f16", "f16x3"):
            for spike in (False, True):
                key = f"{name} {mode}" + (" spike" if spike else "")
                cases[key] = sweep_case(name, mode, scales, exponents, spike)
                worst = {str(E): max(cases[key][str(k)][str(E)] for k in scales) for E in ["none"] + exponents}
                finite = {E: v for E, v in worst.items() if E != "none"}
                best = min(finite, key=finite.get)
                print(f"{key:18s} worst share of the cap over the scales:  none {worst['none']:.3g}   E=2 {worst.get('2', float('nan')):.3g}   "
                      f"E=14 {worst.get('14', float('nan')):.3g}   E=15 {worst.get('15', float('nan')):.3g}   smallest at E={best} ({finite[best]:.3g})", flush=True)
    result = {"tool": "conv_grad_scale_sweep", "what": "error added by the f16 / f16x3 rounding of grad_y alone, as a multiple of the tests' cap, max over grad_x and "
              "grad_w; rows: incoming scale k (grad_y 2^k), columns: target exponent E of s = 2^(E - floor(log2 amax)) or 'none' (no rescale)",
              "shapes": {n: list(CC.SHAPES[n][1]) for n in sorted({n for n, _, _ in CC.REAL})}, "scales": scales, "exponents": exponents, "cases": cases}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    else:
        print(line)


if __name__ == "__main__":
    main()
