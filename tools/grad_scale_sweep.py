#!/usr/bin/env python3
"""Where should the incoming gradient of the f16 backward sit?  The measurement behind GRAD_AMAX_EXP (csrc/dd_kernels.h).

    python tools/grad_scale_sweep.py [--emu] [--precs f16x3,f16] [--cases denoise_bwd_res,denoise_bwd_swin] [--out profiles/grad_scale_sweep.json]

With option "grad_autoscale" = 0 (the gradient travels as it comes) dd_denoise_once_backward runs on 2^k x grad_eps of the golden cases for
k = -30 .. +20 in steps of 2; every result is divided by 2^k in fp64 and compared, as relative L2 per tensor, with the reference's autograd
golden (linear in grad_eps: the k = 0 file is the reference at every k).  Per case and precision the tool reports the contiguous range of k
around the best one over which EVERY tensor stays within 1.5 x its own best error, and the log2 centre of that range as the amax the
scaled gradient should have (the cases draw grad_eps from a standard normal: amax = 2^k x max|grad_eps|).

--emu runs the library's host emulation (tests/hostemu_util: no GPU, about 7 s per call); without it the HIP library on the GPU.  A run
appends its records to the JSON file under "runs" (keyed by where it ran), so the emulation's and the GPU's sweeps sit side by side."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from diffusiondepth_amd import synth  # noqa: E402
from diffusiondepth_amd.backend import HipDenoiser, precision_id  # noqa: E402

KS = list(range(-30, 21, 2))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-300, np.sqrt((b ** 2).sum())))


def golden_params(g, get_grad):
    """{name: (got, want)} of every 'grad.model.*' entry of a golden file (strided samples / embedding rows handled as the tests do)."""
    import re
    out = {}
    for k in g:
        if not k.startswith("grad.model.") or k.endswith((".rows", ".sums")):
            continue
        name = k[len("grad."):]
        m = re.match(r"(.*)\.stride(\d+)$", name)
        if m:
            got = get_grad(m.group(1)).reshape(-1)[::int(m.group(2))]
        elif name == "model.time_embedding.weight":
            got = get_grad(name)[g[k + ".rows"]]
        else:
            got = get_grad(name)
        out[name] = (got, g[k])
    return out


class Emu:
    where = "host emulation"

    def __init__(self, variant):
        import diffusiondepth_amd as dda
        from hostemu_driver import EmuDenoiser
        from hostemu_util import build_library
        self.be = EmuDenoiser(build_library(), variant)
        self.shapes = dict(HipDenoiser.PARAM_SHAPES, **(HipDenoiser.SWIN_PARAM_SHAPES if variant == "swin" else {}))
        self.sched = dda.DDIMScheduler().alphas_cumprod

    def load(self, sd):
        self.be.load_state_dict(sd)
        self.be.set_schedule(self.sched)
        self.be.set_option("hoist_cond", 0)

    def once_backward(self, x, t, cond, ge, prec):
        from hostemu_driver import _p, f32
        be, lib = self.be, self.be.lib
        x, cond, ge, t = f32(x), f32(cond), f32(ge), np.ascontiguousarray(t, np.int64)
        gx, gc = np.full_like(x, np.nan), np.full_like(cond, np.nan)
        B, _, h, w = x.shape
        be.ck(lib.dd_zero_grad(be.h, None), "dd_zero_grad")
        be.ck(lib.dd_denoise_once_backward(be.h, _p(x), _p(t), _p(cond), _p(ge), _p(gx), _p(gc), B, h, w, cond.shape[2], cond.shape[3],
                                           precision_id(prec), None), "dd_denoise_once_backward")

        def get(name):
            out = np.full(self.shapes[name], np.nan, np.float32)
            be.ck(lib.dd_get_grad(be.h, name.encode(), _p(out), out.size, None), "dd_get_grad")
            return out
        return gx, gc, get


class Gpu:
    where = "MI355X"

    def __init__(self, variant):
        import diffusiondepth_amd as dda
        self.be = dda.HipDenoiser(variant=variant)
        self.sched = dda.DDIMScheduler().alphas_cumprod

    def load(self, sd):
        self.be.load_state_dict(sd)
        self.be.set_schedule(self.sched)

    def once_backward(self, x, t, cond, ge, prec):
        import torch
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.be.zero_grad()
        gx, gc = self.be.denoise_once_backward(cu(x), cu(t), cu(cond), cu(ge), prec)
        return gx.cpu().numpy(), gc.cpu().numpy(), lambda name: self.be.grad(name).cpu().numpy()


def flat_region(rows):
    """rows: [(k, {tensor: err})] -> (k_lo, k_hi) of the contiguous range around the best k over which every tensor is within 1.5 x its best."""
    names = list(rows[0][1])
    best = {n: min(e[n] for _, e in rows if math.isfinite(e[n])) for n in names}
    ok = [all(math.isfinite(e[n]) and e[n] <= 1.5 * best[n] for n in names) for _, e in rows]
    if not any(ok):
        return None
    score = [max(e[n] / best[n] if math.isfinite(e[n]) else math.inf for n in names) for _, e in rows]
    i = int(np.argmin(score))
    lo = hi = i
    while lo > 0 and ok[lo - 1]:
        lo -= 1
    while hi + 1 < len(rows) and ok[hi + 1]:
        hi += 1
    return rows[lo][0], rows[hi][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--precs", default="f16x3,f16")
    ap.add_argument("--cases", default="denoise_bwd_res,denoise_bwd_swin")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_scale_sweep.json"))
    args = ap.parse_args()
    with open(os.path.join(GOLDEN_DIR, "cases.json")) as f:
        cases = json.load(f)
    records = []
    for cname in args.cases.split(","):
        c = cases[cname]
        variant = c.get("variant", "res")
        with np.load(os.path.join(GOLDEN_DIR, cname + ".npz")) as z:
            g = {k: z[k] for k in z.files}
        drv = (Emu if args.emu else Gpu)(variant)
        drv.load(synth.make_state_dict(c["wseed"], variant))
        drv.be.set_option("grad_autoscale", 0)
        inp = synth.make_inputs(c["iseed"], c["B"], c["h"], c["w"], tuple(c["cond_hw"]) if "cond_hw" in c else None)
        ge = np.random.RandomState(c["gseed"]).standard_normal(inp["x_T"].shape).astype(np.float32)
        amax0 = float(np.abs(ge).max())
        for prec in args.precs.split(","):
            rows = []
            for k in KS:
                sc = 2.0 ** k
                gx, gc, get = drv.once_backward(inp["x_T"], inp["timesteps"], inp["cond"], (ge * np.float32(sc)).astype(np.float32), prec)
                errs = {"grad_x": rel_l2(gx.astype(np.float64) / sc, g["grad_x"]), "grad_cond": rel_l2(gc[:, :8].astype(np.float64) / sc, g["grad_cond_ch0_8"])}
                for name, (got, want) in golden_params(g, get).items():
                    errs[name.replace("model.", "")] = rel_l2(got.astype(np.float64) / sc, want)
                errs = {n: (e if math.isfinite(e) else float("inf")) for n, e in errs.items()}
                rows.append((k, errs))
                print(f"{cname} {prec} k={k:+d}: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)})", flush=True)
            fr = flat_region(rows)
            rec = {"case": cname, "precision": prec, "grad_eps_amax_at_k0": amax0, "flat_k": fr,
                   "amax_log2_centre": None if fr is None else 0.5 * (fr[0] + fr[1]) + math.log2(amax0),
                   "rows": [{"k": k, "worst": (max(e.values()) if math.isfinite(max(e.values())) else "non-finite"),
                             "errs": {n: (v if math.isfinite(v) else "non-finite") for n, v in e.items()}} for k, e in rows]}
            print(f"{cname} {prec}: flat region k = {fr}, amax centre 2^{rec['amax_log2_centre']}", flush=True)
            records.append(rec)
        drv.be.close()
    doc = {"what": "dd_denoise_once_backward with grad_autoscale = 0 on 2^k x grad_eps; relative L2 per tensor of result / 2^k against the reference's autograd golden",
           "criterion": "contiguous k range around the best k over which every tensor is within 1.5 x its best error; amax centre = mid k + log2 max|grad_eps|", "runs": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    run = doc["runs"].setdefault((Emu if args.emu else Gpu).where, [])
    run[:] = [r for r in run if (r["case"], r["precision"]) not in {(q["case"], q["precision"]) for q in records}] + records
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
