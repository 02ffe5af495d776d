#!/usr/bin/env python3
"""Mint known-answer vectors for the depth metrics and the supervised loss from the REFERENCE's own classes.

Build container only (needs the reference tree, tests/golden/ref_import.py:REF_SRC).  What runs, imported verbatim from there:
  metric.diffusion_dcbase_metric.Diffusion_DCbase_Metric, loss.submodule.l1loss.L1Loss, loss.submodule.l2loss.L2Loss,
  loss.diffusion_dcbase_loss.Diffusion_DCbase_Loss
on the seeded inputs of tests/eval_cases.py, once in fp32 (what the reference computes) and once on ``.double()`` inputs (how far its own fp32
accumulation is from the exact value: the yardstick of the tests' tolerances).  Nothing of this repository's kernels or eager paths is involved.
Inputs are NOT stored (a KITTI case is megabytes): the fixture keeps their sha256, the tests regenerate and compare.

The reference's metric returns only the eight quotients; its nine ``.sum()`` results (num_valid, then the sums of diff_sqr, diff_abs, diff_inv_sqr,
diff_inv_abs, rel, del_1, del_2, del_3, diffusion_dcbase_metric.py:41-90) are recorded on their way by wrapping ``torch.Tensor.sum`` for the
duration of the call.  Per-image rows come from calling the class on each image alone.

Re-run:  python tests/golden/make_golden_eval.py      ->  tests/golden/eval_metric.npz, tests/golden/eval_loss.npz
Keys: "<case>/<what>"; every floating value is stored as float64 (an fp32 result is exactly representable).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from ref_import import REF_SRC  # noqa: E402
import eval_cases as E  # noqa: E402

sys.path.insert(0, REF_SRC)
from metric.diffusion_dcbase_metric import Diffusion_DCbase_Metric  # noqa: E402
from loss.submodule.l1loss import L1Loss  # noqa: E402
from loss.submodule.l2loss import L2Loss  # noqa: E402
from loss.diffusion_dcbase_loss import Diffusion_DCbase_Loss  # noqa: E402

# order in which evaluate() calls .sum()  ->  position in the ABI's row [n_valid, S|d|, Sd^2, S|dinv|, Sdinv^2, Srel, #d1, #d2, #d3]
CALL_TO_ROW = [0, 2, 1, 4, 3, 5, 6, 7, 8]


def metric_with_sums(metric, pred, gt):
    """(metrics [8], sums [9]) of one evaluate() call, both as float64 arrays of whatever precision the call ran in."""
    rec = []
    orig = torch.Tensor.sum

    def spy(self, *a, **k):
        r = orig(self, *a, **k)
        rec.append(float(r))
        return r

    torch.Tensor.sum = spy
    try:
        res = metric.evaluate({"gt": gt}, {"pred": pred}, "test")
    finally:
        torch.Tensor.sum = orig
    assert len(rec) == 9 and tuple(res.shape) == (1, 8), (len(rec), res.shape)
    row = np.zeros(9)
    for i, v in enumerate(rec):
        row[CALL_TO_ROW[i]] = v
    return res[0].double().numpy(), row


def mint_metric():
    out = {}
    metric = Diffusion_DCbase_Metric(types.SimpleNamespace())
    for name in E.CASES:
        pred, gt, _ = E.make_case(name)
        out[name + "/sha_pred"], out[name + "/sha_gt"] = E.sha256(pred), E.sha256(gt)
        for tag, cast in (("32", lambda t: t), ("64", lambda t: t.double())):
            p, g = cast(torch.from_numpy(pred)), cast(torch.from_numpy(gt))
            m, s = metric_with_sums(metric, p, g)
            out[f"{name}/metrics{tag}"], out[f"{name}/batch_sums{tag}"] = m, s
            rows = [metric_with_sums(metric, p[b:b + 1], g[b:b + 1]) for b in range(p.shape[0])]
            out[f"{name}/image_metrics{tag}"] = np.stack([r[0] for r in rows])
            out[f"{name}/sums{tag}"] = np.stack([r[1] for r in rows])
        print(name, "metrics32", out[name + "/metrics32"], "rel |32-64|",
              np.abs(out[name + "/metrics32"] - out[name + "/metrics64"]) / np.maximum(np.abs(out[name + "/metrics64"]), 1e-300))
    np.savez_compressed(os.path.join(HERE, "eval_metric.npz"), **out)


def grads(fn, pred, gt):
    p = pred.clone().requires_grad_(True)
    val = fn(p, gt)
    val.backward()
    return float(val.detach()), p.grad.double().numpy()


def mint_loss():
    out = {}
    for name in E.LOSS_CASES:
        pred, gt, max_depth = E.make_case(name)
        args = types.SimpleNamespace(max_depth=max_depth, loss=f"{E.W1}*L1+{E.W2}*L2+1.0*DDIM")
        l1, l2, full = L1Loss(args), L2Loss(args), Diffusion_DCbase_Loss(args)
        out[name + "/sha_pred"], out[name + "/sha_gt"] = E.sha256(pred), E.sha256(gt)
        g = {}
        for tag, cast in (("32", lambda t: t), ("64", lambda t: t.double())):
            p, t = cast(torch.from_numpy(pred)), cast(torch.from_numpy(gt))
            out[f"{name}/l1_{tag}"], g["l1" + tag] = grads(l1, p, t)
            out[f"{name}/l2_{tag}"], g["l2" + tag] = grads(l2, p, t)
            ddim = cast(torch.tensor(0.125))
            pp = p.clone().requires_grad_(True)
            loss_sum, loss_val = full({"gt": t}, {"pred": pp, "ddim_loss": ddim})
            loss_sum.backward()
            g["comb" + tag] = pp.grad.double().numpy()
            out[f"{name}/loss_sum{tag}"], out[f"{name}/loss_val{tag}"] = loss_sum.detach().double().numpy(), loss_val.double().numpy()
        out[name + "/loss_name"] = np.array(full.loss_name)
        for k, (a, b) in (("l1", (1.0, 0.0)), ("l2", (0.0, 1.0)), ("comb", (E.W1, E.W2))):
            out[f"{name}/grad_{k}_err32"] = E.rel_l2(g[k + "32"], g[k + "64"])                  # the reference's own fp32 autograd against its fp64
            out[f"{name}/grad_{k}_formula_vs_ref64"] = E.rel_l2(E.grad_formula64(pred, gt, max_depth, a, b), g[k + "64"])
            if name in E.SMALL:
                out[f"{name}/grad_{k}_32"], out[f"{name}/grad_{k}_64"] = g[k + "32"], g[k + "64"]
        print(name, "L1", out[name + "/l1_32"], "L2", out[name + "/l2_32"],
              {k: float(v) for k, v in out.items() if k.startswith(name + "/grad_") and np.ndim(v) == 0})
    np.savez_compressed(os.path.join(HERE, "eval_loss.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(1)      # one summation order for the fp32 sums, whatever machine mints them
    mint_metric()
    mint_loss()
