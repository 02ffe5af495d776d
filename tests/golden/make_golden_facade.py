#!/usr/bin/env python3
"""Mint the known answers of tests/test_reference_facade.py from the REFERENCE's own facade and heads.

Needs the reference's classes (tests/golden/ref_import.py: the reference tree, or the bytecode oracle/ref_py/build_ref.py stages from it).
What runs: the reference's unmodified ``Diffusion_DCbase_Model`` (diffusion_dcbase_model.py:26-224) with its ``HEADS`` registry holding the
reference's own head class; it builds the backbone (the stand-in factories the test shares with diffusiondepth_amd.model) and then its head
through ``HEADS.build(depth_head_cfg)`` (:77-91), gets the seeded synthetic head parameters and backbone BatchNorm statistics, and runs
``forward(sample)`` (src/main.py:232, :434) under torch.manual_seed(1234).  Stored per case: the predicted depth, pred_init, ddim_loss, the
output dict's keys (and which are None), the kwargs the facade passed to HEADS.build, and a sha256 per state_dict entry -- the parameters the
test rebuilds must be these, bit for bit.

    python tests/golden/make_golden_facade.py            # case cpu_res (CPU tensors)
    python tests/golden/make_golden_facade.py --gpu      # cases gpu_res, gpu_swin_hahi (cuda:0: the pipeline draws x_T on the device)
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_import  # noqa: E402
import test_reference_facade as F  # noqa: E402

CASES = {"cpu_res": ("res", "DDIMDepthEstimate_Res", "mmbev_res18", 5, (64, 96), 1, "cpu"),
         "gpu_res": ("res", "DDIMDepthEstimate_Res", "mmbev_res18", 20, (96, 160), 2, "cuda"),
         "gpu_swin_hahi": ("swin_hahi", "DDIMDepthEstimate_Swin_ADDHAHI", "swin_l_standin", 20, (96, 160), 2, "cuda")}


class _Recording:
    """HEADS stand-in: builds the registered class and keeps the cfg the facade passed"""

    def __init__(self, cls):
        self.cls, self.cfg = cls, None

    def build(self, cfg):
        self.cfg = dict(cfg)
        cfg = dict(cfg)
        cfg.pop("type")
        return self.cls(**cfg)


def _reference_head(family):
    ns = ref_import.load_reference()
    if family == "swin_hahi":
        import make_golden_hahi as G
        return G.load_hahi_reference()[2]
    return ns.DDIMDepthEstimate_Res


def mint(name):
    family, head, backbone, T, hw, B, dev = CASES[name]
    dev = torch.device(dev)
    fac = ref_import.load_reference_facade()
    bb = sys.modules["model.backbone"]
    bb.BACKBONE_FACTORIES.update(F.backbone_factories())
    fac.HEADS = rec = _Recording(_reference_head(family))
    torch.manual_seed(F.INIT_SEED)
    model = fac.Diffusion_DCbase_Model(F.facade_args(head, backbone, T))
    F.load_head_and_bn(model, family)
    model = model.to(dev).eval()
    sample = F.make_sample(B, hw[0], hw[1], dev)
    torch.manual_seed(F.FORWARD_SEED)
    if dev.type == "cuda":
        torch.cuda.manual_seed_all(F.FORWARD_SEED)
    with torch.no_grad():
        r = model(sample)
    cfg = {k: (None if k == "init_cfg" else v) for k, v in rec.cfg.items()}          # init_cfg = the args namespace itself (rebuilt by the test)
    sd = model.state_dict()
    out = {"pred": r["pred"].float().cpu().numpy(), "pred_init": r["pred_init"].float().cpu().numpy(),
           "ddim_loss": np.float64(float(r["ddim_loss"])),
           "keys": np.array(sorted(r)), "none_keys": np.array(sorted(k for k in r if r[k] is None)),
           "build_cfg": np.array(json.dumps(cfg, sort_keys=True)), "init_cfg_is_args": np.array(rec.cfg["init_cfg"] is model.args),
           "sd_keys": np.array(list(sd)), "sd_sha256": np.array([hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()])}
    path = os.path.join(HERE, f"facade_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"facade_{name}: {os.path.getsize(path) / 1024:.1f} KiB, pred {out['pred'].shape}, ddim_loss {float(out['ddim_loss']):.6f}")


if __name__ == "__main__":
    if not ref_import.reference_available():
        raise SystemExit("needs the reference tree or its staged bytecode (oracle/ref_py/build_ref.py)")
    for n in (["gpu_res", "gpu_swin_hahi"] if "--gpu" in sys.argv else ["cpu_res"]):
        mint(n)
