"""The parameter sets whose packed images are pinned by tests/golden/weight_digests.json (dd_debug_weights_digest: FNV-1a over every packed
weight buffer of the handle).  The fixture holds what the host-side packer of the commit named in its "how_recorded" note left in memory, per
platform: "hostemu" (tests/test_library_host_emulation.py) and "mi355x" (tests/test_zzz_gpu_device_weights.py; the denoiser digest contains the
device-computed E[t] table, so the platforms need not coincide).  The library has packed on the device alone since; the fixture is what ties
its images to that packer's bytes."""
from __future__ import annotations

import json
import os

import numpy as np

from diffusiondepth_amd import synth

SWINL, MPVIT = (192, 384, 768, 1536), (128, 216, 288, 288)
# name -> (variant, larger case: host emulation runs it under DD_EMU_FULL=1 only)
CASES = {
    "res": ("res", False), "res_updated": ("res", False), "res_fpn": ("res", False),
    "swin": ("swin", False), "swin_updated": ("swin", False),
    "swin_fpn_swinl": ("swin", True), "swin_fpn_mpvit": ("swin", True),
    "swin_neck_swinl": ("swin", True), "swin_neck_mpvit": ("swin", True),
}


def updated(sd):
    """The second parameter set of the route tests: every denoiser parameter moved."""
    return {k: (v * 1.25 + 0.01).astype(np.float32) for k, v in sd.items() if k.startswith("model.")}


def state_dict(name):
    variant = CASES[name][0]
    sd = synth.make_state_dict(7301, variant)
    if name.endswith("_updated"):
        return {**sd, **updated(sd)}
    if name == "res_fpn":
        return {**sd, **synth.make_fpn_state_dict(7241)}
    if "_fpn_" in name or "_neck_" in name:
        chans = SWINL if name.endswith("swinl") else MPVIT
        sd = {**sd, **synth.make_fpn_state_dict(7241, in_channels=chans)}
        if "_neck_" in name:
            sd.update(synth.make_hahi_state_dict(7246, chans))
    return sd


def recorded(platform):
    """{case: digest} of one platform ({} where none was stored)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_digests.json")) as f:
        return {k: int(v, 16) for k, v in json.load(f)["digests"].get(platform, {}).items()}
