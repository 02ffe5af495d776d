"""The drop-in claim on the REFERENCE's own facade: the reference's unmodified ``Diffusion_DCbase_Model``
(diffusion_dcbase_model.py:26-224) builds its backbone and then its head through ``HEADS.build(depth_head_cfg)`` with the kwarg set of :77-91
(type, in_channels, inference_steps, num_train_timesteps, depth_feature_dim, the two loss_cfgs, init_cfg=args).  What it did with the
reference's own heads is recorded in tests/golden/facade_<case>.npz (tests/golden/make_golden_facade.py): the kwargs it passed to HEADS.build,
a sha256 of every state_dict entry, and the outputs of ``forward(sample)`` -- the call ``main.py`` makes (src/main.py:232, :434) -- under a
fixed seed.  Here diffusiondepth_amd's head class registered under the same name is built with exactly those kwargs, in the facade's order
(backbone, then head) and under the same seed, inside ``diffusiondepth_amd.model.Diffusion_DCbase_Model``; it gets the same parameters -- the
state_dict must be the reference model's, entry for entry and bit for bit -- and ``forward(sample)`` must agree within the north star's 1e-3 abs
on the predicted depth.

CPU test: diffusiondepth_amd's heads evaluate non-HIP tensors with their own torch children (BASELINE configs[0]: the plumbing configuration).
GPU test (-m gpu): the same on cuda:0 in fp32, where diffusiondepth_amd's heads run the HIP library (encoder, FPN / HAHI neck, T-step loop,
decoder, the ddim_loss call), for the Res family and the Swin-HAHI family (README.md:215 headline configuration)."""
from __future__ import annotations

import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

INIT_SEED, FORWARD_SEED = 11, 1234      # torch's seed in front of the model's construction / of forward(sample)


class _Pyramid(nn.Module):
    """A four-level stand-in backbone with the given widths at strides 4 / 8 / 16 / 32 (the Swin-L / MPViT pyramids: the backbones stay upstream
    PyTorch per the north star and are not part of the path; both sides of a comparison get the SAME instance weights)."""

    def __init__(self, widths):
        super().__init__()
        self.stem = nn.Conv2d(3, widths[0], 4, 4)
        self.down = nn.ModuleList(nn.Conv2d(a, b, 2, 2) for a, b in zip(widths[:-1], widths[1:]))

    def forward(self, x):
        x = torch.relu(self.stem(x))
        out = [x]
        for d in self.down:
            x = torch.relu(d(x))
            out.append(x)
        return out


def backbone_factories():
    """the zero-argument backbone factories both sides use (the reference facade's `model.backbone.get` serves the same ones when minting)"""
    from diffusiondepth_amd import model as M
    return dict(M.BACKBONES, swin_l_standin=lambda: _Pyramid([192, 384, 768, 1536]))


def facade_args(head, backbone, T):
    # the attributes Diffusion_DCbase_Model.__init__ reads (src/config.py flags; diffusion_dcbase_model.py:67-81)
    return SimpleNamespace(backbone_module="mmbev_resnet", backbone_name=backbone, head_specify=head, inference_steps=T, num_train_timesteps=1000)


def make_sample(B, H, W, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randn(B, 3, H, W, generator=g)
    gt = torch.rand(B, 1, H, W, generator=g) * 9.0 + 0.5
    dep = gt * (torch.rand(B, 1, H, W, generator=g) < 0.05)
    return {k: v.to(dev) for k, v in dict(rgb=rgb, gt=gt, dep=dep, depth_map=dep.clone(), depth_mask=(dep > 0).float()).items()}


def load_head_and_bn(model, family):
    """the head's parameters: the seeded synthetic weights of the head goldens (tests/golden/cases.json: a decoder gain that keeps the untrained loop's
    output in a few units -- with torch's default initialisation the 20-step loop amplifies the last bits of two different fp32 convolution
    implementations to metres); the backbone keeps its seeded initialisation, with non-trivial BatchNorm statistics"""
    from diffusiondepth_amd import synth
    chans = {"res": (64, 128, 256, 512), "swin_hahi": (192, 384, 768, 1536)}[family]
    hsd = dict(synth.make_state_dict(7240, "res" if family == "res" else "swin", 0.05, 0.0))
    hsd.update({k: v for k, v in synth.make_fpn_state_dict(7241 if family == "res" else 7243, in_channels=chans).items() if family == "res" or not k.startswith("convup_fp")})
    if family == "swin_hahi":
        hsd.update(synth.make_hahi_state_dict(7242, chans))
    missing, unexpected = model.depth_head.load_state_dict({k: torch.from_numpy(v) for k, v in hsd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    g = torch.Generator().manual_seed(3)
    for mod in model.depth_backbone.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _build_ours(g, family, head, backbone, T, dev):
    """diffusiondepth_amd's head built as the reference facade builds its head (the recorded HEADS.build kwargs, backbone first, same seed)"""
    from diffusiondepth_amd import head as H
    from diffusiondepth_amd.model import Diffusion_DCbase_Model
    args = facade_args(head, backbone, T)
    cfg = json.loads(str(g["build_cfg"]))
    assert cfg["type"] == head and bool(g["init_cfg_is_args"]) and cfg["init_cfg"] is None and len(cfg["loss_cfgs"]) == 2
    cfg["init_cfg"] = args
    torch.manual_seed(INIT_SEED)
    depth_backbone = backbone_factories()[backbone]()                                   # :65-68
    depth_head = H.HEADS[cfg.pop("type")](**cfg)                                        # :91
    model = Diffusion_DCbase_Model(args, depth_backbone=depth_backbone, depth_head=depth_head)
    assert type(model.depth_head).__module__.startswith("diffusiondepth_amd"), "diffusiondepth_amd's head under the reference's registered name"
    load_head_and_bn(model, family)
    sd = model.state_dict()
    want = dict(zip(g["sd_keys"].tolist(), g["sd_sha256"].tolist()))
    assert set(sd) == set(want), set(sd) ^ set(want)                                    # same parameter tree: state_dicts load unchanged
    bad = [k for k, v in sd.items() if _sha(v) != want[k]]
    assert not bad, f"parameters differ from the reference model's: {bad[:8]}"
    return model.to(dev).eval()


def _compare(g, model, sample, tol_pred=1e-3):
    torch.manual_seed(FORWARD_SEED)
    if sample["rgb"].is_cuda:
        torch.cuda.manual_seed_all(FORWARD_SEED)
    with torch.no_grad():
        o = model(sample)
    assert sorted(o) == g["keys"].tolist(), "the 13-key output dict of the reference head (…res.py:171-177)"
    assert sorted(k for k in o if o[k] is None) == g["none_keys"].tolist()
    pred = o["pred"].float().cpu().numpy()
    d_pred = float(np.abs(pred - g["pred"]).max())
    assert np.isfinite(pred).all() and d_pred <= tol_pred, d_pred
    assert float(np.abs(o["pred_init"].float().cpu().numpy() - g["pred_init"]).max()) <= 1e-4 * float(np.abs(g["pred_init"]).max())
    assert abs(float(g["ddim_loss"]) - float(o["ddim_loss"])) <= 1e-3 * max(1.0, abs(float(g["ddim_loss"])))
    return d_pred


def test_reference_facade_builds_and_runs_our_res_head_on_cpu(golden):
    """Res family built as the reference's facade builds it, on CPU tensors (our head: its own torch children; no HIP device here), against the
    facade's recorded result with the reference's head."""
    g = golden("facade_cpu_res")
    our_model = _build_ours(g, "res", "DDIMDepthEstimate_Res", "mmbev_res18", T=5, dev=torch.device("cpu"))
    d = _compare(g, our_model, make_sample(1, 64, 96, torch.device("cpu")))
    assert d <= 1e-4        # (same fp32 torch operators on both sides)


@pytest.mark.gpu
@pytest.mark.parametrize("family,head,backbone,T,hw", [
    ("res", "DDIMDepthEstimate_Res", "mmbev_res18", 20, (96, 160)),
    ("swin_hahi", "DDIMDepthEstimate_Swin_ADDHAHI", "swin_l_standin", 20, (96, 160)),
])
def test_reference_facade_forward_matches_with_our_heads_on_the_gpu(golden, family, head, backbone, T, hw):
    """forward(sample) with the HIP heads built as the reference's facade builds its head, against the facade's recorded result with the reference's
    heads on cuda:0, fp32 (the heads' default profile "reference"): 1e-3 abs on the predicted depth, both head families."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from gpu_util import record
    dev = torch.device("cuda", 0)
    g = golden(f"facade_gpu_{family}")
    our_model = _build_ours(g, family, head, backbone, T, dev)
    d = _compare(g, our_model, make_sample(2, hw[0], hw[1], dev))
    be = our_model.depth_head._bound
    assert be.backend is not None and be.backend.counter("graph_launches") + be.backend.counter("eager_loops") > 0, "the T-step loop ran in the HIP library"
    record(f"reference_facade_{family}", depth_max_abs=d)
