"""CPU: the C-ABI library loads and exports every symbol include/ddepth.h declares; the host-side
mirrors behave like the reference's (scheduler tables / timesteps / step / add_noise vs golden,
state_dict key names).  No compute calls into the library here (no GPU in this container)."""
import os
import re

import numpy as np
import pytest
import torch

import diffusiondepth_amd as dda
from diffusiondepth_amd import synth
from diffusiondepth_amd.backend import ABI_SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ABI_SYMBOLS), declared ^ set(ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.dd_version()


def test_create_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dda.HipDenoiser()
    head = dda.DDIMDepthEstimate_Res().eval()
    # the LIBRARY has no CPU path: asking the binding for a backend on a CPU device raises ...
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head._bound.ensure("cpu")
    # ... tensors that are not on a HIP device never reach it: they run the module's own torch children in eager mode (BASELINE
    # configs[0] "plumbing, no GPU"; tests/test_heads_cpu.py holds that path to the reference golden).  HIP tensors have no such alternative.
    with torch.no_grad():
        lat = head.depth_transform.t(torch.zeros(1, 1, 8, 8))
    assert lat.shape == (1, 16, 4, 4) and head._bound.backend is None


def test_scheduler_matches_reference_tables(golden):
    g = golden("sched")
    s = dda.DDIMScheduler(num_train_timesteps=1000, clip_sample=False)
    assert np.array_equal(s.alphas_cumprod.numpy(), g["alphas_cumprod"])
    assert np.array_equal(s.betas.numpy(), g["betas"])
    for T in (5, 20, 50):
        s.set_timesteps(T)
        assert np.array_equal(s.timesteps.numpy(), g[f"timesteps_T{T}"])
    assert s.hip_supported(0.0) is None and s.hip_supported(0.5) is not None


def test_scheduler_cosine_schedule_matches_the_reference_class(golden):
    """beta_schedule="squaredcos_cap_v2" (reference scheduling_ddim.py:137-139, betas_for_alpha_bar :67-94): no head uses it, the mirror carries it so
    that the scheduler interface has no hole.  Compared with what the reference's own class computed (tests/golden/sched_cosine.npz, minted by
    tests/golden/make_golden.py), bit for bit."""
    g = golden("sched_cosine")
    for n in (1000, 250):
        s = dda.DDIMScheduler(num_train_timesteps=n, beta_schedule="squaredcos_cap_v2", clip_sample=False)
        assert s.betas.dtype == torch.float32 and s.alphas_cumprod.dtype == torch.float32
        assert np.array_equal(s.betas.numpy(), g[f"betas_n{n}"]) and np.array_equal(s.alphas_cumprod.numpy(), g[f"alphas_cumprod_n{n}"])
        s.set_timesteps(20)
        assert np.array_equal(np.asarray(s.timesteps), g[f"timesteps_n{n}_T20"])


def test_scheduler_step_and_add_noise_match_reference(golden, cases):
    c, g = cases["sched"], golden("sched")
    rs = np.random.RandomState(c["seed"])
    x = torch.from_numpy(rs.standard_normal(c["shape"]).astype(np.float32))
    eps = torch.from_numpy(np.abs(rs.standard_normal(c["shape"])).astype(np.float32))
    s = dda.DDIMScheduler()
    s.set_timesteps(20)
    for i, t in enumerate(s.timesteps):
        out = s.step(eps, t, x, eta=0.0, use_clipped_model_output=True)["prev_sample"]
        assert torch.equal(out, torch.from_numpy(g["step_T20"][i]))          # same formula order -> same bits
    B = len(c["add_noise_t"])
    x0 = torch.from_numpy(rs.standard_normal((B,) + tuple(c["shape"][1:])).astype(np.float32))
    nz = torch.from_numpy(rs.standard_normal((B,) + tuple(c["shape"][1:])).astype(np.float32))
    assert torch.equal(s.add_noise(x0, nz, torch.tensor(c["add_noise_t"])), torch.from_numpy(g["add_noise"]))


def test_head_state_dict_keys_match_reference_names():
    head = dda.DDIMDepthEstimate_Res()
    keys = {k for k in head.state_dict() if not k.endswith("num_batches_tracked")}
    want = set(synth.make_state_dict(1)) | set(synth.make_fpn_state_dict(1))
    assert keys == want, keys ^ want
    for k, v in synth.make_state_dict(1).items():
        assert tuple(head.state_dict()[k].shape) == v.shape, k


def test_model_facade_builds_and_names_backbones():
    m = dda.Diffusion_DCbase_Model(dda.model.default_args(backbone_name="mmbev_res18", inference_steps=5))
    assert m.depth_head.diffusion_inference_steps == 5
    feats = m.depth_backbone(torch.zeros(1, 3, 32, 48))
    assert [f.shape[1] for f in feats] == [64, 128, 256, 512]
    assert [tuple(f.shape[-2:]) for f in feats] == [(16, 24), (8, 12), (4, 6), (2, 3)]


def test_graph_replay_only_where_the_runtimes_graph_fast_path_was_switched_off_in_time():
    """Round 6 (profiles/r06_experiments.md section 10): the HIP runtime reads DEBUG_CLR_GRAPH_PACKET_CAPTURE once, at its first HIP call -- which may be as little as
    torch.cuda.is_available().  The package therefore replays hipGraphs only when the variable was ALREADY "0" in the process's environment at import
    (GRAPH_REPLAY_SAFE: the job exported it; bench.py and this session's conftest set it in their first lines, before torch is imported); otherwise it exports the
    variable for what it is worth and its handles enqueue their loops eagerly.  The caller's own value is never overwritten."""
    import subprocess, sys
    code = ("import os, sys; sys.path.insert(0, %r); import diffusiondepth_amd as d; "
            "print(d.GRAPH_REPLAY_SAFE, os.environ.get('DEBUG_CLR_GRAPH_PACKET_CAPTURE'))" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "DEBUG_CLR_GRAPH_PACKET_CAPTURE"}
    run = lambda e: subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
    assert run(env) == "False 0"
    assert run(dict(env, DEBUG_CLR_GRAPH_PACKET_CAPTURE="0")) == "True 0"
    assert run(dict(env, DEBUG_CLR_GRAPH_PACKET_CAPTURE="1")) == "False 1"
    assert dda.GRAPH_REPLAY_SAFE and os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0"          # this session: tests/conftest.py, first lines
    top = open(os.path.join(ROOT, "bench.py")).read().split("import torch")[0]
    assert 'os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")' in top                        # bench.py: before torch is imported
    assert "setdefault(\"DEBUG_CLR_GRAPH_PACKET_CAPTURE\"" not in open(os.path.join(ROOT, "__graft_entry__.py")).read()      # an entry point imported by others cannot know
