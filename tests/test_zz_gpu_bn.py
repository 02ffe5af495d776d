"""GPU (`-m gpu`): the batch-statistics BatchNorm of include/ddepth_bn.h / diffusiondepth_amd.batchnorm on the MI355X.

Every compared tensor is held to the rule of tests/bn_cases.py: max|hip - ref64| <= 4 * max(max|ref32 - ref64|, 2^-23 max|ref64|) against the torch
CPU evaluation of F.batch_norm(training=True) + activation and its autograd; activation cases are built with min|z64| >= 1e-4 and compared
without exclusions.  Beyond that: bitwise repeatability, no host synchronisation, the split ABI used as an exchange between two "ranks" without a
process group, a one-rank RCCL group, and a Res head in .train() against the same head on MIOpen's BatchNorm."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_cases as BC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23


def _module(shape, act, affine, kind):
    from diffusiondepth_amd import batchnorm as BN
    inp = BC.make_inputs(shape, act, affine, kind)
    m = BN.HipBatchNorm2d(shape[1], eps=BC.EPS, momentum=BC.MOMENTUM, affine=affine, activation={"none": None, "relu": "relu", "leaky": "leaky_relu"}[act],
                          negative_slope=BC.ACTS[act][1])
    with torch.no_grad():
        if affine:
            m.weight.copy_(inp["weight"])
            m.bias.copy_(inp["bias"])
        m.running_mean.copy_(inp["running_mean"])
        m.running_var.copy_(inp["running_var"])
    return m.cuda().train(), inp


def _run_module(shape, act, affine, kind):
    m, inp = _module(shape, act, affine, kind)
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    y = m(x)
    y.backward(inp["grad_y"].cuda())
    assert int(m.num_batches_tracked) == 1
    return {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(),
            "grad_weight": m.weight.grad.cpu().numpy() if affine else None, "grad_bias": m.bias.grad.cpu().numpy() if affine else None,
            "running_mean": m.running_mean.cpu().numpy(), "running_var": m.running_var.cpu().numpy()}


@pytest.mark.parametrize("variant", BC.VARIANTS, ids=BC.variant_id)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=str)
def test_module_forward_and_backward_against_torch_cpu(shape, variant):
    act, affine, kind = variant
    BC.check(_run_module(shape, act, affine, kind), shape, act, affine, kind, "gpu")


@pytest.mark.parametrize("shape", [BC.SHAPES[1], BC.SHAPES[2]], ids=str)
def test_two_runs_give_the_same_bits(shape):
    a, b = _run_module(shape, "leaky", True, "normal"), _run_module(shape, "leaky", True, "normal")
    for k in BC.KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_forward_and_backward_do_not_synchronise_the_host():
    m, inp = _module(BC.SHAPES[2], "relu", True, "normal")
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    m(x).backward(gy)                       # (the first call loads the library and allocates the workspace)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = m(x)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and int(m.num_batches_tracked) == 2


def test_a_single_value_per_channel_raises_as_in_torch():
    from diffusiondepth_amd import batchnorm as BN
    m = BN.HipBatchNorm2d(3).cuda().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.randn(1, 3, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        torch.nn.BatchNorm2d(3).cuda().train()(torch.randn(1, 3, 1, 1, device="cuda"))


def test_non_contiguous_and_half_inputs_take_the_torch_path():
    """No silent copy or conversion: such inputs run torch's BatchNorm and the module's own activation, and equal nn.BatchNorm2d + ReLU."""
    from diffusiondepth_amd import batchnorm as BN
    torch.manual_seed(0)
    m = BN.HipBatchNorm2d(8, activation="relu").cuda().train()
    ref = torch.nn.Sequential(torch.nn.BatchNorm2d(8), torch.nn.ReLU()).cuda().train()
    for x in (torch.randn(2, 6, 5, 8, device="cuda").permute(0, 3, 1, 2), torch.randn(2, 8, 5, 6, device="cuda").half()):
        assert torch.equal(m(x), ref(x))


@pytest.mark.parametrize("shape", [(4, 3, 5, 7), (4, 16, 11, 19), (4, 4, 67, 131)], ids=str)
def test_the_split_abi_as_an_exchange_between_two_halves_of_a_batch(shape):
    """A batch of 4 treated as two ranks of 2: dd_bn_stats per half, the two `sums` added on the device (what an all-reduce does), finalize and
    apply per half; the same for the backward.  y and grad_x must equal the whole-batch calls to 2^-22 relative per element: the fp64 sums are
    only reordered, and one fp32 rounding follows."""
    from diffusiondepth_amd import batchnorm as BN
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    x, gy = (torch.randn(shape, generator=g) * 1.5 + 0.3).cuda(), torch.randn(shape, generator=g).cuda()
    w, b = (0.5 + torch.rand(C, generator=g)).cuda(), torch.randn(C, generator=g).cuda()
    act, slope = BN.ACT_LEAKY_RELU, 0.2
    # the whole batch
    sums = BN.bn_stats(x)
    mi = BN.bn_finalize(sums, BC.EPS)
    y = BN.bn_apply(x, mi, w, b, act, slope)
    sums2 = BN.bn_backward_reduce(x, gy, mi, w, b, act, slope)
    gx = BN.bn_backward_apply(x, gy, mi, sums2, sums, w, b, act, slope)
    # two "ranks"
    halves = [(x[:2].contiguous(), gy[:2].contiguous()), (x[2:].contiguous(), gy[2:].contiguous())]
    part = [BN.bn_stats(xh) for xh, _ in halves]
    assert float(part[0][2 * C]) == 2 * shape[2] * shape[3]
    ex = part[0] + part[1]                                   # the exchange
    assert float(ex[2 * C]) == float(sums[2 * C])
    mi_h = BN.bn_finalize(ex, BC.EPS)
    y_h = torch.cat([BN.bn_apply(xh, mi_h, w, b, act, slope) for xh, _ in halves])
    part2 = [BN.bn_backward_reduce(xh, gh, mi_h, w, b, act, slope) for xh, gh in halves]
    ex2 = part2[0] + part2[1]
    gx_h = torch.cat([BN.bn_backward_apply(xh, gh, mi_h, ex2, ex, w, b, act, slope) for xh, gh in halves])
    for name, got, want in (("y", y_h, y), ("grad_x", gx_h, gx)):
        rel = ((got - want).abs() / want.abs().clamp_min(1e-30)).max().item()
        print(f"split-abi {shape} {name}: max relative difference {rel:.3e}")
        assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs()).all()), (name, rel)
    # the local sums2 are the parameter gradients of each half: together the whole batch's
    assert torch.allclose(ex2, sums2, rtol=1e-12, atol=1e-12)


RCCL_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, os.environ["DD_ROOT"]); sys.path.insert(0, os.path.join(os.environ["DD_ROOT"], "tests"))
import torch.distributed as dist
import bn_cases as BC
from diffusiondepth_amd import batchnorm as BN, dist as ddist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
ddist.SyncBatchNorm.force_sync = True                       # one rank, but through the all-reduces
calls = []
real = dist.all_reduce
def counting(t, *a, **k):
    calls.append((t.dtype, t.numel()))
    return real(t, *a, **k)
dist.all_reduce = counting
shape, act, affine, kind = BC.SHAPES[1], "leaky", True, "normal"
inp = BC.make_inputs(shape, act, affine, kind)
net = torch.nn.Sequential(torch.nn.BatchNorm2d(shape[1], eps=BC.EPS, momentum=BC.MOMENTUM), torch.nn.LeakyReLU(0.2))
with torch.no_grad():
    net[0].weight.copy_(inp["weight"]); net[0].bias.copy_(inp["bias"])
    net[0].running_mean.copy_(inp["running_mean"]); net[0].running_var.copy_(inp["running_var"])
net = BN.convert_hip_batchnorm(net).cuda().train()
m = net[0]
assert isinstance(m, BN.HipBatchNorm2d) and m._exchanges()
x = inp["x"].detach().clone().cuda().requires_grad_(True)
y = net(x)
y.backward(inp["grad_y"].cuda())
C = shape[1]
assert calls == [(torch.float64, 2 * C + 1), (torch.float64, 2 * C)], calls      # one fp64 collective per direction
BC.check({"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_weight": m.weight.grad.cpu().numpy(),
          "grad_bias": m.bias.grad.cpu().numpy(), "running_mean": m.running_mean.cpu().numpy(), "running_var": m.running_var.cpu().numpy()},
         shape, act, affine, kind, "rccl-one-rank")
dist.barrier(); dist.destroy_process_group()
print("HIPBN-RCCL-ONE-RANK-OK")
"""


def test_one_rank_rccl_group_with_force_sync_against_fp64():
    with socket.socket() as s:
        s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        s.bind(("127.0.0.1", 0))
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]), RANK="0", WORLD_SIZE="1", DD_ROOT=ROOT,
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run([sys.executable, "-c", RCCL_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "HIPBN-RCCL-ONE-RANK-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- head level ---------------------------------------------------------------------------------------------------------------------------
def _head_step(head, fp, gt, lat, ups, dev, dtype):
    """aggregate_condition, depth_transform.t and inv_t of a .train() head, each with its upstream gradient; -> dict name -> fp64 numpy."""
    head = head.to(dev).train()
    head.zero_grad()
    f = [t.to(dev, dtype).clone().requires_grad_(True) for t in fp]
    g = gt.to(dev, dtype).clone().requires_grad_(True)
    z = lat.to(dev, dtype).clone().requires_grad_(True)
    cond = head.aggregate_condition(f)
    enc = head.depth_transform.t(g)
    dec = head.depth_transform.inv_t(z)
    torch.autograd.backward([cond, enc, dec], [u.to(dev, dtype) for u in ups])
    out = {"cond": cond, "enc": enc, "dec": dec, "grad_gt": g.grad, "grad_latent": z.grad}
    out.update({f"grad_fp{i}": t.grad for i, t in enumerate(f)})
    tracked = ("conv_lateral.", "conv_up.", "depth_transform.")
    out.update({"grad:" + k: p.grad for k, p in head.named_parameters() if k.startswith(tracked) and p.grad is not None})
    out.update({"buf:" + k: v for k, v in head.named_buffers() if k.startswith(tracked) and k.endswith(("running_mean", "running_var"))})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def test_res_head_in_train_mode_against_the_same_head_on_torch_batchnorm():
    """Convolution error is outside this module, so the bound is measured here: per tensor, the error of bn_backend="hip" against the fp64 CPU
    evaluation must be <= 2 x the error of bn_backend="torch" on the GPU for the same inputs (floor 2^-23 max|ref64|).  The factor covers
    reordered fp32 rounding in a path that shares the convolutions and only widens an accumulation."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    torch.manual_seed(0)
    a = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="torch")
    b = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip")
    r = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="torch")
    b.load_state_dict(a.state_dict())
    r.load_state_dict(a.state_dict())
    r = r.double()
    B, H, W = 2, 32, 64
    g = torch.Generator().manual_seed(5)
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W)]
    gt = torch.rand(B, 1, H, W, generator=g) * 60.0 + 1.0
    lat = torch.randn(B, 16, H // 2, W // 2, generator=g)
    ups = [torch.randn(B, 256, H // 2, W // 2, generator=g), torch.randn(B, 16, H // 2, W // 2, generator=g), torch.randn(B, 1, H, W, generator=g)]
    ref = _head_step(r, fp, gt, lat, ups, "cpu", torch.float64)
    tor = _head_step(a, fp, gt, lat, ups, "cuda", torch.float32)
    from diffusiondepth_amd import batchnorm as BN
    native, real = [], BN.bn_stats
    BN.bn_stats = lambda x: (native.append(tuple(x.shape)), real(x))[1]
    try:
        hip = _head_step(b, fp, gt, lat, ups, "cuda", torch.float32)
    finally:
        BN.bn_stats = real
    assert len(native) == 10, native        # the ten BatchNorm sites of a Res head all ran in the library
    assert set(ref) == set(tor) == set(hip) and any(k.startswith("grad:conv_lateral.0.1.") for k in ref) and any(k.startswith("buf:") for k in ref)
    failures = []
    for k in sorted(ref):
        e_t, e_h = float(np.max(np.abs(tor[k] - ref[k]))), float(np.max(np.abs(hip[k] - ref[k])))
        bnd = max(2.0 * e_t, ULP * float(np.max(np.abs(ref[k]))))
        print(f"head {k}: torch {e_t:.3e} hip {e_h:.3e} bound {bnd:.3e}")
        if not e_h <= bnd:
            failures.append((k, e_t, e_h, bnd))
    assert not failures, failures
