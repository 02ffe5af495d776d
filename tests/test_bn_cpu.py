"""CPU: everything about diffusiondepth_amd.batchnorm that needs no GPU -- the C ABI of include/ddepth_bn.h (declared == bound == exported, the
workspace query and the argument checks), the converter (same tensors, same keys, the fused activation's nn.Identity at the old index), the head
keyword / environment variable, and that on CPU tensors a converted head IS the unconverted one, bit for bit, in .eval() and in .train(), alone
and on two gloo ranks (there the module takes the torch path it inherits and applies its activation behind it)."""
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import batchnorm as BN
from diffusiondepth_amd import dist as ddist
from diffusiondepth_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERTED = ("conv_lateral", "conv_up", "depth_transform", "hahineck", "convup_fp")


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_bn_header_declares_the_bound_symbols_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ddepth_bn.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(BN.ABI_SYMBOLS), declared ^ set(BN.ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    # a header and a binding of their own: nothing leaked into the handle-based ABI
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    assert not any(s in main for s in declared) and not declared & set(backend.ABI_SYMBOLS)


def test_workspace_query_and_argument_checks_need_no_device():
    lib = BN._lib()
    n, small = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.dd_bn_workspace_bytes(4, 256, 176 * 608, ctypes.byref(n)) == 0 and n.value >= 4 * 256 * 2 * 8
    assert lib.dd_bn_workspace_bytes(1, 3, 35, ctypes.byref(small)) == 0 and 0 < small.value < n.value
    assert lib.dd_bn_workspace_bytes(0, 3, 35, ctypes.byref(small)) != 0 and b"positive" in lib.dd_bn_last_error()
    assert lib.dd_bn_workspace_bytes(1, 70000, 35, ctypes.byref(small)) != 0 and b"65535" in lib.dd_bn_last_error()
    assert lib.dd_bn_stats(None, None, None, 1, 3, 35, None) != 0 and b"null" in lib.dd_bn_last_error()
    assert lib.dd_bn_finalize(None, 1e-5, 0.1, None, None, None, 3, None) != 0
    assert lib.dd_bn_apply(None, None, None, None, None, 0, 0.0, 1, 3, 35, None) != 0
    assert lib.dd_bn_backward_reduce(None, None, None, None, None, 0, 0.0, None, None, 1, 3, 35, None) != 0
    assert lib.dd_bn_backward_apply(None, None, None, None, None, None, None, None, 0, 0.0, 1, 3, 35, None) != 0


def test_exports():
    assert dda.HipBatchNorm2d is BN.HipBatchNorm2d and dda.convert_hip_batchnorm is BN.convert_hip_batchnorm


def test_the_function_and_the_six_calls_refuse_cpu_tensors():
    x = torch.randn(2, 3, 4, 5, requires_grad=True)
    rm, rv = torch.zeros(3), torch.ones(3)
    with pytest.raises(RuntimeError, match="HIP device"):
        BN.BatchNormTrainFunction.apply(x, None, None, rm, rv, 1e-5, 0.1, BN.ACT_RELU, 0.0, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        BN.bn_stats(x.detach())
    with pytest.raises(RuntimeError, match="HIP device"):
        BN.bn_apply(x.detach(), torch.zeros(6))


# ---- the converter ------------------------------------------------------------------------------------------------------------------------
def _small_net():
    torch.manual_seed(3)
    net = nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.BatchNorm2d(6), nn.ReLU(True),
                        nn.Sequential(nn.ConvTranspose2d(6, 5, 2, stride=2), nn.BatchNorm2d(5), nn.LeakyReLU(0.2, inplace=True)),
                        nn.Conv2d(5, 4, 1), nn.BatchNorm2d(4), nn.Tanh(), nn.BatchNorm2d(4, affine=False), nn.ReLU6())
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d) and m.affine:
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return net


def test_converter_keeps_tensors_keys_and_indices_and_fuses_only_relu_and_leaky_relu():
    net = _small_net()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    params = [id(p) for p in net.parameters()]
    out = BN.convert_hip_batchnorm(net)
    assert out is net and list(net.state_dict()) == list(before)
    assert {k: v.data_ptr() for k, v in net.state_dict().items()} == before and [id(p) for p in net.parameters()] == params
    assert not any(type(m) is nn.BatchNorm2d for m in net.modules())
    assert isinstance(net[1], BN.HipBatchNorm2d) and net[1].activation == "relu" and type(net[2]) is nn.Identity
    assert net[3][1].activation == "leaky_relu" and net[3][1].negative_slope == 0.2 and type(net[3][2]) is nn.Identity
    assert net[5].activation is None and type(net[6]) is nn.Tanh                       # not a fusable activation: left alone
    assert net[7].activation is None and type(net[8]) is nn.ReLU6 and not net[7].affine
    again = BN.convert_hip_batchnorm(net)                                              # idempotent
    assert again is net and net[1].activation == "relu"
    unfused = BN.convert_hip_batchnorm(_small_net(), fuse_activation=False)
    assert unfused[1].activation is None and type(unfused[2]) is nn.ReLU
    # a later SyncBN conversion leaves the modules in place; a SyncBatchNorm met by the converter is taken over with its group
    mods = [m for m in net.modules() if isinstance(m, BN.HipBatchNorm2d)]
    assert ddist.convert_sync_batchnorm(net) is net and [m for m in net.modules() if isinstance(m, BN.HipBatchNorm2d)] == mods
    sync = ddist.convert_sync_batchnorm(_small_net(), process_group="G")
    conv = BN.convert_hip_batchnorm(sync)
    assert isinstance(conv[1], BN.HipBatchNorm2d) and conv[1].process_group == "G" and conv[1].activation == "relu"
    with pytest.raises(ValueError):
        BN.HipBatchNorm2d(4, activation="gelu")


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_converted_net_on_cpu_tensors_is_the_unconverted_one_bit_for_bit(train):
    a, b = _small_net().train(train), BN.convert_hip_batchnorm(_small_net()).train(train)
    x = torch.randn(4, 3, 7, 9, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    (ya ** 2).sum().backward()
    (yb ** 2).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(a.buffers(), b.buffers()))
    if train:
        assert int(b[1].num_batches_tracked) == 1
        with pytest.raises(ValueError, match="4D"):
            b[1](torch.randn(4, 6))


# ---- heads --------------------------------------------------------------------------------------------------------------------------------
def _pair(cls, **kw):
    torch.manual_seed(0)
    a = cls(bn_backend="torch", **kw)
    b = cls(bn_backend="hip", **kw)
    b.load_state_dict(a.state_dict())                 # strict: the keys are the same
    return a, b


def _bn_census(head):
    return [(n, type(m)) for n, m in head.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm) and n.split(".")[0] in CONVERTED]


def test_bn_backend_keyword_and_environment_variable(monkeypatch):
    monkeypatch.delenv("DDEPTH_BN_BACKEND", raising=False)
    assert dda.DDIMDepthEstimate_Res(inference_steps=2).bn_backend == "torch"
    monkeypatch.setenv("DDEPTH_BN_BACKEND", "")
    plain = dda.DDIMDepthEstimate_Res(inference_steps=2)
    assert plain.bn_backend == "torch" and all(t is nn.BatchNorm2d for _, t in _bn_census(plain))
    monkeypatch.setenv("DDEPTH_BN_BACKEND", "hip")
    head = dda.DDIMDepthEstimate_Res(inference_steps=2)
    assert head.bn_backend == "hip" and len(_bn_census(head)) == 11 and all(t is BN.HipBatchNorm2d for _, t in _bn_census(head))
    assert dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="torch").bn_backend == "torch"      # the keyword wins
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="miopen")


def test_res_head_conversion_keeps_keys_and_the_parameter_intake():
    a, b = _pair(dda.DDIMDepthEstimate_Res, inference_steps=2)
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in _bn_census(a)] == [n for n, _ in _bn_census(b)]
    assert all(t is BN.HipBatchNorm2d for _, t in _bn_census(b))
    # the fused activations: nn.Identity at the old index, the activation inside the BatchNorm
    assert type(b.conv_lateral[0][2]) is nn.Identity and b.conv_lateral[0][1].activation == "relu"
    assert type(b.conv_up[0][2]) is nn.Identity and type(b.convup_fp[2]) is nn.Identity
    enc = b.depth_transform.conv_transform
    assert enc[0][1].activation == "leaky_relu" and enc[0][1].negative_slope == 0.2 and type(enc[0][2]) is nn.Identity
    assert enc[1][1].activation is None                                             # (followed by Tanh one level up)
    assert b.depth_transform.conv_inv_transform[1].activation == "relu"
    # what the library's eval-mode parameter intake walks is unchanged: same groups, same number of tensors, live signatures
    for group in ("fpn", "codec"):
        assert len(a._bound._signature(group)) == len(b._bound._signature(group)) > 0
    # dist.convert_sync_batchnorm afterwards: nothing moves
    census = _bn_census(b)
    assert ddist.convert_sync_batchnorm(b) is b and _bn_census(b) == census


def test_swin_hahi_head_conversion_keeps_keys():
    a, b = _pair(dda.DDIMDepthEstimate_Swin_ADDHAHI, in_channels=[192, 384, 768, 1536], inference_steps=2)
    assert list(a.state_dict()) == list(b.state_dict())
    census = _bn_census(b)
    assert any(n.startswith("hahineck.") for n, _ in census) and all(t is BN.HipBatchNorm2d for _, t in census)
    assert [n for n, _ in _bn_census(a)] == [n for n, _ in census]
    assert len(a._bound._signature("fpn")) == len(b._bound._signature("fpn"))


def _head_inputs(B=2, H=32, W=64):
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W)]
    gt = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(2)) * 60.0 + 1.0
    return fp, gt


def test_res_head_eval_forward_on_cpu_is_bit_identical_after_conversion():
    a, b = _pair(dda.DDIMDepthEstimate_Res, inference_steps=2)
    a.eval(), b.eval()
    fp, gt = _head_inputs()
    outs = []
    for head in (a, b):
        torch.manual_seed(7)
        with torch.no_grad():
            outs.append(head(fp, gt, gt > 0, gt_depth_map=gt))
    for k in ("pred", "gt_map_t", "ddim_loss"):
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_res_head_train_forward_and_backward_on_cpu_are_bit_identical_after_conversion():
    a, b = _pair(dda.DDIMDepthEstimate_Res, inference_steps=2)
    a.train(), b.train()
    fp, gt = _head_inputs()
    res = []
    for head in (a, b):
        torch.manual_seed(7)
        f = [t.clone().requires_grad_(True) for t in fp]
        out = head(f, gt, gt > 0, gt_depth_map=gt)
        (out["pred"].mean() + out["ddim_loss"] + out["gt_map_t"].mean()).backward()
        res.append((out, f))
    for k in ("pred", "gt_map_t", "ddim_loss"):
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(res[0][1], res[1][1]))
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(ga) == list(gb)
    for k in ga:
        assert (ga[k].grad is None) == (gb[k].grad is None) and (ga[k].grad is None or torch.equal(ga[k].grad, gb[k].grad)), k
    assert any(g.grad is not None for k, g in gb.items() if k.startswith("conv_lateral.0.1."))
    for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(u, v), k


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gloo_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    ddist.init_from_env("gloo")
    ref = ddist.convert_sync_batchnorm(_small_net()).train()
    new = BN.convert_hip_batchnorm(_small_net()).train()
    x = torch.randn(6, 3, 7, 9, generator=torch.Generator().manual_seed(1)) * 2.0 + 0.5
    sl = slice(0, 4) if rank == 0 else slice(4, 6)               # uneven shards
    xa, xb = x[sl].clone().requires_grad_(True), x[sl].clone().requires_grad_(True)
    ya, yb = ref(xa), new(xb)
    (ya ** 2).sum().backward()
    (yb ** 2).sum().backward()
    same = (torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
            and all(torch.equal(p.grad, q.grad) for p, q in zip(ref.parameters(), new.parameters()))
            and all(torch.equal(p, q) for p, q in zip(ref.buffers(), new.buffers())))
    # ... and the statistics really were the global batch's: the local ones differ
    local = nn.functional.batch_norm(ref[0](x[sl]), None, None, ref[1].weight, ref[1].bias, True, 0.0, ref[1].eps).relu()
    exchanged = not torch.allclose(local, new[2](new[1](new[0](x[sl]))), atol=1e-3)
    torch.save({"same": bool(same), "exchanged": bool(exchanged)}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_of_a_converted_module_equal_sync_batchnorm(tmp_path):
    out = str(tmp_path / "hipbn.pt")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    for rank in (0, 1):
        r = torch.load(out + f".{rank}")
        assert r["same"] and r["exchanged"], (rank, r)
