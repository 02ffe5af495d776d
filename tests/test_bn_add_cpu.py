"""CPU: everything about the BatchNorm with an addend that needs no GPU -- the C ABI of include/ddepth_bn_add.h (declared == bound == exported, apart
from the other headers), the autograd Function's refusal of CPU tensors, ``fuse_basic_block_tails`` (same tensors, same keys, idempotent, other
blocks left alone), the two facade values ``backbone_backend="hip+bn"`` and ``bn_backend="hip+add"``, and that on CPU tensors a fused backbone and
a "hip+add" head ARE the unconverted ones, bit for bit (there the modules take their torch path and add behind or in front of their activation)."""
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import batchnorm as BN
from diffusiondepth_amd import model as M
from diffusiondepth_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\("


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_add_header_declares_the_bound_symbols_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ddepth_bn_add.h")).read()
    declared = set(re.findall(DECL, hdr, flags=re.M))
    assert declared == set(BN.ADD_ABI_SYMBOLS), declared ^ set(BN.ADD_ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    # a header of its own: disjoint from the handle-based ABI and from ddepth_bn.h, whose symbol set stays what it was
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    bn = set(re.findall(DECL, open(os.path.join(ROOT, "include", "ddepth_bn.h")).read(), flags=re.M))
    assert not any(s in main for s in declared) and not declared & set(backend.ABI_SYMBOLS)
    assert not declared & bn and not declared & set(BN.ABI_SYMBOLS) and bn == set(BN.ABI_SYMBOLS)
    assert "DD_BN_ADD_PRE = 0" in hdr and "DD_BN_ADD_POST = 1" in hdr and (BN.ADD_PRE, BN.ADD_POST) == (0, 1)


def test_argument_checks_need_no_device():
    lib = BN._lib()
    assert lib.dd_bn_apply_add(None, None, None, None, None, None, 0, 0.0, 0, 1, 3, 35, None) != 0 and b"null" in lib.dd_bn_last_error()
    assert lib.dd_bn_backward_reduce_add(None, None, None, None, 0, 0.0, None, None, None, 1, 3, 35, None) != 0 and b"null" in lib.dd_bn_last_error()


def test_exports():
    assert dda.fuse_basic_block_tails is M.fuse_basic_block_tails and "fuse_basic_block_tails" in dda.__all__


def test_the_function_and_the_two_calls_refuse_cpu_tensors():
    x, r = torch.randn(2, 3, 4, 5, requires_grad=True), torch.randn(2, 3, 4, 5, requires_grad=True)
    rm, rv = torch.zeros(3), torch.ones(3)
    for mode in (BN.ADD_PRE, BN.ADD_POST):
        with pytest.raises(RuntimeError, match="HIP device"):
            BN.BatchNormAddTrainFunction.apply(x, r, None, None, rm, rv, 1e-5, 0.1, BN.ACT_RELU, 0.0, mode, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        BN.bn_apply_add(x.detach(), torch.zeros(6), r.detach())
    with pytest.raises(RuntimeError, match="HIP device"):
        BN.bn_backward_reduce_add(x.detach(), r.detach(), r.detach(), torch.zeros(6))


@pytest.mark.parametrize("mode", ["pre", "post"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_the_module_with_an_addend_on_cpu_tensors_is_the_torch_expression(train, mode):
    torch.manual_seed(1)
    ref = nn.BatchNorm2d(5).train(train)
    m = BN.HipBatchNorm2d(5, activation="leaky_relu", negative_slope=0.2).train(train)
    m.add_mode = mode
    m.load_state_dict(ref.state_dict())
    x, r = torch.randn(3, 5, 4, 6), torch.randn(3, 5, 4, 6)
    act = nn.LeakyReLU(0.2)
    want = act(ref(x) + r) if mode == "pre" else act(ref(x)) + r
    assert torch.equal(m(x, addend=r), want) and torch.equal(m.running_var, ref.running_var)
    assert torch.equal(m(x, r), want)                             # positional too
    m.add_mode = "sideways"
    with pytest.raises(ValueError, match="add_mode"):
        m(x, addend=r)
    assert torch.equal(m(x), act(ref(x)))                         # without an addend the attribute is not read


# ---- fuse_basic_block_tails ---------------------------------------------------------------------------------------------------------------
def _backbone(seed=3):
    torch.manual_seed(seed)
    net = M.BACKBONES["mmbev_res18"]()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return net


def _blocks(net):
    return [m for m in net.modules() if isinstance(m, M._BasicBlock)]


def test_fuse_basic_block_tails_keeps_tensors_and_keys_is_idempotent_and_leaves_unconverted_blocks_alone():
    net = _backbone()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    params = [id(p) for p in net.parameters()]
    assert all(not b.fused_tail for b in _blocks(net))
    assert M.fuse_basic_block_tails(net) is net                                     # torch BatchNorms: nothing to fuse
    assert all(not b.fused_tail and type(b.bn1) is nn.BatchNorm2d for b in _blocks(net))
    # one block converted by hand, the rest not: only that one is fused
    first = _blocks(net)[0]
    first.bn1, first.bn2 = BN.convert_hip_batchnorm(first.bn1), BN.convert_hip_batchnorm(first.bn2)
    M.fuse_basic_block_tails(net)
    assert [b.fused_tail for b in _blocks(net)] == [True] + [False] * 7
    out = M.fuse_basic_block_tails(BN.convert_hip_batchnorm(net))
    assert out is net and len(_blocks(net)) == 8
    for b in _blocks(net):
        assert b.fused_tail and isinstance(b.bn1, BN.HipBatchNorm2d) and isinstance(b.bn2, BN.HipBatchNorm2d)
        assert b.bn1.activation == "relu" and b.bn2.activation == "relu" and b.bn2.add_mode == "pre" and type(b.relu) is nn.ReLU
    assert list(net.state_dict()) == list(before) and {k: v.data_ptr() for k, v in net.state_dict().items()} == before
    assert [id(p) for p in net.parameters()] == params
    census = [(n, type(m)) for n, m in net.named_modules()]
    assert M.fuse_basic_block_tails(net) is net and [(n, type(m)) for n, m in net.named_modules()] == census      # idempotent
    assert all(b.fused_tail and b.bn1.activation == "relu" for b in _blocks(net))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_fused_backbone_on_cpu_tensors_is_the_unconverted_one_bit_for_bit(train):
    a = _backbone().train(train)
    b = M.fuse_basic_block_tails(BN.convert_hip_batchnorm(_backbone())).train(train)
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    fa, fb = a(xa), b(xb)
    assert len(fa) == len(fb) == 4 and all(torch.equal(u, v) for u, v in zip(fa, fb))
    sum((f ** 2).sum() for f in fa).backward()
    sum((f ** 2).sum() for f in fb).backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(a.buffers(), b.buffers()))
    if train:
        assert int(_blocks(b)[0].bn2.num_batches_tracked) == 1


# ---- the two facade values ------------------------------------------------------------------------------------------------------------------
def _model(**args):
    return M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, **args))


def test_backbone_backend_hip_bn_keyword_environment_variable_and_value_error(monkeypatch):
    from diffusiondepth_amd.conv import HipConv2d
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND", raising=False)
    plain = _model(precision="bf16")
    for extra, convs in (({"precision": "bf16"}, True), ({"precision": "fp32"}, False), ({}, False)):      # BatchNorm is fp32: at every precision
        m = _model(backbone_backend="hip+bn", **extra)
        assert m.backbone_backend == "hip+bn" and list(m.state_dict()) == list(plain.state_dict())
        bns = [c for c in m.depth_backbone.modules() if isinstance(c, nn.modules.batchnorm._BatchNorm)]
        assert len(bns) == 16 and all(isinstance(c, BN.HipBatchNorm2d) for c in bns)
        assert all(b.fused_tail for b in _blocks(m.depth_backbone))
        assert any(isinstance(c, HipConv2d) for c in m.depth_backbone.modules()) == convs      # what "hip" does for the convolutions
    monkeypatch.setenv("DDEPTH_BACKBONE_BACKEND", "hip+bn")
    assert _model(precision="bf16").backbone_backend == "hip+bn"
    assert _model(precision="bf16", backbone_backend="hip").backbone_backend == "hip"      # the keyword wins
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND")
    # "torch" and "hip" are what they were: no BatchNorm of the backbone is touched
    for choice in ("torch", "hip"):
        m = _model(precision="bf16", backbone_backend=choice)
        assert not any(isinstance(c, BN.HipBatchNorm2d) for c in m.depth_backbone.modules()) and not any(b.fused_tail for b in _blocks(m.depth_backbone))
    for bad in ("hip+add", "bn", "hip+"):
        with pytest.raises(ValueError, match="backbone_backend"):
            _model(precision="bf16", backbone_backend=bad)


def test_bn_backend_hip_add_keyword_environment_variable_and_value_error(monkeypatch):
    monkeypatch.delenv("DDEPTH_BN_BACKEND", raising=False)
    head = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip+add")
    assert head.bn_backend == "hip+add"
    assert all(isinstance(l[1], BN.HipBatchNorm2d) and l[1].add_mode == "post" and l[1].activation == "relu" for l in head.conv_lateral)
    assert all(u[1].add_mode == "pre" for u in head.conv_up)
    hip = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip")
    assert list(hip.state_dict()) == list(head.state_dict()) and all(l[1].add_mode == "pre" for l in hip.conv_lateral)
    assert [(n, type(m)) for n, m in hip.named_modules()] == [(n, type(m)) for n, m in head.named_modules()]
    monkeypatch.setenv("DDEPTH_BN_BACKEND", "hip+add")
    assert dda.DDIMDepthEstimate_Res(inference_steps=2).bn_backend == "hip+add"
    assert dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip").bn_backend == "hip"
    monkeypatch.delenv("DDEPTH_BN_BACKEND")
    for bad in ("hip+bn", "add", "hip+"):
        with pytest.raises(ValueError, match="bn_backend"):
            dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend=bad)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("size", [(32, 64), (36, 68)], ids=["even", "odd"])
def test_hip_add_res_head_on_cpu_is_the_torch_head_bit_for_bit(size, train):
    """(36, 68): the pyramid is 18x34, 9x17, 5x9, 3x5 -- conv_up's 2x map is larger than the lateral one at two levels, and the pool averages."""
    torch.manual_seed(0)
    a = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="torch")
    b = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip+add")
    b.load_state_dict(a.state_dict())
    a.train(train), b.train(train)
    H, W = size
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, 2, H, W)]
    if size == (36, 68):
        assert any(2 * fp[i + 1].shape[-1] != fp[i].shape[-1] or 2 * fp[i + 1].shape[-2] != fp[i].shape[-2] for i in range(3))
    res = []
    for head in (a, b):
        f = [t.clone().requires_grad_(True) for t in fp]
        cond = head.aggregate_condition(f)
        (cond ** 2).sum().backward()
        res.append((cond, f))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(res[0][1], res[1][1]))
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert (ga[k].grad is None) == (gb[k].grad is None) and (ga[k].grad is None or torch.equal(ga[k].grad, gb[k].grad)), k
    assert any(g.grad is not None for k, g in gb.items() if k.startswith("conv_up.0.1."))
    for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(u, v), k
