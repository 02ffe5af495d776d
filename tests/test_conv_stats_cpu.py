"""CPU: the statistics-emitting training forward (include/ddepth_conv_stats.h; ``conv_stats_forward``, ``ConvStatsFunction`` and ``conv_bn_train``
of diffusiondepth_amd.conv, ``HipBatchNorm2d.forward_sums``, ``fuse_conv_bn_stats`` / ``backbone_backend="hip+stats"`` of the facade and the heads'
``conv_bn_stats``) as far as no GPU is needed -- the ABI (declared == bound == exported, disjoint from the other headers, which are untouched),
the support and workspace queries and argument errors of the built library, the switches, and that a "hip+stats" backbone and a
``conv_bn_stats=True`` Res head on CPU tensors are the unconverted ones bit for bit, forward and gradients."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import batchnorm as BN
from diffusiondepth_amd import conv as CV
from diffusiondepth_amd import model as M
from diffusiondepth_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ["dd_conv3x3_stats_supported", "dd_conv3x3_stats_workspace_bytes", "dd_conv3x3_stats_forward"]


def _declared(header):
    return re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), flags=re.M)


def test_the_header_the_bound_set_and_the_library_agree_and_the_other_lists_are_untouched():
    assert _declared("ddepth_conv_stats.h") == STATS == CV.ABI_SYMBOLS_STATS
    lib = CV._lib_stats()
    for s, nargs in zip(STATS, (4, 8, 14)):
        f = getattr(lib, s)      # (exported: ctypes resolves the symbol)
        assert f.argtypes is not None and len(f.argtypes) == nargs, s
    others = set(CV.ABI_SYMBOLS) | set(CV.ABI_SYMBOLS_SCALED) | set(CV.ABI_SYMBOLS_STRIDED) | set(CV.ABI_SYMBOLS_FUSED) | set(backend.ABI_SYMBOLS) | \
        set(BN.ABI_SYMBOLS) | set(BN.ADD_ABI_SYMBOLS)
    assert not set(STATS) & others
    assert _declared("ddepth_conv.h") == CV.ABI_SYMBOLS and len(CV.ABI_SYMBOLS) == 17
    assert _declared("ddepth_conv_scaled.h") == CV.ABI_SYMBOLS_SCALED and len(CV.ABI_SYMBOLS_SCALED) == 3
    assert _declared("ddepth_conv_strided.h") == CV.ABI_SYMBOLS_STRIDED and len(CV.ABI_SYMBOLS_STRIDED) == 5
    assert _declared("ddepth_conv_fused.h") == CV.ABI_SYMBOLS_FUSED and len(CV.ABI_SYMBOLS_FUSED) == 4
    for header in ("ddepth.h", "ddepth_conv.h", "ddepth_conv_scaled.h", "ddepth_conv_strided.h", "ddepth_conv_fused.h", "ddepth_bn.h",
                   "ddepth_bn_add.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(s in text for s in STATS), header


def test_support_and_workspace_queries_and_argument_errors_need_no_device():
    lib = CV._lib_stats()
    for p in ("bf16", "f16", "f16x3"):
        # the ranges of dd_conv3x3_affine_supported: those of the un-fused operators
        for cin, cout in ((64, 64), (3, 64), (72, 216), (8, 24), (2048, 2048), (4, 64), (64, 60), (2056, 8), (0, 64)):
            for stride in (0, 1, 2, 3):
                assert CV.supported_stats(stride, cin, cout, p) == CV.supported_affine(stride, cin, cout, p)
            assert CV.supported_stats(1, cin, cout, p) == CV.supported(CV.OP_CONV3X3, cin, cout, p, "any")
            assert CV.supported_stats(2, cin, cout, p) == CV.supported_s2(cin, cout, p)
        assert CV.supported_stats(2, 3, 64, p) and not CV.supported_stats(1, 3, 64, p)      # the RGB planes: the stride-2 contract only
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported_stats(1, 64, 64, p) and not CV.supported_stats(2, 64, 64, p)
    n = ctypes.c_int64(0)
    # the packed weight image (9 taps, Cout up to 64 rows, Cin up to the K step, twice in the split mode), then one fp64 pair per channel, image and
    # 4 x 32 tile, each part rounded up to 256 bytes
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 4, 64, 256, 176, 608, 2, ctypes.byref(n)) == 0
    assert n.value == 9 * 256 * 64 * 2 + 256 * 4 * (44 * 19) * 16
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 4, 64, 64, 176, 608, 4, ctypes.byref(n)) == 0 and n.value == 9 * 64 * 64 * 4 + 64 * 4 * (44 * 19) * 16
    assert lib.dd_conv3x3_stats_workspace_bytes(2, 1, 3, 64, 40, 72, 2, ctypes.byref(n)) == 0 and n.value == 9 * 64 * 16 * 2 + 64 * 1 * (5 * 2) * 16
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 1, 72, 72, 5, 35, 3, ctypes.byref(n)) == 0 and n.value == 9 * 128 * 96 * 2 + 72 * 1 * (2 * 2) * 16
    assert lib.dd_conv3x3_stats_workspace_bytes(3, 1, 64, 64, 3, 5, 2, ctypes.byref(n)) == 1 and b"stride" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 1, 4, 64, 3, 5, 2, ctypes.byref(n)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_workspace_bytes(2, 0, 64, 64, 3, 5, 2, ctypes.byref(n)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 1, 64, 64, -3, 5, 2, ctypes.byref(n)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 1, 64, 64, 3, 5, 0, ctypes.byref(n)) == 4 and b"precision" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_workspace_bytes(1, 1, 64, 64, 3, 5, 2, None) == 1
    assert lib.dd_conv3x3_stats_forward(None, None, None, None, None, None, 1, 1, 64, 64, 3, 5, 2, None) == 1 and b"null" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_forward(None, None, None, None, None, None, 4, 1, 64, 64, 3, 5, 2, None) == 1 and b"stride" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_stats_forward(None, None, None, None, None, None, 1, 0, 64, 64, 3, 5, 2, None) == 1 and b"positive" in lib.dd_conv_last_error()
    # every pointer but the bias is needed: a host address is enough to get past the others' null checks, nothing is launched before all passed
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16      # (distinct, 16-byte aligned addresses: neither the alias nor the alignment check answers first)
    for missing in (0, 1, 3, 4, 5):
        args = [ctypes.c_void_p(base + 16 * i) for i in range(6)]
        args[missing] = None
        assert lib.dd_conv3x3_stats_forward(*args, 1, 1, 64, 64, 3, 5, 2, None) == 1 and b"null" in lib.dd_conv_last_error(), missing


def test_the_functions_refuse_cpu_tensors_and_conv_bn_train_declines_them():
    x, w = torch.randn(2, 64, 4, 5), torch.randn(64, 64, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.conv_stats_forward(x, w, None, 1, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.ConvStatsFunction.apply(x, w, None, 2, 1, "any", False)
    with pytest.raises(ValueError, match="stride 2 only"):      # the stride-1 backward has no bias gradient to give: refused, not dropped
        CV.ConvStatsFunction.apply(x, w, torch.zeros(64), 2, 1, "any", False)
    conv = CV.convert_hip_conv(nn.Conv2d(64, 64, 3, 1, 1, bias=False), "bf16", channels="any")
    bn = BN.HipBatchNorm2d(64, activation="relu").train()
    assert isinstance(conv, CV.HipConv2d)
    before = [b.clone() for b in bn.buffers()]
    assert CV.conv_bn_train(conv, bn, x) is None                                                       # CPU tensors
    assert CV.conv_bn_train(nn.Conv2d(64, 64, 3, 1, 1, bias=False), bn, x) is None                     # not a HipConv2d
    assert CV.conv_bn_train(conv, nn.BatchNorm2d(64), x) is None                                       # not a HipBatchNorm2d
    assert CV.conv_bn_train(conv, bn.eval(), x) is None                                                # .eval()
    bn.train()
    assert CV.conv_bn_train(conv, bn, x.double()) is None and CV.conv_bn_train(conv, bn, x.permute(0, 1, 3, 2)) is None
    assert CV.conv_bn_train(conv, bn, x, addend=torch.randn(2, 64, 4, 5)) is None
    assert all(torch.equal(a, b) for a, b in zip(before, bn.buffers())), "a declined call touched the running buffers"
    with pytest.raises(RuntimeError):
        bn.forward_sums(x, torch.zeros(129, dtype=torch.float64))                                      # never a silent torch path
    for fn, args in ((BN.BatchNormSumsTrainFunction, (x, None, None, None, None, 1e-5, 0.1, 0, 0.0, None, torch.zeros(129, dtype=torch.float64))),
                     (BN.BatchNormAddSumsTrainFunction, (x, x, None, None, None, None, 1e-5, 0.1, 0, 0.0, 0, None, torch.zeros(129, dtype=torch.float64)))):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn.apply(*args)


def test_exports_and_the_existing_functions_keep_their_signatures():
    import inspect
    assert dda.fuse_conv_bn_stats is M.fuse_conv_bn_stats and dda.conv_bn_train is CV.conv_bn_train
    assert "fuse_conv_bn_stats" in dda.__all__ and "conv_bn_train" in dda.__all__
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(BN.BatchNormTrainFunction.forward) == ["ctx", "x", "weight", "bias", "running_mean", "running_var", "eps", "momentum", "act", "slope",
                                                       "exchange"]
    assert names(BN.BatchNormSumsTrainFunction.forward) == names(BN.BatchNormTrainFunction.forward) + ["sums"]
    assert names(BN.BatchNormAddSumsTrainFunction.forward) == names(BN.BatchNormAddTrainFunction.forward) + ["sums"]
    assert names(CV.Conv3x3Function.forward) == ["ctx", "x", "weight", "prec", "channels", "grad_autoscale"]
    assert names(CV.Conv3x3S2Function.forward) == ["ctx", "x", "weight", "bias", "prec", "grad_autoscale"]


# ---- the facade and the head ----------------------------------------------------------------------------------------------------------------------
def _model(name="mmbev_res18", **args):
    return M.Diffusion_DCbase_Model(M.default_args(backbone_name=name, inference_steps=2, **args))


def _blocks(module):
    return [m for m in module.modules() if isinstance(m, M._BasicBlock)]


def test_hip_stats_resolves_and_is_hip_fold_plus_the_flag(monkeypatch):
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND", raising=False)
    monkeypatch.delenv("DDEPTH_BACKBONE_PRECISION", raising=False)
    assert M.BACKBONE_BACKENDS == ("torch", "hip", "hip+bn", "hip+fold", "hip+stats")      # appended: the earlier entries keep their places
    assert M.resolve_backbone_backend("hip+stats") == "hip+stats" and M.resolve_backbone_backend() == "torch"
    monkeypatch.setenv("DDEPTH_BACKBONE_BACKEND", "hip+stats")
    assert M.resolve_backbone_backend() == "hip+stats" and M.resolve_backbone_backend("hip") == "hip"
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND")
    with pytest.raises(ValueError):
        M.resolve_backbone_backend("hip+stat")
    plain, fold, stats = _model(precision="bf16"), _model(precision="bf16", backbone_backend="hip+fold"), _model(precision="bf16",
                                                                                                           backbone_backend="hip+stats")
    assert stats.backbone_backend == "hip+stats" and list(stats.state_dict()) == list(plain.state_dict())
    assert [(n, type(m)) for n, m in stats.depth_backbone.named_modules()] == [(n, type(m)) for n, m in fold.depth_backbone.named_modules()]
    assert len(_blocks(stats.depth_backbone)) == 8
    assert all(b.conv_bn_stats and b.folded_eval and b.fused_tail for b in _blocks(stats.depth_backbone))
    assert not any(b.conv_bn_stats for b in _blocks(fold.depth_backbone)) and not any(b.conv_bn_stats for b in _blocks(plain.depth_backbone))


def test_fuse_conv_bn_stats_is_idempotent_and_keeps_tensors_and_keys():
    net = M.ResNetForMMBEV([2, 1], channels=(64, 128))
    keys, ptrs, ids = list(net.state_dict()), [v.data_ptr() for v in net.state_dict().values()], [id(p) for p in net.parameters()]
    types = [type(m) for m in net.modules()]
    assert M.fuse_conv_bn_stats(net) is net and M.fuse_conv_bn_stats(net) is net
    assert all(b.conv_bn_stats for b in _blocks(net)) and len(_blocks(net)) == 3
    assert list(net.state_dict()) == keys and [v.data_ptr() for v in net.state_dict().values()] == ptrs
    assert [id(p) for p in net.parameters()] == ids and [type(m) for m in net.modules()] == types


def test_the_head_keyword_the_environment_variable_and_a_value_error(monkeypatch):
    monkeypatch.delenv("DDEPTH_CONV_BN_STATS", raising=False)
    kw = dict(inference_steps=2, precision="bf16", bn_backend="hip+add", conv_backend="hip")
    off, on = dda.DDIMDepthEstimate_Res(**kw), dda.DDIMDepthEstimate_Res(conv_bn_stats=True, **kw)
    assert off.conv_bn_stats is False and on.conv_bn_stats is True
    assert list(off.state_dict()) == list(on.state_dict())
    assert [(n, type(m)) for n, m in off.named_modules()] == [(n, type(m)) for n, m in on.named_modules()]
    assert all(isinstance(l[0], CV.HipConv2d) and isinstance(l[1], BN.HipBatchNorm2d) for l in on.conv_lateral)
    monkeypatch.setenv("DDEPTH_CONV_BN_STATS", "1")
    assert dda.DDIMDepthEstimate_Res(**kw).conv_bn_stats is True and dda.DDIMDepthEstimate_Res(conv_bn_stats=False, **kw).conv_bn_stats is False
    monkeypatch.setenv("DDEPTH_CONV_BN_STATS", "0")
    assert dda.DDIMDepthEstimate_Res(**kw).conv_bn_stats is False
    monkeypatch.setenv("DDEPTH_CONV_BN_STATS", "yes")
    with pytest.raises(ValueError, match="DDEPTH_CONV_BN_STATS"):
        dda.DDIMDepthEstimate_Res(**kw)


def _seeded_backbone():
    torch.manual_seed(5)
    return M.ResNetForMMBEV([2, 1], channels=(64, 128))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_a_hip_stats_backbone_on_cpu_tensors_is_the_unconverted_one_bit_for_bit(train):
    args = M.default_args(inference_steps=2, precision="bf16", backbone_backend="hip+stats")
    plain, conv = _seeded_backbone(), M.Diffusion_DCbase_Model(args, depth_backbone=_seeded_backbone()).depth_backbone
    assert all(b.conv_bn_stats for b in _blocks(conv)) and sum(isinstance(m, CV.HipConv2d) for m in conv.modules()) == 8
    assert list(plain.state_dict()) == list(conv.state_dict())
    plain.train(train), conv.train(train)
    x = torch.randn(2, 3, 20, 36, generator=torch.Generator().manual_seed(7))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    fa, fb = plain(xa), conv(xb)
    assert len(fa) == 2 and all(torch.equal(a, b) for a, b in zip(fa, fb))
    sum((f ** 2).sum() for f in fa).backward()
    sum((f ** 2).sum() for f in fb).backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(plain.parameters(), conv.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(plain.buffers(), conv.buffers()))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("size", [(32, 64), (36, 68)], ids=["even", "odd"])
def test_a_conv_bn_stats_res_head_on_cpu_is_the_torch_head_bit_for_bit(size, train):
    torch.manual_seed(0)
    a = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16")
    b = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", bn_backend="hip+add", conv_backend="hip", conv_bn_stats=True)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    a.train(train), b.train(train)
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, 2, *size)]
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
    for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(u, v), k


# ---- the network case T2: which precisions its bound applies to -------------------------------------------------------------------------------------
def test_the_operand_rounding_alone_keeps_t2_within_half_the_bound_in_f16x3_and_not_in_bf16():
    """The precondition N1 ties its bounds to (tests/conv_strided_cases.py), evaluated for T2 on the CPU: it decides which precisions the GPU test
    asserts (tests/conv_stats_cases.py)."""
    import conv_stats_cases as SC
    import conv_strided_cases as ZC
    ref = SC.t2_reference()
    over = {}
    for prec in ("f16x3", "bf16"):
        grads, feats = ZC.n1_errors(SC.t2_emulation(prec), ref)
        assert len(grads) == 28 and len(feats) == 2
        worst = max(grads, key=grads.get)
        print(f"T2 emulation {prec}: worst gradient {worst} {grads[worst]:.3e}, features {feats[0]:.3e} {feats[1]:.3e} (bound {ZC.N1_BOUNDS[prec]:.0e})")
        over[prec] = [k for k, v in list(grads.items()) + list(enumerate(feats)) if not v <= 0.5 * ZC.N1_BOUNDS[prec]]
    assert over["f16x3"] == [] and SC.T2_ASSERTED == ("f16x3",)
    assert over["bf16"], "bf16 meets the precondition after all: assert it on the GPU too"
