"""CPU: the folded eval-mode forward (include/ddepth_conv_fused.h; ``conv_bn_act`` of diffusiondepth_amd.conv, ``fold_eval_basic_blocks`` and
``backbone_backend="hip+fold"`` / ``backbone_precision`` of the facade) as far as no GPU is needed -- the ABI (declared == bound == exported,
disjoint from the other headers, which are untouched), the support and workspace queries and argument errors of the built library, the two
facade switches, and that a "hip+fold" model on CPU tensors is the unconverted model bit for bit in .eval() and in .train()."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

from diffusiondepth_amd import backend
from diffusiondepth_amd import batchnorm as BN
from diffusiondepth_amd import conv as CV
from diffusiondepth_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = ["dd_bn_fold", "dd_conv3x3_affine_supported", "dd_conv3x3_affine_workspace_bytes", "dd_conv3x3_affine_forward"]
HIP = (CV.HipConv2d, CV.HipConvTranspose2d)


def _declared(header):
    return re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), flags=re.M)


def test_the_header_the_bound_set_and_the_library_agree_and_the_other_lists_are_untouched():
    assert _declared("ddepth_conv_fused.h") == FUSED == CV.ABI_SYMBOLS_FUSED
    lib = CV._lib_fused()
    for s, nargs in zip(FUSED, (9, 4, 8, 15)):
        f = getattr(lib, s)      # (exported: ctypes resolves the symbol)
        assert f.argtypes is not None and len(f.argtypes) == nargs, s
    others = set(CV.ABI_SYMBOLS) | set(CV.ABI_SYMBOLS_SCALED) | set(CV.ABI_SYMBOLS_STRIDED) | set(backend.ABI_SYMBOLS) | set(BN.ABI_SYMBOLS) | \
        set(BN.ADD_ABI_SYMBOLS)
    assert not set(FUSED) & others
    assert _declared("ddepth_conv.h") == CV.ABI_SYMBOLS and len(CV.ABI_SYMBOLS) == 17
    assert _declared("ddepth_conv_scaled.h") == CV.ABI_SYMBOLS_SCALED and len(CV.ABI_SYMBOLS_SCALED) == 3
    assert _declared("ddepth_conv_strided.h") == CV.ABI_SYMBOLS_STRIDED and len(CV.ABI_SYMBOLS_STRIDED) == 5
    for header in ("ddepth.h", "ddepth_conv.h", "ddepth_conv_scaled.h", "ddepth_conv_strided.h", "ddepth_bn.h", "ddepth_bn_add.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert not any(s in text for s in FUSED), header


def test_support_and_workspace_queries_and_argument_errors_need_no_device():
    lib = CV._lib_fused()
    for p in ("bf16", "f16", "f16x3"):
        for cin, cout in ((64, 64), (64, 128), (8, 24), (72, 72), (2048, 2048)):
            assert CV.supported_affine(1, cin, cout, p) and CV.supported_affine(2, cin, cout, p)
        assert CV.supported_affine(2, 3, 64, p) and not CV.supported_affine(1, 3, 64, p)      # the RGB planes: the stride-2 contract only
        for cin, cout in ((4, 64), (64, 60), (2056, 64), (0, 64)):
            assert not CV.supported_affine(1, cin, cout, p) and not CV.supported_affine(2, cin, cout, p)
        assert not CV.supported_affine(3, 64, 64, p) and not CV.supported_affine(0, 64, 64, p)
        # the same ranges as the un-fused operators
        for cin, cout in ((64, 64), (3, 64), (72, 216), (4, 64), (2056, 8)):
            assert CV.supported_affine(1, cin, cout, p) == CV.supported(CV.OP_CONV3X3, cin, cout, p, "any")
            assert CV.supported_affine(2, cin, cout, p) == CV.supported_s2(cin, cout, p)
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported_affine(1, 64, 64, p) and not CV.supported_affine(2, 64, 64, p)
    n = ctypes.c_int64(0)
    # the packed weight image alone: 9 taps, Cout up to 64 rows, Cin up to the K step (32 at stride 1, 16 at stride 2), twice in the split mode
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 4, 64, 64, 176, 608, 2, ctypes.byref(n)) == 0 and n.value == 9 * 64 * 64 * 2
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 4, 64, 64, 176, 608, 4, ctypes.byref(n)) == 0 and n.value == 9 * 64 * 64 * 4
    assert lib.dd_conv3x3_affine_workspace_bytes(2, 1, 3, 64, 40, 72, 2, ctypes.byref(n)) == 0 and n.value == 9 * 64 * 16 * 2
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 1, 72, 72, 5, 35, 3, ctypes.byref(n)) == 0 and n.value == 9 * 128 * 96 * 2
    assert lib.dd_conv3x3_affine_workspace_bytes(3, 1, 64, 64, 3, 5, 2, ctypes.byref(n)) == 1 and b"stride" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 1, 4, 64, 3, 5, 2, ctypes.byref(n)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_affine_workspace_bytes(2, 0, 64, 64, 3, 5, 2, ctypes.byref(n)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 1, 64, 64, 3, 5, 0, ctypes.byref(n)) == 4 and b"precision" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_affine_workspace_bytes(1, 1, 64, 64, 3, 5, 2, None) == 1
    assert lib.dd_conv3x3_affine_forward(None, None, None, None, None, None, 1, 1, 1, 64, 64, 3, 5, 2, None) != 0 and b"null" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_affine_forward(None, None, None, None, None, None, 4, 1, 1, 64, 64, 3, 5, 2, None) == 1 and b"stride" in lib.dd_conv_last_error()
    assert lib.dd_bn_fold(None, None, None, None, 1e-5, None, None, 64, None) == 1 and b"scale_shift" in lib.dd_conv_last_error()


def test_the_functions_refuse_cpu_tensors_and_conv_bn_act_declines_them():
    x, w = torch.randn(1, 64, 4, 5), torch.randn(64, 64, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.conv_affine_forward(x, w, torch.ones(2, 64), None, True, 2, 1)
    bn = nn.BatchNorm2d(64).eval()
    with pytest.raises(RuntimeError):
        CV.bn_fold(bn)
    with pytest.raises(ValueError):
        CV.bn_fold(None)
    conv = CV.convert_hip_conv(nn.Conv2d(64, 64, 3, 1, 1, bias=False), "bf16", channels="any")
    assert isinstance(conv, CV.HipConv2d)
    assert CV.conv_bn_act(conv, bn, x) is None                                   # CPU tensors
    assert CV.conv_bn_act(nn.Conv2d(64, 64, 3, 1, 1, bias=False), bn, x) is None      # not a HipConv2d
    assert CV.conv_bn_act(conv, bn, x.double()) is None and CV.conv_bn_act(conv, bn, x.permute(0, 1, 3, 2)) is None


# ---- the facade -------------------------------------------------------------------------------------------------------------------------------
def _model(name="mmbev_res18", **args):
    return M.Diffusion_DCbase_Model(M.default_args(backbone_name=name, inference_steps=2, **args))


def _blocks(module):
    return [m for m in module.modules() if isinstance(m, M._BasicBlock)]


def test_hip_fold_resolves_and_is_hip_bn_plus_the_fold(monkeypatch):
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND", raising=False)
    monkeypatch.delenv("DDEPTH_BACKBONE_PRECISION", raising=False)
    assert "hip+fold" in M.BACKBONE_BACKENDS and M.BACKBONE_BACKENDS[:3] == ("torch", "hip", "hip+bn")
    assert M.resolve_backbone_backend("hip+fold") == "hip+fold" and M.resolve_backbone_backend() == "torch"
    monkeypatch.setenv("DDEPTH_BACKBONE_BACKEND", "hip+fold")
    assert M.resolve_backbone_backend() == "hip+fold" and M.resolve_backbone_backend("hip") == "hip"
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND")
    with pytest.raises(ValueError):
        M.resolve_backbone_backend("hip+folded")
    plain, bn, fold = _model(precision="bf16"), _model(precision="bf16", backbone_backend="hip+bn"), _model(precision="bf16", backbone_backend="hip+fold")
    assert fold.backbone_backend == "hip+fold" and list(fold.state_dict()) == list(plain.state_dict())
    assert [type(m) for m in fold.depth_backbone.modules()] == [type(m) for m in bn.depth_backbone.modules()]
    assert len(_blocks(fold.depth_backbone)) == 8 and all(b.folded_eval and b.fused_tail for b in _blocks(fold.depth_backbone))
    assert not any(b.folded_eval for b in _blocks(bn.depth_backbone)) and not any(b.folded_eval for b in _blocks(plain.depth_backbone))
    assert all(b.fused_tail for b in _blocks(bn.depth_backbone))
    assert sum(isinstance(m, CV.HipConv2d) for m in fold.depth_backbone.modules()) == 20


def test_fold_eval_basic_blocks_is_idempotent_and_keeps_tensors_and_keys():
    net = M.ResNetForMMBEV([2, 1], channels=(64, 128))
    keys, ptrs, ids = list(net.state_dict()), [v.data_ptr() for v in net.state_dict().values()], [id(p) for p in net.parameters()]
    types = [type(m) for m in net.modules()]
    assert M.fold_eval_basic_blocks(net) is net and M.fold_eval_basic_blocks(net) is net
    assert all(b.folded_eval for b in _blocks(net)) and len(_blocks(net)) == 3
    assert list(net.state_dict()) == keys and [v.data_ptr() for v in net.state_dict().values()] == ptrs
    assert [id(p) for p in net.parameters()] == ids and [type(m) for m in net.modules()] == types


def test_backbone_precision_resolution(monkeypatch):
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND", raising=False)
    monkeypatch.delenv("DDEPTH_BACKBONE_PRECISION", raising=False)
    assert M.resolve_backbone_precision() is None and M.resolve_backbone_precision("f16x3") == "f16x3"
    for bad in ("fp32", "f16r", "half"):
        with pytest.raises(ValueError):
            M.resolve_backbone_precision(bad)
    convs = lambda m: [c for c in m.depth_backbone.modules() if isinstance(c, HIP)]
    # absent: today's rule -- the head's precision; a fast-profile head converts nothing
    assert _model(precision="f16r", backbone_backend="hip").backbone_precision is None
    assert not convs(_model(precision="f16r", backbone_backend="hip")) and not convs(_model(precision="f16r", backbone_backend="hip+fold"))
    assert {c.precision for c in convs(_model(precision="bf16", backbone_backend="hip"))} == {"bf16"}
    # given: the backbone's own, whatever the head's
    for head, own in (("f16r", "f16x3"), ("f16r", "bf16"), ("bf16", "f16"), (None, "f16x3")):
        m = _model(precision=head, backbone_backend="hip+fold", backbone_precision=own)
        assert m.backbone_precision == own and len(convs(m)) == 20 and {c.precision for c in convs(m)} == {own}
    monkeypatch.setenv("DDEPTH_BACKBONE_PRECISION", "bf16")
    m = _model(precision="f16r", backbone_backend="hip")
    assert m.backbone_precision == "bf16" and {c.precision for c in convs(m)} == {"bf16"}
    assert {c.precision for c in convs(_model(precision="f16r", backbone_backend="hip", backbone_precision="f16x3"))} == {"f16x3"}      # the keyword wins
    # with "torch" nothing changes
    t = _model(precision="f16r", backbone_precision="f16x3")
    assert t.backbone_backend == "torch" and not convs(t) and not any(isinstance(b, BN.HipBatchNorm2d) for b in t.depth_backbone.modules())
    monkeypatch.setenv("DDEPTH_BACKBONE_PRECISION", "")
    assert _model(precision="f16r", backbone_backend="hip").backbone_precision is None
    with pytest.raises(ValueError):
        _model(precision="bf16", backbone_backend="hip", backbone_precision="fp32")


def _seeded_backbone():
    torch.manual_seed(5)
    net = M.ResNetForMMBEV([2, 1], channels=(64, 128))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.num_features, generator=g))
    return net


@pytest.mark.parametrize("mode", ["eval", "eval_no_grad", "train"])
def test_a_hip_fold_model_on_cpu_tensors_is_the_unconverted_one_bit_for_bit(mode):
    args = M.default_args(inference_steps=2, precision="f16r", backbone_backend="hip+fold", backbone_precision="f16x3")
    plain, conv = _seeded_backbone(), M.Diffusion_DCbase_Model(args, depth_backbone=_seeded_backbone()).depth_backbone
    assert all(b.folded_eval for b in _blocks(conv)) and sum(isinstance(m, CV.HipConv2d) for m in conv.modules()) == 8
    plain.train(mode == "train")
    conv.train(mode == "train")
    x = torch.randn(2, 3, 20, 36, generator=torch.Generator().manual_seed(7))
    if mode == "eval_no_grad":
        with torch.no_grad():
            fa, fb = plain(x), conv(x)
        assert all(torch.equal(a, b) for a, b in zip(fa, fb)) and len(fa) == 2
        return
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    fa, fb = plain(xa), conv(xb)
    assert all(torch.equal(a, b) for a, b in zip(fa, fb))
    sum((f ** 2).sum() for f in fa).backward()
    sum((f ** 2).sum() for f in fb).backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(plain.parameters(), conv.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(plain.buffers(), conv.buffers()))
