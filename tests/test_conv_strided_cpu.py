"""CPU: the 3x3 stride-2 operator (include/ddepth_conv_strided.h; ``strided`` of diffusiondepth_amd.conv, ``backbone_backend`` of the facade) as far as
no GPU is needed -- the ABI (declared == bound == exported, disjoint from the other headers), the support and workspace queries, the converter
with and without ``strided=True``, that on CPU tensors a converted net is the torch net bit for bit, ``needs_input_grad`` on stand-ins of the
library calls, the facade switch, the module census of the bundled backbones, and the precondition of the GPU network case N1
(tests/conv_strided_cases.py): rounding the operands alone keeps N1 within half of each asserted bound."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import conv_strided_cases as ZC
import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import conv as CV
from diffusiondepth_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDED = ["dd_conv3x3s2_supported", "dd_conv3x3s2_workspace_bytes", "dd_conv3x3s2_forward", "dd_conv3x3s2_backward_data",
           "dd_conv3x3s2_backward_weight"]
HIP = (CV.HipConv2d, CV.HipConvTranspose2d)


def _declared(header):
    return re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), flags=re.M)


def test_the_header_the_bound_set_and_the_library_agree_and_the_other_lists_are_untouched():
    assert _declared("ddepth_conv_strided.h") == STRIDED == CV.ABI_SYMBOLS_STRIDED
    lib = CV._lib_strided()
    for s, nargs in zip(STRIDED, (3, 7, 12, 12, 13)):
        f = getattr(lib, s)
        assert f.argtypes is not None and len(f.argtypes) == nargs, s
    others = set(CV.ABI_SYMBOLS) | set(CV.ABI_SYMBOLS_SCALED) | set(backend.ABI_SYMBOLS)
    assert not set(STRIDED) & others
    assert _declared("ddepth_conv.h") == CV.ABI_SYMBOLS and len(CV.ABI_SYMBOLS) == 17 and _declared("ddepth_conv_scaled.h") == CV.ABI_SYMBOLS_SCALED
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    assert not any(s in main for s in STRIDED)


def test_support_and_workspace_queries_need_no_device():
    lib = CV._lib_strided()
    for p in ("bf16", "f16", "f16x3"):
        for cin, cout in ((3, 64), (64, 128), (128, 256), (256, 512), (72, 216), (8, 8), (2048, 2048)):
            assert CV.supported_s2(cin, cout, p)
        assert CV.supported_s2(64, 128, p, "block64") and not CV.supported_s2(3, 64, p, "block64") and not CV.supported_s2(72, 216, p, "block64")
        for cin, cout in ((4, 64), (64, 60), (64, 3), (2056, 64), (0, 64)):
            assert not CV.supported_s2(cin, cout, p)
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported_s2(64, 128, p)
    # the old operators still refuse the RGB planes
    assert CV._lib().dd_conv_supported(0, 3, 64, 2) == 0 and CV._lib().dd_convx_supported(0, 3, 64, 2) == 0
    n, small = ctypes.c_int64(0), ctypes.c_int64(0)
    # conv1 of stage 2 at KITTI size, B = 4: the weight gradient's partials.  88 x 304 outputs = 4 * 44 * 10 = 1760 tiles of 2 x 32, 28 per split
    # (at most 64 splits), 63 splits
    assert lib.dd_conv3x3s2_workspace_bytes(4, 64, 128, 176, 608, 2, ctypes.byref(n)) == 0 and n.value == 63 * 9 * 64 * 128 * 4
    assert lib.dd_conv3x3s2_workspace_bytes(1, 3, 64, 3, 5, 2, ctypes.byref(small)) == 0 and 0 < small.value < n.value
    assert lib.dd_conv3x3s2_workspace_bytes(1, 4, 64, 3, 5, 2, ctypes.byref(small)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_workspace_bytes(0, 64, 64, 3, 5, 2, ctypes.byref(small)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_workspace_bytes(1, 64, 64, 3, 5, 0, ctypes.byref(small)) == 4 and b"precision" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_forward(None, None, None, None, None, 1, 64, 64, 3, 5, 2, None) != 0 and b"null" in lib.dd_conv_last_error()
    assert [CV.strided_out(n) for n in (1, 2, 3, 4, 9, 16)] == [1, 1, 2, 2, 5, 8]


def test_the_functions_refuse_cpu_tensors():
    x, w = torch.randn(1, 64, 4, 5, requires_grad=True), torch.randn(64, 64, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.Conv3x3S2Function.apply(x, w, None, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.conv_s2_backward_weight(x, torch.randn(1, 64, 2, 3), w.shape, 2, with_bias=True)


def _small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(3, 64, 3, 2, 1, bias=True),               # RGB, stride 2, a bias
                         nn.BatchNorm2d(64), nn.ReLU(True),
                         nn.Conv2d(64, 128, 3, 2, 1, bias=False),            # stride 2, block-64
                         nn.Sequential(nn.Conv2d(128, 72, 3, 2, 1), nn.ReLU()),      # stride 2, ragged, a bias
                         nn.Conv2d(72, 64, 3, 1, 1, bias=False),             # stride 1
                         nn.Conv2d(64, 64, 3, 1, 1, bias=True),              # stride 1 with a bias: no operator takes it
                         nn.Conv2d(64, 64, 3, 2, 0, bias=False),             # stride 2 without padding
                         nn.Conv2d(64, 64, 3, 2, 1, bias=False, groups=2),
                         nn.Conv2d(64, 64, 3, 2, 1, bias=False, dilation=2),
                         nn.Conv2d(64, 60, 3, 2, 1, bias=False))             # 60 output channels


def _types(net):
    return [type(m) for m in (net[0], net[3], net[4][0], net[5], net[6], net[7], net[8], net[9], net[10])]


def test_the_default_converter_leaves_every_strided_convolution_alone():
    net = CV.convert_hip_conv(_small_net(), "bf16", channels="any")
    assert _types(net) == [nn.Conv2d] * 3 + [CV.HipConv2d] + [nn.Conv2d] * 5
    assert CV.HipConv2d.strided is False and "strided" not in net[5].__dict__ and "strided" not in repr(net[5])
    assert not CV.eligible(nn.Conv2d(64, 128, 3, 2, 1), "bf16") and not CV.eligible(nn.Conv2d(64, 128, 3, 2, 1), "bf16", channels="any")
    assert CV.eligible(nn.Conv2d(64, 128, 3, 2, 1), "bf16", strided=True) and CV.eligible(nn.Conv2d(3, 64, 3, 2, 1), "bf16", channels="any", strided=True)
    assert not CV.eligible(nn.Conv2d(3, 64, 3, 2, 1), "bf16", strided=True)            # block-64 modules take block-64 shapes only
    assert not CV.eligible(nn.Conv2d(64, 64, 3, 1, 1, bias=True), "bf16", strided=True)      # the stride-1 operators still take no bias


def test_the_strided_converter_keeps_tensors_keys_indices_and_the_bias():
    net = _small_net()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    params = [id(p) for p in net.parameters()]
    out = CV.convert_hip_conv(net, "bf16", channels="any", strided=True)
    assert out is net and list(net.state_dict()) == list(before)
    assert {k: v.data_ptr() for k, v in net.state_dict().items()} == before and [id(p) for p in net.parameters()] == params
    assert _types(net) == [CV.HipConv2d] * 4 + [nn.Conv2d] * 5
    assert [net[0].strided, net[3].strided, net[4][0].strided, net[5].strided] == [True, True, True, False]
    assert net[0].bias is not None and net[4][0].bias is not None and net[3].bias is None
    assert all(m.channels == "any" and m.precision == "bf16" for m in (net[0], net[3], net[4][0]))
    assert "strided=True" in repr(net[0]) and "stride=(2, 2)" in repr(net[0])
    assert CV.convert_hip_conv(net, "bf16", channels="any", strided=True) is net and _types(net) == [CV.HipConv2d] * 4 + [nn.Conv2d] * 5      # idempotent
    block = CV.convert_hip_conv(_small_net(), "f16x3", strided=True, grad_autoscale=True)      # the block-64 contract gates the new operator too
    assert _types(block) == [nn.Conv2d, CV.HipConv2d] + [nn.Conv2d] * 7 and block[3].grad_autoscale is True and block[3].strided is True
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not any(isinstance(m, HIP) for m in CV.convert_hip_conv(_small_net(), p, channels="any", strided=True).modules())


def test_a_converted_net_on_cpu_tensors_is_the_unconverted_one_bit_for_bit():
    a, b = _small_net()[:6], CV.convert_hip_conv(_small_net(), "f16x3", channels="any", strided=True)[:6]
    x = torch.randn(2, 3, 21, 34, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    (ya ** 2).sum().backward()
    (yb ** 2).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))


def test_needs_input_grad_is_honoured(monkeypatch):
    """The Function's backward asks only for what autograd needs, and the bias gradient comes from the weight gradient's call (stand-ins of the
    three library calls: no device here)."""
    calls = []
    monkeypatch.setattr(CV, "conv_s2_forward", lambda x, w, b, prec: x.new_zeros(x.shape[0], w.shape[0], CV.strided_out(x.shape[2]),
                                                                                 CV.strided_out(x.shape[3])))
    monkeypatch.setattr(CV, "conv_s2_backward_data", lambda gy, w, shape, prec: (calls.append("data"), gy.new_zeros(tuple(shape)))[1])

    def weight(x, gy, shape, prec, with_bias=False):
        calls.append("weight+bias" if with_bias else "weight")
        return gy.new_zeros(tuple(shape)), (gy.new_zeros(shape[0]) if with_bias else None)
    monkeypatch.setattr(CV, "conv_s2_backward_weight", weight)
    cases = ((True, True, True, ["data", "weight+bias"]), (False, True, True, ["weight+bias"]), (True, False, False, ["data"]),
             (True, True, None, ["data", "weight"]), (False, False, True, ["weight+bias"]), (False, True, False, ["weight"]))
    for need_x, need_w, need_b, want in cases:
        calls.clear()
        x = torch.randn(1, 3, 4, 5, requires_grad=need_x)
        w = torch.randn(64, 3, 3, 3, requires_grad=need_w)
        b = None if need_b is None else torch.randn(64, requires_grad=need_b)
        CV.Conv3x3S2Function.apply(x, w, b, 2).sum().backward()
        assert calls == want, (need_x, need_w, need_b, calls)
        assert (x.grad is not None) == need_x and (w.grad is not None) == need_w and (b is None or (b.grad is not None) == need_b)
    assert not CV.Conv3x3S2Function.apply(torch.randn(1, 3, 4, 5), torch.randn(64, 3, 3, 3), torch.randn(64), 2).requires_grad


# ---- the facade -------------------------------------------------------------------------------------------------------------------------------
def _plain_convs(module):
    return [n for n, m in module.named_modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and not isinstance(m, HIP)]


def _model(name="mmbev_res18", **args):
    return M.Diffusion_DCbase_Model(M.default_args(backbone_name=name, inference_steps=2, **args))


def test_the_facade_keyword_the_environment_variable_and_the_value_error(monkeypatch):
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND", raising=False)
    plain = _model(precision="bf16")
    assert plain.backbone_backend == "torch" and not any(isinstance(m, HIP) for m in plain.depth_backbone.modules())
    monkeypatch.setenv("DDEPTH_BACKBONE_BACKEND", "")
    assert _model(precision="bf16").backbone_backend == "torch"
    monkeypatch.setenv("DDEPTH_BACKBONE_BACKEND", "hip")
    env = _model(precision="bf16")
    assert env.backbone_backend == "hip" and not _plain_convs(env.depth_backbone)
    assert list(env.state_dict()) == list(plain.state_dict())
    assert _model(precision="bf16", backbone_backend="torch").backbone_backend == "torch"      # the keyword wins
    monkeypatch.delenv("DDEPTH_BACKBONE_BACKEND")
    with pytest.raises(ValueError):
        _model(precision="bf16", backbone_backend="miopen")
    # an fp32 or f16r model: the keyword is honoured, nothing is eligible, nothing is replaced
    for extra in ({}, {"precision": "fp32"}, {"precision": "f16r"}):
        m = _model(backbone_backend="hip", **extra)
        assert m.backbone_backend == "hip" and not any(isinstance(c, HIP) for c in m.depth_backbone.modules())
    # an injected backbone is converted too, in place: the same parameter tensors
    bb = M.ResNetForMMBEV([1, 1, 1, 1])
    ids = [id(p) for p in bb.parameters()]
    inj = M.Diffusion_DCbase_Model(M.default_args(inference_steps=2, precision="f16x3", backbone_backend="hip"), depth_backbone=bb)
    assert not _plain_convs(inj.depth_backbone) and [id(p) for p in inj.depth_backbone.parameters()] == ids


@pytest.mark.parametrize("name,convs", [("mmbev_res18", 20), ("mmbev_res50", 36)])
def test_the_hip_backbone_has_no_plain_convolution_left(name, convs):
    m = _model(name, precision="bf16", backbone_backend="hip")
    mods = [c for c in m.depth_backbone.modules() if isinstance(c, nn.Conv2d)]
    assert len(mods) == convs and not _plain_convs(m.depth_backbone)
    strided = [c for c in mods if c.strided]
    assert len(strided) == 8 and all(c.stride == (2, 2) for c in strided) and sum(c.bias is not None for c in strided) == 4
    assert [c.in_channels for c in strided] == [3, 3, 64, 64, 128, 128, 256, 256]
    assert all(c.channels == "any" and c.precision == "bf16" and not c.grad_autoscale for c in mods)
    # the autoscale choice of the head travels to the backbone
    auto = M.Diffusion_DCbase_Model(M.default_args(backbone_name=name, inference_steps=2, precision="f16x3", backbone_backend="hip"),
                                    depth_head=dda.DDIMDepthEstimate_Res(inference_steps=2, precision="f16x3", conv_grad_autoscale=True))
    assert all(c.grad_autoscale for c in auto.depth_backbone.modules() if isinstance(c, nn.Conv2d))


# ---- N1's precondition ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_rounding_the_operands_alone_keeps_n1_within_half_of_each_bound(prec):
    grads, feats = ZC.n1_errors(ZC.n1_emulation(prec))
    worst = max(grads, key=grads.get)
    print(f"N1 {prec}: worst gradient {worst} {grads[worst]:.3e}, features {max(feats):.3e}, bound {ZC.N1_BOUNDS[prec]:.1e}")
    assert len(grads) == 6 + 2 + 8 and len(feats) == 2
    assert grads[worst] <= ZC.N1_BOUNDS[prec] / 2 and max(feats) <= ZC.N1_BOUNDS[prec] / 2


def test_n1_f16_is_recorded_not_asserted():
    grads, feats = ZC.n1_errors(ZC.n1_emulation("f16"))
    print(f"N1 f16: worst gradient {max(grads.values()):.3e}, features {max(feats):.3e}")
    assert all(v == v for v in grads.values())
