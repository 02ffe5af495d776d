"""CPU: everything about diffusiondepth_amd.codec that needs no GPU -- the C ABI of include/ddepth_codec.h (declared == bound == exported, the
workspace query), the converter (same tensors, same keys, same indices, either order with convert_hip_batchnorm, idempotent), the head keyword /
environment variable, and that on CPU tensors the converted codec IS the torch one, bit for bit, forward and gradients."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import batchnorm as BN
from diffusiondepth_amd import codec as CD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_TYPES = (CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecTail)


def test_codec_header_declares_the_bound_symbols_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ddepth_codec.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(CD.ABI_SYMBOLS), declared ^ set(CD.ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    assert not any(s in main for s in declared) and not declared & set(backend.ABI_SYMBOLS)


def test_workspace_query_and_argument_checks_need_no_device():
    lib = CD._lib()
    n, small = ctypes.c_int64(0), ctypes.c_int64(0)
    # DEC0 at KITTI size, B = 4: at most kMaxSplits = 1024 splits of 16 * 16 * 16 weight and 16 bias partials
    assert lib.dd_codec_workspace_bytes(CD.OP_DEC0, 4, 176, 608, ctypes.byref(n)) == 0 and 4112 * 4 <= n.value <= 1024 * 4112 * 4
    assert lib.dd_codec_workspace_bytes(CD.OP_DEC0, 1, 3, 5, ctypes.byref(small)) == 0 and 0 < small.value < n.value
    assert lib.dd_codec_workspace_bytes(9, 1, 3, 5, ctypes.byref(small)) == 1 and b"op" in lib.dd_codec_last_error()
    assert lib.dd_codec_workspace_bytes(CD.OP_ENC0, 0, 3, 5, ctypes.byref(small)) == 1 and b"positive" in lib.dd_codec_last_error()
    assert lib.dd_codec_conv_forward(CD.OP_ENC1, None, None, None, None, None, 1, 3, 5, None) != 0 and b"null" in lib.dd_codec_last_error()
    assert lib.dd_codec_tail_forward(None, None, 4, 1e-6, None) != 0 and b"null" in lib.dd_codec_last_error()


def test_exports():
    assert dda.HipCodecConv2d is CD.HipCodecConv2d and dda.HipCodecConvTranspose2d is CD.HipCodecConvTranspose2d
    assert dda.HipCodecTail is CD.HipCodecTail and dda.convert_hip_codec is CD.convert_hip_codec


def test_the_functions_refuse_cpu_tensors():
    x = torch.randn(1, 16, 4, 5, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        CD.Enc1Function.apply(x, torch.randn(16, 16, 3, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        CD.Dec0Function.apply(x, torch.randn(16, 16, 4, 4), torch.randn(16))
    with pytest.raises(RuntimeError, match="HIP device"):
        CD.TailFunction.apply(x, 1e-6)


def test_the_four_geometries_and_nothing_else():
    assert CD.codec_op(nn.Conv2d(1, 16, 3, 2, 1, bias=False)) == CD.OP_ENC0
    assert CD.codec_op(nn.Conv2d(16, 16, 3, 1, 1, bias=False)) == CD.OP_ENC1
    assert CD.codec_op(nn.ConvTranspose2d(16, 16, 4, 2, 1)) == CD.OP_DEC0
    assert CD.codec_op(nn.Conv2d(16, 1, 3, 1, 1)) == CD.OP_DEC1
    for m in (nn.Conv2d(1, 16, 3, 2, 1), nn.Conv2d(16, 16, 3, 1, 1), nn.Conv2d(16, 1, 3, 1, 1, bias=False), nn.ConvTranspose2d(16, 16, 4, 2, 1, bias=False),
              nn.Conv2d(16, 16, 3, 2, 1, bias=False), nn.Conv2d(16, 16, 3, 1, 1, bias=False, groups=2), nn.Conv2d(16, 16, 3, 1, 1, bias=False, dilation=2),
              nn.ConvTranspose2d(16, 16, 4, 2, 1, output_padding=1), nn.ConvTranspose2d(16, 16, 2, 2), nn.Conv2d(32, 16, 3, 1, 1, bias=False),
              nn.Conv2d(16, 16, 3, 1, "same", bias=False), nn.Sigmoid()):
        assert CD.codec_op(m) is None, m


def _codec(seed=3):
    torch.manual_seed(seed)
    return dda.DeepDepthTransformWithUpsampling()


def _types(dt):
    return [type(dt.conv_transform[0][0]), type(dt.conv_transform[1][0]), type(dt.conv_inv_transform[0]), type(dt.conv_inv_transform[3][0]),
            type(dt.conv_inv_transform[4])]


@pytest.mark.parametrize("order", ["codec", "codec+bn", "bn+codec"])
def test_converter_keeps_tensors_keys_and_indices_in_either_order_with_the_batchnorm_converter(order):
    dt = _codec()
    assert _types(dt) == [nn.Conv2d, nn.Conv2d, nn.ConvTranspose2d, nn.Conv2d, nn.Sigmoid]
    before = {k: v.data_ptr() for k, v in dt.state_dict().items()}
    params = [id(p) for p in dt.parameters()]
    for step in order.split("+"):
        out = CD.convert_hip_codec(dt) if step == "codec" else BN.convert_hip_batchnorm(dt)
        assert out is dt
    assert list(dt.state_dict()) == list(before)
    assert {k: v.data_ptr() for k, v in dt.state_dict().items()} == before and [id(p) for p in dt.parameters()] == params
    assert _types(dt) == [CD.HipCodecConv2d, CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecConv2d, CD.HipCodecTail]
    assert dt.conv_inv_transform[4].eps == dt.eps == 1e-6
    assert len(dt.conv_transform) == 3 and len(dt.conv_inv_transform) == 5 and type(dt.conv_transform[2]) is nn.Tanh
    bns = [dt.conv_transform[0][1], dt.conv_transform[1][1], dt.conv_inv_transform[1]]
    assert all(isinstance(b, BN.HipBatchNorm2d) == ("bn" in order) for b in bns)
    mods = [id(m) for m in dt.modules()]
    assert CD.convert_hip_codec(dt) is dt and [id(m) for m in dt.modules()] == mods      # idempotent: nothing is replaced twice
    with pytest.raises(TypeError):
        CD.convert_hip_codec(nn.Sequential(nn.Sigmoid()))


@pytest.mark.parametrize("train", [True, False])
def test_converted_codec_on_cpu_tensors_is_the_unconverted_one_bit_for_bit(train):
    a, b = _codec(), CD.convert_hip_codec(_codec())
    a.train(train), b.train(train)
    g = torch.Generator().manual_seed(1)
    depth = torch.rand(2, 1, 12, 20, generator=g) * 10
    lat = torch.randn(2, 16, 6, 10, generator=g)
    la, lb = lat.clone().requires_grad_(True), lat.clone().requires_grad_(True)
    ta, tb = a.t(depth), b.t(depth)
    da, db = a.inv_t(la), b.inv_t(lb)
    assert torch.equal(ta, tb) and torch.equal(da, db)
    (ta.sum() + da.log1p().sum()).backward()
    (tb.sum() + db.log1p().sum()).backward()
    assert torch.equal(la.grad, lb.grad)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    assert torch.equal(b.conv_inv_transform[4](lat), torch.sigmoid(lat))      # off the library route the tail is the sigmoid it inherits


def test_needs_input_grad_is_honoured(monkeypatch):
    """The Functions' backward asks only for the gradients autograd needs (driven on stand-ins of the library calls: no device here)."""
    calls = []
    monkeypatch.setattr(CD, "conv_forward", lambda op, x, w, bias=None: x.new_zeros(x.shape[0], CD.GEOMETRY[op][1], *CD.output_hw(op, *x.shape[2:])))
    monkeypatch.setattr(CD, "conv_backward_data", lambda op, gy, w, shape: (calls.append("data"), gy.new_zeros(tuple(shape)))[1])
    monkeypatch.setattr(CD, "conv_backward_weight", lambda op, x, gy, need_bias=False: (
        calls.append("weight+bias" if need_bias else "weight"), (gy.new_zeros(CD.weight_shape(op)), gy.new_zeros(CD.GEOMETRY[op][1]) if need_bias else None))[1])
    for need_x, need_w, need_b, want in ((True, True, True, ["data", "weight+bias"]), (False, True, True, ["weight+bias"]), (True, False, False, ["data"]),
                                         (False, True, False, ["weight"]), (False, False, True, ["weight+bias"])):
        calls.clear()
        x = torch.randn(1, 16, 4, 5, requires_grad=need_x)
        w = torch.randn(16, 16, 4, 4, requires_grad=need_w)
        b = torch.randn(16, requires_grad=need_b)
        CD.Dec0Function.apply(x, w, b).sum().backward()
        assert calls == want and (x.grad is not None) == need_x and (w.grad is not None) == need_w and (b.grad is not None) == need_b
    calls.clear()
    x, w = torch.randn(1, 1, 4, 5), torch.randn(16, 1, 3, 3, requires_grad=True)      # ENC0 in a head: the ground-truth depth carries no gradient
    CD.Enc0Function.apply(x, w).sum().backward()
    assert calls == ["weight"]
    assert not CD.Enc1Function.apply(torch.randn(1, 16, 4, 5), torch.randn(16, 16, 3, 3)).requires_grad


# ---- heads --------------------------------------------------------------------------------------------------------------------------------
def _census(head):
    return [type(m) for m in head.depth_transform.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Sigmoid))]


def test_codec_backend_keyword_and_environment_variable(monkeypatch):
    monkeypatch.delenv("DDEPTH_CODEC_BACKEND", raising=False)
    assert CD.resolve_codec_backend() == "torch" and CD.resolve_codec_backend("hip") == "hip"
    plain = dda.DDIMDepthEstimate_Res(inference_steps=2)
    assert plain.codec_backend == "torch"
    assert _census(plain) == [nn.Conv2d, nn.Conv2d, nn.ConvTranspose2d, nn.Conv2d, nn.Sigmoid]      # the default: every codec child a plain torch module
    assert not any(isinstance(m, HIP_TYPES) for m in plain.modules())
    monkeypatch.setenv("DDEPTH_CODEC_BACKEND", "")
    assert dda.DDIMDepthEstimate_Res(inference_steps=2).codec_backend == "torch"
    monkeypatch.setenv("DDEPTH_CODEC_BACKEND", "hip")
    head = dda.DDIMDepthEstimate_Res(inference_steps=2)              # an fp32 head takes it too: the codec is fp32 in every precision mode
    assert head.codec_backend == "hip" and head.model.precision == "fp32"
    assert _census(head) == [CD.HipCodecConv2d, CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecConv2d, CD.HipCodecTail]
    assert sum(isinstance(m, HIP_TYPES) for m in head.modules()) == 5      # nothing outside the codec
    assert dda.DDIMDepthEstimate_Res(inference_steps=2, codec_backend="torch").codec_backend == "torch"      # the keyword wins
    monkeypatch.setenv("DDEPTH_CODEC_BACKEND", "miopen")
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Res(inference_steps=2)
    monkeypatch.delenv("DDEPTH_CODEC_BACKEND")
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Res(inference_steps=2, codec_backend="miopen")


@pytest.mark.parametrize("cls,kw", [("DDIMDepthEstimate_Res", {}), ("DDIMDepthEstimate_Swin_ADDHAHI", {"in_channels": [192, 384, 768, 1536]})])
def test_head_conversion_keeps_keys_and_loads_a_default_state_dict(cls, kw):
    torch.manual_seed(0)
    a = getattr(dda, cls)(inference_steps=2, **kw)
    b = getattr(dda, cls)(inference_steps=2, codec_backend="hip", bn_backend="hip", **kw)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())                       # strict
    assert _census(b) == [CD.HipCodecConv2d, CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecConv2d, CD.HipCodecTail]
    assert len(a._bound._signature("codec")) == len(b._bound._signature("codec")) > 0
