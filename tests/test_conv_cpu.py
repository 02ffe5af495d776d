"""CPU: everything about diffusiondepth_amd.conv that needs no GPU -- the C ABI of include/ddepth_conv.h (declared == bound == exported, the support
and workspace queries), the converter (same tensors, same keys, same indices), the head keyword / environment variable, and that on CPU tensors
the converted modules ARE nn.Conv2d / nn.ConvTranspose2d, bit for bit, forward and gradients."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import backend
from diffusiondepth_amd import conv as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_header_declares_the_bound_symbols_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ddepth_conv.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(CV.ABI_SYMBOLS), declared ^ set(CV.ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    assert not any(s in main for s in declared) and not declared & set(backend.ABI_SYMBOLS)


def test_support_and_workspace_queries_need_no_device():
    lib = CV._lib()
    for p in ("bf16", "f16", "f16x3"):
        assert CV.supported(CV.OP_CONV3X3, 64, 256, p) and CV.supported(CV.OP_DECONV2X2, 256, 256, p) and CV.supported(CV.OP_CONV3X3, 1536, 256, p)
        assert CV.supported(CV.OP_CONV3X3, 256, 192, p)                                  # the data gradient's direction of a Swin lateral
        assert not CV.supported(CV.OP_CONV3X3, 216, 256, p) and not CV.supported(CV.OP_CONV3X3, 64, 1600, p)      # MPViT's 216; beyond 1536
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported(CV.OP_CONV3X3, 64, 256, p) and CV.precision_id(p) is None
    n, small = ctypes.c_int64(0), ctypes.c_int64(0)
    # lateral0 at KITTI size, B = 4: the weight gradient's partials (at most 64 splits of Cout * Cin * 9 floats)
    assert lib.dd_conv_workspace_bytes(0, 4, 64, 256, 176, 608, 2, ctypes.byref(n)) == 0 and 64 * 256 * 9 * 4 <= n.value <= 64 * 64 * 256 * 9 * 4
    assert lib.dd_conv_workspace_bytes(0, 1, 64, 64, 3, 5, 2, ctypes.byref(small)) == 0 and 0 < small.value < n.value
    assert lib.dd_conv_workspace_bytes(0, 1, 216, 256, 3, 5, 2, ctypes.byref(small)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv_workspace_bytes(0, 0, 64, 64, 3, 5, 2, ctypes.byref(small)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3_forward(None, None, None, None, 1, 64, 64, 3, 5, 2, None) != 0 and b"null" in lib.dd_conv_last_error()


def test_exports():
    assert dda.HipConv2d is CV.HipConv2d and dda.HipConvTranspose2d is CV.HipConvTranspose2d and dda.convert_hip_conv is CV.convert_hip_conv


def test_the_functions_refuse_cpu_tensors():
    x, w = torch.randn(1, 64, 4, 5, requires_grad=True), torch.randn(64, 64, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.Conv3x3Function.apply(x, w, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.ConvTranspose2x2Function.apply(x, torch.randn(64, 64, 2, 2), 2)


def _small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(64, 128, 3, 1, 1, bias=False), nn.BatchNorm2d(128), nn.ReLU(True),
                         nn.Sequential(nn.ConvTranspose2d(128, 64, 2, 2, bias=False), nn.ReLU()),
                         nn.Conv2d(64, 64, 3, 1, 1, bias=True),              # a bias
                         nn.Conv2d(64, 64, 3, 2, 1, bias=False),             # stride 2
                         nn.Conv2d(64, 48, 3, 1, 1, bias=False),             # 48 output channels
                         nn.ConvTranspose2d(48, 64, 2, 2, bias=False),       # 48 input channels
                         nn.Conv2d(64, 64, 1, bias=False),                   # 1x1
                         nn.Conv2d(64, 64, 3, 1, 1, bias=False, groups=2))


def test_converter_keeps_tensors_keys_and_indices_and_takes_only_eligible_convolutions():
    net = _small_net()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    params = [id(p) for p in net.parameters()]
    out = CV.convert_hip_conv(net, "bf16")
    assert out is net and list(net.state_dict()) == list(before)
    assert {k: v.data_ptr() for k, v in net.state_dict().items()} == before and [id(p) for p in net.parameters()] == params
    assert type(net[0]) is CV.HipConv2d and net[0].precision == "bf16" and type(net[3][0]) is CV.HipConvTranspose2d
    assert [type(net[i]) for i in (4, 5, 6, 8, 9)] == [nn.Conv2d] * 5 and type(net[7]) is nn.ConvTranspose2d
    assert "precision=bf16" in repr(net[0])
    assert CV.convert_hip_conv(net, "bf16") is net and type(net[0]) is CV.HipConv2d              # idempotent
    for p in ("fp32", "f16r", "naive_fp32"):                                                     # nothing is eligible: nothing is replaced
        other = CV.convert_hip_conv(_small_net(), p)
        assert not any(isinstance(m, (CV.HipConv2d, CV.HipConvTranspose2d)) for m in other.modules())


def test_converted_net_on_cpu_tensors_is_the_unconverted_one_bit_for_bit():
    a, b = _small_net(), CV.convert_hip_conv(_small_net(), "f16x3")
    x = torch.randn(2, 64, 6, 10, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    (ya ** 2).sum().backward()
    (yb ** 2).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))


def test_needs_input_grad_is_honoured(monkeypatch):
    """The Function's backward asks only for the gradients autograd needs (driven on stand-ins of the two library calls: no device here)."""
    calls = []
    monkeypatch.setattr(CV, "conv_forward", lambda op, x, w, prec: x.new_zeros(x.shape[0], w.shape[0], *x.shape[2:]))
    monkeypatch.setattr(CV, "conv_backward_data", lambda op, gy, w, shape, prec: (calls.append("data"), gy.new_zeros(tuple(shape)))[1])
    monkeypatch.setattr(CV, "conv_backward_weight", lambda op, x, gy, shape, prec: (calls.append("weight"), gy.new_zeros(tuple(shape)))[1])
    for need_x, need_w, want in ((True, True, ["data", "weight"]), (False, True, ["weight"]), (True, False, ["data"])):
        calls.clear()
        x = torch.randn(1, 64, 4, 5, requires_grad=need_x)
        w = torch.randn(64, 64, 3, 3, requires_grad=need_w)
        y = CV.Conv3x3Function.apply(x, w, 2)
        y.sum().backward()
        assert calls == want and (x.grad is not None) == need_x and (w.grad is not None) == need_w
    x, w = torch.randn(1, 64, 4, 5), torch.randn(64, 64, 3, 3)
    assert not CV.Conv3x3Function.apply(x, w, 2).requires_grad


# ---- heads --------------------------------------------------------------------------------------------------------------------------------
def _census(head):
    return [(n, type(m)) for n, m in head.named_modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))
            and n.split(".")[0] in ("conv_lateral", "conv_up", "convup_fp")]


def test_conv_backend_keyword_and_environment_variable(monkeypatch):
    monkeypatch.delenv("DDEPTH_CONV_BACKEND", raising=False)
    plain = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16")
    assert plain.conv_backend == "torch" and len(_census(plain)) == 8
    assert not any(isinstance(m, (CV.HipConv2d, CV.HipConvTranspose2d)) for m in plain.modules())
    monkeypatch.setenv("DDEPTH_CONV_BACKEND", "")
    assert dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16").conv_backend == "torch"
    monkeypatch.setenv("DDEPTH_CONV_BACKEND", "hip")
    head = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16")
    assert head.conv_backend == "hip" and [n for n, _ in _census(head)] == [n for n, _ in _census(plain)]
    assert all(t in (CV.HipConv2d, CV.HipConvTranspose2d) for _, t in _census(head))
    assert all(m.precision == "bf16" for m in head.modules() if isinstance(m, (CV.HipConv2d, CV.HipConvTranspose2d)))
    assert dda.DDIMDepthEstimate_Res(inference_steps=2, conv_backend="torch").conv_backend == "torch"      # the keyword wins
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Res(inference_steps=2, conv_backend="miopen")
    # the default head is fp32: the keyword is honoured, nothing is eligible, nothing is replaced
    fp32 = dda.DDIMDepthEstimate_Res(inference_steps=2, conv_backend="hip")
    assert fp32.model.precision == "fp32" and not any(isinstance(m, (CV.HipConv2d, CV.HipConvTranspose2d)) for m in fp32.modules())


@pytest.mark.parametrize("cls,kw", [("DDIMDepthEstimate_Res", {}), ("DDIMDepthEstimate_Swin_ADD", {"in_channels": [192, 384, 768, 1536]})])
def test_head_conversion_keeps_keys_and_loads_a_default_state_dict(cls, kw):
    torch.manual_seed(0)
    a = getattr(dda, cls)(inference_steps=2, precision="f16x3", conv_backend="torch", **kw)
    b = getattr(dda, cls)(inference_steps=2, precision="f16x3", conv_backend="hip", bn_backend="hip", **kw)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())                       # strict
    assert type(b.conv_lateral[0][0]) is CV.HipConv2d and type(b.conv_up[0][0]) is CV.HipConvTranspose2d and type(b.convup_fp[0]) is CV.HipConvTranspose2d
    assert b.conv_lateral[3][0].in_channels == a.conv_lateral[3][0].in_channels
    assert len(a._bound._signature("fpn")) == len(b._bound._signature("fpn")) > 0


def test_mpvit_widths_keep_the_torch_convolutions_where_unsupported():
    head = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=[128, 216, 288, 288], inference_steps=2, precision="bf16", conv_backend="hip")
    kinds = [type(head.conv_lateral[i][0]) for i in range(4)]
    assert kinds == [CV.HipConv2d, nn.Conv2d, nn.Conv2d, nn.Conv2d]      # 128 is a multiple of 64; 216 and 288 are not


def test_res_head_train_forward_and_backward_on_cpu_are_bit_identical_after_conversion():
    from diffusiondepth_amd import synth
    torch.manual_seed(0)
    a = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="torch").train()
    b = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="hip").train()
    b.load_state_dict(a.state_dict())
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, 2, 32, 64)]
    up = torch.randn(2, 256, 16, 32, generator=torch.Generator().manual_seed(4))
    res = []
    for head in (a, b):
        f = [t.clone().requires_grad_(True) for t in fp]
        cond = head.aggregate_condition(f)
        cond.backward(up)
        res.append((cond, f))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(res[0][1], res[1][1]))
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
