"""CPU: the pointwise (1x1) operator and the HAHI neck's conversion, as far as no GPU is needed -- the support and workspace queries for
dd_conv_op 2, that Conv1x1Function refuses CPU tensors, the converter with and without ``pointwise``, the head's "hip+neck" back end (keyword and
environment variable; same tensors, same keys), and that on CPU tensors a converted neck IS the unconverted one, bit for bit."""
import ctypes

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import conv as CV

SWIN_L = [192, 384, 768, 1536]


def test_support_and_workspace_queries_for_the_pointwise_operator():
    lib = CV._lib()
    assert CV.OP_CONV1X1 == 2 and set(CV._ENTRY[CV.OP_CONV1X1]) <= set(CV.ABI_SYMBOLS)
    for p in ("bf16", "f16", "f16x3"):
        for c in SWIN_L:
            assert CV.supported(CV.OP_CONV1X1, c, c, p) and CV.supported(CV.OP_CONV1X1, c, 512, p) and CV.supported(CV.OP_CONV1X1, 512, c, p)
        assert not CV.supported(CV.OP_CONV1X1, 216, 512, p) and not CV.supported(CV.OP_CONV1X1, 2048, 1536, p) and not CV.supported(CV.OP_CONV1X1, 32, 64, p)
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported(CV.OP_CONV1X1, 192, 192, p)
    assert not CV.supported(3, 64, 64, "bf16")
    n, small = ctypes.c_int64(0), ctypes.c_int64(0)
    # conv_proj at KITTI size, B = 4: the weight gradient's partials (at most 64 splits of Cout * Cin floats); the packed weights at a tiny plane
    assert lib.dd_conv_workspace_bytes(2, 4, 192, 512, 88, 304, 2, ctypes.byref(n)) == 0 and 192 * 512 * 4 < n.value <= 64 * 192 * 512 * 4
    assert lib.dd_conv_workspace_bytes(2, 1, 64, 64, 1, 3, 4, ctypes.byref(small)) == 0 and small.value == 64 * 64 * 4      # one split; hi and lo are as large
    assert lib.dd_conv_workspace_bytes(2, 1, 216, 512, 3, 5, 2, ctypes.byref(small)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv_workspace_bytes(2, 0, 64, 64, 3, 5, 2, ctypes.byref(small)) == 1 and b"positive" in lib.dd_conv_last_error()
    assert lib.dd_conv1x1_forward(None, None, None, None, 1, 64, 64, 3, 5, 2, None) != 0 and b"null" in lib.dd_conv_last_error()


def test_the_pointwise_function_refuses_cpu_tensors():
    x, w = torch.randn(1, 64, 4, 5, requires_grad=True), torch.randn(64, 64, 1, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.Conv1x1Function.apply(x, w, 2)


def _small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(64, 128, 1, bias=False), nn.BatchNorm2d(128), nn.ReLU(True),
                         nn.Sequential(nn.Conv2d(128, 64, 3, 1, 1, bias=False), nn.ReLU()),
                         nn.Conv2d(64, 64, 1, bias=True),                    # a bias
                         nn.Conv2d(64, 64, 1, 2, bias=False),                # stride 2
                         nn.Conv2d(64, 48, 1, bias=False),                   # 48 output channels
                         nn.Conv2d(48, 64, 1, 1, 1, bias=False),             # padding 1
                         nn.Conv2d(64, 64, 1, bias=False, groups=2),
                         nn.Conv2d(64, 64, 1, bias=False))


def test_converter_takes_a_pointwise_convolution_only_when_asked_to():
    net = _small_net()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    params = [id(p) for p in net.parameters()]
    assert not CV.eligible(net[0], "bf16") and CV.eligible(net[0], "bf16", pointwise=True) and not CV.eligible(net[4], "bf16", pointwise=True)
    assert CV.convert_hip_conv(net, "bf16") is net                                       # the default: today's behaviour
    assert type(net[0]) is nn.Conv2d and type(net[9]) is nn.Conv2d and type(net[3][0]) is CV.HipConv2d
    out = CV.convert_hip_conv(net, "bf16", pointwise=True)
    assert out is net and list(net.state_dict()) == list(before)
    assert {k: v.data_ptr() for k, v in net.state_dict().items()} == before and [id(p) for p in net.parameters()] == params
    assert type(net[0]) is CV.HipConv2d and type(net[9]) is CV.HipConv2d and net[0].precision == "bf16" and net[0].kernel_size == (1, 1)
    assert [type(net[i]) for i in (4, 5, 6, 7, 8)] == [nn.Conv2d] * 5
    assert "precision=bf16" in repr(net[0])
    first = net[0]
    assert CV.convert_hip_conv(net, "bf16", pointwise=True) is net and net[0] is first     # idempotent
    for p in ("fp32", "f16r", "naive_fp32"):                                               # nothing is eligible: nothing is replaced
        other = CV.convert_hip_conv(_small_net(), p, pointwise=True)
        assert not any(isinstance(m, CV.HipConv2d) for m in other.modules())


def test_a_pointwise_module_on_cpu_tensors_and_other_geometries_runs_torch():
    m = CV.HipConv2d(64, 64, 1, 1, 0, precision="bf16")
    x = torch.randn(1, 64, 3, 5)
    assert m._native(x) is None and torch.equal(m(x), nn.functional.conv2d(x, m.weight))
    assert CV.HipConv2d(64, 64, 5, 1, 2, precision="bf16")._native(x) is None


def _neck_convs(head_or_neck):
    return {n: type(m) for n, m in head_or_neck.named_modules() if isinstance(m, nn.Conv2d)}


def test_hip_neck_backend_keyword_and_environment_variable(monkeypatch):
    monkeypatch.delenv("DDEPTH_CONV_BACKEND", raising=False)
    torch.manual_seed(0)
    kw = dict(in_channels=list(SWIN_L), inference_steps=2, precision="f16x3")
    plain = dda.DDIMDepthEstimate_Swin_ADDHAHI(**kw)
    hip = dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip", **kw)
    assert plain.conv_backend == "torch" and hip.conv_backend == "hip"
    assert _neck_convs(hip.hahineck) == _neck_convs(plain.hahineck) and set(_neck_convs(plain.hahineck).values()) == {nn.Conv2d}     # "hip" leaves the neck alone
    assert type(hip.conv_lateral[0][0]) is CV.HipConv2d
    monkeypatch.setenv("DDEPTH_CONV_BACKEND", "hip+neck")
    both = dda.DDIMDepthEstimate_Swin_ADDHAHI(**kw)
    monkeypatch.delenv("DDEPTH_CONV_BACKEND")
    keyword = dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip+neck", bn_backend="hip", **kw)
    for head in (both, keyword):
        assert head.conv_backend == "hip+neck"
        kinds = _neck_convs(head.hahineck)
        assert len(kinds) == 12 and kinds.pop("trans_fusion.2.conv") is nn.Conv2d                 # 2048 input channels: beyond the library's 1536
        assert set(kinds.values()) == {CV.HipConv2d}
        assert all(m.precision == "f16x3" for m in head.hahineck.modules() if isinstance(m, CV.HipConv2d))
        assert sorted(m.kernel_size for m in head.hahineck.modules() if isinstance(m, CV.HipConv2d)) == [(1, 1)] * 8 + [(3, 3)] * 3
        assert type(head.conv_lateral[0][0]) is CV.HipConv2d and type(head.conv_up[0][0]) is CV.HipConvTranspose2d      # everything "hip" does
        assert list(head.state_dict()) == list(plain.state_dict())
        head.load_state_dict(plain.state_dict())                                                  # strict
    # a head without a neck: "hip+neck" equals "hip"
    res = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="hip+neck")
    ref = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="hip")
    assert res.conv_backend == "hip+neck" and [(n, type(m)) for n, m in res.named_modules()] == [(n, type(m)) for n, m in ref.named_modules()]
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip+fpn", **kw)


def test_mpvit_widths_convert_what_is_supported_and_leave_the_rest():
    head = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=[128, 216, 288, 288], inference_steps=2, precision="bf16", conv_backend="hip+neck")
    converted = sorted(n for n, t in _neck_convs(head.hahineck).items() if t is CV.HipConv2d)
    assert converted == ["conv_fusion.0.conv", "conv_proj.0.conv", "lateral_convs.0.conv"]        # 640 -> 128 (3x3), 128 -> 512, 128 -> 128
    assert len(_neck_convs(head.hahineck)) == 12


def _small_neck():
    torch.manual_seed(11)
    neck = dda.HAHIHeteroNeck([64, 128, 192, 256], [64, 128, 192, 256], embedding_dim=64, cross_att=False, self_att=False)
    neck.init_weights()
    return neck.train()


def test_a_converted_small_neck_on_cpu_tensors_is_the_unconverted_one_bit_for_bit():
    a, b = _small_neck(), CV.convert_hip_conv(_small_neck(), "f16x3", pointwise=True)
    assert sum(isinstance(m, CV.HipConv2d) for m in b.modules()) == 12 and list(a.state_dict()) == list(b.state_dict())
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip((64, 128, 192, 256), ((12, 20), (6, 10), (3, 5), (2, 3)))]
    res = []
    for neck in (a, b):
        f = [t.clone().requires_grad_(True) for t in xs]
        outs = neck(f)
        sum((o ** 2).sum() for o in outs).backward()
        res.append((outs, f))
    assert all(torch.equal(p, q) for p, q in zip(res[0][0], res[1][0]))
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(res[0][1], res[1][1]))
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
