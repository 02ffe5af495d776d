"""CPU: the extended channel range of diffusiondepth_amd.conv (``channels="any"``, dd_convx_*: multiples of 8 in 8..2048) and the head back end
"hip+all", as far as no GPU is needed -- the ABI (declared == bound == exported), the support queries beside the block-64 ones, the census of the
MPViT, Swin-L and Res heads (every FPN and neck convolution converted; same tensors, same keys), the environment variable, that on CPU tensors
the converted modules are the unconverted ones bit for bit, and that every default still behaves as before."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
from diffusiondepth_amd import conv as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPVIT, SWIN_L = [128, 216, 288, 288], [192, 384, 768, 1536]
NEW = ["dd_convx_supported", "dd_convx_workspace_bytes", "dd_convx_forward", "dd_convx_backward_data", "dd_convx_backward_weight"]
HIP = (CV.HipConv2d, CV.HipConvTranspose2d)


def test_the_header_the_bound_set_and_the_library_agree_on_the_five_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "ddepth_conv.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(CV.ABI_SYMBOLS) and set(NEW) <= declared and len(CV.ABI_SYMBOLS) == 17
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    assert "multiples of 8 in 8 .. 2048" in hdr and "multiples of 64 in 64 .. 1536" in hdr      # the "Channels:" paragraph states both contracts


def test_supported_with_channels_any_beside_the_block64_answers():
    for p in ("bf16", "f16", "f16x3"):
        for op in (CV.OP_CONV3X3, CV.OP_DECONV2X2, CV.OP_CONV1X1):
            for cin, cout in ((8, 8), (216, 256), (2048, 1536), (288, 512), (728, 216), (72, 8)):
                assert CV.supported(op, cin, cout, p, "any") and CV.supported(op, cin, cout, p, channels="any")
                assert not CV.supported(op, cin, cout, p) and not CV.supported(op, cin, cout, p, "block64")
            for cin, cout in ((64, 256), (1536, 192)):                       # a block-64 pair: both contracts take it
                assert CV.supported(op, cin, cout, p, "any") and CV.supported(op, cin, cout, p)
            for c in (4, 12, 2056, 0):
                assert not CV.supported(op, c, 64, p, "any") and not CV.supported(op, 64, c, p, "any")
        assert not CV.supported(3, 72, 72, p, "any")
    for p in ("fp32", "f16r", "naive_fp32"):
        assert not CV.supported(CV.OP_CONV3X3, 72, 72, p, "any")
    with pytest.raises(ValueError):
        CV.supported(CV.OP_CONV3X3, 72, 72, "bf16", "all")


def test_workspace_queries_of_the_extended_range_need_no_device():
    lib = CV._lib()
    n, old = ctypes.c_int64(0), ctypes.c_int64(0)
    # Swin-L trans_fusion.2 at the KITTI level-3 geometry, B = 4: six splits of 2048 * 1536 * 9 floats
    assert lib.dd_convx_workspace_bytes(0, 4, 2048, 1536, 11, 38, 2, ctypes.byref(n)) == 0 and n.value == 6 * 2048 * 1536 * 9 * 4
    assert lib.dd_conv_workspace_bytes(0, 4, 2048, 1536, 11, 38, 2, ctypes.byref(old)) == 4 and b"unsupported" in lib.dd_conv_last_error()
    # a block-64 shape: the same size through both queries
    assert lib.dd_convx_workspace_bytes(0, 4, 64, 256, 176, 608, 2, ctypes.byref(n)) == 0
    assert lib.dd_conv_workspace_bytes(0, 4, 64, 256, 176, 608, 2, ctypes.byref(old)) == 0 and n.value == old.value
    # a ragged 1x1 at one pixel, split mode: the padded image (128 rows of 96, hi and lo) is larger than 72 * 72 weights
    assert lib.dd_convx_workspace_bytes(2, 1, 72, 72, 1, 1, 4, ctypes.byref(n)) == 0 and n.value == 128 * 96 * 2 * 2
    assert lib.dd_convx_workspace_bytes(2, 1, 12, 72, 1, 1, 4, ctypes.byref(n)) == 4 and b"multiples of 8" in lib.dd_conv_last_error()
    assert lib.dd_convx_forward(0, None, None, None, None, 1, 72, 72, 3, 5, 2, None) != 0 and b"null" in lib.dd_conv_last_error()


def test_the_functions_refuse_cpu_tensors_on_the_extended_route_too():
    x = torch.randn(1, 72, 4, 5, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.Conv3x3Function.apply(x, torch.randn(72, 72, 3, 3), 2, "any")
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.Conv1x1Function.apply(x, torch.randn(216, 72, 1, 1), 2, "any")
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.ConvTranspose2x2Function.apply(x, torch.randn(72, 88, 2, 2), 2, "any")
    with pytest.raises(ValueError):
        CV.conv_forward(CV.OP_CONV3X3, x, torch.randn(72, 72, 3, 3), 2, "all")


def test_the_choice_travels_positionally_and_in_ctx_conf(monkeypatch):
    """The autograd Functions hand ``channels`` to the three direction functions as a trailing positional argument (callers wrap them with
    ``lambda *a``) and only when it is not the default, and carry it to the backward in ``ctx.conf``."""
    seen = []
    monkeypatch.setattr(CV, "conv_forward", lambda *a: (seen.append(("fwd",) + a[4:]), a[1].new_zeros(a[1].shape[0], a[2].shape[0], *a[1].shape[2:]))[1])
    monkeypatch.setattr(CV, "conv_backward_data", lambda *a: (seen.append(("data",) + a[5:]), a[1].new_zeros(tuple(a[3])))[1])
    monkeypatch.setattr(CV, "conv_backward_weight", lambda *a: (seen.append(("weight",) + a[5:]), a[1].new_zeros(tuple(a[3])))[1])
    for channels, extra in (("any", ("any",)), ("block64", ())):
        seen.clear()
        x, w = torch.randn(1, 72, 4, 5, requires_grad=True), torch.randn(72, 72, 3, 3, requires_grad=True)
        y = CV.Conv3x3Function.apply(x, w, 2, channels)
        assert y.grad_fn.conf == (CV.OP_CONV3X3, 2, channels)
        y.sum().backward()
        assert seen == [("fwd",) + extra, ("data",) + extra, ("weight",) + extra]


def _small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(72, 216, 3, 1, 1, bias=False), nn.BatchNorm2d(216), nn.ReLU(True),
                         nn.Sequential(nn.ConvTranspose2d(216, 88, 2, 2, bias=False), nn.ReLU()),
                         nn.Conv2d(88, 64, 1, bias=False),                   # 1x1
                         nn.Conv2d(64, 64, 3, 1, 1, bias=False),             # block-64
                         nn.Conv2d(64, 60, 3, 1, 1, bias=False),             # 60 output channels: no multiple of 8
                         nn.Conv2d(60, 72, 3, 1, 1, bias=True))              # a bias


def test_converter_passes_the_choice_through_and_the_default_is_unchanged():
    net = _small_net()
    before = {k: v.data_ptr() for k, v in net.state_dict().items()}
    assert not CV.eligible(net[0], "bf16") and CV.eligible(net[0], "bf16", False, "any") and CV.eligible(net[0], "bf16", channels="any")
    assert not CV.eligible(net[4], "bf16", False, "any") and CV.eligible(net[4], "bf16", True, "any") and not CV.eligible(net[6], "bf16", True, "any")
    assert CV.convert_hip_conv(net, "bf16") is net                       # the default: the block-64 contract, no 1x1
    assert [type(net[i]) for i in (0, 4, 6, 7)] == [nn.Conv2d] * 4 and type(net[3][0]) is nn.ConvTranspose2d and type(net[5]) is CV.HipConv2d
    assert net[5].channels == "block64" and "channels" not in net[5].__dict__ and "channels" not in repr(net[5])
    out = CV.convert_hip_conv(net, "bf16", pointwise=True, channels="any")
    assert out is net and list(net.state_dict()) == list(before) and {k: v.data_ptr() for k, v in net.state_dict().items()} == before
    assert type(net[0]) is CV.HipConv2d and type(net[3][0]) is CV.HipConvTranspose2d and type(net[4]) is CV.HipConv2d
    assert [type(net[i]) for i in (6, 7)] == [nn.Conv2d] * 2
    assert net[0].channels == net[3][0].channels == net[4].channels == "any" and net[5].channels == "block64"      # (converted before: left alone)
    assert "precision=bf16, channels=any" in repr(net[0]) and "channels=any" in repr(net[3][0])
    assert CV.HipConv2d.channels == "block64" and CV.HipConvTranspose2d.channels == "block64"
    assert CV.HipConv2d(72, 72, precision="bf16").channels == "block64"
    for p in ("fp32", "f16r", "naive_fp32"):
        other = CV.convert_hip_conv(_small_net(), p, True, "any")
        assert not any(isinstance(m, HIP) for m in other.modules())
    with pytest.raises(ValueError):
        CV.convert_hip_conv(_small_net(), "bf16", True, "all")


def test_converted_net_on_cpu_tensors_is_the_unconverted_one_bit_for_bit():
    a, b = _small_net(), CV.convert_hip_conv(_small_net(), "f16x3", True, "any")
    assert sum(isinstance(m, HIP) for m in b.modules()) == 4
    x = torch.randn(2, 72, 6, 10, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    (ya ** 2).sum().backward()
    (yb ** 2).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))


# ---- heads --------------------------------------------------------------------------------------------------------------------------------
def _convs(module):
    return {n: m for n, m in module.named_modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))}


def test_mpvit_head_with_hip_all_converts_every_fpn_and_neck_convolution():
    torch.manual_seed(0)
    plain = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=list(MPVIT), inference_steps=2, precision="bf16")
    head = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=list(MPVIT), precision="bf16", conv_backend="hip+all")
    assert head.conv_backend == "hip+all"
    laterals = [head.conv_lateral[i][0] for i in range(4)]
    assert [type(m) for m in laterals] == [CV.HipConv2d] * 4 and [m.in_channels for m in laterals] == MPVIT
    ups = [head.conv_up[i][0] for i in range(3)]
    assert [type(m) for m in ups] == [CV.HipConvTranspose2d] * 3
    neck = _convs(head.hahineck)
    assert len(neck) == 12 and all(type(m) is CV.HipConv2d for m in neck.values())
    assert sorted(m.kernel_size for m in neck.values()) == [(1, 1)] * 8 + [(3, 3)] * 4
    assert {(m.in_channels, m.out_channels) for m in neck.values()} >= {(216, 216), (288, 288), (216, 512), (288, 512), (728, 216), (800, 288)}
    assert all(m.channels == "any" and m.precision == "bf16" for m in laterals + ups + list(neck.values()))
    assert list(head.state_dict()) == list(plain.state_dict())
    head.load_state_dict(plain.state_dict())                                                      # strict
    assert not hasattr(head, "convup_fp")


def test_swin_l_head_with_hip_all_converts_all_twelve_neck_convolutions():
    kw = dict(in_channels=list(SWIN_L), inference_steps=2, precision="f16x3")
    plain = dda.DDIMDepthEstimate_Swin_ADDHAHI(**kw)
    head = dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip+all", bn_backend="hip", **kw)
    neck = _convs(head.hahineck)
    assert len(neck) == 12 and all(type(m) is CV.HipConv2d and m.channels == "any" for m in neck.values())
    big = neck["trans_fusion.2.conv"]
    assert (big.in_channels, big.out_channels, big.kernel_size) == (2048, 1536, (3, 3))
    assert type(head.conv_lateral[3][0]) is CV.HipConv2d and type(head.conv_up[0][0]) is CV.HipConvTranspose2d
    assert list(head.state_dict()) == list(plain.state_dict())
    head.load_state_dict(plain.state_dict())
    # "hip+neck" still leaves it, and "hip+fpn" is still no back end
    neck_only = _convs(dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip+neck", **kw).hahineck)
    assert type(neck_only["trans_fusion.2.conv"]) is nn.Conv2d
    assert all(m.channels == "block64" for m in neck_only.values() if isinstance(m, CV.HipConv2d))
    with pytest.raises(ValueError):
        dda.DDIMDepthEstimate_Swin_ADDHAHI(conv_backend="hip+fpn", **kw)


def test_res_head_with_hip_all_builds_the_module_types_of_hip():
    res = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="hip+all")
    ref = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="bf16", conv_backend="hip")
    assert res.conv_backend == "hip+all" and [(n, type(m)) for n, m in res.named_modules()] == [(n, type(m)) for n, m in ref.named_modules()]
    assert sum(isinstance(m, HIP) for m in res.modules()) == 8 and all(m.channels == "any" for m in res.modules() if isinstance(m, HIP))
    assert all(m.channels == "block64" for m in ref.modules() if isinstance(m, HIP))
    # the default head is fp32: the keyword is honoured, nothing is eligible, nothing is replaced
    fp32 = dda.DDIMDepthEstimate_Res(inference_steps=2, conv_backend="hip+all")
    assert fp32.model.precision == "fp32" and not any(isinstance(m, HIP) for m in fp32.modules())


def test_the_environment_variable_route(monkeypatch):
    monkeypatch.setenv("DDEPTH_CONV_BACKEND", "hip+all")
    assert CV.resolve_conv_backend() == "hip+all" and CV.resolve_conv_backend("hip") == "hip"
    head = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=list(MPVIT), inference_steps=2, precision="bf16")
    assert head.conv_backend == "hip+all" and type(head.conv_lateral[1][0]) is CV.HipConv2d and head.conv_lateral[1][0].channels == "any"
    assert all(type(m) is CV.HipConv2d for m in _convs(head.hahineck).values())
    assert dda.DDIMDepthEstimate_MPVIT_ADDHAHI(in_channels=list(MPVIT), inference_steps=2, precision="bf16", conv_backend="torch").conv_backend == "torch"
    monkeypatch.setenv("DDEPTH_CONV_BACKEND", "hip+fpn")
    with pytest.raises(ValueError):
        CV.resolve_conv_backend()


def test_the_default_converter_on_the_mpvit_neck_still_converts_exactly_three():
    torch.manual_seed(0)
    neck = dda.HAHIHeteroNeck(list(MPVIT), list(MPVIT), embedding_dim=512, cross_att=False, self_att=False)
    neck = CV.convert_hip_conv(neck, "bf16", pointwise=True)
    converted = sorted(n for n, m in _convs(neck).items() if type(m) is CV.HipConv2d)
    assert converted == ["conv_fusion.0.conv", "conv_proj.0.conv", "lateral_convs.0.conv"] and len(_convs(neck)) == 12
    assert all(m.channels == "block64" for m in neck.modules() if isinstance(m, CV.HipConv2d))


def test_a_converted_ragged_neck_on_cpu_tensors_is_the_unconverted_one_bit_for_bit():
    def make():
        torch.manual_seed(11)
        neck = dda.HAHIHeteroNeck([72, 88, 216, 104], [72, 88, 216, 104], embedding_dim=72, cross_att=False, self_att=False)
        neck.init_weights()
        return neck.train()
    a, b = make(), CV.convert_hip_conv(make(), "f16x3", True, "any")
    assert sum(isinstance(m, CV.HipConv2d) for m in b.modules()) == 12 and list(a.state_dict()) == list(b.state_dict())
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip((72, 88, 216, 104), ((12, 20), (6, 10), (3, 5), (2, 3)))]
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
