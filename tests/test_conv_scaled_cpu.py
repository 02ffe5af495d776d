"""CPU: the opt-in rescale of grad_y (include/ddepth_conv_scaled.h; ``grad_autoscale`` of diffusiondepth_amd.conv, the head keyword
``conv_grad_autoscale``) as far as no GPU is needed -- the ABI (declared == bound == exported, the old header still its 17), that the choice
travels from the head keyword and the environment variable through the converter to the modules and from there to the autograd Functions, that
every default still builds and calls what it did, and that on CPU tensors a module with the option on is the torch module bit for bit."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import conv_scaled_cases as SC
import diffusiondepth_amd as dda
from diffusiondepth_amd import conv as CV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALED = ["dd_conv_grad_scale", "dd_convx_backward_data_scaled", "dd_convx_backward_weight_scaled"]
HIP = (CV.HipConv2d, CV.HipConvTranspose2d)


def _declared(header):
    return re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", open(os.path.join(ROOT, "include", header)).read(), flags=re.M)


def test_the_new_header_the_bound_set_and_the_library_agree_on_three_symbols():
    assert _declared("ddepth_conv_scaled.h") == SCALED == CV.ABI_SYMBOLS_SCALED
    lib = CV._lib_scaled()
    for s in SCALED:
        f = getattr(lib, s)
        assert f.argtypes is not None and len(f.argtypes) == (5 if s == "dd_conv_grad_scale" else 13), s
    assert lib.dd_conv_grad_scale(None, 4, 3, None, None) == 1 and b"scale" in lib.dd_conv_last_error()      # DD_ERR_INVALID_ARG, no device needed
    assert lib.dd_convx_backward_data_scaled(0, None, None, None, None, None, 1, 4, 72, 2, 2, 3, None) == 4
    assert b"multiples of 8 in 8..2048" in lib.dd_conv_last_error()


def test_the_old_header_still_declares_exactly_its_seventeen():
    declared = _declared("ddepth_conv.h")
    assert len(declared) == 17 and declared == CV.ABI_SYMBOLS and not set(declared) & set(SCALED)


def test_the_numpy_rule_of_the_tests():
    f = lambda *v: SC.scale_of(np.array(v, dtype=np.float32))
    assert f(0.0, -0.0) == 1.0 and f(np.nan, np.inf) == 1.0
    assert f(1.0) == 2.0 ** 14 and f(-1.999) == 2.0 ** 14 and f(2.0, 0.5) == 2.0 ** 13 and f(3e-7) == 2.0 ** 36 and f(np.inf, 2.0 ** 14, np.nan) == 1.0
    assert f(2.0 ** 15) == 0.5 and f(65504.0 * 2) == 0.25 and f(3e38) == 2.0 ** -113 and f(1e-45) == 2.0 ** 126 and f(2.0 ** -126) == 2.0 ** 126
    for v in (1.0, 1.999, 3e-7, 7e4, 1e-30):
        assert 2.0 ** 14 <= v * f(v) < 2.0 ** 15


def test_the_environment_variable_and_the_keyword_resolve(monkeypatch):
    monkeypatch.delenv("DDEPTH_CONV_GRAD_AUTOSCALE", raising=False)
    assert CV.resolve_conv_grad_autoscale() is False and CV.resolve_conv_grad_autoscale(None) is False
    assert CV.resolve_conv_grad_autoscale(True) is True and CV.resolve_conv_grad_autoscale(False) is False
    for value, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("DDEPTH_CONV_GRAD_AUTOSCALE", value)
        assert CV.resolve_conv_grad_autoscale() is want
    monkeypatch.setenv("DDEPTH_CONV_GRAD_AUTOSCALE", "1")
    assert CV.resolve_conv_grad_autoscale(False) is False      # the keyword wins
    monkeypatch.setenv("DDEPTH_CONV_GRAD_AUTOSCALE", "yes")
    with pytest.raises(ValueError):
        CV.resolve_conv_grad_autoscale()


def _small_net():
    torch.manual_seed(3)
    return nn.Sequential(nn.Conv2d(72, 216, 3, 1, 1, bias=False), nn.BatchNorm2d(216), nn.ReLU(True),
                         nn.Sequential(nn.ConvTranspose2d(216, 88, 2, 2, bias=False), nn.ReLU()),
                         nn.Conv2d(88, 64, 1, bias=False), nn.Conv2d(64, 64, 3, 1, 1, bias=False))


def test_the_converter_carries_the_choice_and_the_default_is_unchanged():
    net = CV.convert_hip_conv(_small_net(), "f16x3", True, "any")
    mods = [m for m in net.modules() if isinstance(m, HIP)]
    assert len(mods) == 4 and not any(m.grad_autoscale for m in mods)
    assert all("grad_autoscale" not in m.__dict__ and "grad_autoscale" not in repr(m) for m in mods)
    assert CV.HipConv2d.grad_autoscale is False and CV.HipConvTranspose2d.grad_autoscale is False
    net = CV.convert_hip_conv(_small_net(), "f16x3", True, "any", grad_autoscale=True)
    mods = [m for m in net.modules() if isinstance(m, HIP)]
    assert len(mods) == 4 and all(m.grad_autoscale is True and m.channels == "any" for m in mods)
    assert all("channels=any, grad_autoscale=True" in repr(m) for m in mods)
    block = CV.convert_hip_conv(_small_net(), "f16", grad_autoscale=True)      # the block-64 contract: only 64 -> 64 is eligible
    mods = [m for m in block.modules() if isinstance(m, HIP)]
    assert len(mods) == 1 and mods[0].grad_autoscale and mods[0].channels == "block64" and "precision=f16, grad_autoscale=True" in repr(mods[0])


def test_the_head_keyword_carries_the_choice(monkeypatch):
    monkeypatch.delenv("DDEPTH_CONV_GRAD_AUTOSCALE", raising=False)
    kw = dict(in_channels=[128, 216, 288, 288], inference_steps=2, precision="f16x3", conv_backend="hip+all")
    head = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(conv_grad_autoscale=True, **kw)
    mods = [m for m in head.modules() if isinstance(m, HIP)]
    assert head.conv_grad_autoscale is True and len(mods) == 19 and all(m.grad_autoscale for m in mods)
    plain = dda.DDIMDepthEstimate_MPVIT_ADDHAHI(**kw)
    assert plain.conv_grad_autoscale is False and not any(m.grad_autoscale for m in plain.modules() if isinstance(m, HIP))
    assert list(head.state_dict()) == list(plain.state_dict())
    monkeypatch.setenv("DDEPTH_CONV_GRAD_AUTOSCALE", "1")
    env = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="f16", conv_backend="hip")
    assert env.conv_grad_autoscale is True and all(m.grad_autoscale for m in env.modules() if isinstance(m, HIP))
    off = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="f16", conv_backend="hip", conv_grad_autoscale=False)
    assert not any(m.grad_autoscale for m in off.modules() if isinstance(m, HIP))
    torch_head = dda.DDIMDepthEstimate_Res(inference_steps=2, precision="f16")      # nothing converted: the option has nothing to mark
    assert torch_head.conv_grad_autoscale is True and not any(isinstance(m, HIP) for m in torch_head.modules())


def test_the_functions_compute_the_scale_once_and_hand_it_to_both_directions(monkeypatch):
    """With the option off the three direction functions are called with exactly the positional arguments they always had."""
    seen = []
    token = torch.zeros(4)
    monkeypatch.setattr(CV, "conv_forward", lambda *a: a[1].new_zeros(a[1].shape[0], a[2].shape[0], *a[1].shape[2:]))
    monkeypatch.setattr(CV, "grad_scale", lambda gy, prec: (seen.append(("scale", prec)), token)[1])
    monkeypatch.setattr(CV, "conv_backward_data", lambda *a, **kw: (seen.append(("data", a[5:], kw)), a[1].new_zeros(tuple(a[3])))[1])
    monkeypatch.setattr(CV, "conv_backward_weight", lambda *a, **kw: (seen.append(("weight", a[5:], kw)), a[1].new_zeros(tuple(a[3])))[1])
    for fn, w_shape in ((CV.Conv3x3Function, (72, 72, 3, 3)), (CV.Conv1x1Function, (72, 72, 1, 1))):
        for channels, extra in (("any", ("any",)), ("block64", ())):
            for on in (True, False):
                seen.clear()
                x, w = torch.randn(1, 72, 4, 5, requires_grad=True), torch.randn(*w_shape, requires_grad=True)
                y = fn.apply(x, w, 3, channels, True) if on else fn.apply(x, w, 3, channels)
                assert y.grad_fn.conf[1:] == (3, channels) and y.grad_fn.grad_autoscale is on
                y.sum().backward()
                kw = {"scale": token} if on else {}
                assert seen == ([("scale", 3)] if on else []) + [("data", extra, kw), ("weight", extra, kw)]
    seen.clear()
    x = torch.randn(1, 72, 4, 5)                                       # a detached input: one direction, still one scale
    y = CV.Conv3x3Function.apply(x, torch.randn(72, 72, 3, 3, requires_grad=True), 4, "any", True)
    y.sum().backward()
    assert [s[0] for s in seen] == ["scale", "weight"]


def test_the_scaled_calls_refuse_cpu_tensors():
    gy = torch.randn(1, 72, 4, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.grad_scale(gy, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        CV.conv_backward_data(CV.OP_CONV3X3, gy, torch.randn(72, 72, 3, 3), gy.shape, 3, "any", scale=torch.ones(4))


def test_with_the_option_on_cpu_tensors_run_the_torch_modules_bit_for_bit():
    a, b = _small_net(), CV.convert_hip_conv(_small_net(), "f16x3", True, "any", grad_autoscale=True)
    assert sum(isinstance(m, HIP) for m in b.modules()) == 4
    x = torch.randn(2, 72, 6, 10, generator=torch.Generator().manual_seed(1))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = a(xa), b(xb)
    assert torch.equal(ya, yb)
    ((ya ** 2).sum() * 2.0 ** -20).backward()
    ((yb ** 2).sum() * 2.0 ** -20).backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    conv, deconv = CV.HipConv2d(8, 8, precision="f16"), CV.HipConvTranspose2d(8, 8, precision="f16")
    conv.grad_autoscale = deconv.grad_autoscale = True
    x = torch.randn(1, 8, 4, 4)
    assert torch.equal(conv(x), nn.functional.conv2d(x, conv.weight, None, 1, 1))
    assert torch.equal(deconv(x), nn.functional.conv_transpose2d(x, deconv.weight, None, 2))
