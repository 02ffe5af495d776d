"""CPU: everything about diffusiondepth_amd.swin that needs no GPU -- the C ABI of include/ddepth_swin.h (declared == bound == exported, disjoint
from every other header, whose counts are unchanged), ``HipShiftWindowMSA`` on CPU tensors (the torch route) against ``window_attention_torch``
and the fp64 oracle of tests/swin_cases.py, the converter (same tensors, same keys, idempotent, unsupported modules left alone), the facade's
switches, and that with grad enabled the module takes the torch route with the composition's gradients."""
import glob
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
import swin_cases as SC
from diffusiondepth_amd import backend
from diffusiondepth_amd import model as M
from diffusiondepth_amd import swin as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\("
# what every other header declared before this one existed
COUNTS = {"ddepth.h": 26, "ddepth_bn.h": 7, "ddepth_bn_add.h": 2, "ddepth_codec.h": 7, "ddepth_conv.h": 17, "ddepth_conv_fused.h": 4,
          "ddepth_conv_scaled.h": 3, "ddepth_conv_stats.h": 3, "ddepth_conv_strided.h": 5, "ddepth_dcn.h": 7, "ddepth_eval.h": 6, "ddepth_msda.h": 3}


def _declared(header):
    return re.findall(DECL, open(os.path.join(ROOT, "include", header)).read(), flags=re.M)


def test_the_header_declares_the_bound_symbols_and_the_library_exports_them():
    declared = _declared("ddepth_swin.h")
    assert declared == SW.ABI_SYMBOLS and len(declared) == 3
    lib = SW._lib()
    for s in declared:
        f = getattr(lib, s)      # (exported: ctypes resolves the symbol)
        assert f.argtypes is not None, s      # (bound with a prototype)
    assert len(lib.dd_window_attention_forward.argtypes) == 13 and len(lib.dd_window_attention_supported.argtypes) == 4
    others = {os.path.basename(h): _declared(os.path.basename(h)) for h in glob.glob(os.path.join(ROOT, "include", "*.h"))}
    del others["ddepth_swin.h"]
    assert {h: len(d) for h, d in others.items()} == COUNTS
    for h, d in others.items():
        assert not set(d) & set(declared), h
    assert not set(declared) & set(backend.ABI_SYMBOLS)


def test_support_query_and_argument_checks_need_no_device():
    assert SW.supported(192, 6, 7) and SW.supported(1536, 48, 7, "bf16") and SW.supported(32, 1, 7, "f16")
    assert not SW.supported(192, 6, 8) and not SW.supported(192, 4, 7) and not SW.supported(96, 6, 7) and not SW.supported(0, 0, 7)
    with pytest.raises(ValueError, match="precision"):
        SW.supported(192, 6, 7, "f16x3")
    lib = SW._lib()
    assert lib.dd_window_attention_supported(192, 6, 7, 4) == 0 and lib.dd_window_attention_supported(192, 6, 7, 0) == 0
    assert lib.dd_window_attention_forward(None, None, None, None, 1, 7, 7, 32, 1, 7, 0, 1, None) == SC.DD_ERR_INVALID_ARG
    assert b"null" in lib.dd_swin_last_error()
    with pytest.raises(RuntimeError, match="HIP device"):
        SW.window_attention_forward(torch.zeros(1, 7, 7, 96), None, torch.zeros(1, 49, 49), 1, 7, 0)


def test_exports():
    assert dda.HipShiftWindowMSA is SW.HipShiftWindowMSA and dda.convert_hip_window_attention is SW.convert_hip_window_attention
    assert dda.window_attention is SW.window_attention and dda.window_attention_torch is SW.window_attention_torch


def test_the_relative_position_index_is_the_double_step_construction():
    """The reference builds the index as (13 y + x)[None, :] + (13 y + x)[:, None], flipped along the keys."""
    base = (13 * torch.arange(7)[:, None] + torch.arange(7)[None, :]).reshape(1, -1)
    assert torch.equal(SW.relative_position_index(7), (base + base.T).flip(1))
    assert np.array_equal(SW.relative_position_index(7).numpy(), SC.rel_index())


@pytest.mark.parametrize("shift", SC.SHIFTS)
@pytest.mark.parametrize("name", ["one", "whole", "ragged", "sub", "last"])
def test_the_torch_composition_is_the_fp64_oracle(name, shift):
    """window_attention_torch (pad, roll, mask, partition ... as ops) against swin_cases.attend (index arithmetic), both in fp64: <= 1e-12; in fp32
    through ``window_attention`` on CPU tensors: <= 1e-5.  The exact cases come out exactly."""
    for bias_scale in SC.BIAS_SCALES:
        qkv, pad, bias = SC.real_inputs(name, shift, bias_scale)
        heads = SC.SHAPES[name][3]
        t = lambda a, dt: None if a is None else torch.tensor(a, dtype=dt)
        got64 = SW.window_attention_torch(t(qkv, torch.float64), t(pad, torch.float64), t(bias, torch.float64), heads, 7, shift).numpy()
        assert np.abs(got64 - SC.real_oracle(name, shift, bias_scale)).max() <= 1e-12
        got32 = SW.window_attention(t(qkv, torch.float32), t(pad, torch.float32), t(bias, torch.float32), heads, 7, shift).numpy()
        assert np.abs(got32 - SC.real_oracle(name, shift, bias_scale)).max() <= 1e-5
        for prec in ("bf16", "f16"):      # the rounding emulation of the composition is the cases' own
            emu = SW.window_attention_torch(t(qkv, torch.float32), t(pad, torch.float32), t(bias, torch.float32), heads, 7, shift, round_to=SC.ROUND[prec])
            assert np.abs(emu.numpy() - SC.real_emulation(name, shift, bias_scale, prec)).max() <= 2e-2
    for kind in ("identity", "permutation"):
        qkv, pad, bias = SC.exact_inputs(name, shift, kind)
        t32 = lambda a: None if a is None else torch.tensor(a)
        got = SW.window_attention_torch(t32(qkv), t32(pad), t32(bias), SC.SHAPES[name][3], 7, shift).numpy()
        assert np.array_equal(got, SC.exact_expected(name, shift, kind))


def _module(heads=3, shift=3, seed=0, **kw):
    torch.manual_seed(seed)
    m = SW.HipShiftWindowMSA(32 * heads, heads, 7, shift_size=shift, **kw)
    m.w_msa.init_weights()
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.mul_(50.0)
    return m


@pytest.mark.parametrize("shift", SC.SHIFTS)
@pytest.mark.parametrize("name", ["ragged", "sub", "last"])
def test_the_module_on_cpu_tensors_is_the_composition_and_the_oracle(name, shift):
    B, H, W, heads = SC.SHAPES[name]
    m = _module(heads, shift).eval()
    x = torch.randn(B, H * W, 32 * heads)
    with torch.no_grad():
        got = m(x, (H, W))
        w = m.w_msa
        qkv = w.qkv(x).view(B, H, W, -1)
        bias = SW.dense_bias(w.relative_position_bias_table, w.relative_position_index)
        comp = w.proj(SW.window_attention_torch(qkv, w.qkv.bias, bias, heads, 7, shift).view(B, H * W, -1))
        ora = SC.attend(qkv.double().numpy(), w.qkv.bias.double().numpy(), bias.double().numpy(), heads, shift)
        ora = torch.from_numpy(ora).view(B, H * W, -1) @ w.proj.weight.double().T + w.proj.bias.double()
    assert got.shape == (B, H * W, 32 * heads)
    assert (got - comp).abs().max() <= 1e-5 and (got.double() - ora).abs().max() <= 1e-5


def test_constructor_keywords_attributes_and_state_dict_keys_are_the_reference_s():
    m = SW.HipShiftWindowMSA(embed_dims=64, num_heads=2, window_size=7, shift_size=3, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0,
                             proj_drop_rate=0.0, dropout_layer=dict(type="DropPath", drop_prob=0.0), init_cfg=None)
    assert m.window_size == 7 and m.shift_size == 3 and m.w_msa.window_size == (7, 7) and m.w_msa.num_heads == 2 and m.w_msa.embed_dims == 64
    assert m.w_msa.scale == 32 ** -0.5 and isinstance(m.drop, nn.Module)
    assert list(m.state_dict()) == ["w_msa.relative_position_bias_table", "w_msa.relative_position_index", "w_msa.qkv.weight", "w_msa.qkv.bias",
                                    "w_msa.proj.weight", "w_msa.proj.bias"]
    assert tuple(m.w_msa.relative_position_bias_table.shape) == (169, 2) and tuple(m.w_msa.relative_position_index.shape) == (49, 49)
    assert list(SW.HipShiftWindowMSA(64, 2, 7, qkv_bias=False).state_dict()) == [k for k in m.state_dict() if k != "w_msa.qkv.bias"]
    with pytest.raises(AssertionError):
        SW.HipShiftWindowMSA(64, 2, 7, shift_size=7)
    with pytest.raises(ValueError, match="precision"):
        SW.HipShiftWindowMSA(64, 2, 7, precision="f16x3")


def test_the_dense_bias_follows_the_table_s_version():
    m = _module(2, 0).eval()
    a = m._dense_bias()
    assert m._dense_bias() is a and tuple(a.shape) == (2, 49, 49)
    assert torch.equal(a, SW.dense_bias(m.w_msa.relative_position_bias_table.detach(), m.w_msa.relative_position_index))
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.add_(1.0)      # (what an optimizer step or load_state_dict does: the version moves)
    b = m._dense_bias()
    assert b is not a and torch.equal(b, a + 1.0)
    assert "_bias_cache" not in m.state_dict() and len(m.state_dict()) == 6


def test_the_converter_keeps_tensors_and_keys_skips_what_the_operator_does_not_run_and_is_idempotent():
    net = SC.tiny_backbone()
    keys, ids = list(net.state_dict()), [id(t) for t in net.state_dict(keep_vars=True).values()]
    x = torch.randn(1, 3, 40, 68)
    with torch.no_grad():
        want = net(x)
    ducks = [m for m in net.modules() if SW._matches(m)]
    assert len(ducks) == 2 and not any(isinstance(m, SW.HipShiftWindowMSA) for m in ducks)
    out = SW.convert_hip_window_attention(net, "bf16")
    assert out is net
    hips = [m for m in net.modules() if isinstance(m, SW.HipShiftWindowMSA)]
    assert len(hips) == 2 and [h.shift_size for h in hips] == [0, 3] and all(h.precision == "bf16" and h.window_size == 7 for h in hips)
    assert [h.w_msa for h in hips] == [d.w_msa for d in ducks]
    assert list(net.state_dict()) == keys and [id(t) for t in net.state_dict(keep_vars=True).values()] == ids
    with torch.no_grad():
        got = net(x)
    assert all(torch.equal(a, b) for a, b in zip(got, want))      # CPU tensors: the same torch sequence
    again = SW.convert_hip_window_attention(net, "f16")
    assert [m for m in again.modules() if isinstance(m, SW.HipShiftWindowMSA)] == hips and all(h.precision == "bf16" for h in hips)

    # a window of 8, a head dimension of 16 and a custom qk_scale stay what they are; a matching root module is returned converted
    class Duck(nn.Module):
        def __init__(self, dims, heads, window, **kw):
            super().__init__()
            self.window_size, self.shift_size = window, 0
            self.w_msa = SW.WindowMSA(dims, heads, (window, window), **kw)
    holder = nn.ModuleList([Duck(64, 2, 8), Duck(64, 4, 7), Duck(64, 2, 7, qk_scale=0.5), Duck(64, 2, 7)])
    kept = list(holder)
    SW.convert_hip_window_attention(holder)
    assert [holder[i] is kept[i] for i in range(4)] == [True, True, True, False] and isinstance(holder[3], SW.HipShiftWindowMSA)
    root = Duck(64, 2, 7)
    conv = SW.convert_hip_window_attention(root)
    assert isinstance(conv, SW.HipShiftWindowMSA) and conv.w_msa is root.w_msa and conv.precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        SW.convert_hip_window_attention(Duck(64, 2, 7), "f16x3")


def test_with_grad_enabled_the_module_takes_the_torch_route_with_the_composition_s_gradients():
    B, H, W, heads = 2, 10, 17, 3
    m = _module(heads, 3).train()
    x = torch.randn(B, H * W, 32 * heads, requires_grad=True)
    assert not m._library_route(x)
    m.eval()
    assert not m._library_route(x)      # (CPU tensors, and parameters that require grad)
    m.train()
    g = torch.randn(B, H * W, 32 * heads)
    (m(x, (H, W)) * g).sum().backward()
    got = [x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    x.grad = None
    m.zero_grad()
    w = m.w_msa
    bias = SW.dense_bias(w.relative_position_bias_table, w.relative_position_index)
    y = w.proj(SW.window_attention_torch(w.qkv(x).view(B, H, W, -1), w.qkv.bias, bias, heads, 7, 3).view(B, H * W, -1))
    (y * g).sum().backward()
    want = [x.grad] + [p.grad for p in m.parameters()]
    assert len(got) == 6 and all(a is not None for a in want)
    for a, b in zip(got, want):
        assert (a - b).abs().max() <= 1e-5 * max(1.0, float(b.abs().max()))
    # window_attention itself: a tensor that needs a gradient keeps the composition, whatever the device
    q = torch.randn(1, 7, 7, 96, requires_grad=True)
    assert SW.window_attention(q, None, torch.zeros(1, 49, 49), 1, 7, 0).requires_grad


def _model(**args):
    a = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, **args)
    return M.Diffusion_DCbase_Model(a, depth_backbone=SC.tiny_backbone())


def test_the_facade_switches_defaults_and_rejected_values(monkeypatch):
    for v in ("DDEPTH_BACKBONE_ATTENTION", "DDEPTH_BACKBONE_ATTENTION_PRECISION", "DDEPTH_BACKBONE_BACKEND"):
        monkeypatch.delenv(v, raising=False)
    hips = lambda m: [c for c in m.depth_backbone.modules() if isinstance(c, SW.HipShiftWindowMSA)]
    plain = _model()
    assert plain.backbone_attention == "torch" and plain.backbone_attention_precision == "fp32" and not hips(plain)
    assert plain.backbone_backend == "torch" and M.BACKBONE_BACKENDS == ("torch", "hip", "hip+bn", "hip+fold", "hip+stats")
    assert M.BACKBONE_PRECISIONS == ("bf16", "f16", "f16x3")
    hip = _model(backbone_attention="hip")
    assert hip.backbone_attention == "hip" and len(hips(hip)) == 2 and all(h.precision == "fp32" for h in hips(hip))
    assert hip.backbone_backend == "torch" and list(hip.state_dict()) == list(plain.state_dict())
    assert all(h.precision == "f16" for h in hips(_model(backbone_attention="hip", backbone_attention_precision="f16")))
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION", "")
    assert _model().backbone_attention == "torch"
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION", "hip")
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION_PRECISION", "bf16")
    env = _model()
    assert env.backbone_attention == "hip" and env.backbone_attention_precision == "bf16" and all(h.precision == "bf16" for h in hips(env))
    assert not hips(_model(backbone_attention="torch"))      # the keyword wins
    assert _model(backbone_attention_precision="fp32").backbone_attention_precision == "fp32"
    monkeypatch.delenv("DDEPTH_BACKBONE_ATTENTION")
    monkeypatch.delenv("DDEPTH_BACKBONE_ATTENTION_PRECISION")
    with pytest.raises(ValueError, match="backbone_attention"):
        _model(backbone_attention="miopen")
    with pytest.raises(ValueError, match="backbone_attention_precision"):
        _model(backbone_attention="hip", backbone_attention_precision="f16x3")
    # an injected backbone is converted in place: the same parameter tensors; a backbone without attention is left alone
    bb = SC.tiny_backbone()
    ids = [id(p) for p in bb.parameters()]
    inj = M.Diffusion_DCbase_Model(M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, backbone_attention="hip"), depth_backbone=bb)
    assert inj.depth_backbone is bb and [id(p) for p in bb.parameters()] == ids
    res = M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, backbone_attention="hip"))
    assert res.backbone_attention == "hip" and not hips(res)
