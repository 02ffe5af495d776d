"""CPU: everything about diffusiondepth_amd.linear that needs no GPU -- the C ABI of include/swin/ddepth_linear.h (declared == bound == exported,
disjoint from every other header), the support and size queries, the converter on the tiny backbone of tests/linear_cases.py (same tensors, same
keys, idempotent, unsupported modules left alone), the pack cache's key, converted modules on CPU tensors and in .train() against the
unconverted ones (the same bits), and the facade's switches."""
import copy
import glob
import os
import re

import pytest
import torch
from torch import nn

import diffusiondepth_amd as dda
import linear_cases as LC
from diffusiondepth_amd import backend
from diffusiondepth_amd import linear as LN
from diffusiondepth_amd import model as M
from diffusiondepth_amd import swin as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\("


def _declared(path):
    return re.findall(DECL, open(path).read(), flags=re.M)


def test_the_header_declares_the_bound_symbols_and_the_library_exports_them():
    declared = _declared(os.path.join(ROOT, "include", "swin", "ddepth_linear.h"))
    assert declared == LN.ABI_SYMBOLS and len(declared) == 5
    lib = LN._lib()
    for s in declared:
        f = getattr(lib, s)      # (exported: ctypes resolves the symbol)
        assert f.argtypes is not None, s      # (bound with a prototype)
    assert len(lib.dd_linear_forward.argtypes) == 11 and len(lib.dd_linear_pack.argtypes) == 6 and len(lib.dd_linear_supported.argtypes) == 4
    others = glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "include", "train", "*.h"))
    assert len(others) >= 14
    for h in others:
        assert not set(_declared(h)) & set(declared), h
    assert not set(declared) & set(backend.ABI_SYMBOLS) and not set(declared) & set(SW.ABI_SYMBOLS + SW.BACKWARD_ABI_SYMBOLS)
    assert SW.ABI_SYMBOLS == ["dd_swin_last_error", "dd_window_attention_supported", "dd_window_attention_forward"]


def test_support_and_size_queries_need_no_device():
    for C in (96, 128, 192, 384, 768, 1536):      # every Linear of the Swin-T/S/B/L widths, and PatchMerging's reduction
        for K, N in ((C, 3 * C), (C, C), (C, 4 * C), (4 * C, C), (4 * C, 2 * C)):
            for prec in LN.PRECISIONS:
                assert LN.supported(K, N, LN.ACT_NONE, prec) and LN.supported(K, N, LN.ACT_GELU, prec), (K, N, prec)
    assert LN.supported(32, 32) and LN.supported(8192, 8192, 1, "fp32")
    for K, N, act in ((48, 64, 0), (64, 48, 0), (8224, 64, 0), (64, 8224, 0), (0, 64, 0), (64, 64, 2), (64, 64, -1), (16, 32, 0)):
        assert not LN.supported(K, N, act), (K, N, act)
    with pytest.raises(ValueError, match="precision"):
        LN.supported(64, 64, 0, "f16x3")
    lib = LN._lib()
    assert lib.dd_linear_supported(64, 64, 0, 4) == 0 and lib.dd_linear_supported(64, 64, 0, 0) == 0
    assert LN.packed_bytes(96, 288, "fp32") == 96 * 288 * 4 and LN.packed_bytes(96, 288, "bf16") == LN.packed_bytes(96, 288, "f16") == 96 * 288 * 2
    with pytest.raises(RuntimeError, match="multiples of 32"):
        LN.packed_bytes(48, 64)
    assert lib.dd_linear_forward(None, None, None, None, None, 1, 32, 32, 0, 1, None) == LC.DD_ERR_INVALID_ARG
    assert b"null" in lib.dd_linear_last_error()
    with pytest.raises(RuntimeError, match="HIP device"):
        LN.pack_weight(torch.zeros(32, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        LN.linear_forward(torch.zeros(2, 32), LN.PackedWeight(torch.zeros(2048, dtype=torch.uint8), 32, 32, "bf16"))


def test_exports():
    assert dda.HipFFN is LN.HipFFN and dda.convert_hip_swin_linears is LN.convert_hip_swin_linears
    assert dda.linear_forward is LN.linear_forward and dda.pack_weight is LN.pack_weight
    assert all(n in dda.__all__ for n in ("HipFFN", "convert_hip_swin_linears", "linear_forward", "pack_weight"))
    assert SW.ATTENTION_BACKENDS == ("torch", "hip", "hip+train") and SW.BACKWARDS == ("torch", "hip") and LN.LINEAR_BACKENDS == ("torch", "hip")


def test_hipffn_has_the_ffn_s_keywords_keys_and_torch_sequence():
    torch.manual_seed(0)
    m = LN.HipFFN(embed_dims=64, feedforward_channels=256, num_fcs=2, act_cfg=dict(type="GELU"), ffn_drop=0.0, dropout_layer=None, add_identity=True,
                  init_cfg=None)
    assert list(m.state_dict()) == ["layers.0.0.weight", "layers.0.0.bias", "layers.1.weight", "layers.1.bias"] and m.precision == "bf16"
    assert isinstance(m.layers[0][1], nn.GELU) and isinstance(m.dropout_layer, nn.Identity) and m.add_identity
    x, idt = torch.randn(2, 5, 64), torch.randn(2, 5, 64)
    with torch.no_grad():
        body = m.layers[1](torch.nn.functional.gelu(m.layers[0][0](x)))
        assert torch.equal(m(x), x + body) and torch.equal(m(x, identity=idt), idt + body)
        m.add_identity = False
        assert torch.equal(m(x, identity=idt), body)
    assert not m._library_route(x)      # CPU tensors
    with pytest.raises(ValueError, match="precision"):
        LN.HipFFN(64, 256, precision="f16x3")
    assert isinstance(LN.HipFFN(64, 256, act_cfg=dict(type="ReLU")).layers[0][1], nn.ReLU)


def _ducks(net):
    return [m for m in net.modules() if LN._ffn_matches(m)]


def test_the_converter_keeps_tensors_and_keys_skips_what_the_operator_does_not_run_and_is_idempotent():
    net = LC.tiny_backbone()
    keys, ids = list(net.state_dict()), [id(t) for t in net.state_dict(keep_vars=True).values()]
    x = torch.randn(1, 3, 40, 68)
    with torch.no_grad():
        want = net(x)
    ducks = _ducks(net)
    assert len(ducks) == 2 and not any(isinstance(m, (LN.HipFFN, SW.HipShiftWindowMSA)) for m in net.modules())
    # without the library attention module only the FFNs convert
    out = LN.convert_hip_swin_linears(net, "f16")
    assert out is net
    ffns = [m for m in net.modules() if isinstance(m, LN.HipFFN)]
    assert len(ffns) == 2 and all(f.precision == "f16" and f.add_identity for f in ffns) and [f.layers for f in ffns] == [d.layers for d in ducks]
    assert not any(isinstance(m, SW.HipShiftWindowMSA) for m in net.modules())
    # after the attention conversion its Linears follow, at the second call's precision; the FFNs keep theirs
    SW.convert_hip_window_attention(net, "fp32")
    hips = [m for m in net.modules() if isinstance(m, SW.HipShiftWindowMSA)]
    assert len(hips) == 2 and all(h.linear == "torch" and h.linear_precision is None for h in hips)
    LN.convert_hip_swin_linears(net, "bf16")
    assert all(h.linear == "hip" and h.linear_precision == "bf16" and h.precision == "fp32" for h in hips)
    assert [m for m in net.modules() if isinstance(m, LN.HipFFN)] == ffns and all(f.precision == "f16" for f in ffns)
    LN.convert_hip_swin_linears(net, "fp32")      # again: nothing moves
    assert all(h.linear_precision == "bf16" for h in hips) and all(f.precision == "f16" for f in ffns)
    assert [m for m in net.modules() if isinstance(m, SW.HipShiftWindowMSA)] == hips
    assert list(net.state_dict()) == keys and [id(t) for t in net.state_dict(keep_vars=True).values()] == ids
    with torch.no_grad():
        got = net(x)
    assert all(torch.equal(a, b) for a, b in zip(got, want))      # CPU tensors: the same torch sequence, the same bits
    net.train()
    ref = LC.tiny_backbone().train()
    ref.load_state_dict(net.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(net(x), ref(x)))      # .train(): the unconverted modules' bits, with a graph
    assert net(x)[0].requires_grad

    # what the operator does not run stays what it is; a matching root module is returned converted
    holder = nn.ModuleList([LC.DuckFFN(48, 192), LC.DuckFFN(64, 200), LC.DuckFFN(64, 256, act=nn.ReLU()), LC.DuckFFN(64, 256, act=nn.GELU(approximate="tanh")),
                            LC.DuckFFN(64, 256, add_identity=False, bias=False)])
    three = LC.DuckFFN(64, 256)
    three.layers = nn.Sequential(three.layers[0], copy.deepcopy(three.layers[0]), three.layers[1], three.layers[2])
    holder.append(three)
    kept = list(holder)
    LN.convert_hip_swin_linears(holder)
    assert [holder[i] is kept[i] for i in range(6)] == [True, True, True, True, False, True]
    assert isinstance(holder[4], LN.HipFFN) and holder[4].precision == "bf16" and not holder[4].add_identity
    root = LC.DuckFFN(64, 256)
    conv = LN.convert_hip_swin_linears(root, "fp32")
    assert isinstance(conv, LN.HipFFN) and conv.layers is root.layers and conv.precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        LN.convert_hip_swin_linears(LC.DuckFFN(64, 256), "f16x3")
    att = SW.HipShiftWindowMSA(64, 2, 7)
    assert att.linear == "torch" and LN.convert_hip_swin_linears(att) is att and att.linear == "hip" and att.linear_precision == "bf16"
    assert SW.HipShiftWindowMSA(64, 2, 7, linear="hip", linear_precision="f16").linear_precision == "f16"
    with pytest.raises(ValueError, match="linear"):
        SW.HipShiftWindowMSA(64, 2, 7, linear="miopen")


def test_the_pack_cache_follows_the_weight_s_version_and_stays_out_of_the_state_dict(monkeypatch):
    """packed_for with pack_weight replaced by a recorder (the real one needs a device): one pack per (version, storage, precision)."""
    packs = []
    monkeypatch.setattr(LN, "pack_weight", lambda w, precision: (packs.append((w._version, precision)), object())[1])
    ffn = LN.HipFFN(64, 256)
    fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
    keys = list(ffn.state_dict())
    a = LN.packed_for(ffn, "fc1", fc1, "bf16")
    assert LN.packed_for(ffn, "fc1", fc1, "bf16") is a and len(packs) == 1
    b = LN.packed_for(ffn, "fc2", fc2, "bf16")
    assert b is not a and len(packs) == 2 and LN.packed_for(ffn, "fc1", fc1, "bf16") is a
    with torch.no_grad():
        fc1.weight.mul_(2.0)      # (what an optimizer step or load_state_dict does: the version moves)
    c = LN.packed_for(ffn, "fc1", fc1, "bf16")
    assert c is not a and len(packs) == 3 and LN.packed_for(ffn, "fc1", fc1, "bf16") is c and LN.packed_for(ffn, "fc2", fc2, "bf16") is b
    assert LN.packed_for(ffn, "fc1", fc1, "f16") is not c and packs[-1][1] == "f16"      # another precision: another image
    ffn.load_state_dict(copy.deepcopy(ffn.state_dict()))
    assert LN.packed_for(ffn, "fc2", fc2, "bf16") is not b
    assert list(ffn.state_dict()) == keys and "_linear_packs" not in ffn.state_dict() and "_linear_packs" in ffn.__dict__
    assert not any(isinstance(v, torch.Tensor) for v in ffn.__dict__["_linear_packs"].values())
    assert len(list(ffn.buffers())) == 0 and len(list(ffn.parameters())) == 4


def _model(backbone=None, **args):
    a = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, **args)
    return M.Diffusion_DCbase_Model(a, depth_backbone=backbone if backbone is not None else LC.tiny_backbone())


def test_the_facade_switches_defaults_and_rejected_values(monkeypatch):
    for v in ("DDEPTH_BACKBONE_ATTENTION", "DDEPTH_BACKBONE_ATTENTION_PRECISION", "DDEPTH_BACKBONE_BACKEND", "DDEPTH_BACKBONE_LINEAR",
              "DDEPTH_BACKBONE_LINEAR_PRECISION"):
        monkeypatch.delenv(v, raising=False)
    ffns = lambda m: [c for c in m.depth_backbone.modules() if isinstance(c, LN.HipFFN)]
    hips = lambda m: [c for c in m.depth_backbone.modules() if isinstance(c, SW.HipShiftWindowMSA)]
    plain = _model()
    assert plain.backbone_linear == "torch" and plain.backbone_linear_precision == "bf16" and not ffns(plain) and not hips(plain)
    only = _model(backbone_linear="hip")      # backbone_attention="torch": only the FFNs convert
    assert only.backbone_linear == "hip" and len(ffns(only)) == 2 and not hips(only) and all(f.precision == "bf16" for f in ffns(only))
    assert list(only.state_dict()) == list(plain.state_dict())
    both = _model(backbone_attention="hip", backbone_linear="hip", backbone_linear_precision="fp32")
    assert len(ffns(both)) == 2 and len(hips(both)) == 2 and all(f.precision == "fp32" for f in ffns(both))
    assert all(h.linear == "hip" and h.linear_precision == "fp32" and h.precision == "fp32" for h in hips(both))
    att = _model(backbone_attention="hip")      # the attention switch alone leaves the Linears torch
    assert not ffns(att) and all(h.linear == "torch" for h in hips(att))
    monkeypatch.setenv("DDEPTH_BACKBONE_LINEAR", "")
    assert _model().backbone_linear == "torch"
    monkeypatch.setenv("DDEPTH_BACKBONE_LINEAR", "hip")
    monkeypatch.setenv("DDEPTH_BACKBONE_LINEAR_PRECISION", "f16")
    env = _model()
    assert env.backbone_linear == "hip" and env.backbone_linear_precision == "f16" and all(f.precision == "f16" for f in ffns(env))
    assert not ffns(_model(backbone_linear="torch"))      # the keyword wins
    assert _model(backbone_linear_precision="fp32").backbone_linear_precision == "fp32"
    monkeypatch.delenv("DDEPTH_BACKBONE_LINEAR")
    monkeypatch.delenv("DDEPTH_BACKBONE_LINEAR_PRECISION")
    with pytest.raises(ValueError, match="backbone_linear"):
        _model(backbone_linear="hipblaslt")
    with pytest.raises(ValueError, match="backbone_linear_precision"):
        _model(backbone_linear="hip", backbone_linear_precision="f16x3")
    # an injected backbone is converted in place: the same parameter tensors; a backbone without Swin blocks is left alone
    bb = LC.tiny_backbone()
    ids = [id(p) for p in bb.parameters()]
    inj = _model(backbone=bb, backbone_attention="hip", backbone_linear="hip")
    assert inj.depth_backbone is bb and [id(p) for p in bb.parameters()] == ids
    res = M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, backbone_linear="hip"))
    assert res.backbone_linear == "hip" and not ffns(res)


def test_a_default_built_model_is_untouched(monkeypatch):
    """With both switches absent nothing of the new module is in the model: no HipFFN, no linear="hip", the backbone's own modules and bits."""
    for v in ("DDEPTH_BACKBONE_LINEAR", "DDEPTH_BACKBONE_LINEAR_PRECISION", "DDEPTH_BACKBONE_ATTENTION"):
        monkeypatch.delenv(v, raising=False)
    bb = LC.tiny_backbone(1)
    mods = [type(m) for m in bb.modules()]
    x = torch.randn(1, 3, 40, 68)
    with torch.no_grad():
        want = bb(x)
    args = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2)
    model = M.Diffusion_DCbase_Model(args, depth_backbone=bb)
    assert model.depth_backbone is bb and [type(m) for m in bb.modules()] == mods
    assert not any(type(m).__name__ == "HipFFN" or getattr(m, "linear", "torch") != "torch" for m in model.modules())
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(bb(x), want))
