"""CPU: everything about the attention backward that needs no GPU -- the C ABI of include/train/ddepth_swin_backward.h (declared == bound ==
exported; include/ddepth_swin.h keeps its three symbols), the workspace query, ``backward="hip"`` on CPU tensors (the torch route with the
composition's gradients), the converter's and the facade's switches, and the deterministic fold of the dense bias gradient into the table's."""
import os
import re

import pytest
import torch

import diffusiondepth_amd as dda
import swin_cases as SC
from diffusiondepth_amd import build
from diffusiondepth_amd import model as M
from diffusiondepth_amd import swin as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\("


def _declared(*path):
    return re.findall(DECL, open(os.path.join(ROOT, "include", *path)).read(), flags=re.M)


def test_the_header_declares_the_bound_symbols_and_the_library_exports_them():
    declared = _declared("train", "ddepth_swin_backward.h")
    assert declared == SW.BACKWARD_ABI_SYMBOLS and len(declared) == 3
    assert _declared("ddepth_swin.h") == SW.ABI_SYMBOLS and len(SW.ABI_SYMBOLS) == 3
    lib = SW._lib()
    for s in declared:
        assert getattr(lib, s).argtypes is not None, s      # (exported, and bound with a prototype)
    assert len(lib.dd_window_attention_backward.argtypes) == 18 and len(lib.dd_window_attention_backward_workspace_bytes.argtypes) == 8
    assert {"dd_api_swin_bwd.cpp", "dd_swin_bwd.hip"} <= set(build.SOURCES)
    assert any(h.replace(os.sep, "/").endswith("include/train/ddepth_swin_backward.h") for h in build.HEADERS)      # (the stale check sees it)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    assert dda.WindowAttentionFunction is SW.WindowAttentionFunction and dda.window_attention_backward is SW.window_attention_backward


def test_the_workspace_query_and_the_argument_checks_need_no_device():
    per = (49 * 49 + 96) * 4
    assert SW.backward_workspace_bytes(1, 7, 7, 32, 1) == per
    assert SW.backward_workspace_bytes(4, 88, 304, 192, 6, precision="bf16") == 143 * 6 * per      # 2 288 windows in slices of 16
    assert SW.backward_workspace_bytes(1, 11, 38, 1536, 48, precision="f16") == 12 * 48 * per
    with pytest.raises(RuntimeError, match="window 7"):
        SW.backward_workspace_bytes(1, 7, 7, 32, 1, window=8)
    lib = SW._lib()
    assert lib.dd_window_attention_backward_supported(192, 6, 7, 1) == 1 and lib.dd_window_attention_backward_supported(192, 6, 7, 4) == 0
    assert lib.dd_window_attention_backward(*([None] * 9), 1, 7, 7, 32, 1, 7, 0, 1, None) == SC.DD_ERR_INVALID_ARG
    assert b"null" in lib.dd_swin_last_error()
    with pytest.raises(RuntimeError, match="HIP device"):
        SW.window_attention_backward(torch.zeros(1, 7, 7, 96), None, torch.zeros(1, 49, 49), torch.zeros(1, 7, 7, 32), 1, 7, 0)


def _module(heads=3, shift=3, seed=0, **kw):
    torch.manual_seed(seed)
    m = SW.HipShiftWindowMSA(32 * heads, heads, 7, shift_size=shift, **kw)
    m.w_msa.init_weights()
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.mul_(50.0)
    return m


def test_backward_hip_on_cpu_tensors_takes_the_torch_route_with_the_composition_s_gradients():
    B, H, W, heads = 2, 10, 17, 3
    m = _module(heads, 3, backward="hip").train()
    assert m.backward == "hip" and m.grad_autoscale is True and _module(heads, 3).backward == "torch"
    x = torch.randn(B, H * W, 32 * heads, requires_grad=True)
    assert not m._train_route(x) and not m._library_route(x)
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
    assert len(got) == 6
    for a, b in zip(got, want):
        assert (a - b).abs().max() <= 1e-5 * max(1.0, float(b.abs().max()))
    with pytest.raises(ValueError, match="backward"):
        SW.HipShiftWindowMSA(64, 2, 7, backward="miopen")


def test_the_converter_s_backward_switch():
    net = SW.convert_hip_window_attention(SC.tiny_backbone(), "f16", backward="hip", grad_autoscale=False)
    hips = [m for m in net.modules() if isinstance(m, SW.HipShiftWindowMSA)]
    assert len(hips) == 2 and all(h.backward == "hip" and h.precision == "f16" and h.grad_autoscale is False for h in hips)
    plain = [m for m in SW.convert_hip_window_attention(SC.tiny_backbone()).modules() if isinstance(m, SW.HipShiftWindowMSA)]
    assert len(plain) == 2 and all(h.backward == "torch" and h.grad_autoscale is True for h in plain)
    with pytest.raises(ValueError, match="backward"):
        SW.convert_hip_window_attention(SC.tiny_backbone(), "fp32", backward="triton")


def _model(**args):
    a = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, **args)
    return M.Diffusion_DCbase_Model(a, depth_backbone=SC.tiny_backbone())


def test_the_facade_s_training_switch_and_rejected_values(monkeypatch):
    for v in ("DDEPTH_BACKBONE_ATTENTION", "DDEPTH_BACKBONE_ATTENTION_PRECISION", "DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE", "DDEPTH_BACKBONE_BACKEND"):
        monkeypatch.delenv(v, raising=False)
    assert SW.ATTENTION_BACKENDS == ("torch", "hip", "hip+train")
    hips = lambda m: [c for c in m.depth_backbone.modules() if isinstance(c, SW.HipShiftWindowMSA)]
    train = _model(backbone_attention="hip+train", backbone_attention_precision="bf16")
    assert train.backbone_attention == "hip+train" and train.backbone_attention_grad_autoscale is True
    assert len(hips(train)) == 2 and all(h.backward == "hip" and h.precision == "bf16" and h.grad_autoscale for h in hips(train))
    hip = _model(backbone_attention="hip")
    assert len(hips(hip)) == 2 and all(h.backward == "torch" for h in hips(hip))      # "hip" stays inference only
    assert list(train.state_dict()) == list(hip.state_dict()) == list(_model().state_dict())
    assert not any(h.grad_autoscale for h in hips(_model(backbone_attention="hip+train", backbone_attention_grad_autoscale=False)))
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION", "hip+train")
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE", "0")
    env = _model()
    assert env.backbone_attention == "hip+train" and env.backbone_attention_grad_autoscale is False
    assert all(h.backward == "hip" and not h.grad_autoscale for h in hips(env))
    assert all(h.grad_autoscale for h in hips(_model(backbone_attention_grad_autoscale=True)))      # the keyword wins
    assert not hips(_model(backbone_attention="torch"))
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE", "maybe")
    with pytest.raises(ValueError, match="backbone_attention_grad_autoscale"):
        _model()
    monkeypatch.delenv("DDEPTH_BACKBONE_ATTENTION_GRAD_AUTOSCALE")
    monkeypatch.setenv("DDEPTH_BACKBONE_ATTENTION", "hip+training")
    with pytest.raises(ValueError, match="backbone_attention"):
        _model()


def test_the_table_s_gradient_is_a_fixed_gather_of_the_dense_one():
    heads = 6
    fold = SW.bias_fold_index(7)
    assert tuple(fold.shape) == (169, 49) and int((fold < 2401).sum()) == 2401 and fold[fold < 2401].unique().numel() == 2401
    assert int((fold[84] < 2401).sum()) == 49 and int((fold[0] < 2401).sum()) == 1      # the centre of the table is read 49 times, a corner once
    index = SW.relative_position_index(7)
    torch.manual_seed(3)
    table = torch.randn(169, heads, dtype=torch.float64, requires_grad=True)      # fp64: the 1e-6 below is absolute, on sums of up to 49 terms
    g = torch.randn(heads, 49, 49, dtype=torch.float64)
    (SW.dense_bias(table, index) * g).sum().backward()
    want = table.grad.clone()
    table.grad = None
    dense = SW.dense_bias_folded(table, index, fold)
    assert torch.equal(dense, SW.dense_bias(table.detach(), index))
    (dense * g).sum().backward()
    got = table.grad.clone()
    assert tuple(got.shape) == (169, heads) and (got - want).abs().max() <= 1e-6
    g32 = g.float()
    assert torch.equal(SW.fold_bias_grad(g32, fold), SW.fold_bias_grad(g32.clone(), fold)) and torch.equal(got, SW.fold_bias_grad(g, fold))
    assert (SW.fold_bias_grad(g32, fold).double() - want).abs().max() <= 1e-6 * float(want.abs().max())
