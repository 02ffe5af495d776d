"""GPU (`-m gpu`): the shifted-window attention of include/ddepth_swin.h / diffusiondepth_amd.swin on the MI355X -- the cases of tests/swin_cases.py
through the built library (exact cases bit-equal at every precision, real-valued cases within 4 x the baseline's own error against the fp64
oracle, batch / repeat / NaN identities, sentinels around qkv, rel_bias and out, argument validation), no host synchronisation,
``HipShiftWindowMSA`` in .eval() against the torch composition on the device, and a tiny Swin-like backbone under ``backbone_attention="hip"``
against ``"torch"`` through ``Diffusion_DCbase_Model.forward`` with a Swin head."""
import numpy as np
import pytest
import torch

import swin_cases as SC

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


def _guarded(a):
    """A device copy of ``a`` with 16 sentinel floats (64 bytes: the alignment stays) in front of and behind it -> (buffer, view)."""
    buf = torch.full((a.size + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[16:16 + a.size].view(a.shape)
    view.copy_(torch.tensor(a))
    return buf, view


def run(qkv, pad, bias, heads, shift, prec):
    from diffusiondepth_amd import swin as SW
    B, H, W, K = qkv.shape
    bufs = [_guarded(qkv), _guarded(bias), _guarded(np.full((B, H, W, K // 3), np.nan, dtype=np.float32))]
    p = None if pad is None else torch.from_numpy(pad.copy()).cuda()
    lib = SW._lib()
    q, bs, out = (v for _, v in bufs)
    rc = lib.dd_window_attention_forward(q.data_ptr(), p.data_ptr() if p is not None else None, bs.data_ptr(), out.data_ptr(), B, H, W, K // 3, heads,
                                         SC.WINDOW, shift, SC.PRECISIONS[prec], int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dd_swin_last_error()
    torch.cuda.synchronize()
    for (buf, view), src in zip(bufs, (qkv, bias, None)):
        edge = torch.cat([buf[:16], buf[16 + view.numel():]]).cpu().numpy()
        assert (edge == np.float32(SENTINEL)).all(), "the kernel wrote outside a tensor"
        if src is not None:
            assert np.array_equal(view.cpu().numpy(), src, equal_nan=True), "an input was written"
    return out.cpu().numpy()


def torch_fp32(qkv, pad, bias, heads, shift):
    """The torch composition in fp32 on the device: the fp32 mode's yardstick."""
    from diffusiondepth_amd import swin as SW
    t = lambda a: None if a is None else torch.tensor(a).cuda()
    with torch.no_grad():
        return SW.window_attention_torch(t(qkv), t(pad), t(bias), heads, SC.WINDOW, shift).cpu().numpy()


@pytest.mark.parametrize("kind", ("identity", "permutation"))
@pytest.mark.parametrize("case", SC.cases(), ids=SC.case_id)
def test_exact_cases_are_bit_equal(case, kind):
    SC.check_exact(run, *case, kind)


@pytest.mark.parametrize("bias_scale", SC.BIAS_SCALES)
@pytest.mark.parametrize("case", SC.cases(), ids=SC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(case, bias_scale):
    import gpu_util
    SC.check_real(run, torch_fp32, *case, bias_scale, record=gpu_util.record, where="gpu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_batch_repeat_and_nan_identities(prec):
    SC.check_batch_and_repeat(run, prec)
    SC.check_nan(run, prec)


def test_argument_errors_leave_out_untouched():
    from diffusiondepth_amd import swin as SW
    lib = SW._lib()
    heads, C = 2, 64
    qkv = torch.zeros(1, 7, 7, 3 * C, device="cuda")
    pad = torch.zeros(3 * C, device="cuda")
    bias = torch.zeros(heads, 49, 49, device="cuda")
    out = torch.full((1, 7, 7, C), SENTINEL, device="cuda")
    f = lib.dd_window_attention_forward
    call = lambda B=1, H=7, W=7, C_=C, h=heads, win=7, shift=0, prec=1: f(qkv.data_ptr(), pad.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W, C_, h,
                                                                         win, shift, prec, None)
    for kw in (dict(C_=96), dict(h=4), dict(win=8), dict(win=14, shift=7), dict(prec=0), dict(prec=4), dict(prec=5)):
        assert call(**kw) == SC.DD_ERR_UNSUPPORTED, kw
    for kw in (dict(shift=7), dict(shift=-1), dict(B=0), dict(H=0), dict(W=-3), dict(C_=0), dict(h=0), dict(win=0)):
        assert call(**kw) == SC.DD_ERR_INVALID_ARG, kw
    assert f(qkv.data_ptr(), pad.data_ptr(), bias.data_ptr(), qkv.data_ptr(), 1, 7, 7, C, heads, 7, 0, 1, None) == SC.DD_ERR_INVALID_ARG
    assert f(qkv.data_ptr(), pad.data_ptr() + 4, bias.data_ptr(), out.data_ptr(), 1, 7, 7, C, heads, 7, 0, 1, None) == SC.DD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to out"
    with pytest.raises(ValueError, match="rel_bias"):
        SW.window_attention_forward(qkv, pad, bias[:1], heads, 7, 0)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


def _module(heads, shift, precision="fp32"):
    from diffusiondepth_amd import swin as SW
    torch.manual_seed(5)
    m = SW.HipShiftWindowMSA(32 * heads, heads, 7, shift_size=shift, precision=precision)
    m.w_msa.init_weights()
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.mul_(50.0)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.cuda().eval()


def test_the_operator_and_the_module_do_not_synchronise_the_host():
    from diffusiondepth_amd import swin as SW
    B, H, W, heads = SC.SHAPES["ragged"]
    m = _module(heads, 3)
    x = torch.randn(B, H * W, 32 * heads, device="cuda")
    qkv = torch.randn(B, H, W, 96 * heads, device="cuda")
    pad = torch.randn(96 * heads, device="cuda")
    bias = torch.randn(heads, 49, 49, device="cuda")
    m(x, (H, W))                      # (the first call loads the library and builds the dense bias)
    SW.window_attention(qkv, pad, bias, heads, 7, 3, "bf16")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = m(x, (H, W))
        z = SW.window_attention(qkv, pad, bias, heads, 7, 3, "bf16")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y).all() and torch.isfinite(z).all()


@pytest.mark.parametrize("shift", SC.SHIFTS)
@pytest.mark.parametrize("name", ["ragged", "last"])
def test_the_module_in_eval_against_the_torch_composition_on_the_device(name, shift):
    """fp32: the module's max-abs error against the fp64 oracle (qkv and proj Linears in fp64 on the CPU around swin_cases.attend) is at most
    4 x max(the torch sequence's error on the device, 1e-6)."""
    import gpu_util
    from diffusiondepth_amd import swin as SW
    B, H, W, heads = SC.SHAPES[name]
    m = _module(heads, shift)
    x = torch.randn(B, H * W, 32 * heads, device="cuda")
    calls, real = [], SW.window_attention_forward
    SW.window_attention_forward = lambda *a, **k: (calls.append(a[3:]), real(*a, **k))[1]
    try:
        with torch.no_grad():
            got = m(x, (H, W))
            assert calls == [(heads, 7, shift, "fp32")], "the module did not take the library route"
            base = m._forward_torch(x, H, W)
        assert len(calls) == 1
        y = m(x.clone().requires_grad_(True), (H, W))      # an input that needs a gradient: the torch sequence
        assert len(calls) == 1 and y.requires_grad
    finally:
        SW.window_attention_forward = real
    w = m.w_msa
    d = lambda t: t.detach().double().cpu()
    qkv = (d(x) @ d(w.qkv.weight).T + d(w.qkv.bias)).view(B, H, W, -1)
    bias = SW.dense_bias(d(w.relative_position_bias_table), w.relative_position_index.cpu())
    ora = torch.from_numpy(SC.attend(qkv.numpy(), d(w.qkv.bias).numpy(), bias.numpy(), heads, shift)).view(B, H * W, -1)
    ora = ora @ d(w.proj.weight).T + d(w.proj.bias)
    err, base_err = float((d(got) - ora).abs().max()), float((d(base) - ora).abs().max())
    print(f"module {name} shift {shift}: library {err:.3e} torch {base_err:.3e}")
    gpu_util.record("swin_module_eval", shape=name, shift=shift, err=err, baseline_err=base_err)
    assert err <= 4.0 * max(base_err, 1e-6), (err, base_err)


def test_a_tiny_backbone_with_hip_attention_through_the_model_forward():
    """backbone_attention="hip" against "torch": the same backbone weights and the same head; pred within the project's 1e-3 absolute depth bound."""
    import copy

    import diffusiondepth_amd as dda
    import gpu_util
    from diffusiondepth_amd import model as M
    from diffusiondepth_amd import swin as SW
    from diffusiondepth_amd import synth
    chans = (192, 384, 768, 1536)
    sd = synth.make_state_dict(7240, "swin", 0.05, 0.0)
    sd.update({k: v for k, v in synth.make_fpn_state_dict(7241, in_channels=chans).items() if not k.startswith("convup_fp")})
    head = dda.DDIMDepthEstimate_Swin_ADD(in_channels=list(chans), inference_steps=2, num_train_timesteps=1000, depth_feature_dim=16, loss_cfgs=[],
                                          precision="fp32")
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    head = head.cuda().eval()
    bb = SC.tiny_backbone(3)
    for p in bb.parameters():
        p.requires_grad_(False)
    models = {}
    for kind in ("torch", "hip"):
        args = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, precision="fp32", backbone_attention=kind)
        models[kind] = M.Diffusion_DCbase_Model(args, depth_backbone=copy.deepcopy(bb), depth_head=head).cuda().eval()
    assert sum(isinstance(m, SW.HipShiftWindowMSA) for m in models["hip"].depth_backbone.modules()) == 2
    assert not any(isinstance(m, SW.HipShiftWindowMSA) for m in models["torch"].depth_backbone.modules())
    B, H, W = 1, 96, 160      # the stride-4 map is 24 x 40: padded to 28 x 42
    g = torch.Generator().manual_seed(11)
    gt = torch.from_numpy(synth.make_gt_depth(12, B, H, W)).cuda()
    sample = {"rgb": torch.randn(B, 3, H, W, generator=g).cuda(), "gt": gt, "dep": gt, "depth_mask": gt > 0}
    calls, real = [], SW.window_attention_forward
    SW.window_attention_forward = lambda *a, **k: (calls.append(a[3:]), real(*a, **k))[1]
    out = {}
    try:
        for kind, model in models.items():
            torch.manual_seed(99)      # (the head draws x_T from the device generator)
            with torch.no_grad():
                out[kind] = model(sample)["pred"]
            assert len(calls) == (2 if kind == "hip" else 0)
    finally:
        SW.window_attention_forward = real
    assert calls == [(6, 7, 0, "fp32"), (6, 7, 3, "fp32")]
    err = float((out["hip"] - out["torch"]).abs().max())
    gpu_util.record("swin_tiny_backbone_model", pred_maxabs=err, pred_max=float(out["torch"].abs().max()))
    print(f"tiny backbone through the model: pred max-abs difference {err:.3e} (pred up to {float(out['torch'].abs().max()):.3f})")
    assert torch.isfinite(out["hip"]).all() and err < 1e-3
