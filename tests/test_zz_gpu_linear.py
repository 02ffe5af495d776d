"""GPU (`-m gpu`): the token Linears of include/swin/ddepth_linear.h / diffusiondepth_amd.linear on the MI355X -- the cases of tests/linear_cases.py
through the built library (exact families bit-equal at every precision, real-valued cases within 4 x the baseline's own error against the fp64
oracle, repeat / row-prefix / NaN identities, sentinels around every tensor and the packed image, argument validation), no host
synchronisation, ``HipFFN`` and ``HipShiftWindowMSA(linear="hip")`` in .eval() against an fp64 oracle, the pack cache, and the tiny backbone of
whole blocks under ``backbone_linear="hip"`` through ``Diffusion_DCbase_Model.forward`` with a Swin head."""
import numpy as np
import pytest
import torch

import linear_cases as LC
import swin_cases as SC

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


def _guarded(a):
    """A device copy of ``a`` with 16 sentinel floats (64 bytes: the alignment stays) in front of and behind it -> (buffer, view)."""
    buf = torch.full((a.size + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[16:16 + a.size].view(a.shape)
    view.copy_(torch.tensor(a))
    return buf, view


def run(x, w, bias, addend, act, prec):
    from diffusiondepth_amd import linear as LN
    (M, K), N = x.shape, w.shape[0]
    lib = LN._lib()
    nbytes = LN.packed_bytes(K, N, prec)
    srcs = [x, w, bias, addend, np.full(nbytes // 4, np.nan, dtype=np.float32), np.full((M, N), np.nan, dtype=np.float32)]
    bufs = [None if a is None else _guarded(a) for a in srcs]
    ptr = lambda i: None if bufs[i] is None else bufs[i][1].data_ptr()
    stream = int(torch.cuda.current_stream().cuda_stream)
    rc = lib.dd_linear_pack(ptr(1), ptr(4), K, N, LC.PRECISIONS[prec], stream)
    assert rc == 0, lib.dd_linear_last_error()
    image = bufs[4][1].clone()
    rc = lib.dd_linear_forward(ptr(0), ptr(4), ptr(2), ptr(3), ptr(5), M, K, N, act, LC.PRECISIONS[prec], stream)
    assert rc == 0, lib.dd_linear_last_error()
    torch.cuda.synchronize()
    for pair, src in zip(bufs, srcs[:4] + [None, None]):
        if pair is None:
            continue
        buf, view = pair
        edge = torch.cat([buf[:16], buf[16 + view.numel():]]).cpu().numpy()
        assert (edge == np.float32(SENTINEL)).all(), "a kernel wrote outside a tensor"
        if src is not None:
            assert np.array_equal(view.cpu().numpy(), src, equal_nan=True), "an input was written"
    assert torch.equal(bufs[4][1].view(torch.int32), image.view(torch.int32)), "the forward wrote the packed image"
    return bufs[5][1].cpu().numpy()


@pytest.mark.parametrize("case", LC.cases(), ids=LC.case_id)
def test_exact_cases_are_bit_equal(case):
    LC.check_ints(run, *case)
    LC.check_selection(run, *case)


@pytest.mark.parametrize("variant", LC.VARIANTS)
@pytest.mark.parametrize("case", LC.cases(), ids=LC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(case, variant):
    import gpu_util
    LC.check_real(run, *case, variant, record=gpu_util.record, where="gpu")


@pytest.mark.parametrize("prec", list(LC.PRECISIONS))
def test_repeat_row_prefix_and_nan_identities(prec):
    LC.check_repeat_and_rows(run, prec)
    LC.check_nan(run, prec)


@pytest.mark.parametrize("prec", ("bf16", "f16"))
def test_row_prefixes_across_the_two_tile_heights(prec):
    LC.check_repeat_and_rows(run, prec, name="big+1", edges=LC.TILE_EDGES["big"])


def test_argument_errors_leave_y_untouched():
    from diffusiondepth_amd import linear as LN
    lib = LN._lib()
    M, K, N = 5, 64, 96
    x, w, bias, addend = (torch.ones(s, device="cuda") for s in ((M, K), (N, K), (N,), (M, N)))
    wp = LN.pack_weight(w, "fp32").data
    y = torch.full((M, N), SENTINEL, device="cuda")
    f = lib.dd_linear_forward
    P = lambda t: None if t is None else t.data_ptr()
    call = lambda M_=M, K_=K, N_=N, act=0, prec=1, x_=x, wp_=wp, b_=bias, a_=addend, y_=y: f(P(x_), P(wp_), P(b_), P(a_), P(y_), M_, K_, N_, act, prec, None)
    for kw in (dict(K_=48), dict(N_=8224), dict(act=2), dict(prec=0), dict(prec=4), dict(prec=9)):
        assert call(**kw) == LC.DD_ERR_UNSUPPORTED, kw
        assert lib.dd_linear_last_error()
    for kw in (dict(M_=0), dict(x_=None), dict(y_=x), dict(y_=addend), dict(y_=wp)):
        assert call(**kw) == LC.DD_ERR_INVALID_ARG, kw
    assert call(x_=None) == LC.DD_ERR_INVALID_ARG and b"null" in lib.dd_linear_last_error()
    assert f(P(x), P(wp), P(bias), P(addend), P(y) + 4, M, K, N, 0, 1, None) == LC.DD_ERR_INVALID_ARG and b"aligned" in lib.dd_linear_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()), "a refused call wrote to y"
    with pytest.raises(ValueError, match="addend"):
        LN.linear_forward(x, LN.pack_weight(w, "bf16"), bias, addend[:2])
    with pytest.raises(ValueError, match="packed for"):
        LN.linear_forward(x, LN.pack_weight(w, "bf16"), bias, None, 0, "f16")
    with pytest.raises(RuntimeError, match="does not run"):
        LN.pack_weight(torch.ones(48, 64, device="cuda"))
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == K + 2).all())


def _ffn(dims, precision):
    from diffusiondepth_amd import linear as LN
    torch.manual_seed(7)
    m = LN.HipFFN(dims, 4 * dims, precision=precision)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.cuda().eval()


def _attention(heads, shift, linear_precision):
    from diffusiondepth_amd import swin as SW
    torch.manual_seed(5)
    m = SW.HipShiftWindowMSA(32 * heads, heads, 7, shift_size=shift, precision="fp32", linear="hip", linear_precision=linear_precision)
    m.w_msa.init_weights()
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.mul_(50.0)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.cuda().eval()


def test_the_operator_and_the_modules_do_not_synchronise_the_host_and_pack_once():
    from diffusiondepth_amd import linear as LN
    B, H, W, heads = SC.SHAPES["ragged"]
    C = 32 * heads
    ffn, att = _ffn(C, "bf16"), _attention(heads, 3, "bf16")
    x = torch.randn(B, H * W, C, device="cuda")
    w, b = torch.randn(3 * C, C, device="cuda"), torch.randn(3 * C, device="cuda")
    before = LN.PACK_COUNT
    ffn(x), att(x, (H, W))      # (the first calls load the library, build the dense bias and pack the four weights)
    assert LN.PACK_COUNT == before + 4
    packed = LN.pack_weight(w, "f16")
    torch.cuda.synchronize()
    count = LN.PACK_COUNT
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = ffn(x, identity=x)
        z = att(x, (H, W))
        q = LN.linear_forward(x, packed, b, None, LN.ACT_GELU, "f16")
        p2 = LN.pack_weight(w, "bf16")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert LN.PACK_COUNT == count + 1, "a second forward packed a weight again"
    assert torch.isfinite(y).all() and torch.isfinite(z).all() and torch.isfinite(q).all() and p2.data.numel() == 2 * w.numel()
    with torch.no_grad():
        ffn.layers[1].weight.mul_(0.5)      # an in-place update: exactly that image is rebuilt
    y2 = ffn(x, identity=x)
    assert LN.PACK_COUNT == count + 2 and not torch.equal(y2, y)


@pytest.mark.parametrize("prec", list(LC.PRECISIONS))
@pytest.mark.parametrize("tokens", ["ragged", "last"])
def test_hipffn_in_eval_against_the_fp64_oracle(tokens, prec):
    """(340, 96) and (418, 192).  fp32: at most 4 x max(the torch route's error on the device, 1e-6); 16-bit modes: recorded."""
    import gpu_util
    from diffusiondepth_amd import linear as LN
    B, H, W, heads = SC.SHAPES[tokens]
    C = 32 * heads
    m = _ffn(C, prec)
    g = torch.Generator().manual_seed(3)
    x, idt = torch.randn(B, H * W, C, generator=g).cuda(), torch.randn(B, H * W, C, generator=g).cuda()
    calls, real = [], LN.linear_forward
    LN.linear_forward = lambda *a, **k: (calls.append(a[4:]), real(*a, **k))[1]
    try:
        with torch.no_grad():
            got = m(x, identity=idt)
            assert calls == [(LN.ACT_GELU, prec), (LN.ACT_NONE, prec)], "the module did not take the library route"
            base = idt + m.layers(x)
        y = m(x.clone().requires_grad_(True))      # an input that needs a gradient: the torch sequence
        assert len(calls) == 2 and y.requires_grad
        m.train()
        for p in m.parameters():
            p.requires_grad_(True)
        assert m(x).requires_grad and len(calls) == 2
    finally:
        LN.linear_forward = real
    d = lambda t: t.detach().double().cpu()
    fc1, fc2 = m.layers[0][0], m.layers[1]
    ora = d(idt) + torch.nn.functional.gelu(d(x) @ d(fc1.weight).T + d(fc1.bias)) @ d(fc2.weight).T + d(fc2.bias)
    err, base_err = float((d(got) - ora).abs().max()), float((d(base) - ora).abs().max())
    print(f"HipFFN {tokens} {prec}: library {err:.3e} torch {base_err:.3e}")
    gpu_util.record("swin_linear_ffn_eval", shape=tokens, precision=prec, err=err, baseline_err=base_err)
    assert torch.isfinite(got).all()
    if prec == "fp32":
        assert err <= 4.0 * max(base_err, 1e-6), (err, base_err)


@pytest.mark.parametrize("prec", list(LC.PRECISIONS))
@pytest.mark.parametrize("tokens,shift", [("ragged", 3), ("last", 0)])
def test_the_attention_module_with_hip_linears_against_the_fp64_oracle(tokens, shift, prec):
    import gpu_util
    from diffusiondepth_amd import linear as LN
    from diffusiondepth_amd import swin as SW
    B, H, W, heads = SC.SHAPES[tokens]
    m = _attention(heads, shift, prec)
    x = torch.randn(B, H * W, 32 * heads, generator=torch.Generator().manual_seed(4)).cuda()
    calls, real = [], LN.linear_forward
    LN.linear_forward = lambda *a, **k: (calls.append(a[4:]), real(*a, **k))[1]
    try:
        with torch.no_grad():
            got = m(x, (H, W))
            assert calls == [(LN.ACT_NONE, prec)] * 2, "the module did not run qkv and proj in the library"
            m.linear = "torch"
            plain = m(x, (H, W))      # the parent's inference branch: torch Linears around the library attention
            base = m._forward_torch(x, H, W)
            m.linear = "hip"
        assert len(calls) == 2
        y = m(x.clone().requires_grad_(True), (H, W))
        assert len(calls) == 2 and y.requires_grad
    finally:
        LN.linear_forward = real
    w = m.w_msa
    d = lambda t: t.detach().double().cpu()
    qkv = (d(x) @ d(w.qkv.weight).T + d(w.qkv.bias)).view(B, H, W, -1)
    bias = SW.dense_bias(d(w.relative_position_bias_table), w.relative_position_index.cpu())
    ora = torch.from_numpy(SC.attend(qkv.numpy(), d(w.qkv.bias).numpy(), bias.numpy(), heads, shift)).view(B, H * W, -1)
    ora = ora @ d(w.proj.weight).T + d(w.proj.bias)
    err, base_err, plain_err = (float((d(t) - ora).abs().max()) for t in (got, base, plain))
    print(f"attention {tokens} shift {shift} linear {prec}: library {err:.3e} torch {base_err:.3e} torch Linears {plain_err:.3e}")
    gpu_util.record("swin_linear_attention_eval", shape=tokens, shift=shift, precision=prec, err=err, baseline_err=base_err, torch_linear_err=plain_err)
    assert torch.isfinite(got).all()
    if prec == "fp32":
        assert err <= 4.0 * max(base_err, 1e-6), (err, base_err)


def test_a_tiny_backbone_with_hip_linears_through_the_model_forward():
    """backbone_attention="hip" + backbone_linear="hip" at fp32 against the all-torch model: the same backbone weights and the same head; pred
    within the project's 1e-3 absolute depth bound.  The bf16 difference is recorded."""
    import copy

    import diffusiondepth_amd as dda
    import gpu_util
    from diffusiondepth_amd import linear as LN
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
    bb = LC.tiny_backbone(3)
    for p in bb.parameters():
        p.requires_grad_(False)
    kinds = {"torch": {}, "fp32": dict(backbone_attention="hip", backbone_linear="hip", backbone_linear_precision="fp32"),
             "bf16": dict(backbone_attention="hip", backbone_linear="hip", backbone_linear_precision="bf16")}
    models = {}
    for kind, kw in kinds.items():
        args = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, precision="fp32", **kw)
        models[kind] = M.Diffusion_DCbase_Model(args, depth_backbone=copy.deepcopy(bb), depth_head=head).cuda().eval()
    count = lambda model, cls: sum(isinstance(m, cls) for m in model.depth_backbone.modules())
    assert count(models["fp32"], LN.HipFFN) == 2 and count(models["fp32"], SW.HipShiftWindowMSA) == 2
    assert count(models["torch"], LN.HipFFN) == 0 and count(models["torch"], SW.HipShiftWindowMSA) == 0
    B, H, W = 1, 96, 160      # the stride-4 map is 24 x 40: 960 tokens of 192 channels
    g = torch.Generator().manual_seed(11)
    gt = torch.from_numpy(synth.make_gt_depth(12, B, H, W)).cuda()
    sample = {"rgb": torch.randn(B, 3, H, W, generator=g).cuda(), "gt": gt, "dep": gt, "depth_mask": gt > 0}
    calls, real = [], LN.linear_forward
    LN.linear_forward = lambda *a, **k: (calls.append(a[4:]), real(*a, **k))[1]
    out = {}
    try:
        for kind, model in models.items():
            n = len(calls)
            torch.manual_seed(99)      # (the head draws x_T from the device generator)
            with torch.no_grad():
                out[kind] = model(sample)["pred"]
            assert len(calls) - n == (0 if kind == "torch" else 8)      # two blocks of qkv, proj, fc1, fc2
    finally:
        LN.linear_forward = real
    assert calls[:4] == [(LN.ACT_NONE, "fp32"), (LN.ACT_NONE, "fp32"), (LN.ACT_GELU, "fp32"), (LN.ACT_NONE, "fp32")]
    err = float((out["fp32"] - out["torch"]).abs().max())
    err16 = float((out["bf16"] - out["torch"]).abs().max())
    gpu_util.record("swin_linear_tiny_backbone_model", pred_maxabs_fp32=err, pred_maxabs_bf16=err16, pred_max=float(out["torch"].abs().max()))
    print(f"tiny backbone through the model: pred max-abs difference fp32 {err:.3e}, bf16 {err16:.3e} (pred up to {float(out['torch'].abs().max()):.3f})")
    assert torch.isfinite(out["fp32"]).all() and torch.isfinite(out["bf16"]).all() and err < 1e-3
