"""GPU (`-m gpu`): the attention backward of include/train/ddepth_swin_backward.h / diffusiondepth_amd.swin on the MI355X -- the cases of
tests/swin_backward_cases.py through the built library (sentinels around every tensor and the workspace), no host synchronisation, the module
in .train() with ``backward="hip"`` against an fp64 oracle and the torch route, what one module forward saves for its backward, and one
training step of a tiny Swin-like backbone under ``backbone_attention="hip+train"`` against ``"torch"``."""
import copy

import numpy as np
import pytest
import torch

import swin_backward_cases as BC
import swin_cases as SC

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678


def _guarded(a, fill=None):
    """A device copy of ``a`` (or ``fill``) with 16 sentinel floats (64 bytes: the alignment stays) in front of and behind it -> (buffer, view)."""
    buf = torch.full((a.size + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[16:16 + a.size].view(a.shape)
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    else:
        view.fill_(fill)
    return buf, view


def run(qkv, pad, bias, gout, heads, shift, prec, scale=None, want_pad=True, want_bias=True, poison=False):
    from diffusiondepth_amd import swin as SW
    B, H, W, K = qkv.shape
    C = K // 3
    nan = float("nan")
    ins = [_guarded(qkv), _guarded(bias), _guarded(gout)] + ([_guarded(pad)] if pad is not None else [])
    ws_floats = SW.backward_workspace_bytes(B, H, W, C, heads, 7, prec) // 4
    outs = [_guarded(np.empty((B, H, W, K), dtype=np.float32), nan), _guarded(np.empty(K, dtype=np.float32), nan),
            _guarded(np.empty((heads, 49, 49), dtype=np.float32), nan), _guarded(np.empty(ws_floats, dtype=np.float32), nan if poison else 7.0)]
    q, bs, go = (v for _, v in ins[:3])
    p = ins[3][1] if pad is not None else None
    gq, gp, gb, ws = (v for _, v in outs)
    sc = None if scale is None else torch.from_numpy(scale.copy()).cuda()
    ptr = lambda t, on=True: t.data_ptr() if (t is not None and on) else None
    lib = SW._lib()
    rc = lib.dd_window_attention_backward(ptr(q), ptr(p), ptr(bs), ptr(go), ptr(gq), ptr(gp, want_pad), ptr(gb, want_bias), ptr(ws), ptr(sc), B, H, W, C,
                                          heads, SC.WINDOW, shift, SC.PRECISIONS[prec], int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.dd_swin_last_error()
    torch.cuda.synchronize()
    for buf, view in ins + outs:
        edge = torch.cat([buf[:16], buf[16 + view.numel():]]).cpu().numpy()
        assert (edge == np.float32(SENTINEL)).all(), "a kernel wrote outside a tensor"
    for (_, view), src in zip(ins, (qkv, bias, gout, pad)):
        assert np.array_equal(view.cpu().numpy(), src, equal_nan=True), "an input was written"
    if not want_pad:
        assert bool(torch.isnan(gp).all())
    if not want_bias:
        assert bool(torch.isnan(gb).all())
    return gq.cpu().numpy(), gp.cpu().numpy() if want_pad else None, gb.cpu().numpy() if want_bias else None


@pytest.mark.parametrize("bias_scale", SC.BIAS_SCALES)
@pytest.mark.parametrize("case", SC.cases(), ids=SC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(case, bias_scale):
    import gpu_util
    BC.check_real(run, *case, bias_scale, record=gpu_util.record, where="gpu")


@pytest.mark.parametrize("kind", ("identity", "permutation"))
@pytest.mark.parametrize("case", SC.cases(), ids=SC.case_id)
def test_one_hot_cases_are_exact(case, kind):
    BC.check_onehot(run, *case, kind)


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
@pytest.mark.parametrize("name", list(SC.SHAPES))
def test_half_half_cases_are_exact(name, prec):
    BC.check_halves(run, name, prec)


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_repeat_batch_workspace_null_and_nan_identities(prec):
    BC.check_identities(run, prec)
    BC.check_nan(run, prec)


def test_f16_grad_out_scale_is_exact_in_powers_of_two():
    BC.check_f16_scale(run)


def test_the_library_s_own_scale_is_the_rule_of_the_cases():
    """dd_conv_grad_scale on the device writes what swin_backward_cases.grad_scale computes: the Function's f16 backward runs the checked path."""
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd import swin as SW
    for k in (-24, 0, 16):
        g = (BC.grad_out("ragged", 3) * np.float32(2.0 ** k)).astype(np.float32)
        got = CV.grad_scale(torch.from_numpy(g).cuda(), SW.PRECISIONS["f16"]).cpu().numpy()
        assert np.array_equal(got[:2], BC.grad_scale(g)[:2]), (k, got)


def test_argument_errors_leave_the_outputs_untouched():
    from diffusiondepth_amd import swin as SW
    lib = SW._lib()
    heads, C = 2, 64
    z = lambda *s: torch.zeros(*s, device="cuda")
    qkv, pad, bias, gout = z(1, 7, 7, 3 * C), z(3 * C), z(heads, 49, 49), z(1, 7, 7, C)
    s = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    gq, gp, gb, ws = s(1, 7, 7, 3 * C), s(3 * C), s(heads, 49, 49), s(SW.backward_workspace_bytes(1, 7, 7, C, heads) // 4)
    f = lib.dd_window_attention_backward

    def call(B=1, H=7, W=7, C_=C, h=heads, win=7, shift=0, prec=1, **swap):
        a = dict(qkv=qkv.data_ptr(), pad=pad.data_ptr(), bias=bias.data_ptr(), gout=gout.data_ptr(), gq=gq.data_ptr(), gp=gp.data_ptr(),
                 gb=gb.data_ptr(), ws=ws.data_ptr(), scale=None)
        a.update(swap)
        return f(*(a[k] for k in ("qkv", "pad", "bias", "gout", "gq", "gp", "gb", "ws", "scale")), B, H, W, C_, h, win, shift, prec, None)

    for kw in (dict(C_=96), dict(h=4), dict(win=8), dict(prec=0), dict(prec=4)):
        assert call(**kw) == SC.DD_ERR_UNSUPPORTED, kw
    for kw in (dict(shift=7), dict(shift=-1), dict(B=0), dict(W=-3), dict(gq=None), dict(ws=None), dict(gq=qkv.data_ptr()), dict(gp=gb.data_ptr()),
               dict(gout=gout.data_ptr() + 4)):
        assert call(**kw) == SC.DD_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (gq, gp, gb, ws)), "a refused call wrote to an output"
    with pytest.raises(ValueError, match="grad_out"):
        SW.window_attention_backward(qkv, pad, bias, gout[:, :3], heads, 7, 0)
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(bool((t == SENTINEL).any()) for t in (gq, gp, gb))


def _module(heads, shift, precision="fp32", drop=0.0, **kw):
    from diffusiondepth_amd import swin as SW
    torch.manual_seed(5)
    m = SW.HipShiftWindowMSA(32 * heads, heads, 7, shift_size=shift, precision=precision, dropout_layer=dict(type="DropPath", drop_prob=drop), **kw)
    m.w_msa.init_weights()
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.mul_(50.0)
    return m.cuda().train()


def test_the_function_s_backward_and_the_module_do_not_synchronise_the_host():
    from diffusiondepth_amd import swin as SW
    B, H, W, heads = SC.SHAPES["ragged"]
    m = _module(heads, 3, "f16", drop=0.2, backward="hip")
    x = torch.randn(B, H * W, 32 * heads, device="cuda", requires_grad=True)
    qkv = torch.randn(B, H, W, 96 * heads, device="cuda", requires_grad=True)
    pad = torch.randn(96 * heads, device="cuda", requires_grad=True)
    bias = torch.randn(heads, 49, 49, device="cuda", requires_grad=True)
    g = torch.randn(B, H, W, 32 * heads, device="cuda")

    def step():
        m(x, (H, W)).sum().backward()
        out = SW.WindowAttentionFunction.apply(qkv, pad, bias, heads, 7, 3, "f16", True)
        return torch.autograd.grad(out, (qkv, pad, bias), g)

    step()                      # (the first call loads the library, builds the fold index and allocates the workspace)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        grads = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t).all()) for t in grads) and all(p.grad is not None for p in m.parameters())


def _oracle_module_grads(m, x, g, H, W, shift, keep_mask):
    """fp64 on the CPU: the two Linears around swin_backward_cases.attend_indexed, times the DropPath factor -> gradients of x and the parameters."""
    from diffusiondepth_amd import swin as SW
    w = m.w_msa
    d = lambda t: t.detach().double().cpu().requires_grad_(True)
    xs, params = d(x), [d(p) for p in m.parameters()]
    table, qw, qb, pw, pb = params      # (the order of WindowMSA's parameters)
    B = x.shape[0]
    qkv = (xs @ qw.T + qb).view(B, H, W, -1)
    bias = SW.dense_bias(table, w.relative_position_index.cpu())
    y = BC.attend_indexed(qkv, qb, bias, int(w.num_heads), shift).view(B, H * W, -1) @ pw.T + pb
    y = y * keep_mask.double().cpu()
    grads = torch.autograd.grad(y, [xs] + params, g.double().cpu())
    return y.detach(), grads


@pytest.mark.parametrize("shift", SC.SHIFTS)
@pytest.mark.parametrize("name", ["ragged", "last"])
def test_the_module_in_train_against_the_fp64_oracle_and_the_torch_route(name, shift):
    """fp32, an active DropPath under one seed on both routes: per tensor (the input and the five parameters) the library route's max-abs error
    against the fp64 oracle is at most 4 x max(the torch route's error on the device, 1e-6 max(1, max |oracle|))."""
    import gpu_util
    from diffusiondepth_amd import swin as SW
    B, H, W, heads = SC.SHAPES[name]
    drop = 0.25
    m = _module(heads, shift, drop=drop, backward="hip")
    assert [n for n, _ in m.named_parameters()] == ["w_msa.relative_position_bias_table", "w_msa.qkv.weight", "w_msa.qkv.bias", "w_msa.proj.weight",
                                                    "w_msa.proj.bias"]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(B, H * W, 32 * heads, generator=gen).cuda()
    g = torch.randn(B, H * W, 32 * heads, generator=gen).cuda()
    torch.manual_seed(1234)
    keep = torch.empty((B, 1, 1), device="cuda").bernoulli_(1.0 - drop) / (1.0 - drop)      # what DropPath draws first under this seed
    calls, real = [], SW.window_attention_backward
    SW.window_attention_backward = lambda *a, **k: (calls.append(a[4:8]), real(*a, **k))[1]
    results = {}
    try:
        for route in ("hip", "torch"):
            m.backward = route
            m.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            torch.manual_seed(1234)
            y = m(xr, (H, W))
            y.backward(g)
            results[route] = (y.detach(), [xr.grad] + [p.grad for p in m.parameters()])
            assert len(calls) == 1, "the hip route did not make exactly one backward call, or the torch route made one"
    finally:
        SW.window_attention_backward = real
    assert calls == [(heads, 7, shift, "fp32")]
    y64, want = _oracle_module_grads(m, x, g, H, W, shift, keep)
    for route in ("hip", "torch"):      # (the forward agrees with the oracle: the DropPath mask is the one the oracle used)
        assert float((results[route][0].double().cpu() - y64).abs().max()) <= 1e-4 * max(1.0, float(y64.abs().max()))
    names = ["input"] + [n for n, _ in m.named_parameters()]
    rows = []
    for n, a, b, o in zip(names, results["hip"][1], results["torch"][1], want):
        err, base = float((a.double().cpu() - o).abs().max()), float((b.double().cpu() - o).abs().max())
        bound = 4.0 * max(base, 1e-6 * max(1.0, float(o.abs().max())))
        print(f"module train {name} shift {shift} {n}: library {err:.3e} torch {base:.3e} bound {bound:.3e}")
        gpu_util.record("swin_module_train", shape=name, shift=shift, tensor=n, err=err, baseline_err=base)
        rows.append((n, err, bound))
    for n, err, bound in rows:
        assert err <= bound, (n, err, bound)


def test_what_one_module_forward_saves_for_its_backward():
    """Saved-tensor bytes of one forward on the "hip" route (distinct tensors; the module's own parameters, which live anyway, not counted on
    either side): at most what the two Linears save plus qkv plus the dense bias, and no [.., heads, 49, 49] tensor; the torch route saves
    the probabilities."""
    B, H, W, heads = SC.SHAPES["last"]
    C = 32 * heads
    m = _module(heads, 3, backward="hip")
    x = torch.randn(B, H * W, C, device="cuda", requires_grad=True)

    own = {p.data_ptr() for p in m.parameters()}

    def saved(fn):
        seen = {}

        def pack(t):
            if t.data_ptr() in own:
                return t
            seen[(t.data_ptr(), tuple(t.shape))] = (t.numel() * t.element_size(), tuple(t.shape))
            return t
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            fn()
        return seen

    hip = saved(lambda: m(x, (H, W)))
    w = m.w_msa
    x2 = torch.randn_like(x).requires_grad_(True)      # (proj reads the attention's output, not the module's input)
    linears = saved(lambda: (w.qkv(x), w.proj(x2)))
    budget = sum(b for b, _ in linears.values()) + 4 * B * H * W * 3 * C + 4 * heads * 49 * 49
    total = sum(b for b, _ in hip.values())
    print(f"saved for the backward: hip route {total} bytes, budget {budget} bytes")
    assert total <= budget, (total, budget, sorted(s for _, s in hip.values()))
    scores = lambda seen: [s for _, s in seen.values() if len(s) >= 4 and s[-2:] == (49, 49)]
    assert not scores(hip)
    m.backward = "torch"
    assert len(scores(saved(lambda: m(x, (H, W))))) >= 1


def test_one_training_step_of_a_tiny_backbone_through_the_model():
    """backbone_attention="hip+train" against "torch": the same weights, the same head, one training forward + backward under one seed.  Every
    backbone parameter's gradient within 1e-4 relative L2 -- the 1e-5 of the CPU gradient test, one order looser for the device's fp32 GEMMs --
    or 4 x the torch route's own run-to-run distance where that is larger (recorded)."""
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
    head = head.cuda().train()
    bb = SC.tiny_backbone(3)
    models = {}
    for kind in ("torch", "hip+train"):
        args = M.default_args(head_specify="DDIMDepthEstimate_Swin_ADD", inference_steps=2, precision="fp32", backbone_attention=kind)
        models[kind] = M.Diffusion_DCbase_Model(args, depth_backbone=copy.deepcopy(bb), depth_head=head).cuda().train()
    hips = [m for m in models["hip+train"].depth_backbone.modules() if isinstance(m, SW.HipShiftWindowMSA)]
    assert len(hips) == 2 and all(h.backward == "hip" for h in hips)
    B, H, W = 1, 96, 160      # the stride-4 map is 24 x 40: padded to 28 x 42
    rgb = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(11)).cuda()
    gt = torch.from_numpy(synth.make_gt_depth(12, B, H, W)).cuda()
    calls, real = [], SW.window_attention_backward
    SW.window_attention_backward = lambda *a, **k: (calls.append(a[4:8]), real(*a, **k))[1]

    def step(model):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(99)      # (the head draws its noise from the device generator)
        out = model.extract_depth(rgb, gt, gt > 0, gt_depth_map=gt, return_loss=True)
        loss = (out["pred"] - gt).abs().mean() + out["ddim_loss"]
        loss.backward()
        return {k: p.grad.detach().double().clone() for k, p in model.depth_backbone.named_parameters()}

    try:
        torch_a = step(models["torch"])
        torch_b = step(models["torch"])
        assert not calls
        got = step(models["hip+train"])
    finally:
        SW.window_attention_backward = real
    assert sorted(calls) == [(6, 7, 0, "fp32"), (6, 7, 3, "fp32")]
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    assert set(got) == set(torch_a) and len(got) >= 10
    for k in sorted(got):
        err, noise = rel(got[k], torch_a[k]), rel(torch_b[k], torch_a[k])
        bound = max(1e-4, 4.0 * noise)
        print(f"{k}: hip+train against torch {err:.3e}, torch run to run {noise:.3e}, bound {bound:.3e}")
        gpu_util.record("swin_tiny_backbone_train_step", parameter=k, rel_l2=err, torch_run_to_run=noise)
        assert torch.isfinite(got[k]).all() and err <= bound, (k, err, bound)
