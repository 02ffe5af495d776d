"""GPU (`-m gpu`): the power-of-two rescale of grad_y in the f16 / f16x3 backward of the training convolutions (include/ddepth_conv_scaled.h;
``grad_autoscale`` of diffusiondepth_amd.conv) on the MI355X.

Operator level, through ``conv.grad_scale`` and ``conv.conv_backward_data / _weight(..., scale=...)``: the cases of tests/conv_scaled_cases.py --
equivariance under 2^k, the caps at training scale (grad_y 2^-20, and with a spike), exact integer data through the multi-split reduce twin,
bf16 and s = 1 identities with the unscaled entry points, Inf / NaN elements; nothing synchronises the host.  Module level: the Res head's FPN
and a ragged neck (MPViT widths 216 / 288) in .train() with ``grad_autoscale`` on, at a loss 2^-20 times the unit one: every gradient equals
2^-20 times the unit-scale gradient of the same module bit for bit, and the FPN's stay within the relative L2 bound of tests/test_gpu_backward.py
for the precision (5e-3 for f16x3, 6e-2 for f16) of the default head in fp64 on the CPU."""
import numpy as np
import pytest
import torch

import conv_scaled_cases as SC

pytestmark = pytest.mark.gpu
TOL = {"f16x3": 5e-3, "f16": 6e-2}      # tests/test_gpu_backward.py: relative L2 per tensor
ONE = np.float32(1).view(np.uint32)


def _backward(case, prec, x, w, grad_y, scaled=True, channels="any"):
    """The two gradients through diffusiondepth_amd.conv -> {"grad_x", "grad_w", "scale" (4 uint32, scaled only)} as numpy."""
    from diffusiondepth_amd import conv as CV
    op, _ = SC.geometry(case)
    p = SC.PRECISIONS[prec]
    xs, ws, ys = SC.shapes(case)
    xd, wd, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x.reshape(xs), w.reshape(ws), grad_y.reshape(ys)))
    extra = (channels,) if channels != "block64" else ()
    kw = {"scale": CV.grad_scale(gd, p)} if scaled else {}
    gx = CV.conv_backward_data(op, gd, wd, xd.shape, p, *extra, **kw)
    gw = CV.conv_backward_weight(op, xd, gd, wd.shape, p, *extra, **kw)
    out = {"grad_x": gx.cpu().numpy(), "grad_w": gw.cpu().numpy()}
    if scaled:
        out["scale"] = kw["scale"].cpu().numpy().view(np.uint32)
        want = np.array([ONE, ONE, 0, 0], dtype=np.uint32) if prec == "bf16" else SC.scale_words(grad_y)
        assert np.array_equal(out["scale"], want), (out["scale"], want)
    return out


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in SC.KEYS)


@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EQUIVARIANCE)
def test_a_gradient_two_to_the_k_times_another_gives_two_to_the_k_times_the_result(case, prec):
    inp = SC.inputs(case)
    base = _backward(case, prec, inp["x"], inp["w"], inp["grad_y"])
    bad = []
    for k in SC.K_SMALL:
        got = _backward(case, prec, inp["x"], inp["w"], SC.small(inp["grad_y"], k))
        bad += [(k,) + b for b in SC.check_equivariant(got, base, k, f"gpu {case} {prec}")]
    assert not bad, bad


@pytest.mark.parametrize("which", ["small", "spike"])
@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.CAPS)
def test_a_gradient_at_training_scale_stays_within_the_cap(case, prec, which):
    inp = SC.inputs(case)
    SC.check_caps(_backward(case, prec, inp["x"], inp["w"], SC.variant(case, which)), case, which, prec, "gpu")


@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EXACT)
def test_integer_data_at_two_to_the_minus_twenty_is_exact(case, prec):
    inp = SC.inputs(case, "int")
    SC.check_exact(_backward(case, prec, inp["x"], inp["w"], SC.small(inp["grad_y"], -20)), case, -20, "gpu")


@pytest.mark.parametrize("case", SC.BF16_IDENTITY)
def test_bf16_runs_the_unscaled_kernels(case):
    inp = SC.inputs(case)
    gy = SC.small(inp["grad_y"], -20)
    assert _same_bits(_backward(case, "bf16", inp["x"], inp["w"], gy), _backward(case, "bf16", inp["x"], inp["w"], gy, scaled=False))


@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.BLOCK64_IDENTITY)
def test_with_s_equal_to_one_a_block64_shape_gives_the_bits_of_the_old_entry_points(case, prec):
    inp = SC.inputs(case)
    gy = SC.power_of_two_into_top_binade(inp["grad_y"])
    a = _backward(case, prec, inp["x"], inp["w"], gy)
    assert a["scale"][0] == ONE
    assert _same_bits(a, _backward(case, prec, inp["x"], inp["w"], gy, scaled=False, channels="block64"))


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EDGE)
def test_an_inf_or_nan_element_takes_no_part_in_the_scale_and_stays_in_its_footprint(case, prec, value):
    inp = SC.inputs(case)
    idx = SC.edge_element(case)
    zeroed = SC.small(inp["grad_y"], -20)
    zeroed[idx] = 0
    bad = zeroed.copy()
    bad[idx] = value
    a, b = _backward(case, prec, inp["x"], inp["w"], bad), _backward(case, prec, inp["x"], inp["w"], zeroed)
    assert np.array_equal(a["scale"], b["scale"])
    for k, mask in SC.footprint(case, idx).items():
        assert np.array_equal(a[k].view(np.uint32)[~mask], b[k].view(np.uint32)[~mask]), k
        assert not np.isfinite(a[k][mask]).all(), "the element travels through as it is"


def test_an_all_zero_gradient_gives_s_one_and_zeros():
    for case in SC.EDGE:
        inp = SC.inputs(case)
        got = _backward(case, "f16x3", inp["x"], inp["w"], np.zeros_like(inp["grad_y"]))
        assert got["scale"][0] == ONE and got["scale"][2] == 0 and not got["grad_x"].any() and not got["grad_w"].any()


@pytest.mark.parametrize("case", ["cc:S2", "cc:D1", "rg:P2"])
def test_the_scaled_backward_does_not_synchronise_the_host(case):
    from diffusiondepth_amd import conv as CV
    op, _ = SC.geometry(case)
    inp = SC.inputs(case)
    p = SC.PRECISIONS["f16x3"]
    x, w, gy = (torch.from_numpy(inp[k]).cuda() for k in ("x", "w", "grad_y"))
    run = lambda: (lambda s: (CV.conv_backward_data(op, gy, w, x.shape, p, "any", scale=s), CV.conv_backward_weight(op, x, gy, w.shape, p, "any", scale=s),
                              s))(CV.grad_scale(gy, p))
    first = run()                           # (the first call loads the library and allocates the workspaces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.isfinite(second[0]).all() and torch.isfinite(second[1]).all()


# ---- module level ---------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-30, np.sqrt((b ** 2).sum())))


def _np(d):
    return {k: v.detach().double().cpu().numpy() for k, v in d.items()}


def _head_step(head, fp, up, dev, dtype):
    head = head.to(dev).train()
    head.zero_grad()
    f = [t.to(dev, dtype).clone().requires_grad_(True) for t in fp]
    head.aggregate_condition(f).backward(up.to(dev, dtype))
    out = {f"grad_fp{i}": t.grad for i, t in enumerate(f)}
    out.update({"grad:" + k: p.grad for k, p in head.named_parameters() if k.startswith(("conv_lateral.", "conv_up.")) and p.grad is not None})
    return _np(out)


_fpn = {}


def _fpn_case():
    """Inputs, state dict and the default head's gradients in fp64 on the CPU (once)."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    if not _fpn:
        chans = (64, 128, 256, 512)
        torch.manual_seed(0)
        r = dda.DDIMDepthEstimate_Res(in_channels=list(chans), inference_steps=2)
        sd = {k: v.clone() for k, v in r.state_dict().items()}
        B, H, W = 2, 64, 96                                  # pyramid levels 32x48, 16x24, 8x12, 4x6
        fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W, in_channels=chans)]
        up = torch.randn(B, 256, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
        _fpn.update(sd=sd, fp=fp, up=up, ref=_head_step(r.double(), fp, up, "cpu", torch.float64))
    return _fpn


def _count_scaled(fn):
    """fn() with the scaled library calls counted: (result, number of grad_scale calls, number of backward calls that were handed a scale)."""
    from diffusiondepth_amd import conv as CV
    n = {"scale": 0, "calls": 0}
    real_s, real_d, real_w = CV.grad_scale, CV.conv_backward_data, CV.conv_backward_weight

    def counted(real):
        def f(*a, **kw):
            n["calls"] += kw.get("scale") is not None
            return real(*a, **kw)
        return f
    CV.grad_scale = lambda *a: (n.__setitem__("scale", n["scale"] + 1), real_s(*a))[1]
    CV.conv_backward_data, CV.conv_backward_weight = counted(real_d), counted(real_w)
    try:
        return fn(), n["scale"], n["calls"]
    finally:
        CV.grad_scale, CV.conv_backward_data, CV.conv_backward_weight = real_s, real_d, real_w


@pytest.mark.parametrize("prec", SC.F16_MODES)
def test_fpn_in_train_mode_at_a_loss_two_to_the_minus_twenty(prec):
    """The seven convolutions of the Res head's FPN (BatchNorm and ReLU between them, whose backward commutes with a power of two)."""
    import diffusiondepth_amd as dda
    c = _fpn_case()
    head = dda.DDIMDepthEstimate_Res(in_channels=[64, 128, 256, 512], inference_steps=2, precision=prec, conv_backend="hip", conv_grad_autoscale=True)
    head.load_state_dict(c["sd"])
    assert all(m.grad_autoscale for m in head.modules() if type(m).__name__.startswith("HipConv"))
    unit = _head_step(head, c["fp"], c["up"], "cuda", torch.float32)
    tiny, n_scale, n_calls = _count_scaled(lambda: _head_step(head, c["fp"], c["up"] * 2.0 ** -20, "cuda", torch.float32))
    assert n_scale == 7 and n_calls == 14, (n_scale, n_calls)      # one reduction per site, handed to both of its directions
    assert set(tiny) == set(unit) == set(c["ref"]) and sum(k.endswith(".0.weight") for k in unit) == 7
    bad = {k: int((tiny[k] != unit[k] * 2.0 ** -20).sum()) for k in unit if not np.array_equal(tiny[k], unit[k] * 2.0 ** -20)}
    assert not bad, bad
    errs = {k: _rel_l2(tiny[k], c["ref"][k] * 2.0 ** -20) for k in sorted(unit)}
    for k, v in errs.items():
        print(f"fpn {prec} grad_autoscale {k}: relative L2 {v:.3e} (bound {TOL[prec]:.0e})")
    bad = {k: v for k, v in errs.items() if not v <= TOL[prec]}
    assert not bad, bad


def _neck_step(neck, xs, ups):
    neck = neck.cuda().train()
    neck.zero_grad()
    f = [t.cuda().clone().requires_grad_(True) for t in xs]
    torch.autograd.backward(neck(f), [u.cuda() for u in ups])
    res = {f"grad_in{i}": t.grad for i, t in enumerate(f)}
    res.update({"grad:" + k: p.grad for k, p in neck.named_parameters() if p.grad is not None})
    return _np(res)


@pytest.mark.parametrize("prec", SC.F16_MODES)
def test_ragged_neck_in_train_mode_at_a_loss_two_to_the_minus_twenty(prec):
    """Twelve convolutions at MPViT's 216 / 288 (no width a multiple of 64) through ``channels="any"``, the 1x1 included."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import conv as CV
    chans, sizes = [72, 216, 288, 104], ((12, 20), (6, 10), (3, 5), (2, 3))
    torch.manual_seed(11)
    neck = dda.HAHIHeteroNeck(list(chans), list(chans), embedding_dim=72, cross_att=False, self_att=False)
    neck.init_weights()
    neck = CV.convert_hip_conv(neck, prec, True, "any", grad_autoscale=True)
    hip = [m for m in neck.modules() if isinstance(m, (CV.HipConv2d, CV.HipConvTranspose2d))]
    assert len(hip) == 12 and all(m.grad_autoscale and m.channels == "any" for m in hip)
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
    ups = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
    unit = _neck_step(neck, xs, ups)
    tiny, n_scale, n_calls = _count_scaled(lambda: _neck_step(neck, xs, [u * 2.0 ** -20 for u in ups]))
    assert n_scale == 12 and n_calls == 24, (n_scale, n_calls)
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in tiny.values())
    bad = {k: int((tiny[k] != unit[k] * 2.0 ** -20).sum()) for k in unit if not np.array_equal(tiny[k], unit[k] * 2.0 ** -20)}
    assert not bad, bad
