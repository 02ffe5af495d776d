"""GPU (`-m gpu`): the extended channel range (``channels="any"``, dd_convx_*: multiples of 8 in 8..2048) of diffusiondepth_amd.conv on the MI355X.

The exact cases of tests/conv_ragged_cases.py must EQUAL the fp64 reference, the real-valued ones stay within the worst-case cap of an fp32
accumulation.  Beyond that, without any tolerance: a ragged shape equals the block-64 operator on tensors zero-padded to 128 channels, and a
block-64 shape gives the same bits through both contracts; repeatability; no host synchronisation.  Module level: a small ragged HAHIHeteroNeck,
an MPViT-small-width head and a Swin-L-width head (its 2048 -> 1536 trans_fusion.2 included) with every FPN and neck convolution in the library,
in .train() against the unconverted module in fp64 on the CPU, held to the relative L2 bound tests/test_zz_gpu_conv_neck.py asserts for the
precision (5e-3 for f16x3, 2e-1 for bf16)."""
import numpy as np
import pytest
import torch

import conv_cases as CC
import conv_pw_cases as PC
import conv_ragged_cases as RC

pytestmark = pytest.mark.gpu
TOL = {"f16x3": 5e-3, "bf16": 2e-1}      # tests/test_zz_gpu_conv_neck.py: relative L2 per tensor


def _three(op, inp, prec, channels):
    """The three directions through the functions of diffusiondepth_amd.conv -> dict of KEYS (numpy)."""
    from diffusiondepth_amd import conv as CV
    p = RC.PRECISIONS[prec]
    x, w, gy = (inp[k].cuda() for k in ("x", "w", "grad_y"))
    extra = (channels,) if channels != "block64" else ()
    y = CV.conv_forward(op, x, w, p, *extra)
    gx = CV.conv_backward_data(op, gy, w, x.shape, p, *extra)
    gw = CV.conv_backward_weight(op, x, gy, w.shape, p, *extra)
    return {"y": y.cpu().numpy(), "grad_x": gx.cpu().numpy(), "grad_w": gw.cpu().numpy()}


def _run(name, prec, kind):
    return _three(RC.SHAPES[name][0], RC.make_inputs(name, kind), prec, "any")


@pytest.mark.parametrize("case", RC.EXACT + RC.WIDE, ids=RC.case_id)
def test_exact_cases_equal_the_fp64_reference(case):
    name, prec, kind = case
    RC.check_exact(_run(name, prec, kind), name, kind, "gpu")


@pytest.mark.parametrize("case", RC.REAL, ids=RC.case_id)
def test_real_valued_cases_stay_within_the_cap(case):
    import gpu_util
    name, prec, _ = case
    ratios = RC.check_real(_run(name, prec, "normal"), name, prec, "gpu")
    gpu_util.record("conv_ragged_real", case=name, prec=prec, **{"ratio_to_usual_bound_" + k: v for k, v in ratios.items()})


@pytest.mark.parametrize("prec", list(RC.PRECISIONS))
@pytest.mark.parametrize("name", RC.PADDED)
def test_a_ragged_shape_equals_the_block64_operator_on_zero_padded_tensors(name, prec):
    op, _ = RC.SHAPES[name]
    got = _run(name, prec, "normal")
    _, padded = RC.zero_padded(name)
    want = RC.cut(name, _three(op, padded, prec, "block64"))
    for k in RC.KEYS:
        assert np.isfinite(got[k]).all() and got[k].shape == want[k].shape
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_a_block64_shape_gives_the_same_bits_through_both_contracts(prec):
    cases = [(n,) + CC.SHAPES[n][:1] + (CC.make_inputs(n, "normal"),) for n in ("S1", "D1")] + [("P1", RC.CONV1X1, PC.make_inputs("P1", "normal"))]
    for name, op, inp in cases:
        a, b = _three(op, inp, prec, "any"), _three(op, inp, prec, "block64")
        for k in RC.KEYS:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize("name,prec", [("R2", "bf16"), ("R2", "f16x3"), ("T2", "f16x3"), ("P2", "bf16"), ("R4", "f16x3")])
def test_two_runs_give_the_same_bits(name, prec):
    a, b = _run(name, prec, "normal"), _run(name, prec, "normal")
    for k in RC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _module(name, prec):
    from diffusiondepth_amd import conv as CV
    op, (B, Cin, Cout, H, W) = RC.SHAPES[name]
    inp = RC.make_inputs(name, "normal")
    if op == RC.DECONV:
        m = CV.HipConvTranspose2d(Cin, Cout, precision=prec)
    else:
        m = CV.HipConv2d(Cin, Cout, precision=prec) if op == RC.CONV else CV.HipConv2d(Cin, Cout, 1, 1, 0, precision=prec)
    m.channels = "any"
    with torch.no_grad():
        m.weight.copy_(inp["w"])
    return m.cuda().train(), inp


def _counted(fn):
    """fn() with the operator and the trailing arguments of every library forward call recorded."""
    from diffusiondepth_amd import conv as CV
    taken, real = [], CV.conv_forward
    CV.conv_forward = lambda *a: (taken.append((a[0],) + a[4:]), real(*a))[1]
    try:
        return fn(), taken
    finally:
        CV.conv_forward = real


@pytest.mark.parametrize("name", ["R2", "T2", "P2"])
def test_forward_and_backward_do_not_synchronise_the_host(name):
    m, inp = _module(name, "f16x3")
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    _, taken = _counted(lambda: m(x).backward(gy))      # (the first call loads the library and allocates the workspaces)
    assert taken == [(RC.SHAPES[name][0], "any")], "the module did not take the library's extended route"
    x.grad = None
    m.weight.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = m(x)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(m.weight.grad).all()


def test_a_module_of_the_default_contract_keeps_the_torch_path_at_ragged_widths():
    """``channels`` is opt-in: HipConv2d(216, 256) as made before this contract existed runs torch's convolution."""
    from diffusiondepth_amd import conv as CV
    torch.manual_seed(0)
    m = CV.HipConv2d(216, 256, precision="bf16").cuda()
    x = torch.randn(1, 216, 5, 6, device="cuda")
    y, taken = _counted(lambda: m(x))
    assert taken == [] and torch.equal(y, torch.nn.functional.conv2d(x, m.weight, None, 1, 1))


# ---- the neck and the heads ---------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-30, np.sqrt((b ** 2).sum())))


def _conv_grads(module, prefixes):
    return {"grad:" + k: p.grad for k, p in module.named_parameters() if p.dim() == 4 and p.grad is not None and k.startswith(prefixes)}


def _np(d):
    return {k: v.detach().double().cpu().numpy() for k, v in d.items()}


def _compare(got, ref, prec, label):
    assert set(got) == set(ref), set(got) ^ set(ref)
    errs = {k: _rel_l2(got[k], ref[k]) for k in sorted(ref)}
    for k, v in errs.items():
        print(f"{label} {prec} {k}: relative L2 {v:.3e} (bound {TOL[prec]:.0e})")
    bad = {k: v for k, v in errs.items() if not v <= TOL[prec]}
    assert not bad, bad


SMALL = ([72, 88, 216, 104], ((12, 20), (6, 10), (3, 5), (2, 3)))
_cache = {}


def _neck_step(neck, xs, ups, dev, dtype):
    neck = neck.to(dev).train()
    neck.zero_grad()
    f = [t.to(dev, dtype).clone().requires_grad_(True) for t in xs]
    outs = neck(f)
    torch.autograd.backward(outs, [u.to(dev, dtype) for u in ups])
    res = {f"out{i}": o for i, o in enumerate(outs)}
    res.update({f"grad_in{i}": t.grad for i, t in enumerate(f)})
    res.update(_conv_grads(neck, ("",)))
    return _np(res)


def _small_neck_case():
    import diffusiondepth_amd as dda
    if "neck" not in _cache:
        chans, sizes = SMALL
        torch.manual_seed(11)
        r = dda.HAHIHeteroNeck(list(chans), list(chans), embedding_dim=72, cross_att=False, self_att=False)
        r.init_weights()
        sd = {k: v.clone() for k, v in r.state_dict().items()}
        g = torch.Generator().manual_seed(2)
        xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
        ups = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
        _cache["neck"] = (sd, xs, ups, _neck_step(r.double(), xs, ups, "cpu", torch.float64))
    return _cache["neck"]


@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_small_ragged_neck_in_train_mode_against_the_unconverted_neck_in_fp64(prec):
    """Outputs, input gradients and the weight gradient of all twelve convolutions; no width here is a multiple of 64."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import conv as CV
    sd, xs, ups, ref = _small_neck_case()
    chans, _ = SMALL
    neck = dda.HAHIHeteroNeck(list(chans), list(chans), embedding_dim=72, cross_att=False, self_att=False)
    neck.load_state_dict(sd)
    neck = CV.convert_hip_conv(neck, prec, True, "any")
    got, taken = _counted(lambda: _neck_step(neck, xs, ups, "cuda", torch.float32))
    assert sorted(t[0] for t in taken) == [0] * 4 + [2] * 8 and all(t[1:] == ("any",) for t in taken), taken
    assert sum(k.startswith("grad:") for k in ref) == 12
    _compare(got, ref, prec, "small ragged neck")


def _head_step(head, fp, up, dev, dtype):
    head = head.to(dev).train()
    head.zero_grad()
    f = [t.to(dev, dtype).clone().requires_grad_(True) for t in fp]
    cond = head.aggregate_condition(head.hahineck(f))      # as DDIMDepthEstimate_*HAHI._forward does in .train()
    cond.backward(up.to(dev, dtype))
    res = {"cond": cond}
    res.update({f"grad_fp{i}": t.grad for i, t in enumerate(f)})
    res.update(_conv_grads(head, ("hahineck.", "conv_lateral.", "conv_up.")))
    return _np(res)


# The seed of the heads' initial weights.  The comparison against fp64 is discontinuous where a ReLU input is zero to within the arithmetic's
# error: one such element of a small tensor moves a gradient's relative L2 by ~1 / sqrt(elements), several 1e-3 here.  So the weights are those
# of the FIRST seed for which the reference has no such tie at fp32 precision, measured on the reference alone: PyTorch's own fp32 evaluation of
# the unconverted head on the CPU agrees with its fp64 evaluation to 1.1e-6 on every tensor.  Swin-L widths: seed 0.  MPViT widths: seed 1;
# with seed 0 a pre-activation of lateral_convs.1 (channel 93, one pixel) is such a tie and PyTorch's fp32 itself, CPU or MIOpen, is 6.8e-3 off
# on grad_fp1 and lateral_convs.1's weight gradient (seeds 0..9: 6.8e-3, 1.0e-6, 1.5e-3, 1.2e-3, 2.6e-3, 1.3e-3, 1.1e-6, 1.0e-6, 1.0e-6, 1.0e-6).
@pytest.mark.parametrize("cls_name,chans,seed", [("DDIMDepthEstimate_MPVIT_ADDHAHI", (128, 216, 288, 288), 1),
                                                 ("DDIMDepthEstimate_Swin_ADDHAHI", (192, 384, 768, 1536), 0)], ids=["mpvit_small", "swin_l"])
def test_head_with_every_fpn_and_neck_convolution_in_the_library_against_the_default_head_in_fp64(cls_name, chans, seed):
    """"hip+all": four laterals, three transposed, and the neck's four 3x3 and eight 1x1 -- for Swin-L the eighth 3x3 is trans_fusion.2,
    2048 -> 1536 at 4 x 6 pixels."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    torch.manual_seed(seed)
    r = getattr(dda, cls_name)(in_channels=list(chans), inference_steps=2)
    sd = {k: v.clone() for k, v in r.state_dict().items()}
    B, H, W = 2, 64, 96                                  # pyramid levels 32x48, 16x24, 8x12, 4x6
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W, in_channels=chans)]
    up = torch.randn(B, 256, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
    ref = _head_step(r.double(), fp, up, "cpu", torch.float64)
    head = getattr(dda, cls_name)(in_channels=list(chans), inference_steps=2, precision="f16x3", conv_backend="hip+all")
    head.load_state_dict(sd)
    got, taken = _counted(lambda: _head_step(head, fp, up, "cuda", torch.float32))
    assert sorted(t[0] for t in taken) == [0] * 8 + [1] * 3 + [2] * 8 and all(t[1:] == ("any",) for t in taken), taken
    assert sum(k.startswith("grad:") for k in ref) == 19
    _compare(got, ref, "f16x3", cls_name)
