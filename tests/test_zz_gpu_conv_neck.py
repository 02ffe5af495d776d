"""GPU (`-m gpu`): the pointwise (1x1) operator of include/ddepth_conv.h through diffusiondepth_amd.conv.HipConv2d, and the HAHI neck trained on it.

The exact cases of tests/conv_pw_cases.py must EQUAL the fp64 reference (integer data, and the wide f16x3 data that one f16 MFMA cannot carry);
the real-valued cases stay within the worst-case cap of an fp32 accumulation.  Beyond that: bitwise repeatability, no host synchronisation,
skipped gradients, and the neck's own path -- a small HAHIHeteroNeck converted with pointwise=True, and a Swin-L-width Swin_ADDHAHI head with
conv_backend="hip+neck", both in .train() against the unconverted module in fp64 on the CPU, held to the relative L2 bound
tests/test_gpu_backward.py and tests/test_zz_gpu_conv.py assert for the precision (5e-3 for f16x3, 2e-1 for bf16)."""
import numpy as np
import pytest
import torch

import conv_pw_cases as PC

pytestmark = pytest.mark.gpu
TOL = {"f16x3": 5e-3, "bf16": 2e-1}      # tests/test_gpu_backward.py: relative L2 per tensor


def _module(name, prec, kind):
    from diffusiondepth_amd import conv as CV
    B, Cin, Cout, H, W = PC.SHAPES[name]
    inp = PC.make_inputs(name, kind)
    m = CV.HipConv2d(Cin, Cout, 1, 1, 0, precision=prec)
    with torch.no_grad():
        m.weight.copy_(inp["w"])
    return m.cuda().train(), inp


def _run(name, prec, kind):
    from diffusiondepth_amd import conv as CV
    m, inp = _module(name, prec, kind)
    taken, real = [], CV.conv_forward
    CV.conv_forward = lambda *a: (taken.append(a[0]), real(*a))[1]
    try:
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        y = m(x)
    finally:
        CV.conv_forward = real
    assert taken == [PC.CONV1X1], "the module did not take the library's pointwise route"
    y.backward(inp["grad_y"].cuda())
    return {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_w": m.weight.grad.cpu().numpy()}


@pytest.mark.parametrize("case", PC.EXACT + PC.WIDE, ids=PC.case_id)
def test_exact_cases_equal_the_fp64_reference(case):
    name, prec, kind = case
    PC.check_exact(_run(name, prec, kind), name, kind, "gpu")


@pytest.mark.parametrize("case", PC.REAL, ids=PC.case_id)
def test_real_valued_cases_stay_within_the_cap(case):
    import gpu_util
    name, prec, _ = case
    ratios = PC.check_real(_run(name, prec, "normal"), name, prec, "gpu")
    gpu_util.record("conv_pw_real", case=name, prec=prec, **{"ratio_to_usual_bound_" + k: v for k, v in ratios.items()})


@pytest.mark.parametrize("name,prec", [("P4", "bf16"), ("P4", "f16x3"), ("P2", "bf16"), ("P2", "f16x3")])
def test_two_runs_give_the_same_bits(name, prec):
    kind = "normal" if name == "P2" else "int"
    a, b = _run(name, prec, kind), _run(name, prec, kind)
    for k in PC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_forward_and_backward_do_not_synchronise_the_host():
    m, inp = _module("P2", "f16x3", "normal")
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    m(x).backward(gy)                       # (the first call loads the library and allocates the workspaces)
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


def test_a_detached_input_and_a_frozen_weight_skip_their_gradient():
    from diffusiondepth_amd import conv as CV
    m, inp = _module("P3", "bf16", "int")
    calls = []
    real_d, real_w = CV.conv_backward_data, CV.conv_backward_weight
    CV.conv_backward_data = lambda *a: (calls.append(("data", a[0])), real_d(*a))[1]
    CV.conv_backward_weight = lambda *a: (calls.append(("weight", a[0])), real_w(*a))[1]
    try:
        m(inp["x"].cuda()).backward(inp["grad_y"].cuda())                      # detached input
        m.weight.requires_grad_(False)
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x).backward(inp["grad_y"].cuda())                                    # frozen weight
    finally:
        CV.conv_backward_data, CV.conv_backward_weight = real_d, real_w
    assert calls == [("weight", PC.CONV1X1), ("data", PC.CONV1X1)] and x.grad is not None


# ---- the neck -----------------------------------------------------------------------------------------------------------------------------------
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


def _counted(fn):
    """fn() with the operator of every library forward call recorded."""
    from diffusiondepth_amd import conv as CV
    taken, real = [], CV.conv_forward
    CV.conv_forward = lambda *a: (taken.append(a[0]), real(*a))[1]
    try:
        return fn(), taken
    finally:
        CV.conv_forward = real


SMALL = ([64, 128, 192, 256], ((12, 20), (6, 10), (3, 5), (2, 3)))
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
        r = dda.HAHIHeteroNeck(list(chans), list(chans), embedding_dim=64, cross_att=False, self_att=False)
        r.init_weights()
        sd = {k: v.clone() for k, v in r.state_dict().items()}
        g = torch.Generator().manual_seed(2)
        xs = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
        ups = [torch.randn(2, c, h, w, generator=g) for c, (h, w) in zip(chans, sizes)]
        _cache["neck"] = (sd, xs, ups, _neck_step(r.double(), xs, ups, "cpu", torch.float64))
    return _cache["neck"]


@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_small_neck_in_train_mode_against_the_unconverted_neck_in_fp64(prec):
    """Outputs, input gradients and the weight gradient of every convolution (twelve here: at these widths trans_fusion.2 is supported too)."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import conv as CV
    sd, xs, ups, ref = _small_neck_case()
    chans, _ = SMALL
    neck = dda.HAHIHeteroNeck(list(chans), list(chans), embedding_dim=64, cross_att=False, self_att=False)
    neck.load_state_dict(sd)
    neck = CV.convert_hip_conv(neck, prec, pointwise=True)
    got, taken = _counted(lambda: _neck_step(neck, xs, ups, "cuda", torch.float32))
    assert sorted(taken) == [0] * 4 + [2] * 8, taken
    assert sum(k.startswith("grad:") for k in ref) == 12
    _compare(got, ref, prec, "small neck")


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


def test_swin_l_width_head_with_the_neck_in_train_mode_against_the_default_head_in_fp64():
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    chans = (192, 384, 768, 1536)
    torch.manual_seed(0)
    r = dda.DDIMDepthEstimate_Swin_ADDHAHI(in_channels=list(chans), inference_steps=2)
    sd = {k: v.clone() for k, v in r.state_dict().items()}
    B, H, W = 2, 64, 96                                  # pyramid levels 32x48, 16x24, 8x12, 4x6
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W, in_channels=chans)]
    up = torch.randn(B, 256, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
    ref = _head_step(r.double(), fp, up, "cpu", torch.float64)
    head = dda.DDIMDepthEstimate_Swin_ADDHAHI(in_channels=list(chans), inference_steps=2, precision="f16x3", conv_backend="hip+neck")
    head.load_state_dict(sd)
    got, taken = _counted(lambda: _head_step(head, fp, up, "cuda", torch.float32))
    assert sorted(taken) == [0] * 7 + [1] * 3 + [2] * 8, taken      # FPN: four 3x3, three transposed; neck: three 3x3 (trans_fusion.2 stays torch), eight 1x1
    assert sum(k.startswith("grad:") for k in ref) == 19
    _compare(got, ref, "f16x3", "Swin_ADDHAHI head")
