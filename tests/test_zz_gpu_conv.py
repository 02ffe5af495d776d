"""GPU (`-m gpu`): the training convolutions of include/ddepth_conv.h / diffusiondepth_amd.conv on the MI355X.

The exact cases of tests/conv_cases.py must EQUAL the fp64 reference (integer data, and the wide f16x3 data that one f16 MFMA cannot carry); the
real-valued cases stay within the worst-case cap of an fp32 accumulation.  Beyond that: bitwise repeatability, no host synchronisation, and the
head's own path -- a Res and a Swin-width head in .train() with conv_backend="hip" against the same head with default back ends in fp64 on the
CPU, held to the relative L2 bound tests/test_gpu_backward.py asserts for the precision (5e-3 for f16x3, 2e-1 for bf16)."""
import numpy as np
import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu
TOL = {"f16x3": 5e-3, "bf16": 2e-1}      # tests/test_gpu_backward.py: relative L2 per tensor


def _modules(name, prec, kind):
    from diffusiondepth_amd import conv as CV
    op, (B, Cin, Cout, H, W) = CC.SHAPES[name]
    inp = CC.make_inputs(name, kind)
    m = CV.HipConv2d(Cin, Cout, precision=prec) if op == CC.CONV else CV.HipConvTranspose2d(Cin, Cout, precision=prec)
    with torch.no_grad():
        m.weight.copy_(inp["w"])
    return m.cuda().train(), inp


def _run(name, prec, kind):
    from diffusiondepth_amd import conv as CV
    m, inp = _modules(name, prec, kind)
    taken, real = [], CV.conv_forward
    CV.conv_forward = lambda *a: (taken.append(a[0]), real(*a))[1]
    try:
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        y = m(x)
    finally:
        CV.conv_forward = real
    assert taken == [CC.SHAPES[name][0]], "the module did not take the library route"
    y.backward(inp["grad_y"].cuda())
    return {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_w": m.weight.grad.cpu().numpy()}


@pytest.mark.parametrize("case", CC.EXACT + CC.WIDE, ids=CC.case_id)
def test_exact_cases_equal_the_fp64_reference(case):
    name, prec, kind = case
    CC.check_exact(_run(name, prec, kind), name, kind, "gpu")


@pytest.mark.parametrize("case", CC.REAL, ids=CC.case_id)
def test_real_valued_cases_stay_within_the_cap(case):
    import gpu_util
    name, prec, _ = case
    ratios = CC.check_real(_run(name, prec, "normal"), name, prec, "gpu")
    gpu_util.record("conv_real", case=name, prec=prec, **{"ratio_to_usual_bound_" + k: v for k, v in ratios.items()})


@pytest.mark.parametrize("name,prec", [("S4", "bf16"), ("S4", "f16x3"), ("D1", "bf16"), ("D1", "f16x3")])
def test_two_runs_give_the_same_bits(name, prec):
    kind = "normal" if name == "D1" else "int"
    a, b = _run(name, prec, kind), _run(name, prec, kind)
    for k in CC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("name", ["S2", "D1"])
def test_forward_and_backward_do_not_synchronise_the_host(name):
    m, inp = _modules(name, "f16x3", "normal")
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
    m, inp = _modules("S3", "bf16", "int")
    calls = []
    real_d, real_w = CV.conv_backward_data, CV.conv_backward_weight
    CV.conv_backward_data = lambda *a: (calls.append("data"), real_d(*a))[1]
    CV.conv_backward_weight = lambda *a: (calls.append("weight"), real_w(*a))[1]
    try:
        m(inp["x"].cuda()).backward(inp["grad_y"].cuda())                      # detached input
        m.weight.requires_grad_(False)
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x).backward(inp["grad_y"].cuda())                                    # frozen weight
    finally:
        CV.conv_backward_data, CV.conv_backward_weight = real_d, real_w
    assert calls == ["weight", "data"] and x.grad is not None


def test_non_contiguous_half_and_fp32_mode_inputs_take_the_torch_path():
    """No silent copy or conversion: such inputs run torch's convolution and equal nn.Conv2d on the same weight."""
    from diffusiondepth_amd import conv as CV
    torch.manual_seed(0)
    m = CV.HipConv2d(64, 64, precision="bf16").cuda()
    ref = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False).cuda()
    ref.weight = m.weight
    for x in (torch.randn(2, 6, 5, 64, device="cuda").permute(0, 3, 1, 2), ):
        assert torch.equal(m(x), ref(x))
    m.precision = "fp32"
    x = torch.randn(2, 64, 5, 6, device="cuda")
    assert torch.equal(m(x), ref(x))


# ---- head level ---------------------------------------------------------------------------------------------------------------------------
def _head_step(head, fp, up, dev, dtype):
    head = head.to(dev).train()
    head.zero_grad()
    f = [t.to(dev, dtype).clone().requires_grad_(True) for t in fp]
    cond = head.aggregate_condition(f)
    cond.backward(up.to(dev, dtype))
    out = {"cond": cond}
    out.update({f"grad_fp{i}": t.grad for i, t in enumerate(f)})
    out.update({"grad:" + k: p.grad for k, p in head.named_parameters()
                if k.startswith(("conv_lateral.", "conv_up.")) and k.endswith(".0.weight") and p.grad is not None})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def _rel_l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-30, np.sqrt((b ** 2).sum())))


_reference_cache = {}


def _head_case(cls_name, in_channels):
    """Inputs, the default-back-end fp64 CPU reference (computed once per head class) and its state dict."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    if cls_name not in _reference_cache:
        torch.manual_seed(0)
        r = getattr(dda, cls_name)(in_channels=list(in_channels), inference_steps=2)
        sd = {k: v.clone() for k, v in r.state_dict().items()}
        B, H, W = 2, 64, 96                                  # pyramid levels 32x48, 16x24, 8x12, 4x6
        fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W, in_channels=tuple(in_channels))]
        up = torch.randn(B, 256, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
        ref = _head_step(r.double(), fp, up, "cpu", torch.float64)
        _reference_cache[cls_name] = (sd, fp, up, ref)
    return _reference_cache[cls_name]


def _check_head(cls_name, in_channels, prec, bn_backend):
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import conv as CV
    sd, fp, up, ref = _head_case(cls_name, in_channels)
    head = getattr(dda, cls_name)(in_channels=list(in_channels), inference_steps=2, precision=prec, conv_backend="hip", bn_backend=bn_backend)
    head.load_state_dict(sd)
    taken, real = [], CV.conv_forward
    CV.conv_forward = lambda *a: (taken.append(a[0]), real(*a))[1]
    try:
        got = _head_step(head, fp, up, "cuda", torch.float32)
    finally:
        CV.conv_forward = real
    assert sorted(taken) == [0] * 4 + [1] * 3, taken            # the seven FPN sites all ran in the library
    assert set(got) == set(ref) and sum(k.startswith("grad:") for k in ref) == 7
    errs = {k: _rel_l2(got[k], ref[k]) for k in sorted(ref)}
    for k, v in errs.items():
        print(f"head {cls_name} {prec} bn={bn_backend} {k}: relative L2 {v:.3e} (bound {TOL[prec]:.0e})")
    bad = {k: v for k, v in errs.items() if not v <= TOL[prec]}
    assert not bad, bad


@pytest.mark.parametrize("bn_backend", ["torch", "hip"])
@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_res_head_in_train_mode_against_the_default_head_in_fp64(prec, bn_backend):
    _check_head("DDIMDepthEstimate_Res", (64, 128, 256, 512), prec, bn_backend)


def test_swin_width_head_in_train_mode_against_the_default_head_in_fp64():
    _check_head("DDIMDepthEstimate_Swin_ADD", (192, 384, 768, 1536), "f16x3", "torch")
