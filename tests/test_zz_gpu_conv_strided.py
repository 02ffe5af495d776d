"""GPU (`-m gpu`): the 3x3 stride-2 operator of include/ddepth_conv_strided.h / diffusiondepth_amd.conv on the MI355X.

The exact cases of tests/conv_strided_cases.py must EQUAL the fp64 reference through ``HipConv2d`` (integer data, and the wide f16x3 data that one
f16 MFMA cannot carry), with and without a bias; the real-valued cases stay within the worst-case cap of an fp32 accumulation; the scaled
gradients follow the rules of tests/conv_scaled_cases.py with the scale pair built in numpy.  Beyond that: bitwise repeatability, the zero-padding
identities, no host synchronisation, skipped gradients, the torch path of foreign inputs, and the network case N1 (a two-stage ResNetForMMBEV in
.train() against the unconverted net in fp64 on the CPU, relative L2 per gradient tensor and feature map: f16x3 <= 5e-3, bf16 <= 2e-1)."""
import numpy as np
import pytest
import torch

import conv_strided_cases as ZC

pytestmark = pytest.mark.gpu


def _module(name, prec, kind, bias, inp=None, dims=None):
    from diffusiondepth_amd import conv as CV
    B, Cin, Cout, H, W = dims or ZC.SHAPES[name]
    inp = inp or ZC.make_inputs(name, kind)
    m = CV.HipConv2d(Cin, Cout, 3, 2, 1, bias=bias, precision=prec)
    m.strided, m.channels = True, "any"
    with torch.no_grad():
        m.weight.copy_(inp["w"])
        if bias:
            m.bias.copy_(inp["bias"])
    return m.cuda().train(), inp


def _run(name, prec, kind, bias=True, inp=None, dims=None):
    """Forward and backward through the module -> dict of ZC.KEYS (grad_bias None without a bias)."""
    from diffusiondepth_amd import conv as CV
    m, inp = _module(name, prec, kind, bias, inp, dims)
    taken, real = [], CV.conv_s2_forward
    CV.conv_s2_forward = lambda *a: (taken.append(1), real(*a))[1]
    try:
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        y = m(x)
    finally:
        CV.conv_s2_forward = real
    assert taken == [1], "the module did not take the library route"
    y.backward(inp["grad_y"].cuda())
    return {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_w": m.weight.grad.cpu().numpy(),
            "grad_bias": m.bias.grad.cpu().numpy() if bias else None}


def _run_scaled(name, prec, kind, grad_y):
    """The two gradients (bias included) through the functions on `grad_y` (numpy) with the scale pair of the rule, built in numpy."""
    from diffusiondepth_amd import conv as CV
    inp = ZC.make_inputs(name, kind)
    p = ZC.PRECISIONS[prec]
    x, w, gy = inp["x"].cuda(), inp["w"].cuda(), torch.from_numpy(grad_y).cuda()
    scale = torch.from_numpy(ZC.scale_words(grad_y).view(np.float32).copy()).cuda()
    gx = CV.conv_s2_backward_data(gy, w, x.shape, p, scale=scale)
    gw, gb = CV.conv_s2_backward_weight(x, gy, w.shape, p, with_bias=True, scale=scale)
    return {"grad_x": gx.cpu().numpy(), "grad_w": gw.cpu().numpy(), "grad_bias": gb.cpu().numpy()}


@pytest.mark.parametrize("bias", ZC.BIAS, ids=["bias", "nobias"])
@pytest.mark.parametrize("case", ZC.EXACT + ZC.WIDE, ids=ZC.case_id)
def test_exact_cases_equal_the_fp64_reference(case, bias):
    name, prec, kind = case
    ZC.check_exact(_run(name, prec, kind, bias), name, kind, bias, "gpu")


@pytest.mark.parametrize("bias", ZC.BIAS, ids=["bias", "nobias"])
@pytest.mark.parametrize("case", ZC.REAL, ids=ZC.case_id)
def test_real_valued_cases_stay_within_the_cap(case, bias):
    import gpu_util
    name, prec, _ = case
    ratios = ZC.check_real(_run(name, prec, "normal", bias), name, prec, bias, "gpu")
    gpu_util.record("conv_strided_real", case=name, prec=prec, bias=bias, **{"err_over_tol_" + k: v for k, v in ratios.items()})


@pytest.mark.parametrize("prec", ["f16", "f16x3"])
@pytest.mark.parametrize("name", ZC.EQUIVARIANCE)
def test_scaled_gradients_are_equivariant_under_powers_of_two(name, prec):
    gy = ZC.make_inputs(name, "normal")["grad_y"].numpy()
    base = _run_scaled(name, prec, "normal", gy)
    bad = []
    for k in ZC.K_SMALL:
        bad += [(k,) + b for b in ZC.check_equivariant(_run_scaled(name, prec, "normal", ZC.small(gy, k)), base, k, f"gpu {name} {prec}")]
    assert not bad, bad


@pytest.mark.parametrize("prec", list(ZC.PRECISIONS))
@pytest.mark.parametrize("name", ZC.SCALED_EXACT)
def test_scaled_integer_gradients_times_two_to_the_minus_20_are_exact(name, prec):
    gy = ZC.small(ZC.make_inputs(name, "int")["grad_y"].numpy(), -20)
    ZC.check_exact(_run_scaled(name, prec, "int", gy), name, "int", True, "gpu scaled", scale_exp=-20)


@pytest.mark.parametrize("prec", ["f16", "f16x3"])
def test_grad_autoscale_on_the_module_is_the_scaled_call(prec):
    """One grad_scale per backward, handed to both gradients: the module's result equals the functions' with the numpy rule's pair."""
    from diffusiondepth_amd import conv as CV
    inp = ZC.make_inputs("Z6", "normal")
    gy = ZC.small(inp["grad_y"].numpy(), -20)
    m, _ = _module("Z6", prec, "normal", True)
    m.grad_autoscale = True
    scales, real = [], CV.grad_scale
    CV.grad_scale = lambda *a: (scales.append(1), real(*a))[1]
    try:
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x).backward(torch.from_numpy(gy).cuda())
    finally:
        CV.grad_scale = real
    assert scales == [1]
    want = _run_scaled("Z6", prec, "normal", gy)
    got = {"grad_x": x.grad, "grad_w": m.weight.grad, "grad_bias": m.bias.grad}
    for k in ZC.GRAD_KEYS:
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k


@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_two_runs_give_the_same_bits(prec):
    a, b = _run("Z7", prec, "normal"), _run("Z7", prec, "normal")
    for k in ZC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _same(got, want):
    for k in ZC.KEYS:
        assert np.isfinite(got[k]).all() and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("prec", list(ZC.PRECISIONS))
def test_the_zero_padding_identities(prec):
    """A block-64 shape equals itself zero-padded by 64 channels; a ragged shape equals the block-64 instantiation on zero-padded tensors."""
    up = lambda n: -(-n // 64) * 64
    for name, grow in ((ZC.PAD64, 64), (ZC.PAD_RAGGED, 0)):
        B, Cin, Cout, H, W = ZC.SHAPES[name]
        dims, padded = ZC.zero_padded(name, up(Cin) + grow, up(Cout) + grow)
        _same(_run(name, prec, "normal"), ZC.cut(name, _run(name, prec, "normal", inp=padded, dims=dims)))


@pytest.mark.parametrize("name", ["Z2", "Z5"])
def test_forward_and_backward_do_not_synchronise_the_host(name):
    m, inp = _module(name, "f16x3", "normal", True)
    m.grad_autoscale = True
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    m(x).backward(gy)                       # (the first call loads the library and allocates the workspaces)
    x.grad = m.weight.grad = m.bias.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = m(x)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(t).all() for t in (y, x.grad, m.weight.grad, m.bias.grad))


def test_a_detached_input_a_frozen_weight_and_a_frozen_bias_skip_their_gradient():
    from diffusiondepth_amd import conv as CV
    m, inp = _module("Z3", "bf16", "int", True)
    calls = []
    real_d, real_w = CV.conv_s2_backward_data, CV.conv_s2_backward_weight
    CV.conv_s2_backward_data = lambda *a, **k: (calls.append("data"), real_d(*a, **k))[1]
    CV.conv_s2_backward_weight = lambda *a, **k: (calls.append("weight+bias" if k.get("with_bias") else "weight"), real_w(*a, **k))[1]
    try:
        m(inp["x"].cuda()).backward(inp["grad_y"].cuda())                      # detached input (the RGB image of a backbone)
        m.bias.requires_grad_(False)
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x).backward(inp["grad_y"].cuda())                                    # frozen bias
        m.weight.requires_grad_(False)
        x2 = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x2).backward(inp["grad_y"].cuda())                                   # frozen weight and bias
    finally:
        CV.conv_s2_backward_data, CV.conv_s2_backward_weight = real_d, real_w
    assert calls == ["weight+bias", "data", "weight", "data"] and x.grad is not None and x2.grad is not None


def test_non_contiguous_half_and_fp32_mode_inputs_take_the_torch_path():
    """No silent copy or conversion: such inputs run torch's convolution and equal nn.Conv2d on the same parameters."""
    from diffusiondepth_amd import conv as CV
    torch.manual_seed(0)
    m = CV.HipConv2d(64, 64, 3, 2, 1, bias=True, precision="bf16").cuda()
    m.strided = True
    ref = torch.nn.Conv2d(64, 64, 3, 2, 1, bias=True).cuda()
    ref.weight, ref.bias = m.weight, m.bias
    taken, real = [], CV.conv_s2_forward
    CV.conv_s2_forward = lambda *a: (taken.append(1), real(*a))[1]
    try:
        x = torch.randn(2, 6, 5, 64, device="cuda").permute(0, 3, 1, 2)
        assert torch.equal(m(x), ref(x))
        xh = torch.randn(2, 64, 5, 6, device="cuda").half()
        assert torch.equal(m.half()(xh), ref(xh))
        m.float()
        m.precision = "fp32"
        x = torch.randn(2, 64, 5, 6, device="cuda")
        assert torch.equal(m(x), ref(x))
        m.precision, m.strided = "bf16", False      # not marked: the torch path as well
        assert torch.equal(m(x), ref(x))
        assert taken == []
        m.strided = True
        m(x)
        assert taken == [1]
    finally:
        CV.conv_s2_forward = real


# ---- the network case N1 ------------------------------------------------------------------------------------------------------------------------
def _n1_gpu(prec, bn_hip):
    """N1 converted and run on the GPU -> (n1_run result, library calls seen)."""
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd.batchnorm import convert_hip_batchnorm
    net = CV.convert_hip_conv(ZC.n1_net(), prec, channels="any", strided=True)
    if bn_hip:
        net = convert_hip_batchnorm(net)
    net = net.cuda().train()
    x, ups = ZC.n1_data()
    seen, real_s2, real_s1 = [], CV.conv_s2_forward, CV.conv_forward
    CV.conv_s2_forward = lambda *a: (seen.append("s2"), real_s2(*a))[1]
    CV.conv_forward = lambda *a: (seen.append("s1"), real_s1(*a))[1]
    try:
        result = ZC.n1_run(net, x.cuda(), [u.cuda() for u in ups])
    finally:
        CV.conv_s2_forward, CV.conv_forward = real_s2, real_s1
    return result, seen


@pytest.mark.parametrize("bn_hip", [False, True], ids=["bn-torch", "bn-hip"])
@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_n1_against_the_unconverted_net_in_fp64(prec, bn_hip):
    result, seen = _n1_gpu(prec, bn_hip)
    assert sorted(seen) == ["s1"] * 2 + ["s2"] * 4, seen            # all six convolutions ran in the library
    grads, feats = ZC.n1_errors(result)
    assert len(grads) == 16 and len(feats) == 2
    for k, v in list(grads.items()) + [(f"feature{i}", v) for i, v in enumerate(feats)]:
        print(f"N1 {prec} bn_hip={bn_hip} {k}: relative L2 {v:.3e} (bound {ZC.N1_BOUNDS[prec]:.0e})")
    bad = {k: v for k, v in list(grads.items()) + [(f"feature{i}", v) for i, v in enumerate(feats)] if not v <= ZC.N1_BOUNDS[prec]}
    assert not bad, bad


def test_n1_in_f16_is_recorded():
    import gpu_util
    result, seen = _n1_gpu("f16", False)
    assert sorted(seen) == ["s1"] * 2 + ["s2"] * 4, seen
    grads, feats = ZC.n1_errors(result)
    gpu_util.record("conv_strided_n1_f16", worst_gradient=max(grads.values()), worst_feature=max(feats))
    assert all(np.isfinite(v) for v in list(grads.values()) + feats)


def test_res18_with_the_hip_backbone_runs_every_convolution_in_the_library():
    """No whole-backbone gradient bound (ReLU-mask flips and small-norm BatchNorm tensors; tests/conv_strided_cases.py): the module census, finite
    outputs and gradients, and the feature shapes.  The errors against the unconverted backbone in fp64 are recorded."""
    import copy

    import gpu_util
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd import model as M
    torch.manual_seed(0)
    model = M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, precision="bf16", backbone_backend="hip"))
    bb = model.depth_backbone
    convs = [m for m in bb.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 20 and all(isinstance(m, CV.HipConv2d) for m in convs) and sum(m.strided for m in convs) == 8
    ref_net = copy.deepcopy(bb).double().train()      # (on the CPU the converted modules are the torch ones)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 64, 96, generator=g)
    ups = [torch.randn(2, c, 64 >> (i + 1), 96 >> (i + 1), generator=g) for i, c in enumerate((64, 128, 256, 512))]
    ref = ZC.n1_run(ref_net, x.double(), [u.double() for u in ups])
    seen, real_s2, real_s1 = [], CV.conv_s2_forward, CV.conv_forward
    CV.conv_s2_forward = lambda *a: (seen.append("s2"), real_s2(*a))[1]
    CV.conv_forward = lambda *a: (seen.append("s1"), real_s1(*a))[1]
    try:
        got = ZC.n1_run(bb.cuda().train(), x.cuda(), [u.cuda() for u in ups])
    finally:
        CV.conv_s2_forward, CV.conv_forward = real_s2, real_s1
    assert sorted(seen) == ["s1"] * 12 + ["s2"] * 8
    assert [f.shape for f in got[0]] == [tuple(u.shape) for u in ups]
    assert all(np.isfinite(f).all() for f in got[0]) and all(np.isfinite(v).all() for v in got[1].values())
    assert set(got[1]) == set(ref[1])
    grads, feats = ZC.n1_errors(got, ref)
    gpu_util.record("conv_strided_res18_bf16", worst_gradient=max(grads.values()), worst_feature=max(feats))
