"""GPU (`-m gpu`): the latent codec's training convolutions and decoder tail of include/ddepth_codec.h / diffusiondepth_amd.codec on the MI355X.

The exact cases of tests/codec_cases.py must EQUAL the fp64 reference; the real-valued cases stay within the worst-case cap of an fp32
accumulation; the tail within its ulp bound, and bit for bit what dd_decode's last stage computes.  Beyond that: bitwise repeatability, no host
synchronisation, and the codec's own path -- the whole codec in .train() and a Res head with codec_backend="hip" -- against the same module in
fp64 on the CPU, held per tensor to a relative L2 error of at most 4 x that of the unconverted fp32 module on the same device (floor 1e-6): the
two fp32 paths sum in different orders and BatchNorm's batch statistics sit between the layers.

One deviation from that rule, for one tensor: the gradient of ``conv_inv_transform.0.bias``.  The transpose convolution's bias sits in front of
batch-statistics BatchNorm, so its exact gradient is ZERO (the test asserts that the fp64 reference is zero at fp32 resolution) and a relative error
against it is rounding noise over rounding noise.  Its error is taken relative to the fp64 sum of |grad_y| per channel instead, same margin and
floor.  That is a weak check (an absolute error of about 4e-6 x 7e3 would pass); what holds DEC0's bias gradient to account are the exact and
real-valued ``grad_bias`` cases of T1 .. T5 above, where grad_y is arbitrary."""
import numpy as np
import pytest
import torch

import codec_cases as CC

pytestmark = pytest.mark.gpu
MARGIN, FLOOR = 4.0, 1e-6


def _module(name, kind):
    from diffusiondepth_amd import codec as CD
    op = CC.SHAPES[name][0]
    inp = CC.make_inputs(name, kind)
    cin, cout, k, s, p, bias, transposed = CD.GEOMETRY[op]
    m = CD.HipCodecConvTranspose2d(cin, cout, k, s, p) if transposed else CD.HipCodecConv2d(cin, cout, k, s, p, bias=bias)
    with torch.no_grad():
        m.weight.copy_(inp["w"])
        if bias:
            m.bias.copy_(inp["bias"])
    return m.cuda().train(), inp


def _run(name, kind):
    from diffusiondepth_amd import codec as CD
    m, inp = _module(name, kind)
    taken, real = [], CD.conv_forward
    CD.conv_forward = lambda *a: (taken.append(a[0]), real(*a))[1]
    try:
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        y = m(x)
    finally:
        CD.conv_forward = real
    assert taken == [CC.SHAPES[name][0]], "the module did not take the library route"
    y.backward(inp["grad_y"].cuda())
    out = {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_w": m.weight.grad.cpu().numpy()}
    if m.bias is not None:
        out["grad_bias"] = m.bias.grad.cpu().numpy()
    return out


@pytest.mark.parametrize("case", CC.EXACT, ids=CC.case_id)
def test_exact_cases_equal_the_fp64_reference(case):
    name, kind = case
    CC.check_exact(_run(name, kind), name, kind, "gpu")


@pytest.mark.parametrize("case", CC.REAL, ids=CC.case_id)
def test_real_valued_cases_stay_within_the_cap(case):
    import gpu_util
    name, _ = case
    ratios = CC.check_real(_run(name, "normal"), name, "gpu")
    gpu_util.record("codec_real", case=name, **{"ratio_to_usual_bound_" + k: v for k, v in ratios.items()})


@pytest.mark.parametrize("name", ["T4-enc0", "T4-enc1", "T4-dec0", "T4-dec1"])
def test_two_runs_give_the_same_bits(name):
    a, b = _run(name, "normal"), _run(name, "normal")
    for k in CC.keys_of(name):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _tail(z, gd):
    from diffusiondepth_amd import codec as CD
    tail = CD.HipCodecTail(CC.EPS)
    z = z.detach().clone().cuda().requires_grad_(True)
    assert tail.returns_depth(z)
    depth = tail(z)
    depth.backward(gd.cuda())
    return depth.detach().cpu().numpy(), z.grad.cpu().numpy()


def test_the_tail_forward_and_backward():
    z, gd = CC.tail_inputs()
    depth, gz = _tail(z, gd)
    CC.check_tail(depth, gz, "gpu")
    again = _tail(z, gd)
    assert np.array_equal(depth.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(gz.view(np.uint32), again[1].view(np.uint32))


def test_the_tail_forward_is_the_eval_decoders_tail_bit_for_bit():
    """dd_decode against the fused tail on the same z.  The decoder is given weights that make z EXACT in any order of summation, so that the torch
    layers in front of the tail and the fused eval kernel hold the same z: BatchNorm weight 0 (the mid tensor is relu(beta_c), small integers), the
    last convolution's weights multiples of 1/128 and its bias a multiple of 1/4.  z differs at the borders (4, 6 or 9 live taps) and with the bias."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import codec as CD
    dt = dda.DeepDepthTransformWithUpsampling().cuda().eval()
    g = torch.Generator().manual_seed(77)
    dec = dt.conv_inv_transform
    lat = torch.randn(2, 16, 9, 13, generator=g).cuda()
    tail = CD.HipCodecTail(dt.eps)
    seen = set()
    for b1 in (-20.0, -14.5, -3.25, 0.0, 2.5, 14.0):
        with torch.no_grad():
            dec[1].weight.zero_()
            dec[1].bias.copy_(torch.randint(0, 4, (16,), generator=g).float())
            dec[3][0].weight.copy_(torch.randint(-8, 9, (1, 16, 3, 3), generator=g).float() / 8 / 16)
            dec[3][0].bias.fill_(b1)
            z = lat
            for layer in list(dec)[:-1]:
                z = layer(z)
            z = z.contiguous()
            want = dt.inv_t(lat)                      # eval, no grad: dd_decode
            got = tail(z)
        assert torch.equal((z * 128).round(), z * 128), "z is not exact"
        seen.update(z.unique().tolist())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), b1
    assert len(seen) >= 12


@pytest.mark.parametrize("name", ["T2-enc0", "T2-enc1", "T2-dec0", "T2-dec1"])
def test_forward_and_backward_do_not_synchronise_the_host(name):
    from diffusiondepth_amd import codec as CD
    m, inp = _module(name, "normal")
    tail = CD.HipCodecTail(CC.EPS)
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    tail(m(x)).backward(gy)                 # (the first call loads the library and allocates the workspaces)
    x.grad = None
    m.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = tail(m(x))
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_a_detached_input_and_frozen_parameters_skip_their_gradient():
    from diffusiondepth_amd import codec as CD
    m, inp = _module("T1-dec0", "int")
    calls = []
    real_d, real_w = CD.conv_backward_data, CD.conv_backward_weight
    CD.conv_backward_data = lambda *a, **k: (calls.append("data"), real_d(*a, **k))[1]
    CD.conv_backward_weight = lambda *a, **k: (calls.append("weight"), real_w(*a, **k))[1]
    try:
        m(inp["x"].cuda()).backward(inp["grad_y"].cuda())                      # detached input
        m.weight.requires_grad_(False)
        m.bias.requires_grad_(False)
        x = inp["x"].detach().clone().cuda().requires_grad_(True)
        m(x).backward(inp["grad_y"].cuda())                                    # frozen parameters
    finally:
        CD.conv_backward_data, CD.conv_backward_weight = real_d, real_w
    assert calls == ["weight", "data"] and x.grad is not None


def test_non_contiguous_and_half_inputs_take_the_torch_path():
    """No silent copy or conversion: such inputs run torch's convolution / sigmoid and equal the torch module on the same parameters."""
    from diffusiondepth_amd import codec as CD
    torch.manual_seed(0)
    m = CD.HipCodecConv2d(16, 16, 3, 1, 1, bias=False).cuda()
    ref = torch.nn.Conv2d(16, 16, 3, 1, 1, bias=False).cuda()
    ref.weight = m.weight
    x = torch.randn(2, 6, 5, 16, device="cuda").permute(0, 3, 1, 2)
    assert torch.equal(m(x), ref(x))
    tail = CD.HipCodecTail(1e-6)
    assert torch.equal(tail(x), torch.sigmoid(x))
    h = torch.randn(2, 16, 5, 6, device="cuda").half()
    assert torch.equal(tail(h), torch.sigmoid(h))


# ---- the whole codec ------------------------------------------------------------------------------------------------------------------------
def _held_to_the_rule(got, base, ref, label, ref_base=None):
    """Per tensor: relative L2 error of `got` against the fp64 `ref` <= 4 x max(that of the unconverted fp32 `base` (against `ref_base`, where the
    two runs have references of their own), 1e-6)."""
    bad = {}
    ref_base = ref if ref_base is None else ref_base
    for k in sorted(ref):
        if k.startswith("scale:"):
            continue
        if "scale:" + k in ref:
            # a gradient that is zero in exact arithmetic (codec_cases.whole_codec_step): a relative error against rounding noise means nothing, so
            # both errors are taken relative to the tensor's scale, the fp64 sum of |grad_y|; margin and floor as for every other tensor
            scale = float(np.sqrt((ref["scale:" + k] ** 2).sum()))
            assert float(np.sqrt((ref[k] ** 2).sum())) <= CC.ULP * scale, "the reference is not zero at fp32 resolution"
            e_got = float(np.sqrt(((got[k] - ref[k]) ** 2).sum())) / scale
            e_base = float(np.sqrt(((base[k] - ref_base[k]) ** 2).sum())) / scale
        else:
            e_got, e_base = CC.rel_l2(got[k], ref[k]), CC.rel_l2(base[k], ref_base[k])
        print(f"{label} {k}: relative L2 error hip {e_got:.3e}, torch fp32 {e_base:.3e}")
        if not (np.isfinite(got[k]).all() and e_got <= MARGIN * max(e_base, FLOOR)):
            bad[k] = (e_got, e_base)
    assert not bad, bad


@pytest.mark.parametrize("bn_backend", ["torch", "hip"])
def test_the_whole_codec_in_train_mode_against_fp64(bn_backend):
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import batchnorm as BN
    from diffusiondepth_amd import codec as CD
    plain = CC.init_codec(dda.DeepDepthTransformWithUpsampling())
    sd = {k: v.clone() for k, v in plain.state_dict().items()}
    ref = CC.whole_codec_step(CC.init_codec(dda.DeepDepthTransformWithUpsampling()).double(), "cpu", torch.float64)
    assert 0.5 <= ref["inv_t(latent)"].min() and ref["inv_t(latent)"].max() <= 80.0
    base = CC.whole_codec_step(plain, "cuda", torch.float32)
    conv = dda.DeepDepthTransformWithUpsampling()
    conv.load_state_dict(sd)
    CD.convert_hip_codec(conv)
    if bn_backend == "hip":
        BN.convert_hip_batchnorm(conv)
    taken, real_c, real_t = [], CD.conv_forward, CD.tail_forward
    CD.conv_forward = lambda *a: (taken.append(a[0]), real_c(*a))[1]
    CD.tail_forward = lambda *a: (taken.append("tail"), real_t(*a))[1]
    try:
        got = CC.whole_codec_step(conv, "cuda", torch.float32)
    finally:
        CD.conv_forward, CD.tail_forward = real_c, real_t
    assert taken == [0, 1, 2, 3, "tail"], taken            # the four sites and the tail all ran in the library
    assert set(got) == set(ref) and sum(k.startswith("grad:") for k in ref) == len(list(plain.parameters())) == 12
    assert sorted(k for k in ref if k.startswith("scale:")) == ["scale:" + CC.ZERO_GRADIENT]
    _held_to_the_rule(got, base, ref, f"codec bn={bn_backend}")


def test_res_head_in_train_mode_with_the_hip_codec():
    """One training step of a small Res head with codec_backend="hip" against the default head from the same seed.  The denoiser is the same
    library call in both, so the latent the decoder receives is the same tensor and `ddim_loss` (which never meets the codec) the same number;
    `pred` is held to the rule above, the fp64 reference of either head being the same codec evaluated in fp64 on the CPU on the latent that head's
    decoder received."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import codec as CD
    from diffusiondepth_amd import synth
    B, H, W = 2, 32, 64
    fp = [torch.from_numpy(f).cuda() for f in synth.make_backbone_features(3, B, H, W)]
    gt = torch.from_numpy(synth.make_gt_depth(4, B, H, W)).cuda()
    torch.manual_seed(0)
    first = dda.DDIMDepthEstimate_Res(inference_steps=2, codec_backend="torch")
    CC.init_codec(first.depth_transform)
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    res, latents = {}, {}
    for backend in ("torch", "hip"):
        head = dda.DDIMDepthEstimate_Res(inference_steps=2, codec_backend=backend)
        head.load_state_dict(sd)
        head = head.cuda().train()
        kinds = [type(m) for m in head.depth_transform.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Sigmoid))]
        if backend == "hip":
            assert kinds == [CD.HipCodecConv2d, CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecConv2d, CD.HipCodecTail]
        else:
            assert not any(issubclass(k, (CD.HipCodecConv2d, CD.HipCodecConvTranspose2d, CD.HipCodecTail)) for k in kinds)
        real_inv = head.depth_transform.inv_t
        head.depth_transform.inv_t = lambda v, _b=backend, _f=real_inv: (latents.__setitem__(_b, v.detach().clone()), _f(v))[1]
        torch.manual_seed(11)
        out = head([f.clone() for f in fp], gt, gt > 0, gt_depth_map=gt)
        (out["pred"].mean() + out["ddim_loss"]).backward()
        grads = {k: p.grad for k, p in head.named_parameters() if p.grad is not None}
        assert any(k.startswith("depth_transform.conv_inv_transform.") for k in grads)
        assert all(bool(torch.isfinite(g).all()) for g in grads.values()), [k for k, g in grads.items() if not torch.isfinite(g).all()]
        res[backend] = {"pred": out["pred"].detach().double().cpu().numpy(), "ddim_loss": out["ddim_loss"].detach().double().cpu().numpy()}
    refs = {}
    for backend in ("torch", "hip"):
        ref_codec = dda.DeepDepthTransformWithUpsampling()
        ref_codec.load_state_dict({k[len("depth_transform."):]: v for k, v in sd.items() if k.startswith("depth_transform.")})
        with torch.no_grad():
            refs[backend] = {"pred": ref_codec.double().train().inv_t(latents[backend].double().cpu()).numpy(), "ddim_loss": res["torch"]["ddim_loss"]}
    _held_to_the_rule(res["hip"], res["torch"], refs["hip"], "res head", refs["torch"])
