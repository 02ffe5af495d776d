"""GPU (`-m gpu`): the BatchNorm with an addend of include/ddepth_bn_add.h / diffusiondepth_amd.batchnorm on the MI355X.

Every compared tensor of the module cases is held to the rule of tests/bn_add_cases.py: max|hip - ref64| <= 4 * max(max|ref32 - ref64|,
2^-23 max|ref64|) against the torch CPU evaluation of act(bn(x) + r) / act(bn(x)) + r and its autograd; activation cases are built with
min|kink64| >= 1e-4 and compared without exclusions.  Beyond that: the exact identities that tie the new kernels to the existing ones, the fused
tail against its un-fused composition bit for bit, bitwise repeatability, no host synchronisation, the split ABI used as an exchange between two
"ranks", a small fused backbone against the same net on torch's BatchNorm, and a "hip+add" Res head against the "hip" one."""
import copy

import numpy as np
import pytest
import torch

import bn_add_cases as AC
import bn_cases as BC

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
ACT_NAMES = {"none": None, "relu": "relu", "leaky": "leaky_relu"}


def _module(shape, mode, act, affine, kind):
    from diffusiondepth_amd import batchnorm as BN
    inp = AC.make_inputs(shape, mode, act, affine, kind)
    m = BN.HipBatchNorm2d(shape[1], eps=BC.EPS, momentum=BC.MOMENTUM, affine=affine, activation=ACT_NAMES[act], negative_slope=AC.ACTS[act][1])
    m.add_mode = mode
    with torch.no_grad():
        if affine:
            m.weight.copy_(inp["weight"])
            m.bias.copy_(inp["bias"])
        m.running_mean.copy_(inp["running_mean"])
        m.running_var.copy_(inp["running_var"])
    return m.cuda().train(), inp


def _collect(m, x, r, y, affine):
    return {"y": y.detach().cpu().numpy(), "grad_x": x.grad.cpu().numpy(), "grad_addend": r.grad.cpu().numpy(),
            "grad_weight": m.weight.grad.cpu().numpy() if affine else None, "grad_bias": m.bias.grad.cpu().numpy() if affine else None,
            "running_mean": m.running_mean.cpu().numpy(), "running_var": m.running_var.cpu().numpy()}


def _count_apply_add(fn):
    """fn() with diffusiondepth_amd.batchnorm.bn_apply_add counted; -> (fn's result, the add_mode of every call)."""
    from diffusiondepth_amd import batchnorm as BN
    calls, real = [], BN.bn_apply_add

    def counting(x, mean_invstd, addend, weight=None, bias=None, act=0, slope=0.0, add_mode=0):
        calls.append(int(add_mode))
        return real(x, mean_invstd, addend, weight, bias, act, slope, add_mode)

    BN.bn_apply_add = counting
    try:
        return fn(), calls
    finally:
        BN.bn_apply_add = real


def _run_module(shape, mode, act, affine, kind):
    m, inp = _module(shape, mode, act, affine, kind)
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    r = inp["addend"].detach().clone().cuda().requires_grad_(True)
    y, calls = _count_apply_add(lambda: m(x, addend=r))
    assert calls == [AC.MODES[mode]], calls                  # the library path, not the torch one
    y.backward(inp["grad_y"].cuda())
    assert int(m.num_batches_tracked) == 1
    return _collect(m, x, r, y, affine)


@pytest.mark.parametrize("variant", AC.VARIANTS, ids=AC.variant_id)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_module_with_an_addend_against_torch_cpu(shape, variant):
    AC.check(_run_module(shape, *variant), shape, *variant, "gpu")


# ---- exact identities, through the Python calls ---------------------------------------------------------------------------------------------------
def _parts(shape, mode, act):
    from diffusiondepth_amd import batchnorm as BN
    inp = AC.make_inputs(shape, mode, act, True, "normal")
    x, r, gy, w, b = (inp[k].cuda() for k in ("x", "addend", "grad_y", "weight", "bias"))
    mi = BN.bn_finalize(BN.bn_stats(x), BC.EPS)
    return BN, inp, x, r, gy, w, b, mi


@pytest.mark.parametrize("act", list(AC.ACTS))
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_identities_a_and_b_zero_addend_and_post_mode(shape, act):
    """(a) "pre" with r = 0 is dd_bn_apply; (b) "post" is dd_bn_apply's y plus r in numpy fp32, bit for bit (the add is never contracted into
    the LeakyReLU's multiply)."""
    act_id, slope = AC.ACTS[act]
    BN, inp, x, r, gy, w, b, mi = _parts(shape, "post", act)
    plain = BN.bn_apply(x, mi, w, b, act_id, slope)
    assert torch.equal(BN.bn_apply_add(x, mi, torch.zeros_like(x), w, b, act_id, slope, BN.ADD_PRE), plain)
    post = BN.bn_apply_add(x, mi, r, w, b, act_id, slope, BN.ADD_POST)
    assert np.array_equal(post.cpu().numpy(), (plain.cpu().numpy() + inp["addend"].numpy()).astype(np.float32))


@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_identities_c_and_d_pre_relu_forward_mask_and_sums(shape):
    """(c) y = max(dd_bn_apply(act none) + r, 0) in numpy fp32; (d) g = grad_y * (y > 0), and sums2 has the bits dd_bn_backward_reduce gives on
    (x, g) without an activation."""
    BN, inp, x, r, gy, w, b, mi = _parts(shape, "pre", "relu")
    y = BN.bn_apply_add(x, mi, r, w, b, BN.ACT_RELU, 0.0, BN.ADD_PRE)
    z = BN.bn_apply(x, mi, w, b, BN.ACT_NONE, 0.0).cpu().numpy()
    assert np.array_equal(y.cpu().numpy(), np.maximum((z + inp["addend"].numpy()).astype(np.float32), np.float32(0)))
    g, sums2 = BN.bn_backward_reduce_add(x, gy, y, mi, BN.ACT_RELU, 0.0)
    assert np.array_equal(g.cpu().numpy(), inp["grad_y"].numpy() * (y.cpu().numpy() > 0))
    assert torch.equal(sums2, BN.bn_backward_reduce(x, g, mi, None, None, BN.ACT_NONE, 0.0))


@pytest.mark.parametrize("shape", [AC.SHAPES[1], AC.SHAPES[2]], ids=str)
def test_the_fused_tail_equals_its_unfused_composition_bit_for_bit(shape):
    """relu(HipBatchNorm2d(act None)(x) + r) with torch's add and ReLU against the one fused module: y, grad_x, grad_addend, the parameter
    gradients and the running statistics."""
    fused = _run_module(shape, "pre", "relu", True, "normal")
    m, inp = _module(shape, "pre", "none", True, "normal")
    src = AC.make_inputs(shape, "pre", "relu", True, "normal")      # the fused run's inputs (the case's seed depends on the activation)
    with torch.no_grad():
        m.weight.copy_(src["weight"])
        m.bias.copy_(src["bias"])
        m.running_mean.copy_(src["running_mean"])
        m.running_var.copy_(src["running_var"])
    x = src["x"].detach().clone().cuda().requires_grad_(True)
    r = src["addend"].detach().clone().cuda().requires_grad_(True)
    y = torch.relu(m(x) + r)
    y.backward(src["grad_y"].cuda())
    unfused = _collect(m, x, r, y, True)
    for k in AC.KEYS:
        assert np.array_equal(fused[k], unfused[k]), k


@pytest.mark.parametrize("mode", list(AC.MODES))
@pytest.mark.parametrize("shape", [AC.SHAPES[1], AC.SHAPES[2]], ids=str)
def test_two_runs_give_the_same_bits(shape, mode):
    a, b = _run_module(shape, mode, "leaky", True, "normal"), _run_module(shape, mode, "leaky", True, "normal")
    for k in AC.KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", list(AC.MODES))
def test_forward_and_backward_do_not_synchronise_the_host(mode):
    m, inp = _module(AC.SHAPES[2], mode, "relu", True, "normal")
    x = inp["x"].detach().clone().cuda().requires_grad_(True)
    r = inp["addend"].detach().clone().cuda().requires_grad_(True)
    gy = inp["grad_y"].cuda()
    m(x, addend=r).backward(gy)             # (the first call loads the library and allocates the workspace)
    x.grad = r.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = m(x, addend=r)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(r.grad).all() and int(m.num_batches_tracked) == 2


def test_unsuitable_addends_take_the_torch_path():
    """No silent copy or conversion: a non-contiguous or half addend, and a "pre" LeakyReLU of negative slope, run torch's expression."""
    from diffusiondepth_amd import batchnorm as BN
    torch.manual_seed(0)
    x = torch.randn(2, 8, 5, 6, device="cuda")
    for mode in ("pre", "post"):
        m = BN.HipBatchNorm2d(8, activation="relu").cuda().train()
        m.add_mode = mode
        ref = torch.nn.BatchNorm2d(8).cuda().train()
        for r in (torch.randn(2, 5, 6, 8, device="cuda").permute(0, 3, 1, 2), torch.randn(2, 8, 5, 6, device="cuda").half()):
            got, calls = _count_apply_add(lambda: m(x, addend=r))
            want = torch.relu(ref(x) + r) if mode == "pre" else torch.relu(ref(x)) + r
            assert calls == [] and got.dtype == want.dtype and torch.equal(got, want)
    m = BN.HipBatchNorm2d(8, activation="leaky_relu", negative_slope=-0.5).cuda().train()
    ref = torch.nn.BatchNorm2d(8).cuda().train()
    r = torch.randn(2, 8, 5, 6, device="cuda")
    got, calls = _count_apply_add(lambda: m(x, addend=r))
    assert calls == [] and torch.equal(got, torch.nn.functional.leaky_relu(ref(x) + r, -0.5))
    m.add_mode = "post"                      # behind the activation the mask comes from x: any slope runs in the library
    got, calls = _count_apply_add(lambda: m(x, addend=r))
    assert calls == [BN.ADD_POST] and torch.allclose(got, torch.nn.functional.leaky_relu(ref(x), -0.5) + r, atol=1e-5)


@pytest.mark.parametrize("mode", list(AC.MODES))
@pytest.mark.parametrize("shape", [(4, 3, 5, 7), (4, 16, 11, 19), (4, 4, 67, 131)], ids=str)
def test_the_split_abi_as_an_exchange_between_two_halves_of_a_batch(shape, mode):
    """A batch of 4 treated as two ranks of 2, as in tests/test_zz_gpu_bn.py: the statistics (of x alone) are exchanged as before, the apply
    with the addend and the one-pass backward reduction run per half.  y, grad_addend and grad_x must equal the whole-batch calls to 2^-22
    relative per element: the fp64 sums are only reordered, and one fp32 rounding follows."""
    from diffusiondepth_amd import batchnorm as BN
    gen = torch.Generator().manual_seed(sum(shape) + 1)
    C = shape[1]
    x, gy = (torch.randn(shape, generator=gen) * 1.5 + 0.3).cuda(), torch.randn(shape, generator=gen).cuda()
    r = torch.randn(shape, generator=gen).cuda()
    w, b = (0.5 + torch.rand(C, generator=gen)).cuda(), torch.randn(C, generator=gen).cuda()
    act, slope, mode_id = BN.ACT_LEAKY_RELU, 0.2, AC.MODES[mode]

    def backward(xh, gh, yh, mi_, sums_):
        """-> (g, local sums2, grad_x given the exchanged sums2)"""
        if mode == "pre":
            g, s2 = BN.bn_backward_reduce_add(xh, gh, yh, mi_, act, slope)
            return g, s2, lambda ex2: BN.bn_backward_apply(xh, g, mi_, ex2, sums_, w, None, BN.ACT_NONE, 0.0)
        s2 = BN.bn_backward_reduce(xh, gh, mi_, w, b, act, slope)
        return gh, s2, lambda ex2: BN.bn_backward_apply(xh, gh, mi_, ex2, sums_, w, b, act, slope)

    # the whole batch
    sums = BN.bn_stats(x)
    mi = BN.bn_finalize(sums, BC.EPS)
    y = BN.bn_apply_add(x, mi, r, w, b, act, slope, mode_id)
    g, sums2, apply = backward(x, gy, y, mi, sums)
    gx = apply(sums2)
    # two "ranks"
    halves = [tuple(t[s].contiguous() for t in (x, gy, r)) for s in (slice(0, 2), slice(2, 4))]
    part = [BN.bn_stats(xh) for xh, _, _ in halves]
    ex = part[0] + part[1]                                   # the exchange
    assert float(ex[2 * C]) == float(sums[2 * C])
    mi_h = BN.bn_finalize(ex, BC.EPS)
    y_halves = [BN.bn_apply_add(xh, mi_h, rh, w, b, act, slope, mode_id) for xh, _, rh in halves]
    back = [backward(xh, gh, yh, mi_h, ex) for (xh, gh, _), yh in zip(halves, y_halves)]
    ex2 = back[0][1] + back[1][1]
    y_h, g_h, gx_h = torch.cat(y_halves), torch.cat([t[0] for t in back]), torch.cat([t[2](ex2) for t in back])
    for name, got, want in (("y", y_h, y), ("grad_addend", g_h, g), ("grad_x", gx_h, gx)):
        rel = ((got - want).abs() / want.abs().clamp_min(1e-30)).max().item()
        print(f"split-abi {mode} {shape} {name}: max relative difference {rel:.3e}")
        assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs()).all()), (name, rel)
    # the local sums2 are the parameter gradients of each half: together the whole batch's
    assert torch.allclose(ex2, sums2, rtol=1e-12, atol=1e-12)


# ---- backbone level -------------------------------------------------------------------------------------------------------------------------------
def _backbone_step(net, x, ups, dev, dtype):
    """One .train() forward and backward of a backbone with an upstream gradient per emitted map; -> dict name -> fp64 numpy."""
    net = net.to(dev).to(dtype).train()
    net.zero_grad()
    xi = x.to(dev, dtype).clone().requires_grad_(True)
    feats = net(xi)
    torch.autograd.backward(feats, [u.to(dev, dtype) for u in ups])
    out = {f"feat{i}": f for i, f in enumerate(feats)}
    out["grad_x"] = xi.grad
    out.update({"grad:" + k: p.grad for k, p in net.named_parameters()})
    out.update({"buf:" + k: v for k, v in net.named_buffers() if k.endswith(("running_mean", "running_var"))})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def test_fused_two_stage_backbone_in_train_mode_against_the_same_net_on_torch_batchnorm():
    """The rule of the head test in tests/test_zz_gpu_bn.py (the convolutions are outside this module, so the bound is measured): per tensor, the
    error of the fused backbone against the fp64 CPU evaluation must be <= 2 x the error of the same net on torch's BatchNorm, add and ReLU on
    the GPU for the same inputs (floor 2^-23 max|ref64|).  Every block tail must have run dd_bn_apply_add.

    Both GPU evaluations run with torch.backends.cudnn.deterministic (MIOpen's deterministic solvers): in its default mode torch's convolution
    backward gives other bits from one process to the next, and both errors are rounding noise of those convolutions carried through four
    blocks -- maxima over tensors of as few as 8 values, whose ratio then moves around 1 from run to run (measured with the default mode: worst
    ratio to the bound 0.91 in one process, 1.0007 at grad:layers.1.1.bn1.bias in another).  In deterministic mode two processes give the
    same bits and the worst ratio is 0.91 (grad:layers.1.0.bn2.weight: 1.8e-5 against torch's 9.8e-6).  For the record, with MIOpen switched
    off altogether (torch's im2col + GEMM convolutions and native BatchNorm; also bit-stable) the same rule is MISSED at two tensors:
    grad:layers.0.1.bn1.weight 2.42e-5 against 2 x 1.15e-5 and grad:layers.0.1.bn2.weight 2.12e-5 against 2 x 0.98e-5 (ratio 1.08).  That
    configuration is not the one the rule names (the head test's reference is MIOpen's BatchNorm) and is not asserted here."""
    from diffusiondepth_amd import batchnorm as BN
    from diffusiondepth_amd import model as M
    torch.manual_seed(11)
    a = M.ResNetForMMBEV([2, 2], channels=(8, 16))
    with torch.no_grad():
        for m in a.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    b = M.fuse_basic_block_tails(BN.convert_hip_batchnorm(copy.deepcopy(a)))
    r = copy.deepcopy(a)
    assert list(b.state_dict()) == list(a.state_dict()) and all(blk.fused_tail for blk in b.modules() if isinstance(blk, M._BasicBlock))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 22, 38, generator=gen)
    ups = [torch.randn(2, 8, 11, 19, generator=gen), torch.randn(2, 16, 6, 10, generator=gen)]
    ref = _backbone_step(r, x, ups, "cpu", torch.float64)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        tor = _backbone_step(a, x, ups, "cuda", torch.float32)
        hip, calls = _count_apply_add(lambda: _backbone_step(b, x, ups, "cuda", torch.float32))
    finally:
        torch.backends.cudnn.deterministic = det
    assert calls == [BN.ADD_PRE] * 4, calls              # four blocks, four tails in the library
    assert set(ref) == set(tor) == set(hip) and any(k.startswith("grad:layers.0.1.bn2.") for k in ref) and any(k.startswith("buf:") for k in ref)
    failures = []
    for k in sorted(ref):
        e_t, e_h = float(np.max(np.abs(tor[k] - ref[k]))), float(np.max(np.abs(hip[k] - ref[k])))
        bnd = max(2.0 * e_t, ULP * float(np.max(np.abs(ref[k]))))
        print(f"backbone {k}: torch {e_t:.3e} hip {e_h:.3e} bound {bnd:.3e}")
        if not e_h <= bnd:
            failures.append((k, e_t, e_h, bnd))
    assert not failures, failures


# ---- head level -----------------------------------------------------------------------------------------------------------------------------------
def _condition_step(head, fp, up):
    """aggregate_condition of a .train() head and its backward; what the BatchNorm path computes: the condition, the gradients of the pyramid
    and of the BatchNorm parameters, the running statistics."""
    head = head.cuda().train()
    head.zero_grad()
    f = [t.cuda().clone().requires_grad_(True) for t in fp]
    cond = head.aggregate_condition(f)
    cond.backward(up.cuda())
    out = {"cond": cond}
    out.update({f"grad_fp{i}": t.grad for i, t in enumerate(f)})
    out.update({"grad:" + k: p.grad for k, p in head.named_parameters()      # (index 1 of each Sequential: the BatchNorm)
                if k.startswith(("conv_lateral.", "conv_up.")) and k.split(".")[2] == "1" and p.grad is not None})
    out.update({"buf:" + k: v for k, v in head.named_buffers() if k.startswith(("conv_lateral.", "conv_up.")) and k.endswith(("running_mean", "running_var"))})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def test_hip_add_res_head_in_train_mode_equals_the_hip_head_bit_for_bit():
    """Skipping the identity pool and fusing the add change no bits: on the inputs of the bn_backend="hip" head, the "hip+add" head gives the
    same condition, the same gradients and the same running statistics, and all three top-down sites ran in the library."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import batchnorm as BN
    from diffusiondepth_amd import synth
    torch.manual_seed(0)
    a = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip")
    b = dda.DDIMDepthEstimate_Res(inference_steps=2, bn_backend="hip+add")
    b.load_state_dict(a.state_dict())
    B, H, W = 2, 32, 64
    fp = [torch.from_numpy(f) for f in synth.make_backbone_features(3, B, H, W)]
    up = torch.randn(B, 256, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
    det = torch.backends.cudnn.deterministic      # torch's convolutions sit between the compared tensors: the same algorithm in both runs
    torch.backends.cudnn.deterministic = True
    try:
        want, none = _count_apply_add(lambda: _condition_step(a, fp, up))
        got, calls = _count_apply_add(lambda: _condition_step(b, fp, up))
    finally:
        torch.backends.cudnn.deterministic = det
    assert none == [] and calls == [BN.ADD_POST] * 3, (none, calls)
    assert set(got) == set(want) and any(k.startswith("grad:conv_lateral.0.1.") for k in got) and any(k.startswith("buf:conv_up.") for k in got)
    for k in sorted(want):
        assert np.array_equal(got[k], want[k]), k
