"""GPU (`-m gpu`): the folded eval-mode forward of include/ddepth_conv_fused.h / diffusiondepth_amd.conv on the MI355X.

The cases of tests/conv_fused_cases.py with the verdicts of the host emulation: the exact cases EQUAL the fp64 reference, the real-valued ones
stay within the cap, the identities with the un-fused operators and with zero-padded tensors hold as value equality, two runs give the same bits,
nothing is written outside y (every output sits between guard bands, as does the workspace's end), the ReLU keeps a NaN, and dd_bn_fold is within
one ulp of numpy.  Beyond that: no host synchronisation, the torch-path fallbacks, the network case F1 (a two-stage ResNetForMMBEV in .eval()
against the unconverted net in fp64 on the CPU) with its call census, and the facade with ``backbone_backend="hip+fold"``."""
import ctypes

import numpy as np
import pytest
import torch

import conv_fused_cases as FC

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats in front of and behind every output
SENTINEL = -12345.678


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _run(stride, dims, inp, prec, addend=True, relu=True):
    """dd_conv3x3_affine_forward on device copies of `inp` -> y (numpy).  y lies between guard bands, and so does the end of a workspace of exactly
    the queried size."""
    from diffusiondepth_amd import conv as CV
    lib = CV._lib_fused()
    B, Cin, Cout, H, W = dims
    p = FC.PRECISIONS[prec]
    x, w, ss, a = (inp[k].cuda().contiguous() for k in ("x", "w", "scale_shift", "addend"))
    ybuf, y = _guarded(FC.shapes_for(stride, dims)[3])
    n = ctypes.c_int64(0)
    CV._ck(lib.dd_conv3x3_affine_workspace_bytes(stride, B, Cin, Cout, H, W, p, ctypes.byref(n)), "dd_conv3x3_affine_workspace_bytes")
    ws = torch.full((n.value + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    CV._ck(lib.dd_conv3x3_affine_forward(x.data_ptr(), w.data_ptr(), ss.data_ptr(), a.data_ptr() if addend else None, y.data_ptr(), ws.data_ptr(),
                                         stride, int(relu), B, Cin, Cout, H, W, p, CV._stream(x)), "dd_conv3x3_affine_forward")
    torch.cuda.synchronize()
    assert _guards_intact(ybuf), "a kernel wrote outside y"
    assert bool((ws[n.value:] == 0x5A).all()), "a call wrote behind its workspace"
    for k, t in (("x", x), ("w", w), ("scale_shift", ss), ("addend", a)):
        assert torch.equal(t.cpu().view(torch.int32), inp[k].contiguous().view(torch.int32)), "an input was written"
    return y.cpu().numpy()


def _run_case(name, prec, kind, **kw):
    stride, dims = FC.SHAPES[name]
    return _run(stride, dims, FC.make_inputs(name, kind), prec, **kw)


@pytest.mark.parametrize("variant", FC.VARIANTS, ids=FC.variant_id)
@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_exact_cases_equal_the_fp64_reference(case, variant):
    name, prec = case
    addend, relu = variant
    FC.check_exact(_run_case(name, prec, "int", addend=addend, relu=relu), name, addend, relu, "gpu")


@pytest.mark.parametrize("variant", FC.VARIANTS, ids=FC.variant_id)
@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_real_valued_cases_stay_within_the_cap(case, variant):
    name, prec = case
    addend, relu = variant
    FC.check_real(_run_case(name, prec, "normal", addend=addend, relu=relu), name, prec, addend, relu, "gpu")


def _identity(inp, shift=None):
    cout = inp["scale_shift"].shape[1]
    return dict(inp, scale_shift=torch.stack([torch.ones(cout), torch.zeros(cout) if shift is None else shift]))


@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_the_identity_fold_equals_the_unfused_forward(case):
    """scale = 1, shift = 0, no addend, relu = 0: dd_convx_forward at stride 1, dd_conv3x3s2_forward(bias = NULL) at stride 2; at stride 2 also
    shift = bias against dd_conv3x3s2_forward(bias).  Value equality."""
    from diffusiondepth_amd import conv as CV
    name, prec = case
    stride, dims = FC.SHAPES[name]
    inp = FC.make_inputs(name, "normal")
    p = FC.PRECISIONS[prec]
    got = _run(stride, dims, _identity(inp), prec, addend=False, relu=False)
    if stride == 1:
        want = CV.conv_forward(CV.OP_CONV3X3, inp["x"].cuda(), inp["w"].cuda(), p, "any").cpu().numpy()
    else:
        want = CV.conv_s2_forward(inp["x"].cuda(), inp["w"].cuda(), None, p).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())
    if stride == 2:
        bias = inp["scale_shift"][1].contiguous()
        got = _run(stride, dims, _identity(inp, bias), prec, addend=False, relu=False)
        want = CV.conv_s2_forward(inp["x"].cuda(), inp["w"].cuda(), bias.cuda(), p).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("prec", list(FC.PRECISIONS))
@pytest.mark.parametrize("name", FC.PAD_RAGGED)
def test_a_ragged_shape_equals_the_block64_instantiation_on_zero_padded_tensors(name, prec):
    stride = FC.SHAPES[name][0]
    got = _run_case(name, prec, "normal")
    dims, padded = FC.zero_padded(name)
    want = FC.cut(name, _run(stride, dims, padded, prec))
    assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("name", ["S1", "Z6"])
def test_two_runs_give_the_same_bits(name):
    a, b = _run_case(name, "f16x3", "normal"), _run_case(name, "f16x3", "normal")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("in_shift", (False, True), ids=["x", "x+shift"])
@pytest.mark.parametrize("addend", FC.ADDEND, ids=["add", "noadd"])
@pytest.mark.parametrize("prec", list(FC.PRECISIONS))
def test_the_relu_keeps_a_nan(prec, addend, in_shift):
    stride, dims = FC.SHAPES[FC.NAN_CASE]
    FC.check_nan(_run(stride, dims, FC.nan_inputs(in_shift), prec, addend=addend, relu=True), in_shift, addend, "gpu")


class _Bn:
    """What bn_fold reads of a BatchNorm."""

    def __init__(self, v, absent):
        t = lambda k: torch.from_numpy(v[k]).cuda()
        self.weight = None if absent == "gamma" else t("gamma")
        self.bias = None if absent == "beta" else t("beta")
        self.running_mean, self.running_var, self.eps, self.num_features = t("mean"), t("var"), FC.FOLD_EPS, v["mean"].size


@pytest.mark.parametrize("absent", FC.FOLD_ABSENT, ids=str)
@pytest.mark.parametrize("C", FC.FOLD_C)
def test_bn_fold_is_within_one_ulp_of_numpy(C, absent):
    from diffusiondepth_amd import conv as CV
    v = FC.fold_inputs(C)
    got = CV.bn_fold(_Bn(v, absent), None if absent == "conv_bias" else torch.from_numpy(v["conv_bias"]).cuda())
    assert got.shape == (2, C) and got.dtype == torch.float32
    FC.check_fold(got.cpu().numpy(), v, absent, "gpu")
    if absent is None:
        cb = torch.from_numpy(v["conv_bias"]).cuda()
        ident = CV.bn_fold(None, cb)
        assert torch.equal(ident[0], torch.ones_like(cb)) and torch.equal(ident[1], cb)


# ---- the module layer ---------------------------------------------------------------------------------------------------------------------------
def _block(cin=64, cout=64, stride=1, first=False, prec="f16x3"):
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd import model as M
    torch.manual_seed(4)
    blk = M._BasicBlock(cin, cout, stride, first=first)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for bn in (blk.bn1, blk.bn2):
            bn.weight.copy_(0.5 + torch.rand(cout, generator=g))
            bn.bias.copy_(0.3 * torch.randn(cout, generator=g))
            bn.running_mean.copy_(0.3 * torch.randn(cout, generator=g))
            bn.running_var.copy_(0.5 + 1.5 * torch.rand(cout, generator=g))
    return M.fold_eval_basic_blocks(CV.convert_hip_conv(blk, prec, channels="any", strided=True)).cuda().eval()


class _census:
    """Counts the calls of conv.conv_affine_forward and of F.batch_norm while it is active."""

    def __enter__(self):
        import torch.nn.functional as F
        from diffusiondepth_amd import conv as CV
        self.affine, self.batch_norm, self._real = [], [], (CV.conv_affine_forward, F.batch_norm)
        CV.conv_affine_forward = lambda *a, **k: (self.affine.append(1), self._real[0](*a, **k))[1]
        F.batch_norm = lambda *a, **k: (self.batch_norm.append(1), self._real[1](*a, **k))[1]
        return self

    def __exit__(self, *exc):
        import torch.nn.functional as F
        from diffusiondepth_amd import conv as CV
        CV.conv_affine_forward, F.batch_norm = self._real


def test_the_folded_block_does_not_synchronise_the_host():
    blk = _block(3, 64, 2, first=True)
    x = torch.randn(2, 3, 20, 36, device="cuda")
    with torch.no_grad():
        blk(x)                              # (the first call loads the library and allocates the workspaces)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with _census() as c:
                y = blk(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert len(c.affine) == 3 and not c.batch_norm and torch.isfinite(y).all()


def test_foreign_inputs_and_modes_take_the_path_the_block_took_before():
    """Half and non-contiguous inputs, a convolution of a precision the library does not run, a BatchNorm without running statistics, .train() and
    grad mode: conv_bn_act declines or is not asked, and the block equals the unfolded one bit for bit."""
    from diffusiondepth_amd import conv as CV
    blk = _block()
    x = torch.randn(2, 64, 9, 14, device="cuda")
    with torch.no_grad(), _census() as c:
        want = blk(x)
    assert len(c.affine) == 2 and not c.batch_norm
    plain = lambda t: (setattr(blk, "folded_eval", False), blk(t), setattr(blk, "folded_eval", True))[1]
    with torch.no_grad():
        assert CV.conv_bn_act(blk.conv1, blk.bn1, x.half()) is None
        xt = torch.randn(2, 14, 9, 64, device="cuda").permute(0, 3, 2, 1)
        assert not xt.is_contiguous() and CV.conv_bn_act(blk.conv1, blk.bn1, xt) is None
        assert CV.conv_bn_act(blk.conv1, blk.bn1, x, addend=x[:, :, :4]) is None
        with _census() as c:
            got = blk(xt)
        assert not c.affine and len(c.batch_norm) == 2 and torch.equal(got, plain(xt))
        blk.conv1.precision = "fp32"
        assert CV.conv_bn_act(blk.conv1, blk.bn1, x) is None
        with _census() as c:
            got = blk(x)
        assert not c.affine and len(c.batch_norm) == 2 and torch.equal(got, plain(x))
        blk.conv1.precision = "f16x3"
        nostats = torch.nn.BatchNorm2d(64, track_running_stats=False).cuda().eval()
        assert CV.conv_bn_act(blk.conv1, nostats, x) is None and CV.conv_bn_act(blk.conv1, blk.bn1.train(), x) is None
        blk.eval()
        with _census() as c:
            assert torch.equal(blk(x), want)
        assert len(c.affine) == 2
    with _census() as c:      # grad enabled in .eval(): the un-fused path
        y = blk(x)
    assert not c.affine and len(c.batch_norm) == 2 and y.requires_grad
    assert torch.equal(y, plain(x))
    blk.train()
    with torch.no_grad(), _census() as c:
        blk(x)
    assert not c.affine and len(c.batch_norm) == 2


# ---- the network case F1 ------------------------------------------------------------------------------------------------------------------------
def _f1(prec, fold):
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd import model as M
    from diffusiondepth_amd.batchnorm import convert_hip_batchnorm
    net = CV.convert_hip_conv(FC.f1_net(), prec, channels="any", strided=True)
    if fold:      # what backbone_backend="hip+fold" does
        net = M.fold_eval_basic_blocks(M.fuse_basic_block_tails(convert_hip_batchnorm(net)))
    return net.cuda().eval()


def _f1_errors(prec):
    """(err(fold), err(un-fused "hip"), err(fp32 torch eval)) per feature map, and the census of the folded run."""
    x = FC.f1_input().cuda()
    with torch.no_grad():
        e32 = FC.f1_errors(FC.f1_net().cuda()(x))
        ehip = FC.f1_errors(_f1(prec, False)(x))
        with _census() as c:
            efold = FC.f1_errors(_f1(prec, True)(x))
    return efold, ehip, e32, c


@pytest.mark.parametrize("prec", FC.F1_ASSERTED)
def test_f1_the_fold_is_as_close_to_fp64_as_the_unfused_path(prec):
    efold, ehip, e32, c = _f1_errors(prec)
    assert len(c.affine) == 6 and not c.batch_norm, "each of the two opening blocks makes three fused calls and no F.batch_norm"
    for i, (f, h, t) in enumerate(zip(efold, ehip, e32)):
        print(f"F1 {prec} feature{i}: relative L2 fold {f:.3e} un-fused {h:.3e} fp32 torch {t:.3e} allowed {h + 4 * max(t, 1e-6):.3e}")
    assert len(efold) == 2 and all(f <= h + 4 * max(t, 1e-6) for f, h, t in zip(efold, ehip, e32))


def test_f1_in_f16_is_recorded():
    import gpu_util
    efold, ehip, e32, c = _f1_errors("f16")
    assert len(c.affine) == 6 and not c.batch_norm
    gpu_util.record("conv_fused_f1_f16", fold=max(efold), unfused=max(ehip), fp32=max(e32))
    assert all(np.isfinite(v) for v in efold + ehip + e32)


def test_f1_with_grad_enabled_is_the_unfused_path_and_gradients_reach_the_weights():
    from diffusiondepth_amd import model as M
    x = FC.f1_input().cuda()
    fold, plain = _f1("bf16", True), _f1("bf16", True)
    for m in plain.modules():
        if isinstance(m, M._BasicBlock):
            m.folded_eval = False
    with _census() as c:
        fa, fb = fold(x), plain(x)
    assert not c.affine and all(torch.equal(a, b) for a, b in zip(fa, fb))
    sum((f ** 2).sum() for f in fa).backward()
    convs = [m for m in fold.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 6 and all(m.weight.grad is not None and torch.isfinite(m.weight.grad).all() and m.weight.grad.abs().sum() > 0 for m in convs)


# ---- the facade ---------------------------------------------------------------------------------------------------------------------------------
def _facade(backend):
    from diffusiondepth_amd import model as M
    torch.manual_seed(0)
    return M.Diffusion_DCbase_Model(M.default_args(backbone_name="mmbev_res18", inference_steps=2, precision="f16r", backbone_backend=backend,
                                                   backbone_precision="f16x3")).cuda()


def test_a_fast_profile_facade_runs_a_folded_f16x3_backbone():
    from diffusiondepth_amd import conv as CV
    from diffusiondepth_amd import model as M
    from diffusiondepth_amd import synth
    model = _facade("hip+fold").eval()
    bb = model.depth_backbone
    assert sum(isinstance(m, CV.HipConv2d) for m in bb.modules()) == 20
    blocks = [m for m in bb.modules() if isinstance(m, M._BasicBlock)]
    assert len(blocks) == 8 and all(b.folded_eval for b in blocks)
    rgb = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    gt = torch.from_numpy(synth.make_gt_depth(6, 2, 64, 96)).cuda()
    with torch.no_grad(), _census() as c:
        out = model({"rgb": rgb, "gt": gt, "dep": gt, "depth_map": gt, "depth_mask": gt > 0})
    assert out["pred"].shape == (2, 1, 64, 96) and torch.isfinite(out["pred"]).all()
    assert len(c.affine) == 4 * 3 + 4 * 2, "four opening blocks of three fused calls, four plain blocks of two"


def test_the_facade_in_train_makes_the_calls_hip_bn_makes():
    from diffusiondepth_amd import batchnorm as BN
    from diffusiondepth_amd import conv as CV
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    names = (("conv", CV, "conv_s2_forward"), ("conv", CV, "conv_forward"), ("bn", BN, "bn_apply"), ("bn", BN, "bn_apply_add"),
             ("affine", CV, "conv_affine_forward"))
    seen = {}
    for backend in ("hip+bn", "hip+fold"):
        bb = _facade(backend).train().depth_backbone
        calls, real = [], {}
        for _, mod, fn in names:
            real[fn] = getattr(mod, fn)
            setattr(mod, fn, (lambda fn: lambda *a, **k: (calls.append(fn), real[fn](*a, **k))[1])(fn))
        try:
            feats = bb(x)
        finally:
            for _, mod, fn in names:
                setattr(mod, fn, real[fn])
        assert all(torch.isfinite(f).all() for f in feats)
        seen[backend] = calls
    assert seen["hip+fold"] == seen["hip+bn"] and "conv_affine_forward" not in seen["hip+fold"]
    assert len(seen["hip+bn"]) == 20 + 16 and seen["hip+bn"].count("bn_apply_add") == 8
