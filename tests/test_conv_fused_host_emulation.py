"""CPU: include/ddepth_conv_fused.h (the folded eval-mode forward: 3x3 pad 1, stride 1 or 2, BatchNorm + residual + ReLU in the epilogue) with
csrc/dd_conv.hip + csrc/dd_api_conv.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h, built as
tests/test_conv_strided_host_emulation.py builds them: the cases of tests/conv_fused_cases.py against the fp64 references under both wave
schedules, sentinels around every tensor, a guard behind a workspace of exactly the queried size, and the workspace refilled with 0x5A or 0xFF
bytes before every call.  Beyond the references: the identities with the un-fused operators, the zero-padding identity, repeatability, NaN
propagation through the ReLU, dd_bn_fold against numpy, and the argument errors."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import conv_fused_cases as FC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_conv.h", "dd_conv_kernels.h", "dd_status.h")] + \
    [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", h) for h in ("ddepth.h", "ddepth_conv.h", "ddepth_conv_scaled.h", "ddepth_conv_strided.h",
                                                  "ddepth_conv_fused.h")]
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4
DD_CONV_3X3 = 0


@pytest.fixture(scope="module")
def lib():
    cxx = U._clangxx()
    if cxx is None:
        pytest.skip("no clang++ (the kernels use clang vector extensions; g++ cannot compile them)")
    if not U.have_f16c():
        pytest.skip("host without F16C (the emulation's common compile flags ask for it)")
    hsh = hashlib.sha1()
    for d in DEPS:
        with open(d, "rb") as f:
            hsh.update(f.read())
    with U._BuildLock():
        out = os.path.join(U.OUT, "conv_fused_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_conv_hostemu.so")
        if not os.path.exists(so):
            os.makedirs(out, exist_ok=True)
            objs = []
            for src in UNITS:
                obj = os.path.join(out, os.path.basename(src).rsplit(".", 1)[0] + ".o")
                r = U._cc(cxx, src, obj, [U.EMU, U.CSRC])
                if r.returncode != 0:
                    pytest.fail("host build of %s failed:\n%s" % (src, r.stderr[-4000:]))
                objs.append(obj)
            U._link(cxx, objs, so)
    lib = ctypes.CDLL(so)
    c_int, c_vp = ctypes.c_int, ctypes.c_void_p
    lib.dd_conv_last_error.restype = ctypes.c_char_p
    lib.dd_bn_fold.argtypes = [c_vp] * 4 + [ctypes.c_double] + [c_vp] * 2 + [c_int, c_vp]
    lib.dd_conv3x3_affine_supported.argtypes = [c_int] * 4
    lib.dd_conv3x3_affine_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_conv3x3_affine_forward.argtypes = [c_vp] * 6 + [c_int] * 8 + [c_vp]
    lib.dd_convx_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_convx_forward.argtypes = [c_int] + [c_vp] * 4 + [c_int] * 6 + [c_vp]
    lib.dd_conv3x3s2_workspace_bytes.argtypes = [c_int] * 6 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_conv3x3s2_forward.argtypes = [c_vp] * 5 + [c_int] * 6 + [c_vp]
    lib.emu_set_order.argtypes = [c_int]
    return lib


def ok(lib, rc):
    assert rc == 0, lib.dd_conv_last_error()


SENTINEL = np.float32(-12345.678)


class Guarded:
    """Tensors with sentinel values in front of and behind them, 16 floats each; what lies around a tensor must come back untouched."""

    def __init__(self):
        self.bufs = []

    def __call__(self, a):
        buf = np.full(a.size + 32, SENTINEL, dtype=np.float32)
        view = buf[16:16 + a.size].reshape(a.shape)
        view[...] = a
        self.bufs.append((buf, a.size))
        return view

    def check(self):
        for buf, size in self.bufs:
            assert (buf[:16] == SENTINEL).all() and (buf[16 + size:] == SENTINEL).all(), "a kernel wrote outside a tensor"


def _workspace(nbytes, fill):
    raw = np.full(nbytes + 64 + 16, 0x5A, dtype=np.uint8)
    ws = raw[(-raw.ctypes.data) % 16:]      # 16-byte aligned
    ws[:nbytes] = fill
    return ws


def run(lib, stride, dims, inp, prec, addend=True, relu=True, fill=0x5A):
    """One dd_conv3x3_affine_forward on numpy memory -> y.  The workspace has exactly the size the API asks for, is filled with `fill` bytes and
    has a 0x5A guard behind it; every tensor sits between sentinels."""
    B, Cin, Cout, H, W = dims
    ys = FC.shapes_for(stride, dims)[3]
    p = FC.PRECISIONS[prec]
    guard = Guarded()
    x, w, ss, a = (guard(inp[k].numpy()) for k in ("x", "w", "scale_shift", "addend"))
    y = guard(np.full(ys, np.nan, dtype=np.float32))
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_conv3x3_affine_workspace_bytes(stride, B, Cin, Cout, H, W, p, ctypes.byref(n)))
    ws = _workspace(n.value, fill)
    P = U.ptr
    ok(lib, lib.dd_conv3x3_affine_forward(P(x), P(w), P(ss), P(a) if addend else None, P(y), P(ws), stride, int(relu), B, Cin, Cout, H, W, p, None))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("scale_shift", ss), ("addend", a)):
        assert np.array_equal(src, inp[k].numpy(), equal_nan=True), "an input was written"
    return y.copy()


def run_case(lib, name, prec, kind, **kw):
    stride, dims = FC.SHAPES[name]
    return run(lib, stride, dims, FC.make_inputs(name, kind), prec, **kw)


class order:
    def __init__(self, lib, which):
        self.lib, self.which = lib, which

    def __enter__(self):
        self.lib.emu_set_order(self.which)

    def __exit__(self, *a):
        self.lib.emu_set_order(0)


@pytest.mark.parametrize("variant", FC.VARIANTS, ids=FC.variant_id)
@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_exact_cases_equal_the_fp64_reference(lib, case, variant):
    name, prec = case
    addend, relu = variant
    for sched, fill in ((0, 0x5A), (1, 0xFF)):
        with order(lib, sched):
            FC.check_exact(run_case(lib, name, prec, "int", addend=addend, relu=relu, fill=fill), name, addend, relu, f"hostemu order{sched}")


@pytest.mark.parametrize("variant", FC.VARIANTS, ids=FC.variant_id)
@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_real_valued_cases_stay_within_the_cap(lib, case, variant):
    name, prec = case
    addend, relu = variant
    sched, fill = (0, 0xFF) if addend == relu else (1, 0x5A)      # both schedules and both fills across the variants
    with order(lib, sched):
        FC.check_real(run_case(lib, name, prec, "normal", addend=addend, relu=relu, fill=fill), name, prec, addend, relu, "hostemu")


def _identity(inp, shift=None):
    """The case's tensors with scale = 1 and shift = 0 (or `shift`)."""
    cout = inp["scale_shift"].shape[1]
    ss = np.stack([np.ones(cout, np.float32), np.zeros(cout, np.float32) if shift is None else shift])
    import torch
    return dict(inp, scale_shift=torch.from_numpy(ss))


def _unfused(lib, stride, dims, inp, prec, bias=None):
    B, Cin, Cout, H, W = dims
    p = FC.PRECISIONS[prec]
    x, w = inp["x"].numpy(), inp["w"].numpy()
    y = np.full(FC.shapes_for(stride, dims)[3], np.nan, dtype=np.float32)
    n = ctypes.c_int64(0)
    P = U.ptr
    if stride == 1:
        ok(lib, lib.dd_convx_workspace_bytes(DD_CONV_3X3, B, Cin, Cout, H, W, p, ctypes.byref(n)))
        ok(lib, lib.dd_convx_forward(DD_CONV_3X3, P(x), P(w), P(y), P(_workspace(n.value, 0x5A)), B, Cin, Cout, H, W, p, None))
    else:
        ok(lib, lib.dd_conv3x3s2_workspace_bytes(B, Cin, Cout, H, W, p, ctypes.byref(n)))
        ok(lib, lib.dd_conv3x3s2_forward(P(x), P(w), P(bias) if bias is not None else None, P(y), P(_workspace(n.value, 0x5A)), B, Cin, Cout, H, W, p,
                                         None))
    return y


@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_the_identity_fold_equals_the_unfused_forward(lib, case):
    """scale = 1, shift = 0, no addend, relu = 0: dd_convx_forward at stride 1, dd_conv3x3s2_forward(bias = NULL) at stride 2 (value equality)."""
    name, prec = case
    stride, dims = FC.SHAPES[name]
    inp = FC.make_inputs(name, "normal")
    got = run(lib, stride, dims, _identity(inp), prec, addend=False, relu=False, fill=0xFF)
    want = _unfused(lib, stride, dims, inp, prec)
    assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("case", [c for c in FC.CASES if FC.SHAPES[c[0]][0] == 2], ids=FC.case_id)
def test_a_bias_as_the_shift_equals_the_biased_strided_forward(lib, case):
    name, prec = case
    stride, dims = FC.SHAPES[name]
    inp = FC.make_inputs(name, "normal")
    bias = np.ascontiguousarray(inp["scale_shift"][1].numpy())
    got = run(lib, stride, dims, _identity(inp, bias), prec, addend=False, relu=False)
    want = _unfused(lib, stride, dims, inp, prec, bias)
    assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("prec", list(FC.PRECISIONS))
@pytest.mark.parametrize("name", FC.PAD_RAGGED)
def test_a_ragged_shape_equals_the_block64_instantiation_on_zero_padded_tensors(lib, name, prec):
    stride = FC.SHAPES[name][0]
    got = run_case(lib, name, prec, "normal", fill=0xFF)
    dims, padded = FC.zero_padded(name)
    want = FC.cut(name, run(lib, stride, dims, padded, prec))
    assert np.isfinite(got).all() and np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("name", ["S1", "Z6"])
def test_two_runs_give_the_same_bits(lib, name):
    a, b = run_case(lib, name, "f16x3", "normal"), run_case(lib, name, "f16x3", "normal", fill=0xFF)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("in_shift", (False, True), ids=["x", "x+shift"])
@pytest.mark.parametrize("addend", FC.ADDEND, ids=["add", "noadd"])
@pytest.mark.parametrize("prec", list(FC.PRECISIONS))
def test_the_relu_keeps_a_nan(lib, prec, addend, in_shift):
    stride, dims = FC.SHAPES[FC.NAN_CASE]
    FC.check_nan(run(lib, stride, dims, FC.nan_inputs(in_shift), prec, addend=addend, relu=True), in_shift, addend, "hostemu")


@pytest.mark.parametrize("absent", FC.FOLD_ABSENT, ids=str)
@pytest.mark.parametrize("C", FC.FOLD_C)
def test_bn_fold_is_within_one_ulp_of_numpy(lib, C, absent):
    v = FC.fold_inputs(C)
    guard = Guarded()
    g, b, m, var, cb = (guard(v[k]) for k in ("gamma", "beta", "mean", "var", "conv_bias"))
    out = guard(np.full((2, C), np.nan, dtype=np.float32))
    P = U.ptr
    ok(lib, lib.dd_bn_fold(None if absent == "gamma" else P(g), None if absent == "beta" else P(b), P(m), P(var), FC.FOLD_EPS,
                           None if absent == "conv_bias" else P(cb), P(out), C, None))
    guard.check()
    FC.check_fold(out, v, absent, "hostemu")


def test_bn_fold_without_statistics_is_the_identity_scale_and_the_bias(lib):
    cb = FC.fold_inputs(72)["conv_bias"]
    out = np.full((2, 72), np.nan, dtype=np.float32)
    ok(lib, lib.dd_bn_fold(None, None, None, None, 0.0, U.ptr(cb), U.ptr(out), 72, None))
    assert np.array_equal(out[0], np.ones(72, np.float32)) and np.array_equal(out[1], cb)
    ok(lib, lib.dd_bn_fold(None, None, None, None, 0.0, None, U.ptr(out), 72, None))
    assert np.array_equal(out[0], np.ones(72, np.float32)) and np.array_equal(out[1], np.zeros(72, np.float32))


def test_support_workspace_and_argument_errors(lib):
    n = ctypes.c_int64(0)
    up = lambda v, s: -(-v // s) * s
    for stride, kstep, pairs in ((1, 32, ((64, 64), (8, 24), (72, 72), (2048, 2048))), (2, 16, ((3, 64), (8, 8), (72, 216), (2048, 2048)))):
        for cin, cout in pairs:
            for prec, halves in ((2, 1), (3, 1), (4, 2)):
                assert lib.dd_conv3x3_affine_supported(stride, cin, cout, prec) == 1
                ok(lib, lib.dd_conv3x3_affine_workspace_bytes(stride, 1, cin, cout, 5, 7, prec, ctypes.byref(n)))
                assert n.value == up(9 * up(cout, 64) * up(cin, kstep) * 2 * halves, 256), (stride, cin, cout, prec)
    assert lib.dd_conv3x3_affine_supported(1, 3, 64, 2) == 0 and lib.dd_conv3x3_affine_supported(2, 3, 64, 2) == 1      # RGB: stride 2 only
    for stride in (0, 3, -1):
        assert lib.dd_conv3x3_affine_supported(stride, 64, 64, 2) == 0
        assert lib.dd_conv3x3_affine_workspace_bytes(stride, 1, 64, 64, 4, 4, 2, ctypes.byref(n)) == DD_ERR_INVALID_ARG
        assert b"stride" in lib.dd_conv_last_error()
    for stride in (1, 2):
        for cin, cout in ((4, 64), (64, 60), (2056, 64), (64, 0)):
            assert lib.dd_conv3x3_affine_supported(stride, cin, cout, 2) == 0
            assert lib.dd_conv3x3_affine_workspace_bytes(stride, 1, cin, cout, 4, 4, 2, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        for prec in (0, 1, 5):
            assert lib.dd_conv3x3_affine_supported(stride, 64, 64, prec) == 0
            assert lib.dd_conv3x3_affine_workspace_bytes(stride, 1, 64, 64, 4, 4, prec, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
            assert b"precision" in lib.dd_conv_last_error()
        assert lib.dd_conv3x3_affine_workspace_bytes(stride, 1, 64, 64, 4, 4, 2, None) == DD_ERR_INVALID_ARG
    x = np.zeros(64 * 16, dtype=np.float32)
    w = np.zeros(64 * 64 * 9, dtype=np.float32)
    ss = np.zeros(2 * 64, dtype=np.float32)
    a = np.zeros(64 * 16, dtype=np.float32)
    o = np.zeros(64 * 16, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    P = U.ptr
    for stride in (1, 2):
        call = lambda *t, s=stride, r=1: lib.dd_conv3x3_affine_forward(P(x), P(w), P(ss), P(a), P(o), P(ws), s, r, *t, None)
        assert call(1, 64, 64, 4, 4, 2) == 0
        assert call(0, 64, 64, 4, 4, 2) == DD_ERR_INVALID_ARG and b"positive" in lib.dd_conv_last_error()
        assert call(1, 64, 64, 0, 4, 2) == DD_ERR_INVALID_ARG
        assert call(1, 4, 64, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 60, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 64, 4, 4, 0) == DD_ERR_UNSUPPORTED and b"precision" in lib.dd_conv_last_error()
        assert call(1, 64, 64, 4, 4, 2, r=2) == DD_ERR_INVALID_ARG and b"relu" in lib.dd_conv_last_error()
    tail = (1, 1, 1, 64, 64, 4, 4, 2, None)
    f = lib.dd_conv3x3_affine_forward
    assert f(None, P(w), P(ss), P(a), P(o), P(ws), *tail) == DD_ERR_INVALID_ARG and b"null" in lib.dd_conv_last_error()
    assert f(P(x), None, P(ss), P(a), P(o), P(ws), *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), None, P(a), P(o), P(ws), *tail) == DD_ERR_INVALID_ARG and b"null" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(ss), P(a), None, P(ws), *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), P(ss), P(a), P(o), None, *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), P(ss), None, P(o), P(ws), *tail) == 0      # the addend is optional
    assert f(P(x), P(w), P(ss), P(a), P(x), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(ss), P(o), P(o), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(o), P(a), P(o), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    fold = lib.dd_bn_fold
    assert fold(None, None, P(ss), P(ss), 1e-5, None, None, 64, None) == DD_ERR_INVALID_ARG
    assert fold(None, None, P(ss), P(a), 1e-5, None, P(o), 0, None) == DD_ERR_INVALID_ARG and b"positive" in lib.dd_conv_last_error()
    assert fold(None, None, P(ss), None, 1e-5, None, P(o), 64, None) == DD_ERR_INVALID_ARG and b"both" in lib.dd_conv_last_error()
    assert fold(None, None, P(ss), P(a), -1.0, None, P(o), 64, None) == DD_ERR_INVALID_ARG and b"eps" in lib.dd_conv_last_error()
    assert fold(None, None, P(o), P(a), 1e-5, None, P(o), 64, None) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
