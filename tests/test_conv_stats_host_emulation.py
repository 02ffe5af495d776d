"""CPU: include/ddepth_conv_stats.h (the training 3x3 forward that emits the BatchNorm statistics from its epilogue) with csrc/dd_conv.hip +
csrc/dd_api_conv.cpp -- and csrc/dd_bn.hip + csrc/dd_api_bn.cpp for dd_bn_stats, the pass it replaces -- compiled for the host on top of
tests/host_emul/hip/hip_runtime.h, built as tests/test_conv_fused_host_emulation.py builds them: the cases of tests/conv_stats_cases.py under
both wave schedules (bit-equal), sentinels around every tensor, a guard behind a workspace of exactly the queried size, and the workspace refilled
with 0x5A or 0xFF bytes before every call."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import conv_fused_cases as FC
import conv_stats_cases as SC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, f) for f in ("dd_conv.hip", "dd_api_conv.cpp", "dd_bn.hip", "dd_api_bn.cpp")] + [os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_conv.h", "dd_conv_kernels.h", "dd_status.h", "dd_bn.h")] + \
    [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", h) for h in ("ddepth.h", "ddepth_conv.h", "ddepth_conv_scaled.h", "ddepth_conv_strided.h", "ddepth_conv_fused.h",
                                                  "ddepth_conv_stats.h", "ddepth_bn.h", "ddepth_bn_add.h")]
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
        out = os.path.join(U.OUT, "conv_stats_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_conv_stats_hostemu.so")
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
    lib.dd_bn_last_error.restype = ctypes.c_char_p
    lib.dd_conv3x3_stats_supported.argtypes = [c_int] * 4
    lib.dd_conv3x3_stats_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_conv3x3_stats_forward.argtypes = [c_vp] * 6 + [c_int] * 7 + [c_vp]
    lib.dd_conv3x3_affine_supported.argtypes = [c_int] * 4
    lib.dd_convx_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_convx_forward.argtypes = [c_int] + [c_vp] * 4 + [c_int] * 6 + [c_vp]
    lib.dd_conv3x3s2_workspace_bytes.argtypes = [c_int] * 6 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_conv3x3s2_forward.argtypes = [c_vp] * 5 + [c_int] * 6 + [c_vp]
    lib.dd_bn_workspace_bytes.argtypes = [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.dd_bn_stats.argtypes = [c_vp] * 3 + [c_int] * 3 + [c_vp]
    lib.emu_set_order.argtypes = [c_int]
    return lib


def ok(lib, rc):
    assert rc == 0, lib.dd_conv_last_error()


SENTINEL = np.float32(-12345.678)
SENTINEL64 = np.float64(-12345.678)


class Guarded:
    """Tensors with sentinel values in front of and behind them, 16 elements each; what lies around a tensor must come back untouched."""

    def __init__(self):
        self.bufs = []

    def __call__(self, a):
        fill = SENTINEL if a.dtype == np.float32 else SENTINEL64
        buf = np.full(a.size + 32, fill, dtype=a.dtype)
        view = buf[16:16 + a.size].reshape(a.shape)
        view[...] = a
        self.bufs.append((buf, a.size, fill))
        return view

    def check(self):
        for buf, size, fill in self.bufs:
            assert (buf[:16] == fill).all() and (buf[16 + size:] == fill).all(), "a kernel wrote outside a tensor"


def _workspace(nbytes, fill):
    raw = np.full(nbytes + 64 + 16, 0x5A, dtype=np.uint8)
    ws = raw[(-raw.ctypes.data) % 16:]      # 16-byte aligned
    ws[:nbytes] = fill
    return ws


def run(lib, stride, dims, inp, prec, bias, fill=0x5A):
    """One dd_conv3x3_stats_forward on numpy memory -> (y, sums).  The workspace has exactly the size the API asks for, is filled with `fill` bytes
    and has a 0x5A guard behind it; every tensor sits between sentinels (item 6 of the contract: y, sums, and behind the workspace)."""
    B, Cin, Cout, H, W = dims
    ys = FC.shapes_for(stride, dims)[3]
    p = SC.PRECISIONS[prec]
    guard = Guarded()
    x, w, bv = (guard(inp[k].numpy()) for k in ("x", "w", "bias"))
    y = guard(np.full(ys, np.nan, dtype=np.float32))
    sums = guard(np.full(2 * Cout + 1, np.nan, dtype=np.float64))
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_conv3x3_stats_workspace_bytes(stride, B, Cin, Cout, H, W, p, ctypes.byref(n)))
    ws = _workspace(n.value, fill)
    P = U.ptr
    ok(lib, lib.dd_conv3x3_stats_forward(P(x), P(w), P(bv) if bias else None, P(y), P(sums), P(ws), stride, B, Cin, Cout, H, W, p, None))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("bias", bv)):
        assert np.array_equal(src, inp[k].numpy(), equal_nan=True), "an input was written"
    return y.copy(), sums.copy()


def run_case(lib, name, prec, kind, bias, **kw):
    stride, dims = SC.SHAPES[name]
    return run(lib, stride, dims, SC.make_inputs(name, kind), prec, bias, **kw)


def unfused(lib, stride, dims, inp, prec, bias):
    B, Cin, Cout, H, W = dims
    p = SC.PRECISIONS[prec]
    x, w, bv = inp["x"].numpy(), inp["w"].numpy(), inp["bias"].numpy()
    y = np.full(FC.shapes_for(stride, dims)[3], np.nan, dtype=np.float32)
    n = ctypes.c_int64(0)
    P = U.ptr
    if stride == 1:
        assert not bias
        ok(lib, lib.dd_convx_workspace_bytes(DD_CONV_3X3, B, Cin, Cout, H, W, p, ctypes.byref(n)))
        ok(lib, lib.dd_convx_forward(DD_CONV_3X3, P(x), P(w), P(y), P(_workspace(n.value, 0x5A)), B, Cin, Cout, H, W, p, None))
    else:
        ok(lib, lib.dd_conv3x3s2_workspace_bytes(B, Cin, Cout, H, W, p, ctypes.byref(n)))
        ok(lib, lib.dd_conv3x3s2_forward(P(x), P(w), P(bv) if bias else None, P(y), P(_workspace(n.value, 0x5A)), B, Cin, Cout, H, W, p, None))
    return y


def bn_stats(lib, y):
    B, C, H, W = y.shape
    n = ctypes.c_int64(0)
    assert lib.dd_bn_workspace_bytes(B, C, H * W, ctypes.byref(n)) == 0, lib.dd_bn_last_error()
    sums = np.full(2 * C + 1, np.nan, dtype=np.float64)
    yc = np.ascontiguousarray(y)
    assert lib.dd_bn_stats(U.ptr(yc), U.ptr(sums), U.ptr(_workspace(n.value, 0x5A)), B, C, H * W, None) == 0, lib.dd_bn_last_error()
    return sums


class order:
    def __init__(self, lib, which):
        self.lib, self.which = lib, which

    def __enter__(self):
        self.lib.emu_set_order(self.which)

    def __exit__(self, *a):
        self.lib.emu_set_order(0)


def both_orders(lib, name, prec, kind, bias):
    """(y, sums) of the case, run under both wave schedules and both workspace fills: bit-equal."""
    with order(lib, 0):
        y0, s0 = run_case(lib, name, prec, kind, bias, fill=0x5A)
    with order(lib, 1):
        y1, s1 = run_case(lib, name, prec, kind, bias, fill=0xFF)
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64)), "the wave schedule shows"
    return y0, s0


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_exact_data_gives_the_unfused_y_and_the_integer_sums(lib, case):
    name, bias, prec = case
    stride, dims = SC.SHAPES[name]
    y, sums = both_orders(lib, name, prec, "int", bias)
    SC.check_y(y, unfused(lib, stride, dims, SC.make_inputs(name, "int"), prec, bias), f"hostemu {SC.case_id(case)}")
    SC.check_exact(sums, y, name, bn_stats(lib, y), "hostemu")


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_real_valued_data_gives_the_unfused_y_and_sums_within_the_fsum_bound(lib, case):
    name, bias, prec = case
    stride, dims = SC.SHAPES[name]
    y, sums = both_orders(lib, name, prec, "normal", bias)
    SC.check_y(y, unfused(lib, stride, dims, SC.make_inputs(name, "normal"), prec, bias), f"hostemu {SC.case_id(case)}")
    SC.check_real(sums, y, name, "hostemu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
@pytest.mark.parametrize("name", (SC.NAN_WEIGHT_CASE, SC.NAN_BIAS_CASE))
def test_a_nan_stays_in_its_channel(lib, name, prec):
    stride, dims = SC.SHAPES[name]
    bias = name == SC.NAN_BIAS_CASE
    _, clean = run_case(lib, name, prec, "normal", bias)
    _, sums = run(lib, stride, dims, SC.nan_inputs(name), prec, bias, fill=0xFF)
    SC.check_nan(sums, clean, name, "hostemu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
@pytest.mark.parametrize("name", SC.PAD_RAGGED)
def test_a_ragged_shape_gives_the_sums_of_the_block64_instantiation_on_zero_padded_tensors(lib, name, prec):
    stride, (B, Cin, Cout, H, W) = SC.SHAPES[name]
    bias = stride == 2
    y, got = run_case(lib, name, prec, "int", bias, fill=0xFF)
    dims, padded = SC.zero_padded(name)
    yp, sp = run(lib, stride, dims, padded, prec, bias)
    assert np.array_equal(y, yp[:, :Cout])
    assert np.array_equal(got.view(np.uint64), SC.cut_sums(sp, dims[2], Cout).view(np.uint64))


def test_support_workspace_and_argument_errors(lib):
    n = ctypes.c_int64(0)
    up = lambda v, s: -(-v // s) * s
    for stride, kstep, pairs in ((1, 32, ((64, 64), (8, 24), (72, 72), (2048, 2048))), (2, 16, ((3, 64), (8, 8), (72, 216), (2048, 2048)))):
        for cin, cout in pairs:
            for prec, halves in ((2, 1), (3, 1), (4, 2)):
                assert lib.dd_conv3x3_stats_supported(stride, cin, cout, prec) == 1
                ok(lib, lib.dd_conv3x3_stats_workspace_bytes(stride, 3, cin, cout, 9, 70, prec, ctypes.byref(n)))
                ho, wo = (5, 35) if stride == 2 else (9, 70)
                tiles = up(ho, 4) // 4 * (up(wo, 32) // 32)
                assert n.value == up(9 * up(cout, 64) * up(cin, kstep) * 2 * halves, 256) + up(cout * 3 * tiles * 16, 256), (stride, cin, cout, prec)
    for stride in (0, 1, 2, 3):
        for cin, cout in ((64, 64), (3, 64), (4, 64), (64, 60), (2056, 64)):
            for prec in (0, 1, 2, 3, 4, 5):
                assert lib.dd_conv3x3_stats_supported(stride, cin, cout, prec) == lib.dd_conv3x3_affine_supported(stride, cin, cout, prec)
    for stride in (0, 3, -1):
        assert lib.dd_conv3x3_stats_workspace_bytes(stride, 1, 64, 64, 4, 4, 2, ctypes.byref(n)) == DD_ERR_INVALID_ARG
        assert b"stride" in lib.dd_conv_last_error()
    for stride in (1, 2):
        assert lib.dd_conv3x3_stats_workspace_bytes(stride, 1, 4, 64, 4, 4, 2, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        assert lib.dd_conv3x3_stats_workspace_bytes(stride, 1, 64, 64, 4, 4, 0, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        assert b"precision" in lib.dd_conv_last_error()
        assert lib.dd_conv3x3_stats_workspace_bytes(stride, 1, 64, 64, 4, 4, 2, None) == DD_ERR_INVALID_ARG
        assert lib.dd_conv3x3_stats_workspace_bytes(stride, 0, 64, 64, 4, 4, 2, ctypes.byref(n)) == DD_ERR_INVALID_ARG
    x = np.zeros(64 * 16, dtype=np.float32)
    w = np.zeros(64 * 64 * 9, dtype=np.float32)
    bv = np.zeros(64, dtype=np.float32)
    o = np.zeros(64 * 16, dtype=np.float32)
    s = np.zeros(129, dtype=np.float64)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    P = U.ptr
    f = lib.dd_conv3x3_stats_forward
    for stride in (1, 2):
        call = lambda *t, st=stride: f(P(x), P(w), P(bv), P(o), P(s), P(ws), st, *t, None)
        assert call(1, 64, 64, 4, 4, 2) == 0
        assert call(0, 64, 64, 4, 4, 2) == DD_ERR_INVALID_ARG and b"positive" in lib.dd_conv_last_error()
        assert call(1, 64, 64, 0, 4, 2) == DD_ERR_INVALID_ARG
        assert call(1, 64, 64, 4, -1, 2) == DD_ERR_INVALID_ARG
        assert call(1, 4, 64, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 60, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 64, 4, 4, 0) == DD_ERR_UNSUPPORTED and b"precision" in lib.dd_conv_last_error()
    tail = (1, 1, 64, 64, 4, 4, 2, None)
    assert f(None, P(w), P(bv), P(o), P(s), P(ws), *tail) == DD_ERR_INVALID_ARG and b"null" in lib.dd_conv_last_error()
    assert f(P(x), None, P(bv), P(o), P(s), P(ws), *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), P(bv), None, P(s), P(ws), *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), P(bv), P(o), None, P(ws), *tail) == DD_ERR_INVALID_ARG and b"null" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(bv), P(o), P(s), None, *tail) == DD_ERR_INVALID_ARG
    assert f(P(x), P(w), None, P(o), P(s), P(ws), *tail) == 0      # the bias is optional
    assert f(P(x), P(w), P(bv), P(x), P(s), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(o), P(o), P(s), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    assert f(P(x), P(w), P(bv), P(s), P(s), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
