"""CPU: include/ddepth_conv_strided.h (3x3 stride 2 pad 1, optional bias) with csrc/dd_conv.hip + csrc/dd_api_conv.cpp compiled for the host on top
of tests/host_emul/hip/hip_runtime.h, built as tests/test_conv_ragged_host_emulation.py builds them: the cases of tests/conv_strided_cases.py
against the fp64 references under both wave schedules, sentinels around every tensor, a guard behind a workspace of exactly the queried size,
and the workspace refilled with 0x5A or 0xFF bytes before EVERY call (0xFF is a NaN in each operand type, so a pad region of the packed weights
that is read without having been written shows up as NaN).  Beyond the references: the scaled rules, repeatability, the two zero-padding
identities and the argument errors."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import conv_strided_cases as ZC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_conv.h", "dd_conv_kernels.h", "dd_status.h")] + \
    [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", h) for h in ("ddepth.h", "ddepth_conv.h", "ddepth_conv_scaled.h", "ddepth_conv_strided.h")]
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4


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
        out = os.path.join(U.OUT, "conv_strided_" + hsh.hexdigest()[:12])
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
    lib.dd_conv3x3s2_supported.argtypes = [c_int] * 3
    lib.dd_conv3x3s2_workspace_bytes.argtypes = [c_int] * 6 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_conv3x3s2_forward.argtypes = [c_vp] * 5 + [c_int] * 6 + [c_vp]
    lib.dd_conv3x3s2_backward_data.argtypes = [c_vp] * 5 + [c_int] * 6 + [c_vp]
    lib.dd_conv3x3s2_backward_weight.argtypes = [c_vp] * 6 + [c_int] * 6 + [c_vp]
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


def run_three(lib, dims, inp, prec, bias=True, fill=0x5A, grad_y=None, scaled=False, dirs=(0, 1, 2)):
    """Forward, data gradient and weight (+ bias) gradient on numpy memory -> dict of ZC.KEYS (grad_bias None without a bias).  grad_y replaces the
    case's; scaled: the gradients run with the scale pair of the rule, built in numpy.  The workspace has exactly the size the API asks for, is
    refilled with `fill` bytes before each call, and has a 0x5A guard behind it."""
    B, Cin, Cout, H, W = dims
    xs, ws_, bs, ys = ZC.shapes_for(dims)
    p = ZC.PRECISIONS[prec]
    gy0 = inp["grad_y"].numpy() if grad_y is None else grad_y
    guard = Guarded()
    x, w, b, gy = guard(inp["x"].numpy()), guard(inp["w"].numpy()), guard(inp["bias"].numpy()), guard(gy0)
    y, gx, gw, gb = (guard(np.full(s, np.nan, dtype=np.float32)) for s in (ys, xs, ws_, bs))
    scale = guard(ZC.scale_words(gy0).view(np.float32)) if scaled else None
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_conv3x3s2_workspace_bytes(B, Cin, Cout, H, W, p, ctypes.byref(n)))
    raw = np.full(n.value + 64 + 16, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16      # the workspace is 16-byte aligned
    ws = raw[off:]
    tail = (B, Cin, Cout, H, W, p, None)
    P = U.ptr
    if 0 in dirs:
        ws[:n.value] = fill
        ok(lib, lib.dd_conv3x3s2_forward(P(x), P(w), P(b) if bias else None, P(y), P(ws), *tail))
    if 1 in dirs:
        ws[:n.value] = fill
        ok(lib, lib.dd_conv3x3s2_backward_data(P(gy), P(w), P(gx), P(ws), P(scale), *tail))
    if 2 in dirs:
        ws[:n.value] = fill
        ok(lib, lib.dd_conv3x3s2_backward_weight(P(x), P(gy), P(gw), P(gb) if bias else None, P(ws), P(scale), *tail))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("bias", b)):
        assert np.array_equal(src, inp[k].numpy()), "an input was written"
    assert np.array_equal(gy, gy0), "an input was written"
    if not bias:
        assert np.isnan(gb).all(), "grad_bias was written though NULL was passed"
    return {"y": y.copy() if 0 in dirs else None, "grad_x": gx.copy() if 1 in dirs else None, "grad_w": gw.copy() if 2 in dirs else None,
            "grad_bias": gb.copy() if bias and 2 in dirs else None}


def run_case(lib, name, prec, kind, **kw):
    return run_three(lib, ZC.SHAPES[name], ZC.make_inputs(name, kind), prec, **kw)


class order:
    def __init__(self, lib, which):
        self.lib, self.which = lib, which

    def __enter__(self):
        self.lib.emu_set_order(self.which)

    def __exit__(self, *a):
        self.lib.emu_set_order(0)


@pytest.mark.parametrize("sched,fill,bias", [(0, 0x5A, True), (1, 0xFF, False)], ids=["order0-5A-bias", "order1-FF-nobias"])
@pytest.mark.parametrize("case", ZC.EXACT + ZC.WIDE, ids=ZC.case_id)
def test_exact_cases_equal_the_fp64_reference(lib, case, sched, fill, bias):
    name, prec, kind = case
    with order(lib, sched):
        ZC.check_exact(run_case(lib, name, prec, kind, bias=bias, fill=fill), name, kind, bias, "hostemu")


@pytest.mark.parametrize("name", ["Z4", "Z5", "Z6"])
def test_the_other_pairing_of_schedule_fill_and_bias(lib, name):
    """The exact cases above pair schedule 0 with 0x5A and a bias, schedule 1 with 0xFF and none; here the other pairings in the split mode at the
    shapes with the largest pad share of the packed image."""
    for sched, fill, bias in ((0, 0xFF, False), (1, 0x5A, True)):
        with order(lib, sched):
            ZC.check_exact(run_case(lib, name, "f16x3", "int", bias=bias, fill=fill), name, "int", bias, "hostemu")


@pytest.mark.parametrize("sched,fill,bias", [(0, 0xFF, True), (1, 0x5A, False)], ids=["order0-FF-bias", "order1-5A-nobias"])
@pytest.mark.parametrize("case", ZC.REAL, ids=ZC.case_id)
def test_real_valued_cases_stay_within_the_cap(lib, case, sched, fill, bias):
    name, prec, _ = case
    with order(lib, sched):
        ZC.check_real(run_case(lib, name, prec, "normal", bias=bias, fill=fill), name, prec, bias, "hostemu")


@pytest.mark.parametrize("prec", ["f16", "f16x3"])
@pytest.mark.parametrize("name", ZC.EQUIVARIANCE)
def test_scaled_gradients_are_equivariant_under_powers_of_two(lib, name, prec):
    gy = ZC.make_inputs(name, "normal")["grad_y"].numpy()
    base = run_case(lib, name, prec, "normal", scaled=True, dirs=(1, 2), fill=0xFF)
    bad = []
    for k in ZC.K_SMALL:
        got = run_case(lib, name, prec, "normal", grad_y=ZC.small(gy, k), scaled=True, dirs=(1, 2))
        bad += [(k,) + b for b in ZC.check_equivariant(got, base, k, f"hostemu {name} {prec}")]
    assert not bad, bad


@pytest.mark.parametrize("prec", list(ZC.PRECISIONS))
@pytest.mark.parametrize("name", ZC.SCALED_EXACT)
def test_scaled_integer_gradients_times_two_to_the_minus_20_are_exact(lib, name, prec):
    gy = ZC.small(ZC.make_inputs(name, "int")["grad_y"].numpy(), -20)
    got = run_case(lib, name, prec, "int", grad_y=gy, scaled=True, dirs=(1, 2), fill=0xFF)
    ZC.check_exact(got, name, "int", True, "hostemu scaled", scale_exp=-20)


def test_bf16_ignores_the_values_of_the_scale_pair(lib):
    a = run_case(lib, "Z6", "bf16", "normal", scaled=True, dirs=(1, 2))
    b = run_case(lib, "Z6", "bf16", "normal", scaled=False, dirs=(1, 2))
    for k in ZC.GRAD_KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("name", ["Z6", "Z5"])
def test_two_runs_give_the_same_bits(lib, name):
    a, b = run_case(lib, name, "f16x3", "normal"), run_case(lib, name, "f16x3", "normal", fill=0xFF)
    for k in ZC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _same(got, want):
    for k in ZC.KEYS:
        assert np.isfinite(got[k]).all() and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("prec", list(ZC.PRECISIONS))
def test_a_block64_shape_equals_itself_zero_padded_to_the_next_multiple_of_64(lib, prec):
    """No tolerance: the padding's terms are zeros, the order of the others is the same."""
    B, Cin, Cout, H, W = ZC.SHAPES[ZC.PAD64]
    got = run_case(lib, ZC.PAD64, prec, "normal", fill=0xFF)
    dims, padded = ZC.zero_padded(ZC.PAD64, Cin + 64, Cout + 64)
    _same(got, ZC.cut(ZC.PAD64, run_three(lib, dims, padded, prec)))


@pytest.mark.parametrize("prec", list(ZC.PRECISIONS))
def test_a_ragged_shape_equals_the_block64_instantiation_on_zero_padded_tensors(lib, prec):
    up = lambda n: -(-n // 64) * 64
    B, Cin, Cout, H, W = ZC.SHAPES[ZC.PAD_RAGGED]
    got = run_case(lib, ZC.PAD_RAGGED, prec, "normal", fill=0xFF)
    dims, padded = ZC.zero_padded(ZC.PAD_RAGGED, up(Cin), up(Cout))
    _same(got, ZC.cut(ZC.PAD_RAGGED, run_three(lib, dims, padded, prec)))


def test_the_weight_gradient_of_z7_runs_many_splits_with_a_partial_last_one(lib):
    """40 x 70 outputs in tiles of 2 x 32: 3 * 20 * 3 = 180 tiles = 22 splits of 8 and one of 4; the workspace is those partials."""
    n = ctypes.c_int64(0)
    B, Cin, Cout, H, W = ZC.SHAPES["Z7"]
    ok(lib, lib.dd_conv3x3s2_workspace_bytes(B, Cin, Cout, H, W, 2, ctypes.byref(n)))
    assert n.value == 23 * 9 * Cin * Cout * 4


def test_support_workspace_and_argument_errors(lib):
    n = ctypes.c_int64(0)
    up = lambda v, s: -(-v // s) * s
    for cin, cout in ((3, 64), (8, 8), (64, 128), (72, 216), (2048, 2048), (256, 512)):
        for prec, halves in ((2, 1), (3, 1), (4, 2)):
            assert lib.dd_conv3x3s2_supported(cin, cout, prec) == 1
            ok(lib, lib.dd_conv3x3s2_workspace_bytes(1, cin, cout, 1, 1, prec, ctypes.byref(n)))
            packed = 9 * max(up(cout, 64) * up(cin, 16), up(cin, 64) * up(cout, 32))      # forward K step 16, data gradient 32
            assert n.value == up(max(packed * 2 * halves, 9 * cin * cout * 4), 256), (cin, cout, prec)
    for cin, cout in ((4, 64), (0, 64), (-8, 64), (12, 64), (2056, 64), (64, 3), (64, 60), (64, 0), (64, 2056), (6, 64)):
        assert lib.dd_conv3x3s2_supported(cin, cout, 2) == 0
        assert lib.dd_conv3x3s2_workspace_bytes(1, cin, cout, 4, 4, 2, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        assert b"Cin 3 or a multiple of 8" in lib.dd_conv_last_error()
    for prec in (0, 1, 5):      # fp32 and the others
        assert lib.dd_conv3x3s2_supported(64, 64, prec) == 0
        assert lib.dd_conv3x3s2_workspace_bytes(1, 64, 64, 4, 4, prec, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        assert b"precision" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_workspace_bytes(1, 64, 64, 4, 4, 2, None) == DD_ERR_INVALID_ARG
    x = np.zeros(64 * 16, dtype=np.float32)
    w = np.zeros(64 * 64 * 9, dtype=np.float32)
    o = np.zeros(64 * 64 * 9, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    P = U.ptr
    calls = [lambda *t: lib.dd_conv3x3s2_forward(P(x), P(w), None, P(o), P(ws), *t, None),
             lambda *t: lib.dd_conv3x3s2_backward_data(P(x), P(w), P(o), P(ws), None, *t, None),
             lambda *t: lib.dd_conv3x3s2_backward_weight(P(x), P(w), P(o), None, P(ws), None, *t, None)]
    for call in calls:
        assert call(1, 64, 64, 4, 4, 2) == 0
        assert call(0, 64, 64, 4, 4, 2) == DD_ERR_INVALID_ARG and b"positive" in lib.dd_conv_last_error()
        assert call(1, 64, 64, 0, 4, 2) == DD_ERR_INVALID_ARG
        assert call(1, 4, 64, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 60, 4, 4, 2) == DD_ERR_UNSUPPORTED
        assert call(1, 64, 64, 4, 4, 0) == DD_ERR_UNSUPPORTED and b"precision" in lib.dd_conv_last_error()
    tail = (1, 64, 64, 4, 4, 2, None)
    assert lib.dd_conv3x3s2_forward(None, P(w), None, P(o), P(ws), *tail) == DD_ERR_INVALID_ARG and b"null" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_forward(P(x), P(w), None, None, P(ws), *tail) == DD_ERR_INVALID_ARG
    assert lib.dd_conv3x3s2_forward(P(x), P(w), None, P(o), None, *tail) == DD_ERR_INVALID_ARG
    assert lib.dd_conv3x3s2_forward(P(x), P(w), None, P(x), P(ws), *tail) == DD_ERR_INVALID_ARG and b"alias" in lib.dd_conv_last_error()
    assert lib.dd_conv3x3s2_backward_data(P(x), None, P(o), P(ws), None, *tail) == DD_ERR_INVALID_ARG
    assert lib.dd_conv3x3s2_backward_weight(P(x), None, P(o), None, P(ws), None, *tail) == DD_ERR_INVALID_ARG
    assert lib.dd_conv3x3s2_backward_weight(P(x), P(w), P(o), P(o), P(ws), None, *tail) == DD_ERR_INVALID_ARG
