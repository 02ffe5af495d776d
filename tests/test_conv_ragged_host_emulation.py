"""CPU: the extended channel range of include/ddepth_conv.h (dd_convx_*: multiples of 8 in 8..2048) with csrc/dd_conv.hip + csrc/dd_api_conv.cpp
compiled for the host on top of tests/host_emul/hip/hip_runtime.h, as tests/test_conv_host_emulation.py does for the block-64 contract: the
cases of tests/conv_ragged_cases.py against the fp64 references under both wave schedules, sentinels around every tensor, a guard behind the
workspace, and the workspace filled with 0x5A or with 0xFF bytes before EVERY call -- 0xFF is a NaN in each operand type (bf16, f16, fp32), so a
pad region of the packed weights that is read without having been written shows up as NaN.  Beyond the references: the zero-padding identity
(a ragged shape equals the block-64 operator on tensors zero-padded to 128 channels), the superset identity (a block-64 shape through
dd_convx_* gives the bits of the old entry points), repeatability, and both channel contracts side by side."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import conv_cases as CC
import conv_pw_cases as PC
import conv_ragged_cases as RC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_conv.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"), os.path.join(U.ROOT, "include", "ddepth_conv.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4
OLD = {RC.CONV: ("dd_conv3x3_forward", "dd_conv3x3_backward_data", "dd_conv3x3_backward_weight"),
       RC.DECONV: ("dd_deconv2x2_forward", "dd_deconv2x2_backward_data", "dd_deconv2x2_backward_weight"),
       RC.CONV1X1: ("dd_conv1x1_forward", "dd_conv1x1_backward_data", "dd_conv1x1_backward_weight")}
NEW = ("dd_convx_forward", "dd_convx_backward_data", "dd_convx_backward_weight")


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
        out = os.path.join(U.OUT, "conv_" + hsh.hexdigest()[:12])      # (the build tests/test_conv_host_emulation.py makes: shared)
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
    for q in ("dd_conv_supported", "dd_convx_supported"):
        getattr(lib, q).argtypes = [c_int] * 4
    for q in ("dd_conv_workspace_bytes", "dd_convx_workspace_bytes"):
        getattr(lib, q).argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    for names in OLD.values():
        for n in names:
            getattr(lib, n).argtypes = [c_vp] * 4 + [c_int] * 6 + [c_vp]
    for n in NEW:
        getattr(lib, n).argtypes = [c_int] + [c_vp] * 4 + [c_int] * 6 + [c_vp]
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


def run_three(lib, op, dims, inp, prec, api="x", fill=0x5A):
    """Forward, data gradient and weight gradient on numpy memory -> dict of KEYS.  api "x": dd_convx_*, "old": the block-64 entry points.
    The workspace has exactly the size the API asks for, is refilled with `fill` bytes before each call, and has a 0x5A guard behind it."""
    B, Cin, Cout, H, W = dims
    xs, ws_, ys = RC.shapes_for(op, dims)
    p = RC.PRECISIONS[prec]
    guard = Guarded()
    x, w, gy = guard(inp["x"].numpy()), guard(inp["w"].numpy()), guard(inp["grad_y"].numpy())
    y, gx, gw = (guard(np.full(s, np.nan, dtype=np.float32)) for s in (ys, xs, ws_))
    n = ctypes.c_int64(0)
    if api == "x":
        ok(lib, lib.dd_convx_workspace_bytes(op, B, Cin, Cout, H, W, p, ctypes.byref(n)))
        calls = [lambda *a, f=getattr(lib, f): f(op, *a) for f in NEW]
    else:
        ok(lib, lib.dd_conv_workspace_bytes(op, B, Cin, Cout, H, W, p, ctypes.byref(n)))
        calls = [getattr(lib, f) for f in OLD[op]]
    raw = np.full(n.value + 64 + 16, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16      # the workspace is 16-byte aligned
    ws = raw[off:]
    tail = (B, Cin, Cout, H, W, p, None)
    for call, args in zip(calls, ((x, w, y), (gy, w, gx), (x, gy, gw))):
        ws[:n.value] = fill
        ok(lib, call(*(U.ptr(a) for a in args), U.ptr(ws), *tail))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("grad_y", gy)):
        assert np.array_equal(src, inp[k].numpy()), "an input was written"
    return {"y": y.copy(), "grad_x": gx.copy(), "grad_w": gw.copy()}


def run_case(lib, name, prec, kind, **kw):
    op, dims = RC.SHAPES[name]
    return run_three(lib, op, dims, RC.make_inputs(name, kind), prec, **kw)


@pytest.mark.parametrize("order,fill", [(0, 0x5A), (1, 0xFF)], ids=["order0-5A", "order1-FF"])
@pytest.mark.parametrize("case", RC.EXACT + RC.WIDE, ids=RC.case_id)
def test_exact_cases_equal_the_fp64_reference(lib, case, order, fill):
    name, prec, kind = case
    lib.emu_set_order(order)
    try:
        RC.check_exact(run_case(lib, name, prec, kind, fill=fill), name, kind, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("name", ["R1", "R5", "T1", "P1", "P2"])
def test_the_other_pairing_of_schedule_and_fill(lib, name):
    """The exact cases above run schedule 0 on a 0x5A workspace and schedule 1 on a 0xFF one; here the other two pairings, in the split mode
    (both halves of the packed image) at the shapes with the smallest channel counts and the largest pad share."""
    for order, fill in ((0, 0xFF), (1, 0x5A)):
        lib.emu_set_order(order)
        try:
            RC.check_exact(run_case(lib, name, "f16x3", "int", fill=fill), name, "int", "hostemu")
        finally:
            lib.emu_set_order(0)


@pytest.mark.parametrize("order,fill", [(0, 0xFF), (1, 0x5A)], ids=["order0-FF", "order1-5A"])
@pytest.mark.parametrize("case", RC.REAL, ids=RC.case_id)
def test_real_valued_cases_stay_within_the_cap(lib, case, order, fill):
    name, prec, _ = case
    lib.emu_set_order(order)
    try:
        RC.check_real(run_case(lib, name, prec, "normal", fill=fill), name, prec, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("prec", list(RC.PRECISIONS))
@pytest.mark.parametrize("name", RC.PADDED)
def test_a_ragged_shape_equals_the_block64_operator_on_zero_padded_tensors(lib, name, prec):
    """No tolerance: the guarded kernels add the same terms in the same order, and the terms of the padding are zeros."""
    op, _ = RC.SHAPES[name]
    got = run_case(lib, name, prec, "normal", fill=0xFF)
    dims, padded = RC.zero_padded(name)
    want = RC.cut(name, run_three(lib, op, dims, padded, prec, api="old"))
    for k in RC.KEYS:
        assert np.isfinite(got[k]).all() and got[k].shape == want[k].shape
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def _block64_cases():
    for name in ("S1", "D1"):
        op, dims = CC.SHAPES[name]
        yield name, op, dims, CC.make_inputs(name, "normal")
    yield "P1", RC.CONV1X1, PC.SHAPES["P1"], PC.make_inputs("P1", "normal")


@pytest.mark.parametrize("prec", ["bf16", "f16x3"])
def test_a_block64_shape_gives_the_same_bits_through_both_entry_points(lib, prec):
    for name, op, dims, inp in _block64_cases():
        a, b = run_three(lib, op, dims, inp, prec, api="x"), run_three(lib, op, dims, inp, prec, api="old")
        n_x, n_old = ctypes.c_int64(0), ctypes.c_int64(0)
        ok(lib, lib.dd_convx_workspace_bytes(op, *dims, RC.PRECISIONS[prec], ctypes.byref(n_x)))
        ok(lib, lib.dd_conv_workspace_bytes(op, *dims, RC.PRECISIONS[prec], ctypes.byref(n_old)))
        assert n_x.value == n_old.value, name
        for k in RC.KEYS:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize("name", ["R1", "T2", "P1"])
def test_two_runs_give_the_same_bits(lib, name):
    a, b = run_case(lib, name, "f16x3", "normal"), run_case(lib, name, "f16x3", "normal", fill=0xFF)
    for k in RC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_the_workspace_covers_the_padded_weight_image(lib):
    """taps * (N rounded up to 64) * (K rounded up to the K step) halfs, the larger direction, twice in the split mode (csrc/dd_conv.h:
    packed_halfs).  One pixel, so the weight gradient's partials (one split of taps * Cin * Cout floats) are known too."""
    up = lambda n, s: -(-n // s) * s
    n = ctypes.c_int64(0)
    for op, cin, cout in ((0, 72, 72), (0, 8, 24), (0, 216, 256), (1, 72, 72), (1, 216, 88), (2, 72, 72), (2, 2048, 72), (0, 2048, 1536)):
        for prec, halves in ((2, 1), (4, 2)):
            ok(lib, lib.dd_convx_workspace_bytes(op, 1, cin, cout, 1, 1, prec, ctypes.byref(n)))
            if op == 0:
                packed, taps = 9 * max(up(cout, 64) * up(cin, 32), up(cin, 64) * up(cout, 32)), 9
            elif op == 1:
                packed, taps = max(up(4 * cout, 64) * up(cin, 32), 4 * up(cin, 64) * up(cout, 16)), 4
            else:
                packed, taps = max(up(cout, 64) * up(cin, 32), up(cin, 64) * up(cout, 32)), 1
            assert n.value == up(max(packed * 2 * halves, taps * cin * cout * 4), 256), (op, cin, cout, prec)


def test_both_channel_contracts(lib):
    n = ctypes.c_int64(0)
    for op in (0, 1, 2):
        for cin, cout in ((8, 8), (216, 256), (2048, 1536), (64, 64)):
            for prec in (2, 3, 4):
                assert lib.dd_convx_supported(op, cin, cout, prec) == 1
        for c in (4, 12, 2056, 0, -8):
            for cin, cout in ((c, 64), (64, c)):
                assert lib.dd_convx_supported(op, cin, cout, 2) == 0
                assert lib.dd_convx_workspace_bytes(op, 1, cin, cout, 4, 4, 2, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
                assert b"multiples of 8 in 8..2048" in lib.dd_conv_last_error()
        for prec in (0, 1, 5):
            assert lib.dd_convx_supported(op, 72, 72, prec) == 0
            assert lib.dd_convx_workspace_bytes(op, 1, 72, 72, 4, 4, prec, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
            assert b"precision" in lib.dd_conv_last_error() and b"unsupported" in lib.dd_conv_last_error()
    for op in (3, 7, -1):
        assert lib.dd_convx_supported(op, 72, 72, 2) == 0
        assert lib.dd_convx_workspace_bytes(op, 1, 72, 72, 4, 4, 2, ctypes.byref(n)) == DD_ERR_INVALID_ARG
        assert b"dd_conv_op" in lib.dd_conv_last_error()
    x = np.zeros(72 * 4, dtype=np.float32)
    w = np.zeros(72 * 72 * 9, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    for f in NEW:
        call = getattr(lib, f)
        assert call(0, U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 12, 72, 2, 2, 2, None) == DD_ERR_UNSUPPORTED
        assert b"multiples of 8" in lib.dd_conv_last_error()
        assert call(0, U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 72, 2056, 2, 2, 2, None) == DD_ERR_UNSUPPORTED
        assert call(0, U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 72, 72, 2, 2, 1, None) == DD_ERR_UNSUPPORTED
        assert b"precision" in lib.dd_conv_last_error()
        assert call(5, U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 72, 72, 2, 2, 2, None) == DD_ERR_INVALID_ARG
        assert call(0, None, None, None, None, 1, 72, 72, 2, 2, 2, None) != 0 and b"null" in lib.dd_conv_last_error()
        assert call(0, U.ptr(x), U.ptr(w), U.ptr(x), U.ptr(ws), 1, 72, 72, 2, 2, 2, None) != 0 and b"alias" in lib.dd_conv_last_error()
        assert call(0, U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 72, 72, 0, 2, 2, None) != 0 and b"positive" in lib.dd_conv_last_error()
    # the block-64 contract is still its own: the old functions refuse what only the extended range takes
    assert lib.dd_conv_supported(0, 216, 256, 2) == 0 and lib.dd_conv_supported(2, 2048, 1536, 2) == 0 and lib.dd_conv_supported(0, 8, 8, 2) == 0
    assert lib.dd_conv_workspace_bytes(0, 1, 216, 256, 4, 4, 2, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
    assert b"multiples of 64 in 64..1536" in lib.dd_conv_last_error()
    for names in OLD.values():
        for f in names:
            assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 216, 64, 2, 2, 2, None) == DD_ERR_UNSUPPORTED
            assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 2048, 64, 2, 2, 2, None) == DD_ERR_UNSUPPORTED
            assert b"multiples of 64" in lib.dd_conv_last_error()
