"""CPU: include/swin/ddepth_linear.h with csrc/dd_linear.hip + csrc/dd_api_linear.cpp compiled for the host on top of
tests/host_emul/hip/hip_runtime.h, built as tests/test_swin_host_emulation.py builds its units: the cases of tests/linear_cases.py under both wave
schedules (bit-equal), sentinels around every tensor and the packed image, no host-blocking call, and the argument checks."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import hostemu_util as U
import linear_cases as LC

UNITS = [os.path.join(U.CSRC, f) for f in ("dd_linear.hip", "dd_api_linear.cpp")] + [os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_linear.h", "dd_status.h")] + [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", "ddepth.h"), os.path.join(U.ROOT, "include", "swin", "ddepth_linear.h")]
SENTINEL = np.float32(-12345.678)
BIG = ("big-1", "big", "big+1")      # 256 .. 320 workgroups each: one schedule, their own tests
EMU_SHAPES = tuple(n for n in LC.SHAPES if n not in BIG)


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
        out = os.path.join(U.OUT, "linear_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_linear_hostemu.so")
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
    c_int, c_vp, c_ll = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    lib.dd_linear_last_error.restype = ctypes.c_char_p
    lib.dd_linear_supported.argtypes = [c_int] * 4
    lib.dd_linear_packed_bytes.argtypes = [c_int] * 3 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_linear_pack.argtypes = [c_vp, c_vp] + [c_int] * 3 + [c_vp]
    lib.dd_linear_forward.argtypes = [c_vp] * 5 + [c_ll] + [c_int] * 4 + [c_vp]
    lib.emu_set_order.argtypes = [c_int]
    lib.emu_blocking_calls.restype = ctypes.c_ulong
    return lib


class Guarded:
    """Tensors with sentinel values in front of and behind them, 16 elements each (64 bytes: the 16-byte alignment stays)."""

    def __init__(self):
        self.bufs = []

    def __call__(self, a):
        raw = np.full(a.size + 32 + 4, SENTINEL, dtype=np.float32)
        off = ((-raw.ctypes.data) % 16) // 4
        buf = raw[off:off + a.size + 32]
        view = buf[16:16 + a.size].reshape(a.shape)
        view[...] = a
        self.bufs.append((buf, a.size))
        return view

    def check(self):
        for buf, size in self.bufs:
            assert (buf[:16] == SENTINEL).all() and (buf[16 + size:] == SENTINEL).all(), "a kernel wrote outside a tensor"


def packed_bytes(lib, K, N, prec):
    n = ctypes.c_int64(0)
    assert lib.dd_linear_packed_bytes(K, N, LC.PRECISIONS[prec], ctypes.byref(n)) == 0, lib.dd_linear_last_error()
    return int(n.value)


def run(lib, x, w, bias, addend, act, prec):
    (M, K), N = x.shape, w.shape[0]
    guard = Guarded()
    gx, gw = guard(x), guard(w)
    gb = guard(bias) if bias is not None else None
    ga = guard(addend) if addend is not None else None
    nbytes = packed_bytes(lib, K, N, prec)
    assert nbytes == N * K * (4 if prec == "fp32" else 2)
    wp = guard(np.full(nbytes // 4, np.nan, dtype=np.float32))
    y = guard(np.full((M, N), np.nan, dtype=np.float32))
    before = lib.emu_blocking_calls()
    rc = lib.dd_linear_pack(U.ptr(gw), U.ptr(wp), K, N, LC.PRECISIONS[prec], None)
    assert rc == 0, lib.dd_linear_last_error()
    image = wp.copy()
    rc = lib.dd_linear_forward(U.ptr(gx), U.ptr(wp), U.ptr(gb), U.ptr(ga), U.ptr(y), M, K, N, act, LC.PRECISIONS[prec], None)
    assert rc == 0, lib.dd_linear_last_error()
    assert lib.emu_blocking_calls() == before, "a call blocked the host"
    guard.check()
    same = lambda a, b: b is None or np.array_equal(a, b, equal_nan=True)
    assert same(gx, x) and same(gw, w) and same(gb, bias) and same(ga, addend), "an input was written"
    assert np.array_equal(wp.view(np.uint32), image.view(np.uint32)), "the forward wrote the packed image"
    return y.copy()


def both_orders(lib):
    """run() under both wave schedules of the emulation, bit-equal."""
    def f(*a):
        lib.emu_set_order(0)
        o0 = run(lib, *a)
        lib.emu_set_order(1)
        try:
            o1 = run(lib, *a)
        finally:
            lib.emu_set_order(0)
        assert np.array_equal(LC.bits(o0), LC.bits(o1)), "the wave schedule shows"
        return o0
    return f


@pytest.mark.parametrize("case", LC.cases(EMU_SHAPES), ids=LC.case_id)
def test_exact_cases_are_bit_equal(lib, case):
    LC.check_ints(both_orders(lib), *case)
    LC.check_selection(both_orders(lib), *case)


@pytest.mark.parametrize("variant", LC.VARIANTS)
@pytest.mark.parametrize("case", LC.cases(EMU_SHAPES), ids=LC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(lib, case, variant):
    LC.check_real(both_orders(lib), *case, variant, where="hostemu")


@pytest.mark.parametrize("case", LC.cases(BIG), ids=LC.case_id)
def test_the_big_tile_shapes(lib, case):
    """256 and more tiles of 128 x 128: the big-tile instantiation in the 16-bit modes (the fp32 mode keeps the 64-row tile).  One schedule."""
    f = lambda *a: run(lib, *a)
    LC.check_ints(f, *case)
    LC.check_selection(f, *case)
    LC.check_real(f, *case, "full", where="hostemu")


@pytest.mark.parametrize("prec", list(LC.PRECISIONS))
def test_repeat_row_prefix_and_nan_identities(lib, prec):
    f = lambda *a: run(lib, *a)
    LC.check_repeat_and_rows(f, prec)
    LC.check_nan(f, prec)


@pytest.mark.parametrize("prec", ("bf16", "f16"))
def test_row_prefixes_across_the_two_tile_heights(lib, prec):
    """(513, 32, 8192) runs on 128-row tiles, its prefixes of 127 .. 129 rows on 64-row tiles, the prefix of 511 rows on 128-row tiles again:
    the same bits."""
    LC.check_repeat_and_rows(lambda *a: run(lib, *a), prec, name="big+1", edges=LC.TILE_EDGES["big"])


def test_support_and_argument_errors_leave_y_untouched(lib):
    sup = lib.dd_linear_supported
    for prec in (1, 2, 3):
        for K, N in ((32, 32), (96, 288), (192, 576), (1536, 6144), (6144, 1536), (8192, 8192), (768, 384)):
            assert sup(K, N, 0, prec) == 1 and sup(K, N, 1, prec) == 1, (K, N, prec)
    for K, N, act, prec in ((48, 64, 0, 1), (64, 48, 0, 1), (0, 64, 0, 1), (64, 0, 0, 1), (-32, 64, 0, 1), (8224, 64, 0, 1), (64, 8224, 0, 2), (64, 64, 2, 1),
                            (64, 64, -1, 1), (64, 64, 0, 0), (64, 64, 0, 4), (64, 64, 0, 5), (16, 64, 0, 1)):
        assert sup(K, N, act, prec) == 0, (K, N, act, prec)
    n = ctypes.c_int64(-1)
    assert lib.dd_linear_packed_bytes(48, 64, 1, ctypes.byref(n)) == LC.DD_ERR_UNSUPPORTED and n.value == -1
    assert lib.dd_linear_packed_bytes(64, 64, 4, ctypes.byref(n)) == LC.DD_ERR_UNSUPPORTED and b"precision" in lib.dd_linear_last_error()
    assert lib.dd_linear_packed_bytes(64, 64, 1, None) == LC.DD_ERR_INVALID_ARG
    assert packed_bytes(lib, 96, 288, "fp32") == 96 * 288 * 4 and packed_bytes(lib, 96, 288, "bf16") == 96 * 288 * 2

    M, K, N = 5, 64, 96
    g = Guarded()
    x, w, bias, addend = g(np.ones((M, K), np.float32)), g(np.ones((N, K), np.float32)), g(np.ones(N, np.float32)), g(np.ones((M, N), np.float32))
    wp = g(np.zeros((N, K), np.float32))
    y = g(np.full((M, N), SENTINEL, dtype=np.float32))
    P = U.ptr
    f = lib.dd_linear_forward
    call = lambda M_=M, K_=K, N_=N, act=0, prec=1, x_=x, wp_=wp, b_=bias, a_=addend, y_=y: f(P(x_), P(wp_), P(b_), P(a_), P(y_), M_, K_, N_, act, prec, None)
    for kw in (dict(K_=48), dict(N_=8224), dict(K_=8224), dict(N_=80), dict(act=2), dict(act=-1), dict(prec=0), dict(prec=4), dict(prec=9)):
        assert call(**kw) == LC.DD_ERR_UNSUPPORTED, kw
        assert lib.dd_linear_last_error()
    assert call(prec=0) == LC.DD_ERR_UNSUPPORTED and b"precision" in lib.dd_linear_last_error()
    assert call(act=3) == LC.DD_ERR_UNSUPPORTED and b"act" in lib.dd_linear_last_error()
    for kw in (dict(M_=0), dict(M_=-4), dict(x_=None), dict(wp_=None), dict(y_=None)):
        assert call(**kw) == LC.DD_ERR_INVALID_ARG, kw
    assert call(x_=None) == LC.DD_ERR_INVALID_ARG and b"null" in lib.dd_linear_last_error()
    for kw in (dict(y_=x), dict(y_=wp), dict(y_=addend), dict(y_=bias)):
        assert call(**kw) == LC.DD_ERR_INVALID_ARG and b"alias" in lib.dd_linear_last_error(), kw
    off = lambda a: ctypes.c_void_p(a.ctypes.data + 4)
    tail = (M, K, N, 0, 1, None)
    for args in ((P(x), P(wp), P(bias), P(addend), off(y)), (off(x), P(wp), P(bias), P(addend), P(y)), (P(x), off(wp), P(bias), P(addend), P(y)),
                 (P(x), P(wp), P(bias), off(addend), P(y))):
        assert f(*args, *tail) == LC.DD_ERR_INVALID_ARG and b"aligned" in lib.dd_linear_last_error()
    assert lib.dd_linear_pack(None, P(wp), K, N, 1, None) == LC.DD_ERR_INVALID_ARG
    assert lib.dd_linear_pack(P(w), P(w), K, N, 1, None) == LC.DD_ERR_INVALID_ARG
    assert lib.dd_linear_pack(P(w), P(wp), 48, N, 1, None) == LC.DD_ERR_UNSUPPORTED
    assert (y == SENTINEL).all() and (wp == 0).all(), "a refused call wrote"
    assert lib.dd_linear_pack(P(w), P(wp), K, N, 1, None) == 0
    assert call(b_=None, a_=None) == 0      # bias and addend are optional
    assert (y == np.float32(K)).all()
    assert call() == 0 and (y == np.float32(K + 2)).all()
    g.check()
