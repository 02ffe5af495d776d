"""CPU: include/train/ddepth_swin_backward.h with csrc/dd_swin_bwd.hip + csrc/dd_api_swin_bwd.cpp (and the forward's two units, whose support
query and error text they share) compiled for the host on top of tests/host_emul/hip/hip_runtime.h, built as tests/test_swin_host_emulation.py
builds its units: the cases of tests/swin_backward_cases.py under both wave schedules (bit-equal), sentinels around every tensor and the
workspace, untouched inputs, no blocking call, and the argument checks."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import hostemu_util as U
import swin_backward_cases as BC
import swin_cases as SC

UNITS = [os.path.join(U.CSRC, f) for f in ("dd_swin.hip", "dd_api_swin.cpp", "dd_swin_bwd.hip", "dd_api_swin_bwd.cpp")] + \
    [os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_swin.h", "dd_swin_dev.h", "dd_swin_bwd.h", "dd_status.h")] + \
    [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", h) for h in ("ddepth.h", "ddepth_swin.h", os.path.join("train", "ddepth_swin_backward.h"))]
SENTINEL = np.float32(-12345.678)
EMU_SHAPES = ("one", "whole", "ragged", "sub", "last")      # "big" runs once per precision, in its own test: it is the slow one here


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
        out = os.path.join(U.OUT, "swin_bwd_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_swin_bwd_hostemu.so")
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
    lib.dd_swin_last_error.restype = ctypes.c_char_p
    lib.dd_window_attention_backward_supported.argtypes = [c_int] * 4
    lib.dd_window_attention_backward_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    lib.dd_window_attention_backward.argtypes = [c_vp] * 9 + [c_int] * 8 + [c_vp]
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
            assert (buf[:16] == SENTINEL).all() and (buf[16 + size:] == SENTINEL).all(), "the kernel wrote outside a tensor"


def workspace_floats(lib, B, H, W, C, heads, prec):
    n = ctypes.c_int64(-1)
    assert lib.dd_window_attention_backward_workspace_bytes(B, H, W, C, heads, SC.WINDOW, SC.PRECISIONS[prec], ctypes.byref(n)) == 0
    assert n.value > 0 and n.value % 4 == 0
    return n.value // 4


def run(lib, qkv, pad, bias, gout, heads, shift, prec, scale=None, want_pad=True, want_bias=True, poison=False):
    B, H, W, K = qkv.shape
    C = K // 3
    guard = Guarded()
    q, bs, go = guard(qkv), guard(bias), guard(gout)
    p = guard(pad) if pad is not None else None
    sc = guard(scale) if scale is not None else None
    gq = guard(np.full((B, H, W, K), np.nan, dtype=np.float32))
    gp = guard(np.full(K, np.nan, dtype=np.float32)) if want_pad else None
    gb = guard(np.full((heads, 49, 49), np.nan, dtype=np.float32)) if want_bias else None
    ws = guard(np.full(workspace_floats(lib, B, H, W, C, heads, prec), np.nan if poison else 7.0, dtype=np.float32))
    before = lib.emu_blocking_calls()
    rc = lib.dd_window_attention_backward(U.ptr(q), U.ptr(p), U.ptr(bs), U.ptr(go), U.ptr(gq), U.ptr(gp), U.ptr(gb), U.ptr(ws), U.ptr(sc), B, H, W, C,
                                          heads, SC.WINDOW, shift, SC.PRECISIONS[prec], None)
    assert rc == 0, lib.dd_swin_last_error()
    assert lib.emu_blocking_calls() == before, "the call blocked the host"
    guard.check()
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(q, qkv) and same(bs, bias) and same(go, gout) and (pad is None or same(p, pad)) and (scale is None or same(sc, scale)), \
        "an input was written"
    return gq.copy(), None if gp is None else gp.copy(), None if gb is None else gb.copy()


def both_orders(lib):
    """run() under both wave schedules of the emulation, bit-equal."""
    def f(*a, **kw):
        lib.emu_set_order(0)
        o0 = run(lib, *a, **kw)
        lib.emu_set_order(1)
        try:
            o1 = run(lib, *a, **kw)
        finally:
            lib.emu_set_order(0)
        for x, y in zip(o0, o1):
            assert np.array_equal(SC.bits(x), SC.bits(y)), "the wave schedule shows"
        return o0
    return f


@pytest.mark.parametrize("bias_scale", SC.BIAS_SCALES)
@pytest.mark.parametrize("case", SC.cases(EMU_SHAPES), ids=SC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(lib, case, bias_scale):
    BC.check_real(both_orders(lib), *case, bias_scale, where="hostemu")


@pytest.mark.parametrize("kind", ("identity", "permutation"))
@pytest.mark.parametrize("case", SC.cases(EMU_SHAPES), ids=SC.case_id)
def test_one_hot_cases_are_exact(lib, case, kind):
    BC.check_onehot(both_orders(lib), *case, kind)


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
@pytest.mark.parametrize("name", EMU_SHAPES)
def test_half_half_cases_are_exact(lib, name, prec):
    BC.check_halves(both_orders(lib), name, prec)


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_several_slices_per_head_and_several_windows_per_slice(lib, prec):
    """(2, 70, 70, 6): 200 windows in 67 slices of 3 per head, shifted, exact and real-valued, one schedule."""
    f = lambda *a, **kw: run(lib, *a, **kw)
    BC.check_onehot(f, "big", 3, prec, "permutation")
    BC.check_halves(f, "big", prec)
    BC.check_real(f, "big", 3, prec, 1.0, where="hostemu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_repeat_batch_workspace_null_and_nan_identities(lib, prec):
    f = lambda *a, **kw: run(lib, *a, **kw)
    BC.check_identities(f, prec)
    BC.check_nan(f, prec)


def test_f16_grad_out_scale_is_exact_in_powers_of_two(lib):
    BC.check_f16_scale(lambda *a, **kw: run(lib, *a, **kw))


def test_the_workspace_query_needs_no_device_and_follows_the_shape(lib):
    n = ctypes.c_int64(-1)
    f = lib.dd_window_attention_backward_workspace_bytes
    per = (49 * 49 + 96) * 4
    for (B, H, W, heads), slices in (((1, 7, 7, 1), 1), ((2, 10, 17, 3), 12), ((2, 70, 70, 6), 67), ((4, 88, 304, 6), 143), ((1, 11, 38, 48), 12)):
        for prec in (1, 2, 3):
            assert f(B, H, W, 32 * heads, heads, 7, prec, ctypes.byref(n)) == 0 and n.value == slices * heads * per, (B, H, W, heads, n.value)
    n.value = -1
    assert f(1, 7, 7, 32, 1, 8, 1, ctypes.byref(n)) == SC.DD_ERR_UNSUPPORTED and f(1, 7, 7, 32, 1, 7, 0, ctypes.byref(n)) == SC.DD_ERR_UNSUPPORTED
    assert f(0, 7, 7, 32, 1, 7, 1, ctypes.byref(n)) == SC.DD_ERR_INVALID_ARG and f(1, 7, 7, 32, 1, 7, 1, None) == SC.DD_ERR_INVALID_ARG
    assert n.value == -1


def test_support_and_argument_errors_leave_the_outputs_untouched(lib):
    sup = lib.dd_window_attention_backward_supported
    for prec in (1, 2, 3):
        assert sup(32, 1, 7, prec) == 1 and sup(192, 6, 7, prec) == 1 and sup(1536, 48, 7, prec) == 1
    for C, heads, window, prec in ((192, 6, 7, 0), (192, 6, 7, 4), (192, 6, 8, 1), (192, 4, 7, 1), (96, 6, 7, 1), (0, 0, 7, 1), (-32, -1, 7, 1)):
        assert sup(C, heads, window, prec) == 0, (C, heads, window, prec)
    heads, C = 2, 64
    qkv = np.zeros((1, 7, 7, 3 * C), dtype=np.float32)
    pad = np.zeros(3 * C, dtype=np.float32)
    bias = np.zeros((heads, 49, 49), dtype=np.float32)
    gout = np.zeros((1, 7, 7, C), dtype=np.float32)
    scale = np.array([1, 1, 0, 0], dtype=np.float32)
    outs = [np.full(s, SENTINEL, dtype=np.float32) for s in ((1, 7, 7, 3 * C), (3 * C,), (heads, 49, 49), (workspace_floats(lib, 1, 7, 7, C, heads, "fp32"),))]
    gq, gp, gb, ws = outs
    P = U.ptr
    f = lib.dd_window_attention_backward
    ptrs = dict(qkv=qkv, pad=pad, bias=bias, gout=gout, gq=gq, gp=gp, gb=gb, ws=ws, scale=scale)

    def call(B=1, H=7, W=7, C_=C, h=heads, win=7, shift=0, prec=1, **swap):
        a = dict(ptrs, **swap)
        return f(*(P(a[k]) for k in ("qkv", "pad", "bias", "gout", "gq", "gp", "gb", "ws", "scale")), B, H, W, C_, h, win, shift, prec, None)

    for kw in (dict(C_=96), dict(h=4), dict(C_=128, h=2), dict(win=8), dict(win=14, shift=7), dict(prec=0), dict(prec=4), dict(prec=9)):
        assert call(**kw) == SC.DD_ERR_UNSUPPORTED, kw
        assert lib.dd_swin_last_error()
    assert call(prec=0) == SC.DD_ERR_UNSUPPORTED and b"precision" in lib.dd_swin_last_error()
    for kw in (dict(shift=7), dict(shift=-1), dict(B=0), dict(H=0), dict(W=-3), dict(C_=0), dict(h=0), dict(win=0)):
        assert call(**kw) == SC.DD_ERR_INVALID_ARG, kw
    assert call(shift=7) == SC.DD_ERR_INVALID_ARG and b"shift" in lib.dd_swin_last_error()
    for name in ("qkv", "bias", "gout", "gq", "ws"):
        assert call(**{name: None}) == SC.DD_ERR_INVALID_ARG and b"null" in lib.dd_swin_last_error(), name
    for kw in (dict(gq=qkv), dict(gp=pad), dict(gb=bias), dict(gq=gout.reshape(-1)), dict(gp=gb), dict(ws=gq), dict(gb=scale)):
        assert call(**kw) == SC.DD_ERR_INVALID_ARG and b"alias" in lib.dd_swin_last_error(), list(kw)
    assert call(gout=gout.reshape(-1)[1:]) == SC.DD_ERR_INVALID_ARG and b"aligned" in lib.dd_swin_last_error()
    for o in outs:
        assert (o == SENTINEL).all(), "a refused call wrote to an output"
    assert call(pad=None, gp=None, gb=None, scale=None) == 0      # the optional pointers
    assert not (gq == SENTINEL).any() and (gp == SENTINEL).all() and (gb == SENTINEL).all()
    assert call() == 0 and not (gp == SENTINEL).any() and not (gb == SENTINEL).any()
