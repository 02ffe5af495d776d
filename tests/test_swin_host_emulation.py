"""CPU: include/ddepth_swin.h with csrc/dd_swin.hip + csrc/dd_api_swin.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h, built
as tests/test_conv_stats_host_emulation.py builds its units: the cases of tests/swin_cases.py under both wave schedules (bit-equal), sentinels
around every tensor, and the argument checks.  The emulated device has 4 CUs, so the persistent grid is 8 workgroups = 16 waves and every
shape but the smallest makes several passes."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import hostemu_util as U
import swin_cases as SC
from diffusiondepth_amd import swin as SW

UNITS = [os.path.join(U.CSRC, f) for f in ("dd_swin.hip", "dd_api_swin.cpp")] + [os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_swin.h", "dd_status.h")] + [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", h) for h in ("ddepth.h", "ddepth_swin.h")]
SENTINEL = np.float32(-12345.678)
EMU_SHAPES = ("one", "whole", "ragged", "sub", "last")      # "big" runs once, in its own test: it is the slow one here


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
        out = os.path.join(U.OUT, "swin_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_swin_hostemu.so")
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
    lib.dd_window_attention_supported.argtypes = [c_int] * 4
    lib.dd_window_attention_forward.argtypes = [c_vp] * 4 + [c_int] * 8 + [c_vp]
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


def run(lib, qkv, pad, bias, heads, shift, prec):
    B, H, W, K = qkv.shape
    guard = Guarded()
    q, bs = guard(qkv), guard(bias)
    p = guard(pad) if pad is not None else None
    out = guard(np.full((B, H, W, K // 3), np.nan, dtype=np.float32))
    before = lib.emu_blocking_calls()
    rc = lib.dd_window_attention_forward(U.ptr(q), U.ptr(p), U.ptr(bs), U.ptr(out), B, H, W, K // 3, heads, SC.WINDOW, shift, SC.PRECISIONS[prec], None)
    assert rc == 0, lib.dd_swin_last_error()
    assert lib.emu_blocking_calls() == before, "the call blocked the host"
    guard.check()
    assert np.array_equal(q, qkv, equal_nan=True) and np.array_equal(bs, bias) and (pad is None or np.array_equal(p, pad)), "an input was written"
    return out.copy()


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
        assert np.array_equal(SC.bits(o0), SC.bits(o1)), "the wave schedule shows"
        return o0
    return f


def torch_fp32(qkv, pad, bias, heads, shift):
    t = lambda a: None if a is None else torch.tensor(a)
    return SW.window_attention_torch(t(qkv), t(pad), t(bias), heads, SC.WINDOW, shift).numpy()


@pytest.mark.parametrize("kind", ("identity", "permutation"))
@pytest.mark.parametrize("case", SC.cases(EMU_SHAPES), ids=SC.case_id)
def test_exact_cases_are_bit_equal(lib, case, kind):
    SC.check_exact(both_orders(lib), *case, kind)


@pytest.mark.parametrize("bias_scale", SC.BIAS_SCALES)
@pytest.mark.parametrize("case", SC.cases(EMU_SHAPES), ids=SC.case_id)
def test_real_valued_cases_against_the_fp64_oracle(lib, case, bias_scale):
    SC.check_real(both_orders(lib), torch_fp32, *case, bias_scale, where="hostemu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_more_tasks_than_the_grid_holds(lib, prec):
    """(2, 70, 70, 6): 1 200 tasks on 16 waves, shifted, exact and real-valued, one schedule."""
    f = lambda *a: run(lib, *a)
    SC.check_exact(f, "big", 3, prec, "permutation")
    SC.check_real(f, torch_fp32, "big", 3, prec, 1.0, where="hostemu")


@pytest.mark.parametrize("prec", list(SC.PRECISIONS))
def test_batch_repeat_and_nan_identities(lib, prec):
    f = lambda *a: run(lib, *a)
    SC.check_batch_and_repeat(f, prec)
    SC.check_nan(f, prec)


def test_support_and_argument_errors_leave_out_untouched(lib):
    sup = lib.dd_window_attention_supported
    for prec in (1, 2, 3):
        assert sup(32, 1, 7, prec) == 1 and sup(192, 6, 7, prec) == 1 and sup(1536, 48, 7, prec) == 1
    for C, heads, window, prec in ((192, 6, 7, 0), (192, 6, 7, 4), (192, 6, 7, 5), (192, 6, 8, 1), (192, 6, 12, 2), (192, 4, 7, 1), (96, 6, 7, 1),
                                   (64, 1, 7, 1), (0, 0, 7, 1), (-32, -1, 7, 1)):
        assert sup(C, heads, window, prec) == 0, (C, heads, window, prec)
    heads, C = 2, 64
    qkv = np.zeros((1, 7, 7, 3 * C), dtype=np.float32)
    pad = np.zeros(3 * C, dtype=np.float32)
    bias = np.zeros((heads, 49, 49), dtype=np.float32)
    out = np.full((1, 7, 7, C), SENTINEL, dtype=np.float32)
    P = U.ptr
    f = lib.dd_window_attention_forward
    call = lambda B=1, H=7, W=7, C_=C, h=heads, win=7, shift=0, prec=1: f(P(qkv), P(pad), P(bias), P(out), B, H, W, C_, h, win, shift, prec, None)
    for kw in (dict(C_=96), dict(h=4), dict(C_=128, h=2), dict(win=8), dict(win=14, shift=7), dict(prec=0), dict(prec=4), dict(prec=5), dict(prec=9)):
        assert call(**kw) == SC.DD_ERR_UNSUPPORTED, kw
        assert lib.dd_swin_last_error()
    assert call(prec=0) == SC.DD_ERR_UNSUPPORTED and b"precision" in lib.dd_swin_last_error()
    for kw in (dict(shift=7), dict(shift=-1), dict(shift=9), dict(B=0), dict(H=0), dict(W=-3), dict(C_=0), dict(h=0), dict(win=0)):
        assert call(**kw) == SC.DD_ERR_INVALID_ARG, kw
    assert call(shift=7) == SC.DD_ERR_INVALID_ARG and b"shift" in lib.dd_swin_last_error()
    tail = (1, 7, 7, C, heads, 7, 0, 1, None)
    assert f(None, P(pad), P(bias), P(out), *tail) == SC.DD_ERR_INVALID_ARG and b"null" in lib.dd_swin_last_error()
    assert f(P(qkv), P(pad), None, P(out), *tail) == SC.DD_ERR_INVALID_ARG
    assert f(P(qkv), P(pad), P(bias), None, *tail) == SC.DD_ERR_INVALID_ARG
    assert f(P(qkv), P(pad), P(bias), P(qkv), *tail) == SC.DD_ERR_INVALID_ARG and b"alias" in lib.dd_swin_last_error()
    assert (out == SENTINEL).all(), "a refused call wrote to out"
    assert f(P(qkv), None, P(bias), P(out), *tail) == 0      # qkv_pad is optional
    assert not (out == SENTINEL).any()
