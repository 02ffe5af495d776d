"""CPU: the pointwise (1x1) operator of include/ddepth_conv.h -- csrc/dd_conv.hip + csrc/dd_api_conv.cpp compiled for the host on top of
tests/host_emul/hip/hip_runtime.h and executed work-item by work-item, the MFMA builtins emulated: dd_conv1x1_forward / _backward_data /
_backward_weight against the fp64 references of tests/conv_pw_cases.py, at the shapes and cases the GPU tests use
(tests/test_zz_gpu_conv_neck.py), under both wave schedules of the emulation.  "Device" memory is host memory, so numpy arrays are the tensors;
every tensor has sentinels around it and the workspace a guard behind it."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import conv_pw_cases as PC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_conv.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"), os.path.join(U.ROOT, "include", "ddepth_conv.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4
ENTRY = ("dd_conv1x1_forward", "dd_conv1x1_backward_data", "dd_conv1x1_backward_weight")


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
        out = os.path.join(U.OUT, "conv_" + hsh.hexdigest()[:12])      # (the directory tests/test_conv_host_emulation.py builds into: one build serves both)
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
    lib.dd_conv_supported.argtypes = [c_int] * 4
    lib.dd_conv_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    for n in ENTRY:
        getattr(lib, n).argtypes = [c_vp] * 4 + [c_int] * 6 + [c_vp]
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


def run_three(lib, name, prec, kind):
    """Forward, data gradient and weight gradient on numpy memory -> dict of conv_pw_cases.KEYS."""
    B, Cin, Cout, H, W = PC.SHAPES[name]
    inp = PC.make_inputs(name, kind)
    xs, ws_, ys = PC.shapes_of(name)
    p = PC.PRECISIONS[prec]
    guard = Guarded()
    x, w, gy = guard(inp["x"].numpy()), guard(inp["w"].numpy()), guard(inp["grad_y"].numpy())
    y, gx, gw = (guard(np.full(s, np.nan, dtype=np.float32)) for s in (ys, xs, ws_))
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_conv_workspace_bytes(PC.CONV1X1, B, Cin, Cout, H, W, p, ctypes.byref(n)))
    raw = np.full(n.value + 64 + 16, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16      # the workspace is 16-byte aligned; 0x5A bytes inside (its contents on entry do not matter) and behind it
    ws = raw[off:]
    fwd, bwd_data, bwd_weight = (getattr(lib, f) for f in ENTRY)
    dims = (B, Cin, Cout, H, W, p, None)
    ok(lib, fwd(U.ptr(x), U.ptr(w), U.ptr(y), U.ptr(ws), *dims))
    ok(lib, bwd_data(U.ptr(gy), U.ptr(w), U.ptr(gx), U.ptr(ws), *dims))
    ok(lib, bwd_weight(U.ptr(x), U.ptr(gy), U.ptr(gw), U.ptr(ws), *dims))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("grad_y", gy)):
        assert np.array_equal(src, inp[k].numpy()), "an input was written"
    return {"y": y.copy(), "grad_x": gx.copy(), "grad_w": gw.copy()}


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", PC.EXACT + PC.WIDE, ids=PC.case_id)
def test_exact_cases_equal_the_fp64_reference(lib, case, order):
    name, prec, kind = case
    lib.emu_set_order(order)
    try:
        PC.check_exact(run_three(lib, name, prec, kind), name, kind, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", PC.REAL, ids=PC.case_id)
def test_real_valued_cases_stay_within_the_cap(lib, case, order):
    name, prec, _ = case
    lib.emu_set_order(order)
    try:
        PC.check_real(run_three(lib, name, prec, "normal"), name, prec, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("name,kind", [("P1", "wide_x"), ("P2", "normal")])
def test_two_runs_give_the_same_bits(lib, name, kind):
    a = run_three(lib, name, "f16x3", kind)
    b = run_three(lib, name, "f16x3", kind)
    for k in PC.KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_the_weight_gradient_of_P4_runs_at_least_three_splits_with_a_partial_last_one(lib):
    """66 flat pixel tiles of kPwTile = 128 at kSplitTiles = 8 per split (csrc/dd_conv.h): 8 full splits and one of 2; the workspace query says
    the same (the partial sums are what it holds at this shape)."""
    hdr = open(os.path.join(U.CSRC, "dd_conv.h")).read()
    per = int(re.search(r"kSplitTiles = (\d+);", hdr).group(1))
    most = int(re.search(r"kMaxSplits = (\d+);", hdr).group(1))
    tile = int(re.search(r"kPwTile = (\d+);", hdr).group(1))
    assert tile == PC.PW_TILE
    B, Cin, Cout, H, W = PC.SHAPES["P4"]
    tiles = B * -(-(H * W) // tile)
    per = max(per, -(-tiles // most))
    splits = -(-tiles // per)
    assert tiles == 66 and splits >= 3 and tiles % per != 0 and splits <= most
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_conv_workspace_bytes(PC.CONV1X1, B, Cin, Cout, H, W, 2, ctypes.byref(n)))
    assert n.value == splits * Cin * Cout * 4


def test_unsupported_and_invalid_arguments(lib):
    n = ctypes.c_int64(0)
    assert lib.dd_conv_supported(PC.CONV1X1, 64, 192, 2) == 1 and lib.dd_conv_supported(PC.CONV1X1, 1536, 1536, 4) == 1
    for cin, cout, prec in ((216, 256, 2), (256, 216, 4), (32, 64, 3), (1600, 64, 3), (2048, 1536, 2), (64, 256, 1), (64, 256, 5), (64, 256, 0)):
        assert lib.dd_conv_supported(PC.CONV1X1, cin, cout, prec) == 0
        assert lib.dd_conv_workspace_bytes(PC.CONV1X1, 1, cin, cout, 4, 4, prec, ctypes.byref(n)) == DD_ERR_UNSUPPORTED
        assert b"unsupported" in lib.dd_conv_last_error()
    assert lib.dd_conv_supported(3, 64, 64, 2) == 0
    assert lib.dd_conv_workspace_bytes(3, 1, 64, 64, 4, 4, 2, ctypes.byref(n)) == DD_ERR_INVALID_ARG and b"dd_conv_op" in lib.dd_conv_last_error()
    x = np.zeros(64 * 4, dtype=np.float32)
    w = np.zeros(64 * 64, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    for f in ENTRY:
        assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 216, 64, 2, 2, 2, None) == DD_ERR_UNSUPPORTED
        assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 64, 64, 2, 2, 1, None) == DD_ERR_UNSUPPORTED
        assert b"unsupported" in lib.dd_conv_last_error()
        assert getattr(lib, f)(None, None, None, None, 1, 64, 64, 2, 2, 2, None) != 0 and b"null" in lib.dd_conv_last_error()
        assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x), U.ptr(ws), 1, 64, 64, 2, 2, 2, None) != 0 and b"alias" in lib.dd_conv_last_error()
        assert getattr(lib, f)(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws[1:]), 1, 64, 64, 2, 2, 2, None) != 0 and b"aligned" in lib.dd_conv_last_error()
    assert lib.dd_conv1x1_forward(U.ptr(x), U.ptr(w), U.ptr(x.copy()), U.ptr(ws), 1, 64, 64, 0, 2, 2, None) != 0
    assert b"positive" in lib.dd_conv_last_error()
