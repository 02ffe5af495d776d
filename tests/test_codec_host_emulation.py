"""CPU: csrc/dd_codec.hip + csrc/dd_api_codec.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h and executed work-item by
work-item: the calls of include/ddepth_codec.h against the fp64 references of tests/codec_cases.py, at the shapes and cases the GPU tests use
(tests/test_zz_gpu_codec.py), under both wave schedules of the emulation.  "Device" memory is host memory, so numpy arrays are the tensors; every
tensor has sentinels around it and the workspace a guard behind it."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import codec_cases as CC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_codec.hip"), os.path.join(U.CSRC, "dd_api_codec.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_codec.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"), os.path.join(U.ROOT, "include", "ddepth_codec.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]
DD_ERR_INVALID_ARG = 1


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
        out = os.path.join(U.OUT, "codec_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_codec_hostemu.so")
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
    c_int, c_vp, c_i64, c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    lib.dd_codec_last_error.restype = ctypes.c_char_p
    lib.dd_codec_workspace_bytes.argtypes = [c_int] * 4 + [ctypes.POINTER(c_i64)]
    lib.dd_codec_conv_forward.argtypes = [c_int] + [c_vp] * 5 + [c_int] * 3 + [c_vp]
    lib.dd_codec_conv_backward_data.argtypes = [c_int] + [c_vp] * 4 + [c_int] * 3 + [c_vp]
    lib.dd_codec_conv_backward_weight.argtypes = [c_int] + [c_vp] * 5 + [c_int] * 3 + [c_vp]
    lib.dd_codec_tail_forward.argtypes = [c_vp, c_vp, c_i64, c_f, c_vp]
    lib.dd_codec_tail_backward.argtypes = [c_vp, c_vp, c_vp, c_i64, c_f, c_vp]
    lib.emu_set_order.argtypes = [c_int]
    return lib


def ok(lib, rc):
    assert rc == 0, lib.dd_codec_last_error()


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


def run_three(lib, name, kind):
    """Forward, data gradient and weight (+ bias) gradient on numpy memory -> dict of codec_cases.KEYS."""
    op, (B, H, W) = CC.SHAPES[name]
    inp = CC.make_inputs(name, kind)
    xs, ws_, bs, ys = CC.shapes_of(name)
    guard = Guarded()
    x, w, gy = guard(inp["x"].numpy()), guard(inp["w"].numpy()), guard(inp["grad_y"].numpy())
    bias = guard(inp["bias"].numpy()) if bs else None
    y, gx, gw = (guard(np.full(s, np.nan, dtype=np.float32)) for s in (ys, xs, ws_))
    gb = guard(np.full(bs, np.nan, dtype=np.float32)) if bs else None
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_codec_workspace_bytes(op, B, H, W, ctypes.byref(n)))
    raw = np.full(n.value + 64 + 16, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16      # the workspace is 16-byte aligned; 0x5A bytes inside (its contents on entry do not matter) and behind it
    ws = raw[off:]
    ok(lib, lib.dd_codec_conv_forward(op, U.ptr(x), U.ptr(w), U.ptr(bias), U.ptr(y), U.ptr(ws), B, H, W, None))
    ok(lib, lib.dd_codec_conv_backward_data(op, U.ptr(gy), U.ptr(w), U.ptr(gx), U.ptr(ws), B, H, W, None))
    ok(lib, lib.dd_codec_conv_backward_weight(op, U.ptr(x), U.ptr(gy), U.ptr(gw), U.ptr(gb), U.ptr(ws), B, H, W, None))
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for k, src in (("x", x), ("w", w), ("grad_y", gy), ("bias", bias)):
        assert src is None or np.array_equal(src, inp[k].numpy()), "an input was written"
    out = {"y": y.copy(), "grad_x": gx.copy(), "grad_w": gw.copy()}
    if bs:
        out["grad_bias"] = gb.copy()
    return out


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", CC.EXACT, ids=CC.case_id)
def test_exact_cases_equal_the_fp64_reference(lib, case, order):
    name, kind = case
    lib.emu_set_order(order)
    try:
        CC.check_exact(run_three(lib, name, kind), name, kind, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", CC.REAL, ids=CC.case_id)
def test_real_valued_cases_stay_within_the_cap(lib, case, order):
    name, _ = case
    lib.emu_set_order(order)
    try:
        CC.check_real(run_three(lib, name, "normal"), name, "hostemu")
    finally:
        lib.emu_set_order(0)


@pytest.mark.parametrize("name", ["T2-enc1", "T4-dec0", "T4-dec1", "T2-enc0"])
def test_two_runs_give_the_same_bits(lib, name):
    a = run_three(lib, name, "normal")
    b = run_three(lib, name, "normal")
    for k in CC.keys_of(name):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_the_bias_gradient_is_skipped_when_it_is_null(lib):
    name = "T1-dec0"
    op, (B, H, W) = CC.SHAPES[name]
    inp = CC.make_inputs(name, "int")
    x, gy = inp["x"].numpy().copy(), inp["grad_y"].numpy().copy()
    gw = np.full(CC.shapes_of(name)[1], np.nan, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:]
    ok(lib, lib.dd_codec_conv_backward_weight(op, U.ptr(x), U.ptr(gy), U.ptr(gw), None, U.ptr(ws), B, H, W, None))
    assert np.array_equal(gw.astype(np.float64), CC.reference(name, "int")["grad_w"])


def test_dec0_forward_into_an_output_that_is_not_8_byte_aligned(lib):
    """The pair stores of DEC0's forward fall back to 4-byte stores: same result, nothing written around the tensor."""
    name = "T3-dec0"
    op, (B, H, W) = CC.SHAPES[name]
    inp = CC.make_inputs(name, "int")
    ys = CC.shapes_of(name)[3]
    n = int(np.prod(ys))
    buf = np.full(n + 35, SENTINEL, dtype=np.float32)
    off = 16 + (1 if (buf.ctypes.data + 64) % 8 == 0 else 0)      # an odd number of floats past an 8-byte boundary
    y = buf[off:off + n].reshape(ys)
    assert y.ctypes.data % 8 == 4
    ws = np.zeros(1 << 20, dtype=np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:]
    x, w, b = (inp[k].numpy().copy() for k in ("x", "w", "bias"))
    ok(lib, lib.dd_codec_conv_forward(op, U.ptr(x), U.ptr(w), U.ptr(b), U.ptr(y), U.ptr(ws), B, H, W, None))
    assert np.array_equal(y.astype(np.float64), CC.reference(name, "int")["y"])
    assert (buf[:off] == SENTINEL).all() and (buf[off + n:] == SENTINEL).all()


@pytest.mark.parametrize("name", [n for n in CC.SHAPES if n.startswith("T4")])
def test_the_weight_gradient_of_T4_runs_at_least_three_splits_with_a_partial_last_one(name):
    """20 pixel tiles of 64 at kSplitTiles = 8 per split (csrc/dd_codec.h): two full splits and one of 4."""
    k = CC.header_constants()
    tiles = CC.wgrad_tiles(name, k["kWgTileW"])
    per = max(k["kSplitTiles"], -(-tiles // k["kMaxSplits"]))
    assert tiles == 20 and -(-tiles // per) >= 3 and tiles % per != 0


@pytest.mark.parametrize("order", [0, 1])
def test_the_tail(lib, order):
    z, gd = (t.numpy() for t in CC.tail_inputs())
    guard = Guarded()
    zz, gg = guard(z), guard(gd)
    depth, gz = guard(np.full(z.shape, 7.0, dtype=np.float32)), guard(np.full(z.shape, 7.0, dtype=np.float32))
    lib.emu_set_order(order)
    try:
        ok(lib, lib.dd_codec_tail_forward(U.ptr(zz), U.ptr(depth), z.size, CC.EPS, None))
        ok(lib, lib.dd_codec_tail_backward(U.ptr(zz), U.ptr(gg), U.ptr(gz), z.size, CC.EPS, None))
    finally:
        lib.emu_set_order(0)
    guard.check()
    assert np.array_equal(zz, z, equal_nan=True) and np.array_equal(gg, gd), "an input was written"
    CC.check_tail(depth, gz, "hostemu")


def test_invalid_arguments(lib):
    n = ctypes.c_int64(0)
    x = np.zeros(16 * 16, dtype=np.float32)
    w = np.zeros(16 * 16 * 16, dtype=np.float32)
    y = np.zeros(16 * 64, dtype=np.float32)
    b = np.zeros(16, dtype=np.float32)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:]
    err = lib.dd_codec_last_error
    # unknown op
    for op in (-1, 4, 7):
        assert lib.dd_codec_workspace_bytes(op, 1, 4, 4, ctypes.byref(n)) == DD_ERR_INVALID_ARG and b"op" in err()
        assert lib.dd_codec_conv_forward(op, U.ptr(x), U.ptr(w), None, U.ptr(y), U.ptr(ws), 1, 4, 4, None) == DD_ERR_INVALID_ARG and b"op" in err()
    assert lib.dd_codec_workspace_bytes(CC.ENC1, 1, 4, 4, None) == DD_ERR_INVALID_ARG
    for op in (CC.ENC0, CC.ENC1, CC.DEC0, CC.DEC1):
        fwd = lambda *a: lib.dd_codec_conv_forward(op, *a, None)
        bwd = lambda *a: lib.dd_codec_conv_backward_data(op, *a, None)
        wgr = lambda *a: lib.dd_codec_conv_backward_weight(op, *a, None)
        # null
        assert fwd(None, U.ptr(w), None, U.ptr(y), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"null" in err()
        assert fwd(U.ptr(x), U.ptr(w), None, None, U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"null" in err()
        assert fwd(U.ptr(x), U.ptr(w), None, U.ptr(y), None, 1, 4, 4) == DD_ERR_INVALID_ARG and b"null" in err()
        assert bwd(U.ptr(y), None, U.ptr(x), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"null" in err()
        assert wgr(U.ptr(x), U.ptr(y), None, None, U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"null" in err()
        # alias
        assert fwd(U.ptr(x), U.ptr(w), None, U.ptr(x), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"alias" in err()
        assert bwd(U.ptr(y), U.ptr(w), U.ptr(y), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"alias" in err()
        assert wgr(U.ptr(x), U.ptr(y), U.ptr(x), None, U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"alias" in err()
        # non-positive
        for dims in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
            assert fwd(U.ptr(x), U.ptr(w), None, U.ptr(y), U.ptr(ws), *dims) == DD_ERR_INVALID_ARG and b"positive" in err()
            assert lib.dd_codec_workspace_bytes(op, *dims, ctypes.byref(n)) == DD_ERR_INVALID_ARG and b"positive" in err()
        # a bias where the layer has none
        if not CC.has_bias(op):
            assert fwd(U.ptr(x), U.ptr(w), U.ptr(b), U.ptr(y), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"bias" in err()
            assert wgr(U.ptr(x), U.ptr(y), U.ptr(w), U.ptr(b), U.ptr(ws), 1, 4, 4) == DD_ERR_INVALID_ARG and b"bias" in err()
    # a misaligned workspace
    assert lib.dd_codec_conv_forward(CC.ENC1, U.ptr(x), U.ptr(w), None, U.ptr(y), U.ptr(ws[4:]), 1, 4, 4, None) == DD_ERR_INVALID_ARG and b"aligned" in err()
    # the tail
    z = np.zeros(8, dtype=np.float32)
    assert lib.dd_codec_tail_forward(None, U.ptr(z), 8, CC.EPS, None) == DD_ERR_INVALID_ARG and b"null" in err()
    assert lib.dd_codec_tail_forward(U.ptr(z), U.ptr(z), 8, CC.EPS, None) == DD_ERR_INVALID_ARG and b"alias" in err()
    assert lib.dd_codec_tail_forward(U.ptr(z), U.ptr(z.copy()), 0, CC.EPS, None) == DD_ERR_INVALID_ARG and b"positive" in err()
    assert lib.dd_codec_tail_backward(U.ptr(z), None, U.ptr(z.copy()), 8, CC.EPS, None) == DD_ERR_INVALID_ARG and b"null" in err()
    assert lib.dd_codec_tail_backward(U.ptr(z), U.ptr(z.copy()), U.ptr(z), 8, CC.EPS, None) == DD_ERR_INVALID_ARG and b"alias" in err()
    assert lib.dd_codec_tail_backward(U.ptr(z), U.ptr(z.copy()), U.ptr(z.copy()), -3, CC.EPS, None) == DD_ERR_INVALID_ARG and b"positive" in err()
