"""CPU: include/ddepth_conv_scaled.h (dd_conv_grad_scale, dd_convx_backward_data_scaled, dd_convx_backward_weight_scaled) with csrc/dd_conv.hip +
csrc/dd_api_conv.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h, as tests/test_conv_ragged_host_emulation.py does for
dd_convx_*: the cases of tests/conv_scaled_cases.py under both wave schedules, the workspace (exactly the size dd_convx_workspace_bytes asks for,
a guard behind it) refilled with 0x5A or 0xFF bytes before every call, sentinels around every tensor and behind the 16-byte scale buffer."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import conv_scaled_cases as SC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_conv.h"), os.path.join(U.CSRC, "dd_conv_kernels.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"),
                os.path.join(U.ROOT, "include", "ddepth_conv.h"), os.path.join(U.ROOT, "include", "ddepth_conv_scaled.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]
DD_ERR_INVALID_ARG, DD_ERR_UNSUPPORTED = 1, 4
OLD = {SC.CONV: ("dd_conv3x3_backward_data", "dd_conv3x3_backward_weight"), SC.DECONV: ("dd_deconv2x2_backward_data", "dd_deconv2x2_backward_weight"),
       SC.CONV1X1: ("dd_conv1x1_backward_data", "dd_conv1x1_backward_weight")}
SCHEDULES = [(0, 0x5A), (1, 0xFF)]
SCHEDULE_IDS = ["order0-5A", "order1-FF"]


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
        out = os.path.join(U.OUT, "conv_scaled_" + hsh.hexdigest()[:12])
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
    lib.dd_convx_workspace_bytes.argtypes = [c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    for names in OLD.values():
        for n in names:
            getattr(lib, n).argtypes = [c_vp] * 4 + [c_int] * 6 + [c_vp]
    for n in ("dd_convx_backward_data", "dd_convx_backward_weight"):
        getattr(lib, n).argtypes = [c_int] + [c_vp] * 4 + [c_int] * 6 + [c_vp]
    for n in ("dd_convx_backward_data_scaled", "dd_convx_backward_weight_scaled"):
        getattr(lib, n).argtypes = [c_int] + [c_vp] * 5 + [c_int] * 6 + [c_vp]
    lib.dd_conv_grad_scale.argtypes = [c_vp, ctypes.c_int64, c_int, c_vp, c_vp]
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


def run_backward(lib, case, prec, x, w, grad_y, api="scaled", fill=0x5A, order=0):
    """The two gradients on numpy memory -> {"grad_x", "grad_w", "scale" (4 uint32; api "scaled" only)}.  api: "scaled" (dd_conv_grad_scale once,
    then the two *_scaled functions), "x" (dd_convx_backward_*) or "old" (the block-64 entry points)."""
    op, dims = SC.geometry(case)
    B, Cin, Cout, H, W = dims
    xs, ws_, ys = SC.shapes(case)
    p = SC.PRECISIONS[prec]
    guard = Guarded()
    xg, wg, gy = guard(x.reshape(xs)), guard(w.reshape(ws_)), guard(grad_y.reshape(ys))
    gx, gw = guard(np.full(xs, np.nan, dtype=np.float32)), guard(np.full(ws_, np.nan, dtype=np.float32))
    scale = guard(np.full(4, np.nan, dtype=np.float32))      # 16 bytes, sentinels on both sides
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_convx_workspace_bytes(op, B, Cin, Cout, H, W, p, ctypes.byref(n)))
    raw = np.full(n.value + 64 + 16, 0x5A, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16      # the workspace is 16-byte aligned
    ws = raw[off:]
    tail = (B, Cin, Cout, H, W, p, None)
    lib.emu_set_order(order)
    try:
        if api == "scaled":
            ok(lib, lib.dd_conv_grad_scale(U.ptr(gy), gy.size, p, U.ptr(scale), None))
            calls = [lambda a, b, c, d: lib.dd_convx_backward_data_scaled(op, a, b, c, d, U.ptr(scale), *tail),
                     lambda a, b, c, d: lib.dd_convx_backward_weight_scaled(op, a, b, c, d, U.ptr(scale), *tail)]
        elif api == "x":
            calls = [lambda a, b, c, d: lib.dd_convx_backward_data(op, a, b, c, d, *tail), lambda a, b, c, d: lib.dd_convx_backward_weight(op, a, b, c, d, *tail)]
        else:
            calls = [lambda a, b, c, d, f=getattr(lib, f): f(a, b, c, d, *tail) for f in OLD[op]]
        for call, args in zip(calls, ((gy, wg, gx), (xg, gy, gw))):
            ws[:n.value] = fill
            ok(lib, call(*(U.ptr(a) for a in args), U.ptr(ws)))
    finally:
        lib.emu_set_order(0)
    assert (ws[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    guard.check()
    for got, src in ((xg, x), (wg, w)):
        assert np.array_equal(got.ravel(), src.ravel()), "an input was written"
    assert np.array_equal(gy.ravel().view(np.uint32), grad_y.ravel().view(np.uint32)), "grad_y was written"
    out = {"grad_x": gx.copy(), "grad_w": gw.copy()}
    if api == "scaled":
        out["scale"] = scale.view(np.uint32).copy()
        one = np.float32(1).view(np.uint32)
        want = np.array([one, one, 0, 0], dtype=np.uint32) if prec == "bf16" else SC.scale_words(grad_y)      # (bf16: {1, 1}, no reduction)
        assert np.array_equal(out["scale"], want), (out["scale"], want)
    return out


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in SC.KEYS)


@pytest.mark.parametrize("order,fill", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EQUIVARIANCE)
def test_a_gradient_two_to_the_k_times_another_gives_two_to_the_k_times_the_result(lib, case, prec, order, fill):
    inp = SC.inputs(case)
    base = run_backward(lib, case, prec, inp["x"], inp["w"], inp["grad_y"], fill=fill, order=order)
    bad = []
    for k in SC.K_SMALL:
        got = run_backward(lib, case, prec, inp["x"], inp["w"], SC.small(inp["grad_y"], k), fill=fill, order=order)
        bad += [(k,) + b for b in SC.check_equivariant(got, base, k, f"hostemu {case} {prec}")]
    assert not bad, bad


@pytest.mark.parametrize("order,fill", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("which", ["small", "spike"])
@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.CAPS)
def test_a_gradient_at_training_scale_stays_within_the_cap(lib, case, prec, which, order, fill):
    inp = SC.inputs(case)
    got = run_backward(lib, case, prec, inp["x"], inp["w"], SC.variant(case, which), fill=fill, order=order)
    SC.check_caps(got, case, which, prec, "hostemu")


@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EXACT)
def test_integer_data_at_two_to_the_minus_twenty_is_exact(lib, case, prec):
    """Every product and partial sum is an integer times 2^-20 * s / s: exact whatever the order, through the reduce twin's several partials too
    (S4: 23 splits).  One schedule per precision: the schedules are covered by the cases above at a fraction of S4's emulation time."""
    inp = SC.inputs(case, "int")
    order, fill = SCHEDULES[SC.F16_MODES.index(prec)]
    got = run_backward(lib, case, prec, inp["x"], inp["w"], SC.small(inp["grad_y"], -20), fill=fill, order=order)
    SC.check_exact(got, case, -20, "hostemu")


@pytest.mark.parametrize("case", SC.BF16_IDENTITY)
def test_bf16_runs_the_unscaled_kernels(lib, case):
    inp = SC.inputs(case)
    gy = SC.small(inp["grad_y"], -20)
    a = run_backward(lib, case, "bf16", inp["x"], inp["w"], gy, fill=0xFF)
    b = run_backward(lib, case, "bf16", inp["x"], inp["w"], gy, api="x")
    assert same_bits(a, b)
    one = np.float32(1).view(np.uint32)
    assert a["scale"][0] == one and a["scale"][1] == one


@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.BLOCK64_IDENTITY)
def test_with_s_equal_to_one_a_block64_shape_gives_the_bits_of_the_old_entry_points(lib, case, prec):
    inp = SC.inputs(case)
    gy = SC.power_of_two_into_top_binade(inp["grad_y"])
    a = run_backward(lib, case, prec, inp["x"], inp["w"], gy, fill=0xFF)
    b = run_backward(lib, case, prec, inp["x"], inp["w"], gy, api="old")
    assert a["scale"][0] == np.float32(1).view(np.uint32)
    assert same_bits(a, b)


@pytest.mark.parametrize("case", SC.EDGE)
def test_an_all_zero_gradient_gives_s_one_and_zeros(lib, case):
    inp = SC.inputs(case)
    for prec in SC.F16_MODES:
        got = run_backward(lib, case, prec, inp["x"], inp["w"], np.zeros_like(inp["grad_y"]), fill=0xFF)
        assert got["scale"][0] == np.float32(1).view(np.uint32) and got["scale"][2] == 0
        assert not got["grad_x"].any() and not got["grad_w"].any()


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("prec", SC.F16_MODES)
@pytest.mark.parametrize("case", SC.EDGE)
def test_an_inf_or_nan_element_takes_no_part_in_the_scale_and_stays_in_its_footprint(lib, case, prec, value):
    inp = SC.inputs(case)
    idx = SC.edge_element(case)
    zeroed = SC.small(inp["grad_y"], -20)
    zeroed[idx] = 0
    bad = zeroed.copy()
    bad[idx] = value
    a, b = run_backward(lib, case, prec, inp["x"], inp["w"], bad), run_backward(lib, case, prec, inp["x"], inp["w"], zeroed)
    assert np.array_equal(a["scale"], b["scale"])
    for k, mask in SC.footprint(case, idx).items():
        assert np.array_equal(a[k].view(np.uint32)[~mask], b[k].view(np.uint32)[~mask]), k
        assert not np.isfinite(a[k][mask]).all(), "the element travels through as it is"


@pytest.mark.parametrize("case", ["rg:R1", "rg:T2", "rg:P1"])
def test_two_runs_give_the_same_bits(lib, case):
    inp = SC.inputs(case)
    gy = SC.spike(inp["grad_y"])
    a = run_backward(lib, case, "f16x3", inp["x"], inp["w"], gy)
    b = run_backward(lib, case, "f16x3", inp["x"], inp["w"], gy, fill=0xFF, order=1)
    assert same_bits(a, b) and np.array_equal(a["scale"], b["scale"])


def test_the_scale_of_extreme_magnitudes(lib):
    """The shift is held to +-126 (a subnormal or a huge amax), every element takes part, the last one of an odd count too."""
    scale = np.zeros(4, dtype=np.float32)
    for vals in ([1e-45, 0.0, -3e-42], [3e38, -1.0], [0.0, 0.0, 2.0 ** -126], [1.0] * 1029 + [-40000.0], [np.nan, np.inf, 5.0, -np.inf]):
        g = np.array(vals, dtype=np.float32)
        for prec in (3, 4):
            scale[:] = np.nan
            ok(lib, lib.dd_conv_grad_scale(U.ptr(g), g.size, prec, U.ptr(scale), None))
            assert np.array_equal(scale.view(np.uint32), SC.scale_words(g)), vals[:4]
            assert np.isfinite(scale[:2]).all() and scale[0] * scale[1] == 1.0 and scale[0] >= 2.0 ** -126 and scale[1] >= 2.0 ** -126


def test_argument_errors(lib):
    x = np.zeros(72 * 4, dtype=np.float32)
    w = np.zeros(72 * 72 * 9, dtype=np.float32)
    ws = np.zeros(1 << 20, dtype=np.uint8)
    scale = np.ones(4, dtype=np.float32)
    for name in ("dd_convx_backward_data_scaled", "dd_convx_backward_weight_scaled"):
        call = getattr(lib, name)
        out = np.zeros(w.size, dtype=np.float32)      # (room for either gradient)
        args = (U.ptr(x), U.ptr(w), U.ptr(out), U.ptr(ws)) if name.endswith("data_scaled") else (U.ptr(x), U.ptr(x.copy()), U.ptr(out), U.ptr(ws))
        assert call(0, *args, U.ptr(scale), 1, 72, 72, 2, 2, 3, None) == 0
        assert call(0, *args, None, 1, 72, 72, 2, 2, 3, None) == DD_ERR_INVALID_ARG and b"scale" in lib.dd_conv_last_error()
        assert call(0, *args, None, 1, 72, 72, 2, 2, 2, None) == DD_ERR_INVALID_ARG      # (bf16 too: the contract, not the kernels)
        assert call(3, *args, U.ptr(scale), 1, 72, 72, 2, 2, 3, None) == DD_ERR_INVALID_ARG and b"dd_conv_op" in lib.dd_conv_last_error()
        for prec in (0, 1, 5):
            assert call(0, *args, U.ptr(scale), 1, 72, 72, 2, 2, prec, None) == DD_ERR_UNSUPPORTED and b"precision" in lib.dd_conv_last_error()
        assert call(0, *args, U.ptr(scale), 1, 4, 72, 2, 2, 3, None) == DD_ERR_UNSUPPORTED
        assert b"multiples of 8 in 8..2048" in lib.dd_conv_last_error()
    assert lib.dd_conv_grad_scale(U.ptr(x), x.size, 3, None, None) == DD_ERR_INVALID_ARG and b"scale" in lib.dd_conv_last_error()
    assert lib.dd_conv_grad_scale(None, 4, 3, U.ptr(scale), None) == DD_ERR_INVALID_ARG
    assert lib.dd_conv_grad_scale(U.ptr(x), -1, 3, U.ptr(scale), None) == DD_ERR_INVALID_ARG
    assert lib.dd_conv_grad_scale(U.ptr(x), x.size, 1, U.ptr(scale), None) == DD_ERR_UNSUPPORTED
    assert lib.dd_conv_grad_scale(U.ptr(x), 0, 3, U.ptr(scale), None) == 0 and scale[0] == 1.0 and scale[1] == 1.0
