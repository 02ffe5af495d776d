"""CPU: csrc/dd_bn.hip + csrc/dd_api_bn.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h and executed work-item by work-item:
the six calls of include/ddepth_bn.h against the torch CPU references of tests/bn_cases.py, at the shapes and cases the GPU tests use
(tests/test_zz_gpu_bn.py), under both wave schedules of the emulation.  The two translation units and the emulation's globals
(tests/host_emul/ddepth_host.cpp) make a small shared object of their own; "device" memory is host memory, so numpy arrays are the tensors."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import bn_cases as BC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_bn.hip"), os.path.join(U.CSRC, "dd_api_bn.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_bn.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"), os.path.join(U.ROOT, "include", "ddepth_bn.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]


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
        out = os.path.join(U.OUT, "bn_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_bn_hostemu.so")
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
    c_int, c_vp, c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    lib.dd_bn_last_error.restype = ctypes.c_char_p
    lib.dd_bn_workspace_bytes.argtypes = [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.dd_bn_stats.argtypes = [c_vp] * 3 + [c_int] * 3 + [c_vp]
    lib.dd_bn_finalize.argtypes = [c_vp, c_f, c_f, c_vp, c_vp, c_vp, c_int, c_vp]
    lib.dd_bn_apply.argtypes = [c_vp] * 5 + [c_int, c_f] + [c_int] * 3 + [c_vp]
    lib.dd_bn_backward_reduce.argtypes = [c_vp] * 5 + [c_int, c_f, c_vp, c_vp] + [c_int] * 3 + [c_vp]
    lib.dd_bn_backward_apply.argtypes = [c_vp] * 8 + [c_int, c_f] + [c_int] * 3 + [c_vp]
    lib.emu_set_order.argtypes = [c_int]
    return lib


def ok(lib, rc):
    assert rc == 0, lib.dd_bn_last_error()


SENTINEL = np.float32(-12345.678)
_slack = []      # (buffer, start, size) of every tensor handed to the library: what lies around the tensor must come back untouched


def unaligned(a, offset_floats):
    """A copy of `a` whose first element sits `offset_floats` floats behind a 64-byte boundary (the planes' alignment is the test's choice), with
    sentinel values in front of and behind it."""
    buf = np.full(a.size + 48, SENTINEL, dtype=a.dtype)
    start = 16 + (-(buf.ctypes.data // a.itemsize + 16) % 16 + offset_floats) % 16
    view = buf[start:start + a.size].reshape(a.shape)
    view[...] = a
    assert (view.ctypes.data // 4) % 16 == offset_floats % 16
    _slack.append((buf, start, a.size))
    return view


def check_slack():
    for buf, start, size in _slack:
        assert (buf[:start] == SENTINEL).all() and (buf[start + size:] == SENTINEL).all(), "a kernel wrote outside a tensor"
    _slack.clear()


def run_six(lib, shape, act, affine, kind, offsets=(0, 0, 0, 0)):
    """The six calls on numpy memory; offsets = misalignment (in floats) of x, y, grad_y, grad_x."""
    inp = BC.make_inputs(shape, act, affine, kind)
    B, C, H, W = shape
    HW = H * W
    act_id, slope = BC.ACTS[act]
    x = unaligned(inp["x"].numpy(), offsets[0])
    gy = unaligned(inp["grad_y"].numpy(), offsets[2])
    w = inp["weight"].numpy().copy() if affine else None
    b = inp["bias"].numpy().copy() if affine else None
    rm, rv = inp["running_mean"].numpy().copy(), inp["running_var"].numpy().copy()
    n = ctypes.c_int64(0)
    ok(lib, lib.dd_bn_workspace_bytes(B, C, HW, ctypes.byref(n)))
    ws = np.zeros(n.value, dtype=np.uint8)
    guard = np.full(64, 0x5A, dtype=np.uint8)
    ws_all = np.concatenate([ws, guard])      # the calls stay inside the size they asked for
    sums = np.full(2 * C + 1, np.nan)
    ok(lib, lib.dd_bn_stats(U.ptr(x), U.ptr(sums), U.ptr(ws_all), B, C, HW, None))
    assert sums[2 * C] == B * HW
    mi = np.full(2 * C, np.nan, dtype=np.float32)
    ok(lib, lib.dd_bn_finalize(U.ptr(sums), BC.EPS, BC.MOMENTUM, U.ptr(mi), U.ptr(rm), U.ptr(rv), C, None))
    y = unaligned(np.full(shape, np.nan, dtype=np.float32), offsets[1])
    ok(lib, lib.dd_bn_apply(U.ptr(x), U.ptr(mi), U.ptr(w), U.ptr(b), U.ptr(y), act_id, slope, B, C, HW, None))
    sums2 = np.full(2 * C, np.nan)
    ok(lib, lib.dd_bn_backward_reduce(U.ptr(x), U.ptr(gy), U.ptr(mi), U.ptr(w), U.ptr(b), act_id, slope, U.ptr(sums2), U.ptr(ws_all), B, C, HW, None))
    gx = unaligned(np.full(shape, np.nan, dtype=np.float32), offsets[3])
    ok(lib, lib.dd_bn_backward_apply(U.ptr(x), U.ptr(gy), U.ptr(mi), U.ptr(w), U.ptr(b), U.ptr(sums2), U.ptr(sums), U.ptr(gx), act_id, slope,
                                     B, C, HW, None))
    assert (ws_all[n.value:] == 0x5A).all(), "a call wrote behind its workspace"
    check_slack()
    return {"y": y.copy(), "grad_x": gx.copy(), "grad_weight": sums2[C:].astype(np.float32), "grad_bias": sums2[:C].astype(np.float32),
            "running_mean": rm, "running_var": rv, "sums": sums, "sums2": sums2}


@pytest.mark.parametrize("variant", BC.VARIANTS, ids=BC.variant_id)
@pytest.mark.parametrize("shape", BC.SHAPES, ids=str)
def test_six_calls_against_torch_cpu(lib, shape, variant):
    act, affine, kind = variant
    lib.emu_set_order(0)
    BC.check(run_six(lib, shape, act, affine, kind), shape, act, affine, kind, "hostemu")


@pytest.mark.parametrize("shape", BC.SHAPES[:3], ids=str)
def test_bits_do_not_depend_on_the_wave_schedule_or_the_alignment(lib, shape):
    """The last wave running ahead instead of the first (a missing barrier shows), and every tensor at another misalignment -- the all-scalar
    path where they disagree: the reductions add in another order then, so those runs are held to the tolerance rule, not to equal bits."""
    lib.emu_set_order(0)
    a = run_six(lib, shape, "leaky", True, "normal")
    lib.emu_set_order(1)
    b = run_six(lib, shape, "leaky", True, "normal")
    lib.emu_set_order(0)
    for k in ("y", "grad_x", "sums", "sums2", "running_mean", "running_var"):
        assert np.array_equal(a[k], b[k]), k
    c = run_six(lib, shape, "leaky", True, "normal", offsets=(1, 1, 1, 1))      # aligned to each other, 4 bytes off a 16-byte boundary
    d = run_six(lib, shape, "leaky", True, "normal", offsets=(0, 3, 2, 1))      # no two agree: all scalar
    for r in (c, d):
        BC.check(r, shape, "leaky", True, "normal", "hostemu-misaligned")


def test_argument_checks(lib):
    n = ctypes.c_int64(0)
    assert lib.dd_bn_workspace_bytes(0, 4, 4, ctypes.byref(n)) != 0 and b"positive" in lib.dd_bn_last_error()
    assert lib.dd_bn_stats(None, None, None, 1, 1, 1, None) != 0 and b"null" in lib.dd_bn_last_error()
    x = np.zeros(4, dtype=np.float32)
    mi = np.zeros(2, dtype=np.float32)
    assert lib.dd_bn_apply(U.ptr(x), U.ptr(mi), None, None, U.ptr(x), 0, 0.0, 1, 1, 4, None) != 0 and b"alias" in lib.dd_bn_last_error()
    y = np.zeros(4, dtype=np.float32)
    assert lib.dd_bn_apply(U.ptr(x), U.ptr(mi), None, None, U.ptr(y), 7, 0.0, 1, 1, 4, None) != 0 and b"dd_bn_act" in lib.dd_bn_last_error()
