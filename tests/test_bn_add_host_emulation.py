"""CPU: csrc/dd_bn.hip + csrc/dd_api_bn.cpp compiled for the host on top of tests/host_emul/hip/hip_runtime.h and executed work-item by work-item:
the two calls of include/ddepth_bn_add.h (with the calls of include/ddepth_bn.h around them) against the torch CPU references of
tests/bn_add_cases.py, at the shapes and cases the GPU tests use (tests/test_zz_gpu_bn_add.py), under both wave schedules of the emulation, plus
the exact identities that tie the new kernels to the existing ones.  "Device" memory is host memory, so numpy arrays are the tensors; every
tensor sits between sentinel values and the workspace in front of a guard, and all of them must come back untouched."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import bn_add_cases as AC
import bn_cases as BC
import hostemu_util as U

UNITS = [os.path.join(U.CSRC, "dd_bn.hip"), os.path.join(U.CSRC, "dd_api_bn.cpp"), os.path.join(U.EMU, "ddepth_host.cpp")]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_bn.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"), os.path.join(U.ROOT, "include", "ddepth_bn.h"),
                os.path.join(U.ROOT, "include", "ddepth_bn_add.h"), os.path.join(U.ROOT, "include", "ddepth.h")]
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
PRE, POST = 0, 1
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
        out = os.path.join(U.OUT, "bnadd_" + hsh.hexdigest()[:12])
        so = os.path.join(out, "libddepth_bn_add_hostemu.so")
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
    lib.dd_bn_apply_add.argtypes = [c_vp] * 6 + [c_int, c_f, c_int] + [c_int] * 3 + [c_vp]
    lib.dd_bn_backward_reduce_add.argtypes = [c_vp] * 4 + [c_int, c_f, c_vp, c_vp, c_vp] + [c_int] * 3 + [c_vp]
    lib.emu_set_order.argtypes = [c_int]
    return lib


def ok(lib, rc):
    assert rc == 0, lib.dd_bn_last_error()


SENTINEL = np.float32(-12345.678)
_slack = []      # (buffer, start, size) of every tensor handed to the library: what lies around the tensor must come back untouched


def unaligned(a, offset_floats):
    """A copy of `a` whose first element sits `offset_floats` floats behind a 64-byte boundary, with sentinel values in front of and behind it."""
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


class Calls:
    """The calls of the two headers on numpy memory for one (B, C, H, W), with one guarded workspace."""

    def __init__(self, lib, shape):
        self.lib, self.shape = lib, shape
        self.B, self.C, self.HW = shape[0], shape[1], shape[2] * shape[3]
        n = ctypes.c_int64(0)
        ok(lib, lib.dd_bn_workspace_bytes(self.B, self.C, self.HW, ctypes.byref(n)))
        self.ws_bytes = n.value
        self.ws = np.concatenate([np.zeros(n.value, dtype=np.uint8), np.full(64, 0x5A, dtype=np.uint8)])

    def dims(self):
        return self.B, self.C, self.HW, None

    def empty(self, offset):
        return unaligned(np.full(self.shape, np.nan, dtype=np.float32), offset)

    def stats(self, x):
        sums = np.full(2 * self.C + 1, np.nan)
        ok(self.lib, self.lib.dd_bn_stats(U.ptr(x), U.ptr(sums), U.ptr(self.ws), *self.dims()))
        return sums

    def finalize(self, sums, rm=None, rv=None):
        mi = np.full(2 * self.C, np.nan, dtype=np.float32)
        ok(self.lib, self.lib.dd_bn_finalize(U.ptr(sums), BC.EPS, BC.MOMENTUM, U.ptr(mi), U.ptr(rm), U.ptr(rv), self.C, None))
        return mi

    def apply(self, x, mi, w, b, act, slope, offset=0):
        y = self.empty(offset)
        ok(self.lib, self.lib.dd_bn_apply(U.ptr(x), U.ptr(mi), U.ptr(w), U.ptr(b), U.ptr(y), act, slope, *self.dims()))
        return y

    def apply_add(self, x, mi, w, b, r, act, slope, mode, offset=0):
        y = self.empty(offset)
        ok(self.lib, self.lib.dd_bn_apply_add(U.ptr(x), U.ptr(mi), U.ptr(w), U.ptr(b), U.ptr(r), U.ptr(y), act, slope, mode, *self.dims()))
        return y

    def backward_reduce(self, x, gy, mi, w, b, act, slope):
        sums2 = np.full(2 * self.C, np.nan)
        ok(self.lib, self.lib.dd_bn_backward_reduce(U.ptr(x), U.ptr(gy), U.ptr(mi), U.ptr(w), U.ptr(b), act, slope, U.ptr(sums2), U.ptr(self.ws),
                                                    *self.dims()))
        return sums2

    def backward_reduce_add(self, x, gy, y, mi, act, slope, offset=0):
        g, sums2 = self.empty(offset), np.full(2 * self.C, np.nan)
        ok(self.lib, self.lib.dd_bn_backward_reduce_add(U.ptr(x), U.ptr(gy), U.ptr(y), U.ptr(mi), act, slope, U.ptr(g), U.ptr(sums2),
                                                        U.ptr(self.ws), *self.dims()))
        return g, sums2

    def backward_apply(self, x, gy, mi, w, b, sums2, sums, act, slope, offset=0):
        gx = self.empty(offset)
        ok(self.lib, self.lib.dd_bn_backward_apply(U.ptr(x), U.ptr(gy), U.ptr(mi), U.ptr(w), U.ptr(b), U.ptr(sums2), U.ptr(sums), U.ptr(gx), act,
                                                   slope, *self.dims()))
        return gx

    def done(self):
        assert (self.ws[self.ws_bytes:] == 0x5A).all(), "a call wrote behind its workspace"
        check_slack()


def run_add(lib, shape, variant, offsets=(0, 0, 0, 0, 0, 0)):
    """Forward and backward of one case; offsets = misalignment (in floats) of x, addend, y, grad_y, g, grad_x."""
    mode, act, affine, kind = variant
    inp = AC.make_inputs(shape, mode, act, affine, kind)
    act_id, slope = AC.ACTS[act]
    k = Calls(lib, shape)
    x, r = unaligned(inp["x"].numpy(), offsets[0]), unaligned(inp["addend"].numpy(), offsets[1])
    gy = unaligned(inp["grad_y"].numpy(), offsets[3])
    w = inp["weight"].numpy().copy() if affine else None
    b = inp["bias"].numpy().copy() if affine else None
    rm, rv = inp["running_mean"].numpy().copy(), inp["running_var"].numpy().copy()
    sums = k.stats(x)
    assert sums[2 * k.C] == k.B * k.HW
    mi = k.finalize(sums, rm, rv)
    y = k.apply_add(x, mi, w, b, r, act_id, slope, AC.MODES[mode], offsets[2])
    if mode == "pre":
        g, sums2 = k.backward_reduce_add(x, gy, y, mi, act_id, slope, offsets[4])
        gx = k.backward_apply(x, g, mi, w, None, sums2, sums, ACT_NONE, 0.0, offsets[5])
    else:
        g = gy
        sums2 = k.backward_reduce(x, gy, mi, w, b, act_id, slope)
        gx = k.backward_apply(x, gy, mi, w, b, sums2, sums, act_id, slope, offsets[5])
    k.done()
    C = k.C
    return {"y": y.copy(), "grad_x": gx.copy(), "grad_addend": g.copy(), "grad_weight": sums2[C:].astype(np.float32),
            "grad_bias": sums2[:C].astype(np.float32), "running_mean": rm, "running_var": rv, "sums": sums, "sums2": sums2}


@pytest.mark.parametrize("variant", AC.VARIANTS, ids=AC.variant_id)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_all_cases_against_torch_cpu(lib, shape, variant):
    lib.emu_set_order(0)
    AC.check(run_add(lib, shape, variant), shape, *variant, "hostemu")


@pytest.mark.parametrize("mode", list(AC.MODES))
@pytest.mark.parametrize("shape", AC.SHAPES[:3], ids=str)
def test_bits_do_not_depend_on_the_wave_schedule_and_misaligned_tensors_hold_the_tolerance(lib, shape, mode):
    """The last wave running ahead instead of the first (a missing barrier shows).  Then every tensor 4 bytes off a 16-byte boundary (vectors
    behind a scalar head) and no two tensors agreeing (the all-scalar path): the reductions add in another order, so the tolerance rule holds
    those runs, not equal bits."""
    variant = (mode, "leaky", True, "normal")
    lib.emu_set_order(0)
    a = run_add(lib, shape, variant)
    lib.emu_set_order(1)
    b = run_add(lib, shape, variant)
    lib.emu_set_order(0)
    for k in ("y", "grad_x", "grad_addend", "sums", "sums2", "running_mean", "running_var"):
        assert np.array_equal(a[k], b[k]), k
    for offsets in ((1, 1, 1, 1, 1, 1), (0, 3, 2, 1, 7, 5)):
        AC.check(run_add(lib, shape, variant, offsets), shape, *variant, f"hostemu-misaligned{offsets}")


def _setup(lib, shape, mode, act, affine=True):
    inp = AC.make_inputs(shape, mode, act, affine, "normal")
    k = Calls(lib, shape)
    x, r, gy = (unaligned(inp[n].numpy(), 0) for n in ("x", "addend", "grad_y"))
    w, b = inp["weight"].numpy().copy(), inp["bias"].numpy().copy()
    mi = k.finalize(k.stats(x))
    return k, x, r, gy, w, b, mi


@pytest.mark.parametrize("act", list(AC.ACTS))
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_identity_a_pre_with_a_zero_addend_is_dd_bn_apply(lib, shape, act):
    lib.emu_set_order(0)
    act_id, slope = AC.ACTS[act]
    k, x, r, gy, w, b, mi = _setup(lib, shape, "pre", act)
    zero = unaligned(np.zeros(shape, dtype=np.float32), 0)
    assert np.array_equal(k.apply_add(x, mi, w, b, zero, act_id, slope, PRE), k.apply(x, mi, w, b, act_id, slope))
    k.done()


@pytest.mark.parametrize("act", list(AC.ACTS))
@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_identity_b_post_is_dd_bn_apply_plus_the_addend_in_fp32(lib, shape, act):
    lib.emu_set_order(0)
    act_id, slope = AC.ACTS[act]
    k, x, r, gy, w, b, mi = _setup(lib, shape, "post", act)
    want = (k.apply(x, mi, w, b, act_id, slope) + r).astype(np.float32)
    assert np.array_equal(k.apply_add(x, mi, w, b, r, act_id, slope, POST), want)
    k.done()


@pytest.mark.parametrize("shape", AC.SHAPES, ids=str)
def test_identities_c_and_d_pre_relu_forward_mask_and_sums(lib, shape):
    """(c) y = max(dd_bn_apply(act none) + r, 0) in numpy fp32; (d) g = grad_y * (y > 0), and sums2 has the bits dd_bn_backward_reduce gives
    on (x, g) without an activation."""
    lib.emu_set_order(0)
    k, x, r, gy, w, b, mi = _setup(lib, shape, "pre", "relu")
    y = k.apply_add(x, mi, w, b, r, ACT_RELU, 0.0, PRE)
    want = np.maximum((k.apply(x, mi, w, b, ACT_NONE, 0.0) + r).astype(np.float32), np.float32(0))
    assert np.array_equal(y, want)
    g, sums2 = k.backward_reduce_add(x, gy, y, mi, ACT_RELU, 0.0)
    assert np.array_equal(g, gy * (y > 0))
    assert np.array_equal(sums2, k.backward_reduce(x, g, mi, None, None, ACT_NONE, 0.0))
    k.done()


def test_argument_checks(lib):
    x, r, y, gy, g = (np.zeros(4, dtype=np.float32) for _ in range(5))
    mi = np.zeros(2, dtype=np.float32)
    sums2, ws = np.zeros(2), np.zeros(1024, dtype=np.uint8)
    P = U.ptr
    err = lib.dd_bn_last_error
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, None, P(y), 0, 0.0, PRE, 1, 1, 4, None) == DD_ERR_INVALID_ARG and b"null" in err()
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(x), 0, 0.0, PRE, 1, 1, 4, None) == DD_ERR_INVALID_ARG and b"alias" in err()
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(r), 0, 0.0, POST, 1, 1, 4, None) == DD_ERR_INVALID_ARG and b"alias" in err()
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(y), 0, 0.0, 2, 1, 1, 4, None) == DD_ERR_INVALID_ARG and b"add_mode" in err()
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(y), 7, 0.0, PRE, 1, 1, 4, None) == DD_ERR_INVALID_ARG and b"dd_bn_act" in err()
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(y), 0, 0.0, PRE, 1, 0, 4, None) == DD_ERR_INVALID_ARG and b"positive" in err()
    # a negative slope is fine in the forward (both modes) and in the POST backward (the existing reduce); the PRE backward cannot read its mask from y
    assert lib.dd_bn_apply_add(P(x), P(mi), None, None, P(r), P(y), ACT_LEAKY, -0.5, PRE, 1, 1, 4, None) == 0
    args = (P(sums2), P(ws), 1, 1, 4, None)
    assert lib.dd_bn_backward_reduce_add(P(x), P(gy), P(y), P(mi), ACT_LEAKY, -0.5, P(g), *args) == DD_ERR_UNSUPPORTED and b"negative slope" in err()
    assert lib.dd_bn_backward_reduce_add(P(x), P(gy), P(y), P(mi), ACT_LEAKY, 0.0, P(g), *args) == 0
    assert lib.dd_bn_backward_reduce_add(P(x), P(gy), None, P(mi), ACT_RELU, 0.0, P(g), *args) == DD_ERR_INVALID_ARG and b"null" in err()
    assert lib.dd_bn_backward_reduce_add(P(x), P(gy), P(y), P(mi), ACT_RELU, 0.0, None, *args) == DD_ERR_INVALID_ARG and b"null" in err()
    for alias in (x, gy, y):
        assert lib.dd_bn_backward_reduce_add(P(x), P(gy), P(y), P(mi), ACT_RELU, 0.0, P(alias), *args) == DD_ERR_INVALID_ARG and b"alias" in err()
    assert lib.dd_bn_backward_reduce_add(P(x), P(gy), P(y), P(mi), 9, 0.0, P(g), *args) == DD_ERR_INVALID_ARG and b"dd_bn_act" in err()
