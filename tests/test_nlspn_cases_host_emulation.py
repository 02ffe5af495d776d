"""CPU: the cases of tests/nlspn_cases.py -- NLSPN propagation, both affinity stages and the DCNv2 operator at the places where the kernels of
csrc/dd_dcn.hip branch -- on the host-emulated library (tests/hostemu_util.py; dd_dcn.hip is one of its sources), through the C ABI of
include/ddepth_dcn.h; the kernels that stage a tile in LDS run under both wave schedules of the emulation, bit-equal.  Every output lies between sentinel bands that must be intact after the call, every input must be bit-identical after it.
The conditions a case has to meet to reach its branch are asserted from index arithmetic alone (the first two tests need no library)."""
import ctypes

import numpy as np
import pytest

import hostemu_util as U
import nlspn_cases as NC

WHERE = "hostemu"


def test_main_shape_reaches_the_fallback_sampler_and_every_seam():
    for k_f in NC.KFS:
        NC.check_prop_conditions(k_f)


def test_dcn_cases_have_two_slabs_and_integer_positions():
    NC.check_dcn_conditions()


@pytest.fixture(scope="module")
def lib():
    lib = U.build_library()
    c_int, c_vp = ctypes.c_int, ctypes.c_void_p
    lib.dd_dcn_last_error.restype = ctypes.c_char_p
    lib.dd_dcn_forward.argtypes = [c_vp] * 6 + [c_int] * 16 + [c_vp]
    lib.dd_dcn_backward.argtypes = [c_vp] * 11 + [c_int] * 16 + [c_vp]
    lib.dd_nlspn_offset_affinity.argtypes = [c_vp] * 7 + [c_int] * 7 + [c_vp]
    lib.dd_nlspn_guided_offset_affinity.argtypes = [c_vp] * 9 + [c_int] * 9 + [c_vp]
    lib.dd_nlspn_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.dd_nlspn_propagate.argtypes = [c_vp] * 8 + [c_int] * 6 + [c_vp]
    lib.emu_launch_count.restype = ctypes.c_ulong
    lib.emu_set_order.argtypes = [c_int]
    return lib


P = U.ptr


def run_prop(lib, feat, offset, aff, fix, w, b, k_f, prop_time, preserve):
    B, _, H, W = feat.shape
    g = NC.Guarded()
    a = [g.inp(t) for t in (feat, offset, aff, fix, w, b)]
    feats = g.out((prop_time, B, 1, H, W))
    ws = None
    if preserve:
        nb = ctypes.c_int64()
        assert lib.dd_nlspn_workspace_bytes(B, H, W, 1, ctypes.byref(nb)) == 0
        assert nb.value == 2 * B * H * W * 4
        ws = g.out((nb.value // 4,))
    n0 = lib.emu_launch_count()
    rc = lib.dd_nlspn_propagate(P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[4]), P(a[5]), P(feats), P(ws), B, H, W, k_f, prop_time, preserve, None)
    assert rc == 0, lib.dd_dcn_last_error()
    assert lib.emu_launch_count() - n0 == prop_time + (1 if preserve else 0)
    g.check()
    return feats.copy()


def run_affinity(lib, raw, conf, gamma, w_conf, b_conf, k_f, mode, conf_prop, legacy):
    B, _, H, W = raw.shape
    K = k_f * k_f
    g = NC.Guarded()
    a = [g.inp(t) for t in (raw, conf, gamma, w_conf, b_conf)]
    offset, aff = g.out((B, 2 * K, H, W)), g.out((B, K, H, W))
    rc = lib.dd_nlspn_offset_affinity(*[P(t) for t in a], P(offset), P(aff), B, H, W, k_f, mode, conf_prop, legacy, None)
    assert rc == 0, lib.dd_dcn_last_error()
    g.check()
    return offset.copy(), aff.copy()


def run_guided(lib, guide, cw, cb, conf, gamma, w_conf, b_conf, mode, conf_prop, legacy):
    B, _, H, W = guide.shape
    g = NC.Guarded()
    a = [g.inp(t) for t in (guide, cw, cb, conf, gamma, w_conf, b_conf)]
    offset, aff = g.out((B, 18, H, W)), g.out((B, 9, H, W))
    rc = lib.dd_nlspn_guided_offset_affinity(*[P(t) for t in a], P(offset), P(aff), B, 8, H, W, 3, 3, mode, conf_prop, legacy, None)
    assert rc == 0, lib.dd_dcn_last_error()
    g.check()
    return offset.copy(), aff.copy()


def run_dcn(lib, x, w, b, off, m, go, geo):
    g = NC.Guarded()
    a = [g.inp(t) for t in (x, w, b, off, m, go)]
    out = g.out(go.shape)
    assert lib.dd_dcn_forward(*[P(t) for t in a[:5]], P(out), *geo, None) == 0, lib.dd_dcn_last_error()
    grads = [g.out(t.shape) for t in (x, off, m, w, b)]
    assert lib.dd_dcn_backward(*[P(t) for t in a], *[P(t) for t in grads], *geo, None) == 0, lib.dd_dcn_last_error()
    g.check()
    return out.copy(), [t.copy() for t in grads]


def bound(f, lib):
    return lambda *a: f(lib, *a)


def both_orders(f, lib):
    """f under both wave schedules of the emulation (the first / the last wave runs ahead as far as the barriers allow), bit-equal."""
    def g(*a):
        lib.emu_set_order(0)
        r0 = f(lib, *a)
        lib.emu_set_order(1)
        try:
            r1 = f(lib, *a)
        finally:
            lib.emu_set_order(0)
        for x, y in zip(r0, r1) if isinstance(r0, tuple) else ((r0, r1),):
            assert np.array_equal(NC.bits(x), NC.bits(y)), "the wave schedule shows"
        return r0
    return g


@pytest.fixture()
def default_kernel(monkeypatch):
    monkeypatch.delenv("DD_NLSPN_KERNEL", raising=False)


@pytest.mark.parametrize("case", NC.prop_cases(), ids=NC.case_id)
def test_propagation_against_the_fp64_oracle(lib, default_kernel, case):
    NC.check_prop_real(both_orders(run_prop, lib), *case, where=WHERE)


@pytest.mark.parametrize("case", NC.exact_cases(), ids=NC.case_id)
def test_propagation_exact_cases_are_bit_equal(lib, default_kernel, case):
    NC.check_prop_exact(both_orders(run_prop, lib), *case)


@pytest.mark.parametrize("case", NC.variant_cases(), ids=NC.case_id)
def test_kernel_variants(lib, monkeypatch, case):
    def set_variant(v):
        if v is None:
            monkeypatch.delenv("DD_NLSPN_KERNEL", raising=False)
        else:
            monkeypatch.setenv("DD_NLSPN_KERNEL", v)
    NC.check_variant(bound(run_prop, lib), set_variant, *case, where=WHERE)


@pytest.mark.parametrize("case", NC.affinity_grid(), ids=NC.case_id)
def test_affinity_stage_against_the_fp64_oracle(lib, case):
    NC.check_affinity(bound(run_affinity, lib), *case, where=WHERE)


@pytest.mark.parametrize("case", [c[1:] for c in NC.affinity_grid((3,))], ids=NC.case_id)
def test_guided_affinity_stage_against_the_fp64_oracle(lib, case):
    NC.check_guided(both_orders(run_guided, lib), *case, where=WHERE)


@pytest.mark.parametrize("name", list(NC.DCN_CASES))
def test_dcn_forward_and_gradients_against_the_fp64_oracle(lib, name):
    NC.check_dcn(bound(run_dcn, lib), name, where=WHERE)
