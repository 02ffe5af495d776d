"""GPU (`-m gpu`): the cases of tests/nlspn_cases.py -- NLSPN propagation (every k_f, every DD_NLSPN_KERNEL variant), both affinity stages over the
whole mode x conf_prop x legacy grid and the DCNv2 operator with two gradient slabs and integer sampling positions -- through the built
library on the MI355X.  Each call goes to the C ABI of include/ddepth_dcn.h (diffusiondepth_amd.dcn's bound library) on device tensors that
lie between sentinel bands, which must be intact afterwards, with inputs that must be bit-identical afterwards; the drop-in functions of
diffusiondepth_amd.dcn then have to return the same bits (where no atomics are involved).  Measured errors go to the parity report (gpu_util.record)."""
import ctypes

import numpy as np
import pytest
import torch

import nlspn_cases as NC

pytestmark = pytest.mark.gpu
WHERE = "gpu"
MODE_NAME = {v: k for k, v in NC.MODES.items()}


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a HIP device: the product has no CPU fallback")
    import gpu_util
    return gpu_util


class Guarded:
    """Device tensors with NC.GUARD sentinel floats in front of and behind them (64 bytes: the 16-byte alignment of the allocation stays)."""

    def __init__(self):
        self.bufs = []

    def _place(self, shape, src):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * NC.GUARD,), float(NC.SENTINEL), dtype=torch.float32, device="cuda")
        view = buf[NC.GUARD:NC.GUARD + n].view(*shape)
        if src is None:
            view.fill_(float("nan"))
        else:
            view.copy_(torch.tensor(src))
        self.bufs.append((buf, view, src))
        return view

    def out(self, shape):
        return self._place(tuple(shape), None)

    def inp(self, a):
        return None if a is None else self._place(a.shape, a)

    def check(self):
        torch.cuda.synchronize()
        for buf, view, src in self.bufs:
            edge = torch.cat([buf[:NC.GUARD], buf[NC.GUARD + view.numel():]]).cpu().numpy()
            assert (edge == NC.SENTINEL).all(), "the library wrote outside a tensor"
            if src is not None:
                assert np.array_equal(NC.bits(view.cpu().numpy()), NC.bits(src)), "the library wrote to an input"


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def same_bits(a, b):
    return np.array_equal(NC.bits(a.cpu().numpy()), NC.bits(b.cpu().numpy()))


def run_prop(feat, offset, aff, fix, w, b, k_f, prop_time, preserve):
    from diffusiondepth_amd import dcn
    lib = dcn._lib()
    B, _, H, W = feat.shape
    g = Guarded()
    a = [g.inp(t) for t in (feat, offset, aff, fix, w, b)]
    feats = g.out((prop_time, B, 1, H, W))
    ws = None
    if preserve:
        nb = ctypes.c_int64()
        assert lib.dd_nlspn_workspace_bytes(B, H, W, 1, ctypes.byref(nb)) == 0 and nb.value == 2 * B * H * W * 4
        ws = g.out((nb.value // 4,))
    rc = lib.dd_nlspn_propagate(*[P(t) for t in a], P(feats), P(ws), B, H, W, k_f, prop_time, preserve, stream())
    assert rc == 0, lib.dd_dcn_last_error()
    g.check()
    again = dcn.nlspn_propagate(a[0], a[1], a[2], a[3], a[4], a[5], k_f, prop_time, bool(preserve))
    assert same_bits(again, feats), "diffusiondepth_amd.dcn.nlspn_propagate differs from the C ABI call"
    return feats.cpu().numpy()


def run_affinity(raw, conf, gamma, w_conf, b_conf, k_f, mode, conf_prop, legacy):
    from diffusiondepth_amd import dcn
    lib = dcn._lib()
    B, _, H, W = raw.shape
    K = k_f * k_f
    g = Guarded()
    a = [g.inp(t) for t in (raw, conf, gamma, w_conf, b_conf)]
    offset, aff = g.out((B, 2 * K, H, W)), g.out((B, K, H, W))
    rc = lib.dd_nlspn_offset_affinity(*[P(t) for t in a], P(offset), P(aff), B, H, W, k_f, mode, conf_prop, legacy, stream())
    assert rc == 0, lib.dd_dcn_last_error()
    g.check()
    o2, a2 = dcn.nlspn_offset_affinity(a[0], a[1], a[2], a[3], a[4], k_f, MODE_NAME[mode], bool(conf_prop), bool(legacy))
    assert same_bits(o2, offset) and same_bits(a2, aff), "diffusiondepth_amd.dcn.nlspn_offset_affinity differs from the C ABI call"
    return offset.cpu().numpy(), aff.cpu().numpy()


def run_guided(guide, cw, cb, conf, gamma, w_conf, b_conf, mode, conf_prop, legacy):
    from diffusiondepth_amd import dcn
    lib = dcn._lib()
    B, _, H, W = guide.shape
    g = Guarded()
    a = [g.inp(t) for t in (guide, cw, cb, conf, gamma, w_conf, b_conf)]
    offset, aff = g.out((B, 18, H, W)), g.out((B, 9, H, W))
    rc = lib.dd_nlspn_guided_offset_affinity(*[P(t) for t in a], P(offset), P(aff), B, 8, H, W, 3, 3, mode, conf_prop, legacy, stream())
    assert rc == 0, lib.dd_dcn_last_error()
    g.check()
    o2, a2 = dcn.nlspn_guided_offset_affinity(a[0], a[1], a[2], a[3], a[4], a[5], a[6], 3, 3, MODE_NAME[mode], bool(conf_prop), bool(legacy))
    assert same_bits(o2, offset) and same_bits(a2, aff), "diffusiondepth_amd.dcn.nlspn_guided_offset_affinity differs from the C ABI call"
    return offset.cpu().numpy(), aff.cpu().numpy()


def run_dcn(x, w, b, off, m, go, geo):
    from diffusiondepth_amd import dcn
    lib = dcn._lib()
    g = Guarded()
    a = [g.inp(t) for t in (x, w, b, off, m, go)]
    out = g.out(go.shape)
    assert lib.dd_dcn_forward(*[P(t) for t in a[:5]], P(out), *geo, stream()) == 0, lib.dd_dcn_last_error()
    grads = [g.out(t.shape) for t in (x, off, m, w, b)]
    assert lib.dd_dcn_backward(*[P(t) for t in a], *[P(t) for t in grads], *geo, stream()) == 0, lib.dd_dcn_last_error()
    g.check()
    kh, kw = w.shape[2:]
    tail = (kh, kw) + tuple(geo[7:])
    assert same_bits(dcn.modulated_deform_conv_forward(*a[:5], *tail), out), "the drop-in's forward differs from the C ABI call"
    g2 = dcn.modulated_deform_conv_backward(*a, *tail)
    assert same_bits(g2[1], grads[1]) and same_bits(g2[2], grads[2]), "the drop-in's offset / mask gradients differ from the C ABI call"
    return out.cpu().numpy(), [t.cpu().numpy() for t in grads]


@pytest.fixture()
def default_kernel(monkeypatch):
    monkeypatch.delenv("DD_NLSPN_KERNEL", raising=False)


@pytest.mark.parametrize("case", NC.prop_cases(), ids=NC.case_id)
def test_propagation_against_the_fp64_oracle(U, default_kernel, case):
    NC.check_prop_real(run_prop, *case, record=U.record, where=WHERE)


@pytest.mark.parametrize("case", NC.exact_cases(), ids=NC.case_id)
def test_propagation_exact_cases_are_bit_equal(U, default_kernel, case):
    NC.check_prop_exact(run_prop, *case)


@pytest.mark.parametrize("case", NC.variant_cases(), ids=NC.case_id)
def test_kernel_variants(U, monkeypatch, case):
    def set_variant(v):
        if v is None:
            monkeypatch.delenv("DD_NLSPN_KERNEL", raising=False)
        else:
            monkeypatch.setenv("DD_NLSPN_KERNEL", v)
    NC.check_variant(run_prop, set_variant, *case, record=U.record, where=WHERE)


@pytest.mark.parametrize("case", NC.affinity_grid(), ids=NC.case_id)
def test_affinity_stage_against_the_fp64_oracle(U, case):
    NC.check_affinity(run_affinity, *case, record=U.record, where=WHERE)


@pytest.mark.parametrize("case", [c[1:] for c in NC.affinity_grid((3,))], ids=NC.case_id)
def test_guided_affinity_stage_against_the_fp64_oracle(U, case):
    NC.check_guided(run_guided, *case, record=U.record, where=WHERE)


@pytest.mark.parametrize("name", list(NC.DCN_CASES))
def test_dcn_forward_and_gradients_against_the_fp64_oracle(U, name):
    NC.check_dcn(run_dcn, name, record=U.record, where=WHERE)
