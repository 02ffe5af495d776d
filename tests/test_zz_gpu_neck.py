"""GPU (`-m gpu`): the HAHI neck and the condition pyramid behind it (dd_neck_condition / dd_condition; kernel ids 30..41 and 54..65, the lateral
ids 10..13 / 15..18 / 24..26 and KID_FPN_UP) against the fp64 oracle (oracle.ddim_oracle.hahi_neck -> fpn_aggregate) in all five precisions, at the
shapes of tests/neck_cases.py: two tiles across with one-pixel remainders, exact tiles, less than a tile, three tiles per axis; B = 2 and 3 for both
pyramids.  The bounds come from the oracle's own fp32 evaluation and from its operand-rounding emulations (neck_cases docstring), never from
what the kernels give.  Around that: which kernel ids a call launches, images of a batch against the same images run alone, a workspace reused
across shapes and across neck / no neck, and a NaN staying inside its image -- all bit for bit.

The fp64 reference and its three error maps are computed once per (pyramid, shape, neck) on the host and shared by every test; that is where this
module's time goes, each device call takes milliseconds.

Measured on an MI355X (`neck_parity` lines of the parity report; per pyramid and precision the shape nearest to a bound; measured / bound;
max-abs over max|ref|, the worst strip and the per-image distance from the emulation as relative L2; 80 cases, all inside):
                        shape  max-abs            worst strip                     distance from the emulation
  neck    swin  fp32    B      1.62e-06 / 2.00e-05   row7     7.09e-07 / 2.00e-05   -
  neck    swin  f16x3   C      1.40e-06 / 2.00e-05   row0     4.78e-07 / 2.00e-05   -          (f16r: the same kernels, the same bits)
  neck    swin  bf16    A      5.44e-03 / 1.63e-02   col_last 2.50e-03 / 6.89e-03   9.19e-04 / 3.24e-03
  neck    swin  f16     C      5.99e-04 / 1.56e-03   col_last 3.68e-04 / 8.55e-04   2.32e-04 / 8.19e-04
  neck    mpvit fp32    A      9.80e-07 / 2.00e-05   row7     5.07e-07 / 2.00e-05   -
  neck    mpvit f16x3   A      9.28e-07 / 2.00e-05   row8     4.58e-07 / 2.00e-05   -
  neck    mpvit bf16    C      4.20e-03 / 1.03e-02   row_last 2.15e-03 / 5.72e-03   9.27e-04 / 2.64e-03      (shape D: 1.11e-03 / 2.83e-03)
  neck    mpvit f16     B      6.61e-04 / 1.24e-03   col_last 3.39e-04 / 7.49e-04   2.27e-04 / 7.95e-04
  pyramid swin  fp32    C      1.46e-06 / 2.00e-05   col0     4.62e-07 / 2.00e-05   -
  pyramid swin  f16x3   C      9.76e-07 / 2.00e-05   col0     3.07e-07 / 2.00e-05   -
  pyramid swin  bf16    C      2.57e-03 / 7.33e-03   row_last 1.99e-03 / 5.55e-03   6.55e-04 / 2.49e-03
  pyramid swin  f16     C      5.14e-04 / 1.04e-03   col0     3.05e-04 / 6.51e-04   2.21e-04 / 7.25e-04
  pyramid mpvit fp32    A      1.30e-06 / 2.00e-05   col31    4.97e-07 / 2.00e-05   -
  pyramid mpvit f16x3   B      6.66e-07 / 2.00e-05   row8     3.25e-07 / 2.00e-05   -
  pyramid mpvit bf16    C      2.72e-03 / 7.00e-03   col_last 1.92e-03 / 5.40e-03   6.64e-04 / 2.36e-03
  pyramid mpvit f16     A      4.36e-04 / 7.91e-04   row0     3.09e-04 / 6.64e-04   2.16e-04 / 7.25e-04
  pyramid res   fp32    B      7.93e-07 / 2.00e-05   col32    3.66e-07 / 2.00e-05   -
  pyramid res   f16x3   A      5.21e-07 / 2.00e-05   row7     2.35e-07 / 2.00e-05   -
  pyramid res   bf16    C      1.95e-03 / 5.23e-03   row0     2.00e-03 / 5.56e-03   6.80e-04 / 2.37e-03
  pyramid res   f16     C      3.92e-04 / 6.61e-04   row_last 3.23e-04 / 6.82e-04   2.18e-04 / 7.29e-04
The fp32 class sits at 0.08 of its bound (the 5e-6 floor decides it: the oracle's own fp32 error is 3..6e-7), bf16 at 0.4, f16 at 0.6 of 3 x the
emulation's error; the results lie at a third of the emulation's own error from the emulation.  No kernel or launch code had to change.
"""
import numpy as np
import pytest
import torch

import neck_cases as NC

pytestmark = pytest.mark.gpu

KID_FPN_UP = 14
KID_LATERAL = {"res": [10, 11, 12, 13], "swin": [15, 16, 17, 18], "mpvit": [24, 25, 26, 26]}      # per level; MPViT's levels 2 and 3 share id 26
KID_NECK = {"swin": list(range(30, 42)), "mpvit": list(range(54, 66))}
ALL_KIDS = sorted({KID_FPN_UP, *sum(KID_LATERAL.values(), []), *sum(KID_NECK.values(), [])})


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a HIP device: the product has no CPU fallback")
    import gpu_util
    return gpu_util


def new_handle(pyr):
    import diffusiondepth_amd as dda
    sd, fsd, hsd = NC.weights(pyr)
    b = dda.HipDenoiser(variant="res" if pyr == "res" else "swin")
    b.load_state_dict({**sd, **fsd, **(hsd or {})})
    b.set_schedule(dda.DDIMScheduler().alphas_cumprod)
    b.set_option("graph", 0)
    return b


@pytest.fixture(scope="module")
def handle(U):
    """handle(pyramid): ONE HipDenoiser per pyramid for the module."""
    made = {}

    def get(pyr):
        if pyr not in made:
            made[pyr] = new_handle(pyr)
        return made[pyr]

    yield get
    for b in made.values():
        b.close()


def dev(f):
    return torch.tensor(np.asarray(f)).cuda()          # a copy: the shared features are read-only arrays


def cond(U, be, fp, prec, neck):
    return be.condition([dev(f) for f in fp], prec, neck=neck).cpu().numpy()


def check_against_oracle(U, be, pyr, shape, prec, neck):
    r = NC.reference(pyr, shape, neck)
    x = cond(U, be, NC.features(pyr, shape), prec, neck)

    def report(st):
        name, e, b = st["worst_strip"]
        te = max(st["to_emu"], key=lambda t: t[0] / t[1]) if st["to_emu"] else (0.0, 0.0)
        print("neck_parity", pyr, shape, prec, "neck" if neck else "pyramid", "rel %.3e bound %.3e" % (st["rel"], st["bound"]),
              "worst strip %s %.3e bound %.3e" % (name, e, b), "to emulation %.3e bound %.3e" % te)
        U.record("neck_parity", pyramid=pyr, shape=shape, prec=prec, neck=int(neck), maxabs=st["maxabs"], scale=st["scale"], rel=st["rel"], bound=st["bound"],
                 worst_strip=name, strip_rel_l2=e, strip_bound=b, to_emu=te[0], to_emu_bound=te[1])

    NC.assert_cond_close(x, r["ref"], NC.emu_err_for(r, prec), prec, report=report)


# ---- a. neck + pyramid, b. pyramid alone, against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr,shape", NC.NECK_CASES)
def test_neck_and_pyramid_match_the_fp64_oracle(U, handle, pyr, shape, prec):
    check_against_oracle(U, handle(pyr), pyr, shape, prec, True)


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr,shape", NC.PYRAMID_CASES)
def test_pyramid_alone_matches_the_fp64_oracle(U, handle, pyr, shape, prec):
    check_against_oracle(U, handle(pyr), pyr, shape, prec, False)


# ---- c. which kernels ran ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr", ["swin", "mpvit"])
def test_a_neck_call_launches_exactly_its_kernel_ids(U, handle, pyr, prec):
    be = handle(pyr)
    fp = [dev(f) for f in NC.features(pyr, "A")]
    want = {k: 0 for k in ALL_KIDS}
    for k in KID_NECK[pyr] + KID_LATERAL[pyr] + [KID_FPN_UP] * 3:
        want[k] += 1
    before = {k: be.counter("kid_launches:%d" % k) for k in ALL_KIDS}
    n0 = be.counter("neck_launches")
    x = be.condition(fp, prec, neck=True).cpu().numpy()
    delta = {k: be.counter("kid_launches:%d" % k) - before[k] for k in ALL_KIDS}
    assert delta == want, (pyr, prec, {k: (delta[k], want[k]) for k in ALL_KIDS if delta[k] != want[k]})
    assert be.counter("neck_launches") == n0 + 12
    if prec in ("f16x3", "f16r"):
        assert be.counter("cond_split_ok") == 3                       # FPN and neck weights fit the split-f16 images: those kernels ran ...
        x32 = be.condition(fp, "fp32", neck=True).cpu().numpy()
        be.set_option("cond_split", 0)
        try:
            off = be.condition(fp, prec, neck=True).cpu().numpy()
        finally:
            be.set_option("cond_split", 1)
        assert np.array_equal(off, x32)                               # ... without the switch the fp32 mode's kernels, bit for bit
        assert not np.array_equal(x, x32)                             # ... with it, another kernel family


# ---- d. batch addressing -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr,shape", [(p, s) for p in ("swin", "mpvit", "res") for s in ("A", "C")])
def test_every_image_of_a_batch_equals_that_image_run_alone(U, handle, pyr, shape, prec):
    """Nothing in this path reduces across images: b * in_cstride + in_coff / b * out_cstride + out_coff and the per-image buffer descriptors."""
    be = handle(pyr)
    fp = NC.features(pyr, shape)
    for neck in ((True, False) if pyr != "res" else (False,)):
        full = cond(U, be, fp, prec, neck)
        for i in range(fp[0].shape[0]):
            one = cond(U, be, [f[i:i + 1] for f in fp], prec, neck)
            assert np.array_equal(full[i:i + 1], one), (pyr, shape, prec, neck, i, U.maxabs(full[i:i + 1], one))


# ---- e. workspace reuse ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pyr", ["swin", "mpvit"])
def test_a_reused_workspace_gives_the_same_bits(U, handle, pyr):
    """The pyramid workspace is kept while shape, batch, tensor kind and pyramid stay; a workspace made for the neck serves a call without it;
    the pooled buffers exist only for the levels whose sizes are odd (shape A: all, shape B: none)."""
    be = handle(pyr)
    fresh = new_handle(pyr)
    try:
        for prec in NC.PRECS:
            a1 = cond(U, be, NC.features(pyr, "A"), prec, True)
            cond(U, be, NC.features(pyr, "B"), prec, True)
            a3 = cond(U, be, NC.features(pyr, "A"), prec, True)
            plain = cond(U, be, NC.features(pyr, "A"), prec, False)      # on the neck's workspace
            assert np.array_equal(a3, a1), (pyr, prec, U.maxabs(a3, a1))
            want = cond(U, fresh, NC.features(pyr, "A"), prec, False)    # a handle that never ran the neck
            assert np.array_equal(plain, want), (pyr, prec, U.maxabs(plain, want))
    finally:
        fresh.close()


# ---- f. NaN containment ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16", "f16x3"])
@pytest.mark.parametrize("pyr", ["swin", "mpvit"])
def test_a_nan_stays_inside_its_image(U, handle, pyr, prec):
    be = handle(pyr)
    fp = NC.features(pyr, "A")
    clean = cond(U, be, fp, prec, True)
    bad = [f.copy() for f in fp]
    bad[2][1, 5, 2, 3] = np.nan
    x = cond(U, be, bad, prec, True)
    assert np.isfinite(clean).all()
    assert np.array_equal(x[0], clean[0]), (pyr, prec)
    assert np.isnan(x[1]).any()
