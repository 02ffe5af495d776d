"""GPU (`-m gpu`): the special FORMS of the denoiser's kernels -- the ones the tile-count rules and the A/B options select, and the ones the
benchmark's headline configuration times -- on sizes where their edge handling matters, against the fp64 oracle:

  16x32-pixel tiles      BIG_CONV3C / BIG_CONV3H / SWIN_PRED5B_H   kernel ids 48, 49, 51   (plan_big_tiles; option "big_tiles")
  one patch buffer       ONE_CONV3H                                 id 46                   (conv3h_kid; option "one_buffer")
  NCHW-reading layer 8   CONV3C_NCHW                                id 47                   (refined f16; option "cond_direct")
  streaming conv4        dd_thin.hip, several tiles per workgroup   no id                   (options "thin_stream", "thin_slots")
  refined-f16 hand-overs options "f16r_wide", "f16r_c1", "f16r_p4" on both tile orders (launch_cadd_reformat)

Which kernel RAN is asserted, not assumed: the counters "kid_launches:<id>" / "thin_stream_launches" (include/ddepth.h) count the launches a
call enqueues, so every call here is made with option "graph" = 0 (a replay enqueues nothing; the kernel choice is a function of the plan key and
the options, so the graph of the same key holds the same kernels) and its counter deltas are compared with the whole expected set: an option
that is silently ignored, or a plan that outlives a set_option, fails the test instead of passing it on the wrong kernel.

Shapes: the smallest that have every edge class of a 16x32 tiling -- (25, 40): 2 x 2 big tiles, the bottom one with one full 8-row half and
one row, the right one 8 columns wide; (17, 33): one-row / one-column remainders; (16, 32): exactly one big tile = two small ones; (7, 5): less
than a tile of either form; (33, 70): three tiles per axis, an interior tile, remainders 1 and 6.  T = 2, B = 2 unless noted.
Tolerances: the project's own (tests/test_gpu_parity.py), restated below.  The handles are this module's own (a forced option can never leak
into the cached backends of the other files), one lane ("streams" = 1: a plan sees the whole batch) unless a test is about lanes.

What the ids are in the refined f16 mode (dd_api_plans.cpp): its once-per-image term is ALWAYS computed by the split-f16 layer 8 on 8x32 tiles
(id 47 from an explicit NCHW tensor, id 8 otherwise -- and in the Swin denoiser) and then reformatted into the order of the loop kernel's tiles,
so BIG_CONV3C (48) runs in the bf16 / f16 modes only; the loop kernels are 9 / 46 / 49 and 53 / 51 in every 2-byte mode."""
import contextlib

import numpy as np
import pytest
import torch

from diffusiondepth_amd import synth

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py's bounds, restated identically
LATENT_TOL = {"naive_fp32": 2e-5, "fp32": 2e-5, "f16x3": 2e-5, "f16": 1.5e-3, "bf16": 1e-2, "f16r": 8e-4}   # x max|x_0|
EPS_TOL = {"naive_fp32": 5e-5, "fp32": 5e-5, "f16x3": 5e-5, "f16": 1.5e-2, "bf16": 1e-1, "f16r": 1e-2}      # abs on eps

T = 2
WATCH = (1, 2, 3, 4, 5, 6, 7, 8, 9, 46, 47, 48, 49, 50, 51, 52, 53)      # every kernel id a denoiser call can launch
STREAMS_CONV4 = ("bf16", "f16", "f16r")                                  # conv4 is the streaming kernel by default (else id 4)


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a HIP device: the product has no CPU fallback")
    import gpu_util
    return gpu_util


def _handle(variant, wseed):
    import diffusiondepth_amd as dda
    be = dda.HipDenoiser(variant=variant)
    sd = synth.make_state_dict(wseed, variant)
    be.load_state_dict(sd)
    be.set_schedule(dda.DDIMScheduler().alphas_cumprod)
    be.set_option("graph", 0)
    be.set_option("streams", 1)
    slots = be.counter("resident_slots")
    be.defaults = dict(big_tiles=-1, one_buffer=1, thin_stream=1, thin_slots=min(slots, 4096), f16r_wide=1, f16r_c1=1, f16r_p4=0, cond_direct=1,
                       hoist_cond=-1, streams=1)
    return be, sd


@pytest.fixture(scope="module")
def res(U):
    be, sd = _handle("res", 7244)
    yield be, sd
    be.close()


@pytest.fixture(scope="module")
def swin(U):
    be, sd = _handle("swin", 7245)
    yield be, sd
    be.close()


@contextlib.contextmanager
def options(be, **kv):
    """Set options for a block; every one of them is back at the handle's default behind it, whatever happened inside."""
    try:
        for k, v in kv.items():
            be.set_option(k, v)
        yield
    finally:
        for k in kv:
            be.set_option(k, be.defaults[k])


def launched(be, call):
    """(result of call(), {kernel id or "thin": launches it enqueued}) -- only what moved."""
    def read():
        d = {k: be.counter(f"kid_launches:{k}") for k in WATCH}
        d["thin"] = be.counter("thin_stream_launches")
        return d
    a = read()
    out = call()
    b = read()
    return out, {k: b[k] - a[k] for k in b if b[k] != a[k]}


def conv4_of(prec, n, stream=True):
    return {"thin": n} if (prec in STREAMS_CONV4 and stream) else {4: n}


def res_ids(prec, n, loop, cond, stream=True):
    """What a hoisted Res call of n network evaluations launches: conv1, conv2, the loop's conv3 form, conv3(cond) once, conv4."""
    return {1: n, 2: n, loop: n, cond: 1, **conv4_of(prec, n, stream)}


def swin_ids(prec, n, pred, cond):
    """Hoisted Swin call: conv1, conv2, convA', the 5x5 form per evaluation; convA and convB (id 6 twice) and layer 8 once per call; conv4."""
    return {1: n, 2: n, 50: n, pred: n, 6: 2, cond: 1, **conv4_of(prec, n)}


# ---- inputs and fp64 references: computed once per (variant, B, h, w), shared, never written to -------------------------------------------------
_inputs, _loop_ref, _once_ref = {}, {}, {}


def inputs(variant, B, h, w):
    key = (variant, B, h, w)
    if key not in _inputs:
        chw = None if variant == "res" else ((h + 1) // 2, (w + 1) // 2)
        _inputs[key] = synth.make_inputs(7000 + 131 * h + w + 17 * B, B, h, w, chw)
    return _inputs[key]


def loop_ref(sd, variant, B, h, w):
    from oracle import ddim_oracle as O
    key = (variant, B, h, w)
    if key not in _loop_ref:
        i = inputs(variant, B, h, w)
        r = O.ddim_loop(sd, i["x_T"], i["cond"], T, variant)
        r.setflags(write=False)
        _loop_ref[key] = (r, float(np.abs(r).max()))
    return _loop_ref[key]


def once_ref(sd, variant, B, h, w, tt):
    from oracle import ddim_oracle as O
    key = (variant, B, h, w, tuple(tt))
    if key not in _once_ref:
        i = inputs(variant, B, h, w)
        r = O.denoiser_forward(sd, i["x_T"], np.asarray(tt, np.int64), i["cond"], variant)
        r.setflags(write=False)
        _once_ref[key] = r
    return _once_ref[key]


def run_loop(U, be, variant, B, h, w, prec, steps=T):
    i = inputs(variant, B, h, w)
    return launched(be, lambda: be.denoise(U.cu(i["x_T"]), U.cu(i["cond"]), steps, prec).cpu().numpy())


def run_once(U, be, variant, B, h, w, prec, tt):
    i = inputs(variant, B, h, w)
    return launched(be, lambda: be.denoise_once(U.cu(i["x_T"]), torch.tensor(tt, device="cuda", dtype=torch.long), U.cu(i["cond"]), prec).cpu().numpy())


def ids_json(ids):
    return {str(k): v for k, v in ids.items()}


RES_SHAPES = [(25, 40), (17, 33), (16, 32), (7, 5), (33, 70)]
ONCE_T_RES = [37, 950]
ONCE_T_SWIN = [500, 33]


# ---- a. Res hoisted conv3: two-buffer 8x32, one-buffer 8x32, 16x32 tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("hw", RES_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("prec", ["bf16", "f16", "f16r"])
def test_res_hoisted_conv3_in_its_three_tile_forms_vs_oracle(U, res, prec, hw):
    """The loop's hoisted conv3 as KID_CONV3H (9), ONE_CONV3H (46) and BIG_CONV3H (49), with the once-per-image conv3(cond) that feeds each
    (bf16 / f16: id 8, and BIG_CONV3C = 48 for the 16x32 tiles; f16r: the NCHW reader, id 47, for all three), each against the fp64 oracle.
    The one-buffer kernel has the two-buffer kernel's tiles and accumulation order: bit-identical.  The 16x32 tiles regroup the GroupNorm
    partial sums: held to the oracle only."""
    be, sd = res
    h, w = hw
    B = 2
    ref, scale = loop_ref(sd, "res", B, h, w)
    c8 = 47 if prec == "f16r" else 8
    c48 = 47 if prec == "f16r" else 48
    settings = [("two_buffer", dict(big_tiles=0, one_buffer=0), 9, c8), ("one_buffer", dict(big_tiles=0, one_buffer=2), 46, c8),
                ("big_tiles", dict(big_tiles=1), 49, c48)]
    outs, eps = {}, {}
    for name, opts, loop_id, cond_id in settings:
        with options(be, **opts):
            x0, ids = run_loop(U, be, "res", B, h, w, prec)
            e = U.maxabs(x0, ref)
            U.record("kernel_forms", test="a_res_conv3", form=name, prec=prec, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
            assert ids == res_ids(prec, T, loop_id, cond_id), (name, prec, hw, ids)
            assert np.isfinite(x0).all() and e < LATENT_TOL[prec] * scale, (name, prec, hw, e, scale)
            outs[name] = x0
            if hw == (25, 40):      # one call with per-sample timesteps through the same forms
                eref = once_ref(sd, "res", B, h, w, ONCE_T_RES)
                ep, ids1 = run_once(U, be, "res", B, h, w, prec, ONCE_T_RES)
                ee = U.maxabs(ep, eref)
                U.record("kernel_forms", test="a_res_conv3_once", form=name, prec=prec, B=B, h=h, w=w, eps_maxabs=ee, ids=ids_json(ids1))
                assert ids1 == res_ids(prec, 1, loop_id, cond_id), (name, prec, ids1)
                assert ee < EPS_TOL[prec], (name, prec, ee)
                eps[name] = ep
    assert np.array_equal(outs["one_buffer"], outs["two_buffer"]), (prec, hw, U.maxabs(outs["one_buffer"], outs["two_buffer"]))
    if eps:
        assert np.array_equal(eps["one_buffer"], eps["two_buffer"]), (prec, hw)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_big_tiles_leave_the_fp32_and_split_modes_on_their_8x32_kernels(U, res, prec):
    """plan_big_tiles excludes the fp32 and the split-f16 kind (no 16x32 instantiation): forcing "big_tiles" = 1 must leave ids 8 / 9 running --
    bit-identical to "big_tiles" = 0 -- and must not fail the call.  (fp32 hoists its condition term on request only: "hoist_cond" = 1.)"""
    be, sd = res
    B, h, w = 2, 25, 40
    ref, scale = loop_ref(sd, "res", B, h, w)
    out = {}
    for big in (0, 1):
        with options(be, big_tiles=big, one_buffer=0, hoist_cond=1):
            x0, ids = run_loop(U, be, "res", B, h, w, prec)
        e = U.maxabs(x0, ref)
        U.record("kernel_forms", test="a_res_conv3_excluded_kinds", big_tiles=big, prec=prec, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
        assert ids == res_ids(prec, T, 9, 8), (prec, big, ids)
        assert e < LATENT_TOL[prec] * scale, (prec, big, e, scale)
        out[big] = x0
    assert np.array_equal(out[0], out[1])


# ---- b. refined-f16 hand-over variants on both tile orders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("wide,c1,p4", [(1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1)])
def test_refined_f16_hand_over_variants_on_both_tile_orders(U, res, wide, c1, p4, big):
    """y3 and the hoisted term as block-scaled int16 ("f16r_wide") or f16, conv1 on the weight pair ("f16r_c1") or not, conv4's operand as a pair
    ("f16r_p4"): the term is reformatted into the 8x32 or the 16x32 tile order (launch_cadd_reformat) for each.  With f16r_wide = 0 or
    f16r_c1 = 0 the mode degrades toward the f16 mode's hand-overs by design: those two are held to the f16 bounds, the others to f16r's."""
    be, sd = res
    B, h, w = 2, 25, 40
    ref, scale = loop_ref(sd, "res", B, h, w)
    eref = once_ref(sd, "res", B, h, w, ONCE_T_RES)
    tol = "f16r" if (wide and c1) else "f16"
    loop_id = 49 if big else 9
    with options(be, f16r_wide=wide, f16r_c1=c1, f16r_p4=p4, big_tiles=big, one_buffer=0):
        x0, ids = run_loop(U, be, "res", B, h, w, "f16r")
        ep, ids1 = run_once(U, be, "res", B, h, w, "f16r", ONCE_T_RES)
    e, ee = U.maxabs(x0, ref), U.maxabs(ep, eref)
    U.record("kernel_forms", test="b_f16r_variants", wide=wide, c1=c1, p4=p4, big_tiles=big, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale,
             eps_maxabs=ee, held_to=tol, ids=ids_json(ids), ids_once=ids_json(ids1))
    assert ids == res_ids("f16r", T, loop_id, 47) and ids1 == res_ids("f16r", 1, loop_id, 47), (ids, ids1)
    assert np.isfinite(x0).all() and e < LATENT_TOL[tol] * scale, (wide, c1, p4, big, e, scale)
    assert ee < EPS_TOL[tol], (wide, c1, p4, big, ee)


# ---- c. the NCHW-reading conv3(cond) in front of 16x32-tile consumers -----------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(25, 40), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cond_direct_on_ragged_sizes_with_big_tile_consumers(U, res, hw):
    """CONV3C_NCHW (47) against the split-f16 layer 8 on the channel-blocked copy (8): same values, same arithmetic, same output order --
    bit-identical x_0 and eps, as the KITTI-size test asserts, here with ragged right / bottom tiles and the reformat into the 16x32 order."""
    be, sd = res
    h, w = hw
    B = 2
    ref, scale = loop_ref(sd, "res", B, h, w)
    got = {}
    for direct, cond_id in ((0, 8), (1, 47)):
        with options(be, cond_direct=direct, big_tiles=1):
            x0, ids = run_loop(U, be, "res", B, h, w, "f16r")
            ep, ids1 = run_once(U, be, "res", B, h, w, "f16r", ONCE_T_RES)
        e = U.maxabs(x0, ref)
        U.record("kernel_forms", test="c_cond_direct", cond_direct=direct, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids), ids_once=ids_json(ids1))
        assert ids == res_ids("f16r", T, 49, cond_id) and ids1 == res_ids("f16r", 1, 49, cond_id), (direct, ids, ids1)      # (47 moves with cond_direct = 1 only)
        assert np.isfinite(x0).all() and e < LATENT_TOL["f16r"] * scale, (direct, hw, e, scale)
        got[direct] = (x0, ep)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), hw


# ---- d. the streaming conv4 across tile boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16", "bf16", "f16r"])
def test_streaming_conv4_walks_tiles_on_hardware(U, res, prec):
    """dd_thin.hip on a 17 x 70 latent = 3 x 3 tiles per image with ragged right / bottom edges: "thin_slots" = 3 (two images: one workgroup per
    image walks all nine tiles, its rolling prefetch crossing every tile boundary), 512 (one tile each), and the general kernel (id 4,
    "thin_stream" = 0; the refined mode has the streaming form only).  All against the oracle."""
    be, sd = res
    B, h, w = 2, 17, 70
    ref, scale = loop_ref(sd, "res", B, h, w)
    cond_id = 47 if prec == "f16r" else 8
    cases = [("walk9", dict(thin_slots=3), True), ("one_tile_each", dict(thin_slots=512), True)]
    if prec != "f16r":
        cases.append(("general", dict(thin_stream=0), False))
    for name, opts, stream in cases:
        with options(be, big_tiles=0, one_buffer=0, **opts):
            x0, ids = run_loop(U, be, "res", B, h, w, prec)
        e = U.maxabs(x0, ref)
        U.record("kernel_forms", test="d_stream_conv4", form=name, prec=prec, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
        assert ids == res_ids(prec, T, 9, cond_id, stream), (name, prec, ids)
        assert np.isfinite(x0).all() and e < LATENT_TOL[prec] * scale, (name, prec, e, scale)


@pytest.mark.parametrize("prec", ["f16", "bf16", "f16r"])
def test_more_images_than_streaming_slots_takes_the_general_conv4(U, res, prec):
    """The rule B <= thin_slots (enqueue_fused_step): three images on two slots send the f16 / bf16 modes to the general kernel; the refined
    mode always streams (one workgroup per image, whatever the slots).  Either way the result meets the oracle."""
    be, sd = res
    B, h, w = 3, 17, 70
    ref, scale = loop_ref(sd, "res", B, h, w)
    with options(be, big_tiles=0, one_buffer=0, thin_slots=2):
        x0, ids = run_loop(U, be, "res", B, h, w, prec)
    e = U.maxabs(x0, ref)
    U.record("kernel_forms", test="d_stream_conv4_rule", prec=prec, B=B, h=h, w=w, T=T, thin_slots=2, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
    if prec == "f16r":
        assert ids == res_ids(prec, T, 9, 47, True), ids
    else:
        assert ids == res_ids(prec, T, 9, 8, False), ids
    assert np.isfinite(x0).all() and e < LATENT_TOL[prec] * scale, (prec, e, scale)


# ---- e. the Swin 5x5 form on both tilings ---------------------------------------------------------------------------------------------------------
SWIN_SHAPES = [(25, 40), (17, 33), (7, 5), (5, 17)]      # the last two: an axis shorter than seven pixels -- every E[t] border class, the whole border ring


@pytest.mark.parametrize("hw", SWIN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("prec", ["f16", "bf16", "f16r"])
def test_swin_5x5_form_on_both_tilings_vs_oracle(U, swin, prec, hw):
    """SWIN_PRED5_H (53) against SWIN_PRED5B_H (51), each started from the once-per-image term in its own tile order -- KID_CONV3C (8) against
    BIG_CONV3C (48) in the f16 / bf16 modes, the split-f16 layer 8 plus the reformat in the refined mode -- against the fp64 oracle.  A single
    call with per-sample timesteps runs the hoisted form in the refined mode only (one E[t] table per image); the other modes run the
    reference's order (ids 5, 6, 7) there, whatever "big_tiles" says."""
    be, sd = swin
    h, w = hw
    B = 2
    ref, scale = loop_ref(sd, "swin", B, h, w)
    for big in (0, 1):
        pred = 51 if big else 53
        cond_id = 48 if (big and prec != "f16r") else 8
        with options(be, big_tiles=big):
            x0, ids = run_loop(U, be, "swin", B, h, w, prec)
            e = U.maxabs(x0, ref)
            U.record("kernel_forms", test="e_swin_5x5", big_tiles=big, prec=prec, B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
            assert ids == swin_ids(prec, T, pred, cond_id), (prec, hw, big, ids)
            assert np.isfinite(x0).all() and e < LATENT_TOL[prec] * scale, (prec, hw, big, e, scale)
            if hw == (25, 40):
                eref = once_ref(sd, "swin", B, h, w, ONCE_T_SWIN)
                ep, ids1 = run_once(U, be, "swin", B, h, w, prec, ONCE_T_SWIN)
                ee = U.maxabs(ep, eref)
                U.record("kernel_forms", test="e_swin_5x5_once", big_tiles=big, prec=prec, B=B, h=h, w=w, eps_maxabs=ee, ids=ids_json(ids1))
                want = swin_ids(prec, 1, pred, cond_id) if prec == "f16r" else {1: 1, 2: 1, 5: 1, 6: 1, 7: 1, **conv4_of(prec, 1)}
                assert ids1 == want, (prec, big, ids1)
                assert ee < EPS_TOL[prec], (prec, big, ee)


def test_big_tiles_leave_the_swin_split_mode_on_the_8x32_5x5_form(U, swin):
    """f16x3 has no 16x32 instantiation: "big_tiles" = 1 stays on ids 53 / 8 and inside the fp32-class bound."""
    be, sd = swin
    B, h, w = 2, 25, 40
    ref, scale = loop_ref(sd, "swin", B, h, w)
    with options(be, big_tiles=1):
        x0, ids = run_loop(U, be, "swin", B, h, w, "f16x3")
    e = U.maxabs(x0, ref)
    U.record("kernel_forms", test="e_swin_5x5_excluded_kind", big_tiles=1, prec="f16x3", B=B, h=h, w=w, T=T, latent_maxabs=e, latent_scale=scale, ids=ids_json(ids))
    assert ids == swin_ids("f16x3", T, 53, 8), ids
    assert e < LATENT_TOL["f16x3"] * scale, (e, scale)


# ---- f. the automatic rules ------------------------------------------------------------------------------------------------------------------------
def _threshold_heights(be):
    """Latent heights (width 40 = two tiles across, B = 1) whose 8x32 tile count just exceeds / just does not exceed the chip's resident slots."""
    slots = be.counter("resident_slots")
    over, under = 8 * (slots // 2 + 1), 8 * (slots // 2)
    assert 2 * (over // 8) > slots >= 2 * (under // 8) > 0
    return over, under


def test_automatic_rule_gives_the_res_denoiser_the_one_buffer_form_above_the_resident_slots(U, res):
    """conv3h_kid: more 8x32 tiles than resident slots -> ONE_CONV3H (46), one tile row fewer -> KID_CONV3H (9); never the 16x32 tiles for the
    Res denoiser (plan_big_tiles).  Each automatic choice is bit-identical to the OTHER 8x32 form forced on the same input.  This is the one test
    whose size follows the chip (one T = 1 loop per call)."""
    be, _ = res
    over, under = _threshold_heights(be)
    try:
        for h, auto_id, forced, forced_id in ((over, 46, dict(one_buffer=0), 9), (under, 9, dict(one_buffer=2), 46)):
            with options(be, big_tiles=-1, one_buffer=1, streams=1):
                a, ids = run_loop(U, be, "res", 1, h, 40, "f16r", steps=1)
            assert ids == res_ids("f16r", 1, auto_id, 47), (h, ids)
            with options(be, big_tiles=-1, streams=1, **forced):
                f, idsf = run_loop(U, be, "res", 1, h, 40, "f16r", steps=1)
            assert idsf == res_ids("f16r", 1, forced_id, 47), (h, idsf)
            U.record("kernel_forms", test="f_auto_rule_res", h=h, w=40, B=1, T=1, slots=be.counter("resident_slots"), ids=ids_json(ids), ids_forced=ids_json(idsf),
                     auto_vs_forced_maxabs=U.maxabs(a, f))
            assert np.isfinite(a).all() and np.array_equal(a, f), h
    finally:
        _inputs.pop(("res", 1, over, 40), None); _inputs.pop(("res", 1, under, 40), None)


@pytest.mark.parametrize("prec", ["f16r", "f16"])
def test_automatic_rule_gives_the_swin_denoiser_the_16x32_tiles_above_the_resident_slots(U, swin, prec):
    """plan_big_tiles: more 8x32 tiles than resident slots -> SWIN_PRED5B_H (51), its start values in the 16x32 order (f16: BIG_CONV3C, 48; the
    refined mode: layer 8 + reformat); one tile row fewer -> SWIN_PRED5_H (53) with id 8.  Each automatic choice agrees with the other tiling
    forced on the same input within the precision's bound (other GroupNorm partial-sum order)."""
    be, _ = swin
    over, under = _threshold_heights(be)
    try:
        for h, auto_big in ((over, 1), (under, 0)):
            want = lambda big: swin_ids(prec, 1, 51 if big else 53, 48 if (big and prec != "f16r") else 8)
            with options(be, big_tiles=-1, streams=1):
                a, ids = run_loop(U, be, "swin", 1, h, 40, prec, steps=1)
            assert ids == want(auto_big), (h, ids)
            with options(be, big_tiles=1 - auto_big, streams=1):
                f, idsf = run_loop(U, be, "swin", 1, h, 40, prec, steps=1)
            assert idsf == want(1 - auto_big), (h, idsf)
            scale = float(np.abs(a).max())
            d = U.maxabs(a, f)
            U.record("kernel_forms", test="f_auto_rule_swin", prec=prec, h=h, w=40, B=1, T=1, slots=be.counter("resident_slots"), ids=ids_json(ids), ids_forced=ids_json(idsf),
                     auto_vs_forced_maxabs=d, latent_scale=scale)
            assert np.isfinite(a).all() and np.isfinite(f).all() and d < LATENT_TOL[prec] * scale, (h, d, scale)
    finally:
        _inputs.pop(("swin", 1, over, 40), None); _inputs.pop(("swin", 1, under, 40), None)


# ---- g. lanes on a forced form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "f16r"])
def test_two_lanes_on_the_16x32_tiles_equal_the_one_lane_call(U, res, prec):
    """"streams" = 2 with three images (sub-batches of 2 and 1, each its own plan) on the forced 16x32 tiles: every image bit-identical to the
    one-lane call -- the header's contract for equal tile forms -- and the call did run as lanes."""
    be, _ = res
    B, h, w = 3, 25, 40
    cond_id = 47 if prec == "f16r" else 48
    with options(be, big_tiles=1, streams=1):
        one, ids1 = run_loop(U, be, "res", B, h, w, prec)
    with options(be, big_tiles=1, streams=2):
        n0 = be.counter("lane_calls")
        two, ids2 = run_loop(U, be, "res", B, h, w, prec)
        lanes = be.counter("lane_calls") - n0
    U.record("kernel_forms", test="g_lanes", prec=prec, B=B, h=h, w=w, T=T, lane_calls=lanes, lanes_vs_one_maxabs=U.maxabs(one, two), ids=ids_json(ids2))
    assert ids1 == res_ids(prec, T, 49, cond_id), ids1
    assert ids2 == {k: 2 * v for k, v in res_ids(prec, T, 49, cond_id).items()}, ids2      # two plans, each the whole sequence
    assert lanes == 1
    assert np.isfinite(two).all()
    for i in range(B):
        assert np.array_equal(one[i], two[i]), (prec, i, U.maxabs(one[i], two[i]))
