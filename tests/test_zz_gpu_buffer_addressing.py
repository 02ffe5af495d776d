"""GPU: the convolution kernels' buffer addressing (dd_gcn.h) at the sizes and in the kernel forms of tests/buffer_addressing_cases.py -- one
8x32 tile, 2x2 tiles with one-pixel ragged edges, a single pixel, 3x3 ragged tiles; conv1 with the DDIM update, the dual-split conv2, the
one-buffer hoisted conv3 (int16 hand-over in the refined mode), the streaming conv4 walking several tiles, conv3(cond) from the NCHW tensor --
against the fp64 oracle with the bounds tests/test_gpu_parity.py holds each precision to; graph replay against the eager loop and a two-lane
batch against its images run alone, bit for bit (at these sizes every GroupNorm statistics slot receives one workgroup's sum, so nothing
depends on the order of the atomics).  The oracle runs once per size and is shared."""
import numpy as np
import pytest
import torch

import buffer_addressing_cases as BC
from test_gpu_parity import LATENT_TOL

pytestmark = pytest.mark.gpu
PRECS = ["f16r", "bf16", "f16x3", "fp32"]
C = {"wseed": BC.WSEED}
_ref = {}


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a HIP device: the product has no CPU fallback")
    import gpu_util
    return gpu_util


@pytest.fixture()
def be(U):
    b = U.backend_for(C)
    for k, v in BC.OPTIONS.items():
        b.set_option(k, v)
    yield b
    for k, v in BC.RESTORE.items():
        b.set_option(k, v)
    b.set_option("graph", 1 if b.graph_replay else 0)
    b.set_option("streams", b.n_streams)


def reference(U, h, w):
    if (h, w) not in _ref:
        from oracle import ddim_oracle as O
        inp = BC.inputs(h, w)
        _ref[(h, w)] = (inp, O.ddim_loop(U.sd_for(C), inp["x_T"], inp["cond"], BC.T))
    return _ref[(h, w)]


@pytest.mark.parametrize("h,w", BC.SHAPES)
def test_forms_and_sizes_vs_oracle(U, be, h, w):
    inp, ref = reference(U, h, w)
    x, cond = U.cu(inp["x_T"]), U.cu(inp["cond"])
    scale = float(np.abs(ref).max())
    for prec in PRECS:
        before = {k: be.counter("kid_launches:%d" % k) for k in BC.KIDS}
        s0 = be.counter("thin_stream_launches")
        x0 = be.denoise(x, cond, BC.T, prec).cpu().numpy()
        e = U.maxabs(x0, ref)
        print("buffer_addressing", prec, h, w, "latent max|err| %.3e" % e, "bound %.3e" % (LATENT_TOL[prec] * scale))
        U.record("buffer_addressing", prec=prec, h=h, w=w, latent_maxabs=e, latent_scale=scale)
        assert np.isfinite(x0).all() and e < LATENT_TOL[prec] * scale, (prec, h, w, e, scale)
        if prec == "f16r":      # the five forms really ran (the other modes take their own kernels for conv1 / conv3)
            assert all(be.counter("kid_launches:%d" % k) > before[k] for k in BC.KIDS) and be.counter("thin_stream_launches") > s0


@pytest.mark.parametrize("prec", ["f16r", "fp32"])
def test_graph_replay_equals_the_eager_loop_bit_for_bit(U, be, prec):
    if not be.graph_replay:
        pytest.fail("graph replay is off in this process: the session's conftest switches the runtime's graph fast path off before HIP starts")
    for h, w in ((9, 33), (17, 70)):
        inp, _ = reference(U, h, w)
        x, cond = U.cu(inp["x_T"]), U.cu(inp["cond"])
        be.set_option("graph", 1)
        g0 = be.counter("graph_launches")
        a = be.denoise(x, cond, BC.T, prec).cpu().numpy()
        assert be.counter("graph_launches") > g0 and be.counter("graph_capture_failures") == 0
        be.set_option("graph", 0)
        e0 = be.counter("eager_loops")
        b = be.denoise(x, cond, BC.T, prec).cpu().numpy()
        assert be.counter("eager_loops") > e0
        assert np.array_equal(a, b), (prec, h, w, U.maxabs(a, b))


@pytest.mark.parametrize("prec", ["f16r", "fp32"])
def test_two_lanes_equal_their_images_run_alone(U, be, prec):
    for h, w in ((9, 33), (17, 70)):
        inp, _ = reference(U, h, w)
        x, cond = U.cu(inp["x_T"]), U.cu(inp["cond"])
        be.set_option("streams", 2)
        both = be.denoise(x, cond, BC.T, prec).cpu().numpy()
        for i in range(BC.B):
            solo = be.denoise(x[i:i + 1].contiguous(), cond[i:i + 1].contiguous(), BC.T, prec).cpu().numpy()
            assert np.array_equal(both[i:i + 1], solo), (prec, h, w, i, U.maxabs(both[i:i + 1], solo))
