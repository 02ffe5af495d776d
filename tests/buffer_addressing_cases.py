"""Cases shared by tests/test_buffer_addressing_host_emulation.py and tests/test_zz_gpu_buffer_addressing.py: the refined-f16 DDIM loop in
the configuration that runs, in ONE call, the five kernel forms whose global accesses go through buffer descriptors --

  conv1 with the DDIM update in its prologue (kernel id 1, second loop step), the dual-split conv2 (id 2), the one-buffer hoisted conv3
  with the int16 hand-over (id 46), the streaming conv4 in its refined-f16 form (dd_thin.hip) and conv3(cond) reading the caller's NCHW
  tensor (id 47)

-- at the sizes where their addressing can go wrong: exactly one 8x32 tile, 2x2 tiles with one-pixel ragged edges, a single pixel, and 3x3
tiles with ragged edges (conv4 walking several tiles per workgroup).

    python tests/buffer_addressing_cases.py --write

records the emulated outputs' digests (tests/golden/buffer_addressing_digests.json).  The committed file was written by the commit BEFORE the
kernels moved to buffer addressing: the test asserts that the emulated kernels still produce those bytes."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "buffer_addressing_digests.json")
B, T, WSEED = 2, 2, 7244
SHAPES = [(8, 32), (9, 33), (1, 1), (17, 70)]
OPTIONS = {"hoist_cond": 1, "big_tiles": 0, "one_buffer": 2, "thin_stream": 1, "thin_slots": 3}
RESTORE = {"hoist_cond": 0, "big_tiles": -1, "one_buffer": 1, "thin_stream": 1, "thin_slots": 512}
KIDS = (1, 2, 46, 47)          # kernel ids that must have been launched (dd_kernel_ids.h); the streaming conv4 has its own counter
TIMINGS = ((0, 0), (1, 1))     # (which wave runs ahead, LDS-DMA lands at issue / as late as the waits allow)


def case_name(h, w):
    return "f16r_b%d_%dx%d_t%d" % (B, h, w, T)


def inputs(h, w):
    from diffusiondepth_amd import synth
    return synth.make_inputs(100 + h, B, h, w, None)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def run_emulated(be, h, w, order, late):
    """-> (x0, launch counters that moved).  `be`: hostemu_driver.EmuDenoiser with weights and schedule loaded."""
    inp = inputs(h, w)
    for k, v in OPTIONS.items():
        be.set_option(k, v)
    try:
        be.timing(order, late)
        before = {k: be.counter("kid_launches:%d" % k) for k in KIDS}
        s0 = be.counter("thin_stream_launches")
        x0 = be.denoise(inp["x_T"], inp["cond"], T, "f16r")
        moved = {k: be.counter("kid_launches:%d" % k) - before[k] for k in KIDS}
        moved["thin_stream"] = be.counter("thin_stream_launches") - s0
    finally:
        for k, v in RESTORE.items():
            be.set_option(k, v)
        be.timing(0, 0)
    return x0, moved


def make_backend(lib):
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import synth
    from hostemu_driver import EmuDenoiser
    be = EmuDenoiser(lib, "res")
    sd = synth.make_state_dict(WSEED, "res")
    be.load_state_dict(sd)
    be.set_schedule(dda.DDIMScheduler().alphas_cumprod)
    return be, sd


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from hostemu_util import build_library
    be, _ = make_backend(build_library())
    out = {}
    for h, w in SHAPES:
        x0, moved = run_emulated(be, h, w, 0, 0)
        assert np.isfinite(x0).all() and all(v > 0 for v in moved.values()), (h, w, moved)
        out[case_name(h, w)] = {"x0_sha256": digest(x0), "launches": {str(k): v for k, v in moved.items()}}
        print(case_name(h, w), out[case_name(h, w)])
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
