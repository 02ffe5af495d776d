"""Buffer addressing of the convolution kernels (dd_gcn.h: descriptor + per-lane offset + scalar offset + immediate instead of 64-bit per-lane
addresses) changes HOW an address is formed and nothing else: the emulated kernels must still produce, byte for byte, what the kernels of
the commit before the change produced.  tests/golden/buffer_addressing_digests.json holds that commit's digests (tests/buffer_addressing_cases.py
wrote it, and says which kernel forms and sizes the cases cover).  The emulation's buffer helpers abort the process when an access ends beyond
its descriptor's size, so a passing run is also a run in which every buffer access stayed inside its tensor; the last two tests show that the
check is live in this very build, and the size rule that keeps a per-image tensor inside a 32-bit offset."""
from __future__ import annotations

import ctypes
import json
import subprocess
import textwrap

import numpy as np
import pytest

import buffer_addressing_cases as BC
from diffusiondepth_amd.backend import precision_id
from hostemu_util import CSRC, EMU, _clangxx, build_library


@pytest.fixture(scope="module")
def lib():
    return build_library()


@pytest.fixture(scope="module")
def backend(lib):
    be, _ = BC.make_backend(lib)
    yield be
    be.close()


@pytest.fixture(scope="module")
def golden():
    with open(BC.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("h,w", BC.SHAPES)
def test_emulated_outputs_are_the_parent_commits_bytes(backend, golden, h, w):
    want = golden[BC.case_name(h, w)]
    for order, late in BC.TIMINGS:
        x0, moved = BC.run_emulated(backend, h, w, order, late)
        assert {str(k): v for k, v in moved.items()} == want["launches"], "the case no longer runs the kernel forms it was recorded for"
        assert np.isfinite(x0).all()
        assert BC.digest(x0) == want["x0_sha256"], (h, w, order, late)


def test_the_emulations_range_check_is_live(tmp_path):
    """The very helpers the kernels call (dd_gcn.h, host half), in a stand-alone program: the last 16 bytes of a buffer load and store fine, one
    byte further the program aborts with the helper's message -- for a load, a store, and a scalar offset that carries the access out."""
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++")
    src = tmp_path / "range.cpp"
    src.write_text(textwrap.dedent("""
        #include <hip/hip_runtime.h>
        hostemu::Idx3 threadIdx, blockIdx, blockDim, gridDim;
        extern "C" void hostemu_switch(void**, void*) {}
        #include "dd_gcn.h"
        int main(int argc, char** argv) {
          static char mem[64];
          const dd_buf_t d = dd_make_buf(mem, 48);
          const int mode = atoi(argv[1]);
          if (mode == 0) { dd_buf_store16(d, 16, 8, 8, make_uint4(1, 2, 3, 4)); return dd_buf_load16(d, 0, 16, 16).w == 4 && dd_buf_load4(d, 44, 0, 0) == 4 ? 0 : 3; }
          if (mode == 1) return (int)dd_buf_load16(d, 17, 8, 8).x;
          if (mode == 2) dd_buf_store16(d, 0, 33, 0, make_uint4(0, 0, 0, 0));
          if (mode == 3) return (int)dd_buf_load8(d, 32, 0, 9).x;
          return 0;
        }
        """))
    exe = tmp_path / "range"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-DDD_HOST_EMULATION", "-I", EMU, "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([str(exe), "0"]).returncode == 0
    for mode in ("1", "2", "3"):
        r = subprocess.run([str(exe), mode], capture_output=True, text=True)
        assert r.returncode == -6 and "leaves its 48-byte buffer" in r.stderr, (mode, r.returncode, r.stderr)


def test_size_rule_at_the_32_bit_boundary(lib):
    """conv_buffer_addressable (dd_kernels.h, through the library's test hook): a per-image tensor is addressable when its LAST 16-byte access still has a 32-bit offset"""
    fn = lib.dd_debug_buffer_addressable
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_ulonglong]
    assert fn(0) == 1 and fn(16) == 1
    assert fn(2 ** 32 - 16) == 1
    assert fn(2 ** 32) == 0
    assert fn(2 ** 32 + 16) == 0


def test_plan_creation_refuses_an_image_beyond_the_limit_before_any_allocation(lib):
    """h x w = 2048 x 2048: the condition map of one image is 256 channels x 4 bytes x 2^22 pixels = 2^32 bytes.  dd_denoise must return the
    status code of dd_status.h for an unsupported size, with an error text that names the rule, and must not have asked for memory."""
    be, _ = BC.make_backend(lib)
    try:
        lib.emu_blocking_calls.restype = ctypes.c_ulong
        x = np.zeros(1, np.float32)          # never read: the size check comes first
        n0 = lib.emu_blocking_calls()
        rc = lib.dd_denoise(be.h, x.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p),
                            1, 2048, 2048, 2048, 2048, 2, precision_id("f16r"), None)
        assert rc == 4                       # DD_ERR_UNSUPPORTED (include/ddepth.h)
        assert "32-bit" in lib.dd_last_error(be.h).decode()
        assert lib.emu_blocking_calls() == n0, "an allocation (or another blocking call) was made before the size was refused"
    finally:
        be.close()
