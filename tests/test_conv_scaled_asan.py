"""CPU: out-of-bounds reads and writes of the scaled gradients (include/ddepth_conv_scaled.h), which sentinels around a tensor cannot all see.
tests/host_emul/conv_scaled_asan_main.cpp -- a stand-alone program with its own main -- is compiled together with csrc/dd_conv.hip,
csrc/dd_api_conv.cpp and the emulation's host unit under -fsanitize=address and run as a child process, as tests/test_conv_ragged_asan.py does
for dd_convx_*: no Python in that process, nothing preloaded.  It allocates every tensor, the workspace and the 16-byte scale buffer at exactly
the size the API asks for and runs dd_conv_grad_scale and the two scaled gradients of R1, T1 and P1 (tests/conv_ragged_cases.py) in bf16, f16
and f16x3.  The test passes when the child exits 0 without a sanitizer report."""
import hashlib
import os
import subprocess

import pytest

import hostemu_util as U

MAIN = os.path.join(U.EMU, "conv_scaled_asan_main.cpp")
UNITS = [os.path.join(U.CSRC, "dd_conv.hip"), os.path.join(U.CSRC, "dd_api_conv.cpp"), os.path.join(U.EMU, "ddepth_host.cpp"), MAIN]
DEPS = UNITS + [os.path.join(U.CSRC, "dd_conv.h"), os.path.join(U.CSRC, "dd_conv_kernels.h"), os.path.join(U.EMU, "hip", "hip_runtime.h"),
                os.path.join(U.ROOT, "include", "ddepth_conv.h"), os.path.join(U.ROOT, "include", "ddepth_conv_scaled.h"),
                os.path.join(U.ROOT, "include", "ddepth.h")]
ASAN = ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]


def _have_asan(cxx, out):
    """Can this toolchain link and run a sanitized program at all?"""
    src, exe = os.path.join(out, "probe.cpp"), os.path.join(out, "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run([cxx] + ASAN + [src, "-o", exe], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def program():
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
        out = os.path.join(U.OUT, "conv_scaled_asan_" + hsh.hexdigest()[:12])
        exe = os.path.join(out, "conv_scaled_asan")
        os.makedirs(out, exist_ok=True)
        if not _have_asan(cxx, out):
            pytest.skip("this toolchain has no AddressSanitizer runtime for the host")
        if not os.path.exists(exe):
            objs = []
            for src in UNITS:
                obj = os.path.join(out, os.path.basename(src).rsplit(".", 1)[0] + ".o")
                cmd = [cxx] + U._FLAGS + ASAN + ["-I", U.EMU, "-I", U.CSRC, src, "-o", obj]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    pytest.fail("sanitized host build of %s failed:\n%s" % (src, r.stderr[-4000:]))
                objs.append(obj)
            r = subprocess.run([cxx] + ASAN + objs + ["-o", exe + ".tmp", "-lpthread"], capture_output=True, text=True)
            if r.returncode != 0:
                pytest.fail("sanitized host link failed:\n" + r.stderr[-4000:])
            os.replace(exe + ".tmp", exe)
    return exe


def test_the_scaled_gradients_stay_inside_exactly_sized_allocations(program):
    if os.environ.get("LD_PRELOAD"):
        # the check is only worth something with nothing preloaded in front of the sanitizer's runtime, and this test does not take a preload
        # of its environment away
        pytest.skip("LD_PRELOAD is set in this environment: the sanitized child must run with nothing preloaded")
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}      # (no ambient option may switch a report off)
    r = subprocess.run([program], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr, "sanitizer report"
    assert r.returncode == 0
    assert r.stdout.count(": ok") == 9 and "FAILED" not in r.stdout
