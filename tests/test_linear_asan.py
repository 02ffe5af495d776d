"""CPU: rows beyond M and columns beyond N that are read from memory, bias reads beyond N and stores outside [M, N], which sentinels around a
tensor cannot all see.  tests/host_emul/linear_asan_main.cpp -- a stand-alone program with its own main -- is compiled together with
csrc/dd_linear.hip, csrc/dd_api_linear.cpp and the emulation's host unit under -fsanitize=address,undefined and run as a child process, in the
manner of tests/test_swin_asan.py: no Python in that process, nothing preloaded.  It allocates every tensor and the packed image at exactly
their size and runs dd_linear_pack + dd_linear_forward on the shapes "one", "ragged" and "tile+1" of tests/linear_cases.py at the three
precisions with bias, addend and GELU.  The test passes when the child exits 0 without a sanitizer report."""
import hashlib
import os
import subprocess

import pytest

import hostemu_util as U

MAIN = os.path.join(U.EMU, "linear_asan_main.cpp")
UNITS = [os.path.join(U.CSRC, "dd_linear.hip"), os.path.join(U.CSRC, "dd_api_linear.cpp"), os.path.join(U.EMU, "ddepth_host.cpp"), MAIN]
DEPS = UNITS + [os.path.join(U.CSRC, h) for h in ("dd_linear.h", "dd_status.h")] + [os.path.join(U.EMU, "hip", "hip_runtime.h")] + \
    [os.path.join(U.ROOT, "include", "ddepth.h"), os.path.join(U.ROOT, "include", "swin", "ddepth_linear.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
# -O0 in place of the emulation's -O1, as tests/test_swin_asan.py: the instrumented kernel unit compiles in seconds
FLAGS = [f for f in U._FLAGS if f != "-O1"] + ["-O0"]


def _have_sanitizers(cxx, out):
    """Can this toolchain link and run a sanitized program at all?"""
    src, exe = os.path.join(out, "probe.cpp"), os.path.join(out, "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run([cxx] + SAN + [src, "-o", exe], capture_output=True, text=True)
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
    hsh.update(" ".join(FLAGS + SAN).encode())
    with U._BuildLock():
        out = os.path.join(U.OUT, "linear_asan_" + hsh.hexdigest()[:12])
        exe = os.path.join(out, "linear_asan")
        os.makedirs(out, exist_ok=True)
        if not _have_sanitizers(cxx, out):
            pytest.skip("this toolchain has no AddressSanitizer / UndefinedBehaviorSanitizer runtime for the host")
        if not os.path.exists(exe):
            objs = []
            for src in UNITS:
                obj = os.path.join(out, os.path.basename(src).rsplit(".", 1)[0] + ".o")
                cmd = [cxx] + FLAGS + SAN + ["-I", U.EMU, "-I", U.CSRC, src, "-o", obj]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    pytest.fail("sanitized host build of %s failed:\n%s" % (src, r.stderr[-4000:]))
                objs.append(obj)
            r = subprocess.run([cxx] + SAN + objs + ["-o", exe + ".tmp", "-lpthread"], capture_output=True, text=True)
            if r.returncode != 0:
                pytest.fail("sanitized host link failed:\n" + r.stderr[-4000:])
            os.replace(exe + ".tmp", exe)
    return exe


def _run(program, **extra):
    if os.environ.get("LD_PRELOAD"):
        # the check is only worth something with nothing preloaded in front of the sanitizer's runtime, and this test does not take a preload
        # of its environment away
        pytest.skip("LD_PRELOAD is set in this environment: the sanitized child must run with nothing preloaded")
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LINEAR_ASAN_SHORT")}      # (no ambient option may switch a report off)
    env.update(extra)
    r = subprocess.run([program], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr[-6000:])
    return r


def test_the_linear_kernels_stay_inside_exactly_sized_allocations(program):
    r = _run(program)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, "sanitizer report"
    assert r.returncode == 0
    assert r.stdout.count(": ok") == 9 and "FAILED" not in r.stdout


def test_an_x_sixteen_bytes_short_is_reported(program):
    """The check can see what it is for: the last row's last staged piece ends with x, so with 16 bytes less that load lies outside the block."""
    r = _run(program, LINEAR_ASAN_SHORT="1")
    assert r.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in r.stderr
