#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same?  For a refactor that must not change a kernel.

    python tools/code_object_diff.py OLD_BUILD_DIR NEW_BUILD_DIR        # two diffusiondepth_amd/_build directories (object files of build.py)
    python tools/code_object_diff.py --allow-added OLD_BUILD_DIR NEW_BUILD_DIR      # for a change that may ADD kernels but not touch one

Per translation unit: pulls the gfx950 code object out of each object file (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler
--unbundle) and compares
  * the sha256 of the code objects -- equal only when nothing at all moved: hipcc names one symbol per unit after a hash of its command line
    (__hip_cuid_<hash>), so two builds into different directories differ in that name even for an untouched source file;
  * the set of symbols (name, type, size; without that __hip_cuid_ name);
  * for every function its instruction stream (llvm-objdump -d without addresses and encodings), whatever the order the functions were emitted in;
  * for every kernel its amdhsa.kernels metadata entry (registers, LDS, scratch, arguments; llvm-readelf --notes).
Exit status 0 when symbols, instruction streams and metadata agree for every unit.  With --allow-added a unit also passes when everything the
OLD build holds is in the NEW one unchanged (symbol, instruction stream, metadata) and the new one only has more; the added kernels are counted.
"""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), capture_output=True, text=True, check=True).stdout


def code_object(obj, out):
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + out + ".fat", obj)
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + out + ".fat", "--targets=" + TARGET, "--output=" + out)
    return out


def symbols(co):
    r = {}
    for ln in tool("llvm-readelf", "-sW", co).splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] in ("FUNC", "OBJECT") and not f[7].startswith("__hip_cuid_"):
            r[f[7]] = (f[3], f[2])
    return r


def functions(co):
    r, cur = {}, None
    for ln in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln)
        if m:
            cur = r.setdefault(m.group(1), [])
        elif cur is not None and ln.strip() and ln.strip() != "...":          # "...": the padding between two functions
            cur.append(re.sub(r"//.*$", "", ln).strip())                       # (branch targets are printed as offsets; the trailing comment holds the address)
    return r


def kernel_metadata(co):
    r = {}
    for b in re.split(r"\n\s*- \.agpr_count:", tool("llvm-readelf", "--notes", co))[1:]:
        b = ".agpr_count:" + b
        end = b.find("amdhsa.target")
        r[re.search(r"\.name:\s+(\S+)", b).group(1)] = (b[:end] if end > 0 else b).strip()
    return r


def main():
    argv = [a for a in sys.argv[1:] if a != "--allow-added"]
    allow_added = len(argv) != len(sys.argv) - 1
    old, new = argv[0], argv[1]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(f for f in os.listdir(old) if f.endswith(".o")):
            try:
                a, b = code_object(os.path.join(old, o), os.path.join(tmp, "a_" + o)), code_object(os.path.join(new, o), os.path.join(tmp, "b_" + o))
            except subprocess.CalledProcessError:
                continue                                                        # a host-only unit: no device code
            sha = [hashlib.sha256(open(p, "rb").read()).hexdigest()[:12] for p in (a, b)]
            sa, sb, fa, fb, ka, kb = symbols(a), symbols(b), functions(a), functions(b), kernel_metadata(a), kernel_metadata(b)
            nf = sum(1 for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
            nk = sum(1 for k in set(ka) | set(kb) if ka.get(k) != kb.get(k))
            same = sa == sb and nf == 0 and nk == 0
            # everything of the old build unchanged, the new one only has more
            kept = all(sb.get(k) == v for k, v in sa.items()) and all(fb.get(k) == v for k, v in fa.items()) and all(kb.get(k) == v for k, v in ka.items())
            if allow_added and kept and not same:
                print("%-14s symbols %d / %d  functions %d / %d  kernels %d / %d: every symbol, instruction stream and metadata entry of the old build unchanged, "
                      "%d kernels added  -> OLD DEVICE CODE IDENTICAL, KERNELS ADDED" % (o[:-2], len(sa), len(sb), len(fa), len(fb), len(ka), len(kb), len(set(kb) - set(ka))))
                continue
            bad += not same
            print("%-14s sha256 %s / %s  symbols %d / %d %s  functions %d, differing %d  kernels %d, metadata differing %d  emission order %s  -> %s" % (
                o[:-2], sha[0], sha[1], len(sa), len(sb), "same" if sa == sb else "DIFFER", len(fa), nf, len(ka), nk,
                "same" if list(fa) == list(fb) else "changed", "IDENTICAL DEVICE CODE" if same else "DEVICE CODE DIFFERS"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
