#!/usr/bin/env python3
"""Mint tests/golden/kernel_table.json: which (kernel id, element kind) pairs the fused-convolution launcher routes, and the packed-weight geometry
of every routed pair -- as the commit BEFORE the kernel-id table (63a316b, the last one with the seven hand-written switches of dd_igemm2.hip)
answers, so that tests/test_igemm2_host_emulation.py::test_kernel_table_matches_parent pins the generated dispatch against it.

Never run against the working tree: the fixture is the parent's behaviour.  Re-run:

    git worktree add /tmp/dd_parent 63a316b
    python tests/golden/make_golden_kernel_table.py /tmp/dd_parent

What runs is the PARENT's host-emulated library (its tests/hostemu_util.py builds it from its csrc/):
  routed    emu_conv2(id, kind, every pointer NULL, B = 0, h = 8, w = 32) launches an empty grid and returns 0 exactly when the launcher has a kernel
            for the pair (hipErrorInvalidValue otherwise);
  geometry  dd::conv_pack_geom2(id, kind), all ten PackGeom fields -- the parent's emu_geom2 hands out eight, so a three-line shim compiled
            against the parent's headers and linked to the parent's library reads the struct itself.
For every id in 0..71 and kind in 0..5 the fixture holds null (not routed) or the ten fields.
"""
from __future__ import annotations

import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ["cin", "cout", "cout_pad", "ck", "tg", "nt", "th", "ks", "planes", "stack"]
N_IDS, N_KINDS = 72, 6
SHIM = """#include "dd_kernels.h"
extern "C" void mint_geom10(int layer, int ek, int* out) {
  const dd::PackGeom g = dd::conv_pack_geom2(layer, ek);
  static_assert(sizeof(g) == 10 * sizeof(int), "PackGeom: ten ints");
  __builtin_memcpy(out, &g, sizeof(g));
}
"""


def main():
    parent = os.path.abspath(sys.argv[1])
    assert os.path.realpath(parent) != os.path.realpath(os.path.dirname(os.path.dirname(HERE))), "mint from a checkout of the parent commit, not from this tree"
    rev = subprocess.run(["git", "-C", parent, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    spec = importlib.util.spec_from_file_location("parent_hostemu_util", os.path.join(parent, "tests", "hostemu_util.py"))
    hu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hu)
    lib = hu.bind_igemm2(hu.build_library())
    with tempfile.TemporaryDirectory() as tmp:
        src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so")
        with open(src, "w") as f:
            f.write(SHIM)
        flags = [a for a in hu._FLAGS if a != "-c"]
        subprocess.run([hu._clangxx()] + flags + ["-I", hu.EMU, "-I", hu.CSRC, "-shared", src, "-o", so, "-Wl," + lib._name], check=True)
        shim = ctypes.CDLL(so)
        table = []
        for ek in range(N_KINDS):
            row = []
            for kid in range(N_IDS):
                rc = lib.emu_conv2(kid, ek, *([None] * 11), 0, 0, None, None, None, 0, 0, 8, 32, None, None, None)
                g = (ctypes.c_int * 10)()
                shim.mint_geom10(kid, ek, g)
                row.append(list(g) if rc == 0 else None)
            table.append(row)
    out = {"minted_from": rev, "fields": FIELDS, "index": "geometry[kind][id], kind 0..5 (dd::ElemKind), id 0..71; null = the launcher has no kernel for the pair",
           "routed_per_kind": [sum(g is not None for g in row) for row in table], "geometry": table}
    path = os.path.join(HERE, "kernel_table.json")
    with open(path, "w") as f:
        f.write("{\n")
        for k in ("minted_from", "fields", "index", "routed_per_kind"):
            f.write('  "%s": %s,\n' % (k, json.dumps(out[k])))
        f.write('  "geometry": [\n' + ",\n".join("    [" + ", ".join(json.dumps(g) for g in row) + "]" for row in table) + "\n  ]\n}\n")
    print(path, out["routed_per_kind"], sum(out["routed_per_kind"]))


if __name__ == "__main__":
    main()
