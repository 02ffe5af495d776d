#!/usr/bin/env python3
"""Instruction mix of the convolution kernels' code objects: compiles a kernel source to assembly (device only, no GPU needed) and prints, per
selected instantiation, VGPRs and scratch, the static MFMA / VALU / SALU / LDS / VMEM instruction counts, the most frequent VALU opcodes and a
DYNAMIC count per wave and tile.

    python tools/isa_mix.py 'Cfg2<(2|5), (1|2|46)>' [--mfma-per-tile 576] [--src dd_thin.hip] [--asm FILE.s] [extra hipcc flags]

Dynamic count: the kernel's main loop (the innermost loop that holds every MFMA: conv2's loop over its two cout splits, conv3's loop over pairs
of channel chunks) runs  trips = mfma-per-tile / static MFMAs  times, everything else once:  dynamic = static + (trips - 1) * loop body.  The
loop body is the text between the loop's header and its last back edge plus the out-of-line blocks behind it that jump back into it (hipcc
places rarely taken blocks, e.g. a conditional DMA piece, behind the loop).  Without --mfma-per-tile the dynamic count is the static one.
--asm reads an assembly file made earlier (e.g. of the parent commit) instead of compiling."""
import os, re, subprocess, sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def take(argv, flag, default=None):
    if flag in argv:
        i = argv.index(flag)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


def kind(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.startswith("v_"): return "valu"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")): return "scratch" if op.startswith("scratch_") else "vmem"
    return "other"


def parse(body):
    """-> (instructions [(opcode, operands)], {label: index of the instruction that follows it})"""
    labels, insts = {}, []
    for ln in body.split(".Lfunc_end")[0].split("\n"):
        m = re.match(r"^(\.LBB[0-9_]+):", ln)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\b(.*)", ln)
        if m and not ln.lstrip().startswith((";", ".")):
            insts.append((m.group(1), m.group(2)))
    return insts, labels


def main_loop(insts, labels):
    """indices of the instructions of the innermost loop that contains every MFMA (with its out-of-line blocks), or [] when there is none"""
    mf = [i for i, (op, _) in enumerate(insts) if op.startswith("v_mfma")]
    if not mf:
        return []
    branches = []      # (index, target index)
    for i, (op, rest) in enumerate(insts):
        if op.startswith("s_cbranch") or op == "s_branch":
            m = re.search(r"(\.LBB[0-9_]+)", rest)
            if m and m.group(1) in labels:
                branches.append((i, labels[m.group(1)]))
    ends = {}
    for i, t in branches:
        if t <= i and t <= mf[0] and i >= mf[-1]:
            ends[t] = max(ends.get(t, 0), i)
    if not ends:
        return []
    head = max(ends)          # the innermost such header
    end = ends[head]
    body = set(range(head, end + 1))
    starts = sorted(set(labels.values()))
    for i, t in branches:      # out-of-line blocks: behind the loop, jumping back into it
        if i > end and head < t <= end:
            blk = max(s for s in starts if s <= i)
            if blk > end:
                body.update(range(blk, i + 1))
    return sorted(body)


def main():
    argv = sys.argv[1:]
    src_name = take(argv, "--src", "dd_igemm2.hip")
    asm = take(argv, "--asm")
    per_tile = take(argv, "--mfma-per-tile")
    pat = argv[0] if argv else r"Cfg2<(2|5), (1|2|46)>"
    if asm is None:
        asm = "/tmp/" + src_name.replace(".", "_") + "_isa.s"
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-x", "hip",
                        "--cuda-device-only", "-S", "-o", asm, os.path.join(ROOT, "diffusiondepth_amd", "csrc", src_name)] + argv[1:], check=True, capture_output=True)
    s = open(asm).read()
    parts = re.split(r"\n(_ZN2dd[0-9A-Za-z_]*_kernel[^\n:]*):[^\n]*\n", s)
    names, bodies = parts[1::2], parts[2::2]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    for n, mangled, b in zip(dem, names, bodies):
        if not re.search(pat, n):
            continue
        insts, labels = parse(b)
        c = Counter(op for op, _ in insts)
        st = Counter(kind(op) for op, _ in insts)
        meta = s[s.find(".name:           " + mangled):][:4000] if (".name:           " + mangled) in s else ""
        vg = re.search(r"\.vgpr_count:\s+(\d+)", meta)
        ag = re.search(r"\.agpr_count:\s+(\d+)", meta)
        sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        print(n)
        print("   vgpr", vg.group(1) if vg else "?", "agpr", ag.group(1) if ag else "?", "scratch", sc.group(1) if sc else "?",
              "| static: mfma", st["mfma"], "valu", st["valu"], "salu", st["salu"], "lds", st["lds"], "vmem", st["vmem"], "scratch ops", st["scratch"],
              "| buffer_load", sum(v for k, v in c.items() if k.startswith("buffer_load")), "buffer_store", sum(v for k, v in c.items() if k.startswith("buffer_store")),
              "global_load", sum(v for k, v in c.items() if k.startswith("global_load")), "global_store", sum(v for k, v in c.items() if k.startswith("global_store")))
        loop = Counter(kind(insts[i][0]) for i in main_loop(insts, labels))
        trips = (float(per_tile) / st["mfma"]) if (per_tile and st["mfma"]) else 1.0
        dyn = {k: st[k] + (trips - 1.0) * loop[k] for k in ("mfma", "valu", "salu")}
        if st["mfma"]:
            print("   main loop: mfma %d valu %d salu %d, trips %.3g | dynamic per wave and tile: valu %.0f salu %.0f mfma %.0f -> VALU/MFMA %.2f SALU/MFMA %.2f"
                  % (loop["mfma"], loop["valu"], loop["salu"], trips, dyn["valu"], dyn["salu"], dyn["mfma"], dyn["valu"] / dyn["mfma"], dyn["salu"] / dyn["mfma"]))
        print("   ", [(k, v) for k, v in c.most_common(60) if k.startswith("v_") and not k.startswith("v_mfma")][:30])


if __name__ == "__main__":
    main()
