"""Shared cases of the HAHI-neck / condition-pyramid parity tests (tests/test_neck_oracle_cpu.py on the host, tests/test_zz_gpu_neck.py on the
device): pyramids, shapes, seeded weights and features, the fp64 reference with its own error measures, and the ONE comparison both files use.

Shapes: the smallest that reach each edge class of the kernels' 8 x 32-pixel tiling at level 0 and below.  (H, W) is what
synth.make_backbone_features takes; level 0 is ceil(H/2) x ceil(W/2).
    A (34, 66)  B=2   17x33, 9x17, 5x9, 3x5     2 x 2 tiles with a one-row and a one-column remainder; every level odd: pooling everywhere
    B (32, 128) B=2   16x64, 8x32, 4x16, 2x8    exact tiles; exactly one tile at level 1; no pooling
    C (16, 16)  B=3   8x8, 4x4, 2x2, 1x1        a single-pixel top level; less than a tile everywhere
    D (50, 140) B=2   25x70, 13x35, 7x18, 4x9   three tiles per axis, an interior tile, remainders 1 and 6 (MPViT only: a cheap fp64 reference)

Where the bounds come from (never from the kernels' output):
  fp32 / f16x3 / f16r   E32 = the error of THIS oracle evaluated in fp32 (dtype=np.float32) against its fp64 evaluation; bound = 4 x max(E32, 5e-6):
                        the margin the codec tests give a kernel over a plain fp32 evaluation's own error.  The floor covers the split-f16 kernels,
                        whose operand pairs carry about 22 mantissa bits where fp32 has 24: four times the unit round-off, on products that
                        cancel (post-ReLU sums of mixed-sign terms) through five to eleven convolutions in a row.  Never looser than the bound the
                        suite already holds the neck to against the PyTorch modules, 1e-4 x max(1, max|cond|).
  bf16 / f16            the error of the oracle's operand-rounding emulation of that type (quant=: BatchNorm folded, input tensor and folded weights
                        rounded, fp64 accumulation) against fp64; bound = 3 x that.  The 3 covers what the emulation leaves out: fp32 accumulation
                        order, the 16-bit store of the up / pooled addend, the final 16-bit store.
Both measures are taken twice: max-abs over the whole map divided by max|ref|, and the relative L2 error on strips of the level-0 map (first / last
row and column, the rows 7 | 8 and columns 31 | 32 on either side of a tile seam where the map has them), each strip against the same multiple of the
reference's own relative L2 error ON THAT STRIP -- an edge or seam error that the whole map's max-abs at bf16 scale would pass.

bf16 / f16 only, a third measure per image: the relative L2 distance of the result from the EMULATION (ref + its error map) is at most the emulation's
own relative L2 error on that image plus 2^-11.  Most of a 16-bit mode's error is systematic -- the rounded weights move every pixel of a channel the
same way -- and the emulation predicts it; what it leaves out is second order next to eleven convolutions' operand roundings, except the final store
(the condition map leaves both modes as f16: at most 2^-11 relative per element, hence in L2).  So a correct kernel lies nearer to the emulation than
the emulation does to fp64, and an error the emulation does not predict is seen once it is as large as the emulation's own instead of three times
that: a wrong top-down term from two levels up (a mixed-up image at level 2) is 0.4 % of the level-0 map, inside 3 x bf16's 0.28 %.
"""
import numpy as np
import torch

from diffusiondepth_amd import synth
from oracle import ddim_oracle as O

PYRAMIDS = {"swin": (192, 384, 768, 1536), "mpvit": (128, 216, 288, 288), "res": (64, 128, 256, 512)}
SHAPES = {"A": (34, 66, 2), "B": (32, 128, 2), "C": (16, 16, 3), "D": (50, 140, 2)}          # name -> (H, W, B)
NECK_CASES = [("swin", "A"), ("swin", "B"), ("swin", "C"), ("mpvit", "A"), ("mpvit", "B"), ("mpvit", "C"), ("mpvit", "D")]
PYRAMID_CASES = [(p, s) for p in ("swin", "mpvit", "res") for s in ("A", "B", "C")]
PRECS = ("fp32", "bf16", "f16", "f16x3", "f16r")
FP32_CLASS = ("fp32", "f16x3", "f16r")
WSEED, FSEED, HSEED, ISEED = 7245, 7241, 7246, 300

FP32_MARGIN, FP32_FLOOR, EMU_MARGIN = 4.0, 5e-6, 3.0
STORE_REL = 2.0 ** -11       # f16 store of the result (bf16 mode: inner tensors bf16, the condition map f16)
EXISTING_REL = 1e-4          # x max(1, max|cond|): what test_zz_gpu_heads.py holds the neck to against the PyTorch modules


def quant_bf16(a):
    return torch.tensor(np.asarray(a)).to(torch.bfloat16).to(torch.float64).numpy()


def quant_f16(a):
    return torch.tensor(np.asarray(a)).to(torch.float16).to(torch.float64).numpy()


QUANT = {"bf16": quant_bf16, "f16": quant_f16}

_weights, _feats, _refs = {}, {}, {}


def _taps_outermost(v):
    """The same array with its taps outermost in memory: the oracle's per-tap weight slices w[:, :, dy, dx] are then contiguous matrices and its
    matmuls run in BLAS instead of NumPy's strided loop (the values, and what the library is given, do not change)."""
    return np.ascontiguousarray(v.transpose(2, 3, 0, 1)).transpose(2, 3, 0, 1) if v.ndim == 4 else v


def weights(pyr):
    """(denoiser state dict, FPN state dict, neck state dict or None) of a pyramid; fixed seeds."""
    if pyr not in _weights:
        chans = PYRAMIDS[pyr]
        sd = synth.make_state_dict(WSEED, "res" if pyr == "res" else "swin")
        fsd = {k: _taps_outermost(v) for k, v in synth.make_fpn_state_dict(FSEED, in_channels=chans).items() if not k.startswith("convup_fp")}
        hsd = None if pyr == "res" else {k: _taps_outermost(v) for k, v in synth.make_hahi_state_dict(HSEED, chans).items()}
        _weights[pyr] = (sd, fsd, hsd)
    return _weights[pyr]


def features(pyr, shape):
    key = (pyr, shape)
    if key not in _feats:
        H, W, B = SHAPES[shape]
        fp = synth.make_backbone_features(ISEED + sum(map(ord, pyr + shape)), B, H, W, in_channels=PYRAMIDS[pyr])
        for f in fp:
            f.setflags(write=False)
        _feats[key] = fp
    return _feats[key]


def oracle_cond(pyr, fp, neck, dtype=np.float64, quant=None, hsd=None):
    """The condition map of the oracle alone: [hahi_neck ->] fpn_aggregate."""
    _, fsd, hsd0 = weights(pyr)
    if neck:
        fp = O.hahi_neck(hsd0 if hsd is None else hsd, fp, dtype=dtype, quant=quant)
    return O.fpn_aggregate(fsd, fp, dtype=dtype, quant=quant)


def reference(pyr, shape, neck):
    """{"ref": fp64 map, "err": {"fp32" | "bf16" | "f16": (that evaluation of the oracle) - ref}}, computed once per (pyramid, shape, neck) and read-only."""
    key = (pyr, shape, bool(neck))
    if key not in _refs:
        fp = features(pyr, shape)
        ref = oracle_cond(pyr, fp, neck)
        err = {"fp32": oracle_cond(pyr, fp, neck, dtype=np.float32).astype(np.float64) - ref}
        for name, q in QUANT.items():
            err[name] = oracle_cond(pyr, fp, neck, quant=q) - ref
        for a in (ref, *err.values()):
            a.setflags(write=False)
        _refs[key] = {"ref": ref, "err": err}
    return _refs[key]


def emu_err_for(r, prec):
    """The error map of reference() a precision is judged by."""
    return r["err"]["fp32" if prec in FP32_CLASS else prec]


def strips(h, w):
    """name -> index into (B, C, h, w) of the level-0 strips: the map's border, and both sides of the first tile seam per axis where it exists."""
    s = {"row0": np.s_[:, :, 0, :], "col0": np.s_[:, :, :, 0], "row_last": np.s_[:, :, h - 1, :], "col_last": np.s_[:, :, :, w - 1]}
    for y in (7, 8):
        if h > 8:
            s[f"row{y}"] = np.s_[:, :, y, :]
    for x in (31, 32):
        if w > 32:
            s[f"col{x}"] = np.s_[:, :, :, x]
    return s


def _l2(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def cond_stats(got, ref, emu_err, prec):
    """The figures assert_cond_close judges: {"maxabs", "scale", "rel", "bound", "strips": {name: (rel L2, bound)}, "worst_strip": (name, rel L2, bound),
    "to_emu": [(rel L2 distance from the emulation, bound) per image] (16-bit precisions; [] otherwise)}."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == emu_err.shape, (got.shape, ref.shape, emu_err.shape)
    scale = float(np.abs(ref).max())
    d = got - ref

    def bound_of(own, cap=None):
        if prec in FP32_CLASS:
            b = FP32_MARGIN * max(own, FP32_FLOOR)
            return min(b, cap) if cap is not None else b
        return EMU_MARGIN * own

    st = {"maxabs": float(np.abs(d).max()) if np.isfinite(d).all() else float("inf"), "scale": scale}
    st["rel"] = st["maxabs"] / scale
    st["bound"] = bound_of(float(np.abs(emu_err).max()) / scale, cap=EXISTING_REL * max(1.0, scale) / scale)
    st["strips"] = {}
    for name, ix in strips(ref.shape[2], ref.shape[3]).items():
        n = _l2(ref[ix])
        e = _l2(d[ix]) / n
        st["strips"][name] = (e if np.isfinite(e) else float("inf"), bound_of(_l2(emu_err[ix]) / n))
    st["to_emu"] = []
    if prec not in FP32_CLASS:
        for b in range(ref.shape[0]):
            n = _l2(ref[b])
            e = _l2(d[b] - emu_err[b]) / n
            st["to_emu"].append((e if np.isfinite(e) else float("inf"), _l2(emu_err[b]) / n + STORE_REL))
    st["worst_strip"] = max(((k, e, b) for k, (e, b) in st["strips"].items()), key=lambda t: t[1] / t[2])
    return st


def assert_cond_close(got, ref, emu_err, prec, report=None):
    """got: a condition map (B, 256, h, w); ref: the fp64 oracle's; emu_err: the error map of the reference's own evaluation this precision is judged by
    (emu_err_for).  Raises AssertionError unless the whole-map max-abs and every strip's relative L2 are inside the bounds of the module docstring.
    report(stats): called with the figures BEFORE anything is asserted.  Returns the figures."""
    st = cond_stats(got, ref, emu_err, prec)
    if report is not None:
        report(st)
    assert np.isfinite(np.asarray(got)).all(), "non-finite values in the condition map"
    assert st["rel"] <= st["bound"], (prec, "max-abs / max|ref|", st["rel"], "bound", st["bound"])
    for name, (e, b) in st["strips"].items():
        assert e <= b, (prec, "relative L2 on strip", name, e, "bound", b)
    for i, (e, b) in enumerate(st["to_emu"]):
        assert e <= b, (prec, "relative L2 distance from the emulation, image", i, e, "bound", b)
    return st
