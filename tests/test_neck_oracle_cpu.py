"""CPU: the fp64 oracle of the HAHI neck (oracle.ddim_oracle.hahi_neck) and the comparison the GPU neck tests judge the kernels by
(neck_cases.assert_cond_close), before either is trusted on the device:
  * the oracle against the product's own PyTorch module in fp64 (diffusiondepth_amd.necks.HAHIHeteroNeck, attention off -- the module the
    goldens of tests/golden/make_golden_hahi.py tie to the reference), 1e-10 x max;
  * fpn_aggregate(..., quant=None) is the function it was, bit for bit;
  * the comparison REJECTS four wrong answers, built with the oracle alone, under every precision's bound -- the mistakes a neck kernel can make
    behind buffer descriptors (an out-of-range read gives zero, an out-of-range store is dropped) without faulting.
"""
import numpy as np
import pytest
import torch

import neck_cases as NC
from diffusiondepth_amd import synth
from diffusiondepth_amd.necks import HAHIHeteroNeck
from oracle import ddim_oracle as O


@pytest.mark.parametrize("pyr,shape", [("swin", "C"), ("mpvit", "C"), ("mpvit", "A")])
def test_hahi_neck_oracle_matches_the_product_module_in_fp64(pyr, shape):
    chans = list(NC.PYRAMIDS[pyr])
    _, _, hsd = NC.weights(pyr)
    fp = NC.features(pyr, shape)
    neck = HAHIHeteroNeck(in_channels=chans, out_channels=chans, embedding_dim=512, cross_att=False, self_att=False).double().eval()
    missing, unexpected = neck.load_state_dict({k[len("hahineck."):]: torch.from_numpy(v).double() for k, v in hsd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    with torch.no_grad():
        want = [t.numpy() for t in neck([torch.tensor(f).double() for f in fp])]
    got = O.hahi_neck(hsd, fp)
    assert len(got) == len(want) == 4
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float64 and g.shape == w.shape == fp[i].shape
        assert np.abs(g - w).max() <= 1e-10 * np.abs(w).max(), (pyr, shape, i, np.abs(g - w).max())


def _fpn_aggregate_before(fsd, fp, dtype=np.float64):
    """oracle.ddim_oracle.fpn_aggregate as it stood before it took `quant` (kept here verbatim to pin the default path)."""
    sd = O._cast_sd(fsd, dtype)
    n = len(fp)
    x = None
    for i in range(n):
        lvl = n - i - 1
        f = np.asarray(fp[lvl], dtype=dtype)
        cur = O.relu(O.batch_norm_eval(O.conv2d(f, sd[f"conv_lateral.{lvl}.0.weight"]), *O._bn_args(sd, f"conv_lateral.{lvl}.1")))
        if i > 0:
            up = O.conv_transpose2d(x, sd[f"conv_up.{lvl}.0.weight"], None, stride=2, pad=0)
            up = O.relu(O.batch_norm_eval(up, *O._bn_args(sd, f"conv_up.{lvl}.1")))
            cur = cur + O.adaptive_avg_pool2d(up, cur.shape[2], cur.shape[3])
        x = cur
    return x


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fpn_aggregate_without_quant_is_bit_identical_to_the_function_it_was(dtype):
    fsd = synth.make_fpn_state_dict(7241)
    fp = synth.make_backbone_features(5, 2, 18, 22)          # 9x11, 5x6, 3x3, 2x2: pooling active
    a = O.fpn_aggregate(fsd, fp, dtype=dtype, quant=None)
    b = O.fpn_aggregate(fsd, fp, dtype=dtype)
    want = _fpn_aggregate_before(fsd, fp, dtype)
    assert a.dtype == want.dtype and np.array_equal(a, want) and np.array_equal(b, want)


def test_quant_emulation_folds_batchnorm_and_rounds_operands_only():
    """quant = identity is the folded form of the same arithmetic (fp64 round-off apart); quant = a rounding moves the result by that format's
    operand error and no more (bf16: 2^-9 per operand, K <= 4608 products of mixed sign)."""
    fsd = synth.make_fpn_state_dict(7241)
    fp = synth.make_backbone_features(5, 2, 18, 22)
    ref = O.fpn_aggregate(fsd, fp)
    scale = np.abs(ref).max()
    assert np.abs(O.fpn_aggregate(fsd, fp, quant=lambda a: a) - ref).max() <= 1e-12 * scale
    e_bf, e_h = (np.abs(O.fpn_aggregate(fsd, fp, quant=q) - ref).max() / scale for q in (NC.quant_bf16, NC.quant_f16))
    assert 2.0 ** -13 < e_bf < 2.0 ** -5 and e_h < e_bf / 4 and e_h > 2.0 ** -16, (e_bf, e_h)


# ---- the comparison can reject wrong answers ------------------------------------------------------------------------------------------------------
def _corrupted(pyr, which):
    """A condition map that is wrong in one of the ways a neck kernel behind buffer descriptors can be, from the oracle alone (shape A)."""
    fp = [f.copy() for f in NC.features(pyr, "A")]
    _, _, hsd = NC.weights(pyr)
    hsd = dict(hsd)
    if which == "last_column_zero":                # the last column of the level-0 feature read as zero (an extent one column short)
        fp[0][:, :, :, -1] = 0
    elif which == "cat_swapped":                   # level 0 fused from [l_0 | e_0] instead of [e_0 | l_0]: the same weights on the other channel order
        k = "hahineck.conv_fusion.0.conv.weight"   # W . [l | e] == roll(W, 512 input channels) . [e | l]
        hsd[k] = np.roll(hsd[k], 512, axis=1)
    elif which == "image_mixed":                   # image 1's level-2 neck input is image 0's (a batch offset not applied)
        fp[2][1] = fp[2][0]
    elif which == "gap_misplaced":                 # MPViT: the level-1 fusion's input channels rolled by 8 (216 carried as 224: the gap in the wrong place)
        k = "hahineck.trans_fusion.0.conv.weight"
        hsd[k] = np.roll(hsd[k], 8, axis=1)
    else:
        raise ValueError(which)
    return NC.oracle_cond(pyr, fp, True, hsd=hsd)


_bad = {}


def _bad_for(pyr, which):
    if (pyr, which) not in _bad:
        b = _corrupted(pyr, which)
        b.setflags(write=False)
        _bad[(pyr, which)] = b
    return _bad[(pyr, which)]


WRONG = [(p, w) for p in ("swin", "mpvit") for w in ("last_column_zero", "cat_swapped", "image_mixed")] + [("mpvit", "gap_misplaced")]


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr,which", WRONG)
def test_the_comparison_rejects_a_wrong_answer(pyr, which, prec):
    r = NC.reference(pyr, "A", True)
    bad = _bad_for(pyr, which)
    with pytest.raises(AssertionError):
        NC.assert_cond_close(bad, r["ref"], NC.emu_err_for(r, prec), prec)


@pytest.mark.parametrize("prec", NC.PRECS)
@pytest.mark.parametrize("pyr", ["swin", "mpvit"])
def test_the_comparison_accepts_the_references_own_evaluations(pyr, prec):
    """... and passes what it should: the fp32 evaluation under the fp32 class's bound, each emulation under its own."""
    r = NC.reference(pyr, "A", True)
    err = NC.emu_err_for(r, prec)
    st = NC.assert_cond_close(r["ref"] + err, r["ref"], err, prec)
    assert st["bound"] <= NC.EXISTING_REL * max(1.0, st["scale"]) / st["scale"] or prec in ("bf16", "f16")
    assert set(st["strips"]) == {"row0", "col0", "row_last", "col_last", "row7", "row8", "col31", "col32"}      # shape A: 17 x 33


def test_the_comparison_rejects_a_single_wrong_seam_column_at_bf16_scale():
    """What the strips are for: one level-0 column (31, the last of the first tile) off by 2 % -- inside the whole map's bf16 max-abs bound
    where the map is small, far outside that column's own relative L2."""
    r = NC.reference("mpvit", "A", True)
    bad = r["ref"].copy()
    small = np.abs(bad[:, :, :, 31]) < 0.2 * np.abs(r["ref"]).max()
    bad[:, :, :, 31] = np.where(small, bad[:, :, :, 31] * 1.02, bad[:, :, :, 31])
    st = NC.cond_stats(bad, r["ref"], r["err"]["bf16"], "bf16")
    assert st["rel"] <= st["bound"]                                      # the whole-map measure lets it through ...
    with pytest.raises(AssertionError, match="col31"):                     # ... the strip does not
        NC.assert_cond_close(bad, r["ref"], r["err"]["bf16"], "bf16")
