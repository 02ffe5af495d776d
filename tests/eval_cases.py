"""Seeded inputs of the depth-metric / supervised-loss fixtures (tests/golden/eval_*.npz), shared by tests/golden/make_golden_eval.py, which
mints the reference's answers for them, and by tests/test_eval_cpu.py / tests/test_zz_gpu_eval.py, which regenerate the same tensors instead of
loading megabytes.  A fixture stores the sha256 of every input; ``check_inputs`` compares before anything else is tested.

Every case is (pred, gt) of shape (B, 1, H, W), fp32, plus max_depth for the loss.  gt is 0 where a pixel has no measurement, as in KITTI."""
import hashlib

import numpy as np

T_VALID = 0.0001

#            name          B    H     W   valid  max_depth  seed
CASES = {
    "kitti_b1": dict(B=1, H=352, W=1216, valid=0.16, max_depth=88.0, seed=101),      # one KITTI map, about 16 % of the pixels measured
    "kitti_b4": dict(B=4, H=352, W=1216, valid=0.16, max_depth=88.0, seed=102),
    "nyu_b2": dict(B=2, H=228, W=304, valid=1.0, max_depth=10.0, seed=103),          # NYU: dense ground truth
    "odd_b3": dict(B=3, H=37, W=53, valid=0.5, max_depth=88.0, seed=104),            # n = 1961: not a multiple of 4, images 1 and 2 start unaligned
    "empty_b3": dict(B=3, H=40, W=64, valid=0.3, max_depth=88.0, seed=105),          # image 1 has no valid pixel
    "edge_b2": dict(B=2, H=48, W=64, valid=0.4, max_depth=88.0, seed=106),           # valid pixels with pred <= t_valid, pred < 0; the clamp's edges
    "nan_b2": dict(B=2, H=48, W=64, valid=0.4, max_depth=88.0, seed=107),            # a NaN in pred at a valid pixel of image 0
}
SMALL = ("odd_b3", "empty_b3", "edge_b2")      # cases whose reference gradients are stored in full
LOSS_CASES = tuple(k for k in CASES if k != "nan_b2")
# upstream gradients of the combined backward check: loss = W1 * L1 + W2 * L2
W1, W2 = 0.7, 1.3


def make_case(name):
    """-> (pred, gt, max_depth); fp32 arrays (B, 1, H, W).  Deterministic in ``name`` alone."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    shape = (c["B"], 1, c["H"], c["W"])
    hi = 0.9 * c["max_depth"]
    depth = rs.uniform(0.5, hi, size=shape)
    gt = np.where(rs.uniform(size=shape) < c["valid"], depth, 0.0).astype(np.float32)
    # a prediction everywhere (the network is dense): log-normal around the scene's depth, so that ratios fall on both sides of 1.25, 1.25^2, 1.25^3
    pred = (depth * np.exp(0.3 * rs.standard_normal(shape)) + 0.05 * rs.standard_normal(shape)).astype(np.float32)
    if name == "empty_b3":
        gt[1] = 0.0
    if name in ("edge_b2", "nan_b2"):
        # rewrite the first pixels of row 0 of image 0 (and row 1 of image 1) with hand-picked values at VALID pixels
        md = np.float32(c["max_depth"])
        picks = [(0.0, 1.0), (md, 1.0), (-1.0, 1.0), (md + 1.0, 1.0), (7.25, 7.25),       # the loss's edge rules: 0, max_depth, below, above, pred == gt
                 (5e-5, 3.0), (-0.5, 20.0), (1e-3, 2e-3), (0.0, 100.0), (120.0, 100.0),    # pred <= t_valid, pred < 0, tiny depths, gt above max_depth
                 (md, md), (0.0, 5e-5), (3.0, 0.0), (-2.0, 0.0)]                           # both at the clamp; invalid pixels
        for b, row in ((0, 0), (1, 1)):
            for i, (p, g) in enumerate(picks):
                pred[b, 0, row, i] = p
                gt[b, 0, row, i] = g
    if name == "nan_b2":
        gt[0, 0, 5, 7], pred[0, 0, 5, 7] = 10.0, np.nan       # valid pixel, NaN prediction: reaches the metrics
        gt[0, 0, 6, 9], pred[0, 0, 6, 9] = 0.0, np.nan        # invalid pixel: must not
        gt[1, 0, 3, 3], pred[1, 0, 3, 3] = np.nan, 4.0        # NaN ground truth: not valid
    return np.ascontiguousarray(pred), np.ascontiguousarray(gt), float(c["max_depth"])


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_inputs(name, pred, gt, fixture):
    """The regenerated inputs are the ones the fixture's answers were computed for."""
    assert sha256(pred) == str(fixture[name + "/sha_pred"]), f"{name}: pred differs from the tensor the fixture was minted for"
    assert sha256(gt) == str(fixture[name + "/sha_gt"]), f"{name}: gt differs from the tensor the fixture was minted for"


def grad_formula64(pred, gt, max_depth, g1, g2):
    """d(g1 L1 + g2 L2)/d pred in fp64 from the closed form (used where the reference's fp64 autograd result is too large to store; the fixture
    records how closely the two agree on every case)."""
    p64, g64 = pred.astype(np.float64), gt.astype(np.float64)
    p, g = np.clip(p64, 0.0, max_depth), np.clip(g64, 0.0, max_depth)
    m = (g > T_VALID).astype(np.float64)
    inside = ((p64 >= 0.0) & (p64 <= max_depth)).astype(np.float64)
    den = m.reshape(m.shape[0], -1).sum(axis=1).reshape(-1, 1, 1, 1) + 1e-8
    d = p - g
    return inside * m * (g1 * np.sign(d) + g2 * 2.0 * d) / den


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))
