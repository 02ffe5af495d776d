"""CPU: the depth metric and the supervised loss without a GPU -- the eager torch paths of diffusiondepth_amd.metric / .loss against answers minted
from the reference's own classes (tests/golden/eval_*.npz, tests/golden/make_golden_eval.py), the loss-string parser, MetricAccumulator over a
2-rank gloo group, and the C ABI of include/ddepth_eval.h (declared == bound == exported).

Tolerances.  The fixtures hold every reference value twice: fp32 (what the reference computes) and the same class on .double() inputs.  A value v of
the code under test must satisfy |v - ref32| <= 4 * max(|ref32 - ref64|, 2^-23 |ref64|): the first term is the reference's own fp32 accumulation
error, which another summation order repeats with another sign, hence a small multiple; the second is one ulp of an fp32 result.  n_valid and the
three delta counts are integers and must be equal.  Gradients: relative L2 error against the reference's fp64 autograd within 4x that of the
reference's own fp32 autograd, floor 2^-23; where the reference gives an exact 0 (masked, clamped-out, pred == gt) the result must be 0."""
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusiondepth_amd as dda
from diffusiondepth_amd import dist as ddist
from diffusiondepth_amd import loss as L
from diffusiondepth_amd import metric as M

import eval_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
COUNTS = [0, 6, 7, 8]
FLOATS = [1, 2, 3, 4, 5]


def bound(ref32, ref64):
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    return 4.0 * np.maximum(np.abs(ref32 - ref64), ULP * np.abs(ref64))


def assert_close(v, ref32, ref64, what):
    """NaN exactly where the reference has NaN; elsewhere within the bound.  Returns the largest achieved |v - ref32| / bound."""
    v, ref32, ref64 = (np.asarray(a, np.float64) for a in (v, ref32, ref64))
    assert np.array_equal(np.isnan(v), np.isnan(ref32)), (what, v, ref32)
    ok = ~np.isnan(ref32)
    err, b = np.abs(v - ref32)[ok], bound(ref32, ref64)[ok]
    assert np.all(err <= b), (what, v, ref32, err, b)
    return float(np.max(err / np.maximum(b, 1e-300))) if err.size else 0.0


def tensors(name):
    pred, gt, max_depth = E.make_case(name)
    return torch.from_numpy(pred), torch.from_numpy(gt), max_depth


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_eval_header_declares_the_bound_symbols_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ddepth_eval.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(dd_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(M.ABI_SYMBOLS), declared ^ set(M.ABI_SYMBOLS)
    lib = dda.load_library()
    for s in declared:
        assert hasattr(lib, s), s
    # none of them leaked into the handle-based header
    main = open(os.path.join(ROOT, "include", "ddepth.h")).read()
    assert not any(s in main for s in declared)


def test_workspace_query_and_argument_checks_need_no_device():
    import ctypes
    lib = M._lib()
    n = ctypes.c_int64(0)
    assert lib.dd_eval_workspace_bytes(4, 352, 1216, ctypes.byref(n)) == 0 and n.value >= 16 + 4 * 9 * 8
    small = ctypes.c_int64(0)
    assert lib.dd_eval_workspace_bytes(1, 8, 8, ctypes.byref(small)) == 0 and 16 < small.value < n.value
    assert lib.dd_eval_workspace_bytes(0, 8, 8, ctypes.byref(small)) != 0 and b"positive" in lib.dd_eval_last_error()
    assert lib.dd_depth_metric_sums(None, None, None, None, 1, 8, 8, 1e-4, 0, None) != 0 and b"null" in lib.dd_eval_last_error()
    assert lib.dd_sup_loss_backward(None, None, None, None, None, None, 1, 8, 8, 88.0, 1e-4, None) != 0


def test_exports():
    assert dda.Diffusion_DCbase_Metric is M.Diffusion_DCbase_Metric and dda.MetricAccumulator is M.MetricAccumulator
    assert dda.Diffusion_DCbase_Loss is L.Diffusion_DCbase_Loss


def test_hip_only_entry_points_refuse_cpu_tensors():
    p, g, _ = tensors("odd_b3")
    with pytest.raises(RuntimeError, match="HIP device"):
        M.metric_sums(p, g)


# ---- metric ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.CASES))
def test_eager_metric_matches_the_reference(golden, name):
    fx = golden("eval_metric")
    pred, gt, _ = tensors(name)
    E.check_inputs(name, pred.numpy(), gt.numpy(), fx)
    sums = M.eager_metric_sums(pred, gt, 1e-4)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (pred.shape[0], 9)
    s = sums.numpy()
    assert np.array_equal(s[:, COUNTS], fx[name + "/sums32"][:, COUNTS])                       # integers: equal
    assert_close(s[:, FLOATS], fx[name + "/sums32"][:, FLOATS], fx[name + "/sums64"][:, FLOATS], "sums")
    assert np.array_equal(s.sum(axis=0)[COUNTS], fx[name + "/batch_sums32"][COUNTS])
    batch, image = M.metrics_from_sums(sums, per_image=True)
    assert batch.dtype == torch.float32 and tuple(batch.shape) == (1, 8) and tuple(image.shape) == (pred.shape[0], 8)
    assert_close(batch[0].numpy(), fx[name + "/metrics32"], fx[name + "/metrics64"], "batch metrics")
    assert_close(image.numpy(), fx[name + "/image_metrics32"], fx[name + "/image_metrics64"], "image metrics")


def test_metric_class_is_the_references_interface(golden):
    fx = golden("eval_metric")
    m = dda.Diffusion_DCbase_Metric(types.SimpleNamespace())
    assert m.metric_name == ["RMSE", "MAE", "iRMSE", "iMAE", "REL", "D^1", "D^2", "D^3"] and m.t_valid == 0.0001
    pred, gt, _ = tensors("empty_b3")
    r = m.evaluate({"gt": gt}, {"pred": pred.requires_grad_(True)}, "val")
    assert tuple(r.shape) == (1, 8) and r.dtype == torch.float32 and not r.requires_grad and r.device == pred.device
    assert_close(r[0].numpy(), fx["empty_b3/metrics32"], fx["empty_b3/metrics64"], "evaluate")
    # no valid pixel at all: 0 / 1e-8 = 0, as in the reference
    z = m.evaluate({"gt": torch.zeros(1, 1, 4, 6)}, {"pred": torch.ones(1, 1, 4, 6)}, "val")
    assert torch.equal(z, torch.zeros(1, 8))


def test_nan_case_has_nan_where_the_reference_has(golden):
    fx = golden("eval_metric")
    assert np.isnan(fx["nan_b2/metrics32"][:5]).all() and not np.isnan(fx["nan_b2/metrics32"][5:]).any()      # what the reference does
    assert not np.isnan(fx["nan_b2/image_metrics32"][1]).any()                                                  # image 1 is clean


# ---- loss -----------------------------------------------------------------------------------------------------------------------------------
def check_grad(got, name, key, fx, pred, gt, max_depth, g1, g2):
    """got against the reference's fp64 autograd (stored for the small cases, the closed form elsewhere: the fixture records that the two agree)."""
    assert float(fx[f"{name}/grad_{key}_formula_vs_ref64"]) < 1e-15
    ref64 = fx[f"{name}/grad_{key}_64"] if name in E.SMALL else E.grad_formula64(pred, gt, max_depth, g1, g2)
    got = np.asarray(got, np.float64)
    err, lim = E.rel_l2(got, ref64), max(4.0 * float(fx[f"{name}/grad_{key}_err32"]), ULP)
    assert err <= lim, (name, key, err, lim)
    zero = ref64 == 0.0
    assert zero.any() and np.all(got[zero] == 0.0), (name, key, "pixels with an exact zero gradient")
    if name in E.SMALL:
        assert np.array_equal(fx[f"{name}/grad_{key}_32"] == 0.0, zero)
    return err / lim


@pytest.mark.parametrize("name", list(E.LOSS_CASES))
def test_eager_loss_and_autograd_match_the_reference(golden, name):
    fx = golden("eval_loss")
    pred, gt, max_depth = tensors(name)
    E.check_inputs(name, pred.numpy(), gt.numpy(), fx)
    for key, idx, (g1, g2) in (("l1", 0, (1.0, 0.0)), ("l2", 1, (0.0, 1.0))):
        p = pred.clone().requires_grad_(True)
        val = L.supervised_loss(p, gt, max_depth)
        assert tuple(val.shape) == (2,)
        assert_close(val[idx].item(), fx[f"{name}/{key}_32"], fx[f"{name}/{key}_64"], key)
        val[idx].backward()
        check_grad(p.grad.numpy(), name, key, fx, pred.numpy(), gt.numpy(), max_depth, g1, g2)


@pytest.mark.parametrize("name", ["edge_b2", "nyu_b2"])
def test_loss_class_matches_the_reference(golden, name):
    fx = golden("eval_loss")
    pred, gt, max_depth = tensors(name)
    crit = dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=max_depth, loss=f"{E.W1}*L1+{E.W2}*L2+1.0*DDIM"))
    assert crit.loss_name == list(fx[name + "/loss_name"]) == ["L1", "L2", "DDIM", "Total"]
    p = pred.clone().requires_grad_(True)
    loss_sum, loss_val = crit({"gt": gt}, {"pred": p, "ddim_loss": torch.tensor(0.125)})
    assert tuple(loss_sum.shape) == (1,) and tuple(loss_val.shape) == (1, 4) and loss_sum.requires_grad and not loss_val.requires_grad
    assert_close(loss_sum.detach().numpy(), fx[name + "/loss_sum32"], fx[name + "/loss_sum64"], "loss_sum")
    assert_close(loss_val.numpy(), fx[name + "/loss_val32"], fx[name + "/loss_val64"], "loss_val")
    loss_sum.backward()
    check_grad(p.grad.numpy(), name, "comb", fx, pred.numpy(), gt.numpy(), max_depth, E.W1, E.W2)


def test_the_edge_rules_of_the_gradient():
    """clamp passes gradient at both ends of [0, max_depth], abs has gradient 0 at 0, masked pixels get 0: pred = 0, 88, -1, 89, pred == gt with gt = 1
    give -1, +1, 0, 0, 0 for L1 (one image, five valid pixels: times 1 / 5)."""
    pred = torch.tensor([0.0, 88.0, -1.0, 89.0, 1.0, 3.0]).view(1, 1, 1, 6).requires_grad_(True)
    gt = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 0.0]).view(1, 1, 1, 6)
    L.supervised_loss(pred, gt, 88.0)[0].backward()
    assert torch.allclose(pred.grad.flatten() * 5, torch.tensor([-1.0, 1.0, 0.0, 0.0, 0.0, 0.0]), rtol=1e-6, atol=0)


def test_loss_string_parser():
    assert list(L.parse_loss("1.0*L1+1.0*L2+1.0*DDIM").items()) == [("L1", 1.0), ("L2", 1.0), ("DDIM", 1.0)]
    assert list(L.parse_loss("0.5*DDIM+2*L2").items()) == [("DDIM", 0.5), ("L2", 2.0)]
    assert list(L.parse_loss("1e-1*Sig+3*BIN+0.25*L1").items()) == [("Sig", 0.1), ("BIN", 3.0), ("L1", 0.25)]
    for bad in ("1.0*L3", "1.0*L1+1.0*Chamfer", "1.0*l1"):
        with pytest.raises(NotImplementedError):
            L.parse_loss(bad)
    with pytest.raises(NotImplementedError):
        dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=88.0, loss="1.0*L1+1.0*Smoth"))
    with pytest.raises(ValueError):
        L.parse_loss("L1")
    crit = dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=88.0, loss="2.0*L2+0.5*BIN+1.0*Sig"))
    assert crit.loss_name == ["L2", "BIN", "Sig", "Total"]
    assert [crit.loss_dict[k]["weight"] for k in crit.loss_name] == [2.0, 0.5, 1.0, 1.0] and crit.loss_dict["Total"]["func"] is None
    pred, gt, _ = tensors("odd_b3")
    pred = pred.abs() + 0.1
    out = {"pred": pred, "bin_losses": {"loss_depth": torch.tensor(0.5), "loss_chamfer": torch.tensor(0.25)}}
    loss_sum, loss_val = crit({"gt": gt}, out)
    l2 = L.supervised_loss(pred, gt, 88.0)[1]
    assert tuple(loss_val.shape) == (1, 4)
    assert torch.allclose(loss_val[0, 0], 2.0 * l2) and torch.allclose(loss_val[0, 1], torch.tensor(0.375))
    keep = gt > 0
    g = torch.log(pred[keep] + 0.001) - torch.log(gt[keep] + 0.001)
    assert torch.allclose(loss_val[0, 2], 2.0 * torch.sqrt(g.var() + 0.15 * g.mean() ** 2))
    assert torch.allclose(loss_val[0, 3], loss_val[0, :3].sum()) and torch.allclose(loss_sum, loss_val[0, 3:])


# ---- accumulator ----------------------------------------------------------------------------------------------------------------------------
N_BATCHES = 5


def _batch(i):
    rs = np.random.RandomState(900 + i)
    shape = (1 + i % 2, 1, 12, 20)
    gt = np.where(rs.uniform(size=shape) < 0.5, rs.uniform(1, 60, size=shape), 0.0).astype(np.float32)
    pred = (gt + rs.standard_normal(shape) + 20.0 * (gt == 0)).astype(np.float32)
    return {"gt": torch.from_numpy(gt)}, {"pred": torch.from_numpy(pred)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _acc_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    ddist.init_from_env("gloo")
    acc = dda.MetricAccumulator()
    for i in ddist.shard_indices(N_BATCHES, rank, world):
        acc.update(*_batch(i))
    res = acc.reduce().result()
    if rank == 0:
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_accumulator_over_two_gloo_ranks_equals_one_process_over_the_union(tmp_path):
    out = str(tmp_path / "acc.pt")
    mp.spawn(_acc_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    two = torch.load(out, weights_only=False)
    acc, metric = dda.MetricAccumulator(), dda.Diffusion_DCbase_Metric()
    rows = []
    for i in range(N_BATCHES):
        row = acc.update(*_batch(i))
        assert torch.equal(row, metric.evaluate(*_batch(i), "test"))
        rows.append(row)
    one = acc.reduce().result()          # not distributed: the identity
    assert two["batches"] == one["batches"] == N_BATCHES and two["n_valid"] == one["n_valid"] > 0
    assert np.array_equal(two["sums"][COUNTS], one["sums"][COUNTS])
    # fp64 sums added in another order (rank 0's shard + rank 1's): equal up to fp64 rounding
    assert np.allclose(two["sums"], one["sums"], rtol=1e-13, atol=0) and np.allclose(two["batch_mean"], one["batch_mean"], rtol=1e-6, atol=0)
    assert np.allclose(two["exact"], one["exact"], rtol=1e-6, atol=0)
    assert np.allclose(one["batch_mean"], torch.cat(rows).double().mean(dim=0).numpy(), rtol=1e-6, atol=0)
    # the exact metrics are those of ONE evaluate over every image of the set
    gts, preds = zip(*[(s["gt"].flatten(), o["pred"].flatten()) for s, o in map(_batch, range(N_BATCHES))])
    whole = metric.evaluate({"gt": torch.cat(gts).view(1, 1, 1, -1)}, {"pred": torch.cat(preds).view(1, 1, 1, -1)}, "test")
    assert np.allclose(one["exact"], whole[0].numpy(), rtol=1e-6, atol=0)
    with pytest.raises(RuntimeError):
        acc.update(*_batch(0))
