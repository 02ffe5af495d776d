"""GPU (`-m gpu`): the depth metrics and the supervised L1 / L2 loss (csrc/dd_eval.hip through the C ABI of include/ddepth_eval.h) against answers
minted from the reference's own classes (tests/golden/eval_*.npz, tests/golden/make_golden_eval.py) on the seeded inputs of tests/eval_cases.py.

What is asserted (both ways of combining the workgroup partials, which must also agree bit for bit):
  * n_valid and the three delta counts equal the reference's exactly, per image and over the batch;
  * every other sum and every metric v: |v - ref32| <= 4 * max(|ref32 - ref64|, 2^-23 |ref64|) -- the reference's own fp32 accumulation error (the
    device repeats it in another order, hence a small multiple) or one ulp of the fp32 result; achieved ratios are recorded with gpu_util.record;
  * grad_pred: relative L2 error against the reference's fp64 autograd within 4x that of the reference's own fp32 autograd, floor 2^-23; pixels where
    the reference's gradient is an exact 0 (masked, clamped out, pred == gt) are exactly 0;
  * NaN exactly where the reference has NaN;
  * two calls are bitwise equal, a torch.cuda.graph replayed three times equals the eager call bitwise, the ticket is left re-armed;
  * nothing synchronises the host;
  * end to end behind the Res head's forward.
(The file name sorts behind the other kernel suites on purpose: these kernels are the newest.)"""
import types

import numpy as np
import pytest
import torch

import eval_cases as E

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
COUNTS = [0, 6, 7, 8]
FLOATS = [1, 2, 3, 4, 5]
MODES = {"two_launch": 1, "ticket": 2}


@pytest.fixture(scope="module")
def U():
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a HIP device: the product has no CPU fallback")
    import gpu_util
    return gpu_util


def bound(ref32, ref64):
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    return 4.0 * np.maximum(np.abs(ref32 - ref64), ULP * np.abs(ref64))


def assert_close(v, ref32, ref64, what):
    """NaN exactly where the reference has NaN, finite and within the bound elsewhere.  Returns the largest achieved |v - ref32| / bound."""
    v, ref32, ref64 = (np.asarray(a, np.float64) for a in (v, ref32, ref64))
    assert np.array_equal(np.isnan(v), np.isnan(ref32)), (what, v, ref32)
    ok = ~np.isnan(ref32)
    assert np.isfinite(v[ok]).all(), (what, v)
    err, b = np.abs(v - ref32)[ok], bound(ref32, ref64)[ok]
    ratio = float(np.max(err / np.maximum(b, 1e-300))) if err.size else 0.0
    print(what, "max |v - ref32| / bound =", ratio)
    assert np.all(err <= b), (what, v, ref32, err, b)
    return ratio


def device_case(name, U):
    pred, gt, max_depth = E.make_case(name)
    return pred, gt, U.cu(pred), U.cu(gt), max_depth


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(E.CASES))
def test_metric_sums_and_metrics_match_the_reference(U, golden, name, mode):
    from diffusiondepth_amd import metric as M
    fx = golden("eval_metric")
    pred, gt, dp, dg, _ = device_case(name, U)
    E.check_inputs(name, pred, gt, fx)
    sums = M.metric_sums(dp, dg, 1e-4, reduce=MODES[mode])
    batch, image = M.metrics_from_sums(sums, per_image=True)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (pred.shape[0], 9) and tuple(batch.shape) == (1, 8)
    s = sums.cpu().numpy()
    print(name, mode, "counts", s[:, COUNTS].tolist(), "reference", fx[name + "/sums32"][:, COUNTS].tolist())
    assert np.array_equal(s[:, COUNTS], fx[name + "/sums32"][:, COUNTS])                          # integers: exactly the reference's
    assert np.array_equal(s[:, COUNTS].sum(axis=0), fx[name + "/batch_sums32"][COUNTS])
    r_sums = assert_close(s[:, FLOATS], fx[name + "/sums32"][:, FLOATS], fx[name + "/sums64"][:, FLOATS], f"{name} {mode} sums")
    r_batch = assert_close(batch[0].cpu().numpy(), fx[name + "/metrics32"], fx[name + "/metrics64"], f"{name} {mode} batch metrics")
    r_image = assert_close(image.cpu().numpy(), fx[name + "/image_metrics32"], fx[name + "/image_metrics64"], f"{name} {mode} image metrics")
    U.record(f"eval_metric_{name}_{mode}", sums_over_bound=r_sums, batch_metrics_over_bound=r_batch, image_metrics_over_bound=r_image)
    # the other way of combining the partials gives the same bits, and so does a second call
    other = M.metric_sums(dp, dg, 1e-4, reduce=3 - MODES[mode])
    again = M.metric_sums(dp, dg, 1e-4, reduce=MODES[mode])
    assert torch.equal(sums.view(torch.int64), other.view(torch.int64)) and torch.equal(sums.view(torch.int64), again.view(torch.int64))
    # the class: the batch row
    row = M.Diffusion_DCbase_Metric(types.SimpleNamespace()).evaluate({"gt": dg}, {"pred": dp}, "test")
    assert row.is_cuda and tuple(row.shape) == (1, 8)
    assert_close(row[0].cpu().numpy(), fx[name + "/metrics32"], fx[name + "/metrics64"], f"{name} evaluate")


def test_nan_reaches_the_metrics_only_from_a_valid_pixel(U, golden):
    from diffusiondepth_amd import metric as M
    fx = golden("eval_metric")
    _, _, dp, dg, _ = device_case("nan_b2", U)
    batch, image = M.metrics_from_sums(M.metric_sums(dp, dg), per_image=True)
    b, im = batch[0].cpu().numpy(), image.cpu().numpy()
    assert np.array_equal(np.isnan(b), np.isnan(fx["nan_b2/metrics32"])) and np.isnan(b[:5]).all() and np.isfinite(b[5:]).all()
    assert np.array_equal(np.isnan(im), np.isnan(fx["nan_b2/image_metrics32"])) and np.isfinite(im[1]).all()


def check_grad(got, name, key, fx, pred, gt, max_depth, g1, g2, U, tag):
    assert float(fx[f"{name}/grad_{key}_formula_vs_ref64"]) < 1e-15
    ref64 = fx[f"{name}/grad_{key}_64"] if name in E.SMALL else E.grad_formula64(pred, gt, max_depth, g1, g2)
    got = np.asarray(got, np.float64)
    err, lim = E.rel_l2(got, ref64), max(4.0 * float(fx[f"{name}/grad_{key}_err32"]), ULP)
    print(name, key, tag, "grad rel L2", err, "limit", lim, "reference fp32", float(fx[f"{name}/grad_{key}_err32"]))
    U.record(f"eval_grad_{name}_{key}_{tag}", rel_l2=err, limit=lim, reference_fp32=float(fx[f"{name}/grad_{key}_err32"]))
    assert err <= lim, (name, key, err, lim)
    zero = ref64 == 0.0
    assert zero.any() and np.all(got[zero] == 0.0), (name, key, "pixels with an exact zero gradient")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(E.LOSS_CASES))
def test_supervised_loss_forward_and_backward_match_the_reference(U, golden, name, mode):
    from diffusiondepth_amd import loss as L
    fx = golden("eval_loss")
    pred, gt, dp, dg, max_depth = device_case(name, U)
    E.check_inputs(name, pred, gt, fx)
    vals = {}
    for key, idx, (g1, g2) in (("l1", 0, (1.0, 0.0)), ("l2", 1, (0.0, 1.0))):
        p = dp.clone().requires_grad_(True)
        val = L.supervised_loss(p, dg, max_depth, reduce=MODES[mode])
        assert val.is_cuda and tuple(val.shape) == (2,) and val.requires_grad
        r = assert_close(val[idx].item(), fx[f"{name}/{key}_32"], fx[f"{name}/{key}_64"], f"{name} {mode} {key}")
        U.record(f"eval_loss_{name}_{key}_{mode}", value_over_bound=r)
        val[idx].backward()
        check_grad(p.grad.cpu().numpy(), name, key, fx, pred, gt, max_depth, g1, g2, U, mode)
        vals[key] = val.detach().clone()
    assert torch.equal(vals["l1"], vals["l2"])                                                   # the same call twice: the same bits
    assert torch.equal(vals["l1"], L.supervised_loss(dp, dg, max_depth, reduce=3 - MODES[mode]))   # ... and from the other combine step


@pytest.mark.parametrize("name", ["edge_b2", "kitti_b4"])
def test_loss_class_on_the_device_matches_the_reference(U, golden, name):
    import diffusiondepth_amd as dda
    fx = golden("eval_loss")
    pred, gt, dp, dg, max_depth = device_case(name, U)
    crit = dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=max_depth, loss=f"{E.W1}*L1+{E.W2}*L2+1.0*DDIM"))
    p = dp.clone().requires_grad_(True)
    loss_sum, loss_val = crit({"gt": dg}, {"pred": p, "ddim_loss": torch.tensor(0.125, device="cuda")})
    assert tuple(loss_sum.shape) == (1,) and tuple(loss_val.shape) == (1, 4) and loss_sum.requires_grad and not loss_val.requires_grad
    assert_close(loss_sum.detach().cpu().numpy(), fx[name + "/loss_sum32"], fx[name + "/loss_sum64"], name + " loss_sum")
    assert_close(loss_val.cpu().numpy(), fx[name + "/loss_val32"], fx[name + "/loss_val64"], name + " loss_val")
    loss_sum.backward()
    check_grad(p.grad.cpu().numpy(), name, "comb", fx, pred, gt, max_depth, E.W1, E.W2, U, "class")
    # two backward passes: the same bits
    q = dp.clone().requires_grad_(True)
    crit({"gt": dg}, {"pred": q, "ddim_loss": torch.tensor(0.125, device="cuda")})[0].backward()
    assert torch.equal(p.grad, q.grad)


def test_the_edge_rules_of_the_gradient_on_the_device(U):
    from diffusiondepth_amd import loss as L
    pred = torch.tensor([0.0, 88.0, -1.0, 89.0, 1.0, 3.0], device="cuda").view(1, 1, 1, 6).requires_grad_(True)
    gt = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 0.0], device="cuda").view(1, 1, 1, 6)
    L.supervised_loss(pred, gt, 88.0)[0].backward()
    want = torch.tensor([-1.0, 1.0, 0.0, 0.0, 0.0, 0.0]) * (torch.tensor(1.0) / (torch.tensor(5.0) + 1e-8))
    assert torch.equal(pred.grad.flatten().cpu(), want), pred.grad


@pytest.mark.parametrize("mode", list(MODES))
def test_graph_replay_equals_the_eager_call_and_the_ticket_is_rearmed(U, mode):
    from diffusiondepth_amd import loss as L
    from diffusiondepth_amd import metric as M
    _, _, dp, dg, max_depth = device_case("kitti_b4", U)
    go = torch.tensor([E.W1, E.W2], device="cuda")

    def run():
        sums = M.metric_sums(dp, dg, 1e-4, reduce=MODES[mode])
        row = M.metrics_from_sums(sums)
        p = dp.detach().requires_grad_(True)
        val = L.supervised_loss(p, dg, max_depth, reduce=MODES[mode])
        grad, = torch.autograd.grad(val, p, go)
        return sums, row, val.detach(), grad

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # warm the capture stream's workspace, as for any torch graph
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        captured = run()
    for _ in range(3):
        for t in captured:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(int(ws[:4096].view(torch.int32).abs().sum().item()) == 0 for ws in M._workspaces.values())      # every ticket is back at zero


def test_evaluate_and_the_loss_enqueue_without_a_host_synchronisation(U):
    import diffusiondepth_amd as dda
    _, _, dp, dg, max_depth = device_case("kitti_b1", U)
    metric = dda.Diffusion_DCbase_Metric(types.SimpleNamespace())
    crit = dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=max_depth, loss="1.0*L1+1.0*L2+1.0*DDIM"))
    ddim = torch.tensor(0.125, device="cuda")

    def work():
        row = metric.evaluate({"gt": dg}, {"pred": dp}, "test")
        p = dp.detach().requires_grad_(True)
        loss_sum, _ = crit({"gt": dg}, {"pred": p, "ddim_loss": ddim})
        loss_sum.backward()
        return row, p.grad

    work()                                   # warm-up: workspace, code objects
    torch.cuda.synchronize()
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            work()                           # raises if anything on the way synchronises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        # the build does not enforce the mode: the calls must return while long kernels enqueued in front of them are still running
        a = torch.randn(8192, 8192, device="cuda")
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        done = torch.cuda.Event()
        for _ in range(30):                  # some tenths of a second of fp32 GEMMs
            torch.mm(a, a, out=c)
        work()
        done.record()
        still_running = not done.query()
        torch.cuda.synchronize()
        assert still_running, "evaluate / loss forward+backward waited for the device"
    U.record("eval_no_host_sync", sync_debug_mode_enforced=bool(enforced))
    torch.cuda.synchronize()


def test_end_to_end_behind_the_res_head(U, golden, cases):
    """The Res head's forward on the head_res golden input, then the new metric and loss on its pred, against the eager path on the same pred (run on
    the host, where torch's fp32 division is IEEE).  Both accumulate the same fp32 per-pixel values: the counts are equal, the fp64 sums agree to fp64
    rounding, the metrics to one fp32 ulp; the loss is held to the eager fp32 composition by the rule of this file with the eager path on .double()
    inputs as the exact value."""
    import diffusiondepth_amd as dda
    from diffusiondepth_amd import loss as L
    from diffusiondepth_amd import metric as M
    from diffusiondepth_amd import synth
    c = cases["head_res"]
    sd = synth.make_state_dict(c["wseed"], "res", c["decoder_gain"], c["decoder_log_scale"])
    sd.update(synth.make_fpn_state_dict(c["fseed"]))
    B, H, W = c["B"], c["H"], c["W"]
    fp = [U.cu(f) for f in synth.make_backbone_features(c["iseed"], B, H, W)]
    gt = U.cu(synth.make_gt_depth(c["iseed"] + 1, B, H, W))
    head = dda.DDIMDepthEstimate_Res(in_channels=[64, 128, 256, 512], inference_steps=c["T"], num_train_timesteps=1000, depth_feature_dim=16,
                                     loss_cfgs=[], profile="fast").eval()
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    head = head.cuda()
    torch.manual_seed(7)
    with torch.no_grad():
        out = head(fp, gt, gt > 0, gt_depth_map=gt, return_loss=False)
    pred = out["pred"]
    assert pred.shape == gt.shape and torch.isfinite(pred).all()
    sample = {"gt": gt}
    # metric
    sums = M.metric_sums(pred, gt).cpu().numpy()
    want = M.eager_metric_sums(pred.cpu(), gt.cpu()).numpy()
    assert want[:, 0].sum() > 0
    assert np.array_equal(sums[:, COUNTS], want[:, COUNTS])
    assert np.allclose(sums, want, rtol=1e-12, atol=0)
    row = dda.Diffusion_DCbase_Metric(None).evaluate(sample, out, "test").cpu().numpy()
    want_row = M.eager_metrics_from_sums(torch.from_numpy(want)).numpy()
    assert np.all(np.abs(row - want_row) <= ULP * np.abs(want_row)), (row, want_row)
    # loss
    max_depth = 88.0
    crit = dda.Diffusion_DCbase_Loss(types.SimpleNamespace(max_depth=max_depth, loss="1.0*L1+1.0*L2+1.0*DDIM"))
    p = pred.detach().clone().requires_grad_(True)
    loss_sum, loss_val = crit(sample, {"pred": p, "ddim_loss": out["ddim_loss"].detach()})
    loss_sum.backward()
    ref = {}
    for tag, cast in (("32", lambda t: t), ("64", lambda t: t.double())):
        q = cast(pred.detach().cpu()).requires_grad_(True)
        v = L.eager_supervised_loss(q, cast(gt.cpu()), max_depth)
        v.sum().backward()
        ref[tag] = (v.detach().double().numpy(), q.grad.double().numpy())
    assert_close(loss_val[0, :2].cpu().numpy(), ref["32"][0], ref["64"][0], "head_res L1, L2")
    err, lim = E.rel_l2(p.grad.cpu().numpy(), ref["64"][1]), max(4.0 * E.rel_l2(ref["32"][1], ref["64"][1]), ULP)
    U.record("eval_end_to_end_head_res", grad_rel_l2=err, grad_limit=lim, n_valid=float(want[:, 0].sum()))
    assert err <= lim, (err, lim)
    assert abs(float(loss_val[0, 3]) - float(loss_val[0, :3].sum())) <= 1e-6 * abs(float(loss_val[0, 3]))
