"""Drop-in for the reference's evaluation metric, over the C ABI of include/ddepth_eval.h.

Reference interface mirrored here (same names, attributes, argument order and result shape):
  Diffusion_DCbase_Metric           src/metric/diffusion_dcbase_metric.py:20-93  (RMSE, MAE, iRMSE, iMAE, REL, D^1, D^2, D^3)
so a reference checkout switches over with ``from diffusiondepth_amd.metric import Diffusion_DCbase_Metric``.

HIP tensors go through libddepth_hip.so (csrc/dd_eval.hip): one streaming pass makes nine fp64 sums per image, a second tiny launch turns
them into the eight metrics; nothing synchronises the host, so an evaluation loop no longer drains the device after every image (the
reference's four boolean-mask gathers each do).  Tensors that are not on a HIP device run the eager torch path below, written from the
same formulas (the package's usual "plumbing, no GPU" rule); it uses ``torch.where`` instead of gathers and accumulates in fp64 like the
kernel.

``MetricAccumulator`` adds what the reference lacks: running sums kept ON THE DEVICE and one final reduce over ranks.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch

from . import backend
from . import dist as ddist

# every symbol include/ddepth_eval.h declares (checked by tests/test_eval_cpu.py)
ABI_SYMBOLS = ["dd_eval_last_error", "dd_eval_workspace_bytes", "dd_depth_metric_sums", "dd_depth_metrics", "dd_sup_loss_forward",
               "dd_sup_loss_backward"]

METRIC_NAMES = ["RMSE", "MAE", "iRMSE", "iMAE", "REL", "D^1", "D^2", "D^3"]
N_SUMS = 9          # DD_METRIC_SUMS: [n_valid, S|d|, Sd^2, S|dinv|, Sdinv^2, S|d|/(gt+1e-8), #(ratio<1.25), #(ratio<1.25^2), #(ratio<1.25^3)]
REDUCE_DEFAULT, REDUCE_TWO_LAUNCH, REDUCE_TICKET = 0, 1, 2      # dd_eval_reduce

_bound = None
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def _lib():
    global _bound
    if _bound is None:
        lib = backend.load_library()
        c_int, c_vp, c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
        lib.dd_eval_last_error.restype, lib.dd_eval_last_error.argtypes = ctypes.c_char_p, []
        lib.dd_eval_workspace_bytes.restype = c_int
        lib.dd_eval_workspace_bytes.argtypes = [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64)]
        lib.dd_depth_metric_sums.restype, lib.dd_depth_metric_sums.argtypes = c_int, [c_vp] * 4 + [c_int] * 3 + [c_f, c_int, c_vp]
        lib.dd_depth_metrics.restype, lib.dd_depth_metrics.argtypes = c_int, [c_vp] * 3 + [c_int, c_vp]
        lib.dd_sup_loss_forward.restype, lib.dd_sup_loss_forward.argtypes = c_int, [c_vp] * 5 + [c_int] * 3 + [c_f, c_f, c_int, c_vp]
        lib.dd_sup_loss_backward.restype, lib.dd_sup_loss_backward.argtypes = c_int, [c_vp] * 6 + [c_int] * 3 + [c_f, c_f, c_vp]
        _bound = lib
    return _bound


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {_lib().dd_eval_last_error().decode()}")


def _stream(t):
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def _image_shape(t: torch.Tensor) -> Tuple[int, int, int]:
    """(B, H, W) as the ABI counts them: the first dimension is the batch, the last the row, everything between is folded into H."""
    if t.dim() < 2:
        raise RuntimeError(f"expected a (B,1,H,W) depth map, got shape {tuple(t.shape)}")
    B, W = int(t.shape[0]), int(t.shape[-1])
    return B, int(t.numel() // max(B * W, 1)), W


def _pair(pred: torch.Tensor, gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if pred.shape != gt.shape:
        raise RuntimeError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    if pred.device != gt.device:
        raise RuntimeError(f"pred ({pred.device}) and gt ({gt.device}) must be on the same device")
    if pred.numel() == 0:
        raise RuntimeError("empty depth map")
    return pred.detach().float().contiguous(), gt.detach().float().contiguous()


def workspace_for(t: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """The device scratch of the two reductions: one buffer per (device, stream), zeroed ONCE when it is allocated (the ticket of the
    ticket reducer; every call re-arms it) and grown when a larger shape arrives.  Steady state allocates nothing.  A first call inside
    a graph capture would allocate from the capture's pool: call once eagerly before capturing, as for any torch graph."""
    need = ctypes.c_int64(0)
    _ck(_lib().dd_eval_workspace_bytes(B, H, W, ctypes.byref(need)), "dd_eval_workspace_bytes")
    key = (t.device.index if t.device.index is not None else torch.cuda.current_device(), _stream(t))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need.value:
        ws = torch.zeros(int(need.value), dtype=torch.uint8, device=t.device)
        _workspaces[key] = ws
    return ws


# ---- the library path -------------------------------------------------------------------------------------------------------------------
def metric_sums(pred: torch.Tensor, gt: torch.Tensor, t_valid: float = 1e-4, reduce: int = REDUCE_DEFAULT) -> torch.Tensor:
    """(B, 9) fp64 sums per image (dd_depth_metric_sums).  HIP tensors only; enqueues on the current stream and returns at once."""
    if not pred.is_cuda:
        raise RuntimeError("metric_sums runs only on a HIP device (eager_metric_sums is the torch path)")
    p, g = _pair(pred, gt)
    B, H, W = _image_shape(p)
    sums = torch.empty((B, N_SUMS), dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        ws = workspace_for(p, B, H, W)
        _ck(_lib().dd_depth_metric_sums(p.data_ptr(), g.data_ptr(), sums.data_ptr(), ws.data_ptr(), B, H, W, float(t_valid), int(reduce),
                                        _stream(p)), "dd_depth_metric_sums")
    return sums


def metrics_from_sums(sums: torch.Tensor, per_image: bool = False):
    """(1, 8) fp32 metrics over all valid pixels of the batch [and (B, 8) per image] from (B, 9) fp64 sums (dd_depth_metrics)."""
    if not sums.is_cuda:
        return eager_metrics_from_sums(sums, per_image)
    s = sums.detach().double().contiguous().view(-1, N_SUMS)
    B = int(s.shape[0])
    batch = torch.empty((1, 8), dtype=torch.float32, device=s.device)
    image = torch.empty((B, 8), dtype=torch.float32, device=s.device) if per_image else None
    with torch.cuda.device(s.device):
        _ck(_lib().dd_depth_metrics(s.data_ptr(), batch.data_ptr(), image.data_ptr() if per_image else None, B, _stream(s)), "dd_depth_metrics")
    return (batch, image) if per_image else batch


# ---- the eager torch path (tensors that are not on a HIP device) -----------------------------------------------------------------------------
def eager_metric_sums(pred: torch.Tensor, gt: torch.Tensor, t_valid: float = 1e-4) -> torch.Tensor:
    """The same nine sums with torch ops: fp32 per pixel in the reference's order, fp64 accumulation, no gather (``torch.where`` drops what a
    mask would; an invalid pixel contributes an exact 0, whatever it holds)."""
    p, g = _pair(pred, gt)
    B = p.shape[0]
    p, g = p.reshape(B, -1), g.reshape(B, -1)
    valid = g > t_valid
    zero = torch.zeros((), dtype=torch.float32, device=p.device)
    pe, ge = p + 1e-8, g + 1e-8
    pinv = torch.where(p <= t_valid, zero, 1.0 / pe)
    ginv = torch.where(g <= t_valid, zero, 1.0 / ge)
    d = p - g
    ad = d.abs()
    di = pinv - ginv
    ratio = torch.max(g / pe, p / ge)

    def acc(x):
        return torch.where(valid, x, zero).double().sum(dim=1)

    def cnt(m):
        return (valid & m).double().sum(dim=1)

    return torch.stack([valid.double().sum(dim=1), acc(ad), acc(d * d), acc(di.abs()), acc(di * di), acc(ad / ge),
                        cnt(ratio < 1.25), cnt(ratio < 1.25 ** 2), cnt(ratio < 1.25 ** 3)], dim=1)


def _metrics_rows(s: torch.Tensor) -> torch.Tensor:
    den = s[:, 0] + 1e-8
    return torch.stack([(s[:, 2] / den).sqrt(), s[:, 1] / den, (s[:, 4] / den).sqrt(), s[:, 3] / den, s[:, 5] / den,
                        s[:, 6] / den, s[:, 7] / den, s[:, 8] / den], dim=1).float()


def eager_metrics_from_sums(sums: torch.Tensor, per_image: bool = False):
    s = sums.detach().double().reshape(-1, N_SUMS)
    total = s[0:1].clone()
    for b in range(1, s.shape[0]):          # image order, as the kernel adds them
        total = total + s[b:b + 1]
    batch = _metrics_rows(total)
    return (batch, _metrics_rows(s)) if per_image else batch


class Diffusion_DCbase_Metric:
    """``Diffusion_DCbase_Metric(args).evaluate(sample, output, mode)`` -> (1, 8) tensor on the input's device, as the reference's class."""

    def __init__(self, args=None):
        self.args = args
        self.t_valid = 0.0001
        self.metric_name = list(METRIC_NAMES)

    def sums(self, sample, output) -> torch.Tensor:
        """(B, 9) fp64 per-image sums of this batch: what ``MetricAccumulator`` pools exactly."""
        pred, gt = output["pred"], sample["gt"]
        if pred.is_cuda:
            return metric_sums(pred, gt, self.t_valid)
        return eager_metric_sums(pred, gt, self.t_valid)

    def finalize(self, sums: torch.Tensor) -> torch.Tensor:
        """(1, 8) fp32 row over all valid pixels of the batch from its (B, 9) sums."""
        return metrics_from_sums(sums)

    def evaluate(self, sample, output, mode=None) -> torch.Tensor:
        with torch.no_grad():
            return self.finalize(self.sums(sample, output))


class MetricAccumulator:
    """Running evaluation state of one rank, kept on the device:
      * the sum of the per-batch metric rows and the number of batches (their mean is what the reference's summary writer logs), and
      * the nine per-pixel sums over every image of the shard (from which the metrics of the WHOLE set follow exactly, however it was batched
        or sharded).
    ``update`` enqueues and returns the batch's (1, 8) row like ``evaluate``; ``reduce`` all-reduces both through ``dist.reduce_sums``;
    ``result`` is the only call that copies to the host."""

    def __init__(self, metric: Optional[Diffusion_DCbase_Metric] = None):
        self.metric = metric if metric is not None else Diffusion_DCbase_Metric()
        self._state: Optional[torch.Tensor] = None       # fp64 [8 row sums | batch count | 9 pixel sums]
        self._reduced = False

    def update(self, sample, output, mode=None) -> torch.Tensor:
        if self._reduced:
            raise RuntimeError("MetricAccumulator.update after reduce(): start a new accumulator")
        with torch.no_grad():
            sums = self.metric.sums(sample, output)
            row = self.metric.finalize(sums)
            if self._state is None:
                self._state = torch.zeros(8 + 1 + N_SUMS, dtype=torch.float64, device=sums.device)
            self._state[0:8] += row[0].double()
            self._state[8] += 1.0
            self._state[9:] += sums.sum(dim=0)
        return row

    def reduce(self) -> "MetricAccumulator":
        if self._state is None:
            raise RuntimeError("MetricAccumulator.reduce before any update")
        if self._reduced:
            raise RuntimeError("MetricAccumulator.reduce called twice")
        self._state = ddist.reduce_sums(self._state)
        self._reduced = True
        return self

    def result(self) -> dict:
        if self._state is None:
            raise RuntimeError("MetricAccumulator.result before any update")
        s = self._state.cpu()
        batches = float(s[8])
        mean = (s[0:8] / max(batches, 1.0)).float()
        exact = eager_metrics_from_sums(s[9:].reshape(1, N_SUMS))[0]
        return {"names": list(self.metric.metric_name), "batches": int(batches), "n_valid": int(s[9]),
                "batch_mean": mean.numpy(), "exact": exact.numpy(), "sums": s[9:].numpy()}
