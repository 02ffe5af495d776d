"""nn.Module mirrors of the reference's hot-path modules with IDENTICAL parameter names and shapes,
so reference checkpoints (state_dict keys depth_head.model.*, depth_head.depth_transform.*) load
unchanged.  The modules hold parameters only; their forward() calls the HIP library.

  ScheduledCNNRefine                 reference src/model/head/ddim_depth_estimate_res.py:300-344
  CNNDDIMPipiline                    reference src/model/head/ddim_depth_estimate_res.py:238-297
  DeepDepthTransformWithUpsampling   reference src/model/ops/depth_transform.py:10-35
"""
from __future__ import annotations

import contextlib
import copy
import os
import weakref
from typing import Optional

import torch
from torch import nn
import torch.nn.functional as F

from .backend import HipDenoiser
from .codec import HipCodecTail
from .scheduler import DDIMScheduler

DEFAULT_PRECISION = os.environ.get("DDEPTH_PRECISION", "fp32")


def _on_hip_device(t) -> bool:
    """Does this tensor take the library?  Tensors on a HIP device: always (the library is their only path).  Anything else runs the modules'
    own torch children in eager mode (BASELINE configs[0]).  One predicate for every dispatch point (the host-emulation tests patch it to
    drive the emulated library with CPU tensors)."""
    return t.is_cuda


def _invalidate_bound_hook(module, incompatible_keys):
    """load_state_dict post-hook (torch asserts that such hooks return None): invalidate the HipBound this module is registered with."""
    bound = module.__dict__.get("_ddepth_bound")
    if bound is not None:
        bound.invalidate()


class HipBound:
    """Shares one HipDenoiser between the modules of a head and re-uploads parameters when any of
    them changed (torch bumps ``Tensor._version`` on every in-place update, e.g. optimizer.step()).

    Staleness is detected from (data_ptr, Tensor._version) of every parameter and buffer.  That signature does NOT see writes that bypass
    the version counter: ``p.data.copy_()`` / ``p.data.mul_()`` / ``weight.data.zero_()`` idioms and raw-pointer updaters (apex
    multi_tensor_applier behind amp O2 and FusedAdam -- the reference trains with apex amp).  Three guards cover them:
      * in .train() mode the denoiser group is re-uploaded in front of EVERY forward (one refresh per iteration, which a training step
        needs anyway; with DDEPTH_DEVICE_WEIGHTS=1 it is ~40 small launches and no host copy) -- no reliance on the counter at all;
      * ``invalidate()`` drops every signature (call it after any out-of-band write in eval mode); ``attach_optimizer(opt)`` registers it
        as a step post-hook; the modules' ``_load_from_state_dict`` calls it too;
      * eval mode without such writes keeps the cheap signature check.

    Parameters are tracked per GROUP of the library (include/ddepth.h: the denoiser "model.*", the codec "depth_transform.*", the
    condition FPN "conv_lateral.* / conv_up.*") and a group travels only when a call that needs it is about to run: a training
    iteration changes every parameter, but in .train() mode only the denoiser runs in the library (codec and FPN use batch-statistics
    BatchNorm in PyTorch), so only that group is refreshed per step -- and with ``DDEPTH_DEVICE_WEIGHTS=1`` without leaving the device
    (HipDenoiser.load_state_dict(device_route=True))."""

    GROUPS = ("model", "codec", "fpn")

    def __init__(self, variant: str = "res"):
        self.variant = variant
        self.backend: Optional[HipDenoiser] = None
        self._modules = []
        self._sig = {}             # group -> signature of what the backend holds
        self._sched_sig = None
        self._hold_depth = 0
        self._held = set()         # groups verified inside the current hold() scope

    @staticmethod
    def _group_of(prefix: str) -> str:
        return "model" if prefix.startswith("model.") else "codec" if prefix.startswith("depth_transform.") else "fpn"

    def register(self, prefix: str, module: nn.Module):
        self._modules.append((prefix, weakref.ref(module)))
        # load_state_dict() copies under no_grad (that does bump the version counter); hooking it anyway costs nothing and also covers
        # custom _load_from_state_dict paths that assign .data.  The hook finds the HipBound THROUGH the module it is called on: a
        # deep-copied head carries copies of the hooks, and those must invalidate the copy's HipBound, not the original's.
        module.__dict__["_ddepth_bound"] = self
        module.register_load_state_dict_post_hook(_invalidate_bound_hook)

    def __deepcopy__(self, memo):
        """copy.deepcopy(head): a fresh HipBound (own library handle, created on first use) tracking the COPIED modules -- the weak
        references of the original would keep pointing at the original's parameters."""
        new = HipBound(self.variant)
        memo[id(self)] = new
        for prefix, ref in self._modules:
            m = ref()
            if m is not None:
                new._modules.append((prefix, weakref.ref(copy.deepcopy(m, memo))))     # memoised: the module of the copied tree
        return new

    def invalidate(self):
        """Forget what the library holds: the next call that needs a group uploads it again.  For updates the version counter cannot
        see (``.data`` writes, apex multi-tensor kernels)."""
        self._sig = {}
        self._held.clear()

    def attach_optimizer(self, optimizer):
        """invalidate() after every optimizer.step() (also fused / multi-tensor optimizers that write through raw pointers)."""
        return optimizer.register_step_post_hook(lambda *_a, **_k: self.invalidate())

    def _any_training(self, group: str) -> bool:
        return any(ref().training for prefix, ref in self._modules if self._group_of(prefix) == group and ref() is not None)

    def _signature(self, group: str):
        """(data_ptr, version) of every parameter and buffer of the group's registered modules, in traversal order.  Walks the modules'
        own ``_parameters`` / ``_buffers`` dicts (what ``state_dict()`` would visit, without building the prefixed OrderedDict)."""
        sig = []
        for prefix, ref in self._modules:
            if self._group_of(prefix) != group:
                continue
            for m in ref().modules():
                for v in m._parameters.values():
                    if v is not None:
                        sig.append((v.data_ptr(), v._version))
                for v in m._buffers.values():
                    if v is not None:
                        sig.append((v.data_ptr(), v._version))
        return tuple(sig)

    @contextlib.contextmanager
    def hold(self):
        """Scope in which the parameters are known not to change (one head.forward): the first ``ensure`` for a group inside it checks /
        uploads as usual, the following ones reuse its verdict instead of re-walking the tensors each time (0.13 ms x 7 library calls per
        forward otherwise -- a fifth of the B=1 head latency).  Re-entrant; leaving the outermost scope drops the verdicts."""
        self._hold_depth += 1
        try:
            yield self
        finally:
            self._hold_depth -= 1
            if self._hold_depth == 0:
                self._held.clear()

    def ensure(self, device, scheduler: Optional[DDIMScheduler] = None, need=GROUPS) -> HipDenoiser:
        """The backend for ``device`` with the parameter groups ``need`` (subset of GROUPS) up to date; registered groups only."""
        want = self._hip_device(device)
        if self.backend is None or self.backend.device != want:
            self.backend = self._make_backend(want)
            self._sig = {}
            self._sched_sig = None
            self._held.clear()
        registered = {self._group_of(p) for p, _ in self._modules}
        for group in need:
            if group not in registered or group in self._held:
                continue
            sig = self._signature(group)
            # .train(): never trust the version counter (see the class docstring); once per hold() scope / per call
            if sig != self._sig.get(group) or self._any_training(group):
                if group == "model":
                    self.check_grad_guard()
                sd = {}
                for prefix, ref in self._modules:
                    if self._group_of(prefix) == group:
                        sd.update({prefix + k: v for k, v in ref().state_dict().items()})
                self.backend.load_state_dict(sd)
                self._sig[group] = sig
            if self._hold_depth > 0:
                self._held.add(group)
        if scheduler is not None:
            ssig = (id(scheduler), scheduler.config.num_train_timesteps)
            if ssig != self._sched_sig:
                self.backend.set_schedule(scheduler._acp_host)
                self._sched_sig = ssig
        return self.backend

    def check_grad_guard(self, wait: bool = False):
        """Raise if a backward of the library returned a non-finite value (``_note_grads``).  Called in front of every refresh of the denoiser's
        parameters (once per training iteration) without blocking: only entries whose event has completed are read; ``wait=True`` (callable by hand
        after ``loss.backward()``) reads them all."""
        be = self.backend
        q = getattr(be, "_grad_guard", None) if be is not None else None
        if not q:
            return
        bad = False
        while q:
            flag, ev = q[0]
            if not wait and ev is not None and len(q) <= 4 and not ev.query():
                break
            q.pop(0)
            bad = bad or not bool(torch.isfinite(flag))
        if bad:
            q.clear()
            raise FloatingPointError("diffusiondepth_amd: a backward pass of the HIP denoiser returned non-finite gradients (NaN / Inf); refusing to continue "
                                     "training on parameters built from them (DDEPTH_GRAD_GUARD=0 disables this check; dd_set_option('check_finite', 2) names "
                                     "the first non-finite tensor)")

    @staticmethod
    def _hip_device(device) -> torch.device:
        """The HIP device (with index) the tensors live on; anything else is an error -- there is no CPU path."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the DDIM hot path runs only on a HIP device (got tensors on {device}); "
                               "diffusiondepth_amd has no CPU fallback")
        return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())

    def _make_backend(self, device) -> HipDenoiser:
        return HipDenoiser(device, self.variant)


class _ConvModule(nn.Module):
    """mmcv ConvModule(norm_cfg=None, act_cfg=None): a biased Conv2d stored under ``.conv`` (key names match)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1)


class UpSample_add(nn.Module):
    """Parameter container of the Swin/MPViT fusion (reference …swin_addHAHI.py:321-333):
    convB(convA(bilinear_up(feat) + noise_embedding)), no norm / activation in between."""

    def __init__(self, skip_input, output_features):
        super().__init__()
        self.convA = _ConvModule(skip_input, output_features)
        self.convB = _ConvModule(output_features, output_features)


def _param_order(variant: str):
    """"model.<name>" in the order the Functions below return gradients."""
    return list(HipDenoiser.PARAM_SHAPES) + (list(HipDenoiser.SWIN_PARAM_SHAPES) if variant == "swin" else [])


def _ordered_params(model: nn.Module):
    named = dict(model.named_parameters())
    return [named[n[len("model."):]] for n in _param_order(model.variant)]


GRAD_GUARD = os.environ.get("DDEPTH_GRAD_GUARD", "1") != "0"


def _note_grads(be, tensors):
    """Always-on guard of the training path (round 6; ADVICE r5 medium: the 16-bit training steps once continued silently on NaN parameters): every
    backward of the library folds the sum of everything it returns -- parameter gradients, grad_x, grad_cond -- into ONE device scalar (asynchronous: a
    handful of reduction kernels) and queues it on the backend with an event recorded behind it.  A NaN / Inf anywhere makes that scalar non-finite.
    ``HipBound.check_grad_guard`` -- called in front of every refresh of the denoiser's parameters, i.e. once per training iteration -- looks only at the
    entries whose event has COMPLETED (no host synchronisation: the host keeps running ahead of the device as before; an entry is read one or two
    iterations after it was made, a queue longer than four entries waits for its oldest) and raises FloatingPointError instead of uploading parameters
    that an optimizer built from non-finite gradients.  DDEPTH_GRAD_GUARD=0 switches it off."""
    if not GRAD_GUARD:
        return
    parts = [t.sum() for t in tensors if t is not None]
    if not parts:
        return
    s = torch.stack(parts).sum()
    ev = None
    if s.is_cuda:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(s.device))
    q = getattr(be, "_grad_guard", None)
    if q is None:
        q = be._grad_guard = []
    q.append((s, ev))


class _DenoiseOnceFn(torch.autograd.Function):
    """autograd node of one epsilon-network call: forward dd_denoise_once, backward dd_denoise_once_backward (what
    loss.backward() sends through ``self.model(...)`` in the reference's training step, …res.py:211, src/main.py:232-241)."""

    @staticmethod
    def forward(ctx, be, precision, x, t, cond, *params):
        ctx.be, ctx.precision = be, precision
        ctx.save_for_backward(x, t, cond)
        out = be.denoise_once(x, t, cond, precision, keep_trajectory=True)          # the backward reads this call's activations
        ctx.ticket = be.last_trajectory_ticket
        return out

    @staticmethod
    def backward(ctx, g):
        x, t, cond = ctx.saved_tensors
        be = ctx.be
        be.zero_grad()
        gx, gc = be.denoise_once_backward(x, t, cond, g.contiguous().float(), ctx.precision,
                                          need_grad_x=ctx.needs_input_grad[2], need_grad_cond=ctx.needs_input_grad[4],
                                          trajectory_ticket=ctx.ticket)
        grads = [be.grad(n) if ctx.needs_input_grad[5 + i] else None for i, n in enumerate(_param_order(be.variant))]
        _note_grads(be, [gx, gc, *grads])
        return (None, None, gx, None, gc, *grads)


class _DenoiseLoopFn(torch.autograd.Function):
    """autograd node of the whole T-step loop: forward dd_denoise (one hipGraph), backward dd_denoise_backward (the reference
    does not detach the loop output: its depth losses back-propagate through all T calls, …res.py:124-169)."""

    @staticmethod
    def forward(ctx, be, precision, T, x_T, cond, *params):
        ctx.be, ctx.precision, ctx.T = be, precision, T
        ctx.save_for_backward(x_T, cond)
        out = be.denoise(x_T, cond, T, precision, keep_trajectory=True)     # the backward reads the states of this very pass
        ctx.ticket = be.last_trajectory_ticket
        return out

    @staticmethod
    def backward(ctx, g):
        x_T, cond = ctx.saved_tensors
        be = ctx.be
        be.zero_grad()
        gx, gc = be.denoise_backward(x_T, cond, g.contiguous().float(), ctx.T, ctx.precision,
                                     need_grad_xT=ctx.needs_input_grad[3], need_grad_cond=ctx.needs_input_grad[4],
                                     trajectory_ticket=ctx.ticket)
        grads = [be.grad(n) if ctx.needs_input_grad[5 + i] else None for i, n in enumerate(_param_order(be.variant))]
        _note_grads(be, [gx, gc, *grads])
        return (None, None, None, gx, gc, *grads)


def _wants_grad(model: nn.Module, *tensors) -> bool:
    """Record an autograd node?  Yes in .train() mode or when an input carries gradient, under enabled grad mode (an .eval()
    module fed plain tensors runs the bare kernels even outside torch.no_grad())."""
    return torch.is_grad_enabled() and (model.training or any(t is not None and t.requires_grad for t in tensors))


class ScheduledCNNRefine(nn.Module):
    """epsilon-network: same constructor and parameter tree as the reference (…res.py:300-322; with
    variant="swin" the tree of …swin_addHAHI.py:336-362, i.e. plus ``upsample_fuse.conv{A,B}.conv``)."""

    def __init__(self, channels_in: int = 256, channels_noise: int = 16, bound: Optional[HipBound] = None,
                 precision: Optional[str] = None, variant: str = "res", **kwargs):
        super().__init__()
        if variant not in ("res", "swin"):
            raise ValueError(f"unknown variant {variant!r}")
        self.variant = variant
        if channels_in != 256 or channels_noise != 16:
            raise ValueError("the HIP kernels are specialised for channels_in=256, channels_noise=16 "
                             "(the only configuration the reference heads build, …res.py:27-37)")
        self.noise_embedding = nn.Sequential(
            nn.Conv2d(channels_noise, 64, kernel_size=3, stride=1, padding=1), nn.GroupNorm(4, 64), nn.ReLU(True),
            nn.Conv2d(64, channels_in, kernel_size=3, stride=1, padding=1), nn.GroupNorm(4, channels_in), nn.ReLU(True))
        if variant == "swin":
            self.upsample_fuse = UpSample_add(channels_in, channels_in)
        self.time_embedding = nn.Embedding(1280, channels_in)
        self.pred = nn.Sequential(
            nn.Conv2d(channels_in, 64, kernel_size=3, stride=1, padding=1), nn.GroupNorm(4, 64), nn.ReLU(True),
            nn.Conv2d(64, channels_noise, kernel_size=3, stride=1, padding=1), nn.GroupNorm(4, channels_noise), nn.ReLU(True))
        self.precision = precision or DEFAULT_PRECISION
        self.bound = bound if bound is not None else HipBound(variant)
        if self.bound.variant != variant:
            raise ValueError("HipBound variant does not match the module variant")
        self.bound.register("model.", self)

    @property
    def single_call_precision(self) -> str:
        """The precision ONE epsilon-network call (this module's forward: the heads' ddim_loss evaluation, …res.py:211) really runs in: ``self.precision``.
        (Until round 5 the Swin / MPViT denoiser in the refined f16 mode fell back to its plain f16 kernels here -- "f16r" existed for it as hoisted plans of
        the T-step loop only.  Since round 6 dd_denoise_once runs the hoisted form for that denoiser as well, with one E[t] border table per image built
        from the call's own timesteps: a "fast" Swin head's `ddim_loss` is an f16r value like its `pred`.)"""
        return self.precision

    def forward(self, noisy_image, t, *args):
        """forward(noisy_image, t, feat, blur_depth, sparse_depth, sparse_mask) -> eps (…res.py:324-344)."""
        feat = args[0]
        if not _on_hip_device(noisy_image):
            return self._eager_forward(noisy_image, t, feat)
        be = self.bound.ensure(noisy_image.device, need=("model",))
        t = torch.as_tensor(t, device=noisy_image.device)
        prec = self.single_call_precision
        if _wants_grad(self, noisy_image, feat):
            tt = t.to(torch.int64).reshape(-1)
            if tt.numel() == 1 and noisy_image.shape[0] > 1:
                tt = tt.expand(noisy_image.shape[0])
            return _DenoiseOnceFn.apply(be, prec, noisy_image.float().contiguous(), tt.contiguous(), feat.float().contiguous(),
                                        *_ordered_params(self))
        return be.denoise_once(noisy_image.float(), t, feat.float(), prec)


def _eager_upsample_add(fuse, x, concat_with):
    """UpSample_add.forward (reference …swin_addHAHI.py:331-333) on the parameter container above."""
    up_x = F.interpolate(x, size=[concat_with.size(2), concat_with.size(3)], mode="bilinear", align_corners=True)
    return fuse.convB.conv(fuse.convA.conv(up_x + concat_with))


def _scheduled_cnn_refine_eager(self, noisy_image, t, feat):
    """The module's own Conv2d / GroupNorm / Embedding children evaluated by PyTorch (reference …res.py:324-344, …swin_addHAHI.py:364-382):
    what runs for tensors that are NOT on a HIP device -- BASELINE.json configs[0], "plumbing, no GPU".  It is the product's own module
    tree in eager mode, never the test oracle, and it is never taken for tensors on a HIP device (there the library is the only path)."""
    t = torch.as_tensor(t, device=noisy_image.device).long()
    feat = feat + self.time_embedding(t)[..., None, None]
    if self.variant == "swin":
        feat = _eager_upsample_add(self.upsample_fuse, feat, self.noise_embedding(noisy_image))
    else:
        feat = feat + self.noise_embedding(noisy_image)
    return self.pred(feat)


ScheduledCNNRefine._eager_forward = _scheduled_cnn_refine_eager


class CNNDDIMPipiline:
    """Same call signature as the reference pipeline (…res.py:248-297).  With eta == 0 the whole
    T-step loop is one dd_denoise call (one hipGraph replay); otherwise it falls back to stepping
    model / scheduler.step on the GPU."""

    def __init__(self, model: ScheduledCNNRefine, scheduler: DDIMScheduler):
        self.model = model
        self.scheduler = scheduler

    def __call__(self, batch_size, device, dtype, shape, input_args, generator=None, eta: float = 0.0,
                 num_inference_steps: int = 50, return_dict: bool = True, x_T=None, **kwargs):
        image_shape = (batch_size, *shape)
        # x_T ~ N(0,1) drawn by the caller-side RNG exactly as the reference does (:277); the library never draws
        image = x_T if x_T is not None else torch.randn(image_shape, generator=generator, device=device, dtype=dtype)
        self.scheduler.set_timesteps(num_inference_steps)
        why_not = self.scheduler.hip_supported(eta)
        if why_not is None and not _on_hip_device(image):
            why_not = "tensors are not on a HIP device: eager PyTorch stepping (model + scheduler.step), as the reference"
        if why_not is None:
            be = self.model.bound.ensure(image.device, self.scheduler, need=("model",))
            if _wants_grad(self.model, image, input_args[0]):
                image = _DenoiseLoopFn.apply(be, self.model.precision, int(num_inference_steps), image.float().contiguous(),
                                             input_args[0].float().contiguous(), *_ordered_params(self.model)).to(dtype)
            else:
                if self.model.variant == "swin" and str(self.model.precision).lower() == "bf16" and not getattr(self.model, "_warned_bf16_inference", False):
                    # bf16 operands are this denoiser's TRAINING precision: its inference depth RMSE is 1.3e-3 at the near range and 7.6e-3 at KITTI's
                    # range with the synthetic weights -- outside the 1e-3 tolerance; the in-tolerance modes are f16r / f16x3 / fp32
                    import warnings
                    warnings.warn("diffusiondepth_amd: precision='bf16' on the Swin / MPViT denoiser is its training precision; for inference it is outside "
                                  "the 1e-3 depth tolerance (use precision='f16r', or 'f16x3' / 'fp32' for the absolute bound)", stacklevel=3)
                    self.model._warned_bf16_inference = True
                image = be.denoise(image.float(), input_args[0].float(), num_inference_steps, self.model.precision).to(dtype)
        else:
            for t in self.scheduler.timesteps:
                model_output = self.model(image, t.to(device), *input_args)
                image = self.scheduler.step(model_output, t, image, eta=eta, use_clipped_model_output=True,
                                            generator=generator)["prev_sample"]
        if not return_dict:
            return (image,)
        return {"images": image}


class CNNDDIMPipilineVis(CNNDDIMPipiline):
    """Pipeline of the reference's *Vis heads (src/model/head/ddim_depth_estimate_res_vis.py:238-301): additionally returns
    ``image_list``, the sample after every step.  eta == 0, no autograd: one dd_denoise_trace call."""

    def __call__(self, batch_size, device, dtype, shape, input_args, generator=None, eta: float = 0.0,
                 num_inference_steps: int = 50, return_dict: bool = True, x_T=None, **kwargs):
        image_shape = (batch_size, *shape)
        image = x_T if x_T is not None else torch.randn(image_shape, generator=generator, device=device, dtype=dtype)
        self.scheduler.set_timesteps(num_inference_steps)
        if self.scheduler.hip_supported(eta) is None and _on_hip_device(image) and not _wants_grad(self.model, image, input_args[0]):
            be = self.model.bound.ensure(image.device, self.scheduler, need=("model",))
            states = be.denoise_trace(image.float(), input_args[0].float(), num_inference_steps, self.model.precision).to(dtype)
            image_list = list(states.unbind(0))
            image = image_list[-1]
        else:
            image_list = []
            for t in self.scheduler.timesteps:
                model_output = self.model(image, t.to(device), *input_args)
                image = self.scheduler.step(model_output, t, image, eta=eta, use_clipped_model_output=True,
                                            generator=generator)["prev_sample"]
                image_list.append(image)
        if not return_dict:
            return (image, image_list)
        return {"images": image, "image_list": image_list}


def _conv_bn_relu(ch_in, ch_out, kernel, stride=1, padding=0, bn=True, relu=True):
    layers = [nn.Conv2d(ch_in, ch_out, kernel, stride, padding, bias=not bn)]
    if bn:
        layers.append(nn.BatchNorm2d(ch_out))
    if relu:
        layers.append(nn.LeakyReLU(0.2, inplace=True))
    return nn.Sequential(*layers)


class DeepDepthTransformWithUpsampling(nn.Module):
    """Latent encoder t() / decoder inv_t() (reference depth_transform.py:10-35).  Eval-mode BatchNorm (running statistics)
    is what the HIP kernels implement; in .train() mode (batch statistics, autograd into the codec weights) the same torch
    modules run in PyTorch-ROCm -- the codec is ~1 GFLOP per image.

    After ``codec.convert_hip_codec`` the last child of ``conv_inv_transform`` is a ``codec.HipCodecTail``, which returns the DEPTH (not the
    sigmoid) for a contiguous fp32 tensor on a HIP device: call ``inv_t``, never ``conv_inv_transform(x)`` directly, on a converted codec."""

    def __init__(self, hidden: int = 16, eps: float = 1e-6, bound: Optional[HipBound] = None):
        super().__init__()
        if hidden != 16 or eps != 1e-6:
            raise ValueError("HIP codec kernels are specialised for hidden=16, eps=1e-6 (…res.py:23)")
        self.conv_transform = nn.Sequential(_conv_bn_relu(1, hidden, 3, 2, 1), _conv_bn_relu(hidden, hidden, 3, 1, 1, relu=False),
                                            nn.Tanh())
        self.conv_inv_transform = nn.Sequential(
            nn.ConvTranspose2d(hidden, hidden, kernel_size=4, stride=2, padding=1), nn.BatchNorm2d(hidden), nn.ReLU(inplace=True),
            _conv_bn_relu(hidden, 1, 3, 1, 1, bn=False, relu=False), nn.Sigmoid())
        self.eps = eps
        self.bound = bound if bound is not None else HipBound("res")
        self.bound.register("depth_transform.", self)

    def _torch_path(self, x) -> bool:
        # (tensors that are not on a HIP device: the same torch modules in eager mode -- BASELINE configs[0], "plumbing, no GPU")
        return self.training or (torch.is_grad_enabled() and x.requires_grad) or not _on_hip_device(x)

    def t(self, depth):
        if self._torch_path(depth):
            return self.conv_transform(depth)                                        # depth_transform.py:29-31
        return self.bound.ensure(depth.device, need=("codec",)).encode(depth.float())

    def inv_t(self, value):
        if self._torch_path(value):
            tail = self.conv_inv_transform[-1]
            if isinstance(tail, HipCodecTail):                                       # (codec.convert_hip_codec)
                z = value
                for layer in list(self.conv_inv_transform)[:-1]:
                    z = layer(z)
                if tail.returns_depth(z):                                            # decided before the call: the fused tail IS the depth
                    return tail(z)
                return 1.0 / tail(z).clamp(self.eps) - 1
            return 1.0 / self.conv_inv_transform(value).clamp(self.eps) - 1          # depth_transform.py:33-35
        return self.bound.ensure(value.device, need=("codec",)).decode(value.float())
