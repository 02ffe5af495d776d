"""The cases of the shifted-window attention backward (include/train/ddepth_swin_backward.h), shared by tests/test_swin_backward_host_emulation.py
(the kernel's source on the CPU) and tests/test_zz_gpu_swin_backward.py (the built library).  Shapes, ``slot_map``, ``gather``, ``permutation`` and
``real_inputs`` are those of tests/swin_cases.py.  The checks take a callable

    run(qkv, qkv_pad, rel_bias, grad_out, heads, shift, prec, scale=None, want_pad=True, want_bias=True, poison=False)
        -> (grad_qkv [B, H, W, 3 C], grad_qkv_pad [3 C] or None, grad_rel_bias [heads, 49, 49] or None)       fp32 numpy

``scale``: None or the four floats {s, 1 / s, bits of amax, 0} of dd_conv_grad_scale; ``poison``: fill the workspace with NaN before the call.

Oracle: ``attend_indexed`` restates swin_cases.attend as differentiable torch index arithmetic (advanced indexing into the token list plus one
pad row; no pad / roll / partition op); its fp64 forward equals swin_cases.attend to 1e-12 and its gradients come from torch.autograd.grad.
Baselines: fp32 mode -- autograd through diffusiondepth_amd.swin.window_attention_torch in fp32; bf16 / f16 -- ``formulas``: the header's
formulas written out in fp32 with the six roundings.
Bound, per output tensor: err <= 4 x max(the baseline's own error against the oracle, 1e-6 max(1, max |oracle tensor|)) -- the project's 4 x
rule; the floor is scaled because grad_rel_bias and grad_qkv_pad sum hundreds of terms."""
import functools

import numpy as np
import torch

import swin_cases as SC
from swin_cases import HD, N, SHAPES, WINDOW, gather, permutation, real_inputs, slot_map      # noqa: F401  (the shared vocabulary)

KSCALE = np.float32(0.17677669529663687)      # 32^-0.5 as the kernels hold it
OUTPUTS = ("grad_qkv", "grad_qkv_pad", "grad_rel_bias")


# ---- index arithmetic ---------------------------------------------------------------------------------------------------------------------------
def token_index(H, W, shift):
    """-> idx [nwy, nwx, 49]: the flat token y * W + x of every slot, H * W for a padded position; inv [H * W]: the flat (window, slot) of every
    token (each token is the slot of exactly one window)."""
    y, x, inside, _ = slot_map(H, W, shift)
    idx = np.where(inside, y * W + x, H * W)
    inv = np.full(H * W, -1, dtype=np.int64)
    inv[idx[inside]] = np.arange(idx.size).reshape(idx.shape)[inside]
    assert (inv >= 0).all()
    return idx, inv


def _windows(t, idx, pad_row):
    """t [B, H * W, K] -> [B, nwy, nwx, 49, K] with ``pad_row`` [K] at the padded positions."""
    B, _, K = t.shape
    return torch.cat([t, pad_row.view(1, 1, K).expand(B, 1, K)], dim=1)[:, torch.from_numpy(idx)]


def _mask(H, W, shift, dtype):
    _, _, _, label = slot_map(H, W, shift)
    lab = torch.from_numpy(label)
    return torch.where(lab[:, :, :, None] != lab[:, :, None, :], -100.0, 0.0).to(dtype)[None, :, :, None]      # [1, nwy, nwx, 1, 49, 49]


def attend_indexed(qkv, pad, bias, heads, shift):
    """Differentiable: torch tensors qkv [B, H, W, 3 C], pad [3 C], bias [heads, 49, 49] of one dtype -> out [B, H, W, C]."""
    B, H, W, K = qkv.shape
    C = K // 3
    idx, inv = token_index(H, W, shift)
    win = _windows(qkv.reshape(B, H * W, K), idx, pad)
    win = win.view(B, *idx.shape[:2], N, 3, heads, HD).permute(4, 0, 1, 2, 5, 3, 6)      # [3, B, nwy, nwx, heads, 49, 32]
    s = (win[0] * (HD ** -0.5)) @ win[1].transpose(-1, -2) + bias
    if shift:
        s = s + _mask(H, W, shift, qkv.dtype)
    o = torch.softmax(s, dim=-1) @ win[2]
    o = o.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, C)
    return o[:, torch.from_numpy(inv)].view(B, H, W, C)


def oracle_grads(qkv, pad, bias, gout, heads, shift):
    """fp64 autograd through attend_indexed -> (grad_qkv, grad_qkv_pad, grad_rel_bias) as fp64 numpy.  pad None: zeros (its gradient exists)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True)
    q, p, b = t(qkv), t(np.zeros(qkv.shape[-1]) if pad is None else pad), t(bias)
    out = attend_indexed(q, p, b, heads, shift)
    ref = SC.attend(qkv, pad, bias, heads, shift)
    assert np.abs(out.detach().numpy() - ref).max() <= 1e-12, "the differentiable restatement is not swin_cases.attend"
    return tuple(g.numpy() for g in torch.autograd.grad(out, (q, p, b), torch.tensor(gout, dtype=torch.float64)))


def formulas(qkv, pad, bias, gout, heads, shift, round_to=None, dtype=torch.float32):
    """The header's formulas, no autograd: every sum in ``dtype``; ``round_to`` rounds scale q, k, v, P (for dV), dO and dS (for dQ, dK) once."""
    B, H, W, K = qkv.shape
    C = K // 3
    idx, inv = token_index(H, W, shift)
    rnd = (lambda a: a.to(round_to).to(dtype)) if round_to is not None else (lambda a: a)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    prow = t(np.zeros(K) if pad is None else pad)
    heads_of = lambda w, k: w.view(B, *idx.shape[:2], N, k, heads, HD).permute(4, 0, 1, 2, 5, 3, 6)
    win = heads_of(_windows(t(qkv).reshape(B, H * W, K), idx, prow), 3)
    dO = rnd(heads_of(_windows(t(gout).reshape(B, H * W, C), idx, torch.zeros(C, dtype=dtype)), 1)[0])
    qs, k, v = rnd(win[0] * float(KSCALE) if dtype == torch.float64 else win[0] * torch.tensor(KSCALE)), rnd(win[1]), rnd(win[2])
    s = qs @ k.transpose(-1, -2) + t(bias)
    if shift:
        s = s + _mask(H, W, shift, dtype)
    P = torch.softmax(s, dim=-1)
    dP = dO @ v.transpose(-1, -2)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dV = rnd(P).transpose(-1, -2) @ dO
    dK = rnd(dS).transpose(-1, -2) @ qs
    dQ = (rnd(dS) @ k) * (float(KSCALE) if dtype == torch.float64 else torch.tensor(KSCALE))
    g = torch.stack([dQ, dK, dV], dim=0).permute(1, 2, 3, 5, 0, 4, 6).reshape(B, -1, K)      # [B, (nwy nwx 49), 3 C]
    flat_idx = torch.from_numpy(idx.reshape(-1))
    grad_pad = g[:, flat_idx == H * W].sum(dim=(0, 1))
    return g[:, torch.from_numpy(inv)].view(B, H, W, K).numpy(), grad_pad.numpy(), dS.sum(dim=(0, 1, 2)).numpy()


def torch_fp32(qkv, pad, bias, gout, heads, shift):
    """Autograd through the torch composition in fp32: the fp32 mode's baseline."""
    from diffusiondepth_amd import swin as SW
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, requires_grad=True)
    q, p, b = t(qkv), t(np.zeros(qkv.shape[-1]) if pad is None else pad), t(bias)
    out = SW.window_attention_torch(q, p, b, heads, WINDOW, shift)
    gq, gp, gb = torch.autograd.grad(out, (q, p, b), torch.tensor(gout), allow_unused=True)
    return gq.numpy(), (torch.zeros_like(p) if gp is None else gp).numpy(), gb.numpy()


# ---- real-valued cases ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_out(name, shift, seed=0):
    B, H, W, heads = SHAPES[name]
    g = torch.Generator().manual_seed(4242 + 100 * list(SHAPES).index(name) + 10 * shift + seed)
    a = torch.randn(B, H, W, heads * HD, generator=g).numpy()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def real_oracle(name, shift, bias_scale):
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    return oracle_grads(qkv, pad, bias, grad_out(name, shift), SHAPES[name][3], shift)


@functools.lru_cache(maxsize=None)
def real_baseline(name, shift, bias_scale, prec):
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    a = (qkv, pad, bias, grad_out(name, shift), SHAPES[name][3], shift)
    return torch_fp32(*a) if prec == "fp32" else formulas(*a, round_to=SC.ROUND[prec])


def errors(got, base, oracle):
    """-> [(output name, library error, baseline error, bound)]"""
    rows = []
    for name, g, b, o in zip(OUTPUTS, got, base, oracle):
        err = float(np.abs(g.astype(np.float64) - o).max())
        base_err = float(np.abs(b.astype(np.float64) - o).max())
        rows.append((name, err, base_err, 4.0 * max(base_err, 1e-6 * max(1.0, float(np.abs(o).max())))))
    return rows


def check_real(run, name, shift, prec, bias_scale, record=None, where=""):
    qkv, pad, bias = real_inputs(name, shift, bias_scale)
    got = run(qkv, pad, bias, grad_out(name, shift), SHAPES[name][3], shift, prec)
    rows = errors(got, real_baseline(name, shift, bias_scale, prec), real_oracle(name, shift, bias_scale))
    for out, err, base_err, bound in rows:
        print(f"{where} {name} shift {shift} {prec} bias x{bias_scale:g} {out}: library {err:.3e} baseline {base_err:.3e} bound {bound:.3e}")
        if record is not None:
            record("swin_window_attention_backward", where=where, shape=name, shift=shift, precision=prec, bias_scale=bias_scale, output=out, err=err,
                   baseline_err=base_err)
    for g in got:
        assert np.isfinite(g).all()
    for out, err, base_err, bound in rows:
        assert err <= bound, (name, shift, prec, bias_scale, out, err, base_err)


# ---- exact family E1: one-hot probabilities -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_grad_out(name, shift):
    """Integers with 1 <= |g| <= 15."""
    B, H, W, heads = SHAPES[name]
    g = torch.Generator().manual_seed(99 + list(SHAPES).index(name) + 10 * shift)
    shape = (B, H, W, heads * HD)
    a = (torch.randint(1, 16, shape, generator=g).float() * (2 * torch.randint(0, 2, shape, generator=g) - 1)).numpy()
    a.setflags(write=False)
    return a


def check_onehot(run, name, shift, prec, kind):
    """exact_inputs: P is one-hot at pi_h, so grad_v at slot j is grad_out at slot pi_h^-1(j) (0 where that slot is padded: a padded query has no
    grad_out) and the v part of grad_qkv_pad is an integer sum.  Without a shift grad_q, grad_k and grad_rel_bias are exactly +-0; with one the
    exp(-100) of a masked selection is a denormal, not 0: those three stay below 1e-30 and a grad_v that should be 0 does too."""
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    qkv, pad, bias = SC.exact_inputs(name, shift, kind)
    gout = int_grad_out(name, shift)
    gq, gp, gb = run(qkv, pad, bias, gout, heads, shift, prec)
    idx, inv = token_index(H, W, shift)
    dO = np.concatenate([gout.reshape(B, H * W, C), np.zeros((B, 1, C), dtype=np.float32)], axis=1)[:, idx]      # [B, nwy, nwx, 49, C]
    dV = np.empty_like(dO)
    for h in range(heads):
        inverse = np.argsort(permutation(kind, h))
        dV[..., h * HD:(h + 1) * HD] = dO[:, :, :, inverse, h * HD:(h + 1) * HD]
    want_v = dV.reshape(B, -1, C)[:, inv].reshape(B, H, W, C)
    want_pad_v = dV.reshape(B, -1, C)[:, idx.reshape(-1) == H * W].sum(axis=(0, 1))
    for got, want in ((gq[..., 2 * C:], want_v), (gp[2 * C:], want_pad_v)):
        if shift == 0:
            assert np.array_equal(got, want), f"{name} {prec} {kind}: grad_v differs"
        else:
            nz = want != 0
            assert np.array_equal(got[nz], want[nz]) and (np.abs(got[~nz]) <= 1e-30).all(), f"{name} shift {shift} {prec} {kind}: grad_v differs"
    tiny = 0.0 if shift == 0 else 1e-30
    for what, a in (("grad_q, grad_k", gq[..., :2 * C]), ("grad_qkv_pad q, k", gp[:2 * C]), ("grad_rel_bias", gb)):
        assert (np.abs(a) <= tiny).all(), f"{name} shift {shift} {prec} {kind}: {what} up to {np.abs(a).max()}"


# ---- exact family E2: probabilities of exactly 1/2, 1/2 (shift 0) -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def half_inputs(name):
    """q = 0; bias 0 at pi_h(i) and pi'_h(i) = (pi_h(i) + 1) mod 49, -200 elsewhere; v in {-2..2}; k in {+-1, +-2}; grad_out +-1 at one d per token
    and head.  dS is a multiple of 1/4 then: exact in bf16 and f16."""
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    g = torch.Generator().manual_seed(555 + list(SHAPES).index(name))
    k = torch.randint(1, 3, (B, H, W, C), generator=g).float() * (2 * torch.randint(0, 2, (B, H, W, C), generator=g) - 1)
    v = torch.randint(-2, 3, (B, H, W, C), generator=g).float()
    qkv = torch.cat([torch.zeros(B, H, W, C), k, v], dim=-1).numpy()
    d = torch.randint(0, HD, (B, H, W, heads), generator=g)
    sign = (2 * torch.randint(0, 2, (B, H, W, heads), generator=g) - 1).float()
    gout = torch.zeros(B, H, W, heads, HD).scatter_(-1, d.unsqueeze(-1), sign.unsqueeze(-1)).reshape(B, H, W, C).numpy()
    bias = np.full((heads, N, N), -200.0, dtype=np.float32)
    for h in range(heads):
        p = permutation("permutation", h)
        bias[h, np.arange(N), p] = 0.0
        bias[h, np.arange(N), (p + 1) % N] = 0.0
    for a in (qkv, gout, bias):
        a.setflags(write=False)
    return qkv, gout, bias


def check_halves(run, name, prec):
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    qkv, gout, bias = half_inputs(name)
    gq, gp, gb = run(qkv, None, bias, gout, heads, 0, prec)
    # every quantity below is a small dyadic rational: fp64 index arithmetic is exact
    idx, inv = token_index(H, W, 0)
    pad0 = lambda a: np.concatenate([a.reshape(B, H * W, -1).astype(np.float64), np.zeros((B, 1, a.shape[-1]))], axis=1)[:, idx]
    split = lambda w: w.reshape(*w.shape[:4], heads, HD).transpose(0, 1, 2, 4, 3, 5)      # [B, nwy, nwx, heads, 49, 32]
    k, v, dO = split(pad0(qkv[..., C:2 * C])), split(pad0(qkv[..., 2 * C:])), split(pad0(gout))
    P = np.where(bias == 0.0, 0.5, 0.0)[None, None, None]
    dP = dO @ np.swapaxes(v, -1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    assert np.array_equal(dS * 4, np.round(dS * 4))
    merge = lambda a: a.transpose(0, 1, 2, 4, 3, 5).reshape(B, -1, C)[:, inv].reshape(B, H, W, C)
    want_q = KSCALE * merge(dS @ k).astype(np.float32)      # float32(scale) times the exact sum: one rounding
    want_v = merge(np.swapaxes(P, -1, -2) @ dO).astype(np.float32)
    want_b = dS.sum(axis=(0, 1, 2)).astype(np.float32)
    assert np.array_equal(SC.bits(gb + 0.0), SC.bits(want_b + 0.0)), f"{name} {prec}: grad_rel_bias differs"
    assert np.array_equal(gq[..., :C], want_q), f"{name} {prec}: grad_q is not float32(scale) x the exact sum"
    assert np.array_equal(gq[..., 2 * C:], want_v), f"{name} {prec}: grad_v differs"


# ---- identities -------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    for name, x, y in zip(OUTPUTS, a, b):
        assert np.array_equal(SC.bits(x), SC.bits(y)), f"{what}: {name} differs"


def check_identities(run, prec, shift=3, name="ragged"):
    """Two calls, a B = 1 call per image, a NaN-filled workspace and NULL outputs: bit-equal."""
    qkv, pad, bias = real_inputs(name, shift, 1.0)
    heads = SHAPES[name][3]
    gout = grad_out(name, shift)
    both = run(qkv, pad, bias, gout, heads, shift, prec)
    _same(both, run(qkv, pad, bias, gout, heads, shift, prec), "two calls")
    _same(both, run(qkv, pad, bias, gout, heads, shift, prec, poison=True), "a workspace full of NaN")
    for b in range(qkv.shape[0]):
        one = run(np.ascontiguousarray(qkv[b:b + 1]), pad, bias, np.ascontiguousarray(gout[b:b + 1]), heads, shift, prec)
        assert np.array_equal(SC.bits(one[0][0]), SC.bits(both[0][b])), f"image {b} of the batched call differs from the single call"
    lone = run(qkv, pad, bias, gout, heads, shift, prec, want_pad=False, want_bias=False)
    assert lone[1] is None and lone[2] is None and np.array_equal(SC.bits(lone[0]), SC.bits(both[0])), "NULL outputs change grad_qkv"


def check_nan(run, prec, shift=3, name="ragged"):
    """NaN in one token's grad_out, all 32 values of one head: grad_qkv outside that (window, head) is bit-identical to the clean run, its v part inside is NaN."""
    qkv, pad, bias = real_inputs(name, shift, 1.0)
    B, H, W, heads = SHAPES[name]
    C = heads * HD
    gout = grad_out(name, shift)
    clean = run(qkv, pad, bias, gout, heads, shift, prec)[0]
    a = SC.NAN_AT
    dirty = gout.copy()
    dirty[a["b"], a["y"], a["x"], a["head"] * HD:(a["head"] + 1) * HD] = np.nan      # (the token's whole head slice: every d of grad_v sees it)
    got = run(qkv, pad, bias, dirty, heads, shift, prec)[0]
    y, x, inside, _ = slot_map(H, W, shift)
    wy, wx = np.argwhere(((y == a["y"]) & (x == a["x"])).any(axis=-1))[0]
    touched = np.zeros((B, H, W, 3, C), dtype=bool)
    m = inside[wy, wx]
    touched[a["b"], y[wy, wx][m], x[wy, wx][m], :, a["head"] * HD:(a["head"] + 1) * HD] = True
    touched = touched.reshape(B, H, W, 3 * C)
    v_part = touched.copy()
    v_part[..., :2 * C] = False
    assert np.isnan(got[v_part]).all(), "the NaN did not reach every grad_v of its window and head"
    assert np.array_equal(SC.bits(got)[~touched], SC.bits(clean)[~touched]), "the NaN left its window or head"


def grad_scale(gout):
    """The rule of include/ddepth_conv_scaled.h for f16: s = 2^(14 - floor(log2 amax)) over the finite elements -> the four floats of the buffer."""
    amax = np.float32(np.abs(gout[np.isfinite(gout)]).max())
    e = int(np.floor(np.log2(float(amax)))) if amax > 0 else 14
    s = np.float32(2.0) ** np.float32(np.clip(14 - e, -126, 126))
    return np.array([s, np.float32(1.0) / s, amax.view(np.float32), 0.0], dtype=np.float32)


SCALE_EXPONENTS = (-24, -12, 0, 8, 16)


def check_f16_scale(run, shift=3, name="ragged"):
    """f16 with ``scale``: grad_out 2^k gives exactly 2^k x the results; the scaled run at k = -24 stays inside the bound (the unscaled one is
    printed beside it: f16 flushes most of such a grad_out)."""
    qkv, pad, bias = real_inputs(name, shift, 1.0)
    heads = SHAPES[name][3]
    gout = grad_out(name, shift)
    ref = run(qkv, pad, bias, gout, heads, shift, "f16", scale=grad_scale(gout))
    oracle, base = real_oracle(name, shift, 1.0), real_baseline(name, shift, 1.0, "f16")
    for k in SCALE_EXPONENTS:
        g = (gout * np.float32(2.0 ** k)).astype(np.float32)
        got = run(qkv, pad, bias, g, heads, shift, "f16", scale=grad_scale(g))
        for out, x, r in zip(OUTPUTS, got, ref):
            assert np.array_equal(x, r * np.float32(2.0 ** k)), f"k = {k}: {out} is not 2^k x the k = 0 result"
        if k == SCALE_EXPONENTS[0]:
            plain = run(qkv, pad, bias, g, heads, shift, "f16")
            unscale = lambda t: tuple(x.astype(np.float64) * 2.0 ** -k for x in t)
            for (out, err, base_err, bound), (_, perr, _, _) in zip(errors(unscale(got), base, oracle), errors(unscale(plain), base, oracle)):
                print(f"f16 grad_out x 2^{k} {out}: scaled {err:.3e} unscaled {perr:.3e} baseline {base_err:.3e} bound {bound:.3e}")
                assert err <= bound, (k, out, err, bound)
