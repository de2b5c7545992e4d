"""Inputs and oracle evaluations of the per-ray kernel tests (test_ray_kernels_cpu.py, test_ray_kernels_gpu.py): the loss kernel, the
static loss, the stand-alone compositing and the library Adam at the shapes and values where csrc/nca_kernels_loss.hip branches.

Everything here runs on the CPU.  The high-precision reference is the project's oracle evaluated in f64; the same oracle in f32 is
the noise floor.  Gradients over [R, S] are measured PER RAY (row_err): one ray whose dynamic field is all zero has gradient entries
of ~1e18 (the reference divides by clip(M, 1e-19)), and a whole-tensor max-norm would hide every other ray behind it.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerfca_oracle as O

# ------------------------------------------------------------------------------------------ shapes
# (1, 1); the three residues of R mod 4 with S around the wave width; S around the 512 samples whose q values the loss kernel keeps in
# registers; 1026 blocks (a second trip of the finishing kernel, 17 trips of the dists sum); a second trip of the dists sum at ordinary S
LOSS_SHAPES = [(1, 1), (3, 63), (5, 64), (9, 65), (8, 512), (9, 513), (11, 577), (2, 1100), (4101, 3), (300, 48)]
DISTS_GRAD_SHAPES = [(9, 65), (9, 513), (300, 48), (4101, 3)]
TERM_GRAD_SHAPES = [(9, 65), (9, 513), (11, 577)]      # (at S = 513 the one recomputed sample is the 1e-10 tail: 577 has 65 ordinary ones)
STATIC_SHAPES = [(1, 1), (3, 63), (5, 64), (6, 65), (2, 1100), (4101, 3)]
COMPOSITE_SHAPES = [(1, 1), (3, 63), (5, 64), (6, 65), (2, 200), (1025, 2)]
SKEWS = [1.0, 2.0]            # (a skew below 1 with an exact zero density: the reference's autograd returns NaN, 0 * inf through pow)
SEED = 11

WEIGHTS = (0.7, 0.9, 0.5, 0.25)                                          # favor, dynamic entropy, occlusion, l1 (= l2)
TERM_WEIGHTS = (0.3, 0, 0, 0.7, 1.3, 0.4, 0.9, 0.6, 0.5, 0.25, 2.0)      # every differentiable term of the 11-tuple
MASK_THRE, WEIGHTED_THRESH = 1e-4, 0.03
TERM_NAMES = ["loss", "pixel", "blendw", "sigma_s_max", "sigma_d_max", "favor_s", "s_entropy", "s_entropy_sum", "d_entropy",
              "d_entropy_sum", "d_occl", "s_l1", "s_l2"]

CLASSES = ("ordinary", "zero_dyn_masked", "zero_dyn_weighted", "zero_static", "below_mask", "zero_dyn_samples", "zero_static_samples",
           "weighted", "clipped_dyn")
# the classes whose f32 reference is O(1) from f64 in g_sigma_s: f32 rounds b = vd / (vd + 1e-10) to 1.0 where the static density is 0
ILL_CONDITIONED = ("zero_static", "zero_static_samples")


def ray_dists(S):
    """Interval lengths of linspace(3.4259, 5.5741, S) with the reference's 1e-10 tail, f64.  The depths are f32 values, so their
    differences are exact in f32 as in f64: the f32 oracle sees the same intervals (but for the tail's rounding)."""
    z = torch.linspace(3.4259, 5.5741, S)
    return O.ray_dists(z.double(), torch.float64), z


def loss_args(skew):
    return O.LossArgs(skewness_val=skew, entro_mask_thre=MASK_THRE, entro_use_weighting=True, entro_weighted_thresh=WEIGHTED_THRESH)


def run_args(skew):
    """The same flags as the run_args namespace the library's entry points read."""
    return SimpleNamespace(favor_s_opt=None, skewness_val=skew, entro_mask_thre=MASK_THRE, entro_use_weighting=True,
                           entro_weighted_thresh=WEIGHTED_THRESH, occl_reg_perc=0.2)


@functools.lru_cache(maxsize=None)
def loss_case(R, S, skew, seed=SEED):
    """sig_s, sig_d f32[R, S]; dists, wpix, pix, gt f64; I0 f64[R] (pix = I0 - sum (sig_s + sig_d) dists, what the dists gradient
    differentiates through); cls: one label of CLASSES per ray.  Draws, in this order: rand(R, S) twice, rand(R), randn(R).

    Ordinary rays: sigma = 0.002 + 0.018 rand, so vs / (vs + vd) >= 0.09 and the f32 blend-weight entropy is well conditioned; weights
    in [1, 1.02].  Where R >= 8, rays 1 .. 7 are the classes 1 .. 7 of CLASSES; where R >= 9, ray 8 is clipped_dyn: a weighted ray whose
    dynamic field is scaled by 1e-18, so that 0 < Md < 5e-20 -- BELOW the 1e-19 clip without being 0, the one place where d clip(M) / dM
    = 0 changes a gradient (with Md = 0 every p is 0 and both arms give the same bits).  The zeros of zero_dyn_samples sit at s % 3 == 0 of
    sig_d and those of zero_static_samples at s % 4 == 0 of sig_s, on different rays: no sample has both densities zero (its g_sigma_d
    would be ~1e10 times its neighbours')."""
    gen = torch.Generator().manual_seed(seed + 1000 * R + S)
    sig_s = 0.002 + 0.018 * torch.rand(R, S, generator=gen)
    sig_d = 0.002 + 0.018 * torch.rand(R, S, generator=gen)
    wpix = (1.0 + 0.02 * torch.rand(R, generator=gen)).double()
    gt = torch.randn(R, generator=gen).double()
    cls = ["ordinary"] * R
    if R >= 8:
        cls[1:8] = CLASSES[1:8]
        sig_d[1] = 0.0
        wpix[1] = 1.0
        sig_d[2] = 0.0
        wpix[2] = 1.5
        sig_s[3] = 0.0
        sig_s[4] *= 1e-5
        sig_d[4] *= 1e-5
        sig_d[5, 0::3] = 0.0
        sig_s[6, 0::4] = 0.0
        wpix[7] = 1.5
    if R >= 9:
        cls[8] = CLASSES[8]
        sig_d[8] *= 1e-18
        wpix[8] = 1.5
    dists, _ = ray_dists(S)
    I0 = torch.full((R,), 2.16, dtype=torch.float64)
    pix = I0 - ((sig_s + sig_d).double() * dists).sum(-1)
    return SimpleNamespace(R=R, S=S, skew=skew, sig_s=sig_s, sig_d=sig_d, dists=dists, wpix=wpix, pix=pix, gt=gt, I0=I0, cls=tuple(cls),
                           largs=loss_args(skew), run_args=run_args(skew))


# ------------------------------------------------------------------------------------------ per-ray measures
def row_err(a, b):
    """Per ray: max_s |a - b| / max_s |b|, f64[R].  A ray whose reference is all zero gives 0 where `a` is all zero too, else inf."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    num, den = (a - b).abs().amax(-1), b.abs().amax(-1)
    e = num / den.clamp_min(1e-300)
    return torch.where(den == 0, torch.where(num == 0, torch.zeros_like(e), torch.full_like(e, math.inf)), e)


def rows_pass(got, g32, g64, tol=1e-5):
    """The suite's rule per ray: within `tol` of the f32 oracle, or within max(tol, 3 x the f32 oracle's own distance from the f64 oracle)
    of the f64 oracle.  Returns (ok bool[R], e32, e64, floor, margin = e64 / max(tol, 3 floor))."""
    e32, e64, floor = row_err(got, g32), row_err(got, g64), row_err(g32, g64)
    bound = torch.clamp(3 * floor, min=tol)
    return (e32 < tol) | (e64 < bound), e32, e64, floor, e64 / bound


def class_margins(margin, cls):
    """Worst margin per class present in `cls`."""
    out = {}
    for r, c in enumerate(cls):
        out[c] = max(out.get(c, 0.0), float(margin[r]))
    return out


# ------------------------------------------------------------------------------------------ the oracle on a loss case
def _terms_dict(t, loss, pixel):
    vals = [loss, pixel, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10]]
    return {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in zip(TERM_NAMES, vals)}


@functools.lru_cache(maxsize=None)
def oracle_loss(R, S, skew, dt, unit_mse=False, through_dists=False):
    """The loss assembly of the training step (pixel + favor + dynamic entropy + occlusion + l1 (l2 + l1)) through the oracle in dtype
    `dt`: terms (dict of TERM_NAMES), g_pix f64[R], g_sigma_s / g_sigma_d f64[R, S] and, with through_dists, g_dists f64[S] (pix is
    then a function of dists).  The pixel term is f64 in either case, as in the training script (the ray table is f64)."""
    c = loss_case(R, S, skew)
    a, b = c.sig_s.to(dt).clone().requires_grad_(True), c.sig_d.to(dt).clone().requires_grad_(True)
    do = c.dists.to(dt).clone().requires_grad_(through_dists)
    if through_dists:
        po = c.I0 - ((a.detach() + b.detach()) * do).sum(-1).double()
    else:
        po = c.pix.clone().requires_grad_(True)
    t = O.compute_losses(a, b, do, c.wpix, c.largs)
    wm = torch.ones_like(c.wpix) if unit_mse else c.wpix
    pixel = O.weighted_mse(po, c.gt, wm).mean()
    w = WEIGHTS
    loss = pixel + w[0] * t[3] + w[1] * t[6] + w[2] * t[8] + w[3] * t[10] + w[3] * t[9]
    loss.backward()
    return SimpleNamespace(terms=_terms_dict(t, loss, pixel), g_pix=None if through_dists else po.grad.double(), g_s=a.grad.double(),
                           g_d=b.grad.double(), g_dists=do.grad.double() if through_dists else None)


@functools.lru_cache(maxsize=None)
def oracle_terms(R, S, skew, dt):
    """The 11-tuple weighted by TERM_WEIGHTS through the oracle in dtype `dt`: (values list[11], g_sigma_s, g_sigma_d f64[R, S])."""
    c = loss_case(R, S, skew)
    a, b = c.sig_s.to(dt).clone().requires_grad_(True), c.sig_d.to(dt).clone().requires_grad_(True)
    t = O.compute_losses(a, b, c.dists.to(dt), c.wpix, c.largs)
    sum(w * r for w, r in zip(TERM_WEIGHTS, t) if w).backward()
    return [float(x.detach()) for x in t], a.grad.double(), b.grad.double()


def term_ok(v, v64, v32):
    """The suite's rule for a scalar term; a term whose f64 value is exactly 0 must be 0."""
    if v64 == 0.0:
        return v == 0.0
    return abs(v - v64) <= max(2e-6 * abs(v64), 3 * abs(v32 - v64)) + 1e-12


# ------------------------------------------------------------------------------------------ static loss, closed form
def static_reference(R, S, w_occl=0.37):
    """The static-only loop's loss on the densities of loss_case(R, S, 1.0) in numpy f64, sums exactly rounded (math.fsum over the
    same f64 products the kernel forms): pixel, occl, their bounds count * 2^-53 * sum |term| (the operations are identical, only the
    order of the sum is free), g_pix and the f32 g_sigma row."""
    c = loss_case(R, S, 1.0)
    sig = c.sig_s.numpy()                                 # one field: where R >= 8, a ray and single samples of exact zeros included
    dists, w, pix, gt = c.dists.numpy(), c.wpix.numpy(), c.pix.numpy(), c.gt.numpy()
    inv_R = 1.0 / R
    diff = pix - gt
    pterms = (w * diff) * diff
    oterms = sig.astype(np.float64) * dists[None, :]
    u = 2.0 ** -53
    return SimpleNamespace(sigma=torch.from_numpy(sig), w_occl=w_occl,
                           pixel=math.fsum(pterms.tolist()) * inv_R, pixel_bound=pterms.size * u * float(np.abs(pterms).sum()) * inv_R,
                           occl=math.fsum(oterms.ravel().tolist()) * inv_R, occl_bound=oterms.size * u * float(np.abs(oterms).sum()) * inv_R,
                           g_pix=2.0 * w * diff * inv_R, g_sigma_row=np.float32((w_occl * inv_R) * dists))


# ------------------------------------------------------------------------------------------ compositing
X_CLAMP = math.log(math.e - 1.0)           # softplus(x) = 1: 0.5413...
PLANTED = (20.0, float(np.nextafter(np.float32(20.0), np.float32(21.0))), 25.0, 60.0, -20.0, -104.0, 0.5, 0.6, 5.0, 30.0, -89.0)


@functools.lru_cache(maxsize=None)
def composite_case(R, S, seed=SEED):
    """raw_s, raw_d f32[R, S] = 3 randn with PLANTED at fixed positions from the start of ray 0 (raw_s in order, raw_d reversed) and from
    the end of the last ray (raw_d in order, raw_s reversed), every S // 11 samples so that they spread over the lanes and trips of a
    wave (consecutive where S < 11, running into the neighbouring rays).  planted: (field, ray, sample, x) of every planted value that
    is in the arrays.  dists f64 and the f32 depths z they are the differences of; I0 f32[R]."""
    gen = torch.Generator().manual_seed(seed + 1000 * R + S)
    raw = [3 * torch.randn(R, S, generator=gen), 3 * torch.randn(R, S, generator=gen)]
    n, step = R * S, max(1, S // len(PLANTED))
    where = {}
    for k, x in enumerate(PLANTED):
        xr = PLANTED[len(PLANTED) - 1 - k]
        for f, idx, v in ((0, k * step, x), (1, k * step, xr), (1, n - 1 - k * step, x), (0, n - 1 - k * step, xr)):
            if 0 <= idx < n:
                where[(f, idx)] = v
    for (f, idx), v in where.items():
        raw[f].view(-1)[idx] = v
    planted = tuple((f, idx // S, idx % S, float(raw[f].view(-1)[idx])) for (f, idx) in sorted(where))
    dists, z = ray_dists(S)
    return SimpleNamespace(R=R, S=S, raw_s=raw[0], raw_d=raw[1], planted=planted, dists=dists, z=z, I0=torch.full((R,), 2.15991))


@functools.lru_cache(maxsize=None)
def oracle_composite(R, S, act, single, scale, dt):
    """O.composite / O.composite_single in dtype `dt` with the upstream gradients of the existing compositing test: cp = linspace(-1, 1, R)
    on pix, +3 on sigma_s, -2 on sigma_d.  pix, sigma_s[, sigma_d], g_raw_s[, g_raw_d] in f64, and mag = |I0| + sum |term| per ray."""
    c = composite_case(R, S)
    rs, rd = c.raw_s.to(dt)[..., None].clone().requires_grad_(True), c.raw_d.to(dt)[..., None].clone().requires_grad_(True)
    dirs = torch.zeros(R, 3, dtype=dt)
    cp = torch.linspace(-1, 1, R, dtype=torch.float64).to(dt)
    if single:
        pix, a, dists = O.composite_single(rs, c.I0.to(dt), dirs, c.z.to(dt), act, scale)
        ((pix * cp).sum() + (a * 3).sum()).backward()
        b, mag = None, c.I0.double().abs() + (a.detach().double() * dists.double() * scale).abs().sum(-1)
    else:
        pix, a, b, dists = O.composite(rs, rd, c.I0.to(dt), dirs, c.z.to(dt), act, scale)
        ((pix * cp).sum() + (a * 3).sum() - (b * 2).sum()).backward()
        mag = c.I0.double().abs() + ((a + b).detach().double() * dists.double()).abs().sum(-1)
    return SimpleNamespace(pix=pix.detach().double(), sig_s=a.detach().double(), sig_d=None if single else b.detach().double(),
                           g_s=rs.grad[..., 0].double(), g_d=None if single else rd.grad[..., 0].double(), mag=mag)


# ------------------------------------------------------------------------------------------ Adam + LinearLR, closed form
def adam_lr(done, lr, end_factor, total_iters):
    """LinearLR with start_factor 1 after `done` scheduler steps."""
    return lr * (1.0 + (end_factor - 1.0) * min(done, total_iters) / total_iters)


def adam_updates_f64(grads, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, end_factor=0.1, total_iters=4):
    """torch.optim.Adam's default path + LinearLR in numpy f64 on one flat segment, from the f32 gradients of every step: the list of
    updates p_after - p_before (they do not depend on p) and the lr of every step."""
    m = v = np.zeros(grads[0].shape, dtype=np.float64)
    ups, lrs = [], []
    for it, g in enumerate(grads):
        g = g.astype(np.float64)
        t = it + 1
        m = m + (1.0 - betas[0]) * (g - m)
        v = betas[1] * v + (1.0 - betas[1]) * g * g
        lr_t = adam_lr(it, lr, end_factor, total_iters)
        ups.append(-(lr_t / (1.0 - betas[0] ** t)) * (m / (np.sqrt(v) / math.sqrt(1.0 - betas[1] ** t) + eps)))
        lrs.append(lr_t)
    return ups, lrs


def adam_updates_torch_f32(p0, grads, lr=1e-2, end_factor=0.1, total_iters=4):
    """The same steps through torch.optim.Adam + LinearLR in f32 on the CPU (the noise floor): updates as f64 arrays."""
    p = p0.detach().clone().cpu().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1, end_factor=end_factor, total_iters=total_iters)
    ups = []
    for g in grads:
        before = p.detach().clone()
        p.grad = torch.from_numpy(g).clone()
        opt.step()
        sched.step()
        ups.append((p.detach().double() - before.double()).numpy())
    return ups


def adam_gradients(n, n_steps, seed):
    """randn * 10^(it - 3) per step, f32 numpy; the slice ZERO_SLICE(n) is exactly 0 in every step."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for it in range(n_steps):
        g = torch.randn(n, generator=gen) * (10.0 ** (it - 3))
        g[zero_slice(n)] = 0.0
        out.append(g.numpy())
    return out


def zero_slice(n):
    """100 elements that end 37 before the end of the segment: in the last trip of the kernel's grid-stride loop where there is one."""
    return slice(n - 137, n - 37)
