"""Cone-beam projection of voxel volumes on the device (csrc/view/nca_drr.hip): digitally reconstructed radiographs.

The reference makes its training projections from a CT or phantom volume with TIGRE (preprocess/datatoray.py,
tigre_helpers.py: ``tigre.Ax``), a CUDA library; here the same step is ``nca_drr_project``: line integrals of a trilinearly
interpolated f32 grid along the rays ``nca_view_rays`` generates, by the renderer's own quadrature
``pix = I0 - sum_s sigma(o + d z_s) dists_s``.  Two uses:

* coming in: ``volume_teacher`` is a ``render=`` hook of ``synthetic.make_dataset``, so a dataset can be made from a volume pair
  instead of a teacher network pair;
* going out: ``project_sequence`` / ``project_view`` reproject the grids ``export.density_volumes`` writes through the C-arm geometry,
  with the keys and shapes of ``export.render_sequence`` / ``render_view``.

A grid is ``export.density_volume``'s: ``linspace(lo, hi, n)`` nodes per axis, the volume ``[n0, n1, n2]`` with the last axis fastest;
outside the grid the volume is 0.  There is no torch implementation behind these functions.

``project_rays`` is differentiable in ``volumes`` (``nca_drr_backproject``, the adjoint kernel), and ``fit_volumes`` descends on a
static volume and a stack of phase volumes until their projections match measured frames: the iterative voxel reconstruction a field
is compared with, and the check of an exported grid against images.  ``total_variation`` (csrc/view/nca_voltv.hip) is the prior such a
reconstruction carries when the views are few: the smoothed total variation of the volumes in space and between neighbouring heart phases,
differentiable in the volumes; ``fit_volumes`` adds it to the data term with ``tv_space`` / ``tv_time``, and a structural term
(``metrics.ssim``) with ``ssim_weight``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _capi
from . import _view
from . import export as _export
from . import fused as _fused
from . import metrics as _metrics

Bounds = Tuple[Tuple[float, float], ...]
UNIT_BOUNDS: Bounds = ((-1.0, 1.0),) * 3


grid_desc = _capi.grid_desc          # the public name; the leaf module has it so that metrics and phantom need not import this one


def _default_dists(z: torch.Tensor) -> torch.Tensor:
    from .train.model_helpers import _interval_lengths
    return _interval_lengths(z, torch.empty(0, dtype=torch.float64, device=z.device))


def _launch_project(volumes, o, d, z, dists, i0, desc):
    """pix f64 [n_vol,R]: one nca_drr_project of checked, contiguous operands."""
    n_vol = 1 if volumes.dim() == 3 else volumes.shape[0]
    R, S = o.shape[0], z.shape[0]
    pix = torch.empty((n_vol, R), dtype=torch.float64, device=volumes.device)
    _view.launch(_capi.check_drr, _capi.lib().nca_drr_project, volumes.device, C.byref(desc), _capi.ptr(volumes), n_vol, R, S, _capi.ptr(o), _capi.ptr(d),
                 _capi.ptr(z), _capi.ptr(dists), float(i0), _capi.ptr(pix))
    return pix


class _ProjectRays(torch.autograd.Function):
    """``project_rays`` with a gradient in ``volumes``: the forward is the same launch, the backward is ``nca_drr_backproject`` into a
    zeroed f64 buffer, returned as f32 in the volumes' shape.  Rays, depths, interval lengths and ``i0`` get no gradient."""

    @staticmethod
    def forward(ctx, volumes, o, d, z, dists, i0, desc):
        ctx.save_for_backward(o, d, z, dists)
        ctx.desc, ctx.shape = desc, volumes.shape
        return _launch_project(volumes.detach(), o, d, z, dists, i0, desc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pix):
        o, d, z, dists = ctx.saved_tensors
        shape = ctx.shape
        dev = o.device
        if g_pix.device != dev:
            raise _capi.NcaError(f"project_rays backward: the pixel gradient lives on {g_pix.device}, the volumes on {dev}")
        n_vol = 1 if len(shape) == 3 else shape[0]
        R, S = o.shape[0], z.shape[0]
        g_pix = g_pix.to(torch.float64).contiguous().view(n_vol, R)
        g_vol = torch.zeros((n_vol, math.prod(shape[-3:])), dtype=torch.float64, device=dev)
        _view.launch(_capi.check_drr, _capi.lib().nca_drr_backproject, dev, C.byref(ctx.desc), n_vol, R, S, _capi.ptr(o), _capi.ptr(d), _capi.ptr(z),
                     _capi.ptr(dists), _capi.ptr(g_pix), _capi.ptr(g_vol))
        return g_vol.to(torch.float32).reshape(shape), None, None, None, None, None, None


def project_rays(volumes: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, z: torch.Tensor, dists: Optional[torch.Tensor] = None, *,
                 i0: float, bounds: Bounds) -> torch.Tensor:
    """``i0 - sum_s volume(o + d z_s) dists_s`` of f32 ``volumes`` ``[n0,n1,n2]`` (returns f64 ``[R]``) or ``[n_vol,n0,n1,n2]``
    (returns f64 ``[n_vol,R]``; the volumes share one grid and are marched in one pass) along the rays ``origins`` / ``dirs``
    ``[R,3]`` (f64, or f32 widened) at the depths ``z`` ``[S]`` shared by all rays.  ``dists`` ``[S]`` defaults to
    ``model_helpers._interval_lengths(z)``.  ``bounds`` places the grid (``grid_desc``).

    With grad mode on and ``volumes.requires_grad`` the result carries a gradient in ``volumes`` (f32, the volumes' shape; the adjoint
    kernel sums in f64 atomics, so its last bits can differ from run to run).  Rays, ``z``, ``dists`` and ``i0`` get no gradient.  In
    every other case nothing is recorded and the result is the plain launch's."""
    if torch.is_grad_enabled() and isinstance(volumes, torch.Tensor) and volumes.requires_grad:
        return _project_rays(volumes, origins, dirs, z, dists, i0, bounds, True)
    with torch.no_grad():
        return _project_rays(volumes, origins, dirs, z, dists, i0, bounds, False)


def _project_rays(volumes, origins, dirs, z, dists, i0, bounds, differentiable):
    for t, what in ((volumes, "volumes"), (origins, "ray origins"), (dirs, "ray directions"), (z, "depth values")):
        _fused._require_cuda(t, what)
    dev = volumes.device
    if dists is not None:
        _fused._require_cuda(dists, "interval lengths")
    if any(t.device != dev for t in (origins, dirs, z) + (() if dists is None else (dists,))):
        raise _capi.NcaError("project_rays: volumes, rays, depths and interval lengths must live on one device")
    _view.check_contiguous_volumes(volumes, "project_rays")
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape != dirs.shape or origins.shape[0] == 0:
        raise _capi.NcaError(f"project_rays takes ray origins and directions [R,3], got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    if any(t.dtype not in (torch.float32, torch.float64) for t in (origins, dirs)):
        raise _capi.NcaError("rays are float32 or float64")
    if z.dim() != 1 or z.shape[0] == 0:
        raise _capi.NcaError("project_rays takes ONE depth vector [S] shared by all rays")
    z = z.detach().to(torch.float32).contiguous()
    dists = _default_dists(z) if dists is None else dists.detach()
    if dists.shape != z.shape:
        raise _capi.NcaError(f"interval lengths {tuple(dists.shape)} do not match the depth vector {tuple(z.shape)}")
    dists = dists.to(torch.float64).contiguous()
    o = origins.detach().to(torch.float64).contiguous()
    d = dirs.detach().to(torch.float64).contiguous()
    desc = grid_desc(volumes.shape[-3:], bounds)
    pix = _ProjectRays.apply(volumes, o, d, z, dists, float(i0), desc) if differentiable else _launch_project(volumes, o, d, z, dists, i0, desc)
    return pix[0] if volumes.dim() == 3 else pix


class _TotalVariation(torch.autograd.Function):
    """``total_variation`` with a gradient in ``volumes``: the forward is one ``nca_vol_tv``, the backward one ``nca_vol_tv_grad`` whose device
    ``scale`` holds the two upstream gradients times the normalisations -- nothing is read back."""

    @staticmethod
    def forward(ctx, volumes, desc, eps_space, eps_time, cyclic):
        ctx.save_for_backward(volumes)
        ctx.args = (desc, eps_space, eps_time, cyclic)
        return _launch_tv(volumes.detach(), desc, eps_space, eps_time, cyclic)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_space, g_time):
        (volumes,) = ctx.saved_tensors
        desc, eps_space, eps_time, cyclic = ctx.args
        dev = volumes.device
        if g_space.device != dev or g_time.device != dev:
            raise _capi.NcaError(f"total_variation backward: the upstream gradients live on {g_space.device} and {g_time.device}, the volumes on {dev}")
        n_vol, voxels, n_pairs = _tv_counts(volumes, cyclic)
        scale = torch.stack([g_space.to(torch.float64).reshape(()) / float(n_vol * voxels),
                             g_time.to(torch.float64).reshape(()) / float(n_pairs * voxels) if n_pairs else torch.zeros((), dtype=torch.float64, device=dev)])
        g_vol = torch.empty_like(volumes)
        _view.launch(_capi.check_vol, _capi.lib().nca_vol_tv_grad, dev, C.byref(desc), _capi.ptr(volumes), n_vol, eps_space, eps_time, int(cyclic),
                     _capi.ptr(scale), _capi.ptr(g_vol))
        return g_vol, None, None, None, None


def _tv_counts(volumes, cyclic):
    """(n_vol, voxels, n_pairs) of a stack: pairs (p, p + 1), and (n_vol - 1, 0) when cyclic and n_vol >= 2."""
    n_vol = 1 if volumes.dim() == 3 else volumes.shape[0]
    return n_vol, math.prod(volumes.shape[-3:]), n_vol - 1 + (1 if cyclic and n_vol >= 2 else 0)


def _launch_tv(volumes, desc, eps_space, eps_time, cyclic):
    """(tv_space, tv_time) f64 0-d: one nca_vol_tv of checked, contiguous volumes into a zeroed pair, divided by the counts."""
    n_vol, voxels, n_pairs = _tv_counts(volumes, cyclic)
    sums = torch.zeros(2, dtype=torch.float64, device=volumes.device)
    _view.launch(_capi.check_vol, _capi.lib().nca_vol_tv, volumes.device, C.byref(desc), _capi.ptr(volumes), n_vol, eps_space, eps_time, int(cyclic), _capi.ptr(sums))
    return sums[0] / float(n_vol * voxels), (sums[1] / float(n_pairs * voxels) if n_pairs else torch.zeros((), dtype=torch.float64, device=volumes.device))


def total_variation(volumes: torch.Tensor, *, bounds: Bounds, eps_space: float = 1e-3, eps_time: float = 1e-3, cyclic: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Smoothed total variation of f32 ``volumes`` ``[n0,n1,n2]`` or ``[n_vol,n0,n1,n2]`` (contiguous, on the device, nodes
    ``linspace(lo, hi, n)`` of ``bounds``), as two f64 0-d device tensors ``(tv_space, tv_time)``:

    * ``tv_space``: the mean over volumes and nodes of ``sqrt(eps_space^2 + |forward differences / node spacing|^2) - eps_space``;
    * ``tv_time``: the volumes are one stack of heart phases; the mean over pairs ``(p, p + 1)`` and nodes of
      ``sqrt(eps_time^2 + (x[p+1] - x[p])^2) - eps_time``.  ``cyclic`` adds the pair ``(n_vol - 1, 0)`` of a periodic cycle (``n_vol >= 2``);
      without pairs (one volume) it is exactly 0.

    Means, so that a weight means the same at every resolution; a flat stack gives exactly ``(0, 0)``.  The definition, operation by
    operation, is in include/nerfca_hip.h ("vol").  The sums are f64 atomics over blocks: their last bits can differ from run to run.

    With grad mode on and ``volumes.requires_grad`` both results carry a gradient in ``volumes`` (f32, the volumes' shape, one gathered
    kernel launch, the same bits on every run).  In every other case nothing is recorded."""
    _fused._require_cuda(volumes, "volumes")
    _view.check_contiguous_volumes(volumes, "total_variation")
    eps_space, eps_time = float(eps_space), float(eps_time)
    for eps, what in ((eps_space, "eps_space"), (eps_time, "eps_time")):
        if not (math.isfinite(eps) and eps > 0):
            raise _capi.NcaError(f"total_variation: {what} = {eps} is not finite and positive")
    desc = grid_desc(volumes.shape[-3:], bounds)
    cyclic = bool(cyclic)
    if torch.is_grad_enabled() and volumes.requires_grad:
        return _TotalVariation.apply(volumes, desc, eps_space, eps_time, cyclic)
    with torch.no_grad():
        return _launch_tv(volumes.detach(), desc, eps_space, eps_time, cyclic)


@torch.no_grad()
def project_sequence(sigma_static: torch.Tensor, sigma_dynamic: Optional[torch.Tensor], geo: dict, views: Sequence[Sequence[float]], samples: int, *,
                     bounds: Bounds = UNIT_BOUNDS, z: Optional[torch.Tensor] = None, chunk_rays: int = 65536, normalize: bool = False) -> dict:
    """Project the static volume ``[n0,n1,n2]`` and the P dynamic volumes ``[P,n0,n1,n2]`` (what ``export.density_volumes`` returns:
    sigma already scaled) through every view ``(theta, phi[, larm])`` of ``views``: f32 images ``pred`` and ``pred_dynamic``
    ``[V,P,W,H]`` and ``pred_static`` ``[V,W,H]``, the keys, shapes and composition of ``export.render_sequence``.  Per view and ray
    chunk there is one projection of the static volume and one of all P dynamic volumes.  ``sigma_dynamic=None`` behaves like
    ``temp_model=None`` there (P = 1, ``pred = pred_static``, ``pred_dynamic`` is ``I0`` everywhere).  ``z`` defaults to the un-jittered
    ``create_depth_values(near, far, samples)``; ``I0 = geo["max_pixel_value"]``; ``normalize=True`` adds the ``*_norm`` images and
    ``minmax`` as there."""
    from .train.data_helpers import create_depth_values
    _fused._require_cuda(sigma_static, "the static volume")
    dev = sigma_static.device
    if sigma_static.dim() != 3:
        raise _capi.NcaError(f"the static volume is [n0,n1,n2], got {tuple(sigma_static.shape)}")
    if sigma_dynamic is not None:
        _fused._require_cuda(sigma_dynamic, "the dynamic volumes")
        if sigma_dynamic.dim() != 4 or sigma_dynamic.shape[1:] != sigma_static.shape or sigma_dynamic.shape[0] == 0 or sigma_dynamic.device != dev:
            raise _capi.NcaError(f"the dynamic volumes are [P,n0,n1,n2] on the static volume's grid and device, got {tuple(sigma_dynamic.shape)} "
                                 f"for a static volume {tuple(sigma_static.shape)}")
    views = [tuple(float(a) for a in v) for v in views]
    if not views or any(len(v) not in (2, 3) for v in views):
        raise ValueError("views is a non-empty list of (theta, phi) or (theta, phi, larm)")
    W, H = (int(v) for v in geo["nDetector"])
    npix, V, P = W * H, len(views), (1 if sigma_dynamic is None else sigma_dynamic.shape[0])
    if z is None:
        z = create_depth_values(geo["near_thresh"], geo["far_thresh"], int(samples), dev)
    z = z.detach().to(device=dev, dtype=torch.float32).contiguous()
    if z.dim() != 1:
        raise _capi.NcaError("volume projection takes ONE depth vector [S] shared by all rays")
    dists = _default_dists(z).to(torch.float64).contiguous()
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))          # the f32 value render_sequence starts every ray sum from
    pred = torch.empty((V, P, npix), dtype=torch.float32, device=dev)
    pred_d = torch.empty((V, P, npix), dtype=torch.float32, device=dev)
    pred_s = torch.empty((V, npix), dtype=torch.float32, device=dev)
    plan = _export.chunk_plan(npix, int(chunk_rays))
    with torch.cuda.device(dev):
        for v, view in enumerate(views):
            desc = _export.pack_view(geo, *view)
            for p0, n in plan:
                o, d = _export._rays_of(desc, p0, n, dev, torch.float64)
                pix_s = project_rays(sigma_static, o, d, z, dists, i0=i0, bounds=bounds)
                if sigma_dynamic is None:
                    _export.compose_images(pix_s, None, i0, pred[v, 0, p0:p0 + n], pred_s[v, p0:p0 + n], pred_d[v, 0, p0:p0 + n])
                    continue
                pix_d = project_rays(sigma_dynamic, o, d, z, dists, i0=i0, bounds=bounds)
                for j in range(P):
                    _export.compose_images(pix_s, pix_d[j], i0, pred[v, j, p0:p0 + n], pred_s[v, p0:p0 + n], pred_d[v, j, p0:p0 + n])
    out = {"pred": pred.reshape(V, P, W, H), "pred_static": pred_s.reshape(V, W, H), "pred_dynamic": pred_d.reshape(V, P, W, H)}
    if normalize:
        out["minmax"] = {}
        for k in ("pred", "pred_static", "pred_dynamic"):
            img = out[k]
            norm, mm = _export.normalize_images(img.reshape(-1, W, H))
            out[k + "_norm"], out["minmax"][k] = norm.reshape(img.shape), mm.reshape(img.shape[:-2] + (2,))
    return out


def project_view(sigma_static: torch.Tensor, sigma_dynamic: Optional[torch.Tensor], geo: dict, theta: float, phi: float, samples: int, *,
                 larm: float = 0, bounds: Bounds = UNIT_BOUNDS, z: Optional[torch.Tensor] = None, chunk_rays: int = 65536, normalize: bool = False) -> dict:
    """One view of one volume pair: ``project_sequence`` for ``[(theta, phi, larm)]`` and a static volume ``[n0,n1,n2]`` with a
    dynamic volume ``[n0,n1,n2]`` (or ``None``), the leading axes dropped -- ``pred``, ``pred_static``, ``pred_dynamic`` as f32
    ``[W,H]`` like ``export.render_view``."""
    if sigma_dynamic is not None and sigma_dynamic.dim() != 3:
        raise _capi.NcaError(f"project_view takes ONE dynamic volume [n0,n1,n2], got {tuple(sigma_dynamic.shape)}")
    out = project_sequence(sigma_static, None if sigma_dynamic is None else sigma_dynamic[None], geo, [(theta, phi, larm)], samples, bounds=bounds, z=z,
                           chunk_rays=chunk_rays, normalize=normalize)
    res = {k: t.reshape(t.shape[-2:]) for k, t in out.items() if k != "minmax"}
    if normalize:
        res["minmax"] = {k: t.reshape(2) for k, t in out["minmax"].items()}
    return res


def volume_teacher(bounds: Bounds) -> Callable:
    """A ``render=`` hook of ``synthetic.make_dataset`` for ``teacher=(vol_static [n0,n1,n2], vol_dynamic [P,n0,n1,n2])``: the target
    images are projections of the volume pair instead of renders of a network pair.  ``pix = (pix_s + pix_d[phase]) - I0`` in f64 in
    that order, as ``nca_view_compose`` forms the composite.  The dynamic stack is one heart cycle: phase ``p`` reads volume ``p mod P``.
    All rays of one call share one phase and one I0 (how ``make_dataset`` calls its hook); anything else is refused."""

    def render(vol_static, vol_dynamic, origins, dirs, phase_ids, I0, z, dists):
        _fused._require_cuda(phase_ids, "phase ids")
        _fused._require_cuda(I0, "I0")
        if vol_dynamic.dim() != 4 or vol_dynamic.shape[1:] != vol_static.shape:
            raise _capi.NcaError(f"volume_teacher takes teacher=(static [n0,n1,n2], dynamic [P,n0,n1,n2]), got {tuple(vol_static.shape)} and "
                                 f"{tuple(vol_dynamic.shape)}")
        if phase_ids.numel() != origins.shape[0] or I0.numel() != origins.shape[0]:
            raise _capi.NcaError("volume_teacher: one phase id and one I0 per ray")
        lo, hi, i_lo, i_hi = (float(x) for x in torch.stack([phase_ids.min().double(), phase_ids.max().double(), I0.min().double(), I0.max().double()]).tolist())
        if lo != hi:
            raise _capi.NcaError(f"volume_teacher projects ONE phase per call: the rays carry phases {int(lo)} .. {int(hi)}")
        if i_lo != i_hi:
            raise _capi.NcaError(f"volume_teacher takes ONE I0 per call: the rays carry {i_lo} .. {i_hi}")
        if lo < 0:
            raise _capi.NcaError(f"volume_teacher: phase {int(lo)} is negative")
        phase = int(lo) % vol_dynamic.shape[0]          # the heart cycle is periodic: make_dataset's held-out image is phase 3 whatever n_phases
        with torch.no_grad():          # a dataset is made of numbers: nothing is recorded, whatever the teacher volumes require
            pix_s = project_rays(vol_static, origins, dirs, z, dists, i0=i_lo, bounds=bounds)
            pix_d = project_rays(vol_dynamic[phase], origins, dirs, z, dists, i0=i_lo, bounds=bounds)
        return (pix_s + pix_d) - i_lo

    return render


def fit_volumes(frames: Sequence[Tuple[float, float, int, torch.Tensor]], geo: dict, shape: Sequence[int], samples: int, *, bounds: Bounds = UNIT_BOUNDS,
                n_phases: int, steps: int, lr: float = 1e-2, init: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, nonneg: bool = True,
                chunk_rays: int = 65536, z: Optional[torch.Tensor] = None, tv_space: float = 0.0, tv_time: float = 0.0, tv_eps: float = 1e-3,
                ssim_weight: float = 0.0, ssim_win: int = 11) -> dict:
    """Voxel reconstruction from projections by gradient descent: fit a static volume ``[n0,n1,n2]`` and a dynamic stack
    ``[n_phases,n0,n1,n2]`` (f32, nodes ``linspace(lo, hi, n)`` of ``bounds``) to ``frames``, a list of ``(theta, phi, phase, image)``
    with ``image`` f32 ``[W,H]`` on the device in the log space the datasets hold (``I0 = geo["max_pixel_value"]``).

    A frame's prediction is ``(A s + A d_phase) - I0`` in f64, composed as ``volume_teacher`` composes it, so a dataset made by that
    hook is reproduced at loss 0.  Frames are grouped by view: per view and ray chunk a step makes one ``project_rays`` of the static
    volume and ONE of all the phase volumes that view has.  The loss is the mean squared error over all pixels of all frames, the
    optimiser ``torch.optim.Adam(lr)``; ``nonneg`` clamps both volumes at 0 after each step.  ``init`` is a pair of starting volumes
    (default: zeros); ``z`` defaults to the un-jittered ``create_depth_values(near, far, samples)``.  Nothing is read back inside the
    loop.  Returns ``{"static", "dynamic", "loss"}``: the fitted f32 volumes and the loss before each step as a list of floats.

    ``tv_space`` / ``tv_time`` > 0 add the priors of ``total_variation`` (``eps_space = eps_time = tv_eps``, ``cyclic=True``: the stack is one
    periodic heart cycle): the objective is ``mse + tv_space (TVs(static) + TVs(dynamic)) + tv_time TVt(dynamic)``.  The result then also
    holds ``"tv_space"`` and ``"tv_time"``, the unweighted ``TVs(static) + TVs(dynamic)`` and ``TVt(dynamic)`` before each step as lists of
    floats; ``"loss"`` stays the data term.  With both weights 0 no prior kernel is launched and the result is as above.

    ``ssim_weight`` > 0 adds a structural term (``metrics.ssim``, window ``ssim_win``): the objective gains
    ``ssim_weight (1 - mean over frames of SSIM(prediction, image))``.  A view's ray chunks are concatenated into whole f32 ``[W,H]``
    predictions before the call; the range of a frame is ``max - min`` of its image, formed once before the loop.  The result then also holds
    ``"ssim"``, the unweighted mean SSIM before each step as a list of floats.  With weight 0 nothing of it is launched and the keys and bits
    of the result are as without the argument.

    Refused (``NcaError``): no frames, a phase outside ``[0, n_phases)``, an image that is not f32 ``[W,H]`` on the volumes' device, a
    weight that is negative or not finite, a ``tv_eps`` that is not finite and positive, with ``ssim_weight`` > 0 an ``ssim_win`` that is
    not odd, above 11 or larger than the detector, and with ``ssim_weight`` > 0 a frame that is constant (its range is 0, for which SSIM is
    NaN and would turn the whole objective into NaN; checked once before the loop, the one read-back the term costs)."""
    from .train.data_helpers import create_depth_values
    frames = list(frames)
    if not frames:
        raise _capi.NcaError("fit_volumes: no frames to fit")
    shape = tuple(int(n) for n in shape)
    grid_desc(shape, bounds)          # refuses a bad grid before anything is allocated
    n_phases, steps = int(n_phases), int(steps)
    if n_phases < 1 or steps < 1:
        raise _capi.NcaError(f"fit_volumes: n_phases = {n_phases} and steps = {steps} must be positive")
    tv_space, tv_time, tv_eps = float(tv_space), float(tv_time), float(tv_eps)
    for w, what in ((tv_space, "tv_space"), (tv_time, "tv_time")):
        if not (math.isfinite(w) and w >= 0):
            raise _capi.NcaError(f"fit_volumes: {what} = {w} is not a finite weight >= 0")
    if not (math.isfinite(tv_eps) and tv_eps > 0):
        raise _capi.NcaError(f"fit_volumes: tv_eps = {tv_eps} is not finite and positive")
    priors = tv_space > 0 or tv_time > 0
    ssim_weight = float(ssim_weight)
    if not (math.isfinite(ssim_weight) and ssim_weight >= 0):
        raise _capi.NcaError(f"fit_volumes: ssim_weight = {ssim_weight} is not a finite weight >= 0")
    structural = ssim_weight > 0
    W, H = (int(v) for v in geo["nDetector"])
    npix = W * H
    if structural:
        if int(ssim_win) != ssim_win or not 1 <= int(ssim_win) <= _metrics.MAX_WIN or int(ssim_win) % 2 == 0:
            raise _capi.NcaError(f"fit_volumes: ssim_win = {ssim_win} is not an odd window length in [1, {_metrics.MAX_WIN}]")
        ssim_win = int(ssim_win)
        if ssim_win > min(W, H):
            raise _capi.NcaError(f"fit_volumes: ssim_win = {ssim_win} is larger than the detector, {W} x {H}")
    first = frames[0][3]
    if not isinstance(first, torch.Tensor):
        raise _capi.NcaError("fit_volumes: a frame is (theta, phi, phase, image) with image a tensor")
    _fused._require_cuda(first, "frame images")
    dev = first.device
    by_view = {}
    for k, frame in enumerate(frames):
        if len(frame) != 4:
            raise _capi.NcaError(f"fit_volumes: frame {k} is not (theta, phi, phase, image)")
        theta, phi, phase, image = frame
        if int(phase) != phase or not 0 <= int(phase) < n_phases:
            raise _capi.NcaError(f"fit_volumes: frame {k} has phase {phase}, outside [0, {n_phases})")
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or tuple(image.shape) != (W, H):
            raise _capi.NcaError(f"fit_volumes: the image of frame {k} is not float32 [{W},{H}]: got "
                                 f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
        if image.device != dev:
            raise _capi.NcaError(f"fit_volumes: the image of frame {k} lives on {image.device}, frame 0 on {dev}")
        by_view.setdefault((float(theta), float(phi)), []).append((int(phase), image.detach().reshape(npix).to(torch.float64)))
    if init is None:
        static = torch.zeros(shape, dtype=torch.float32, device=dev)
        dynamic = torch.zeros((n_phases,) + shape, dtype=torch.float32, device=dev)
    else:
        static, dynamic = (t.detach().to(device=dev, dtype=torch.float32).clone().contiguous() for t in init)
        if tuple(static.shape) != shape or tuple(dynamic.shape) != (n_phases,) + shape:
            raise _capi.NcaError(f"fit_volumes: init is (static {shape}, dynamic {(n_phases,) + shape}), got {tuple(static.shape)} and {tuple(dynamic.shape)}")
    static.requires_grad_(True)
    dynamic.requires_grad_(True)
    if z is None:
        z = create_depth_values(geo["near_thresh"], geo["far_thresh"], int(samples), dev)
    z = z.detach().to(device=dev, dtype=torch.float32).contiguous()
    if z.dim() != 1:
        raise _capi.NcaError("volume projection takes ONE depth vector [S] shared by all rays")
    dists = _default_dists(z).to(torch.float64).contiguous()
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    plan = _export.chunk_plan(npix, int(chunk_rays))
    # per view, once: the rays of every chunk, the rows of the dynamic stack the view's frames use, and the targets [F,npix] in f64
    work: List[tuple] = []
    with torch.cuda.device(dev), torch.no_grad():
        for (theta, phi), items in by_view.items():
            desc = _export.pack_view(geo, theta, phi)
            rays = [_export._rays_of(desc, p0, n, dev, torch.float64) for p0, n in plan]
            rows = torch.tensor([p for p, _ in items], dtype=torch.int64, device=dev)
            target = torch.stack([img for _, img in items])
            if structural:          # the f32 images and their ranges, once
                images = target.to(torch.float32).reshape(-1, W, H)
                work.append((rays, rows, target, images, images.amax(dim=(-2, -1)).double() - images.amin(dim=(-2, -1)).double()))
            else:
                work.append((rays, rows, target))
    if structural:          # a constant image has range 0, for which SSIM is NaN: refused here, once, before the loop
        flat = torch.cat([w[4] for w in work])
        if not bool(((flat > 0) & torch.isfinite(flat)).all()):
            raise _capi.NcaError(f"fit_volumes: ssim_weight > 0 needs frames whose max - min is finite and positive; {int((~((flat > 0) & torch.isfinite(flat))).sum())} "
                                 f"of the {len(frames)} frames are constant or not finite")
    total = float(len(frames) * npix)
    opt = torch.optim.Adam([static, dynamic], lr=float(lr))
    losses = torch.zeros(steps, dtype=torch.float64, device=dev)
    tvs = torch.zeros((2, steps), dtype=torch.float64, device=dev) if priors else None
    ssims = torch.zeros(steps, dtype=torch.float64, device=dev) if structural else None
    with torch.cuda.device(dev):
        for step in range(steps):
            opt.zero_grad(set_to_none=True)
            loss = torch.zeros((), dtype=torch.float64, device=dev)
            similarity = torch.zeros((), dtype=torch.float64, device=dev) if structural else None
            for rays, rows, target, *whole in work:
                stack = dynamic.index_select(0, rows)          # [F,n0,n1,n2]: the phases this view has, projected in one pass
                chunks = []
                for (p0, n), (o, d) in zip(plan, rays):
                    pix_s = project_rays(static, o, d, z, dists, i0=i0, bounds=bounds)
                    pix_d = project_rays(stack, o, d, z, dists, i0=i0, bounds=bounds)
                    pred = (pix_s[None] + pix_d) - i0
                    diff = pred - target[:, p0:p0 + n]
                    loss = loss + (diff * diff).sum()
                    if structural:
                        chunks.append(pred)
                if structural:
                    images, ranges = whole
                    frames_pred = (chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=1)).to(torch.float32).reshape(-1, W, H)
                    similarity = similarity + _metrics.ssim(frames_pred, images, data_range=ranges, win_size=ssim_win).sum()
            loss = loss / total
            losses[step] = loss.detach()
            if structural:
                similarity = similarity / float(len(frames))
                ssims[step] = similarity.detach()
                loss = loss + ssim_weight * (1.0 - similarity)
            if priors:
                space_s, _ = total_variation(static, bounds=bounds, eps_space=tv_eps, eps_time=tv_eps)
                space_d, time_d = total_variation(dynamic, bounds=bounds, eps_space=tv_eps, eps_time=tv_eps, cyclic=True)
                space = space_s + space_d
                tvs[0, step], tvs[1, step] = space.detach(), time_d.detach()
                loss = loss + tv_space * space + tv_time * time_d
            loss.backward()
            opt.step()
            if nonneg:
                with torch.no_grad():
                    static.clamp_(min=0)
                    dynamic.clamp_(min=0)
    out = {"static": static.detach(), "dynamic": dynamic.detach(), "loss": losses.tolist()}
    if priors:
        out["tv_space"], out["tv_time"] = tvs.tolist()
    if structural:
        out["ssim"] = ssims.tolist()
    return out
