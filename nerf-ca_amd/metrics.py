"""Comparing image stacks and voxel stacks on the device: PSNR and the structural similarity of Wang et al. (csrc/view/nca_ssim.hip), and
the exact Euclidean distance transform with the vessel distances built on it (csrc/view/nca_edt.hip).

NeRF-CA reports its 2-D results as PSNR and SSIM.  ``ssim`` is one pass over the two stacks in f64 (``nca_ssim``): Gaussian-windowed
means, variances and the covariance at every window position that lies inside the image (no padding), combined as include/nerfca_hip.h
("ssim") writes it, and averaged per image.  It is differentiable in the prediction (``nca_ssim_grad``: gathered, the same
bits on every run), so ``1 - ssim`` serves as a loss; ``drr.fit_volumes`` takes it with ``ssim_weight``.  ``compare_sequences`` sets the
stacks of ``export.render_sequence`` / ``drr.project_sequence`` side by side.  There is no torch implementation behind ``ssim``.

In 3-D, ``distance_transform`` is the exact distance from every node of a voxel stack to the nearest node above a threshold
(``nca_vol_edt``; include/nerfca_hip.h, "edt").  ``mask_distances`` (mean, Hausdorff and percentile distances between two thresholded
stacks) and ``centreline_coverage`` (the share of a known centreline that lies within a tolerance of a thresholded stack) are torch
reductions over two such maps: measures that stay graded where the Dice coefficient of thin vessels is 0.  There is no torch
implementation behind ``distance_transform``.

``soft_skeleton`` is the soft skeleton of Shit et al. (clDice, CVPR 2021), built from minimum and maximum stencils
(``nca_vol_softskel``; include/nerfca_hip.h, "skel"), and ``cldice`` the centreline Dice of two stacks: how much of each volume's
skeleton lies inside the other volume.  It judges the topology of a vessel where the Dice coefficient only counts shared nodes, and it
needs no analytic centreline.  There is no torch implementation behind ``soft_skeleton``.

``label`` numbers the connected components of a thresholded stack as ``scipy.ndimage.label`` does (``nca_vol_label``; include/nerfca_hip.h,
"label": a union-find over the voxel grid), ``component_sizes`` counts their nodes, ``keep_largest`` reduces a mask to its largest
components and ``component_report`` sets the component counts of a prediction and the truth side by side: is the fit one tree, or a tree
plus speckle?  There is no torch implementation behind ``label``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _capi
from . import _view
from . import fused as _fused

MAX_WIN = 11          # NCA_SSIM_MAX_WIN


def gaussian_window(win_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The 1-D window of Wang et al.: ``exp(-d^2 / (2 sigma^2))`` at ``d = -(K-1)/2 .. (K-1)/2``, normalised to sum 1, numpy f64 ``[K]``.
    One half is computed and mirrored, so the window is symmetric bit for bit."""
    K, sigma = int(win_size), float(sigma)
    if K != win_size or K < 1 or K % 2 == 0:
        raise _capi.NcaError(f"gaussian_window: win_size = {win_size} is not an odd positive length")
    if not (math.isfinite(sigma) and sigma > 0):
        raise _capi.NcaError(f"gaussian_window: sigma = {sigma} is not finite and positive")
    h = K // 2
    half = np.exp(-(np.arange(h, -1, -1, dtype=np.float64) ** 2) / (2.0 * sigma * sigma))          # d = -h .. 0
    g = np.concatenate([half, half[-2::-1]])
    g = g / g.sum()
    g[h + 1:] = g[:h][::-1]
    return g


def _c_window(win: np.ndarray):
    win = np.ascontiguousarray(win, dtype=np.float64)
    return (C.c_double * win.size)(*win.tolist())


def _launch_ssim(x, y, rng, win, k1, k2, want_map):
    """(sums f64 [N], map f32 [N,Hv,Wv] or None): one nca_ssim of checked, contiguous stacks [N,H,W] into zeroed sums."""
    N, H, W = x.shape
    K = len(win)
    sums = torch.zeros(N, dtype=torch.float64, device=x.device)
    smap = torch.empty((N, H - K + 1, W - K + 1), dtype=torch.float32, device=x.device) if want_map else None
    _view.launch(_capi.check_ssim, _capi.lib().nca_ssim, x.device, N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), K, win, k1, k2, _capi.ptr(sums),
                 _capi.ptr(smap))
    return sums, smap


class _Ssim(torch.autograd.Function):
    """The per-image mean SSIM with a gradient in the prediction: the forward is one ``nca_ssim``, the backward one ``nca_ssim_grad`` whose
    device ``scale`` holds the upstream gradients over the position count -- nothing is read back.  The map, when asked for, is returned
    without a gradient."""

    @staticmethod
    def forward(ctx, x, y, rng, win, k1, k2, want_map):
        ctx.save_for_backward(x, y, rng)
        ctx.args = (win, k1, k2)
        N, H, W = x.shape
        K = len(win)
        sums, smap = _launch_ssim(x.detach(), y, rng, win, k1, k2, want_map)
        mean = sums / float((H - K + 1) * (W - K + 1))
        if want_map:
            ctx.mark_non_differentiable(smap)
            return mean, smap
        return mean, None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mean, _g_map):
        x, y, rng = ctx.saved_tensors
        win, k1, k2 = ctx.args
        N, H, W = x.shape
        K = len(win)
        dev = x.device
        if g_mean.device != dev:
            raise _capi.NcaError(f"ssim backward: the upstream gradient lives on {g_mean.device}, the images on {dev}")
        scale = (g_mean.to(torch.float64) / float((H - K + 1) * (W - K + 1))).contiguous()
        g_x = torch.empty_like(x)
        lib = _capi.lib()
        nbytes = int(lib.nca_ssim_grad_workspace(N, H, W, K))
        work = _view.workspace(nbytes, dev)
        _view.launch(_capi.check_ssim, lib.nca_ssim_grad, dev, N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), K, win, k1, k2, _capi.ptr(scale), _capi.ptr(g_x),
                     _capi.ptr(work), nbytes)
        return g_x, None, None, None, None, None, None


def _range_vector(data_range, lead, dev) -> torch.Tensor:
    """f64 [N] on the device from a float or a tensor broadcastable to the leading shape; nothing is read back."""
    if isinstance(data_range, torch.Tensor):
        r = data_range.detach().to(device=dev, dtype=torch.float64)
    else:
        r = torch.tensor(float(data_range), dtype=torch.float64, device=dev)
    try:
        r = torch.broadcast_to(r, lead)
    except RuntimeError:
        raise _capi.NcaError(f"data_range of shape {tuple(r.shape)} does not broadcast to the leading shape {tuple(lead)}") from None
    return r.reshape(-1).contiguous()


def _check_pair(pred, truth, who):
    for t, what in ((pred, "pred"), (truth, "truth")):
        if not isinstance(t, torch.Tensor):
            raise _capi.NcaError(f"{who}: {what} is not a tensor")
        _fused._require_cuda(t, what)
    if pred.dtype != torch.float32 or truth.dtype != torch.float32:
        raise _capi.NcaError(f"{who} takes float32 images, got {pred.dtype} and {truth.dtype}")
    if pred.dim() < 2 or pred.shape != truth.shape or pred.numel() == 0:
        raise _capi.NcaError(f"{who} takes two stacks [..., A, B] of one shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise _capi.NcaError(f"{who}: pred lives on {pred.device}, truth on {truth.device}")


def ssim(pred: torch.Tensor, truth: torch.Tensor, *, data_range: Union[float, torch.Tensor], win_size: int = 11, sigma: float = 1.5, k1: float = 0.01,
         k2: float = 0.03, full: bool = False):
    """Mean structural similarity per image of f32 stacks ``pred`` and ``truth`` ``[..., A, B]`` on the device (the last two axes are the
    image), as an f64 device tensor of the leading shape.  ``data_range`` is the dynamic range ``L`` of the images (``C1 = (k1 L)^2``,
    ``C2 = (k2 L)^2``): a float, or a tensor broadcastable to the leading shape -- it stays on the device.  A range that is not finite and
    positive gives NaN for that image.  The window is ``gaussian_window(win_size, sigma)`` on both axes; statistics are taken only where the
    window lies inside the image, so the mean runs over ``(A - K + 1) (B - K + 1)`` positions and both axes must be at least ``win_size``
    (odd, at most 11).  ``full=True`` returns ``(mean, map)`` with the f32 map ``[..., A - K + 1, B - K + 1]`` (no gradient).

    Identical stacks give exactly 1.  The definition, operation by operation, is in include/nerfca_hip.h ("ssim"); the per-image sum is
    f64 atomics over blocks, so its last bits can differ from run to run.

    With grad mode on and ``pred.requires_grad`` the mean carries a gradient in ``pred`` (f32, gathered: the same bits on
    every run); ``truth`` and ``data_range`` get none.  In every other case nothing is recorded."""
    _check_pair(pred, truth, "ssim")
    k1, k2 = float(k1), float(k2)
    win = gaussian_window(win_size, sigma)
    K = len(win)
    A, B = pred.shape[-2:]
    if K > MAX_WIN:
        raise _capi.NcaError(f"ssim: win_size = {K} is larger than {MAX_WIN}")
    if A < K or B < K:
        raise _capi.NcaError(f"ssim: images of {A} x {B} are smaller than the window, win_size = {K}")
    lead = pred.shape[:-2]
    rng = _range_vector(data_range, lead, pred.device)
    cwin = _c_window(win)
    y = truth.detach().reshape(-1, A, B).contiguous()
    if torch.is_grad_enabled() and pred.requires_grad:
        mean, smap = _Ssim.apply(pred.reshape(-1, A, B).contiguous(), y, rng, cwin, k1, k2, bool(full))
    else:
        with torch.no_grad():
            sums, smap = _launch_ssim(pred.detach().reshape(-1, A, B).contiguous(), y, rng, cwin, k1, k2, bool(full))
            mean = sums / float((A - K + 1) * (B - K + 1))
    mean = mean.reshape(lead)
    return (mean, smap.reshape(lead + smap.shape[-2:])) if full else mean


def psnr(pred: torch.Tensor, truth: torch.Tensor, *, data_range: Union[float, torch.Tensor]) -> torch.Tensor:
    """Peak signal-to-noise ratio per image, ``10 log10(range^2 / mse)`` in f64, of stacks ``[..., A, B]``: an f64 tensor of the leading
    shape (``inf`` for identical images).  Plain torch: a handful of reductions."""
    _check_pair(pred, truth, "psnr")
    lead = pred.shape[:-2]
    diff = pred.detach().double() - truth.detach().double()
    mse = (diff * diff).mean(dim=(-2, -1))
    rng = _range_vector(data_range, lead, pred.device).reshape(lead)
    return 10.0 * torch.log10(rng * rng / mse)


def compare_sequences(pred: dict, truth: dict, *, data_range: Optional[Union[float, torch.Tensor]] = None) -> dict:
    """PSNR and SSIM of two sequence dicts as ``export.render_sequence`` / ``drr.project_sequence`` return them.  For every key both hold
    as f32 image stacks of one shape (``pred`` ``[V,P,W,H]``, ``pred_static`` ``[V,W,H]``, ...): ``{"psnr", "ssim"}`` per ``(view, phase)``
    as f64 device tensors of the leading shape, and ``"psnr_mean"``, ``"ssim_mean"`` as 0-d tensors.  ``data_range`` defaults to ``max - min``
    of each TRUTH image, formed in f64 on the device.  A constant truth image (for
    instance the ``pred_dynamic`` of a static scene, ``I0`` everywhere) has range 0: its SSIM is NaN by the kernel's rule and its PSNR
    ``-inf`` or NaN, and so are the means of that stack; pass ``data_range`` to compare such stacks."""
    out = {}
    for key in pred:
        a, b = pred[key], truth.get(key)
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.dim() < 3 or a.shape != b.shape or not a.dtype.is_floating_point:
            continue
        a, b = a.detach().to(torch.float32), b.detach().to(torch.float32)
        rng = b.amax(dim=(-2, -1)).double() - b.amin(dim=(-2, -1)).double() if data_range is None else data_range
        with torch.no_grad():
            p, s = psnr(a, b, data_range=rng), ssim(a, b, data_range=rng)
        out[key] = {"psnr": p, "ssim": s, "psnr_mean": p.mean(), "ssim_mean": s.mean()}
    if not out:
        raise _capi.NcaError("compare_sequences: the two dicts share no image stack of one shape")
    return out


# ----------------------------------------------------------------------------- distances in 3-D
MAX_AXIS = 512          # NCA_EDT_MAX_AXIS


@torch.no_grad()
def distance_transform(vol: torch.Tensor, bounds, *, threshold: float, inside: bool = False) -> torch.Tensor:
    """The exact Euclidean distance transform of a thresholded f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device, as an f32 tensor of
    the same shape: the grid is ``drr.grid_desc(vol.shape[-3:], bounds)`` and distances are in its world units (anisotropic spacings are
    honoured).  ``inside=False``: the distance from every node to the nearest node with ``vol > threshold`` (0 on the mask).
    ``inside=True``: the distance to the nearest node that is NOT ``> threshold`` -- what
    ``scipy.ndimage.distance_transform_edt(vol > threshold, sampling=h)`` returns.  A NaN value is not ``> threshold``.  A volume of the
    stack with no such node is ``+inf`` everywhere; every volume is transformed on its own.

    One ``nca_vol_edt`` (three launches; its definition, operation by operation, is in include/nerfca_hip.h, "edt"): the same bits on
    every run.  Not differentiable: it runs under ``no_grad`` and the result is detached.  An axis longer than 512 nodes is refused."""
    _view.check_volume(vol, "distance_transform")          # refused before the threshold is looked at
    threshold = _view.finite_threshold(threshold, "distance_transform")
    desc, x, n_vol, _ = _view.volume_stack(vol, "distance_transform", bounds)
    out = torch.empty_like(x)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_edt_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_edt, lib.nca_vol_edt, x.device, C.byref(desc), _capi.ptr(x), n_vol, threshold, 1 if inside else 0, _capi.ptr(out), _capi.ptr(work), nbytes)
    return out.reshape(vol.shape)


def _directed(dist, mask, percentile):
    """(count i64, sum f64, max f64, quantile f64) per leading index of ``dist`` over the nodes of ``mask``; NaN where the mask is empty."""
    lead = mask.shape[:-3]
    m = mask.reshape(-1, mask.shape[-3] * mask.shape[-2] * mask.shape[-1])
    d = dist.reshape(m.shape).double()
    n = m.sum(dim=1)
    nan = torch.full((), math.nan, dtype=torch.float64, device=d.device)
    total = torch.where(m, d, torch.zeros((), dtype=torch.float64, device=d.device)).sum(dim=1)
    top = torch.where(m, d, torch.full((), -math.inf, dtype=torch.float64, device=d.device)).amax(dim=1)
    quant = []
    for k in range(m.shape[0]):          # the masked sets differ in size: one quantile per entry
        quant.append(torch.quantile(d[k][m[k]], percentile / 100.0, interpolation="higher") if int(n[k]) else nan)
    quant = torch.stack(quant) if quant else torch.empty(0, dtype=torch.float64, device=d.device)
    empty = n == 0
    return (n.reshape(lead), torch.where(empty, nan, total).reshape(lead), torch.where(empty, nan, top).reshape(lead), quant.reshape(lead))


@torch.no_grad()
def mask_distance_reductions(a: torch.Tensor, b: torch.Tensor, dist_to_a: torch.Tensor, dist_to_b: torch.Tensor, percentile: float = 95.0) -> dict:
    """The reductions of ``mask_distances`` from the two masks ``a``, ``b`` (bool ``[..., n0, n1, n2]``) and the two distance maps (to the
    nearest node of ``a`` / of ``b``, any float dtype): plain torch on whatever device the tensors live on."""
    percentile = float(percentile)
    if not 0.0 <= percentile <= 100.0:
        raise _capi.NcaError(f"mask_distances: percentile = {percentile} is outside [0, 100]")
    if not (a.shape == b.shape == dist_to_a.shape == dist_to_b.shape) or a.dim() < 3:
        raise _capi.NcaError(f"mask_distances: masks {tuple(a.shape)}, {tuple(b.shape)} and maps {tuple(dist_to_a.shape)}, {tuple(dist_to_b.shape)} differ in shape")
    n_a, sum_a, max_a, q_a = _directed(dist_to_b, a, percentile)
    n_b, sum_b, max_b, q_b = _directed(dist_to_a, b, percentile)
    either = (n_a == 0) | (n_b == 0)
    nan = torch.full((), math.nan, dtype=torch.float64, device=sum_a.device)

    def both(x):
        return torch.where(either, nan, x)

    return {"n_pred": n_a, "n_truth": n_b, "pred_to_truth": both(sum_a / n_a), "truth_to_pred": both(sum_b / n_b),
            "assd": both((sum_a + sum_b) / (n_a + n_b)), "hausdorff": both(torch.maximum(max_a, max_b)), "hd_percentile": both(torch.maximum(q_a, q_b))}


@torch.no_grad()
def mask_distances(pred: torch.Tensor, truth: torch.Tensor, bounds, *, threshold: float, pred_threshold: Optional[float] = None,
                   percentile: float = 95.0, surface: bool = False) -> dict:
    """Distances between the masks ``A = pred > pred_threshold`` (``threshold`` when ``pred_threshold`` is ``None``) and
    ``B = truth > threshold`` of two f32 stacks ``[..., n0, n1, n2]`` on the device, in the world units of ``bounds``: f64 device tensors of
    the leading shape (a stack ``[P, n0, n1, n2]`` gives ``[P]``).

    ``n_pred``, ``n_truth``: the node counts (i64).  ``pred_to_truth``: the mean over A of the distance to the nearest node of B;
    ``truth_to_pred`` the other way round; ``assd``: the mean over both together, ``(sum_A + sum_B) / (|A| + |B|)``; ``hausdorff``: the
    larger of the two directed maxima; ``hd_percentile``: the larger of the two directed ``percentile`` quantiles
    (``torch.quantile(..., interpolation="higher")``).  The masks are whole bodies, not surfaces: a node of A inside B counts with distance 0.

    ``surface=True`` measures between SURFACES instead: A and B are first replaced by their borders, ``ccta.mask_border`` (the nodes one
    6-connected erosion removes; a node of a mask on a face of the grid is a border node), and everything above -- the two distance maps, the
    reductions, and the counts ``n_pred`` and ``n_truth`` -- is taken of those.  This is MedPy's ``__surface_distances`` with connectivity
    1, on which its ``assd`` and ``hd95`` rest: a prediction lying wholly inside the truth no longer scores 0.

    Two ``distance_transform`` calls (and, with ``surface``, two ``ccta.mask_border``); the reductions are torch on the device.  An entry
    whose A or B is empty is NaN in every distance (its counts are still returned); identical masks give exactly 0 in every distance."""
    _view.check_volume(pred, "mask_distances", "pred")
    _view.check_volume(truth, "mask_distances", "truth")
    if pred.shape != truth.shape:
        raise _capi.NcaError(f"mask_distances takes two stacks of one shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise _capi.NcaError(f"mask_distances: pred lives on {pred.device}, truth on {truth.device}")
    threshold = float(threshold)
    pred_threshold = threshold if pred_threshold is None else float(pred_threshold)
    if surface:
        from . import ccta          # ccta imports this module
        a, b = ccta.mask_border(pred, threshold=pred_threshold), ccta.mask_border(truth, threshold=threshold)
        to_a = distance_transform(a.to(torch.float32), bounds, threshold=0.5)
        to_b = distance_transform(b.to(torch.float32), bounds, threshold=0.5)
        return mask_distance_reductions(a, b, to_a, to_b, percentile)
    to_a = distance_transform(pred, bounds, threshold=pred_threshold)
    to_b = distance_transform(truth, bounds, threshold=threshold)
    return mask_distance_reductions(pred.detach() > pred_threshold, truth.detach() > threshold, to_a, to_b, percentile)


def nearest_nodes(points, shape, bounds):
    """(index i64 ``[n, 3]``, inside bool ``[n]``) of host points f64 ``[n, 3]``: the node nearest each point, ``floor(g_a + 0.5)`` with
    ``g_a = (x_a - lo_a) inv_a`` of ``drr.grid_desc(shape, bounds)``; ``inside`` is False where an index falls outside the grid."""
    desc = _capi.grid_desc(shape, bounds)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    lo, inv = np.array(list(desc.lo)), np.array(list(desc.inv))
    idx = np.floor((pts - lo) * inv + 0.5)
    n = np.array([int(s) for s in shape])
    inside = np.isfinite(idx).all(axis=1) & (idx >= 0).all(axis=1) & (idx <= n - 1).all(axis=1)
    return np.where(inside[:, None], idx, 0).astype(np.int64), inside


@torch.no_grad()
def coverage_reductions(dist: torch.Tensor, bounds, points, tol: float) -> dict:
    """The reductions of ``centreline_coverage`` from the distance maps ``dist`` ``[P, n0, n1, n2]`` (or ``[n0, n1, n2]``): plain torch on
    whatever device the maps live on."""
    tol = float(tol)
    if not tol >= 0.0:
        raise _capi.NcaError(f"centreline_coverage: tol = {tol} is not a non-negative length")
    if dist.dim() == 3:
        dist = dist[None]
    if isinstance(points, np.ndarray) and points.ndim == 2:
        points = [points]
    points = list(points)
    if dist.dim() != 4 or len(points) not in (1, dist.shape[0]):
        raise _capi.NcaError(f"centreline_coverage: {len(points)} point sets for maps of shape {tuple(dist.shape)}")
    P, shape = dist.shape[0], tuple(dist.shape[1:])
    cov, mean, n_pts, n_out = [], [], [], []
    for p in range(P):
        idx, inside = nearest_nodes(points[p if len(points) > 1 else 0], shape, bounds)
        idx = torch.from_numpy(idx[inside]).to(dist.device)
        d = dist[p][idx[:, 0], idx[:, 1], idx[:, 2]].double()
        n_pts.append(int(inside.sum()))
        n_out.append(int((~inside).sum()))
        cov.append((d <= tol).double().mean() if n_pts[-1] else torch.full((), math.nan, dtype=torch.float64, device=dist.device))
        mean.append(d.mean() if n_pts[-1] else torch.full((), math.nan, dtype=torch.float64, device=dist.device))
    return {"coverage": torch.stack(cov), "mean_distance": torch.stack(mean), "n_points": torch.tensor(n_pts, dtype=torch.int64, device=dist.device),
            "n_outside": torch.tensor(n_out, dtype=torch.int64, device=dist.device)}


@torch.no_grad()
def centreline_coverage(vol: torch.Tensor, bounds, points, *, threshold: float, tol: float) -> dict:
    """How much of a known centreline a thresholded stack reaches.  ``vol`` is f32 ``[P, n0, n1, n2]`` (or one volume) on the device,
    ``points`` a list of P host arrays f64 ``[n_p, 3]`` in world coordinates (``phantom.centreline_points``; one array serves every
    phase).  Per phase, the distance map of ``vol > threshold`` is read at the node nearest each point, index ``floor(g_a + 0.5)``; a point
    whose index falls outside the grid is dropped and counted in ``n_outside``.  Returns per phase: ``coverage`` (the share of the
    remaining points with distance ``<= tol``, f64), ``mean_distance`` (f64; ``inf`` when the mask is empty), ``n_points`` and
    ``n_outside`` (i64).  A phase with no point inside the grid is NaN.

    The nearest-node read adds at most half a cell diagonal to a point's true distance from the mask (the node is at most that far from
    the point), so a ``tol`` of one cell diagonal accepts centreline points up to one and a half diagonals away and never rejects one
    within half a diagonal."""
    _view.check_volume(vol, "centreline_coverage")
    if vol.dim() not in (3, 4):
        raise _capi.NcaError(f"centreline_coverage takes [P, n0, n1, n2] or [n0, n1, n2], got {tuple(vol.shape)}")
    return coverage_reductions(distance_transform(vol, bounds, threshold=float(threshold)), bounds, points, tol)


# ----------------------------------------------------------------------------- the soft skeleton and clDice
MAX_SKEL_ITER = 512          # NCA_SKEL_MAX_ITER


def _skel_iterations(iterations, who):
    n = int(iterations)
    if n != iterations or isinstance(iterations, bool) or not 0 <= n <= MAX_SKEL_ITER:
        raise _capi.NcaError(f"{who}: iterations = {iterations!r} is not a whole number in 0 .. {MAX_SKEL_ITER}")
    return n


def _skel_input(vol, threshold, who, what="vol"):
    """The f32 stack the kernels take: ``(vol > threshold)`` as 0 / 1 with a threshold, else ``vol`` itself; a bool mask becomes 0 / 1 first."""
    if isinstance(vol, torch.Tensor) and vol.dtype == torch.bool:
        _fused._require_cuda(vol, what)
        vol = vol.to(torch.float32)
    _view.check_volume(vol, who, what)
    if threshold is None:
        return vol
    return (vol.detach() > _view.finite_threshold(threshold, who)).to(torch.float32)


@torch.no_grad()
def soft_skeleton(vol: torch.Tensor, iterations: int, *, threshold: Optional[float] = None) -> torch.Tensor:
    """The soft skeleton (Shit et al., clDice, CVPR 2021) of every volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device, as
    an f32 tensor of the same shape: with ``erode`` the minimum over a node and its six axis neighbours, ``dilate`` the maximum over the
    3 x 3 x 3 box, ``open = dilate(erode)``, neighbours outside the grid left out,

        ``S = relu(E_0 - open(E_0))``, then for ``j = 1 .. iterations``: ``E_j = erode(E_{j-1})``, ``d = relu(E_j - open(E_j))``,
        ``S = S + relu(d - S d)``.

    For finite input this is, as values, the published torch expression (``soft_erode`` from three 1-D ``-max_pool3d(-x)``, ``soft_dilate =
    max_pool3d(x, 3, 1, 1)``).  ``iterations`` should reach the largest vessel radius in nodes: a straight tube of radius 2 has an empty
    skeleton at ``iterations = 1`` and its axis from 3 on; more iterations than needed change nothing.  At most 512.

    With ``threshold`` the input is ``vol > threshold`` as 0 / 1 (a bool mask is accepted too), and the result is binary and a subset of
    that mask.  The faces of the grid do not erode: a volume that is 1 everywhere has an empty skeleton.

    One ``nca_vol_softskel`` (``iterations + 1`` launches, minimum and maximum stencils in f32: exact, the same bits on every run; the
    definition with the order of the comparisons is in include/nerfca_hip.h, "skel").  Not differentiable: it runs under ``no_grad`` and
    the result is detached."""
    who = "soft_skeleton"
    x_in = _skel_input(vol, threshold, who)
    K = _skel_iterations(iterations, who)
    desc, x, n_vol, _ = _view.volume_stack(x_in, who)
    out = torch.empty_like(x)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_softskel_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_skel, lib.nca_vol_softskel, x.device, C.byref(desc), _capi.ptr(x), n_vol, K, _capi.ptr(out), _capi.ptr(work), nbytes)
    return out.reshape(vol.shape)


def _overlap_sums(a, b, who):
    """f64 ``[n_vol, 2]``: ``(sum a b, sum a)`` per volume of two checked f32 stacks of one shape on one device (``nca_vol_overlap_sums``)."""
    desc, x, n_vol, _ = _view.volume_stack(a, who)
    y = _view.volume_stack(b, who)[1]
    sums = torch.empty((n_vol, 2), dtype=torch.float64, device=x.device)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_overlap_sums_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_skel, lib.nca_vol_overlap_sums, x.device, C.byref(desc), _capi.ptr(x), _capi.ptr(y), n_vol, _capi.ptr(sums), _capi.ptr(work), nbytes)
    return sums


def _cldice_of_sums(sp_t, sp, st_p, st, smooth):
    smooth = float(smooth)
    if not (math.isfinite(smooth) and smooth >= 0.0):
        raise _capi.NcaError(f"cldice: smooth = {smooth} is not finite and non-negative")
    tprec = (sp_t + smooth) / (sp + smooth)
    tsens = (st_p + smooth) / (st + smooth)
    den = tprec + tsens
    zero = torch.zeros((), dtype=torch.float64, device=den.device)
    return {"cldice": torch.where(den == 0, zero, 2.0 * tprec * tsens / den), "tprec": tprec, "tsens": tsens}


@torch.no_grad()
def cldice_reductions(skel_pred: torch.Tensor, pred: torch.Tensor, skel_truth: torch.Tensor, truth: torch.Tensor, smooth: float = 0.0) -> dict:
    """The reductions of ``cldice`` from the two skeletons and the two volumes they are measured in (any float or bool dtype,
    ``[..., n0, n1, n2]`` of one shape): plain torch in f64 on whatever device the tensors live on."""
    if not (skel_pred.shape == pred.shape == skel_truth.shape == truth.shape) or pred.dim() < 3:
        raise _capi.NcaError(f"cldice: skeletons {tuple(skel_pred.shape)}, {tuple(skel_truth.shape)} and volumes {tuple(pred.shape)}, {tuple(truth.shape)} differ in shape")

    def total(x):
        return x.sum(dim=(-3, -2, -1))

    sp, st, p, t = (x.detach().double() for x in (skel_pred, skel_truth, pred, truth))
    return _cldice_of_sums(total(sp * t), total(sp), total(st * p), total(st), smooth)


@torch.no_grad()
def cldice(pred: torch.Tensor, truth: torch.Tensor, *, iterations: int, threshold: Optional[float] = None, pred_threshold: Optional[float] = None,
           smooth: float = 0.0) -> dict:
    """The centreline Dice (Shit et al., CVPR 2021) of two f32 stacks ``[..., n0, n1, n2]`` on the device, per volume: ``{"cldice",
    "tprec", "tsens"}`` as f64 device tensors of the leading shape.  With ``S_pred`` and ``S_truth`` the ``soft_skeleton`` of the two
    volumes at ``iterations``,

        ``tprec = (sum S_pred truth + smooth) / (sum S_pred + smooth)``      how much of the prediction's skeleton lies in the truth,
        ``tsens = (sum S_truth pred + smooth) / (sum S_truth + smooth)``     how much of the truth's skeleton lies in the prediction,
        ``cldice = 2 tprec tsens / (tprec + tsens)``, and 0 where ``tprec + tsens == 0``.

    An entry with an empty skeleton is NaN at ``smooth = 0`` (the quotient as it is).

    With ``threshold`` both volumes are binarised first, ``truth > threshold`` and ``pred > pred_threshold`` (``threshold`` when
    ``pred_threshold`` is ``None``; bool masks are accepted): this is the metric, and a mask against itself gives exactly 1.  Without a
    threshold the volumes are taken as they are, values in [0, 1]: the soft clDice of the paper.  The soft clDice of a volume that is not
    binary with itself is NOT 1 (0.49 for the 64^3 phantom's vessel volume divided by its maximum): a skeleton value s at a node of
    value v counts s v, not s.

    Two ``nca_vol_softskel`` and two ``nca_vol_overlap_sums`` calls (f64 sums in a fixed order: the same bits on every run); nothing is
    read back.  Not differentiable."""
    who = "cldice"
    if threshold is None and pred_threshold is not None:
        raise _capi.NcaError("cldice: pred_threshold is given without threshold")
    pthr = threshold if pred_threshold is None else pred_threshold
    K = _skel_iterations(iterations, who)
    p, t = _skel_input(pred, pthr, who, "pred"), _skel_input(truth, threshold, who, "truth")
    if p.shape != t.shape:
        raise _capi.NcaError(f"{who} takes two stacks of one shape, got {tuple(p.shape)} and {tuple(t.shape)}")
    if p.device != t.device:
        raise _capi.NcaError(f"{who}: pred lives on {p.device}, truth on {t.device}")
    lead = p.shape[:-3]
    a = _overlap_sums(soft_skeleton(p, K), t, who)
    b = _overlap_sums(soft_skeleton(t, K), p, who)
    out = _cldice_of_sums(a[:, 0], a[:, 1], b[:, 0], b[:, 1], smooth)
    return {k: v.reshape(lead) for k, v in out.items()}


# ----------------------------------------------------------------------------- connected components
def _connectivity(connectivity, who):
    c = int(connectivity)
    if c != connectivity or isinstance(connectivity, bool) or c not in (1, 2, 3):
        raise _capi.NcaError(f"{who}: connectivity = {connectivity!r} is not 1, 2 or 3 (6, 18 or 26 neighbours)")
    return c


def _keep_rule(k, min_size, who):
    """(k, min_size) with exactly one of them deciding: ``min_size`` when given (``k`` must then be left at 1), else ``k >= 1``."""
    if min_size is not None:
        m = int(min_size)
        if k != 1:
            raise _capi.NcaError(f"{who}: k = {k!r} and min_size = {min_size!r} are both given: one of them decides")
        if m != min_size or isinstance(min_size, bool) or m < 1:
            raise _capi.NcaError(f"{who}: min_size = {min_size!r} is not a whole number >= 1")
        return None, m
    n = int(k)
    if n != k or isinstance(k, bool) or n < 1:
        raise _capi.NcaError(f"{who}: k = {k!r} is not a whole number >= 1")
    return n, None


@torch.no_grad()
def label(vol: torch.Tensor, *, threshold: float, connectivity: int = 1, invert: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The connected components of ``M = vol > threshold`` (``~(vol > threshold)`` with ``invert``) of every volume of the f32 stack
    ``vol`` ``[..., n0, n1, n2]`` on the device: ``(labels, counts)`` with ``labels`` int32 of the same shape -- the component's number
    ``1 .. count`` on the mask, 0 elsewhere -- and ``counts`` int64 of the leading shape.  A bool mask is accepted too, with a ``threshold``
    in [0, 1).  A NaN value is not ``> threshold``.

    Two nodes of the mask are neighbours when they differ by at most 1 along every axis and in at most ``connectivity`` axes: 1 / 2 / 3
    gives 6 / 18 / 26 neighbours (``scipy.ndimage.generate_binary_structure(3, connectivity)``; the default is scipy's).  The components of
    a volume are numbered in increasing order of their smallest linear node index.  This is
    ``scipy.ndimage.label(vol > threshold, generate_binary_structure(3, connectivity))``, numbering included, for every volume on its own.

    One ``nca_vol_label`` (six launches: a union-find in LDS per tile, the unions across tiles, flattening, the ranking of the roots, the
    relabelling; the definition is in include/nerfca_hip.h, "label").  The result is a function of the mask alone: the same bits on every
    run.  Nothing is read back.  Not differentiable.  A volume of more than 2^31 - 2 nodes is refused."""
    who = "label"
    x_in = _skel_input(vol, None, who)          # refused before the threshold is looked at
    threshold = _view.finite_threshold(threshold, who)
    conn = _connectivity(connectivity, who)
    desc, x, n_vol, _ = _view.volume_stack(x_in, who)
    labels = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    counts = torch.empty((n_vol,), dtype=torch.int32, device=x.device)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_label_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_label, lib.nca_vol_label, x.device, C.byref(desc), _capi.ptr(x), n_vol, threshold, conn, 1 if invert else 0, _capi.ptr(labels),
                 _capi.ptr(counts), _capi.ptr(work), nbytes)
    return labels.reshape(vol.shape), counts.to(torch.int64).reshape(vol.shape[:-3])


def _check_labels(labels, counts, who):
    if not isinstance(labels, torch.Tensor) or not isinstance(counts, torch.Tensor):
        raise _capi.NcaError(f"{who}: labels and counts are tensors, as label returns them")
    if labels.dtype != torch.int32 or labels.dim() < 3 or labels.numel() == 0:
        raise _capi.NcaError(f"{who} takes int32 labels [..., n0, n1, n2], got {labels.dtype} {tuple(labels.shape)}")
    if counts.dtype != torch.int64 or counts.shape != labels.shape[:-3]:
        raise _capi.NcaError(f"{who}: counts is int64 of the leading shape {tuple(labels.shape[:-3])}, got {counts.dtype} {tuple(counts.shape)}")
    if counts.device != labels.device:
        raise _capi.NcaError(f"{who}: labels live on {labels.device}, counts on {counts.device}")


@torch.no_grad()
def component_sizes(labels: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """The node count of every component: int64 ``[..., max_count + 1]`` from the ``(labels, counts)`` of ``label``.  Entry 0 is the
    background, entry ``l`` the component numbered ``l``; entries past a volume's own count are 0.  A stack with no component at all returns
    the single background column.  Reading ``counts.max()`` is the one host sync; then one ``nca_vol_label_sizes`` (integer atomics, merged
    per wave and per workgroup first: exact in any order)."""
    who = "component_sizes"
    _check_labels(labels, counts, who)
    _fused._require_cuda(labels, "labels")
    lead, shape = labels.shape[:-3], tuple(labels.shape[-3:])
    x = labels.reshape((-1,) + shape).contiguous()
    cap = int(counts.max()) + 1
    if cap < 1:
        raise _capi.NcaError(f"{who}: counts holds a negative count")
    desc = _capi.grid_desc(shape, tuple((0.0, float(n - 1)) for n in shape))
    sizes = torch.empty((x.shape[0], cap), dtype=torch.int32, device=x.device)
    _view.launch(_capi.check_label, _capi.lib().nca_vol_label_sizes, x.device, C.byref(desc), _capi.ptr(x), x.shape[0], cap, _capi.ptr(sizes))
    return sizes.to(torch.int64).reshape(lead + (cap,))


@torch.no_grad()
def largest_components(labels: torch.Tensor, sizes: torch.Tensor, k: int = 1, *, min_size: Optional[int] = None) -> torch.Tensor:
    """The selection of ``keep_largest`` from ``labels`` ``[..., n0, n1, n2]`` (any integer dtype) and their ``sizes`` ``[..., cap]`` as
    ``component_sizes`` returns them: the bool mask of the nodes whose component is among the ``k`` largest of its volume (ties go to the
    smaller label; a volume with fewer components keeps all), or, with ``min_size``, has at least that many nodes.  Plain torch on whatever
    device the tensors live on."""
    who = "keep_largest"
    k, min_size = _keep_rule(k, min_size, who)
    if labels.dim() < 3 or sizes.dim() != labels.dim() - 2 or sizes.shape[:-1] != labels.shape[:-3]:
        raise _capi.NcaError(f"{who}: labels {tuple(labels.shape)} and sizes {tuple(sizes.shape)} do not belong together")
    cap = sizes.shape[-1]
    s = sizes.reshape(-1, cap).to(torch.int64)
    comp = s[:, 1:]
    if min_size is not None:
        keep_comp = comp >= min_size
    else:
        order = torch.sort(comp, dim=1, descending=True, stable=True)[1]          # stable: among equal sizes the smaller label comes first
        keep_comp = torch.zeros_like(comp, dtype=torch.bool)
        keep_comp.scatter_(1, order[:, :k], True)
        keep_comp &= comp > 0          # a number no node carries
    keep = torch.cat([torch.zeros((s.shape[0], 1), dtype=torch.bool, device=s.device), keep_comp], dim=1)
    flat = labels.reshape(s.shape[0], -1).to(torch.int64)
    return torch.gather(keep, 1, flat).reshape(labels.shape)


@torch.no_grad()
def keep_largest(vol: torch.Tensor, k: int = 1, *, threshold: float, connectivity: int = 3, min_size: Optional[int] = None) -> torch.Tensor:
    """The mask ``vol > threshold`` of an f32 stack ``[..., n0, n1, n2]`` on the device (or a bool mask, ``threshold`` in [0, 1)) reduced to
    the ``k`` largest components of every volume, as a bool tensor of the same shape: the usual cleanup of a thresholded vessel before a
    surface distance.  Components are those of ``label`` at ``connectivity`` (26 neighbours by default: a vessel one node wide may run
    diagonally).  Ties in size go to the smaller label -- the component that comes first in raster order -- so the result is the same on
    every run.  A volume with fewer than ``k`` components keeps all of them.  With ``min_size`` every component of at least that many nodes
    is kept instead, however many there are.  Exactly one of the two decides: ``min_size`` together with a ``k`` other than 1, or
    ``k < 1``, is refused.

    ``label``, ``component_sizes`` (one host sync for the largest count) and a sort of the sizes in torch."""
    who = "keep_largest"
    _keep_rule(k, min_size, who)          # refused before anything runs
    labels, counts = label(_skel_input(vol, None, who), threshold=threshold, connectivity=connectivity)
    return largest_components(labels, component_sizes(labels, counts), k, min_size=min_size)


@torch.no_grad()
def component_report_reductions(counts_pred: torch.Tensor, sizes_pred: torch.Tensor, counts_truth: torch.Tensor, sizes_truth: torch.Tensor) -> dict:
    """The reductions of ``component_report`` from the ``counts`` ``[...]`` and ``sizes`` ``[..., cap]`` of the two stacks (the two caps may
    differ): plain torch on whatever device the tensors live on."""
    if counts_pred.shape != counts_truth.shape or sizes_pred.shape[:-1] != counts_pred.shape or sizes_truth.shape[:-1] != counts_truth.shape:
        raise _capi.NcaError(f"component_report: counts {tuple(counts_pred.shape)}, {tuple(counts_truth.shape)} and sizes {tuple(sizes_pred.shape)}, "
                             f"{tuple(sizes_truth.shape)} do not belong together")

    def share(sizes):
        comp = sizes[..., 1:].to(torch.int64)
        total = comp.sum(dim=-1)
        top = comp.amax(dim=-1) if comp.shape[-1] else torch.zeros_like(total)
        nan = torch.full((), math.nan, dtype=torch.float64, device=sizes.device)
        return torch.where(total == 0, nan, top.double() / total.double())

    cp, ct = counts_pred.to(torch.int64), counts_truth.to(torch.int64)
    return {"components_pred": cp, "components_truth": ct, "betti0_error": (cp - ct).abs(), "largest_share_pred": share(sizes_pred),
            "largest_share_truth": share(sizes_truth)}


@torch.no_grad()
def component_report(pred: torch.Tensor, truth: torch.Tensor, *, threshold: float, pred_threshold: Optional[float] = None, connectivity: int = 3) -> dict:
    """Is the prediction one tree, or a tree plus speckle?  For the masks ``pred > pred_threshold`` (``threshold`` when ``pred_threshold`` is
    ``None``) and ``truth > threshold`` of two f32 stacks ``[..., n0, n1, n2]`` of one shape on the device (bool masks are accepted), per
    volume, as device tensors of the leading shape:

        ``components_pred``, ``components_truth``     the component counts of ``label`` at ``connectivity`` (i64),
        ``betti0_error``                              their absolute difference, the Betti-0 error reported beside clDice (i64),
        ``largest_share_pred``, ``largest_share_truth``   the nodes of the largest component over the nodes of the mask (f64; NaN for an
                                                      empty mask): 1 for a single tree, lower the more of the mask is debris.

    Two ``label`` and two ``component_sizes`` calls (one host sync each)."""
    who = "component_report"
    p, t = _skel_input(pred, None, who, "pred"), _skel_input(truth, None, who, "truth")
    if p.shape != t.shape:
        raise _capi.NcaError(f"{who} takes two stacks of one shape, got {tuple(p.shape)} and {tuple(t.shape)}")
    if p.device != t.device:
        raise _capi.NcaError(f"{who}: pred lives on {p.device}, truth on {t.device}")
    pthr = threshold if pred_threshold is None else pred_threshold
    lp, cp = label(p, threshold=pthr, connectivity=connectivity)
    lt, ct = label(t, threshold=threshold, connectivity=connectivity)
    return component_report_reductions(cp, component_sizes(lp, cp), ct, component_sizes(lt, ct))
