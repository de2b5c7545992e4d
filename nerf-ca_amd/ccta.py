"""From a CT and a vessel segmentation to the two volumes that get projected, on the device: the preprocessing of the reference's
preprocess/preprocess_ccta.py:54-130 without scipy.ndimage and without a host copy (csrc/view/nca_filt.hip).

``gaussian_filter`` is ``scipy.ndimage.gaussian_filter`` with the ``reflect`` boundary (``nca_vol_smooth``: separable, f64 inside, one
rounding to f32).  ``cityblock_distance`` counts nodes along the axes to the nearest node above (or not above) a threshold
(``nca_vol_cityblock``); ``binary_dilation``, ``binary_erosion`` and ``mask_border`` are one such call and a comparison, for the
6-connected structure and any number of iterations.  Both definitions, operation by operation, are in include/nerfca_hip.h ("filt").
``vessel_contrast`` and ``prepare_ccta`` chain them with ``metrics.distance_transform`` into the reference's pipeline: a static attenuation
volume without the vessels and a dynamic vessel-contrast volume, in the shapes ``drr.project_sequence``, ``drr.volume_teacher`` and
``drr.fit_volumes`` take.  There is no torch implementation behind the kernels: without the library these functions raise.

``zoom`` is ``scipy.ndimage.zoom`` at order 3 (the cubic spline with its prefilter, ``spline_filter``) and order 0, ``resample`` brings a
volume on ``bounds`` to a target spacing with it, and ``prepare_ccta(resample=...)`` is the reference's resampling to unit spacing
(preprocess_ccta.py:57-60) before everything that counts in nodes (csrc/view/nca_resample.hip; the definition is in include/nerfca_hip.h,
"resample").  One deliberate difference from scipy: the last output node of an axis is always the last input node, where scipy writes 0
into the whole last plane for the size pairs at which its coordinate overshoots by one ulp (4 -> 188 nodes, about 4 % of all pairs).

``vesselness`` is the multi-scale Hessian tubeness of Frangi et al. (MICCAI 1998): per scale one ``gaussian_filter`` and one launch that
forms the scale-normalised Hessian, its eigenvalues (five sweeps of cyclic Jacobi in f64) and the tubeness of every node, merged over the
scales on the device; ``hessian_eigenvalues`` returns the sorted eigenvalues of one scale (csrc/view/nca_vess.hip; the definition,
operation by operation, is in include/nerfca_hip.h, "vess").  It asks what shape a node's neighbourhood has -- bright, thin along two axes,
long along the third -- where a threshold asks how dense the node is.

Not here: spline orders 1, 2, 4 and 5, ``grid_mode``, file readers, other boundary modes, other structuring elements; for the vesselness,
anisotropic spacing (everything counts in nodes: bring the volume to an isotropic grid with ``resample`` first), dark and bright tubes in
one call, the 2-D filter; gradients of any of it.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from . import _view
from . import fused as _fused
from . import metrics as _metrics

MAX_RADIUS = 32          # NCA_SMOOTH_MAX_RADIUS
MAX_AXIS = 512           # NCA_EDT_MAX_AXIS: the city-block transform and the spline prefilter stage whole lines

MU_WATER = 0.1494 * 2.5e-2
MU_AIR = 0.0430 * 2.5e-2


def gaussian_weights(sigma: float, radius: Optional[int] = None, truncate: float = 4.0) -> np.ndarray:
    """The half-weights ``w[0 .. r]`` (``w[0]`` the centre) of scipy's Gaussian kernel, numpy f64: ``phi = exp(-0.5 / sigma^2 x^2)`` at
    ``x = -r .. r`` divided by its sum, with ``r = radius`` or ``int(truncate sigma + 0.5)``.  The right half is mirrored from the left, so the
    kernel is symmetric bit for bit.  ``sigma <= 1e-15`` gives ``[1.0]``: scipy leaves such an axis as it is."""
    sigma, truncate = float(sigma), float(truncate)
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise _capi.NcaError(f"gaussian_weights: sigma = {sigma} is not finite and non-negative")
    if not sigma > 1e-15:
        return np.ones(1, dtype=np.float64)
    if radius is None:
        if not (math.isfinite(truncate) and truncate >= 0.0):
            raise _capi.NcaError(f"gaussian_weights: truncate = {truncate} is not finite and non-negative")
        r = int(truncate * sigma + 0.5)
    else:
        r = int(radius)
        if r != radius or r < 0:
            raise _capi.NcaError(f"gaussian_weights: radius = {radius} is not a non-negative whole number")
    if r > MAX_RADIUS:
        raise _capi.NcaError(f"gaussian_weights: radius = {r} is larger than {MAX_RADIUS} (sigma = {sigma}, truncate = {truncate})")
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[:r + 1][::-1])          # x = 0, -1, .., -r


def _per_axis(value, name, who):
    if isinstance(value, (tuple, list, np.ndarray)):
        if len(value) != 3:
            raise _capi.NcaError(f"{who}: {name} is a scalar or one value per axis, got {value!r}")
        return list(value)
    return [value] * 3


@torch.no_grad()
def gaussian_filter(vol: torch.Tensor, sigma, *, radius=None, truncate: float = 4.0) -> torch.Tensor:
    """``scipy.ndimage.gaussian_filter(vol.astype(f64), sigma, radius=radius, truncate=truncate, mode="reflect").astype(f32)`` of every
    volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device, bit for bit: an f32 tensor of the same shape.  ``sigma`` and
    ``radius`` are a scalar or one value per axis, in nodes; an axis with ``sigma <= 1e-15`` is left as it is.  A radius above 32 is refused.

    One ``nca_vol_smooth`` (three launches, f64 intermediates; the summation order is part of the definition in include/nerfca_hip.h,
    "filt"): the same bits on every run.  Not differentiable: it runs under ``no_grad`` and the result is detached."""
    _view.check_volume(vol, "gaussian_filter")          # refused before sigma and radius are looked at
    sig = _per_axis(sigma, "sigma", "gaussian_filter")
    rad = _per_axis(radius, "radius", "gaussian_filter")
    halves = [gaussian_weights(s, r, truncate) for s, r in zip(sig, rad)]
    desc, x, n_vol, _ = _view.volume_stack(vol, "gaussian_filter")
    out = torch.empty_like(x)
    c_radius = (C.c_int32 * 3)(*[len(h) - 1 for h in halves])
    flat = np.concatenate(halves)
    c_weights = (C.c_double * flat.size)(*flat.tolist())
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_smooth_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_filt, lib.nca_vol_smooth, x.device, C.byref(desc), _capi.ptr(x), n_vol, c_radius, c_weights, _capi.ptr(out), _capi.ptr(work), nbytes)
    return out.reshape(vol.shape)


@torch.no_grad()
def cityblock_distance(vol: torch.Tensor, *, threshold: float, inside: bool = False, border: bool = False) -> torch.Tensor:
    """The city-block (L1) distance in nodes, ``|d0| + |d1| + |d2|``, from every node of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on the
    device to the nearest node with ``vol > threshold`` (``inside=False``; 0 on the mask) or to the nearest node that is NOT ``> threshold``
    (``inside=True``; 0 off the mask): an int32 tensor of the same shape.  ``border=True`` counts the nodes just outside the grid as such
    nodes too.  A NaN value is not ``> threshold``.  A volume with no such node (and no border) is ``0x7fffffff`` everywhere; every volume is
    transformed on its own.  ``inside=False`` is ``scipy.ndimage.distance_transform_cdt(~(vol > threshold), metric="taxicab")``.

    One ``nca_vol_cityblock`` (three launches, exact in integers): the same bits on every run.  An axis longer than 512 nodes is refused."""
    _view.check_volume(vol, "cityblock_distance")          # refused before the threshold is looked at
    threshold = _view.finite_threshold(threshold, "cityblock_distance")
    desc, x, n_vol, _ = _view.volume_stack(vol, "cityblock_distance")
    out = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_cityblock_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_filt, lib.nca_vol_cityblock, x.device, C.byref(desc), _capi.ptr(x), n_vol, threshold, 1 if inside else 0, 1 if border else 0,
                 _capi.ptr(out), _capi.ptr(work), nbytes)
    return out.reshape(vol.shape)


def _mask_input(vol, who):
    """f32 on the device from an f32 stack or a bool mask (a mask becomes 0 / 1, which any threshold in [0, 1) separates)."""
    if isinstance(vol, torch.Tensor) and vol.dtype == torch.bool:
        _fused._require_cuda(vol, "vol")
        vol = vol.to(torch.float32)
    _view.check_volume(vol, who)
    return vol


def _iterations(iterations, who):
    n = int(iterations)
    if n != iterations or n < 1:
        raise _capi.NcaError(f"{who}: iterations = {iterations} is not a whole number >= 1 (the repeat-until-stable mode of scipy is not offered)")
    return n


@torch.no_grad()
def binary_dilation(vol: torch.Tensor, iterations: int = 1, *, threshold: float = 0.0) -> torch.Tensor:
    """``scipy.ndimage.binary_dilation(vol > threshold, iterations=iterations)`` with the default 6-connected structure, per volume of
    the stack ``[..., n0, n1, n2]`` (f32, or a bool mask) on the device: a bool tensor of the same shape.  One ``cityblock_distance`` and
    a comparison, ``distance <= iterations``, whatever the number of iterations."""
    n = _iterations(iterations, "binary_dilation")
    return cityblock_distance(_mask_input(vol, "binary_dilation"), threshold=threshold) <= n


@torch.no_grad()
def binary_erosion(vol: torch.Tensor, iterations: int = 1, *, threshold: float = 0.0) -> torch.Tensor:
    """``scipy.ndimage.binary_erosion(vol > threshold, iterations=iterations)`` (6-connected, ``border_value = 0``: the mask is eroded from
    the faces of the grid too), as a bool tensor: the distance to the nearest node off the mask or outside the grid is ``> iterations``."""
    n = _iterations(iterations, "binary_erosion")
    return cityblock_distance(_mask_input(vol, "binary_erosion"), threshold=threshold, inside=True, border=True) > n


@torch.no_grad()
def mask_border(vol: torch.Tensor, *, threshold: float) -> torch.Tensor:
    """The nodes of ``M = vol > threshold`` that one erosion removes, ``M & ~binary_erosion(M)``, as a bool tensor: the surface of a mask
    as MedPy's surface distances take it (connectivity 1).  A node of M on a face of the grid is a border node."""
    return cityblock_distance(_mask_input(vol, "mask_border"), threshold=threshold, inside=True, border=True) == 1


@torch.no_grad()
def spline_filter(vol: torch.Tensor) -> torch.Tensor:
    """The cubic B-spline coefficients of every volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device, the prefilter of
    ``zoom``: an f64 tensor of the same shape.  ``scipy.ndimage.spline_filter(vol, 3, output=float64)`` (mirror boundary) within ``2^-44`` of
    the largest ``|vol|``; bit for bit the definition in include/nerfca_hip.h ("resample"), the same bits on every run.

    One ``nca_vol_spline_filter`` (three launches; a thread owns a line).  An axis longer than 512 nodes is refused."""
    desc, x, n_vol, _ = _view.volume_stack(vol, "spline_filter")
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    _view.launch(_capi.check_resample, _capi.lib().nca_vol_spline_filter, x.device, C.byref(desc), _capi.ptr(x), n_vol, _capi.ptr(out))
    return out.reshape(vol.shape)


def _zoom_shape(shape, zoom, output_shape, who):
    if output_shape is not None:
        m = list(output_shape) if isinstance(output_shape, (tuple, list, np.ndarray)) else []
        if len(m) != 3 or any(int(v) != v for v in m):
            raise _capi.NcaError(f"{who}: output_shape = {output_shape!r} is not three whole numbers")
        m = [int(v) for v in m]
    else:
        if zoom is None:
            raise _capi.NcaError(f"{who}: zoom or output_shape is needed")
        fac = [float(v) for v in _per_axis(zoom, "zoom", who)]
        if any(not (math.isfinite(f) and f > 0.0) for f in fac):
            raise _capi.NcaError(f"{who}: zoom = {zoom!r} is not finite and positive")
        m = [int(round(n * f)) for n, f in zip(shape, fac)]          # Python's round, as scipy
    for a in range(3):
        if m[a] < 2:
            raise _capi.NcaError(f"{who}: axis {a} of the output would have {m[a]} nodes: at least 2 are needed (the input has {shape[a]})")
    return m


@torch.no_grad()
def zoom(vol: torch.Tensor, zoom=None, *, order: int = 3, output_shape=None) -> torch.Tensor:
    """``scipy.ndimage.zoom(vol, zoom, order=order)`` (``mode="constant"``, ``prefilter=True``, ``grid_mode=False``) of every volume of the
    f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device: an f32 tensor ``[..., m0, m1, m2]``.  ``zoom`` is a scalar or one factor per axis
    and ``m_a = int(round(n_a zoom_a))``; ``output_shape`` ``(m0, m1, m2)`` overrides it.  End nodes map to end nodes: output node ``o`` of an
    axis lies at ``o (n - 1) / (m - 1)`` on the input.

    ``order=3``: the cubic spline, its prefilter included.  Within ``ulp + 2^-44 max|vol|`` of scipy per node (the interpolation has scipy's
    bits, the prefilter is a few f64 units off) -- except that the last output node is always the last input node, where scipy writes 0
    into the last plane for the size pairs at which its coordinate overshoots.  ``order=0``: the nearest node, exact, NaN and infinities
    included.  Other orders are refused.  At order 3 an axis longer than 512 nodes is refused.

    One ``nca_vol_zoom``: the same bits on every run.  Not differentiable: it runs under ``no_grad`` and the result is detached."""
    who = "zoom"
    desc, x, n_vol, shape = _view.volume_stack(vol, who)
    if order not in (0, 3) or isinstance(order, bool):
        raise _capi.NcaError(f"{who}: order = {order!r} is neither 0 nor 3")
    m = _zoom_shape(shape, zoom, output_shape, who)
    out = torch.empty((n_vol,) + tuple(m), dtype=torch.float32, device=x.device)
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_zoom_workspace(C.byref(desc), n_vol, order))
    work = _view.workspace(nbytes, x.device)
    _view.launch(_capi.check_resample, lib.nca_vol_zoom, x.device, C.byref(desc), _capi.ptr(x), n_vol, (C.c_int32 * 3)(*m), int(order), _capi.ptr(out),
                 _capi.ptr(work), nbytes)
    return out.reshape(tuple(vol.shape[:-3]) + tuple(m))


def _zoom_factors(shape, bounds, spacing, who):
    """``((hi - lo) / (n - 1)) / spacing_a`` per axis: the grid's own spacing over the target's."""
    _capi.grid_desc(shape, bounds)          # refuses bad bounds
    target = [float(v) for v in _per_axis(spacing, "spacing", who)]
    if any(not (math.isfinite(s) and s > 0.0) for s in target):
        raise _capi.NcaError(f"{who}: spacing = {spacing!r} is not finite and positive")
    return [((float(b[1]) - float(b[0])) / (n - 1)) / s for b, n, s in zip(bounds, shape, target)], target


@torch.no_grad()
def resample(vol: torch.Tensor, bounds, spacing, *, order: int = 3):
    """The f32 stack ``vol`` ``[..., n0, n1, n2]`` on the grid of ``bounds`` brought to the node spacing ``spacing`` (a scalar or one value
    per axis, in the units of ``bounds``): ``(zoom(vol, factors, order=order), bounds)`` with the factors
    ``((hi - lo) / (n - 1)) / spacing_a``.  The bounds come back unchanged, since end nodes map to end nodes; as the node count is a whole
    number, the spacing of the result is ``(hi - lo) / (m_a - 1)``, the nearest to ``spacing_a`` that scipy's rule reaches."""
    who = "resample"
    _view.check_volume(vol, who)
    fac, _ = _zoom_factors(tuple(vol.shape[-3:]), bounds, spacing, who)
    return zoom(vol, fac, order=order), tuple((float(b[0]), float(b[1])) for b in bounds)


def _round_half_away(x):
    """What scipy's zoom writes into an integer array: ``trunc(x + 0.5)`` for ``x > 0``, else ``trunc(x - 0.5)``; as f64."""
    x = x.double()
    return torch.where(x > 0, x + 0.5, x - 0.5).trunc()


def hounsfield_to_attenuation(vol: torch.Tensor, mu_water: float = MU_WATER, mu_air: float = MU_AIR) -> torch.Tensor:
    """``vol / 1000 * (mu_water - mu_air) + mu_water`` (preprocess_ccta.py:7-12), formed in f64 and rounded to f32 once.  Plain torch, on
    whatever device ``vol`` lives on."""
    if not isinstance(vol, torch.Tensor):
        raise _capi.NcaError("hounsfield_to_attenuation: vol is not a tensor")
    return _attenuation64(vol, mu_water, mu_air).to(torch.float32)


def _attenuation64(vol, mu_water=MU_WATER, mu_air=MU_AIR):
    return vol.double() / 1000 * (float(mu_water) - float(mu_air)) + float(mu_water)


def _interp(x, xp, fp):
    """``np.interp(x, xp, fp)`` of an f64 tensor: clamped at both ends, ``slope (x - xp[j]) + fp[j]`` in between."""
    xp_t = torch.tensor(xp, dtype=torch.float64, device=x.device)
    fp_t = torch.tensor(fp, dtype=torch.float64, device=x.device)
    j = (torch.bucketize(x, xp_t, right=True) - 1).clamp(0, len(xp) - 2)
    slope = (fp_t[1:] - fp_t[:-1]) / (xp_t[1:] - xp_t[:-1])
    y = slope[j] * (x - xp_t[j]) + fp_t[j]
    y = torch.where(x >= xp_t[-1], fp_t[-1], y)
    return torch.where(x <= xp_t[0], fp_t[0], y)


@torch.no_grad()
def vessel_contrast(mask: torch.Tensor, bounds, *, grow: int = 3, shrink: int = 1, sigma=1.0, radius=2, xp: Sequence[float] = (0, 1, 2, 4, 5),
                    fp: Sequence[float] = (0, 0.2, 0.5, 0.75, 1), contrast: float = 0.05) -> Tuple[torch.Tensor, torch.Tensor]:
    """The vessel-contrast volume of preprocess_ccta.py:88-120 from a vessel segmentation ``mask`` ``[..., n0, n1, n2]`` (f32, or bool;
    a node belongs to it when ``> 0``) on the device: ``(contrast volume f32, closed mask bool)``.

    1. ``M = binary_erosion(binary_dilation(mask > 0, grow), shrink)``: the closed mask;
    2. ``metrics.distance_transform(M, bounds, threshold=0.5, inside=True)``: the depth of every node inside M, in the world units of
       ``bounds`` (the reference has resampled to unit spacing before this step);
    3. ``gaussian_filter(sigma, radius=radius)``;
    4. ``np.interp`` through ``(xp, fp * contrast)``, clamped at both ends, in f64 (``bucketize`` and a lerp), rounded to f32;
    5. 0 outside M.
    Steps 2 and 3 hand over f32 volumes where the reference keeps f64: the result is within
    ``s 2^-24 d_max + 2^-24 max(fp) contrast`` of it (s the largest slope of the transfer function, d_max the largest depth)."""
    who = "vessel_contrast"
    m = _mask_input(mask, who)
    xp, fp, contrast = [float(v) for v in xp], [float(v) for v in fp], float(contrast)
    if len(xp) != len(fp) or len(xp) < 2:
        raise _capi.NcaError(f"{who}: xp and fp are two lists of one length >= 2, got {len(xp)} and {len(fp)}")
    if any(not (math.isfinite(a) and math.isfinite(b)) for a, b in zip(xp, fp)) or any(not a < b for a, b in zip(xp, xp[1:])):
        raise _capi.NcaError(f"{who}: xp = {xp} is not finite and strictly increasing")
    if not math.isfinite(contrast):
        raise _capi.NcaError(f"{who}: contrast = {contrast} is not finite")
    closed = binary_erosion(binary_dilation(m, grow), shrink)
    depth = _metrics.distance_transform(closed.to(torch.float32), bounds, threshold=0.5, inside=True)
    smooth = gaussian_filter(depth, sigma, radius=radius)
    value = _interp(smooth.double(), xp, [v * contrast for v in fp]).to(torch.float32)
    return torch.where(closed, value, torch.zeros((), dtype=torch.float32, device=value.device)), closed


@torch.no_grad()
def prepare_ccta(raw_hu: torch.Tensor, vessel_mask: torch.Tensor, bounds, *, labels: Optional[torch.Tensor] = None, aorta_label: Optional[int] = None,
                 heart_label: Optional[int] = None, resample=None, label_order: int = 3, **vessel_kw) -> dict:
    """A CT in Hounsfield units ``raw_hu`` and a vessel segmentation ``vessel_mask``, both ``[P, n0, n1, n2]`` (or one volume
    ``[n0, n1, n2]``) on the device and on the grid of ``bounds``, to the pair of volumes that gets projected (preprocess_ccta.py:54-130):
    ``{"static", "dynamic", "mask", "bounds"}``.

    1. ``hounsfield_to_attenuation(raw_hu)``;
    1a. with ``resample`` (a target node spacing in the units of ``bounds``, a scalar or one value per axis; the reference's is 1): the
       attenuation is brought to that spacing with ``zoom`` at order 3, ``vessel_mask > 0`` and ``labels`` with ``zoom`` at ``label_order``
       (preprocess_ccta.py:57-60; the factors are those of ``resample``).  At ``label_order=3`` the two segmentations are then rounded half
       away from zero, which is what scipy does for the reference's integer arrays, and the mask is ``> 0`` after the rounding: a cubic
       spline through labels invents values between them; ``label_order=0`` takes the nearest node and invents none.  Everything below
       runs on the new grid, and like the reference (``spacing = (1, 1, 1)`` at :61) it takes the target spacing for the grid's own when it
       measures the depth inside the vessel; the returned ``bounds`` are the input's, since end nodes map to end nodes.
       ``resample=None``: no resampling, the volumes stay on the grid they came on;
    2. with ``labels`` (a segmentation of the same shape, any integer or float dtype): the nodes with ``labels == aorta_label`` get the mean
       (f64) of the nodes with ``labels == heart_label`` of the same volume -- NaN if that volume has no heart node, as numpy's mean;
    3. ``dynamic, mask = vessel_contrast(vessel_mask, bounds, **vessel_kw)``;
    4. ``static`` is the attenuation where the closed ``mask`` is False and 0 elsewhere.
    ``static + dynamic`` is the reference's ``full_volume``.  The reference zeroes its vessel-free volume (``raw-no-vessel``) with the
    segmentation as given; here the CLOSED mask is used, so that the pair sums to the full volume and no attenuation is counted twice
    under the contrast.  ``static[p]`` with ``dynamic`` (or ``dynamic[p:p+1]``) and ``bounds`` are what ``drr.project_sequence``,
    ``drr.volume_teacher`` and ``drr.fit_volumes`` take."""
    who = "prepare_ccta"
    _view.check_volume(raw_hu, who, "raw_hu")
    m = _mask_input(vessel_mask, who)
    if raw_hu.dim() not in (3, 4) or m.shape != raw_hu.shape or m.device != raw_hu.device:
        raise _capi.NcaError(f"{who} takes raw_hu and vessel_mask [P, n0, n1, n2] or [n0, n1, n2] of one shape on one device, got {tuple(raw_hu.shape)} and "
                             f"{tuple(m.shape)}")
    att = _attenuation64(raw_hu.detach())          # f64 until the aorta is filled in: one rounding to f32
    if labels is not None:
        if aorta_label is None or heart_label is None:
            raise _capi.NcaError(f"{who}: labels need aorta_label and heart_label")
        if not isinstance(labels, torch.Tensor) or labels.shape != raw_hu.shape or labels.device != raw_hu.device:
            raise _capi.NcaError(f"{who}: labels is a tensor of the shape and device of raw_hu, {tuple(raw_hu.shape)}")
    elif aorta_label is not None or heart_label is not None:
        raise _capi.NcaError(f"{who}: aorta_label and heart_label need labels")
    depth_bounds = bounds
    if resample is not None:
        if label_order not in (0, 3) or isinstance(label_order, bool):
            raise _capi.NcaError(f"{who}: label_order = {label_order!r} is neither 0 nor 3")
        fac, target = _zoom_factors(tuple(raw_hu.shape[-3:]), bounds, resample, who)

        def labels_to_grid(x):
            y = zoom(x, fac, order=label_order)
            return _round_half_away(y) if label_order == 3 else y

        att = zoom(att.to(torch.float32), fac, order=3).double()
        m = (labels_to_grid((m > 0).to(torch.float32)) > 0).to(torch.float32)
        if labels is not None:
            labels = labels_to_grid(labels.to(torch.float32))
        depth_bounds = tuple((float(b[0]), float(b[0]) + (n - 1) * s) for b, n, s in zip(bounds, att.shape[-3:], target))
    if labels is not None:
        heart, aorta = labels == heart_label, labels == aorta_label
        dims = (-3, -2, -1)
        mean = torch.where(heart, att, torch.zeros((), dtype=torch.float64, device=att.device)).sum(dim=dims, keepdim=True) / heart.sum(dim=dims, keepdim=True)
        att = torch.where(aorta, mean, att)
    dynamic, closed = vessel_contrast(m, depth_bounds, **vessel_kw)
    static = torch.where(closed, torch.zeros((), dtype=torch.float32, device=att.device), att.to(torch.float32))
    return {"static": static, "dynamic": dynamic, "mask": closed, "bounds": tuple((float(b[0]), float(b[1])) for b in bounds)}


def _vess_sigmas(sigmas, who):
    """The scales as floats: at least one, each finite and positive."""
    try:
        sig = [float(s) for s in sigmas]
    except TypeError:
        raise _capi.NcaError(f"{who}: sigmas = {sigmas!r} is not a sequence of numbers") from None
    if not sig:
        raise _capi.NcaError(f"{who}: sigmas is empty")
    for s in sig:
        if not (math.isfinite(s) and s > 0.0):
            raise _capi.NcaError(f"{who}: sigma = {s} is not finite and positive")
    return sig


def _vess_param(value, name, who, zero_ok=False):
    """alpha, beta (finite and positive) or c (finite and non-negative) as a float."""
    v = float(value)
    if not (math.isfinite(v) and (v > 0.0 or (zero_ok and v == 0.0))):
        raise _capi.NcaError(f"{who}: {name} = {v} is not finite and {'non-negative' if zero_ok else 'positive'}")
    return v


@torch.no_grad()
def hessian_eigenvalues(vol: torch.Tensor, sigma: float) -> torch.Tensor:
    """The eigenvalues of the scale-normalised Hessian ``sigma^2 d^2/dx_a dx_b gaussian_filter(vol, sigma)`` at every node of the f32 stack
    ``vol`` ``[..., n0, n1, n2]`` on the device, sorted by absolute value (the smaller value first on a tie): an f32 tensor
    ``[..., 3, n0, n1, n2]``.  Second differences in nodes with the edge values repeated, five sweeps of cyclic Jacobi in f64 (within
    ``2^-49`` of the matrix norm of LAPACK's), one rounding to f32; a node whose Hessian is not finite gets three NaN.

    One ``gaussian_filter`` and one ``nca_vol_hessian_eig``: the same bits on every run.  Not differentiable."""
    who = "hessian_eigenvalues"
    _view.check_volume(vol, who)
    sigma, = _vess_sigmas((sigma,), who)
    desc, x, n_vol, shape = _view.volume_stack(gaussian_filter(vol, sigma), who)
    out = torch.empty((n_vol, 3) + shape, dtype=torch.float32, device=x.device)
    _view.launch(_capi.check_vess, _capi.lib().nca_vol_hessian_eig, x.device, C.byref(desc), _capi.ptr(x), n_vol, sigma * sigma, _capi.ptr(out))
    return out.reshape(tuple(vol.shape[:-3]) + (3,) + shape)


@torch.no_grad()
def vesselness(vol: torch.Tensor, sigmas: Sequence[float] = (1.0, 2.0, 3.0), *, alpha: float = 0.5, beta: float = 0.5, c: Optional[float] = None,
               bright: bool = True, return_scale: bool = False):
    """The multi-scale Hessian vesselness of Frangi et al. (MICCAI 1998) of every volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on
    the device: an f32 tensor of the same shape with values in [0, 1], the largest response over ``sigmas`` (in nodes).  With
    ``return_scale`` also an int32 tensor of the same shape: the index into ``sigmas`` of the scale that gave it, the smallest on a tie.

    With the eigenvalues ``|l1| <= |l2| <= |l3|`` of ``hessian_eigenvalues(vol, sigma)`` a node responds only where ``l2 < 0`` and
    ``l3 < 0`` (``bright=False``: both ``> 0``, tubes darker than their surroundings):
    ``V = (1 - exp(-(l2 / l3)^2 / (2 alpha^2))) exp(-l1^2 / |l2 l3| / (2 beta^2)) (1 - exp(-(l1^2 + l2^2 + l3^2) / (2 c^2)))``.
    ``c=None`` is Frangi's rule, half the largest Hessian norm ``sqrt(l1^2 + l2^2 + l3^2)`` of each volume at each scale, formed on the
    device; ``c=0`` drops the last factor.  A node whose Hessian is not finite gets 0.

    Per scale one ``gaussian_filter(vol, sigma)`` (truncate 4: a sigma above 8.1 exceeds its radius limit of 32), one
    ``nca_vol_hessian_norm_max`` when ``c`` is None, and one ``nca_vol_vesselness``; nothing is read back to the host and the bits are the
    same on every run.  The spacing is taken as isotropic.  Not differentiable: it runs under ``no_grad`` and the result is detached."""
    who = "vesselness"
    _view.check_volume(vol, who)
    sig = _vess_sigmas(sigmas, who)
    alpha, beta = _vess_param(alpha, "alpha", who), _vess_param(beta, "beta", who)
    if c is not None:
        c = _vess_param(c, "c", who, zero_ok=True)
    desc, x, n_vol, shape = _view.volume_stack(vol, who)
    out = torch.empty_like(x)
    index = torch.empty(x.shape, dtype=torch.int32, device=x.device) if return_scale else None
    lib = _capi.lib()
    for i, sigma in enumerate(sig):
        s, scale = gaussian_filter(x, sigma), sigma * sigma
        if c is None:
            c_vol = torch.empty(n_vol, dtype=torch.float64, device=x.device)
            _view.launch(_capi.check_vess, lib.nca_vol_hessian_norm_max, x.device, C.byref(desc), _capi.ptr(s), n_vol, scale, _capi.ptr(c_vol))
            c_vol = 0.5 * torch.sqrt(c_vol)
        else:
            c_vol = torch.full((n_vol,), c, dtype=torch.float64, device=x.device)
        _view.launch(_capi.check_vess, lib.nca_vol_vesselness, x.device, C.byref(desc), _capi.ptr(s), n_vol, scale, alpha, beta, _capi.ptr(c_vol),
                     1 if bright else 0, i, _capi.ptr(out), _capi.ptr(index))
    out = out.reshape(vol.shape)
    return (out, index.reshape(vol.shape)) if return_scale else out
