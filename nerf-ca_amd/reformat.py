"""Vessel cross-sections and lumen profiles along a centreline, on the device: what quantitative coronary analysis reads off a
reconstruction.

``frames`` (host, numpy f64) turns an ordered point list -- a path of ``centreline.extract``, or ``phantom.centreline_points`` of a segment
table -- into equally spaced origins with a rotation-minimising frame.  ``cross_sections`` gathers one small oblique plane per frame from
every volume of a stack (``nca_vol_sample_planes``): the straightened reformation, whose centre column is the curved-planar image.
``lumen_profile`` shoots a fan of rays in every plane to the first crossing of a density level (``nca_vol_lumen``): the radius per
direction, the area, the smallest and largest diameter.  The definition of both, operation by operation, is in include/nerfca_hip.h,
"cpr".  ``stenosis`` is plain torch on a profile; ``along`` runs the three on every path of a ``centreline.Centreline``.  There is no
torch implementation behind the kernels and no CPU path; nothing here is differentiable.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _capi
from . import _view
from . import ccta as _ccta

MAX_ANGLES = 1024          # NCA_CPR_MAX_ANGLES
STATUS_CENTRE, STATUS_OPEN, STATUS_GRID = 1, 2, 4          # NCA_CPR_STATUS_*


class Frames(NamedTuple):
    """``K`` planes along a curve, numpy f64: ``origin`` ``[K, 3]``, the unit ``tangent`` ``[K, 3]``, the plane's axes ``e1`` and
    ``e2 = tangent x e1`` ``[K, 3]``, and the arclength ``s`` ``[K]`` of every origin from the first point."""
    origin: np.ndarray
    tangent: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    s: np.ndarray


class LumenProfile(NamedTuple):
    """Of a stack ``[..., n0, n1, n2]`` and ``K`` planes: ``radius`` f32 ``[..., K, n_angles]``; ``area``, ``d_min``, ``d_max`` and
    ``d_eq = 2 sqrt(area / pi)`` f64 ``[..., K]``; ``status`` int32 ``[..., K]`` (bit 1: the plane's centre is not in the lumen; bit 2: a ray
    reached ``r_max`` without a crossing; bit 4: a ray left the grid); ``s`` f64 ``[K]``, the planes' arclength, on the device."""
    radius: torch.Tensor
    area: torch.Tensor
    d_min: torch.Tensor
    d_max: torch.Tensor
    d_eq: torch.Tensor
    status: torch.Tensor
    s: torch.Tensor


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(a):
    return a / np.sqrt(_dot(a, a))[..., None]


def frames(points, *, step: Optional[float] = None, smooth: int = 0, up=None) -> Frames:
    """Equally spaced planes along the polyline ``points`` ``[N, 3]`` (a tensor, an array or a list; world coordinates).  On the host in
    numpy f64, deterministic, in this order:

    - a point equal to the one before it is dropped; fewer than two distinct points are refused;
    - ``smooth`` passes of the 1-2-1 filter ``((p[i-1] + 2 p[i]) + p[i+1]) / 4`` with both ends fixed (a TEASAR path is voxel-jagged);
    - resampling by linear interpolation at the arclengths ``s_k = k step``, ``k = 0 .. floor(L / step + 1e-9)``, ``L`` the polyline's
      length; ``step`` defaults to the mean segment length ``L / (N - 1)``; a ``step`` that leaves fewer than two planes is refused;
    - tangents by central differences ``p[k+1] - p[k-1]``, one-sided at the ends, normalised;
    - a rotation-minimising frame by the double-reflection method (Wang, Juettler, Zheng and Liu, "Computation of rotation minimizing
      frames", ACM TOG 2008), re-orthonormalised against the tangent at every step; it starts from ``up`` projected off the first
      tangent, or, with ``up=None``, from the coordinate axis least aligned with the first tangent (the first such axis on a tie);
      ``e2 = tangent x e1``."""
    who = "frames"
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu().numpy()
    try:
        p = np.array(points, dtype=np.float64)
    except (TypeError, ValueError):
        raise _capi.NcaError(f"{who}: points is not an array of numbers") from None
    if p.ndim != 2 or p.shape[1] != 3:
        raise _capi.NcaError(f"{who}: points is [N, 3], got {tuple(p.shape)}")
    if not np.isfinite(p).all():
        raise _capi.NcaError(f"{who}: points holds a value that is not finite")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0:
        raise _capi.NcaError(f"{who}: smooth = {smooth!r} is not a whole number >= 0")
    if p.shape[0] > 1:
        p = p[np.concatenate([[True], (p[1:] != p[:-1]).any(axis=1)])]
    if p.shape[0] < 2:
        raise _capi.NcaError(f"{who}: {p.shape[0]} distinct points: at least two are needed")
    for _ in range(int(smooth)):
        q = p.copy()
        q[1:-1] = ((p[:-2] + 2.0 * p[1:-1]) + p[2:]) / 4.0
        p = q
    d = p[1:] - p[:-1]
    seg = np.sqrt(_dot(d, d))
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    length = float(cum[-1])
    if not length > 0.0:
        raise _capi.NcaError(f"{who}: the smoothed polyline has no length")
    if step is None:
        step = length / (p.shape[0] - 1)
    step = float(step)
    if not (math.isfinite(step) and step > 0.0):
        raise _capi.NcaError(f"{who}: step = {step!r} is not finite and positive")
    count = int(math.floor(length / step + 1e-9)) + 1
    if count < 2:
        raise _capi.NcaError(f"{who}: step = {step!r} is longer than the polyline ({length!r}): fewer than two planes")
    s = np.minimum(np.arange(count).astype(np.float64) * step, length)
    idx = np.clip(np.searchsorted(cum, s, side="right") - 1, 0, p.shape[0] - 2)
    live = seg[idx] > 0.0
    t = np.where(live, (s - cum[idx]) / np.where(live, seg[idx], 1.0), 0.0)
    origin = p[idx] + t[:, None] * (p[idx + 1] - p[idx])
    tan = np.empty_like(origin)
    tan[1:-1] = origin[2:] - origin[:-2]
    tan[0] = origin[1] - origin[0]
    tan[-1] = origin[-1] - origin[-2]
    norm = np.sqrt(_dot(tan, tan))
    if not (norm > 0.0).all():
        raise _capi.NcaError(f"{who}: the resampled curve has a zero tangent at plane {int(np.argmin(norm))} (it folds back onto itself)")
    tan = tan / norm[:, None]
    if up is None:
        start = np.zeros(3)
        start[int(np.argmin(np.abs(tan[0])))] = 1.0
    else:
        try:
            start = np.array(up, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise _capi.NcaError(f"{who}: up is not a vector of three numbers") from None
        if start.shape != (3,) or not np.isfinite(start).all():
            raise _capi.NcaError(f"{who}: up = {up!r} is not a vector of three finite numbers")
    r = start - _dot(start, tan[0]) * tan[0]
    if not math.sqrt(float(_dot(r, r))) > 1e-8 * max(math.sqrt(float(_dot(start, start))), 1e-300):
        raise _capi.NcaError(f"{who}: up = {up!r} is parallel to the first tangent")
    e1 = np.empty_like(origin)
    e1[0] = _unit(r)
    for i in range(count - 1):
        v1 = origin[i + 1] - origin[i]
        c1 = _dot(v1, v1)
        rl = e1[i] - (2.0 / c1 * _dot(v1, e1[i])) * v1
        tl = tan[i] - (2.0 / c1 * _dot(v1, tan[i])) * v1
        v2 = tan[i + 1] - tl
        c2 = _dot(v2, v2)
        rn = rl - (2.0 / c2 * _dot(v2, rl)) * v2 if c2 > 0.0 else rl
        e1[i + 1] = _unit(rn - _dot(rn, tan[i + 1]) * tan[i + 1])
    return Frames(origin, tan, e1, _cross(tan, e1), s)


def to_device(frames: Frames, device) -> Frames:
    """The same frames with every field an f64 tensor on ``device``.  ``cross_sections`` and ``lumen_profile`` upload host frames on every
    call (a host-to-device copy, which a graph capture refuses); frames that are on the device already are used as they are, so a call
    with them can be captured."""
    if not isinstance(frames, Frames):
        raise _capi.NcaError("to_device: frames is not a Frames, as reformat.frames returns it")
    return Frames(*(f if isinstance(f, torch.Tensor) and f.device == torch.device(device) else
                    torch.as_tensor(np.ascontiguousarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f, dtype=np.float64)).to(device) for f in frames))


def _plane_vectors(fr, dev, who):
    """(K, origin, e1, e2) with the three as contiguous f64 [K, 3] tensors on ``dev``"""
    if not isinstance(fr, Frames):
        raise _capi.NcaError(f"{who}: frames is not a Frames, as reformat.frames returns it")
    out, k = [], None
    for name in ("origin", "e1", "e2"):
        a = getattr(fr, name)
        shape, dtype = (tuple(a.shape), a.dtype) if isinstance(a, (np.ndarray, torch.Tensor)) else ((), None)
        if k is None and len(shape) == 2:
            k = shape[0]
        if dtype not in (np.float64, torch.float64) or shape != (k, 3) or k == 0:
            raise _capi.NcaError(f"{who}: frames.{name} is f64 [K, 3] with K >= 1, got {dtype} {shape}")
        if isinstance(a, torch.Tensor):
            if a.device != dev:
                raise _capi.NcaError(f"{who}: frames.{name} is on {a.device}, the volumes are on {dev}")
            out.append(a.detach().contiguous())
        else:
            out.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return (k,) + tuple(out)


_DIRS = {}          # (n_angles, device) -> dirs on the device: uploaded once, so that a later call makes no copy


def _directions_on(n_angles, dev):
    key = (n_angles, str(dev))
    if key not in _DIRS:
        _DIRS[key] = torch.from_numpy(directions(n_angles)).to(dev)
    return _DIRS[key]


def _positive(value, name, who):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise _capi.NcaError(f"{who}: {name} = {value!r} is not a number") from None
    if not (math.isfinite(value) and value > 0.0):
        raise _capi.NcaError(f"{who}: {name} = {value!r} is not finite and positive")
    return value


def _pair(value, name, who):
    if isinstance(value, (tuple, list, np.ndarray)):
        if len(value) != 2:
            raise _capi.NcaError(f"{who}: {name} = {value!r} is neither one value nor one per axis of the plane")
        return value[0], value[1]
    return value, value


def _count(value, name, who):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise _capi.NcaError(f"{who}: {name} = {value!r} is not a positive integer")
    return int(value)


@torch.no_grad()
def cross_sections(vol: torch.Tensor, bounds, frames: Frames, *, size, spacing, order: int = 1, fill: float = 0.0) -> torch.Tensor:
    """The planes of ``frames`` through every volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` on the device, whose nodes are
    ``linspace(lo, hi, n)`` on each axis of ``bounds`` (``None``: node units): an f32 tensor ``[..., K, nu, nv]``.  ``size`` is ``nu`` =
    ``nv`` or ``(nu, nv)``, ``spacing`` the pixel size in world units (one value or ``(du, dv)``).  Pixel ``(i, j)`` of plane ``k`` lies at
    ``origin[k] + (i - (nu - 1) / 2) du e1[k] + (j - (nv - 1) / 2) dv e2[k]``; a pixel outside the grid is ``fill``.

    This is the STRAIGHTENED reformation: the planes stacked along the arclength ``frames.s``.  Its centre column ``[..., :, :, nv // 2]`` --
    arclength by the ``e1`` axis through the centreline -- is the curved-planar image (with an odd ``nv``).

    ``order=0``: the nearest node, exact.  ``order=1``: trilinear in f64, rounded once.  ``order=3``: the cubic spline of ``ccta.zoom``:
    ``ccta.spline_filter`` runs first (an axis longer than 512 nodes is refused) and its coefficients are sampled with the mirror boundary.
    One ``nca_vol_sample_planes``: a pixel's coordinates, taps and weights are formed once for all volumes; the same bits on every run; no
    host read.  Not differentiable."""
    who = "cross_sections"
    if isinstance(order, bool) or order not in (0, 1, 3):
        raise _capi.NcaError(f"{who}: order = {order!r} is not 0, 1 or 3")
    nu, nv = (_count(v, "size", who) for v in _pair(size, "size", who))
    du, dv = (_positive(v, "spacing", who) for v in _pair(spacing, "spacing", who))
    try:
        fill = float(fill)
    except (TypeError, ValueError):
        raise _capi.NcaError(f"{who}: fill = {fill!r} is not a number") from None
    if not isinstance(frames, Frames):
        raise _capi.NcaError(f"{who}: frames is not a Frames, as reformat.frames returns it")
    desc, x, n_vol, _ = _view.volume_stack(vol, who, bounds)
    dev = x.device
    k, origin, e1, e2 = _plane_vectors(frames, dev, who)
    src = _ccta.spline_filter(x) if order == 3 else x
    out = torch.empty((n_vol, k, nu, nv), dtype=torch.float32, device=dev)
    _view.launch(_capi.check_cpr, _capi.lib().nca_vol_sample_planes, dev, C.byref(desc), n_vol, _capi.ptr(src), int(order), k, _capi.ptr(origin), _capi.ptr(e1),
                 _capi.ptr(e2), nu, nv, du, dv, fill, _capi.ptr(out))
    return out.reshape(tuple(vol.shape[:-3]) + (k, nu, nv))


def directions(n_angles: int) -> np.ndarray:
    """f64 ``[n_angles, 2]``: ``(cos, sin)`` of ``2 pi a / n_angles`` from ``math.cos`` / ``math.sin``, what ``nca_vol_lumen`` takes as ``dirs``."""
    return np.array([[math.cos(2.0 * math.pi * a / n_angles), math.sin(2.0 * math.pi * a / n_angles)] for a in range(n_angles)], dtype=np.float64)


@torch.no_grad()
def lumen_profile(vol: torch.Tensor, bounds, frames: Frames, *, level: float, r_max: float, n_angles: int = 64, dr: Optional[float] = None) -> LumenProfile:
    """The lumen of every volume of the f32 stack ``vol`` ``[..., n0, n1, n2]`` in every plane of ``frames``: ``n_angles`` rays (even,
    4 .. 1024) leave the plane's origin in the directions ``cos e1 + sin e2`` and stop where the trilinear value first fails to exceed
    ``level``; the crossing is placed by linear interpolation between the two samples around it.  Samples lie ``dr`` apart (default: half
    the smallest grid spacing) up to ``ceil(r_max / dr)`` steps.  ``area`` is that of the polygon through the ray ends, ``d_min`` and
    ``d_max`` the smallest and largest sum of two opposite radii, ``d_eq = 2 sqrt(area / pi)``.  ``status`` is 0 for a plane whose rays all
    found a crossing inside the grid.

    One ``nca_vol_lumen``; the same bits on every run; no host read.  Not differentiable."""
    who = "lumen_profile"
    n_angles = _count(n_angles, "n_angles", who)
    if n_angles < 4 or n_angles % 2 or n_angles > MAX_ANGLES:
        raise _capi.NcaError(f"{who}: n_angles = {n_angles} is not an even number in 4 .. {MAX_ANGLES}")
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise _capi.NcaError(f"{who}: level = {level!r} is not a number") from None
    if math.isnan(level):
        raise _capi.NcaError(f"{who}: level = nan is not a number")
    r_max = _positive(r_max, "r_max", who)
    if dr is not None:
        dr = _positive(dr, "dr", who)
    if not isinstance(frames, Frames):
        raise _capi.NcaError(f"{who}: frames is not a Frames, as reformat.frames returns it")
    desc, x, n_vol, _ = _view.volume_stack(vol, who, bounds)
    k, origin, e1, e2 = _plane_vectors(frames, x.device, who)
    dr = min(0.5 / desc.inv[a] for a in range(3)) if dr is None else dr
    steps = math.ceil(r_max / dr)
    if steps > 2 ** 31 - 1:
        raise _capi.NcaError(f"{who}: r_max = {r_max!r} at dr = {dr!r} makes {steps} steps, more than 2^31 - 1")
    n_steps = max(int(steps), 1)
    dev = x.device
    dirs = _directions_on(n_angles, dev)
    radius = torch.empty((n_vol, k, n_angles), dtype=torch.float32, device=dev)
    stats = torch.empty((n_vol, k, 4), dtype=torch.float64, device=dev)
    status = torch.empty((n_vol, k), dtype=torch.int32, device=dev)
    _view.launch(_capi.check_cpr, _capi.lib().nca_vol_lumen, dev, C.byref(desc), n_vol, _capi.ptr(x), k, _capi.ptr(origin), _capi.ptr(e1), _capi.ptr(e2), n_angles,
                 _capi.ptr(dirs), math.sin(2.0 * math.pi / n_angles), level, dr, n_steps, _capi.ptr(radius), _capi.ptr(stats), _capi.ptr(status))
    lead = tuple(vol.shape[:-3])
    stats = stats.reshape(lead + (k, 4))
    area = stats[..., 0]
    return LumenProfile(radius.reshape(lead + (k, n_angles)), area, stats[..., 1], stats[..., 2], 2.0 * torch.sqrt(area / math.pi), status.reshape(lead + (k,)),
                        frames.s if isinstance(frames.s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames.s, dtype=np.float64)).to(dev))


def stenosis(profile: LumenProfile, *, reference="median") -> List[dict]:
    """Per volume of a profile (the leading dimensions flattened) a dict: ``mld`` the minimal lumen diameter, the smallest ``d_eq`` over the
    planes of status 0, and ``mld_s`` its arclength (the first such plane); ``reference`` the reference diameter -- the median of ``d_eq``
    over those planes (the lower of the two middle values, as ``torch.median``), or the number given; ``diameter_stenosis`` =
    ``100 (1 - mld / reference)`` and ``area_stenosis`` = ``100 (1 - (mld / reference)^2)`` in percent; ``planes`` and ``excluded``, the
    planes counted and those left out because a status bit is set.  A volume without a plane of status 0 has ``None`` for the figures.
    Plain torch; this reads the device back."""
    who = "stenosis"
    if not isinstance(profile, LumenProfile):
        raise _capi.NcaError(f"{who}: profile is not a LumenProfile, as reformat.lumen_profile returns it")
    if isinstance(reference, str):
        if reference != "median":
            raise _capi.NcaError(f"{who}: reference = {reference!r} is neither \"median\" nor a diameter")
        ref = None
    else:
        ref = _positive(reference, "reference", who)
    k = profile.d_eq.shape[-1]
    d_eq = profile.d_eq.detach().reshape(-1, k).to(torch.float64).cpu()
    status = profile.status.detach().reshape(-1, k).cpu()
    s = profile.s.detach().to(torch.float64).cpu()
    out = []
    for d, st in zip(d_eq, status):
        ok = st == 0
        n = int(ok.sum())
        rec = {"mld": None, "mld_s": None, "reference": ref, "diameter_stenosis": None, "area_stenosis": None, "planes": n, "excluded": k - n}
        if n:
            at = int(torch.where(ok, d, torch.full_like(d, math.inf)).argmin())
            mld = float(d[at])
            r = float(d[ok].median()) if ref is None else ref
            rec.update(mld=mld, mld_s=float(s[at]), reference=r, diameter_stenosis=100.0 * (1.0 - mld / r), area_stenosis=100.0 * (1.0 - (mld / r) ** 2))
        out.append(rec)
    return out


def along(vol: torch.Tensor, bounds, centreline, *, level: float, r_max: float, size, spacing, order: int = 1, fill: float = 0.0, n_angles: int = 64,
          dr: Optional[float] = None, step: Optional[float] = None, smooth: int = 2, up=None, reference="median") -> List[dict]:
    """``frames``, ``cross_sections``, ``lumen_profile`` and ``stenosis`` of the stack ``vol`` on every path of ``centreline`` (a
    ``centreline.Centreline``; a path runs from its tip to where it joins the tree): a list with one dict per path, ``frames``,
    ``sections``, ``profile`` and ``stenosis``.  A path of fewer than two distinct points gives ``None``.  ``smooth`` defaults to 2 here:
    the paths are node lists."""
    who = "along"
    points = getattr(centreline, "points", None)
    if not isinstance(points, (list, tuple)):
        raise _capi.NcaError(f"{who}: centreline is not a Centreline, as centreline.extract returns it")
    out = []
    for pts in points:
        p = pts.detach().cpu().numpy().astype(np.float64) if isinstance(pts, torch.Tensor) else np.asarray(pts, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 2 or not (p[1:] != p[:-1]).any():
            out.append(None)
            continue
        fr = frames(p, step=step, smooth=smooth, up=up)
        prof = lumen_profile(vol, bounds, fr, level=level, r_max=r_max, n_angles=n_angles, dr=dr)
        out.append({"frames": fr, "sections": cross_sections(vol, bounds, fr, size=size, spacing=spacing, order=order, fill=fill), "profile": prof,
                    "stenosis": stenosis(prof, reference=reference)})
    return out
