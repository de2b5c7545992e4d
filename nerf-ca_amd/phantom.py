"""A procedural 4-D phantom with known 3-D truth (csrc/view/nca_phantom.hip): a static thorax of soft ellipsoids and a coronary tree of
thin tapered vessels that moves with the heart phase, rasterised on the device into the f32 grids ``drr``, ``export`` and
``synthetic.make_dataset(render=drr.volume_teacher(...))`` take.

The generator is host-side numpy and small: ``thorax`` makes a table of ellipsoids, ``coronary_tree`` / ``tree_at`` a table of segments
per heart phase.  ``voxelize`` is the device pass (``nca_phantom_voxelize``; its definition, operation by operation, is in
include/nerfca_hip.h, "phantom").  ``make_phantom`` puts them together for a C-arm geometry, and ``volume_errors`` compares a reconstructed
volume with the truth.  There is no torch implementation behind ``voxelize``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi
from . import _view

SEG_BATCH = 512          # NCA_PHANTOM_SEG_BATCH: the segments staged through LDS at once

# The default densities, in the units of the volumes drr projects (absorption per unit length).  Chosen so that, at
# synthetic.xcat_geometry with the four training views, every projected pixel stays above 0 and the largest vessel deficit is at least a
# tenth of the largest static one (tests/test_phantom_gpu.py holds both).
RHO_BODY, RHO_LUNG, RHO_HEART, RHO_SPINE = 1.0, -0.7, 0.3, 1.0
RHO_VESSEL = 12.0
HEART_AXES = (1.0, 0.85, 1.15)          # semi-axes of the uncontracted heart in units of heart_radius; the long axis is the last
HEART_EXTENT = max(HEART_AXES)          # every vessel point lies within HEART_EXTENT * heart_radius of the heart's centre
HEART_CENTER = (0.0, 0.2, 0.0)          # of make_phantom's heart, in units of the half width, from the isocentre
HEART_RADIUS = 0.25                     # of make_phantom's heart, in units of the half width


def fov_half_width(geo: dict) -> float:
    """Half the width of the field of view at the isocentre: ``0.5 nDetector dDetector DSO / DSD``, the smaller detector axis.  The
    volume bounds of ``drr`` default to +-1; a phantom is sized from the geometry (0.18 for ``synthetic.xcat_geometry``)."""
    return min(0.5 * float(n) * float(d) for n, d in zip(geo["nDetector"], geo["dDetector"])) * float(geo["DSO"]) / float(geo["DSD"])


def _ellipsoid(center, semi, w, rho):
    return np.concatenate([np.asarray(center, dtype=np.float64), np.diag(1.0 / np.asarray(semi, dtype=np.float64)).reshape(9), [float(w), float(rho)]])


def thorax(center: Sequence[float], half_width: float) -> np.ndarray:
    """f64 ``[5, 14]`` ellipsoid rows (centre, row-major matrix, soft width, density): body, two lungs (negative density: the table is
    additive), heart muscle, spine.  Axis 0 is left-right, axis 1 front-back, axis 2 head-foot.  With their soft shells all of them lie
    inside the cube of ``half_width`` around ``center``."""
    c = np.asarray(center, dtype=np.float64)
    hw = float(half_width)
    if c.shape != (3,) or not np.isfinite(c).all() or not (math.isfinite(hw) and hw > 0):
        raise _capi.NcaError(f"thorax takes a finite centre of three coordinates and a positive half width, got {center!r} and {half_width!r}")
    heart = c + hw * np.asarray(HEART_CENTER)
    rows = [_ellipsoid(c, hw * np.array([0.95, 0.70, 0.95]), 0.08, RHO_BODY),
            _ellipsoid(c + hw * np.array([-0.55, 0.0, 0.05]), hw * np.array([0.28, 0.45, 0.60]), 0.08, RHO_LUNG),
            _ellipsoid(c + hw * np.array([0.55, 0.0, 0.05]), hw * np.array([0.28, 0.45, 0.60]), 0.08, RHO_LUNG),
            _ellipsoid(heart, hw * HEART_RADIUS * np.asarray(HEART_AXES), 0.08, RHO_HEART),
            _ellipsoid(c + hw * np.array([0.0, -0.5, 0.0]), hw * np.array([0.10, 0.10, 0.85]), 0.2, RHO_SPINE)]
    return np.stack(rows)


def _unit(v):
    return v / np.linalg.norm(v)


def _tree_normalised(seed, step, main_steps, branch_prob, root_radius, tip_radius, taper):
    """The tree on the unit sphere of heart-normalised coordinates (the long axis is the last, the base at +1): points f64 [M,3] and
    segments as (point a, point b, ra, rb, parent segment or -1), radii in units of heart_radius.  A parent precedes its children."""
    rng = np.random.default_rng(seed)
    pts, segs = [], []
    apex = np.array([0.0, 0.0, -1.0])
    queue = []
    for azimuth in (0.7, 0.7 + math.pi):          # the two main arteries leave the base on opposite sides
        polar = 0.45 + 0.1 * rng.random()
        az = azimuth + 0.3 * (rng.random() - 0.5)
        u = np.array([math.sin(polar) * math.cos(az), math.sin(polar) * math.sin(az), math.cos(polar)])
        around = _unit(np.cross(np.array([0.0, 0.0, 1.0]), u))          # first along the groove around the base, then down
        pts.append(u)
        queue.append((len(pts) - 1, around, root_radius, -1, main_steps, 0))
    while queue:
        ia, direction, radius, parent, steps, generation = queue.pop(0)
        for _ in range(steps):
            u = pts[ia]
            v = _unit(u + step * direction)
            pts.append(v)
            ib = len(pts) - 1
            rb = max(tip_radius, radius * taper)
            segs.append((ia, ib, radius, rb, parent))
            parent = len(segs) - 1
            pull = apex - v * float(apex @ v)          # towards the apex, in the tangent plane
            direction = direction + 0.25 * rng.standard_normal(3) + 0.35 * pull
            direction = _unit(direction - v * float(direction @ v))
            if generation < 2 and rng.random() < branch_prob:
                side = 1.0 if rng.random() < 0.5 else -1.0
                angle = side * (0.6 + 0.6 * rng.random())
                turned = math.cos(angle) * direction + math.sin(angle) * np.cross(v, direction)
                queue.append((ib, _unit(turned), max(tip_radius, 0.75 * rb), parent, max(3, (steps * 2) // 3 if generation == 0 else steps // 2), generation + 1))
            ia, radius = ib, rb
    return np.stack(pts), segs


def _heart_matrix(fraction, contraction, shortening, twist):
    """The linear part of the heart's map at a fraction of the cycle: g = 0.5 - 0.5 cos(2 pi f) contracts the short axes by
    ``contraction g``, the long axis by ``shortening g`` and turns the heart about its long axis by ``twist g`` radians."""
    g = 0.5 - 0.5 * math.cos(2.0 * math.pi * float(fraction))
    s = np.diag([HEART_AXES[0] * (1.0 - contraction * g), HEART_AXES[1] * (1.0 - contraction * g), HEART_AXES[2] * (1.0 - shortening * g)])
    a = twist * g
    rot = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return rot @ s


def tree_at(fraction: float, *, seed: int = 0, center: Sequence[float], heart_radius: float, step: float = 0.1, main_steps: int = 22,
            branch_prob: float = 0.25, root_radius: float = 0.08, tip_radius: float = 0.025, taper: float = 0.95, contraction: float = 0.18,
            shortening: float = 0.08, twist: float = 0.25, return_parents: bool = False):
    """The coronary tree at ``fraction`` of the heart cycle: f64 ``[N, 8]`` segment rows (endpoints a, b, radii ra, rb).  The tree of a
    seed is fixed in heart-normalised coordinates (two main arteries that start near the base of the heart ellipsoid, walk over its surface
    towards the apex and branch twice; ``root_radius`` / ``tip_radius`` in units of ``heart_radius``, radii never increase from root to
    tip); the world position of a point is ``center + heart_radius M(fraction) point``, an affine map that contracts and twists the heart
    periodically (``_heart_matrix``).  ``fraction = 0`` is the uncontracted heart.  Every endpoint lies within
    ``HEART_EXTENT heart_radius`` of ``center``.  ``return_parents=True`` also returns i64 ``[N]``: the row whose end is this row's start,
    -1 for the two roots."""
    c = np.asarray(center, dtype=np.float64)
    hr = float(heart_radius)
    if c.shape != (3,) or not np.isfinite(c).all() or not (math.isfinite(hr) and hr > 0):
        raise _capi.NcaError(f"the heart has a finite centre of three coordinates and a positive radius, got {center!r} and {heart_radius!r}")
    if not 0 < tip_radius <= root_radius or not 0 < taper <= 1:
        raise _capi.NcaError(f"radii do not increase along a vessel: 0 < tip_radius <= root_radius and 0 < taper <= 1, got {tip_radius}, {root_radius}, {taper}")
    pts, segs = _tree_normalised(int(seed), float(step), int(main_steps), float(branch_prob), float(root_radius), float(tip_radius), float(taper))
    world = c + hr * (pts @ _heart_matrix(fraction, float(contraction), float(shortening), float(twist)).T)
    ia = np.array([s[0] for s in segs])
    ib = np.array([s[1] for s in segs])
    radii = hr * np.array([[s[2], s[3]] for s in segs], dtype=np.float64)
    rows = np.concatenate([world[ia], world[ib], radii], axis=1)
    if return_parents:
        return rows, np.array([s[4] for s in segs], dtype=np.int64)
    return rows


def coronary_tree(n_phases: int, *, seed: int = 0, center: Sequence[float], heart_radius: float, **kw) -> np.ndarray:
    """f64 ``[P, N, 8]``: ``tree_at(p / P)`` for the P phases of one cycle, bit for bit; phase 0 is the uncontracted heart.  Keywords as
    ``tree_at``."""
    n_phases = int(n_phases)
    if n_phases < 1:
        raise _capi.NcaError(f"coronary_tree: n_phases = {n_phases} is not positive")
    kw.pop("return_parents", None)
    return np.stack([tree_at(p / n_phases, seed=seed, center=center, heart_radius=heart_radius, **kw) for p in range(n_phases)])


def _table(t, width, name):
    """A host table as f64 [P or 1, rows, width] (a 2-D table is one phase), or None."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64))
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] != width or t.shape[0] == 0:
        raise _capi.NcaError(f"voxelize: {name} is [rows,{width}] or [P,rows,{width}], got {tuple(t.shape)}")
    if not np.isfinite(t).all():
        raise _capi.NcaError(f"voxelize: {name} holds a value that is not finite")
    return t


def voxelize(shape: Sequence[int], bounds, *, ellipsoids=None, segments=None, rho_vessel: float, edge: Optional[float] = None, device) -> torch.Tensor:
    """Rasterise ``ellipsoids`` f64 ``[P,E,14]`` and ``segments`` f64 ``[P,N,8]`` (host tables; a 2-D table is the same at every phase;
    either may be ``None`` or empty, not both) into f32 ``[P,n0,n1,n2]`` on ``device``: nodes ``linspace(lo, hi, n)`` of ``bounds``, one
    ``nca_phantom_voxelize``.  The value of a node is the sum of ``rho cov`` over the ellipsoids plus ``rho_vessel`` times the largest
    coverage of any segment; a coverage falls from 1 to 0 over the length ``edge`` (default: the coarsest node spacing) across a vessel
    wall, and over the fraction ``w`` of its radius across an ellipsoid's.

    Refused (``NcaError``), on the host tables before anything is uploaded: a non-finite entry, a negative radius, ``w <= 0``, two tables
    with different phase counts (other than 1), no rows at all, a ``rho_vessel`` that is not finite, an ``edge`` that is not finite and
    positive."""
    desc = _capi.grid_desc(shape, bounds)
    shape = tuple(int(n) for n in shape)
    ell, seg = _table(ellipsoids, 14, "ellipsoids"), _table(segments, 8, "segments")
    if ell is not None and (ell[:, :, 12] <= 0).any():
        raise _capi.NcaError("voxelize: an ellipsoid has a soft width w <= 0")
    if seg is not None and (seg[:, :, 6:8] < 0).any():
        raise _capi.NcaError("voxelize: a segment has a negative radius")
    n_ell, n_seg = (0 if ell is None else ell.shape[1]), (0 if seg is None else seg.shape[1])
    if n_ell == 0 and n_seg == 0:
        raise _capi.NcaError("voxelize: no ellipsoids and no segments: there is nothing to rasterise")
    counts = {t.shape[0] for t in (ell, seg) if t is not None and t.shape[1]}
    if len(counts - {1}) > 1:
        raise _capi.NcaError(f"voxelize: the ellipsoids have {ell.shape[0]} phases, the segments {seg.shape[0]}")
    P = max(counts)
    rho_vessel = float(rho_vessel)
    if not math.isfinite(rho_vessel):
        raise _capi.NcaError(f"voxelize: rho_vessel = {rho_vessel} is not finite")
    if edge is None:
        edge = max(1.0 / desc.inv[a] for a in range(3))
    edge = float(edge)
    if not (math.isfinite(edge) and edge > 0):
        raise _capi.NcaError(f"voxelize: edge = {edge} is not finite and positive")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _capi.NcaError(f"voxelize runs on the GPU: device is {dev}")

    def upload(t, n):
        if not n:
            return None
        return torch.from_numpy(np.array(np.broadcast_to(t, (P,) + t.shape[1:]), order="C")).to(dev)

    d_ell, d_seg = upload(ell, n_ell), upload(seg, n_seg)
    out = torch.empty((P,) + shape, dtype=torch.float32, device=dev)
    _view.launch(_capi.check_phantom, _capi.lib().nca_phantom_voxelize, out.device, C.byref(desc), P, n_ell, _capi.ptr(d_ell), n_seg, _capi.ptr(d_seg), rho_vessel,
                 edge, _capi.ptr(out))
    return out


def set_cull(on: bool) -> None:
    """Tile-level culling of segments on (the default) or off, process-wide; both give the same bits (include/nerfca_hip.h)."""
    _capi.check_phantom(_capi.lib().nca_phantom_set_cull(1 if on else 0))


def get_cull() -> bool:
    return bool(_capi.lib().nca_phantom_get_cull())


def make_phantom(shape: Sequence[int], n_phases: int, geo: dict, *, seed: int = 0, bounds=None, device, rho_vessel: float = RHO_VESSEL,
                 edge: Optional[float] = None) -> dict:
    """A thorax with a beating coronary tree sized for the geometry ``geo``: ``{"static" f32 [n0,n1,n2], "dynamic" f32 [P,n0,n1,n2],
    "bounds", "ellipsoids" f64 [E,14], "segments" f64 [P,N,8]}``.  Static is ``thorax`` around the isocentre, dynamic the
    ``coronary_tree(n_phases, seed=seed)`` on its heart, both in a cube of ``fov_half_width(geo)``; ``bounds`` defaults to that cube.  The
    pair is what ``synthetic.make_dataset(teacher=(static, dynamic), render=drr.volume_teacher(bounds))``, ``drr.project_sequence`` and
    ``drr.fit_volumes`` take; the tables are the truth at any resolution."""
    hw = fov_half_width(geo)
    if bounds is None:
        bounds = ((-hw, hw),) * 3
    bounds = tuple((float(b[0]), float(b[1])) for b in bounds)
    center = (0.0, 0.0, 0.0)
    ell = thorax(center, hw)
    seg = coronary_tree(n_phases, seed=seed, center=tuple(hw * c for c in HEART_CENTER), heart_radius=hw * HEART_RADIUS)
    static = voxelize(shape, bounds, ellipsoids=ell, rho_vessel=0.0, edge=edge, device=device)[0]
    dynamic = voxelize(shape, bounds, segments=seg, rho_vessel=rho_vessel, edge=edge, device=device)
    return {"static": static, "dynamic": dynamic, "bounds": bounds, "ellipsoids": ell, "segments": seg}


def centreline_points(segments, step: float) -> list:
    """The centrelines of a segment table as points: a list of P host arrays f64 ``[n_p, 3]`` from ``segments`` f64 ``[P, N, 8]`` (a 2-D
    table is one phase).  Each row (endpoints a, b) is sampled at ``a + t (b - a)``, ``t = k / m``, ``k = 0 .. m``,
    ``m = max(1, ceil(|b - a| / step))``: consecutive points of a row are at most ``step`` apart, both endpoints are included (a joint of
    two rows appears twice).  Host numpy, deterministic; what ``metrics.centreline_coverage`` takes."""
    step = float(step)
    if not (math.isfinite(step) and step > 0):
        raise _capi.NcaError(f"centreline_points: step = {step} is not finite and positive")
    seg = np.asarray(segments, dtype=np.float64)
    if seg.ndim == 2:
        seg = seg[None]
    if seg.ndim != 3 or seg.shape[2] != 8 or not np.isfinite(seg[:, :, :6]).all():
        raise _capi.NcaError(f"centreline_points: segments is a finite table [N,8] or [P,N,8], got {tuple(seg.shape)}")
    out = []
    for table in seg:
        pts = []
        for row in table:
            a, b = row[0:3], row[3:6]
            m = max(1, int(math.ceil(float(np.linalg.norm(b - a)) / step)))
            t = np.arange(m + 1, dtype=np.float64) / m
            pts.append(a[None, :] + t[:, None] * (b - a)[None, :])
        out.append(np.concatenate(pts, axis=0) if pts else np.zeros((0, 3)))
    return out


@torch.no_grad()
def volume_errors(pred: torch.Tensor, truth: torch.Tensor, threshold: Optional[float] = None) -> dict:
    """``{"rmse", "dice"}`` of a reconstructed volume (or stack) against the truth, in torch on the tensors' device: the root mean square
    error over all nodes in f64 and, with a ``threshold``, the Dice coefficient ``2 |A and B| / (|A| + |B|)`` of the masks
    ``pred > threshold`` and ``truth > threshold`` (1.0 when both are empty; ``None`` without a threshold)."""
    if pred.shape != truth.shape or pred.device != truth.device:
        raise _capi.NcaError(f"volume_errors: {tuple(pred.shape)} on {pred.device} against {tuple(truth.shape)} on {truth.device}")
    diff = pred.double() - truth.double()
    out = {"rmse": float(torch.sqrt((diff * diff).mean())), "dice": None}
    if threshold is not None:
        a, b = pred > threshold, truth > threshold
        total = int(a.sum()) + int(b.sum())
        out["dice"] = 2.0 * int((a & b).sum()) / total if total else 1.0
    return out
