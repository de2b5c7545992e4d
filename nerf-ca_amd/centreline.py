"""Centrelines of vessel volumes by minimal paths, on the device: the geodesic distance transform under a cost, its predecessor field,
traced paths, ball cover, and the TEASAR loop (Sato et al. 2000) on top of them.

``geodesic_distance`` is the primitive (``nca_vol_geodesic``; the definition, operation by operation, is in include/nerfca_hip.h, "path"):
tile-wise relaxation sweeps that reach exactly the bits of a heap Dijkstra with the same two expressions.  ``predecessors``,
``trace_paths`` and ``ball_cover`` are the other three kernels.  ``extract`` is the loop: the penalised distance from the tree so far, the
farthest uncovered tip, the back-trace, invalidation by balls scaled with the local radius -- one ordered, one-node-wide, connected tree
with the lumen radius along it.  ``overlap`` and ``summary`` are plain torch / Python.  There is no torch implementation behind the kernels
and no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _capi
from . import _view
from . import fused as _fused
from . import metrics as _metrics


class Centreline(NamedTuple):
    """``paths``: int32 node tensors (linear indices in the volume), each from its tip to the node where it joins the tree (the first one:
    to the root).  ``points``: f32 world ``[len, 3]`` per path.  ``radius``: f32 ``[len]`` per path, the Euclidean distance transform at the
    nodes.  ``parent``: per path ``(path it joins, position in it)``, ``(-1, -1)`` for the first.  ``length``: world length per path.
    ``reached``: the share of the mask's nodes that are geodesically reachable from the root."""
    paths: List[torch.Tensor]
    points: List[torch.Tensor]
    radius: List[torch.Tensor]
    parent: List[Tuple[int, int]]
    length: List[float]
    reached: float


def _connectivity(connectivity, who):
    if connectivity not in (1, 2, 3):
        raise _capi.NcaError(f"{who}: connectivity = {connectivity!r} is not 1, 2 or 3 (6, 18 or 26 neighbours)")
    return int(connectivity)


def _positive_int(value, name, who):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise _capi.NcaError(f"{who}: {name} = {value!r} is not a positive integer")
    return int(value)


def set_skip(on: bool) -> None:
    """Switch the skipping of tiles that cannot change in a sweep (on by default).  The bits are the same either way."""
    _capi.check_path(_capi.lib().nca_path_set_skip(1 if on else 0))


def get_skip() -> bool:
    return bool(_capi.lib().nca_path_get_skip())


def _sweep(desc, cost, dist, n_vol, conn, sweeps, changed, work, nbytes):
    _view.launch(_capi.check_path, _capi.lib().nca_vol_geodesic, cost.device, C.byref(desc), n_vol, _capi.ptr(cost), _capi.ptr(dist), conn, sweeps,
                 _capi.ptr(changed), _capi.ptr(work), nbytes)


@torch.no_grad()
def geodesic_distance(cost: torch.Tensor, bounds, *, seeds=None, init: Optional[torch.Tensor] = None, connectivity: int = 3, sweeps: Optional[int] = None,
                      batch: int = 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(dist, changed)``: the geodesic distance (f64, the shape of ``cost``) inside the open nodes of the f32 stack ``cost``
    ``[..., n0, n1, n2]`` on the device, whose nodes are ``linspace(lo, hi, n)`` on each axis of ``bounds`` (``None``: node units).  A node
    is open when its cost is finite and >= 0, every other node is a wall and gets ``+inf``; an edge to one of the 6, 18 or 26 neighbours
    (``connectivity`` 1, 2, 3) weighs its length times the mean cost of its ends.

    ``seeds``: a bool / uint8 stack of the same shape (distance 0 where set), or integer node indices into the flattened stack.  ``init``:
    an f64 field of the same shape to continue from (any non-negative values; seeds, if given too, are lowered to 0 in a copy).  One of the
    two is needed.  ``sweeps=N``: exactly N sweeps and no host read -- capturable; ``changed`` (int32 per volume, on the device) counts the
    tiles that changed in the last one, 0 meaning converged.  ``sweeps=None``: batches of ``batch`` sweeps, ``changed`` read once per batch
    until it is 0 everywhere; the fixed point does not depend on ``batch``.  The same bits on every run.  Not differentiable."""
    who = "geodesic_distance"
    conn = _connectivity(connectivity, who)
    if sweeps is not None:
        sweeps = _positive_int(sweeps, "sweeps", who)
    batch = _positive_int(batch, "batch", who)
    desc, x, n_vol, shape = _view.volume_stack(cost, who, bounds, what="cost")
    dev = x.device
    if init is None and seeds is None:
        raise _capi.NcaError(f"{who}: neither seeds nor init is given")
    if init is not None:
        if not isinstance(init, torch.Tensor) or init.dtype != torch.float64 or init.shape != cost.shape or init.device != dev:
            raise _capi.NcaError(f"{who}: init is an f64 tensor of cost's shape on its device")
        dist = init.detach().reshape(x.shape).clone()
    else:
        dist = torch.full(x.shape, math.inf, dtype=torch.float64, device=dev)
    if seeds is not None:
        s = torch.as_tensor(seeds, device=dev)
        if s.dtype in (torch.bool, torch.uint8):
            if s.shape != cost.shape:
                raise _capi.NcaError(f"{who}: a seed mask has cost's shape {tuple(cost.shape)}, got {tuple(s.shape)}")
            dist.masked_fill_(s.reshape(x.shape) != 0, 0.0)
        elif s.dtype in (torch.int32, torch.int64):
            dist.view(-1).index_fill_(0, s.reshape(-1).to(torch.int64), 0.0)          # (an index outside the stack raises in torch)
        else:
            raise _capi.NcaError(f"{who}: seeds is a bool or uint8 mask or int32 / int64 node indices, got {s.dtype}")
    lib = _capi.lib()
    nbytes = int(lib.nca_vol_geodesic_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, dev)
    changed = torch.empty((n_vol,), dtype=torch.int32, device=dev)
    if sweeps is not None:
        _sweep(desc, x, dist, n_vol, conn, sweeps, changed, work, nbytes)
    else:
        while True:
            _sweep(desc, x, dist, n_vol, conn, batch, changed, work, nbytes)
            if int(changed.max()) == 0:          # the host read of the batch
                break
    return dist.reshape(cost.shape), changed


@torch.no_grad()
def predecessors(cost: torch.Tensor, dist: torch.Tensor, bounds, connectivity: int = 3) -> torch.Tensor:
    """The predecessor field (int32, the shape of ``cost``) of a distance field: for every open node the linear index, within its volume, of
    the open neighbour with a strictly smaller distance that minimises distance plus edge weight (the first in offset order on a tie), -1
    where there is none.  Chains strictly decrease in ``dist``: no cycles."""
    who = "predecessors"
    conn = _connectivity(connectivity, who)
    desc, x, n_vol, _ = _view.volume_stack(cost, who, bounds, what="cost")
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.float64 or dist.shape != cost.shape or dist.device != x.device:
        raise _capi.NcaError(f"{who}: dist is an f64 tensor of cost's shape on its device")
    d = dist.detach().reshape(x.shape).contiguous()
    pred = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    _view.launch(_capi.check_path, _capi.lib().nca_vol_geodesic_pred, x.device, C.byref(desc), n_vol, _capi.ptr(x), _capi.ptr(d), conn, _capi.ptr(pred))
    return pred.reshape(cost.shape)


@torch.no_grad()
def trace_paths(pred: torch.Tensor, starts, *, stop: Optional[torch.Tensor] = None, max_len: int):
    """``(paths, lengths, status)`` of following ``pred`` (int32, ONE volume, on the device) from every node of ``starts``: ``paths`` int32
    ``[n_paths, max_len]`` padded with -1, ``lengths`` int32, ``status`` int32 -- 0: ended at a node without predecessor, 1: at a node of
    ``stop`` (uint8 / bool of pred's shape, the node included), 2: truncated at ``max_len``, 3: the start is outside the volume.  A start ON A
    WALL is NOT status 3: ``pred`` holds -1 on a wall as on a seed and the costs are not seen here, so it gives one node and status 0.
    Bounded by ``max_len`` for any contents of ``pred``.  No host read."""
    who = "trace_paths"
    max_len = _positive_int(max_len, "max_len", who)
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32 or pred.numel() == 0:
        raise _capi.NcaError(f"{who}: pred is an int32 tensor, as predecessors returns it for one volume")
    _fused._require_cuda(pred, "pred")
    dev = pred.device
    p = pred.detach().contiguous()
    s = torch.as_tensor(starts, device=dev).reshape(-1)
    if s.dtype not in (torch.int32, torch.int64) or s.numel() == 0:
        raise _capi.NcaError(f"{who}: starts is a non-empty list of int32 / int64 node indices")
    big = torch.iinfo(torch.int32).max
    s = s.clamp(-1, big).to(torch.int32).contiguous()
    st = None
    if stop is not None:
        if not isinstance(stop, torch.Tensor) or stop.dtype not in (torch.bool, torch.uint8) or stop.shape != pred.shape or stop.device != dev:
            raise _capi.NcaError(f"{who}: stop is a bool or uint8 tensor of pred's shape on its device")
        st = stop.detach().to(torch.uint8).contiguous()
    n = s.numel()
    paths = torch.empty((n, max_len), dtype=torch.int32, device=dev)
    lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    _view.launch(_capi.check_path, _capi.lib().nca_vol_trace_paths, dev, p.numel(), _capi.ptr(p), _capi.ptr(st), n, _capi.ptr(s), max_len, _capi.ptr(paths),
                 _capi.ptr(lengths), _capi.ptr(status))
    return paths, lengths, status


@torch.no_grad()
def ball_cover(covered: torch.Tensor, nodes, radius, bounds) -> torch.Tensor:
    """Set ``covered`` (uint8 ``[n0, n1, n2]`` on the device, IN PLACE, only ever set to 1) at every node within ``radius[i]`` world units of
    node ``nodes[i]`` (linear index; a negative entry is skipped) on the grid of ``bounds``.  Returns ``covered``.  No host read."""
    who = "ball_cover"
    if not isinstance(covered, torch.Tensor) or covered.dtype != torch.uint8 or covered.dim() != 3 or not covered.is_contiguous():
        raise _capi.NcaError(f"{who}: covered is a contiguous uint8 volume [n0, n1, n2]")
    _fused._require_cuda(covered, "covered")
    dev = covered.device
    shape = tuple(covered.shape)
    desc = _capi.grid_desc(shape, tuple((0.0, float(n - 1)) for n in shape) if bounds is None else bounds)
    nd = torch.as_tensor(nodes, device=dev).reshape(-1)
    if nd.dtype not in (torch.int32, torch.int64) or nd.numel() == 0:
        raise _capi.NcaError(f"{who}: nodes is a non-empty list of int32 / int64 node indices")
    nd = nd.clamp(-1, torch.iinfo(torch.int32).max).to(torch.int32).contiguous()
    r = torch.as_tensor(radius, device=dev).to(torch.float32).reshape(-1).contiguous()
    if r.numel() != nd.numel():
        raise _capi.NcaError(f"{who}: {nd.numel()} nodes and {r.numel()} radii")
    _view.launch(_capi.check_path, _capi.lib().nca_vol_ball_cover, dev, C.byref(desc), nd.numel(), _capi.ptr(nd), _capi.ptr(r), _capi.ptr(covered))
    return covered


def _first_index(flag):
    """The smallest flat index at which ``flag`` is set, as a 0-d int64 tensor (the number of entries when none is)."""
    n = flag.numel()
    idx = torch.arange(n, device=flag.device)
    return torch.where(flag.reshape(-1), idx, torch.full_like(idx, n)).min()


@torch.no_grad()
def extract(vol: torch.Tensor, bounds, *, threshold: float, root=None, scale: float = 1.5, const: Optional[float] = None, pdrf_scale: float = 5000.0,
            pdrf_exponent: int = 16, max_paths: int = 256) -> Centreline:
    """The centreline tree of ONE f32 volume ``vol`` ``[n0, n1, n2]`` on the device: the TEASAR loop on the mask ``vol > threshold``.

    ``R`` is ``metrics.distance_transform(..., inside=True)``.  The root is the node nearest the world point ``root`` (it must lie on the
    mask), or with ``None`` the mask node of largest ``R`` (the smallest index on a tie).  ``g0`` is the geodesic distance from the root at
    cost 1 (26 neighbours).  The penalised cost is ``c = pdrf_scale * x^pdrf_exponent + 1`` with ``x = 1 - R / (1.01 max R)`` in f64, the
    power as ``pdrf_exponent - 1`` successive multiplications, rounded to f32.  Then, until no reachable node is uncovered or ``max_paths``
    paths are found: the tip is the uncovered reachable node of largest ``g0`` (smallest index on a tie); ``g1`` is the geodesic distance at
    cost ``c`` from ALL tree nodes so far -- the previous ``g1`` with the tree lowered to 0, continued, not recomputed; the tip is traced
    along the predecessors of ``g1`` until it meets the tree; the path joins the tree, and balls of radius ``scale * R + const`` around its
    nodes are covered (``const`` defaults to twice the largest spacing).  An empty mask gives an empty tree; a volume that lies wholly
    above the threshold is refused (its distance transform is infinite: there is no radius).

    Host reads, each a synchronisation: two at the start (the mask's counts, the first tip), one per batch of sweeps of every ``g1`` (as
    ``geodesic_distance`` makes them) and ONE per branch (the path's length and the next tip together); the paths come to the host once at
    the end, for ``parent``.  The same bits on every run."""
    who = "extract"
    _view.check_volume(vol, who)
    if vol.dim() != 3:
        raise _capi.NcaError(f"{who} takes ONE volume [n0, n1, n2], got {tuple(vol.shape)}")
    threshold = _view.finite_threshold(threshold, who)
    max_paths = _positive_int(max_paths, "max_paths", who)
    pdrf_exponent = _positive_int(pdrf_exponent, "pdrf_exponent", who)
    shape = tuple(vol.shape)
    desc = _capi.grid_desc(shape, tuple((0.0, float(n - 1)) for n in shape) if bounds is None else bounds)
    h = [1.0 / desc.inv[a] for a in range(3)]
    lo = [desc.lo[a] for a in range(3)]
    if const is None:
        const = 2.0 * max(h)
    dev = vol.device
    x = vol.detach().contiguous()
    mask = x > threshold
    R = _metrics.distance_transform(x, bounds, threshold=threshold, inside=True)
    voxels = x.numel()
    nan = torch.full((), math.nan, dtype=torch.float32, device=dev)
    empty = Centreline([], [], [], [], [], 0.0)

    Rm = torch.where(mask, R, torch.full_like(R, -1.0))
    r_max = Rm.max()
    if root is None:
        root_t = _first_index(Rm == r_max)
    else:
        idx, inside = _metrics.nearest_nodes([root], shape, tuple((0.0, float(n - 1)) for n in shape) if bounds is None else bounds)
        if not inside[0]:
            raise _capi.NcaError(f"{who}: root = {tuple(root)!r} lies outside the grid")
        root_t = torch.tensor((int(idx[0, 0]) * shape[1] + int(idx[0, 1])) * shape[2] + int(idx[0, 2]), device=dev)
    n_mask, root_i, root_on, r_finite = (int(v) for v in torch.stack([mask.sum(), root_t, mask.reshape(-1)[root_t.clamp(max=voxels - 1)].to(torch.int64),
                                                                       torch.isfinite(r_max).to(torch.int64)]).cpu())
    if n_mask == 0:
        return empty
    if not r_finite:
        raise _capi.NcaError(f"{who}: every node lies above threshold = {threshold}: there is no vessel wall to measure a radius from")
    if not root_on:
        raise _capi.NcaError(f"{who}: the node nearest root = {tuple(root)!r} is not on the mask")

    unit = torch.where(mask, torch.ones_like(x), nan)
    g0, _ = geodesic_distance(unit, bounds, seeds=torch.tensor([root_i], device=dev))
    reach = torch.isfinite(g0) & mask
    xx = 1.0 - R.to(torch.float64) / (r_max.to(torch.float64) * 1.01)
    p = xx
    for _ in range(pdrf_exponent - 1):
        p = p * xx
    c = torch.where(mask, (p * float(pdrf_scale) + 1.0).to(torch.float32), nan)

    tree_flat = torch.zeros((voxels + 1,), dtype=torch.uint8, device=dev)          # one spare slot past the volume
    tree = tree_flat[:voxels].view(shape)
    tree_flat[root_i] = 1
    covered = torch.zeros(shape, dtype=torch.uint8, device=dev)
    g1 = torch.full(shape, math.inf, dtype=torch.float64, device=dev)
    radius_of = (R.to(torch.float64) * float(scale) + float(const)).to(torch.float32).reshape(-1)

    def next_tip():
        cand = torch.where(reach & (covered == 0), g0, torch.full_like(g0, -1.0))
        m = cand.max()
        return torch.where(m >= 0, _first_index(cand == m), torch.full((), -1, dtype=torch.int64, device=dev))

    tip = int(next_tip())
    n_reach, n_tree = None, 1
    rows, lens = [], []
    while tip >= 0 and len(rows) < max_paths:
        g1, _ = geodesic_distance(c, bounds, init=g1, seeds=tree)
        pred = predecessors(c, g1, bounds)
        if n_reach is None:
            n_reach = int(reach.sum())
        # a path has distinct nodes, none but its last on the tree: no longer than the reachable nodes off the tree, plus one
        paths, lengths, _ = trace_paths(pred, torch.tensor([tip], device=dev), stop=tree, max_len=max(n_reach - n_tree + 1, 1))
        row = paths[0]
        live = row >= 0
        safe = row.clamp(min=0).to(torch.int64)
        tree_flat.index_fill_(0, torch.where(live, safe, torch.full_like(safe, voxels)), 1)          # the padding goes to the spare slot
        ball_cover(covered, row, radius_of[safe], bounds)
        n, tip = (int(v) for v in torch.stack([lengths[0].to(torch.int64), next_tip()]).cpu())          # the one host read of the branch
        rows.append(row)
        lens.append(n)
        n_tree += n - 1

    if n_reach is None:
        n_reach = int(reach.sum())
    host = [r[:n].cpu().numpy() for r, n in zip(rows, lens)]
    where = {}
    parent = []
    for k, nodes in enumerate(host):
        parent.append(where.get(int(nodes[-1]), (-1, -1)))
        for pos, node in enumerate(nodes.tolist()):
            where.setdefault(node, (k, pos))
    out_paths, points, radius, length = [], [], [], []
    lo_t, h_t = torch.tensor(lo, dtype=torch.float64, device=dev), torch.tensor(h, dtype=torch.float64, device=dev)
    for r, n in zip(rows, lens):
        nodes = r[:n].clone()
        i = nodes.to(torch.int64)
        ijk = torch.stack([i // (shape[1] * shape[2]), (i // shape[2]) % shape[1], i % shape[2]], dim=1).to(torch.float64)
        w = lo_t + ijk * h_t
        out_paths.append(nodes)
        points.append(w.to(torch.float32))
        radius.append(R.reshape(-1)[i])
        length.append(float(((ijk[1:] - ijk[:-1]) * h_t).square().sum(dim=1).sqrt().sum()) if n > 1 else 0.0)
    return Centreline(out_paths, points, radius, parent, length, n_reach / n_mask)


def overlap(points_a: torch.Tensor, points_b: torch.Tensor, tol: float) -> Tuple[float, float]:
    """``(share of points_a within tol of some point of points_b, share of points_b within tol of some point of points_a)``: plain torch on
    ``[n, 3]`` point sets on one device.  An empty set has share 0."""
    a, b = torch.as_tensor(points_a).to(torch.float64).reshape(-1, 3), torch.as_tensor(points_b).to(torch.float64).reshape(-1, 3)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0.0, 0.0
    d = torch.cdist(a, b.to(a.device), compute_mode="donot_use_mm_for_euclid_dist")
    return float((d.min(dim=1)[0] <= tol).double().mean()), float((d.min(dim=0)[0] <= tol).double().mean())


def summary(c: Centreline) -> dict:
    """``branches``, ``total_length`` and per path ``length``, ``nodes``, ``radius_min`` / ``radius_mean`` / ``radius_max``, ``parent``."""
    per = []
    for k, r in enumerate(c.radius):
        r = r.to(torch.float64)
        per.append({"nodes": int(r.numel()), "length": float(c.length[k]), "radius_min": float(r.min()), "radius_mean": float(r.mean()),
                    "radius_max": float(r.max()), "parent": [int(v) for v in c.parent[k]]})
    return {"branches": len(c.paths), "total_length": float(sum(c.length)), "reached": float(c.reached), "paths": per}
