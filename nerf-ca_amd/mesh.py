"""Iso-surfaces of voxel volumes as indexed triangle meshes, extracted on the device, and what a surface can be asked that voxels cannot.

``isosurface`` is marching tetrahedra on the Kuhn split of every grid cell (``nca_vol_iso_count`` / ``nca_vol_iso_emit``; the definition is
in include/nerfca_hip.h, "mesh"): a 16-case table without ambiguous cases, and a mesh that is an oriented closed 2-manifold wherever the
surface does not touch a face of the grid.  Vertices are shared (an indexed mesh without duplicates), triangles are counter-clockwise seen
from the side at or below the level, and the bits are the same on every run.  There is no torch implementation behind it and no CPU path.

``surface_area``, ``enclosed_volume`` and ``euler_characteristic`` are plain torch on a ``Mesh`` on any device: the area, the
divergence-theorem volume (sub-voxel, positive for a bright blob) and ``V - E + F`` -- 2 per closed surface without handles, 2 less per
handle -- which together with ``metrics.label`` answers "one tree, or a tree with loops and bubbles?".  ``write_ply`` and ``write_vtk``
write the two formats ParaView, MeshLab and pyvista read.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Union

import numpy as np
import torch

from . import _capi
from . import _view


class Mesh(NamedTuple):
    """``verts`` f32 ``[V, 3]`` in world coordinates, ``faces`` int32 ``[T, 3]`` (indices into ``verts``), ``normals`` f32 ``[V, 3]`` or None."""
    verts: torch.Tensor
    faces: torch.Tensor
    normals: Optional[torch.Tensor] = None


def _level(level, who):
    try:
        value = float(level)
    except (TypeError, ValueError):
        raise _capi.NcaError(f"{who}: level = {level!r} is not a number") from None
    with np.errstate(over="ignore"):
        as_f32 = float(np.float32(value)) if math.isfinite(value) else value
    if not math.isfinite(as_f32):
        raise _capi.NcaError(f"{who}: level = {value} is not finite as float32")
    return as_f32


@torch.no_grad()
def isosurface(vol: torch.Tensor, level: float, bounds, *, normals: bool = False) -> Union[Mesh, List[Mesh]]:
    """The surface ``vol == level`` of the f32 volume ``vol`` ``[n0, n1, n2]`` on the device, whose nodes are ``linspace(lo, hi, n)`` on each
    axis of ``bounds`` (``None``: node units): a ``Mesh`` on the same device.  A stack ``[..., n0, n1, n2]`` gives a list of them in stack
    order, each meshed on its own with vertex indices from 0.  A node is inside iff its value is above ``level`` (a NaN is not); a vertex lies
    on every grid edge, face diagonal and body diagonal of the Kuhn split whose ends differ, where the linear interpolant meets the level.
    ``normals=True`` adds the normalised negative gradient of ``vol`` (central differences) at every vertex: it points to the outside.  A
    volume the surface does not cross gives empty ``[0, 3]`` tensors.

    Two passes with the totals read in between: like ``torch.nonzero`` this makes exactly ONE host read per call (``n_vol`` pairs of
    int64), to size the outputs, and so synchronises with the device.  The same bits on every run.  Not differentiable."""
    who = "isosurface"
    level = _level(level, who)
    desc, x, n_vol, shape = _view.volume_stack(vol, who, bounds)
    lib = _capi.lib()
    dev = x.device
    nbytes = int(lib.nca_vol_iso_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, dev)
    totals = torch.empty((n_vol, 2), dtype=torch.int64, device=dev)
    _view.launch(_capi.check_mesh, lib.nca_vol_iso_count, dev, C.byref(desc), _capi.ptr(x), n_vol, level, _capi.ptr(totals), _capi.ptr(work), nbytes)
    counts = totals.cpu().tolist()          # the one host read
    n_vert, n_tri = sum(c[0] for c in counts), sum(c[1] for c in counts)
    verts = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_tri, 3), dtype=torch.int32, device=dev)
    norm = torch.empty((n_vert, 3), dtype=torch.float32, device=dev) if normals else None
    if n_vert or n_tri:
        _view.launch(_capi.check_mesh, lib.nca_vol_iso_emit, dev, C.byref(desc), _capi.ptr(x), n_vol, level, _capi.ptr(work), nbytes, n_vert, n_tri, _capi.ptr(verts),
                     _capi.ptr(faces), _capi.ptr(norm))
    out, v0, t0 = [], 0, 0
    for nv, nt in counts:
        out.append(Mesh(verts[v0:v0 + nv], faces[t0:t0 + nt], norm[v0:v0 + nv] if normals else None))
        v0, t0 = v0 + nv, t0 + nt
    return out[0] if vol.dim() == 3 else out


# ----------------------------------------------------------------------------- measures: plain torch, any device
def _check_mesh(mesh, who):
    if not isinstance(mesh, Mesh) or not isinstance(mesh.verts, torch.Tensor) or not isinstance(mesh.faces, torch.Tensor):
        raise _capi.NcaError(f"{who}: mesh is a Mesh of tensors, as isosurface returns it")
    v, f = mesh.verts, mesh.faces
    if v.dim() != 2 or v.shape[1] != 3 or not v.dtype.is_floating_point:
        raise _capi.NcaError(f"{who}: verts is a float tensor [V, 3], got {v.dtype} {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype not in (torch.int32, torch.int64):
        raise _capi.NcaError(f"{who}: faces is an int32 or int64 tensor [T, 3], got {f.dtype} {tuple(f.shape)}")
    if f.device != v.device:
        raise _capi.NcaError(f"{who}: verts live on {v.device}, faces on {f.device}")
    n = mesh.normals
    if n is not None and (not isinstance(n, torch.Tensor) or n.shape != v.shape or n.device != v.device):
        raise _capi.NcaError(f"{who}: normals is None or a tensor like verts")


def _corners(mesh):
    p = mesh.verts.to(torch.float64)[mesh.faces.to(torch.int64)]          # [T, 3, 3]
    return p[:, 0], p[:, 1], p[:, 2]


def surface_area(mesh: Mesh) -> torch.Tensor:
    """The sum of the triangle areas, a 0-d f64 tensor on the mesh's device."""
    _check_mesh(mesh, "surface_area")
    a, b, c = _corners(mesh)
    return 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1).sum()


def enclosed_volume(mesh: Mesh) -> torch.Tensor:
    """The divergence-theorem volume ``sum a . (b x c) / 6`` over the triangles ``(a, b, c)``, a 0-d f64 tensor: what a closed mesh encloses,
    positive where the inside is the brighter side.  The corners are taken relative to the centre of the mesh's box first, so a mesh far from
    the origin loses nothing; on an open mesh (a surface that leaves the grid) the number has no meaning."""
    _check_mesh(mesh, "enclosed_volume")
    if mesh.faces.shape[0] == 0:
        return torch.zeros((), dtype=torch.float64, device=mesh.verts.device)
    v = mesh.verts.to(torch.float64)
    centre = 0.5 * (v.min(dim=0)[0] + v.max(dim=0)[0])
    a, b, c = _corners(Mesh(v - centre, mesh.faces))
    return (a * torch.linalg.cross(b, c)).sum() / 6.0


def euler_characteristic(mesh: Mesh) -> int:
    """``V - E + F`` over the vertices the faces refer to, the edges as unordered pairs: 2 for every closed surface without handles, 2 - 2g
    for one of genus g, and their sum over the components.  One host read."""
    _check_mesh(mesh, "euler_characteristic")
    f = mesh.faces.to(torch.int64)
    if f.shape[0] == 0:
        return 0
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.sort(e, dim=1)[0]
    top = int(f.max()) + 1
    n_edges = torch.unique(e[:, 0] * top + e[:, 1]).numel()
    return int(torch.unique(f).numel()) - int(n_edges) + int(f.shape[0])


# ----------------------------------------------------------------------------- files
def _host(mesh, who):
    _check_mesh(mesh, who)
    v = np.ascontiguousarray(mesh.verts.detach().cpu().numpy(), dtype="<f4")
    f = np.ascontiguousarray(mesh.faces.detach().cpu().numpy(), dtype="<i4")
    n = None if mesh.normals is None else np.ascontiguousarray(mesh.normals.detach().cpu().numpy(), dtype="<f4")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise _capi.NcaError(f"{who}: faces refer to vertices outside [0, {v.shape[0]})")
    return v, f, n


def write_ply(path, mesh: Mesh) -> None:
    """``mesh`` as a binary little-endian PLY file: ``x y z`` (and ``nx ny nz`` when the mesh has normals) as float per vertex, a list of
    three int vertex indices per face."""
    v, f, n = _host(mesh, "write_ply")
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
    header = ["ply", "format binary_little_endian 1.0", "comment iso-surface", f"element vertex {v.shape[0]}"] + [f"property float {p}" for p in props] + \
             [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = v if n is None else np.concatenate([v, n], axis=1)
    faces = np.empty(f.shape[0], dtype=[("k", "u1"), ("i", "<i4", (3,))])
    faces["k"] = 3
    faces["i"] = f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(np.ascontiguousarray(rows, dtype="<f4").tobytes())
        out.write(faces.tobytes())


def write_vtk(path, mesh: Mesh) -> None:
    """``mesh`` as a legacy VTK PolyData file (binary, which that format defines as big-endian): POINTS float, POLYGONS, and the normals as
    POINT_DATA NORMALS when the mesh has them -- what ``pyvista.read`` and ParaView open."""
    v, f, n = _host(mesh, "write_vtk")
    cells = np.empty((f.shape[0], 4), dtype=">i4")
    cells[:, 0] = 3
    cells[:, 1:] = f
    with open(path, "wb") as out:
        out.write(b"# vtk DataFile Version 3.0\niso-surface\nBINARY\nDATASET POLYDATA\n")
        out.write(f"POINTS {v.shape[0]} float\n".encode("ascii"))
        out.write(v.astype(">f4").tobytes())
        out.write(f"\nPOLYGONS {f.shape[0]} {4 * f.shape[0]}\n".encode("ascii"))
        out.write(cells.tobytes())
        out.write(b"\n")
        if n is not None:
            out.write(f"POINT_DATA {v.shape[0]}\nNORMALS normals float\n".encode("ascii"))
            out.write(n.astype(">f4").tobytes())
            out.write(b"\n")


def write_vtk_polylines(path, points, radius=None) -> None:
    """Polylines as a legacy VTK PolyData file (binary, big-endian): ``points`` is a list of ``[n_k, 3]`` arrays or tensors, one polyline
    each (what ``centreline.extract`` returns as ``points``) -- POINTS float, LINES with one cell per polyline, and with ``radius`` (a list of
    ``[n_k]``) the scalar ``radius`` as POINT_DATA."""
    def host(t):
        return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)

    rows = [host(p).reshape(-1, 3) for p in points]
    if radius is not None and [host(r).size for r in radius] != [p.shape[0] for p in rows]:
        raise _capi.NcaError("write_vtk_polylines: radius has one value per point of every polyline")
    pts = np.concatenate(rows) if rows else np.zeros((0, 3))
    cells, first = [], 0
    for p in rows:
        cells.append(np.concatenate([[p.shape[0]], np.arange(first, first + p.shape[0])]))
        first += p.shape[0]
    cells = np.concatenate(cells).astype(">i4") if cells else np.zeros((0,), dtype=">i4")
    with open(path, "wb") as out:
        out.write(b"# vtk DataFile Version 3.0\ncentreline\nBINARY\nDATASET POLYDATA\n")
        out.write(f"POINTS {pts.shape[0]} float\n".encode("ascii"))
        out.write(pts.astype(">f4").tobytes())
        out.write(f"\nLINES {len(rows)} {cells.size}\n".encode("ascii"))
        out.write(cells.tobytes())
        out.write(b"\n")
        if radius is not None:
            rad = np.concatenate([host(r).reshape(-1) for r in radius]) if rows else np.zeros((0,))
            out.write(f"POINT_DATA {pts.shape[0]}\nSCALARS radius float 1\nLOOKUP_TABLE default\n".encode("ascii"))
            out.write(rad.astype(">f4").tobytes())
            out.write(b"\n")
