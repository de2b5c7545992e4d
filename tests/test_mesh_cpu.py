"""Iso-surfaces (nca_vol_iso_workspace / nca_vol_iso_count / nca_vol_iso_emit, mesh.isosurface and its measures and writers): everything
that can be checked without a launch -- the C-ABI surface, every refusal of the entry points (with device pointers that are never read),
the workspace query, the kernel's table against the oracle's, the numpy oracle of the GPU tests (tests/mesh_ref.py) held to the mathematics
(closed oriented manifolds, Euler characteristics, the enclosed volume against an independent cut of every tetrahedron, the complement, a
plane), the plain-torch measures, the file writers read back, the refusals of the Python layer and the command lines."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import nca_testlib as T
import mesh_ref as ref
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_iso_workspace", "nca_vol_iso_count", "nca_vol_iso_emit", "nca_mesh_last_error")
refused = functools.partial(T.refused, "mesh")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_vess_last_error(void)", "---- mesh:", "size_t nca_vol_iso_workspace(", "int nca_vol_iso_count(", "int nca_vol_iso_emit(", "nca_mesh_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert callable(capi.check_mesh)
    import nerfca_amd
    from nerfca_amd import export, mesh
    assert nerfca_amd.mesh is mesh and "mesh" in nerfca_amd.__all__
    for name in ("isosurface", "surface_area", "enclosed_volume", "euler_characteristic", "write_ply", "write_vtk", "Mesh"):
        assert callable(getattr(mesh, name)), name
    assert callable(export.density_surfaces)
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(CSRC)/view/nca_mesh.hip" in makefile


def test_the_kernels_table_is_the_oracles():
    """The 16-case table, the corner codes and the parities of csrc/view/nca_mesh.hip, read from its source, are those of tests/mesh_ref.py
    (which the tests below hold to the mathematics), and the header prints the same table."""
    src = open(os.path.join(ROOT, "nerf-ca_amd", "csrc", "view", "nca_mesh.hip")).read()

    def array(name):
        body = re.search(name + r"(?:\[\d+\])+ = (\{.*?\});", src, re.S).group(1)
        return [int(x) for x in re.findall(r"\d+", body)]

    tri = array("MS_TRI")
    assert len(tri) == 96
    for case in range(16):
        want = list(ref.TRIANGLES[case]) + [0] * (6 - len(ref.TRIANGLES[case]))
        assert tri[6 * case:6 * case + 6] == want, case
    assert array("MS_P1") == [ref.corner_codes(q)[1] for q in range(6)] and array("MS_P2") == [ref.corner_codes(q)[2] for q in range(6)]
    assert array("MS_ODD") == [int(o) for o in ref.ODD]
    assert array("MS_EI") == [e[0] for e in ref.EDGES] and array("MS_EJ") == [e[1] for e in ref.EDGES]
    assert int(re.search(r"MS_BLOCK = (\d+)", src).group(1)) == ref.SCAN_BATCH and ref.SCAN_CHUNK == 4 * ref.SCAN_BATCH and "MS_CHUNK = MS_BLOCK * MS_NPT" in src
    header = open(os.path.join(ROOT, "include", "nerfca_hip.h")).read()
    for case in range(1, 15):
        es = ref.TRIANGLES[case]
        text = ", ".join(" ".join(str(e) for e in es[3 * s:3 * s + 3]) for s in range(len(es) // 3))
        assert re.search(rf"\b{case}: {text}\b", header), (case, text)
    # the parity is the sign of det[p1 - p0, p2 - p0, p3 - p0], and a tetrahedron's edge is the edge k = the difference of its ends
    for q in range(6):
        P = [np.array(ref.direction(c)) for c in ref.corner_codes(q)]
        assert round(float(np.linalg.det(np.stack([P[1] - P[0], P[2] - P[0], P[3] - P[0]]).astype(float)))) == (-1 if ref.ODD[q] else 1)
        codes = ref.corner_codes(q)
        for i, j in ref.EDGES:
            assert codes[i] & codes[j] == codes[i] and codes[i] ^ codes[j] in range(1, 8)


# ----------------------------------------------------------------------------- refusals
def workspace_formula(n, n_vol):
    nodes = n[0] * n[1] * n[2]
    s = (nodes + 3) // 4 * 4
    r = lambda b: (b + 255) // 256 * 256          # noqa: E731
    return r(2 * n_vol * s) + 2 * r(4 * n_vol * s) + r(8 * n_vol * ((nodes + 1023) // 1024)) + 2 * r(16 * n_vol)


def _shared_refusals(capi, lib, call, who):
    """From n_vol on, what both entry points refuse, in order; the last refusal (the launch limit) is the proof of the order: a call that
    passed every check would launch."""
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("mesh", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    # offsets are int32: 7 vertices per node and 12 triangles per cell must fit
    most = (2 ** 31 - 1) // 7
    assert call(n=(2, 2, most // 4), n_vol=1, work=None) == E_WORKSPACE
    refused(capi, lib, call(n=(2, 2, most // 4 + 1), n_vol=1), who, "2^31 - 1", "int32", code=E_UNSUPPORTED)
    refused(capi, lib, call(n=(600, 600, 600), n_vol=1), who, "600 x 600 x 600", "int32", code=E_UNSUPPORTED)
    assert call(n=(512, 512, 512), n_vol=1, work=None) == E_WORKSPACE          # 12 x 511^3 triangles fit
    for bad, word in ((math.nan, "nan"), (math.inf, "inf"), (-math.inf, "-inf")):
        refused(capi, lib, call(level=bad), f"level = {word}", "not finite")
    for ok in (0.0, -3.5, 3.0e38):
        assert call(level=ok, work=None) == E_WORKSPACE
    need = lib.nca_vol_iso_workspace(C.byref(grid(capi)), 2)
    assert need == workspace_formula((4, 5, 6), 2)
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)
    # the workspace comes before the launch limits
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30, work=None), "work is NULL", code=E_WORKSPACE)
    # 4 x 8 x 65 is two tiles and three runs of 1024 nodes: 2^30 such volumes are more than one launch covers, and the larger count is named
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30), "tiles", "one launch", str(3 << 30))
    refused(capi, lib, call(n=(4, 4, 128), n_vol=1 << 30), "tiles", "one launch", str(1 << 31))
    # the tiling sets no limit on an axis
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE


def test_iso_count_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, level=0.5, totals=FAKE + 64, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_iso_count(g, vol, n_vol, level, totals, work, work_bytes, None)

    who = "nca_vol_iso_count:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(totals=None), who, "totals is NULL")
    refused(capi, lib, call(vol=None, n_vol=0), "vol is NULL")          # pointers before n_vol
    _shared_refusals(capi, lib, call, who)


def test_iso_emit_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, level=0.5, work=FAKE, work_bytes=1 << 62, vert_cap=10, tri_cap=10, verts=FAKE + 64, tris=FAKE + 128, normals=None, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_iso_emit(g, vol, n_vol, level, work, work_bytes, vert_cap, tri_cap, verts, tris, normals, None)

    who = "nca_vol_iso_emit:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    for bad in (-1, -(1 << 40)):
        refused(capi, lib, call(vert_cap=bad), f"vert_cap = {bad}", "negative")
        refused(capi, lib, call(tri_cap=bad), f"tri_cap = {bad}", "negative")
    refused(capi, lib, call(verts=None), who, "verts is NULL")
    refused(capi, lib, call(tris=None), who, "tris is NULL")
    refused(capi, lib, call(verts=None, n_vol=0), "verts is NULL")
    _shared_refusals(capi, lib, call, who)
    # nothing to write: the outputs may be NULL, every other check is still made, and nothing is launched (the pointers here are not memory)
    assert call(vert_cap=0, tri_cap=0, verts=None, tris=None) == 0
    assert call(vert_cap=0, tri_cap=0) == 0
    refused(capi, lib, call(vert_cap=0, tri_cap=0, verts=None, tris=None, level=math.nan), "level = nan")
    refused(capi, lib, call(vert_cap=0, tri_cap=0, verts=None, tris=None, work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(vert_cap=0, tri_cap=3, verts=None, tris=None), "tris is NULL")
    refused(capi, lib, call(vert_cap=3, tri_cap=0, verts=None, tris=None), "verts is NULL")


def test_workspace_query(capi, lib):
    def q(n, n_vol, **kw):
        return lib.nca_vol_iso_workspace(C.byref(grid(capi, n=n, **kw)), n_vol)

    assert q((2, 2, 2), 1) == 256 + 2 * 256 + 256 + 2 * 256
    for n_vol in (1, 2, 7):
        for n in ((3, 4, 5), (3, 3, 3), (9, 4, 130), (33, 17, 65), (256, 256, 256), (4, 4, 1 << 20)):
            assert q(n, n_vol) == workspace_formula(n, n_vol) and q(n, n_vol) % 256 == 0, (n, n_vol)
    assert q((512,) * 3, 64) == workspace_formula((512,) * 3, 64) > 1 << 32          # a size_t
    assert lib.nca_vol_iso_workspace(None, 1) == 0
    for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1), ((600, 600, 600), 1)):
        assert q(*bad) == 0, bad
    assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0


# ----------------------------------------------------------------------------- the oracle against the mathematics
def bounds_of(shape):
    return tuple((ref.LO[a], ref.LO[a] + (shape[a] - 1) / ref.INV[a]) for a in range(3))


CLOSED = {"ball": lambda: (ref.ball((12, 12, 12), 4.3), 0.0), "torus": lambda: (ref.torus((12, 20, 20)), 0.0), "two balls": lambda: (ref.two_balls((12, 12, 30)), 0.0),
          "branching tube": lambda: (ref.branching_tube((16, 16, 24)), 0.5), "random": lambda: (ref.zero_border(ref.random_volume((7, 8, 9), 3)), 0.5)}


@functools.lru_cache(maxsize=None)
def closed(name):
    vol, level = CLOSED[name]()
    return vol, level, ref.mesh(vol, level, ref.LO, ref.INV, normals=True)


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_volumes_give_closed_oriented_manifolds(name):
    vol, level, m = closed(name)
    border = np.ones(vol.shape, dtype=bool)
    border[1:-1, 1:-1, 1:-1] = False
    assert (vol[border] <= level).all() and (vol > level).any()
    tris = m["tris"]
    assert tris.dtype == np.int32 and tris.shape[0] > 100 and ref.is_closed_oriented(tris)
    assert np.array_equal(np.unique(tris), np.arange(m["verts"].shape[0]))          # every vertex is referred to: no orphan, no gap
    assert m["verts"].shape[0] - 3 * tris.shape[0] // 2 + tris.shape[0] == ref.euler_characteristic(tris)          # closed: E = 3 F / 2
    # an open surface is told apart: a ball that leaves the grid
    cut = ref.mesh(ref.ball((8, 8, 8), 4.5), 0.0, ref.LO, ref.INV)
    assert not ref.is_closed_oriented(cut["tris"])


def test_euler_characteristics():
    assert ref.euler_characteristic(closed("ball")[2]["tris"]) == 2
    assert ref.euler_characteristic(closed("torus")[2]["tris"]) == 0
    assert ref.euler_characteristic(closed("two balls")[2]["tris"]) == 4
    assert ref.euler_characteristic(closed("branching tube")[2]["tris"]) == 2          # one tree, no loop, no bubble


@pytest.mark.parametrize("name", list(CLOSED))
def test_enclosed_volume_equals_the_inside_volume(name):
    """The divergence-theorem volume of the unrounded f64 vertices against the volume above the level summed tetrahedron by tetrahedron, which
    never looks at the mesh.  The gate is the bound of the sum's rounding, T 2^-52 sum |term| (measured: 4e-16 .. 7e-16 of the volume, at
    T = 1000 .. 4400)."""
    vol, level, m = closed(name)
    terms = ref.volume_terms(m["verts64"], m["tris"])
    got, want = float(terms.sum()), ref.inside_volume(vol, level, bounds_of(vol.shape))
    gate = terms.size * 2.0 ** -52 * float(np.abs(terms).sum())
    print(f"{name}: T = {terms.size}, enclosed {got!r}, inside {want!r}, |difference| {abs(got - want):.3e} = {abs(got - want) / want:.3e} relative, gate {gate:.3e}")
    assert want > 0 and got > 0 and abs(got - want) <= gate
    # and the f32 vertices lose no more than their rounding: 2^-24 of the coordinates over the surface
    got32 = float(ref.volume_terms(m["verts"], m["tris"]).sum())
    assert abs(got32 - want) <= 2.0 ** -22 * float(np.abs(m["verts64"]).max()) * ref.area(m["verts64"], m["tris"])


def _canonical(tris):
    """Every triangle rotated so that its smallest index comes first; the rows sorted."""
    t = np.asarray(tris, dtype=np.int64)
    k = t.argmin(axis=1)
    rot = np.stack([t[np.arange(len(t)), (k + j) % 3] for j in range(3)], axis=1)
    return rot[np.lexsort(rot.T[::-1])]


def test_the_complement_has_the_same_vertices_and_the_reversed_winding():
    for vol, level in ((ref.random_volume((6, 7, 8), 5), 0.5), (closed("torus")[0], 0.0625), (ref.ball((9, 9, 9), 3.1), 0.03125)):
        assert not (vol == np.float32(level)).any()
        a = ref.mesh(vol, level, ref.LO, ref.INV, normals=True)
        b = ref.mesh(-vol, -level, ref.LO, ref.INV, normals=True)
        assert T.same_bits(a["verts"], b["verts"]) and np.array_equal(a["verts64"], b["verts64"])
        assert a["tris"].shape == b["tris"].shape and a["tris"].shape[0] > 0
        assert np.array_equal(_canonical(a["tris"]), _canonical(b["tris"][:, [0, 2, 1]]))
        assert not np.array_equal(_canonical(a["tris"]), _canonical(b["tris"]))
        assert np.array_equal(a["normals"], -b["normals"])


def test_a_plane():
    shape = (6, 7, 9)
    i, j, k = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    h = [1.0 / v for v in ref.INV]
    X = [ref.LO[a] + x * h[a] for a, x in enumerate((i, j, k))]
    # a linear field in world coordinates with exactly representable values: the vertices lie on its zero plane
    coef, d = (0.5, -0.25, 0.125), 2.40625          # through the middle of the box
    vol = (coef[0] * X[0] + coef[1] * X[1] + coef[2] * X[2] - d).astype(np.float32)
    assert np.array_equal(vol.astype(np.float64), coef[0] * X[0] + coef[1] * X[1] + coef[2] * X[2] - d) and not (vol == 0).any()
    m = ref.mesh(vol, 0.0, ref.LO, ref.INV, normals=True)
    assert m["tris"].shape[0] > 50
    off = m["verts64"] @ np.array(coef) - d
    assert np.abs(off).max() <= 2.0 ** -48, np.abs(off).max()          # a few roundings of coordinates of size <= 18
    unit = -np.array(coef) / np.linalg.norm(coef)
    q = (m["verts64"] - np.array(ref.LO)) * np.array(ref.INV)          # in nodes; at a face the replicated edge value halves the difference
    away = ((q >= 1.0) & (q <= np.array(shape) - 2.0)).all(axis=1)
    assert away.sum() > 20 and np.abs(m["normals"][away].astype(np.float64) - unit).max() <= 2.0 ** -23          # a linear field's gradient is exact: one f32 rounding
    # axis-aligned planes: the area is the box's cross-section, and the vertices have the plane's coordinate exactly
    ext = [(shape[a] - 1) * h[a] for a in range(3)]
    for a, x in enumerate((i, j, k)):
        m = ref.mesh(x.astype(np.float32), 2.5, ref.LO, ref.INV)
        want = ext[(a + 1) % 3] * ext[(a + 2) % 3]
        assert abs(ref.area(m["verts64"], m["tris"]) - want) <= 1e-13 * want
        assert (m["verts64"][:, a] == ref.LO[a] + 2.5 * h[a]).all()
        # per cell the axis comes first, second or last in two permutations each: 1, 2 and 1 triangles
        assert m["tris"].shape[0] == 8 * (shape[(a + 1) % 3] - 1) * (shape[(a + 2) % 3] - 1)


def test_sphere_volume_is_informative_only():
    """The piecewise linear surface cuts the corners of a sphere: the ratio to 4/3 pi r^3 is recorded, not gated."""
    for side, r in ((12, 4.3), (24, 8.6)):
        m = ref.mesh(ref.ball((side,) * 3, r), 0.0, (0.0,) * 3, (1.0,) * 3)
        ratio = float(ref.volume_terms(m["verts64"], m["tris"]).sum()) / (4.0 / 3.0 * math.pi * r ** 3)
        print(f"sphere of radius {r} in {side}^3: enclosed / exact = {ratio:.4f}")
        assert 0.9 < ratio < 1.0          # (it cannot exceed 1: the chords lie inside)


def test_rules_at_the_level_and_off_the_numbers():
    # a node exactly at the level is outside; its edges to inside nodes carry vertices AT the node (t = 0 or 1): zero-area triangles stay
    vol = np.zeros((3, 3, 3), dtype=np.float32)
    vol[1, 1, 1] = 2.0
    vol[0, 1, 1] = 1.0
    m = ref.mesh(vol, 1.0, (0.0,) * 3, (1.0,) * 3)
    assert ref.is_closed_oriented(m["tris"]) and ref.euler_characteristic(m["tris"]) == 2
    assert (m["verts"] == np.array([0.0, 1.0, 1.0], dtype=np.float32)).all(axis=1).sum() == 1
    x = np.array([np.nan, 0.5, 1.0, -np.inf, np.inf], dtype=np.float32)
    assert ref.inside(x, 0.5).tolist() == [False, False, True, False, True]
    t = ref._crossing_t(np.array([np.inf, 0.0, np.nan, 1.0, 0.25]), np.array([0.0, np.inf, 1.0, np.nan, 0.75]), 0.5)
    assert t.tolist() == [0.5, 0.0, 0.5, 0.5, 0.5]
    for name in ref.CASE_NAMES:          # every case of the GPU tests: totals, and the totals of a mesh that is consistent
        e = ref.expected((4, 5, 6), name)
        assert e["totals"].shape == (2, 2) and e["verts"].shape == (int(e["totals"][:, 0].sum()), 3) and e["tris"].shape == (int(e["totals"][:, 1].sum()), 3)
        assert e["normals"].shape == e["verts"].shape and np.isfinite(e["verts"]).all() and np.isfinite(e["normals"]).all()
    assert ref.expected((4, 5, 6), "empty and full")["totals"].tolist() == [[0, 0], [0, 0]]
    assert ref.expected((4, 5, 6), "checkerboard")["totals"][:, 1].tolist() == [12 * 3 * 4 * 5] * 2          # 12 triangles in every cell


# ----------------------------------------------------------------------------- the plain-torch measures and the writers
def _torch_mesh(m, normals=True):
    from nerfca_amd import mesh
    return mesh.Mesh(torch.from_numpy(m["verts"].copy()), torch.from_numpy(m["tris"].copy()), torch.from_numpy(m["normals"].copy()) if normals else None)


def test_measures_on_cpu_tensors():
    from nerfca_amd import mesh
    for name, chi in (("ball", 2), ("torus", 0), ("two balls", 4)):
        vol, level, m = closed(name)
        tm = _torch_mesh(m)
        area, volume = mesh.surface_area(tm), mesh.enclosed_volume(tm)
        assert area.dtype == torch.float64 and area.shape == () and volume.dtype == torch.float64 and volume.shape == ()
        want_area, want_volume = ref.area(m["verts"], m["tris"]), ref.inside_volume(vol, level, bounds_of(vol.shape))
        assert abs(float(area) - want_area) <= 1e-12 * want_area
        assert abs(float(volume) - want_volume) <= 1e-6 * want_volume          # f32 vertices
        assert mesh.euler_characteristic(tm) == chi
        assert mesh.euler_characteristic(mesh.Mesh(tm.verts, tm.faces.long())) == chi
        flipped = mesh.Mesh(tm.verts, tm.faces[:, [0, 2, 1]])
        assert float(mesh.enclosed_volume(flipped)) == pytest.approx(-float(volume), rel=1e-12)
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    assert float(mesh.surface_area(empty)) == 0.0 and float(mesh.enclosed_volume(empty)) == 0.0 and mesh.euler_characteristic(empty) == 0
    one = mesh.Mesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32))
    assert float(mesh.enclosed_volume(one)) == pytest.approx(1.0 / 6.0, rel=1e-15) and mesh.euler_characteristic(one) == 2
    assert float(mesh.surface_area(one)) == pytest.approx(1.5 + math.sqrt(3.0) / 2.0, rel=1e-15)


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    props = [ln.split()[-1] for ln in lines if ln.startswith("property float")]
    assert "property list uchar int vertex_indices" in lines
    rows = np.frombuffer(body, dtype="<f4", count=nv * len(props)).reshape(nv, len(props))
    at, faces = 4 * nv * len(props), []
    for _ in range(nf):
        k, a, b, c = struct.unpack_from("<Biii", body, at)
        assert k == 3
        faces.append((a, b, c))
        at += 13
    assert at == len(body)
    return props, rows, np.array(faces, dtype=np.int32).reshape(-1, 3)


def read_vtk(path):
    raw = open(path, "rb").read()
    assert raw.startswith(b"# vtk DataFile Version 3.0\n")
    lines = raw.split(b"\n", 4)
    assert lines[2] == b"BINARY" and lines[3] == b"DATASET POLYDATA"
    rest = lines[4]
    head, rest = rest.split(b"\n", 1)
    word, nv, kind = head.decode().split()
    assert word == "POINTS" and kind == "float"
    nv = int(nv)
    pts = np.frombuffer(rest, dtype=">f4", count=3 * nv).reshape(nv, 3)
    rest = rest[12 * nv:]
    assert rest.startswith(b"\nPOLYGONS ")
    head, rest = rest[1:].split(b"\n", 1)
    _, nf, size = head.decode().split()
    nf = int(nf)
    assert int(size) == 4 * nf
    cells = np.frombuffer(rest, dtype=">i4", count=4 * nf).reshape(nf, 4)
    assert (cells[:, 0] == 3).all() if nf else True
    rest = rest[16 * nf:]
    normals = None
    if rest.strip():
        assert rest.startswith(f"\nPOINT_DATA {nv}\nNORMALS normals float\n".encode())
        rest = rest[len(f"\nPOINT_DATA {nv}\nNORMALS normals float\n"):]
        normals = np.frombuffer(rest, dtype=">f4", count=3 * nv).reshape(nv, 3)
        assert rest[12 * nv:] == b"\n"
    return pts, cells[:, 1:], normals


def test_writers_read_back(tmp_path):
    from nerfca_amd import mesh
    m = closed("ball")[2]
    for with_normals in (True, False):
        tm = _torch_mesh(m, with_normals)
        p = str(tmp_path / f"a{int(with_normals)}.ply")
        mesh.write_ply(p, tm)
        props, rows, faces = read_ply(p)
        assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
        assert T.same_bits(np.ascontiguousarray(rows[:, :3]), m["verts"]) and np.array_equal(faces, m["tris"])
        assert not with_normals or T.same_bits(np.ascontiguousarray(rows[:, 3:]), m["normals"])
        p = str(tmp_path / f"a{int(with_normals)}.vtk")
        mesh.write_vtk(p, tm)
        pts, cells, normals = read_vtk(p)
        assert np.array_equal(pts.astype(np.float32), m["verts"]) and np.array_equal(cells.astype(np.int32), m["tris"])
        assert (normals is not None) == with_normals and (normals is None or np.array_equal(normals.astype(np.float32), m["normals"]))
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    mesh.write_ply(str(tmp_path / "e.ply"), empty)
    mesh.write_vtk(str(tmp_path / "e.vtk"), empty)
    assert read_ply(str(tmp_path / "e.ply"))[2].shape == (0, 3) and read_vtk(str(tmp_path / "e.vtk"))[1].shape == (0, 3)
    with pytest.raises(mesh._capi.NcaError, match="outside"):
        mesh.write_ply(str(tmp_path / "bad.ply"), mesh.Mesh(torch.zeros(2, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)))


def test_the_python_layer_refuses_before_anything_touches_a_device(capi, monkeypatch):
    from nerfca_amd import export, mesh

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library")

    monkeypatch.setattr(mesh._view, "launch", no_launch)
    a = torch.zeros(4, 4, 4)
    b3 = ((0.0, 1.0),) * 3
    calls = [lambda: mesh.isosurface(a, 0.5, b3), lambda: mesh.isosurface(a.numpy(), 0.5, b3), lambda: mesh.isosurface(None, 0.5, b3),
             lambda: mesh.isosurface(a, math.nan, b3), lambda: mesh.isosurface(a, math.inf, b3), lambda: mesh.isosurface(a, 1e39, b3), lambda: mesh.isosurface(a, "high", b3),
             lambda: mesh.surface_area((a, a)), lambda: mesh.surface_area(mesh.Mesh(torch.zeros(3, 2), torch.zeros(1, 3, dtype=torch.int32))),
             lambda: mesh.enclosed_volume(mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3))), lambda: mesh.euler_characteristic(mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 4, dtype=torch.int32))),
             lambda: mesh.surface_area(mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(2, 3))), lambda: mesh.write_ply("x", None),
             lambda: export.density_surfaces(None, None, (0,), 0.5, field="both"), lambda: export.density_surfaces(None, None, (0,), 0.5)]
    for i, call in enumerate(calls):
        with pytest.raises(capi.NcaError):
            call()
    with pytest.raises(capi.NcaError, match="level = nan"):
        mesh.isosurface(a, math.nan, b3)          # the level is looked at first: before the device of vol
    with pytest.raises(capi.NcaError, match="float32"):
        mesh.isosurface(a, 1e39, b3)
    sig = inspect.signature(mesh.isosurface).parameters
    assert list(sig) == ["vol", "level", "bounds", "normals"] and sig["normals"].kind is inspect.Parameter.KEYWORD_ONLY and sig["normals"].default is False
    sig = inspect.signature(export.density_surfaces).parameters
    assert list(sig)[:4] == ["static_model", "temp_model", "phases", "level"] and sig["field"].default == "dynamic" and sig["normals"].default is False
    assert "host read" in mesh.isosurface.__doc__ and "Not differentiable" in mesh.isosurface.__doc__


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(capsys, tmp_path):
    iso = _tool("isosurface")
    args = iso.parser().parse_args(["--vol", "v.npy", "--level", "0.3", "--out", "d"])
    assert args.level == 0.3 and args.bounds is None and args.normals is False and args.format == "ply" and args.device == "cuda:0"
    args = iso.parser().parse_args(["--vol", "v.npy", "--level", "-1", "--bounds=-1,1,0,2,0.5,1.5", "--normals", "--format", "vtk", "--out", "d"])
    assert args.bounds == ((-1.0, 1.0), (0.0, 2.0), (0.5, 1.5)) and args.normals is True and args.format == "vtk" and args.level == -1.0
    mb = _tool("mesh_bench")
    args = mb.parser().parse_args(["--out", "profiles/mesh_bench.txt"])
    assert args.out == "profiles/mesh_bench.txt" and args.passes == 3 and args.sides == "256" and args.volumes == "1" and args.fields == "tree,noise" and args.normals is False
    assert mb.floors(1000, 10, 20, False) == (18000, 14000 + 120 + 240) and mb.floors(1000, 10, 20, True)[1] == 14000 + 240 + 240
    for tool, argv in ((iso, ["--help"]), (iso, ["--vol", "v.npy", "--out", "d"]), (iso, ["--vol", "v.npy", "--level", "x", "--out", "d"]),
                       (iso, ["--vol", "v.npy", "--level", "1", "--out", "d", "--bounds", "0,1,0,1"]), (iso, ["--vol", "v.npy", "--level", "1", "--out", "d", "--bounds", "1,0,0,1,0,1"]),
                       (iso, ["--vol", "v.npy", "--level", "1", "--out", "d", "--format", "stl"]), (mb, ["--help"]), (mb, ["--passes", "many"]), (mb, ["--nonsense"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    np.save(str(tmp_path / "flat.npy"), np.zeros((4, 4)))
    with pytest.raises(SystemExit) as e:
        iso.main(["--vol", str(tmp_path / "flat.npy"), "--level", "0.5", "--out", str(tmp_path / "o")])
    assert "a numeric volume" in str(e.value.code)
