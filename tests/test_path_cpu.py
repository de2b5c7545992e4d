"""Minimal paths (nca_vol_geodesic*, nca_vol_trace_paths, nca_vol_ball_cover, nerfca_amd.centreline): everything that can be checked without
a launch -- the C-ABI surface, every refusal of the entry points (with device pointers that are never read), the workspace query, the numpy
oracle of the GPU tests (tests/path_ref.py) held to the mathematics (sweeps reach a heap Dijkstra's bits, a closed form in an open box,
strictly decreasing predecessor chains, re-seeding, tubes and a blob), the plain-torch measures and the refusals of the Python layer."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import nca_testlib as T
import path_ref as ref
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_geodesic_workspace", "nca_vol_geodesic", "nca_vol_geodesic_pred", "nca_vol_trace_paths", "nca_vol_ball_cover", "nca_path_set_skip",
       "nca_path_get_skip", "nca_path_last_error")
refused = functools.partial(T.refused, "path")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_mesh_last_error(void)", "---- path:", "size_t nca_vol_geodesic_workspace(", "int nca_vol_geodesic(", "int nca_vol_geodesic_pred(",
             "int nca_vol_trace_paths(", "int nca_vol_ball_cover(", "int nca_path_set_skip(", "int nca_path_get_skip(", "nca_path_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert callable(capi.check_path)
    import nerfca_amd
    from nerfca_amd import centreline
    assert nerfca_amd.centreline is centreline and "centreline" in nerfca_amd.__all__
    for name in ("geodesic_distance", "predecessors", "trace_paths", "ball_cover", "extract", "overlap", "summary", "Centreline", "set_skip", "get_skip"):
        assert callable(getattr(centreline, name)), name
    assert "$(CSRC)/view/nca_path.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_skip_switch(capi, lib):
    assert lib.nca_path_get_skip() == 1
    for bad in (2, -1):
        refused(capi, lib, lib.nca_path_set_skip(bad), f"on = {bad}", "neither 0 nor 1")
    assert lib.nca_path_set_skip(0) == 0 and lib.nca_path_get_skip() == 0
    assert lib.nca_path_set_skip(1) == 0 and lib.nca_path_get_skip() == 1


# ----------------------------------------------------------------------------- refusals
def workspace_formula(n, n_vol):
    r = lambda b: (b + 255) // 256 * 256          # noqa: E731
    tiles = -(-n[0] // 4) * -(-n[1] // 8) * -(-n[2] // 64)
    return r(8 * n_vol * n[0] * n[1] * n[2]) + 2 * r(n_vol * tiles)


def test_geodesic_refusals(capi, lib):
    def call(g="default", n_vol=2, cost=FAKE, dist=FAKE + 64, conn=3, sweeps=2, changed=FAKE + 128, work=FAKE + 256, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_geodesic(g, n_vol, cost, dist, conn, sweeps, changed, work, work_bytes, None)

    who = "nca_vol_geodesic:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(cost=None), who, "cost is NULL")
    refused(capi, lib, call(dist=None), who, "dist is NULL")
    refused(capi, lib, call(changed=None), who, "changed is NULL")
    refused(capi, lib, call(cost=None, n_vol=0), "cost is NULL")          # pointers before n_vol
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("path", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for bad in (0, 4, -1):
        refused(capi, lib, call(conn=bad), f"conn = {bad}", "1, 2 or 3", code=E_UNSUPPORTED)
    refused(capi, lib, call(conn=0, sweeps=0), "conn = 0", code=E_UNSUPPORTED)          # conn before sweeps
    for bad in (0, -2):
        refused(capi, lib, call(sweeps=bad), f"sweeps = {bad}", "positive")
    need = lib.nca_vol_geodesic_workspace(C.byref(grid(capi)), 2)
    assert need == workspace_formula((4, 5, 6), 2)
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(sweeps=0, work=None), "sweeps = 0")          # sweeps before the workspace
    # the workspace comes before the launch limits, those before the node count
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30, work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30), "tiles", "one launch", str(2 << 30))
    refused(capi, lib, call(n=(2048, 1024, 1024), n_vol=1), who, "2^31 - 2", "2048 x 1024 x 1024", code=E_UNSUPPORTED)
    refused(capi, lib, call(n=(2048, 1024, 1024), n_vol=1, work=None), "work is NULL", code=E_WORKSPACE)
    for a in range(3):          # the tiling sets no limit on an axis
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE


def test_pred_refusals(capi, lib):
    def call(g="default", n_vol=2, cost=FAKE, dist=FAKE + 64, conn=3, pred=FAKE + 128, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_geodesic_pred(g, n_vol, cost, dist, conn, pred, None)

    who = "nca_vol_geodesic_pred:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    for name in ("cost", "dist", "pred"):
        refused(capi, lib, call(**{name: None}), who, f"{name} is NULL")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("path", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for bad in (0, 4):
        refused(capi, lib, call(conn=bad), f"conn = {bad}", code=E_UNSUPPORTED)
    refused(capi, lib, call(n=(2, 2, 1024), n_vol=1 << 30), "one launch", str(1 << 34))          # runs of 256 nodes
    refused(capi, lib, call(n=(2048, 1024, 1024), n_vol=1), who, "2^31 - 2", code=E_UNSUPPORTED)


def test_trace_refusals(capi, lib):
    def call(voxels=100, pred=FAKE, stop=None, n_paths=2, starts=FAKE + 64, max_len=5, paths=FAKE + 128, lengths=FAKE + 192, status=FAKE + 256):
        return lib.nca_vol_trace_paths(voxels, pred, stop, n_paths, starts, max_len, paths, lengths, status, None)

    who = "nca_vol_trace_paths:"
    for name in ("pred", "starts", "paths", "lengths", "status"):
        refused(capi, lib, call(**{name: None}), who, f"{name} is NULL")
    for name in ("voxels", "n_paths", "max_len"):
        for bad in (0, -4):
            refused(capi, lib, call(**{name: bad}), f"{name} = {bad}", "positive")
    refused(capi, lib, call(voxels=(1 << 31) - 1), "2^31 - 2", code=E_UNSUPPORTED)


def test_cover_refusals(capi, lib):
    def call(g="default", n_points=3, nodes=FAKE, radius=FAKE + 64, covered=FAKE + 128, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_ball_cover(g, n_points, nodes, radius, covered, None)

    who = "nca_vol_ball_cover:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    for name in ("nodes", "radius", "covered"):
        refused(capi, lib, call(**{name: None}), who, f"{name} is NULL")
    for bad in (0, -1):
        refused(capi, lib, call(n_points=bad), f"n_points = {bad}", "positive")
    refused(capi, lib, call(n=(1, 4, 4)), "n[0] = 1")
    refused(capi, lib, call(inv=(1.0, math.nan, 1.0)), "inv[1] = nan")
    refused(capi, lib, call(reserved=2), "reserved = 2")
    refused(capi, lib, call(n=(2048, 1024, 1024)), "2^31 - 2", code=E_UNSUPPORTED)


def test_workspace_query(capi, lib):
    def q(n, n_vol, **kw):
        return lib.nca_vol_geodesic_workspace(C.byref(grid(capi, n=n, **kw)), n_vol)

    assert q((2, 2, 2), 1) == 256 + 2 * 256
    for n_vol in (1, 2, 7):
        for n in ((3, 4, 5), (4, 8, 64), (5, 9, 65), (9, 17, 130), (256, 256, 256), (4, 4, 1 << 20)):
            assert q(n, n_vol) == workspace_formula(n, n_vol) and q(n, n_vol) % 256 == 0, (n, n_vol)
    assert lib.nca_vol_geodesic_workspace(None, 1) == 0
    for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1)):
        assert q(*bad) == 0, bad
    assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0


# ----------------------------------------------------------------------------- the oracle against the mathematics
@pytest.mark.parametrize("conn", (1, 2, 3))
def test_sweeps_converge_to_dijkstras_bits(conn):
    shape, inv = (5, 7, 9), (1.0, 2.0, 3.0)
    cost = ref.random_cost(shape, 21 + conn)
    assert (cost == 0).any() and not ref.is_open(cost).all()
    g = ref.Graph(cost, inv, conn)
    d0 = ref.seeded(shape, ref.random_seeds(cost, 3))
    assert same_bits(g.converge(d0)[0], g.dijkstra(d0))
    for shape in ((5, 9, 65),):          # eight tiles: the sweeps exchange values across tile faces
        cost = ref.random_cost(shape, 31 + conn)
        g = ref.Graph(cost, inv, conn)
        d0 = ref.seeded(shape, ref.random_seeds(cost, 4))
        fixed, n = g.converge(d0)
        assert n > 2 and same_bits(fixed, g.dijkstra(d0))
        assert np.isinf(fixed[~ref.is_open(cost)]).all()
        states = g.sweeps(d0, 3)          # every sweep lowers or keeps, and the count of changed tiles is that of the states
        prev = g.clean(d0).reshape(shape)
        for d, c in states:
            assert (d <= prev).all() and c > 0
            prev = d


def test_open_box_closed_form():
    """cost 1, 26 neighbours, unit spacing, from a corner: with the offsets sorted a >= b >= c the distance is c sqrt3 + (b - c) sqrt2 + (a - b)"""
    shape = (6, 7, 9)
    d = ref.geodesic(np.ones(shape, dtype=np.float32), ref.seeded(shape, [0]), (1.0, 1.0, 1.0), 3)
    for node in ((0, 0, 0), (0, 0, 8), (5, 6, 8), (3, 3, 3), (2, 6, 4), (5, 0, 7)):
        a, b, c = sorted(node, reverse=True)
        assert d[node] == pytest.approx(c * math.sqrt(3) + (b - c) * math.sqrt(2) + (a - b), rel=1e-14), node
    d6 = ref.geodesic(np.ones(shape, dtype=np.float32), ref.seeded(shape, [0]), (1.0, 2.0, 4.0), 1)
    assert d6[5, 6, 8] == 5 * 1.0 + 6 * 0.5 + 8 * 0.25          # 6 neighbours: the city-block distance in world units, exact here


@pytest.mark.parametrize("zeros", (0.0, 0.15))
@pytest.mark.parametrize("conn", (1, 2, 3))
def test_pred_chains_strictly_decrease_and_end_at_a_seed(conn, zeros):
    shape = (5, 7, 9)
    cost = ref.random_cost(shape, 41, zeros=zeros)
    seeds = ref.random_seeds(cost, 6, count=3)
    g = ref.Graph(cost, (1.0, 2.0, 3.0), conn)
    d = g.dijkstra(ref.seeded(shape, seeds))
    pred = g.pred(d).reshape(-1)
    flat = d.reshape(-1)
    assert (pred[~ref.is_open(cost).reshape(-1)] == -1).all() and (pred[seeds] == -1).all()
    zero = set(np.flatnonzero(flat == 0).tolist())
    for v in np.flatnonzero(np.isfinite(flat)):
        x, steps = int(v), 0
        while pred[x] >= 0:
            assert flat[pred[x]] < flat[x]
            x, steps = int(pred[x]), steps + 1
            assert steps <= flat.size
        if zeros == 0.0:
            assert x in seeds
        elif x not in zero:          # a zero-weight plateau: a neighbour at the same distance over an edge of weight 0
            e = g.v == x
            assert ((flat[g.u[e]] == flat[x]) & (g.w[e] == 0)).any()
    assert (pred[np.isinf(flat)] == -1).all()


def test_reseeding_from_init_equals_a_fresh_run():
    shape = (5, 9, 65)
    cost = ref.random_cost(shape, 51)
    a, b = ref.random_seeds(cost, 8), ref.random_seeds(cost, 9, count=5)
    g = ref.Graph(cost, (1.0, 2.0, 3.0), 3)
    first = g.dijkstra(ref.seeded(shape, a))
    lowered = first.copy()
    lowered.reshape(-1)[b] = 0.0
    assert same_bits(g.dijkstra(lowered), g.dijkstra(ref.seeded(shape, sorted(set(a) | set(b)))))
    assert same_bits(g.converge(lowered)[0], g.dijkstra(lowered))


def test_serpentine_needs_more_than_three_and_fewer_than_forty_sweeps():
    cost, seed = ref.serpentine()
    for inv in ref.INVS:
        for conn in (1, 2, 3):
            g = ref.Graph(cost, inv, conn)
            fixed, n = g.converge(ref.seeded(cost.shape, [seed]))
            assert 3 < n < 40, n
            assert np.isfinite(fixed[ref.is_open(cost)]).all() and same_bits(fixed, g.dijkstra(ref.seeded(cost.shape, [seed])))


def test_trace_and_cover_of_the_oracle():
    pred = np.array([-1, 0, 1, 2, 5, 4, 99, -1], dtype=np.int32)          # 4 <-> 5 is a cycle, 6 points outside
    stop = np.zeros(8, dtype=np.uint8)
    stop[1] = 1
    paths, lens, status = ref.trace(pred, [3, 3, 4, 8, -2, 6], None, 4)
    assert paths.tolist() == [[3, 2, 1, 0], [3, 2, 1, 0], [4, 5, 4, 5], [-1] * 4, [-1] * 4, [6, -1, -1, -1]]
    assert lens.tolist() == [4, 4, 4, 0, 0, 1] and status.tolist() == [0, 0, 2, 3, 3, 0]
    paths, lens, status = ref.trace(pred, [3, 7, 1], stop, 3)
    assert paths.tolist() == [[3, 2, 1], [7, -1, -1], [1, -1, -1]] and status.tolist() == [1, 0, 1]
    assert ref.trace(pred, [3, 0], None, 1)[2].tolist() == [2, 0]
    cov = ref.cover(np.zeros((5, 5, 5), dtype=np.uint8), [62, -1], [0.0, 9.0], (1.0, 1.0, 1.0))
    assert cov.sum() == 1 and cov[2, 2, 2] == 1
    cov = ref.cover(cov, [62], [1.0], (1.0, 2.0, 4.0))          # spacings 1, 0.5, 0.25: reach 1, 2 and 4 nodes
    assert cov[1, 2, 2] and cov[2, 4, 2] and cov[2, 2, 0] and not cov[0, 2, 2] and not cov[1, 3, 2]
    x = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1) - 2
    assert cov.sum() == int((((x * np.array([1.0, 0.5, 0.25])) ** 2).sum(-1) <= 1.0).sum())          # all distances here are exact
    assert ref.cover(np.zeros((3, 4, 5), dtype=np.uint8), [0], [1e9], (1.0, 1.0, 1.0)).all()


def test_tubes_and_blob():
    straight = ref.tube((9, 9, 40), (((4, 4, 4), (4, 4, 35), 3.0),))
    paths, parents, radii, lens, reached = ref.extract(straight, ref.bounds_of((9, 9, 40), (1.0,) * 3), 0.5)
    assert len(paths) == 1 and parents == [(-1, -1)] and reached == 1.0
    i0, i1, i2 = np.unravel_index(paths[0], straight.shape)
    # from the tip in the far cap, off the axis, in three steps onto the axis, then along it, every node once, to the root at the first end
    assert len(paths[0]) == 34 and i2.tolist() == list(range(37, 3, -1))
    assert (i0[0], i1[0]) == (2, 3) and (i0[1], i1[1]) == (3, 3) and (i0[2], i1[2]) == (3, 3)
    assert (i0[3:] == 4).all() and (i1[3:] == 4).all()          # exactly on the axis from i2 = 34 to the end at i2 = 4
    assert lens[0] == pytest.approx(30.0 + 1.0 + math.sqrt(2.0) + math.sqrt(3.0), rel=1e-12) and radii[0][-1] == np.float32(math.sqrt(10.0))          # the nearest node off the mask is (3, 1) off the axis

    blob = np.zeros((4, 5, 6), dtype=np.float32)
    blob[1:3, 1:4, 1:5] = 1.0
    paths, parents, _, _, _ = ref.extract(blob, ref.bounds_of(blob.shape, (1.0,) * 3), 0.5)
    assert len(paths) == 1 and len(paths[0]) == 4

    # the Y of ref.Y_SEGMENTS (fork at (8, 16, 40)): the node counts, the join, the ends and the lengths of this geometry, pinned
    pinned = {ref.Y_INVS[0]: ([66, 25], (0, 24), [(7, 28, 68), (8, 5, 66)], (8, 17, 44), [70.28839999367293, 28.14213562373095]),
              ref.Y_INVS[1]: ([66, 26], (0, 23), [(8, 27, 68), (7, 4, 65)], (8, 18, 45), [85.10859165294033, 33.30781059358212])}
    for inv in ref.Y_INVS:
        vol = ref.tube(ref.Y_SHAPE, ref.Y_SEGMENTS, inv)
        paths, parents, radii, lens, reached = ref.extract(vol, ref.bounds_of(ref.Y_SHAPE, inv), 0.5)
        counts, parent, tips, join, lengths = pinned[inv]
        assert [len(p) for p in paths] == counts and parents == [(-1, -1), parent] and reached == 1.0
        assert [tuple(int(v) for v in np.unravel_index(int(p[0]), ref.Y_SHAPE)) for p in paths] == tips
        assert np.unravel_index(int(paths[0][-1]), ref.Y_SHAPE) == (8, 16, 3)          # the root: the deepest node, smallest index
        assert tuple(int(v) for v in np.unravel_index(int(paths[1][-1]), ref.Y_SHAPE)) == join and paths[0][parent[1]] == paths[1][-1]
        assert lens == pytest.approx(lengths, rel=1e-13)
        assert not set(paths[1][:-1].tolist()) & set(paths[0].tolist())
        assert all(r.min() > 0 for r in radii) and radii[0].max() >= 3.0          # on the mask, through the trunk's axis


# ----------------------------------------------------------------------------- the plain-torch measures and the Python layer
def test_overlap_and_summary():
    from nerfca_amd import centreline
    a = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [5.0, 0.0, 0.0], [9.0, 0.0, 0.0]])
    b = torch.tensor([[0.0, 0.5, 0.0], [5.0, 0.0, 0.2]])
    assert centreline.overlap(a, b, 0.5) == (0.5, 1.0)
    assert centreline.overlap(a, b, 0.1) == (0.0, 0.0)
    assert centreline.overlap(a, b, 2.0) == (0.75, 1.0)
    assert centreline.overlap(a, torch.zeros((0, 3)), 1.0) == (0.0, 0.0)
    c = centreline.Centreline([torch.tensor([3, 2, 1], dtype=torch.int32), torch.tensor([7, 2], dtype=torch.int32)], [torch.zeros(3, 3), torch.zeros(2, 3)],
                              [torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.5, 2.0])], [(-1, -1), (0, 1)], [2.0, 1.5], 0.75)
    s = centreline.summary(c)
    assert s["branches"] == 2 and s["total_length"] == 3.5 and s["reached"] == 0.75
    assert s["paths"][0] == {"nodes": 3, "length": 2.0, "radius_min": 1.0, "radius_mean": 2.0, "radius_max": 3.0, "parent": [-1, -1]}
    assert s["paths"][1]["radius_mean"] == 1.25 and s["paths"][1]["parent"] == [0, 1]


def test_python_layer_refusals(capi):
    from nerfca_amd import centreline as cl
    cpu = torch.zeros((3, 4, 5))

    def no(fn, *words):
        with pytest.raises(capi.NcaError) as e:
            fn()
        for w in words:
            assert w in str(e.value), str(e.value)

    no(lambda: cl.geodesic_distance(cpu, None, seeds=[0]), "GPU")
    no(lambda: cl.geodesic_distance(np.zeros((3, 4, 5)), None, seeds=[0]), "not a tensor")
    no(lambda: cl.geodesic_distance(cpu, None, seeds=[0], connectivity=4), "connectivity = 4")
    no(lambda: cl.geodesic_distance(cpu, None, seeds=[0], sweeps=0), "sweeps = 0")
    no(lambda: cl.geodesic_distance(cpu, None, seeds=[0], batch=-1), "batch = -1")
    no(lambda: cl.predecessors(cpu, cpu.double(), None, connectivity=0), "connectivity = 0")
    no(lambda: cl.predecessors(cpu, cpu.double(), None), "GPU")
    no(lambda: cl.trace_paths(cpu.int(), [0], max_len=0), "max_len = 0")
    no(lambda: cl.trace_paths(cpu, [0], max_len=3), "int32")
    no(lambda: cl.trace_paths(cpu.int(), [0], max_len=3), "GPU")
    no(lambda: cl.ball_cover(cpu, [0], [1.0], None), "uint8")
    no(lambda: cl.ball_cover(cpu.to(torch.uint8), [0], [1.0], None), "GPU")
    no(lambda: cl.extract(cpu, None, threshold=0.5), "GPU")
    no(lambda: cl.extract(np.zeros(3), None, threshold=0.5), "not a tensor")


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_write_vtk_polylines_byte_layout(tmp_path, capi):
    from nerfca_amd import mesh
    points = [np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.0], [2.0, 1.0, -1.0]], dtype=np.float32), torch.tensor([[1.0, 0.5, 0.0], [1.0, 2.0, 3.0]])]
    radius = [np.array([1.0, 0.75, 0.5], dtype=np.float32), torch.tensor([0.75, 0.25])]
    mesh.write_vtk_polylines(tmp_path / "tree.vtk", points, radius)
    raw = (tmp_path / "tree.vtk").read_bytes()
    head = b"# vtk DataFile Version 3.0\ncentreline\nBINARY\nDATASET POLYDATA\nPOINTS 5 float\n"
    assert raw.startswith(head)
    at = len(head)
    assert np.array_equal(np.frombuffer(raw, ">f4", 15, at).reshape(5, 3), np.concatenate([points[0], points[1].numpy()]))
    at += 60
    lines = b"\nLINES 2 7\n"
    assert raw[at:at + len(lines)] == lines
    at += len(lines)
    assert np.frombuffer(raw, ">i4", 7, at).tolist() == [3, 0, 1, 2, 2, 3, 4]          # a count, then the point numbers, per polyline
    at += 28
    data = b"\nPOINT_DATA 5\nSCALARS radius float 1\nLOOKUP_TABLE default\n"
    assert raw[at:at + len(data)] == data
    at += len(data)
    assert np.frombuffer(raw, ">f4", 5, at).tolist() == [1.0, 0.75, 0.5, 0.75, 0.25] and raw[at + 20:] == b"\n"
    mesh.write_vtk_polylines(tmp_path / "bare.vtk", points)
    assert b"POINT_DATA" not in (tmp_path / "bare.vtk").read_bytes()
    mesh.write_vtk_polylines(tmp_path / "none.vtk", [], [])
    assert b"POINTS 0 float" in (tmp_path / "none.vtk").read_bytes()
    with pytest.raises(capi.NcaError):
        mesh.write_vtk_polylines(tmp_path / "bad.vtk", points, [radius[0]])


def test_command_lines(tmp_path, capsys):
    ct, pb, ps = _tool("centreline"), _tool("path_bench"), _tool("phantom_study")
    args = ct.parser().parse_args(["--vol", "v.npy", "--threshold", "0.3", "--bounds=-1,1,-1,1,-1,1", "--root", "0.5,-0.25,0", "--vtk", "--out", "d"])
    assert args.bounds == ((-1.0, 1.0),) * 3 and args.root == (0.5, -0.25, 0.0) and args.vtk and args.max_paths == 256 and args.const is None
    for argv in (["--help"], ["--vol", "v.npy", "--out", "d"], ["--vol", "v.npy", "--threshold", "0.3", "--out", "d", "--root", "1,2"],
                 ["--vol", "v.npy", "--threshold", "0.3", "--out", "d", "--root", "1,2,inf"]):
        with pytest.raises(SystemExit) as e:
            ct.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    bad = tmp_path / "stack.npy"
    np.save(bad, np.zeros((2, 4, 4, 4), dtype=np.float32))          # ONE volume: refused before a device is asked for
    with pytest.raises(SystemExit) as e:
        ct.main(["--vol", str(bad), "--threshold", "0.5", "--out", str(tmp_path / "o")])
    assert "n0, n1, n2" in str(e.value.code)
    args = pb.parser().parse_args(["--out", "profiles/path_bench.txt"])
    assert args.sides == "128,256" and args.volumes == "1,10" and args.passes == 3
    assert len(pb.offsets()) == 26 and pb.offsets() == ref.offsets(3)
    flag = torch.zeros((2, 5, 9, 65), dtype=torch.bool)
    flag[0, 4, 0, 0] = flag[1, 0, 8, 64] = flag[1, 3, 7, 63] = True
    tiles = pb.tile_map(flag)
    assert tuple(tiles.shape) == (2, 2, 2, 2) and tiles.nonzero().tolist() == [[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 1, 1]]
    assert ps.parser().parse_args([]).centreline is False and ps.parser().parse_args(["--centreline"]).centreline is True
    table = np.array([[0, 0, 0, 1, 0, 0, 0.2, 0.1], [1, 0, 0, 2, 0, 0, 0.1, 0.1], [1, 0, 0, 1, 1, 0, 0.1, 0.05]], dtype=np.float64)
    pts, rad, leaves = ps.truth_tree(table, 0.5)
    assert pts.shape == (9, 3) and rad.tolist() == [0.2, 0.15000000000000002, 0.1, 0.1, 0.1, 0.1, 0.1, 0.07500000000000001, 0.05] and leaves == 2
    from nerfca_amd import phantom
    assert np.array_equal(pts, phantom.centreline_points(table, 0.5)[0])
