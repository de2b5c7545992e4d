"""Minimal paths on the GPU: nca_vol_geodesic, nca_vol_geodesic_pred, nca_vol_trace_paths and nca_vol_ball_cover and nerfca_amd.centreline
against the numpy transcription of the definition (tests/path_ref.py, held to the mathematics in tests/test_path_cpu.py).  Every comparison
is bit for bit: f64 fields as int64 words, node lists as int32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import nca_testlib as T
import path_ref as ref
from nca_testlib import dev  # noqa: F401

pytestmark = pytest.mark.gpu

LO = (0.0, -1.0, 2.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def grid_of(shape, inv):
    from nerfca_amd import _capi
    return T.grid(_capi, n=shape, lo=LO, inv=inv)


def geodesic(dev, shape, inv, cost, dist, conn, sweeps, skip=True):
    """(dist f64 [n_vol, ...], changed [n_vol]) of ONE raw call on stacks [n_vol, n0, n1, n2]; the workspace is exactly the query's and poisoned"""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    g = grid_of(shape, inv)
    c = torch.tensor(np.ascontiguousarray(cost, dtype=np.float32)).to(dev)
    d = torch.tensor(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    n_vol = c.shape[0]
    nbytes = lib.nca_vol_geodesic_workspace(C.byref(g), n_vol)
    assert nbytes >= 8 * c.numel() and nbytes % 256 == 0
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    changed = torch.full((n_vol,), -7, dtype=torch.int32, device=dev)
    assert lib.nca_path_set_skip(1 if skip else 0) == 0
    try:
        with torch.cuda.device(dev):
            _capi.check_path(lib.nca_vol_geodesic(C.byref(g), n_vol, _capi.ptr(c), _capi.ptr(d), conn, sweeps, _capi.ptr(changed), _capi.ptr(work), nbytes, fused._stream()))
        torch.cuda.synchronize(dev)
    finally:
        lib.nca_path_set_skip(1)
    return d.cpu().numpy(), changed.cpu().numpy()


def pred_of(dev, shape, inv, cost, dist, conn):
    from nerfca_amd import _capi, fused
    g = grid_of(shape, inv)
    c = torch.tensor(np.ascontiguousarray(cost, dtype=np.float32)).to(dev)
    d = torch.tensor(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    out = torch.full(c.shape, -9, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check_path(_capi.lib().nca_vol_geodesic_pred(C.byref(g), c.shape[0], _capi.ptr(c), _capi.ptr(d), conn, _capi.ptr(out), fused._stream()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(shape, inv, conn):
    """(cost, the seeded field, the reference's states after 1, 2, 3 sweeps with their changed counts, its fixed point, its sweep count)"""
    if shape == ref.SERPENTINE:
        cost, seed = ref.serpentine()
        seeds = [seed]
    else:
        cost = ref.random_cost(shape, 100 + shape[2])
        seeds = ref.random_seeds(cost, 17)
    g = ref.Graph(cost, inv, conn)
    d0 = ref.seeded(shape, seeds)
    fixed, n = g.converge(d0)
    return cost, d0, g.sweeps(d0, 3), fixed, n, g


@pytest.mark.parametrize("inv", ref.INVS)
@pytest.mark.parametrize("conn", (1, 2, 3))
@pytest.mark.parametrize("shape", ref.GRIDS + (ref.SERPENTINE,))
def test_states_after_1_2_3_sweeps_and_converged(dev, shape, conn, inv):
    cost, d0, states, fixed, n, g = case(shape, inv, conn)
    assert (cost == 0).any() or shape == (2, 2, 2)
    if shape == ref.SERPENTINE:
        assert 3 < n < 40, n
    for skip in (True, False):
        for s, (want, want_changed) in enumerate(states, start=1):
            got, changed = geodesic(dev, shape, inv, cost[None], d0[None], conn, s, skip)
            assert same(got[0], want), (shape, conn, inv, skip, s)
            assert changed.tolist() == [want_changed], (skip, s)
        got, changed = geodesic(dev, shape, inv, cost[None], d0[None], conn, n, skip)
        assert same(got[0], fixed) and changed.tolist() == [0], (shape, conn, inv, skip)
        assert np.isinf(got[0][~ref.is_open(cost)]).all()
        if n > 1:
            assert geodesic(dev, shape, inv, cost[None], d0[None], conn, n - 1, skip)[1][0] > 0          # not a sweep sooner
    assert same(fixed, g.dijkstra(d0))


def test_seed_on_a_wall_no_seed_and_walls_with_finite_input(dev):
    shape, inv = (5, 9, 65), ref.INVS[0]
    cost = ref.random_cost(shape, 165)
    wall = int(np.flatnonzero(~ref.is_open(cost).reshape(-1))[3])
    g = ref.Graph(cost, inv, 3)
    got, changed = geodesic(dev, shape, inv, cost[None], ref.seeded(shape, [wall])[None], 3, 2)
    assert np.isinf(got).all() and changed.tolist() == [0]          # the wall went to +inf in the first sweep, nothing moved in the second
    got, changed = geodesic(dev, shape, inv, cost[None], ref.seeded(shape, [wall])[None], 3, 1)
    assert np.isinf(got).all() and changed.tolist() == [1] and g.sweep(ref.seeded(shape, [wall]))[1] == 1
    got, changed = geodesic(dev, shape, inv, cost[None], ref.seeded(shape, [])[None], 3, 1)
    assert np.isinf(got).all() and changed.tolist() == [0]
    field = np.random.default_rng(5).random(shape) * 30.0          # any non-negative field: finite on walls too
    want, n = g.converge(field)
    got, changed = geodesic(dev, shape, inv, cost[None], field[None], 3, n)
    assert same(got[0], want) and changed.tolist() == [0]
    for s, (w, c) in enumerate(g.sweeps(field, 2), start=1):
        got, changed = geodesic(dev, shape, inv, cost[None], field[None], 3, s)
        assert same(got[0], w) and changed.tolist() == [c]


def test_two_volumes_resumed_runs_and_the_same_bits_twice(dev):
    shape, inv, conn = (5, 9, 65), ref.INVS[0], 2
    costs = np.stack([ref.random_cost(shape, 201), ref.random_cost(shape, 202, walls=0.55)])
    graphs = [ref.Graph(c, inv, conn) for c in costs]
    d0 = np.stack([ref.seeded(shape, ref.random_seeds(c, 9)) for c in costs])
    for skip in (True, False):
        for s in (1, 3, 7):
            got, changed = geodesic(dev, shape, inv, costs, d0, conn, s, skip)
            for v in range(2):
                want, c = graphs[v].sweeps(d0[v], s)[-1]
                assert same(got[v], want) and changed[v] == c, (skip, s, v)
        three, _ = geodesic(dev, shape, inv, costs, d0, conn, 3, skip)
        seven, changed7 = geodesic(dev, shape, inv, costs, d0, conn, 7, skip)
        resumed, changed34 = geodesic(dev, shape, inv, costs, three, conn, 4, skip)
        assert same(resumed, seven) and changed34.tolist() == changed7.tolist()
        again, _ = geodesic(dev, shape, inv, costs, d0, conn, 7, skip)
        assert same(again, seven)
    assert len({graphs[v].converge(d0[v])[1] for v in range(2)}) == 2          # the two volumes converge at different sweeps
    n = max(graphs[v].converge(d0[v])[1] for v in range(2))
    got, changed = geodesic(dev, shape, inv, costs, d0, conn, n)
    assert changed.tolist() == [0, 0] and all(same(got[v], graphs[v].dijkstra(d0[v])) for v in range(2))


@pytest.mark.parametrize("conn", (1, 2, 3))
def test_predecessors(dev, conn):
    for shape in ((5, 9, 65), ref.SERPENTINE, (2, 2, 2)):
        for inv in ref.INVS:
            cost, d0, states, fixed, n, g = case(shape, inv, conn)
            for field in (fixed, states[1][0]):          # converged, and a state that is not
                got = pred_of(dev, shape, inv, cost[None], field[None], conn)[0]
                assert got.dtype == np.int32 and np.array_equal(got, g.pred(field)), (shape, inv, conn)


def test_python_geodesic_distance_and_predecessors(dev):
    from nerfca_amd import centreline as cl
    shape, inv = (5, 9, 65), (1.0, 2.0, 3.0)
    bounds = ref.bounds_of(shape, inv)
    inv = ref.inv_of(shape, bounds)
    costs = np.stack([ref.random_cost(shape, 301), ref.random_cost(shape, 302)])
    seeds = np.zeros(costs.shape, dtype=bool)
    for v in range(2):
        seeds[v].reshape(-1)[ref.random_seeds(costs[v], 3)] = True
    want = [ref.Graph(costs[v], inv, 3).dijkstra(np.where(seeds[v], 0.0, np.inf)) for v in range(2)]
    c = torch.tensor(costs).to(dev)
    for batch in (1, 5, 16):
        dist, changed = cl.geodesic_distance(c, bounds, seeds=torch.tensor(seeds).to(dev), batch=batch)
        assert dist.dtype == torch.float64 and dist.shape == c.shape and changed.tolist() == [0, 0]
        assert all(same(dist[v].cpu().numpy(), want[v]) for v in range(2)), batch
    flat = np.flatnonzero(seeds.reshape(-1))
    two, changed = cl.geodesic_distance(c, bounds, seeds=torch.tensor(flat).to(dev), sweeps=2)
    for v in range(2):
        w, n = ref.Graph(costs[v], inv, 3).sweeps(np.where(seeds[v], 0.0, np.inf), 2)[-1]
        assert same(two[v].cpu().numpy(), w) and int(changed[v]) == n
    more, _ = cl.geodesic_distance(c, bounds, init=two)          # continued to the same fixed point
    assert all(same(more[v].cpu().numpy(), want[v]) for v in range(2))
    pred = cl.predecessors(c, more, bounds)
    assert pred.dtype == torch.int32 and all(np.array_equal(pred[v].cpu().numpy(), ref.Graph(costs[v], inv, 3).pred(want[v])) for v in range(2))
    with pytest.raises(RuntimeError):
        cl.geodesic_distance(c, bounds)


def test_trace_paths(dev):
    from nerfca_amd import centreline as cl
    pred = np.array([-1, 0, 1, 2, 5, 4, 99, -1, 3, -(2 ** 31)], dtype=np.int32)          # 4 <-> 5 is a cycle; 6 and 9 point outside
    stop = np.zeros(10, dtype=np.uint8)
    stop[1] = 1
    p = torch.tensor(pred).to(dev)
    for starts, st, max_len in (([3, 8, 4, 10, -2, 6, 9, 2 ** 40], None, 4), ([3, 7, 1, 8, 5], stop, 3), ([3, 0, 4, 1], stop, 1), ([4, 5], None, 7)):
        want = ref.trace(pred, starts, st, max_len)
        got = cl.trace_paths(p, torch.tensor(starts, dtype=torch.int64).to(dev), stop=None if st is None else torch.tensor(st).to(dev), max_len=max_len)
        for g, w in zip(got, want):
            assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (starts, max_len)
    paths, lengths, status = (t.cpu().numpy() for t in cl.trace_paths(p, [3, 4, 10, 1], stop=torch.tensor(stop).to(dev), max_len=5))
    assert status.tolist() == [1, 2, 3, 1] and lengths.tolist() == [3, 5, 0, 1]          # every status but 0 ...
    assert cl.trace_paths(p, [0], max_len=5)[2].tolist() == [0]                          # ... and 0
    assert paths[1].tolist() == [4, 5, 4, 5, 4]          # the cycle: max_len nodes, status 2


def test_ball_cover(dev):
    from nerfca_amd import centreline as cl
    shape = (7, 9, 70)
    for inv in ((1.0, 1.0, 1.0), (1.0, 2.0, 4.0), (0.8, 1.0, 1.25)):
        bounds = ref.bounds_of(shape, inv)
        inv_b = ref.inv_of(shape, bounds)
        nodes = [0, -1, 3 * 9 * 70 + 4 * 70 + 35, 7 * 9 * 70 - 1, -5, 2 * 9 * 70 + 8 * 70 + 66, 100]
        radius = [0.0, 5.0, 2.5, 1.0, 3.0, 3.2, float("nan")]
        start = np.zeros(shape, dtype=np.uint8)
        start[6, 0, 0] = 1          # only ever set
        got = cl.ball_cover(torch.tensor(start).to(dev), torch.tensor(nodes).to(dev), torch.tensor(radius), bounds)
        want = ref.cover(start, nodes, radius, inv_b)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want) and want[6, 0, 0] == 1 and want[0, 0, 0] == 1
        assert 10 < want.sum() < want.size // 2
    whole = cl.ball_cover(torch.zeros(shape, dtype=torch.uint8, device=dev), [5], [1e6], None)          # a radius past the grid
    assert bool(whole.all())
    none = cl.ball_cover(torch.zeros(shape, dtype=torch.uint8, device=dev), [-1, -3], [4.0, 4.0], None)
    assert not bool(none.any())


def check_extract(dev, vol, bounds, **kw):
    from nerfca_amd import centreline as cl, metrics
    shape = vol.shape
    R = metrics.distance_transform(torch.tensor(vol).to(dev), bounds, threshold=0.5, inside=True).cpu().numpy()
    scipy_R = ref.edt_inside(vol > 0.5, ref.inv_of(shape, bounds))
    print("distance transform: device vs scipy rounded to f32, nodes that differ:", int((R.view(np.int32) != scipy_R.view(np.int32)).sum()))
    want = ref.extract(vol, bounds, 0.5, R=R, **kw)          # the loop is held to the reference on the device's own R ...
    got = cl.extract(torch.tensor(vol).to(dev), bounds, threshold=0.5, **kw)
    assert len(got.paths) == len(want[0])
    for k in range(len(want[0])):
        assert got.paths[k].dtype == torch.int32 and np.array_equal(got.paths[k].cpu().numpy(), want[0][k]), k
        assert T.same_bits(got.radius[k].cpu().numpy(), want[2][k])
        assert got.length[k] == pytest.approx(want[3][k], rel=1e-12)
        ijk = np.stack(np.unravel_index(want[0][k], shape), axis=1)
        world = np.array([b[0] for b in bounds]) + ijk / np.array(ref.inv_of(shape, bounds))
        assert np.allclose(got.points[k].cpu().numpy(), world, rtol=1e-6, atol=1e-6) and got.points[k].dtype == torch.float32
    assert [tuple(p) for p in got.parent] == [tuple(p) for p in want[1]] and got.reached == want[4]
    loose = ref.extract(vol, bounds, 0.5, **kw)          # ... and with scipy's R the tree has the same branches
    assert [len(p) for p in loose[0]] == [len(p) for p in want[0]] and loose[1] == want[1]
    return got


@pytest.mark.parametrize("inv", ref.Y_INVS)
def test_extract_y_tube(dev, inv):
    from nerfca_amd import centreline as cl
    vol = ref.tube(ref.Y_SHAPE, ref.Y_SEGMENTS, inv)
    got = check_extract(dev, vol, ref.bounds_of(ref.Y_SHAPE, inv))
    assert len(got.paths) == 2 and got.parent[0] == (-1, -1) and got.parent[1][0] == 0 and got.reached == 1.0
    s = cl.summary(got)
    assert s["branches"] == 2 and s["total_length"] == pytest.approx(sum(got.length))
    assert cl.overlap(torch.cat(got.points), torch.cat(got.points), 1e-6) == (1.0, 1.0)


def test_extract_phantom_tree_with_a_given_root(dev):
    from nerfca_amd import phantom
    shape = (33, 33, 33)
    bounds = ((-1.0, 1.0),) * 3
    segments = np.array([[-0.8, 0.0, 0.0, 0.0, 0.0, 0.0, 0.2, 0.16], [0.0, 0.0, 0.0, 0.6, 0.5, 0.1, 0.14, 0.1], [0.0, 0.0, 0.0, 0.55, -0.5, -0.2, 0.12, 0.1]])
    vol = phantom.voxelize(shape, bounds, segments=segments, rho_vessel=1.0, device=dev)[0].cpu().numpy()
    got = check_extract(dev, vol, bounds, root=(-0.8, 0.0, 0.0))
    assert len(got.paths) == 2 and got.parent[1][0] == 0
    first = got.points[0][-1].cpu().numpy()
    assert np.abs(first - np.array([-0.8, 0.0, 0.0])).max() <= 1.0 / 16 + 1e-6          # the first path ends at the root


def test_captured_geodesic_replays_to_the_eager_result(dev):
    """nca_vol_geodesic with sweeps = 4, captured on a side stream and replayed on three inputs over poisoned dist, changed and workspace."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    shape, inv, n_vol, conn, sweeps = T.REPLAY_TILE_SHAPE, (1.0, 2.0, 3.0), 2, 3, 4
    g = grid_of(shape, inv)
    nbytes = lib.nca_vol_geodesic_workspace(C.byref(g), n_vol)
    costs = [np.stack([ref.random_cost(shape, 400 + 10 * k + v) for v in range(n_vol)]) for k in range(T.REPLAY_INPUTS)]
    fields = [np.stack([ref.seeded(shape, ref.random_seeds(c[v], k)) for v in range(n_vol)]) for k, c in enumerate(costs)]

    def buffers():
        return {"cost": torch.empty((n_vol,) + shape, dtype=torch.float32, device=dev), "init": torch.empty((n_vol,) + shape, dtype=torch.float64, device=dev),
                "dist": torch.empty((n_vol,) + shape, dtype=torch.float64, device=dev), "changed": torch.empty((n_vol,), dtype=torch.int32, device=dev),
                "work": torch.empty((nbytes,), dtype=torch.uint8, device=dev)}

    def load(b, k):
        b["cost"].copy_(torch.tensor(costs[k]))
        b["init"].copy_(torch.tensor(fields[k]))
        for n in ("dist", "changed", "work"):
            b[n].view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize(dev)

    def sequence(b):
        b["dist"].copy_(b["init"])
        _capi.check_path(lib.nca_vol_geodesic(C.byref(g), n_vol, b["cost"].data_ptr(), b["dist"].data_ptr(), conn, sweeps, b["changed"].data_ptr(), b["work"].data_ptr(),
                                              nbytes, torch.cuda.current_stream().cuda_stream))

    with torch.cuda.device(dev):
        static = buffers()
        load(static, 0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sequence(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            sequence(static)
        torch.cuda.synchronize(dev)
        for k in (0, 1, 2, 2):
            load(static, k)
            graph.replay()
            torch.cuda.synchronize(dev)
            fresh = buffers()
            load(fresh, k)
            sequence(fresh)
            torch.cuda.synchronize(dev)
            for v in range(n_vol):
                want, c = ref.Graph(costs[k][v], inv, conn).sweeps(fields[k][v], sweeps)[-1]
                assert same(fresh["dist"][v].cpu().numpy(), want) and int(fresh["changed"][v]) == c
            assert torch.equal(static["dist"].view(torch.int64), fresh["dist"].view(torch.int64)) and torch.equal(static["changed"], fresh["changed"]), k


def test_extract_refuses_a_volume_wholly_above_the_threshold_and_returns_nothing_for_an_empty_mask(dev):
    from nerfca_amd import _capi, centreline as cl
    with pytest.raises(_capi.NcaError) as e:
        cl.extract(torch.ones((5, 6, 7), device=dev), None, threshold=0.5)
    assert "above threshold" in str(e.value)
    assert cl.extract(torch.zeros((5, 6, 7), device=dev), None, threshold=0.5).paths == []
    with pytest.raises(_capi.NcaError) as e:
        cl.extract(torch.tensor(ref.tube(ref.Y_SHAPE, ref.Y_SEGMENTS)).to(dev), None, threshold=0.5, root=(0.0, 0.0, 0.0))
    assert "not on the mask" in str(e.value)


def test_command_line_writes_the_tree(dev, tmp_path, capsys):
    import importlib.util
    import json
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("centreline_tool", os.path.join(ROOT, "tools", "centreline.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    inv = ref.Y_INVS[1]
    bounds = ref.bounds_of(ref.Y_SHAPE, inv)
    vol = ref.tube(ref.Y_SHAPE, ref.Y_SEGMENTS, inv)
    np.save(tmp_path / "v.npy", vol)
    out = tmp_path / "o"
    tool.main(["--vol", str(tmp_path / "v.npy"), "--threshold", "0.5", "--bounds=" + ",".join(repr(v) for b in bounds for v in b), "--vtk", "--out", str(out), "--device", str(dev)])
    record = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = ref.extract(vol, bounds, 0.5)
    paths, points, radius = np.load(out / "paths.npy"), np.load(out / "points.npy"), np.load(out / "radius.npy")
    assert paths.dtype == np.int32 and paths.shape == (2, 66) and points.shape == (2, 66, 3) and radius.shape == (2, 66)
    for k in range(2):
        n = len(want[0][k])
        assert np.array_equal(paths[k, :n], want[0][k]) and (paths[k, n:] == -1).all() and np.isnan(points[k, n:]).all() and np.isnan(radius[k, n:]).all()
        assert T.same_bits(radius[k, :n], want[2][k])
    assert record["branches"] == 2 and record["paths"][1]["parent"] == list(want[1][1]) and json.load(open(out / "summary.json")) == record
    raw = (out / "tree.vtk").read_bytes()
    assert b"POINTS 92 float" in raw and b"LINES 2 94" in raw and b"SCALARS radius float 1" in raw
