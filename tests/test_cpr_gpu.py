"""nca_vol_sample_planes and nca_vol_lumen on the GPU against the numpy transcription of the header (tests/cpr_ref.py), bit for bit: out,
radius, stats and status.  The shapes are the smallest that cross every seam: volumes (9, 12, 70) and (5, 6, 7), one and three of them,
unit and anisotropic spacing; planes of 1 x 1, 3 x 5 and 17 x 17 pixels (the last across the 16-pixel tile seam), one and five of them,
oblique, partly and wholly outside the grid, on nodes and on the last node; NaN and infinite nodes, a NaN fill; fans of 4, 64 and 258 rays
(the last beyond the workgroup's 256 threads) of 1 and 200 steps.  Then the same bits on a second run, the two wrappers under graph
capture, and reformat.along on the Y tube of tests/path_ref.py.

A NaN the arithmetic PRODUCES (inf - inf, 0 * inf) has the sign the processor gives it, which IEEE 754 leaves open: where both sides hold
a NaN they agree (`same_or_nan`); everything else, a NaN or an infinity copied at order 0 and the fill's payload included, is held bit
for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cpr_ref as ref
import nca_testlib as T
import path_ref
from nca_testlib import dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345
PIXEL = (0.7, 0.45)          # du, dv


def same_or_nan(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    kind = {4: np.int32, 8: np.int64}[want.dtype.itemsize]
    return bool(((got.view(kind) == want.view(kind)) | (np.isnan(got) & np.isnan(want))).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def gpu_planes(dev, vol, inv, order, origin, e1, e2, nu, nv, du, dv, fill):
    """One raw nca_vol_sample_planes on the f32 stack vol [n_vol, n0, n1, n2]: f32 [n_vol, K, nu, nv] as numpy; `out` is pre-filled, so a pixel
    the kernel did not write shows.  At order 3 the coefficients come from ccta.spline_filter."""
    from nerfca_amd import _capi, ccta, fused
    x = _dev(np.asarray(vol, dtype=np.float32), dev)
    src = ccta.spline_filter(x) if order == 3 else x
    o, a, b = (_dev(np.asarray(v, dtype=np.float64), dev) for v in (origin, e1, e2))
    out = torch.full((x.shape[0], o.shape[0], nu, nv), 1234.5, dtype=torch.float32, device=dev)
    g = T.grid_of(vol.shape[-3:], inv)
    with torch.cuda.device(dev):
        _capi.check_cpr(_capi.lib().nca_vol_sample_planes(C.byref(g), x.shape[0], _capi.ptr(src), order, o.shape[0], _capi.ptr(o), _capi.ptr(a), _capi.ptr(b), nu, nv, du, dv,
                                                          fill, _capi.ptr(out), fused._stream()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def gpu_lumen(dev, vol, inv, origin, e1, e2, n_ang, level, dr, n_steps):
    """One raw nca_vol_lumen: (radius f32 [n_vol, K, n_ang], stats f64 [n_vol, K, 4], status int32 [n_vol, K]) as numpy, each pre-filled."""
    from nerfca_amd import _capi, fused
    x = _dev(np.asarray(vol, dtype=np.float32), dev)
    o, a, b = (_dev(np.asarray(v, dtype=np.float64), dev) for v in (origin, e1, e2))
    dirs = _dev(ref.directions(n_ang), dev)
    k = o.shape[0]
    radius = torch.full((x.shape[0], k, n_ang), 1234.5, dtype=torch.float32, device=dev)
    stats = torch.full((x.shape[0], k, 4), 1234.5, dtype=torch.float64, device=dev)
    status = torch.full((x.shape[0], k), -7, dtype=torch.int32, device=dev)
    g = T.grid_of(vol.shape[-3:], inv)
    with torch.cuda.device(dev):
        _capi.check_cpr(_capi.lib().nca_vol_lumen(C.byref(g), x.shape[0], _capi.ptr(x), k, _capi.ptr(o), _capi.ptr(a), _capi.ptr(b), n_ang, _capi.ptr(dirs), ref.sin_step(n_ang),
                                                  level, dr, n_steps, _capi.ptr(radius), _capi.ptr(stats), _capi.ptr(status), fused._stream()))
    torch.cuda.synchronize(dev)
    return radius.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()


# ----------------------------------------------------------------------------- the planes
@pytest.mark.parametrize("n_planes", (1, 5))
@pytest.mark.parametrize("size", ref.PLANE_SIZES)
@pytest.mark.parametrize("n_vol,inv", ((1, ref.INVS[0]), (3, ref.INVS[1])))
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_oblique_planes_have_the_transcriptions_bits(dev, shape, n_vol, inv, size, n_planes):
    vol = ref.volumes(shape, n_vol, seed=size[0])
    origin, e1, e2 = ref.oblique_planes(shape, ref.LO, inv, n_planes, seed=10 * size[0] + n_planes, spread=1.1)          # inside, partly and wholly outside
    nu, nv = size
    for order in (0, 1, 3):
        want = ref.sample_planes(vol, ref.LO, inv, order, origin, e1, e2, nu, nv, *PIXEL, -2.5)
        got = gpu_planes(dev, vol, inv, order, origin, e1, e2, nu, nv, *PIXEL, -2.5)
        assert T.same_bits(got, want), (order, int((got != want).sum()), float(np.abs(got - want).max()))


def test_the_planes_cover_inside_outside_and_the_tile_seam(dev):
    """What the cases above rely on, and a plane wholly outside, one that the grid's face cuts, and a second run with the same bits."""
    shape, inv = ref.SHAPES[0], ref.INVS[1]
    vol = ref.volumes(shape, 3, seed=9)
    origin, e1, e2 = ref.oblique_planes(shape, ref.LO, inv, 5, seed=22, spread=1.4)
    origin[0] = np.array(ref.LO) - 50.0                                           # wholly outside
    origin[1] = ref.node_to_world((4, 5, 69), ref.LO, inv)                        # on the last node of axis 2: the face cuts the plane
    _, inside = ref.world_to_grid(ref.plane_points(origin, e1, e2, 17, 17, *PIXEL), ref.LO, inv, shape)
    assert not inside[0].any() and inside[1].any() and not inside[1].all() and inside[1, 8, 8]
    assert inside[:, 16, :].any() and inside[:, :, 16].any()                      # the seventeenth row and column hold pixels inside
    for order in (0, 1, 3):
        want = ref.sample_planes(vol, ref.LO, inv, order, origin, e1, e2, 17, 17, *PIXEL, 0.25)
        got = gpu_planes(dev, vol, inv, order, origin, e1, e2, 17, 17, *PIXEL, 0.25)
        assert T.same_bits(got, want), order
        assert (got[:, 0] == 0.25).all()
        assert T.same_bits(gpu_planes(dev, vol, inv, order, origin, e1, e2, 17, 17, *PIXEL, 0.25), got)          # the same bits on a second run


@pytest.mark.parametrize("inv", ref.INVS)
def test_planes_on_nodes_return_the_slices(dev, inv):
    shape = ref.SHAPES[1]
    vol = ref.volumes(shape, 3, seed=1)
    for axis in range(3):
        origin, e1, e2, nu, nv, du, dv = ref.axis_planes(shape, ref.LO, inv, axis, list(range(shape[axis])))          # the last plane included
        slices = np.ascontiguousarray(np.moveaxis(vol, 1 + axis, 1))
        for order in (0, 1):
            assert T.same_bits(gpu_planes(dev, vol, inv, order, origin, e1, e2, nu, nv, du, dv, math.nan), slices), (axis, order)
        got = gpu_planes(dev, vol, inv, 3, origin, e1, e2, nu, nv, du, dv, math.nan)
        assert T.same_bits(got, ref.sample_planes(vol, ref.LO, inv, 3, origin, e1, e2, nu, nv, du, dv, math.nan)) and T.ulp_distance(got, slices).max() <= 1.0, axis


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_nan_and_infinite_nodes_and_a_nan_fill(dev, shape):
    inv = ref.INVS[1]
    vol = ref.volumes(shape, 3, seed=4, special=True)
    fill = float(np.array([POISON], dtype=np.int32).view(np.float32)[0])          # a NaN with a payload
    planes = [ref.oblique_planes(shape, ref.LO, inv, 5, seed=31, spread=1.2) + (3, 5), ref.oblique_planes(shape, ref.LO, inv, 5, seed=32, spread=1.2) + (17, 17),
              ref.axis_planes(shape, ref.LO, inv, 0, [0, shape[0] - 1, shape[0]])[:5]]
    for origin, e1, e2, nu, nv in planes:
        du, dv = (1.0 / inv[1], 1.0 / inv[2]) if nu == shape[1] else PIXEL
        _, inside = ref.world_to_grid(ref.plane_points(origin, e1, e2, nu, nv, du, dv), ref.LO, inv, shape)
        for order in (0, 1, 3):
            want = ref.sample_planes(vol, ref.LO, inv, order, origin, e1, e2, nu, nv, du, dv, fill)
            got = gpu_planes(dev, vol, inv, order, origin, e1, e2, nu, nv, du, dv, fill)
            assert same_or_nan(got, want), order
            assert (got[:, ~inside].view(np.int32) == POISON).all() and not inside.all()          # the fill's own bits
            if order == 0:
                assert T.same_bits(got, want)          # copies: exact, the NaN and the infinities included
    special = ~np.isfinite(ref.sample_planes(vol, ref.LO, inv, 0, *planes[2], 1.0 / inv[1], 1.0 / inv[2], 0.0))
    assert special.any()          # the node planes do pass through special nodes


# ----------------------------------------------------------------------------- the lumen
def _lumen_case(name, special=False):
    """(vol, inv, origin, e1, e2, level, dr): "tube": three noisy tubes along axis 2 of (9, 12, 70) at unit spacing, planes along the axis in
    random orientation -- rays cross the wall near 3 and, with 200 steps, leave the thin grid; "noise": one volume (5, 6, 7) of normal data at
    anisotropic spacing, planes inside and outside -- centres outside the lumen and outside the grid."""
    if name == "tube":
        shape, inv = ref.SHAPES[0], ref.INVS[0]
        field = ref.tube_field(shape, ref.LO, inv, ref.node_to_world((4, 5.5, -9), ref.LO, inv), ref.node_to_world((4, 5.5, 90), ref.LO, inv), 3.0)
        vol = field[None] + 0.3 * ref.volumes(shape, 3, seed=6)
        origin, e1, e2 = ref.oblique_planes(shape, ref.LO, inv, 5, seed=41, spread=0.0)
        origin = origin + np.array([[0.0, 0.0, z] for z in (-30.0, -11.3, 0.4, 12.9, 33.0)])
        level, dr = 0.0, 0.05
    else:
        shape, inv = ref.SHAPES[1], ref.INVS[1]
        vol = ref.volumes(shape, 1, seed=7)
        origin, e1, e2 = ref.oblique_planes(shape, ref.LO, inv, 5, seed=42, spread=0.9)
        origin[3] = ref.node_to_world(np.unravel_index(int(vol[0].argmin()), shape), ref.LO, inv)          # a centre outside the lumen
        origin[4] = np.array(ref.LO) - 1.0          # a centre outside the grid
        level, dr = 0.0, 0.03
    if special:
        vol = vol.copy()
        rng = np.random.default_rng(77)
        for q in range(vol.shape[0]):
            for val in (np.nan, np.inf, -np.inf) * 6:
                vol[q][tuple(int(rng.integers(0, s)) for s in shape)] = val
    return vol.astype(np.float32), inv, origin, e1, e2, level, dr


@pytest.mark.parametrize("n_steps", (1, 200))
@pytest.mark.parametrize("n_ang", (4, 64, 258))
@pytest.mark.parametrize("name", ("tube", "noise"))
def test_lumen_has_the_transcriptions_bits(dev, name, n_ang, n_steps):
    vol, inv, origin, e1, e2, level, dr = _lumen_case(name)
    want_radius, want_stats, want_status, _ = ref.lumen(vol, ref.LO, inv, origin, e1, e2, n_ang, level, dr, n_steps)
    radius, stats, status = gpu_lumen(dev, vol, inv, origin, e1, e2, n_ang, level, dr, n_steps)
    assert np.array_equal(status, want_status), (status.tolist(), want_status.tolist())
    assert T.same_bits(radius, want_radius), int((radius != want_radius).sum())
    assert np.array_equal(stats.view(np.int64), want_stats.view(np.int64)), np.abs(stats - want_stats).max()
    again = gpu_lumen(dev, vol, inv, origin, e1, e2, n_ang, level, dr, n_steps)          # the same bits on a second run
    assert T.same_bits(again[0], radius) and np.array_equal(again[1].view(np.int64), stats.view(np.int64)) and np.array_equal(again[2], status)


def test_lumen_cases_reach_every_ending():
    """What the cases above rely on: every status bit and the plain crossing occur, per ray"""
    seen = set()
    for name, n_steps in (("tube", 1), ("tube", 200), ("noise", 200)):
        vol, inv, origin, e1, e2, level, dr = _lumen_case(name)
        for q in range(vol.shape[0]):
            r, bits = ref.rays(vol[q], ref.LO, inv, origin, e1, e2, ref.directions(64), level, dr, n_steps)
            seen |= set(np.unique(bits).tolist())
            assert n_steps == 1 or ((bits == 0) & (r > 0)).any()
    assert seen == {0, ref.CENTRE, ref.OPEN, ref.GRID}


@pytest.mark.parametrize("name", ("tube", "noise"))
def test_lumen_with_nan_and_infinite_nodes(dev, name):
    vol, inv, origin, e1, e2, level, dr = _lumen_case(name, special=True)
    want_radius, want_stats, want_status, _ = ref.lumen(vol, ref.LO, inv, origin, e1, e2, 64, level, dr, 200)
    radius, stats, status = gpu_lumen(dev, vol, inv, origin, e1, e2, 64, level, dr, 200)
    assert np.array_equal(status, want_status) and same_or_nan(radius, want_radius) and same_or_nan(stats, want_stats)
    assert not np.array_equal(want_radius, ref.lumen(_lumen_case(name)[0], ref.LO, inv, origin, e1, e2, 64, level, dr, 200)[0])          # the special nodes are met


# ----------------------------------------------------------------------------- the wrappers
def test_wrappers_against_the_transcription(dev):
    from nerfca_amd import reformat as R
    shape, inv = ref.SHAPES[0], ref.INVS[1]
    bounds = tuple((ref.LO[a], ref.LO[a] + (shape[a] - 1) / inv[a]) for a in range(3))
    assert ref.inv_of(shape, bounds) == inv
    vol = ref.volumes(shape, 6, seed=12).reshape((2, 3) + shape)
    x = _dev(vol, dev)
    pts = np.array([ref.node_to_world(n, ref.LO, inv) for n in ((1, 2, 3), (3, 5, 20), (6, 7, 41), (7, 9, 66))])
    fr = R.frames(pts, step=7.0)
    for order in (0, 1, 3):
        got = R.cross_sections(x, bounds, fr, size=(3, 17), spacing=(0.7, 0.45), order=order, fill=-1.0)
        assert tuple(got.shape) == (2, 3, len(fr.s), 3, 17)
        want = ref.sample_planes(vol.reshape((6,) + shape), ref.LO, inv, order, fr.origin, fr.e1, fr.e2, 3, 17, 0.7, 0.45, -1.0)
        assert T.same_bits(got.cpu().numpy().reshape(want.shape), want), order
    on_dev = R.to_device(fr, dev)
    assert all(isinstance(f, torch.Tensor) and f.dtype == torch.float64 and f.device == x.device for f in on_dev)
    assert torch.equal(R.cross_sections(x, bounds, on_dev, size=5, spacing=0.5), R.cross_sections(x, bounds, fr, size=5, spacing=0.5))
    prof = R.lumen_profile(x, bounds, fr, level=0.2, r_max=4.1, n_angles=12)
    dr = 0.5 * min(1.0 / v for v in inv)
    radius, stats, status, _ = ref.lumen(vol.reshape((6,) + shape), ref.LO, inv, fr.origin, fr.e1, fr.e2, 12, 0.2, dr, math.ceil(4.1 / dr))
    assert tuple(prof.radius.shape) == (2, 3, len(fr.s), 12) and tuple(prof.d_eq.shape) == (2, 3, len(fr.s)) and prof.status.dtype == torch.int32
    assert T.same_bits(prof.radius.cpu().numpy().reshape(radius.shape), radius) and np.array_equal(prof.status.cpu().numpy().reshape(status.shape), status)
    for k, name in enumerate(("area", "d_min", "d_max")):
        assert np.array_equal(getattr(prof, name).cpu().numpy().reshape(-1), stats[..., k].reshape(-1)), name
    assert np.allclose(prof.d_eq.cpu().numpy().reshape(-1), 2.0 * np.sqrt(stats[..., 0].reshape(-1) / math.pi), rtol=1e-15, atol=0)
    assert np.array_equal(prof.s.cpu().numpy(), fr.s)
    with pytest.raises(R._capi.NcaError, match="frames.origin is on"):
        R.cross_sections(x, bounds, R.to_device(fr, "cpu"), size=5, spacing=0.5)


def _poison(t):
    t.view(-1).view(torch.uint8)[:t.numel() * t.element_size() // 4 * 4].view(torch.int32).fill_(POISON)


def _poisoned(t):
    return bool((t.view(-1).view(torch.uint8)[:t.numel() * t.element_size() // 4 * 4].view(torch.int32) == POISON).all())


@pytest.mark.parametrize("what", ("sections_1", "sections_3", "lumen"))
def test_captured_wrappers_replay_to_the_eager_result(dev, what):
    """As tests/test_graph_replay_gpu.py does for the other sections: an eager warm-up on a side stream, one capture, then for each input
    of nca_testlib's sequence (the last one twice) the input copied into the static tensor, every output poisoned, a replay, and the bytes
    of an eager call on a fresh tensor."""
    from nerfca_amd import reformat as R
    shape = T.REPLAY_TILE_SHAPE
    bounds = tuple((0.0, float(n - 1)) for n in shape)
    host = R.frames(np.array([[0.5, 1.0, 2.0], [2.0, 4.0, 30.0], [3.5, 7.0, 63.0]]), step=5.0)
    fr = R.to_device(host, dev)

    def run(vol):
        if what == "lumen":
            p = R.lumen_profile(vol, bounds, fr, level=T.REPLAY_THRESHOLD, r_max=3.0, n_angles=64)
            return {"radius": p.radius, "area": p.area.contiguous(), "d_min": p.d_min.contiguous(), "d_max": p.d_max.contiguous(), "d_eq": p.d_eq, "status": p.status}
        return {"out": R.cross_sections(vol, bounds, fr, size=17, spacing=0.5, order=int(what[-1]), fill=-1.0)}

    inputs = [_dev(T.replay_volumes(shape, k), dev) for k in range(T.REPLAY_INPUTS)]
    static = inputs[0].clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    torch.cuda.synchronize()
    results = []
    for i, k in enumerate(list(range(T.REPLAY_INPUTS)) + [T.REPLAY_INPUTS - 1]):
        static.copy_(inputs[k])
        for t in outs.values():
            _poison(t)
        torch.cuda.synchronize()
        assert all(_poisoned(t) for t in outs.values())
        graph.replay()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            eager = run(inputs[k].clone())
        side.synchronize()
        for name, want in eager.items():
            got = outs[name]
            assert got.shape == want.shape and got.dtype == want.dtype and not _poisoned(got), (name, i)
            assert torch.equal(got.contiguous().view(-1).view(torch.uint8), want.contiguous().view(-1).view(torch.uint8)), (what, name, "replay", i, "input", k)
        results.append({n: t.clone() for n, t in outs.items()})
    first = next(iter(outs))
    assert not torch.equal(results[0][first], results[1][first]) and torch.equal(results[2][first], results[3][first])          # the inputs do move the outputs


def test_along_on_the_y_tube(dev):
    """One record per path of the tree; away from the junction and from the paths' ends (by 6, twice the trunk's radius) every plane finds
    the wall in every direction, and the equivalent diameter is the tube's within the half node a binary mask leaves open."""
    from nerfca_amd import centreline, reformat as R
    inv = path_ref.Y_INVS[0]
    vol = path_ref.tube(path_ref.Y_SHAPE, path_ref.Y_SEGMENTS, inv)
    bounds = path_ref.bounds_of(path_ref.Y_SHAPE, inv)
    x = _dev(vol, dev)
    tree = centreline.extract(x, bounds, threshold=0.5)
    assert [int(p.numel()) for p in tree.paths] == [66, 25]          # as tests/test_path_cpu.py pins them
    per = R.along(x, bounds, tree, level=0.5, r_max=6.0, size=9, spacing=0.5, dr=0.5)
    assert len(per) == 2 and all(set(one) == {"frames", "sections", "profile", "stenosis"} for one in per)
    fork = np.array(path_ref.Y_SEGMENTS[0][1], dtype=np.float64)
    for one, diameters in zip(per, ((5.0, 6.0), (4.0,))):
        fr, prof = one["frames"], one["profile"]
        k = len(fr.s)
        assert tuple(one["sections"].shape) == (k, 9, 9) and tuple(prof.radius.shape) == (k, 64) and len(one["stenosis"]) == 1
        away = (fr.s >= 6.0) & (fr.s <= fr.s[-1] - 6.0) & (np.linalg.norm(fr.origin - fork, axis=1) > 6.0)
        status, d_eq = prof.status.cpu().numpy(), prof.d_eq.cpu().numpy()
        assert away.sum() >= 10 and not status[away].any(), status.tolist()
        assert all(min(abs(d - want) for want in diameters) < 1.0 for d in d_eq[away]), d_eq[away].tolist()          # half a node on either side
        assert (one["sections"][torch.from_numpy(away).to(dev), 4, 4] > 0.5).all()          # the centre pixel lies in the vessel
        radius, stats, want_status, _ = ref.lumen(vol[None], (0.0, 0.0, 0.0), inv, fr.origin, fr.e1, fr.e2, 64, 0.5, 0.5, 12)
        assert T.same_bits(prof.radius.cpu().numpy(), radius[0]) and np.array_equal(status, want_status[0])
        assert one["stenosis"][0]["excluded"] == int((status != 0).sum())
