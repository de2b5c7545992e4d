"""The phantom rasteriser on the GPU: nca_phantom_voxelize against the f64 numpy transcription of its definition (tests/phantom_ref.py), with
tile-level culling on and off, and nerfca_amd.phantom end to end into drr and synthetic.

The bound of every comparison: |out - want64| <= 2^-24 |want64| + 2^-52 * 4 max(1, L / edge) * mass, L the diagonal of the bounds and
mass = sum |rho_e| + |rho_v|.  The first term is the one rounding to f32.  The second allows for a device square root or division that is
an ulp off the host's: an ulp of t moves the closest point by at most 2^-52 L, so d by as much and cov by that over edge; with correctly
rounded intrinsics it is never used.  Culling, a second run and a shuffled table must not change a bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev, same_bits  # noqa: F401

import phantom_ref as ref

pytestmark = pytest.mark.gpu

BOUNDS = ref.BOUNDS
EDGE = 0.11
RHO_V = ref.RHO_V


def seg_counts():
    from nerfca_amd import phantom
    return (0, 1, 7, 2 * phantom.SEG_BATCH + 3)


@functools.lru_cache(maxsize=None)
def tables(P, n_ell, n_seg):
    ell = ref.random_ellipsoids(P, n_ell, BOUNDS, seed=100 + 10 * P + n_ell) if n_ell else None
    # few segments are thick, so that they meet nodes of the coarsest grid; many are thin, so that they do not fill the volume
    seg = ref.random_segments(P, n_seg, BOUNDS, seed=200 + 10 * P + n_seg, r_max=0.35 if n_seg <= 7 else 0.04) if n_seg else None
    return ell, seg


@functools.lru_cache(maxsize=None)
def oracle(shape, P, n_ell, n_seg):
    ell, seg = tables(P, n_ell, n_seg)
    return ref.voxelize(shape, BOUNDS, ell, seg, RHO_V, EDGE)


def gpu_voxelize(dev, shape, ell, seg, rho_v, edge, cull, bounds=BOUNDS):
    """out f32 [P,n0,n1,n2] (numpy) of one nca_phantom_voxelize into a buffer pre-filled with NaN, with culling set to `cull`."""
    from nerfca_amd import _capi, drr, fused
    lib = _capi.lib()
    P = (ell if ell is not None else seg).shape[0]
    d_ell = None if ell is None else torch.from_numpy(np.ascontiguousarray(ell)).to(dev)
    d_seg = None if seg is None else torch.from_numpy(np.ascontiguousarray(seg)).to(dev)
    out = torch.full((P,) + tuple(shape), math.nan, dtype=torch.float32, device=dev)
    desc = drr.grid_desc(shape, bounds)
    old = lib.nca_phantom_get_cull()
    _capi.check_phantom(lib.nca_phantom_set_cull(int(cull)))
    try:
        with torch.cuda.device(dev):
            _capi.check_phantom(lib.nca_phantom_voxelize(C.byref(desc), P, 0 if ell is None else ell.shape[1], _capi.ptr(d_ell),
                                                         0 if seg is None else seg.shape[1], _capi.ptr(d_seg), rho_v, edge, _capi.ptr(out), fused._stream()))
        return out.cpu().numpy()
    finally:
        _capi.check_phantom(lib.nca_phantom_set_cull(old))


def check(got, want64, mass, edge, bounds=BOUNDS):
    assert got.shape == want64.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} nodes were not written"          # the buffer started as NaN
    err = np.abs(got.astype(np.float64) - want64)
    tol = ref.bound(want64, mass, bounds, edge)
    assert (err <= tol).all(), (float((err - tol).max()), np.unravel_index(np.argmax(err - tol), err.shape))
    exact = np.abs(got.astype(np.float64) - want64.astype(np.float32).astype(np.float64)).max()
    return float(exact)


# ----------------------------------------------------------------------------- 1. parity
CONFIGS = [(5, 0), (5, 1), (5, 7), (5, "2B+3"), (0, 7)]          # (ellipsoids, segments)


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: f"ell{c[0]}-seg{c[1]}")
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_f64_oracle_and_culling_changes_no_bit(dev, shape, P, config):
    n_ell, n_seg = config
    n_seg = seg_counts()[-1] if n_seg == "2B+3" else n_seg
    ell, seg = tables(P, n_ell, n_seg)
    want64, mass = oracle(shape, P, n_ell, n_seg)
    on = gpu_voxelize(dev, shape, ell, seg, RHO_V, EDGE, cull=1)
    off = gpu_voxelize(dev, shape, ell, seg, RHO_V, EDGE, cull=0)
    beyond_f32 = check(on, want64, mass, EDGE)
    check(off, want64, mass, EDGE)
    assert same_bits(on, off)
    if n_seg >= 7:          # the case is not empty, and not saturated either
        cov = want64 / RHO_V if not n_ell else None
        assert (want64 != 0).any() and (cov is None or ((cov > 0) & (cov < 1)).any())
    print(f"grid {shape}, P {P}, {n_ell} ellipsoids, {n_seg} segments: largest distance from the oracle rounded to f32 {beyond_f32:.3e}")


# ----------------------------------------------------------------------------- 2. special segments
def special_segments(shape):
    """(name, row) of segments at the places where the kernel takes another path; edge is SPECIAL_EDGE."""
    xs = ref.node_positions(shape, BOUNDS)
    h = ref.spacing(shape, BOUNDS)
    lo = [b[0] for b in BOUNDS]
    hi = [b[1] for b in BOUNDS]
    rows = [("degenerate", [0.1, 0.2, -0.1, 0.1, 0.2, -0.1, 0.15, 0.15]),
            ("degenerate, unequal radii", [-0.3, 0.0, 0.2, -0.3, 0.0, 0.2, 0.2, 0.05]),
            ("outside", [2.0, 2.5, 1.9, 2.4, 2.6, 2.2, 0.3, 0.1]),
            ("rb = 0", [-0.5, -0.4, -0.6, 0.4, 0.5, 0.3, 0.1, 0.0]),
            ("both radii 0", [-0.5, 0.5, -0.6, 0.4, -0.5, 0.3, 0.0, 0.0])]
    tile_edge = {0: 3, 1: 7, 2: 63}          # the last node of the first tile on each axis
    for axis, idx in tile_edge.items():
        along = (axis + 1) % 3
        for delta in (-2.0 ** -30, 0.0, 2.0 ** -30, 1e-3):
            # in the plane half-way between the two tiles, reaching the first node on either side by a relative delta
            a, b = [0.5 * (lo[k] + hi[k]) for k in range(3)], [0.5 * (lo[k] + hi[k]) for k in range(3)]
            a[axis] = b[axis] = xs[axis][idx] + 0.5 * h[axis]
            a[along], b[along] = lo[along] - 0.1, hi[along] + 0.1
            r = 0.5 * h[axis] * (1 + delta) - 0.5 * SPECIAL_EDGE
            rows.append((f"between the tiles of axis {axis}, delta {delta:g}", a + b + [r, r]))
            # in the first node plane of the second tile, reaching one node into the first tile
            a, b = list(a), list(b)
            a[axis] = b[axis] = xs[axis][idx + 1]
            r = h[axis] * (1 + delta) - 0.5 * SPECIAL_EDGE
            rows.append((f"on the first plane of the second tile of axis {axis}, delta {delta:g}", a + b + [r, r]))
    assert all(row[6] >= 0 and row[7] >= 0 for _, row in rows)
    return [(name, np.array(row, dtype=np.float64)) for name, row in rows]


SPECIAL_SHAPE = (9, 17, 70)
SPECIAL_EDGE = 0.02


def test_special_segments(dev):
    rows = special_segments(SPECIAL_SHAPE)
    for name, row in rows + [("all together", np.stack([r for _, r in rows]))]:
        seg = row.reshape(1, -1, 8)
        want64, mass = ref.voxelize(SPECIAL_SHAPE, BOUNDS, None, seg, RHO_V, SPECIAL_EDGE)
        on = gpu_voxelize(dev, SPECIAL_SHAPE, None, seg, RHO_V, SPECIAL_EDGE, cull=1)
        off = gpu_voxelize(dev, SPECIAL_SHAPE, None, seg, RHO_V, SPECIAL_EDGE, cull=0)
        check(on, want64, mass, SPECIAL_EDGE)
        assert same_bits(on, off), name
        if name == "outside":
            assert not on.any() and not want64.any()          # exact zeros
        elif want64.max() > 1e-6:
            assert on.max() > 0, name


# ----------------------------------------------------------------------------- 3. the same bits
def test_two_runs_and_a_shuffled_table_give_the_same_bits(dev):
    shape, P = (9, 17, 70), 3
    n_seg = seg_counts()[-1]
    ell, seg = tables(P, 5, n_seg)
    first = gpu_voxelize(dev, shape, ell, seg, RHO_V, EDGE, cull=1)
    for cull in (1, 0):
        assert same_bits(first, gpu_voxelize(dev, shape, ell, seg, RHO_V, EDGE, cull=cull))
        perm = np.random.default_rng(9).permutation(n_seg)
        assert not np.array_equal(perm, np.arange(n_seg))
        assert same_bits(first, gpu_voxelize(dev, shape, ell, seg[:, perm], RHO_V, EDGE, cull=cull))          # a maximum: the order is free


def test_voxelize_broadcasts_a_2d_table_and_defaults_the_edge(dev):
    from nerfca_amd import phantom
    shape, P = (9, 17, 70), 3
    ell, seg = tables(1, 5, 7)[0][0], tables(P, 0, 7)[1]
    once = phantom.voxelize(shape, BOUNDS, ellipsoids=ell, segments=seg, rho_vessel=RHO_V, device=dev)
    rep = phantom.voxelize(shape, BOUNDS, ellipsoids=np.stack([ell] * P), segments=seg, rho_vessel=RHO_V, device=dev)
    assert once.shape == (P,) + shape and once.dtype == torch.float32 and once.device == dev and torch.equal(once, rep)
    edge = ref.default_edge(shape, BOUNDS)          # the coarsest node spacing
    want64, mass = ref.voxelize(shape, BOUNDS, np.stack([ell] * P), seg, RHO_V, edge)
    check(once.cpu().numpy(), want64, mass, edge)
    assert same_bits(once.cpu().numpy(), gpu_voxelize(dev, shape, np.stack([ell] * P), seg, RHO_V, edge, cull=0))
    only = phantom.voxelize(shape, BOUNDS, segments=seg[0], rho_vessel=RHO_V, edge=EDGE, device=dev)          # one phase, no ellipsoids
    check(only.cpu().numpy(), *ref.voxelize(shape, BOUNDS, None, seg[:1], RHO_V, EDGE), EDGE)


# ----------------------------------------------------------------------------- 4. end to end
N_DET, S, PHASES, SIDE = 16, 32, 4, 24


def test_make_phantom_projects_and_makes_a_dataset(dev):
    from nerfca_amd import drr, phantom, synthetic
    geo = synthetic.xcat_geometry(N_DET)
    ph = phantom.make_phantom((SIDE,) * 3, PHASES, geo, device=dev)
    assert set(ph) == {"static", "dynamic", "bounds", "ellipsoids", "segments"}
    hw = phantom.fov_half_width(geo)
    assert ph["bounds"] == ((-hw, hw),) * 3
    static, dynamic = ph["static"], ph["dynamic"]
    assert static.shape == (SIDE,) * 3 and dynamic.shape == (PHASES,) + (SIDE,) * 3 and static.dtype == dynamic.dtype == torch.float32
    assert ph["ellipsoids"].shape == (5, 14) and ph["segments"].shape[0] == PHASES and ph["segments"].shape[2] == 8
    assert torch.isfinite(static).all() and torch.isfinite(dynamic).all() and static.min() >= 0 and dynamic.min() == 0 and dynamic.max() > 0
    edge = ref.default_edge((SIDE,) * 3, ph["bounds"])
    want64, mass = ref.voxelize((SIDE,) * 3, ph["bounds"], None, ph["segments"], phantom.RHO_VESSEL, edge)
    check(dynamic.cpu().numpy(), want64, mass, edge, ph["bounds"])

    out = drr.project_sequence(static, dynamic, geo, synthetic.TRAIN_VIEWS, S, bounds=ph["bounds"])
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    pred, pred_s, pred_d = out["pred"], out["pred_static"], out["pred_dynamic"]
    assert pred.shape == pred_d.shape == (4, PHASES, N_DET, N_DET) and pred_s.shape == (4, N_DET, N_DET)
    for p in range(PHASES):          # the static part is the same at every phase: pred = (static + dynamic) - I0
        assert ((pred[:, p] - pred_d[:, p] + i0) - pred_s).abs().max() <= 8 * 2.0 ** -24 * i0
    assert not torch.equal(pred_d[:, 0], pred_d[:, 2])          # the vessels moved
    deficit_s, deficit_d = float((i0 - pred_s).max()), float((i0 - pred_d).max())
    print(f"pred in [{float(pred.min()):.4f}, {float(pred.max()):.4f}], I0 {i0:.4f}; largest deficit: static {deficit_s:.4f}, vessels {deficit_d:.4f}")
    assert pred.min() > 0
    assert deficit_d >= 0.1 * deficit_s

    data = synthetic.make_dataset(n_det=N_DET, S=S, device=dev, n_phases=PHASES, teacher=(static, dynamic), render=drr.volume_teacher(ph["bounds"]))
    assert data.n_images == 4 * PHASES and torch.isfinite(data.rays_train).all() and torch.isfinite(data.test_image).all()
    weights = data.rays_train[:, 3, 0]
    assert weights.min() >= 1.0 and weights.max() > 2.0 - 1e-6          # the temporal variance reaches its maximum somewhere: a vessel moved
    assert len(data.var_ray_ids) > 0

    errs = phantom.volume_errors(dynamic, dynamic.clone(), 0.5 * phantom.RHO_VESSEL)
    assert errs == {"rmse": 0.0, "dice": 1.0}
    shifted = phantom.volume_errors(dynamic.roll(1, 0), dynamic, 0.25 * phantom.RHO_VESSEL)
    assert shifted["rmse"] > 0 and 0 <= shifted["dice"] < 1
