"""The procedural phantom (nca_phantom_voxelize, nerfca_amd.phantom): everything that can be checked without a launch -- the C-ABI surface,
every refusal of the entry points (with pointers that are never read), the f64 oracle of the GPU tests (tests/phantom_ref.py) on its own,
the host-side generator, and the refusals of the Python layer, which look at the host tables before any device is touched."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import phantom_ref as ref
import nca_testlib as T
from nca_testlib import FAKE, capi, grid, lib  # noqa: F401

NEW = ("nca_phantom_voxelize", "nca_phantom_set_cull", "nca_phantom_get_cull", "nca_phantom_last_error")
refused = functools.partial(T.refused, "phantom")


@pytest.fixture(scope="module")
def phantom():
    from nerfca_amd import phantom
    return phantom


def test_new_names_are_declared_bound_and_exported(capi, phantom):
    header = T.declared_bound_and_exported(capi, NEW)
    assert header.index("nca_vol_last_error(void)") < header.index("int nca_phantom_voxelize(") < header.index("int nca_phantom_set_cull(") \
        < header.index("nca_phantom_last_error(void)")
    assert int(re.search(r"NCA_PHANTOM_SEG_BATCH = (\d+)", header).group(1)) == phantom.SEG_BATCH
    assert callable(capi.check_phantom)
    import nerfca_amd
    assert nerfca_amd.phantom is phantom and "phantom" in nerfca_amd.__all__


def test_refusals(capi, lib):
    def call(g="default", n_phase=1, n_ell=2, ell=FAKE, n_seg=3, seg=FAKE, rho_v=1.0, edge=0.1, out=FAKE):
        g = grid(capi) if g == "default" else g
        return lib.nca_phantom_voxelize(C.byref(g) if g is not None else None, n_phase, n_ell, ell, n_seg, seg, rho_v, edge, out, None)

    who = "nca_phantom_voxelize:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    refused(capi, lib, call(n_phase=0), "n_phase = 0")
    refused(capi, lib, call(n_phase=-3), "n_phase = -3")
    refused(capi, lib, call(n_ell=-1), "n_ell = -1")
    refused(capi, lib, call(n_seg=-7), "n_seg = -7")
    refused(capi, lib, call(n_ell=0, n_seg=0), "n_ell = 0", "n_seg = 0")
    refused(capi, lib, call(ell=None), "ell is NULL", "n_ell = 2")
    refused(capi, lib, call(seg=None), "seg is NULL", "n_seg = 3")
    for bad, word in ((0.0, "0"), (-1e-3, "-0.001"), (math.inf, "inf"), (-math.inf, "-inf"), (math.nan, "nan")):
        refused(capi, lib, call(edge=bad), f"edge = {word}", "positive")
    for bad, word in ((math.inf, "inf"), (-math.inf, "-inf"), (math.nan, "nan")):
        refused(capi, lib, call(rho_v=bad), f"rho_v = {word}", "finite")
    T.grid_refusals("phantom", capi, lib, lambda g, count: call(g=g, n_phase=count or 1))
    # 2^50 voxels fit int64, but make 2^39 tiles of 4 x 8 x 64 nodes: more than the 2^31 - 1 blocks of one launch
    refused(capi, lib, call(g=grid(capi, n=(1 << 20, 1 << 20, 1 << 10))), "tiles", "one launch", str(1 << 39))
    # 2^30 tiles pass alone and are too many with 2 phases: the phase is an outer grid dimension of the same launch
    refused(capi, lib, call(g=grid(capi, n=(1 << 17, 1 << 17, 1 << 7)), n_phase=2), "tiles", "one launch", str(1 << 30))
    # the optional tables: a count of 0 takes a NULL table, and is then refused for what comes next, not for the pointer
    refused(capi, lib, call(n_ell=0, ell=None, edge=0.0), "edge = 0")
    refused(capi, lib, call(n_seg=0, seg=None, edge=0.0), "edge = 0")


def test_set_cull_round_trips_and_refuses(capi, lib):
    old = lib.nca_phantom_get_cull()
    assert old in (0, 1)
    try:
        for v in (0, 1, 0):
            assert lib.nca_phantom_set_cull(v) == 0 and lib.nca_phantom_get_cull() == v
        for bad in (2, -1, 7):
            refused(capi, lib, lib.nca_phantom_set_cull(bad), "nca_phantom_set_cull", f"on = {bad}")
            assert lib.nca_phantom_get_cull() == 0
    finally:
        assert lib.nca_phantom_set_cull(old) == 0


# ----------------------------------------------------------------------------- the oracle on its own
def test_oracle_sphere_integrates_to_its_volume():
    """A sphere of radius 0.4 with edge 0.05 on 65^3 nodes over +-1: the sum of the coverage times the cell volume is 4/3 pi r^3 to 1 %."""
    b = ((-1.0, 1.0),) * 3
    seg = np.array([[[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.4, 0.4]]])
    out, mass = ref.voxelize((65,) * 3, b, None, seg, 1.0, 0.05)
    got = float(out.sum()) * (2.0 / 64) ** 3
    want = 4.0 / 3.0 * math.pi * 0.4 ** 3
    print(f"sphere integral {got:.5f} against {want:.5f}")
    assert abs(got - want) <= 0.01 * want
    assert out.max() == 1.0 and out.min() == 0.0 and (mass == 1.0).all()
    # the same sphere as an ellipsoid row: A = I / 0.4, w = edge / 0.4
    ell = np.concatenate([[0.0, 0.0, 0.0], (np.eye(3) / 0.4).reshape(9), [0.05 / 0.4, 1.0]])[None, None]
    as_ell = ref.voxelize((65,) * 3, b, ell, None, 0.0, 0.05)[0]
    assert np.abs(as_ell - out).max() <= 1e-12


def test_oracle_swapped_segment_gives_the_same_field():
    x = ref.node_positions((9, 17, 70), ref.BOUNDS)
    x = (x[0][:, None, None], x[1][None, :, None], x[2][None, None, :])
    hit = 0
    for row in ref.random_segments(1, 12, ref.BOUNDS, seed=3)[0]:
        swapped = np.concatenate([row[3:6], row[0:3], [row[7], row[6]]])
        a, b = ref.segment_cov(x, row, 0.07)[0], ref.segment_cov(x, swapped, 0.07)[0]
        hit += int(a.max() > 0)
        assert np.abs(a - b).max() <= 1e-15
    assert hit >= 6          # some of the random segments lie outside the grid


def test_oracle_flat_tables_give_exact_zeros():
    ell = ref.random_ellipsoids(2, 5, ref.BOUNDS, seed=4)
    ell[:, :, 13] = 0.0
    out, mass = ref.voxelize((5, 3, 4), ref.BOUNDS, ell, None, 0.0, 0.1)
    assert out.shape == (2, 5, 3, 4) and not out.any() and not mass.any()
    far = np.array([[[5.0, 5.0, 5.0, 6.0, 5.0, 5.0, 0.1, 0.0]]])
    out, mass = ref.voxelize((5, 3, 4), ref.BOUNDS, None, far, 3.0, 0.1)
    assert not out.any() and (mass == 3.0).all()


def test_oracle_coverage_is_zero_beyond_the_reach():
    """What the kernel's culling relies on: cov == 0 exactly wherever the computed distance d >= (max(ra, rb) + edge / 2) (1 + 2^-20)."""
    x = ref.node_positions((9, 17, 70), ref.BOUNDS)
    x = (x[0][:, None, None], x[1][None, :, None], x[2][None, None, :])
    edge = 0.07
    for row in ref.random_segments(1, 200, ref.BOUNDS, seed=5)[0]:
        cov, d = ref.segment_cov(x, row, edge)
        far = d >= (max(row[6], row[7]) + edge / 2) * (1 + 2.0 ** -20)
        assert far.any() and not cov[far].any()


# ----------------------------------------------------------------------------- the generator
HEART = dict(center=(0.01, 0.036, -0.005), heart_radius=0.045)


def test_fov_half_width(phantom):
    from nerfca_amd import synthetic
    assert abs(phantom.fov_half_width(synthetic.xcat_geometry(64)) - 0.18) <= 1e-15
    geo = dict(synthetic.xcat_geometry(16), nDetector=[12, 20], dDetector=[0.1, 0.1])
    assert abs(phantom.fov_half_width(geo) - 0.5 * 12 * 0.1 * 4.5 / 25.0) <= 1e-15          # the smaller axis


def test_thorax_lies_inside_its_cube(phantom):
    c, hw = np.array([0.02, -0.01, 0.03]), 0.18
    ell = phantom.thorax(c, hw)
    assert ell.dtype == np.float64 and ell.shape == (5, 14) and np.isfinite(ell).all()
    assert (ell[:, 12] > 0).all() and (ell[:, 13] < 0).sum() == 2          # two lungs
    for row in ell:
        A = row[3:12].reshape(3, 3)
        semi = 1.0 / np.diag(A)
        assert np.array_equal(A, np.diag(np.diag(A))) and (semi > 0).all()
        reach = np.abs(row[0:3] - c) + semi * (1 + row[12] / 2)          # cov == 0 beyond r = 1 + w / 2
        assert (reach <= hw).all(), reach / hw


def test_tree_is_deterministic_per_seed_and_seeds_differ(phantom):
    a = phantom.coronary_tree(3, seed=0, **HEART)
    b = phantom.coronary_tree(3, seed=0, **HEART)
    c = phantom.coronary_tree(3, seed=1, **HEART)
    assert a.dtype == np.float64 and a.ndim == 3 and a.shape[0] == 3 and a.shape[2] == 8 and 100 <= a.shape[1] <= 2000
    assert np.array_equal(a, b)
    assert a.shape != c.shape or not np.array_equal(a, c)
    assert not np.array_equal(a[0], a[1])          # the heart moves


def test_tree_phases_are_tree_at(phantom):
    P = 5
    tree = phantom.coronary_tree(P, seed=2, **HEART)
    for p in range(P):
        assert np.array_equal(tree[p], phantom.tree_at(p / P, seed=2, **HEART))
    assert np.abs(phantom.tree_at(1.0, seed=2, **HEART) - phantom.tree_at(0.0, seed=2, **HEART)).max() <= 1e-12
    # phase 0 is the uncontracted heart: the farthest any point gets from the centre
    r = [np.linalg.norm(tree[p, :, 0:3] - np.array(HEART["center"]), axis=1).max() for p in range(P)]
    assert r[0] == max(r)


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_tree_is_connected_tapered_and_inside_the_heart(phantom, seed):
    from nerfca_amd import synthetic
    hw = phantom.fov_half_width(synthetic.xcat_geometry(16))
    center = tuple(hw * c for c in phantom.HEART_CENTER)
    hr = hw * phantom.HEART_RADIUS
    for f in (0.0, 0.3, 0.5):
        seg, parent = phantom.tree_at(f, seed=seed, center=center, heart_radius=hr, return_parents=True)
        assert parent.shape == (seg.shape[0],) and (parent == -1).sum() == 2 and (parent < np.arange(seg.shape[0])).all()
        child = parent >= 0
        assert np.array_equal(seg[child, 0:3], seg[parent[child], 3:6])          # a child starts where its parent ends, bit for bit
        assert (seg[:, 7] <= seg[:, 6]).all() and (seg[:, 7] > 0).all()          # radii do not increase along a segment
        assert (seg[child, 6] <= seg[parent[child], 7]).all()                    # nor from a parent to its child
        for ends in (seg[:, 0:3], seg[:, 3:6]):
            assert (np.linalg.norm(ends - np.array(center), axis=1) <= phantom.HEART_EXTENT * hr * (1 + 1e-12)).all()
            assert (np.abs(ends) + seg[:, 6:7] < hw).all()


# ----------------------------------------------------------------------------- the Python layer
def test_voxelize_refuses_bad_tables_before_any_device_is_touched(capi, phantom):
    """Every call names the device cuda:0; the refusals come from the host tables, so they are raised on a machine without one."""
    ell = ref.random_ellipsoids(1, 2, ref.BOUNDS, seed=1)[0]
    seg = ref.random_segments(3, 4, ref.BOUNDS, seed=2)
    kw = dict(rho_vessel=1.0, device="cuda:0")

    def bad(word, **over):
        with pytest.raises(capi.NcaError, match=re.escape(word)):
            phantom.voxelize((5, 3, 4), ref.BOUNDS, **dict(kw, **over))

    for value in (math.nan, math.inf):
        t = seg.copy()
        t[1, 2, 4] = value
        bad("segments holds a value that is not finite", segments=t)
        t = ell.copy()
        t[1, 7] = value
        bad("ellipsoids holds a value that is not finite", ellipsoids=t)
    t = seg.copy()
    t[2, 0, 7] = -1e-9
    bad("negative radius", segments=t)
    for w in (0.0, -0.5):
        t = ell.copy()
        t[0, 12] = w
        bad("w <= 0", ellipsoids=t)
    bad("the ellipsoids have 2 phases, the segments 3", ellipsoids=np.stack([ell, ell]), segments=seg)
    bad("nothing to rasterise")
    bad("nothing to rasterise", segments=np.zeros((2, 0, 8)))
    bad("[P,rows,8]", segments=seg[:, :, :7])
    bad("[P,rows,14]", ellipsoids=np.zeros((14,)))
    bad("rho_vessel = nan", segments=seg, rho_vessel=math.nan)
    for e in (0.0, -1.0, math.inf, math.nan):
        bad(f"edge = {e}", segments=seg, edge=e)
    with pytest.raises(capi.NcaError):
        phantom.voxelize((5, 1, 4), ref.BOUNDS, segments=seg, **kw)          # drr.grid_desc's refusal
    bad("runs on the GPU", segments=seg, device="cpu")
    with pytest.raises(capi.NcaError):
        phantom.coronary_tree(0, **HEART)
    with pytest.raises(capi.NcaError):
        phantom.tree_at(0.0, center=(0.0, 0.0), heart_radius=1.0)
    with pytest.raises(capi.NcaError):
        phantom.tree_at(0.0, center=(0.0, 0.0, 0.0), heart_radius=1.0, tip_radius=0.2, root_radius=0.1)


def test_volume_errors_on_the_host(capi, phantom):
    """volume_errors is plain torch: checked here on CPU tensors."""
    import torch
    truth = torch.zeros(2, 3, 4)
    truth[0, 1, :] = 1.0
    pred = truth.clone()
    assert phantom.volume_errors(pred, truth, 0.5) == {"rmse": 0.0, "dice": 1.0}
    pred[0, 1, 0] = 0.0
    pred[1, 2, 3] = 1.0
    got = phantom.volume_errors(pred, truth, 0.5)
    assert abs(got["rmse"] - math.sqrt(2 / 24)) <= 1e-15 and abs(got["dice"] - 2 * 3 / 8) <= 1e-15
    assert phantom.volume_errors(pred, truth)["dice"] is None
    assert phantom.volume_errors(torch.zeros(2, 2), torch.zeros(2, 2), 0.5)["dice"] == 1.0
    with pytest.raises(capi.NcaError):
        phantom.volume_errors(torch.zeros(2, 2), torch.zeros(2, 3))
