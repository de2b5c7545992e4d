"""The distance transform (nca_vol_edt, metrics.distance_transform / mask_distances / centreline_coverage, phantom.centreline_points):
everything that can be checked without a launch -- the C-ABI surface, every refusal of the entry point (with device pointers that are
never read), the workspace query, the numpy oracle of the GPU tests (tests/edt_ref.py) written two ways and held to scipy, the centreline
sampling, the reductions on CPU tensors with the distance maps injected from the oracle, the refusals of the Python layer and the command
lines."""
import ctypes as C
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import scipy.ndimage
import torch

from conftest import ROOT

import edt_ref as ref
import nca_testlib as T
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_edt_workspace", "nca_vol_edt", "nca_edt_last_error")
MAX_AXIS = 512
refused = functools.partial(T.refused, "edt")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    assert header.index("nca_ssim_last_error(void)") < header.index("size_t nca_vol_edt_workspace(") < header.index("int nca_vol_edt(") < header.index("nca_edt_last_error(void)")
    assert int(re.search(r"NCA_EDT_MAX_AXIS = (\d+)", header).group(1)) == MAX_AXIS >= 512
    assert callable(capi.check_edt)
    import nerfca_amd
    assert nerfca_amd.metrics.distance_transform and nerfca_amd.metrics.MAX_AXIS == MAX_AXIS
    assert nerfca_amd.metrics.mask_distances and nerfca_amd.metrics.centreline_coverage and nerfca_amd.phantom.centreline_points


grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def test_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, threshold=0.5, invert=0, out=FAKE, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_edt(g, vol, n_vol, threshold, invert, out, work, work_bytes, None)

    who = "nca_vol_edt:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    for bad in (2, -1):
        refused(capi, lib, call(invert=bad), f"invert = {bad}")
    refused(capi, lib, call(threshold=math.nan), "threshold = nan")
    assert call(threshold=math.inf, work=None) == E_WORKSPACE          # an infinite threshold is a threshold: the call gets as far as the workspace
    T.grid_refusals("edt", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    big = (1 << 31) - 1
    refused(capi, lib, call(n=(big, big, big), n_vol=big), "overflow", str(big))
    # an axis beyond what a line tile in LDS holds
    for a in range(3):
        n = [4, 5, 6]
        n[a] = MAX_AXIS + 1
        refused(capi, lib, call(n=n), f"n[{a}] = {MAX_AXIS + 1}", "NCA_EDT_MAX_AXIS", code=E_UNSUPPORTED)
    n = [MAX_AXIS, MAX_AXIS, MAX_AXIS]
    assert call(n=n, work=None) == E_WORKSPACE          # the longest axis itself is accepted
    # 257 volumes of 512^3 are 257 * 2^18 rows, four to a workgroup: more than the 2^24 workgroups of one launch
    refused(capi, lib, call(n=n, n_vol=257), "tiles", "one launch", str(257 << 16))
    assert call(n=n, n_vol=256, work=None) == E_WORKSPACE
    g = grid(capi)
    need = lib.nca_vol_edt_workspace(C.byref(g), 2)
    assert need == 3072          # 2 * 120 nodes * 12 bytes = 2880, rounded up to 256
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_workspace_query(capi, lib):
    def q(n, n_vol, **kw):
        return lib.nca_vol_edt_workspace(C.byref(grid(capi, n=n, **kw)), n_vol)

    assert q((2, 2, 2), 1) == 256 and q((4, 4, 4), 1) == 768 and q((4, 4, 4), 3) == 2304 and q((3, 5, 65), 2) == (2 * 975 * 12 + 255) // 256 * 256
    assert lib.nca_vol_edt_workspace(None, 1) == 0
    for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, MAX_AXIS + 1), 1)):
        assert q(*bad) == 0, bad
    assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0
    base = [3, 4, 5, 2]
    for axis in range(4):
        last = 0
        for step in range(0, 40, 3):
            args = list(base)
            args[axis] += step
            got = q(tuple(args[:3]), args[3])
            assert got >= last and got > 0 and got % 256 == 0 and got >= 12 * args[0] * args[1] * args[2] * args[3], args
            last = got
    assert q((MAX_AXIS,) * 3, 256) == 12 * 256 * MAX_AXIS ** 3          # beyond 2^32: a size_t


# ----------------------------------------------------------------------------- the oracle
ORACLE_SHAPES = ref.SHAPES + ((9, 7, 130),)


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_brute_force_equals_the_separable_oracle_bit_for_bit(shape):
    for pattern in ref.PATTERNS:
        for inv in (ref.UNIT, ref.ANISO):
            for invert in ((0, 1) if pattern == "d0.05" else (0,)):
                feat = ref.features(ref.volume(shape, pattern), ref.THRESHOLD, invert)
                a, b = ref.brute(feat, inv), ref.separable(feat, inv)
                assert np.array_equal(a, b), (shape, pattern, inv, invert)
                assert (b[feat] == 0).all() and (np.isinf(b).all() if not feat.any() else np.isfinite(b).all())


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_against_scipy(shape):
    """Unit spacing: every q is a whole number below 2^53, exact in both, and sqrt and the rounding to f32 are correctly rounded: equal bits.
    Anisotropic: scipy forms sum_a (d_a h_a)^2, the oracle sum_a (h_a h_a) d_a^2 -- a few 2^-53 relative apart in f64 (printed below: 5.84 at
    worst in the squares, half of that in the roots), which moves a rounding to f32 by at most one step."""
    worst = 0.0
    for pattern in ref.PATTERNS:
        vol = ref.volume(shape, pattern)
        for invert in (0, 1):
            feat = ref.features(vol, ref.THRESHOLD, invert)
            if not feat.any():
                continue          # scipy has no answer for a mask without a feature; the oracle's +inf is held by the test above
            for inv in (ref.UNIT, ref.ANISO):
                q = ref.separable(feat, inv)
                got = np.sqrt(q).astype(np.float32)
                assert np.array_equal(got, ref.edt(vol, inv, ref.THRESHOLD, invert))
                sci = scipy.ndimage.distance_transform_edt(~feat, sampling=ref.spacing(inv))
                steps = int(T.ulp_distance(got, sci.astype(np.float32)).max())
                assert steps <= (0 if inv == ref.UNIT else 1), (shape, pattern, invert, inv, steps)
                if q.max() > 0:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        worst = max(worst, float(np.nan_to_num(np.abs(sci * sci - q) / (q * 2.0 ** -53)).max()))
    print(f"{shape}: q within {worst:.2f} of 2^-53 relative of scipy's squared distance")


def test_threshold_and_nan_rules():
    vol = np.array([0.25, 0.5, np.nan, 0.75], dtype=np.float32)
    assert ref.features(vol, 0.5, 0).tolist() == [False, False, False, True]          # equal to the threshold: not a feature; NaN: not a feature
    assert ref.features(vol, 0.5, 1).tolist() == [True, True, True, False]            # ... and both are under invert


# ----------------------------------------------------------------------------- centrelines
def test_centreline_points():
    from nerfca_amd import phantom
    seg = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.1, 0.1],          # length 1, step 0.3: m = 4
                    [1.0, 0.0, 0.0, 1.0, 0.6, 0.0, 0.1, 0.05],         # length 0.6: m = 2 exactly
                    [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 0.1, 0.1],          # a point: m = 1, both endpoints
                    [0.0, 0.0, 0.0, 0.1, 0.1, 0.1, 0.1, 0.1]])         # shorter than the step: m = 1
    (pts,) = phantom.centreline_points(seg, 0.3)
    want = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.75, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0.3, 0], [1, 0.6, 0], [2, 2, 2], [2, 2, 2], [0, 0, 0],
                     [0.1, 0.1, 0.1]])
    assert pts.dtype == np.float64 and pts.shape == want.shape and np.array_equal(pts, want)
    two = phantom.centreline_points(np.stack([seg, seg + 1.0]), 0.3)
    assert len(two) == 2 and np.array_equal(two[0], pts) and np.array_equal(two[1][:5], want[:5] + 1.0)
    assert np.array_equal(phantom.centreline_points(seg, 0.3)[0], pts)          # deterministic
    gaps = np.linalg.norm(np.diff(phantom.centreline_points(seg[:1], 0.07)[0], axis=0), axis=1)
    assert len(gaps) == 15 and gaps.max() <= 0.07
    from nerfca_amd import _capi
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(_capi.NcaError):
            phantom.centreline_points(seg, bad)
    with pytest.raises(_capi.NcaError):
        phantom.centreline_points(np.zeros((3, 7)), 0.1)


# ----------------------------------------------------------------------------- the reductions, on CPU tensors
BOUNDS = ((0.0, 0.37 * 8), (0.0, 0.11 * 9), (0.0, 0.29 * 10))          # 9 x 10 x 11 nodes: the spacings 0.37, 0.11, 0.29


def _stack():
    rng = np.random.default_rng(5)
    shape = (9, 10, 11)
    truth = np.stack([ref.volume(shape, "d0.05"), ref.volume(shape, "none"), ref.volume(shape, "d0.5"), ref.volume(shape, "d0.05")])
    truth[0, -1] = 0.1          # nothing of the mask in the last plane: the roll below wraps nothing around
    pred = np.stack([np.roll(truth[0], 1, axis=0), ref.volume(shape, "d0.05"), ref.volume(shape, "none"), truth[3]]) * 0.5          # thresholded at 0.25
    inv = tuple((n - 1) / (b[1] - b[0]) for n, b in zip(shape, BOUNDS))
    return pred.astype(np.float32), truth.astype(np.float32), inv, rng


def test_mask_distance_reductions_on_injected_maps():
    from nerfca_amd import metrics
    pred, truth, inv, _ = _stack()
    a, b = pred > 0.25, truth > 0.5
    to_a, to_b = ref.edt(pred, inv, 0.25), ref.edt(truth, inv, 0.5)
    got = metrics.mask_distance_reductions(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b), 95.0)
    assert set(got) == {"n_pred", "n_truth", "pred_to_truth", "truth_to_pred", "assd", "hausdorff", "hd_percentile"}
    for k, v in got.items():
        assert v.shape == (4,) and v.dtype == (torch.int64 if k.startswith("n_") else torch.float64), k
    for p in range(4):
        na, sa, ma, qa = ref.directed(to_b[p], a[p], 95.0)
        nb, sb, mb, qb = ref.directed(to_a[p], b[p], 95.0)
        assert int(got["n_pred"][p]) == na and int(got["n_truth"][p]) == nb
        if na == 0 or nb == 0:
            assert all(math.isnan(float(got[k][p])) for k in got if not k.startswith("n_")), p
            continue
        tol = (na + nb) * 2.0 ** -53 * (sa + sb)          # the order of an f64 sum
        assert abs(float(got["pred_to_truth"][p]) - sa / na) <= tol and abs(float(got["truth_to_pred"][p]) - sb / nb) <= tol
        assert abs(float(got["assd"][p]) - (sa + sb) / (na + nb)) <= tol
        assert float(got["hausdorff"][p]) == max(ma, mb) and float(got["hd_percentile"][p]) == max(qa, qb)
        assert float(got["hd_percentile"][p]) <= float(got["hausdorff"][p])
    assert (1, 2) == tuple(p for p in range(4) if math.isnan(float(got["assd"][p])))          # an empty truth, an empty prediction
    for k in ("pred_to_truth", "truth_to_pred", "assd", "hausdorff", "hd_percentile"):
        assert float(got[k][3]) == 0.0, k          # identical masks: exactly 0
    h0 = float(np.float32(0.37)) * (1 + 2.0 ** -23)          # the maps are f32: h_0 rounded once
    assert 0 < float(got["assd"][0]) <= h0 and 0 < float(got["hausdorff"][0]) <= h0          # rolled by one node along axis 0
    q50 = metrics.mask_distance_reductions(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b), 50.0)
    assert float(q50["hd_percentile"][0]) == max(ref.directed(to_b[0], a[0], 50.0)[3], ref.directed(to_a[0], b[0], 50.0)[3])
    from nerfca_amd import _capi
    with pytest.raises(_capi.NcaError, match="percentile"):
        metrics.mask_distance_reductions(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b), 101.0)
    with pytest.raises(_capi.NcaError, match="shape"):
        metrics.mask_distance_reductions(torch.from_numpy(a[:2]), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b))


def test_coverage_reductions_on_injected_maps():
    from nerfca_amd import metrics
    _, truth, inv, rng = _stack()
    dist = ref.edt(truth, inv, 0.5)
    h = np.array(ref.spacing(inv))
    n = np.array(truth.shape[1:])
    points = []
    for p in range(4):
        pts = rng.random((40, 3)) * (h * (n - 1))
        pts[:3] = [[-0.2, 0.1, 0.1], [0.1, 0.1, h[2] * (n[2] - 1) + 0.51 * h[2]], [0.1, -0.51 * h[1], 0.1]]          # three outside
        pts[3] = [0.0 - 0.49 * h[0], 0.0, h[2] * (n[2] - 1) + 0.49 * h[2]]                                          # just inside: rounds to a border node
        points.append(pts)
    tol = 0.3
    got = metrics.coverage_reductions(torch.from_numpy(dist), BOUNDS, points, tol)
    assert set(got) == {"coverage", "mean_distance", "n_points", "n_outside"}
    for p in range(4):
        idx = np.floor(points[p] * np.array(inv) + 0.5).astype(np.int64)
        inside = ((idx >= 0) & (idx <= n - 1)).all(axis=1)
        assert int(got["n_outside"][p]) == int((~inside).sum()) == 3 and int(got["n_points"][p]) == 37
        d = dist[p][tuple(idx[inside].T)].astype(np.float64)
        assert float(got["coverage"][p]) == pytest.approx(float((d <= tol).mean()), abs=1e-15)
        if np.isinf(d).any():
            assert math.isinf(float(got["mean_distance"][p])) and float(got["coverage"][p]) == 0.0 and p == 1
        else:
            assert float(got["mean_distance"][p]) == pytest.approx(float(d.mean()), rel=1e-14)
    one = metrics.coverage_reductions(torch.from_numpy(dist), BOUNDS, points[0], tol)          # one set serves every phase
    assert float(one["coverage"][0]) == float(got["coverage"][0]) and one["coverage"].shape == (4,)
    # the nodes of the mask themselves are covered at tolerance 0
    nodes = np.argwhere(truth[0] > 0.5) * h
    exact = metrics.coverage_reductions(torch.from_numpy(dist[0]), BOUNDS, [nodes], 0.0)
    assert float(exact["coverage"][0]) == 1.0 and float(exact["mean_distance"][0]) == 0.0 and int(exact["n_outside"][0]) == 0
    none = metrics.coverage_reductions(torch.from_numpy(dist[:1]), BOUNDS, [np.array([[-5.0, 0, 0]])], tol)
    assert math.isnan(float(none["coverage"][0])) and int(none["n_points"][0]) == 0 and int(none["n_outside"][0]) == 1
    from nerfca_amd import _capi
    with pytest.raises(_capi.NcaError):
        metrics.coverage_reductions(torch.from_numpy(dist), BOUNDS, points[:3], tol)
    with pytest.raises(_capi.NcaError, match="tol"):
        metrics.coverage_reductions(torch.from_numpy(dist), BOUNDS, points, -1.0)


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import metrics
    a = torch.zeros(2, 4, 4, 4)
    bounds = ((-1.0, 1.0),) * 3
    with pytest.raises(capi.NcaError):
        metrics.distance_transform(a, bounds, threshold=0.5)
    with pytest.raises(capi.NcaError):
        metrics.mask_distances(a, a, bounds, threshold=0.5)
    with pytest.raises(capi.NcaError):
        metrics.centreline_coverage(a, bounds, [np.zeros((1, 3))] * 2, threshold=0.5, tol=0.1)
    with pytest.raises(capi.NcaError):
        metrics.distance_transform(a.numpy(), bounds, threshold=0.5)


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines_parse():
    cv = _tool("compare_volumes")
    args = cv.parser().parse_args(cv.join_args(["a", "b", "--bounds", "-0.18,0.18,0,2,0,3", "--threshold", "3", "--out", "x.json"]))
    assert args.pred == "a" and args.truth == "b" and args.threshold == 3.0 and args.out == "x.json" and args.pred_threshold is None
    assert args.bounds == ((-0.18, 0.18), (0.0, 2.0), (0.0, 3.0)) and args.pred_fraction is None and args.percentile == 95.0
    eb = _tool("edt_bench")
    args = eb.parser().parse_args(["--out", "profiles/edt_bench.txt"])
    assert args.out == "profiles/edt_bench.txt" and args.passes == 3
    ps = _tool("phantom_study")
    assert ps.parser().parse_args([]).distances is False and ps.parser().parse_args(["--distances"]).distances is True
