"""The filters of the CCTA pipeline (nca_vol_smooth, nca_vol_cityblock, nerfca_amd.ccta, surface=True of metrics.mask_distances): everything
that can be checked without a launch -- the C-ABI surface, every refusal of both entry points (with device pointers that are never read),
the workspace queries, the numpy oracle of the GPU tests (tests/filt_ref.py) held to scipy.ndimage bit for bit, gaussian_weights, the
surface reductions on CPU tensors with the borders and distance maps injected from the oracle, the refusals of the Python layer and the
command lines."""
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

import edt_ref
import filt_ref as ref
import nca_testlib as T
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_smooth_workspace", "nca_vol_smooth", "nca_vol_cityblock_workspace", "nca_vol_cityblock", "nca_filt_last_error")
MAX_AXIS, MAX_RADIUS = 512, 32
refused = functools.partial(T.refused, "filt")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_edt_last_error(void)", "size_t nca_vol_smooth_workspace(", "int nca_vol_smooth(", "size_t nca_vol_cityblock_workspace(", "int nca_vol_cityblock(",
             "nca_filt_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert int(re.search(r"NCA_SMOOTH_MAX_RADIUS = (\d+)", header).group(1)) == MAX_RADIUS
    assert callable(capi.check_filt)
    import nerfca_amd
    from nerfca_amd import ccta
    assert nerfca_amd.ccta is ccta and "ccta" in nerfca_amd.__all__ and ccta.MAX_RADIUS == MAX_RADIUS and ccta.MAX_AXIS == MAX_AXIS
    for name in ("gaussian_weights", "gaussian_filter", "cityblock_distance", "binary_dilation", "binary_erosion", "mask_border", "hounsfield_to_attenuation",
                 "vessel_contrast", "prepare_ccta"):
        assert callable(getattr(ccta, name)), name


grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def c_radius(r):
    return (C.c_int32 * 3)(*r)


def c_weights(w):
    return (C.c_double * len(w))(*w)


# ----------------------------------------------------------------------------- refusals
def test_smooth_refusals(capi, lib):
    ok_r, ok_w = c_radius((1, 0, 2)), c_weights([0.5, 0.25, 1.0, 0.4, 0.2, 0.1])

    def call(g="default", vol=FAKE, n_vol=2, radius=ok_r, weights=ok_w, out=FAKE + 64, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_smooth(g, vol, n_vol, radius, weights, out, work, work_bytes, None)

    who = "nca_vol_smooth:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    refused(capi, lib, call(radius=None), who, "radius is NULL")
    refused(capi, lib, call(weights=None), who, "weights is NULL")
    refused(capi, lib, call(out=FAKE), who, "out is vol")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("filt", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for a in range(3):
        r = [1, 0, 2]
        r[a] = -1
        refused(capi, lib, call(radius=c_radius(r), weights=c_weights([0.1] * 8)), f"radius[{a}] = -1", "negative")
        r[a] = MAX_RADIUS + 1
        refused(capi, lib, call(radius=c_radius(r), weights=c_weights([0.1] * 40)), f"radius[{a}] = {MAX_RADIUS + 1}", "NCA_SMOOTH_MAX_RADIUS", code=E_UNSUPPORTED)
    assert call(radius=c_radius((MAX_RADIUS,) * 3), weights=c_weights([0.01] * (3 * MAX_RADIUS + 3)), work=None) == E_WORKSPACE          # the largest radius is accepted
    # weights: [axis 0: k = 0, 1] [axis 1: k = 0] [axis 2: k = 0, 1, 2]
    for at, (axis, k) in enumerate(((0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (2, 2))):
        for bad, word, why in ((math.nan, "nan", "finite"), (math.inf, "inf", "finite"), (-0.25, "-0.25", "negative")):
            w = [0.5, 0.25, 1.0, 0.4, 0.2, 0.1]
            w[at] = bad
            refused(capi, lib, call(weights=c_weights(w)), f"weight {k} of axis {axis} = {word}", why)
    assert call(weights=c_weights([0.0] * 6), work=None) == E_WORKSPACE          # zero is a weight
    # no limit on an axis: 2^20 nodes along each in turn get as far as the workspace
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE
    # 2^24 + 1 volumes of 2 x 2 x 2: the axis 0 and axis 1 launches take one workgroup per volume and per plane
    refused(capi, lib, call(n=(2, 2, 2), n_vol=(1 << 24) + 1), "tiles", "one launch", str(((1 << 24) + 1) * 2))
    g = grid(capi)
    need = lib.nca_vol_smooth_workspace(C.byref(g), 2)
    assert need == 3840          # 2 * 120 nodes * 16 bytes
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_cityblock_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, threshold=0.5, invert=0, border=0, out=FAKE, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_cityblock(g, vol, n_vol, threshold, invert, border, out, work, work_bytes, None)

    who = "nca_vol_cityblock:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    for bad in (2, -1):
        refused(capi, lib, call(invert=bad), f"invert = {bad}")
        refused(capi, lib, call(border=bad), f"border = {bad}")
    refused(capi, lib, call(threshold=math.nan), "threshold = nan")
    assert call(threshold=-math.inf, invert=1, border=1, work=None) == E_WORKSPACE
    T.grid_refusals("filt", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for a in range(3):
        n = [4, 5, 6]
        n[a] = MAX_AXIS + 1
        refused(capi, lib, call(n=n), f"n[{a}] = {MAX_AXIS + 1}", "NCA_EDT_MAX_AXIS", code=E_UNSUPPORTED)
    n = [MAX_AXIS, MAX_AXIS, MAX_AXIS]
    assert call(n=n, work=None) == E_WORKSPACE
    refused(capi, lib, call(n=n, n_vol=257), "tiles", "one launch", str(257 << 16))          # as nca_vol_edt: four rows to a workgroup
    assert call(n=n, n_vol=256, work=None) == E_WORKSPACE
    g = grid(capi)
    need = lib.nca_vol_cityblock_workspace(C.byref(g), 2)
    assert need == 2048          # 2 * 120 nodes * 8 bytes = 1920, rounded up to 256
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_workspace_queries(capi, lib):
    for name, per_node in (("nca_vol_smooth_workspace", 16), ("nca_vol_cityblock_workspace", 8)):
        fn = getattr(lib, name)

        def q(n, n_vol, **kw):
            return fn(C.byref(grid(capi, n=n, **kw)), n_vol)

        assert q((2, 2, 2), 1) == 256 and q((4, 4, 4), 1) == 64 * per_node and q((4, 4, 4), 3) == 192 * per_node
        assert q((3, 5, 65), 2) == (2 * 975 * per_node + 255) // 256 * 256
        assert fn(None, 1) == 0
        for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1)):
            assert q(*bad) == 0, bad
        assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0
        assert q((MAX_AXIS,) * 3, 256) == per_node * 256 * MAX_AXIS ** 3          # beyond 2^32: a size_t
        for n_vol in (1, 2, 7):
            for n in ((3, 4, 5), (9, 4, 130), (33, 17, 65)):
                assert q(n, n_vol) == (n_vol * n[0] * n[1] * n[2] * per_node + 255) // 256 * 256
    assert lib.nca_vol_cityblock_workspace(C.byref(grid(capi, n=(4, 4, MAX_AXIS + 1))), 1) == 0
    assert lib.nca_vol_smooth_workspace(C.byref(grid(capi, n=(4, 4, MAX_AXIS + 1))), 1) == 16 * 16 * (MAX_AXIS + 1)


# ----------------------------------------------------------------------------- the oracle against scipy
@pytest.mark.parametrize("shape,sigma,radius", ref.SMOOTH_CASES, ids=lambda v: str(v))
def test_smoothing_oracle_equals_scipy_bit_for_bit(shape, sigma, radius):
    x = ref.smooth_volume(shape)
    sci = scipy.ndimage.gaussian_filter(x.astype(np.float64), sigma, radius=radius, mode="reflect")
    ws = [ref.half_weights(float(s), int(r)) for s, r in zip(ref.per_axis(sigma), ref.per_axis(radius))]
    mine = x.astype(np.float64)
    for a in range(3):
        mine = ref.smooth_axis(mine, a, ws[a])
    assert np.array_equal(mine.view(np.int64), sci.view(np.int64))          # in f64, before the rounding
    got = ref.smooth(x, sigma, radius)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), sci.astype(np.float32).view(np.int32))
    stack = np.stack([x, ref.smooth_volume(shape, seed=1)])
    assert np.array_equal(ref.smooth(stack, sigma, radius)[0].view(np.int32), got.view(np.int32))          # the leading axis is not filtered


def test_reflect_is_scipys():
    for n in (2, 3, 7):
        j = np.arange(-3 * n, 4 * n)
        want = np.pad(np.arange(n), (3 * n, 3 * n), mode="symmetric")
        assert np.array_equal(ref.reflect(j, n), want)


@pytest.mark.parametrize("shape", ref.CITY_SHAPES, ids=str)
def test_cityblock_oracle_equals_scipy(shape):
    for fill in ref.FILLS:
        vol = ref.mask_volume(shape, fill)
        M = vol > 0.5
        d = ref.cityblock(vol, 0.5)
        assert d.dtype == np.int32
        if M.any():          # scipy has no answer for a mask without a feature; the oracle's sentinel is held by the brute-force test
            assert np.array_equal(d, scipy.ndimage.distance_transform_cdt(~M, metric="taxicab"))
        else:
            assert (d == ref.NONE).all() and shape == (3, 3, 3) and fill == 0.02
        for n in (1, 2, 3, 5):
            assert np.array_equal(ref.dilate(M, n), scipy.ndimage.binary_dilation(M, iterations=n)), (fill, n)
            assert np.array_equal(ref.erode(M, n), scipy.ndimage.binary_erosion(M, iterations=n)), (fill, n)
            assert np.array_equal(ref.cityblock(vol, 0.5, 1, 1) > n, scipy.ndimage.binary_erosion(M, iterations=n))
        assert np.array_equal(ref.border_of(M), M ^ scipy.ndimage.binary_erosion(M))
        assert np.array_equal(ref.erode(ref.dilate(M, 3), 1), scipy.ndimage.binary_erosion(scipy.ndimage.binary_dilation(M, iterations=3), iterations=1))


@pytest.mark.parametrize("shape", [(4, 5, 6), (3, 3, 3), (2, 2, 2), (6, 8, 10)], ids=str)
def test_cityblock_brute_force_equals_the_separable_form(shape):
    for fill in ref.FILLS + (0.0, 1.0):
        vol = ref.mask_volume(shape, fill)
        for invert in (0, 1):
            feat = ref.features(vol, 0.5, invert)
            for border in (0, 1):
                a, b = ref.cityblock_brute(feat, border), ref.cityblock_separable(feat, border)
                assert np.array_equal(a, b), (fill, invert, border)
                assert (b[feat] == 0).all()
                if not feat.any():
                    assert (b == ref.NONE).all() if not border else np.array_equal(b, ref.border_term(shape))


def test_threshold_and_nan_rules():
    vol = np.array([0.25, 0.5, np.nan, 0.75], dtype=np.float32)
    assert ref.features(vol, 0.5, 0).tolist() == [False, False, False, True]
    assert ref.features(vol, 0.5, 1).tolist() == [True, True, True, False]


def test_gaussian_weights_are_scipys():
    from scipy.ndimage._filters import _gaussian_kernel1d
    from nerfca_amd import ccta
    for sigma, radius in ((1.0, 2), (1.5, 6), (0.7, 3), (2.0, 8), (2.5, 10), (8.0, 32), (4.0, 16), (1.0, 0)):
        k = _gaussian_kernel1d(sigma, 0, radius)
        w = ccta.gaussian_weights(sigma, radius)
        assert w.dtype == np.float64 and w.shape == (radius + 1,)
        assert np.array_equal(w, k[radius:]) and np.array_equal(w, k[:radius + 1][::-1]) and np.array_equal(w, ref.half_weights(sigma, radius))
    for sigma, truncate in ((1.0, 4.0), (2.5, 4.0), (1.3, 3.0), (0.2, 4.0)):
        r = int(truncate * sigma + 0.5)
        assert np.array_equal(ccta.gaussian_weights(sigma, truncate=truncate), _gaussian_kernel1d(sigma, 0, r)[r:])
    assert ccta.gaussian_weights(0.0).tolist() == [1.0] and ccta.gaussian_weights(1e-16, 5).tolist() == [1.0]
    for bad in (dict(sigma=-1.0), dict(sigma=math.nan), dict(sigma=math.inf), dict(sigma=1.0, radius=-1), dict(sigma=1.0, radius=1.5), dict(sigma=1.0, radius=33),
                dict(sigma=9.0), dict(sigma=1.0, truncate=-1.0)):
        with pytest.raises(ccta._capi.NcaError):
            ccta.gaussian_weights(**bad)


def test_interp_is_numpys():
    from nerfca_amd import ccta
    xp, fp = list(ref.XP), [v * 0.05 for v in ref.FP]
    x = np.concatenate([np.linspace(-1, 7, 321), np.array(xp, dtype=np.float64), np.nextafter(np.array(xp, dtype=np.float64), 9)])
    got = ccta._interp(torch.from_numpy(x), xp, fp).numpy()
    assert np.abs(got - np.interp(x, xp, fp)).max() <= 2.0 ** -53 * 0.05 * 4          # a few roundings of values up to 0.05
    assert got[0] == 0.0 and got[-1] == 0.05


def test_hounsfield_to_attenuation():
    from nerfca_amd import ccta
    hu = torch.tensor([-1000.0, 0.0, 40.0, 1000.0])
    got = ccta.hounsfield_to_attenuation(hu)
    want = (hu.double().numpy() / 1000 * (0.1494 * 2.5e-2 - 0.0430 * 2.5e-2) + 0.1494 * 2.5e-2).astype(np.float32)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert abs(float(got[0]) - 0.0430 * 2.5e-2) < 1e-9 and float(got[1]) == float(np.float32(0.1494 * 2.5e-2))


# ----------------------------------------------------------------------------- surface distances, on CPU tensors
def test_surface_reductions_on_injected_borders():
    """metrics.mask_distance_reductions with the borders and maps surface=True hands it, from the oracle, against MedPy's formula in scipy."""
    from nerfca_amd import metrics
    pred, truth = ref.blobs()
    h = (0.5, 0.4, 0.3)
    inv = tuple(1.0 / v for v in h)
    a, b = ref.border_of(pred > 0.5), ref.border_of(truth > 0.5)
    want = ref.surface_distances_ref(pred > 0.5, truth > 0.5, h)
    assert np.array_equal(a, want["border_pred"]) and np.array_equal(b, want["border_truth"])
    assert 0 < a.sum() < (pred > 0.5).sum() and 0 < b.sum() < (truth > 0.5).sum()
    to_a, to_b = edt_ref.edt(a.astype(np.float32), inv, 0.5), edt_ref.edt(b.astype(np.float32), inv, 0.5)
    got = metrics.mask_distance_reductions(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b), 95.0)
    assert int(got["n_pred"]) == want["n_pred"] and int(got["n_truth"]) == want["n_truth"]
    for k in ("pred_to_truth", "truth_to_pred", "assd", "hausdorff", "hd_percentile"):
        assert abs(float(got[k]) - want[k]) <= 2.0 ** -23 * want[k], k          # the maps are f32, one step at non-unit spacing
    whole = metrics.mask_distance_reductions(torch.from_numpy(pred > 0.5), torch.from_numpy(truth > 0.5),
                                             torch.from_numpy(edt_ref.edt(pred, inv, 0.5)), torch.from_numpy(edt_ref.edt(truth, inv, 0.5)), 95.0)
    assert float(whole["assd"]) < float(got["assd"])          # whole bodies overlap at distance 0: the surfaces do not


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import ccta, metrics
    a = torch.zeros(2, 4, 4, 4)
    bounds = ((0.0, 3.0),) * 3
    for call in (lambda: ccta.gaussian_filter(a, 1.0), lambda: ccta.cityblock_distance(a, threshold=0.5), lambda: ccta.binary_dilation(a),
                 lambda: ccta.binary_erosion(a > 0), lambda: ccta.mask_border(a, threshold=0.5), lambda: ccta.vessel_contrast(a, bounds),
                 lambda: ccta.prepare_ccta(a, a, bounds), lambda: metrics.mask_distances(a, a, bounds, threshold=0.5, surface=True),
                 lambda: ccta.gaussian_filter(a.numpy(), 1.0), lambda: ccta.cityblock_distance(None, threshold=0.5)):
        with pytest.raises(capi.NcaError):
            call()
    import inspect
    assert inspect.signature(metrics.mask_distances).parameters["surface"].default is False


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(capsys):
    pc = _tool("prepare_ccta")
    args = pc.parser().parse_args(pc.join_args(["--raw", "raw.npy", "--mask", "mask.npy", "--bounds", "-0.18,0.18,0,2,0,3", "--out", "d/"]))
    assert args.raw == "raw.npy" and args.mask == "mask.npy" and args.labels is None and args.bounds == ((-0.18, 0.18), (0.0, 2.0), (0.0, 3.0)) and args.out == "d/"
    assert args.grow == 3 and args.shrink == 1 and args.sigma == 1.0 and args.radius == 2 and args.contrast == 0.05
    args = pc.parser().parse_args(pc.join_args(["--raw", "r", "--mask", "m", "--labels", "t.npy", "--aorta", "52", "--heart", "51", "--bounds", "0,1,0,1,0,1", "--out", "d"]))
    assert args.labels == "t.npy" and args.aorta == 52 and args.heart == 51
    fb = _tool("filt_bench")
    args = fb.parser().parse_args(["--out", "profiles/filt_bench.txt"])
    assert args.out == "profiles/filt_bench.txt" and args.passes == 3 and args.sides == "128,256" and args.volumes == "1,10"
    cv = _tool("compare_volumes")
    base = ["a", "b", "--bounds", "0,1,0,1,0,1", "--threshold", "3"]
    assert cv.parser().parse_args(cv.join_args(base)).surface is False and cv.parser().parse_args(cv.join_args(base + ["--surface"])).surface is True
    for tool, argv in ((pc, ["--help"]), (fb, ["--help"]), (pc, ["--raw", "r"]), (pc, pc.join_args(["--raw", "r", "--mask", "m", "--out", "d", "--bounds", "0,1,0,1"])),
                       (fb, ["--passes", "many"]), (fb, ["--nonsense"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    # labels without both label values: refused before anything is loaded
    with pytest.raises(SystemExit) as e:
        pc.main(["--raw", "r", "--mask", "m", "--labels", "t", "--bounds", "0,1,0,1,0,1", "--out", "d"])
    assert "--aorta" in str(e.value.code)
