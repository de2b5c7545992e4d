"""The soft skeleton and clDice (nca_vol_softskel, nca_vol_overlap_sums, metrics.soft_skeleton / cldice): everything that can be checked
without a launch -- the C-ABI surface, every refusal of both entry points (with device pointers that are never read), the workspace
queries, the numpy oracle of the GPU tests (tests/skel_ref.py) held to the published torch expression as values, the analytic properties
of the skeleton, the clDice reductions on CPU tensors with the skeletons injected from the oracle, the refusals of the Python layer and the
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

import nca_testlib as T
import skel_ref as ref
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_softskel_workspace", "nca_vol_softskel", "nca_vol_overlap_sums_workspace", "nca_vol_overlap_sums", "nca_skel_last_error")
MAX_ITER = 512
refused = functools.partial(T.refused, "skel")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_resample_last_error(void)", "size_t nca_vol_softskel_workspace(", "int nca_vol_softskel(", "size_t nca_vol_overlap_sums_workspace(",
             "int nca_vol_overlap_sums(", "nca_skel_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert int(re.search(r"NCA_SKEL_MAX_ITER = (\d+)", header).group(1)) == MAX_ITER
    assert callable(capi.check_skel)
    from nerfca_amd import metrics
    assert metrics.MAX_SKEL_ITER == MAX_ITER
    for name in ("soft_skeleton", "cldice", "cldice_reductions"):
        assert callable(getattr(metrics, name)), name


# ----------------------------------------------------------------------------- refusals
def test_softskel_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, iterations=3, out=FAKE + 64, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_softskel(g, vol, n_vol, iterations, out, work, work_bytes, None)

    who = "nca_vol_softskel:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    refused(capi, lib, call(out=FAKE), who, "out is vol")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("skel", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for bad in (-1, -7):
        refused(capi, lib, call(iterations=bad), f"iterations = {bad}", "negative")
    refused(capi, lib, call(iterations=MAX_ITER + 1), f"iterations = {MAX_ITER + 1}", "NCA_SKEL_MAX_ITER", code=E_UNSUPPORTED)
    for ok in (0, MAX_ITER):          # both ends are accepted: they get as far as the workspace
        assert call(iterations=ok, work=None) == E_WORKSPACE
    # no limit on an axis: 2^20 nodes along each in turn get as far as the workspace
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE
    # one tile per volume of 2 x 2 x 2: 2^31 - 1 of them are one launch, 2^31 are not... an int32 count cannot say 2^31, so 4 x 8 x 65 (two tiles)
    assert call(n=(2, 2, 2), n_vol=(1 << 31) - 1, work=None) == E_WORKSPACE
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30), "tiles", "one launch", str(1 << 31))
    g = grid(capi)
    need = lib.nca_vol_softskel_workspace(C.byref(g), 2)
    assert need == 2048          # 2 * 120 nodes * 8 bytes = 1920, rounded up to 256
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_overlap_sums_refusals(capi, lib):
    def call(g="default", a=FAKE, b=FAKE + 64, n_vol=2, sums=FAKE + 128, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_overlap_sums(g, a, b, n_vol, sums, work, work_bytes, None)

    who = "nca_vol_overlap_sums:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(a=None), who, "a is NULL")
    refused(capi, lib, call(b=None), who, "b is NULL")
    refused(capi, lib, call(sums=None), who, "sums is NULL")
    assert call(b=FAKE, work=None) == E_WORKSPACE          # a stack against itself is a valid call
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("skel", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE
    # a workgroup per 4096 nodes of a volume: 2^24 volumes of 2 x 2 x 2 are one launch, one more is not
    assert call(n=(2, 2, 2), n_vol=1 << 24, work=None) == E_WORKSPACE
    refused(capi, lib, call(n=(2, 2, 2), n_vol=(1 << 24) + 1), "tiles", "one launch", str((1 << 24) + 1))
    g = grid(capi)
    need = lib.nca_vol_overlap_sums_workspace(C.byref(g), 2)
    assert need == 256          # 2 volumes of one workgroup, 16 bytes each
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_workspace_queries(capi, lib):
    def q(fn, n, n_vol, **kw):
        return fn(C.byref(grid(capi, n=n, **kw)), n_vol)

    skel, over = lib.nca_vol_softskel_workspace, lib.nca_vol_overlap_sums_workspace
    assert q(skel, (2, 2, 2), 1) == 256 and q(skel, (4, 4, 4), 1) == 512 and q(skel, (4, 4, 4), 3) == 1536
    assert q(skel, (3, 5, 65), 2) == (2 * 975 * 8 + 255) // 256 * 256
    assert q(skel, (512,) * 3, 256) == 8 * 256 * 512 ** 3          # beyond 2^32: a size_t
    assert q(skel, (4, 4, 1 << 20), 1) == 8 * 16 << 20          # no axis limit
    for n_vol in (1, 2, 7):
        for n in ((3, 4, 5), (9, 4, 130), (33, 17, 65)):
            nodes = n[0] * n[1] * n[2]
            assert q(skel, n, n_vol) == (n_vol * nodes * 8 + 255) // 256 * 256
            assert q(over, n, n_vol) == (n_vol * ((nodes + 4095) // 4096) * 16 + 255) // 256 * 256
    assert q(over, (2, 2, 2), 1) == 256 and q(over, (16, 16, 16), 1) == 256 and q(over, (16, 16, 17), 1) == 256 and q(over, (64, 64, 64), 5) == 5 * 64 * 16
    for fn in (skel, over):
        assert fn(None, 1) == 0
        for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1)):
            assert q(fn, *bad) == 0, bad
        assert q(fn, (4, 4, 4), 1, reserved=1) == 0 and q(fn, (4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0


# ----------------------------------------------------------------------------- the oracle against the published torch expression
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_oracle_equals_the_torch_expression(shape):
    for kind in ("random", "signed", "binary"):
        stack = np.stack([ref.volume(shape, kind, seed=s) for s in range(2)])
        for K in (0, 1, 3, 5):
            got = ref.soft_skeleton(stack, K)
            want = ref.torch_soft_skeleton(torch.from_numpy(stack)[:, None], K)[:, 0].numpy()
            assert got.dtype == np.float32 and np.array_equal(got, want), (kind, K)
            assert np.array_equal(ref.soft_skeleton(stack[1], K), got[1])          # every volume on its own
            if kind == "binary":
                assert set(np.unique(got).tolist()) <= {0.0, 1.0} and (got <= stack).all(), K          # binary, a subset of the mask


def test_the_order_of_the_comparisons_decides_nan_and_the_sign_of_zero():
    x = np.zeros((3, 3, 3), dtype=np.float32)
    x[1, 1, 1] = np.nan
    e = ref.erode(x)
    assert np.isnan(e[1, 1, 1]) and np.isnan(e).sum() == 1          # a NaN centre stays, a NaN neighbour is passed over
    d = ref.dilate(x)
    assert np.isnan(d[1, 1, 1]) and np.isnan(d).sum() == 1
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32).reshape(1, 1, 3).repeat(2, 0).repeat(2, 1)
    assert np.array_equal(np.signbit(ref.erode(z)), np.signbit(z)) and np.array_equal(np.signbit(ref.dilate(z)), np.signbit(z))          # the centre comes first
    assert not np.signbit(ref.relu(np.array([-0.0, -1.0, np.nan], dtype=np.float32))).any()


# ----------------------------------------------------------------------------- analytic properties
def test_a_straight_tube_has_its_axis_as_skeleton():
    for r in (1, 2, 3.5):
        for K in (3, 4, 10):
            s = ref.soft_skeleton(ref.tube(r), K)
            assert np.array_equal(s, ref.tube_axis()) and s.sum() == 40, (r, K)
    assert not ref.soft_skeleton(ref.tube(2), 1).any()          # too few iterations for radius 2: empty
    assert np.array_equal(ref.soft_skeleton(ref.tube(3.5), 10), ref.soft_skeleton(ref.tube(3.5), 40))          # an empty E_j changes nothing
    assert not ref.soft_skeleton(np.ones((5, 6, 7), dtype=np.float32), 3).any()          # the faces do not erode: a full volume has no skeleton


# ----------------------------------------------------------------------------- clDice from oracle skeletons, on CPU tensors
def oracle_cldice(pred, truth, K, smooth=0.0):
    from nerfca_amd import metrics
    sp, st = ref.soft_skeleton(pred, K), ref.soft_skeleton(truth, K)
    return metrics.cldice_reductions(torch.from_numpy(sp), torch.from_numpy(pred), torch.from_numpy(st), torch.from_numpy(truth), smooth), sp, st


def test_cldice_reductions_on_injected_skeletons():
    K = 4
    for mask in (ref.tube(2), ref.thick_tree()[0]):          # a mask against itself
        got, _, _ = oracle_cldice(mask, mask, K)
        assert float(got["cldice"]) == float(got["tprec"]) == float(got["tsens"]) == 1.0
        assert all(v.dtype == torch.float64 and v.shape == () for v in got.values())
    got, _, _ = oracle_cldice(ref.tube(2), ref.tube(2, shift=2), K)          # each axis still inside the other tube
    assert float(got["cldice"]) == float(got["tprec"]) == float(got["tsens"]) == 1.0
    got, _, _ = oracle_cldice(ref.tube(2), ref.tube(2, shift=7), K)          # disjoint
    assert float(got["tprec"]) == 0.0 and float(got["tsens"]) == 0.0 and float(got["cldice"]) == 0.0
    got, sp, _ = oracle_cldice(ref.tube(2, length=20), ref.tube(2), K)          # half the tube
    assert sp.sum() == 18 and sp[12, 12, :].sum() == 18          # the open end erodes: 18 nodes on the axis
    assert float(got["tprec"]) == 1.0 and float(got["tsens"]) == 0.5
    assert abs(float(got["cldice"]) - 2.0 / 3.0) <= 4 * 2.0 ** -53
    # a leading shape, and the empty skeleton: NaN at smooth = 0, the quotient with smooth
    pair = np.stack([ref.tube(2), np.ones(ref.TUBE_SHAPE, dtype=np.float32)])
    got, _, _ = oracle_cldice(pair, np.stack([ref.tube(2)] * 2), K)
    assert got["cldice"].shape == (2,) and float(got["cldice"][0]) == 1.0 and math.isnan(float(got["tprec"][1])) and math.isnan(float(got["cldice"][1]))
    got, _, _ = oracle_cldice(pair, np.stack([ref.tube(2)] * 2), K, smooth=1.0)
    assert float(got["tprec"][1]) == 1.0 and float(got["tsens"][1]) == 1.0 and float(got["cldice"][0]) == 1.0
    from nerfca_amd import metrics
    a = torch.zeros(2, 3, 4, 5)
    with pytest.raises(metrics._capi.NcaError, match="differ in shape"):
        metrics.cldice_reductions(a, a, a, a[:1])
    with pytest.raises(metrics._capi.NcaError, match="smooth"):
        metrics.cldice_reductions(a, a, a, a, smooth=-1.0)


def test_the_skeleton_of_a_thick_phantom_tree_follows_its_centreline():
    """The seed-0 tree at 64^3, its centreline thickened to 2.5 nodes, K = 4: measured with the torch expression, every centreline node lies
    within 2 nodes of the skeleton and 99 % of the skeleton within 1.5 nodes of the centreline; the margins cover another rasterisation."""
    mask, centre = ref.thick_tree()
    s = ref.thick_tree_skeleton(4)
    assert set(np.unique(s).tolist()) == {0.0, 1.0} and (s <= mask).all()
    to_skeleton, to_centre = scipy.ndimage.distance_transform_edt(s == 0), scipy.ndimage.distance_transform_edt(~centre)
    covered, close = float((to_skeleton[centre] <= 2.0).mean()), float((to_centre[s > 0] <= 1.5).mean())
    print(f"thick tree: {int(mask.sum())} nodes, {int(centre.sum())} on the centreline, {int(s.sum())} in the skeleton; covered {covered:.4f}, close {close:.4f}")
    assert covered >= 0.97 and close >= 0.97


def test_overlap_sums_oracle():
    a, b = np.stack([ref.volume((4, 5, 6), "binary", s) for s in (0, 1)]), np.stack([ref.volume((4, 5, 6), "binary", s) for s in (2, 3)])
    got = ref.overlap_sums(a, b)
    assert got.dtype == np.float64 and np.array_equal(got, np.stack([(a * b).sum(axis=(1, 2, 3)), a.sum(axis=(1, 2, 3))], axis=1))


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import metrics
    a = torch.zeros(2, 4, 4, 4)
    for call in (lambda: metrics.soft_skeleton(a, 3), lambda: metrics.soft_skeleton(a > 0, 3), lambda: metrics.soft_skeleton(a, 3, threshold=0.5),
                 lambda: metrics.soft_skeleton(a.numpy(), 3), lambda: metrics.soft_skeleton(None, 3), lambda: metrics.cldice(a, a, iterations=3),
                 lambda: metrics.cldice(a, a > 0, iterations=3, threshold=0.5), lambda: metrics.cldice(a, None, iterations=3)):
        with pytest.raises(capi.NcaError):
            call()
    import inspect
    sig = inspect.signature(metrics.cldice).parameters
    assert sig["iterations"].kind is inspect.Parameter.KEYWORD_ONLY and sig["iterations"].default is inspect.Parameter.empty
    assert sig["threshold"].default is None and sig["pred_threshold"].default is None and sig["smooth"].default == 0.0
    assert inspect.signature(metrics.soft_skeleton).parameters["threshold"].default is None
    for bad in (-1, 1.5, MAX_ITER + 1, True):
        with pytest.raises(capi.NcaError, match="iterations"):
            metrics._skel_iterations(bad, "soft_skeleton")
    assert metrics._skel_iterations(0, "x") == 0 and metrics._skel_iterations(4.0, "x") == 4 and metrics._skel_iterations(MAX_ITER, "x") == MAX_ITER


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(capsys):
    cv = _tool("compare_volumes")
    base = ["a", "b", "--bounds", "0,1,0,1,0,1", "--threshold", "3"]
    assert cv.parser().parse_args(cv.join_args(base)).cldice is None
    assert cv.parser().parse_args(cv.join_args(base + ["--cldice", "4"])).cldice == 4
    ps = _tool("phantom_study")
    assert ps.parser().parse_args([]).cldice is None and ps.parser().parse_args(["--distances", "--cldice", "4"]).cldice == 4
    sb = _tool("skel_bench")
    args = sb.parser().parse_args(["--out", "profiles/skel_bench.txt"])
    assert args.out == "profiles/skel_bench.txt" and args.passes == 3 and args.sides == "128,256" and args.volumes == "1,10" and args.iterations == "4,10"
    for tool, argv in ((sb, ["--help"]), (sb, ["--passes", "many"]), (sb, ["--nonsense"]), (cv, cv.join_args(base + ["--cldice", "four"])), (ps, ["--cldice"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    # the column needs the study it is a column of: refused before anything runs
    with pytest.raises(SystemExit) as e:
        ps.main(["--cldice", "4"])
    assert "--distances" in str(e.value.code)
