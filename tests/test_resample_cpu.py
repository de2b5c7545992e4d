"""The cubic-spline zoom (nca_vol_spline_filter, nca_vol_zoom, ccta.spline_filter / zoom / resample, resample= of ccta.prepare_ccta):
everything that can be checked without a launch -- the C-ABI surface, every refusal (with device pointers that are never read), the
workspace query, the numpy oracle of the GPU tests (tests/resample_ref.py) held to scipy.ndimage, the refusals of the Python layer and the
command lines.

The oracle against scipy 1.15: the interpolation from scipy's own coefficients is scipy's bit for bit at orders 0 and 3; the prefilter is a
few f64 units off scipy.ndimage.spline_filter, G = max|oracle - scipy| / max|vol| between 2^-47.9 and 2^-47.2 on the five cases below, held
to 2^-44; the whole zoom is within one f32 step plus that."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import scipy.ndimage
import torch

from conftest import ROOT

import resample_ref as ref
import nca_testlib as T
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_spline_filter", "nca_vol_zoom_workspace", "nca_vol_zoom", "nca_resample_last_error")
MAX_AXIS = 512
refused = functools.partial(T.refused, "resample")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_filt_last_error(void)", "int nca_vol_spline_filter(", "size_t nca_vol_zoom_workspace(", "int nca_vol_zoom(", "nca_resample_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert callable(capi.check_resample)
    from nerfca_amd import ccta
    for name in ("spline_filter", "zoom", "resample"):
        assert callable(getattr(ccta, name)), name


grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def c_m(m):
    return (C.c_int32 * 3)(*m)


# ----------------------------------------------------------------------------- refusals
def test_spline_filter_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, coeff=FAKE + 64, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_spline_filter(g, vol, n_vol, coeff, None)

    who = "nca_vol_spline_filter:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(coeff=None), who, "coeff is NULL")
    refused(capi, lib, call(coeff=FAKE), who, "coeff is vol")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("resample", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for a in range(3):
        n = [4, 5, 6]
        n[a] = MAX_AXIS + 1
        refused(capi, lib, call(n=n), f"n[{a}] = {MAX_AXIS + 1}", "NCA_EDT_MAX_AXIS", code=E_UNSUPPORTED)
    # 2^24 + 1 volumes of 2 x 2 x 2: one workgroup per volume (axis 0) and per plane (axis 1)
    refused(capi, lib, call(n=(2, 2, 2), n_vol=(1 << 24) + 1), "tiles", "one launch", str(((1 << 24) + 1) * 2))
    refused(capi, lib, call(n=(MAX_AXIS, MAX_AXIS, 2), n_vol=1025), "tiles", "one launch", str(1025 << 14))          # the rows of axis 2, sixteen to a workgroup


def test_zoom_refusals(capi, lib):
    ok_m = c_m((3, 9, 4))

    def call(g="default", vol=FAKE, n_vol=2, m=ok_m, order=3, out=FAKE + 64, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_zoom(g, vol, n_vol, m, order, out, work, work_bytes, None)

    who = "nca_vol_zoom:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(m=None), who, "m is NULL")
    refused(capi, lib, call(out=None), who, "out is NULL")
    refused(capi, lib, call(out=FAKE), who, "out is vol")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    for order in (0, 3):
        T.grid_refusals("resample", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2, order=order))
    for bad in (1, 2, 4, 5, -1):
        refused(capi, lib, call(order=bad), f"order = {bad}", "neither 0 nor 3")
    for a in range(3):
        for bad in (1, 0, -7):
            m = [3, 9, 4]
            m[a] = bad
            refused(capi, lib, call(m=c_m(m)), f"m[{a}] = {bad}", "2 nodes")
            refused(capi, lib, call(m=c_m(m), order=0), f"m[{a}] = {bad}", "2 nodes")
        n = [4, 5, 6]
        n[a] = MAX_AXIS + 1
        refused(capi, lib, call(n=n), f"n[{a}] = {MAX_AXIS + 1}", "NCA_EDT_MAX_AXIS", code=E_UNSUPPORTED)
        m = [2, 2, 2]
        m[a] = 1 << 20          # no limit on the output: 2^20 nodes along each axis in turn get as far as the workspace
        assert call(m=c_m(m), work=None) == E_WORKSPACE
    big = (1 << 31) - 1
    refused(capi, lib, call(m=c_m((big, big, big))), "overflow", str(big))
    refused(capi, lib, call(m=c_m((1 << 11, 1 << 11, 1 << 10)), n_vol=2), "one launch", str(1 << 33))          # 2^33 output nodes
    assert call(m=c_m((1 << 11, 1 << 11, 1 << 10)), n_vol=1, work=None) == E_WORKSPACE                          # 2^32 are one launch
    refused(capi, lib, call(n=(MAX_AXIS, MAX_AXIS, 2), n_vol=1025), "tiles", "one launch", str(1025 << 14))          # the prefilter's rows, sixteen to a workgroup
    assert call(n=(MAX_AXIS, MAX_AXIS, 2), n_vol=1024, work=None) == E_WORKSPACE
    g = grid(capi)
    need = lib.nca_vol_zoom_workspace(C.byref(g), 2, 3)
    assert need == 2048          # 2 * 120 nodes * 8 bytes = 1920, rounded up to 256
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)
    # order 0 stages nothing: a long axis is accepted (refused here only for the output size, the last check before the launch)
    refused(capi, lib, call(n=(2, 2, 1 << 20), order=0, work=None, work_bytes=0, m=c_m((1 << 11, 1 << 11, 1 << 11))), "one launch")


def test_workspace_query(capi, lib):
    fn = lib.nca_vol_zoom_workspace

    def q(n, n_vol, order=3, **kw):
        return fn(C.byref(grid(capi, n=n, **kw)), n_vol, order)

    assert q((2, 2, 2), 1) == 256 and q((4, 4, 4), 1) == 512 and q((4, 4, 4), 3) == 1536
    assert q((3, 5, 65), 2) == (2 * 975 * 8 + 255) // 256 * 256
    assert fn(None, 1, 3) == 0 and fn(None, 1, 0) == 0
    for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1)):
        assert q(*bad) == 0, bad
    assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0
    for order in (1, 2, 4, 5, -1):
        assert q((4, 4, 4), 1, order) == 0
    assert q((4, 4, 4), 1, 0) == 0 and q((4, 4, MAX_AXIS + 1), 1, 0) == 0          # order 0 needs none
    assert q((4, 4, MAX_AXIS + 1), 1) == 0 and q((MAX_AXIS,) * 3, 64) == 8 * 64 * MAX_AXIS ** 3          # beyond 2^32: a size_t
    for n_vol in (1, 2, 7):
        for n in ((3, 4, 5), (9, 4, 130), (33, 17, 65)):
            assert q(n, n_vol) == (n_vol * n[0] * n[1] * n[2] * 8 + 255) // 256 * 256


# ----------------------------------------------------------------------------- the oracle against scipy
def no_overshoot(shape, m):
    for n, k in zip(shape, m):
        assert float(k - 1) * ref.step_of(n, k) <= float(n - 1), (n, k)


def zoom_bound(sci, vol):
    """Per node: one f32 step of scipy's value (the prefilters differ before the rounding) plus the prefilter's bound."""
    return np.spacing(np.abs(sci.astype(np.float32))).astype(np.float64) + ref.G_BOUND * float(np.abs(vol).max())


@pytest.mark.parametrize("shape,factors", ref.SCIPY_CASES, ids=lambda v: str(v))
def test_oracle_against_scipy(shape, factors):
    m = ref.out_shape(shape, factors)
    no_overshoot(shape, m)
    vol = ref.volume(shape)
    sci_c = scipy.ndimage.spline_filter(vol, 3, output=np.float64)
    # the interpolation stage, from scipy's own coefficients: bit for bit
    got3, want3 = ref.interp(sci_c, m, 3), scipy.ndimage.zoom(sci_c, factors, order=3, prefilter=False)
    assert got3.shape == want3.shape == m and np.array_equal(got3.view(np.int64), want3.view(np.int64))
    got0, want0 = ref.interp(vol, m, 0), scipy.ndimage.zoom(vol, factors, order=0)
    assert got0.dtype == np.float32 and np.array_equal(got0.view(np.int32), want0.view(np.int32))
    assert np.array_equal(ref.zoom(vol, m, 0).view(np.int32), want0.view(np.int32))
    # the prefilter: to a bound
    c = ref.spline_filter(vol)
    G = float(np.abs(c - sci_c).max() / np.abs(vol).max())
    print(f"prefilter {shape}: G = {G:.3e} = 2^{np.log2(G) if G else -np.inf:.1f}, bound 2^-44")
    assert c.dtype == np.float64 and G <= ref.G_BOUND
    # the whole zoom
    mine, sci = ref.zoom(vol, m), scipy.ndimage.zoom(vol, factors, order=3)
    assert mine.dtype == sci.dtype == np.float32 and mine.shape == sci.shape
    off = np.abs(mine.astype(np.float64) - sci.astype(np.float64))
    print(f"zoom {shape} -> {m}: {int((off > 0).sum())} of {off.size} nodes differ from scipy, at most {off.max():.3e}")
    assert (off <= zoom_bound(sci, vol)).all()
    stack = np.stack([vol, ref.volume(shape, seed=1)])
    assert np.array_equal(ref.zoom(stack, m)[0].view(np.int32), mine.view(np.int32))          # the leading axis is not resampled


def test_the_overshoot_pair_is_not_scipys():
    """4 -> 188 nodes: scipy's last coordinate lands above 3 and its whole last plane is cval = 0; the oracle's last node is the last input
    node.  Every plane before the last is scipy's."""
    assert ref.overshoots(4, 188) and not ref.overshoots(4, 187) and ref.out_shape((4, 3, 3), (47, 1, 1)) == (188, 3, 3)
    vol = ref.volume((4, 3, 3))
    sci, mine = scipy.ndimage.zoom(vol, (47, 1, 1), order=3), ref.zoom(vol, (188, 3, 3))
    assert (sci[-1] == 0).all() and (np.abs(mine[-1]) > 1.0).all()
    assert (np.abs(mine[:-1].astype(np.float64) - sci[:-1]) <= zoom_bound(sci[:-1], vol)).all()
    assert (np.abs(mine[-1].astype(np.float64) - vol[-1]) <= zoom_bound(vol[-1], vol)).all()          # a spline interpolates its nodes
    # and the plane before the last, 3 / 187 of a node away, is as near as the data's slope allows
    assert np.abs(mine[-1] - mine[-2]).max() <= 3 / 187 * 3.0 * np.abs(vol).max()
    sci0, mine0 = scipy.ndimage.zoom(vol, (47, 1, 1), order=0), ref.zoom(vol, (188, 3, 3), 0)
    assert (sci0[-1] == 0).all() and np.array_equal(mine0[-1], vol[-1]) and np.array_equal(mine0[:-1], sci0[:-1])


def test_oracle_edges():
    assert ref.zn_of(2) == ref.Z and ref.zn_of(4) == ref.Z * ref.Z * ref.Z
    for n in (2, 3, 7):
        j = np.arange(-2, 2 * n + 2)
        want = np.pad(np.arange(n), (2 * n, 2 * n), mode="reflect")[2 * n - 2:2 * n - 2 + len(j)]
        assert np.array_equal(ref.mirror(j, n), want)
    vol = ref.volume((3, 4, 5))
    same = ref.zoom(vol, (3, 4, 5))          # a zoom of 1: the spline interpolates its nodes
    assert (np.abs(same.astype(np.float64) - vol) <= np.spacing(np.abs(vol)) + ref.G_BOUND * np.abs(vol).max()).all()
    x = vol.copy()
    x[1, 2, 3], x[0, 0, 0] = np.nan, np.inf
    got = ref.zoom(x, (3, 4, 5), 0)
    assert np.array_equal(got.view(np.int32), x.view(np.int32))


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import ccta
    a = torch.zeros(2, 4, 4, 4)
    bounds = ((0.0, 3.0),) * 3
    for call in (lambda: ccta.spline_filter(a), lambda: ccta.zoom(a, 2.0), lambda: ccta.zoom(a, 2.0, order=0), lambda: ccta.resample(a, bounds, 0.5),
                 lambda: ccta.prepare_ccta(a, a, bounds, resample=1.0), lambda: ccta.zoom(a.numpy(), 2.0), lambda: ccta.spline_filter(None)):
        with pytest.raises(capi.NcaError):
            call()
    import inspect
    sig = inspect.signature(ccta.prepare_ccta).parameters
    assert sig["resample"].default is None and sig["label_order"].default == 3
    assert inspect.signature(ccta.zoom).parameters["order"].default == 3
    # the shape rule, which runs before anything touches a device: scipy's, with Python's round
    assert ccta._zoom_shape((5, 6, 7), (1.5, 0.8, 2.0), None, "zoom") == [8, 5, 14] == list(ref.out_shape((5, 6, 7), (1.5, 0.8, 2.0)))
    assert ccta._zoom_shape((12, 20, 35), (2.0, 1.2, 0.7), None, "zoom") == [24, 24, 24]          # 35 x 0.7 = 24.5 rounds to even
    assert ccta._zoom_shape((5, 6, 7), 9.0, (2, 3, 4), "zoom") == [2, 3, 4]
    for kw in (dict(zoom=(1.0, 2.0)), dict(zoom=0.0), dict(zoom=-1.0), dict(zoom=float("nan")), dict(zoom=0.2), dict(zoom=None), dict(zoom=1.0, output_shape=(2, 3)),
               dict(zoom=1.0, output_shape=(2, 3, 1)), dict(zoom=1.0, output_shape=(2, 3, 4.5)), dict(zoom=1.0, output_shape=7)):
        with pytest.raises(capi.NcaError):
            ccta._zoom_shape((5, 6, 7), kw["zoom"], kw.get("output_shape"), "zoom")
    fac, target = ccta._zoom_factors((16, 18, 40), ((0.0, 7.5), (1.0, 7.8), (-2.0, 9.7)), 0.25, "resample")
    assert target == [0.25] * 3 and fac == [(7.5 / 15) / 0.25, (6.8 / 17) / 0.25, (11.7 / 39) / 0.25]
    for bad in (0.0, -1.0, float("inf"), (1.0, 2.0)):
        with pytest.raises(capi.NcaError):
            ccta._zoom_factors((4, 4, 4), bounds, bad, "resample")
    with pytest.raises(capi.NcaError):
        ccta._zoom_factors((4, 4, 4), ((0.0, 3.0), (2.0, 2.0), (0.0, 3.0)), 1.0, "resample")
    r = ccta._round_half_away(torch.tensor([0.49, 0.5, 1.5, 2.5, -0.5, -0.49, -1.5, 0.0]))
    assert r.tolist() == [0.0, 1.0, 2.0, 3.0, -1.0, 0.0, -2.0, 0.0]


def test_prepare_ccta_without_resample_takes_the_old_path(monkeypatch):
    """resample=None never reaches zoom: the volumes go to vessel_contrast as they came, on the bounds as given."""
    from nerfca_amd import ccta
    calls, seen = [], {}
    monkeypatch.setattr(ccta, "zoom", lambda *a, **k: calls.append((a, k)) or (_ for _ in ()).throw(AssertionError("zoom was called")))
    monkeypatch.setattr(ccta._view, "check_volume", lambda *a, **k: None)
    monkeypatch.setattr(ccta, "_mask_input", lambda vol, who: vol)

    def contrast(m, bounds, **kw):
        seen["m"], seen["bounds"], seen["kw"] = m, bounds, kw
        return torch.zeros_like(m), m > 0

    monkeypatch.setattr(ccta, "vessel_contrast", contrast)
    hu = torch.arange(64, dtype=torch.float32).reshape(4, 4, 4) * 10 - 300
    mask = (hu > 100).to(torch.float32)
    bounds = ((0.0, 6.0), (0.0, 3.6), (0.0, 2.1))
    out = ccta.prepare_ccta(hu, mask, bounds, grow=2)
    assert calls == [] and seen["m"] is mask and seen["bounds"] is bounds and seen["kw"] == {"grow": 2}
    assert out["bounds"] == bounds and out["static"].shape == hu.shape
    assert torch.equal(out["static"], torch.where(mask > 0, torch.zeros(()), ccta.hounsfield_to_attenuation(hu)))
    # with a spacing it does reach zoom, three times when there are labels, with the factors of resample; the first call is the attenuation
    with pytest.raises(AssertionError, match="zoom was called"):
        ccta.prepare_ccta(hu, mask, bounds, resample=1.0)
    (args, kw), = calls
    assert args[1] == [2.0, (3.6 / 3) / 1.0, (2.1 / 3) / 1.0] and kw == {"order": 3} and args[0].dtype == torch.float32
    with pytest.raises(ccta._capi.NcaError, match="label_order"):
        ccta.prepare_ccta(hu, mask, bounds, resample=1.0, label_order=1)


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(capsys):
    pc = _tool("prepare_ccta")
    base = ["--raw", "raw.npy", "--mask", "mask.npy", "--bounds", "0,22,0,22.8,0,23.8", "--out", "d/"]
    args = pc.parser().parse_args(pc.join_args(base))
    assert args.resample is None and args.label_order == 3
    args = pc.parser().parse_args(pc.join_args(base + ["--resample", "1"]))
    assert args.resample == 1.0 and args.label_order == 3
    args = pc.parser().parse_args(pc.join_args(base + ["--resample", "0.5,0.4,0.3", "--label-order", "0"]))
    assert args.resample == (0.5, 0.4, 0.3) and args.label_order == 0
    zb = _tool("zoom_bench")
    args = zb.parser().parse_args(["--out", "profiles/zoom_bench.txt"])
    assert args.out == "profiles/zoom_bench.txt" and args.passes == 3 and args.sides == "128,256" and args.volumes == "1,10" and args.factors == "0.5,1.6"
    for tool, argv in ((pc, pc.join_args(base + ["--resample", "0"])), (pc, pc.join_args(base + ["--resample", "1,2"])), (pc, pc.join_args(base + ["--resample", "a"])),
                       (pc, pc.join_args(base + ["--resample", "-1"])), (pc, pc.join_args(base + ["--label-order", "1"])), (zb, ["--passes", "many"]), (zb, ["--nonsense"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert e.value.code != 0
    capsys.readouterr()
