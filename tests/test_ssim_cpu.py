"""Structural similarity (nca_ssim, nca_ssim_grad, metrics.ssim / psnr / compare_sequences, the ssim_* arguments of drr.fit_volumes and
tools/fit_volumes.py): everything that can be checked without a launch -- the C-ABI surface, every refusal of the entry points (with device
pointers that are never read), the workspace query, the window, the f64 oracle of the GPU tests (tests/ssim_ref.py) pinned two independent
ways, the refusals of the Python layer and the command lines."""
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

import ssim_ref as ref
import nca_testlib as T
from nca_testlib import E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_ssim", "nca_ssim_grad_workspace", "nca_ssim_grad", "nca_ssim_last_error")
refused = functools.partial(T.refused, "ssim")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    assert header.index("nca_phantom_last_error(void)") < header.index("int nca_ssim(") < header.index("int nca_ssim_grad(") < header.index("nca_ssim_last_error(void)")
    assert int(re.search(r"NCA_SSIM_MAX_WIN = (\d+)", header).group(1)) == 11
    assert callable(capi.check_ssim)
    import nerfca_amd
    assert nerfca_amd.metrics.ssim and nerfca_amd.metrics.MAX_WIN == 11 and "metrics" in nerfca_amd.__all__


def cwin(values):
    return (C.c_double * len(values))(*values)


@pytest.mark.parametrize("entry", ["nca_ssim", "nca_ssim_grad"])
def test_refusals(capi, lib, entry):
    def call(N=2, H=16, W=20, x=FAKE, y=FAKE, range=FAKE, K=11, win="default", k1=0.01, k2=0.03, sum=FAKE, map=None, scale=FAKE, g_x=FAKE, work=FAKE,
             work_bytes=1 << 62):
        win = cwin(list(ref.gaussian(K if 1 <= K <= 64 else 1))) if isinstance(win, str) else win
        if entry == "nca_ssim":
            return lib.nca_ssim(N, H, W, x, y, range, K, win, k1, k2, sum, map, None)
        return lib.nca_ssim_grad(N, H, W, x, y, range, K, win, k1, k2, scale, g_x, work, work_bytes, None)

    for name in ("x", "y", "range", "win") + (("sum",) if entry == "nca_ssim" else ("scale", "g_x")):
        refused(capi, lib, call(**{name: None}), entry + ":", name + " is NULL")
    for name in ("N", "H", "W"):
        refused(capi, lib, call(**{name: 0}), entry + ":", f"{name} = 0", "positive")
        refused(capi, lib, call(**{name: -3}), f"{name} = -3", "positive")
    for bad in (0, -1, 2, 10, 12, 13):
        refused(capi, lib, call(K=bad), f"K = {bad}", "odd")
    refused(capi, lib, call(H=10), "H = 10", "K = 11")
    refused(capi, lib, call(W=4, K=5), "W = 4", "K = 5")
    for a, (bad, word) in ((0, (math.inf, "inf")), (1, (-math.inf, "-inf")), (2, (math.nan, "nan"))):
        w = [0.25, 0.5, 0.25]
        w[a] = bad
        refused(capi, lib, call(K=3, win=cwin(w)), f"win[{a}] = {word}", "finite")
    for name in ("k1", "k2"):
        for bad, word in ((0.0, "0"), (-0.01, "-0.01"), (math.inf, "inf"), (-math.inf, "-inf"), (math.nan, "nan")):
            refused(capi, lib, call(**{name: bad}), f"{name} = {word}", "positive")
    big = (1 << 31) - 1
    refused(capi, lib, call(N=big, H=big, W=big), "overflow", str(big))
    # 2^50 pixels fit int64 byte offsets with room to spare, but make 2^20 x 2^11 x 2^10 tiles of 16 x 32: far more than the 2^24 one launch carries
    refused(capi, lib, call(N=1 << 20, H=1 << 15, W=1 << 15), "tiles", "one launch", str(1 << 41))
    refused(capi, lib, call(N=16, H=1 << 15, W=1 << 15), "tiles", "one launch", str(1 << 25))          # 2^25 tiles of 256 threads: beyond the 2^32 threads of a launch
    if entry == "nca_ssim_grad":
        need = lib.nca_ssim_grad_workspace(2, 16, 20, 11)
        assert need == 24 * 2 * 6 * 10
        refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
        refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
        refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_workspace_query(lib):
    q = lib.nca_ssim_grad_workspace
    assert q(1, 11, 11, 11) == 24 and q(3, 43, 130, 11) == 24 * 3 * 33 * 120 and q(1, 4, 66, 1) == 24 * 4 * 66
    for bad in ((0, 16, 16, 3), (1, 0, 16, 3), (1, 16, -1, 3), (1, 16, 16, 4), (1, 16, 16, 13), (1, 2, 16, 3), (1, 16, 2, 3)):
        assert q(*bad) == 0, bad
    for K in (1, 3, 11):
        base = (2, 16, 20)
        for axis in range(3):
            last = 0
            for step in range(0, 40, 3):
                args = list(base)
                args[axis] += step
                got = q(*args, K)
                assert got >= last and got > 0, (K, args)
                last = got
    assert q(1 << 10, 1 << 14, 1 << 14, 11) == 24 * (1 << 10) * ((1 << 14) - 10) ** 2          # beyond 2^32: a size_t


# ----------------------------------------------------------------------------- the window
@pytest.mark.parametrize("K,sigma", [(11, 1.5), (3, 1.5), (1, 1.5), (7, 0.8), (9, 2.5)])
def test_gaussian_window(K, sigma):
    from nerfca_amd import metrics
    g = metrics.gaussian_window(K, sigma)
    assert g.dtype == np.float64 and g.shape == (K,)
    assert abs(math.fsum(g) - 1.0) <= K * 2.0 ** -53
    assert np.array_equal(g, g[::-1])          # symmetric bit for bit
    d = np.arange(K) - (K - 1) / 2
    want = np.exp(-d * d / (2 * sigma * sigma))
    want = want / math.fsum(want)
    assert np.abs(g - want).max() <= 4 * 2.0 ** -53 * want.max()
    assert np.abs(g - ref.gaussian(K, sigma)).max() <= 4 * 2.0 ** -53 * want.max()


def test_gaussian_window_refuses_bad_arguments(capi):
    from nerfca_amd import metrics
    for bad in (0, 2, -3, 4.5):
        with pytest.raises(capi.NcaError):
            metrics.gaussian_window(bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(capi.NcaError):
            metrics.gaussian_window(11, bad)


# ----------------------------------------------------------------------------- the oracle
WINDOWS = ("gauss", "asym")


def window(K, kind):
    return ref.gaussian(K) if kind == "gauss" else ref.asymmetric(K)


@pytest.mark.parametrize("K,shape", ref.CASES)
def test_oracle_moments_equal_scipy_correlate1d(K, shape):
    """Pins the moment maps of tests/ssim_ref.py to scipy.ndimage.correlate1d along both axes, cropped to the positions whose window lies
    inside the image.  Both are sums of K^2 products of non-negative weights and one field; they differ only in the order of the sums, so
    they agree within K^2 2^-53 times the moment of |field|.  The asymmetric window shows which end of the window meets which pixel."""
    x, y, _ = ref.stack(3, shape)
    h = K // 2
    worst = 0.0
    for kind in WINDOWS:
        win = window(K, kind)
        for n in range(3):
            xd, yd = x[n].astype(np.float64), y[n].astype(np.float64)
            got = ref.ssim_image(x[n], y[n], 1.0, win)["m"]
            for name, v in (("x", xd), ("y", yd), ("xx", xd * xd), ("yy", yd * yd), ("xy", xd * yd)):
                full = scipy.ndimage.correlate1d(scipy.ndimage.correlate1d(v, win, axis=1, mode="constant"), win, axis=0, mode="constant")
                want = full[h:full.shape[0] - h, h:full.shape[1] - h]
                assert want.shape == got[name].shape == (shape[0] - K + 1, shape[1] - K + 1)
                size = ref.moments(np.abs(v), win)
                err = np.abs(got[name] - want)
                assert (err <= K * K * ref.U * size).all(), (kind, n, name)
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nan_to_num(err / (ref.U * size)).max()))
    print(f"K {K}, {shape}: moments within {worst:.2f} of 2^-53 moment(|v|) of scipy")


def test_oracle_window_orientation_is_visible():
    """With the asymmetric window, mirroring the window in either pass moves the moments far beyond rounding: what mutation (a) changes."""
    x, y, _ = ref.stack(3, (12, 75))
    win = ref.asymmetric(11)
    a = ref.ssim_image(x[0], y[0], 1.0, win)
    b = ref.ssim_image(x[0], y[0], 1.0, win[::-1].copy())
    assert np.abs(a["S"] - b["S"]).max() > 1e-3 and np.abs(a["grad"] - b["grad"]).max() > 1e-3 * np.abs(a["grad"]).max()


@pytest.mark.parametrize("K,shape", ref.CASES)
def test_oracle_gradient_equals_torch_autograd_in_f64(K, shape):
    """Pins the value and the gathered gradient of tests/ssim_ref.py (so the header's P, Q, R and F) to torch autograd through the conv2d
    expression of the same functional in f64.  The gradient is held within 512 * 2^-53 * mass(q), mass the sum of the absolute values of
    every term added into the pixel; measured over all cases and both windows: 153.8 at worst, on the smooth pair of (43, 130) (printed
    below; 2 to 25 on the noise pairs).  mass counts the terms of the gather only: the smooth pair's variances are small against its
    second moments, so the two orders of summing the moments already differ by more in b2, P, Q and R there.  S is held within 4e-13 of
    the functional's for the same reason; measured 1.33e-13."""
    worst_g, worst_s = 0.0, 0.0
    for kind in WINDOWS:
        win = window(K, kind)
        for n_img in ref.N_IMAGES:
            x, y, ranges = ref.stack(n_img, shape)
            for n in range(n_img):
                got = ref.ssim_image(x[n], y[n], ranges[n], win)
                xt = torch.from_numpy(x[n].astype(np.float64)).requires_grad_()
                total, S = ref.torch_ssim_sum(xt, torch.from_numpy(y[n].astype(np.float64)), float(ranges[n]), win)
                (want,) = torch.autograd.grad(total, xt)
                assert np.isfinite(got["grad"]).all() and (got["mass"] > 0).all()
                err = np.abs(got["grad"] - want.numpy())
                worst_g = max(worst_g, float((err / (ref.U * got["mass"])).max()))
                assert (err <= 512 * ref.U * got["mass"]).all(), (kind, n_img, n, float((err / (ref.U * got["mass"])).max()))
                err_s = np.abs(got["S"] - S.detach().numpy()).max()
                worst_s = max(worst_s, float(err_s))
                assert err_s <= 4e-13, (kind, n_img, n, err_s)
    print(f"K {K}, {shape}: gradient within {worst_g:.2f} of 2^-53 mass of autograd, S within {worst_s:.2e}")


@pytest.mark.parametrize("K,shape", ref.CASES)
def test_no_case_sits_on_a_pole(K, shape):
    seen_negative = False
    for kind in WINDOWS:
        for n_img in ref.N_IMAGES:
            got = ref.oracle(K, shape, n_img, kind)
            assert (got["b1b2"] >= 0.5 * got["c1c2"][:, None, None]).all()
            for k in ("S", "P", "Q", "R", "grad", "mass"):
                assert np.isfinite(got[k]).all(), k
            seen_negative = seen_negative or bool((got["S"] < 0).any())
    assert seen_negative or K == 1          # the anti-correlated pair (a window of one pixel has no covariance: its S is positive)


@pytest.mark.parametrize("K,shape", ref.CASES)
def test_identical_images_give_exactly_one(K, shape):
    x, y, ranges = ref.stack(3, shape)
    assert np.array_equal(x[2], y[2]) and not np.array_equal(x[0], y[0])
    for kind in WINDOWS:
        got = ref.oracle(K, shape, 3, kind)
        assert (got["S"][2] == 1.0).all() and got["sum"][2] == got["count"][2] == (shape[0] - K + 1) * (shape[1] - K + 1)
        assert not (got["S"][0] == 1.0).all()


def test_a_window_of_one_is_the_pixel_formula():
    x, y, ranges = ref.stack(3, (4, 66))
    for n in range(3):
        got = ref.ssim_image(x[n], y[n], ranges[n], np.array([1.0]))
        xd, yd, L = x[n].astype(np.float64), y[n].astype(np.float64), ranges[n]
        C1, C2 = (ref.K1 * L) * (ref.K1 * L), (ref.K2 * L) * (ref.K2 * L)
        # every variance is exactly 0, so a2 == b2 == C2 and S = a1 C2 / (b1 C2): the pixel formula up to those two roundings
        want = (2 * (xd * yd) + C1) / ((xd * xd + yd * yd) + C1)
        assert got["S"].shape == (4, 66) and np.abs(got["S"] - want).max() <= 4 * ref.U * np.abs(want).max()
        assert np.array_equal(got["m"]["x"], xd) and np.array_equal(got["m"]["xy"], xd * yd)


def test_a_bad_range_gives_nan():
    x, y, _ = ref.stack(3, (5, 70))
    for bad in (0.0, -1.0, math.inf, math.nan):
        got = ref.ssim_image(x[0], y[0], bad, ref.gaussian(3))
        assert np.isnan(got["S"]).all() and np.isnan(got["grad"]).all()


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import drr, metrics, synthetic
    a = torch.zeros(2, 16, 16)
    with pytest.raises(capi.NcaError):
        metrics.ssim(a, a, data_range=1.0)
    with pytest.raises(capi.NcaError):
        metrics.psnr(a, a, data_range=1.0)
    with pytest.raises(capi.NcaError):
        metrics.compare_sequences({"pred": a}, {"other": a})
    geo = synthetic.xcat_geometry(8)
    frames = [(0.0, 0.0, 0, torch.zeros(8, 8))]
    # a bad weight is refused before the frames are looked at (so before anything is allocated): the message names the weight
    for bad, word in ((-0.5, "ssim_weight = -0.5"), (math.nan, "ssim_weight = nan"), (math.inf, "ssim_weight = inf"), (-math.inf, "ssim_weight = -inf")):
        with pytest.raises(capi.NcaError, match=re.escape(word)):
            drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, ssim_weight=bad)
    with pytest.raises(capi.NcaError, match=re.escape("ssim_win = 11 is larger than the detector, 8 x 8")):
        drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, ssim_weight=0.5)
    for bad in (4, 13, 0):
        with pytest.raises(capi.NcaError, match=re.escape(f"ssim_win = {bad}")):
            drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, ssim_weight=0.5, ssim_win=bad)
    with pytest.raises(capi.NcaError, match="frame images"):          # weight 0: the window is not looked at, the CPU image is refused as before
        drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, ssim_weight=0.0, ssim_win=99)


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines_parse():
    fv = _tool("fit_volumes")
    args = fv.parser().parse_args(["--frames", "m.json", "--shape", "4,4,4", "--out", "o"])
    assert args.ssim_weight == 0.0 and args.ssim_win == 11 and args.tv_space == 0.0
    args = fv.parser().parse_args(fv.join_args(["--frames", "m.json", "--shape", "4,4,4", "--out", "o", "--ssim-weight", "0.25", "--ssim-win", "7"]))
    assert args.ssim_weight == 0.25 and args.ssim_win == 7
    cv = _tool("compare_views")
    args = cv.parser().parse_args(["a/manifest.json", "b/manifest.json", "--out", "t.json"])
    assert args.pred == "a/manifest.json" and args.truth == "b/manifest.json" and args.out == "t.json" and args.data_range is None
    sb = _tool("ssim_bench")
    args = sb.parser().parse_args(["--out", "profiles/ssim_bench.txt"])
    assert args.out == "profiles/ssim_bench.txt" and args.passes == 3
