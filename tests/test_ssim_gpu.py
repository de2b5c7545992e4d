"""Structural similarity on the GPU: nca_ssim and nca_ssim_grad against the f64 numpy transcription of their definition (tests/ssim_ref.py,
pinned to scipy and to torch autograd in tests/test_ssim_cpu.py), the autograd path of metrics.ssim, metrics.compare_sequences, and
drr.fit_volumes with the structural term on.  The kernels fix every operation: the map is the oracle's value rounded to f32 once, the
per-image sum is free only in the order of its terms (a sum of `count` terms of total size `sum |S|` lies within count 2^-53 sum |S| of
the exact sum, so two such sums are within twice that of each other), the gradient is gathered and rounded to f32 once.  Shapes: window 11
at one position, one tile row past a tile's width, one row and one column past the 16 x 32 tile, several ragged tiles; windows 3 and 1."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev  # noqa: F401

import ssim_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
START = 0.25          # what `sum` holds before a call: below half of every case's sum |S|, and exact when whole numbers are added to it
SCALES = ((1.0, 0.5, 2.0), (-1.5, 0.25, -0.125), (0.75, 0.0, 1.0))          # per image (a stack of one image takes the first entry of each): a negative vector, a zero entry
WINDOWS = ("gauss", "asym")          # the asymmetric window shows a window applied back to front in either pass


def window(K, kind):
    return ref.gaussian(K) if kind == "gauss" else ref.asymmetric(K)


def cwin(win):
    return (C.c_double * len(win))(*[float(w) for w in win])


def gpu_value(dev, x, y, ranges, win, want_map=True, start=START):
    """(sum f64 [N] after one nca_ssim into a vector that starts as `start`, map f32 [N,Hv,Wv] from a buffer pre-filled with NaN)."""
    from nerfca_amd import _capi, fused
    N, H, W = x.shape
    K = len(win)
    tx, ty = torch.tensor(np.asarray(x)).to(dev), torch.tensor(np.asarray(y)).to(dev)
    tr = torch.tensor(np.asarray(ranges, dtype=np.float64)).to(dev)
    total = torch.full((N,), start, dtype=torch.float64, device=dev)
    smap = torch.full((N, H - K + 1, W - K + 1), math.nan, dtype=torch.float32, device=dev) if want_map else None
    with torch.cuda.device(dev):
        _capi.check_ssim(_capi.lib().nca_ssim(N, H, W, _capi.ptr(tx), _capi.ptr(ty), _capi.ptr(tr), K, cwin(win), ref.K1, ref.K2, _capi.ptr(total),
                                              _capi.ptr(smap), fused._stream()))
    return total.cpu().numpy(), (smap.cpu().numpy() if want_map else None)


def gpu_gradient(dev, x, y, ranges, win, scale):
    """g_x f32 [N,H,W] of one nca_ssim_grad into a buffer pre-filled with NaN, the workspace exactly as large as the query says."""
    from nerfca_amd import _capi, fused
    N, H, W = x.shape
    K = len(win)
    lib = _capi.lib()
    tx, ty = torch.tensor(np.asarray(x)).to(dev), torch.tensor(np.asarray(y)).to(dev)
    tr = torch.tensor(np.asarray(ranges, dtype=np.float64)).to(dev)
    ts = torch.tensor(scale, dtype=torch.float64, device=dev)
    g = torch.full(x.shape, math.nan, dtype=torch.float32, device=dev)
    nbytes = lib.nca_ssim_grad_workspace(N, H, W, K)
    assert nbytes == 24 * N * (H - K + 1) * (W - K + 1)
    work = torch.full((nbytes // 8,), math.nan, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check_ssim(lib.nca_ssim_grad(N, H, W, _capi.ptr(tx), _capi.ptr(ty), _capi.ptr(tr), K, cwin(win), ref.K1, ref.K2, _capi.ptr(ts), _capi.ptr(g),
                                           _capi.ptr(work), nbytes, fused._stream()))
    return g.cpu().numpy()


def map_bound(S64):
    """One rounding to f32, plus room for one division a last bit off the host's."""
    return 2.0 ** -24 * np.abs(S64) + 4 * 2.0 ** -52 * np.abs(S64)


def sum_bound(want):
    """Per image: the order of the sum, plus the per-term slack of map_bound."""
    return 2 * want["count"] * U * want["abs_sum"] + 4 * 2.0 ** -52 * want["abs_sum"]


def configurations():
    for kind in WINDOWS:
        for n in ref.N_IMAGES:
            yield kind, n


# ----------------------------------------------------------------------------- 1. the map, 2. the sums
@pytest.mark.parametrize("K,shape", ref.CASES)
def test_map_and_sums_match_the_f64_oracle(dev, K, shape):
    worst_map, worst_sum, equal = 0.0, 0.0, True
    for kind, n in configurations():
        x, y, ranges = ref.stack(n, shape)
        want = ref.oracle(K, shape, n, kind)
        total, smap = gpu_value(dev, x, y, ranges, window(K, kind))
        assert smap.shape == want["S"].shape and smap.dtype == np.float32
        assert np.isfinite(smap).all(), f"{int((~np.isfinite(smap)).sum())} positions were not written"          # the buffer started as NaN
        err = np.abs(smap.astype(np.float64) - want["S"])
        tol = map_bound(want["S"])
        worst_map = max(worst_map, float((err / tol).max()))
        assert (err <= tol).all(), (kind, n, float((err / tol).max()), np.unravel_index(np.argmax(err - tol), err.shape))
        equal = equal and np.array_equal(smap, want["S"].astype(np.float32))
        got = total - START
        tol_s = sum_bound(want)
        err_s = np.abs(got - want["sum"])
        print(f"K {K}, {shape}, {kind}, N {n}: sums gpu {got} oracle {want['sum']} error {err_s} bound {tol_s}")
        assert (abs(START) <= 0.5 * want["abs_sum"]).all()          # what makes the bound hold for a sum that starts at START
        assert (err_s <= tol_s).all(), (kind, n, err_s, tol_s)
        worst_sum = max(worst_sum, float((err_s / tol_s).max()))
        if n == 3:          # the identical pair: every term is 1.0, the sum is exact
            assert (smap[2] == 1.0).all() and total[2] == START + want["count"][2]
        only_sum, none = gpu_value(dev, x, y, ranges, window(K, kind), want_map=False)          # map = NULL
        assert none is None and (np.abs((only_sum - START) - want["sum"]) <= tol_s).all()
    print(f"K {K}, {shape}: worst map error {worst_map:.3f} of its bound, worst sum error {worst_sum:.3f} of its bound; "
          f"the map {'EQUALS' if equal else 'does NOT equal'} the oracle rounded to f32")


def test_a_bad_range_gives_nan_for_that_image_only(dev):
    x, y, ranges = ref.stack(3, (12, 75))
    for bad in (0.0, -1.0, math.inf, math.nan):
        r = np.array([ranges[0], bad, ranges[2]])
        total, smap = gpu_value(dev, x, y, r, ref.gaussian(11), start=0.0)
        assert np.isnan(smap[1]).all() and np.isnan(total[1]) and np.isfinite(smap[[0, 2]]).all() and np.isfinite(total[[0, 2]]).all()
        g = gpu_gradient(dev, x, y, r, ref.gaussian(11), (1.0, 1.0, 1.0))
        assert np.isnan(g[1]).all() and np.isfinite(g[[0, 2]]).all()


# ----------------------------------------------------------------------------- 3. the gradient
@pytest.mark.parametrize("K,shape", ref.CASES)
def test_gradient_matches_the_f64_oracle(dev, K, shape):
    worst = 0.0
    for kind, n in configurations():
        x, y, ranges = ref.stack(n, shape)
        want = ref.oracle(K, shape, n, kind)
        for scale in SCALES:
            scale = np.array(scale[:n])
            got = gpu_gradient(dev, x, y, ranges, window(K, kind), scale)
            assert got.shape == x.shape and got.dtype == np.float32
            assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} pixels were not written"          # the buffer started as NaN
            want64 = scale[:, None, None] * want["grad"]
            tol = 2.0 ** -24 * np.abs(want64) + 2.0 ** -50 * np.abs(scale)[:, None, None] * want["mass"]
            err = np.abs(got.astype(np.float64) - want64)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nan_to_num(err / tol).max()))
            assert (err <= tol).all(), (kind, n, tuple(scale), float((err - tol).max()), np.unravel_index(np.argmax(err - tol), err.shape))
            for k in np.flatnonzero(scale == 0.0):          # the image with scale 0: all zeros, and finite
                assert not got[k].any()
            again = gpu_gradient(dev, x, y, ranges, window(K, kind), scale)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32))          # gathered: the same bits on every run
    print(f"K {K}, {shape}: worst gradient error {worst:.3f} of its bound")


# ----------------------------------------------------------------------------- 4. metrics.ssim under autograd
@functools.lru_cache(maxsize=None)
def views_and_phases(shape):
    """x, y f32 [2,3,H,W] and ranges [2,3]: the shared stack of three, and the same with prediction and truth exchanged."""
    x, y, ranges = ref.stack(3, shape)
    return np.stack([x, y]), np.stack([y, x]), np.stack([ranges, ranges[::-1]])


@pytest.mark.parametrize("K,shape", [(11, (27, 43)), (11, (43, 130)), (3, (5, 70))])
def test_metrics_ssim_under_autograd(dev, K, shape):
    from nerfca_amd import metrics
    x, y, ranges = views_and_phases(shape)
    win = metrics.gaussian_window(K)
    want = ref.ssim_stack(x.reshape((6,) + shape), y.reshape((6,) + shape), ranges.reshape(6), win)
    count = (shape[0] - K + 1) * (shape[1] - K + 1)
    tx = torch.from_numpy(x).to(dev).requires_grad_()
    ty = torch.from_numpy(y).to(dev).requires_grad_()
    tr = torch.from_numpy(ranges).to(dev)
    mean, smap = metrics.ssim(tx, ty, data_range=tr, win_size=K, full=True)
    assert mean.shape == (2, 3) and mean.dtype == torch.float64 and mean.device == tx.device and mean.requires_grad
    assert smap.shape == (2, 3, shape[0] - K + 1, shape[1] - K + 1) and smap.dtype == torch.float32 and not smap.requires_grad
    tol = (sum_bound(want) / count + 2 * U * np.abs(want["sum"]) / count).reshape(2, 3)
    assert (np.abs(mean.detach().cpu().numpy() - want["sum"].reshape(2, 3) / count) <= tol).all()
    assert (np.abs(smap.cpu().numpy().reshape(want["S"].shape).astype(np.float64) - want["S"]) <= map_bound(want["S"])).all()
    raw_total, raw_map = gpu_value(dev, x.reshape((6,) + shape), y.reshape((6,) + shape), ranges.reshape(6), win, start=0.0)
    assert np.array_equal(smap.cpu().numpy().reshape(raw_map.shape), raw_map)          # the raw call's bits
    assert (np.abs(mean.detach().cpu().numpy().reshape(6) - raw_total / count) <= tol.reshape(6)).all()
    upstream = torch.tensor([[1.0, -2.0, 0.5], [0.0, 3.0, -0.25]], dtype=torch.float64, device=dev)
    (mean * upstream).sum().backward()
    assert ty.grad is None          # truth gets no gradient
    assert tx.grad.shape == tx.shape and tx.grad.dtype == torch.float32
    scale = upstream.cpu().numpy().reshape(6) / count
    raw_grad = gpu_gradient(dev, x.reshape((6,) + shape), y.reshape((6,) + shape), ranges.reshape(6), win, scale)
    assert np.array_equal(tx.grad.cpu().numpy().reshape(raw_grad.shape).view(np.uint32), raw_grad.view(np.uint32))
    want64 = scale[:, None, None] * want["grad"]
    err = np.abs(raw_grad.astype(np.float64) - want64)
    assert (err <= 2.0 ** -24 * np.abs(want64) + 2.0 ** -50 * np.abs(scale)[:, None, None] * want["mass"]).all()
    assert not tx.grad[1, 0].any()          # upstream 0
    with torch.no_grad():
        quiet = metrics.ssim(tx, ty, data_range=tr, win_size=K)
    assert quiet.grad_fn is None and not quiet.requires_grad and quiet.shape == (2, 3)
    assert (np.abs(quiet.cpu().numpy() - mean.detach().cpu().numpy()) <= tol).all()          # the same value up to the order of the sum
    plain = metrics.ssim(tx.detach(), ty, data_range=2.16, win_size=K)          # a float range, nothing to record
    assert plain.grad_fn is None and plain.shape == (2, 3)
    one = metrics.ssim(tx.detach()[0, 1], ty.detach()[0, 1], data_range=float(ranges[0, 1]), win_size=K)          # one image: a 0-d result
    assert one.shape == () and abs(float(one) - want["sum"][1] / count) <= tol[0, 1]
    with pytest.raises(Exception):
        metrics.ssim(tx.detach().double(), ty.detach().double(), data_range=1.0, win_size=K)
    with pytest.raises(Exception):
        metrics.ssim(tx.detach()[..., :K - 1], ty.detach()[..., :K - 1], data_range=1.0, win_size=K)          # smaller than the window
    with pytest.raises(Exception):
        metrics.ssim(tx.detach(), ty.detach()[0], data_range=1.0, win_size=K)


# ----------------------------------------------------------------------------- 5. compare_sequences
N_DET, S, PHASES, SIDE = 16, 32, 4, 24          # the phantom case of tests/test_phantom_gpu.py


@functools.lru_cache(maxsize=None)
def phantom_sequence():
    from nerfca_amd import drr, phantom, synthetic
    dev = torch.device("cuda:0")
    geo = synthetic.xcat_geometry(N_DET)
    ph = phantom.make_phantom((SIDE,) * 3, PHASES, geo, device=dev)
    out = drr.project_sequence(ph["static"], ph["dynamic"], geo, synthetic.TRAIN_VIEWS, S, bounds=ph["bounds"])
    return geo, ph, out


def test_compare_sequences(dev):
    from nerfca_amd import metrics, synthetic
    geo, ph, out = phantom_sequence()
    same = metrics.compare_sequences(out, {k: v.clone() for k, v in out.items()})
    assert set(same) == {"pred", "pred_static", "pred_dynamic"}
    for key, r in same.items():
        lead = out[key].shape[:-2]
        assert set(r) == {"psnr", "ssim", "psnr_mean", "ssim_mean"} and r["psnr"].shape == r["ssim"].shape == lead and r["ssim"].dtype == torch.float64
        assert (r["ssim"] == 1.0).all() and torch.isinf(r["psnr"]).all() and (r["psnr"] > 0).all() and float(r["ssim_mean"]) == 1.0
    gen = torch.Generator(device=dev).manual_seed(5)
    other = {k: v + 0.05 * (torch.rand(v.shape, generator=gen, device=dev) - 0.5) for k, v in out.items()}
    diff = metrics.compare_sequences(other, out)
    win = metrics.gaussian_window(11)
    count = (N_DET - 10) ** 2
    for key, r in diff.items():
        a, b = other[key].cpu().numpy().reshape(-1, N_DET, N_DET), out[key].cpu().numpy().reshape(-1, N_DET, N_DET)
        ranges = b.max(axis=(1, 2)).astype(np.float64) - b.min(axis=(1, 2)).astype(np.float64)
        want = ref.ssim_stack(a, b, ranges, win)
        got = r["ssim"].cpu().numpy().reshape(-1)
        assert (got < 1.0).all() and torch.isfinite(r["psnr"]).all()
        assert (np.abs(got - want["sum"] / count) <= sum_bound(want) / count + 2 * U * np.abs(want["sum"]) / count).all(), key
        d = a.astype(np.float64) - b.astype(np.float64)
        want_psnr = 10 * np.log10(ranges * ranges / (d * d).mean(axis=(1, 2)))
        assert np.abs(r["psnr"].cpu().numpy().reshape(-1) - want_psnr).max() <= 1e-10 * np.abs(want_psnr).max()
        assert abs(float(r["ssim_mean"]) - got.mean()) <= 1e-14 and abs(float(r["psnr_mean"]) - float(r["psnr"].mean())) <= 1e-12
    fixed = metrics.compare_sequences(other, out, data_range=2.0)
    assert float(fixed["pred"]["psnr_mean"]) != float(diff["pred"]["psnr_mean"])


# ----------------------------------------------------------------------------- 6. fit_volumes
@functools.lru_cache(maxsize=None)
def fit_frames():
    from nerfca_amd import synthetic
    geo, ph, out = phantom_sequence()
    frames = [(float(v[0]), float(v[1]), p, out["pred"][i, p].contiguous()) for i, v in enumerate(synthetic.TRAIN_VIEWS) for p in range(PHASES)]
    return geo, ph["bounds"], frames


def test_fit_volumes_with_weight_zero_is_todays(dev):
    """The adjoint kernel sums in f64 atomics whose order is free, so two runs of one fit agree in every bit only as far as those sums round
    to the same f32: the first losses (forward only, gathered) are compared exactly, the volumes after 2 steps bit for bit as the issue of
    this feature asks (a difference there would need an f64 sum to straddle an f32 rounding boundary: about 1e-4 per run)."""
    from nerfca_amd import drr
    geo, bounds, frames = fit_frames()
    kw = dict(bounds=bounds, n_phases=PHASES, steps=2, lr=1e-2)
    plain = drr.fit_volumes(frames, geo, (SIDE,) * 3, S, **kw)
    zero = drr.fit_volumes(frames, geo, (SIDE,) * 3, S, ssim_weight=0.0, ssim_win=11, **kw)
    assert set(plain) == set(zero) == {"static", "dynamic", "loss"}
    assert plain["loss"][0] == zero["loss"][0]
    assert torch.equal(plain["static"], zero["static"]) and torch.equal(plain["dynamic"], zero["dynamic"]) and plain["loss"] == zero["loss"]


def test_fit_volumes_with_the_structural_term(dev):
    from nerfca_amd import drr
    geo, bounds, frames = fit_frames()
    w = 0.1
    out = drr.fit_volumes(frames, geo, (SIDE,) * 3, S, bounds=bounds, n_phases=PHASES, steps=20, lr=1e-2, ssim_weight=w, ssim_win=11)
    assert set(out) == {"static", "dynamic", "loss", "ssim"}
    assert len(out["ssim"]) == len(out["loss"]) == 20 and all(isinstance(v, float) and math.isfinite(v) and -1.0 <= v <= 1.0 for v in out["ssim"])
    objective = [out["loss"][k] + w * (1.0 - out["ssim"][k]) for k in (0, -1)]
    print(f"fit_volumes with ssim_weight {w}, 20 steps: ssim {out['ssim'][0]:.4f} -> {out['ssim'][-1]:.4f}, objective {objective[0]:.4e} -> {objective[1]:.4e}")
    assert out["ssim"][-1] > out["ssim"][0] and objective[1] < objective[0]
    whole = [out["loss"][k] + w * (1.0 - out["ssim"][k]) for k in range(20)]
    assert sum(out["ssim"][-5:]) > sum(out["ssim"][:5]) and sum(whole[-5:]) < sum(whole[:5])          # over the run, not only its two ends
    assert max(out["ssim"][-5:]) >= max(out["ssim"]) - 0.05 and min(whole[-5:]) <= min(whole) + 0.05 * whole[0]          # and it ends near its best
    flat = [(t, p, ph, torch.full_like(img, 2.0)) if k == 3 else (t, p, ph, img) for k, (t, p, ph, img) in enumerate(frames)]
    with pytest.raises(Exception, match="1 of the 16 frames are constant"):
        drr.fit_volumes(flat, geo, (SIDE,) * 3, S, bounds=bounds, n_phases=PHASES, steps=1, ssim_weight=w)
    assert set(drr.fit_volumes(flat, geo, (SIDE,) * 3, S, bounds=bounds, n_phases=PHASES, steps=1)) == {"static", "dynamic", "loss"}          # weight 0: as before
    small = drr.fit_volumes(frames, geo, (SIDE,) * 3, S, bounds=bounds, n_phases=PHASES, steps=1, ssim_weight=w, ssim_win=3, tv_space=1e-3)
    assert set(small) == {"static", "dynamic", "loss", "tv_space", "tv_time", "ssim"}
    assert small["loss"][0] == out["loss"][0] and small["ssim"][0] != out["ssim"][0]          # the data term is untouched; another window, another SSIM
