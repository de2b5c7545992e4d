"""Total-variation priors on the GPU: nca_vol_tv and nca_vol_tv_grad against the f64 numpy transcription of their definition
(tests/voltv_ref.py, pinned to torch autograd in tests/test_voltv_cpu.py), the autograd path of drr.total_variation, and drr.fit_volumes
with the priors on.  The kernels fix every operation: the two values are free only in the order of their sums (a sum of `count` terms of
total size `sum |term|` lies within count 2^-53 sum |term| of the exact sum, so two such sums are within twice that of each other); the
gradient is gathered and rounded to f32 once."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev  # noqa: F401

import drr_adjoint_ref as adj
import drr_ref
import voltv_ref as ref

pytestmark = pytest.mark.gpu

BOUNDS = drr_ref.BOUNDS
U = ref.U
SCALES = ((1.0, 0.0), (0.0, 1.0), (0.5, -2.0))
START = (0.5, -0.25)          # what `out` holds before a call: far below the sums it is added into (or added to exact zeros)
CASES = [(n_vol, cyclic) for n_vol in ref.N_VOLS for cyclic in (False, True)]


@functools.lru_cache(maxsize=None)
def volumes(shape, n_vol):
    return ref.stack(n_vol, shape, seed=sum(shape) + n_vol)


@functools.lru_cache(maxsize=None)
def oracle(shape, n_vol, cyclic, eps_s=ref.EPS_S, eps_t=ref.EPS_T):
    return ref.total_variation(volumes(shape, n_vol), ref.grid_inv(shape, BOUNDS), eps_s, eps_t, cyclic)


def value_bounds(want):
    return 2 * want["count_space"] * U * want["abs_space"], 2 * want["count_time"] * U * want["abs_time"]


def gpu_values(dev, x, cyclic, start=(0.0, 0.0)):
    """out f64 [2] after one nca_vol_tv into a pair that starts as `start`."""
    from nerfca_amd import _capi, drr, fused
    tx = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = torch.tensor(start, dtype=torch.float64, device=dev)
    desc = drr.grid_desc(x.shape[-3:], BOUNDS)
    with torch.cuda.device(dev):
        _capi.check_vol(_capi.lib().nca_vol_tv(C.byref(desc), _capi.ptr(tx), x.shape[0], ref.EPS_S, ref.EPS_T, int(cyclic), _capi.ptr(out), fused._stream()))
    return out.cpu().numpy()


def gpu_gradient(dev, x, cyclic, scale):
    """g_vol f32 [n_vol,n0,n1,n2] of one nca_vol_tv_grad into a buffer pre-filled with NaN."""
    from nerfca_amd import _capi, drr, fused
    tx = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ts = torch.tensor(scale, dtype=torch.float64, device=dev)
    g = torch.full(x.shape, math.nan, dtype=torch.float32, device=dev)
    desc = drr.grid_desc(x.shape[-3:], BOUNDS)
    with torch.cuda.device(dev):
        _capi.check_vol(_capi.lib().nca_vol_tv_grad(C.byref(desc), _capi.ptr(tx), x.shape[0], ref.EPS_S, ref.EPS_T, int(cyclic), _capi.ptr(ts), _capi.ptr(g),
                                                    fused._stream()))
    return g.cpu().numpy()


def gradient_bound(want64, mass, s0, s1):
    """One rounding to f32 of the oracle's value, plus slack for a library sqrt or division that is not the host's last bit."""
    return 2.0 ** -24 * np.abs(want64) + 2.0 ** -50 * (abs(s0) * mass + 2 * abs(s1))


# ----------------------------------------------------------------------------- 1. the two values
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_values_match_the_f64_oracle_and_are_added_into_out(dev, shape):
    worst = 0.0
    for n_vol, cyclic in CASES:
        want = oracle(shape, n_vol, cyclic)
        got = gpu_values(dev, volumes(shape, n_vol), cyclic, START) - np.array(START)
        for k, (name, tol) in enumerate(zip(("space", "time"), value_bounds(want))):
            err = abs(got[k] - want[name])
            print(f"grid {shape}, n_vol {n_vol}, cyclic {cyclic}, {name}: gpu {got[k]!r} oracle {want[name]!r} error {err:.3e} bound {tol:.3e}")
            assert err <= tol, (n_vol, cyclic, name, err, tol)
            if tol:
                worst = max(worst, err / tol)
                assert abs(START[k]) <= 0.5 * want["abs_" + name]          # what makes the bound hold for a sum that starts at START
        if n_vol == 1:
            assert got[1] == 0.0          # no pair: nothing is added
    print(f"grid {shape}: worst value error {worst:.3f} of 2 count 2^-53 sum |term|")


def test_a_constant_stack_gives_exactly_zero(dev):
    for shape in ((5, 3, 4), (33, 18, 67)):
        for n_vol in (1, 3):
            x = np.full((n_vol,) + shape, np.float32(0.7))
            assert np.array_equal(gpu_values(dev, x, True), [0.0, 0.0])
            g = gpu_gradient(dev, x, True, (0.5, -2.0))
            assert g.shape == x.shape and not g.any() and np.isfinite(g).all()


# ----------------------------------------------------------------------------- 2. the gradient
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_gradient_matches_the_f64_oracle(dev, shape):
    worst = 0.0
    for n_vol, cyclic in CASES:
        want = oracle(shape, n_vol, cyclic)
        x = volumes(shape, n_vol)
        flat = want["mass"][0, 0, 0, 0] == 0.0          # the flat row of volume 0: m == eps_s, every quotient 0
        assert flat
        for s0, s1 in SCALES:
            got = gpu_gradient(dev, x, cyclic, (s0, s1))
            assert got.shape == x.shape and got.dtype == np.float32
            assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} nodes were not written"          # the buffer started as NaN
            want64 = s0 * want["g_s"] + s1 * want["g_t"]
            tol = gradient_bound(want64, want["mass"], s0, s1)
            err = np.abs(got.astype(np.float64) - want64)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nan_to_num(err / tol).max()))
            assert (err <= tol).all(), (n_vol, cyclic, (s0, s1), float((err - tol).max()), np.unravel_index(np.argmax(err - tol), err.shape))
            again = gpu_gradient(dev, x, cyclic, (s0, s1))
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32))          # gathered: the same bits on every run
    print(f"grid {shape}: worst gradient error {worst:.3f} of its bound")


# ----------------------------------------------------------------------------- 3. autograd
@pytest.mark.parametrize("shape", [(17, 9, 33), (33, 18, 67)])
def test_autograd_gradient(dev, shape):
    from nerfca_amd import drr
    a, b = 0.7, -1.3
    voxels = shape[0] * shape[1] * shape[2]
    for n_vol, cyclic in CASES:
        want = oracle(shape, n_vol, cyclic)
        x = torch.from_numpy(volumes(shape, n_vol)).to(dev)
        x = (x[0].contiguous() if n_vol == 1 else x).requires_grad_()          # one volume goes in as [n0,n1,n2]
        tv_s, tv_t = drr.total_variation(x, bounds=BOUNDS, eps_space=ref.EPS_S, eps_time=ref.EPS_T, cyclic=cyclic)
        for t in (tv_s, tv_t):
            assert t.dtype == torch.float64 and t.dim() == 0 and t.device == x.device and t.requires_grad
        n_s, n_t = n_vol * voxels, want["n_pairs"] * voxels
        tol_s, tol_t = value_bounds(want)
        assert abs(tv_s.item() - want["space"] / n_s) <= tol_s / n_s + 2 * U * want["space"] / n_s
        if n_t:
            assert abs(tv_t.item() - want["time"] / n_t) <= tol_t / n_t + 2 * U * want["time"] / n_t
        else:
            assert tv_t.item() == 0.0
        (a * tv_s + b * tv_t).backward()
        assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape and x.grad.device == x.device
        s0, s1 = a / n_s, (b / n_t if n_t else 0.0)
        want64 = s0 * want["g_s"] + s1 * want["g_t"]
        err = np.abs(x.grad.cpu().numpy().reshape(want64.shape).astype(np.float64) - want64)
        assert (err <= gradient_bound(want64, want["mass"], s0, s1)).all(), (n_vol, cyclic, float(err.max()))


def test_without_a_gradient_nothing_is_recorded(dev):
    from nerfca_amd import drr
    x = torch.from_numpy(volumes((5, 3, 4), 3)).to(dev)
    for t in drr.total_variation(x, bounds=BOUNDS):
        assert t.grad_fn is None and not t.requires_grad and t.dtype == torch.float64 and t.dim() == 0
    x.requires_grad_()
    with torch.no_grad():
        quiet = drr.total_variation(x, bounds=BOUNDS)
    assert all(t.grad_fn is None and not t.requires_grad for t in quiet)
    loud = drr.total_variation(x, bounds=BOUNDS)
    assert all(t.grad_fn is not None for t in loud)
    with pytest.raises(Exception):
        drr.total_variation(x.detach().double(), bounds=BOUNDS)
    with pytest.raises(Exception):
        drr.total_variation(x.detach()[:, :, :, ::2], bounds=BOUNDS)
    with pytest.raises(Exception):
        drr.total_variation(x.detach(), bounds=BOUNDS, eps_space=0.0)


# ----------------------------------------------------------------------------- 4. fit_volumes
FIT_VIEWS = drr_ref.VIEWS + [(60.0, -30.0), (-30.0, 30.0)]
FIT_SHAPE = (9, 9, 9)


@functools.lru_cache(maxsize=None)
def fit_problem():
    """(geo, S, truth_static, truth_dynamic, frames) on cuda:0, the problem of tests/test_drr_grad_gpu.py: 4 views x 2 phases of a known
    non-negative pair on a 9^3 grid, projected with project_rays and composed as volume_teacher composes."""
    from nerfca_amd import drr, export
    dev = torch.device("cuda:0")
    _, geo, S = drr_ref.geometries()[0]
    W, H = geo["nDetector"]
    vs = torch.from_numpy(np.abs(drr_ref.random_volume(FIT_SHAPE, seed=31))).to(dev)
    vd = torch.from_numpy(np.abs(drr_ref.random_volume((2,) + FIT_SHAPE, seed=32))).to(dev)
    z = torch.from_numpy(drr_ref.depths(geo, S)[0]).to(dev)
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    frames = []
    for theta, phi in FIT_VIEWS:
        o, d = export.view_rays(geo, theta, phi, device=dev)
        pix_s = drr.project_rays(vs, o, d, z, i0=i0, bounds=BOUNDS)
        pix_d = drr.project_rays(vd, o, d, z, i0=i0, bounds=BOUNDS)
        for phase in range(2):
            frames.append((theta, phi, phase, ((pix_s + pix_d[phase]) - i0).to(torch.float32).reshape(W, H)))
    return geo, S, vs, vd, frames


def data_gradient_bound(geo, S, frames):
    """An upper bound of |d mse / d node| at the truth, from the adjoint oracle on the CPU.  There the residual of a pixel is only the
    rounding of its target to f32, at most 2^-24 max |image|; a node's gradient is 2 / (frames x pixels) times the residuals back-projected,
    at most that residual times the node's mass for unit pixel gradients (tests/drr_adjoint_ref.py), summed over the views and, for the
    static volume, over both phases."""
    z, dists = drr_ref.depths(geo, S)
    mass = np.zeros(FIT_SHAPE)
    for theta, phi in FIT_VIEWS:
        o, d = drr_ref.host_rays(geo, theta, phi)
        mass += adj.backproject(FIT_SHAPE, 1, o, d, z, dists, np.ones(o.shape[0]), BOUNDS)[1][0]
    residual = 2.0 ** -24 * max(float(f[3].abs().max()) for f in frames)
    return 2.0 / (len(frames) * 64) * residual * 2 * float(mass.max())


def test_fit_volumes_first_adam_step_follows_the_prior(dev):
    """From the truth, the data term's gradient is f32 rounding only: data_gradient_bound gives at most 1.33e-8 per node (worked out on the
    CPU: the largest pixel is 2.28, the largest unit mass of a node over the 4 views 12.5; printed below), against a total-variation
    gradient G between 6e-6 and 3e-2 whose smallest value above 1e-3 max |G| is 4.3e-5.  Adam's first step -lr g / (|g| + 1e-8) with
    g = G + data is therefore -lr sign(G) to (1.33e-8 + 1e-8) / 4.3e-5 = 5e-4 of lr on those nodes, which are 100 % of the static volume
    and 99.93 % of the dynamic stack."""
    from nerfca_amd import drr
    geo, S, vs, vd, frames = fit_problem()
    lr, eps = 1e-3, 1e-3
    out = drr.fit_volumes(frames, geo, FIT_SHAPE, S, bounds=BOUNDS, n_phases=2, steps=1, lr=lr, init=(vs, vd), nonneg=False, tv_space=1.0, tv_time=1.0,
                          tv_eps=eps)
    assert set(out) == {"static", "dynamic", "loss", "tv_space", "tv_time"}
    bound = data_gradient_bound(geo, S, frames)
    print(f"data-gradient bound at the truth: {bound:.3e} per node")
    assert bound <= 1.4e-8
    inv = ref.grid_inv(FIT_SHAPE, BOUNDS)
    voxels = 9 ** 3
    ws = ref.total_variation(vs.cpu().numpy()[None], inv, eps, eps, True)
    wd = ref.total_variation(vd.cpu().numpy(), inv, eps, eps, True)
    assert wd["n_pairs"] == 2
    G = {"static": ws["g_s"][0] / voxels, "dynamic": wd["g_s"] / (2 * voxels) + wd["g_t"] / (2 * voxels)}
    for name, before in (("static", vs), ("dynamic", vd)):
        g = G[name]
        step = (out[name] - before).cpu().numpy().astype(np.float64)
        big = np.abs(g) > 1e-3 * np.abs(g).max()
        print(f"{name}: |G| in [{np.abs(g).min():.2e}, {np.abs(g).max():.2e}], {100 * big.mean():.2f} % of the nodes above 1e-3 of the largest")
        assert big.mean() >= 0.99 and np.abs(g[big]).min() > 200 * (bound + 1e-8)          # the step is sign(G) lr to 0.5 %
        assert (np.sign(step[big]) == -np.sign(g[big])).all()
        size = np.abs(step[big])
        assert (size >= 0.99 * lr).all() and (size <= 1.01 * lr).all(), (float(size.min()), float(size.max()))
    tol_s = value_bounds(ws)[0] / voxels + value_bounds(wd)[0] / (2 * voxels)
    want_s = ws["space"] / voxels + wd["space"] / (2 * voxels)
    want_t = wd["time"] / (2 * voxels)
    assert len(out["tv_space"]) == len(out["tv_time"]) == len(out["loss"]) == 1
    assert abs(out["tv_space"][0] - want_s) <= tol_s + 4 * U * want_s
    assert abs(out["tv_time"][0] - want_t) <= value_bounds(wd)[1] / (2 * voxels) + 4 * U * want_t
    biggest = max(float(f[3].abs().max()) for f in frames)
    assert 0.0 <= out["loss"][0] <= (2.0 ** -24 * biggest) ** 2          # "loss" stays the data term


def test_fit_volumes_from_zeros_descends_on_the_whole_objective(dev):
    from nerfca_amd import drr
    geo, S, vs, vd, frames = fit_problem()
    w = 1e-3
    out = drr.fit_volumes(frames, geo, FIT_SHAPE, S, bounds=BOUNDS, n_phases=2, steps=30, tv_space=w, tv_time=w)
    assert set(out) == {"static", "dynamic", "loss", "tv_space", "tv_time"}
    for k in ("loss", "tv_space", "tv_time"):
        assert isinstance(out[k], list) and len(out[k]) == 30 and all(isinstance(v, float) and math.isfinite(v) for v in out[k])
    objective = [out["loss"][k] + w * (out["tv_space"][k] + out["tv_time"][k]) for k in (0, -1)]
    print(f"fit_volumes with priors, 30 steps: objective {objective[0]:.4e} -> {objective[1]:.4e} (tv_space {out['tv_space'][-1]:.3e}, tv_time {out['tv_time'][-1]:.3e})")
    assert out["tv_space"][0] == 0.0 and out["tv_time"][0] == 0.0          # zeros are flat
    assert objective[1] < objective[0] and out["tv_space"][-1] > 0
    plain = drr.fit_volumes(frames, geo, FIT_SHAPE, S, bounds=BOUNDS, n_phases=2, steps=1)
    assert set(plain) == {"static", "dynamic", "loss"}
