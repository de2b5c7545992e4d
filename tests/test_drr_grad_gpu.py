"""Back-projection on the GPU: nca_drr_backproject against the f64 numpy transcription of its definition (tests/drr_adjoint_ref.py, pinned
to autograd through grid_sample in tests/test_drr_grad_cpu.py), the autograd path of drr.project_rays, and drr.fit_volumes.  The
kernel-level tests run with both structures the library keeps (nca_drr_set_backproject_runs): one atomic per contribution, and runs of
samples in one cell summed in registers first.  The kernel fixes everything but the order of a node's sum, so a node that receives
`count` contributions of total magnitude `mass` may differ from the oracle by count 2^-53 mass (measured on an MI355X, both structures:
at most 0.93 of that bound, at 17 x 9 x 33 in the small box; the adjoint identity holds to 2 % of its bound)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev  # noqa: F401

import drr_adjoint_ref as adj
import drr_ref as ref

pytestmark = pytest.mark.gpu

I0 = float(np.float32(math.log(8.670397)))
U = 2.0 ** -53
FAR_BOX = ((5.0, 5.5),) * 3          # no ray of any case enters it
N_VOLS = (1, 3, 11)                  # groups 1, 2 + 1 and 8 + 2 + 1


@pytest.fixture(params=[0, 1], ids=["direct", "runs"])
def runs(request):
    from nerfca_amd import _capi
    lib = _capi.lib()
    before = lib.nca_drr_get_backproject_runs()
    _capi.check_drr(lib.nca_drr_set_backproject_runs(request.param))
    yield request.param
    _capi.check_drr(lib.nca_drr_set_backproject_runs(before))


@functools.lru_cache(maxsize=None)
def ray_cases():
    """[(name, o, d, z, dists)] as numpy: the rays export.view_rays generates on the device for both detectors (64 and 240 rays: neither
    fills a 256-thread block, 240 leaves a ragged tail) and both views."""
    from nerfca_amd import export
    out = []
    for name, geo, S in ref.geometries():
        z, dists = ref.depths(geo, S)
        for theta, phi in ref.VIEWS:
            o, d = export.view_rays(geo, theta, phi, device="cuda:0")
            out.append((f"{name}@{theta},{phi}", o.cpu().numpy(), d.cpu().numpy(), z, dists))
    return out


@functools.lru_cache(maxsize=None)
def pixel_gradient(case):
    """g_pix f64 [11,R] of one ray case; a call with fewer volumes takes its first rows."""
    return np.random.default_rng(100 + case).standard_normal((max(N_VOLS), ray_cases()[case][1].shape[0]))


@functools.lru_cache(maxsize=None)
def oracle(shape, bounds, case):
    """(g_vol [11,voxels], mass [11,voxels], count [voxels]) of the oracle for one grid, box and ray case; computed once.  A volume's
    numbers do not depend on the others, so a call with fewer volumes is held to the first rows."""
    _, o, d, z, dists = ray_cases()[case]
    nv = max(N_VOLS)
    g_vol, mass, count = adj.backproject(shape, nv, o, d, z, dists, pixel_gradient(case), bounds)
    return g_vol.reshape(nv, -1), mass.reshape(nv, -1), count.reshape(-1)


def gpu_backproject(dev, shape, case, bounds, g_pix, init=None):
    """g_vol f64 [n_vol,voxels] after one nca_drr_backproject into a buffer that starts as `init` (zeros when None)."""
    from nerfca_amd import _capi, drr, fused
    _, o, d, z, dists = ray_cases()[case]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g_pix = np.asarray(g_pix, dtype=np.float64).reshape(-1, o.shape[0])
    n_vol, voxels = g_pix.shape[0], shape[0] * shape[1] * shape[2]
    buf = torch.zeros((n_vol, voxels), dtype=torch.float64, device=dev) if init is None else t(init).clone()
    assert buf.shape == (n_vol, voxels) and buf.dtype == torch.float64
    to, td, tz, tdists, tg = t(o), t(d), t(z), t(dists), t(g_pix)
    desc = drr.grid_desc(shape, bounds)
    with torch.cuda.device(dev):
        _capi.check_drr(_capi.lib().nca_drr_backproject(C.byref(desc), n_vol, o.shape[0], z.shape[0], _capi.ptr(to), _capi.ptr(td), _capi.ptr(tz),
                                                        _capi.ptr(tdists), _capi.ptr(tg), _capi.ptr(buf), fused._stream()))
    return buf.cpu().numpy()


def gpu_project(dev, vols, case, bounds, i0):
    """pix f64 of a direct nca_drr_project call (not through drr.project_rays)."""
    from nerfca_amd import _capi, drr, fused
    _, o, d, z, dists = ray_cases()[case]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tv, to, td, tz, tdists = t(vols), t(o), t(d), t(z), t(dists)
    n_vol = 1 if vols.ndim == 3 else vols.shape[0]
    pix = torch.empty((n_vol, o.shape[0]), dtype=torch.float64, device=dev)
    desc = drr.grid_desc(vols.shape[-3:], bounds)
    with torch.cuda.device(dev):
        _capi.check_drr(_capi.lib().nca_drr_project(C.byref(desc), _capi.ptr(tv), n_vol, o.shape[0], z.shape[0], _capi.ptr(to), _capi.ptr(td), _capi.ptr(tz),
                                                    _capi.ptr(tdists), float(i0), _capi.ptr(pix), fused._stream()))
    return pix.cpu().numpy()


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_backprojection_matches_the_f64_oracle(dev, runs, shape):
    for bounds, box in ((ref.BOUNDS, "box"), (ref.SMALL_BOX, "small box")):
        worst, hit = 0.0, 0
        for case in range(len(ray_cases())):
            want, mass, count = oracle(shape, bounds, case)
            for n_vol in N_VOLS:
                got = gpu_backproject(dev, shape, case, bounds, pixel_gradient(case)[:n_vol])
                assert got.shape == (n_vol, count.size) and np.isfinite(got).all()
                err = np.abs(got - want[:n_vol])
                tol = count[None] * U * mass[:n_vol]
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nan_to_num(err / tol).max()))
                assert (err <= tol).all(), (ray_cases()[case][0], n_vol, float((err - tol).max()))
                assert (got[:, count == 0] == 0.0).all()          # a node nothing reaches keeps the buffer's value exactly
            hit += int((count > 0).sum())
        print(f"grid {shape}, {box}, runs = {runs}: nodes reached {hit}, worst error {worst:.3f} of count 2^-53 mass")
        assert hit > 0


# ----------------------------------------------------------------------------- 2. added into
def test_contributions_are_added_into_the_buffer(dev, runs):
    shape, case, n_vol = (17, 9, 33), 3, 3
    for bounds in (ref.BOUNDS, ref.SMALL_BOX):
        want, mass, count = oracle(shape, bounds, case)
        pattern = np.random.default_rng(5).uniform(0.5, 2.0, (n_vol, count.size)) * np.where(np.arange(count.size) % 2, -1.0, 1.0)[None]
        got = gpu_backproject(dev, shape, case, bounds, pixel_gradient(case)[:n_vol], init=pattern)
        err = np.abs(got - (pattern + want[:n_vol]))
        assert (err <= (count[None] + 1) * U * (mass[:n_vol] + np.abs(pattern))).all(), float(err.max())
        assert (count == 0).any() and np.array_equal(got[:, count == 0], pattern[:, count == 0])
        assert not np.array_equal(got[:, count > 0], pattern[:, count > 0])


def test_rays_that_miss_the_grid_change_nothing(dev, runs):
    for shape in ref.GRIDS:
        voxels = shape[0] * shape[1] * shape[2]
        pattern = np.random.default_rng(6).standard_normal((3, voxels))
        for case in range(len(ray_cases())):
            got = gpu_backproject(dev, shape, case, FAR_BOX, pixel_gradient(case)[:3], init=pattern)
            assert np.array_equal(got, pattern), (shape, case)          # bit for bit


# ----------------------------------------------------------------------------- 3. adjoint of the library's own forward
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_adjoint_identity_with_the_library_forward(dev, runs, shape):
    """sum((i0 - nca_drr_project(x)) y) = -sum(x nca_drr_backproject(y)) within 2^-50 sum(|x| mass), the CPU test's bound; i0 = 0, so
    that i0 - pix is the ray sum exactly."""
    x = ref.random_volume((3,) + shape, seed=12)
    for bounds in (ref.BOUNDS, ref.SMALL_BOX):
        for case in range(len(ray_cases())):
            y = pixel_gradient(case)[:3]
            _, mass, _ = oracle(shape, bounds, case)
            pix = gpu_project(dev, x, case, bounds, 0.0)
            g_vol = gpu_backproject(dev, shape, case, bounds, y)
            lhs = float(((0.0 - pix) * y).sum())
            rhs = -float((x.reshape(3, -1).astype(np.float64) * g_vol).sum())
            scale = float((np.abs(x.reshape(3, -1)).astype(np.float64) * mass[:3]).sum())
            print(f"grid {shape} {ray_cases()[case][0]}: |lhs - rhs| = {abs(lhs - rhs):.2e}, bound {2.0 ** -50 * scale:.2e}")
            assert abs(lhs - rhs) <= 2.0 ** -50 * scale


# ----------------------------------------------------------------------------- 4. grouping
def test_groups_do_not_interact(dev, runs):
    shape = (17, 9, 33)
    for case in (1, 3):
        for bounds in (ref.BOUNDS, ref.SMALL_BOX):
            _, mass, count = oracle(shape, bounds, case)
            y = pixel_gradient(case)
            together = gpu_backproject(dev, shape, case, bounds, y)
            assert together.shape == (11, count.size)
            for v in range(11):
                alone = gpu_backproject(dev, shape, case, bounds, y[v])
                # two sums of the same terms in two orders: each within count 2^-53 mass of the exact sum
                assert (np.abs(alone[0] - together[v]) <= 2 * count * U * mass[v]).all(), v


# ----------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("n_vol", [None, 3], ids=["one volume", "three volumes"])
def test_autograd_gradient(dev, n_vol):
    from nerfca_amd import drr
    shape, bounds = (17, 9, 33), ref.BOUNDS
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for case in (0, 3):
        _, o, d, z, dists = ray_cases()[case]
        want, mass, count = oracle(shape, bounds, case)
        k = 1 if n_vol is None else n_vol
        vols = ref.random_volume(shape if n_vol is None else (n_vol,) + shape, seed=21)
        y = pixel_gradient(case)[:k]
        vol = t(vols).requires_grad_()
        pix = drr.project_rays(vol, t(o), t(d), t(z), t(dists), i0=I0, bounds=bounds)
        assert pix.requires_grad and pix.dtype == torch.float64 and pix.shape == ((o.shape[0],) if n_vol is None else (n_vol, o.shape[0]))
        assert np.array_equal(pix.detach().cpu().numpy(), gpu_project(dev, vols, case, bounds, I0).reshape(pix.shape))          # the forward is the plain launch
        (pix * t(y).reshape(pix.shape)).sum().backward()
        assert vol.grad.dtype == torch.float32 and vol.grad.shape == vol.shape and vol.grad.device == vol.device
        got = vol.grad.cpu().numpy().reshape(k, -1)
        tol = count[None] * U * mass[:k] + 0.5 * np.spacing(np.abs(got)).astype(np.float64)          # the oracle's bound + half an f32 ulp
        err = np.abs(got.astype(np.float64) - want[:k])
        assert (err <= tol).all(), float((err - tol).max())
        assert (got[:, count == 0] == 0).all() and (got != 0).any()


def test_without_a_gradient_nothing_is_recorded(dev):
    from nerfca_amd import drr
    shape, bounds, case = (5, 3, 4), ref.BOUNDS, 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _, o, d, z, dists = ray_cases()[case]
    vols = ref.random_volume((3,) + shape, seed=22)
    want = gpu_project(dev, vols, case, bounds, I0)
    plain = drr.project_rays(t(vols), t(o), t(d), t(z), t(dists), i0=I0, bounds=bounds)
    assert plain.grad_fn is None and not plain.requires_grad and np.array_equal(plain.cpu().numpy(), want)
    vol = t(vols).requires_grad_()
    with torch.no_grad():
        quiet = drr.project_rays(vol, t(o), t(d), t(z), t(dists), i0=I0, bounds=bounds)
    assert quiet.grad_fn is None and not quiet.requires_grad and np.array_equal(quiet.cpu().numpy(), want)
    # rays that require a gradient do not switch the path on, and get none
    rays = t(o).requires_grad_()
    still = drr.project_rays(t(vols), rays, t(d), t(z), t(dists), i0=I0, bounds=bounds)
    assert still.grad_fn is None and np.array_equal(still.cpu().numpy(), want)
    pix = drr.project_rays(vol, rays, t(d), t(z), t(dists), i0=I0, bounds=bounds)
    pix.sum().backward()
    assert rays.grad is None and vol.grad is not None
    # the dataset hook records nothing either
    hook = drr.volume_teacher(bounds)
    R = o.shape[0]
    out = hook(vol[0], vol, t(o), t(d), torch.zeros(R, dtype=torch.int32, device=dev), torch.full((R,), I0, dtype=torch.float32, device=dev), t(z), t(dists))
    assert out.grad_fn is None


# ----------------------------------------------------------------------------- 6. fit_volumes
FIT_VIEWS = ref.VIEWS + [(60.0, -30.0), (-30.0, 30.0)]


@functools.lru_cache(maxsize=None)
def fit_problem():
    """(geo, S, truth_static, truth_dynamic, frames) on cuda:0: 4 views x 2 phases of a known non-negative pair on a 9^3 grid, projected with
    project_rays and composed as volume_teacher composes."""
    from nerfca_amd import drr, export
    dev = torch.device("cuda:0")
    _, geo, S = ref.geometries()[0]
    W, H = geo["nDetector"]
    vs = torch.from_numpy(np.abs(ref.random_volume((9, 9, 9), seed=31))).to(dev)
    vd = torch.from_numpy(np.abs(ref.random_volume((2, 9, 9, 9), seed=32))).to(dev)
    z = torch.from_numpy(ref.depths(geo, S)[0]).to(dev)
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    frames = []
    for theta, phi in FIT_VIEWS:
        o, d = export.view_rays(geo, theta, phi, device=dev)
        pix_s = drr.project_rays(vs, o, d, z, i0=i0, bounds=ref.BOUNDS)
        pix_d = drr.project_rays(vd, o, d, z, i0=i0, bounds=ref.BOUNDS)
        for phase in range(2):
            frames.append((theta, phi, phase, ((pix_s + pix_d[phase]) - i0).to(torch.float32).reshape(W, H)))
    return geo, S, vs, vd, frames


def test_fit_volumes_descends(dev):
    from nerfca_amd import drr
    geo, S, vs, vd, frames = fit_problem()
    out = drr.fit_volumes(frames, geo, (9, 9, 9), S, bounds=ref.BOUNDS, n_phases=2, steps=30)
    assert set(out) == {"static", "dynamic", "loss"}
    loss = out["loss"]
    assert isinstance(loss, list) and len(loss) == 30 and all(isinstance(v, float) and math.isfinite(v) for v in loss)
    print(f"fit_volumes, 8 frames of 8 x 8, 30 steps: loss {loss[0]:.4e} -> {loss[-1]:.4e}")
    assert loss[-1] < loss[0]
    assert out["static"].shape == (9, 9, 9) and out["dynamic"].shape == (2, 9, 9, 9)
    for k in ("static", "dynamic"):
        assert out[k].dtype == torch.float32 and out[k].device == vs.device and not out[k].requires_grad and (out[k] >= 0).all()
    assert (out["static"] > 0).any() and (out["dynamic"] > 0).any()
    # chunked, the same descent (the sums are formed in another order: close, not equal)
    chunked = drr.fit_volumes(frames, geo, (9, 9, 9), S, bounds=ref.BOUNDS, n_phases=2, steps=3, chunk_rays=24)
    assert np.allclose(chunked["loss"], loss[:3], rtol=1e-6)


def test_fit_volumes_from_the_truth_starts_at_zero(dev):
    from nerfca_amd import drr
    geo, S, vs, vd, frames = fit_problem()
    out = drr.fit_volumes(frames, geo, (9, 9, 9), S, bounds=ref.BOUNDS, n_phases=2, steps=1, init=(vs, vd))
    biggest = max(float(f[3].abs().max()) for f in frames)
    assert 0.0 <= out["loss"][0] <= (2.0 ** -24 * biggest) ** 2          # only the f32 rounding of the images is left


def test_fit_volumes_refusals(dev):
    from nerfca_amd import _capi, drr
    geo, S, vs, vd, frames = fit_problem()
    fit = lambda fr, **kw: drr.fit_volumes(fr, geo, (9, 9, 9), S, bounds=ref.BOUNDS, n_phases=2, steps=1, **kw)
    theta, phi, _, image = frames[0]
    with pytest.raises(_capi.NcaError, match="no frames"):
        fit([])
    for phase in (2, -1):
        with pytest.raises(_capi.NcaError, match="phase"):
            fit(frames[:2] + [(theta, phi, phase, image)])
    with pytest.raises(_capi.NcaError, match=r"float32 \[8,8\]"):
        fit(frames[:2] + [(theta, phi, 0, image[:, :7].contiguous())])
    with pytest.raises(_capi.NcaError, match=r"float32 \[8,8\]"):
        fit(frames[:2] + [(theta, phi, 0, image.double())])
    with pytest.raises(_capi.NcaError, match="lives on"):
        fit(frames[:2] + [(theta, phi, 0, image.cpu())])
    with pytest.raises(_capi.NcaError, match="init"):
        fit(frames[:2], init=(vs, vd[:1]))
