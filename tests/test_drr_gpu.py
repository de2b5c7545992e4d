"""Volume projection on the GPU: nca_drr_project against the f64 numpy transcription of its definition (tests/drr_ref.py, pinned to
grid_sample in tests/test_drr_cpu.py), and drr.project_sequence / project_view / volume_teacher against the pieces they are made of.
The kernel-level tests run with one thread per ray and with four (nca_drr_set_split): both structures live in the library."""
import functools
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev  # noqa: F401

import drr_ref as ref

pytestmark = pytest.mark.gpu

I0 = float(np.float32(math.log(8.670397)))          # synthetic.MAX_PIXEL_VALUE as the f32 the kernels start every ray sum from
TOL = 1e-12          # of |I0| + sum |term| per ray: identical f64 operations, only the order of the sum is free ((S-1) 2^-53 of sum |term|)


@pytest.fixture(params=[1, 4], ids=["split1", "split4"])
def split(request):
    from nerfca_amd import _capi
    lib = _capi.lib()
    before = lib.nca_drr_get_split()
    _capi.check_drr(lib.nca_drr_set_split(request.param))
    yield request.param
    _capi.check_drr(lib.nca_drr_set_split(before))


@functools.lru_cache(maxsize=None)
def ray_cases():
    """[(name, o, d, z, dists)] on the CPU as numpy: the rays export.view_rays generates on the device for both detectors and both views."""
    from nerfca_amd import export
    out = []
    for name, geo, S in ref.geometries():
        z, dists = ref.depths(geo, S)
        for theta, phi in ref.VIEWS:
            o, d = export.view_rays(geo, theta, phi, device="cuda:0")
            out.append((f"{name}@{theta},{phi}", o.cpu().numpy(), d.cpu().numpy(), z, dists))
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, bounds, case):
    """(vols f32 [3,*shape], pix, scale, g) of the oracle for one grid, box and ray case; computed once."""
    _, o, d, z, dists = ray_cases()[case]
    vols = ref.random_volume((3,) + shape, seed=sum(shape))
    return (vols,) + ref.project(vols, o, d, z, dists, I0, bounds)


def gpu_project(dev, vols, case, bounds):
    from nerfca_amd import drr
    _, o, d, z, dists = ray_cases()[case]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return drr.project_rays(t(vols), t(o), t(d), t(z), t(dists), i0=I0, bounds=bounds).cpu().numpy()


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_projection_matches_the_f64_oracle(dev, split, shape):
    worst = 0.0
    for case in range(len(ray_cases())):
        vols, want, scale, _ = oracle(shape, ref.BOUNDS, case)
        got = gpu_project(dev, vols, case, ref.BOUNDS)
        assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all()          # every ray of every volume is compared
        err = np.abs(got - want) / scale
        worst = max(worst, float(err.max()))
        print(f"grid {shape} split {split} {ray_cases()[case][0]}: worst {err.max():.2e} of |I0| + sum |term|")
        assert (err <= TOL).all(), (ray_cases()[case][0], float(err.max()))
        one = gpu_project(dev, vols[2], case, ref.BOUNDS)                                              # a 3-D volume: [R], the same bits
        assert one.shape == want.shape[1:] and np.array_equal(one, got[2])


# ----------------------------------------------------------------------------- 2. the border
@pytest.mark.parametrize("shape", ref.GRIDS)
def test_small_box_outside_rim_and_inside(dev, split, shape):
    n = np.array(shape, dtype=np.float64)
    cases = range(len(ray_cases()))
    gs = [oracle(shape, ref.SMALL_BOX, c)[3] for c in cases]
    outside = [((g <= -1.0) | (g >= n)).any(-1) for g in gs]                # contributes exactly 0: no load
    inside = [((g >= 0.0) & (g < n - 1.0)).all(-1) for g in gs]             # all eight neighbours are nodes
    kinds = [sum(int(m.sum()) for m in outside), sum(int((~a & ~b).sum()) for a, b in zip(outside, inside)), sum(int(m.sum()) for m in inside)]
    assert min(kinds) > 0, kinds                                            # from the oracle's g, before anything is compared (the rim: neither)
    missed = 0
    for case in cases:
        vols, want, scale, g = oracle(shape, ref.SMALL_BOX, case)
        got = gpu_project(dev, vols, case, ref.SMALL_BOX)
        err = np.abs(got - want) / scale
        assert got.shape == want.shape and (err <= TOL).all(), (ray_cases()[case][0], float(err.max()))
        miss = outside[case].all(-1)
        missed += int(miss.sum())
        assert (want[:, miss] == I0).all() and (got[:, miss] == I0).all()   # a ray that misses the box: I0 exactly
    print(f"grid {shape}: samples outside / rim / inside = {kinds}, rays that miss the box: {missed}")
    # rays that miss every grid by construction: the same rays against a box far from the beam
    far = ((5.0, 5.5),) * 3
    vols = oracle(shape, ref.SMALL_BOX, 0)[0]
    assert (gpu_project(dev, vols, 0, far) == I0).all()


# ----------------------------------------------------------------------------- 3. index order, independently of the oracle's structure
def test_affine_volume_is_integrated_exactly(dev, split):
    shape, (a, b, c, e) = (5, 3, 4), (0.7, -1.3, 0.45, 2.1)
    axes = [np.array([lo + i * (hi - lo) / (n - 1) for i in range(n)]) for (lo, hi), n in zip(ref.WIDE, shape)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    exact = a * X + b * Y + c * Z + e
    vol = exact.astype(np.float32)
    for case, (name, o, d, z, dists) in enumerate(ray_cases()):
        g = ref.grid_coords(shape, ref.WIDE, o, d, z)
        assert ((g > 0.0) & (g < np.array(shape) - 1.0)).all(), name          # every sample strictly inside: trilinear interpolation of an affine function is exact
        p = o[:, None, :] + d[:, None, :] * z.astype(np.float64)[None, :, None]
        want = I0 - ((a * p[..., 0] + b * p[..., 1] + c * p[..., 2] + e) * dists[None, :]).sum(-1)
        got = gpu_project(dev, vol, case, ref.WIDE)
        tol = 2.0 ** -23 * float(np.abs(exact).max()) * float(dists.sum()) + 1e-12          # 2^-23 max|v| bounds the f32 rounding of the node values
        err = np.abs(got - want)
        print(f"affine volume, split {split}, {name}: worst {err.max():.2e}, tolerance {tol:.2e}")
        assert got.shape == want.shape and (err <= tol).all(), (name, float(err.max()), tol)


# ----------------------------------------------------------------------------- 4. grouping and chunking
def test_grouping_does_not_change_a_bit(dev, split):
    shape = (17, 9, 33)
    vols = ref.random_volume((11,) + shape, seed=11)
    for case in (1, 3):
        for bounds in (ref.BOUNDS, ref.SMALL_BOX):
            together = gpu_project(dev, vols, case, bounds)
            assert together.shape == (11, ray_cases()[case][1].shape[0])
            for v in range(11):
                assert np.array_equal(gpu_project(dev, vols[v], case, bounds), together[v]), v
            assert np.array_equal(gpu_project(dev, vols, case, bounds), together)          # two runs
            for k in (2, 3, 5, 8):                                                         # other groupings of the same volumes
                assert np.array_equal(gpu_project(dev, vols[:k], case, bounds), together[:k]), k


def test_chunking_does_not_change_a_bit(dev, split):
    from nerfca_amd import drr
    _, geo, S = ref.geometries()[1]
    vs = torch.from_numpy(ref.random_volume((5, 3, 4), seed=1)).to(dev).abs()
    vd = torch.from_numpy(ref.random_volume((3, 5, 3, 4), seed=2)).to(dev).abs()
    whole = drr.project_sequence(vs, vd, geo, ref.VIEWS, S, bounds=ref.BOUNDS)
    for chunk in (7, 64, 12 * 20):
        for _ in range(2):
            out = drr.project_sequence(vs, vd, geo, ref.VIEWS, S, bounds=ref.BOUNDS, chunk_rays=chunk)
            for k in whole:
                assert torch.equal(out[k], whole[k]), (k, chunk)


# ----------------------------------------------------------------------------- 5. project_sequence and project_view
def small_pair(dev, F=32, seed=5):
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    torch.manual_seed(seed)
    sd, td = synthetic.net_definitions(dev, F=F)
    s, t = CPPN(sd).to(dev), Temporal(td).to(dev)
    for m in (s, t):
        m.update_freq_mask_alpha(75000, 150000)
    return s, t


def test_sequence_is_compose_of_project_rays(dev):
    from nerfca_amd import drr, export
    _, geo, S = ref.geometries()[1]
    W, H = geo["nDetector"]
    vs = torch.from_numpy(ref.random_volume((17, 9, 33), seed=3)).to(dev).abs()
    vd = torch.from_numpy(ref.random_volume((3, 17, 9, 33), seed=4)).to(dev).abs()
    z = torch.from_numpy(ref.depths(geo, S)[0]).to(dev)
    out = drr.project_sequence(vs, vd, geo, ref.VIEWS, S, bounds=ref.BOUNDS)
    assert set(out) == {"pred", "pred_static", "pred_dynamic"}
    for v, (theta, phi) in enumerate(ref.VIEWS):
        o, d = export.view_rays(geo, theta, phi, device=dev)
        pix_s = drr.project_rays(vs, o, d, z, i0=I0, bounds=ref.BOUNDS)
        pix_d = drr.project_rays(vd, o, d, z, i0=I0, bounds=ref.BOUNDS)
        for j in range(3):
            pred, pred_s, pred_d = (torch.empty(W * H, dtype=torch.float32, device=dev) for _ in range(3))
            export.compose_images(pix_s, pix_d[j], I0, pred, pred_s, pred_d)
            assert torch.equal(out["pred"][v, j].reshape(-1), pred) and torch.equal(out["pred_dynamic"][v, j].reshape(-1), pred_d)
            assert torch.equal(out["pred_static"][v].reshape(-1), pred_s)
    one = drr.project_view(vs, vd[1], geo, *ref.VIEWS[1], S, bounds=ref.BOUNDS)
    assert set(one) == set(out)
    assert torch.equal(one["pred"], out["pred"][1, 1]) and torch.equal(one["pred_static"], out["pred_static"][1])
    assert torch.equal(one["pred_dynamic"], out["pred_dynamic"][1, 1])


def test_sequence_has_the_keys_and_shapes_of_render_sequence(dev):
    from nerfca_amd import drr, export
    _, geo, S = ref.geometries()[1]
    W, H = geo["nDetector"]
    s, t = small_pair(dev)
    vs = torch.from_numpy(ref.random_volume((5, 3, 4), seed=5)).to(dev).abs()
    vd = torch.from_numpy(ref.random_volume((2, 5, 3, 4), seed=6)).to(dev).abs()
    for normalize in (False, True):
        want = export.render_sequence(s, t, geo, ref.VIEWS, [0, 3], S, normalize=normalize)
        got = drr.project_sequence(vs, vd, geo, ref.VIEWS, S, bounds=ref.BOUNDS, normalize=normalize)
        assert set(got) == set(want)
        for k in want:
            if k == "minmax":
                assert set(got[k]) == set(want[k]) and all(got[k][n].shape == want[k][n].shape for n in want[k])
            else:
                assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].device == want[k].device, k
        want1 = export.render_view(s, t, geo, *ref.VIEWS[0], 3, S, normalize=normalize)
        got1 = drr.project_view(vs, vd[1], geo, *ref.VIEWS[0], S, bounds=ref.BOUNDS, normalize=normalize)
        assert set(got1) == set(want1) and all(got1[k].shape == want1[k].shape for k in want1 if k != "minmax")
        if normalize:
            assert all(got1["minmax"][n].shape == want1["minmax"][n].shape == (2,) for n in want1["minmax"])
    # normalize: the *_norm images are normalize_images of the plain ones, minmax their extrema
    for k in ("pred", "pred_static", "pred_dynamic"):
        img = got[k].reshape(-1, W, H)
        assert torch.equal(got["minmax"][k].reshape(-1, 2), torch.stack([img.amin((1, 2)), img.amax((1, 2))], -1))
        norm, _ = export.normalize_images(img)
        assert torch.equal(got[k + "_norm"].reshape(-1, W, H), norm)


def test_static_only_behaves_like_temp_model_none(dev):
    from nerfca_amd import drr
    _, geo, S = ref.geometries()[0]
    vs = torch.from_numpy(ref.random_volume((5, 3, 4), seed=7)).to(dev).abs()
    out = drr.project_sequence(vs, None, geo, ref.VIEWS, S, bounds=ref.BOUNDS)
    assert out["pred"].shape == out["pred_dynamic"].shape == (2, 1, 8, 8) and out["pred_static"].shape == (2, 8, 8)
    assert torch.equal(out["pred"][:, 0], out["pred_static"])
    assert (out["pred_dynamic"] == np.float32(I0)).all()
    assert (out["pred_static"] < np.float32(I0)).any()                      # the volume is seen
    one = drr.project_view(vs, None, geo, *ref.VIEWS[0], S, bounds=ref.BOUNDS)
    assert torch.equal(one["pred"], out["pred"][0, 0]) and torch.equal(one["pred"], one["pred_static"])


# ----------------------------------------------------------------------------- 6. the dataset hook
def test_volume_teacher_makes_a_dataset(dev):
    from nerfca_amd import _capi, drr, synthetic
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    vs_np, vd_np = np.abs(ref.random_volume((5, 3, 4), seed=8)), np.abs(ref.random_volume((3, 5, 3, 4), seed=9))
    vs, vd = torch.from_numpy(vs_np).to(dev), torch.from_numpy(vd_np).to(dev)
    data = synthetic.make_dataset(8, 16, dev, teacher=(vs, vd), render=drr.volume_teacher(ref.BOUNDS), n_phases=3)
    assert isinstance(data, synthetic.SyntheticData)
    assert data.rays_train.shape == (4 * 3 * 64, 4, 3) and data.phases_train.shape == (4 * 3 * 64,) and data.n_images == 12
    assert torch.isfinite(data.test_image).all() and data.test_image.shape == (64,)
    view, phase = 2, 1                                                      # image (view, phase) holds rows [(view * 3 + phase) * 64, +64)
    rows = data.rays_train[(view * 3 + phase) * 64:(view * 3 + phase + 1) * 64].cpu().numpy()
    assert (data.phases_train[(view * 3 + phase) * 64:(view * 3 + phase + 1) * 64] == phase).all()
    z = create_depth_values(synthetic.NEAR, synthetic.FAR, 16, "cpu").to(torch.float32)
    dists = _interval_lengths(z, torch.empty(0, dtype=torch.float32)).double().numpy()          # make_dataset's: the tail in the rays' f32
    o, d = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    pix_s = ref.project(vs_np, o, d, z.numpy(), dists, I0, ref.BOUNDS)[0]
    pix_d = ref.project(vd_np, o, d, z.numpy(), dists, I0, ref.BOUNDS)[0]
    want = ((pix_s + pix_d[phase]) - I0).astype(np.float32)
    assert (want < 0.999 * I0).any()                                        # the volumes are seen
    assert np.array_equal(rows[:, 2, 0].astype(np.float32), want) and np.array_equal(rows[:, 2, 0], rows[:, 2, 2])
    # a call with two phases, or with a phase the stack does not have, is refused
    hook = drr.volume_teacher(ref.BOUNDS)
    ot, dt = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    I0t, zt, dd = torch.full((64,), I0, dtype=torch.float32, device=dev), z.to(dev), torch.from_numpy(dists).to(dev)
    mixed = torch.zeros(64, dtype=torch.int32, device=dev)
    mixed[5] = 2
    with pytest.raises(_capi.NcaError, match="ONE phase"):
        hook(vs, vd, ot, dt, mixed, I0t, zt, dd)
    with pytest.raises(_capi.NcaError, match="phase -1"):
        hook(vs, vd, ot, dt, mixed.fill_(-1), I0t, zt, dd)
    # the stack is one heart cycle: phase 3 of 3 volumes is volume 0 (make_dataset's held-out image is phase 3 whatever n_phases)
    assert torch.equal(hook(vs, vd, ot, dt, mixed.fill_(3), I0t, zt, dd), hook(vs, vd, ot, dt, mixed.fill_(0), I0t, zt, dd))
    assert not torch.equal(hook(vs, vd, ot, dt, mixed.fill_(3), I0t, zt, dd), hook(vs, vd, ot, dt, mixed.fill_(1), I0t, zt, dd))
    to, td = data.test_origins.double().cpu().numpy(), data.test_directions.double().cpu().numpy()
    test_want = ((ref.project(vs_np, to, td, z.numpy(), dists, I0, ref.BOUNDS)[0] + ref.project(vd_np[0], to, td, z.numpy(), dists, I0, ref.BOUNDS)[0]) - I0)
    assert data.test_phase == 3 and np.array_equal(data.test_image.cpu().numpy(), test_want.astype(np.float32))


# ----------------------------------------------------------------------------- 7. the trained-field loop closes
def test_exported_volumes_reproject_to_the_rendered_view(dev):
    from nerfca_amd import drr, export
    _, geo, S = ref.geometries()[0]
    s, t = small_pair(dev)
    sig_s, sig_d = export.density_volumes(s, t, [3], resolution=(16, 16, 16), bounds=ref.WIDE)
    want = export.render_view(s, t, geo, *ref.VIEWS[0], 3, S)
    got = drr.project_view(sig_s, sig_d[0], geo, *ref.VIEWS[0], S, bounds=ref.WIDE)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and torch.isfinite(got[k]).all(), k
        print(f"reprojection of a 16^3 export vs render_view, {k}: max |difference| {float((got[k] - want[k]).abs().max()):.3e} (recorded, not gated)")
