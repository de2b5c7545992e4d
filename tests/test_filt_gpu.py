"""The filters of the CCTA pipeline on the GPU: nca_vol_smooth and nca_vol_cityblock against the numpy transcription of their definitions
(tests/filt_ref.py, held to scipy.ndimage bit for bit in tests/test_filt_cpu.py), bit for bit in every case, and nerfca_amd.ccta and
metrics.mask_distances(surface=True) on top of them.  Output buffers are pre-filled (NaN, -1), so a node the kernels did not write shows.

Tile sizes of the kernels.  Smoothing: the axis 0 and axis 1 launches take tiles of 64 columns x 32 nodes along the line, the axis 2 launch
one wave per row and 256 nodes of it per tile.  (3,5,70): a row crosses a wave; (2,3,4) with radii (6,3,8): the halo reflects more than
once; (9,4,130): a skipped axis and three chunks of 64 along the row; (5,6,7) at radius 32: the largest halo; (33,17,65): one past a tile on
every axis (33 along the line of axis 0, 65 columns for axis 1, 17 x 65 = 1105 columns for axis 0), three volumes; (2,3,300): two row
tiles.  City-block: the row pass takes chunks of 64 nodes; the line passes take tiles of 16 columns, and the sixteen threads of a line take
segments of ceil(len / 16) nodes: (17,33,5) has lines of 17 (nine segments of 2, the last of 1 node, seven empty) and 33 nodes."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.ndimage
import torch

from nca_testlib import dev, grid_of, gpu_stack_call, same_bits  # noqa: F401

import filt_ref as ref

pytestmark = pytest.mark.gpu


def gpu_smooth(dev, vol, sigma, radius):
    """out f32 of one nca_vol_smooth of a stack [n_vol,n0,n1,n2] into a buffer pre-filled with NaN, the workspace exactly as large as the
    query says (and itself pre-filled, with 0xff bytes)."""
    from nerfca_amd import _capi, ccta
    lib = _capi.lib()
    halves = [ccta.gaussian_weights(float(s), int(r)) for s, r in zip(ref.per_axis(sigma), ref.per_axis(radius))]
    flat = np.concatenate(halves)
    args = ((C.c_int32 * 3)(*[len(h) - 1 for h in halves]), (C.c_double * flat.size)(*flat.tolist()))
    return gpu_stack_call(dev, _capi.check_filt, lib.nca_vol_smooth, lib.nca_vol_smooth_workspace, grid_of(np.shape(vol)[1:]), vol, args, math.nan, torch.float32, 16)


def gpu_cityblock(dev, vol, threshold=0.5, invert=0, border=0):
    """out int32 of one nca_vol_cityblock, likewise, into a buffer pre-filled with -1."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    return gpu_stack_call(dev, _capi.check_filt, lib.nca_vol_cityblock, lib.nca_vol_cityblock_workspace, grid_of(np.shape(vol)[1:]), vol,
                          (float(threshold), invert, border), -1, torch.int32, 8)


# ----------------------------------------------------------------------------- smoothing
SMOOTH_GPU_CASES = ref.SMOOTH_CASES + (((33, 17, 65), (1.2, 2.0, 0.8), (5, 7, 3)), ((2, 3, 300), (0.5, 0.5, 3.0), (1, 2, 12)))


@pytest.mark.parametrize("shape,sigma,radius", SMOOTH_GPU_CASES, ids=lambda v: str(v))
def test_smoothing_bit_for_bit(dev, shape, sigma, radius):
    """A stack of three volumes against the oracle, each volume on its own (volumes are independent), and a second run (the same bits)."""
    stack = np.stack([ref.smooth_volume(shape, seed=s) for s in range(3)])
    want = ref.smooth(stack, sigma, radius)
    got = gpu_smooth(dev, stack, sigma, radius)
    assert not np.isnan(got).any()
    assert same_bits(got, want), int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max())
    assert same_bits(gpu_smooth(dev, stack, sigma, radius), got)
    for k in (0, 2):
        assert same_bits(gpu_smooth(dev, stack[k:k + 1], sigma, radius)[0], got[k]), k


def test_gaussian_filter_against_scipy(dev):
    from nerfca_amd import _capi, ccta
    shape = (9, 4, 130)
    vol = np.stack([ref.smooth_volume(shape, seed=s) for s in range(6)]).reshape((2, 3) + shape)
    x = torch.from_numpy(vol).to(dev).requires_grad_()
    for sigma, radius, truncate in ((1.0, 2, 4.0), ((1, 0, 2.5), (4, 0, 10), 4.0), (1.3, None, 3.0)):
        got = ccta.gaussian_filter(x, sigma, radius=radius, truncate=truncate)
        assert got.shape == x.shape and got.dtype == torch.float32 and not got.requires_grad and got.device == x.device
        flat = ccta.gaussian_filter(x.reshape((6,) + shape), sigma, radius=radius, truncate=truncate)          # a leading shape equals the flattened call
        assert torch.equal(got.reshape(flat.shape).view(torch.int32), flat.view(torch.int32))
        for k in range(6):
            sci = scipy.ndimage.gaussian_filter(vol.reshape((6,) + shape)[k].astype(np.float64), sigma, radius=radius, truncate=truncate, mode="reflect")
            assert same_bits(flat[k].cpu().numpy(), sci.astype(np.float32)), (sigma, k)
    with pytest.raises(_capi.NcaError, match="float32"):
        ccta.gaussian_filter(x.double(), 1.0)
    with pytest.raises(_capi.NcaError, match="32"):
        ccta.gaussian_filter(x, 9.0)
    with pytest.raises(_capi.NcaError, match="per axis"):
        ccta.gaussian_filter(x, (1.0, 2.0))


# ----------------------------------------------------------------------------- the city-block distance
CITY_GPU_SHAPES = ((4, 5, 6), (7, 9, 70), (3, 3, 3), (2, 2, 2), (6, 8, 200), (17, 33, 5))


@pytest.mark.parametrize("shape", CITY_GPU_SHAPES, ids=str)
def test_cityblock_bit_for_bit(dev, shape):
    """Both fills as one stack with an empty volume between them, invert and border in all four combinations; a second run; each alone."""
    for invert in (0, 1):
        for border in (0, 1):
            cases = [ref.city_case(shape, 0.02, invert, border), (np.zeros(shape, dtype=np.float32), ref.cityblock(np.zeros(shape, dtype=np.float32), 0.5, invert, border)),
                     ref.city_case(shape, 0.97, invert, border)]
            vols, want = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
            got = gpu_cityblock(dev, vols, 0.5, invert, border)
            assert got.dtype == np.int32 and (got >= 0).all()
            assert np.array_equal(got, want), (invert, border)
            for k in range(3):          # the sentinel in a volume without a feature and without a border, and only there
                empty = not ref.features(vols[k], 0.5, invert).any()
                assert (got[k] == ref.NONE).all() == (got[k] == ref.NONE).any() == (empty and not border), (invert, border, k)
            if not invert:
                assert (got[1] == ref.NONE).all() if not border else np.array_equal(got[1], ref.border_term(shape))
            assert np.array_equal(gpu_cityblock(dev, vols, 0.5, invert, border), got)
            assert np.array_equal(gpu_cityblock(dev, vols[2:3], 0.5, invert, border)[0], got[2])


def test_a_single_feature_in_the_last_chunk_and_a_nan(dev):
    shape = (6, 8, 200)
    vol = np.zeros(shape, dtype=np.float32)
    vol[5, 7, 199] = 1.0
    for border in (0, 1):
        got = gpu_cityblock(dev, vol[None], 0.5, 0, border)[0]
        assert np.array_equal(got, ref.cityblock(vol, 0.5, 0, border))
    assert gpu_cityblock(dev, vol[None])[0, 0, 0, 0] == 5 + 7 + 199
    # one node equal to the threshold, one NaN, one above: only the last is a feature; under invert the first two are and the last is not
    vol = np.zeros((3, 5, 65), dtype=np.float32)
    vol[0, 0, 0], vol[1, 2, 64], vol[2, 4, 30] = 0.5, np.nan, 0.75
    for invert in (0, 1):
        for border in (0, 1):
            got = gpu_cityblock(dev, vol[None], 0.5, invert, border)[0]
            assert np.array_equal(got, ref.cityblock(vol, 0.5, invert, border)), (invert, border)
    plain, flipped = gpu_cityblock(dev, vol[None])[0], gpu_cityblock(dev, vol[None], invert=1)[0]
    assert plain[2, 4, 30] == 0 and plain[0, 0, 0] > 0 and plain[1, 2, 64] > 0
    assert flipped[2, 4, 30] == 1 and flipped[0, 0, 0] == 0 and flipped[1, 2, 64] == 0


def test_the_longest_axis(dev):
    """512 nodes along each axis in turn: the line tile is the longest the kernel stages (segments of 32 nodes); a single feature at the
    far end crosses every segment."""
    for axis in range(3):
        shape = [2, 3, 2]
        shape[axis] = 512
        vol = np.zeros(shape, dtype=np.float32)
        vol[tuple(s - 1 for s in shape)] = 1.0
        dense = (np.random.default_rng(axis).random(shape) < 0.01).astype(np.float32)
        stack = np.stack([vol, dense])
        for invert, border in ((0, 0), (1, 1)):
            assert np.array_equal(gpu_cityblock(dev, stack, 0.5, invert, border), ref.cityblock(stack, 0.5, invert, border)), (axis, invert, border)


def test_dilation_erosion_and_border_against_scipy(dev):
    from nerfca_amd import _capi, ccta
    shape = (7, 9, 70)
    vols = np.stack([ref.mask_volume(shape, f) for f in (0.02, 0.3, 0.97)])
    x = torch.from_numpy(vols).to(dev)
    M = vols > 0.5
    for n in (1, 3, 5):
        dil, ero = ccta.binary_dilation(x, n, threshold=0.5), ccta.binary_erosion(x, n, threshold=0.5)
        assert dil.dtype == torch.bool and dil.shape == x.shape and ero.dtype == torch.bool and dil.device == x.device
        for k in range(3):
            assert np.array_equal(dil[k].cpu().numpy(), scipy.ndimage.binary_dilation(M[k], iterations=n)), (n, k)
            assert np.array_equal(ero[k].cpu().numpy(), scipy.ndimage.binary_erosion(M[k], iterations=n)), (n, k)
    assert torch.equal(ccta.binary_dilation(x > 0.5, 3), ccta.binary_dilation(x, 3, threshold=0.5))          # a bool mask is taken as it is
    brd = ccta.mask_border(x, threshold=0.5).cpu().numpy()
    dist = ccta.cityblock_distance(x, threshold=0.5).cpu().numpy()
    closed = ccta.binary_erosion(ccta.binary_dilation(x, 3, threshold=0.5), 1).cpu().numpy()
    for k in range(3):
        assert np.array_equal(brd[k], M[k] ^ scipy.ndimage.binary_erosion(M[k]))
        assert np.array_equal(dist[k], scipy.ndimage.distance_transform_cdt(~M[k], metric="taxicab"))
        assert np.array_equal(closed[k], scipy.ndimage.binary_erosion(scipy.ndimage.binary_dilation(M[k], iterations=3), iterations=1))
    lead = ccta.cityblock_distance(x.reshape((3, 1) + shape), threshold=0.5, inside=True, border=True)
    assert lead.shape == (3, 1) + shape and lead.dtype == torch.int32 and np.array_equal(lead.reshape(x.shape).cpu().numpy(), ref.cityblock(vols, 0.5, 1, 1))
    for bad in (0, -1, 1.5):
        with pytest.raises(_capi.NcaError, match="iterations"):
            ccta.binary_dilation(x, bad)
        with pytest.raises(_capi.NcaError, match="iterations"):
            ccta.binary_erosion(x, bad)
    with pytest.raises(_capi.NcaError, match="nan"):
        ccta.cityblock_distance(x, threshold=math.nan)
    with pytest.raises(_capi.NcaError, match="NCA_EDT_MAX_AXIS"):
        ccta.cityblock_distance(torch.zeros((2, 2, 513), device=dev), threshold=0.5)


# ----------------------------------------------------------------------------- the pipeline
UNIT_BOUNDS = tuple((0.0, float(n - 1)) for n in (24, 20, 70))          # unit spacing, as the reference has after its resampling


@pytest.fixture(scope="module")
def tube_case():
    """The reference restatement of the two-tube case, computed once: (hu, mask, labels, full, vessel, closed, bound)."""
    mask = ref.tubes()
    rng = np.random.default_rng(3)
    hu = (rng.random(mask.shape) * 1400 - 1000).astype(np.float32)
    labels = np.zeros(mask.shape, dtype=np.int64)
    labels[2:9, 3:12, 10:30] = 51
    labels[12:20, 5:15, 35:60] = 52
    full, vessel, closed, dist = ref.prepare_ccta_ref(hu, mask, labels, 52, 51)
    bound = ref.contrast_bound(float(dist.max()))
    assert 2.0 < dist.max() < 4.0 and 0 < bound < 1e-8          # the transfer function's first three segments are all reached
    return hu, mask, labels, full, vessel, closed, bound


def test_vessel_contrast_against_the_reference_restatement(dev, tube_case):
    from nerfca_amd import _capi, ccta
    hu, mask, labels, full, vessel, closed, bound = tube_case
    m = torch.from_numpy(np.array(mask)).to(dev)
    got, got_closed = ccta.vessel_contrast(m, UNIT_BOUNDS)
    assert got.dtype == torch.float32 and got.shape == m.shape and got_closed.dtype == torch.bool
    assert np.array_equal(got_closed.cpu().numpy(), closed)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - vessel).max())
    print(f"vessel_contrast: largest error {err:.3e}, bound {bound:.3e}; largest value {vessel.max():.4f}")
    assert err <= bound
    assert (got[~got_closed] == 0).all() and float(got.max()) > 0.02
    again, _ = ccta.vessel_contrast(m > 0, UNIT_BOUNDS)
    assert torch.equal(again, got)
    with pytest.raises(_capi.NcaError, match="increasing"):
        ccta.vessel_contrast(m, UNIT_BOUNDS, xp=(0, 1, 1, 4, 5))
    with pytest.raises(_capi.NcaError, match="one length"):
        ccta.vessel_contrast(m, UNIT_BOUNDS, xp=(0, 1, 2))


def test_prepare_ccta_and_projection(dev, tube_case):
    from nerfca_amd import ccta, drr, synthetic
    hu, mask, labels, full, vessel, closed, bound = tube_case

    def stack(a):          # two volumes: the second flipped along axis 0
        return torch.from_numpy(np.stack([np.array(a), np.array(a)[::-1].copy()])).to(dev)

    out = ccta.prepare_ccta(stack(hu), stack(mask), UNIT_BOUNDS, labels=stack(labels), aorta_label=52, heart_label=51)
    assert set(out) == {"static", "dynamic", "mask", "bounds"} and out["bounds"] == UNIT_BOUNDS
    for k in ("static", "dynamic"):
        assert out[k].shape == (2,) + mask.shape and out[k].dtype == torch.float32 and out[k].is_contiguous()
    total = (out["static"].double() + out["dynamic"].double()).cpu().numpy()
    err = float(np.abs(total[0] - full).max())
    print(f"prepare_ccta: largest error of static + dynamic {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(out["mask"][0].cpu().numpy(), closed) and np.array_equal(out["mask"][1].cpu().numpy(), closed[::-1])
    assert float(np.abs(total[1] - full[::-1]).max()) <= bound          # the volumes of a stack are prepared on their own
    assert (out["static"][out["mask"]] == 0).all() and (out["dynamic"][~out["mask"]] == 0).all()
    one = ccta.prepare_ccta(torch.from_numpy(hu).to(dev), torch.from_numpy(np.array(mask)).to(dev), UNIT_BOUNDS)
    assert one["static"].shape == mask.shape and torch.equal(one["dynamic"], out["dynamic"][0])
    # straight into the projector: the tensors as they are, no copy
    geo = synthetic.xcat_geometry(8)
    world = tuple((-0.18 * n / 70, 0.18 * n / 70) for n in mask.shape)
    seq = drr.project_sequence(out["static"][0], out["dynamic"], geo, [(-5.0, 40.0)], 16, bounds=world)
    assert seq["pred"].shape[:2] == (1, 2) and torch.isfinite(seq["pred"]).all()
    assert not torch.equal(seq["pred"][0, 0], seq["pred"][0, 1])


def test_surface_distances_against_the_medpy_restatement(dev):
    from nerfca_amd import metrics
    pred, truth = ref.blobs()
    h = (0.5, 0.4, 0.3)
    bounds = tuple((0.0, h[a] * (pred.shape[a] - 1)) for a in range(3))
    p, t = torch.from_numpy(np.stack([pred, truth])).to(dev), torch.from_numpy(np.stack([truth, truth])).to(dev)
    got = metrics.mask_distances(p, t, bounds, threshold=0.5, surface=True)
    want = ref.surface_distances_ref(pred > 0.5, truth > 0.5, h)
    assert int(got["n_pred"][0]) == want["n_pred"] and int(got["n_truth"][0]) == want["n_truth"] and int(got["n_pred"][1]) == want["n_truth"]
    for k in ("pred_to_truth", "truth_to_pred", "assd", "hausdorff", "hd_percentile"):
        assert got[k].shape == (2,) and got[k].dtype == torch.float64
        assert abs(float(got[k][0]) - want[k]) <= 2.0 ** -23 * want[k], (k, float(got[k][0]), want[k])          # one f32 step at non-unit spacing
        assert float(got[k][1]) == 0.0, k          # identical surfaces
    plain = metrics.mask_distances(p, t, bounds, threshold=0.5)
    off = metrics.mask_distances(p, t, bounds, threshold=0.5, surface=False)
    assert set(plain) == set(off) == set(got)
    for k in plain:
        assert torch.equal(plain[k], off[k]) and plain[k].dtype == off[k].dtype, k
    assert float(plain["assd"][0]) < float(got["assd"][0]) and int(plain["n_pred"][0]) > want["n_pred"]
