"""The distance transform on the GPU: nca_vol_edt against the numpy transcription of its definition (tests/edt_ref.py, held to the brute-force
minimum and to scipy in tests/test_edt_cpu.py), bit for bit in every case, and metrics.distance_transform / mask_distances /
centreline_coverage on top of it.  The output buffer is pre-filled with NaN, so a node the kernels did not write shows.

Tile sizes of the kernels: the row pass takes one wave per row and chunks of 64 nodes along axis 2; the two line passes take tiles of 16
columns and 16 nodes along the line per step.  Shapes: (2,2,2); (3,5,64) one chunk; (3,5,65) one node past it; (5,9,130) two chunk carries;
(3,17,18) one past the 16 nodes of a step along axis 1 and one column tile past 16; (17,3,6) the same along axis 0 (its columns are the 18
nodes of a plane); (512,2,2) the longest line, the whole 64 KiB of LDS."""
import math

import numpy as np
import pytest
import scipy.ndimage
import torch

from nca_testlib import dev, grid_of, gpu_stack_call, same_bits, ulp_distance  # noqa: F401

import edt_ref as ref

pytestmark = pytest.mark.gpu


def gpu_edt(dev, vol, inv, threshold=ref.THRESHOLD, invert=0):
    """out f32 of one nca_vol_edt of a stack [n_vol,n0,n1,n2] into a buffer pre-filled with NaN, the workspace exactly as large as the query says
    (and itself pre-filled, with 0xff bytes)."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    return gpu_stack_call(dev, _capi.check_edt, lib.nca_vol_edt, lib.nca_vol_edt_workspace, grid_of(np.shape(vol)[1:], inv), vol, (float(threshold), invert), math.nan,
                          torch.float32, 12)


@pytest.mark.parametrize("inv", [ref.UNIT, ref.ANISO], ids=["unit", "aniso"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_every_pattern_bit_for_bit(dev, shape, inv):
    """All patterns of a shape as one stack (the empty volume lies between two others: its neighbours are unaffected), then each on its own:
    a stack equals its volumes one by one, and a second run gives the same bits."""
    cases = [ref.case(shape, p, inv) for p in ref.PATTERNS]
    vols, want = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    assert np.isinf(want[ref.PATTERNS.index("none")]).all() and (want[ref.PATTERNS.index("all")] == 0).all()
    got = gpu_edt(dev, vols, inv)
    for k, p in enumerate(ref.PATTERNS):
        assert not np.isnan(got[k]).any(), p
        assert same_bits(got[k], want[k]), (p, int(ulp_distance(got[k], want[k]).max()))
    assert same_bits(gpu_edt(dev, vols, inv), got)
    for k in (0, ref.PATTERNS.index("d0.05"), ref.PATTERNS.index("none")):
        assert same_bits(gpu_edt(dev, vols[k:k + 1], inv)[0], got[k]), ref.PATTERNS[k]


@pytest.mark.parametrize("inv", [ref.UNIT, ref.ANISO], ids=["unit", "aniso"])
def test_a_stack_of_three_with_an_empty_volume_in_the_middle(dev, inv):
    shape = (5, 9, 130)
    names = ("d0.05", "none", "d0.002")
    vols = np.stack([ref.case(shape, p, inv)[0] for p in names])
    want = np.stack([ref.case(shape, p, inv)[1] for p in names])
    got = gpu_edt(dev, vols, inv)
    assert same_bits(got, want) and np.isinf(got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    for k in range(3):
        assert same_bits(gpu_edt(dev, vols[k:k + 1], inv)[0], got[k])


@pytest.mark.parametrize("shape", [(3, 5, 65), (5, 9, 130), (3, 17, 18)], ids=str)
def test_invert(dev, shape):
    for pattern in ("d0.05", "d0.5", "all", "none", "corner"):
        for inv in (ref.UNIT, ref.ANISO):
            vol, want = ref.case(shape, pattern, inv, 1)
            got = gpu_edt(dev, vol[None], inv, invert=1)[0]
            assert same_bits(got, want), (pattern, inv)
    assert np.isinf(ref.case(shape, "all", ref.UNIT, 1)[1]).all() and (ref.case(shape, "none", ref.UNIT, 1)[1] == 0).all()


def test_a_value_equal_to_the_threshold_and_a_nan(dev):
    """The only candidates are one node equal to the threshold, one NaN and one node above it: only the last is a feature; under invert
    the first two are among the features and the last is not."""
    shape = (3, 5, 65)
    vol = np.zeros(shape, dtype=np.float32)
    vol[0, 0, 0] = 0.5
    vol[1, 2, 64] = np.nan
    vol[2, 4, 30] = 0.75
    for inv in (ref.UNIT, ref.ANISO):
        for invert in (0, 1):
            want = ref.edt(vol, inv, 0.5, invert)
            got = gpu_edt(dev, vol[None], inv, threshold=0.5, invert=invert)[0]
            assert same_bits(got, want), (inv, invert)
        plain = gpu_edt(dev, vol[None], inv, threshold=0.5)[0]
        assert plain[2, 4, 30] == 0 and plain[0, 0, 0] > 0 and plain[1, 2, 64] > 0
        flipped = gpu_edt(dev, vol[None], inv, threshold=0.5, invert=1)[0]
        assert flipped[2, 4, 30] > 0 and flipped[0, 0, 0] == 0 and flipped[1, 2, 64] == 0
    # the threshold is compared in f64: a threshold just above an f32 value
    vol[:] = np.float32(0.1)
    vol[1, 1, 1] = np.nextafter(np.float32(0.1), np.float32(1))
    thr = float(np.float32(0.1)) + 2.0 ** -40
    assert same_bits(gpu_edt(dev, vol[None], ref.ANISO, threshold=thr)[0], ref.edt(vol, ref.ANISO, thr))


def test_the_longest_axis(dev):
    """512 nodes along each axis in turn (the other two of 2 and 3): the line tile fills the 64 KiB of LDS; a single feature at the far end
    is the case in which no search stops early."""
    for axis in range(3):
        shape = [2, 3, 2]
        shape[axis] = 512
        vol = np.zeros(shape, dtype=np.float32)
        vol[tuple(s - 1 for s in shape)] = 1.0
        rng = np.random.default_rng(axis)
        dense = (rng.random(shape) < 0.01).astype(np.float32)
        stack = np.stack([vol, dense])
        assert same_bits(gpu_edt(dev, stack, ref.ANISO), ref.edt(stack, ref.ANISO, ref.THRESHOLD)), axis


# ----------------------------------------------------------------------------- the Python layer
BOUNDS = ((0.0, 0.37 * 4), (-1.0, -1.0 + 0.11 * 8), (2.0, 2.0 + 0.29 * 129))          # (5, 9, 130) nodes: the spacings 0.37, 0.11, 0.29


def test_distance_transform_against_scipy(dev):
    from nerfca_amd import metrics
    shape = (5, 9, 130)
    vol = np.stack([ref.volume(shape, "d0.05"), ref.volume(shape, "d0.5")])
    x = torch.from_numpy(vol).to(dev).requires_grad_()
    h = [(b[1] - b[0]) / (n - 1) for n, b in zip(shape, BOUNDS)]
    inv = [(n - 1) / (b[1] - b[0]) for n, b in zip(shape, BOUNDS)]
    for inside in (False, True):
        got = metrics.distance_transform(x, BOUNDS, threshold=ref.THRESHOLD, inside=inside)
        assert got.shape == x.shape and got.dtype == torch.float32 and not got.requires_grad and got.device == x.device
        assert same_bits(got.cpu().numpy(), ref.edt(vol, inv, ref.THRESHOLD, int(inside)))
        for k in range(2):
            mask = vol[k] > ref.THRESHOLD
            sci = scipy.ndimage.distance_transform_edt(mask if inside else ~mask, sampling=h).astype(np.float32)
            assert int(ulp_distance(got[k].cpu().numpy(), sci).max()) <= 1, (inside, k)
    unit = metrics.distance_transform(x[0], ((0.0, 4.0), (0.0, 8.0), (0.0, 129.0)), threshold=ref.THRESHOLD, inside=True)
    assert same_bits(unit.cpu().numpy(), scipy.ndimage.distance_transform_edt(vol[0] > ref.THRESHOLD).astype(np.float32))
    lead = metrics.distance_transform(x.reshape((2, 1) + shape), BOUNDS, threshold=ref.THRESHOLD)
    assert lead.shape == (2, 1) + shape and same_bits(lead.reshape(x.shape).cpu().numpy(), ref.edt(vol, inv, ref.THRESHOLD))
    from nerfca_amd import _capi
    with pytest.raises(_capi.NcaError, match="float32"):
        metrics.distance_transform(x.double(), BOUNDS, threshold=0.5)
    with pytest.raises(_capi.NcaError, match="nan"):
        metrics.distance_transform(x, BOUNDS, threshold=math.nan)
    with pytest.raises(_capi.NcaError, match="one shape"):
        metrics.mask_distances(x, x[:1], BOUNDS, threshold=0.5)
    with pytest.raises(_capi.NcaError, match="NCA_EDT_MAX_AXIS"):
        metrics.distance_transform(torch.zeros((2, 2, 513), device=dev), ((0.0, 1.0),) * 3, threshold=0.5)


@pytest.fixture(scope="module")
def phantom24(dev):
    from nerfca_amd import phantom, synthetic
    geo = synthetic.xcat_geometry(16)
    # Vessel walls four cells wide.  The node nearest a centreline point is at most half a cell diagonal, 0.866 h, from it, so its coverage
    # is at least 0.5 - 0.866 / 4 = 0.28 and its value above rho / 4: at this edge every centreline point reads a node of the truth mask.
    # (At the default edge of one cell the tips of the tree, thinner than a cell, leave gaps in the mask of a 24^3 grid.)
    return phantom.make_phantom((24, 24, 24), 2, geo, device=dev, edge=4 * 2 * phantom.fov_half_width(geo) / 23)


def test_phantom_distances_against_the_oracle_reductions(dev, phantom24):
    from nerfca_amd import metrics, phantom
    ph = phantom24
    bounds, truth = ph["bounds"], ph["dynamic"]
    thr = 0.25 * phantom.RHO_VESSEL
    pred = 0.3 * torch.roll(truth, shifts=(1, -2), dims=(1, 3))          # a dimmer, displaced copy: thresholded at a quarter of its own maximum
    pthr = 0.25 * float(pred.max())
    inv = [23 / (b[1] - b[0]) for b in bounds]
    h = [1.0 / v for v in inv]
    got = metrics.mask_distances(pred, truth, bounds, threshold=thr, pred_threshold=pthr)
    a, b = pred.cpu().numpy() > pthr, truth.cpu().numpy() > thr
    to_a, to_b = ref.edt(pred.cpu().numpy(), inv, pthr), ref.edt(truth.cpu().numpy(), inv, thr)
    assert a.any(axis=(1, 2, 3)).all() and b.any(axis=(1, 2, 3)).all()
    want = metrics.mask_distance_reductions(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(to_a), torch.from_numpy(to_b))
    for k in want:
        assert got[k].shape == (2,) and got[k].device == truth.device
        if k.startswith("n_") or k in ("hausdorff", "hd_percentile"):
            assert torch.equal(got[k].cpu(), want[k]), k          # counts, a maximum and an order statistic: no rounding of their own
        else:
            assert torch.allclose(got[k].cpu(), want[k], rtol=1e-12, atol=0), k          # f64 sums of at most 24^3 terms in two orders
    assert (got["assd"] > 0).all() and (got["hausdorff"] >= got["hd_percentile"]).all()

    step = 0.5 * min(h)
    points = phantom.centreline_points(ph["segments"], step)
    tol = math.sqrt(sum(x * x for x in h))
    cov = metrics.centreline_coverage(pred, bounds, points, threshold=pthr, tol=tol)
    ref_cov = metrics.coverage_reductions(torch.from_numpy(to_a), bounds, points, tol)
    for k in ref_cov:
        assert cov[k].shape == (2,)
        assert torch.allclose(cov[k].cpu().double(), ref_cov[k].double(), rtol=1e-12, atol=0), k
    assert (cov["n_outside"] == 0).all() and (cov["n_points"] > 100).all()


def test_identical_stacks_and_a_roll_by_one_node(dev, phantom24):
    """Identical stacks: exact zeros and coverage 1.  Rolled by one node along axis 0: every node of either mask has a node of the other
    exactly h_0 away, so the mean and the Hausdorff distance are positive and at most h_0 (rounded to f32 once, as the map is) -- while
    Dice only reports lost overlap (printed).  This is the property the distances exist for."""
    from nerfca_amd import metrics, phantom
    ph = phantom24
    bounds, truth = ph["bounds"], ph["dynamic"]
    thr = 0.25 * phantom.RHO_VESSEL
    h = [(b[1] - b[0]) / 23 for b in bounds]
    same = metrics.mask_distances(truth, truth.clone(), bounds, threshold=thr)
    for k in ("pred_to_truth", "truth_to_pred", "assd", "hausdorff", "hd_percentile"):
        assert (same[k] == 0).all(), k
    assert torch.equal(same["n_pred"], same["n_truth"]) and (same["n_pred"] > 0).all()
    points = phantom.centreline_points(ph["segments"], 0.5 * min(h))
    cov = metrics.centreline_coverage(truth, bounds, points, threshold=thr, tol=math.sqrt(sum(x * x for x in h)))
    assert (cov["coverage"] == 1.0).all() and (cov["mean_distance"] == 0).all() and (cov["n_outside"] == 0).all()          # (see the fixture)

    mask = truth > thr
    assert not mask[:, 0].any() and not mask[:, -1].any()          # nothing wraps around
    rolled = torch.roll(truth, shifts=1, dims=1)
    got = metrics.mask_distances(rolled, truth, bounds, threshold=thr)
    h0 = float(np.float32(h[0])) * (1 + 2.0 ** -23)          # the map is f32: h_0 rounded once
    for k in ("assd", "hausdorff", "hd_percentile", "pred_to_truth", "truth_to_pred"):
        assert (got[k] <= h0).all(), (k, got[k], h[0])
    assert (got["assd"] > 0).all() and (got["hausdorff"] > 0).all()
    dice = phantom.volume_errors(rolled, truth, thr)["dice"]
    print(f"rolled by one node: assd {got['assd'].tolist()} hausdorff {got['hausdorff'].tolist()} of h_0 = {h[0]:.5f}; Dice {dice:.3f}")
    assert dice < 1.0

    empty = torch.zeros_like(truth)
    none = metrics.mask_distances(empty, truth, bounds, threshold=thr)
    assert torch.isnan(none["assd"]).all() and torch.isnan(none["hausdorff"]).all() and (none["n_pred"] == 0).all() and torch.equal(none["n_truth"], same["n_truth"])
