"""The cubic-spline zoom on the GPU: nca_vol_spline_filter and nca_vol_zoom against the numpy transcription of their definition
(tests/resample_ref.py, held to scipy.ndimage in tests/test_resample_cpu.py), bit for bit in every case, and ccta.zoom / resample /
prepare_ccta(resample=...) on top of them.  Output buffers are pre-filled with NaN and workspaces with 0xff bytes, so a node the kernels did
not write shows.

Tile sizes of the kernels.  Prefilter: a workgroup stages sixteen lines; along axes 0 and 1 they are sixteen contiguous columns, along axis 2
sixteen consecutive rows.  (2,2,2): the initial sum is empty, one workgroup holds two volumes' rows; (3,5,70): a row crosses a wave, 15 rows
are one short of a tile; (17,33,5): 165 and 5 columns, uneven tiles on every axis; (2,3,300): 900 columns; 512 nodes along each axis in turn:
the longest line that is staged.  Interpolation: a workgroup is 256 consecutive output nodes."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.ndimage
import torch

from nca_testlib import dev, grid_of, gpu_stack_call, same_bits, ulp_distance  # noqa: F401

import filt_ref
import resample_ref as ref

pytestmark = pytest.mark.gpu


def gpu_filter(dev, vol):
    """coeff f64 of one nca_vol_spline_filter of a stack [n_vol,n0,n1,n2] into a buffer pre-filled with NaN."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    g = grid_of(vol.shape[1:])
    x = torch.tensor(vol).to(dev)
    out = torch.full(vol.shape, math.nan, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check_resample(lib.nca_vol_spline_filter(C.byref(g), _capi.ptr(x), vol.shape[0], _capi.ptr(out), fused._stream()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def gpu_zoom(dev, vol, m, order):
    """out f32 of one nca_vol_zoom of a stack into a buffer pre-filled with NaN (order 3) or with 12345 (order 0, which may carry a NaN), the
    workspace exactly as large as the query says and pre-filled with 0xff bytes; none at all at order 0."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    return gpu_stack_call(dev, _capi.check_resample, lib.nca_vol_zoom, lib.nca_vol_zoom_workspace, grid_of(np.shape(vol)[1:]), vol, ((C.c_int32 * 3)(*m), order),
                          math.nan if order == 3 else 12345.0, torch.float32, 8 if order == 3 else 0, out_shape=(np.shape(vol)[0],) + tuple(m), query_args=(order,))


def same_bits64(got, want):
    """nca_testlib.same_bits for the f64 coefficients."""
    return got.shape == want.shape and got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))


def ulps(got, want):
    return int(ulp_distance(got, want).max())


# (shape, output shape): factors above 1, below 1 and exactly 1 on different axes of one call wherever the shape allows
CASES = (((2, 2, 2), (5, 2, 3)), ((3, 3, 3), (2, 3, 7)), ((3, 5, 70), (3, 9, 41)), ((17, 33, 5), (12, 33, 8)), ((2, 3, 300), (3, 2, 300)),
         ((4, 3, 3), (188, 3, 3)),          # the overshoot pair: scipy's last plane is 0
         ((5, 6, 7), (2, 2, 2)))            # an output_shape with m = 2: the two end nodes


@pytest.mark.parametrize("shape,m", CASES, ids=lambda v: str(v))
def test_filter_and_zoom_bit_for_bit(dev, shape, m):
    """A stack of three volumes against the oracle, a second run (the same bits), and the volumes one by one (they are independent)."""
    stack = np.stack([ref.volume(shape, seed=s) for s in range(3)])
    want_c = ref.spline_filter(stack)
    got_c = gpu_filter(dev, stack)
    assert not np.isnan(got_c).any()
    assert same_bits64(got_c, want_c), ulps(got_c, want_c)
    assert same_bits64(gpu_filter(dev, stack), got_c)
    for order in (3, 0):
        want = ref.zoom(stack, m, order)
        got = gpu_zoom(dev, stack, m, order)
        assert not np.isnan(got).any() and not (got == 12345.0).any()
        assert same_bits(got, want), (order, ulps(got, want))
        assert same_bits(gpu_zoom(dev, stack, m, order), got)
        for k in range(3):
            assert same_bits(gpu_zoom(dev, stack[k:k + 1], m, order)[0], got[k]), (order, k)
    for k in range(3):
        assert same_bits64(gpu_filter(dev, stack[k:k + 1])[0], got_c[k]), k
    if shape == (4, 3, 3):
        assert ref.overshoots(4, 188) and same_bits(gpu_zoom(dev, stack, m, 0)[:, -1], stack[:, -1])


def test_the_longest_axis(dev):
    """512 nodes along each axis in turn, the others 2: the longest line the prefilter stages; 513 is refused by name."""
    from nerfca_amd import _capi, ccta
    for axis in range(3):
        shape = [2, 2, 2]
        shape[axis] = 512
        m = [3, 3, 3]
        m[axis] = 300
        stack = np.stack([ref.volume(tuple(shape), seed=s) for s in range(2)])
        got_c = gpu_filter(dev, stack)
        assert same_bits64(got_c, ref.spline_filter(stack)), (axis, ulps(got_c, ref.spline_filter(stack)))
        got = gpu_zoom(dev, stack, m, 3)
        assert same_bits(got, ref.zoom(stack, m, 3)), axis
        shape[axis] = 513
        x = torch.zeros(shape, device=dev)
        with pytest.raises(_capi.NcaError, match=rf"n\[{axis}\] = 513 is longer than NCA_EDT_MAX_AXIS"):
            ccta.spline_filter(x)
        with pytest.raises(_capi.NcaError, match=rf"n\[{axis}\] = 513 is longer than NCA_EDT_MAX_AXIS"):
            ccta.zoom(x, 1.0)
        assert ccta.zoom(x, 1.0, order=0).shape == tuple(shape)          # order 0 stages nothing


def test_order_0_carries_nan_and_infinity(dev):
    shape, m = (3, 5, 70), (6, 5, 33)
    vol = ref.volume(shape).copy()
    vol[0, 0, 0], vol[1, 2, 64], vol[2, 4, 69], vol[2, 4, 68] = np.nan, np.inf, -np.inf, np.float32(-0.0)
    want = ref.zoom(vol[None], m, 0)
    got = gpu_zoom(dev, vol[None], m, 0)
    assert same_bits(got, want)
    assert np.isnan(got[0, 0, 0, 0]) and np.isnan(got).sum() == np.isnan(want).sum() > 0 and np.isinf(got).sum() == np.isinf(want).sum() >= 2
    assert got[0, -1, -1, -1] == -np.inf


def zoom_bound(sci, vol):
    return np.spacing(np.abs(sci.astype(np.float32))).astype(np.float64) + ref.G_BOUND * float(np.abs(vol).max())


def test_zoom_against_scipy(dev):
    """ccta.zoom against scipy.ndimage.zoom directly, within one f32 step plus 2^-44 of the largest value, on size pairs scipy does not
    overshoot at; order 0 bit for bit; leading dimensions, output_shape and the refusals."""
    from nerfca_amd import _capi, ccta
    for shape, factors in ref.SCIPY_CASES:
        m = ref.out_shape(shape, factors)
        assert not any(ref.overshoots(n, k) for n, k in zip(shape, m))
        vols = np.stack([ref.volume(shape, seed=s) for s in range(2)])
        x = torch.from_numpy(vols).to(dev).requires_grad_()
        got = ccta.zoom(x, factors)
        assert got.shape == (2,) + m and got.dtype == torch.float32 and not got.requires_grad and got.device == x.device
        got0 = ccta.zoom(x, factors, order=0)
        for k in range(2):
            sci = scipy.ndimage.zoom(vols[k], factors, order=3)
            off = np.abs(got[k].cpu().numpy().astype(np.float64) - sci)
            assert (off <= zoom_bound(sci, vols[k])).all(), (shape, k, float(off.max()))
            assert same_bits(got0[k].cpu().numpy(), scipy.ndimage.zoom(vols[k], factors, order=0)), (shape, k)
        c = ccta.spline_filter(x)
        assert c.dtype == torch.float64 and c.shape == x.shape
        sci_c = scipy.ndimage.spline_filter(vols[1], 3, output=np.float64)
        assert np.abs(c[1].cpu().numpy() - sci_c).max() <= ref.G_BOUND * np.abs(vols[1]).max()
    shape, factors = ref.SCIPY_CASES[0]
    x = torch.from_numpy(np.stack([ref.volume(shape, seed=s) for s in range(6)])).to(dev)
    lead = ccta.zoom(x.reshape((2, 3) + shape), factors)
    assert lead.shape == (2, 3) + ref.out_shape(shape, factors) and torch.equal(lead.reshape((6,) + lead.shape[2:]).view(torch.int32), ccta.zoom(x, factors).view(torch.int32))
    one = ccta.zoom(x[0], factors)
    assert one.shape == ref.out_shape(shape, factors) and torch.equal(one, lead[0, 0])
    ends = ccta.zoom(x, 9.0, output_shape=(2, 2, 2))          # m = 2: the two end nodes of every axis
    corners = x[:, ::shape[0] - 1][:, :, ::shape[1] - 1][:, :, :, ::shape[2] - 1]
    assert ends.shape == (6, 2, 2, 2) and ((ends - corners).abs() <= torch.from_numpy(zoom_bound(corners.cpu().numpy(), x.cpu().numpy())).to(dev)).all()
    assert torch.equal(ccta.zoom(x, None, output_shape=(2, 2, 2), order=0), corners)
    with pytest.raises(_capi.NcaError, match="float32"):
        ccta.zoom(x.double(), 2.0)
    for bad in (1, 2, 5, True):
        with pytest.raises(_capi.NcaError, match="order"):
            ccta.zoom(x, 2.0, order=bad)
    with pytest.raises(_capi.NcaError, match="at least 2"):
        ccta.zoom(x, 0.2)
    with pytest.raises(_capi.NcaError, match="per axis"):
        ccta.zoom(x, (1.0, 2.0))


def test_resample_of_an_anisotropic_grid(dev):
    from nerfca_amd import ccta
    pred, _ = filt_ref.blobs()          # (16, 18, 40)
    h = (0.5, 0.4, 0.3)
    bounds = tuple((1.0, 1.0 + h[a] * (pred.shape[a] - 1)) for a in range(3))
    x = torch.from_numpy(pred).to(dev)
    got, new_bounds = ccta.resample(x, bounds, 0.25)
    fac = [((b[1] - b[0]) / (n - 1)) / 0.25 for b, n in zip(bounds, pred.shape)]
    m = tuple(int(round(n * f)) for n, f in zip(pred.shape, fac))
    assert got.shape == m and 31 <= m[0] <= 33 and 28 <= m[1] <= 30 and 47 <= m[2] <= 49 and got.dtype == torch.float32
    assert new_bounds == bounds          # end nodes map to end nodes
    assert same_bits(got.cpu().numpy(), ref.zoom(pred, m))
    per_axis, _ = ccta.resample(x, bounds, (0.25, 0.4, 0.6), order=0)
    assert per_axis.shape[1] in (17, 18, 19) and 19 <= per_axis.shape[2] <= 21
    assert same_bits(per_axis.cpu().numpy(), ref.zoom(pred, tuple(per_axis.shape), 0))
    # the corners of the grid stay where they were
    assert (got[0, 0, 0] - x[0, 0, 0]).abs() <= 2.0 ** -22 and (got[-1, -1, -1] - x[-1, -1, -1]).abs() <= 2.0 ** -22


# ----------------------------------------------------------------------------- the pipeline
CT_SHAPE, CT_SPACING = (12, 20, 35), (2.0, 1.2, 0.7)
CT_BOUNDS = tuple((0.0, (n - 1) * s) for n, s in zip(CT_SHAPE, CT_SPACING))


@pytest.fixture(scope="module")
def ct_case():
    """The reference restatement of the crossing tubes on the anisotropic grid, computed once."""
    m = ref.out_shape(CT_SHAPE, CT_SPACING)
    assert m == (24, 24, 24) and not any(ref.overshoots(n, k) for n, k in zip(CT_SHAPE, m))
    mask = ref.crossing_tubes(CT_SHAPE, CT_SPACING)
    rng = np.random.default_rng(5)
    hu = (rng.random(CT_SHAPE) * 1400 - 1000).astype(np.float32)
    labels = np.zeros(CT_SHAPE, dtype=np.int64)
    labels[1:5, 3:12, 5:15] = 51
    labels[7:11, 5:15, 18:30] = 52
    full, vessel, closed, dist, mask_f, labels_f = ref.prepare_ccta_resampled_ref(hu, mask, CT_SPACING, labels, 52, 51)
    return hu, mask, labels, full, vessel, closed, dist, mask_f, labels_f


def test_prepare_ccta_with_resampling_against_the_reference_restatement(dev, ct_case):
    """resample=1.0 against preprocess_ccta.py:54-130 with :57-60, in scipy calls.  The closed mask is equal: the tubes of
    resample_ref.crossing_tubes are placed so that no node of the resampled segmentation is within the zoom bound of 0.5, the value at which
    the rounding of the reference's integer mask flips, and no node of the resampled labels within it of a half (both asserted below).
    The volume: the reference zooms the attenuation in f64, the library rounds it to f32 first (an error of at most 2^-24 A, A the largest
    attenuation), zooms and rounds again, so outside the mask it is within
        27 2^-24 A      the input's rounding through the prefilter, whose impulse response sqrt(3) z^|k| sums to sqrt(3) (1 + |z|) / (1 - |z|)
                        = 3 in absolute value per axis, and then through B-spline weights, which are non-negative and sum to 1
        + 2^-24 R       the f32 rounding of a result of at most R
        + 2^-44 A       the prefilter's distance from scipy's (the zoom bound),
    and inside it within filt_ref.contrast_bound.  The aorta's fill is a mean over the same nodes of values within that bound."""
    from nerfca_amd import ccta
    hu, mask, labels, full, vessel, closed, dist, mask_f, labels_f = ct_case
    margin = min(np.abs(np.abs(mask_f) - 0.5).min(), np.abs(labels_f - np.floor(labels_f) - 0.5).min())
    assert margin > 2.0 ** -14, margin          # far outside one f32 step of a label (2^-18 at 52) plus the G bound: no node may flip
    assert 0 < closed.sum() < closed.size and 2.0 < dist.max()

    def t(a):
        return torch.from_numpy(np.array(a)).to(dev)

    out = ccta.prepare_ccta(t(hu), t(mask), CT_BOUNDS, labels=t(labels), aorta_label=52, heart_label=51, resample=1.0)
    assert out["static"].shape == out["dynamic"].shape == out["mask"].shape == (24, 24, 24) and out["bounds"] == CT_BOUNDS
    got_closed = out["mask"].cpu().numpy()
    differ = np.argwhere(got_closed != closed)
    assert len(differ) == 0, differ[:10].tolist()
    total = (out["static"].double() + out["dynamic"].double()).cpu().numpy()
    att_in = float(np.abs(hu.astype(np.float64) / 1000 * (0.1494 * 2.5e-2 - 0.0430 * 2.5e-2) + 0.1494 * 2.5e-2).max())
    bound_out = 27 * 2.0 ** -24 * att_in + 2.0 ** -24 * float(np.abs(full[~closed]).max()) + ref.G_BOUND * att_in
    bound_in = filt_ref.contrast_bound(float(dist.max()))
    err_out, err_in = float(np.abs(total - full)[~closed].max()), float(np.abs(total - full)[closed].max())
    print(f"prepare_ccta(resample=1): outside the mask {err_out:.3e} (bound {bound_out:.3e}), inside {err_in:.3e} (bound {bound_in:.3e})")
    assert err_out <= bound_out and err_in <= bound_in
    assert float(np.abs(out["dynamic"].cpu().numpy() - vessel).max()) <= bound_in
    # label_order=0 invents no label: the resampled mask is a subset of nodes of the input's values, and the result differs from order 3
    near = ccta.prepare_ccta(t(hu), t(mask), CT_BOUNDS, labels=t(labels), aorta_label=52, heart_label=51, resample=1.0, label_order=0)
    assert near["mask"].shape == (24, 24, 24) and near["mask"].any() and not torch.equal(near["mask"], out["mask"])
    # without a spacing: today's path on the input grid
    plain = ccta.prepare_ccta(t(hu), t(mask), CT_BOUNDS)
    assert plain["static"].shape == CT_SHAPE
