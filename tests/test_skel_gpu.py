"""The soft skeleton and clDice on the GPU: nca_vol_softskel against the numpy transcription of its definition (tests/skel_ref.py, held to
the published torch expression in tests/test_skel_cpu.py) bit for bit in every case, nca_vol_overlap_sums against exact sums, and
metrics.soft_skeleton / metrics.cldice on top of them.  Output buffers are pre-filled with NaN and the workspace with 0xff bytes, so a node
the kernels did not write shows.

The kernel's tile is 4 x 8 x 64 nodes with a halo of two.  (2,2,2), (3,3,3), (4,5,6): one tile, every halo node outside the grid;
(5,9,65): one node past a tile on every axis, so every face of a tile has a neighbour tile of one node; (7,9,70): likewise with more than
the halo past the tile; (9,17,130): three tiles along every axis, a tile with neighbours on both sides.  Every stack has two volumes that
differ, so a halo read across the volume boundary shows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev, grid_of, gpu_stack_call, same_bits  # noqa: F401

import skel_ref as ref

pytestmark = pytest.mark.gpu

KINDS = ("random", "binary", "signed", "nan", "faces")


def gpu_softskel(dev, vol, K):
    """out f32 of one nca_vol_softskel of a stack [n_vol,n0,n1,n2] into a buffer pre-filled with NaN, the workspace exactly as large as the
    query says (and itself pre-filled, with 0xff bytes)."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    return gpu_stack_call(dev, _capi.check_skel, lib.nca_vol_softskel, lib.nca_vol_softskel_workspace, grid_of(np.shape(vol)[1:]), vol, (int(K),), math.nan, torch.float32, 8)


def gpu_overlap_sums(dev, a, b):
    """sums f64 [n_vol, 2] of one nca_vol_overlap_sums, into a buffer pre-filled with NaN, the workspace as large as the query says and
    pre-filled with 0xff bytes."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    g = grid_of(a.shape[1:])
    n_vol = a.shape[0]
    x, y = torch.tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev), torch.tensor(np.ascontiguousarray(b, dtype=np.float32)).to(dev)
    sums = torch.full((n_vol, 2), math.nan, dtype=torch.float64, device=dev)
    nbytes = lib.nca_vol_overlap_sums_workspace(C.byref(g), n_vol)
    assert nbytes >= 16 * n_vol * ((a[0].size + 4095) // 4096) and nbytes % 256 == 0
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check_skel(lib.nca_vol_overlap_sums(C.byref(g), _capi.ptr(x), _capi.ptr(y), n_vol, _capi.ptr(sums), _capi.ptr(work), nbytes, fused._stream()))
    torch.cuda.synchronize(dev)
    return sums.cpu().numpy()


# ----------------------------------------------------------------------------- the raw skeleton
@pytest.mark.parametrize("shape", ref.GPU_SHAPES, ids=str)
def test_softskel_bit_for_bit(dev, shape):
    """Two volumes that differ, every kind of input, K = 0, 1, 2, 5: the oracle's bits; a second run; the second volume alone."""
    for kind in KINDS:
        # (the smallest grids are all faces: there the second volume is another mask)
        stack = np.stack([ref.volume(shape, kind, seed=0), ref.volume(shape, "binary" if kind == "faces" else kind, seed=1)])
        assert not np.array_equal(stack[0], stack[1], equal_nan=True)
        for K in (0, 1, 2, 5):
            want = ref.soft_skeleton(stack, K)
            got = gpu_softskel(dev, stack, K)
            assert not np.isnan(got).any(), (kind, K)          # relu takes a NaN to +0: nothing unwritten, nothing passed through
            assert same_bits(got, want), (kind, K, int((got.view(np.int32) != want.view(np.int32)).sum()))
        assert same_bits(gpu_softskel(dev, stack, 5), got), kind
        assert same_bits(gpu_softskel(dev, stack[1:2], 5)[0], got[1]), kind


def test_softskel_of_tubes_and_a_full_volume(dev):
    for r in (1, 2, 3.5):
        assert same_bits(gpu_softskel(dev, ref.tube(r)[None], 4)[0], ref.tube_axis()), r
    assert not gpu_softskel(dev, ref.tube(2)[None], 1).any()
    assert same_bits(gpu_softskel(dev, ref.tube(3.5)[None], 40), gpu_softskel(dev, ref.tube(3.5)[None], 10))
    assert not gpu_softskel(dev, np.ones((1, 5, 9, 65), dtype=np.float32), 3).any()          # the faces do not erode


# ----------------------------------------------------------------------------- the raw sums
@pytest.mark.parametrize("shape", [(4, 5, 6), (9, 17, 130)], ids=str)
@pytest.mark.parametrize("n_vol", [1, 3])
def test_overlap_sums(dev, shape, n_vol):
    a = np.stack([ref.volume(shape, "binary", seed=s) for s in range(n_vol)])
    b = np.stack([ref.volume(shape, "faces", seed=s + 5) for s in range(n_vol)])
    got = gpu_overlap_sums(dev, a, b)
    want = ref.overlap_sums(a, b)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))          # whole numbers: exact in any order
    assert (want[:, 0] > 0).all() and (want[:, 0] < want[:, 1]).all()
    a = np.stack([ref.volume(shape, "signed", seed=s) for s in range(n_vol)])
    b = np.stack([ref.volume(shape, "random", seed=s + 5) for s in range(n_vol)])
    got, want = gpu_overlap_sums(dev, a, b), ref.overlap_sums(a, b)
    N = a[0].size
    for v in range(n_vol):          # any order of N additions against the exact sum: N 2^-53 of the sum of the absolute terms
        x, y = a[v].astype(np.float64).ravel(), b[v].astype(np.float64).ravel()
        bound_ab, bound_a = N * 2.0 ** -53 * math.fsum(np.abs(x * y).tolist()), N * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
        print(f"{shape} volume {v}: |sum ab - exact| = {abs(got[v, 0] - want[v, 0]):.3e} (bound {bound_ab:.3e}), |sum a - exact| = {abs(got[v, 1] - want[v, 1]):.3e} (bound {bound_a:.3e})")
        assert abs(got[v, 0] - want[v, 0]) <= bound_ab and abs(got[v, 1] - want[v, 1]) <= bound_a
    again = gpu_overlap_sums(dev, a, b)
    assert np.array_equal(again.view(np.int64), got.view(np.int64))
    if n_vol > 1:          # every volume on its own
        assert np.array_equal(gpu_overlap_sums(dev, a[1:2], b[1:2]).view(np.int64), got[1:2].view(np.int64))
    same = gpu_overlap_sums(dev, a, a)          # a stack against itself
    assert (same[:, 0] > 0).all() and np.array_equal(same[:, 1], got[:, 1])


# ----------------------------------------------------------------------------- the Python layer
def test_soft_skeleton_and_cldice_of_tubes(dev):
    from nerfca_amd import metrics
    K = 4
    whole, cut, near, far = (torch.from_numpy(m).to(dev) for m in (ref.tube(2), ref.tube(2, length=20), ref.tube(2, shift=2), ref.tube(2, shift=7)))
    s = metrics.soft_skeleton(whole, K)
    assert s.dtype == torch.float32 and s.shape == whole.shape and s.device == whole.device and not s.requires_grad
    assert same_bits(s.cpu().numpy(), ref.tube_axis())
    sc = metrics.soft_skeleton(cut, K).cpu().numpy()
    assert sc.sum() == 18 and sc[12, 12, :].sum() == 18
    # with a threshold the input is the mask: of the f32 volume, of twelve times it, and of a bool mask
    for x, thr in ((whole, 0.5), (12.0 * whole, 3.0), (whole > 0, None), (whole > 0, 0.5)):
        assert torch.equal(metrics.soft_skeleton(x, K, threshold=thr), s)
    got = metrics.cldice(whole, whole, iterations=K)
    assert set(got) == {"cldice", "tprec", "tsens"} and all(v.dtype == torch.float64 and v.shape == () and v.device == whole.device for v in got.values())
    assert float(got["cldice"]) == float(got["tprec"]) == float(got["tsens"]) == 1.0
    got = metrics.cldice(whole, near, iterations=K)
    assert float(got["cldice"]) == float(got["tprec"]) == float(got["tsens"]) == 1.0
    got = metrics.cldice(whole, far, iterations=K)
    assert float(got["cldice"]) == float(got["tprec"]) == float(got["tsens"]) == 0.0
    got = metrics.cldice(cut, whole, iterations=K)
    assert float(got["tprec"]) == 1.0 and float(got["tsens"]) == 0.5 and abs(float(got["cldice"]) - 2.0 / 3.0) <= 4 * 2.0 ** -53
    # thresholds: the prediction at a value of its own
    got = metrics.cldice(5.0 * cut, 12.0 * whole, iterations=K, threshold=3.0, pred_threshold=1.0)
    assert float(got["tprec"]) == 1.0 and float(got["tsens"]) == 0.5
    got = metrics.cldice(5.0 * cut, 12.0 * whole, iterations=K, threshold=6.0)          # nothing of the prediction is above 6: an empty skeleton
    assert math.isnan(float(got["tprec"])) and float(got["tsens"]) == 0.0 and math.isnan(float(got["cldice"]))
    got = metrics.cldice(5.0 * cut, 12.0 * whole, iterations=K, threshold=6.0, smooth=1.0)
    assert float(got["tprec"]) == 1.0 and float(got["tsens"]) == 1.0 / 41.0
    # the soft clDice of a volume that is not binary with itself is below 1
    soft = metrics.cldice(0.5 * whole, 0.5 * whole, iterations=K)
    assert float(soft["tprec"]) == 0.5 and float(soft["cldice"]) == 0.5
    with pytest.raises(metrics._capi.NcaError, match="one shape"):
        metrics.cldice(whole, whole[:-1], iterations=K)
    with pytest.raises(metrics._capi.NcaError, match="pred_threshold"):
        metrics.cldice(whole, whole, iterations=K, pred_threshold=0.5)
    with pytest.raises(metrics._capi.NcaError, match="iterations"):
        metrics.soft_skeleton(whole, 513)
    with pytest.raises(metrics._capi.NcaError, match="float32"):
        metrics.soft_skeleton(whole.double(), K)
    with pytest.raises(metrics._capi.NcaError, match="nan"):
        metrics.soft_skeleton(whole, K, threshold=math.nan)


def test_the_thick_tree_and_leading_shapes(dev):
    from nerfca_amd import metrics
    mask, _ = ref.thick_tree()
    want = ref.thick_tree_skeleton(4)
    x = torch.from_numpy(mask).to(dev)
    assert same_bits(metrics.soft_skeleton(x, 4).cpu().numpy(), want)
    got = metrics.cldice(x, x, iterations=4, threshold=0.5)
    assert float(got["cldice"]) == 1.0
    # a leading shape [2, 3, n0, n1, n2], and an input that is not contiguous
    shape = (7, 9, 70)
    vols = np.stack([ref.volume(shape, "random", seed=s) for s in range(6)]).reshape((2, 3) + shape)
    v = torch.from_numpy(vols).to(dev)
    s = metrics.soft_skeleton(v, 3)
    assert s.shape == v.shape and same_bits(s.cpu().numpy(), ref.soft_skeleton(vols, 3))
    wide = torch.zeros((2, 3) + (7, 9, 140), device=dev)
    wide[..., ::2] = v
    strided = wide[..., ::2]
    assert not strided.is_contiguous() and torch.equal(metrics.soft_skeleton(strided, 3), s)
    other = torch.from_numpy(np.stack([ref.volume(shape, "random", seed=s + 9) for s in range(6)]).reshape((2, 3) + shape)).to(dev)
    got = metrics.cldice(strided, other, iterations=3)
    want = metrics.cldice_reductions(torch.from_numpy(ref.soft_skeleton(vols, 3)), torch.from_numpy(vols), torch.from_numpy(ref.soft_skeleton(other.cpu().numpy(), 3)), other.cpu())
    for k in ("cldice", "tprec", "tsens"):
        assert got[k].shape == (2, 3) and got[k].dtype == torch.float64
        # each of the four sums of N = 4410 non-negative terms is within N 2^-53 of the exact one, relatively, in any order; a quotient of
        # two doubles that, the harmonic mean of two quotients (all at most 1) doubles it again
        assert float((got[k].cpu() - want[k]).abs().max()) <= 8 * 4410 * 2.0 ** -53, k
    flat = metrics.cldice(v.reshape((6,) + shape), other.reshape((6,) + shape), iterations=3)
    assert all(torch.equal(flat[k].reshape(2, 3), got[k]) for k in got)          # the same bits whatever the leading shape
