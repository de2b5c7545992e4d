"""Connected components on the GPU: nca_vol_label against the numpy oracle of its definition (tests/label_ref.py, held to
scipy.ndimage.label in tests/test_label_cpu.py) with np.array_equal on labels and counts in every case, nca_vol_label_sizes against
np.bincount, and metrics.label / component_sizes / keep_largest / component_report on top of them.  Output buffers are pre-filled with
0x7f7f7f7f and the workspace with 0xff bytes, so a node the kernels did not write shows.

The kernel's tile is 4 x 8 x 64 nodes.  (2,2,2), (3,3,3), (4,5,6): one tile; (5,9,65), (7,9,70): seams of one node and more on every axis;
(9,17,130): three tiles along every axis, a tile with neighbours on both sides.  Every stack has two volumes that differ, and the second is
also run alone, so a union across the volume boundary shows."""
import ctypes as C

import numpy as np
import pytest
import scipy.ndimage
import torch

from nca_testlib import dev, grid_of  # noqa: F401

import label_ref as ref

pytestmark = pytest.mark.gpu

POISON = 0x7f7f7f7f


def gpu_label(dev, vol, threshold, connectivity, invert=False):
    """(labels int32, counts int32) of one nca_vol_label of a stack [n_vol,n0,n1,n2] into buffers pre-filled with 0x7f7f7f7f, the workspace
    exactly as large as the query says and pre-filled with 0xff bytes."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    n_vol = vol.shape[0]
    g = grid_of(vol.shape[1:])
    x = torch.tensor(vol).to(dev)
    labels = torch.full(vol.shape, POISON, dtype=torch.int32, device=dev)
    counts = torch.full((n_vol,), POISON, dtype=torch.int32, device=dev)
    nbytes = lib.nca_vol_label_workspace(C.byref(g), n_vol)
    assert 4 * vol.size <= nbytes <= 4 * vol.size + 256 + 4 * n_vol * ((vol[0].size + 1023) // 1024) + 256 and nbytes % 256 == 0
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check_label(lib.nca_vol_label(C.byref(g), _capi.ptr(x), n_vol, float(threshold), int(connectivity), 1 if invert else 0, _capi.ptr(labels),
                                            _capi.ptr(counts), _capi.ptr(work), nbytes, fused._stream()))
    torch.cuda.synchronize(dev)
    return labels.cpu().numpy(), counts.cpu().numpy()


def gpu_sizes(dev, labels, cap):
    """sizes int32 [n_vol, cap] of one nca_vol_label_sizes, into a buffer pre-filled with 0x7f7f7f7f: the entry point zeroes it itself."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    g = grid_of(labels.shape[1:])
    x = torch.tensor(labels).to(dev)
    sizes = torch.full((labels.shape[0], cap), POISON, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _capi.check_label(lib.nca_vol_label_sizes(C.byref(g), _capi.ptr(x), labels.shape[0], cap, _capi.ptr(sizes), fused._stream()))
    torch.cuda.synchronize(dev)
    return sizes.cpu().numpy()


# ----------------------------------------------------------------------------- the raw labels
@pytest.mark.parametrize("shape", ref.GPU_SHAPES, ids=str)
def test_label_equals_the_oracle(dev, shape):
    """Two volumes that differ, every mask, connectivity 1, 2 and 3: the oracle's labels and counts; a second run; the second volume alone."""
    for name, stack, thr, inv in ref.cases(shape):
        for conn in ref.CONNECTIVITIES:
            want_l, want_c = ref.expected(shape, name, conn)
            got_l, got_c = gpu_label(dev, stack, thr, conn, inv)
            assert got_l.dtype == np.int32 and got_c.dtype == np.int32
            assert np.array_equal(got_c, want_c), (name, conn, got_c.tolist(), want_c.tolist())
            assert np.array_equal(got_l, want_l), (name, conn, int((got_l != want_l).sum()))
            again_l, again_c = gpu_label(dev, stack, thr, conn, inv)
            assert np.array_equal(again_l, got_l) and np.array_equal(again_c, got_c), (name, conn)
            alone_l, alone_c = gpu_label(dev, stack[1:2], thr, conn, inv)
            assert np.array_equal(alone_l[0], got_l[1]) and alone_c[0] == got_c[1], (name, conn)


# ----------------------------------------------------------------------------- the raw sizes
@pytest.mark.parametrize("shape", [(4, 5, 6), (9, 17, 130)], ids=str)
def test_label_sizes_against_bincount(dev, shape):
    for name, conn in (("random 0.3", 1), ("random 0.7", 3), ("checkerboard", 1), ("empty", 1), ("full", 2), ("serpentine", 1)):
        labels, counts = ref.expected(shape, name, conn)
        top = int(counts.max())
        for cap in sorted({1, 2, max(1, top // 2), top + 1, top + 7}):          # also a cap below the count: the labels from cap on are not counted
            got = gpu_sizes(dev, labels, cap)
            assert got.dtype == np.int32 and np.array_equal(got, ref.sizes(labels, cap)), (name, cap)
            for v in range(2):
                want = np.bincount(labels[v].ravel(), minlength=max(cap, top + 1))[:cap]
                assert np.array_equal(got[v], want), (name, cap, v)
    # labels the kernel did not make: more distinct labels than the table in LDS has slots, labels that share a slot, and negative ones
    rng = np.random.default_rng(5)
    wild = rng.integers(-3, 1500, size=(2,) + shape).astype(np.int32)
    wild[1] = (wild[1] % 3) * 256          # 0, 256 and 512 share a slot
    for cap in (1, 300, 513, 1500):
        assert np.array_equal(gpu_sizes(dev, wild, cap), ref.sizes(wild, cap)), cap


# ----------------------------------------------------------------------------- the Python layer
def test_metrics_label_against_scipy(dev):
    from nerfca_amd import metrics
    shape = (7, 9, 70)
    vols = np.stack([ref.random_volume(shape, s) for s in range(6)]).reshape((2, 3) + shape)
    v = torch.from_numpy(vols).to(dev)
    for conn in (1, 2, 3):
        structure = scipy.ndimage.generate_binary_structure(3, conn)
        labels, counts = metrics.label(v, threshold=0.6, connectivity=conn)
        assert labels.dtype == torch.int32 and labels.shape == v.shape and labels.device == v.device
        assert counts.dtype == torch.int64 and counts.shape == (2, 3) and counts.device == v.device
        for i in range(2):
            for j in range(3):
                want_l, want_c = scipy.ndimage.label(vols[i, j] > 0.6, structure)
                assert int(counts[i, j]) == want_c and np.array_equal(labels[i, j].cpu().numpy(), want_l), (conn, i, j)
        inv_l, inv_c = metrics.label(v, threshold=0.6, connectivity=conn, invert=True)
        want_l, want_c = scipy.ndimage.label(~(vols[1, 2] > 0.6), structure)
        assert int(inv_c[1, 2]) == want_c and np.array_equal(inv_l[1, 2].cpu().numpy(), want_l)
    # the default is scipy's: 6 neighbours
    labels, counts = metrics.label(v[0, 0], threshold=0.6)
    want_l, want_c = scipy.ndimage.label(vols[0, 0] > 0.6)
    assert counts.shape == () and int(counts) == want_c and np.array_equal(labels.cpu().numpy(), want_l)
    # a bool mask, and an input that is not contiguous
    mask = v > 0.6
    bl, bc = metrics.label(mask, threshold=0.5, connectivity=3)
    fl, fc = metrics.label(v, threshold=0.6, connectivity=3)
    assert torch.equal(bl, fl) and torch.equal(bc, fc)
    wide = torch.zeros((2, 3) + (7, 9, 140), device=dev)
    wide[..., ::2] = v
    strided = wide[..., ::2]
    sl, sc = metrics.label(strided, threshold=0.6, connectivity=3)
    assert not strided.is_contiguous() and torch.equal(sl, fl) and torch.equal(sc, fc)
    # sizes: one column more than the largest count, zeros past a volume's own count
    sizes = metrics.component_sizes(fl, fc)
    assert sizes.dtype == torch.int64 and sizes.shape == (2, 3, int(fc.max()) + 1) and sizes.device == v.device
    for i in range(2):
        for j in range(3):
            want = np.bincount(fl[i, j].cpu().numpy().ravel(), minlength=sizes.shape[-1])
            assert np.array_equal(sizes[i, j].cpu().numpy(), want) and not sizes[i, j, int(fc[i, j]) + 1:].any()
    none_l, none_c = metrics.label(torch.zeros((2,) + shape, device=dev), threshold=0.5)
    none = metrics.component_sizes(none_l, none_c)
    assert none_c.tolist() == [0, 0] and none.shape == (2, 1) and none.tolist() == [[7 * 9 * 70]] * 2          # no component at all: a single column
    with pytest.raises(metrics._capi.NcaError, match="nan"):
        metrics.label(v, threshold=float("nan"))
    with pytest.raises(metrics._capi.NcaError, match="connectivity"):
        metrics.label(v, threshold=0.5, connectivity=4)
    with pytest.raises(metrics._capi.NcaError, match="float32"):
        metrics.label(v.double(), threshold=0.5)


def test_the_phantom_tree_with_planted_specks(dev):
    from nerfca_amd import metrics
    tree, speckled, n_specks = ref.tree_with_specks()
    side = ref.TREE_SIDE
    bounds = ((0.0, side - 1.0),) * 3
    t, s = torch.from_numpy(tree).to(dev), torch.from_numpy(speckled).to(dev)
    labels, counts = metrics.label(s, threshold=0.5, connectivity=3)
    assert int(counts) == 1 + n_specks
    sizes = metrics.component_sizes(labels, counts)
    assert sizes.shape == (2 + n_specks,) and int(sizes.sum()) == side ** 3 and int(sizes[0]) == side ** 3 - int(speckled.sum())
    assert sorted(sizes[1:].tolist()) == [1] * n_specks + [int(tree.sum())]
    kept = metrics.keep_largest(s, threshold=0.5)
    assert kept.dtype == torch.bool and kept.shape == s.shape and torch.equal(kept, t > 0.5)          # k = 1 returns exactly the tree
    assert torch.equal(metrics.keep_largest(s > 0.5, 1, threshold=0.5), kept)          # a bool mask
    assert torch.equal(metrics.keep_largest(s, 1 + n_specks, threshold=0.5), s > 0.5) and torch.equal(metrics.keep_largest(s, 99, threshold=0.5), s > 0.5)
    assert torch.equal(metrics.keep_largest(s, threshold=0.5, min_size=2), kept) and torch.equal(metrics.keep_largest(s, threshold=0.5, min_size=1), s > 0.5)
    two = metrics.keep_largest(s, 2, threshold=0.5)          # the specks tie at one node: the one that comes first in raster order
    first = np.argwhere((speckled > 0.5) & ~(tree > 0.5))[0]
    assert int(two.sum()) == int(tree.sum()) + 1 and bool(two[tuple(first)])
    report = metrics.component_report(s, t, threshold=0.5)
    assert set(report) == {"components_pred", "components_truth", "betti0_error", "largest_share_pred", "largest_share_truth"}
    assert all(v.shape == () and v.device == s.device for v in report.values())
    assert int(report["components_pred"]) == 1 + n_specks and int(report["components_truth"]) == 1 and int(report["betti0_error"]) == n_specks
    assert float(report["largest_share_truth"]) == 1.0 and float(report["largest_share_pred"]) == float(tree.sum()) / float(speckled.sum())
    # a stack, a threshold of the prediction's own, and an empty truth
    pair = metrics.component_report(torch.stack([5.0 * s, 5.0 * t]), torch.stack([t, torch.zeros_like(t)]), threshold=0.5, pred_threshold=2.5)
    assert pair["betti0_error"].tolist() == [n_specks, 1] and pair["components_pred"].tolist() == [1 + n_specks, 1] and pair["components_truth"].tolist() == [1, 0] and bool(torch.isnan(pair["largest_share_truth"][1]))
    # the Hausdorff distance is decided by the farthest speck: 0 once they are gone
    raw = metrics.mask_distances(s, t, bounds, threshold=0.5)
    clean = metrics.mask_distances(kept.to(torch.float32), t, bounds, threshold=0.5)
    assert float(raw["hausdorff"]) >= 3.0 and float(clean["hausdorff"]) == 0.0 and float(clean["assd"]) == 0.0
    with pytest.raises(metrics._capi.NcaError, match="one shape"):
        metrics.component_report(s, t[:-1], threshold=0.5)
    with pytest.raises(metrics._capi.NcaError, match="both given"):
        metrics.keep_largest(s, 2, threshold=0.5, min_size=2)


def test_nothing_existing_changed(dev):
    """metrics.cldice and metrics.mask_distances give the same bits before and after the new entry points have run."""
    from nerfca_amd import metrics
    shape = (7, 9, 70)
    a = torch.from_numpy(np.stack([ref.random_volume(shape, s) for s in (0, 1)])).to(dev)
    b = torch.from_numpy(np.stack([ref.random_volume(shape, s) for s in (2, 3)])).to(dev)
    bounds = ((0.0, 1.0), (0.0, 2.0), (-1.0, 1.0))

    def existing():
        c = metrics.cldice(a, b, iterations=3, threshold=0.5)
        d = metrics.mask_distances(a, b, bounds, threshold=0.5)
        return {**{"c_" + k: v.clone() for k, v in c.items()}, **{"d_" + k: v.clone() for k, v in d.items()}}

    before = existing()
    labels, counts = metrics.label(a, threshold=0.5, connectivity=3)
    metrics.component_sizes(labels, counts)
    metrics.keep_largest(a, threshold=0.5)
    after = existing()
    assert set(before) == set(after) and len(before) == 10
    for k in before:
        x, y = before[k].cpu().numpy(), after[k].cpu().numpy()
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
