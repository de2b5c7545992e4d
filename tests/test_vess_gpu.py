"""The Hessian vesselness on the GPU: nca_vol_hessian_eig and nca_vol_hessian_norm_max against the numpy transcription of their definition
(tests/vess_ref.py, held to LAPACK and to the plain scipy expression in tests/test_vess_cpu.py) bit for bit, nca_vol_vesselness against it
to one f32 step (only exp can differ, by a unit of f64) with exact zeros, the merge over scales, and ccta.hessian_eigenvalues /
ccta.vesselness on top of them.  Output buffers are pre-filled with NaN (int32: -7), so a node the kernel did not write shows.

The kernel's tile is 4 x 8 x 64 nodes with a halo of one.  The shapes are those of the soft skeleton's tests: (2,2,2), (3,3,3), (4,5,6): one
tile, every halo node outside the grid; (5,9,65), (7,9,70): one node and more past a tile on every axis; (9,17,130): three tiles along every
axis.  Every stack has two volumes that differ, so a halo read across the volume boundary shows."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from nca_testlib import dev, grid_of, same_bits, ulp_distance  # noqa: F401

import skel_ref
import vess_ref as ref

pytestmark = pytest.mark.gpu

SCALE = 2.25          # sigma = 1.5


def _launch(dev, name, shape, x, *args):
    from nerfca_amd import _capi, fused
    g = grid_of(shape)
    with torch.cuda.device(dev):
        _capi.check_vess(getattr(_capi.lib(), name)(C.byref(g), _capi.ptr(x), x.shape[0], *args, fused._stream()))
    torch.cuda.synchronize(dev)


def _dev(dev, a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def gpu_eig(dev, stack, scale):
    x = _dev(dev, stack)
    out = torch.full((stack.shape[0], 3) + stack.shape[1:], math.inf, dtype=torch.float32, device=dev)          # (a NaN is a legitimate result here)
    _launch(dev, "nca_vol_hessian_eig", stack.shape[1:], x, float(scale), out.data_ptr())
    return out.cpu().numpy()


def gpu_norm_max(dev, stack, scale):
    x = _dev(dev, stack)
    out = torch.full((stack.shape[0],), math.nan, dtype=torch.float64, device=dev)
    _launch(dev, "nca_vol_hessian_norm_max", stack.shape[1:], x, float(scale), out.data_ptr())
    return out.cpu().numpy()


def gpu_vess(dev, stack, scale, c, bright=True, scale_index=0, stored=None, with_index=True, alpha=0.5, beta=0.5):
    """(V, index) of one nca_vol_vesselness; `stored`: (V, index) the buffers hold before the call (default NaN and -7)."""
    x = _dev(dev, stack)
    out = torch.full(stack.shape, math.nan, dtype=torch.float32, device=dev) if stored is None else _dev(dev, stored[0])
    idx = None
    if with_index:
        idx = torch.full(stack.shape, -7, dtype=torch.int32, device=dev) if stored is None else _dev(dev, stored[1], np.int32)
    cd = _dev(dev, np.broadcast_to(np.asarray(c, dtype=np.float64), (stack.shape[0],)), np.float64)
    _launch(dev, "nca_vol_vesselness", stack.shape[1:], x, float(scale), alpha, beta, cd.data_ptr(), 1 if bright else 0, scale_index, out.data_ptr(),
            None if idx is None else idx.data_ptr())
    return out.cpu().numpy(), None if idx is None else idx.cpu().numpy()


def close_with_exact_zeros(got, want, tag):
    """+0 bit for bit wherever the transcription is 0, within one f32 step elsewhere."""
    assert got.shape == want.shape and got.dtype == np.float32, tag
    zero = want == 0
    assert not got.view(np.int32)[zero].any(), (tag, "a node that must be +0 is not")
    assert not np.isnan(got).any(), (tag, "a node was not written")
    steps = ulp_distance(got, want)
    assert steps.max() <= 1, (tag, float(steps.max()), int((steps > 1).sum()))
    return int((steps > 0).sum())


def stack_of(shape, kind):
    stack = np.stack([ref.volume(shape, kind, seed=0), ref.volume(shape, kind, seed=1)])
    assert not np.array_equal(stack[0], stack[1], equal_nan=True)
    return stack


# ----------------------------------------------------------------------------- the raw entry points
@pytest.mark.parametrize("shape", skel_ref.GPU_SHAPES, ids=str)
def test_eigenvalues_and_norm_max_bit_for_bit(dev, shape):
    for kind in ref.KINDS:
        stack = stack_of(shape, kind)
        want = ref.eigenvalues(stack, SCALE)
        got = gpu_eig(dev, stack, SCALE)
        assert not np.isinf(got).any() or kind == "nonfinite", kind          # nothing unwritten
        assert same_bits(got, want), (kind, int((got.view(np.int32) != want.view(np.int32)).sum()))
        assert same_bits(gpu_eig(dev, stack, SCALE), got), kind
        assert same_bits(gpu_eig(dev, stack[1:2], SCALE)[0], got[1]), kind
        if kind == "nonfinite" and min(shape) > 3:
            assert np.isnan(got).any() and not np.isnan(got).all()
        m_want = ref.norm_max(stack, SCALE)
        m = gpu_norm_max(dev, stack, SCALE)
        assert m.dtype == np.float64 and np.array_equal(m.view(np.int64), m_want.view(np.int64)), (kind, m, m_want)
        assert np.array_equal(gpu_norm_max(dev, stack, SCALE).view(np.int64), m.view(np.int64)), kind
        assert np.array_equal(gpu_norm_max(dev, stack[1:2], SCALE).view(np.int64), m[1:2].view(np.int64)), kind
        assert (m > 0).all() or kind == "constant" or (kind == "nonfinite" and min(shape) <= 4), kind          # (a tiny grid is all stencil of the NaN)


@pytest.mark.parametrize("shape", skel_ref.GPU_SHAPES, ids=str)
def test_vesselness_of_one_scale(dev, shape):
    for kind in ref.KINDS:
        stack = stack_of(shape, kind)
        frangi = 0.5 * np.sqrt(ref.norm_max(stack, SCALE))          # one c per volume
        for bright in (True, False):
            for c in (frangi, 0.0):
                want = ref.vesselness_scale(stack, SCALE, 0.5, 0.5, c, bright)
                got, idx = gpu_vess(dev, stack, SCALE, c, bright)
                off = close_with_exact_zeros(got, want, (kind, bright))
                assert not idx.any(), (kind, "scale_index 0 writes 0 into every node")
                assert (got > 0).any() or kind == "constant" or max(shape) <= 3, (kind, bright)
        again, _ = gpu_vess(dev, stack, SCALE, 0.0, False, with_index=False)          # a second run, without the index buffer
        assert same_bits(again, got), kind
        alone, _ = gpu_vess(dev, stack[1:2], SCALE, 0.0, False)
        assert same_bits(alone[0], got[1]), kind
        print(f"{shape} {kind}: {off} nodes one step from the transcription")
    # other alpha and beta
    stack = stack_of(shape, "random")
    got, _ = gpu_vess(dev, stack, SCALE, 0.1, alpha=0.3, beta=0.8)
    close_with_exact_zeros(got, ref.vesselness_scale(stack, SCALE, 0.3, 0.8, 0.1), "alpha, beta")


@pytest.mark.parametrize("shape", skel_ref.GPU_SHAPES[2:], ids=str)
def test_merge_over_scales_and_the_scale_index(dev, shape):
    """Three scales of one stack, smoothed on the host.  The index must equal the transcription's wherever its best value leads the second
    best by more than one f32 step (the device is within one step of it at every scale).  Where the transcription is 0 at
    every scale the device is +0 at every scale (asserted above and here), nothing is ever greater, and the index is 0 on both sides: such
    ties are not exempt.  Exempt are only the nodes with a positive best value within one step of the second best; fewer than 1 %."""
    sigmas = (1.0, 1.5, 2.0)
    for kind in ("random", "binary", "signed"):
        stack = stack_of(shape, kind)
        smoothed = [ref.smooth(stack, s) for s in sigmas]
        per_scale = [ref.vesselness_scale(s, sig * sig, 0.5, 0.5, 0.05) for s, sig in zip(smoothed, sigmas)]
        want, want_idx = ref.merge(per_scale)
        stored = None
        for i, (s, sig) in enumerate(zip(smoothed, sigmas)):
            stored = gpu_vess(dev, s, sig * sig, 0.05, scale_index=i, stored=stored)
        got, idx = stored
        close_with_exact_zeros(got, want, kind)
        ranked = np.sort(np.stack(per_scale), axis=0)
        exempt = (ranked[-1] > 0) & (ulp_distance(ranked[-1], ranked[-2]) <= 1)
        print(f"{shape} {kind}: {int(exempt.sum())} of {exempt.size} nodes exempt, indices used {np.unique(idx).tolist()}")
        assert exempt.mean() < 0.01
        assert np.array_equal(idx[~exempt], want_idx[~exempt]), kind
        assert idx.min() >= 0 and idx.max() <= 2 and len(np.unique(idx)) > 1


def test_merge_keeps_the_larger_value_and_the_smaller_index(dev):
    shape = (7, 9, 70)
    stack = stack_of(shape, "random")
    first = gpu_vess(dev, stack, SCALE, 0.1)
    assert (first[0] > 0).any() and (first[0] == 0).any()
    # the same scale again as scale_index 1: a tie at every node, nothing is replaced
    V, idx = gpu_vess(dev, stack, SCALE, 0.1, scale_index=1, stored=first)
    assert same_bits(V, first[0]) and not idx.any()
    # over zeros: every positive node is replaced, a zero node keeps its index
    zeros = (np.zeros(stack.shape, dtype=np.float32), np.full(stack.shape, 5, dtype=np.int32))
    V, idx = gpu_vess(dev, stack, SCALE, 0.1, scale_index=1, stored=zeros)
    assert same_bits(V, first[0]) and np.array_equal(idx, np.where(first[0] > 0, 1, 5))
    # over ones: nothing is greater
    ones = (np.ones(stack.shape, dtype=np.float32), np.full(stack.shape, 5, dtype=np.int32))
    V, idx = gpu_vess(dev, stack, SCALE, 0.1, scale_index=3, stored=ones)
    assert (V == 1).all() and (idx == 5).all()
    # half of the stored values above, half below
    half = np.where(np.indices(stack.shape).sum(axis=0) % 2 == 0, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    V, idx = gpu_vess(dev, stack, SCALE, 0.1, scale_index=2, stored=(half, np.zeros(stack.shape, dtype=np.int32)))
    assert same_bits(V, np.maximum(half, first[0])) and np.array_equal(idx, np.where(first[0] > half, 2, 0))
    V, none = gpu_vess(dev, stack, SCALE, 0.1, scale_index=2, stored=(half, None), with_index=False)          # without the index buffer
    assert none is None and same_bits(V, np.maximum(half, first[0]))


# ----------------------------------------------------------------------------- the Python layer
def test_tube_ball_and_slab_through_the_python_layer(dev):
    from nerfca_amd import ccta
    h = ref.SIDE // 2
    got = {}
    for name, mask in (("tube", ref.tube()), ("ball", ref.ball()), ("slab", ref.slab()), ("negated tube", -ref.tube())):
        V, idx = ccta.vesselness(torch.from_numpy(mask).to(dev), ref.MEANING_SIGMAS, c=ref.MEANING_C, return_scale=True)
        assert V.dtype == torch.float32 and idx.dtype == torch.int32 and V.shape == idx.shape == (ref.SIDE,) * 3 and V.device == idx.device and not V.requires_grad
        got[name] = V.cpu().numpy(), idx.cpu().numpy()
        want, want_idx = ref.meaning(name)
        close_with_exact_zeros(got[name][0], want, name)
    V, idx = got["tube"]
    assert float(V[h, h, :].min()) > float(got["ball"][0].max()) > 0
    assert abs(float(V[h, h, :].min()) - 0.247) < 1e-3 and abs(float(got["ball"][0].max()) - 0.094) < 1e-3
    assert not got["slab"][0].any() and not got["negated tube"][0].any()
    d, interior = ref.tube_distance()
    assert not V[(d >= 5) & interior].any()
    assert (idx[h, h, :] == 1).all()


def test_frangi_c_bright_and_dark_return_scale_and_leading_shapes(dev):
    from nerfca_amd import ccta
    shape = (7, 9, 70)
    vols = np.stack([ref.volume(shape, "random", seed=s) for s in range(6)]).reshape((2, 3) + shape)
    v = torch.from_numpy(vols).to(dev)
    sigmas = (1.0, 2.0)
    # the eigenvalues: the transcription's bits on the volume smoothed by scipy
    e = ccta.hessian_eigenvalues(v, 2.0)
    assert e.shape == (2, 3, 3) + shape and e.dtype == torch.float32
    assert same_bits(e.cpu().numpy(), ref.eigenvalues(ref.smooth(vols, 2.0), 4.0))
    # c=None is the call with c = 0.5 sqrt(max (l1^2 + l2^2) + l3^2) of hessian_eigenvalues, per volume and scale
    one = v[1, 2]
    for sigma in sigmas:
        l = ccta.hessian_eigenvalues(one, sigma).double()
        c = float(0.5 * torch.sqrt(((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]).max()))
        assert c > 0 and torch.equal(ccta.vesselness(one, (sigma,)), ccta.vesselness(one, (sigma,), c=c)), sigma
    # the whole call against the transcription, Frangi's c per volume and scale
    V, idx = ccta.vesselness(v, sigmas, return_scale=True)
    want, want_idx = ref.vesselness(vols, sigmas)
    assert V.shape == idx.shape == v.shape
    close_with_exact_zeros(V.cpu().numpy(), want, "leading shape")
    assert (idx.cpu().numpy() != want_idx).mean() < 0.01 and set(np.unique(idx.cpu().numpy()).tolist()) == {0, 1}
    assert torch.equal(ccta.vesselness(v, sigmas), V)          # a second run, without return_scale
    assert torch.equal(ccta.vesselness(one, sigmas), V[1, 2])          # every volume on its own, its own c included
    assert torch.equal(ccta.vesselness(v.reshape((6,) + shape), sigmas).reshape(v.shape), V)
    wide = torch.zeros((2, 3) + (7, 9, 140), device=dev)
    wide[..., ::2] = v
    assert not wide[..., ::2].is_contiguous() and torch.equal(ccta.vesselness(wide[..., ::2], sigmas), V)
    # dark tubes of -x are the bright tubes of x, bit for bit
    dark, dark_idx = ccta.vesselness(-v, sigmas, bright=False, return_scale=True)
    assert torch.equal(dark, V) and torch.equal(dark_idx, idx)
    assert not torch.equal(ccta.vesselness(v, sigmas, bright=False), V)
    # c = 0 drops the norm factor: at least as large everywhere
    assert bool((ccta.vesselness(v, sigmas, c=0.0) >= V).all())
    for call in (lambda: ccta.vesselness(v, ()), lambda: ccta.vesselness(v, (1.0, -1.0)), lambda: ccta.vesselness(v, sigmas, c=-1.0), lambda: ccta.vesselness(v, sigmas, c=math.inf),
                 lambda: ccta.vesselness(v, sigmas, alpha=0.0), lambda: ccta.vesselness(v.double(), sigmas), lambda: ccta.vesselness(v, (9.0,)),
                 lambda: ccta.hessian_eigenvalues(v, 0.0)):
        with pytest.raises(ccta._capi.NcaError):
            call()
