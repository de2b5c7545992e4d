"""The numpy oracle of the soft skeleton and of the overlap sums (include/nerfca_hip.h, "skel"): the definition transcribed operation by
operation in f32, the neighbour order included, and the cases the CPU and the GPU tests share.  The published torch expression it is held
to as values lives here too (tests/test_skel_cpu.py)."""
import functools
import math

import numpy as np

ERODE_OFFSETS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))          # raster order
DILATE_OFFSETS = tuple((a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0))
SHAPES = ((2, 2, 2), (3, 3, 3), (4, 5, 6), (5, 9, 65), (7, 9, 70))
GPU_SHAPES = SHAPES + ((9, 17, 130),)


def _stencil(x, offsets, pad, take):
    """a = the centre, then a = take(a, b) for the neighbour b at every offset in order; nodes outside the grid hold `pad`, which no
    comparison ever takes.  x: f32 [..., n0, n1, n2]; every volume on its own."""
    assert x.dtype == np.float32 and x.ndim >= 3
    n0, n1, n2 = x.shape[-3:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 3) + [(1, 1)] * 3, constant_values=np.float32(pad))
    a = x.copy()
    for o0, o1, o2 in offsets:
        b = p[..., 1 + o0:1 + o0 + n0, 1 + o1:1 + o1 + n1, 1 + o2:1 + o2 + n2]
        a = take(a, b)
    return a


def erode(x):
    return _stencil(x, ERODE_OFFSETS, np.inf, lambda a, b: np.where(b < a, b, a))


def dilate(x):
    return _stencil(x, DILATE_OFFSETS, -np.inf, lambda a, b: np.where(b > a, b, a))


def relu(x):
    return np.where(x > 0, x, np.float32(0.0))


def soft_skeleton(x, iterations):
    """S of the definition for an f32 array [..., n0, n1, n2]; every operation one f32 operation."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):          # inf - inf and comparisons with a NaN
        e = x
        s = relu(e - dilate(erode(e)))
        for _ in range(iterations):
            e = erode(e)
            d = relu(e - dilate(erode(e)))
            s = s + relu(d - s * d)
    assert s.dtype == np.float32
    return s


def overlap_sums(a, b):
    """f64 [n_vol, 2]: (sum a b, sum a) per volume of two f32 stacks [n_vol, n0, n1, n2], the f64 products added exactly (math.fsum)."""
    out = np.zeros((a.shape[0], 2), dtype=np.float64)
    for v in range(a.shape[0]):
        x, y = a[v].astype(np.float64).ravel(), b[v].astype(np.float64).ravel()
        out[v] = math.fsum((x * y).tolist()), math.fsum(x.tolist())
    return out


def torch_soft_skeleton(x, iterations):
    """The published expression (Shit et al., clDice, soft_skeleton.py) on a torch f32 tensor [N, 1, n0, n1, n2]."""
    import torch
    import torch.nn.functional as F

    def soft_erode(img):
        p1 = -F.max_pool3d(-img, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        p2 = -F.max_pool3d(-img, (1, 3, 1), (1, 1, 1), (0, 1, 0))
        p3 = -F.max_pool3d(-img, (1, 1, 3), (1, 1, 1), (0, 0, 1))
        return torch.min(torch.min(p1, p2), p3)

    def soft_open(img):
        return F.max_pool3d(soft_erode(img), (3, 3, 3), (1, 1, 1), (1, 1, 1))

    skel = F.relu(x - soft_open(x))
    for _ in range(iterations):
        x = soft_erode(x)
        delta = F.relu(x - soft_open(x))
        skel = skel + F.relu(delta - skel * delta)
    return skel


# ----------------------------------------------------------------------------- inputs
def volume(shape, kind, seed=0):
    """f32 [n0, n1, n2].  "random": uniform in [0, 1); "binary": a mask filled to 60 %; "signed": values in [-1, 1) with exact zeros of both
    signs; "nan": random with a single NaN node; "faces": a binary mask that holds all six faces of the grid."""
    rng = np.random.default_rng(1000 * seed + 7 * shape[0] + 3 * shape[1] + shape[2] + len(kind))
    x = rng.random(shape).astype(np.float32)
    if kind == "random":
        return x
    if kind == "binary":
        return (x < 0.6).astype(np.float32)
    if kind == "signed":
        y = (2 * x - 1).astype(np.float32)
        z = rng.random(shape)
        y[z < 0.15] = 0.0
        y[z > 0.85] = -0.0
        return y
    if kind == "nan":
        x[tuple(s // 2 for s in shape)] = np.nan
        return x
    if kind == "faces":
        m = (x < 0.5).astype(np.float32)
        for a in range(3):
            idx = [slice(None)] * 3
            for end in (0, -1):
                idx[a] = end
                m[tuple(idx)] = 1.0
        return m
    raise ValueError(kind)


TUBE_SHAPE = (24, 24, 40)


def tube(radius, shift=0, length=None):
    """f32 mask of a straight tube of Euclidean radius `radius` nodes along axis 2 of a 24 x 24 x 40 grid, its axis at (12 + shift, 12);
    `length`: only the first `length` slices of axis 2."""
    i, j = np.meshgrid(np.arange(TUBE_SHAPE[0]), np.arange(TUBE_SHAPE[1]), indexing="ij")
    disc = ((i - 12 - shift) ** 2 + (j - 12) ** 2 <= radius * radius).astype(np.float32)
    m = np.repeat(disc[:, :, None], TUBE_SHAPE[2], axis=2)
    if length is not None:
        m[:, :, length:] = 0.0
    return np.ascontiguousarray(m)


def tube_axis(shift=0, length=TUBE_SHAPE[2]):
    m = np.zeros(TUBE_SHAPE, dtype=np.float32)
    m[12 + shift, 12, :length] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def thick_tree(side=64, radius=2.5):
    """(mask f32 [side]^3, centre bool [side]^3): the centreline of the seed-0 phantom tree (phase 0) on a grid of half-width 0.18,
    rasterised at the nearest node, and everything within `radius` nodes of it."""
    import scipy.ndimage
    from nerfca_amd import metrics, phantom
    hw = 0.18
    bounds = ((-hw, hw),) * 3
    seg = phantom.coronary_tree(1, seed=0, center=tuple(hw * c for c in phantom.HEART_CENTER), heart_radius=hw * phantom.HEART_RADIUS)
    pts = phantom.centreline_points(seg, 0.5 * 2 * hw / (side - 1))[0]
    idx, inside = metrics.nearest_nodes(pts, (side,) * 3, bounds)
    idx = idx[inside]
    centre = np.zeros((side,) * 3, dtype=bool)
    centre[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    mask = (scipy.ndimage.distance_transform_edt(~centre) <= radius).astype(np.float32)
    return mask, centre


@functools.lru_cache(maxsize=None)
def thick_tree_skeleton(iterations=4):
    return soft_skeleton(thick_tree()[0], iterations)
