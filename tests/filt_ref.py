"""The numpy oracle of nca_vol_smooth and nca_vol_cityblock (include/nerfca_hip.h, "filt"), and the restatement of the reference's CCTA
pipeline in scipy calls.

`smooth` is the definition of the filter, operation by operation: f64, axes 0, 1, 2 in turn, the `reflect` boundary, the pairs summed
outermost first, one rounding to f32.  `cityblock_brute` is the definition of the city-block distance, the minimum over all features (tiny
grids only); `cityblock` is the separable form the kernels use.  tests/test_filt_cpu.py holds the two to each other and all of it to
scipy.ndimage bit for bit; the GPU tests compare with `smooth` and `cityblock`.

`vessel_contrast_ref` and `prepare_ccta_ref` restate preprocess/preprocess_ccta.py:88-120 and :54-130 of the reference (without the
resampling of :56-61) with the scipy calls those lines make.  Also the volumes both test files share."""
import functools

import numpy as np
import scipy.ndimage

NONE = 0x7fffffff
# (shape, sigma, radius) of the cases the definition was checked at against scipy
SMOOTH_CASES = (((3, 5, 70), 1, 2), ((2, 3, 4), (1.5, 0.7, 2), (6, 3, 8)), ((9, 4, 130), (1, 0, 2.5), (4, 0, 10)), ((5, 6, 7), 8, 32))
CITY_SHAPES = ((4, 5, 6), (7, 9, 70), (3, 3, 3), (6, 8, 10))
FILLS = (0.02, 0.3, 0.97)
XP = (0, 1, 2, 4, 5)
FP = (0, 0.2, 0.5, 0.75, 1)


# ----------------------------------------------------------------------------- smoothing
def per_axis(v):
    return list(v) if isinstance(v, (tuple, list)) else [v] * 3


def half_weights(sigma, radius):
    """scipy's numbers (_gaussian_kernel1d at order 0), written out: the half x = 0 .. r of phi / sum(phi); [1.0] for an axis scipy skips."""
    if not sigma > 1e-15:
        return np.ones(1)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[radius:].copy()


def reflect(j, n):
    m = np.mod(j, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def smooth_axis(x, axis, w):
    """One axis of the definition on an f64 array: acc = x[i] w[0]; for k = r .. 1: acc += (x[R(i-k)] + x[R(i+k)]) w[k]."""
    r = len(w) - 1
    n = x.shape[axis]
    i = np.arange(n)
    acc = x * w[0]
    for k in range(r, 0, -1):
        acc = acc + (np.take(x, reflect(i - k, n), axis=axis) + np.take(x, reflect(i + k, n), axis=axis)) * w[k]
    return acc


def smooth(vol, sigma, radius):
    """What nca_vol_smooth writes for the f32 stack vol [..., n0, n1, n2]: f32 of the same shape."""
    vol = np.asarray(vol, dtype=np.float32)
    ws = [half_weights(float(s), int(r)) for s, r in zip(per_axis(sigma), per_axis(radius))]
    x = vol.astype(np.float64)
    for a in range(3):
        x = smooth_axis(x, x.ndim - 3 + a, ws[a])
    return x.astype(np.float32)


def smooth_volume(shape, seed=0):
    rng = np.random.default_rng([seed, *shape])
    return (rng.standard_normal(shape) * 3 + rng.random(shape)).astype(np.float32)


# ----------------------------------------------------------------------------- the city-block distance
def features(vol, threshold, invert):
    with np.errstate(invalid="ignore"):
        return (np.asarray(vol).astype(np.float64) > threshold) != bool(invert)


def border_term(shape):
    """min over the axes of min(i_a + 1, n_a - i_a): the distance to the nearest node just outside the grid."""
    idx = np.indices(shape)
    return np.min([np.minimum(idx[a] + 1, shape[a] - idx[a]) for a in range(3)], axis=0)


def cityblock_brute(feat, border):
    """The definition: the minimum over all features of |d0| + |d1| + |d2| (int64 [n0,n1,n2]); tiny grids only."""
    shape = feat.shape
    out = np.full(feat.size, NONE, dtype=np.int64)
    f = np.argwhere(feat).astype(np.int64)
    if len(f):
        nodes = np.stack(np.unravel_index(np.arange(feat.size), shape), axis=1).astype(np.int64)
        out = np.abs(nodes[:, None, :] - f[None, :, :]).sum(axis=2).min(axis=1)
    out = out.reshape(shape)
    return np.minimum(out, border_term(shape)) if border else out


def _line_min(f, axis, border):
    """min_j (|i - j| + f(j)) along `axis` of the int64 array f, NONE never added to; with the axis's own border term."""
    n = f.shape[axis]
    f = np.moveaxis(f, axis, -1)
    i = np.arange(n, dtype=np.int64)
    d = np.abs(i[:, None] - i[None, :])                                     # [i, j]
    cand = np.where(f[..., None, :] == NONE, NONE, f[..., None, :] + d)      # [..., i, j]
    out = cand.min(axis=-1)
    if border:
        out = np.minimum(out, np.minimum(i + 1, n - i))
    return np.moveaxis(out, -1, axis)


def cityblock_separable(feat, border):
    n2 = feat.shape[2]
    i = np.arange(n2, dtype=np.int64)
    d = np.abs(i[:, None] - i[None, :])
    g = np.where(feat[:, :, None, :], d[None, None], NONE).min(axis=3)       # the row distance
    if border:
        g = np.minimum(g, np.minimum(i + 1, n2 - i))
    return _line_min(_line_min(g, 1, border), 0, border)


def cityblock(vol, threshold, invert=0, border=0):
    """What nca_vol_cityblock writes for the f32 stack vol [..., n0, n1, n2]: int32 of the same shape."""
    vol = np.asarray(vol)
    flat = vol.reshape((-1,) + vol.shape[-3:])
    out = np.stack([cityblock_separable(features(v, threshold, invert), border) for v in flat])
    return out.reshape(vol.shape).astype(np.int32)


def mask_volume(shape, fill, seed=0):
    """f32 [n0,n1,n2]: about `fill` of the nodes are > 0.5; the values on both sides of the threshold vary."""
    rng = np.random.default_rng([seed, *shape, int(round(fill * 1000))])
    low = (rng.random(shape) * 0.4).astype(np.float32)
    high = (0.6 + rng.random(shape) * 0.4).astype(np.float32)
    return np.where(rng.random(shape) < fill, high, low)


@functools.lru_cache(maxsize=None)
def city_case(shape, fill, invert, border):
    """(vol, expected int32) of one shared case; computed once, callers leave both unchanged."""
    vol = mask_volume(shape, fill)
    want = cityblock(vol, 0.5, invert, border)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def dilate(mask, n):
    return cityblock_separable(mask, 0) <= n


def erode(mask, n):
    return cityblock_separable(~mask, 1) > n


def border_of(mask):
    return mask & (cityblock_separable(~mask, 1) == 1)


# ----------------------------------------------------------------------------- the reference's pipeline in scipy calls
def vessel_contrast_ref(mask, spacing=(1, 1, 1), grow=3, shrink=1, sigma=1, radius=2, xp=XP, fp=FP, contrast=0.05):
    """preprocess_ccta.py:88-120 for one volume: (f64 contrast volume, bool closed mask, f64 distance map before smoothing)."""
    closed = scipy.ndimage.binary_erosion(scipy.ndimage.binary_dilation(mask > 0, iterations=grow).astype("int"), iterations=shrink).astype("int")          # :90
    dist = scipy.ndimage.distance_transform_edt(closed, sampling=np.array(spacing, dtype=np.float64))                                                         # :91
    smooth_d = scipy.ndimage.gaussian_filter(dist, sigma=sigma, radius=radius)                                                                                  # :96
    value = np.interp(smooth_d, np.array(xp, dtype=np.float64), np.array(fp, dtype=np.float64) * contrast)                                                      # :110-113
    out = np.zeros(mask.shape)
    out[closed > 0] = value[closed > 0]                                                                                                                         # :79, :120
    return out, closed > 0, dist


def prepare_ccta_ref(raw_hu, mask, labels=None, aorta=None, heart=None, mu_water=0.1494 * 2.5e-2, mu_air=0.0430 * 2.5e-2, **kw):
    """preprocess_ccta.py:54-130 for one volume, without the resampling of :56-61: (f64 full volume, f64 contrast volume, bool closed mask)."""
    raw = raw_hu.astype(np.float64) / 1000          # :7-12
    raw *= mu_water - mu_air
    raw += mu_water
    if labels is not None:
        raw[labels == aorta] = np.mean(raw[labels == heart])          # :64
    vessel, closed, dist = vessel_contrast_ref(mask, **kw)
    full = np.zeros(raw.shape)
    full[~closed] = raw[~closed]          # :128-130
    full[closed] = vessel[closed]
    return full, vessel, closed, dist


def contrast_bound(d_max, xp=XP, fp=FP, contrast=0.05):
    """s 2^-24 d_max + 2^-24 max(fp) contrast: the two f32 roundings the device pipeline makes and the reference does not (the distance map
    and the result), the first carried through the transfer function by its largest slope s."""
    s = max(abs(b - a) * contrast / (q - p) for a, b, p, q in zip(fp, fp[1:], xp, xp[1:]))
    return s * 2.0 ** -24 * d_max + 2.0 ** -24 * max(fp) * contrast


@functools.lru_cache(maxsize=None)
def tubes(shape=(24, 20, 70)):
    """A vessel segmentation of two crossing tubes, f32 0 / 1: one along axis 2, one slanting across it."""
    idx = np.indices(shape).astype(np.float64)
    c0, c1 = (shape[0] - 1) / 2, (shape[1] - 1) / 2
    a = (idx[0] - c0) ** 2 + (idx[1] - c1) ** 2 <= 1.5 ** 2
    t = idx[2] / (shape[2] - 1)
    b = (idx[0] - (4 + t * (shape[0] - 9))) ** 2 + (idx[1] - (shape[1] - 5 - t * (shape[1] - 10))) ** 2 <= 1.2 ** 2
    b &= (idx[2] >= 6) & (idx[2] <= shape[2] - 8)
    out = (a | b).astype(np.float32)
    out.setflags(write=False)
    return out


def blobs(shape=(16, 18, 40), seed=0):
    """(pred, truth) f32 volumes of two overlapping blobs each, thresholded at 0.5 by the tests."""
    idx = np.indices(shape).astype(np.float64)

    def ball(c, r):
        return sum(((idx[a] - c[a]) / r[a]) ** 2 for a in range(3)) <= 1.0

    truth = ball((7, 8, 14), (4.2, 5.1, 8.3)) | ball((9, 10, 27), (3.1, 3.4, 6.2))
    pred = ball((8, 8, 15), (3.6, 5.4, 7.1)) | ball((9, 11, 28), (3.3, 2.9, 5.2))
    rng = np.random.default_rng(seed)
    lo, hi = rng.random(shape) * 0.4, 0.6 + rng.random(shape) * 0.4
    return np.where(pred, hi, lo).astype(np.float32), np.where(truth, hi, lo).astype(np.float32)


def surface_distances_ref(pred_mask, truth_mask, spacing, percentile=95.0):
    """MedPy's __surface_distances (connectivity 1) both ways, restated with scipy: the counts of border nodes, the two directed sets of
    distances (f64, sorted) and from them assd, the Hausdorff distance and the larger directed percentile (rank 'higher')."""
    a = pred_mask ^ scipy.ndimage.binary_erosion(pred_mask, structure=scipy.ndimage.generate_binary_structure(3, 1), iterations=1)
    b = truth_mask ^ scipy.ndimage.binary_erosion(truth_mask, structure=scipy.ndimage.generate_binary_structure(3, 1), iterations=1)
    to_b = scipy.ndimage.distance_transform_edt(~b, sampling=spacing)
    to_a = scipy.ndimage.distance_transform_edt(~a, sampling=spacing)
    ab, ba = np.sort(to_b[a]), np.sort(to_a[b])

    def higher(d):
        return float(d[int(np.ceil(percentile / 100.0 * (d.size - 1)))])

    return {"n_pred": int(a.sum()), "n_truth": int(b.sum()), "pred_to_truth": float(ab.mean()), "truth_to_pred": float(ba.mean()),
            "assd": float((ab.sum() + ba.sum()) / (ab.size + ba.size)), "hausdorff": float(max(ab[-1], ba[-1])), "hd_percentile": max(higher(ab), higher(ba)),
            "border_pred": a, "border_truth": b}
