"""The numpy oracle of nca_vol_spline_filter and nca_vol_zoom (include/nerfca_hip.h, "resample"), and the restatement of the reference's
CCTA pipeline with its resampling, in scipy calls.

`spline_filter` and `interp` are the definition, operation by operation: every numpy operation below is one rounded f64 operation on whole
arrays, in the order the header writes them; a line is walked node by node, vectorised over the lines.  `zoom` chains them and rounds to
f32 once.  tests/test_resample_cpu.py holds the interpolation to scipy.ndimage bit for bit and the prefilter to it within 2^-44 of the
largest value; the GPU tests compare the library with this file bit for bit.

Deliberately not scipy's: `cc = min(o step, n - 1)`.  scipy writes cval = 0 into the whole last plane of an axis when (m - 1) step lands one
ulp above n - 1 (`overshoots`); here the last output node is the last input node.  Also the volumes both test files share."""
import functools
import math

import numpy as np
import scipy.ndimage

import filt_ref

Z = math.sqrt(3.0) - 2.0
GAIN = (1 - Z) * (1 - 1 / Z)

# (shape, zoom factors) of the cases the definition was checked at against scipy; none overshoots (asserted by the tests)
SCIPY_CASES = (((5, 6, 7), (1.5, 0.8, 2.0)), ((3, 9, 70), (3, 0.625, 0.5)), ((2, 2, 2), (2.5, 3, 1)), ((17, 4, 33), (0.7, 1, 1.3)), ((40, 12, 9), (0.33, 2.2, 1.7)))
G_BOUND = 2.0 ** -44          # of max|vol|: the prefilter against scipy.ndimage.spline_filter


def zn_of(n):
    """z multiplied by z another n - 2 times: no pow."""
    zn = Z
    for _ in range(n - 2):
        zn = zn * Z
    return zn


def out_shape(shape, factors):
    """scipy's output shape: int(round(n zoom)) with Python's round."""
    return tuple(int(round(n * f)) for n, f in zip(shape, factors))


def step_of(n, m):
    return (n - 1) / (m - 1)


def overshoots(n, m):
    """Does scipy's coordinate of the last output node, (m - 1) step, land above n - 1 (and its last plane become cval = 0)?"""
    return float(m - 1) * step_of(n, m) > float(n - 1)


def filter_axis(c, axis):
    """The prefilter along one axis of an f64 array, for every line at once; returns a new array."""
    c = np.moveaxis(np.array(c, dtype=np.float64), axis, 0)
    n = c.shape[0]
    zn = zn_of(n)
    c = c * GAIN
    s = c[0] + zn * c[n - 1]
    zi = Z
    for i in range(1, n - 1):
        s = s + zi * (c[i] + zn * c[n - 1 - i])
        zi = zi * Z
    c[0] = s / (1 - zn * zn)
    for i in range(1, n):
        c[i] = c[i] + Z * c[i - 1]
    c[n - 1] = ((Z * c[n - 2] + c[n - 1]) * Z) / (Z * Z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])
    return np.ascontiguousarray(np.moveaxis(c, 0, axis))


def spline_filter(vol):
    """What nca_vol_spline_filter writes for the f32 stack vol [..., n0, n1, n2]: f64 of the same shape."""
    vol = np.asarray(vol, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = vol.astype(np.float64)
        for a in range(3):
            c = filter_axis(c, c.ndim - 3 + a)
    return c


def mirror(j, n):
    p = 2 * (n - 1)
    m = np.mod(j, p)
    return np.where(m > n - 1, p - m, m)


def coords(n, m):
    return np.minimum(np.arange(m).astype(np.float64) * step_of(n, m), float(n - 1))


def cubic_taps(n, m):
    """(taps int64 [m, 4], weights f64 [m, 4]) of one axis at order 3."""
    cc = coords(n, m)
    f = np.floor(cc)
    y = cc - f
    t = 1 - y
    w1 = (y * y * (y - 2) * 3 + 4) / 6
    w2 = (t * t * (t - 2) * 3 + 4) / 6
    w0 = t * t * t / 6
    w3 = 1 - w0 - w1 - w2
    j = f.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :]
    return mirror(j, n), np.stack([w0, w1, w2, w3], axis=1)


def nearest_taps(n, m):
    return np.floor(coords(n, m) + 0.5).astype(np.int64)


def interp(c, m, order):
    """The interpolation stage for one array [n0, n1, n2] (f64 coefficients at order 3, any dtype at order 0): [m0, m1, m2], in f64 before
    the rounding at order 3, in c's dtype at order 0."""
    n = c.shape
    if order == 0:
        return c[np.ix_(*[nearest_taps(n[a], m[a]) for a in range(3)])]
    assert order == 3
    (j0, w0), (j1, w1), (j2, w2) = [cubic_taps(n[a], m[a]) for a in range(3)]
    acc = np.zeros(tuple(m), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k0 in range(4):
            for k1 in range(4):
                for k2 in range(4):
                    v = c[np.ix_(j0[:, k0], j1[:, k1], j2[:, k2])]
                    acc = acc + ((v * w0[:, k0, None, None]) * w1[None, :, k1, None]) * w2[None, None, :, k2]
    return acc


def zoom(vol, m, order=3):
    """What nca_vol_zoom writes for the f32 stack vol [..., n0, n1, n2] and the output shape m: f32 [..., m0, m1, m2]."""
    vol = np.asarray(vol, dtype=np.float32)
    flat = vol.reshape((-1,) + vol.shape[-3:])
    with np.errstate(all="ignore"):
        out = np.stack([interp(spline_filter(v) if order == 3 else v, m, order).astype(np.float32) for v in flat])
    return out.reshape(vol.shape[:-3] + tuple(m))


def volume(shape, seed=0):
    """f32 [n0, n1, n2]: normal data x 100, the scale the prefilter's distance from scipy was measured at."""
    rng = np.random.default_rng([7, seed, *shape])
    return (rng.standard_normal(shape) * 100).astype(np.float32)


@functools.lru_cache(maxsize=None)
def zoom_case(shape, m, order, seed=0):
    """(vol, expected f32) of one shared case; computed once, callers leave both unchanged."""
    vol = volume(shape, seed)
    want = zoom(vol, m, order)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


# ----------------------------------------------------------------------------- the reference's pipeline with its resampling, in scipy calls
def prepare_ccta_resampled_ref(raw_hu, mask, spacing, labels=None, aorta=None, heart=None, mu_water=0.1494 * 2.5e-2, mu_air=0.0430 * 2.5e-2):
    """preprocess_ccta.py:54-130 for one volume, :57-60 included: the segmentations are integer arrays there, which scipy's zoom rounds half
    away from zero; after :61 every distance counts in unit nodes.  (f64 full volume, f64 contrast volume, bool closed mask, f64 distance
    map, f64 resampled mask and labels before the rounding)."""
    raw = raw_hu.astype(np.float64) / 1000          # :7-12
    raw *= mu_water - mu_air
    raw += mu_water
    mask_i = scipy.ndimage.zoom((mask > 0).astype(np.int64), spacing)          # :58
    mask_f = scipy.ndimage.zoom((mask > 0).astype(np.float64), spacing)
    raw = scipy.ndimage.zoom(raw, spacing)                                     # :59
    labels_f = None
    if labels is not None:
        total = scipy.ndimage.zoom(labels.astype(np.int64), spacing)           # :60
        labels_f = scipy.ndimage.zoom(labels.astype(np.float64), spacing)
        raw[total == aorta] = np.mean(raw[total == heart])                     # :64
    vessel, closed, dist = filt_ref.vessel_contrast_ref(mask_i)
    full = np.zeros(raw.shape)
    full[~closed] = raw[~closed]          # :128-130
    full[closed] = vessel[closed]
    return full, vessel, closed, dist, mask_f, labels_f


def crossing_tubes(shape=(12, 20, 35), spacing=(2.0, 1.2, 0.7)):
    """A vessel segmentation of two crossing tubes on an anisotropic grid, f32 0 / 1: one along axis 2, one slanting across it; radii in
    world units."""
    idx = np.indices(shape).astype(np.float64)
    x = [idx[a] * spacing[a] for a in range(3)]
    ext = [(shape[a] - 1) * spacing[a] for a in range(3)]
    a = (x[0] - ext[0] / 2) ** 2 + (x[1] - ext[1] / 2) ** 2 <= 2.6 ** 2
    t = x[2] / ext[2]
    b = (x[0] - (5 + t * (ext[0] - 10))) ** 2 + (x[1] - (ext[1] - 5 - t * (ext[1] - 10))) ** 2 <= 2.3 ** 2
    b &= (idx[2] >= 4) & (idx[2] <= shape[2] - 5)
    return (a | b).astype(np.float32)
