"""The numpy oracle of nca_vol_edt (include/nerfca_hip.h, "edt"), written two ways: `brute` is the definition, the minimum over all features
of q(i, j) = w_0 d_0^2 + (w_1 d_1^2 + w_2 d_2^2), every operation one rounded f64 operation in that order; `separable` is the form the kernels
use (row distance g, then the minimum along axis 1, then along axis 0).  tests/test_edt_cpu.py holds the two to each other bit for bit and
to scipy; the GPU tests compare with `edt`.  Also the volumes both test files share."""
import functools

import numpy as np

INF = np.inf
NONE = np.iinfo(np.int64).max
ANISO = (1 / 0.37, 1 / 0.11, 1 / 0.29)          # inv per axis
UNIT = (1.0, 1.0, 1.0)
# (2,2,2): the smallest grid.  (3,5,64) / (3,5,65): one chunk of the row pass and one node past it.  (5,9,130): two chunk carries.
# The line kernel takes tiles of 16 columns and 16 nodes along the line per step: (3,17,18) is one past both along axis 1 (columns: 18 of
# axis 2), (17,3,6) one past both along axis 0 (columns: the 18 of a plane).
SHAPES = ((2, 2, 2), (3, 5, 64), (3, 5, 65), (5, 9, 130), (3, 17, 18), (17, 3, 6))
PATTERNS = ("corner", "last_chunk", "d0.002", "d0.05", "d0.5", "none", "all")
THRESHOLD = 0.5


def weights(inv):
    """w_a = h_a h_a with h_a = 1 / inv_a, each one rounded f64 operation."""
    h = [1.0 / float(v) for v in inv]
    return [x * x for x in h]


def spacing(inv):
    return [1.0 / float(v) for v in inv]


def features(vol, threshold, invert):
    with np.errstate(invalid="ignore"):
        return (np.asarray(vol).astype(np.float64) > threshold) != bool(invert)


def brute(feat, inv):
    """min over features of q, f64 [n0,n1,n2]; +inf without a feature."""
    w = weights(inv)
    shape = feat.shape
    out = np.full(feat.size, INF)
    f = np.argwhere(feat).astype(np.int64)
    if len(f) == 0:
        return out.reshape(shape)
    nodes = np.stack(np.unravel_index(np.arange(feat.size), shape), axis=1).astype(np.int64)
    step = max(1, (1 << 22) // len(f))
    for s in range(0, len(nodes), step):
        d = nodes[s:s + step, None, :] - f[None, :, :]
        sq = (d * d).astype(np.float64)
        q = w[0] * sq[..., 0] + (w[1] * sq[..., 1] + w[2] * sq[..., 2])
        out[s:s + step] = q.min(axis=1)
    return out.reshape(shape)


def row_distance(feat):
    """g int64 [n0,n1,n2]: |i_2 - j_2| to the nearest feature of the row, NONE for a row without one."""
    n2 = feat.shape[2]
    i = np.arange(n2, dtype=np.int64)
    d = np.abs(i[:, None] - i[None, :])
    return np.where(feat[:, :, None, :], d[None, None], NONE).min(axis=3)


def separable(feat, inv):
    w = weights(inv)
    n0, n1, n2 = feat.shape
    g = row_distance(feat)
    some = g != NONE
    f = np.where(some, w[2] * (np.where(some, g, 0) ** 2).astype(np.float64), INF)
    i1 = np.arange(n1, dtype=np.int64)
    t1 = w[1] * ((i1[:, None] - i1[None, :]) ** 2).astype(np.float64)          # [i1, j1]
    b = (t1[None, :, :, None] + f[:, None, :, :]).min(axis=2)                 # [i0, i1, i2]
    i0 = np.arange(n0, dtype=np.int64)
    t0 = w[0] * ((i0[:, None] - i0[None, :]) ** 2).astype(np.float64)          # [i0, j0]
    return (t0[:, :, None, None] + b[None, :, :, :]).min(axis=1)


def edt(vol, inv, threshold, invert=0):
    """What nca_vol_edt writes: f32 of the shape of `vol` ([..., n0, n1, n2])."""
    vol = np.asarray(vol)
    flat = vol.reshape((-1,) + vol.shape[-3:])
    out = np.stack([np.sqrt(separable(features(v, threshold, invert), inv)).astype(np.float32) for v in flat])
    return out.reshape(vol.shape)


def volume(shape, pattern, seed=0):
    """f32 [n0,n1,n2] whose nodes > THRESHOLD follow `pattern`; values on both sides of the threshold vary."""
    rng = np.random.default_rng([seed, *shape, PATTERNS.index(pattern)])
    low = (rng.random(shape) * 0.4).astype(np.float32)
    high = (0.6 + rng.random(shape) * 0.4).astype(np.float32)
    mask = np.zeros(shape, dtype=bool)
    if pattern == "corner":
        mask[0, 0, 0] = True
    elif pattern == "last_chunk":
        mask[shape[0] // 2, shape[1] - 1, shape[2] - 1] = True
    elif pattern.startswith("d"):
        mask = rng.random(shape) < float(pattern[1:])
    elif pattern == "all":
        mask[:] = True
    return np.where(mask, high, low)


@functools.lru_cache(maxsize=None)
def case(shape, pattern, inv, invert=0):
    """(vol, expected f32) of one shared case; computed once, callers leave both unchanged."""
    vol = volume(shape, pattern)
    want = edt(vol, inv, THRESHOLD, invert)
    vol.setflags(write=False)
    want.setflags(write=False)
    return vol, want


def directed(dist, mask, percentile):
    """(count, sum, max, quantile "higher") of f64 `dist` over `mask`, in numpy."""
    d = np.sort(np.asarray(dist, dtype=np.float64)[mask])
    if d.size == 0:
        return 0, np.nan, np.nan, np.nan
    k = int(np.ceil(percentile / 100.0 * (d.size - 1)))          # torch.quantile's rank, interpolation="higher"
    return d.size, float(d.sum()), float(d[-1]), float(d[k])
