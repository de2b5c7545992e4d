"""The numpy transcription of the "cpr" section of include/nerfca_hip.h -- nca_vol_sample_planes and nca_vol_lumen -- and of
reformat.frames, written from the header and the docstring, not from the kernels.

Every numpy operation below is one rounded f64 operation on whole arrays in the order the header writes it (numpy does not fuse); the
order-3 weights, taps and accumulation are those of the "resample" section and are taken from resample_ref, as the header refers to that
section.  The rays are marched for all rays at once with a mask of the rays that have not ended.  tests/test_cpr_cpu.py holds this file to
the mathematics and to scipy; the GPU tests compare the library with it bit for bit.  Also the volumes, planes and phantoms both test
files share."""
import math

import numpy as np

import resample_ref

CENTRE, OPEN, GRID = 1, 2, 4          # the status bits


def inv_of(shape, bounds):
    return tuple((shape[a] - 1) / (bounds[a][1] - bounds[a][0]) for a in range(3))


def world_to_grid(p, lo, inv, n):
    """(x [..., 3], inside [...]) of world points p [..., 3]"""
    x = (p - np.array(lo, dtype=np.float64)) * np.array(inv, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.ones(x.shape[:-1], dtype=bool)
        for a in range(3):
            inside &= (x[..., a] >= 0.0) & (x[..., a] <= float(n[a] - 1))
    return x, inside


def cells(x, n):
    """(f int64 [..., 3], y f64 [..., 3]) of inside grid coordinates"""
    fl = np.minimum(np.floor(x), np.array([float(v - 2) for v in n]))
    return fl.astype(np.int64), x - fl


def mix(lo, hi, y):
    return lo + y * (hi - lo)


def trilinear(vol, f, y):
    """g of order 1, f64 [...]: vol f32 [n0, n1, n2], the cells (f, y) of inside points"""
    v = np.asarray(vol, dtype=np.float32).astype(np.float64)
    f0, f1, f2 = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(all="ignore"):
        a00 = mix(v[f0, f1, f2], v[f0, f1, f2 + 1], y[..., 2])
        a01 = mix(v[f0, f1 + 1, f2], v[f0, f1 + 1, f2 + 1], y[..., 2])
        a10 = mix(v[f0 + 1, f1, f2], v[f0 + 1, f1, f2 + 1], y[..., 2])
        a11 = mix(v[f0 + 1, f1 + 1, f2], v[f0 + 1, f1 + 1, f2 + 1], y[..., 2])
        return mix(mix(a00, a01, y[..., 1]), mix(a10, a11, y[..., 1]), y[..., 0])


def cubic_axis(cc, n):
    """(taps int64 [..., 4], weights f64 [..., 4]) of one axis at the coordinates cc: the expressions of resample_ref.cubic_taps"""
    f = np.floor(cc)
    y = cc - f
    t = 1 - y
    w1 = (y * y * (y - 2) * 3 + 4) / 6
    w2 = (t * t * (t - 2) * 3 + 4) / 6
    w0 = t * t * t / 6
    w3 = 1 - w0 - w1 - w2
    j = f.astype(np.int64)[..., None] + np.arange(-1, 3)
    return resample_ref.mirror(j, n), np.stack([w0, w1, w2, w3], axis=-1)


def cubic(coeff, x):
    """acc of order 3, f64 [...]: coeff f64 [n0, n1, n2], inside grid coordinates x [..., 3]"""
    n = coeff.shape
    (j0, w0), (j1, w1), (j2, w2) = [cubic_axis(x[..., a], n[a]) for a in range(3)]
    acc = np.zeros(x.shape[:-1], dtype=np.float64)
    with np.errstate(all="ignore"):
        for k0 in range(4):
            for k1 in range(4):
                for k2 in range(4):
                    acc = acc + ((coeff[j0[..., k0], j1[..., k1], j2[..., k2]] * w0[..., k0]) * w1[..., k1]) * w2[..., k2]
    return acc


def plane_points(origin, e1, e2, nu, nv, du, dv):
    """world points f64 [K, nu, nv, 3] of the pixels"""
    origin, e1, e2 = (np.asarray(a, dtype=np.float64)[:, None, None, :] for a in (origin, e1, e2))
    u = ((np.arange(nu).astype(np.float64) - 0.5 * float(nu - 1)) * du)[None, :, None, None]
    v = ((np.arange(nv).astype(np.float64) - 0.5 * float(nv - 1)) * dv)[None, None, :, None]
    return (origin + u * e1) + v * e2


def sample_planes(vol, lo, inv, order, origin, e1, e2, nu, nv, du, dv, fill):
    """What nca_vol_sample_planes writes for the f32 stack vol [n_vol, n0, n1, n2]: f32 [n_vol, K, nu, nv].  At order 3 the coefficients are
    resample_ref.spline_filter(vol), what nca_vol_spline_filter hands over bit for bit."""
    vol = np.asarray(vol, dtype=np.float32)
    n = vol.shape[-3:]
    x, inside = world_to_grid(plane_points(origin, e1, e2, nu, nv, du, dv), lo, inv, n)
    out = np.full((vol.shape[0],) + inside.shape, np.float32(fill), dtype=np.float32)
    xi = x[inside]
    if order == 0:
        j = np.floor(xi + 0.5).astype(np.int64)
    elif order == 1:
        f, y = cells(xi, n)
    for q in range(vol.shape[0]):
        with np.errstate(all="ignore"):
            if order == 0:
                out[q][inside] = vol[q][j[:, 0], j[:, 1], j[:, 2]]
            elif order == 1:
                out[q][inside] = trilinear(vol[q], f, y).astype(np.float32)
            else:
                assert order == 3
                out[q][inside] = cubic(resample_ref.spline_filter(vol[q]), xi).astype(np.float32)
    return out


def directions(n_ang):
    return np.array([[math.cos(2.0 * math.pi * a / n_ang), math.sin(2.0 * math.pi * a / n_ang)] for a in range(n_ang)], dtype=np.float64)


def sin_step(n_ang):
    return math.sin(2.0 * math.pi / n_ang)


def rays(vol, lo, inv, origin, e1, e2, dirs, level, dr, n_steps):
    """(r f64 [K, n_ang] unrounded, bits int32 [K, n_ang]) of ONE volume [n0, n1, n2]"""
    n = vol.shape
    origin, e1, e2 = (np.asarray(a, dtype=np.float64)[:, None, :] for a in (origin, e1, e2))
    dirs = np.asarray(dirs, dtype=np.float64)
    K, A = origin.shape[0], dirs.shape[0]
    r = np.zeros((K, A), dtype=np.float64)
    bits = np.zeros((K, A), dtype=np.int32)
    live = np.ones((K, A), dtype=bool)
    g_prev = np.zeros((K, A), dtype=np.float64)
    for j in range(n_steps + 1):
        rj = float(j) * dr
        c, s = (rj * dirs[:, 0])[None, :, None], (rj * dirs[:, 1])[None, :, None]
        x, inside = world_to_grid((origin + c * e1) + s * e2, lo, inv, n)
        left = live & ~inside
        r[left] = 0.0 if j == 0 else float(j - 1) * dr
        bits[left] |= GRID
        live &= inside
        g = np.full((K, A), np.nan)
        f, y = cells(x[live], n)
        g[live] = trilinear(vol, f, y)
        with np.errstate(all="ignore"):
            stop = live & ~(g > level)
            if j == 0:
                r[stop] = 0.0
                bits[stop] |= CENTRE
            else:
                t = np.where(np.isfinite(g), (g_prev - level) / (g_prev - g), 0.0)
                r[stop] = ((float(j - 1) + t) * dr)[stop]
        live &= ~stop
        g_prev = g
        if not live.any():
            break
    r[live] = float(n_steps) * dr
    bits[live] |= OPEN
    return r, bits


def ray_stats(r, sin_step_):
    """stats f64 [4] of the unrounded radii r [n_ang] of one plane"""
    n = r.shape[0]
    with np.errstate(all="ignore"):
        acc = 0.0
        for a in range(n):
            acc = acc + r[a] * r[(a + 1) % n]
        area = (0.5 * sin_step_) * acc
        half = n // 2
        lo = hi = r[0] + r[half]
        for a in range(1, half):
            d = r[a] + r[a + half]
            if d < lo:
                lo = d
            if d > hi:
                hi = d
        acc = 0.0
        for a in range(n):
            acc = acc + r[a]
    return np.array([area, lo, hi, acc / float(n)], dtype=np.float64)


def lumen(vol, lo, inv, origin, e1, e2, n_ang, level, dr, n_steps):
    """What nca_vol_lumen writes for the f32 stack vol [n_vol, n0, n1, n2]: (radius f32 [n_vol, K, n_ang], stats f64 [n_vol, K, 4], status
    int32 [n_vol, K]), and the unrounded radii f64 [n_vol, K, n_ang]"""
    vol = np.asarray(vol, dtype=np.float32)
    dirs, ss = directions(n_ang), sin_step(n_ang)
    rs, stats, status = [], [], []
    for q in range(vol.shape[0]):
        r, bits = rays(vol[q], lo, inv, origin, e1, e2, dirs, level, dr, n_steps)
        rs.append(r)
        stats.append(np.stack([ray_stats(row, ss) for row in r]))
        status.append(np.bitwise_or.reduce(bits, axis=1).astype(np.int32))
    r = np.stack(rs)
    return r.astype(np.float32), np.stack(stats), np.stack(status), r


# ------------------------------------------------------------------------------------------------------------------------------ frames
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frames(points, step=None, smooth=0, up=None):
    """(origin, tangent, e1, e2, s) of reformat.frames, point by point"""
    p = [np.array(v, dtype=np.float64) for v in points]
    p = [v for i, v in enumerate(p) if i == 0 or (v != p[i - 1]).any()]
    for _ in range(smooth):
        p = [p[0]] + [((p[i - 1] + 2.0 * p[i]) + p[i + 1]) / 4.0 for i in range(1, len(p) - 1)] + [p[-1]]
    seg = [math.sqrt(_dot(b - a, b - a)) for a, b in zip(p[:-1], p[1:])]
    cum = np.concatenate([[0.0], np.cumsum(np.array(seg))])
    length = float(cum[-1])
    if step is None:
        step = length / (len(p) - 1)
    count = int(math.floor(length / step + 1e-9)) + 1
    origin, s = [], []
    for k in range(count):
        sk = min(float(k) * step, length)
        i = min(max(int(np.searchsorted(cum, sk, side="right")) - 1, 0), len(p) - 2)
        t = (sk - cum[i]) / seg[i] if seg[i] > 0.0 else 0.0
        origin.append(p[i] + t * (p[i + 1] - p[i]))
        s.append(sk)
    tan = []
    for k in range(count):
        d = origin[min(k + 1, count - 1)] - origin[max(k - 1, 0)]
        tan.append(d / math.sqrt(_dot(d, d)))
    if up is None:
        start = np.zeros(3)
        start[int(np.argmin(np.abs(tan[0])))] = 1.0
    else:
        start = np.array(up, dtype=np.float64)
    r = start - _dot(start, tan[0]) * tan[0]
    e1 = [r / math.sqrt(_dot(r, r))]
    for i in range(count - 1):
        v1 = origin[i + 1] - origin[i]
        c1 = _dot(v1, v1)
        rl = e1[i] - (2.0 / c1 * _dot(v1, e1[i])) * v1
        tl = tan[i] - (2.0 / c1 * _dot(v1, tan[i])) * v1
        v2 = tan[i + 1] - tl
        c2 = _dot(v2, v2)
        rn = rl - (2.0 / c2 * _dot(v2, rl)) * v2 if c2 > 0.0 else rl
        rn = rn - _dot(rn, tan[i + 1]) * tan[i + 1]
        e1.append(rn / math.sqrt(_dot(rn, rn)))
    e2 = [np.array([t[1] * e[2] - t[2] * e[1], t[2] * e[0] - t[0] * e[2], t[0] * e[1] - t[1] * e[0]]) for t, e in zip(tan, e1)]
    return np.array(origin), np.array(tan), np.array(e1), np.array(e2), np.array(s)


# ------------------------------------------------------------------------------------------------------------- what both test files share
LO = (0.0, -1.0, 2.0)                                  # of nca_testlib.grid_of
SHAPES = ((9, 12, 70), (5, 6, 7))
INVS = ((1.0, 1.0, 1.0), (1.0, 2.0, 0.5))              # unit and anisotropic spacing
PLANE_SIZES = ((1, 1), (3, 5), (17, 17))               # the last across the 16-pixel tile seam


def volumes(shape, n_vol, seed=0, special=False):
    """f32 [n_vol, n0, n1, n2] of normal data; special: a NaN, a +inf and a -inf node in every volume"""
    rng = np.random.default_rng(5100 + seed + 7 * shape[0] + 3 * shape[1] + shape[2] + 100 * n_vol)
    vol = rng.standard_normal((n_vol,) + tuple(shape)).astype(np.float32)
    if special:
        for q in range(n_vol):
            for val in (np.nan, np.inf, -np.inf):
                vol[q][tuple(int(rng.integers(0, s)) for s in shape)] = val
    return vol


def node_to_world(node, lo, inv):
    return np.array([lo[a] + node[a] / inv[a] for a in range(3)], dtype=np.float64)


def oblique_planes(shape, lo, inv, count, seed=0, spread=1.0):
    """(origin, e1, e2) f64 [count, 3]: orthonormal pairs in random orientation; the origins spread over `spread` times the grid's box about
    its centre (spread > 1: planes partly and wholly outside)"""
    rng = np.random.default_rng(5200 + seed)
    ext = np.array([(shape[a] - 1) / inv[a] for a in range(3)])
    centre = np.array(lo) + 0.5 * ext
    origin = centre + (rng.random((count, 3)) - 0.5) * ext * spread
    a = rng.standard_normal((count, 3))
    b = rng.standard_normal((count, 3))
    e1 = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b - (b * e1).sum(1, keepdims=True) * e1
    e2 = b / np.linalg.norm(b, axis=1, keepdims=True)
    return origin, e1, e2


def axis_planes(shape, lo, inv, axis, slices):
    """The planes whose pixels are the nodes of the slices `slices` of `axis`, in world coordinates: (origin, e1, e2, nu, nv, du, dv) with
    pixel (i, j) on node (i, j) of the two other axes in ascending order.  Exact for the dyadic spacings and odd centres used here."""
    b, c = [a for a in range(3) if a != axis]
    nu, nv = shape[b], shape[c]
    origin, e1, e2 = [], [], []
    for k in slices:
        node = [0.0, 0.0, 0.0]
        node[axis], node[b], node[c] = float(k), 0.5 * (nu - 1), 0.5 * (nv - 1)
        origin.append(node_to_world(node, lo, inv))
        e1.append(np.eye(3)[b])
        e2.append(np.eye(3)[c])
    return np.array(origin), np.array(e1), np.array(e2), nu, nv, 1.0 / inv[b], 1.0 / inv[c]


def tube_field(shape, lo, inv, a, b, rho):
    """f32 [n0, n1, n2]: rho - (distance from the segment a b, world coordinates), at the nodes"""
    x = np.stack(np.meshgrid(*(lo[k] + np.arange(shape[k]) / inv[k] for k in range(3)), indexing="ij"), axis=-1)
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    e = b - a
    q = x - a
    t = np.clip((q * e).sum(-1) / float((e * e).sum()), 0.0, 1.0)
    return (rho - np.sqrt(((q - t[..., None] * e) ** 2).sum(-1))).astype(np.float32)


def narrowing_tube(shape, lo, inv, axis_point, rho, span):
    """f32 [n0, n1, n2]: rho(z) - (distance from the line through axis_point along axis 2), where the radius rho(z) falls linearly from
    rho to rho / 2 over the world interval span = (z0, z1) of axis 2, stays at rho / 2 for the same length and rises again likewise"""
    z0, z1 = span
    x = [lo[k] + np.arange(shape[k]) / inv[k] for k in range(3)]
    d = np.sqrt((x[0][:, None] - axis_point[0]) ** 2 + (x[1][None, :] - axis_point[1]) ** 2)
    w = z1 - z0
    ramp = np.clip((x[2] - z0) / w, 0.0, 1.0) - np.clip((x[2] - (z1 + w)) / w, 0.0, 1.0)
    radius = rho * (1.0 - 0.5 * ramp)
    return (radius[None, None, :] - d[:, :, None]).astype(np.float32)
