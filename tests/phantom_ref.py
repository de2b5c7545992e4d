"""The f64 numpy rasteriser the phantom tests hold the kernel to: a direct transcription of the definition in include/nerfca_hip.h
("phantom"), every operation one rounded f64 operation in the order written.  Plus the tables and bounds the tests share."""
import numpy as np

BOUNDS = ((-0.9, 0.8), (-0.7, 0.9), (-0.8, 0.6))          # tests/drr_ref.BOUNDS: three different extents, none centred
SHAPES = [(5, 3, 4), (9, 17, 70), (2, 2, 130)]            # smaller than a tile; partial tiles on every axis, the 64-lane row crossed; minimum axes
RHO_V = 1.75


def node_positions(shape, bounds):
    """x_a f64 [n_a] per axis: h_a = 1 / inv_a with inv_a = (n_a - 1) / (hi_a - lo_a) (drr.grid_desc), x_a = lo_a + i_a h_a."""
    xs = []
    for n, (lo, hi) in zip(shape, bounds):
        inv = np.float64((int(n) - 1) / (float(hi) - float(lo)))
        h = np.float64(1.0) / inv
        xs.append(np.float64(lo) + np.arange(int(n), dtype=np.float64) * h)
    return xs


def spacing(shape, bounds):
    return [float(x[1] - x[0]) for x in node_positions(shape, bounds)]


def default_edge(shape, bounds):
    """phantom.voxelize's default edge: the coarsest node spacing, max_a 1 / inv_a."""
    return max(1.0 / ((int(n) - 1) / (float(hi) - float(lo))) for n, (lo, hi) in zip(shape, bounds))


def diagonal(bounds):
    return float(np.sqrt(sum((float(hi) - float(lo)) ** 2 for lo, hi in bounds)))


def _clamp01(v):
    return np.minimum(np.maximum(v, 0.0), 1.0)


def ellipsoid_cov(x, row):
    """cov f64 [n0,n1,n2] of one ellipsoid row f64 [14] at the node positions x = (x0 [n0,1,1], x1 [1,n1,1], x2 [1,1,n2])."""
    c, A, w = row[0:3], row[3:12].reshape(3, 3), row[12]
    u = [x[k] - c[k] for k in range(3)]
    q = [(A[k, 0] * u[0] + A[k, 1] * u[1]) + A[k, 2] * u[2] for k in range(3)]
    r = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    return _clamp01(0.5 + (1.0 - r) / w)


def segment_cov(x, row, edge):
    """cov f64 [n0,n1,n2] of one segment row f64 [8]; also returns d, the distance to the axis."""
    a, b, ra, rb = row[0:3], row[3:6], row[6], row[7]
    e = b - a
    ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    q = [x[k] - a[k] for k in range(3)]
    qe = (q[0] * e[0] + q[1] * e[1]) + q[2] * e[2]
    if ee == 0.0:
        t = np.zeros_like(qe)
    else:
        t = _clamp01(qe / ee)
    c = [q[k] - t * e[k] for k in range(3)]
    d = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    r = ra + t * (rb - ra)
    return _clamp01(0.5 + (r - d) / edge), d


def voxelize(shape, bounds, ell, seg, rho_v, edge):
    """(out f64 [P,n0,n1,n2] BEFORE the rounding to f32, mass f64 [P,n0,n1,n2] = sum |rho_e| + |rho_v|, the same at every node of a
    phase) of ell f64 [P,E,14] or None and seg f64 [P,N,8] or None."""
    xs = node_positions(shape, bounds)
    x = (xs[0][:, None, None], xs[1][None, :, None], xs[2][None, None, :])
    P = (ell if ell is not None else seg).shape[0]
    out = np.zeros((P,) + tuple(shape), dtype=np.float64)
    mass = np.zeros_like(out)
    for p in range(P):
        bg = np.zeros(shape, dtype=np.float64)
        m = 0.0
        if ell is not None:
            for row in np.asarray(ell[p], dtype=np.float64):
                bg = bg + row[13] * ellipsoid_cov(x, row)
                m += abs(row[13])
        best = np.zeros(shape, dtype=np.float64)
        if seg is not None and seg.shape[1]:
            for row in np.asarray(seg[p], dtype=np.float64):
                best = np.maximum(best, segment_cov(x, row, edge)[0])
            m += abs(rho_v)
        out[p] = bg + rho_v * best
        mass[p] = m
    return out, mass


def bound(want64, mass, bounds, edge):
    """|out - want64| allowed: one rounding to f32, plus a device square root or division an ulp off the host's, amplified by 1 / edge."""
    return 2.0 ** -24 * np.abs(want64) + 2.0 ** -52 * 4 * max(1.0, diagonal(bounds) / edge) * mass


def random_segments(P, N, bounds, seed, r_max=0.12):
    """f64 [P,N,8]: endpoints inside the bounds grown by a fifth (some segments poke out), radii in [0, r_max]."""
    rng = np.random.default_rng(seed)
    lo = np.array([b[0] for b in bounds])
    hi = np.array([b[1] for b in bounds])
    ext = hi - lo
    a = lo - 0.2 * ext + rng.random((P, N, 3)) * 1.4 * ext
    b = a + (rng.random((P, N, 3)) - 0.5) * 0.6 * ext
    r = rng.random((P, N, 2)) * r_max
    return np.concatenate([a, b, r], axis=-1)


def random_ellipsoids(P, E, bounds, seed):
    """f64 [P,E,14]: centres inside the bounds, a full (not axis-aligned) matrix, widths in [0.05, 0.4], densities of both signs."""
    rng = np.random.default_rng(seed)
    lo = np.array([b[0] for b in bounds])
    hi = np.array([b[1] for b in bounds])
    c = lo + rng.random((P, E, 3)) * (hi - lo)
    A = rng.standard_normal((P, E, 9)) * 1.5 + np.eye(3).reshape(9) * 2.0
    w = 0.05 + 0.35 * rng.random((P, E, 1))
    rho = rng.standard_normal((P, E, 1))
    return np.concatenate([c, A, w, rho], axis=-1)
