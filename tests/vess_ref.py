"""The numpy transcription of the Hessian vesselness (include/nerfca_hip.h, "vess"): the Hessian with clamped indices, five sweeps of cyclic
Jacobi, the sort, V and the merge over scales -- every operation one f64 operation in the order of the header, vectorised over the nodes --
and the inputs the CPU and the GPU tests share.  The plain scipy + LAPACK expression it is held to lives here too
(tests/test_vess_cpu.py)."""
import functools

import numpy as np

SWEEPS = 5
NAN32 = np.float32(np.nan)


# ----------------------------------------------------------------------------- the definition
def hessian(s, scale):
    """The six entries (H00, H01, H02, H11, H12, H22) in f64 of an f32 array [..., n0, n1, n2]; every volume on its own."""
    s = np.asarray(s)
    assert s.dtype == np.float32 and s.ndim >= 3
    n = s.shape[-3:]
    p = np.pad(s.astype(np.float64), [(0, 0)] * (s.ndim - 3) + [(1, 1)] * 3, mode="edge")          # an index clamped on its own axis

    def at(d0, d1, d2):
        return p[..., 1 + d0:1 + d0 + n[0], 1 + d1:1 + d1 + n[1], 1 + d2:1 + d2 + n[2]]

    def e(a, sign=1):
        d = [0, 0, 0]
        d[a] = sign
        return d

    def plus(x, y):
        return [i + j for i, j in zip(x, y)]

    scale = np.float64(scale)
    v = at(0, 0, 0)
    H = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            H[a, a] = scale * ((at(*e(a)) - v) - (v - at(*e(a, -1))))
            for b in range(a + 1, 3):
                H[a, b] = scale * (0.25 * ((at(*plus(e(a), e(b))) - at(*plus(e(a), e(b, -1)))) - (at(*plus(e(a, -1), e(b))) - at(*plus(e(a, -1), e(b, -1))))))
    return H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]


def _rotate(app, aqq, apq, arp, arq):
    """One rotation of the pair (p, q) on arrays; where a_pq == 0 nothing changes."""
    go = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tp = t * apq
        rp, rq = c * arp - s * arq, s * arp + c * arq
    return (np.where(go, app - tp, app), np.where(go, aqq + tp, aqq), np.where(go, 0.0, apq), np.where(go, rp, arp), np.where(go, rq, arq))


def _order(x, y):
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(invalid="ignore"):
        swap = (ay < ax) | ((ay == ax) & (y < x))
    return np.where(swap, y, x), np.where(swap, x, y)


def jacobi(a00, a01, a02, a11, a12, a22, sweeps=SWEEPS, sort=True):
    """(l1, l2, l3) f64 of symmetric 3 x 3 matrices given as six arrays; with sort=False the diagonal as the sweeps leave it, and the
    off-diagonal entries after it."""
    a00, a01, a02, a11, a12, a22 = (np.array(x, dtype=np.float64) for x in (a00, a01, a02, a11, a12, a22))
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)          # (0,1), r = 2
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)          # (0,2), r = 1
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)          # (1,2), r = 0
    if not sort:
        return a00, a11, a22, a01, a02, a12
    a00, a11 = _order(a00, a11)
    a11, a22 = _order(a11, a22)
    a00, a11 = _order(a00, a11)
    return a00, a11, a22


def eigenvalues64(s, scale):
    """(l1, l2, l3) in f64 and the mask of the nodes whose Hessian is finite (elsewhere the three are NaN)."""
    H = hessian(s, scale)
    finite = np.ones(H[0].shape, dtype=bool)
    for h in H:
        finite &= np.isfinite(h)
    l = jacobi(*[np.where(finite, h, 0.0) for h in H])
    return tuple(np.where(finite, x, np.nan) for x in l), finite


def _f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isnan(x), NAN32, x.astype(np.float32))


def eigenvalues(s, scale):
    """What nca_vol_hessian_eig writes: f32 [..., 3, n0, n1, n2]."""
    l, _ = eigenvalues64(s, scale)
    return np.stack([_f32(x) for x in l], axis=-4)


def norm_max(s, scale):
    """What nca_vol_hessian_norm_max writes: f64 [...], the largest (x1 x1 + x2 x2) + x3 x3 of the f32 eigenvalues per volume, a NaN
    passed over, at least +0."""
    e = eigenvalues(s, scale).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s2 = (e[..., 0, :, :, :] * e[..., 0, :, :, :] + e[..., 1, :, :, :] * e[..., 1, :, :, :]) + e[..., 2, :, :, :] * e[..., 2, :, :, :]
    return np.fmax(np.fmax.reduce(s2.reshape(s2.shape[:-3] + (-1,)), axis=-1), 0.0)


def vesselness_from(l, finite, alpha, beta, c, bright=True):
    """V f32 from f64 eigenvalue arrays; c: a scalar or an array that broadcasts against them."""
    l1, l2, l3 = l
    with np.errstate(all="ignore"):
        tube = finite & (((l2 < 0.0) & (l3 < 0.0)) if bright else ((l2 > 0.0) & (l3 > 0.0)))
        q1, q2, q3 = l1 * l1, l2 * l2, l3 * l3
        ra2, rb2, s2 = q2 / q3, q1 / np.abs(l2 * l3), (q1 + q2) + q3
        ta, tb = 2.0 * (np.float64(alpha) * np.float64(alpha)), 2.0 * (np.float64(beta) * np.float64(beta))
        c = np.asarray(c, dtype=np.float64)
        tc = 2.0 * (c * c)
        A, B = 1.0 - np.exp(-ra2 / ta), np.exp(-rb2 / tb)
        C = np.where(tc == 0.0, 1.0, 1.0 - np.exp(-s2 / tc))
        V = ((A * B) * C).astype(np.float32)
    return np.where(tube, V, np.float32(0.0))


def vesselness_scale(s, scale, alpha=0.5, beta=0.5, c=0.5, bright=True):
    """V f32 of one smoothed f32 array [..., n0, n1, n2]; c: a scalar, or one value per volume (of the leading shape)."""
    l, finite = eigenvalues64(s, scale)
    c = np.asarray(c, dtype=np.float64)
    return vesselness_from(l, finite, alpha, beta, c.reshape(c.shape + (1, 1, 1)) if c.ndim else c, bright)


def merge(vs):
    """(V, index) over a list of per-scale f32 arrays: a later scale replaces a node only where its V is greater."""
    out, idx = vs[0].copy(), np.zeros(vs[0].shape, dtype=np.int32)
    for i, v in enumerate(vs[1:], 1):
        with np.errstate(invalid="ignore"):
            take = v > out
        out, idx = np.where(take, v, out), np.where(take, np.int32(i), idx)
    return out, idx


def smooth(vol, sigma):
    """scipy's Gaussian as ccta.gaussian_filter forms it: f64 inside, reflect, truncate 4, one rounding to f32; every volume on its own."""
    import scipy.ndimage
    vol = np.asarray(vol, dtype=np.float32)
    flat = vol.reshape((-1,) + vol.shape[-3:])
    with np.errstate(all="ignore"):
        out = np.stack([scipy.ndimage.gaussian_filter(v.astype(np.float64), sigma, mode="reflect", truncate=4.0).astype(np.float32) for v in flat])
    return out.reshape(vol.shape)


def vesselness(vol, sigmas=(1.0, 2.0, 3.0), alpha=0.5, beta=0.5, c=None, bright=True):
    """(V, index) of ccta.vesselness from the definition: per scale the smoothing, Frangi's c = 0.5 sqrt(norm_max) per volume when c is
    None, V, and the merge."""
    vs = []
    for sigma in sigmas:
        s, scale = smooth(vol, sigma), float(sigma) * float(sigma)
        vs.append(vesselness_scale(s, scale, alpha, beta, 0.5 * np.sqrt(norm_max(s, scale)) if c is None else c, bright))
    return merge(vs)


# ----------------------------------------------------------------------------- the plain expression the transcription is held to
def plain_vesselness(s, scale, alpha, beta, c, bright=True):
    """The expression a user would write for one smoothed f64 volume [n0, n1, n2]: the same differences, numpy.linalg.eigvalsh, a sort by
    absolute value, Frangi's formula.  f64."""
    H = hessian(np.asarray(s, dtype=np.float32), scale)
    M = np.empty(H[0].shape + (3, 3))
    for (a, b), h in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), H):
        M[..., a, b] = M[..., b, a] = h
    w = np.linalg.eigvalsh(M)
    w = np.take_along_axis(w, np.argsort(np.abs(w), axis=-1, kind="stable"), axis=-1)
    l1, l2, l3 = w[..., 0], w[..., 1], w[..., 2]
    with np.errstate(all="ignore"):
        V = (1 - np.exp(-(l2 / l3) ** 2 / (2 * alpha ** 2))) * np.exp(-l1 ** 2 / np.abs(l2 * l3) / (2 * beta ** 2))
        if c:
            V = V * (1 - np.exp(-(l1 ** 2 + l2 ** 2 + l3 ** 2) / (2 * c ** 2)))
    tube = ((l2 < 0) & (l3 < 0)) if bright else ((l2 > 0) & (l3 > 0))
    return np.where(tube, V, 0.0), w


# ----------------------------------------------------------------------------- inputs
FAMILIES = ("random", "near_degenerate", "tube", "scaled", "integers")


def matrices(family, count, seed=0):
    """`count` symmetric 3 x 3 matrices [count, 3, 3] f64.  "random": normal entries; "near_degenerate": Q diag(x, x (1 + d), y) Q^T with
    d from 1e-16 to 1e-4; "tube": Q diag(0, -1, -1) Q^T plus 1e-3 of noise; "scaled": random times 10^u, u uniform in [-16, 16];
    "integers": entries in -3 .. 3."""
    rng = np.random.default_rng(4242 + 17 * seed + FAMILIES.index(family))
    g = rng.standard_normal((count, 3, 3))
    sym = 0.5 * (g + g.transpose(0, 2, 1))
    if family == "random":
        return sym
    if family == "scaled":
        return sym * 10.0 ** rng.uniform(-16, 16, (count, 1, 1))
    if family == "integers":
        m = rng.integers(-3, 4, (count, 3, 3)).astype(np.float64)
        return np.triu(m) + np.triu(m, 1).transpose(0, 2, 1)
    q = np.linalg.qr(g)[0]
    if family == "near_degenerate":
        x, y = rng.standard_normal(count), rng.standard_normal(count)
        d = np.stack([x, x * (1.0 + 10.0 ** rng.uniform(-16, -4, count)), y], axis=1)
    elif family == "tube":
        d = np.tile(np.array([0.0, -1.0, -1.0]), (count, 1))
    else:
        raise ValueError(family)
    m = np.einsum("nij,nj,nkj->nik", q, d, q)
    if family == "tube":
        m = m + 1e-3 * sym
    return 0.5 * (m + m.transpose(0, 2, 1))


def six(m):
    return m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2]


def volume(shape, kind, seed=0):
    """f32 [n0, n1, n2].  "random": uniform in [0, 1); "binary": a mask filled to 60 %; "signed": values in [-1, 1) with exact zeros of both
    signs; "constant": 0.75 everywhere (seed 0) or 0 (any other); "nonfinite": random with one NaN and one +inf node."""
    rng = np.random.default_rng(2000 * seed + 7 * shape[0] + 3 * shape[1] + shape[2] + len(kind))
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
    if kind == "constant":
        return np.full(shape, 0.75 if seed == 0 else 0.0, dtype=np.float32)
    if kind == "nonfinite":
        x[tuple(s // 2 for s in shape)] = np.nan
        x[tuple((s - 1) // 3 for s in shape)] = np.inf
        return x
    raise ValueError(kind)


KINDS = ("random", "binary", "signed", "constant", "nonfinite")
SIDE = 33
MEANING_SIGMAS, MEANING_C = (1.0, 2.0, 3.0), 0.5


def _grid():
    return np.meshgrid(*[np.arange(SIDE) - SIDE // 2] * 3, indexing="ij")


def tube(radius=2.0):
    """f32 mask [33]^3 of a straight tube along axis 2 through the centre."""
    i, j, _ = _grid()
    return (i * i + j * j <= radius * radius).astype(np.float32)


def ball(radius=2.0):
    i, j, k = _grid()
    return (i * i + j * j + k * k <= radius * radius).astype(np.float32)


def slab(half=2):
    """f32 mask of a plate normal to axis 0, 2 half + 1 nodes thick."""
    i, _, _ = _grid()
    return (np.abs(i) <= half).astype(np.float32)


def tube_distance():
    """The distance of every node of the 33^3 grid from the tube's axis, and the mask of the nodes at least 5 nodes inside the grid."""
    i, j, k = _grid()
    h = SIDE // 2
    interior = (np.abs(i) <= h - 5) & (np.abs(j) <= h - 5) & (np.abs(k) <= h - 5)
    return np.sqrt(i * i + j * j), interior


@functools.lru_cache(maxsize=None)
def meaning(name, bright=True):
    """(V, index) of the transcription on one of the 33^3 masks ("tube", "ball", "slab", "negated tube") at sigmas (1, 2, 3), c = 0.5."""
    x = {"tube": tube, "ball": ball, "slab": slab, "negated tube": lambda: -tube()}[name]()
    return vesselness(x, MEANING_SIGMAS, c=MEANING_C, bright=bright)
