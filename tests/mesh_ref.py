"""A vectorised numpy transcription of the iso-surface definition of include/nerfca_hip.h ("mesh": marching tetrahedra on the Kuhn split of
every grid cell), the oracle of tests/test_mesh_gpu.py and the subject of tests/test_mesh_cpu.py; the fields and the case list both use; and
`inside_volume`, which measures the region above the level tetrahedron by tetrahedron and never looks at a mesh.

Every f64 operation below is the header's, in the header's order, one rounding each: the GPU tests hold the kernels to these bits."""
import functools

import numpy as np

# the six tetrahedra of a cell: the permutations (a, b, c) of the axes in lexicographic order; p0 = base, p1 = p0 + e_a, p2 = p1 + e_b, p3 = p2 + e_c
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
ODD = (False, True, True, False, False, True)          # the permutation's parity: det[p1 - p0, p2 - p0, p3 - p0] = -1
# the edges of a tetrahedron as pairs (i, j), i < j, of its corners
EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# case (bit i: corner i is inside) -> the edge numbers of its triangles, three each, for a tetrahedron of even parity
TRIANGLES = ((), (0, 1, 2), (0, 4, 3), (1, 2, 4, 1, 4, 3), (1, 3, 5), (0, 3, 5, 0, 5, 2), (0, 4, 5, 0, 5, 1), (2, 4, 5),
             (2, 5, 4), (0, 1, 5, 0, 5, 4), (0, 2, 5, 0, 5, 3), (1, 5, 3), (1, 3, 4, 1, 4, 2), (0, 3, 4), (0, 2, 1), ())


def direction(k):
    """d of edge k = 1 .. 7: bit 2 is axis 0, bit 1 axis 1, bit 0 axis 2 (the last, contiguous one)."""
    return (k >> 2) & 1, (k >> 1) & 1, k & 1


def corner_codes(q):
    """The corners p0 .. p3 of tetrahedron q as codes 4 d0 + 2 d1 + d2 of their offsets from the cell's base node."""
    a, b, _ = PERMS[q]
    p1 = 4 >> a
    return 0, p1, p1 | (4 >> b), 7


def inside(vol, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, dtype=np.float32) > np.float32(level)


def _crossing_t(va, vb, level):
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (np.float64(np.float32(level)) - va) / (vb - va)
        return np.where(np.isfinite(t), np.minimum(np.maximum(t, 0.0), 1.0), 0.5)


def mesh(vol, level, lo, inv, normals=False):
    """dict(verts f32 [V,3], verts64 f64 [V,3] (the same before the one rounding), tris int32 [T,3], normals f32 [V,3] or None) of ONE volume
    [n0,n1,n2] on the grid (lo, inv)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    n = vol.shape
    N = vol.size
    lo, inv = np.asarray(lo, dtype=np.float64), np.asarray(inv, dtype=np.float64)
    ins = inside(vol, level)
    cross = np.zeros(n + (7,), dtype=bool)
    for k in range(1, 8):
        d = direction(k)
        sa = tuple(slice(0, n[a] - d[a]) for a in range(3))
        sb = tuple(slice(d[a], n[a]) for a in range(3))
        cross[sa + (k - 1,)] = ins[sa] != ins[sb]
    cross = cross.reshape(N, 7)
    vid = np.where(cross, np.cumsum(cross.ravel()).reshape(N, 7) - 1, -1)          # the vertex of (node, k): numbered by (node, k) ascending
    owner, km1 = np.nonzero(cross)
    D = np.array([direction(k) for k in range(1, 8)], dtype=np.int64)[km1]
    ia = np.stack(np.unravel_index(owner, n), axis=-1).astype(np.int64).reshape(-1, 3)
    ib = ia + D
    flat = vol.ravel()
    va = flat[owner].astype(np.float64)
    vb = vol[ib[:, 0], ib[:, 1], ib[:, 2]].astype(np.float64)
    t = _crossing_t(va, vb, level)
    pos = ia.astype(np.float64) + np.where(D == 1, t[:, None], 0.0)
    h = 1.0 / inv
    verts64 = lo + pos * h
    out = dict(verts64=verts64, verts=verts64.astype(np.float32), normals=None)
    if normals:
        def grad(i):
            g = np.empty(i.shape, dtype=np.float64)
            for a in range(3):
                ip, im = i.copy(), i.copy()
                ip[:, a] = np.minimum(i[:, a] + 1, n[a] - 1)
                im[:, a] = np.maximum(i[:, a] - 1, 0)
                g[:, a] = (0.5 * (vol[ip[:, 0], ip[:, 1], ip[:, 2]].astype(np.float64) - vol[im[:, 0], im[:, 1], im[:, 2]].astype(np.float64))) * inv[a]
            return g
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ga, gb = grad(ia), grad(ib)
            nn = -(ga + t[:, None] * (gb - ga))
            length = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
            ok = np.isfinite(length) & (length != 0.0)
            out["normals"] = np.where(ok[:, None], nn / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)
    # triangles: ordered by (cell, tetrahedron, triangle); a cell's number is its base node's
    idx = np.arange(N).reshape(n)
    base = idx[:-1, :-1, :-1].ravel()
    strides = (n[1] * n[2], n[2], 1)
    code_off = np.array([sum(direction(c)[a] * strides[a] for a in range(3)) for c in range(8)], dtype=np.int64)
    insf = ins.ravel()
    tri = np.full((base.size, 6, 2, 3), -1, dtype=np.int64)
    for q in range(6):
        P = corner_codes(q)
        m = sum(insf[base + code_off[P[i]]].astype(np.int64) << i for i in range(4))
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if sel.size == 0:
                continue
            es = TRIANGLES[case]
            for s in range(len(es) // 3):
                three = es[3 * s:3 * s + 3]
                if ODD[q]:
                    three = (three[0], three[2], three[1])
                for r, e in enumerate(three):
                    i, j = EDGES[e]
                    tri[sel, q, s, r] = vid[base[sel] + code_off[P[i]], (P[i] ^ P[j]) - 1]
    tri = tri.reshape(-1, 3)
    tri = tri[tri[:, 0] >= 0]
    assert (tri >= 0).all()
    out["tris"] = tri.astype(np.int32)
    return out


def stack_mesh(stack, level, lo, inv, normals=True):
    """The meshes of a stack [n_vol,n0,n1,n2] as the entry points return them: totals int64 [n_vol,2], verts, tris and normals back to back."""
    ms = [mesh(v, level, lo, inv, normals) for v in stack]
    totals = np.array([[m["verts"].shape[0], m["tris"].shape[0]] for m in ms], dtype=np.int64).reshape(-1, 2)
    cat = lambda key, dt: np.concatenate([m[key] for m in ms]).astype(dt).reshape(-1, 3)          # noqa: E731
    return dict(totals=totals, verts=cat("verts", np.float32), tris=cat("tris", np.int32), normals=cat("normals", np.float32) if normals else None,
                verts64=cat("verts64", np.float64))


# ------------------------------------------------------------------------------------------ measures of a mesh, in f64
def directed_edges(tris):
    t = np.asarray(tris, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented(tris):
    """Every directed edge occurs exactly once and its reverse exactly once."""
    e = directed_edges(tris)
    if e.size == 0:
        return True
    top = int(e.max()) + 1
    key, rev = e[:, 0] * top + e[:, 1], e[:, 1] * top + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).all()) and np.array_equal(uniq, np.unique(rev))


def euler_characteristic(tris):
    t = np.asarray(tris, dtype=np.int64)
    e = np.sort(directed_edges(t), axis=1)
    return int(np.unique(t).size) - int(np.unique(e, axis=0).shape[0]) + int(t.shape[0])


def volume_terms(verts, tris):
    """The divergence-theorem terms p0 . (p1 x p2) / 6 of every triangle."""
    p = np.asarray(verts, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0


def area(verts, tris):
    p = np.asarray(verts, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    return float(0.5 * np.sqrt((np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) ** 2).sum(-1)).sum())


def _tet_volume(a, b, c, d):
    return np.abs(np.einsum("ij,ij->i", b - a, np.cross(c - a, d - a))) / 6.0


def inside_volume(vol, level, bounds):
    """The volume of the part of the grid's box on which the piecewise linear interpolant (linear on every Kuhn tetrahedron) is above `level`:
    tetrahedron by tetrahedron, the part is cut into tetrahedra and their |det| / 6 are added.  Independent of `mesh`: no table, no winding."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    n = vol.shape
    axes = [np.linspace(float(b[0]), float(b[1]), n[a]) for a, b in enumerate(bounds)]
    X = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = np.arange(vol.size).reshape(n)
    base = idx[:-1, :-1, :-1].ravel()
    strides = (n[1] * n[2], n[2], 1)
    f = vol.ravel().astype(np.float64) - np.float64(np.float32(level))
    total = 0.0
    for a, b, c in PERMS:
        corner = [base, base + strides[a], base + strides[a] + strides[b], base + strides[a] + strides[b] + strides[c]]
        F = np.stack([f[i] for i in corner], axis=1)
        Q = np.stack([X[i] for i in corner], axis=1)
        above = F > 0
        # sort the corners of every tetrahedron: those above first (a stable order; volumes are unsigned)
        order = np.argsort(~above, axis=1, kind="stable")
        F, Q, cnt = np.take_along_axis(F, order, 1), np.take_along_axis(Q, order[:, :, None], 1), above.sum(1)

        def cut(sel, i, j):          # the point of edge (i above, j not above) where the interpolant is 0
            t = F[sel, i] / (F[sel, i] - F[sel, j])
            return Q[sel, i] + t[:, None] * (Q[sel, j] - Q[sel, i])

        s = cnt == 4
        total += _tet_volume(Q[s, 0], Q[s, 1], Q[s, 2], Q[s, 3]).sum()
        s = cnt == 1
        total += _tet_volume(Q[s, 0], cut(s, 0, 1), cut(s, 0, 2), cut(s, 0, 3)).sum()
        s = cnt == 2          # the prism between the triangles (0, 02, 03) and (1, 12, 13)
        p02, p03, p12, p13 = cut(s, 0, 2), cut(s, 0, 3), cut(s, 1, 2), cut(s, 1, 3)
        total += (_tet_volume(Q[s, 0], p02, p03, Q[s, 1]) + _tet_volume(p02, p03, Q[s, 1], p12) + _tet_volume(p03, Q[s, 1], p12, p13)).sum()
        s = cnt == 3          # the prism between the triangles (0, 1, 2) and (03, 13, 23)
        p03, p13, p23 = cut(s, 0, 3), cut(s, 1, 3), cut(s, 2, 3)
        total += (_tet_volume(Q[s, 0], Q[s, 1], Q[s, 2], p03) + _tet_volume(Q[s, 1], Q[s, 2], p03, p13) + _tet_volume(Q[s, 2], p03, p13, p23)).sum()
    return float(total)


# ------------------------------------------------------------------------------------------ fields
def _coords(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def random_volume(shape, seed):
    return np.random.default_rng(1000 + seed).random(shape, dtype=np.float32)


def checkerboard(shape, phase=0):
    i, j, k = _coords(shape)
    return (((i + j + k + phase) % 2) == 0).astype(np.float32)


def ball(shape, radius=None, centre=None):
    """radius - |x - centre| in nodes: positive inside."""
    c = [(s - 1) / 2.0 for s in shape] if centre is None else centre
    r = 0.43 * (min(shape) - 1) if radius is None else radius
    i, j, k = _coords(shape)
    return (r - np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2)).astype(np.float32)


def torus(shape, major=None, minor=None):
    """minor - the distance from the circle of radius `major` around axis 0 through the centre."""
    c = [(s - 1) / 2.0 for s in shape]
    R = 0.3 * (min(shape[1:]) - 1) if major is None else major
    r = 0.4 * R if minor is None else minor
    i, j, k = _coords(shape)
    ring = np.sqrt((j - c[1]) ** 2 + (k - c[2]) ** 2) - R
    return (r - np.sqrt(ring ** 2 + (i - c[0]) ** 2)).astype(np.float32)


def two_balls(shape):
    c = [(s - 1) / 2.0 for s in shape]
    r = 0.2 * (min(shape) - 1)
    a = ball(shape, r, (c[0], c[1], c[2] - 1.3 * r))
    b = ball(shape, r, (c[0], c[1], c[2] + 1.3 * r))
    return np.maximum(a, b)


def branching_tube(shape):
    """A trunk along axis 2 that forks into two branches, phantom-style: the maximum over capsules of clip(0.5 + (radius - distance), 0, 1)."""
    i, j, k = _coords(shape)
    X = np.stack([i, j, k], axis=-1)
    c = np.array([(s - 1) / 2.0 for s in shape])
    L = shape[2] - 1
    segs = [((c[0], c[1], 0.15 * L), (c[0], c[1], 0.5 * L), 0.16, 0.13), ((c[0], c[1], 0.5 * L), (c[0] - 0.22 * (shape[0] - 1), c[1] + 0.2 * (shape[1] - 1), 0.85 * L), 0.13, 0.08),
            ((c[0], c[1], 0.5 * L), (c[0] + 0.22 * (shape[0] - 1), c[1] - 0.2 * (shape[1] - 1), 0.8 * L), 0.12, 0.08)]
    out = np.zeros(shape)
    for a, b, ra, rb in segs:
        a, b = np.array(a), np.array(b)
        ab = b - a
        t = np.clip(((X - a) @ ab) / (ab @ ab), 0.0, 1.0)
        d = np.sqrt((((X - a) - t[..., None] * ab) ** 2).sum(-1))
        r = (ra + t * (rb - ra)) * min(shape)
        out = np.maximum(out, np.clip(0.5 + (r - d), 0.0, 1.0))
    return out.astype(np.float32)


def zero_border(vol, value=0.0):
    v = np.array(vol, dtype=np.float32)
    for a in range(3):
        s = [slice(None)] * 3
        s[a] = 0
        v[tuple(s)] = value
        s[a] = -1
        v[tuple(s)] = value
    return v


# ------------------------------------------------------------------------------------------ the cases of the GPU tests
# the grid of the raw launches (nca_testlib.grid_of): a lo that is not 0 and a spacing of its own on every axis
LO, INV = (0.0, -1.0, 2.0), (1.0, 2.0, 0.5)
# The tile is 4 x 8 x 64 nodes; the scan takes SCAN_CHUNK nodes per workgroup and SCAN_BATCH workgroup sums per round of its second level
SCAN_CHUNK, SCAN_BATCH = 1024, 256
GPU_SHAPES = ((2, 2, 2), (3, 3, 3), (4, 5, 6), (5, 9, 65), (9, 17, 130))
# one node more than SCAN_CHUNK * SCAN_BATCH = 2^18 nodes: the second level of the scan carries from its first round into a second
PAST_ONE_SCAN_ROUND = (3, 3, 29128)
assert 9 * 29127 < SCAN_CHUNK * SCAN_BATCH < 9 * 29128
CASE_NAMES = ("random", "checkerboard", "ball", "torus", "empty and full", "at level", "nonfinite")


def case(shape, name):
    """(stack f32 [2,n0,n1,n2] of two volumes that differ, level)."""
    if name == "random":
        return np.stack([random_volume(shape, 0), random_volume(shape, 1)]), 0.5
    if name == "checkerboard":
        return np.stack([checkerboard(shape, 0), checkerboard(shape, 1)]), 0.5
    if name == "ball":
        c = [(s - 1) / 2.0 for s in shape]
        return np.stack([ball(shape), ball(shape, 0.3 * (min(shape) - 1), (c[0] + 0.2, c[1] - 0.3, c[2] + 0.6))]), 0.0
    if name == "torus":
        return np.stack([torus(shape), torus(shape, 0.35 * (min(shape[1:]) - 1))]), 0.0
    if name == "empty and full":
        return np.stack([np.zeros(shape, dtype=np.float32), np.ones(shape, dtype=np.float32)]), 0.5
    if name == "at level":          # small integers: about a third of the nodes lie exactly at the level
        rng = np.random.default_rng(77)
        return rng.integers(0, 3, size=(2,) + tuple(shape)).astype(np.float32), 1.0
    if name == "nonfinite":
        rng = np.random.default_rng(78)
        v = rng.random((2,) + tuple(shape), dtype=np.float32)
        kind = rng.integers(0, 12, size=v.shape)
        v[kind == 0] = np.nan
        v[kind == 1] = np.inf
        v[kind == 2] = -np.inf
        return v, 0.5
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(shape, name):
    """stack_mesh of case (shape, name) with normals on the grid (LO, INV): computed once per case, never modified (read-only arrays)."""
    stack, level = case(shape, name)
    out = stack_mesh(stack, level, LO, INV, normals=True)
    for v in out.values():
        v.setflags(write=False)
    return out
