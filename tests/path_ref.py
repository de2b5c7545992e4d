"""The numpy transcription of the minimal-path definition of include/nerfca_hip.h ("path"): the edge list with the two expressions len(d) and
w(u, v), a heap Dijkstra on it, the sweep-by-sweep state (every tile of 4 x 8 x 64 nodes brought to its own fixed point with the nodes outside
it frozen at the previous state -- as Jacobi rounds over the tile's edges, which end at the same unique fixed point as a per-tile Dijkstra;
tests/test_path_cpu.py holds the converged state to the heap Dijkstra's bits), the predecessor field, trace, ball cover, and the whole
centreline.extract loop with scipy's Euclidean distance transform for R.  Plus the grids and inputs the CPU and the GPU tests share."""
import heapq

import numpy as np

TILE = (4, 8, 64)


def offsets(conn):
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 1 <= (a != 0) + (b != 0) + (c != 0) <= conn]


def spacing(inv):
    return [1.0 / float(v) for v in inv]


def inv_of(shape, bounds):
    """inv as drr.grid_desc forms it"""
    return [(shape[a] - 1) / (float(bounds[a][1]) - float(bounds[a][0])) for a in range(3)]


def lengths(inv, conn):
    h = spacing(inv)
    out = []
    for d in offsets(conn):
        a0, a1, a2 = d[0] * h[0], d[1] * h[1], d[2] * h[2]
        out.append(float(np.sqrt(np.float64((a0 * a0 + a1 * a1) + a2 * a2))))
    return out


def is_open(cost):
    with np.errstate(invalid="ignore"):
        return np.isfinite(cost) & (cost >= 0)


class Graph:
    """The directed edges (v <- u) between open nodes of ONE volume, sorted by v and within v by offset order; w in f64."""

    def __init__(self, cost, inv, conn):
        cost = np.asarray(cost, dtype=np.float32)
        self.shape = cost.shape
        n0, n1, n2 = cost.shape
        self.open = is_open(cost)
        idx = np.arange(cost.size).reshape(cost.shape)
        c64 = cost.astype(np.float64)
        tile = ((idx // (n1 * n2)) // TILE[0] * 4096 + ((idx // n2) % n1) // TILE[1]) * 4096 + (idx % n2) // TILE[2]
        self.tile = tile.reshape(-1)
        vs, us, ws, js = [], [], [], []
        for j, (d, ln) in enumerate(zip(offsets(conn), lengths(inv, conn))):
            sv = tuple(slice(max(0, -d[a]), cost.shape[a] - max(0, d[a])) for a in range(3))
            su = tuple(slice(max(0, d[a]), cost.shape[a] - max(0, -d[a])) for a in range(3))
            both = self.open[sv] & self.open[su]
            v, u = idx[sv][both], idx[su][both]
            with np.errstate(invalid="ignore", over="ignore"):
                w = ln * (0.5 * (c64[su][both] + c64[sv][both]))
            vs.append(v), us.append(u), ws.append(w), js.append(np.full(v.shape, j))
        v, u, w, j = (np.concatenate(x) for x in (vs, us, ws, js))
        order = np.lexsort((j, v))
        self.v, self.u, self.w, self.j = v[order], u[order], w[order], j[order]
        self.nodes, self.start = np.unique(self.v, return_index=True)          # the open nodes with at least one open neighbour
        self.same = self.tile[self.v] == self.tile[self.u]
        self.end = np.append(self.start[1:], self.v.size)

    def clean(self, dist):
        d = np.array(dist, dtype=np.float64).reshape(-1)
        d[~self.open.reshape(-1)] = np.inf
        return d

    def dijkstra(self, dist):
        """The fixed point from the in/out field `dist`, by a heap"""
        d = self.clean(dist)
        first = np.full(d.size, -1)
        first[self.nodes] = self.start
        last = np.zeros(d.size, dtype=np.int64)
        last[self.nodes] = self.end
        heap = [(float(d[i]), int(i)) for i in np.flatnonzero(np.isfinite(d))]
        heapq.heapify(heap)
        done = np.zeros(d.size, dtype=bool)
        while heap:
            dv, v = heapq.heappop(heap)
            if done[v] or dv > d[v]:
                continue
            done[v] = True
            if first[v] < 0:
                continue
            for e in range(first[v], last[v]):
                u = self.u[e]
                cand = np.float64(dv) + self.w[e]
                if cand < d[u]:
                    d[u] = cand
                    heapq.heappush(heap, (float(cand), int(u)))
        return d.reshape(self.shape)

    def sweep(self, prev):
        """(state s, the number of tiles that changed) from state s - 1"""
        prev = np.array(prev, dtype=np.float64).reshape(-1)
        cur = self.clean(prev)
        if self.v.size:
            for _ in range(2 * 2048 + 2):
                cand = np.where(self.same, cur[self.u], prev[self.u]) + self.w
                best = np.minimum(np.minimum.reduceat(cand, self.start), cur[self.nodes])
                if np.array_equal(best, cur[self.nodes]):
                    break
                cur[self.nodes] = best
            else:
                raise AssertionError("a tile did not reach its fixed point")
        with np.errstate(invalid="ignore"):
            changed = np.unique(self.tile[cur != prev]).size
        return cur.reshape(self.shape), changed

    def sweeps(self, dist, n):
        """the states after 1 .. n sweeps and their changed counts"""
        out, d = [], dist
        for _ in range(n):
            d, c = self.sweep(d)
            out.append((d, c))
        return out

    def converge(self, dist, cap=200):
        """(the fixed point, the number of sweeps up to and including the first one that changed nothing)"""
        d = dist
        for s in range(1, cap + 1):
            d, c = self.sweep(d)
            if c == 0:
                return d, s
        raise AssertionError("no fixed point")

    def pred(self, dist):
        d = np.asarray(dist, dtype=np.float64).reshape(-1)
        out = np.full(d.size, -1, dtype=np.int32)
        ok = d[self.u] < d[self.v]
        v, u, j = self.v[ok], self.u[ok], self.j[ok]
        cand = d[u] + self.w[ok]
        order = np.lexsort((j, cand, v))
        v, u = v[order], u[order]
        firsts = np.ones(v.size, dtype=bool)
        firsts[1:] = v[1:] != v[:-1]
        out[v[firsts]] = u[firsts]
        return out.reshape(self.shape)


def geodesic(cost, dist, inv, conn):
    return Graph(cost, inv, conn).dijkstra(dist)


def seeded(shape, seeds):
    d = np.full(shape, np.inf)
    d.reshape(-1)[list(seeds)] = 0.0
    return d


def trace(pred, starts, stop, max_len):
    pred = np.asarray(pred).reshape(-1)
    stop = None if stop is None else np.asarray(stop).reshape(-1)
    paths = np.full((len(starts), max_len), -1, dtype=np.int32)
    lens, status = np.zeros(len(starts), dtype=np.int32), np.zeros(len(starts), dtype=np.int32)
    for p, x in enumerate(starts):
        n, st = 0, 3
        if 0 <= x < pred.size:
            st = 2
            while n < max_len:
                paths[p, n] = x
                n += 1
                if stop is not None and stop[x]:
                    st = 1
                    break
                nx = int(pred[x])
                if not 0 <= nx < pred.size:
                    st = 0
                    break
                x = nx
        lens[p], status[p] = n, st
    return paths, lens, status


def cover(covered, nodes, radius, inv):
    covered = np.array(covered, dtype=np.uint8)
    n0, n1, n2 = covered.shape
    h = spacing(inv)
    x0, x1, x2 = np.meshgrid(np.arange(n0), np.arange(n1), np.arange(n2), indexing="ij")
    for node, r in zip(nodes, np.asarray(radius, dtype=np.float32)):
        if node < 0 or node >= covered.size:
            continue
        p0, p1, p2 = node // (n1 * n2), (node // n2) % n1, node % n2
        a0, a1, a2 = (x0 - p0).astype(np.float64) * h[0], (x1 - p1).astype(np.float64) * h[1], (x2 - p2).astype(np.float64) * h[2]
        with np.errstate(invalid="ignore"):
            covered[(a0 * a0 + a1 * a1) + a2 * a2 <= np.float64(r) * np.float64(r)] = 1
    return covered


def edt_inside(mask, inv):
    import scipy.ndimage
    return scipy.ndimage.distance_transform_edt(mask, sampling=spacing(inv)).astype(np.float32)


def extract(vol, bounds, threshold, root=None, scale=1.5, const=None, pdrf_scale=5000.0, pdrf_exponent=16, max_paths=256, R=None):
    """centreline.extract step by step: (paths, parents, radii, lengths, reached).  `R`: the distance transform to use instead of scipy's."""
    vol = np.asarray(vol, dtype=np.float32)
    shape = vol.shape
    inv = inv_of(shape, bounds)
    h = spacing(inv)
    if const is None:
        const = 2.0 * max(h)
    mask = vol > threshold
    if not mask.any():
        return [], [], [], [], 0.0
    R = edt_inside(mask, inv) if R is None else np.asarray(R, dtype=np.float32)
    Rm = np.where(mask, R, np.float32(-1.0))
    r_max = Rm.max()
    if root is None:
        root_i = int(np.argmax(Rm.reshape(-1) == r_max))
    else:
        i = [int(np.floor((float(root[a]) - float(bounds[a][0])) * inv[a] + 0.5)) for a in range(3)]
        root_i = (i[0] * shape[1] + i[1]) * shape[2] + i[2]
    nan = np.float32(np.nan)
    g0 = Graph(np.where(mask, np.float32(1.0), nan), inv, 3).dijkstra(seeded(shape, [root_i]))
    reach = np.isfinite(g0) & mask
    xx = 1.0 - R.astype(np.float64) / (np.float64(r_max) * 1.01)
    p = xx
    for _ in range(pdrf_exponent - 1):
        p = p * xx
    c = np.where(mask, (p * float(pdrf_scale) + 1.0).astype(np.float32), nan)
    graph = Graph(c, inv, 3)
    tree = np.zeros(shape, dtype=np.uint8)
    tree.reshape(-1)[root_i] = 1
    covered = np.zeros(shape, dtype=np.uint8)
    g1 = np.full(shape, np.inf)
    radius_of = (R.astype(np.float64) * float(scale) + float(const)).astype(np.float32).reshape(-1)
    n_reach = int(reach.sum())
    paths = []
    while len(paths) < max_paths:
        cand = np.where(reach & (covered == 0), g0, -1.0)
        if cand.max() < 0:
            break
        tip = int(np.argmax(cand.reshape(-1) == cand.max()))
        g1 = graph.dijkstra(np.where(tree != 0, 0.0, g1))
        pred = graph.pred(g1)
        rows, lens, _ = trace(pred, [tip], tree, n_reach)
        nodes = rows[0, :lens[0]]
        tree.reshape(-1)[nodes] = 1
        covered = cover(covered, nodes, radius_of[nodes], inv)
        paths.append(nodes.copy())
    where, parents = {}, []
    for k, nodes in enumerate(paths):
        parents.append(where.get(int(nodes[-1]), (-1, -1)))
        for pos, node in enumerate(nodes.tolist()):
            where.setdefault(node, (k, pos))
    radii = [R.reshape(-1)[nodes] for nodes in paths]
    lens = []
    for nodes in paths:
        ijk = np.stack(np.unravel_index(nodes, shape), axis=1).astype(np.float64)
        lens.append(float(np.sqrt((((ijk[1:] - ijk[:-1]) * np.array(h)) ** 2).sum(axis=1)).sum()))
    return paths, parents, radii, lens, n_reach / int(mask.sum())


# ------------------------------------------------------------------------------------------------------------- what the tests share
GRIDS = ((2, 2, 2), (4, 8, 64), (5, 9, 65))
SERPENTINE = (9, 17, 130)
INVS = ((1.0, 2.0, 3.0), (1.0, 1.0, 1.0))


def random_cost(shape, seed, walls=0.3, zeros=0.15):
    """f32 costs in [0, 2) with exact zeros, and walls as NaN, +inf, -inf and negative values in turn"""
    rng = np.random.default_rng(seed)
    c = (rng.random(shape) * 2.0).astype(np.float32)
    c[rng.random(shape) < zeros] = 0.0
    kind = rng.integers(0, 4, size=shape)
    wall = rng.random(shape) < walls
    for k, val in enumerate((np.nan, np.inf, -np.inf, -0.5)):
        c[wall & (kind == k)] = val
    return c


def random_seeds(cost, seed, count=2):
    """`count` open nodes (flat indices); the first open node when there are fewer"""
    op = np.flatnonzero(is_open(cost).reshape(-1))
    rng = np.random.default_rng(seed)
    return sorted(set(int(v) for v in rng.choice(op, size=min(count, op.size), replace=False)))


SERPENTINE_WAYPOINTS = ((0, 0, 0), (0, 0, 129), (0, 9, 129), (0, 9, 60), (5, 9, 60), (5, 9, 129), (5, 16, 129), (5, 16, 0), (8, 16, 0), (8, 2, 0), (8, 2, 70),
                        (2, 2, 70))


def serpentine(seed=7):
    """(cost, the seed's flat index) on SERPENTINE: a channel one node wide along axis-parallel segments that crosses tile faces of all three
    axes seventeen times; everything else is a wall (of every kind)."""
    rng = np.random.default_rng(seed)
    walls = random_cost(SERPENTINE, seed, walls=1.0)
    cost = walls.copy()
    pts = SERPENTINE_WAYPOINTS
    for a, b in zip(pts[:-1], pts[1:]):
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        seg = tuple(slice(int(lo[k]), int(hi[k]) + 1) for k in range(3))
        cost[seg] = 1.0
    chan = cost == 1.0
    vals = (rng.random(SERPENTINE) * 2.0).astype(np.float32)
    vals[rng.random(SERPENTINE) < 0.15] = 0.0
    cost[chan] = vals[chan]
    assert not is_open(walls).any()
    return cost, 0


def tube(shape, segments, inv=(1.0, 1.0, 1.0)):
    """f32 volume: 1 within `radius` (world units) of one of the segments ((a, b, radius), a and b in node coordinates), else 0"""
    h = np.array(spacing(inv))
    x = np.stack(np.meshgrid(*(np.arange(n) for n in shape), indexing="ij"), axis=-1).astype(np.float64)
    vol = np.zeros(shape, dtype=np.float32)
    for a, b, radius in segments:
        a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        e = (b - a) * h
        q = (x - a) * h
        t = np.clip((q * e).sum(-1) / max(float((e * e).sum()), 1e-300), 0.0, 1.0)
        d = np.sqrt(((q - t[..., None] * e) ** 2).sum(-1))
        vol[d <= radius] = 1.0
    return vol


Y_SHAPE = (17, 33, 70)
Y_SEGMENTS = (((8, 16, 3), (8, 16, 40), 3.0), ((8, 16, 40), (8, 27, 66), 2.5), ((8, 16, 40), (8, 5, 64), 2.0))
Y_INVS = ((1.0, 1.0, 1.0), (1.25, 1.0, 0.8))          # spacings (1, 1, 1) and (0.8, 1, 1.25)


def bounds_of(shape, inv):
    return tuple((0.0, (shape[a] - 1) / inv[a]) for a in range(3))
