"""The numpy oracle of the connected components (include/nerfca_hip.h, "label"): a union-find over the edges of the definition, numbered
by smallest linear index, and the cases the CPU and the GPU tests share.  tests/test_label_cpu.py holds it to scipy.ndimage.label."""
import functools

import numpy as np

# the shapes of skel_ref.GPU_SHAPES, re-stated: test modules do not import from one another.  (2,2,2), (3,3,3), (4,5,6): one tile of
# 4 x 8 x 64; (5,9,65), (7,9,70): seams of one node and more on every axis; (9,17,130): a tile with neighbours on both sides
GPU_SHAPES = ((2, 2, 2), (3, 3, 3), (4, 5, 6), (5, 9, 65), (7, 9, 70), (9, 17, 130))
CONNECTIVITIES = (1, 2, 3)
TILE = (4, 8, 64)


def forward_offsets(connectivity):
    """The forward half of the neighbourhood: the offsets after (0,0,0) in raster order with at most `connectivity` non-zero entries:
    3 / 9 / 13 of them."""
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0) and (a != 0) + (b != 0) + (c != 0) <= connectivity]


def mask_of(vol, threshold, invert=False):
    """M of the definition: (double)vol > threshold, a NaN is not; inverted with `invert`."""
    with np.errstate(invalid="ignore"):
        m = np.asarray(vol, dtype=np.float32).astype(np.float64) > float(threshold)
    return ~m if invert else m


def label_mask(mask, connectivity):
    """(labels int32 of mask's shape, count) of ONE volume's bool mask [n0, n1, n2].  Every pair of neighbouring mask nodes is an edge; the
    root of the larger-rooted end is hooked under the smaller root (np.minimum.at) and all paths are compressed, until every edge has one
    root at both ends.  A root is then the smallest index of its component, and the components are numbered by it."""
    assert mask.dtype == np.bool_ and mask.ndim == 3
    n = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(n)
    us, vs = [], []
    for o in forward_offsets(connectivity):
        a = tuple(slice(max(0, -d), n[k] - max(0, d)) for k, d in enumerate(o))
        b = tuple(slice(max(0, d), n[k] - max(0, -d)) for k, d in enumerate(o))
        both = mask[a] & mask[b]
        us.append(idx[a][both])
        vs.append(idx[b][both])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(mask.size, dtype=np.int64)
    while True:
        ru, rv = parent[u], parent[v]
        differ = ru != rv
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ru, rv)[differ], np.minimum(ru, rv)[differ])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    flat = mask.ravel()
    roots = np.flatnonzero(flat & (parent == np.arange(mask.size)))          # ascending: the numbering
    rank = np.zeros(mask.size, dtype=np.int32)
    rank[roots] = np.arange(1, roots.size + 1, dtype=np.int32)
    labels = np.where(flat, rank[parent], 0).astype(np.int32).reshape(n)
    return labels, int(roots.size)


def label(vol, threshold, connectivity, invert=False):
    """(labels int32 [n_vol, n0, n1, n2], counts int32 [n_vol]) of an f32 stack: every volume on its own."""
    vol = np.asarray(vol, dtype=np.float32)
    assert vol.ndim == 4
    out = [label_mask(mask_of(x, threshold, invert), connectivity) for x in vol]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


def sizes(labels, cap):
    """int32 [n_vol, cap]: the nodes of every label in [0, cap) per volume; labels outside are not counted."""
    out = np.zeros((labels.shape[0], cap), dtype=np.int32)
    for v, x in enumerate(labels):
        x = x.ravel()
        x = x[(x >= 0) & (x < cap)]
        out[v] = np.bincount(x, minlength=cap)[:cap]
    return out


# ----------------------------------------------------------------------------- masks
def random_volume(shape, seed):
    """f32 uniform in [0, 1): `> 1 - d` is a mask of density d."""
    return np.random.default_rng(77 * seed + 7 * shape[0] + 3 * shape[1] + shape[2]).random(shape).astype(np.float32)


def checkerboard(shape, phase=0):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2 == phase).astype(np.float32)


def serpentine(shape):
    """A single path one node wide, as f32 0 / 1: in every even slab i0 every even row i1 is a full line along axis 2, consecutive lines are
    joined by one node at alternating ends, and consecutive even slabs by one node of the odd slab between them, below the end of the last
    line.  Node (0,0,0) is on it.  One component at every connectivity; along axis 2 it crosses every tile seam in every line."""
    m = np.zeros(shape, dtype=np.float32)
    n0, n1, n2 = shape
    col = 0          # where along axis 2 the path stands
    for s in range(0, n0, 2):
        rows = list(range(0, n1, 2))
        if (s // 2) % 2:
            rows.reverse()
        for q, r in enumerate(rows):
            m[s, r, :] = 1.0
            col = n2 - 1 - col
            if q + 1 < len(rows):
                m[s, (r + rows[q + 1]) // 2, col] = 1.0
        if s + 2 < n0:
            m[s + 1, rows[-1], col] = 1.0
    return m


def two_serpentines(shape):
    """Two paths that touch only diagonally, at a corner of the first tile: A fills the tile [0,4) x [0,8) x [0,64) as a serpentine turned
    round so that it ends in (3,7,63); B is a serpentine of the box from (3,8,64) on, and (4,8,64).  (3,7,63) and (3,8,64) differ along two
    axes, (3,7,63) and (4,8,64) along three, and no node of A differs from a node of B along fewer than two."""
    assert shape[0] > TILE[0] and shape[1] > TILE[1] and shape[2] > TILE[2], shape
    m = np.zeros(shape, dtype=np.float32)
    m[:TILE[0], :TILE[1], :TILE[2]] = serpentine(TILE)[::-1, ::-1, ::-1]
    m[TILE[0] - 1:, TILE[1]:, TILE[2]:] = serpentine((shape[0] - TILE[0] + 1, shape[1] - TILE[1], shape[2] - TILE[2]))
    m[TILE[0], TILE[1], TILE[2]] = 1.0
    assert m[3, 7, 63] == 1.0 and m[3, 8, 64] == 1.0
    return m


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(name, stack f32 [2, n0, n1, n2] of two different volumes, threshold, invert)] of one shape."""
    out = []
    rnd = np.stack([random_volume(shape, 0), random_volume(shape, 1)])
    for d in (0.3, 0.5, 0.7):
        out.append((f"random {d}", rnd, 1.0 - d, False))
        out.append((f"random {d} inverted", rnd, d, True))
    out.append(("empty", np.stack([np.zeros(shape, dtype=np.float32), (rnd[1] > 0.5).astype(np.float32)]), 0.5, False))
    out.append(("full", np.stack([np.ones(shape, dtype=np.float32), (rnd[0] > 0.5).astype(np.float32)]), 0.5, False))
    out.append(("checkerboard", np.stack([checkerboard(shape, 0), checkerboard(shape, 1)]), 0.5, False))
    nan = rnd.copy()
    nan[0][tuple(s // 2 for s in shape)] = np.nan
    nan[0][0, 0, 0] = np.nan
    nan[1][tuple(s - 1 for s in shape)] = np.nan
    out.append(("nan", nan, 0.4, False))
    out.append(("nan inverted", nan, 0.6, True))
    snake = serpentine(shape)
    cut = snake.copy()
    cut[0, 0, shape[2] // 2] = 0.0          # the same path cut in its first line
    out.append(("serpentine", np.stack([snake, cut]), 0.5, False))
    if all(s > t for s, t in zip(shape, TILE)):
        out.append(("two serpentines", np.stack([two_serpentines(shape), snake]), 0.5, False))
    for name, stack, _, _ in out:
        assert stack.dtype == np.float32 and stack.shape == (2,) + tuple(shape) and not np.array_equal(stack[0], stack[1], equal_nan=True), name
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, name, connectivity):
    """The oracle's (labels, counts) of one case: computed once and shared."""
    for n, stack, thr, inv in cases(shape):
        if n == name:
            return label(stack, thr, connectivity, inv)
    raise KeyError(name)


# ----------------------------------------------------------------------------- the phantom tree with planted specks
TREE_SIDE = 32
SPECKS = ((1, 1, 1), (1, 30, 2), (30, 1, 29), (29, 30, 30), (2, 15, 30))          # one node each, in the corners and on a face of the grid


@functools.lru_cache(maxsize=None)
def tree_with_specks(side=TREE_SIDE, radius=1.5):
    """(tree f32 [side]^3, speckled f32 [side]^3, the number of specks): the centreline of the seed-0 phantom tree (phase 0) rasterised at
    the nearest node and thickened to `radius` nodes, reduced to its largest 26-connected component (by the oracle), and the same with
    single nodes planted at least 3 nodes away from it."""
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
    mask = scipy.ndimage.distance_transform_edt(~centre) <= radius
    lab, n = label_mask(mask, 3)
    tree = lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
    away = scipy.ndimage.distance_transform_edt(~tree)
    speckled = tree.copy()
    planted = 0
    for s in SPECKS:
        if away[s] >= 3.0:
            speckled[s] = True
            planted += 1
    assert planted >= 3 and tree.sum() > 100
    return tree.astype(np.float32), speckled.astype(np.float32), planted
