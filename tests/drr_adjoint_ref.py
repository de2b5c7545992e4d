"""The f64 numpy back-projector the drr gradient tests hold nca_drr_backproject to: a direct transcription of its definition in
include/nerfca_hip.h ("drr"), on the grid coordinates of tests/drr_ref.py.  Every product is a rounded f64 product in the header's
order; a node's sum is formed by np.add.at in (ray, s) order, one neighbour after the other."""
import numpy as np

import drr_ref


def _scatter(shape, n_vol, origins, dirs, z, dists, g_pix, bounds, unit_weights):
    n = tuple(int(k) for k in shape)
    g_pix = np.asarray(g_pix, dtype=np.float64).reshape(n_vol, origins.shape[0])
    dists = np.asarray(dists, dtype=np.float64)
    g = drr_ref.grid_coords(n, bounds, origins, dirs, z)                                  # [R,S,3]
    keep = ((g > -1.0) & (g < np.array(n, dtype=np.float64))).all(-1)                     # the forward's skip test (NaN: skipped)
    fl = np.floor(g)
    f = g - fl
    m = 1.0 - f
    i = np.where(keep[..., None], fl, 0.0).astype(np.int64)
    voxels = n[0] * n[1] * n[2]
    g_vol = np.zeros((n_vol, voxels), dtype=np.float64)
    mass = np.zeros((n_vol, voxels), dtype=np.float64)
    count = np.zeros(voxels, dtype=np.int64)
    t = [-(g_pix[v][:, None] * dists[None, :]) for v in range(n_vol)]                     # -(g_pix dists_s), [R,S]
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                k0, k1, k2 = i[..., 0] + a, i[..., 1] + b, i[..., 2] + c
                ok = keep & (k0 >= 0) & (k0 < n[0]) & (k1 >= 0) & (k1 < n[1]) & (k2 >= 0) & (k2 < n[2])
                x0, x1, x2 = (f if a else m)[..., 0], (f if b else m)[..., 1], (f if c else m)[..., 2]
                w = np.ones_like(x0) if unit_weights else (x0 * x1) * x2
                node = ((k0 * n[1] + k1) * n[2] + k2)[ok]
                np.add.at(count, node, 1)
                for v in range(n_vol):
                    contrib = (t[v] * w)[ok]
                    np.add.at(g_vol[v], node, contrib)
                    np.add.at(mass[v], node, np.abs(contrib))
    return g_vol.reshape((n_vol,) + n), mass.reshape((n_vol,) + n), count.reshape(n)


def backproject(shape, n_vol, origins, dirs, z, dists, g_pix, bounds):
    """(g_vol f64 [n_vol,n0,n1,n2], mass f64 [n_vol,n0,n1,n2], count int64 [n0,n1,n2]): per node the sum of contrib, the sum of
    |contrib| and the number of contributions (the same for every volume), for g_pix f64 [n_vol,R] (or [R] when n_vol is 1)."""
    return _scatter(shape, n_vol, origins, dirs, z, dists, g_pix, bounds, False)


def gross(shape, n_vol, origins, dirs, z, dists, g_pix, bounds):
    """f64 [n_vol,n0,n1,n2]: per node the sum of |g_pix dists_s| over its contributions (the weights left out)."""
    return _scatter(shape, n_vol, origins, dirs, z, dists, g_pix, bounds, True)[1]
