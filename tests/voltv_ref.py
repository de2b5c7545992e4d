"""The f64 numpy transcription of the smoothed total variation of include/nerfca_hip.h ("vol"), which the voltv tests hold the kernels to:
every operation one rounded f64 operation in the order the header writes it.  Plus the shapes and stacks the tests share, and the same
functional as a torch expression (the autograd of which pins this oracle on the CPU)."""
import numpy as np
import torch

import drr_ref

# drr_ref.GRIDS; a grid no multiple of the 4 x 8 x 64 tile on any axis with several tiles on the first two; one that exceeds the tile by ONE node
# on every axis
GRIDS = drr_ref.GRIDS + [(33, 18, 67), (5, 9, 65)]
N_VOLS = (1, 2, 3, 11)
EPS_S, EPS_T = 1e-3, 2e-3
U = 2.0 ** -53


def grid_inv(shape, bounds):
    """inv f64 [3] = (n - 1) / (hi - lo), as drr.grid_desc forms it."""
    return [(int(n) - 1) / (float(b[1]) - float(b[0])) for n, b in zip(shape, bounds)]


def stack(n_vol, shape, seed):
    """f32 [n_vol,n0,n1,n2]: a random stack in which volume 0 has a flat row neighbourhood (m == eps_s there) and, from two volumes on,
    volumes 0 and 1 agree on a block of nodes (a flat phase pair: mt == eps_t there)."""
    x = drr_ref.random_volume((n_vol,) + tuple(shape), seed)
    x[0, : 2, : 2, :] = 0.25          # the node (0, 0, i2 < n2 - 1) sees no difference on any axis
    if n_vol >= 2:
        x[1, -2:, :, :] = x[0, -2:, :, :]
    return x


def pairs(n_vol, cyclic):
    """[(p, q)]: the phase pairs of one stack."""
    out = [(p, p + 1) for p in range(n_vol - 1)]
    if cyclic and n_vol >= 2:
        out.append((n_vol - 1, 0))
    return out


def total_variation(x, inv, eps_s, eps_t, cyclic):
    """Of f32 x [n_vol,n0,n1,n2]: a dict of
    space, time        the two sums (f64), summed by numpy (only the order of these sums is free)
    abs_space/abs_time sum |term|
    count_space/_time  the number of summands
    g_s, g_t           f64 [n_vol,n0,n1,n2]
    mass               f64, the sum of the absolute values of the six quotients of g_s
    n_pairs"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    x = x.astype(np.float64)
    n_vol, n = x.shape[0], x.shape[1:]
    eps_s, eps_t = np.float64(eps_s), np.float64(eps_t)
    d = []
    for a in range(3):
        da = np.zeros_like(x)
        hi = [slice(None)] * 4
        lo = [slice(None)] * 4
        hi[a + 1], lo[a + 1] = slice(1, None), slice(None, -1)
        da[tuple(lo)] = (x[tuple(hi)] - x[tuple(lo)]) * inv[a]          # 0 stays at the last node of axis a
        d.append(da)
    m = np.sqrt(eps_s * eps_s + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    term_s = m - eps_s
    own = -(((d[0] * inv[0] + d[1] * inv[1]) + d[2] * inv[2]) / m)
    mass = np.zeros_like(x)
    back = []
    for a in range(3):
        q = (d[a] * inv[a]) / m
        mass += np.abs(q)
        b = np.zeros_like(x)
        hi = [slice(None)] * 4
        lo = [slice(None)] * 4
        hi[a + 1], lo[a + 1] = slice(1, None), slice(None, -1)
        b[tuple(hi)] = q[tuple(lo)]
        mass += np.abs(b)
        back.append(b)
    g_s = ((own + back[0]) + back[1]) + back[2]
    neg, pos = np.zeros_like(x), np.zeros_like(x)
    terms_t = []
    pr = pairs(n_vol, cyclic)
    for p, q in pr:
        t = x[q] - x[p]
        mt = np.sqrt(eps_t * eps_t + t * t)
        terms_t.append(mt - eps_t)
        neg[p] = -(t / mt)
        pos[q] = t / mt
    g_t = neg + pos
    term_t = np.stack(terms_t) if terms_t else np.zeros((0,) + n)
    return {"space": float(term_s.sum()), "time": float(term_t.sum()), "abs_space": float(np.abs(term_s).sum()), "abs_time": float(np.abs(term_t).sum()),
            "count_space": term_s.size, "count_time": term_t.size, "g_s": g_s, "g_t": g_t, "mass": mass, "n_pairs": len(pr)}


def torch_total_variation(x, inv, eps_s, eps_t, cyclic):
    """(space, time) of a torch stack [n_vol,n0,n1,n2] in ITS dtype: the expression a user of torch would write, differentiable by
    autograd."""
    pad = torch.nn.functional.pad
    d0 = pad((x[:, 1:] - x[:, :-1]) * inv[0], (0, 0, 0, 0, 0, 1))
    d1 = pad((x[:, :, 1:] - x[:, :, :-1]) * inv[1], (0, 0, 0, 1))
    d2 = pad((x[:, :, :, 1:] - x[:, :, :, :-1]) * inv[2], (0, 1))
    space = (torch.sqrt(eps_s * eps_s + ((d0 * d0 + d1 * d1) + d2 * d2)) - eps_s).sum()
    n_vol = x.shape[0]
    if n_vol == 1:
        return space, torch.zeros((), dtype=x.dtype, device=x.device)
    t = (torch.roll(x, -1, 0) - x) if cyclic else (x[1:] - x[:-1])
    return space, (torch.sqrt(eps_t * eps_t + t * t) - eps_t).sum()
