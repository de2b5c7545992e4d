"""The f64 numpy transcription of the structural similarity of include/nerfca_hip.h ("ssim"), which the ssim tests hold the kernels to:
every operation one rounded f64 operation in the order the header writes it (numpy's elementwise products and sums are single rounded
operations: nothing is contracted).  Plus the shapes, windows and image stacks the tests share, and the same functional as a torch
expression with conv2d (the autograd of which pins this oracle on the CPU)."""
import functools

import numpy as np
import torch

U = 2.0 ** -53
K1, K2 = 0.01, 0.03
RANGES = (1.0, 2.16, 0.37)
TILE = (16, 32)          # window positions (value) or pixels (gradient) per workgroup
# (K, (H, W)): one position; one row of positions past a tile's width; one row and one column past the 16 x 32 tile in positions (17 x 33)
# and, with the window's halo, in a 16 x 64 tile's; several tiles, ragged in both axes; and the small windows
CASES = [(11, (11, 11)), (11, (12, 75)), (11, (27, 43)), (11, (27, 75)), (11, (43, 130)), (3, (3, 3)), (3, (5, 70)), (1, (4, 66))]
N_IMAGES = (1, 3)


def gaussian(K, sigma=1.5):
    """Wang's window, written independently of metrics.gaussian_window: exp(-d^2 / (2 sigma^2)) normalised."""
    d = np.arange(K, dtype=np.float64) - (K - 1) / 2
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def asymmetric(K):
    """A window that is not its own mirror image (the C entry points take any weights): rising weights, normalised."""
    g = np.arange(1, K + 1, dtype=np.float64) ** 1.5 + 0.25
    return g / g.sum()


def _smooth(H, W, L):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return L * (0.5 + 0.3 * np.sin(0.23 * i + 0.4) * np.cos(0.17 * j - 0.2))


@functools.lru_cache(maxsize=None)
def stack(n, shape):
    """(x, y, range): f32 [n,H,W] pairs in [0, L] and f64 [n].  n == 3: a smooth pair under noise, a pair anti-correlated with its truth
    (S < 0 occurs), an identical pair.  n == 1: the anti-correlated pair alone."""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W + n)
    xs, ys = [], []
    kinds = ("smooth", "anti", "same") if n == 3 else ("anti",)
    ranges = np.array(RANGES[:n] if n == 3 else RANGES[1:2], dtype=np.float64)
    for kind, L in zip(kinds, ranges):
        noise = rng.random((H, W)) * L
        if kind == "smooth":
            y = np.clip(0.8 * _smooth(H, W, L) + 0.2 * noise, 0, L)
            x = np.clip(y + 0.1 * L * (rng.random((H, W)) - 0.5), 0, L)
        elif kind == "anti":
            y = noise
            x = np.clip((L - y) + 0.05 * L * (rng.random((H, W)) - 0.5), 0, L)
        else:
            x = y = noise
        xs.append(x.astype(np.float32))
        ys.append(y.astype(np.float32))
    x, y = np.stack(xs), np.stack(ys)
    x.setflags(write=False), y.setflags(write=False), ranges.setflags(write=False)
    return x, y, ranges


def moments(v, win):
    """m_v f64 [Hv,Wv] of one field v f64 [H,W]: the row pass, then the column pass, each a left-to-right sum starting from its first term."""
    K = len(win)
    H, W = v.shape
    Hv, Wv = H - K + 1, W - K + 1
    r = win[0] * v[:, 0:Wv]
    for b in range(1, K):
        r = r + win[b] * v[:, b:b + Wv]
    m = win[0] * r[0:Hv]
    for a in range(1, K):
        m = m + win[a] * r[a:a + Hv]
    return m


def spread(M, win, H, W):
    """F[M] f64 [H,W] of a map M [Hv,Wv]: f_M(i', j) = sum_b win[b] M(i', j - b), F(i, j) = sum_a win[a] f_M(i - a, j), increasing index, a term
    outside the map skipped: the first term inside starts the sum."""
    K = len(win)
    Hv, Wv = M.shape
    f = np.zeros((Hv, W))
    started = np.zeros(W, dtype=bool)
    for b in range(K):
        t = win[b] * M
        sl = slice(b, b + Wv)
        f[:, sl] = np.where(started[sl][None, :], f[:, sl] + t, t)
        started[sl] = True
    assert started.all()
    F = np.zeros((H, W))
    started = np.zeros(H, dtype=bool)
    for a in range(K):
        t = win[a] * f
        sl = slice(a, a + Hv)
        F[sl] = np.where(started[sl][:, None], F[sl] + t, t)
        started[sl] = True
    assert started.all()
    return F


def ssim_image(x, y, L, win, k1=K1, k2=K2):
    """Of one f32 pair [H,W]: a dict of
    S            f64 [Hv,Wv]
    sum, abs_sum the sum of S and of |S| (numpy's order: only the order of this sum is free), count = Hv Wv
    P, Q, R      the coefficient maps
    grad         f64 [H,W], d sum / d x (scale 1)
    mass         f64 [H,W], the sum of the absolute values of every term added into a pixel: F[|P|] + |x| F[|Q|] + |y| F[|R|]
    m            the five moment maps;   b1b2, c1c2: for the check that no case sits on a pole"""
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.ndim == 2 and x.shape == y.shape
    win = np.asarray(win, dtype=np.float64)
    H, W = x.shape
    x, y, L = x.astype(np.float64), y.astype(np.float64), float(L)
    good = np.isfinite(L) and L > 0
    C1, C2 = (k1 * L) * (k1 * L), (k2 * L) * (k2 * L)
    m = {name: moments(v, win) for name, v in (("x", x), ("y", y), ("xx", x * x), ("yy", y * y), ("xy", x * y))}
    mx, my = m["x"], m["y"]
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = m["xx"] - mxx, m["yy"] - myy, m["xy"] - mxy
    a1, a2 = 2.0 * mxy + C1, 2.0 * sxy + C2
    b1, b2 = (mxx + myy) + C1, (sxx + syy) + C2
    D = b1 * b2
    with np.errstate(all="ignore"):
        S = (a1 * a2) / D
        P = ((2.0 * my) * (a2 - a1)) / D + (((2.0 * mx) * S) * (b1 - b2)) / D
        Q = -((2.0 * S) / b2)
        R = (2.0 * a1) / D
        if not good:
            S, P, Q, R = (np.full_like(S, np.nan) for _ in range(4))
        grad = (spread(P, win, H, W) + x * spread(Q, win, H, W)) + y * spread(R, win, H, W)
        aw = np.abs(win)
        mass = spread(np.abs(P), aw, H, W) + np.abs(x) * spread(np.abs(Q), aw, H, W) + np.abs(y) * spread(np.abs(R), aw, H, W)
    return {"S": S, "sum": float(S.sum()), "abs_sum": float(np.abs(S).sum()), "count": S.size, "P": P, "Q": Q, "R": R, "grad": grad, "mass": mass, "m": m,
            "b1b2": D, "c1c2": C1 * C2}


def ssim_stack(x, y, ranges, win, k1=K1, k2=K2):
    """ssim_image of every pair of f32 stacks [N,H,W], stacked: the same keys with a leading axis N ("m" dropped)."""
    per = [ssim_image(x[n], y[n], ranges[n], win, k1, k2) for n in range(x.shape[0])]
    return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0] if k != "m"}


@functools.lru_cache(maxsize=None)
def oracle(K, shape, n, window="gauss"):
    x, y, ranges = stack(n, shape)
    return ssim_stack(x, y, ranges, gaussian(K) if window == "gauss" else asymmetric(K))


def torch_ssim_sum(x, y, L, win, k1=K1, k2=K2):
    """(sum of S, S) of one pair of f64 torch tensors [H,W] as a user writes it: one grouped conv2d of the five maps with the outer product
    of the window, then the formula."""
    win = torch.as_tensor(win, dtype=torch.float64)
    kern = torch.outer(win, win)[None, None].repeat(5, 1, 1, 1)
    maps = torch.stack([x, y, x * x, y * y, x * y])[None]
    mx, my, exx, eyy, exy = torch.nn.functional.conv2d(maps, kern, groups=5)[0]
    C1, C2 = (k1 * L) ** 2, (k2 * L) ** 2
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return S.sum(), S
