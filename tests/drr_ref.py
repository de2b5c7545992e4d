"""The f64 numpy projector the drr tests hold the kernel to: a direct transcription of the definition of one sample in
include/nerfca_hip.h ("drr"), summed s = 0 ... S-1 in order.  Plus the shapes, bounds and rays the tests share, and the same
projection through torch's grid_sample (an independent implementation the oracle itself is pinned to on the CPU)."""
import numpy as np
import torch

GRIDS = [(2, 2, 2), (5, 3, 4), (17, 9, 33)]          # minimum size; all-different odd / even extents; an odd last axis, rows beyond one cache line
BOUNDS = ((-0.9, 0.8), (-0.7, 0.9), (-0.8, 0.6))
SMALL_BOX = ((-0.3, 0.2),) * 3
WIDE = ((-1.2, 1.2),) * 3
VIEWS = [(-5.0, 40.0), (137.5, -63.0)]


def geometries():
    """(name, geo, S): the xcat detector of 8 x 8 at 16 samples and a 12 x 20 detector with offsets at 37."""
    from nerfca_amd import synthetic
    return [("xcat8", synthetic.xcat_geometry(8), 16),
            ("det12x20", dict(synthetic.xcat_geometry(16), nDetector=[12, 20], dDetector=[2.0 / 12, 0.1], offDetector=[0.013, -0.02]), 37)]


def host_rays(geo, theta, phi):
    """f64 [W*H,3] origins and directions of one projection from the host geometry (the f32 values of get_ray_values_tigre, widened)."""
    from nerfca_amd.train.proj_helpers import get_ray_values_tigre
    o, d = get_ray_values_tigre(theta, phi, 0, geo, "cpu")
    return np.asarray(o, dtype=np.float32).reshape(-1, 3).astype(np.float64), np.asarray(d, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def depths(geo, S):
    """(z f32 [S], dists f64 [S]) as render_sequence / project_sequence form them."""
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], S, "cpu").to(torch.float32)
    dists = _interval_lengths(z, torch.empty(0, dtype=torch.float64)).to(torch.float64)
    return z.numpy(), dists.numpy()


def random_volume(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def grid_coords(shape, bounds, origins, dirs, z):
    """g f64 [R,S,3]: p = o + d (double)z, g = (p - lo) inv with inv = (n - 1) / (hi - lo), every operation a rounded f64 one."""
    lo = np.array([float(b[0]) for b in bounds], dtype=np.float64)
    inv = np.array([(int(n) - 1) / (float(b[1]) - float(b[0])) for n, b in zip(shape, bounds)], dtype=np.float64)
    p = origins[:, None, :] + dirs[:, None, :] * z.astype(np.float64)[None, :, None]
    return (p - lo) * inv


def project(vol, origins, dirs, z, dists, i0, bounds):
    """(pix f64 [n_vol,R] or [R], scale f64 [...same] = |i0| + sum_s |term|, g f64 [R,S,3]) of f32 volumes [n0,n1,n2] or
    [n_vol,n0,n1,n2]."""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32
    single = vol.ndim == 3
    vols = (vol[None] if single else vol).astype(np.float64)
    n = vols.shape[1:]
    g = grid_coords(n, bounds, origins, dirs, z)
    fl = np.floor(g)
    f = g - fl
    i = fl.astype(np.int64)

    def node(k0, k1, k2):          # [n_vol,R,S]: the volumes at integer nodes, 0 outside
        ok = (k0 >= 0) & (k0 < n[0]) & (k1 >= 0) & (k1 < n[1]) & (k2 >= 0) & (k2 < n[2])
        v = vols[:, np.clip(k0, 0, n[0] - 1), np.clip(k1, 0, n[1] - 1), np.clip(k2, 0, n[2] - 1)]
        return np.where(ok[None], v, 0.0)

    def lerp(fa, v0, v1):
        return (1.0 - fa) * v0 + fa * v1

    i0a, i1a, i2a = i[..., 0], i[..., 1], i[..., 2]
    f0, f1, f2 = f[..., 0][None], f[..., 1][None], f[..., 2][None]
    c = {(a, b): lerp(f2, node(i0a + a, i1a + b, i2a), node(i0a + a, i1a + b, i2a + 1)) for a in (0, 1) for b in (0, 1)}      # the last axis first
    value = lerp(f0, lerp(f1, c[0, 0], c[0, 1]), lerp(f1, c[1, 0], c[1, 1]))                                                # then the middle, then the first
    term = value * dists[None, None, :]
    total = np.zeros(term.shape[:2], dtype=np.float64)
    for s in range(term.shape[2]):          # s = 0 ... S-1 in order
        total = total + term[:, :, s]
    pix = i0 - total
    scale = abs(i0) + np.abs(term).sum(-1)
    return (pix[0], scale[0], g) if single else (pix, scale, g)


def project_grid_sample(vol, origins, dirs, z, dists, i0, bounds, dtype=torch.float64):
    """The same projection through torch.nn.functional.grid_sample(bilinear, zeros, align_corners=True) on the CPU: x addresses the LAST
    volume axis.  Returns pix [n_vol,R] or [R] as a numpy array of `dtype`."""
    vol = torch.as_tensor(np.asarray(vol))
    single = vol.dim() == 3
    vols = (vol[None] if single else vol).to(dtype)
    lo = torch.tensor([float(b[0]) for b in bounds], dtype=dtype)
    hi = torch.tensor([float(b[1]) for b in bounds], dtype=dtype)
    o, d = torch.as_tensor(origins).to(dtype), torch.as_tensor(dirs).to(dtype)
    p = o[:, None, :] + d[:, None, :] * torch.as_tensor(z).to(dtype)[None, :, None]
    u = (p - lo) / (hi - lo) * 2 - 1
    grid = u.flip(-1)[None, None]                                              # [1,1,R,S,(x,y,z)] with x = the last axis
    sig = torch.nn.functional.grid_sample(vols[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]      # [n_vol,R,S]
    pix = i0 - (sig * torch.as_tensor(dists).to(dtype)).sum(-1)
    return (pix[0] if single else pix).numpy()
