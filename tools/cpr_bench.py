#!/usr/bin/env python3
"""Times reformat.cross_sections and reformat.lumen_profile on the phantom against what a user writes without them.

Per grid size (128 and 256 nodes per axis) and stack (1 and 10 heart phases): --planes planes of --size x --size pixels, equally spaced
along the longest chain of segments of the phantom's tree at phase 0 (reformat.frames of the chain's joints), pixel size and ray step half
a node spacing.

  * cross_sections order 1 against the torch loop: per volume, build the pixel coordinates from the frames, normalise them and call
    F.grid_sample (trilinear, f32, align_corners=True);
  * cross_sections order 3 (ccta.spline_filter included) against scipy.ndimage.map_coordinates(order=3, mode="mirror") on the host, the
    copies down and up included (torch has no cubic volume sampler); one pass, the host's noise is small beside its seconds;
  * lumen_profile (64 rays, r_max = eight node spacings) against the same grid_sample expression over the ray samples followed by a
    first-crossing search in torch (argmax of the first sample at or below the level, linear interpolation between it and the one before).

Reported: ms per call (the best of --passes windows of back-to-back calls, about 0.2 s each, between two synchronisations; the library's
call makes no host read, and its Python wrapper is part of the figure), the ratio baseline / library, GB/s of the library's output bytes, the largest difference between the two results, and whether any row is slower.  No figure is a pass criterion.

    python3 tools/cpr_bench.py [--out profiles/cpr_bench.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sides", default="128,256")
    ap.add_argument("--volumes", default="1,10")
    ap.add_argument("--planes", type=int, default=512)
    ap.add_argument("--size", type=int, default=65)
    ap.add_argument("--passes", type=int, default=3)
    return ap


def segment_chains(table):
    """The chains of ONE phase of a segment table [N, 8]: maximal runs of consecutive rows in which every row starts where the one before it
    ends.  A list of (points f64 [m + 1, 3], radius f64 [m + 1]): the joints of a chain in order and the table's radius at them."""
    import numpy as np
    table = np.asarray(table, dtype=np.float64)
    out, first = [], 0
    for i in range(1, table.shape[0] + 1):
        if i == table.shape[0] or not np.array_equal(table[i, 0:3], table[i - 1, 3:6]):
            rows = table[first:i]
            out.append((np.concatenate([rows[:1, 0:3], rows[:, 3:6]]), np.concatenate([rows[:1, 6], rows[:, 7]])))
            first = i
    return out


def longest_chain(table):
    import numpy as np
    return max(segment_chains(table), key=lambda c: float(np.sqrt(((c[0][1:] - c[0][:-1]) ** 2).sum(1)).sum()))


def best_ms(fn, passes, window=0.2):
    """ms per call: the best of `passes` windows, each as many back-to-back calls as fill `window` seconds (sized from one timed call after a
    warm-up), between two synchronisations"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, min(2000, int(window / max(time.perf_counter() - t0, 1e-6))))
    out = math.inf
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out = min(out, (time.perf_counter() - t0) * 1e3 / reps)
    return out


def _normalised(points, bounds):
    """world points [..., 3] -> grid_sample's coordinates (x is the last axis of the volume) for align_corners=True"""
    import torch
    lo = torch.tensor([b[0] for b in bounds], dtype=points.dtype, device=points.device)
    hi = torch.tensor([b[1] for b in bounds], dtype=points.dtype, device=points.device)
    return ((points - lo) / (hi - lo) * 2.0 - 1.0).flip(-1)


def torch_sections(vol, bounds, fr, size, spacing):
    """the loop a user writes today: f32 [n_vol, K, size, size]"""
    import torch
    import torch.nn.functional as F
    out = []
    for v in vol:
        u = (torch.arange(size, device=vol.device, dtype=torch.float32) - 0.5 * (size - 1)) * spacing
        p = fr.origin.float()[:, None, None, :] + u[None, :, None, None] * fr.e1.float()[:, None, None, :] + u[None, None, :, None] * fr.e2.float()[:, None, None, :]
        out.append(F.grid_sample(v[None, None], _normalised(p, bounds)[None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0])
    return torch.stack(out)


def torch_lumen(vol, bounds, fr, dirs, level, dr, n_steps):
    """radius f32 [n_vol, K, n_ang] by grid_sample over all ray samples and a first-crossing search; a ray without a crossing gets n_steps dr"""
    import torch
    import torch.nn.functional as F
    out = []
    for v in vol:
        r = torch.arange(n_steps + 1, device=vol.device, dtype=torch.float32) * dr
        d = dirs.float()[None, :, None, :1] * fr.e1.float()[:, None, None, :] + dirs.float()[None, :, None, 1:] * fr.e2.float()[:, None, None, :]
        p = fr.origin.float()[:, None, None, :] + r[None, None, :, None] * d
        g = F.grid_sample(v[None, None], _normalised(p, bounds)[None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
        below = ~(g > level)
        first = torch.where(below.any(-1), below.float().argmax(-1), torch.full(below.shape[:-1], n_steps + 1, dtype=torch.int64, device=vol.device))
        j = first.clamp(1, n_steps)
        g0, g1 = g.gather(-1, (j - 1)[..., None])[..., 0], g.gather(-1, j[..., None])[..., 0]
        t = (g0 - level) / (g0 - g1)
        out.append(torch.where(first == 0, torch.zeros_like(t), torch.where(first > n_steps, torch.full_like(t, n_steps * dr), ((j - 1).float() + t) * dr)))
    return torch.stack(out)


def scipy_sections(vol, bounds, fr_host, size, spacing):
    """order 3 on the host, the copies included: f32 [n_vol, K, size, size] on the device"""
    import numpy as np
    import scipy.ndimage
    import torch
    host = vol.cpu().numpy()
    u = (np.arange(size) - 0.5 * (size - 1)) * spacing
    p = fr_host.origin[:, None, None, :] + u[None, :, None, None] * fr_host.e1[:, None, None, :] + u[None, None, :, None] * fr_host.e2[:, None, None, :]
    n = host.shape[1:]
    x = np.stack([(p[..., a] - bounds[a][0]) * ((n[a] - 1) / (bounds[a][1] - bounds[a][0])) for a in range(3)])
    out = np.stack([scipy.ndimage.map_coordinates(v.astype(np.float64), x.reshape(3, -1), order=3, mode="mirror", cval=0.0).reshape(p.shape[:-1]) for v in host])
    return torch.from_numpy(out.astype(np.float32)).to(vol.device)


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("cpr_bench needs the GPU")
    from nerfca_amd import phantom, reformat, synthetic
    dev = torch.device("cuda:0")
    lines = [f"{args.planes} planes of {args.size} x {args.size} pixels (cross_sections) or 64 rays (lumen_profile) along the phantom's longest chain of segments at phase 0; "
             f"pixel size and ray step half a node spacing; ms per call are the best of {args.passes} windows of back-to-back calls, about 0.2 s each (scipy: one call); ratio = baseline / library; GB/s of the library's output bytes",
             "side  volumes  what                          library ms   baseline                          baseline ms    ratio   GB/s out   max |difference| (inside the grid)"]
    geo = synthetic.xcat_geometry(128)
    slower = []
    for side in (int(s) for s in args.sides.split(",")):
        ph = phantom.make_phantom((side,) * 3, 10, geo, device=dev)
        bounds = ph["bounds"]
        h = min((b[1] - b[0]) / (side - 1) for b in bounds)
        chain, _ = longest_chain(ph["segments"][0])
        length = float(np.sqrt(((chain[1:] - chain[:-1]) ** 2).sum(1)).sum())
        host = reformat.frames(chain, step=length / (args.planes - 1) * (1.0 - 1e-12))
        host = reformat.Frames(*(f[:args.planes] for f in host))
        fr = reformat.to_device(host, dev)
        spacing, dr, n_steps, level = 0.5 * h, 0.5 * h, 16, 0.25 * phantom.RHO_VESSEL
        dirs = torch.from_numpy(reformat.directions(64)).to(dev)
        for n_vol in (int(v) for v in args.volumes.split(",")):
            vol = ph["dynamic"][:n_vol].contiguous()
            rows = []
            got = reformat.cross_sections(vol, bounds, fr, size=args.size, spacing=spacing, order=1)          # warm-up and the result
            want = torch_sections(vol, bounds, fr, args.size, spacing)
            rows.append(("cross_sections order 1", best_ms(lambda: reformat.cross_sections(vol, bounds, fr, size=args.size, spacing=spacing, order=1), args.passes),
                         "torch loop, grid_sample f32", best_ms(lambda: torch_sections(vol, bounds, fr, args.size, spacing), args.passes), got.numel() * 4,
                         float((got - want).abs().max())))
            got = reformat.cross_sections(vol, bounds, fr, size=args.size, spacing=spacing, order=3)
            t0 = time.perf_counter()
            want = scipy_sections(vol, bounds, host, args.size, spacing)
            host_ms = (time.perf_counter() - t0) * 1e3
            inside = reformat.cross_sections(torch.ones_like(vol), bounds, fr, size=args.size, spacing=spacing, order=0) > 0
            rows.append(("cross_sections order 3", best_ms(lambda: reformat.cross_sections(vol, bounds, fr, size=args.size, spacing=spacing, order=3), args.passes),
                         "scipy map_coordinates, host", host_ms, got.numel() * 4, float(((got - want).abs() * inside).max())))
            prof = reformat.lumen_profile(vol, bounds, fr, level=level, r_max=n_steps * dr, n_angles=64, dr=dr)
            want = torch_lumen(vol, bounds, fr, dirs, level, dr, n_steps)
            clean = (prof.status == 0)[..., None].expand_as(want)
            rows.append(("lumen_profile 64 rays", best_ms(lambda: reformat.lumen_profile(vol, bounds, fr, level=level, r_max=n_steps * dr, n_angles=64, dr=dr), args.passes),
                         "grid_sample + first crossing", best_ms(lambda: torch_lumen(vol, bounds, fr, dirs, level, dr, n_steps), args.passes),
                         prof.radius.numel() * 4 + prof.area.numel() * 32 + prof.status.numel() * 4,
                         float(((prof.radius - want).abs() * clean).max())))
            for what, ms, base, base_ms, nbytes, diff in rows:
                lines.append(f"{side:>4}  {n_vol:>7}  {what:<28}  {ms:>10.3f}   {base:<32}  {base_ms:>11.3f}  {base_ms / ms:>7.2f}   {nbytes / (ms * 1e-3) / 1e9:>8.2f}   {diff:.3e}")
                print(lines[-1], flush=True)
                if base_ms < ms:
                    slower.append(f"{what} at {side}^3 x {n_vol}")
            del vol, got, want, prof
        del ph
        torch.cuda.empty_cache()
    lines.append("rows in which the library is slower than its baseline: " + (", ".join(slower) if slower else "none"))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
