#!/usr/bin/env python3
"""Cross-sections and lumen profiles along the centreline tree of a voxel volume, on the device (centreline.extract, reformat.along).

    python3 tools/reformat.py --vol v.npy --threshold T --level L [--bounds x0,x1,y0,y1,z0,z1] [--root x,y,z]
                              [--size 33 --spacing s --order 3] [--vtk] --out dir/

--vol is a .npy volume [n0,n1,n2], read as float32.  The tree is extracted from the mask above --threshold; the lumen is where the
(trilinear) volume is above --level.  --bounds are the coordinates of the first and the last node on every axis (default: node units; write
--bounds=-1,1,... where the first is negative).  --root is a world point (default: the node deepest inside the vessel).  Every path is
smoothed (--smooth passes of 1-2-1), resampled every --step (default: its mean node distance) and cut by planes of --size x --size pixels
of --spacing (default: half the smallest node spacing) at --order 0, 1 or 3; rays go out to --r-max (default: half the plane's width).

Writes sections_<path>.npy (f32 [K, size, size], the straightened reformation of path <path>; its centre column [:, :, size // 2] is the
curved-planar image), profile.json (per path the arclength, d_eq, d_min, d_max, status and the stenosis record), with --vtk the resampled
tree as legacy VTK polylines (tree.vtk by mesh.write_vtk_polylines, d_eq / 2 as the point radius), and prints the stenosis records as one
JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.centreline import parse_root  # noqa: E402
from tools.isosurface import parse_bounds  # noqa: E402


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vol", required=True, help=".npy volume [n0,n1,n2]")
    ap.add_argument("--threshold", type=float, required=True, help="the tree is extracted where the volume is above it")
    ap.add_argument("--level", type=float, required=True, help="the lumen is where the volume is above it")
    ap.add_argument("--bounds", type=parse_bounds, default=None, help="x0,x1,y0,y1,z0,z1 of the first and last nodes (default: node units)")
    ap.add_argument("--root", type=parse_root, default=None, help="x,y,z of the root (default: the deepest node)")
    ap.add_argument("--size", type=int, default=33, help="pixels per side of a cross-section")
    ap.add_argument("--spacing", type=float, default=None, help="pixel size (default: half the smallest node spacing)")
    ap.add_argument("--order", type=int, default=3, choices=(0, 1, 3))
    ap.add_argument("--step", type=float, default=None, help="distance between planes (default: the path's mean node distance)")
    ap.add_argument("--smooth", type=int, default=2)
    ap.add_argument("--r-max", type=float, default=None, help="length of the rays (default: half the plane's width)")
    ap.add_argument("--angles", type=int, default=64)
    ap.add_argument("--max-paths", type=int, default=256)
    ap.add_argument("--vtk", action="store_true", help="also write the resampled tree as legacy VTK polylines")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch
    vol = np.load(args.vol)
    if vol.ndim != 3 or vol.size == 0 or vol.dtype.kind not in "fiub":
        sys.exit(f"reformat: {args.vol} is {vol.dtype} {vol.shape}: a numeric volume [n0, n1, n2] is needed")
    if not torch.cuda.is_available():
        sys.exit("reformat needs the GPU: there is no CPU path")
    from nerfca_amd import centreline, mesh, reformat
    x = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(torch.device(args.device))
    bounds = args.bounds if args.bounds is not None else tuple((0.0, float(n - 1)) for n in vol.shape)
    h = min((b[1] - b[0]) / (n - 1) for b, n in zip(bounds, vol.shape))
    spacing = args.spacing if args.spacing is not None else 0.5 * h
    r_max = args.r_max if args.r_max is not None else 0.5 * (args.size - 1) * spacing
    tree = centreline.extract(x, bounds, threshold=args.threshold, root=args.root, max_paths=args.max_paths)
    per = reformat.along(x, bounds, tree, level=args.level, r_max=r_max, size=args.size, spacing=spacing, order=args.order, n_angles=args.angles, step=args.step,
                         smooth=args.smooth)
    os.makedirs(args.out, exist_ok=True)
    record = {"out": args.out, "shape": list(vol.shape), "threshold": args.threshold, "level": args.level, "bounds": bounds, "size": args.size, "spacing": spacing,
              "order": args.order, "r_max": r_max, "paths": []}
    points, radius = [], []
    for k, one in enumerate(per):
        if one is None:
            record["paths"].append(None)
            continue
        np.save(os.path.join(args.out, f"sections_{k}.npy"), one["sections"].cpu().numpy())
        prof = one["profile"]
        record["paths"].append({"parent": [int(v) for v in tree.parent[k]], "s": prof.s.cpu().tolist(), "d_eq": prof.d_eq.cpu().tolist(), "d_min": prof.d_min.cpu().tolist(),
                                "d_max": prof.d_max.cpu().tolist(), "status": prof.status.cpu().tolist(), "stenosis": one["stenosis"][0]})
        points.append(one["frames"].origin.astype(np.float32))
        radius.append((0.5 * prof.d_eq).to(torch.float32).cpu().numpy())
    if args.vtk:
        mesh.write_vtk_polylines(os.path.join(args.out, "tree.vtk"), points, radius)
    with open(os.path.join(args.out, "profile.json"), "w") as f:
        json.dump(record, f)
    print(json.dumps({"out": args.out, "paths": len(per), "stenosis": [p and p["stenosis"] for p in record["paths"]]}))


if __name__ == "__main__":
    main()
