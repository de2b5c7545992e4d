#!/usr/bin/env python3
"""The centreline tree of a voxel volume, extracted on the device (centreline.extract).

    python3 tools/centreline.py --vol v.npy --threshold 0.3 [--bounds x0,x1,y0,y1,z0,z1] [--root x,y,z] [--vtk] --out dir/

--vol is a .npy volume [n0,n1,n2], read as float32; the vessel is where its value is above --threshold.  --bounds are the coordinates of the
first and the last node on every axis (default: node units; write --bounds=-1,1,... where the first is negative).  --root is a world point
(default: the node deepest inside the vessel).

Writes paths.npy (int32 [n_paths, longest], node indices padded with -1), points.npy (f32 [n_paths, longest, 3], padded with NaN),
radius.npy (f32 [n_paths, longest], padded with NaN), summary.json (centreline.summary), with --vtk the tree as legacy VTK polylines
(tree.vtk by mesh.write_vtk_polylines, the radius as point data), and prints the summary as one JSON record.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.isosurface import parse_bounds  # noqa: E402


def parse_root(text):
    try:
        v = tuple(float(t) for t in text.split(","))
    except ValueError:
        v = ()
    if len(v) != 3 or any(not (abs(x) < float("inf")) for x in v):
        raise argparse.ArgumentTypeError(f"{text!r} is not x,y,z")
    return v


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vol", required=True, help=".npy volume [n0,n1,n2]")
    ap.add_argument("--threshold", type=float, required=True, help="the vessel is where the volume is above it")
    ap.add_argument("--bounds", type=parse_bounds, default=None, help="x0,x1,y0,y1,z0,z1 of the first and last nodes (default: node units)")
    ap.add_argument("--root", type=parse_root, default=None, help="x,y,z of the root (default: the deepest node)")
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--const", type=float, default=None)
    ap.add_argument("--max-paths", type=int, default=256)
    ap.add_argument("--vtk", action="store_true", help="also write the tree as legacy VTK polylines")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch
    vol = np.load(args.vol)
    if vol.ndim != 3 or vol.size == 0 or vol.dtype.kind not in "fiub":
        sys.exit(f"centreline: {args.vol} is {vol.dtype} {vol.shape}: a numeric volume [n0, n1, n2] is needed")
    if not torch.cuda.is_available():
        sys.exit("centreline needs the GPU: there is no CPU path")
    from nerfca_amd import centreline, mesh
    x = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(torch.device(args.device))
    c = centreline.extract(x, args.bounds, threshold=args.threshold, root=args.root, scale=args.scale, const=args.const, max_paths=args.max_paths)
    os.makedirs(args.out, exist_ok=True)
    longest = max([int(p.numel()) for p in c.paths], default=0)
    paths = np.full((len(c.paths), longest), -1, dtype=np.int32)
    points = np.full((len(c.paths), longest, 3), np.nan, dtype=np.float32)
    radius = np.full((len(c.paths), longest), np.nan, dtype=np.float32)
    for k in range(len(c.paths)):
        n = int(c.paths[k].numel())
        paths[k, :n], points[k, :n], radius[k, :n] = c.paths[k].cpu().numpy(), c.points[k].cpu().numpy(), c.radius[k].cpu().numpy()
    np.save(os.path.join(args.out, "paths.npy"), paths)
    np.save(os.path.join(args.out, "points.npy"), points)
    np.save(os.path.join(args.out, "radius.npy"), radius)
    if args.vtk:
        mesh.write_vtk_polylines(os.path.join(args.out, "tree.vtk"), c.points, c.radius)
    record = dict(centreline.summary(c), out=args.out, shape=list(vol.shape), threshold=args.threshold, bounds=args.bounds, root=args.root)
    with open(os.path.join(args.out, "summary.json"), "w") as f:
        json.dump(record, f)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
