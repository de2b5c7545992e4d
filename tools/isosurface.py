#!/usr/bin/env python3
"""The iso-surface of a voxel volume or stack as a triangle mesh, extracted on the device (mesh.isosurface).

    python3 tools/isosurface.py --vol v.npy --level 0.3 [--bounds x0,x1,y0,y1,z0,z1] [--normals] [--format ply|vtk] --out dir/

--vol is a .npy volume [n0,n1,n2] or a stack [..,n0,n1,n2]; it is read as float32.  --bounds are the coordinates of the first and the last
node on every axis (default: node units, 0 .. n - 1; write --bounds=-1,1,... where the first is negative).  A node is inside where its value is above --level.  --normals adds the normalised
negative gradient at every vertex.

Writes one file per volume, surface_0000.ply (binary little-endian PLY) or .vtk (legacy PolyData) and so on in stack order, and prints one
JSON record with, per volume, the vertex and triangle counts, the surface area, the enclosed volume and the Euler characteristic.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_bounds(text):
    """'x0,x1,y0,y1,z0,z1' -> ((x0, x1), (y0, y1), (z0, z1)), each a finite interval lo < hi."""
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        v = []
    if len(v) != 6 or any(not (abs(x) < float("inf")) for x in v) or any(v[2 * a] >= v[2 * a + 1] for a in range(3)):
        raise argparse.ArgumentTypeError(f"{text!r} is not x0,x1,y0,y1,z0,z1 with x0 < x1, y0 < y1, z0 < z1")
    return tuple((v[2 * a], v[2 * a + 1]) for a in range(3))


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vol", required=True, help=".npy volume [n0,n1,n2] or stack [..,n0,n1,n2]")
    ap.add_argument("--level", type=float, required=True, help="the density level of the surface")
    ap.add_argument("--bounds", type=parse_bounds, default=None, help="x0,x1,y0,y1,z0,z1 of the first and last nodes (default: node units)")
    ap.add_argument("--normals", action="store_true", help="also write a normal per vertex")
    ap.add_argument("--format", choices=("ply", "vtk"), default="ply")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch
    vol = np.load(args.vol)
    if vol.ndim < 3 or vol.size == 0 or vol.dtype.kind not in "fiub":
        sys.exit(f"isosurface: {args.vol} is {vol.dtype} {vol.shape}: a numeric volume [n0, n1, n2] or a stack [.., n0, n1, n2] is needed")
    if not torch.cuda.is_available():
        sys.exit("isosurface needs the GPU: there is no CPU path")
    from nerfca_amd import mesh
    dev = torch.device(args.device)
    x = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(dev)
    meshes = mesh.isosurface(x.reshape((-1,) + tuple(x.shape[-3:])), args.level, args.bounds, normals=args.normals)
    os.makedirs(args.out, exist_ok=True)
    write = mesh.write_ply if args.format == "ply" else mesh.write_vtk
    files, rows = [], []
    for i, m in enumerate(meshes):
        files.append(f"surface_{i:04d}.{args.format}")
        write(os.path.join(args.out, files[-1]), m)
        rows.append({"vertices": int(m.verts.shape[0]), "triangles": int(m.faces.shape[0]), "area": float(mesh.surface_area(m)),
                     "enclosed_volume": float(mesh.enclosed_volume(m)), "euler_characteristic": mesh.euler_characteristic(m)})
    print(json.dumps({"out": args.out, "files": files, "shape": list(vol.shape), "level": args.level, "bounds": args.bounds, "normals": args.normals, "surfaces": rows}))


if __name__ == "__main__":
    main()
