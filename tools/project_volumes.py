#!/usr/bin/env python3
"""Project voxel volumes through C-arm views (drr.project_sequence) and write the images as .npy stacks.

    python3 tools/project_volumes.py --static vs.npy --dynamic vd.npy --bounds -1,1,-1,1,-1,1 --geometry xcat --n-det 128 \\
        --views "-5,40;60,-30" --phases 0,3,7 --samples 192 --normalize --out projections/

--static is a .npy volume [n0,n1,n2], --dynamic a .npy stack [P,n0,n1,n2] on the same grid (what export.density_volumes returns, or a CT /
phantom volume in the loader's units); without --dynamic the static volume is projected alone.  --bounds x0,x1,y0,y1,z0,z1 places node 0
and node n-1 of each axis (the grid is linspace(lo, hi, n), export.density_volume's).  --phases selects rows of the dynamic stack (all of
them when left out).  --geometry, --n-det and --views are those of tools/render_views.py.

Writes the files of tools/render_views.py: pred.npy and pred_dynamic.npy [V,P,W,H], pred_static.npy [V,W,H] (f32, un-normalised
I0 - sum sigma dists), with --normalize the three *_norm.npy stacks, and manifest.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_views import join_views, load_geometry, parse_phases, parse_views  # noqa: E402,F401


def parse_bounds(text):
    """ "x0,x1,y0,y1,z0,z1" -> ((x0, x1), (y0, y1), (z0, z1)) with lo < hi on each axis."""
    v = [float(x) for x in text.split(",") if x.strip()]
    if len(v) != 6:
        raise ValueError(f"bounds are six numbers x0,x1,y0,y1,z0,z1, got {text!r}")
    bounds = tuple((v[2 * a], v[2 * a + 1]) for a in range(3))
    if any(not lo < hi for lo, hi in bounds):
        raise ValueError(f"bounds need lo < hi on each axis, got {text!r}")
    return bounds


def join_args(argv):
    """render_views.join_views for --views, and the same for --bounds: both lists usually start with a minus sign."""
    argv, out = join_views(argv), []
    while argv:
        a = argv.pop(0)
        out.append(a + "=" + argv.pop(0) if a == "--bounds" and argv else a)
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--static", required=True, help=".npy volume [n0,n1,n2] of the static field")
    ap.add_argument("--dynamic", default=None, help=".npy stack [P,n0,n1,n2] of the dynamic field; left out: static volume only")
    ap.add_argument("--bounds", default=((-1.0, 1.0),) * 3, type=parse_bounds, help="x0,x1,y0,y1,z0,z1: positions of the first and last node per axis")
    ap.add_argument("--geometry", default="xcat", help="xcat | magix | path of a JSON geometry")
    ap.add_argument("--n-det", type=int, default=128, help="detector pixels per side of the xcat / magix geometry")
    ap.add_argument("--views", required=True, type=parse_views, help='"theta,phi;theta,phi[,larm];..." in degrees')
    ap.add_argument("--phases", default=None, type=parse_phases, help="rows of the dynamic stack, comma separated (default: all)")
    ap.add_argument("--samples", type=int, default=192, help="depth samples per ray")
    ap.add_argument("--normalize", action="store_true", help="also write the per-frame (x - min) / (max - min) images")
    ap.add_argument("--chunk-rays", type=int, default=65536)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(join_args(sys.argv[1:] if argv is None else argv))
    import numpy as np
    import torch
    from nerfca_amd import drr
    if not torch.cuda.is_available():
        sys.exit("project_volumes needs the GPU: there is no CPU path")
    dev = torch.device(args.device)
    geo = load_geometry(args.geometry, args.n_det)
    static = torch.from_numpy(np.ascontiguousarray(np.load(args.static), dtype=np.float32)).to(dev)
    dynamic, phases = None, None
    if args.dynamic:
        stack = np.load(args.dynamic)
        phases = list(range(stack.shape[0])) if args.phases is None else args.phases
        if any(not 0 <= p < stack.shape[0] for p in phases):
            sys.exit(f"--phases {phases}: the dynamic stack has {stack.shape[0]} volumes")
        dynamic = torch.from_numpy(np.ascontiguousarray(stack[phases], dtype=np.float32)).to(dev)
    out = drr.project_sequence(static, dynamic, geo, args.views, args.samples, bounds=args.bounds, chunk_rays=args.chunk_rays, normalize=args.normalize)
    os.makedirs(args.out, exist_ok=True)
    files = {}
    for k, t in out.items():
        if k != "minmax":
            np.save(os.path.join(args.out, k + ".npy"), t.cpu().numpy())
            files[k] = {"file": k + ".npy", "shape": list(t.shape)}
    manifest = {"views": [list(v) for v in args.views], "phases": phases, "samples": args.samples, "bounds": [list(b) for b in args.bounds],
                "volume_shape": list(static.shape), "geometry": geo, "files": files}
    if args.normalize:
        manifest["minmax"] = {k: t.cpu().tolist() for k, t in out["minmax"].items()}
    with open(os.path.join(args.out, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(json.dumps({"out": args.out, "files": sorted(files)}))


if __name__ == "__main__":
    main()
