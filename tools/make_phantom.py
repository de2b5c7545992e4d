#!/usr/bin/env python3
"""Write a procedural 4-D phantom (nerfca_amd.phantom.make_phantom): a static thorax and a coronary tree that beats with the heart phase,
rasterised on the device for a C-arm geometry.

    python3 tools/make_phantom.py --shape 128,128,128 --phases 10 --out phantom/

writes static.npy [n0,n1,n2] and dynamic.npy [P,n0,n1,n2] (f32; what tools/project_volumes.py and tools/fit_volumes.py read),
segments.npy [P,N,8] and ellipsoids.npy [E,14] (f64: the truth at any resolution) and phantom.json (shape, bounds, seed, densities).  The
bounds are the cube of the geometry's field of view: hand them to the other tools with --bounds.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from fit_volumes import parse_shape  # noqa: E402


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", required=True, type=parse_shape, help="n0,n1,n2: nodes per axis")
    ap.add_argument("--phases", type=int, default=10, help="heart phases of one cycle")
    ap.add_argument("--geometry", default="xcat", help="xcat | magix: the field of view sizes the phantom")
    ap.add_argument("--n-det", type=int, default=128, help="detector pixels per side (the field of view does not depend on it)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the coronary tree")
    ap.add_argument("--rho-vessel", type=float, default=None, help="density of the vessels (default: phantom.RHO_VESSEL)")
    ap.add_argument("--edge", type=float, default=None, help="width of a vessel wall (default: the coarsest node spacing)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    from nerfca_amd import phantom, synthetic
    geo = synthetic.GEOMETRIES[args.geometry](args.n_det)
    rho = phantom.RHO_VESSEL if args.rho_vessel is None else args.rho_vessel
    ph = phantom.make_phantom(args.shape, args.phases, geo, seed=args.seed, device=args.device, rho_vessel=rho, edge=args.edge)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "static.npy"), ph["static"].cpu().numpy())
    np.save(os.path.join(args.out, "dynamic.npy"), ph["dynamic"].cpu().numpy())
    np.save(os.path.join(args.out, "segments.npy"), ph["segments"])
    np.save(os.path.join(args.out, "ellipsoids.npy"), ph["ellipsoids"])
    meta = {"shape": list(args.shape), "phases": args.phases, "geometry": args.geometry, "seed": args.seed, "rho_vessel": rho,
            "bounds": [list(b) for b in ph["bounds"]], "segments_per_phase": int(ph["segments"].shape[1])}
    with open(os.path.join(args.out, "phantom.json"), "w") as f:
        json.dump(meta, f, indent=1)
    flat = ",".join(f"{v:g}" for b in ph["bounds"] for v in b)
    print(f"wrote {args.out}: static {tuple(ph['static'].shape)}, dynamic {tuple(ph['dynamic'].shape)}, {meta['segments_per_phase']} segments per phase; --bounds {flat}")


if __name__ == "__main__":
    main()
