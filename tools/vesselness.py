#!/usr/bin/env python3
"""Multi-scale Hessian vesselness (Frangi) of a voxel volume or stack on the device (ccta.vesselness).

    python3 tools/vesselness.py --vol v.npy --sigmas 1,2,3 [--dark] [--c X] [--alpha 0.5 --beta 0.5] --out dir/

--vol is a .npy volume [n0,n1,n2] or a stack [..,n0,n1,n2]; it is read as float32.  --sigmas are the scales in nodes (the grid is taken as
isotropic: resample first if it is not).  --dark looks for tubes darker than their surroundings.  --c is the norm constant of the third
factor; without it Frangi's rule is used, half the largest Hessian norm of each volume at each scale; --c 0 drops the factor.

Writes vesselness.npy (float32, the shape of --vol, values in [0, 1]) and scale.npy (int32, the index into --sigmas of the scale that gave
the value) and prints one JSON record.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_sigmas(text):
    """'S0,S1,..': at least one positive scale."""
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        v = []
    if not v or any(not 0.0 < s < float("inf") for s in v):
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of positive scales")
    return v


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vol", required=True, help=".npy volume [n0,n1,n2] or stack [..,n0,n1,n2]")
    ap.add_argument("--sigmas", type=parse_sigmas, default=[1.0, 2.0, 3.0], help="scales in nodes, comma separated")
    ap.add_argument("--dark", action="store_true", help="dark tubes on a bright background")
    ap.add_argument("--c", type=float, default=None, help="norm constant (default: half the largest Hessian norm per volume and scale; 0: no norm factor)")
    ap.add_argument("--alpha", type=float, default=0.5, help="sensitivity to plate-like shapes")
    ap.add_argument("--beta", type=float, default=0.5, help="sensitivity to blob-like shapes")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    import numpy as np
    import torch
    vol = np.load(args.vol)
    if vol.ndim < 3 or vol.size == 0 or vol.dtype.kind not in "fiub":
        sys.exit(f"vesselness: {args.vol} is {vol.dtype} {vol.shape}: a numeric volume [n0, n1, n2] or a stack [.., n0, n1, n2] is needed")
    if not torch.cuda.is_available():
        sys.exit("vesselness needs the GPU: there is no CPU path")
    from nerfca_amd import ccta
    dev = torch.device(args.device)
    x = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(dev)
    V, index = ccta.vesselness(x, args.sigmas, alpha=args.alpha, beta=args.beta, c=args.c, bright=not args.dark, return_scale=True)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "vesselness.npy"), V.cpu().numpy())
    np.save(os.path.join(args.out, "scale.npy"), index.cpu().numpy())
    print(json.dumps({"out": args.out, "files": ["scale.npy", "vesselness.npy"], "shape": list(vol.shape), "sigmas": args.sigmas, "bright": not args.dark,
                      "c": "frangi" if args.c is None else args.c, "max": float(V.max()), "nodes_above_half_max": int((V > 0.5 * V.max()).sum())}))


if __name__ == "__main__":
    main()
