#!/usr/bin/env python3
"""Turn a CT in Hounsfield units and a vessel segmentation into the static and dynamic volumes that get projected (ccta.prepare_ccta).

    python3 tools/prepare_ccta.py --raw raw.npy --mask mask.npy [--labels total.npy --aorta 52 --heart 51] \\
        --bounds -0.18,0.18,-0.18,0.18,-0.18,0.18 [--resample 1 [--label-order 0]] --out prepared/

--raw is a .npy volume [n0,n1,n2] or a stack [P,n0,n1,n2] in Hounsfield units, --mask the vessel segmentation of the same shape (a node
belongs to it when > 0), --labels a whole-body segmentation of the same shape: the nodes labelled --aorta get the mean attenuation of the
nodes labelled --heart, per volume.  --bounds x0,x1,y0,y1,z0,z1 places node 0 and node n-1 of each axis; distances inside the vessel are in
its units.  --resample S (or S0,S1,S2) first brings all three volumes to that node spacing, in the units of --bounds, with the cubic-spline
zoom of ccta.zoom: the reference resamples to a spacing of 1 (give --bounds in millimetres and --resample 1 for its numbers; the dilation,
erosion, smoothing and transfer function all count in nodes of the resampled grid).  --label-order 3 (the reference's) resamples --mask and
--labels with the cubic spline and rounds, --label-order 0 takes the nearest node and invents no label.  --grow, --shrink, --sigma,
--radius and --contrast are the arguments of ccta.vessel_contrast.

Writes what tools/project_volumes.py reads: static.npy [n0,n1,n2] (the attenuation outside the closed vessel mask, of volume
--static-volume of a stack) and dynamic.npy [P,n0,n1,n2] (the vessel contrast of every volume), and prints one JSON record with the
--bounds to hand on.  With --resample the files are on the resampled grid and the bounds stay: end nodes map to end nodes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from project_volumes import join_args, parse_bounds  # noqa: E402,F401


def parse_spacing(text):
    """'S' or 'S0,S1,S2': a positive spacing for all axes or one per axis."""
    try:
        v = tuple(float(t) for t in text.split(","))
    except ValueError:
        v = ()
    if len(v) not in (1, 3) or any(not 0.0 < s < float("inf") for s in v):
        raise argparse.ArgumentTypeError(f"{text!r} is not S or S0,S1,S2 with positive spacings")
    return v[0] if len(v) == 1 else v


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--raw", required=True, help=".npy CT volume [n0,n1,n2] or stack [P,n0,n1,n2] in Hounsfield units")
    ap.add_argument("--mask", required=True, help=".npy vessel segmentation of the same shape (> 0 inside)")
    ap.add_argument("--labels", default=None, help=".npy whole-body segmentation of the same shape")
    ap.add_argument("--aorta", type=int, default=None, help="label of the aorta in --labels")
    ap.add_argument("--heart", type=int, default=None, help="label of the heart in --labels")
    ap.add_argument("--bounds", required=True, type=parse_bounds, help="x0,x1,y0,y1,z0,z1: positions of the first and last node per axis")
    ap.add_argument("--resample", type=parse_spacing, default=None, help="S or S0,S1,S2: bring the volumes to this node spacing first (units of --bounds)")
    ap.add_argument("--label-order", type=int, choices=(0, 3), default=3, help="spline order for --mask and --labels under --resample")
    ap.add_argument("--grow", type=int, default=3, help="dilations of the segmentation")
    ap.add_argument("--shrink", type=int, default=1, help="erosions after them")
    ap.add_argument("--sigma", type=float, default=1.0, help="Gaussian smoothing of the depth map, in nodes")
    ap.add_argument("--radius", type=int, default=2, help="its radius, in nodes")
    ap.add_argument("--contrast", type=float, default=0.05, help="attenuation at the vessel's core")
    ap.add_argument("--static-volume", type=int, default=0, help="which volume of a stack gives static.npy")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def main(argv=None):
    args = parser().parse_args(join_args(sys.argv[1:] if argv is None else argv))
    if (args.labels is None) != (args.aorta is None) or (args.labels is None) != (args.heart is None):
        sys.exit("prepare_ccta: --labels, --aorta and --heart go together")
    import numpy as np
    import torch
    from nerfca_amd import ccta
    if not torch.cuda.is_available():
        sys.exit("prepare_ccta needs the GPU: there is no CPU path")
    dev = torch.device(args.device)
    raw, mask = np.load(args.raw), np.load(args.mask)
    if raw.ndim not in (3, 4) or mask.shape != raw.shape:
        sys.exit(f"prepare_ccta: {args.raw} is {raw.shape}, {args.mask} is {mask.shape}: one shape [n0,n1,n2] or [P,n0,n1,n2]")
    labels = None
    if args.labels:
        labels = np.load(args.labels)
        if labels.shape != raw.shape:
            sys.exit(f"prepare_ccta: {args.labels} is {labels.shape}, {args.raw} is {raw.shape}")
        labels = torch.from_numpy(np.ascontiguousarray(labels.astype(np.int64))).to(dev)
    if raw.ndim == 3:
        raw, mask = raw[None], mask[None]
        labels = None if labels is None else labels[None]
    if not 0 <= args.static_volume < raw.shape[0]:
        sys.exit(f"prepare_ccta: --static-volume {args.static_volume}: the stack has {raw.shape[0]} volumes")
    out = ccta.prepare_ccta(torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(mask > 0)).to(dev),
                            args.bounds, labels=labels, aorta_label=args.aorta, heart_label=args.heart, grow=args.grow, shrink=args.shrink, sigma=args.sigma,
                            radius=args.radius, contrast=args.contrast, resample=args.resample, label_order=args.label_order)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "static.npy"), out["static"][args.static_volume].cpu().numpy())
    np.save(os.path.join(args.out, "dynamic.npy"), out["dynamic"].cpu().numpy())
    print(json.dumps({"out": args.out, "files": ["dynamic.npy", "static.npy"], "volumes": int(raw.shape[0]), "volume_shape": list(out["static"].shape[1:]),
                      "mask_nodes": out["mask"].sum(dim=(1, 2, 3)).tolist(), "bounds": ",".join(repr(float(v)) for b in args.bounds for v in b)}))


if __name__ == "__main__":
    main()
