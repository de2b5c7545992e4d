#!/usr/bin/env python3
"""Compare two voxel reconstructions in 3-D: RMSE, the Dice coefficient and the distances of their thresholded masks.

    python3 tools/compare_volumes.py fitted/ phantom/ --bounds -0.18,0.18,-0.18,0.18,-0.18,0.18 --threshold 3 [--pred-threshold 0.5] [--out x.json]

Each directory holds static.npy [n0,n1,n2] and / or dynamic.npy [P,n0,n1,n2] as tools/make_phantom.py and tools/fit_volumes.py write them;
the first is the prediction, the second the truth.  For every file both hold: phantom.volume_errors (RMSE over all nodes, Dice of the masks
> threshold) and metrics.mask_distances (mean, Hausdorff and percentile distances between the masks, in the world units of --bounds, per
volume of the stack).  --pred-threshold thresholds the prediction at a value of its own (a sparse-view fit rarely reaches the truth's
densities); --pred-fraction F sets it to F times the prediction's own maximum instead.  --surface measures between the borders of the two
masks (metrics.mask_distances(surface=True)) and marks the record with "surface": true.  --cldice K adds the centreline Dice of the two
masks (metrics.cldice at K iterations, the same thresholds) per volume: "cldice", "tprec", "tsens" and "cldice_iterations".  --components
adds the component counts of the two masks (metrics.component_report at --connectivity C, 3 by default: 26 neighbours) per volume:
"components_pred", "components_truth", "betti0_error", "largest_share_pred", "largest_share_truth" and "connectivity".  With
--keep-largest K (and --components) the prediction's mask is also reduced to its K largest components (metrics.keep_largest), and the
distances and clDice of that mask against the truth are reported once more under "cleaned", beside the raw figures.  Prints one JSON record,
and writes it with --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from project_volumes import parse_bounds  # noqa: E402

NAMES = ("static", "dynamic")


def join_args(argv):
    """--bounds usually starts with a minus sign, which argparse would take for an option: hand it over as --bounds=LIST."""
    argv, out = list(argv), []
    while argv:
        a = argv.pop(0)
        out.append(a + "=" + argv.pop(0) if a == "--bounds" and argv else a)
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("pred", help="directory of the reconstruction")
    ap.add_argument("truth", help="directory of the truth")
    ap.add_argument("--bounds", required=True, type=parse_bounds, help="x0,x1,y0,y1,z0,z1: positions of the first and last node per axis")
    ap.add_argument("--threshold", required=True, type=float, help="a node belongs to the truth's mask when its value is above this")
    ap.add_argument("--pred-threshold", type=float, default=None, help="threshold of the prediction (default: --threshold)")
    ap.add_argument("--pred-fraction", type=float, default=None, help="threshold the prediction at this fraction of its own maximum")
    ap.add_argument("--percentile", type=float, default=95.0)
    ap.add_argument("--surface", action="store_true", help="measure between the borders of the masks (MedPy's surface distances), not between whole bodies")
    ap.add_argument("--cldice", type=int, default=None, metavar="K", help="add clDice, topology precision and sensitivity of the masks at K skeleton iterations")
    ap.add_argument("--components", action="store_true", help="add the component counts, the Betti-0 error and the share of the largest component of the masks")
    ap.add_argument("--connectivity", type=int, default=3, choices=(1, 2, 3), metavar="C", help="with --components: 1, 2 or 3 for 6, 18 or 26 neighbours (default 3)")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="with --components: also report the distances and clDice of the prediction reduced to its K largest components")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="also write the record to this file")
    return ap


def compare(pred, truth, bounds, threshold, pred_threshold, percentile, surface=False, cldice=None, components=False, connectivity=3, keep_largest=None):
    """The record of one pair of device tensors of one shape."""
    from nerfca_amd import metrics, phantom
    rec = phantom.volume_errors(pred, truth, threshold)
    rec["pred_threshold"] = threshold if pred_threshold is None else pred_threshold
    if surface:
        rec["surface"] = True
    dist = metrics.mask_distances(pred, truth, bounds, threshold=threshold, pred_threshold=pred_threshold, percentile=percentile, surface=surface)
    rec.update({k: v.reshape(-1).tolist() for k, v in dist.items()})
    if cldice is not None:
        rec["cldice_iterations"] = cldice
        rec.update({k: v.reshape(-1).tolist() for k, v in metrics.cldice(pred, truth, iterations=cldice, threshold=threshold, pred_threshold=pred_threshold).items()})
    if components:
        rec["connectivity"] = connectivity
        report = metrics.component_report(pred, truth, threshold=threshold, pred_threshold=pred_threshold, connectivity=connectivity)
        rec.update({k: v.reshape(-1).tolist() for k, v in report.items()})
    if keep_largest is not None:
        import torch
        kept = metrics.keep_largest(pred, keep_largest, threshold=rec["pred_threshold"], connectivity=connectivity)
        truth_mask = (truth > threshold).to(torch.float32)          # the cleaned prediction is a mask: both sides at 0 / 1, threshold one half
        dist = metrics.mask_distances(kept.to(torch.float32), truth_mask, bounds, threshold=0.5, percentile=percentile, surface=surface)
        rec["cleaned"] = {"keep_largest": keep_largest, **{k: v.reshape(-1).tolist() for k, v in dist.items()}}
        if cldice is not None:
            rec["cleaned"].update({k: v.reshape(-1).tolist() for k, v in metrics.cldice(kept, truth_mask, iterations=cldice, threshold=0.5).items()})
    return rec


def main(argv=None):
    args = parser().parse_args(join_args(sys.argv[1:] if argv is None else argv))
    import torch
    if args.pred_threshold is not None and args.pred_fraction is not None:
        sys.exit("compare_volumes: --pred-threshold and --pred-fraction exclude each other")
    if args.keep_largest is not None and not args.components:
        sys.exit("compare_volumes: --keep-largest cleans the mask --components reports on: give --components too")
    if args.keep_largest is not None and args.keep_largest < 1:
        sys.exit(f"compare_volumes: --keep-largest {args.keep_largest} is not a whole number >= 1")
    out = {"pred": args.pred, "truth": args.truth, "bounds": [list(b) for b in args.bounds], "threshold": args.threshold, "percentile": args.percentile}
    for name in NAMES:
        a, b = (os.path.join(d, name + ".npy") for d in (args.pred, args.truth))
        if not (os.path.exists(a) and os.path.exists(b)):
            continue
        pred, truth = (torch.from_numpy(np.load(p).astype(np.float32)).to(args.device) for p in (a, b))
        if pred.shape != truth.shape:
            sys.exit(f"compare_volumes: {a} is {tuple(pred.shape)}, {b} is {tuple(truth.shape)}")
        pthr = args.pred_threshold if args.pred_fraction is None else args.pred_fraction * float(pred.max())
        out[name] = compare(pred, truth, args.bounds, args.threshold, pthr, args.percentile, args.surface, args.cldice, args.components, args.connectivity,
                            args.keep_largest)
    if not any(n in out for n in NAMES):
        sys.exit(f"compare_volumes: {args.pred} and {args.truth} share neither static.npy nor dynamic.npy")
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
