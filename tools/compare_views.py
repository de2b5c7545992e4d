#!/usr/bin/env python3
"""PSNR and SSIM per (view, phase) between two image sequences on disk (metrics.compare_sequences).

    python3 tools/compare_views.py renders/manifest.json projections/manifest.json [--out table.json] [--data-range 1.0]

Both arguments are a manifest.json as tools/render_views.py / tools/project_volumes.py write it: the first is the prediction, the second the
truth.  Every stack both list with one shape (pred [V,P,W,H], pred_static [V,W,H], ...) is compared; the two must list the same views and
phases.  --data-range is the dynamic range of the images (default: max - min of each truth image).  Prints one line per stack, view and
phase, then the means; --out writes the same numbers as JSON.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("pred", help="manifest.json of the prediction")
    ap.add_argument("truth", help="manifest.json of the truth")
    ap.add_argument("--data-range", type=float, default=None, help="dynamic range of the images (default: max - min of each truth image)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="also write the table as JSON to this file")
    return ap


def load_stacks(manifest_path):
    """(manifest, {name: numpy stack}) of the image stacks a manifest lists."""
    import numpy as np
    with open(manifest_path) as f:
        m = json.load(f)
    for key in ("views", "files"):
        if key not in m:
            raise ValueError(f"{manifest_path}: no {key!r} entry: not a manifest of project_volumes / render_views")
    here = os.path.dirname(os.path.abspath(manifest_path))
    return m, {k: np.load(os.path.join(here, v["file"])) for k, v in m["files"].items()}


def table_rows(result, views, phases):
    """[(stack, view, phase or None, psnr, ssim)] of a compare_sequences result, read back once per stack."""
    rows = []
    for key, r in result.items():
        p, s = r["psnr"].cpu().tolist(), r["ssim"].cpu().tolist()
        for v, view in enumerate(views):
            if r["psnr"].dim() == 1:
                rows.append((key, view, None, p[v], s[v]))
            else:
                rows.extend((key, view, phases[j], p[v][j], s[v][j]) for j in range(len(phases)))
    return rows


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    from nerfca_amd import metrics
    if not torch.cuda.is_available():
        sys.exit("compare_views needs the GPU: there is no CPU path")
    dev = torch.device(args.device)
    (ma, a), (mb, b) = load_stacks(args.pred), load_stacks(args.truth)
    if ma["views"] != mb["views"] or ma.get("phases") != mb.get("phases"):
        sys.exit("compare_views: the two manifests list different views or phases")
    views = [tuple(v) for v in ma["views"]]
    phases = [0] if ma.get("phases") is None else list(ma["phases"])
    result = metrics.compare_sequences({k: torch.from_numpy(v).to(dev) for k, v in a.items()}, {k: torch.from_numpy(v).to(dev) for k, v in b.items()},
                                       data_range=args.data_range)
    rows = table_rows(result, views, phases)
    print("stack           view (theta, phi)    phase    PSNR dB    SSIM")
    for key, view, phase, p, s in rows:
        print(f"{key:<15} {str(view):<20} {'-' if phase is None else phase:<8} {p:>8.3f}   {s:.6f}")
    means = {k: {"psnr_mean": float(r["psnr_mean"]), "ssim_mean": float(r["ssim_mean"])} for k, r in result.items()}
    for k, mvals in means.items():
        print(f"{k:<15} mean                          {mvals['psnr_mean']:>8.3f}   {mvals['ssim_mean']:.6f}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"pred": args.pred, "truth": args.truth, "data_range": args.data_range,
                       "rows": [{"stack": k, "view": list(v), "phase": ph, "psnr": p, "ssim": s} for k, v, ph, p, s in rows], "means": means}, f, indent=1)


if __name__ == "__main__":
    main()
