#!/usr/bin/env python3
"""Render C-arm views and heart-phase sequences from two checkpoints (export.render_sequence) and write them as .npy stacks.

    python3 tools/render_views.py --static static.pth --dynamic temporal.pth --geometry xcat --n-det 128 \\
        --views "-5,40;60,-30" --phases 0,3,7 --samples 192 --precision bf16 --normalize --out renders/

--static / --dynamic are files written by CPPN.save / Temporal.save (export.load_checkpoint restores the encoding windows); without
--dynamic the static field is rendered alone.  --geometry is `xcat` or `magix` (with --n-det) or a JSON file with the keys DSD, DSO,
nDetector, dDetector, offDetector, near_thresh, far_thresh, max_pixel_value.  A view is "theta,phi" or "theta,phi,larm" in degrees.

Writes pred.npy and pred_dynamic.npy [V,P,W,H], pred_static.npy [V,W,H] (f32, un-normalised I0 - sum sigma dists), with --normalize
the three *_norm.npy stacks, and manifest.json (views, phases, shapes, geometry, per-frame min / max when normalised).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEO_KEYS = ("DSD", "DSO", "nDetector", "dDetector", "offDetector", "near_thresh", "far_thresh", "max_pixel_value")


def parse_views(text):
    """ "t,p;t,p,l;..." -> [(theta, phi, larm), ...] (larm 0 when left out)."""
    views = []
    for item in text.split(";"):
        item = item.strip()
        if not item:
            continue
        parts = [float(x) for x in item.split(",")]
        if len(parts) not in (2, 3):
            raise ValueError(f"a view is 'theta,phi' or 'theta,phi,larm', got {item!r}")
        views.append((parts[0], parts[1], parts[2] if len(parts) == 3 else 0.0))
    if not views:
        raise ValueError("no views given")
    return views


def parse_phases(text):
    phases = [int(x) for x in text.split(",") if x.strip()]
    if not phases:
        raise ValueError("no phases given")
    return phases


def load_geometry(name, n_det):
    if name in ("xcat", "magix"):
        from nerfca_amd import synthetic
        return synthetic.GEOMETRIES[name](n_det)
    with open(name) as f:
        geo = json.load(f)
    missing = [k for k in GEO_KEYS if k not in geo]
    if missing:
        raise ValueError(f"{name}: geometry keys missing: {', '.join(missing)}")
    return {k: geo[k] for k in GEO_KEYS}


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--static", required=True, help="checkpoint of the static net (CPPN.save)")
    ap.add_argument("--dynamic", default=None, help="checkpoint of the dynamic net (Temporal.save); left out: static field only")
    ap.add_argument("--geometry", default="xcat", help="xcat | magix | path of a JSON geometry")
    ap.add_argument("--n-det", type=int, default=128, help="detector pixels per side of the xcat / magix geometry")
    ap.add_argument("--views", required=True, type=parse_views, help='"theta,phi;theta,phi[,larm];..." in degrees')
    ap.add_argument("--phases", default="0", type=parse_phases, help="heart phases, comma separated")
    ap.add_argument("--samples", type=int, default=192, help="depth samples per ray")
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--normalize", action="store_true", help="also write the per-frame (x - min) / (max - min) images")
    ap.add_argument("--chunk-rays", type=int, default=65536)
    ap.add_argument("--output-activation", default="softplus")
    ap.add_argument("--scale-value", type=float, default=1e-2)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def join_views(argv):
    """A view list usually starts with a minus sign ("-5,40;60,-30"), which argparse would take for an option: hand it over as --views=LIST."""
    argv, out = list(argv), []
    while argv:
        a = argv.pop(0)
        out.append(a + "=" + argv.pop(0) if a == "--views" and argv else a)
    return out


def main(argv=None):
    args = parser().parse_args(join_views(sys.argv[1:] if argv is None else argv))
    import numpy as np
    import torch
    from nerfca_amd import export, set_precision
    if not torch.cuda.is_available():
        sys.exit("render_views needs the GPU: there is no CPU path")
    dev = torch.device(args.device)
    geo = load_geometry(args.geometry, args.n_det)
    static, _ = export.load_checkpoint(args.static, device=dev)
    dynamic = export.load_checkpoint(args.dynamic, device=dev)[0] if args.dynamic else None
    set_precision(args.precision, *([static] + ([dynamic] if dynamic is not None else [])))
    out = export.render_sequence(static, dynamic, geo, args.views, args.phases, args.samples, output_activation=args.output_activation,
                                 scale_value=args.scale_value, chunk_rays=args.chunk_rays, normalize=args.normalize)
    os.makedirs(args.out, exist_ok=True)
    files = {}
    for k, t in out.items():
        if k != "minmax":
            np.save(os.path.join(args.out, k + ".npy"), t.cpu().numpy())
            files[k] = {"file": k + ".npy", "shape": list(t.shape)}
    manifest = {"views": [list(v) for v in args.views], "phases": args.phases if dynamic is not None else None, "samples": args.samples,
                "precision": args.precision, "geometry": geo, "files": files}
    if args.normalize:
        manifest["minmax"] = {k: t.cpu().tolist() for k, t in out["minmax"].items()}
    with open(os.path.join(args.out, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(json.dumps({"out": args.out, "files": sorted(files)}))


if __name__ == "__main__":
    main()
