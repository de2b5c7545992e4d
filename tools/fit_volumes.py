#!/usr/bin/env python3
"""Fit a static volume and a stack of phase volumes to projections (drr.fit_volumes) and write them as .npy.

    python3 tools/fit_volumes.py --frames projections/manifest.json --shape 64,64,64 --bounds -1,1,-1,1,-1,1 --steps 200 --lr 0.01 \\
        --out fitted/

--frames is the manifest.json tools/project_volumes.py or tools/render_views.py wrote: its `pred` stack [V,P,W,H] next to it holds the
composite frames, one per (view, phase), in the log space of the datasets; its geometry is the C-arm the frames were taken with.  A
manifest without phases (a static-only run) is read as phase 0 of every view.  --shape n0,n1,n2 and --bounds x0,x1,y0,y1,z0,z1 place the
grid to fit (linspace(lo, hi, n) nodes per axis; --bounds defaults to the manifest's, else to +-1).  --samples defaults to the manifest's.
--n-phases is the length of the dynamic stack (default: the largest phase of the manifest + 1).  Views with a C-arm roll (larm != 0) are
refused: drr.fit_volumes takes (theta, phi).  --tv-space / --tv-time weigh the total-variation priors in space and between neighbouring
heart phases (drr.total_variation; 0, the default, fits the data term alone), --tv-eps is their smoothing constant.  --ssim-weight adds
ssim_weight (1 - mean SSIM of the predicted frames) to the objective (metrics.ssim; 0, the default, launches nothing of it), --ssim-win
is its window length (odd, at most 11, no larger than the detector).

Writes static.npy [n0,n1,n2] and dynamic.npy [n_phases,n0,n1,n2] (f32), the files tools/project_volumes.py reads back with --static /
--dynamic, and fit.json (the loss before each step; with a prior on, also the two unweighted total variations before each step; with --ssim-weight, also the
mean SSIM before each step).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from project_volumes import parse_bounds  # noqa: E402
from render_views import GEO_KEYS  # noqa: E402


def parse_shape(text):
    """ "n0,n1,n2" -> (n0, n1, n2), each at least 2 nodes."""
    v = [int(x) for x in text.split(",") if x.strip()]
    if len(v) != 3 or any(n < 2 for n in v):
        raise ValueError(f"a shape is three node counts n0,n1,n2 of at least 2, got {text!r}")
    return tuple(v)


def join_args(argv):
    """--bounds usually starts with a minus sign, which argparse would take for an option: hand it over as --bounds=LIST."""
    argv, out = list(argv), []
    while argv:
        a = argv.pop(0)
        out.append(a + "=" + argv.pop(0) if a == "--bounds" and argv else a)
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", required=True, help="manifest.json of tools/project_volumes.py or tools/render_views.py")
    ap.add_argument("--shape", required=True, type=parse_shape, help="n0,n1,n2: nodes per axis of the volumes to fit")
    ap.add_argument("--bounds", default=None, type=parse_bounds, help="x0,x1,y0,y1,z0,z1 (default: the manifest's bounds, else -1,1 on each axis)")
    ap.add_argument("--samples", type=int, default=None, help="depth samples per ray (default: the manifest's)")
    ap.add_argument("--n-phases", type=int, default=None, help="volumes of the dynamic stack (default: largest phase of the manifest + 1)")
    ap.add_argument("--steps", type=int, default=200, help="Adam steps")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--allow-negative", action="store_true", help="do not clamp the volumes at 0 after each step")
    ap.add_argument("--chunk-rays", type=int, default=65536)
    ap.add_argument("--tv-space", type=float, default=0.0, help="weight of the spatial total variation of the static volume and the stack")
    ap.add_argument("--tv-time", type=float, default=0.0, help="weight of the total variation between neighbouring phases of the cyclic stack")
    ap.add_argument("--tv-eps", type=float, default=1e-3, help="smoothing constant of both total variations")
    ap.add_argument("--ssim-weight", type=float, default=0.0, help="weight of 1 - mean SSIM of the predicted frames")
    ap.add_argument("--ssim-win", type=int, default=11, help="window length of the SSIM term (odd, at most 11)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", required=True, help="output directory")
    return ap


def load_frames(manifest_path):
    """(geo, frames, info) of a manifest: frames is [(theta, phi, phase, image f32 numpy [W,H])], one per (view, phase) of the `pred` stack;
    info holds the manifest's samples and bounds (None where it has none) and n_phases = largest phase + 1."""
    import numpy as np
    with open(manifest_path) as f:
        m = json.load(f)
    for key in ("views", "geometry", "files"):
        if key not in m:
            raise ValueError(f"{manifest_path}: no {key!r} entry: not a manifest of project_volumes / render_views")
    missing = [k for k in GEO_KEYS if k not in m["geometry"]]
    if missing:
        raise ValueError(f"{manifest_path}: geometry keys missing: {', '.join(missing)}")
    if "pred" not in m["files"]:
        raise ValueError(f"{manifest_path}: no pred stack listed")
    geo = {k: m["geometry"][k] for k in GEO_KEYS}
    W, H = (int(v) for v in geo["nDetector"])
    views = [tuple(float(a) for a in v) for v in m["views"]]
    if any(len(v) not in (2, 3) for v in views):
        raise ValueError(f"{manifest_path}: a view is (theta, phi[, larm])")
    if any(len(v) == 3 and v[2] != 0.0 for v in views):
        raise ValueError(f"{manifest_path}: a view with a C-arm roll (larm != 0) cannot be fitted")
    phases = [0] if m.get("phases") is None else [int(p) for p in m["phases"]]
    pred = np.load(os.path.join(os.path.dirname(os.path.abspath(manifest_path)), m["files"]["pred"]["file"]))
    if pred.shape != (len(views), len(phases), W, H):
        raise ValueError(f"{manifest_path}: pred is {pred.shape}, the manifest says {(len(views), len(phases), W, H)}")
    if any(p < 0 for p in phases):
        raise ValueError(f"{manifest_path}: negative phase in {phases}")
    frames = [(v[0], v[1], p, np.ascontiguousarray(pred[i, j], dtype=np.float32)) for i, v in enumerate(views) for j, p in enumerate(phases)]
    bounds = m.get("bounds")
    info = {"samples": m.get("samples"), "bounds": None if bounds is None else tuple((float(b[0]), float(b[1])) for b in bounds), "n_phases": max(phases) + 1}
    return geo, frames, info


def main(argv=None):
    args = parser().parse_args(join_args(sys.argv[1:] if argv is None else argv))
    import numpy as np
    import torch
    from nerfca_amd import drr
    if not torch.cuda.is_available():
        sys.exit("fit_volumes needs the GPU: there is no CPU path")
    dev = torch.device(args.device)
    geo, frames, info = load_frames(args.frames)
    samples = info["samples"] if args.samples is None else args.samples
    if samples is None:
        sys.exit("--samples: the manifest names none")
    bounds = args.bounds or info["bounds"] or ((-1.0, 1.0),) * 3
    n_phases = info["n_phases"] if args.n_phases is None else args.n_phases
    out = drr.fit_volumes([(t, p, ph, torch.from_numpy(img).to(dev)) for t, p, ph, img in frames], geo, args.shape, samples, bounds=bounds,
                          n_phases=n_phases, steps=args.steps, lr=args.lr, nonneg=not args.allow_negative, chunk_rays=args.chunk_rays,
                          tv_space=args.tv_space, tv_time=args.tv_time, tv_eps=args.tv_eps, ssim_weight=args.ssim_weight, ssim_win=args.ssim_win)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "static.npy"), out["static"].cpu().numpy())
    np.save(os.path.join(args.out, "dynamic.npy"), out["dynamic"].cpu().numpy())
    record = {"frames": len(frames), "shape": list(args.shape), "bounds": [list(b) for b in bounds], "samples": samples, "n_phases": n_phases,
              "steps": args.steps, "lr": args.lr, "tv_space_weight": args.tv_space, "tv_time_weight": args.tv_time, "tv_eps": args.tv_eps, "loss": out["loss"]}
    if args.ssim_weight > 0:
        record.update({"ssim_weight": args.ssim_weight, "ssim_win": args.ssim_win})
    record.update({k: out[k] for k in ("tv_space", "tv_time", "ssim") if k in out})
    with open(os.path.join(args.out, "fit.json"), "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps({"out": args.out, "files": ["dynamic", "static"], "first_loss": out["loss"][0], "last_loss": out["loss"][-1]}))


if __name__ == "__main__":
    main()
