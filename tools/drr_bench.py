#!/usr/bin/env python3
"""Time of drr.project_sequence against the loop a user of the package writes without it, in ONE process:

    sequence   drr.project_sequence: rays generated on the device per chunk, one nca_drr_project of the static volume and one of all P
               dynamic volumes per (view, chunk), nca_view_compose per frame.  Timed with both kernel structures of nca_drr.hip:
               one thread per ray (split1) and four threads per ray, in four waves, whose sub-sums are folded in order (split4)
    loop       export.view_rays (f32), o + d z in torch, one torch.nn.functional.grid_sample per volume (static and each phase),
               (sigma * dists).sum(-1), and the composite (pix_s + pix_d) - I0: all in f32

at 256 x 256 pixels x 192 samples, V = 4 views, volumes of 128^3 and 256^3 with bounds +-1, P in {1, 10} phases.  Every leg is one warm-up
pass and then three timed passes; the legs alternate.  A whole sequence takes milliseconds here, so a timed pass is INNER = 20 sequences
back to back ending in one device synchronise, and the report is seconds per sequence: best and worst pass, and loop / sequence.  The tool
stops if the composite images of the two legs differ by more than 1e-5 relative (the project's f32 bound: the loop works in f32).

Then, recorded as information and gated nowhere: max |project_sequence(density_volumes(...)) - render_sequence(...)| over one view and
three phases for view_render_bench's default net pair at 64^3 / 128^3 / 256^3 with bounds +-1.2 -- the interpolation error of the grid.

    python3 tools/drr_bench.py [--out profiles/drr_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from view_render_bench import VIEWS, make_models, timed  # noqa: E402

PHASE_COUNTS = (1, 10)
VOLUME_SIDES = (128, 256)
REPEATS = 3
INNER = 20          # sequences per timed pass: one is 1 - 15 ms, too short a window on its own
BOUNDS = ((-1.0, 1.0),) * 3
AGREE = 1e-5
REPROJECT_SIDES = (64, 128, 256)
REPROJECT_BOUNDS = ((-1.2, 1.2),) * 3
REPROJECT_PHASES = [0, 3, 7]


def set_split(k):
    from nerfca_amd import _capi
    _capi.check_drr(_capi.lib().nca_drr_set_split(k))


@torch.no_grad()
def user_loop(vs, vd, geo, views, samples, bounds, chunk_rays=65536):
    """What projecting a volume pair takes without drr.project_sequence."""
    from nerfca_amd import export
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    dev = vs.device
    W, H = geo["nDetector"]
    P = vd.shape[0]
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], samples, dev)
    dists = _interval_lengths(z, z)
    lo = torch.tensor([b[0] for b in bounds], dtype=torch.float32, device=dev)
    hi = torch.tensor([b[1] for b in bounds], dtype=torch.float32, device=dev)
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    pred = torch.empty((len(views), P, W * H), dtype=torch.float32, device=dev)
    pred_d = torch.empty_like(pred)
    pred_s = torch.empty((len(views), W * H), dtype=torch.float32, device=dev)

    def sample(vol, grid):
        sig = torch.nn.functional.grid_sample(vol[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
        return i0 - (sig * dists).sum(-1)

    for v, (theta, phi) in enumerate(views):
        o, d = export.view_rays(geo, theta, phi, device=dev, dtype=torch.float32)
        for i in range(0, W * H, chunk_rays):
            pts = o[i:i + chunk_rays, None, :] + d[i:i + chunk_rays, None, :] * z[None, :, None]
            grid = (((pts - lo) / (hi - lo)) * 2 - 1).flip(-1)[None, None]          # x addresses the last volume axis
            pix_s = sample(vs, grid)
            pred_s[v, i:i + chunk_rays] = pix_s
            for j in range(P):
                pix_d = sample(vd[j], grid)
                pred_d[v, j, i:i + chunk_rays] = pix_d
                pred[v, j, i:i + chunk_rays] = (pix_s + pix_d) - i0
    return pred, pred_s, pred_d


def measure(dev, default_split, n_det, samples, side, n_phases):
    from nerfca_amd import drr, synthetic
    geo = synthetic.xcat_geometry(n_det)
    gen = torch.Generator(device=dev).manual_seed(side + n_phases)
    vs = torch.rand((side,) * 3, generator=gen, device=dev) * 0.02          # sigma of the order act(raw) * scale_value
    vd = torch.rand((n_phases,) + (side,) * 3, generator=gen, device=dev) * 0.02

    def sequence(k):
        set_split(k)
        try:
            return drr.project_sequence(vs, vd, geo, VIEWS, samples, bounds=BOUNDS)
        finally:
            set_split(default_split)

    legs = {"sequence_split1": lambda: sequence(1), "sequence_split4": lambda: sequence(4), "loop": lambda: user_loop(vs, vd, geo, VIEWS, samples, BOUNDS)}
    a1, a4, b = legs["sequence_split1"](), legs["sequence_split4"](), legs["loop"]()          # warm-up
    errs = {}
    for name, a in (("split1", a1), ("split4", a4)):
        errs[name] = float((a["pred"].reshape(b[0].shape) - b[0]).abs().max() / b[0].abs().max())
        if not errs[name] <= AGREE:
            sys.exit(f"drr_bench: the legs do not make the same images ({side}^3, P = {n_phases}, {name}: relative difference {errs[name]:.3e})")
    times = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, fn in legs.items():                              # alternate the legs
            times[k].append(timed(lambda: [fn() for _ in range(INNER)]) / INNER)
    rec = {"pixels": n_det * n_det, "samples": samples, "views": len(VIEWS), "volume": side, "phases": n_phases, "sequences_per_pass": INNER, "pred_rel_diff": errs}
    for k in legs:
        rec[k] = {"best_s": round(min(times[k]), 5), "worst_s": round(max(times[k]), 5)}
    for k in ("sequence_split1", "sequence_split4"):
        rec["loop_over_" + k + "_best"] = round(rec["loop"]["best_s"] / rec[k]["best_s"], 3)
    return rec


def reprojection(dev, n_det, samples, side):
    from nerfca_amd import drr, export, synthetic
    s, t = make_models(dev, "f32")
    geo = synthetic.xcat_geometry(n_det)
    view = [VIEWS[0]]
    want = export.render_sequence(s, t, geo, view, REPROJECT_PHASES, samples)
    sig_s, sig_d = export.density_volumes(s, t, REPROJECT_PHASES, resolution=(side,) * 3, bounds=REPROJECT_BOUNDS)
    got = drr.project_sequence(sig_s, sig_d, geo, view, samples, bounds=REPROJECT_BOUNDS)
    rec = {"reprojection_volume": side, "bounds": 1.2, "view": list(view[0]), "phases": REPROJECT_PHASES}
    for k in ("pred", "pred_static", "pred_dynamic"):
        rec["max_abs_diff_" + k] = float((got[k] - want[k]).abs().max())
    rec["image_range_pred"] = [float(want["pred"].min()), float(want["pred"].max())]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n-det", type=int, default=256)
    ap.add_argument("--samples", type=int, default=192)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("drr_bench needs the GPU: there is nothing to time without one")
    from nerfca_amd import _capi
    dev = torch.device("cuda:0")
    default_split = _capi.lib().nca_drr_get_split()
    lines = []
    for side in VOLUME_SIDES:
        for n_phases in PHASE_COUNTS:
            rec = measure(dev, default_split, args.n_det, args.samples, side, n_phases)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    table = [f"library default: split{default_split}; milliseconds per sequence of all V x P frames, best / worst pass",
             "volume  V x P     split1 ms          split4 ms          loop ms            loop/split1  loop/split4"]
    for r in lines:
        cells = "".join(f"   {1e3 * r[k]['best_s']:>7.3f} / {1e3 * r[k]['worst_s']:<7.3f}" for k in ("sequence_split1", "sequence_split4", "loop"))
        table.append(f"{r['volume']:>4}^3  {r['views']} x {r['phases']:<3}{cells}    {r['loop_over_sequence_split1_best']:>6.2f}       {r['loop_over_sequence_split4_best']:>6.2f}")
    reproj = []
    for side in REPROJECT_SIDES:
        rec = reprojection(dev, args.n_det, args.samples, side)
        print(json.dumps(rec), flush=True)
        reproj.append(rec)
    table.append("reprojection of exported volumes vs render_sequence (recorded, not gated): max |difference| of pred / pred_static / pred_dynamic")
    for r in reproj:
        table.append(f"{r['reprojection_volume']:>4}^3  {r['max_abs_diff_pred']:.3e} / {r['max_abs_diff_pred_static']:.3e} / {r['max_abs_diff_pred_dynamic']:.3e}"
                     f"   (pred spans {r['image_range_pred'][0]:.6f} .. {r['image_range_pred'][1]:.6f})")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines + reproj:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
