#!/usr/bin/env python3
"""What the total-variation priors do to a sparse-view voxel fit against known truth, on the procedural phantom (nerfca_amd.phantom).

Per grid size n (64 and 128 nodes per axis), with P = 10 heart phases at synthetic.xcat_geometry:

  1. make_phantom((n, n, n), 10): the truth, a static thorax and a beating coronary tree.
  2. drr.project_sequence of the truth through the four training views (-30,30), (-30,-30), (60,-30), (60,30) at every phase: 40 frames.
     The frames come from the grid that is fitted, so a volume pair with loss 0 exists: what is measured is what four views leave open.
  3. drr.fit_volumes from zeros, with the priors off and with tv_space / tv_time on (a small table of weights).
  4. phantom.volume_errors of the fitted volumes against the truth: RMSE of the static volume, of the dynamic stack and of their sum
     (the split between the two is not determined by the frames, their sum is what a ray sees), the Dice coefficient of the vessel mask
     (dynamic > a quarter and > a twentieth of the vessel density), the largest fitted dynamic value, and the PSNR of the held-out view
     (-5, 40) over all phases (peak = the range of the true images), and the mean SSIM of the same held-out frames (metrics.ssim, window 11,
     the range of each true frame).

--ssim-weight W[,W..] adds, per grid size and weight, a fit with the structural term alone (ssim_weight = W) and one with it next to the
spatial prior (tv_space 1e-5, the best PSNR row of the table at 64 nodes): whether a structural loss moves the vessel figures.  Without
the option the rows are the table of total-variation weights alone.

Also the reprojection distance of the phantom per grid size: project_sequence of the phantom rasterised at n against the same phantom
rasterised at 256 nodes per axis, over the four training views and all phases.

--distances adds three columns per row, of the fitted dynamic stack against the truth (metrics.mask_distances / centreline_coverage): the
mean symmetric distance `assd` and the 95th-percentile Hausdorff distance `hd95` between the truth's mask (> rho / 4) and the fit's mask
(> a quarter of the fit's OWN maximum: the fits top out far below rho), in units of the node spacing, averaged over the phases, and the
share of the true centreline (phantom.centreline_points at half a node spacing) within one cell diagonal of the fit's mask.  Without the
option the output is what it was.  --cldice K (with --distances) adds a fourth: the centreline Dice of the same two masks at K skeleton
iterations (metrics.cldice), averaged over the phases -- graded where the Dice coefficient of the masks is 0.  --components (with
--distances) adds the component count of the fit's mask (metrics.component_report, 26 neighbours; the truth's count beside it), the share of
its largest component, and `assd` and `hd95` once more for the fit's mask reduced to its --keep-largest K largest components (K = 1 by
default; metrics.keep_largest), all averaged over the phases: how much of the distances is debris and how much is the artery.
--vesselness (with --distances, --cldice and --components) adds, after every fit, a row in which the fitted dynamic stack is replaced by
its multi-scale Hessian vesselness (ccta.vesselness at --vesselness-sigmas, Frangi's c) before it is thresholded at a quarter of its own
maximum, with the same columns against the same truth, and a second table that sets the two inputs side by side, with the Dice
coefficient of the two masks.  --centreline (on its own) adds a table of the centreline TREE centreline.extract finds at phase 0 in the
truth and in every fit, rooted at the mask node nearest the first segment's start: the share of its points within a cell diagonal of
phantom.centreline_points and the reverse, the radius error against the table's radius at the nearest true point, and the branch count
beside the table's leaves (profiles/phantom_study_centreline.txt).  --lumen (on its own) adds a table of LUMEN DIAMETERS: along every
chain of segments of the table (tools/cpr_bench.py segment_chains; reformat.frames of the chain's joints at half a node spacing), at every
heart phase, reformat.lumen_profile of the truth at rho / 4 and of every fit at a quarter of its own maximum (64 rays out to four times the
largest radius of the table): the mean absolute error of d_eq / 2 against the table's radius at the plane, in node spacings, over the
planes of status 0, and the share of such planes (profiles/phantom_study_lumen.txt).  The phantom's wall is a ramp one node spacing wide,
centred on the table's radius, so at rho / 4 the truth itself reads a quarter of a spacing wide.

These numbers are recorded and gated nowhere.

    python3 tools/phantom_study.py [--out profiles/phantom_study.txt]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PHASES = 10
HELD_OUT = (-5.0, 40.0)
WEIGHTS = [(0.0, 0.0), (1e-5, 0.0), (1e-4, 0.0), (0.0, 1e-1), (0.0, 1.0), (0.0, 10.0), (1e-5, 1e-1), (1e-5, 1.0), (1e-4, 1.0)]          # (tv_space, tv_time)
FINE = 256


def psnr(pred, truth):
    mse = float(((pred.double() - truth.double()) ** 2).mean())
    peak = float(truth.max() - truth.min())
    return math.inf if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def ssim_rows(ssim_weights):
    """(tv_space, tv_time, ssim_weight) of the rows --ssim-weight adds."""
    return [(tv_space, 0.0, w) for w in ssim_weights for tv_space in (0.0, 1e-5)]


def distance_columns(fit_dynamic, dynamic, bounds, segments, threshold, cldice=None, keep=None):
    """{"assd_cells", "hd95_cells", "centreline_coverage", ...}: the means over the phases, distances in units of the node spacing."""
    from nerfca_amd import metrics, phantom
    side = dynamic.shape[-1]
    h = [(b[1] - b[0]) / (side - 1) for b in bounds]
    own = 0.25 * float(fit_dynamic.max())
    d = metrics.mask_distances(fit_dynamic, dynamic, bounds, threshold=threshold, pred_threshold=own)
    points = phantom.centreline_points(segments, 0.5 * min(h))
    c = metrics.centreline_coverage(fit_dynamic, bounds, points, threshold=own, tol=math.sqrt(sum(x * x for x in h)))
    cell = max(h)
    extra = {}
    if cldice is not None:
        t = metrics.cldice(fit_dynamic, dynamic, iterations=cldice, threshold=threshold, pred_threshold=own)
        extra = {"cldice_iterations": cldice, "cldice": float(t["cldice"].mean()), "tprec": float(t["tprec"].mean()), "tsens": float(t["tsens"].mean())}
    if keep is not None:
        r = metrics.component_report(fit_dynamic, dynamic, threshold=threshold, pred_threshold=own)
        kept = metrics.keep_largest(fit_dynamic, keep, threshold=own).to(torch.float32)
        k = metrics.mask_distances(kept, (dynamic > threshold).to(torch.float32), bounds, threshold=0.5)
        extra.update({"keep_largest": keep, "components": float(r["components_pred"].double().mean()), "components_truth": float(r["components_truth"].double().mean()),
                      "betti0_error": float(r["betti0_error"].double().mean()), "largest_share": float(r["largest_share_pred"].mean()),
                      "assd_cleaned_cells": float(k["assd"].mean()) / cell, "hd95_cleaned_cells": float(k["hd_percentile"].mean()) / cell,
                      "hausdorff_cleaned_cells": float(k["hausdorff"].mean()) / cell, "n_cleaned_mean": float(k["n_pred"].double().mean())})
    return {**extra, "pred_threshold": own, "assd_cells": float(d["assd"].mean()) / cell, "hd95_cells": float(d["hd_percentile"].mean()) / cell,
            "hausdorff_cells": float(d["hausdorff"].mean()) / cell, "pred_to_truth_cells": float(d["pred_to_truth"].mean()) / cell,
            "truth_to_pred_cells": float(d["truth_to_pred"].mean()) / cell, "n_pred_mean": float(d["n_pred"].double().mean()),
            "n_truth_mean": float(d["n_truth"].double().mean()), "centreline_coverage": float(c["coverage"].mean()),
            "centreline_mean_distance_cells": float(c["mean_distance"].mean()) / cell}


def mask_dice(pred, truth, pred_threshold, threshold):
    """The Dice coefficient of pred > pred_threshold and truth > threshold per volume, averaged over the phases."""
    a, b = pred > pred_threshold, truth > threshold
    dims = (-3, -2, -1)
    return float((2.0 * (a & b).sum(dims).double() / (a.sum(dims).double() + b.sum(dims).double())).mean())


def truth_tree(table, step):
    """(points f64 [n, 3], radius f64 [n], leaves) of ONE phase of a segment table [N, 8]: every row sampled as phantom.centreline_points
    samples it, with the radius interpolated between the row's two; `leaves` counts the row ends that are no row's start."""
    import numpy as np
    pts, rad = [], []
    for row in np.asarray(table, dtype=np.float64):
        a, b = row[0:3], row[3:6]
        m = max(1, int(math.ceil(float(np.linalg.norm(b - a)) / step)))
        t = np.arange(m + 1, dtype=np.float64) / m
        pts.append(a[None, :] + t[:, None] * (b - a)[None, :])
        rad.append(row[6] + t * (row[7] - row[6]))
    starts = {tuple(np.round(row[0:3], 9)) for row in np.asarray(table)}
    leaves = sum(tuple(np.round(row[3:6], 9)) not in starts for row in np.asarray(table))
    return np.concatenate(pts), np.concatenate(rad), leaves


def centreline_row(vol, bounds, table, threshold, max_paths=64):
    """The tree centreline.extract finds in ONE volume against one phase of the segment table: the root is the mask node nearest the first
    segment's start; overlap both ways within a cell diagonal, the radius error at the nearest true point, the branch counts."""
    from nerfca_amd import centreline
    side = vol.shape[-1]
    h = [(b[1] - b[0]) / (side - 1) for b in bounds]
    tol = math.sqrt(sum(x * x for x in h))
    true_pts, true_rad, leaves = truth_tree(table, 0.5 * min(h))
    mask = vol > threshold
    if not bool(mask.any()):
        return {"branches": 0, "branches_truth": leaves, "empty_mask": True}
    idx = mask.nonzero().to(torch.float64)
    world = torch.tensor([b[0] for b in bounds], dtype=torch.float64, device=vol.device) + idx * torch.tensor(h, dtype=torch.float64, device=vol.device)
    start = torch.tensor(table[0][0:3], dtype=torch.float64, device=vol.device)
    gap = (world - start).norm(dim=1)
    root = tuple(float(v) for v in world[int(gap.argmin())])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = centreline.extract(vol, bounds, threshold=threshold, root=root, max_paths=max_paths)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    found = torch.cat(c.points).to(torch.float64)
    truth = torch.tensor(true_pts, device=vol.device)
    found_near, truth_near = centreline.overlap(found, truth, tol)
    d = torch.cdist(found, truth)
    near, which = d.min(dim=1)
    ok = near <= tol
    err = (torch.cat(c.radius).to(torch.float64) - torch.tensor(true_rad, device=vol.device)[which]).abs()[ok]
    return {"branches": len(c.paths), "branches_truth": leaves, "total_length": float(sum(c.length)), "reached": c.reached, "root_gap_cells": float(gap.min()) / max(h),
            "found_within_diagonal_of_truth": found_near, "truth_within_diagonal_of_found": truth_near,
            "radius_error_mean_cells": float(err.mean()) / max(h) if int(ok.sum()) else math.nan, "extract_seconds": round(seconds, 3)}


def lumen_row(stack, bounds, segments, level):
    """reformat.lumen_profile of the stack [P, n, n, n] along every chain of the segment table [P, N, 8], phase by phase, against the table's
    radius: the mean |d_eq / 2 - radius| over the planes of status 0 in node spacings, the mean signed error, and the share of such planes."""
    import numpy as np
    from nerfca_amd import reformat
    from tools.cpr_bench import segment_chains
    side = stack.shape[-1]
    h = [(b[1] - b[0]) / (side - 1) for b in bounds]
    r_max = 4.0 * float(np.asarray(segments)[..., 6:8].max())
    err, signed, ok, planes = 0.0, 0.0, 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(stack.shape[0]):
        for joints, radius in segment_chains(segments[p]):
            fr = reformat.frames(joints, step=0.5 * min(h))
            at = np.concatenate([[0.0], np.cumsum(np.sqrt(((joints[1:] - joints[:-1]) ** 2).sum(1)))])
            want = torch.tensor(np.interp(fr.s, at, radius), device=stack.device)
            prof = reformat.lumen_profile(stack[p], bounds, fr, level=level, r_max=r_max, n_angles=64)
            good = prof.status == 0
            d = (0.5 * prof.d_eq - want)[good]
            err, signed, ok, planes = err + float(d.abs().sum()), signed + float(d.sum()), ok + int(good.sum()), planes + good.numel()
    torch.cuda.synchronize()
    return {"lumen_planes": planes, "lumen_status0_share": ok / planes, "lumen_radius_mae_cells": err / ok / max(h) if ok else math.nan,
            "lumen_radius_bias_cells": signed / ok / max(h) if ok else math.nan, "lumen_seconds": round(time.perf_counter() - t0, 3)}


def study(dev, side, n_det, samples, steps, lr, weights, distances=False, cldice=None, keep=None, vesselness=None, centreline=None, lumen=None):
    """The rows of one grid size; with `vesselness` (the sigmas) also the side-by-side rows of the fit and of its vesselness; with
    `centreline` (a list) the centreline rows of the truth and of every fit, at phase 0, are appended to it; with `lumen` (a list) the lumen
    rows of the truth and of every fit, over all phases."""
    from nerfca_amd import ccta, drr, metrics, phantom, synthetic
    geo = synthetic.xcat_geometry(n_det)
    ph = phantom.make_phantom((side,) * 3, PHASES, geo, device=dev)
    bounds, static, dynamic = ph["bounds"], ph["static"], ph["dynamic"]
    views = [tuple(float(a) for a in v) for v in synthetic.TRAIN_VIEWS]
    train = drr.project_sequence(static, dynamic, geo, views, samples, bounds=bounds)["pred"]
    held = drr.project_sequence(static, dynamic, geo, [HELD_OUT], samples, bounds=bounds)["pred"]
    frames = [(theta, phi, p, train[v, p].contiguous()) for v, (theta, phi) in enumerate(views) for p in range(PHASES)]
    threshold = 0.25 * phantom.RHO_VESSEL
    rows, pairs = [], []
    if centreline is not None:
        centreline.append({"volume": side, "input": "truth", **centreline_row(dynamic[0], bounds, ph["segments"][0], threshold)})
        print(json.dumps(centreline[-1]), flush=True)
    if lumen is not None:
        lumen.append({"volume": side, "input": "truth", "level": threshold, **lumen_row(dynamic, bounds, ph["segments"], threshold)})
        print(json.dumps(lumen[-1]), flush=True)
    held_range = held.amax(dim=(-2, -1)).double() - held.amin(dim=(-2, -1)).double()
    for tv_space, tv_time, *rest in weights:
        ssim_weight = rest[0] if rest else 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = drr.fit_volumes(frames, geo, (side,) * 3, samples, bounds=bounds, n_phases=PHASES, steps=steps, lr=lr, tv_space=tv_space, tv_time=tv_time,
                              ssim_weight=ssim_weight)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        e_s = phantom.volume_errors(fit["static"], static)
        e_d = phantom.volume_errors(fit["dynamic"], dynamic, threshold)
        e_low = phantom.volume_errors(fit["dynamic"], dynamic, 0.2 * threshold)
        e_sum = phantom.volume_errors(fit["static"][None] + fit["dynamic"], static[None] + dynamic)
        again = drr.project_sequence(fit["static"], fit["dynamic"], geo, [HELD_OUT], samples, bounds=bounds)["pred"]
        rows.append({"volume": side, "tv_space": tv_space, "tv_time": tv_time, "steps": steps, "lr": lr, "fit_seconds": round(seconds, 2),
                     "loss_first": fit["loss"][0], "loss_last": fit["loss"][-1], "rmse_static": e_s["rmse"], "rmse_dynamic": e_d["rmse"],
                     "rmse_sum": e_sum["rmse"], "dice_vessels": e_d["dice"], "dice_vessels_low": e_low["dice"], "dynamic_max": float(fit["dynamic"].max()), "truth_dynamic_max": float(dynamic.max()), "psnr_held_out": psnr(again, held),
                     "ssim_weight": ssim_weight, "ssim_held_out": float(metrics.ssim(again, held, data_range=held_range).mean())})
        if distances:
            rows[-1].update(distance_columns(fit["dynamic"], dynamic, bounds, ph["segments"], threshold, cldice, keep))
        if "ssim" in fit:
            rows[-1].update({"ssim_train_first": fit["ssim"][0], "ssim_train_last": fit["ssim"][-1]})
        print(json.dumps(rows[-1]), flush=True)
        if centreline is not None:
            own = 0.25 * float(fit["dynamic"].max())
            centreline.append({"volume": side, "input": "fit", "tv_space": tv_space, "tv_time": tv_time, "ssim_weight": ssim_weight, "dice_vessels": e_d["dice"],
                               **centreline_row(fit["dynamic"][0].contiguous(), bounds, ph["segments"][0], own)})
            print(json.dumps(centreline[-1]), flush=True)
        if lumen is not None:
            own = 0.25 * float(fit["dynamic"].max())
            lumen.append({"volume": side, "input": "fit", "tv_space": tv_space, "tv_time": tv_time, "ssim_weight": ssim_weight, "dice_vessels": e_d["dice"], "level": own,
                          **lumen_row(fit["dynamic"].contiguous(), bounds, ph["segments"], own)})
            print(json.dumps(lumen[-1]), flush=True)
        if vesselness:
            V = ccta.vesselness(fit["dynamic"], vesselness)
            for name, x in (("density", fit["dynamic"]), ("vesselness", V)):
                cols = distance_columns(x, dynamic, bounds, ph["segments"], threshold, cldice, keep)
                pairs.append({"volume": side, "tv_space": tv_space, "tv_time": tv_time, "ssim_weight": ssim_weight, "input": name, "sigmas": list(vesselness),
                              "input_max": float(x.max()), "dice_own_quarter": mask_dice(x, dynamic, cols["pred_threshold"], threshold), **cols})
                print(json.dumps(pairs[-1]), flush=True)
    return rows, pairs


def reprojection(dev, sides, n_det, samples):
    """Distance of the frames of the phantom rasterised at each side from those of the phantom rasterised at FINE nodes per axis."""
    from nerfca_amd import drr, phantom, synthetic
    geo = synthetic.xcat_geometry(n_det)
    views = [tuple(float(a) for a in v) for v in synthetic.TRAIN_VIEWS]
    frames = {}
    for side in tuple(sides) + (FINE,):
        ph = phantom.make_phantom((side,) * 3, PHASES, geo, device=dev)
        frames[side] = drr.project_sequence(ph["static"], ph["dynamic"], geo, views, samples, bounds=ph["bounds"])
        del ph
        torch.cuda.empty_cache()
    rows = []
    for side in sides:
        rec = {"volume": side, "against": FINE}
        for k in ("pred", "pred_static", "pred_dynamic"):
            a, b = frames[side][k].double(), frames[FINE][k].double()
            rec[k] = {"max_abs": float((a - b).abs().max()), "rmse": float(torch.sqrt(((a - b) ** 2).mean())), "psnr": psnr(a, b)}
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    return rows


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sides", default="64,128", help="grid sizes, comma separated")
    ap.add_argument("--n-det", type=int, default=128)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--ssim-weight", default="", help="comma separated weights of the structural term: adds rows (default: none)")
    ap.add_argument("--distances", action="store_true", help="add the mask distances and the centreline coverage of the fitted dynamic stack")
    ap.add_argument("--cldice", type=int, default=None, metavar="K", help="with --distances: add the clDice of the fitted dynamic stack at K skeleton iterations")
    ap.add_argument("--components", action="store_true", help="with --distances: add the component count, the largest component's share and the distances of the cleaned mask")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="with --components: the cleaned mask keeps the K largest components (default 1)")
    ap.add_argument("--vesselness", action="store_true", help="with --distances --cldice K --components: add rows for the vesselness of the fitted dynamic stack")
    ap.add_argument("--centreline", action="store_true", help="add rows for the centreline tree (centreline.extract) of the truth and of every fit, at phase 0")
    ap.add_argument("--lumen", action="store_true", help="add rows for the lumen radius (reformat.lumen_profile) of the truth and of every fit along the segment table's chains, all phases")
    ap.add_argument("--vesselness-sigmas", default="1,2,3", help="its scales in nodes, comma separated")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    if args.cldice is not None and not args.distances:
        sys.exit("phantom_study: --cldice is a column of the --distances study")
    if args.components and not args.distances:
        sys.exit("phantom_study: --components adds columns to the --distances study")
    if args.keep_largest is not None and not args.components:
        sys.exit("phantom_study: --keep-largest sets the cleaned mask of the --components columns")
    if args.keep_largest is not None and args.keep_largest < 1:
        sys.exit(f"phantom_study: --keep-largest {args.keep_largest} is not a whole number >= 1")
    if args.vesselness and not (args.distances and args.cldice is not None and args.components):
        sys.exit("phantom_study: --vesselness adds rows to the --distances --cldice K --components study")
    vess_sigmas = tuple(float(s) for s in args.vesselness_sigmas.split(",")) if args.vesselness else None
    keep = (args.keep_largest or 1) if args.components else None
    if not torch.cuda.is_available():
        sys.exit("phantom_study needs the GPU")
    dev = torch.device("cuda:0")
    sides = tuple(int(s) for s in args.sides.split(","))
    ssim_weights = [float(w) for w in args.ssim_weight.split(",") if w.strip()]
    fits, pairs = [], []
    lines = [] if args.centreline else None
    lumen = [] if args.lumen else None
    for side in sides:
        rows, both = study(dev, side, args.n_det, args.samples, args.steps, args.lr, WEIGHTS + ssim_rows(ssim_weights), args.distances, args.cldice, keep, vess_sigmas, lines, lumen)
        fits += rows
        pairs += both
        torch.cuda.empty_cache()
    rep = reprojection(dev, sides, args.n_det, args.samples)
    table = [f"fit_volumes on the phantom, P = {PHASES}, 4 training views of {args.n_det}^2 pixels x {args.samples} samples, {args.steps} Adam steps at lr {args.lr}, from zeros",
             "volume  tv_space  tv_time   loss first -> last        rmse static  rmse dynamic  rmse sum   Dice >rho/4  Dice >rho/20  dynamic max (truth)  PSNR held-out (-5,40)   seconds   ssim_weight  SSIM held-out"
             + ("   assd (cells)  hd95 (cells)  centreline within a cell diagonal" if args.distances else "")
             + (f"   clDice (K = {args.cldice})" if args.cldice is not None else "")
             + (f"   components (truth)  largest share   assd, hd95 of the {keep} largest (cells)" if keep is not None else "")]
    for r in fits:
        table.append(f"{r['volume']:>4}^3  {r['tv_space']:<8g}  {r['tv_time']:<7g}   {r['loss_first']:.3e} -> {r['loss_last']:.3e}   {r['rmse_static']:>10.4f}   {r['rmse_dynamic']:>10.4f}   "
                     f"{r['rmse_sum']:>8.4f}   {r['dice_vessels']:>10.4f}   {r['dice_vessels_low']:>10.4f}   {r['dynamic_max']:>8.3f} ({r['truth_dynamic_max']:.3f})   {r['psnr_held_out']:>12.2f} dB          {r['fit_seconds']:>7.1f}   {r['ssim_weight']:<11g}  {r['ssim_held_out']:.4f}"
                     + (f"         {r['assd_cells']:>7.3f}      {r['hd95_cells']:>7.3f}       {r['centreline_coverage']:.4f}" if args.distances else "")
                     + (f"                      {r['cldice']:.4f}" if args.cldice is not None else "")
                     + (f"      {r['components']:>8.1f} ({r['components_truth']:.1f})      {r['largest_share']:.4f}         {r['assd_cleaned_cells']:>7.3f}  {r['hd95_cleaned_cells']:>7.3f}"
                        if keep is not None else ""))
    if pairs:
        table.append(f"the fitted dynamic stack and its vesselness (sigmas {args.vesselness_sigmas}, Frangi's c), each thresholded at a quarter of its own maximum, against the truth > rho / 4")
        table.append(f"volume  tv_space  tv_time  input        max        Dice     assd (cells)  hd95 (cells)  clDice (K = {args.cldice})  components (truth)  largest share  centreline within a cell diagonal")
        for r in pairs:
            table.append(f"{r['volume']:>4}^3  {r['tv_space']:<8g}  {r['tv_time']:<7g}  {r['input']:<10}  {r['input_max']:>8.4f}   {r['dice_own_quarter']:.4f}      {r['assd_cells']:>7.3f}       {r['hd95_cells']:>7.3f}       "
                         f"{r['cldice']:.4f}         {r['components']:>8.1f} ({r['components_truth']:.1f})       {r['largest_share']:.4f}        {r['centreline_coverage']:.4f}")
    if lines:
        table.append("the centreline tree (centreline.extract, at most 64 paths, root: the mask node nearest the first segment's start) of phase 0 of the truth > rho / 4 and of every "
                     "fit > a quarter of its own maximum, against the segment table: points within a cell diagonal, both ways")
        table.append("volume  input  tv_space  tv_time  Dice >rho/4  branches (truth)  found near truth  truth near found  radius error (cells)  length    reached  root gap (cells)  seconds")
        for r in lines:
            if r.get("empty_mask"):
                table.append(f"{r['volume']:>4}^3  {r['input']:<5}  empty mask")
                continue
            table.append(f"{r['volume']:>4}^3  {r['input']:<5}  {r.get('tv_space', 0.0):<8g}  {r.get('tv_time', 0.0):<7g}  {r.get('dice_vessels', 1.0):>10.4f}   {r['branches']:>6} ({r['branches_truth']})"
                         f"        {r['found_within_diagonal_of_truth']:.4f}            {r['truth_within_diagonal_of_found']:.4f}            {r['radius_error_mean_cells']:>8.3f}         "
                         f"{r['total_length']:>8.3f}  {r['reached']:.4f}   {r['root_gap_cells']:>8.3f}        {r['extract_seconds']:>8.3f}")
    if lumen:
        table.append("the lumen radius d_eq / 2 (reformat.lumen_profile, 64 rays, planes every half node spacing along every chain of the segment table, all phases) of the truth at rho / 4 "
                     "and of every fit at a quarter of its own maximum, against the table's radius at the plane; planes with a status bit set are left out")
        table.append("volume  input  tv_space  tv_time  Dice >rho/4  level      planes  status 0 share  |radius error| (cells)  signed (cells)  seconds")
        for r in lumen:
            table.append(f"{r['volume']:>4}^3  {r['input']:<5}  {r.get('tv_space', 0.0):<8g}  {r.get('tv_time', 0.0):<7g}  {r.get('dice_vessels', 1.0):>10.4f}   {r['level']:<9.4g}  {r['lumen_planes']:>6}  "
                         f"{r['lumen_status0_share']:>12.4f}   {r['lumen_radius_mae_cells']:>20.3f}   {r['lumen_radius_bias_cells']:>12.3f}   {r['lumen_seconds']:>8.3f}")
    table.append(f"reprojection distance: the frames of the phantom rasterised at n^3 against those of the phantom at {FINE}^3 (4 views x {PHASES} phases)")
    for r in rep:
        table.append(f"{r['volume']:>4}^3   " + "   ".join(f"{k}: max {r[k]['max_abs']:.4e} rmse {r[k]['rmse']:.4e} PSNR {r[k]['psnr']:.2f} dB" for k in ("pred", "pred_static", "pred_dynamic")))
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in fits + pairs + (lines or []) + (lumen or []) + rep:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
