#!/usr/bin/env python3
"""Time of export.render_sequence against the loop a user of the package writes without it, in ONE process:

    sequence   export.render_sequence: rays generated on the device per chunk, the static field rendered once per view, the dynamic
               field once per (view, phase), nca_view_compose per frame
    loop       per view the host geometry (proj_helpers.get_ray_values_tigre) and an upload of the [W*H,3] rays as f64 (the ray table's
               type, so both legs run the render kernels in the same ray mode), then per (view, phase) one composite fused.render_rays:
               the composite image alone
    loop3      loop, plus the static / dynamic images from its sigmas as CompositeTrainer.evaluate forms them (f64 [R,S] torch
               reductions): the same three image stacks as sequence

at 256 x 256 pixels x 192 samples, V = 4 views, P in {1, 2, 10} phases, synthetic.net_definitions' default nets, f32 and bf16.  Every leg
is one warm-up pass and then whole passes ending in a device synchronise; the legs alternate and each runs three times.  Reports best and
worst seconds per pass and the ratios loop / sequence (the comparator: sequence delivers two more image stacks in that time) and
loop3 / sequence (equal output).

    python3 tools/view_render_bench.py [--out profiles/view_render_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

VIEWS = [(-5.0, 40.0), (60.0, -30.0), (-30.0, 30.0), (90.0, 0.0)]
PHASE_COUNTS = (1, 2, 10)
REPEATS = 3


def make_models(dev, prec):
    from nerfca_amd import set_precision, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    torch.manual_seed(1)
    sd, td = synthetic.net_definitions(dev)
    s, t = CPPN(sd).to(dev), Temporal(td).to(dev)
    for m in (s, t):
        m.update_freq_mask_alpha(75000, 150000)
    set_precision(prec, s, t)
    return s, t


@torch.no_grad()
def user_loop(s, t, geo, views, phases, samples, three_images, chunk_rays=65536):
    """What rendering a sequence takes without export.render_sequence."""
    from nerfca_amd import render_rays
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    from nerfca_amd.train.proj_helpers import get_ray_values_tigre
    dev = next(s.parameters()).device
    W, H = geo["nDetector"]
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], samples, dev)
    pred = torch.empty((len(views), len(phases), W * H), dtype=torch.float32, device=dev)
    pred_d = torch.empty_like(pred)
    pred_s = torch.empty((len(views), W * H), dtype=torch.float32, device=dev)
    for v, (theta, phi) in enumerate(views):
        o, d = get_ray_values_tigre(theta, phi, 0, geo, "cpu")
        o = torch.as_tensor(o, dtype=torch.float32).reshape(-1, 3).double().to(dev)
        d = torch.as_tensor(d, dtype=torch.float32).reshape(-1, 3).double().to(dev)
        dists = _interval_lengths(z, d)
        for j, phase in enumerate(phases):
            for i in range(0, W * H, chunk_rays):
                oc, dc = o[i:i + chunk_rays], d[i:i + chunk_rays]
                ph = torch.full((oc.shape[0],), phase, dtype=torch.int32, device=dev)
                I0 = torch.full((oc.shape[0],), geo["max_pixel_value"], dtype=torch.float32, device=dev)
                pix, sig_s, sig_d = render_rays(s, t, oc, dc, ph, I0, z, dists)
                pred[v, j, i:i + chunk_rays] = pix.float()
                if not three_images:
                    continue
                pred_s[v, i:i + chunk_rays] = (geo["max_pixel_value"] - (sig_s.double() * dists).sum(-1)).float()
                pred_d[v, j, i:i + chunk_rays] = (geo["max_pixel_value"] - (sig_d.double() * dists).sum(-1)).float()
    return pred, pred_s, pred_d


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(dev, prec, n_det, samples, n_phases):
    from nerfca_amd import export, synthetic
    s, t = make_models(dev, prec)
    geo = synthetic.xcat_geometry(n_det)
    phases = list(range(n_phases))
    legs = {"sequence": lambda: export.render_sequence(s, t, geo, VIEWS, phases, samples),
            "loop": lambda: user_loop(s, t, geo, VIEWS, phases, samples, False),
            "loop3": lambda: user_loop(s, t, geo, VIEWS, phases, samples, True)}
    a, _, b = legs["sequence"](), legs["loop"](), legs["loop3"]()          # warm-up; sequence and loop3 render the same images
    err = float((a["pred"].reshape(b[0].shape) - b[0]).abs().max() / b[0].abs().max())
    if not err <= (1e-4 if prec == "f32" else 5e-3):            # loose: the test suite holds the tight bounds
        sys.exit(f"view_render_bench: the legs do not render the same images ({prec}, P = {n_phases}: relative difference {err:.3e})")
    times = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, fn in legs.items():                              # alternate the legs
            times[k].append(timed(fn))
    rec = {"prec": prec, "pixels": n_det * n_det, "samples": samples, "views": len(VIEWS), "phases": n_phases, "pred_rel_diff": err}
    for k in legs:
        rec[k] = {"best_s": round(min(times[k]), 5), "worst_s": round(max(times[k]), 5)}
    rec["loop_over_sequence_best"] = round(rec["loop"]["best_s"] / rec["sequence"]["best_s"], 3)
    rec["loop3_over_sequence_best"] = round(rec["loop3"]["best_s"] / rec["sequence"]["best_s"], 3)
    rec["pass_count_prediction"] = round(2 * n_phases / (n_phases + 1), 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n-det", type=int, default=256)
    ap.add_argument("--samples", type=int, default=192)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("view_render_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for prec in ("f32", "bf16"):
        for n_phases in PHASE_COUNTS:
            rec = measure(dev, prec, args.n_det, args.samples, n_phases)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    table = ["prec   V x P    sequence best/worst s    loop best/worst s     loop3 best/worst s   loop/sequence  loop3/sequence  2P/(P+1)"]
    for r in lines:
        table.append(f"{r['prec']:<5}  {r['views']} x {r['phases']:<3}   {r['sequence']['best_s']:>8.4f} / {r['sequence']['worst_s']:<8.4f}"
                     f"    {r['loop']['best_s']:>8.4f} / {r['loop']['worst_s']:<8.4f}    {r['loop3']['best_s']:>8.4f} / {r['loop3']['worst_s']:<8.4f}"
                     f"    {r['loop_over_sequence_best']:>6.2f}         {r['loop3_over_sequence_best']:>6.2f}        {r['pass_count_prediction']:>5.2f}")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
