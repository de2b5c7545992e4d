#!/usr/bin/env python3
"""Time of a gradient step through drr.project_rays against the loop a user of the package writes without it, in ONE process:

    ours       per view: drr.project_rays of the static volume and of the P-volume stack (both requires_grad), the scalar
               sum(pix_s y_s) + sum(pix_d y_d), .backward(): nca_drr_project forward, nca_drr_backproject backward.  Timed with both
               structures of the backward kernel: one atomic per contribution (direct) and runs of samples in one cell summed in registers
               first (runs)
    forward    the same projections under no_grad: what the forward costs on its own
    loop       o + d z in torch, one torch.nn.functional.grid_sample per volume (static and each phase) with requires_grad volumes,
               (sigma * dists).sum(-1), the same scalar, .backward(): all in f32

at 256 x 256 pixels x 192 samples, V = 4 views, volumes of 128^3 and 256^3 with bounds +-1, P in {1, 10} phases.  Every leg is one warm-up
pass and then three timed passes; the legs alternate.  A timed pass is INNER = 20 sequences (all V views, forward and backward) back to back
ending in one device synchronise, and the report is seconds per sequence: best and worst pass, and loop / ours.  Backward time is ours minus
forward (it includes zeroing the f64 buffer and the cast to f32); added bytes per second is 8 neighbours x 8 bytes x n_vol x R x S per view
over that time, an upper count since skipped samples add nothing.  The tool stops if the gradients of the legs differ by more than 1e-4 of
max |grad| (the loop sums in f32 atomics: a few hundred adds per node at 2^-24 each give a few 1e-5 at worst).

    python3 tools/drr_grad_bench.py [--out profiles/drr_grad_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from view_render_bench import VIEWS, timed  # noqa: E402

PHASE_COUNTS = (1, 10)
VOLUME_SIDES = (128, 256)
REPEATS = 3
INNER = 20
BOUNDS = ((-1.0, 1.0),) * 3
AGREE = 1e-4


def set_runs(k):
    from nerfca_amd import _capi
    _capi.check_drr(_capi.lib().nca_drr_set_backproject_runs(k))


def measure(dev, default_runs, n_det, samples, side, n_phases, inner):
    from nerfca_amd import drr, export, synthetic
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    geo = synthetic.xcat_geometry(n_det)
    R = n_det * n_det
    gen = torch.Generator(device=dev).manual_seed(side + n_phases)
    vs = (torch.rand((side,) * 3, generator=gen, device=dev) * 0.02).requires_grad_()
    vd = (torch.rand((n_phases,) + (side,) * 3, generator=gen, device=dev) * 0.02).requires_grad_()
    y_s = torch.randn((len(VIEWS), R), generator=gen, device=dev, dtype=torch.float64)
    y_d = torch.randn((len(VIEWS), n_phases, R), generator=gen, device=dev, dtype=torch.float64)
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], samples, dev).to(torch.float32)
    dists64 = _interval_lengths(z, torch.empty(0, dtype=torch.float64, device=dev)).to(torch.float64)
    dists32 = _interval_lengths(z, z)
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))
    rays64 = [export.view_rays(geo, theta, phi, device=dev) for theta, phi in VIEWS]
    rays32 = [export.view_rays(geo, theta, phi, device=dev, dtype=torch.float32) for theta, phi in VIEWS]
    lo = torch.tensor([b[0] for b in BOUNDS], dtype=torch.float32, device=dev)
    hi = torch.tensor([b[1] for b in BOUNDS], dtype=torch.float32, device=dev)
    y_s32, y_d32 = y_s.float(), y_d.float()

    def ours(k):
        set_runs(k)
        try:
            vs.grad = vd.grad = None
            for v, (o, d) in enumerate(rays64):
                pix_s = drr.project_rays(vs, o, d, z, dists64, i0=i0, bounds=BOUNDS)
                pix_d = drr.project_rays(vd, o, d, z, dists64, i0=i0, bounds=BOUNDS)
                ((pix_s * y_s[v]).sum() + (pix_d * y_d[v]).sum()).backward()
            return vs.grad, vd.grad
        finally:
            set_runs(default_runs)

    @torch.no_grad()
    def forward():
        for o, d in rays64:
            drr.project_rays(vs, o, d, z, dists64, i0=i0, bounds=BOUNDS)
            drr.project_rays(vd, o, d, z, dists64, i0=i0, bounds=BOUNDS)

    def loop():
        vs.grad = vd.grad = None

        def sample(vol, grid):
            sig = torch.nn.functional.grid_sample(vol[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
            return i0 - (sig * dists32).sum(-1)

        for v, (o, d) in enumerate(rays32):
            pts = o[:, None, :] + d[:, None, :] * z[None, :, None]
            grid = (((pts - lo) / (hi - lo)) * 2 - 1).flip(-1)[None, None]          # x addresses the last volume axis
            total = (sample(vs, grid) * y_s32[v]).sum()
            for j in range(n_phases):
                total = total + (sample(vd[j], grid) * y_d32[v, j]).sum()
            total.backward()
        return vs.grad, vd.grad

    legs = {"ours_direct": lambda: ours(0), "ours_runs": lambda: ours(1), "forward": forward, "loop": loop}
    want = [g.clone() for g in legs["loop"]()]          # warm-up, and the agreement check
    errs = {}
    for name in ("ours_direct", "ours_runs"):
        got = legs[name]()
        errs[name] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want))
        if not errs[name] <= AGREE:
            sys.exit(f"drr_grad_bench: the legs do not make the same gradients ({side}^3, P = {n_phases}, {name}: difference {errs[name]:.3e} of max |grad|)")
    legs["forward"]()
    times = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, fn in legs.items():                              # alternate the legs
            times[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
    rec = {"pixels": R, "samples": samples, "views": len(VIEWS), "volume": side, "phases": n_phases, "sequences_per_pass": inner, "grad_diff_of_max": errs}
    for k in legs:
        rec[k] = {"best_s": round(min(times[k]), 5), "worst_s": round(max(times[k]), 5)}
    added = 8 * 8 * (1 + n_phases) * R * samples * len(VIEWS)          # bytes a sequence's backward adds, counted from above
    for k in ("ours_direct", "ours_runs"):
        rec["loop_over_" + k + "_best"] = round(rec["loop"]["best_s"] / rec[k]["best_s"], 3)
        back = rec[k]["best_s"] - rec["forward"]["best_s"]
        rec["backward_over_forward_" + k] = round(back / rec["forward"]["best_s"], 2)
        rec["added_gbytes_per_s_" + k] = round(added / back / 1e9, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n-det", type=int, default=256)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--inner", type=int, default=INNER, help="sequences per timed pass")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("drr_grad_bench needs the GPU: there is nothing to time without one")
    from nerfca_amd import _capi
    dev = torch.device("cuda:0")
    default_runs = _capi.lib().nca_drr_get_backproject_runs()
    lines = []
    for side in VOLUME_SIDES:
        for n_phases in PHASE_COUNTS:
            rec = measure(dev, default_runs, args.n_det, args.samples, side, n_phases, args.inner)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    names = {0: "direct", 1: "runs"}
    table = [f"library default: {names[default_runs]}; milliseconds per sequence of V views (forward + backward of the static volume and the P-volume stack), "
             "best / worst pass",
             "volume  V x P     direct ms            runs ms              forward only ms      loop ms              loop/direct  loop/runs"]
    for r in lines:
        cells = "".join(f"   {1e3 * r[k]['best_s']:>8.3f} / {1e3 * r[k]['worst_s']:<8.3f}" for k in ("ours_direct", "ours_runs", "forward", "loop"))
        table.append(f"{r['volume']:>4}^3  {r['views']} x {r['phases']:<3}{cells}    {r['loop_over_ours_direct_best']:>6.2f}       {r['loop_over_ours_runs_best']:>6.2f}")
    table.append("backward / forward time, and GB/s of added bytes (8 x 8 x n_vol x R x S per view over backward time; backward = ours - forward only, best passes)")
    for r in lines:
        table.append(f"{r['volume']:>4}^3  {r['views']} x {r['phases']:<3}   direct {r['backward_over_forward_ours_direct']:>7.2f}x  {r['added_gbytes_per_s_ours_direct']:>8.1f} GB/s"
                     f"      runs {r['backward_over_forward_ours_runs']:>7.2f}x  {r['added_gbytes_per_s_ours_runs']:>8.1f} GB/s"
                     f"      gradient difference from loop, of max |grad|: {r['grad_diff_of_max']['ours_direct']:.2e} / {r['grad_diff_of_max']['ours_runs']:.2e}")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
