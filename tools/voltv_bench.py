#!/usr/bin/env python3
"""Time of the total-variation priors (drr.total_variation: nca_vol_tv forward, nca_vol_tv_grad backward) against the torch expression of
the same functional under autograd, in ONE process:

    ours       tv_space, tv_time = drr.total_variation(x, cyclic=True) of a requires_grad stack [P,n,n,n]; (tv_space + tv_time).backward()
    loop_f32   forward differences by slicing, pad, sqrt(eps^2 + ...) - eps, mean; the phase differences with torch.roll; the same sum,
               .backward() -- in f32, what a user of torch writes
    loop_f64   the same expression on x.double(): for information (the precision our kernels compute in)

for volumes of 128^3 and 256^3 with bounds +-1 and P in {1, 10} phases.  Every leg is one warm-up pass and then three timed passes; the legs
alternate.  A timed pass is INNER forward + backward pairs back to back ending in one device synchronise; the report is seconds per pair:
best and worst pass, and loop / ours.  The tool stops if the gradients of ours and loop_f32 differ by more than 1e-4 of max |grad|.

The two kernels are also timed on their own (device events around INNER direct launches, best of three) and reported as GB/s of
algorithmic bytes: 4 read per voxel for nca_vol_tv, 4 read + 4 written for nca_vol_tv_grad.

Last, one step of drr.fit_volumes at 128^3, P = 10, 4 views of 256 x 256 pixels x 192 samples, with the priors off and on: the difference
of a 13-step and a 3-step call over 10, so that the set-up cancels.

    python3 tools/voltv_bench.py [--out profiles/voltv_bench.txt]
"""
import argparse
import ctypes as C
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
INNER = 10
BOUNDS = ((-1.0, 1.0),) * 3
EPS = 1e-3
AGREE = 1e-4


def torch_total_variation(x, inv, eps):
    """(tv_space, tv_time) of a stack [P,n0,n1,n2] in its dtype, as means, cyclic in the phase."""
    pad = torch.nn.functional.pad
    d0 = pad((x[:, 1:] - x[:, :-1]) * inv[0], (0, 0, 0, 0, 0, 1))
    d1 = pad((x[:, :, 1:] - x[:, :, :-1]) * inv[1], (0, 0, 0, 1))
    d2 = pad((x[:, :, :, 1:] - x[:, :, :, :-1]) * inv[2], (0, 1))
    space = (torch.sqrt(eps * eps + ((d0 * d0 + d1 * d1) + d2 * d2)) - eps).mean()
    if x.shape[0] == 1:
        return space, torch.zeros((), dtype=x.dtype, device=x.device)
    t = torch.roll(x, -1, 0) - x
    return space, (torch.sqrt(eps * eps + t * t) - eps).mean()


def kernel_times(x, inner):
    """Milliseconds of one nca_vol_tv and one nca_vol_tv_grad launch: device events around `inner` launches, best of REPEATS."""
    from nerfca_amd import _capi, drr, fused
    desc = drr.grid_desc(x.shape[-3:], BOUNDS)
    out = torch.zeros(2, dtype=torch.float64, device=x.device)
    scale = torch.tensor([1.0, 1.0], dtype=torch.float64, device=x.device)
    g = torch.empty_like(x)
    lib, st = _capi.lib(), fused._stream()
    launches = {"nca_vol_tv": lambda: _capi.check_vol(lib.nca_vol_tv(C.byref(desc), _capi.ptr(x), x.shape[0], EPS, EPS, 1, _capi.ptr(out), st)),
                "nca_vol_tv_grad": lambda: _capi.check_vol(lib.nca_vol_tv_grad(C.byref(desc), _capi.ptr(x), x.shape[0], EPS, EPS, 1, _capi.ptr(scale), _capi.ptr(g), st))}
    best = {}
    for name, fn in launches.items():
        fn()
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            best[name] = min(best.get(name, float("inf")), a.elapsed_time(b) / inner)
    return best


def measure(dev, side, n_phases, inner):
    from nerfca_amd import drr
    gen = torch.Generator(device=dev).manual_seed(side + n_phases)
    x = (torch.rand((n_phases,) + (side,) * 3, generator=gen, device=dev) * 0.02).requires_grad_()
    inv = [(side - 1) / (b[1] - b[0]) for b in BOUNDS]

    def ours():
        x.grad = None
        tv_s, tv_t = drr.total_variation(x, bounds=BOUNDS, eps_space=EPS, eps_time=EPS, cyclic=True)
        (tv_s + tv_t).backward()
        return x.grad

    def loop(dtype):
        x.grad = None
        tv_s, tv_t = torch_total_variation(x.to(dtype), inv, EPS)
        (tv_s + tv_t).backward()
        return x.grad

    legs = {"ours": ours, "loop_f32": lambda: loop(torch.float32), "loop_f64": lambda: loop(torch.float64)}
    want = legs["loop_f32"]().clone()          # warm-up, and the agreement check
    got = legs["ours"]()
    err = float((got - want).abs().max() / want.abs().max())
    if not err <= AGREE:
        sys.exit(f"voltv_bench: the legs do not make the same gradients ({side}^3, P = {n_phases}: difference {err:.3e} of max |grad|)")
    err64 = float((got - legs["loop_f64"]()).abs().max() / want.abs().max())
    del want, got
    times = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, fn in legs.items():                              # alternate the legs
            times[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
    x.grad = None
    rec = {"volume": side, "phases": n_phases, "pairs_per_pass": inner, "grad_diff_of_max_vs_f32": err, "grad_diff_of_max_vs_f64": err64}
    for k in legs:
        rec[k] = {"best_s": round(min(times[k]), 6), "worst_s": round(max(times[k]), 6)}
    for k in ("loop_f32", "loop_f64"):
        rec[k + "_over_ours_best"] = round(rec[k]["best_s"] / rec["ours"]["best_s"], 2)
        rec[k + "_worst_over_ours_worst"] = round(rec[k]["worst_s"] / rec["ours"]["worst_s"], 2)
    voxels = n_phases * side ** 3
    with torch.no_grad():
        ms = kernel_times(x.detach(), inner)
    rec["kernel_ms"] = {k: round(v, 4) for k, v in ms.items()}
    rec["kernel_gbytes_per_s"] = {"nca_vol_tv": round(4 * voxels / ms["nca_vol_tv"] / 1e6, 1), "nca_vol_tv_grad": round(8 * voxels / ms["nca_vol_tv_grad"] / 1e6, 1)}
    return rec


def fit_step(dev, side=128, n_phases=10, n_det=256, samples=192):
    """Seconds of one fit_volumes step with the priors off and on."""
    from nerfca_amd import drr, synthetic
    geo = synthetic.xcat_geometry(n_det)
    gen = torch.Generator(device=dev).manual_seed(7)
    frames = [(theta, phi, p, torch.rand((n_det, n_det), generator=gen, device=dev)) for theta, phi in VIEWS for p in range(n_phases)]
    rec = {"volume": side, "phases": n_phases, "views": len(VIEWS), "pixels": n_det * n_det, "samples": samples}
    for name, w in (("priors_off", 0.0), ("priors_on", 1e-3)):
        run = lambda steps: drr.fit_volumes(frames, geo, (side,) * 3, samples, bounds=BOUNDS, n_phases=n_phases, steps=steps, tv_space=w, tv_time=w)
        run(1)
        passes = []
        for _ in range(REPEATS):
            short, long = timed(lambda: run(3)), timed(lambda: run(13))
            passes.append((long - short) / 10)
        rec[name] = {"best_s": round(min(passes), 5), "worst_s": round(max(passes), 5)}
    rec["priors_add_fraction_best"] = round(rec["priors_on"]["best_s"] / rec["priors_off"]["best_s"] - 1, 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--inner", type=int, default=INNER, help="forward + backward pairs per timed pass")
    ap.add_argument("--no-fit", action="store_true", help="leave out the fit_volumes step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("voltv_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in VOLUME_SIDES:
        for n_phases in PHASE_COUNTS:
            rec = measure(dev, side, n_phases, args.inner)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    table = ["milliseconds per forward + backward of both total variations of a [P,n,n,n] stack, best / worst pass",
             "volume  P     ours ms              loop f32 ms          loop f64 ms          f32/ours  f64/ours   (worst/worst: f32, f64)"]
    for r in lines:
        cells = "".join(f"   {1e3 * r[k]['best_s']:>8.3f} / {1e3 * r[k]['worst_s']:<8.3f}" for k in ("ours", "loop_f32", "loop_f64"))
        table.append(f"{r['volume']:>4}^3  {r['phases']:<3}{cells}   {r['loop_f32_over_ours_best']:>7.2f}   {r['loop_f64_over_ours_best']:>7.2f}      "
                     f"{r['loop_f32_worst_over_ours_worst']:>6.2f}, {r['loop_f64_worst_over_ours_worst']:<6.2f}")
    table.append("the kernels alone: milliseconds per launch and GB/s of algorithmic bytes (4 per voxel read; 4 read + 4 written); gradient difference of max |grad|")
    for r in lines:
        table.append(f"{r['volume']:>4}^3  {r['phases']:<3}   nca_vol_tv {r['kernel_ms']['nca_vol_tv']:>8.4f} ms {r['kernel_gbytes_per_s']['nca_vol_tv']:>8.1f} GB/s"
                     f"      nca_vol_tv_grad {r['kernel_ms']['nca_vol_tv_grad']:>8.4f} ms {r['kernel_gbytes_per_s']['nca_vol_tv_grad']:>8.1f} GB/s"
                     f"      vs f32 {r['grad_diff_of_max_vs_f32']:.2e}, vs f64 {r['grad_diff_of_max_vs_f64']:.2e}")
    fit = None
    if not args.no_fit:
        fit = fit_step(dev)
        print(json.dumps(fit), flush=True)
        table.append(f"one fit_volumes step, {fit['volume']}^3, P = {fit['phases']}, {fit['views']} views of {fit['pixels']} pixels x {fit['samples']} samples, best / worst: "
                     f"priors off {1e3 * fit['priors_off']['best_s']:.2f} / {1e3 * fit['priors_off']['worst_s']:.2f} ms, "
                     f"on {1e3 * fit['priors_on']['best_s']:.2f} / {1e3 * fit['priors_on']['worst_s']:.2f} ms ({100 * fit['priors_add_fraction_best']:+.2f} % of the best)")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines + ([fit] if fit else []):
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
