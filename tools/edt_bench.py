#!/usr/bin/env python3
"""Time of an exact Euclidean distance transform of a vessel mask against the two things a user writes without one, in ONE process:

    ours    metrics.distance_transform(dynamic, bounds, threshold=rho / 4): nca_vol_edt, three launches, on the device
    scipy   scipy.ndimage.distance_transform_edt(~mask, sampling=h) per volume on the host, INCLUDING the copy of the stack to the host and
            of the f32 maps back to the device
    cdist   torch.cdist(nodes, mask nodes).min(dim=1) per volume on the device in f64, the nodes in chunks that keep the distance matrix
            below 1 GiB (torch's default compute mode: the matrix-product form, which is close but not exact)

on the coronary tree of phantom.make_phantom (dynamic > rho / 4) at 128^3 and 256^3 nodes, P = 1 and 10 heart phases.  Every leg is one
warm-up pass and then three timed passes; the legs alternate.  A pass ends in one device synchronise; the report is milliseconds per pass,
best and worst, and scipy / ours and cdist / ours.  The share of the three kernels in one call of ours is read from the torch profiler's
device-side kernel records.  The tool stops if ours differs from scipy by more than one f32 step anywhere, or from cdist by more than a
thousandth of a node spacing.

    python3 tools/edt_bench.py [--out profiles/edt_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIDES = (128, 256)
PHASES = (1, 10)
CDIST_BYTES = 1 << 30


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default=",".join(str(s) for s in SIDES), help="nodes per axis, comma separated")
    ap.add_argument("--phases", default=",".join(str(p) for p in PHASES), help="heart phases, comma separated")
    return ap


def kernel_shares(fn):
    """{kernel name: microseconds} of the edt kernels in one call of `fn`, from the profiler's device records; {} when it has none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if "edt_" in ev.key:
                name = "row" if "row" in ev.key else ("axis1" if "ILb1" in ev.key or "<true>" in ev.key else "axis0")
                out[name] = out.get(name, 0.0) + float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
        return out
    except Exception as e:          # the profiler is a convenience here: the timings above do not depend on it
        return {"error": repr(e)}


def measure(dev, side, n_phase, passes):
    import numpy as np
    import scipy.ndimage
    import torch
    from nerfca_amd import metrics, phantom, synthetic
    from view_render_bench import timed
    geo = synthetic.xcat_geometry(128)
    ph = phantom.make_phantom((side,) * 3, n_phase, geo, device=dev)
    vol, bounds = ph["dynamic"], ph["bounds"]
    thr = 0.25 * phantom.RHO_VESSEL
    h = [(b[1] - b[0]) / (side - 1) for b in bounds]
    axes = [torch.arange(side, device=dev, dtype=torch.float64) * h[a] for a in range(3)]

    def ours():
        return metrics.distance_transform(vol, bounds, threshold=thr)

    def by_scipy():
        mask = vol.cpu().numpy() > thr
        out = np.stack([scipy.ndimage.distance_transform_edt(~m, sampling=h).astype(np.float32) for m in mask])
        return torch.from_numpy(out).to(dev)

    def by_cdist():
        nodes = torch.cartesian_prod(*axes)
        out = torch.empty((n_phase, side ** 3), dtype=torch.float32, device=dev)
        for p in range(n_phase):
            feat = nodes[(vol[p] > thr).reshape(-1)]
            chunk = max(1, CDIST_BYTES // (8 * max(1, feat.shape[0])))
            for s in range(0, nodes.shape[0], chunk):
                out[p, s:s + chunk] = torch.cdist(nodes[s:s + chunk], feat).min(dim=1).values.float()
        return out.reshape(vol.shape)

    legs = {"ours": ours, "scipy": by_scipy, "cdist": by_cdist}
    res = {k: fn() for k, fn in legs.items()}          # the warm-up pass, and the agreement check
    got, sci = res["ours"].cpu().numpy(), res["scipy"].cpu().numpy()
    steps = int(np.abs(got.view(np.int32).astype(np.int64) - sci.view(np.int32).astype(np.int64)).max())
    if steps > 1:
        sys.exit(f"edt_bench: ours differs from scipy by {steps} f32 steps at {side}^3, P = {n_phase}")
    rel = float((res["ours"].double() - res["cdist"].double()).abs().max()) / min(h)
    if rel > 1e-3:
        sys.exit(f"edt_bench: ours differs from cdist by {rel:.3e} node spacings at {side}^3, P = {n_phase}")
    n_mask = int((vol > thr).sum())
    far = float(res["ours"].max()) / max(h)
    del res
    times = {k: [] for k in legs}
    for i in range(passes):
        for k, fn in legs.items():          # alternate the legs
            times[k].append(timed(fn))
            print(f"  {side}^3 P={n_phase} pass {i} {k}: {1e3 * times[k][-1]:.2f} ms", flush=True)
    rec = {"side": side, "phases": n_phase, "mask_nodes": n_mask, "largest_distance_cells": round(far, 1), "f32_steps_from_scipy": steps,
           "cells_from_cdist": rel}
    for k in legs:
        rec[k] = {"best_ms": round(1e3 * min(times[k]), 3), "worst_ms": round(1e3 * max(times[k]), 3)}
    rec["scipy_over_ours_best"] = round(rec["scipy"]["best_ms"] / rec["ours"]["best_ms"], 1)
    rec["cdist_over_ours_best"] = round(rec["cdist"]["best_ms"] / rec["ours"]["best_ms"], 1)
    rec["kernel_us"] = kernel_shares(ours)
    nodes = n_phase * side ** 3
    # algorithmic bytes of the three launches: f32 in + int32 out; int32 in + f64 out; f64 in + f32 out = 32 per node
    rec["ours_gbytes_per_s"] = round(32 * nodes / (rec["ours"]["best_ms"] * 1e-3) / 1e9, 1)
    return rec


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("edt_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in (int(s) for s in args.sides.split(",")):
        for n_phase in (int(p) for p in args.phases.split(",")):
            rec = measure(dev, side, n_phase, args.passes)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    table = ["milliseconds per distance transform of the phantom's vessel mask (dynamic > rho / 4), best / worst pass",
             "side   P   mask nodes   ours ms                  scipy (host, with copies) ms     cdist f64 (device) ms          scipy/ours  cdist/ours   ours GB/s   row / axis 1 / axis 0 share"]
    for r in lines:
        cells = "".join(f"   {r[k]['best_ms']:>10.3f} / {r[k]['worst_ms']:<10.3f}" for k in ("ours", "scipy", "cdist"))
        ku = r["kernel_us"]
        total = sum(v for v in ku.values() if isinstance(v, float)) if "error" not in ku else 0.0
        share = " / ".join(f"{100 * ku.get(k, 0.0) / total:.0f}%" for k in ("row", "axis1", "axis0")) if total > 0 else "not recorded"
        table.append(f"{r['side']:>4}  {r['phases']:>2}   {r['mask_nodes']:>10}{cells}   {r['scipy_over_ours_best']:>9.1f}  {r['cdist_over_ours_best']:>9.1f}   {r['ours_gbytes_per_s']:>9.1f}   {share}")
    slower = [f"{r['side']}^3 P={r['phases']} ({k})" for r in lines for k in ("scipy", "cdist") if r["ours"]["best_ms"] > r[k]["best_ms"]]
    table.append("rows in which ours is slower than a competitor: " + (", ".join(slower) if slower else "none"))
    table.append("agreement: at most " + str(max(r["f32_steps_from_scipy"] for r in lines)) + " f32 step(s) from scipy, "
                 + f"{max(r['cells_from_cdist'] for r in lines):.2e} node spacings from cdist; largest distance "
                 + ", ".join(f"{r['largest_distance_cells']} cells at {r['side']}^3 P={r['phases']}" for r in lines))
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
