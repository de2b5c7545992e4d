#!/usr/bin/env python3
"""Time of the two filters of nerfca_amd.ccta against what a user writes without them, in ONE process:

    smooth r2 / r16   ccta.gaussian_filter(vol, 1, radius=2) and (vol, 4, radius=16): nca_vol_smooth, three launches, on the device
        scipy         scipy.ndimage.gaussian_filter(v.astype(f64), sigma, radius=r).astype(f32) per volume on the host, INCLUDING the copy of the
                      stack to the host and of the result back to the device (the f64 call is the one whose bits ours has)
        conv3d        three torch conv3d calls in f64 on the device, one per axis, on a replicate-padded stack (torch has no scipy-`reflect`
                      padding for volumes: the results agree r nodes away from the faces, which is what the tool checks)
    dilate 3          ccta.binary_dilation(mask, 3): nca_vol_cityblock and a comparison, on the device
        scipy         scipy.ndimage.binary_dilation(m, iterations=3) per volume on the host, with both copies
        pool          three steps on the device, each the maximum of three 1-D max_pool3d calls (3x1x1, 1x3x1, 1x1x3: the 6-connected
                      structure; one 3x3x3 pool would be the 26-connected one)

on the vessel volume of phantom.make_phantom at 128^3 and 256^3 nodes, 1 and 10 volumes.  Every leg is one warm-up pass and then
`--passes` timed passes; the legs alternate.  A device leg repeats its call inside a pass until the pass lasts about 0.2 s; a pass ends in
one device synchronise; the report is milliseconds per call, best and worst pass.  Algorithmic bytes: the filter reads and writes 40 per
node (f32 in, f64 out; f64, f64; f64 in, f32 out), the distance transform 24 (three launches of 4 in, 4 out); the GB/s columns are those
bytes over the best time of the WHOLE call (launches, workspace allocation and, for the dilation, the comparison included), so they are a
lower bound on what the kernels reach.  The tool stops if ours differs from scipy in one bit, or from the device baselines where they are
comparable.  A baseline that torch cannot run on this device is reported as "failed", never replaced.

    python3 tools/filt_bench.py [--out profiles/filt_bench.txt]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SMOOTH = (("smooth_r2", 1.0, 2), ("smooth_r16", 4.0, 16))
WINDOW = 0.2          # seconds a timed pass of a device leg should last


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default="128,256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1,10", help="volumes per stack, comma separated")
    return ap


def run_legs(legs, passes, host_legs, tag):
    """{leg: {"best_ms", "worst_ms", "reps"} or {"failed": text}} and the warm-up results of the legs that ran."""
    import torch
    from view_render_bench import timed
    res, reps, failed = {}, {}, {}
    for k, fn in legs.items():          # the warm-up pass
        try:
            res[k] = fn()
            torch.cuda.synchronize()
        except Exception as e:          # a baseline torch cannot run here; ours is never caught
            if k == "ours":
                raise
            failed[k] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
    for k, fn in legs.items():
        if k not in failed:
            reps[k] = 1 if k in host_legs else max(1, min(500, math.ceil(WINDOW / max(timed(fn), 1e-6))))
    times = {k: [] for k in reps}
    for i in range(passes):
        for k, n in reps.items():          # alternate the legs

            def many(fn=legs[k], n=n):
                for _ in range(n):
                    fn()

            times[k].append(timed(many) / n)
            print(f"  {tag} pass {i} {k}: {1e3 * times[k][-1]:.3f} ms x {n}", flush=True)
    out = {k: {"best_ms": round(1e3 * min(t), 4), "worst_ms": round(1e3 * max(t), 4), "reps": reps[k]} for k, t in times.items()}
    out.update({k: {"failed": v} for k, v in failed.items()})
    return out, res


def measure(dev, side, n_vol, passes):
    import numpy as np
    import scipy.ndimage
    import torch
    import torch.nn.functional as F
    from nerfca_amd import ccta, phantom, synthetic
    geo = synthetic.xcat_geometry(128)
    vol = phantom.make_phantom((side,) * 3, n_vol, geo, device=dev)["dynamic"].contiguous()
    thr = 0.25 * phantom.RHO_VESSEL
    nodes = n_vol * side ** 3
    rec = {"side": side, "volumes": n_vol, "mask_nodes": int((vol > thr).sum())}
    tag = f"{side}^3 x {n_vol}"

    for name, sigma, r in SMOOTH:
        half = ccta.gaussian_weights(sigma, r)
        full = torch.from_numpy(np.concatenate([half[:0:-1], half])).to(dev)

        def ours(sigma=sigma, r=r):
            return ccta.gaussian_filter(vol, sigma, radius=r)

        def by_scipy(sigma=sigma, r=r):
            host = vol.cpu().numpy()
            out = np.stack([scipy.ndimage.gaussian_filter(v.astype(np.float64), sigma, radius=r, mode="reflect").astype(np.float32) for v in host])
            return torch.from_numpy(out).to(dev)

        def by_conv3d(r=r, full=full):
            x = vol.double()[:, None]
            for axis in range(3):
                pad = [0, 0, 0, 0, 0, 0]
                pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = r
                shape = [1, 1, 1, 1, 1]
                shape[2 + axis] = 2 * r + 1
                x = F.conv3d(F.pad(x, pad, mode="replicate"), full.reshape(shape))
            return x[:, 0].float()

        got, res = run_legs({"ours": ours, "scipy": by_scipy, "conv3d": by_conv3d}, passes, ("scipy",), f"{tag} {name}")
        if not torch.equal(res["ours"].view(torch.int32), res["scipy"].view(torch.int32)):
            sys.exit(f"filt_bench: ours differs from scipy at {tag} {name}")
        if "conv3d" in res:
            inner = (slice(None),) + (slice(r, side - r),) * 3
            scale = float(res["ours"].abs().max())
            off = float((res["ours"][inner].double() - res["conv3d"][inner].double()).abs().max())
            if off > 2.0 ** -22 * scale:          # two roundings to f32 of sums in another order
                sys.exit(f"filt_bench: ours differs from conv3d by {off:.3e} of {scale:.3e} at {tag} {name}")
        del res
        got["ours_gbytes_per_s"] = round(40 * nodes / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
        rec[name] = got
        torch.cuda.empty_cache()

    mask = (vol > thr).to(torch.float32)

    def ours_d():
        return ccta.binary_dilation(mask, 3, threshold=0.5)

    def scipy_d():
        host = mask.cpu().numpy() > 0.5
        return torch.from_numpy(np.stack([scipy.ndimage.binary_dilation(m, iterations=3) for m in host])).to(dev)

    def pool_d():
        x = mask[:, None]
        for _ in range(3):
            x = torch.maximum(torch.maximum(F.max_pool3d(x, (3, 1, 1), 1, (1, 0, 0)), F.max_pool3d(x, (1, 3, 1), 1, (0, 1, 0))), F.max_pool3d(x, (1, 1, 3), 1, (0, 0, 1)))
        return x[:, 0] > 0.5

    got, res = run_legs({"ours": ours_d, "scipy": scipy_d, "pool": pool_d}, passes, ("scipy",), f"{tag} dilate3")
    for k in ("scipy", "pool"):
        if k in res and not torch.equal(res["ours"], res[k]):
            sys.exit(f"filt_bench: ours differs from {k} at {tag} dilate3")
    del res
    got["ours_gbytes_per_s"] = round(24 * nodes / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
    rec["dilate3"] = got
    return rec


def table_of(lines):
    """The report: one row per size and measured call."""
    names = {"smooth_r2": ("scipy", "conv3d"), "smooth_r16": ("scipy", "conv3d"), "dilate3": ("scipy", "pool")}
    table = ["milliseconds per call, best / worst pass; scipy on the host with both copies; device baseline: conv3d in f64 (smooth), 1-D max_pool3d steps (dilate)",
             "side  vols  call         ours ms                  scipy ms                     device baseline ms           scipy/ours  device/ours   ours GB/s (40 / 24 B per node)"]
    slower = []
    for r in lines:
        for name, (host, devleg) in names.items():
            g = r[name]

            def cell(k):
                return f"{g[k]['best_ms']:>10.3f} / {g[k]['worst_ms']:<10.3f}" if "best_ms" in g[k] else f"{'failed':>10}   {'':<10}"

            def ratio(k):
                return f"{g[k]['best_ms'] / g['ours']['best_ms']:>9.1f}" if "best_ms" in g[k] else f"{'-':>9}"

            table.append(f"{r['side']:>4}  {r['volumes']:>4}  {name:<11}{cell('ours')}   {cell(host)}   {cell(devleg)}   {ratio(host)}   {ratio(devleg)}   {g['ours_gbytes_per_s']:>9.1f}")
            slower += [f"{r['side']}^3 x {r['volumes']} {name} ({k})" for k in (host, devleg) if "best_ms" in g[k] and g["ours"]["best_ms"] > g[k]["best_ms"]]
            for k in (host, devleg):
                if "failed" in g[k]:
                    table.append(f"      {k} failed at {r['side']}^3 x {r['volumes']} {name}: {g[k]['failed']}")
    table.append("rows in which ours is slower than a competitor: " + (", ".join(slower) if slower else "none"))
    table.append("agreement: ours equals scipy bit for bit in every row; conv3d within 2^-22 of the largest value away from the faces; the pooled dilation equal")
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("filt_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in (int(s) for s in args.sides.split(",")):
        for n_vol in (int(p) for p in args.volumes.split(",")):
            rec = measure(dev, side, n_vol, args.passes)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    table = table_of(lines)
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
