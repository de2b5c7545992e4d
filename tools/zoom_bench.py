#!/usr/bin/env python3
"""Time of nerfca_amd.ccta.zoom against what a user writes without it, in ONE process:

    zoom3          ccta.zoom(vol, f, order=3): nca_vol_zoom, the three launches of the prefilter and one gather launch, on the device
      prefilter    ccta.spline_filter(vol) alone (the same three launches into a fresh f64 tensor): its share of zoom3
      scipy        scipy.ndimage.zoom(v, f, order=3) per volume on the host, INCLUDING the copy of the stack to the host and of the result back
                   to the device.  Timed ONCE (it takes seconds), and for a stack of ten on its first volume only: the table shows that time
                   plus nine times its compute part, marked `x10`
      trilinear    F.interpolate(mode="trilinear", align_corners=True) in f32 on the device: the same node placement, a CHEAPER operation
                   (8 taps, no prefilter), not an equal one -- torch has no cubic resampler for volumes
    zoom0          ccta.zoom(vol, f, order=0): one launch
      scipy        scipy.ndimage.zoom(v, f, order=0), as above

on the vessel volume of phantom.make_phantom at 128^3 and 256^3 nodes, 1 and 10 volumes, zoom factors 0.5 and 1.6.  A device leg is one
warm-up pass and then `--passes` timed passes; the legs alternate; a pass repeats its call until it lasts about 0.2 s and ends in one device
synchronise; the report is milliseconds per call, best and worst pass.  Algorithmic bytes of zoom3: 36 per input node for the prefilter
(f32 in, f64 out; then f64 in and out twice) plus 4 per output node; the gather's reads of the coefficients are left out (every coefficient
is read by many output nodes, mostly from cache), so the GB/s column is a lower bound on what the kernels move.  The tool stops if ours
differs from scipy by more than one f32 step plus 2^-44 of the largest value at order 3 or in one bit at order 0 -- on every plane but the
last of an axis at which scipy's coordinate overshoots (there scipy writes 0 and ours the last input node; the report counts them).

    python3 tools/zoom_bench.py [--out profiles/zoom_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per device leg")
    ap.add_argument("--sides", default="128,256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1,10", help="volumes per stack, comma separated")
    ap.add_argument("--factors", default="0.5,1.6", help="zoom factors, comma separated")
    return ap


def overshoots(n, m):
    return float(m - 1) * ((n - 1) / (m - 1)) > float(n - 1)


def measure(dev, side, n_vol, factor, passes):
    import numpy as np
    import scipy.ndimage
    import torch
    import torch.nn.functional as F
    from filt_bench import run_legs
    from nerfca_amd import ccta, phantom, synthetic
    geo = synthetic.xcat_geometry(128)
    vol = phantom.make_phantom((side,) * 3, n_vol, geo, device=dev)["dynamic"].contiguous()
    m = int(round(side * factor))
    over = overshoots(side, m)
    rec = {"side": side, "volumes": n_vol, "factor": factor, "out_side": m, "scipy_overshoots": over}
    tag = f"{side}^3 x {n_vol} x {factor}"
    scale = float(vol.abs().max())

    def by_scipy(order):
        """(seconds in all, seconds of the scipy call, the result of volume 0): both copies of the whole stack, scipy on volume 0."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = vol.cpu().numpy()
        t1 = time.perf_counter()
        first = scipy.ndimage.zoom(host[0], factor, order=order)
        t2 = time.perf_counter()
        back = np.broadcast_to(first, (n_vol,) + first.shape)
        torch.from_numpy(np.ascontiguousarray(back)).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return (t1 - t0) + (t3 - t2) + n_vol * (t2 - t1), t2 - t1, first

    for order, name in ((3, "zoom3"), (0, "zoom0")):
        legs = {"ours": lambda order=order: ccta.zoom(vol, factor, order=order)}
        if order == 3:
            legs["prefilter"] = lambda: ccta.spline_filter(vol)
            legs["trilinear"] = lambda: F.interpolate(vol[:, None], size=(m, m, m), mode="trilinear", align_corners=True)[:, 0]
        got, res = run_legs(legs, passes, (), f"{tag} {name}")
        total, call, sci = by_scipy(order)
        got["scipy"] = {"best_ms": round(1e3 * total, 1), "call_ms": round(1e3 * call, 1), "extrapolated": n_vol > 1}
        mine = res["ours"][0].cpu().numpy()
        keep = slice(None, -1) if over else slice(None)          # scipy's last planes are 0 there
        a, b = mine[keep, keep, keep].astype(np.float64), sci[keep, keep, keep].astype(np.float64)
        off = float(np.abs(a - b).max())
        bound = (np.spacing(np.abs(b).astype(np.float32)).astype(np.float64) + 2.0 ** -44 * scale) if order == 3 else np.zeros_like(b)
        if not (np.abs(a - b) <= bound).all():
            sys.exit(f"zoom_bench: ours differs from scipy by {off:.3e} at {tag} {name}")
        got["differing_nodes"] = int((a != b).sum())
        if order == 3 and "trilinear" in res:          # a different interpolant: only the node placement is comparable, at the corners
            tri = res["trilinear"][0]
            got["trilinear_corner_off"] = float((tri[0, 0, 0] - res["ours"][0, 0, 0, 0]).abs() + (tri[-1, -1, -1] - res["ours"][0, -1, -1, -1]).abs())
        del res
        if order == 3:
            got["ours_gbytes_per_s"] = round((36 * n_vol * side ** 3 + 4 * n_vol * m ** 3) / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
            got["prefilter_share"] = round(got["prefilter"]["best_ms"] / got["ours"]["best_ms"], 3)
        rec[name] = got
        torch.cuda.empty_cache()
    return rec


def table_of(lines):
    table = ["milliseconds per call, best / worst pass; scipy on the host with both copies, timed once (x10: one volume's call time ten times);",
             "trilinear is F.interpolate(align_corners=True) in f32 on the device: a cheaper operation, not an equal one",
             "side  vols  factor  call    ours ms                  prefilter ms (share)            scipy ms        trilinear ms             scipy/ours   ours GB/s"]
    for r in lines:
        for name in ("zoom3", "zoom0"):
            g = r[name]

            def cell(k):
                return f"{g[k]['best_ms']:>10.3f} / {g[k]['worst_ms']:<10.3f}" if k in g and "best_ms" in g[k] else f"{'failed' if k in g else '-':>10}   {'':<10}"

            share = f"({g['prefilter_share']:.2f})" if "prefilter_share" in g else ""
            sci = f"{g['scipy']['best_ms']:>10.1f}{' x10' if g['scipy']['extrapolated'] else '    '}"
            gb = f"{g['ours_gbytes_per_s']:>9.1f}" if "ours_gbytes_per_s" in g else f"{'-':>9}"
            table.append(f"{r['side']:>4}  {r['volumes']:>4}  {r['factor']:>6}  {name:<6}{cell('ours')}   {cell('prefilter')} {share:<6}  {sci}   {cell('trilinear')}   "
                         f"{g['scipy']['best_ms'] / g['ours']['best_ms']:>9.1f}   {gb}")
    over = sorted({(r["side"], r["out_side"]) for r in lines if r["scipy_overshoots"]})
    table.append("agreement: order 3 within one f32 step + 2^-44 of the largest value of scipy in every row, order 0 equal bit for bit" +
                 ("; scipy overshoots at " + ", ".join(f"{n} -> {m}" for n, m in over) + ": its last planes are 0 and are left out" if over else "; no size pair overshoots"))
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("zoom_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in (int(s) for s in args.sides.split(",")):
        for n_vol in (int(p) for p in args.volumes.split(",")):
            for factor in (float(f) for f in args.factors.split(",")):
                rec = measure(dev, side, n_vol, factor, args.passes)
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
