#!/usr/bin/env python3
"""Time of the phantom rasteriser (phantom.voxelize: nca_phantom_voxelize) on the default coronary tree against the torch expression of the
same field, in ONE process:

    cull_on    phantom.voxelize(segments=tree) with tile-level culling of segments
    cull_off   the same launch, every node evaluates every segment
    torch_f64  what a user of torch writes without the kernel: the [nodes, segments] point-to-segment distances by broadcasting in f64,
               chunked over nodes so that the intermediates fit, clamp, amax over the segments, written as f32

for grids of 128^3 and 256^3 nodes over the field of view of synthetic.xcat_geometry and P in {1, 10} heart phases.  Every leg is one
warm-up pass and then three timed passes; the legs alternate.  A timed pass ends in one device synchronise; the report is milliseconds per
call, best and worst pass, and torch / ours.  The tool stops if a leg differs from the torch expression kept in f64 by more than the bound of
tests/test_phantom_gpu.py (2^-24 |v| + 2^-52 4 max(1, L / edge) rho_v), or if culling changes a bit.

The kernel is also timed on its own (device events around INNER direct launches, best of three) and reported as node x segment pairs per
second: the pairs the definition has, whether or not culling skipped them.

    python3 tools/phantom_bench.py [--out profiles/phantom_bench.txt]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from view_render_bench import timed  # noqa: E402

PHASE_COUNTS = (1, 10)
VOLUME_SIDES = (128, 256)
REPEATS = 3
INNER = 5
CHUNK_BYTES = 1 << 28          # of one [chunk, segments] f64 intermediate of the torch leg


def torch_voxelize(shape, bounds, seg, rho_v, edge, out_dtype=torch.float32):
    """[P,n0,n1,n2] of seg f64 [P,N,8] on the device: the definition of include/nerfca_hip.h ("phantom") as broadcasting torch in f64."""
    dev = seg.device
    axes = []
    for n, (lo, hi) in zip(shape, bounds):
        h = 1.0 / ((n - 1) / (hi - lo))
        axes.append(lo + torch.arange(n, dtype=torch.float64, device=dev) * h)
    pts = torch.cartesian_prod(*axes)                                           # [V,3], the last axis fastest
    P, N = seg.shape[0], seg.shape[1]
    out = torch.empty((P, pts.shape[0]), dtype=out_dtype, device=dev)
    chunk = max(1, CHUNK_BYTES // (8 * N))
    for p in range(P):
        a, b, ra, rb = seg[p, :, 0:3], seg[p, :, 3:6], seg[p, :, 6], seg[p, :, 7]
        e = b - a
        ee = (e * e).sum(-1)
        for c0 in range(0, pts.shape[0], chunk):
            q = pts[c0:c0 + chunk, None, :] - a[None]                           # [C,N,3]
            t = torch.where(ee > 0, (q * e).sum(-1) / ee, torch.zeros_like(ee)).clamp(0.0, 1.0)
            d = (q - t[..., None] * e).norm(dim=-1)
            cov = (0.5 + ((ra + t * (rb - ra)) - d) / edge).clamp(0.0, 1.0)
            out[p, c0:c0 + chunk] = (rho_v * cov.amax(dim=1)).to(out_dtype)
    return out.reshape((P,) + tuple(shape))


def kernel_ms(shape, bounds, seg, rho_v, edge, inner):
    """Milliseconds of one nca_phantom_voxelize launch at the current culling: device events around `inner` launches, best of REPEATS."""
    from nerfca_amd import _capi, drr, fused
    desc = drr.grid_desc(shape, bounds)
    out = torch.empty((seg.shape[0],) + tuple(shape), dtype=torch.float32, device=seg.device)
    lib, st = _capi.lib(), fused._stream()
    fn = lambda: _capi.check_phantom(lib.nca_phantom_voxelize(C.byref(desc), seg.shape[0], 0, None, seg.shape[1], _capi.ptr(seg), rho_v, edge, _capi.ptr(out), st))
    fn()
    best = float("inf")
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / inner)
    return best


def measure(dev, side, n_phases, inner):
    from nerfca_amd import phantom, synthetic
    geo = synthetic.xcat_geometry(128)
    hw = phantom.fov_half_width(geo)
    bounds, shape = ((-hw, hw),) * 3, (side,) * 3
    tree = phantom.coronary_tree(n_phases, seed=0, center=tuple(hw * c for c in phantom.HEART_CENTER), heart_radius=hw * phantom.HEART_RADIUS)
    seg = torch.from_numpy(tree).to(dev)
    rho_v, edge = phantom.RHO_VESSEL, 2 * hw / (side - 1)
    default_cull = phantom.get_cull()

    def ours(cull):
        phantom.set_cull(cull)
        return phantom.voxelize(shape, bounds, segments=tree, rho_vessel=rho_v, edge=edge, device=dev)

    legs = {"cull_on": lambda: ours(True), "cull_off": lambda: ours(False), "torch_f64": lambda: torch_voxelize(shape, bounds, seg, rho_v, edge)}
    try:
        want = torch_voxelize(shape, bounds, seg, rho_v, edge, torch.float64)          # warm-up, and the agreement check
        tol = 2.0 ** -24 * want.abs() + 2.0 ** -52 * 4 * max(1.0, math.sqrt(3) * 2 * hw / edge) * abs(rho_v)
        got = {k: legs[k]() for k in legs}
        worst = {k: float(((got[k].double() - want).abs() / tol).max()) for k in legs}
        if not all(w <= 1.0 for w in worst.values()):
            sys.exit(f"phantom_bench: the legs do not make the same volumes ({side}^3, P = {n_phases}: error over bound {worst})")
        if not torch.equal(got["cull_on"], got["cull_off"]):
            sys.exit(f"phantom_bench: culling changed the output ({side}^3, P = {n_phases})")
        filled = float((want > 0).double().mean())
        del want, tol, got
        times = {k: [] for k in legs}
        for _ in range(REPEATS):
            for k, fn in legs.items():                              # alternate the legs
                n = 1 if k == "torch_f64" else inner
                times[k].append(timed(lambda: [fn() for _ in range(n)]) / n)
        rec = {"volume": side, "phases": n_phases, "segments": int(tree.shape[1]), "vessel_fraction": round(filled, 5), "error_over_bound": {k: round(v, 4) for k, v in worst.items()}}
        for k in legs:
            rec[k] = {"best_s": round(min(times[k]), 6), "worst_s": round(max(times[k]), 6)}
        for k in ("cull_on", "cull_off"):
            rec["torch_over_" + k + "_best"] = round(rec["torch_f64"]["best_s"] / rec[k]["best_s"], 1)
            rec["torch_worst_over_" + k + "_worst"] = round(rec["torch_f64"]["worst_s"] / rec[k]["worst_s"], 1)
        pairs = float(n_phases) * side ** 3 * tree.shape[1]
        rec["kernel_ms"], rec["kernel_gpairs_per_s"] = {}, {}
        for k, cull in (("cull_on", True), ("cull_off", False)):
            phantom.set_cull(cull)
            ms = kernel_ms(shape, bounds, seg, rho_v, edge, inner)
            rec["kernel_ms"][k], rec["kernel_gpairs_per_s"][k] = round(ms, 4), round(pairs / ms / 1e6, 1)
    finally:
        phantom.set_cull(default_cull)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--inner", type=int, default=INNER, help="calls per timed pass of our legs (the torch leg makes one)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("phantom_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    from nerfca_amd import phantom
    lines = []
    for side in VOLUME_SIDES:
        for n_phases in PHASE_COUNTS:
            rec = measure(dev, side, n_phases, args.inner)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    table = [f"milliseconds per voxelize of the default coronary tree into [P,n,n,n], best / worst pass (library default: culling {'on' if phantom.get_cull() else 'off'})",
             "volume  P   segments   cull on ms            cull off ms           torch f64 ms            torch/on  torch/off   (worst/worst: on, off)"]
    for r in lines:
        cells = "".join(f"   {1e3 * r[k]['best_s']:>9.3f} / {1e3 * r[k]['worst_s']:<9.3f}" for k in ("cull_on", "cull_off", "torch_f64"))
        table.append(f"{r['volume']:>4}^3  {r['phases']:<3} {r['segments']:>5}{cells}   {r['torch_over_cull_on_best']:>8.1f}   {r['torch_over_cull_off_best']:>8.1f}      "
                     f"{r['torch_worst_over_cull_on_worst']:>7.1f}, {r['torch_worst_over_cull_off_worst']:<7.1f}")
    table.append("the kernel alone: milliseconds per launch and 1e9 node x segment pairs of the definition per second; largest error over the test bound; nodes with a vessel")
    for r in lines:
        table.append(f"{r['volume']:>4}^3  {r['phases']:<3}   cull on {r['kernel_ms']['cull_on']:>9.4f} ms {r['kernel_gpairs_per_s']['cull_on']:>9.1f} Gpairs/s"
                     f"      cull off {r['kernel_ms']['cull_off']:>9.4f} ms {r['kernel_gpairs_per_s']['cull_off']:>9.1f} Gpairs/s"
                     f"      error/bound {max(r['error_over_bound'].values()):.3f}      filled {100 * r['vessel_fraction']:.3f} %")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
