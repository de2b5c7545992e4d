#!/usr/bin/env python3
"""Time of metrics.soft_skeleton against the published torch expression on the same device, in ONE process:

    ours    metrics.soft_skeleton(vol, K): nca_vol_softskel, K + 1 launches of one tiled kernel, f32
    torch   the soft skeleton of the clDice paper as its authors wrote it: soft_erode = the minimum of three 1-D -max_pool3d(-x),
            soft_dilate = max_pool3d(x, 3, 1, 1), and the element-wise update, in f32 -- about fifteen launches per iteration

on the vessel volume of phantom.make_phantom divided by the vessel density (values in [0, 1]) at 128^3 and 256^3 nodes, 1 and 10 volumes,
K = 4 and K = 10.  Every leg is one warm-up pass and then `--passes` timed passes; the legs alternate.  A leg repeats its call inside a pass
until the pass lasts about 0.2 s; a pass ends in one device synchronise; the report is milliseconds per call, best and worst pass.
Algorithmic bytes: an iteration reads E_j and S and writes E_{j+1} and S, 16 bytes per node, K + 1 iterations; the GB/s column is those bytes
over the best time of the WHOLE call (launches and the workspace allocation included), so it is a lower bound on what the kernel reaches.
The tool stops if ours differs from the torch expression in one value.  The yardstick is the torch expression: a row in which ours is
slower is reported as it is.

    python3 tools/skel_bench.py [--out profiles/skel_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default="128,256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1,10", help="volumes per stack, comma separated")
    ap.add_argument("--iterations", default="4,10", help="skeleton iterations K, comma separated")
    return ap


def torch_soft_skeleton(x, iterations):
    """Shit et al., clDice (CVPR 2021), soft_skeleton.py, on f32 [N, 1, n0, n1, n2]."""
    import torch
    import torch.nn.functional as F

    def soft_erode(img):
        p1 = -F.max_pool3d(-img, (3, 1, 1), (1, 1, 1), (1, 0, 0))
        p2 = -F.max_pool3d(-img, (1, 3, 1), (1, 1, 1), (0, 1, 0))
        p3 = -F.max_pool3d(-img, (1, 1, 3), (1, 1, 1), (0, 0, 1))
        return torch.min(torch.min(p1, p2), p3)

    def soft_open(img):
        return F.max_pool3d(soft_erode(img), (3, 3, 3), (1, 1, 1), (1, 1, 1))

    skel = F.relu(x - soft_open(x))
    for _ in range(iterations):
        x = soft_erode(x)
        delta = F.relu(x - soft_open(x))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def measure(dev, side, n_vol, K, passes):
    import torch
    from filt_bench import run_legs
    from nerfca_amd import metrics, phantom, synthetic
    geo = synthetic.xcat_geometry(128)
    vol = (phantom.make_phantom((side,) * 3, n_vol, geo, device=dev)["dynamic"] / phantom.RHO_VESSEL).contiguous()
    nodes = n_vol * side ** 3
    tag = f"{side}^3 x {n_vol} K={K}"

    def ours():
        return metrics.soft_skeleton(vol, K)

    def by_torch():
        with torch.no_grad():
            return torch_soft_skeleton(vol[:, None], K)[:, 0]

    got, res = run_legs({"ours": ours, "torch": by_torch}, passes, (), tag)
    rec = {"side": side, "volumes": n_vol, "iterations": K, "skeleton_sum": float(res["ours"].double().sum()), **got}
    if "torch" in res and not torch.equal(res["ours"], res["torch"]):
        sys.exit(f"skel_bench: ours differs from the torch expression at {tag}: largest difference {float((res['ours'] - res['torch']).abs().max()):.3e}")
    rec["ours_gbytes_per_s"] = round(16 * (K + 1) * nodes / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
    return rec


def table_of(lines):
    """The report: one row per size and K."""
    table = ["milliseconds per call, best / worst pass; torch: the published max_pool3d expression in f32 on the same device",
             "side  vols   K   ours ms                  torch ms                  torch/ours   ours GB/s (16 B per node and iteration)"]
    slower = []
    for r in lines:
        def cell(k):
            return f"{r[k]['best_ms']:>10.3f} / {r[k]['worst_ms']:<10.3f}" if "best_ms" in r[k] else f"{'failed':>10}   {'':<10}"

        ratio = f"{r['torch']['best_ms'] / r['ours']['best_ms']:>9.1f}" if "best_ms" in r["torch"] else f"{'-':>9}"
        table.append(f"{r['side']:>4}  {r['volumes']:>4}  {r['iterations']:>2}  {cell('ours')}   {cell('torch')}   {ratio}   {r['ours_gbytes_per_s']:>9.1f}")
        if "failed" in r["torch"]:
            table.append(f"      torch failed at {r['side']}^3 x {r['volumes']} K={r['iterations']}: {r['torch']['failed']}")
        elif r["ours"]["best_ms"] > r["torch"]["best_ms"]:
            slower.append(f"{r['side']}^3 x {r['volumes']} K={r['iterations']}")
    table.append("rows in which ours is slower than the torch expression: " + (", ".join(slower) if slower else "none"))
    table.append("agreement: ours equals the torch expression value for value in every row")
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("skel_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in (int(s) for s in args.sides.split(",")):
        for n_vol in (int(p) for p in args.volumes.split(",")):
            for K in (int(k) for k in args.iterations.split(",")):
                rec = measure(dev, side, n_vol, K, args.passes)
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
