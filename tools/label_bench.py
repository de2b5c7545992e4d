#!/usr/bin/env python3
"""Time of metrics.label against the two ways to label without it, in ONE process:

    ours    metrics.label(vol, threshold, connectivity): nca_vol_label, six launches (a union-find in LDS per tile, the unions across
            tiles, flattening, the scan of the root counts, the numbering of the roots, relabelling)
    scipy   scipy.ndimage.label(mask, generate_binary_structure(3, connectivity)) per volume on the host, with the copy of the f32 stack
            to the host and of the int32 labels back: what a caller without the kernel does
    pool    label propagation on the device: every mask node starts with its linear index + 1, and max_pool3d over the neighbourhood
            (3 x 3 x 3 at connectivity 3, the maximum of three 1-D pools at connectivity 1), masked, is iterated until nothing changes, with
            one host sync per eight passes.  It needs as many passes as the longest path through a component, so it is run only where
            `--pool-limit` passes suffice, and reported as failed elsewhere.  Its labels are the largest index of a component, not scipy's
            numbering: it is held to ours by the partition only.

on two masks at 128^3 and 256^3 nodes, 1 and 10 volumes, connectivity 1 and 3: `tree`, the vessel volume of phantom.make_phantom above a
quarter of the vessel density (the thickened phantom tree: a few large components), and `random`, a uniform random volume above 0.69:
density 0.31, the 6-connected percolation threshold, where the components are most tangled.  Every leg is one warm-up pass and then
`--passes` timed passes; the legs alternate.  A leg repeats its call inside a pass until the pass lasts about 0.2 s (host legs run once); a
pass ends in one device synchronise; the report is milliseconds per call, best and worst pass.  Algorithmic bytes: 4 read and 4 written per
node; the GB/s column is those bytes over the best time of the WHOLE call.  The share of the call per launch comes from one extra run of the
six kernels under the profiler of torch (kernel times by name).  The tool stops if ours differs from scipy in one label or count.  A row in
which ours is slower than scipy is reported as it is.

    python3 tools/label_bench.py [--out profiles/label_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("local", "seam", "flatten", "scan", "apply", "relabel")
RANDOM_THRESHOLD = 0.69          # density 0.31


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default="128,256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1,10", help="volumes per stack, comma separated")
    ap.add_argument("--connectivities", default="1,3", help="connectivity 1, 2 or 3, comma separated")
    ap.add_argument("--masks", default="tree,random", help="tree, random or both, comma separated")
    ap.add_argument("--pool-limit", type=int, default=2048, help="the max_pool3d propagation gives up after this many passes")
    return ap


def pool_labels(mask, connectivity, limit):
    """Label propagation by max_pool3d on a bool stack [N, n0, n1, n2]: int32 labels (the largest linear index + 1 of the component)."""
    import torch
    import torch.nn.functional as F
    if connectivity == 2:
        raise RuntimeError("max_pool3d has no 18-neighbourhood")
    n = mask.shape[1] * mask.shape[2] * mask.shape[3]
    seed = torch.arange(1, n + 1, dtype=torch.float32, device=mask.device).reshape((1, 1) + tuple(mask.shape[1:]))          # exact below 2^24
    if n >= 1 << 24:
        seed = seed.double()
    m = mask[:, None]
    lab = torch.where(m, seed, torch.zeros((), dtype=seed.dtype, device=mask.device))

    def step(x):
        if connectivity == 3:
            y = F.max_pool3d(x, 3, 1, 1)
        else:
            y = torch.maximum(torch.maximum(F.max_pool3d(x, (3, 1, 1), 1, (1, 0, 0)), F.max_pool3d(x, (1, 3, 1), 1, (0, 1, 0))), F.max_pool3d(x, (1, 1, 3), 1, (0, 0, 1)))
        return torch.where(m, y, torch.zeros((), dtype=x.dtype, device=x.device))

    passes = 0
    while passes < limit:
        for _ in range(8):
            lab = step(lab)
        passes += 8
        if torch.equal(step(lab), lab):          # the one host sync per eight passes
            return lab[:, 0].to(torch.int64), passes
    raise RuntimeError(f"not converged after {limit} passes")


def same_partition(a, b):
    """Do two label stacks (0 = background) cut every volume into the same components?"""
    import torch
    for x, y in zip(a.reshape(a.shape[0], -1).to(torch.int64), b.reshape(b.shape[0], -1).to(torch.int64)):
        if not torch.equal(x > 0, y > 0):
            return False
        pairs = torch.unique(torch.stack([x[x > 0], y[y > 0]]), dim=1)
        if pairs.shape[1] != torch.unique(pairs[0]).numel() or pairs.shape[1] != torch.unique(pairs[1]).numel():
            return False
    return True


def kernel_shares(call):
    """{launch: share of the six kernels' time} from one run under torch's profiler; None where it sees no kernel of ours."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    us = {k: 0.0 for k in KERNELS}
    for e in prof.key_averages():
        for k in KERNELS:
            if f"label_{k}_kernel" in e.key:
                us[k] += float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
    total = sum(us.values())
    return {k: round(v / total, 4) for k, v in us.items()} if total > 0 else None


def measure(dev, kind, side, n_vol, conn, passes, pool_limit):
    import numpy as np
    import scipy.ndimage
    import torch
    from filt_bench import run_legs
    from nerfca_amd import metrics, phantom, synthetic
    if kind == "tree":
        vol = phantom.make_phantom((side,) * 3, n_vol, synthetic.xcat_geometry(128), device=dev)["dynamic"].contiguous()
        thr = 0.25 * phantom.RHO_VESSEL
    else:
        vol = torch.rand((n_vol,) + (side,) * 3, generator=torch.Generator(device=dev).manual_seed(31 * side + n_vol), device=dev)
        thr = RANDOM_THRESHOLD
    nodes = n_vol * side ** 3
    tag = f"{kind} {side}^3 x {n_vol} c={conn}"
    structure = scipy.ndimage.generate_binary_structure(3, conn)

    def ours():
        return metrics.label(vol, threshold=thr, connectivity=conn)

    def by_scipy():
        x = vol.cpu().numpy()
        out = np.empty(x.shape, dtype=np.int32)
        counts = [scipy.ndimage.label(x[v] > thr, structure, output=out[v]) for v in range(x.shape[0])]
        return torch.from_numpy(out).to(dev), torch.tensor(counts, dtype=torch.int64, device=dev)

    def by_pool():
        with torch.no_grad():
            return pool_labels(vol > thr, conn, pool_limit)

    got, res = run_legs({"ours": ours, "scipy": by_scipy, "pool": by_pool}, passes, ("scipy",), tag)
    labels, counts = res["ours"]
    rec = {"mask": kind, "side": side, "volumes": n_vol, "connectivity": conn, "mask_nodes": int((vol > thr).sum()), "components": counts.tolist(), **got}
    if "scipy" in res and not (torch.equal(labels, res["scipy"][0]) and torch.equal(counts, res["scipy"][1])):
        sys.exit(f"label_bench: ours differs from scipy.ndimage.label at {tag}: counts {counts.tolist()} against {res['scipy'][1].tolist()}")
    if "pool" in res:
        rec["pool_passes"] = res["pool"][1]
        if not same_partition(labels, res["pool"][0]):
            sys.exit(f"label_bench: ours and the max_pool3d propagation cut {tag} differently")
    rec["ours_gbytes_per_s"] = round(8 * nodes / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
    try:
        rec["shares"] = kernel_shares(ours)
    except Exception as e:          # the profiler is a convenience: the times above do not depend on it
        rec["shares"] = None
        rec["shares_failed"] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
    return rec


def table_of(lines):
    """The report: one row per mask, size and connectivity."""
    table = ["milliseconds per call, best / worst pass; scipy: the host with both copies; pool: max_pool3d propagation on the device to convergence",
             "mask    side  vols  c   ours ms                  scipy ms                  pool ms (passes)                  scipy/ours  pool/ours  ours GB/s (8 B per node)   share per launch: "
             + " ".join(KERNELS)]
    slower = []
    for r in lines:
        def cell(k):
            return f"{r[k]['best_ms']:>10.3f} / {r[k]['worst_ms']:<10.3f}" if "best_ms" in r[k] else f"{'failed':>10}   {'':<10}"

        def ratio(k):
            return f"{r[k]['best_ms'] / r['ours']['best_ms']:>9.1f}" if "best_ms" in r[k] else f"{'-':>9}"

        shares = " ".join(f"{r['shares'][k]:.2f}" for k in KERNELS) if r.get("shares") else "-"
        table.append(f"{r['mask']:<6}  {r['side']:>4}  {r['volumes']:>4}  {r['connectivity']}  {cell('ours')}   {cell('scipy')}   {cell('pool')} ({r.get('pool_passes', '-'):>5})   {ratio('scipy')}  {ratio('pool')}  "
                     f"{r['ours_gbytes_per_s']:>9.1f}                  {shares}")
        for k in ("scipy", "pool"):
            if "failed" in r[k]:
                table.append(f"        {k} failed at {r['mask']} {r['side']}^3 x {r['volumes']} c={r['connectivity']}: {r[k]['failed']}")
        if "best_ms" in r["scipy"] and r["ours"]["best_ms"] > r["scipy"]["best_ms"]:
            slower.append(f"{r['mask']} {r['side']}^3 x {r['volumes']} c={r['connectivity']}")
    table.append("rows in which ours is slower than scipy on the host: " + (", ".join(slower) if slower else "none"))
    table.append("agreement: ours equals scipy.ndimage.label label for label and count for count in every row; the propagation, where it converged, cuts the same components")
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("label_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for kind in (k.strip() for k in args.masks.split(",")):
        if kind not in ("tree", "random"):
            sys.exit(f"label_bench: --masks {kind!r} is neither tree nor random")
        for side in (int(s) for s in args.sides.split(",")):
            for n_vol in (int(p) for p in args.volumes.split(",")):
                for conn in (int(c) for c in args.connectivities.split(",")):
                    rec = measure(dev, kind, side, n_vol, conn, args.passes, args.pool_limit)
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
