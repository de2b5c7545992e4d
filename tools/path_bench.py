#!/usr/bin/env python3
"""Times the geodesic distance transform (centreline.geodesic_distance, nca_vol_geodesic) on the phantom's vessel mask.

Per grid size (128 and 256 nodes per axis) and stack (1 and 10 heart phases): the mask is dynamic > rho / 4, the cost 1 on it, 26
neighbours, one seed per volume (the mask node nearest the first segment's start).  Reported, with tile skipping on and off:

  * the sweeps to the fixed point (the first sweep that changes nothing included) and the share of tile runs that skipping saves, both
    counted from the states sweep by sweep (a tile runs in sweep s when it or one of its 26 neighbour tiles changed in sweep s - 1);
  * ms of ONE call with exactly that many sweeps (no host read) and of the converging call (batches of 16 sweeps, one read per batch), each
    the best of --passes;
  * GB/s of the 20 algorithmic bytes per node and sweep (8 read, 8 written, 4 of cost) of the tiles that ran.

Against: scipy.sparse.csgraph.dijkstra on the host, graph construction and both copies included (one volume); and the plain-torch
Jacobi expression on the device (26 shifted adds and a minimum per iteration in f64, iterated until nothing changes, checked every 16
iterations; not run for 10 volumes at 256^3, where it needs minutes).  Both results are compared with the kernel's.  Also one
centreline.extract of phase 0.  Every row is reported, slower ones included; no figure is a pass criterion.

    python3 tools/path_bench.py [--out profiles/path_bench.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE = (4, 8, 64)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sides", default="128,256")
    ap.add_argument("--volumes", default="1,10")
    ap.add_argument("--passes", type=int, default=3)
    return ap


def offsets():
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def tile_map(flag):
    """bool [n_vol, nb0, nb1, nb2]: the tiles of 4 x 8 x 64 nodes that hold a set node of bool [n_vol, n0, n1, n2]"""
    import torch.nn.functional as F
    n = flag.shape[1:]
    pad = [(-n[a]) % TILE[a] for a in range(3)]
    x = F.pad(flag, (0, pad[2], 0, pad[1], 0, pad[0]))
    nb = [x.shape[1 + a] // TILE[a] for a in range(3)]
    return x.reshape(x.shape[0], nb[0], TILE[0], nb[1], TILE[1], nb[2], TILE[2]).any(dim=6).any(dim=4).any(dim=2)


def count_sweeps(cl, cost, bounds, d0):
    """(sweeps to the fixed point, tile runs with skipping, tile runs without) from the states, sweep by sweep"""
    import torch
    import torch.nn.functional as F
    d, sweeps, runs, prev_changed = d0, 0, 0, None
    while True:
        new, changed = cl.geodesic_distance(cost, bounds, init=d, sweeps=1)
        sweeps += 1
        tiles = tile_map(new != d)
        runs += tiles.numel() if prev_changed is None else int((F.max_pool3d(prev_changed[:, None].float(), 3, 1, 1) > 0).sum())
        assert int(tiles.sum()) == int(changed.sum())
        prev_changed, d = tiles, new
        if int(changed.max()) == 0:
            return sweeps, runs, tiles.numel() * sweeps


def best_ms(fn, passes):
    import torch
    out = math.inf
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out = min(out, (time.perf_counter() - t0) * 1e3)
    return out


def torch_jacobi(cost, h, d0):
    """(the fixed point, iterations) of D <- min(D, min_d shift_d(D) + w_d) in plain torch, f64; walls carry the cost +inf"""
    import torch
    import torch.nn.functional as F
    n = cost.shape[1:]
    c = torch.where(torch.isfinite(cost) & (cost >= 0), cost.double(), torch.full_like(cost, math.inf, dtype=torch.float64))
    cp = F.pad(c, (1, 1, 1, 1, 1, 1), value=math.inf)
    wall = torch.isinf(c)
    d = torch.where(wall, torch.full_like(d0, math.inf), d0)
    steps = [(o, math.sqrt(((o[0] * h[0]) ** 2 + (o[1] * h[1]) ** 2) + (o[2] * h[2]) ** 2)) for o in offsets()]
    weights = [ln * (0.5 * (cp[:, 1 + o[0]:1 + o[0] + n[0], 1 + o[1]:1 + o[1] + n[1], 1 + o[2]:1 + o[2] + n[2]] + c)) for o, ln in steps]
    its = 0
    while True:
        before = d
        for _ in range(16):
            dp = F.pad(d, (1, 1, 1, 1, 1, 1), value=math.inf)
            new = d
            for (o, _), w in zip(steps, weights):
                new = torch.minimum(new, dp[:, 1 + o[0]:1 + o[0] + n[0], 1 + o[1]:1 + o[1] + n[1], 1 + o[2]:1 + o[2] + n[2]] + w)
            d = torch.where(wall, d, new)
            its += 1
        if torch.equal(d, before):
            return d, its


def scipy_dijkstra(cost_dev, h, seed):
    """the host baseline on ONE volume: the copy down, the graph of the open nodes, scipy's Dijkstra, the copy back"""
    import numpy as np
    import scipy.sparse
    import scipy.sparse.csgraph
    import torch
    cost = cost_dev.cpu().numpy()
    with np.errstate(invalid="ignore"):
        op = np.isfinite(cost) & (cost >= 0)
    number = np.full(cost.shape, -1, dtype=np.int64)
    number[op] = np.arange(int(op.sum()))
    c64 = cost.astype(np.float64)
    rows, cols, vals = [], [], []
    for o in offsets():
        sv = tuple(slice(max(0, -o[a]), cost.shape[a] - max(0, o[a])) for a in range(3))
        su = tuple(slice(max(0, o[a]), cost.shape[a] - max(0, -o[a])) for a in range(3))
        both = op[sv] & op[su]
        ln = math.sqrt(((o[0] * h[0]) ** 2 + (o[1] * h[1]) ** 2) + (o[2] * h[2]) ** 2)
        rows.append(number[sv][both]), cols.append(number[su][both]), vals.append(ln * (0.5 * (c64[su][both] + c64[sv][both])))
    g = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(int(op.sum()),) * 2)
    dist = scipy.sparse.csgraph.dijkstra(g, directed=True, indices=int(number.reshape(-1)[seed]))
    out = np.full(cost.shape, np.inf)
    out[op] = dist
    return torch.from_numpy(out).to(cost_dev.device)


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("path_bench needs the GPU")
    from nerfca_amd import centreline as cl, phantom, synthetic
    dev = torch.device("cuda:0")
    lines = ["geodesic distance on the phantom's vessel mask (dynamic > rho / 4, cost 1, 26 neighbours, one seed per volume); ms are the best of "
             f"{args.passes} passes; GB/s = 20 bytes x 2048 nodes x the tiles that ran / the time of the call without host reads",
             "side  volumes  mask nodes  skip  sweeps  tile runs saved  ms (N sweeps, no read)  ms (converging call)  GB/s     torch Jacobi ms (iterations, same bits)  scipy Dijkstra ms (max |diff|)"]
    geo = synthetic.xcat_geometry(128)
    for side in (int(s) for s in args.sides.split(",")):
        ph = phantom.make_phantom((side,) * 3, 10, geo, device=dev)
        bounds = ph["bounds"]
        h = [(b[1] - b[0]) / (side - 1) for b in bounds]
        for n_vol in (int(v) for v in args.volumes.split(",")):
            mask = ph["dynamic"][:n_vol] > 0.25 * phantom.RHO_VESSEL
            cost = torch.where(mask, 1.0, math.nan).to(torch.float32)
            seeds = []
            for v in range(n_vol):
                idx = mask[v].nonzero()
                world = torch.tensor([b[0] for b in bounds], dtype=torch.float64, device=dev) + idx.double() * torch.tensor(h, dtype=torch.float64, device=dev)
                k = int((world - torch.tensor(ph["segments"][v][0][0:3], device=dev)).norm(dim=1).argmin())
                seeds.append(v * side ** 3 + int((idx[k, 0] * side + idx[k, 1]) * side + idx[k, 2]))
            d0 = torch.full(cost.shape, math.inf, dtype=torch.float64, device=dev)
            d0.view(-1)[torch.tensor(seeds, device=dev)] = 0.0
            sweeps, runs_skip, runs_all = count_sweeps(cl, cost, bounds, d0)
            fixed, _ = cl.geodesic_distance(cost, bounds, init=d0)
            jacobi = scipy = "-"
            if n_vol == 1 or side <= 128:
                got = torch_jacobi(cost, h, d0)          # warm-up and the result
                ms = best_ms(lambda: torch_jacobi(cost, h, d0), 1 if side > 128 else args.passes)
                jacobi = f"{ms:.1f} ({got[1]}, {'yes' if torch.equal(got[0].view(torch.int64), fixed.view(torch.int64)) else 'no'})"
                del got
            if n_vol == 1:
                got = scipy_dijkstra(cost[0], h, seeds[0])
                ms = best_ms(lambda: scipy_dijkstra(cost[0], h, seeds[0]), args.passes)
                both = torch.isfinite(got) & torch.isfinite(fixed[0])
                same_reach = bool((torch.isfinite(got) == torch.isfinite(fixed[0])).all())
                scipy = f"{ms:.1f} ({float((got - fixed[0])[both].abs().max()):.2e}{'' if same_reach else ', reach differs'})"
            for skip in (True, False):
                cl.set_skip(skip)
                try:
                    cl.geodesic_distance(cost, bounds, init=d0, sweeps=sweeps)          # warm-up
                    exact = best_ms(lambda: cl.geodesic_distance(cost, bounds, init=d0, sweeps=sweeps), args.passes)
                    call = best_ms(lambda: cl.geodesic_distance(cost, bounds, init=d0), args.passes)
                finally:
                    cl.set_skip(True)
                runs = runs_skip if skip else runs_all
                lines.append(f"{side:>4}  {n_vol:>7}  {int(mask.sum()):>10}  {'on ' if skip else 'off'}   {sweeps:>5}  {1.0 - runs / runs_all:>14.4f}   {exact:>20.3f}  {call:>20.3f}  "
                             f"{20.0 * 2048 * runs / (exact * 1e-3) / 1e9:>7.1f}  {jacobi:<40} {scipy}")
                print(lines[-1], flush=True)
        vol = ph["dynamic"][0].contiguous()
        c = cl.extract(vol, bounds, threshold=0.25 * phantom.RHO_VESSEL)          # warm-up and the result
        ms = best_ms(lambda: cl.extract(vol, bounds, threshold=0.25 * phantom.RHO_VESSEL), args.passes)
        lines.append(f"{side:>4}  centreline.extract of phase 0: {ms:.1f} ms, {len(c.paths)} paths, {sum(int(p.numel()) for p in c.paths)} nodes, length {sum(c.length):.3f}, "
                     f"reached {c.reached:.4f}")
        print(lines[-1], flush=True)
        del ph
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
