#!/usr/bin/env python3
"""Time of ccta.vesselness against the torch expression a user would write on the same device, in ONE process:

    ours        ccta.vesselness(vol, sigmas) with Frangi's c: per scale one gaussian_filter, one nca_vol_hessian_norm_max and one
                nca_vol_vesselness (csrc/view/nca_vess.hip)
    torch f64   per scale the same gaussian_filter, then sliced second differences of the edge-padded volume, torch.linalg.eigvalsh of the
    torch f32   [nodes, 3, 3] Hessians, a sort by absolute value and Frangi's formula, in f64 and in f32; the maximum over the scales

at 128^3 and 256^3 nodes, 1 and 10 volumes, three scales, on two kinds of data: "phantom", the vessel volume of phantom.make_phantom, which
is 0 at most nodes -- there the Hessian is 0, every rotation of the solver is skipped by whole waves and the launch costs little more than
its bytes; and "noisy", the same volume plus Gaussian noise of 2 % of the vessel density at every node, as a CT has -- there every node
pays the full solver.  The second is the cost to plan with.  The torch legs ALWAYS run on ONE
volume of the stack: the expression holds some 200 bytes per node in f64, so a user loops over the volumes; the table compares
milliseconds per volume.  Before a torch leg runs at a size it is timed once at 32^3, and when that predicts more than --torch-budget
seconds for the leg's passes it is not run and the row says so.  Every leg is one warm-up pass and then `--passes` timed passes; the legs
alternate.  A leg repeats its call inside a pass until the pass lasts about 0.2 s; a pass ends in one device synchronise; the report is
milliseconds per call, best and worst pass.

The parts of our call are timed the same way on their own: the smoothings, the norm-max launches and the vesselness launches of the three
scales (the last two on volumes smoothed beforehand).  Algorithmic bytes: a vesselness launch reads 4 and writes 4 bytes per node, 8 per
node and scale; the GB/s columns are those bytes over the best time of the vesselness launches alone and of the whole call.
Agreement: the largest difference between ours and the f64 torch expression on the first volume is reported.  The yardstick is the torch
expression: a row in which ours is slower is reported as it is.

    python3 tools/vess_bench.py [--out profiles/vess_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vesselness import parse_sigmas  # noqa: E402

ALPHA = BETA = 0.5


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default="128,256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1,10", help="volumes per stack, comma separated")
    ap.add_argument("--sigmas", type=parse_sigmas, default=[1.0, 2.0, 3.0], help="scales in nodes, comma separated")
    ap.add_argument("--torch-budget", type=float, default=40.0, help="seconds a torch leg may take at one size, predicted from 32^3")
    return ap


def torch_vesselness(vol, sigmas, dtype):
    """The expression on one f32 volume [n0, n1, n2] on the device; the smoothing is ccta.gaussian_filter."""
    import torch
    import torch.nn.functional as F
    from nerfca_amd import ccta
    best = None
    for sigma in sigmas:
        s = ccta.gaussian_filter(vol, sigma).to(dtype)
        p = F.pad(s[None, None], (1, 1, 1, 1, 1, 1), mode="replicate")[0, 0]
        n0, n1, n2 = s.shape

        def at(d0, d1, d2):
            return p[1 + d0:1 + d0 + n0, 1 + d1:1 + d1 + n1, 1 + d2:1 + d2 + n2]

        sc = sigma * sigma
        h00 = sc * (at(1, 0, 0) - 2 * s + at(-1, 0, 0))
        h11 = sc * (at(0, 1, 0) - 2 * s + at(0, -1, 0))
        h22 = sc * (at(0, 0, 1) - 2 * s + at(0, 0, -1))
        h01 = sc * 0.25 * (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0))
        h02 = sc * 0.25 * (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1))
        h12 = sc * 0.25 * (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1))
        H = torch.stack([h00, h01, h02, h01, h11, h12, h02, h12, h22], dim=-1).reshape(-1, 3, 3)
        del h00, h01, h02, h11, h12, h22, p
        w = torch.linalg.eigvalsh(H)
        del H
        w = torch.gather(w, 1, w.abs().argsort(dim=1))
        l1, l2, l3 = w[:, 0], w[:, 1], w[:, 2]
        s2 = l1 * l1 + l2 * l2 + l3 * l3
        c = 0.5 * torch.sqrt(s2.max())
        V = (1 - torch.exp(-(l2 / l3) ** 2 / (2 * ALPHA ** 2))) * torch.exp(-l1 * l1 / (l2 * l3).abs() / (2 * BETA ** 2)) * (1 - torch.exp(-s2 / (2 * c * c)))
        V = torch.where((l2 < 0) & (l3 < 0), V, torch.zeros((), dtype=dtype, device=V.device)).reshape(n0, n1, n2)
        best = V if best is None else torch.maximum(best, V)
    return best.to(torch.float32)


def raw_parts(vol, sigmas):
    """The norm-max and the vesselness launches of ccta.vesselness on their own, on volumes smoothed beforehand: two callables."""
    import torch
    from nerfca_amd import _capi, _view, ccta
    desc, x, n_vol, _ = _view.volume_stack(vol, "vess_bench")
    smoothed = [ccta.gaussian_filter(x, s) for s in sigmas]
    c = torch.empty(n_vol, dtype=torch.float64, device=x.device)
    out = torch.empty_like(x)
    lib = _capi.lib()

    def norm_max():
        for s, sigma in zip(smoothed, sigmas):
            _view.launch(_capi.check_vess, lib.nca_vol_hessian_norm_max, x.device, C.byref(desc), _capi.ptr(s), n_vol, sigma * sigma, _capi.ptr(c))

    norm_max()
    c_fixed = 0.5 * torch.sqrt(c)          # the last scale's: the time does not depend on the value

    def vess():
        for i, (s, sigma) in enumerate(zip(smoothed, sigmas)):
            _view.launch(_capi.check_vess, lib.nca_vol_vesselness, x.device, C.byref(desc), _capi.ptr(s), n_vol, sigma * sigma, ALPHA, BETA, _capi.ptr(c_fixed), 1, i,
                         _capi.ptr(out), None)

    return norm_max, vess


_PROBE = {}          # dtype -> seconds of one call at the probe size, or why it failed


def predicted_seconds(dev, dtype, side, sigmas, passes, memo=_PROBE, probe=32):
    """Seconds the passes of a torch leg would take at side^3, from one timed call at 32^3 (after a warm-up call), scaled by the nodes."""
    import torch
    from nerfca_amd import phantom, synthetic
    from view_render_bench import timed
    if dtype not in memo:
        small = phantom.make_phantom((probe,) * 3, 1, synthetic.xcat_geometry(128), device=dev)["dynamic"][0].contiguous()
        try:
            torch_vesselness(small, sigmas, dtype)
            memo[dtype] = timed(lambda: torch_vesselness(small, sigmas, dtype))
        except Exception as e:          # a baseline torch cannot run here
            memo[dtype] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
    if isinstance(memo[dtype], str):
        return memo[dtype]
    return memo[dtype] * (side / probe) ** 3 * (passes + 2)


def measure(dev, side, n_vol, sigmas, passes, budget, data):
    import torch
    from filt_bench import run_legs
    from nerfca_amd import ccta, phantom, synthetic
    vol = phantom.make_phantom((side,) * 3, n_vol, synthetic.xcat_geometry(128), device=dev)["dynamic"].contiguous()
    if data == "noisy":
        vol = vol + 0.02 * phantom.RHO_VESSEL * torch.randn(vol.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(side + n_vol))
    nodes = n_vol * side ** 3
    tag = f"{data} {side}^3 x {n_vol}"
    norm_max, vess = raw_parts(vol, sigmas)
    legs = {"ours": lambda: ccta.vesselness(vol, sigmas), "smooth": lambda: [ccta.gaussian_filter(vol, s) for s in sigmas], "norm_max": norm_max, "vess": vess}
    skipped = {}
    for name, dtype in (("torch_f64", torch.float64), ("torch_f32", torch.float32)):
        est = predicted_seconds(dev, dtype, side, sigmas, passes)
        if isinstance(est, str):
            skipped[name] = {"failed": est}
        elif est > budget:
            skipped[name] = {"failed": f"not run: {est:.0f} s predicted from 32^3 for {passes + 2} calls on one volume, above the budget of {budget:.0f} s"}
        else:
            legs[name] = lambda dtype=dtype: torch_vesselness(vol[0], sigmas, dtype)
    got, res = run_legs(legs, passes, (), tag)
    got.update(skipped)
    rec = {"data": data, "side": side, "volumes": n_vol, "scales": len(sigmas), "vesselness_max": float(res["ours"].max()), **got}
    if "torch_f64" in res:
        d = (res["ours"][0] - res["torch_f64"]).abs()
        rec["largest_difference_from_torch_f64"] = float(d.max())
        rec["nodes_differing_by_1e-4"] = int((d > 1e-4).sum())
    algo = 8 * len(sigmas) * nodes
    rec["vess_gbytes_per_s"] = round(algo / (got["vess"]["best_ms"] * 1e-3) / 1e9, 1)
    rec["ours_gbytes_per_s"] = round(algo / (got["ours"]["best_ms"] * 1e-3) / 1e9, 1)
    return rec


def table_of(lines):
    """The report: one row per size; the torch legs per volume."""
    table = ["milliseconds per call, best / worst pass; ours and its parts on the whole stack, the torch legs on ONE volume of it",
             "data     side  vols   ours ms                  smoothing ms   norm-max ms   vesselness ms   share s / n / v   vess GB/s  call GB/s   torch f64 ms/vol   torch f32 ms/vol   "
             "f64/ours  f32/ours (per volume)"]
    slower, notes = [], []
    for r in lines:
        ours = r["ours"]["best_ms"]
        parts = [r[k]["best_ms"] for k in ("smooth", "norm_max", "vess")]
        share = " / ".join(f"{100 * p / sum(parts):.0f}" for p in parts)
        cells, ratios = [], []
        for k in ("torch_f64", "torch_f32"):
            if "best_ms" in r[k]:
                cells.append(f"{r[k]['best_ms']:>16.3f}")
                ratios.append(f"{r[k]['best_ms'] / (ours / r['volumes']):>8.1f}")
                if ours / r["volumes"] > r[k]["best_ms"]:
                    slower.append(f"{r['data']} {r['side']}^3 x {r['volumes']} against {k}")
            else:
                cells.append(f"{'-':>16}")
                ratios.append(f"{'-':>8}")
                notes.append(f"      {k} at {r['data']} {r['side']}^3 x {r['volumes']}: {r[k]['failed']}")
        table.append(f"{r['data']:<7}  {r['side']:>4}  {r['volumes']:>4}  {ours:>10.3f} / {r['ours']['worst_ms']:<10.3f}   {parts[0]:>10.3f}   {parts[1]:>10.3f}   {parts[2]:>12.3f}   {share:>15}   "
                     f"{r['vess_gbytes_per_s']:>9.1f}  {r['ours_gbytes_per_s']:>9.1f}   {cells[0]}   {cells[1]}   {ratios[0]}  {ratios[1]}")
        if "largest_difference_from_torch_f64" in r:
            notes.append(f"      agreement at {r['data']} {r['side']}^3 x {r['volumes']}: largest |ours - torch f64| on the first volume {r['largest_difference_from_torch_f64']:.3e}, "
                         f"{r['nodes_differing_by_1e-4']} nodes differ by more than 1e-4")
    table += notes
    table.append("rows in which ours is slower per volume than a torch leg: " + (", ".join(slower) if slower else "none"))
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("vess_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for data in ("phantom", "noisy"):
        for side in (int(s) for s in args.sides.split(",")):
            for n_vol in (int(p) for p in args.volumes.split(",")):
                rec = measure(dev, side, n_vol, args.sigmas, args.passes, args.torch_budget, data)
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
