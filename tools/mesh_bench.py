#!/usr/bin/env python3
"""Time of mesh.isosurface and of its two entry points beside the bytes each must move, in ONE process:

    count   nca_vol_iso_count alone (five launches: the per-node words, the three steps of the scan, the stack's bases)
    emit    nca_vol_iso_emit alone, into outputs sized from the totals (one launch)
    ours    mesh.isosurface(vol, level, bounds): both, with the workspace, the host read of the totals and the output tensors between them

on two volumes per size: `tree`, the vessel volume of phantom.make_phantom at a quarter of the vessel density (sparse: the surface crosses few
cells), and `noise`, a uniform random volume at 0.5 (dense: about half of all edges are crossed).  There is no other mesher among the
project's dependencies to race, so each time is set beside a floor instead: the bytes the pass must move over the rate a float4 copy reaches on the MI355X
(6.3 TB/s).  Per node N = n0 n1 n2, V vertices and T triangles:
    count   4 N (vol) + 2 N (the words, written) + 2 N + 2 N (read by the reduce and the add launches) + 8 N (both offsets, written) = 18 N
    emit    4 N (vol) + 2 N + 4 N + 4 N (the words and both offsets, read) + 12 V + 12 T (the outputs; + 12 V with normals)
The halo of a tile (37 % more nodes than the tile) comes from the L2 and is not counted.  Every leg is one warm-up pass and then `--passes`
timed passes; the legs alternate; a leg repeats its call inside a pass until the pass lasts about 0.2 s; a pass ends in one device
synchronise; the report is milliseconds per call, best and worst pass, and floor / best as the achieved fraction.  The microseconds per
launch come from one extra run of the whole call under the profiler of torch (kernel times by name).

    python3 tools/mesh_bench.py [--out profiles/mesh_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 6.3e12          # what a float4 copy reaches
KERNELS = ("count", "reduce", "scan", "bases", "add", "emit")


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    ap.add_argument("--sides", default="256", help="nodes per axis, comma separated")
    ap.add_argument("--volumes", default="1", help="volumes per stack, comma separated")
    ap.add_argument("--fields", default="tree,noise", help="tree, noise or both, comma separated")
    ap.add_argument("--normals", action="store_true", help="emit normals too")
    return ap


def kernel_us(call):
    """{launch: microseconds} of the six kernels from one run under torch's profiler; None where it sees no kernel of ours."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    us = {k: 0.0 for k in KERNELS}
    for e in prof.key_averages():
        for k in KERNELS:
            if f"iso_{k}_kernel" in e.key:
                us[k] += float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
    return {k: round(v, 1) for k, v in us.items()} if sum(us.values()) > 0 else None


def floors(nodes, n_vert, n_tri, normals):
    """(bytes of count, bytes of emit) as the docstring counts them."""
    return 18 * nodes, 14 * nodes + 12 * n_vert + 12 * n_tri + (12 * n_vert if normals else 0)


def measure(dev, kind, side, n_vol, passes, normals):
    import torch
    from filt_bench import run_legs
    from nerfca_amd import _capi, _view, mesh, phantom, synthetic
    if kind == "tree":
        vol = phantom.make_phantom((side,) * 3, n_vol, synthetic.xcat_geometry(128), device=dev)["dynamic"].contiguous()
        level = 0.25 * phantom.RHO_VESSEL
    else:
        vol = torch.rand((n_vol,) + (side,) * 3, generator=torch.Generator(device=dev).manual_seed(31 * side + n_vol), device=dev)
        level = 0.5
    bounds = ((-1.0, 1.0),) * 3
    lib = _capi.lib()
    desc, x, _, _ = _view.volume_stack(vol, "mesh_bench", bounds)
    nbytes = int(lib.nca_vol_iso_workspace(C.byref(desc), n_vol))
    work = _view.workspace(nbytes, dev)
    totals = torch.empty((n_vol, 2), dtype=torch.int64, device=dev)

    def count():
        _view.launch(_capi.check_mesh, lib.nca_vol_iso_count, dev, C.byref(desc), _capi.ptr(x), n_vol, level, _capi.ptr(totals), _capi.ptr(work), nbytes)

    count()
    n_vert, n_tri = (int(v) for v in totals.sum(0).tolist())
    verts = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_tri, 3), dtype=torch.int32, device=dev)
    norm = torch.empty((n_vert, 3), dtype=torch.float32, device=dev) if normals else None

    def emit():
        _view.launch(_capi.check_mesh, lib.nca_vol_iso_emit, dev, C.byref(desc), _capi.ptr(x), n_vol, level, _capi.ptr(work), nbytes, n_vert, n_tri, _capi.ptr(verts),
                     _capi.ptr(faces), _capi.ptr(norm))

    def ours():
        return mesh.isosurface(vol, level, bounds, normals=normals)

    tag = f"{kind} {side}^3 x {n_vol}"
    got, res = run_legs({"count": count, "emit": emit, "ours": ours}, passes, (), tag)
    whole = res["ours"]
    if sum(m.verts.shape[0] for m in whole) != n_vert or sum(m.faces.shape[0] for m in whole) != n_tri:
        sys.exit(f"mesh_bench: mesh.isosurface and the raw entry points disagree on the totals at {tag}")
    nodes = n_vol * side ** 3
    b_count, b_emit = floors(nodes, n_vert, n_tri, normals)
    rec = {"field": kind, "side": side, "volumes": n_vol, "normals": normals, "vertices": n_vert, "triangles": n_tri, "workspace_bytes": nbytes, **got}
    for leg, b in (("count", b_count), ("emit", b_emit), ("ours", b_count + b_emit)):
        floor_ms = 1e3 * b / HBM_BYTES_PER_S
        rec[leg].update(bytes=b, floor_ms=round(floor_ms, 4), fraction_of_floor=round(floor_ms / rec[leg]["best_ms"], 4))
    try:
        rec["kernel_us"] = kernel_us(ours)
    except Exception as e:          # the profiler is a convenience: the times above do not depend on it
        rec["kernel_us"] = None
        rec["kernel_us_failed"] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
    return rec


def table_of(lines):
    table = ["milliseconds per call, best / worst pass; floor: the bytes of the pass at 6.3 TB/s; fraction: floor / best",
             "field  side  vols  vertices    triangles   | count ms (floor, fraction)                | emit ms (floor, fraction)                 | isosurface ms (floor, fraction) | microseconds per launch: " + " ".join(KERNELS)]
    for r in lines:
        def cell(k):
            return f"{r[k]['best_ms']:>9.3f} / {r[k]['worst_ms']:<9.3f} ({r[k]['floor_ms']:.3f}, {r[k]['fraction_of_floor']:.3f})"
        table.append(f"{r['field']:<5}  {r['side']:>4}  {r['volumes']:>4}  {r['vertices']:>10}  {r['triangles']:>10}  | {cell('count')} | {cell('emit')} | {cell('ours')} | "
                     + (" ".join(f"{r['kernel_us'][k]:.1f}" for k in KERNELS) if r.get("kernel_us") else "-"))
    return table


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for kind in (k.strip() for k in args.fields.split(",")):
        if kind not in ("tree", "noise"):
            sys.exit(f"mesh_bench: --fields {kind!r} is neither tree nor noise")
        for side in (int(s) for s in args.sides.split(",")):
            for n_vol in (int(p) for p in args.volumes.split(",")):
                rec = measure(dev, kind, side, n_vol, args.passes, args.normals)
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
