#!/usr/bin/env python3
"""Step time of the static-only loop (train/run_nerf.py, BASELINE configs[0]) in its three forms, in ONE process:

    StaticTrainer.step        autograd, torch loss operations, torch.optim.Adam, host gather and window update
    StaticTrainer.step_fused  no autograd graph, HIP loss kernel (nca_static_loss_fwd_bwd), torch.optim.Adam
    StaticTrainer.step_graph  one captured HIP graph (begin_step, forward, loss, backward, library Adam), no host work per step

at 1 024 rays x 64 samples and 16 384 x 64 (one 128^2 detector: configs[0]'s shape), f32 and bf16, synthetic.net_definitions' default
net.  Every leg is 20 warm-up steps and >= 200 timed steps ending in a device synchronise, stretched so that a leg lasts >= 0.5 s; the
three variants alternate and each runs three times.  Reports best and spread per variant and the ratio step / step_graph; the
acceptance line is "step_graph's worst of three below step's best of three".

    python3 tools/static_step_bench.py [--out FILE]                 # the table (one JSON line per configuration, then a text table)
    python3 tools/static_step_bench.py --trace-leg --prec bf16      # only the 16 384 x 64 graph leg: the program of a
                                                                    # `rocprofv3 --kernel-trace --stats -- python3 ...` run
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WARMUP, MIN_STEPS, MIN_SECONDS, REPEATS = 20, 200, 0.5, 3
VARIANTS = ("step", "step_fused", "step_graph")
SIZES = ((1024, 64), (16384, 64))


def make_trainer(data, dev, prec, rays, samples):
    from nerfca_amd import set_precision, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.train.trainer import StaticTrainer, TrainConfig
    torch.manual_seed(1)
    s = CPPN(synthetic.net_definitions(dev)[0]).to(dev)
    set_precision(prec, s)
    cfg = TrainConfig(depth_samples_per_ray_coarse=samples, img_sample_size=rays)
    return StaticTrainer(cfg, s, data, dev, seed=3)


def leg(fn, it0, n):
    """``n`` consecutive steps from iteration ``it0``, ending in a device synchronise: seconds per step."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(it0, it0 + n):
        fn(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def measure(data, dev, prec, rays, samples):
    trainers = {v: make_trainer(data, dev, prec, rays, samples) for v in VARIANTS}
    fns = {v: getattr(trainers[v], v) for v in VARIANTS}
    nxt = {v: 0 for v in VARIANTS}
    steps = {}
    for v in VARIANTS:                       # warm-up (code objects, the graph's capture), then size the legs
        leg(fns[v], 0, WARMUP)
        nxt[v] = WARMUP
        per = leg(fns[v], nxt[v], 50)
        nxt[v] += 50
        steps[v] = max(MIN_STEPS, int(math.ceil(1.2 * MIN_SECONDS / per)))
    times = {v: [] for v in VARIANTS}
    for _ in range(REPEATS):
        for v in VARIANTS:                   # alternate the variants
            leg(fns[v], nxt[v], WARMUP)
            nxt[v] += WARMUP
            times[v].append(leg(fns[v], nxt[v], steps[v]))
            nxt[v] += steps[v]
    assert getattr(trainers["step_graph"], "_graph", None) is not None, "step_graph did not replay a graph"
    rec = {"prec": prec, "rays": rays, "samples": samples, "timed_steps": steps, "leg_seconds": {v: [round(t * steps[v], 3) for t in times[v]] for v in VARIANTS}}
    for v in VARIANTS:
        ms = [1e3 * t for t in times[v]]
        rec[v] = {"best_ms": round(min(ms), 4), "worst_ms": round(max(ms), 4), "spread_pct": round(100 * (max(ms) - min(ms)) / min(ms), 2)}
    rec["ratio_step_over_graph_best"] = round(rec["step"]["best_ms"] / rec["step_graph"]["best_ms"], 3)
    rec["ratio_step_over_fused_best"] = round(rec["step"]["best_ms"] / rec["step_fused"]["best_ms"], 3)
    rec["graph_worst_below_step_best"] = rec["step_graph"]["worst_ms"] < rec["step"]["best_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--trace-leg", action="store_true", help="run only the 16 384 x 64 graph leg (under a kernel trace)")
    ap.add_argument("--prec", default="bf16", choices=("f32", "bf16"), help="precision of --trace-leg")
    ap.add_argument("--n-det", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("static_step_bench needs the GPU: there is nothing to time without one")
    from nerfca_amd import synthetic
    dev = torch.device("cuda:0")
    data = synthetic.make_dataset(args.n_det, 64, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    if args.trace_leg:
        rays, samples = SIZES[-1]
        tr = make_trainer(data, dev, args.prec, rays, samples)
        leg(tr.step_graph, 0, WARMUP)
        per = leg(tr.step_graph, WARMUP, MIN_STEPS)
        print(json.dumps({"trace_leg": "step_graph", "prec": args.prec, "rays": rays, "samples": samples, "steps": MIN_STEPS, "ms_per_step_under_trace": round(1e3 * per, 4)}))
        return
    lines = []
    for prec in ("f32", "bf16"):
        for rays, samples in SIZES:
            rec = measure(data, dev, prec, rays, samples)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    table = ["prec  rays x samples   step best/worst ms   step_fused best/worst ms   step_graph best/worst ms   step/graph   graph worst < step best"]
    for r in lines:
        table.append(f"{r['prec']:<5} {r['rays']:>6} x {r['samples']:<4}   {r['step']['best_ms']:>8.3f} / {r['step']['worst_ms']:<8.3f}"
                     f"   {r['step_fused']['best_ms']:>8.3f} / {r['step_fused']['worst_ms']:<8.3f}      {r['step_graph']['best_ms']:>8.3f} / {r['step_graph']['worst_ms']:<8.3f}"
                     f"     {r['ratio_step_over_graph_best']:>6.2f}       {r['graph_worst_below_step_best']}")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
