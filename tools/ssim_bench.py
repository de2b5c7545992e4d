#!/usr/bin/env python3
"""Time of a mean SSIM and its gradient in the prediction against the expression a user of torch writes, in ONE process:

    ours       metrics.ssim(pred, truth, data_range=range).mean() and .backward(): nca_ssim forward, nca_ssim_grad backward (f64 arithmetic,
               f32 images)
    torch_f32  one grouped conv2d of the five maps (x, y, xx, yy, xy) with the outer product of the same window, the formula, .mean(),
               .backward() under autograd, in f32
    torch_f64  the same expression on images widened to f64 (the precision of ours)

on stacks of N = 4 and 40 images (4 views x 1 / 10 phases, the shapes of the other view benches) of 256 x 256 and 512 x 512 pixels, window
11, sigma 1.5.  Every leg is one warm-up pass and then three timed passes; the legs alternate.  A timed pass is --inner forward + backward
runs back to back ending in one device synchronise, and the report is milliseconds per run: best and worst pass, torch_f64 / ours and
torch_f32 / ours.  The two kernels' launches alone are timed with device events around --inner back-to-back launches, in GB/s of
algorithmic bytes: 8 per pixel for the value (both images read once), 12 per pixel for the gradient (both images read, one f32 written;
the 24 bytes per position of the coefficient maps that pass through the workspace are NOT counted).  The tool stops if ours differs from
torch_f64, in value or gradient, by more than torch_f32 differs from torch_f64.

    python3 tools/ssim_bench.py [--out profiles/ssim_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

IMAGE_COUNTS = (4, 40)
SIDES = (256, 512)
WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--inner", type=int, default=10, help="forward + backward runs per timed pass")
    ap.add_argument("--passes", type=int, default=3, help="timed passes per leg")
    return ap


def torch_ssim(x, y, rng, win):
    """Per-image mean SSIM [N] of stacks [N,H,W] in their own dtype, as a user writes it."""
    import torch
    w = torch.as_tensor(win, dtype=x.dtype, device=x.device)
    kern = torch.outer(w, w)[None, None].repeat(5, 1, 1, 1)
    maps = torch.stack([x, y, x * x, y * y, x * y], dim=1)
    mx, my, exx, eyy, exy = torch.nn.functional.conv2d(maps, kern, groups=5).unbind(1)
    rng = rng.to(x.dtype)[:, None, None]
    C1, C2 = (K1 * rng) ** 2, (K2 * rng) ** 2
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return S.mean(dim=(-2, -1))


def kernel_times(dev, x, y, rng, inner):
    """(ms per nca_ssim, ms per nca_ssim_grad): device events around `inner` back-to-back launches, after one warm-up launch of each."""
    import ctypes as C
    import torch
    from nerfca_amd import _capi, fused, metrics
    lib = _capi.lib()
    N, H, W = x.shape
    win = metrics.gaussian_window(WIN, SIGMA)
    cwin = (C.c_double * WIN)(*win.tolist())
    sums = torch.zeros(N, dtype=torch.float64, device=dev)
    scale = torch.full((N,), 1.0 / N, dtype=torch.float64, device=dev)
    g = torch.empty_like(x)
    nbytes = int(lib.nca_ssim_grad_workspace(N, H, W, WIN))
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    stream = fused._stream()

    def value():
        _capi.check_ssim(lib.nca_ssim(N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), WIN, cwin, K1, K2, _capi.ptr(sums), None, stream))

    def grad():
        _capi.check_ssim(lib.nca_ssim_grad(N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), WIN, cwin, K1, K2, _capi.ptr(scale), _capi.ptr(g), _capi.ptr(work),
                                           nbytes, stream))

    out = []
    with torch.cuda.device(dev):
        for fn in (value, grad):
            fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / inner)
    return out


def measure(dev, n_img, side, inner, passes):
    import torch
    from nerfca_amd import metrics
    from view_render_bench import timed
    gen = torch.Generator(device=dev).manual_seed(side + n_img)
    i, j = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(0.05 * i) * torch.cos(0.03 * j)
    truth = (0.8 * base[None] + 0.2 * torch.rand((n_img, side, side), generator=gen, device=dev)).float().contiguous()
    pred = (truth + 0.05 * (torch.rand((n_img, side, side), generator=gen, device=dev) - 0.5)).float().contiguous().requires_grad_()
    rng = truth.amax(dim=(-2, -1)).double() - truth.amin(dim=(-2, -1)).double()
    win = metrics.gaussian_window(WIN, SIGMA)
    pred64, truth64 = pred.detach().double().requires_grad_(), truth.double()

    def ours():
        pred.grad = None
        v = metrics.ssim(pred, truth, data_range=rng, win_size=WIN, sigma=SIGMA, k1=K1, k2=K2).mean()
        v.backward()
        return v.detach(), pred.grad

    def torch_f32():
        pred.grad = None
        v = torch_ssim(pred, truth, rng, win).mean()
        v.backward()
        return v.detach(), pred.grad

    def torch_f64():
        pred64.grad = None
        v = torch_ssim(pred64, truth64, rng, win).mean()
        v.backward()
        return v.detach(), pred64.grad

    legs = {"ours": ours, "torch_f32": torch_f32, "torch_f64": torch_f64}
    res = {}
    for k, fn in legs.items():          # the warm-up pass, and the agreement check
        v, g = fn()
        res[k] = (float(v), g.double().clone())
    scale = float(res["torch_f64"][1].abs().max())
    dist = {k: (abs(res[k][0] - res["torch_f64"][0]), float((res[k][1] - res["torch_f64"][1]).abs().max()) / scale) for k in ("ours", "torch_f32")}
    if not (dist["ours"][0] <= dist["torch_f32"][0] and dist["ours"][1] <= dist["torch_f32"][1]):
        sys.exit(f"ssim_bench: ours is further from the f64 torch leg than the f32 torch leg is ({n_img} x {side}^2: value {dist['ours'][0]:.3e} against "
                 f"{dist['torch_f32'][0]:.3e}, gradient {dist['ours'][1]:.3e} against {dist['torch_f32'][1]:.3e} of max |grad|)")
    del res
    times = {k: [] for k in legs}
    for _ in range(passes):
        for k, fn in legs.items():          # alternate the legs
            times[k].append(timed(lambda: [fn() for _ in range(inner)]) / inner)
    ms_value, ms_grad = kernel_times(dev, pred.detach(), truth, rng, inner)
    pixels = n_img * side * side
    rec = {"images": n_img, "side": side, "window": WIN, "runs_per_pass": inner,
           "value_distance_from_f64": {k: dist[k][0] for k in dist}, "grad_distance_from_f64_of_max": {k: dist[k][1] for k in dist}}
    for k in legs:
        rec[k] = {"best_ms": round(1e3 * min(times[k]), 4), "worst_ms": round(1e3 * max(times[k]), 4)}
    rec["f64_over_ours_best"] = round(rec["torch_f64"]["best_ms"] / rec["ours"]["best_ms"], 2)
    rec["f32_over_ours_best"] = round(rec["torch_f32"]["best_ms"] / rec["ours"]["best_ms"], 2)
    rec["kernel_value_ms"], rec["kernel_grad_ms"] = round(ms_value, 4), round(ms_grad, 4)
    rec["kernel_value_gbytes_per_s"] = round(8 * pixels / (ms_value * 1e-3) / 1e9, 1)
    rec["kernel_grad_gbytes_per_s"] = round(12 * pixels / (ms_grad * 1e-3) / 1e9, 1)
    return rec


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("ssim_bench needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lines = []
    for side in SIDES:
        for n_img in IMAGE_COUNTS:
            rec = measure(dev, n_img, side, args.inner, args.passes)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    table = ["milliseconds per forward + backward of the mean SSIM of N images (window 11), best / worst pass",
             "  N  side    ours ms                torch f32 ms           torch f64 ms           f64/ours  f32/ours   value kernel          gradient kernels"]
    for r in lines:
        cells = "".join(f"   {r[k]['best_ms']:>8.3f} / {r[k]['worst_ms']:<8.3f}" for k in ("ours", "torch_f32", "torch_f64"))
        table.append(f"{r['images']:>3}  {r['side']:>4} {cells}   {r['f64_over_ours_best']:>7.2f}  {r['f32_over_ours_best']:>7.2f}"
                     f"    {r['kernel_value_ms']:>7.4f} ms {r['kernel_value_gbytes_per_s']:>7.1f} GB/s   {r['kernel_grad_ms']:>7.4f} ms {r['kernel_grad_gbytes_per_s']:>7.1f} GB/s")
    slower = [f"{r['images']} x {r['side']}^2" for r in lines if r["ours"]["best_ms"] > r["torch_f64"]["best_ms"]]
    table.append("rows in which ours is slower than torch f64: " + (", ".join(slower) if slower else "none"))
    for r in lines:
        table.append(f"{r['images']:>3}  {r['side']:>4}   distance from torch f64: value ours {r['value_distance_from_f64']['ours']:.2e} / f32 {r['value_distance_from_f64']['torch_f32']:.2e}; "
                     f"gradient of max |grad| ours {r['grad_distance_from_f64_of_max']['ours']:.2e} / f32 {r['grad_distance_from_f64_of_max']['torch_f32']:.2e}")
    print("\n".join(table))
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
