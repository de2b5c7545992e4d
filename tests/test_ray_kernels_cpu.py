"""The inputs of test_ray_kernels_gpu.py really are what those tests rely on.  Evaluated with the oracle alone, on the CPU, so that a
failure on the GPU cannot be blamed on the inputs: every class of ray is present, every value is far from the thresholds the loss
kernel branches on, the oracle's gradients are finite in f32 and in f64, and the f32 oracle is within 1e-4 of the f64 oracle on every
ray but those of the two classes where the reference's own f32 arithmetic is ill-conditioned."""
import math

import numpy as np
import pytest
import torch

import ray_kernel_cases as K

LOSS_CASES = [(R, S, skew) for (R, S) in K.LOSS_SHAPES for skew in K.SKEWS]


@pytest.mark.parametrize("R,S,skew", LOSS_CASES)
def test_loss_case_is_what_the_gpu_tests_rely_on(R, S, skew):
    c = K.loss_case(R, S, skew)
    assert c.sig_s.dtype == torch.float32 and c.sig_s.shape == (R, S) and c.dists.dtype == torch.float64 and c.dists.shape == (S,)
    assert float(c.dists[-1]) == 1e-10 and bool((c.dists > 0).all())
    # every class is there, on the ray the builder says
    if R >= 8:
        assert set(c.cls) == set(K.CLASSES[:8 if R == 8 else 9]) and c.cls[1:8] == K.CLASSES[1:8]
        assert not c.sig_d[1].any() and not c.sig_d[2].any() and not c.sig_s[3].any()
        assert int((c.sig_d[5] == 0).sum()) == (S + 2) // 3 and int((c.sig_s[6] == 0).sum()) == (S + 3) // 4
        assert not ((c.sig_s == 0) & (c.sig_d == 0)).any()
    else:
        assert set(c.cls) == {"ordinary"}
    # ray sums: 0, or above 1e-17 (far from the 1e-19 clip), and a factor of 2 from mask_thre; the dynamic sum of the one clipped_dyn ray
    # is below the clip, a factor of 2 away from it as well, and not 0
    clipped = torch.tensor([k == "clipped_dyn" for k in c.cls])
    for sig in (c.sig_s, c.sig_d):
        M = (sig.double() * c.dists).sum(-1)
        below = clipped & (M > 1e-21) & (M < 5e-20) if sig is c.sig_d else torch.zeros(R, dtype=torch.bool)
        assert bool(((M == 0) | (M > 1e-17) | below).all()), M.min()
        assert sig is c.sig_s or bool(below[clipped].all())
        assert bool(((M < K.MASK_THRE / 2) | (M > K.MASK_THRE * 2)).all())
    if R >= 8:
        Md = (c.sig_d.double() * c.dists).sum(-1)
        assert Md[1] == 0 and Md[2] == 0 and Md[4] < K.MASK_THRE / 2
        assert c.wpix[1] == 1.0 and c.wpix[2] == 1.5 and c.wpix[7] == 1.5 and (R == 8 or c.wpix[8] == 1.5)
    assert bool(((c.wpix - (1 + K.WEIGHTED_THRESH)).abs() >= 0.005).all())
    ordinary = [r for r, k in enumerate(c.cls) if k == "ordinary"]
    assert bool((c.wpix[ordinary] >= 1.0).all()) and bool((c.wpix[ordinary] <= 1.02).all())
    assert float(c.sig_s[ordinary].min()) >= 0.002 and float(c.sig_s[ordinary].max()) <= 0.02


@pytest.mark.parametrize("R,S,skew", LOSS_CASES)
def test_oracle_gradients_are_finite_and_f32_is_close_to_f64(R, S, skew):
    """floor_r = max_s |g32 - g64| / max_s |g64| <= 1e-4 on every ray outside K.ILL_CONDITIONED (measured: 9e-6 or better; the two
    excepted classes 0.36 .. 0.96 in g_sigma_s, where f32 rounds b = vd / (vd + 1e-10) to 1.0: a property of the reference)."""
    c = K.loss_case(R, S, skew)
    o32, o64 = K.oracle_loss(R, S, skew, torch.float32), K.oracle_loss(R, S, skew, torch.float64)
    pairs = [("g_sigma_s", o32.g_s, o64.g_s), ("g_sigma_d", o32.g_d, o64.g_d)]
    if (R, S) in K.TERM_GRAD_SHAPES:
        _, s32, d32 = K.oracle_terms(R, S, skew, torch.float32)
        _, s64, d64 = K.oracle_terms(R, S, skew, torch.float64)
        pairs += [("terms g_sigma_s", s32, s64), ("terms g_sigma_d", d32, d64)]
    for o in (o32, o64):
        assert all(math.isfinite(v) for v in o.terms.values()), o.terms
        assert bool(torch.isfinite(o.g_pix).all())
    for name, g32, g64 in pairs:
        assert bool(torch.isfinite(g32).all()) and bool(torch.isfinite(g64).all()), name
        floor = K.row_err(g32, g64)
        worst = K.class_margins(floor, c.cls)
        print(f"floor {name} R={R} S={S} skew={skew}: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
        bad = [(r, c.cls[r], float(floor[r])) for r in range(R) if c.cls[r] not in K.ILL_CONDITIONED and not floor[r] <= 1e-4]
        assert not bad, (name, bad[:5])
    if (R, S) in K.DISTS_GRAD_SHAPES:
        for unit_mse in (False, True):
            for dt in (torch.float32, torch.float64):
                assert bool(torch.isfinite(K.oracle_loss(R, S, skew, dt, unit_mse, True).g_dists).all())


def test_zero_dynamic_ray_would_hide_the_batch_under_a_max_norm():
    """Why the gradients are measured per ray: the weighted ray without a dynamic field has g_sigma_d entries ~1e18 times the others'."""
    o = K.oracle_loss(9, 65, 1.0, torch.float64)
    big = o.g_d[2].abs().max()
    assert big > 1e15 and o.g_d[[0, 1, 3, 4, 5, 6, 7]].abs().max() < 1e-12 * big


@pytest.mark.parametrize("R,S", K.COMPOSITE_SHAPES)
def test_composite_case_is_what_the_gpu_tests_rely_on(R, S):
    c = K.composite_case(R, S)
    assert c.raw_s.dtype == torch.float32 and c.raw_s.shape == (R, S) and c.raw_d.shape == (R, S)
    raws = (c.raw_s, c.raw_d)
    for f, r, s, x in c.planted:
        assert float(raws[f][r, s]) == x and any(np.float32(p) == np.float32(x) for p in K.PLANTED)
        assert not (20 - 1e-3 < x < 20) and abs(x - K.X_CLAMP) >= 1e-3
    if R * S >= 4 * len(K.PLANTED) * max(1, S // len(K.PLANTED)):
        for f in (0, 1):        # every planted value is in both fields
            assert {np.float32(x) for ff, _, _, x in c.planted if ff == f} == {np.float32(p) for p in K.PLANTED}
    # the softplus threshold is hit from both sides, and no value at all is so close to the clamp's corner that f32 and f64 could disagree
    # about the side
    assert np.float32(K.PLANTED[0]) == 20 and np.float32(K.PLANTED[1]) > 20 and np.float32(K.PLANTED[1]) - np.float32(20) < 3e-6
    for raw in raws:
        assert float((raw.double() - K.X_CLAMP).abs().min()) > 1e-5
    for act in ("softplus", "clamp", "Softplus"):
        for single in (False, True):
            for scale in (1e-2, 1.0):
                for dt in (torch.float32, torch.float64):
                    o = K.oracle_composite(R, S, act, single, scale, dt)
                    assert all(bool(torch.isfinite(t).all()) for t in (o.pix, o.sig_s, o.g_s))


def test_adam_closed_form_is_torch_adam():
    """The numpy f64 Adam + LinearLR the GPU test compares with, against torch.optim.Adam in f64 over the same seven steps."""
    n = 1000
    grads = K.adam_gradients(n, 7, 5)
    assert all(not g[K.zero_slice(n)].any() for g in grads) and all(g.dtype == np.float32 for g in grads)
    ups, lrs = K.adam_updates_f64(grads)
    assert lrs[0] == 1e-2 and abs(lrs[4] - 1e-3) < 1e-18 and lrs[4] == lrs[6] and lrs[1] > lrs[2] > lrs[3] > lrs[4]
    p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-2)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1, end_factor=0.1, total_iters=4)
    for g, u, lr in zip(grads, ups, lrs):
        before = p.detach().clone()
        p.grad = torch.from_numpy(g).double()
        opt.step()
        sched.step()
        err = float(((p.detach() - before).numpy() - u).__abs__().max()) / lr
        assert err < 1e-12, err
    f32 = K.adam_updates_torch_f32(torch.zeros(n), grads)
    assert max(float(np.abs(a - b).max()) / lr for a, b, lr in zip(f32, ups, lrs)) < 2e-6
