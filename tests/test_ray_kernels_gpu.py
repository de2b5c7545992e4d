"""The per-ray kernels of csrc/nca_kernels_loss.hip -- the fused loss, the static loss, the stand-alone compositing, the library Adam --
run directly at every shape and value where they branch, against the project's oracle in f64 (the same oracle in f32 is the noise
floor).  The inputs come from ray_kernel_cases.py; test_ray_kernels_cpu.py checks, with the oracle alone, that they are what these tests
rely on.

Branches reached (none of them is reached by the golden inputs of test_hip_parity.py, 20 x 48 and 12 x 24):
  * R mod 4 = 1, 2, 3: the ragged last block of the one-wave-per-ray kernels; S = 1, 63, 64, 65: lane loops of 1 and 2 trips
  * S = 512, 513, 577, 1100: the q values of the ray entropy kept in registers (up to 512 samples) / recomputed beyond, in the
    weighted-loss mode and in term-gradient mode (the static field's twin of the loop)
  * R = 4101: 1026 blocks, a second trip of the finishing kernel; R = 300, 4101: 2 and 17 trips of the dists sum
  * ray sums of exactly 0 and of 2e-20 (clip(M, 1e-19) active, with and without the entropy mask; below the clip without being 0 is
    where d clip(M) / dM = 0 changes the gradient), blend weights of exactly 0, of 1e-18 (its square below the 1e-19 clip) and, in f32, 1
  * softplus beyond its threshold of 20, the clamp's flat arms, exp under- and overflow
  * Adam: segments beyond 64 workgroups x 1024 elements (several trips of the grid-stride loop, with a tail), unequal segments

Gradients over [R, S] are measured per ray (ray_kernel_cases.row_err).  A ray passes if it is within 1e-5 of the f32 oracle or within
max(1e-5, 3 floor_r) of the f64 oracle, floor_r being the f32 oracle's own distance from the f64 oracle on that ray: the suite's rule,
per row.  Every test prints its margins (pytest -s).

Measured on an MI355X, worst e64_r / max(1e-5, 3 floor_r) per class over all cases (1 = the bound; 0.33 = the kernel IS the f32 oracle on a
ray where that oracle is far from f64):
                       ordinary  zero_dyn_masked  zero_dyn_weighted  zero_static  below_mask  zero_dyn_samples  zero_static_samples  weighted  clipped_dyn
  loss  g_sigma_s       6.5e-2       5.5e-3           5.5e-3           0.33        5.8e-2        5.2e-2             0.33           6.8e-2     5.5e-3
  loss  g_sigma_d       0.13         4.2e-3           2.9e-3           0.35        2.3e-2        5.5e-3             0.23           1.3e-2     4.2e-3
  terms g_sigma_s       1.8e-2       5.1e-3           5.3e-3           0.33        4.6e-2        1.7e-2             0.33           2.1e-2     4.8e-3
  terms g_sigma_d       1.0e-2       2.0e-2           2.9e-3           0.33        1.5e-2        1.0e-2             0.20           1.2e-2     4.1e-3
  compositing (rays with planted samples / without): pix 3.7e-3 / 7.9e-3, sigma_s 0.33 / 1.6e-2, sigma_d 1.3e-2 / 1.6e-2, g_raw_s 0.33 / 0.34,
  g_raw_d 0.33 / 0.34; dists gradient <= 7e-8 of its bound; static sums <= 1 ulp; Adam 2.96e-5 lr against a bound of 8.9e-5 lr (0.33: the
  rounding of p - step to f32, the same in torch's f32 Adam).

Arithmetic-only changes of the kernels that these tests catch and the tests of test_hip_parity.py on the golden inputs do not: q without
pd / (pd + eps) in either recompute loop beyond 512 samples; d clip(M) / dM = 1 below the clip; partials of blocks >= 1024 added twice.
"""
import numpy as np
import pytest
import torch

import ray_kernel_cases as K
from conftest import rel_err
from nca_testlib import dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -53
LOSS_CASES = [(R, S, skew) for (R, S) in K.LOSS_SHAPES for skew in K.SKEWS]
_cache = {}


def _fused(dev, R, S, skew):
    """fused_losses on loss_case(R, S, skew), once per case: (terms, g_pix, g_sigma_s, g_sigma_d) on the CPU."""
    key = ("loss", R, S, skew)
    if key not in _cache:
        from nerfca_amd.fused import fused_losses
        c = K.loss_case(R, S, skew)
        out = fused_losses(c.pix.to(dev), c.gt.to(dev), c.wpix.to(dev), c.sig_s.to(dev), c.sig_d.to(dev), c.dists.to(dev), c.run_args, K.WEIGHTS)
        _cache[key] = tuple(t.cpu() for t in out)
    return _cache[key]


def _check_rows(what, cls, got, g32, g64):
    """The per-ray rule on one gradient; prints the worst margin e64_r / max(1e-5, 3 floor_r) per class."""
    ok, e32, e64, floor, margin = K.rows_pass(got, g32, g64)
    print(f"margin {what}: " + "  ".join(f"{k} {v:.1e}" for k, v in K.class_margins(margin, cls).items()))
    zero_rows = g64.abs().amax(-1) == 0
    assert not bool(got.cpu()[zero_rows].any()), what
    bad = [(r, cls[r], float(e32[r]), float(e64[r]), float(floor[r])) for r in range(len(cls)) if not ok[r]]
    assert not bad, (what, "(ray, class, e32, e64, floor)", bad[:6])


# ------------------------------------------------------------------------------------------ the fused loss
@pytest.mark.parametrize("R,S,skew", LOSS_CASES)
def test_loss_terms_and_pixel_gradient(dev, R, S, skew):
    """The 13 terms against the f64 oracle: |v - v64| <= max(2e-6 |v64|, 3 |v32 - v64|) + 1e-12, exactly 0 where the f64 oracle's value
    is; g_pix (the same few f64 operations as the oracle's) to 8 * 2^-53 per ray."""
    from nerfca_amd import _capi
    assert list(_capi.TERM_NAMES) == K.TERM_NAMES
    terms, g_pix, _, _ = _fused(dev, R, S, skew)
    o32, o64 = K.oracle_loss(R, S, skew, F32), K.oracle_loss(R, S, skew, F64)
    got = dict(zip(K.TERM_NAMES, terms.tolist()))
    worst = max(K.TERM_NAMES, key=lambda k: abs(got[k] - o64.terms[k]) / max(abs(o64.terms[k]), 1e-300))
    print(f"terms R={R} S={S} skew={skew}: worst {worst} got {got[worst]!r} f64 {o64.terms[worst]!r} f32 {o32.terms[worst]!r}")
    bad = {k: (got[k], o64.terms[k], o32.terms[k]) for k in K.TERM_NAMES if not K.term_ok(got[k], o64.terms[k], o32.terms[k])}
    assert not bad, bad
    assert bool(((g_pix - o64.g_pix).abs() <= 8 * U * o64.g_pix.abs()).all()), float(((g_pix - o64.g_pix).abs() / o64.g_pix.abs()).max())


@pytest.mark.parametrize("R,S,skew", LOSS_CASES)
def test_loss_gradients_per_ray(dev, R, S, skew):
    c = K.loss_case(R, S, skew)
    _, _, g_s, g_d = _fused(dev, R, S, skew)
    o32, o64 = K.oracle_loss(R, S, skew, F32), K.oracle_loss(R, S, skew, F64)
    assert bool(torch.isfinite(g_s).all()) and bool(torch.isfinite(g_d).all())
    _check_rows(f"loss g_sigma_s R={R} S={S} skew={skew}", c.cls, g_s, o32.g_s, o64.g_s)
    _check_rows(f"loss g_sigma_d R={R} S={S} skew={skew}", c.cls, g_d, o32.g_d, o64.g_d)


@pytest.mark.parametrize("R,S", K.DISTS_GRAD_SHAPES)
@pytest.mark.parametrize("skew", K.SKEWS)
@pytest.mark.parametrize("unit_mse", [False, True])
def test_loss_dists_gradient(dev, R, S, skew, unit_mse):
    """d loss / d dists (pix a function of dists) against autograd through the oracle, max-norm over the S entries: one vector has no
    huge rows (the all-zero dynamic rays contribute exactly 0 to it).  Bound: max(1e-5, 3 x the f32 oracle's distance from f64)."""
    from nerfca_amd.fused import fused_losses
    c = K.loss_case(R, S, skew)
    o32, o64 = K.oracle_loss(R, S, skew, F32, unit_mse, True), K.oracle_loss(R, S, skew, F64, unit_mse, True)
    out = fused_losses(c.pix.to(dev), c.gt.to(dev), c.wpix.to(dev), c.sig_s.to(dev), c.sig_d.to(dev), c.dists.to(dev), c.run_args, K.WEIGHTS,
                       unit_mse=unit_mse, want_dists_grad=True)
    assert K.term_ok(float(out[0][0]), o64.terms["loss"], o32.terms["loss"])
    err, floor = rel_err(out[4].cpu(), o64.g_dists), rel_err(o32.g_dists, o64.g_dists)
    print(f"dists gradient R={R} S={S} skew={skew} unit_mse={unit_mse}: err {err:.2e} floor {floor:.2e} margin {err / max(1e-5, 3 * floor):.1e}")
    assert err < max(1e-5, 3 * floor), (err, floor)
    # the other outputs do not depend on the extra launch
    for x, y in (zip(out[:4], _fused(dev, R, S, skew)) if not unit_mse else ()):
        assert torch.equal(x.cpu(), y)


@pytest.mark.parametrize("R,S", K.TERM_GRAD_SHAPES)
@pytest.mark.parametrize("skew", K.SKEWS)
def test_dropin_compute_losses_term_gradients(dev, R, S, skew):
    """The drop-in compute_losses with every differentiable term weighted: the kernel's term-gradient mode, the only place where the
    static field's ray-entropy gradient runs (and, beyond 512 samples, recomputes its q values: at S = 513 that is the 1e-10 tail alone, at
    577 it is 65 ordinary samples).  Values and per-ray gradients by the rules above."""
    from nerfca_amd.train import model_helpers as MH
    c = K.loss_case(R, S, skew)
    a, b = c.sig_s.to(dev).requires_grad_(True), c.sig_d.to(dev).requires_grad_(True)
    res = MH.compute_losses(a, b, c.dists.to(dev), c.wpix.to(dev), c.run_args)
    sum(w * r for w, r in zip(K.TERM_WEIGHTS, res) if w).backward()
    (t32, s32, d32), (t64, s64, d64) = K.oracle_terms(R, S, skew, F32), K.oracle_terms(R, S, skew, F64)
    bad = [(i, float(r), v64, v32) for i, (r, v64, v32) in enumerate(zip(res, t64, t32)) if not K.term_ok(float(r.detach()), v64, v32)]
    assert not bad, bad
    _check_rows(f"terms g_sigma_s R={R} S={S} skew={skew}", c.cls, a.grad.cpu(), s32, s64)
    _check_rows(f"terms g_sigma_d R={R} S={S} skew={skew}", c.cls, b.grad.cpu(), d32, d64)


def test_loss_weights_from_device_memory_beyond_the_kept_samples(dev):
    """Weights by value and through the device vector give the same bits at (9, 513)."""
    from nerfca_amd.fused import fused_losses
    c = K.loss_case(9, 513, 2.0)
    args = [t.to(dev) for t in (c.pix, c.gt, c.wpix, c.sig_s, c.sig_d, c.dists)]
    two = fused_losses(*args, c.run_args, (0.0, 0.0, 0.0, 0.0), weights_dev=torch.tensor(K.WEIGHTS, dtype=F64, device=dev))
    for x, y in zip(_fused(dev, 9, 513, 2.0), two):
        assert torch.equal(x, y.cpu())


def test_loss_is_deterministic_over_1026_blocks(dev):
    """Two runs give the same bits at (4101, 3): per-block partials, two trips of the finishing kernel, 17 of the dists sum."""
    from nerfca_amd.fused import fused_losses
    c = K.loss_case(4101, 3, 1.0)
    args = [t.to(dev) for t in (c.pix, c.gt, c.wpix, c.sig_s, c.sig_d, c.dists)]
    one = [t.clone() for t in fused_losses(*args, c.run_args, K.WEIGHTS, want_dists_grad=True)]
    two = fused_losses(*args, c.run_args, K.WEIGHTS, want_dists_grad=True)
    for x, y in zip(one, two):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ the static loss
@pytest.mark.parametrize("R,S", K.STATIC_SHAPES)
def test_static_loss_vs_closed_form(dev, R, S):
    """pixel and occl against exactly rounded sums of the same f64 products (bound count * 2^-53 * sum |term|: only the order of the sum
    is free); g_sigma bit-equal to f32((w_occl inv_R) dists) on every ray; g_pix to 8 * 2^-53; want_grads=False gives the same term bits."""
    from nerfca_amd import _capi
    from nerfca_amd.fused import static_losses
    c, ref = K.loss_case(R, S, 1.0), K.static_reference(R, S)
    args = [t.to(dev) for t in (c.pix, c.gt, c.wpix, ref.sigma, c.dists)]
    terms, g_pix, g_sigma = static_losses(*args, ref.w_occl)
    got = dict(zip(_capi.STATIC_TERM_NAMES, terms.cpu().tolist()))
    print(f"static R={R} S={S}: pixel err {abs(got['pixel'] - ref.pixel):.1e} (bound {ref.pixel_bound:.1e})  occl err {abs(got['occl'] - ref.occl):.1e} (bound {ref.occl_bound:.1e})")
    assert abs(got["pixel"] - ref.pixel) <= ref.pixel_bound, (got["pixel"], ref.pixel, ref.pixel_bound)
    assert abs(got["occl"] - ref.occl) <= ref.occl_bound, (got["occl"], ref.occl, ref.occl_bound)
    assert got["loss"] == got["pixel"] + ref.w_occl * got["occl"] and got["reserved"] == 0.0
    assert g_sigma.dtype == F32 and np.array_equal(g_sigma.cpu().numpy(), np.broadcast_to(ref.g_sigma_row, (R, S)))
    assert np.all(np.abs(g_pix.cpu().numpy() - ref.g_pix) <= 8 * U * np.abs(ref.g_pix))
    terms2, none_pix, none_sigma = static_losses(*args, ref.w_occl, want_grads=False)
    assert none_pix is None and none_sigma is None and torch.equal(terms, terms2)


# ------------------------------------------------------------------------------------------ stand-alone compositing
def _planted_checks(c, act, single, scale, cp, sig, grads):
    """The planted samples one by one (field f, ray r, sample s, value x)."""
    s32 = float(np.float32(scale))
    for f, r, s, x in c.planted:
        if single and f == 1:
            continue
        v, g = float(sig[f][r, s]), float(grads[f][r, s])
        up = (3.0, -2.0)[f]
        gp = float(cp[r]) * float(c.dists[s])
        G = up - gp * s32 if single else (up - gp) * s32             # the upstream gradient that reaches the activation's derivative
        where = (act, single, scale, f, r, s, x, v, g)
        if x == -104.0:                                                # expf underflows to 0: softplus, its clamp and the sigmoid all give 0
            assert v == 0.0 and g == 0.0, where
        if act == "softplus" and x == 60.0:                            # beyond the threshold: the identity
            assert v == (60.0 if single else float(np.float32(60.0) * np.float32(scale))), where
            assert abs(g - G) <= 2.0 ** -23 * abs(G), where + (G,)
        if act == "clamp" and x == 5.0:                                # softplus(5) > 1: the clamp's upper flat arm
            assert v == (1.0 if single else s32) and g == 0.0, where
        if act == "Softplus" and x == -89.0:                           # the sigmoid: expf(89) overflows
            assert v == 0.0 and g == 0.0, where


@pytest.mark.parametrize("R,S", K.COMPOSITE_SHAPES)
@pytest.mark.parametrize("act", ["softplus", "clamp", "Softplus"])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("scale", [1e-2, 1.0])
def test_composite_forward_and_backward(dev, R, S, act, single, scale):
    """composite_raw against O.composite / O.composite_single in f64 (f32 = the floor): sigma and the raw gradients per ray, pix to
    max(1e-5, 3 floor) of |I0| + sum |term|; then the planted samples.  ("Softplus", capitalised, is the reference's sigmoid.)"""
    from nerfca_amd.fused import composite_raw
    c = K.composite_case(R, S)
    o32, o64 = K.oracle_composite(R, S, act, single, scale, F32), K.oracle_composite(R, S, act, single, scale, F64)
    rs = c.raw_s.to(dev).requires_grad_(True)
    rd = None if single else c.raw_d.to(dev).requires_grad_(True)
    out = composite_raw(rs, rd, c.I0.to(dev), c.dists.to(dev), act, single, scale, True)
    cp = torch.linspace(-1, 1, R, dtype=F64)
    loss = (out[0] * cp.to(dev)).sum() + (out[1] * 3).sum()
    if not single:
        loss = loss - (out[2] * 2).sum()
    loss.backward()
    pix, sig = out[0].detach().cpu(), [t.detach().cpu() for t in out[1:]]
    grads = [rs.grad.cpu()] + ([] if single else [rd.grad.cpu()])
    assert pix.dtype == F64 and all(t.dtype == F32 for t in sig + grads)
    cls = ["planted" if r in {p[1] for p in c.planted} else "random" for r in range(R)]
    tag = f"R={R} S={S} {act} single={single} scale={scale}"
    floor = (o32.pix - o64.pix).abs() / o64.mag
    perr = (pix - o64.pix).abs() / o64.mag
    bound = torch.clamp(3 * floor, min=1e-5)
    print(f"margin composite pix {tag}: " + "  ".join(f"{k} {v:.1e}" for k, v in K.class_margins(perr / bound, cls).items()))
    assert bool((perr <= bound).all()), (tag, float(perr.max()), float(floor.max()))
    for name, got, g32, g64 in [("sigma_s", sig[0], o32.sig_s, o64.sig_s), ("g_raw_s", grads[0], o32.g_s, o64.g_s)] + \
                               ([] if single else [("sigma_d", sig[1], o32.sig_d, o64.sig_d), ("g_raw_d", grads[1], o32.g_d, o64.g_d)]):
        _check_rows(f"composite {name} {tag}", cls, got, g32, g64)
    _planted_checks(c, act, single, scale, cp, sig, grads)


# ------------------------------------------------------------------------------------------ Adam + LinearLR
def _adam_models(dev, which):
    from nerfca_amd import _capi, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    torch.manual_seed(3)
    if which == "F32":                  # ~7 k elements per segment: 7 workgroups, four trips of the stride loop with a tail
        sdef, tdef = synthetic.net_definitions(dev, F=32)
    elif which == "F128":               # the default nets: segments beyond 64 x 1024 elements
        sdef, tdef = synthetic.net_definitions(dev, F=128, early=4)
    else:                               # unequal segments: a 256-unit static net on the general kernels beside a 32-unit dynamic net
        sdef, tdef = synthetic.net_definitions(dev, F=256, early=1)[0], synthetic.net_definitions(dev, F=32)[1]
    s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
    if which == "wide":
        assert _capi.net_is_general(s._binding.net) and not _capi.net_is_general(t._binding.net)
    return [t, s]


@pytest.mark.parametrize("which", ["F32", "F128", "wide"])
def test_adam_updates_vs_f64(dev, which):
    """Seven steps across total_iters = 4, gradients randn * 10^(it - 3) with a slice of 100 exact zeros per segment.  The UPDATE of every
    step, p_after - p_before, against Adam + LinearLR in numpy f64 from the same f32 gradients, per element and divided by that step's
    lr (Adam's step is at most about lr): <= max(2e-6, 3 x the same distance of torch.optim.Adam in f32 on the CPU).  The zero-gradient
    slices keep their initial bits (m = v = 0: the update is -step * 0 / (0 + eps))."""
    from nerfca_amd.fused import FusedAdam
    models = _adam_models(dev, which)
    adam = FusedAdam(models, lr=1e-2, end_factor=0.1, total_iters=4)
    flats = [b.flat for b in adam.bindings]
    ns = [f.numel() for f in flats]
    if which != "F32":
        assert max(ns) > 65536 and max(ns) % (64 * 256) != 0            # gx is capped at 64: several trips of the stride loop, and a tail
    if which == "wide":
        assert min(ns) < 16384 < max(ns)
    grads = [K.adam_gradients(n, 7, 100 + k) for k, n in enumerate(ns)]
    p0 = [f.detach().clone().cpu() for f in flats]
    prev, got = p0, [[] for _ in ns]
    for it in range(7):
        adam.step([torch.from_numpy(g[it]).to(dev) for g in grads])
        cur = [f.detach().clone().cpu() for f in flats]
        for k in range(len(ns)):
            got[k].append((cur[k].double() - prev[k].double()).numpy())
        prev = cur
    assert int(adam.step_count.item()) == 7
    err = floor = 0.0
    for k in range(len(ns)):
        ref, lrs = K.adam_updates_f64(grads[k])
        f32 = K.adam_updates_torch_f32(p0[k], grads[k])
        for it in range(7):
            assert np.isfinite(got[k][it]).all(), (k, it)              # (max() below would drop a NaN)
            err = max(err, float(np.abs(got[k][it] - ref[it]).max()) / lrs[it])
            floor = max(floor, float(np.abs(f32[it] - ref[it]).max()) / lrs[it])
        assert torch.equal(prev[k][K.zero_slice(ns[k])], p0[k][K.zero_slice(ns[k])]), k
    print(f"adam {which}: segments {ns}  max |update - f64| / lr = {err:.2e}  torch f32 {floor:.2e}  ratio to bound {err / max(2e-6, 3 * floor):.2f}")
    assert err <= max(2e-6, 3 * floor), (err, floor)
