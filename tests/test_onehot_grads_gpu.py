"""Every entry of every parameter gradient of the fused MLP kernels (forward, dgrad sweep, weight-gradient and reduce kernels of
nca_kernels_f32.hip / nca_kernels_bf16.hip, the point kernels) held to the f64 oracle -- not one number per tensor.  Of the general kernels
this module reaches one launch shape (144 units, 300 points in one chunk of three row tiles and splits: identity tile order, no skip layer, one
output channel, no ray batch); their tile, split and run seams are held in tests/test_onehot_general_gpu.py.

The other gradient tests bound rel_err = max |a - b| / max |b| per tensor at 1e-5 (f32) or 5e-2 (bf16): random nets sum thousands of
random-signed samples (cancellation hides small errors) and ReLU pre-activations within rounding of zero flip masks.  Here both causes
are removed by the choice of input, with no change to the oracle (helpers and cases: tests/nca_testlib.py; the CPU half, with the seeded
faults this catches and rel_err does not: tests/test_onehot_grads_cpu.py):
  * a ONE-HOT upstream gradient: only sigma of one net at one sample (r*, s*) gets a coefficient, so every weight gradient is the rank-one
    d_l (x) h_{l-1} of that sample -- no sum, no cancellation;
  * nets whose ReLU masks are decided by their biases (`decided_params`): no rounding can flip one.

Checks (bounds derived, not measured):
  A  rank one: dW[f, j] == db[f] u[j] to 2^-20 per entry, every F-wide layer and the output layer, every run;
  B  exact zeros: rows of off units, columns of zero inputs, every latent row but ph[r*], every parameter of a net without a coefficient;
  C  against the emulating oracle in f64 with `scaled_err` (columns at their own scale down to 1 / 256 of the largest, rows at the
     layer's largest delta): f32 plans max(1e-5, 3 floor), bf16-operand plans max(2^-6, 3 floor), floor = the f32 emulating oracle's own
     distance from the f64 one;
  D  the 8-bit staged plan is the bf16-store plan quantised: e4m3(4 u16) / 4 and e5m2(a16 s) / s per entry to 2^-20 (nca_layout.hpp);
  E  additivity over wave tiles and ray chunks to 2^-20 of the sum of the |terms| (the latents' entries: of their products, see the test).

Measured on an MI355X (profiles/onehot_grad.txt, written by this module when NERFCA_ONEHOT_RECORD names a file; 74 tests, 4 s):
  A  <= 2.3e-7 in f32 mode and from the two stores, <= 2.1e-16 in the recompute plan and on points in bf16 mode (bf16 x bf16 is exact in f32);
  C  f32 plans: the first layer's weights 4.0e-5 .. 1.6e-4 = the floor itself (the kernels round the argument of a band's sine as the
     reference and the f32 oracle do), C / bound 0.33 .. 0.35; bf16 store <= 2.6e-7; bf16 recompute 3.6e-3 .. 9.7e-3 (C / bound <= 0.62: its
     back-propagated deltas are rounded to bf16, which the oracle does not emulate -- largest on the latents, an F-term sum of them);
     points in bf16 mode 2.8e-3 .. 4.1e-3; the general kernels 4.33e-5 (floor 4.34e-5);
  D  dW <= 6.0e-8, db <= 5.9e-8, dWo <= 6.2e-8, latents <= 5.1e-8: the documented arithmetic is complete;
  E  <= 2.1e-7.
No check found a kernel wrong.
"""
import math
import os

import pytest
import torch

from conftest import nca_option
from nca_testlib import (BF_FACTOR, ONEHOT_NETS, ONEHOT_R, ONEHOT_RAY_CASES, dev, entry_err, hip_render_grads, make_dynamic, make_static, onehot_checks_ab,  # noqa: F401
                         onehot_coeffs, onehot_factor_errs, onehot_latent_rows, onehot_points, onehot_rays, rank_one_split, wide_layers)
from oracle import nerfca_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
EXACT = 2.0 ** -20
CAP = 24 << 20
# plan: (precision, fused.STORE_FORWARD_LIMIT_BYTES or None, NCA_OPT_STAGE_FP8, NCA_OPT_BF16_STORE, the store kind meant, the oracle's emulation)
PLANS = {"f32_store": ("f32", None, None, None, "STORE_F32", "f32"), "f32_recompute": ("f32", 0, None, None, "STORE_NONE", "f32"),
         "fp8_store": ("bf16", None, None, None, "STORE_FP8", "fp8_store"), "bf16_store": ("bf16", None, 0, None, "STORE_BF16", "bf16_store"),
         "bf16_recompute": ("bf16", None, 0, 0, "STORE_NONE", "recompute")}
RECORD = {}
_MODELS = {}


def note(row, check, value):
    rec = RECORD.setdefault(row, {})
    rec[check] = max(rec.get(check, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def record():
    """Prints the worst value of every check per case and plan when the module is done; NERFCA_ONEHOT_RECORD=<file> keeps them."""
    yield
    lines = [f"{row:<58s} " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(rec.items())) for row, rec in RECORD.items()]
    print("\n" + "\n".join(lines))
    path = os.environ.get("NERFCA_ONEHOT_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def models(c, dev):
    if id(c) not in _MODELS:
        s = make_static(c.ps, dev, F=c.F, early=c.early, late=c.late)
        t = make_dynamic(c.pd, dev, F=c.F, early=c.early_d, late=0, T=8)
        s.update_freq_mask_alpha(75000, 150000)
        t.update_freq_mask_alpha(getattr(c, "it_d", 75000), 150000)
        _MODELS[id(c)] = (s, t)
    return _MODELS[id(c)]


def run_rays(c, dev, plan, cap, cp, cs, cd):
    """The library's parameter gradients (on the CPU) of the scalar with these coefficients under `plan`, the workspace capped at `cap` bytes."""
    from nerfca_amd import _capi, fused, set_precision
    prec, limit, fp8, store16, kind, _ = PLANS[plan]
    s, t = models(c, dev)
    set_precision(prec, s, t)
    saved = fused.STORE_FORWARD_LIMIT_BYTES, fused.BWD_WORKSPACE_BYTES
    try:
        if limit is not None:
            fused.STORE_FORWARD_LIMIT_BYTES = limit
        if cap:
            fused.BWD_WORKSPACE_BYTES = cap
        with nca_option("STAGE_FP8", fp8), nca_option("BF16_STORE", store16):
            g = hip_render_grads(s, t, dev, c.o, c.d, c.ph, c.I0, c.z, c.dists, cp, cs, cd)[3]
            got = _capi.last_plan()["fwd_store_format"] & _capi.STORE_KIND_MASK
    finally:
        fused.STORE_FORWARD_LIMIT_BYTES, fused.BWD_WORKSPACE_BYTES = saved
    assert got == getattr(_capi, kind), (plan, got)
    return {k: v.cpu() for k, v in g.items()}


def of_net(g, net):
    return {k[2:]: v for k, v in g.items() if k[0] == net}


def check_abc(c, g, i, plan, tag, row, targets="st"):
    """Checks A, B and (but for the 8-bit plan, which check D holds to the bf16 store) C on the gradients of launch i."""
    emu = PLANS[plan][5] if plan in PLANS else plan
    floor = c.floor(i, emu) if emu != "fp8_store" else {}
    want = c.oracle(i, emu)
    for net, where in zip("st", c.launches[i]):
        if net not in targets:
            for k, v in of_net(g, net).items():
                assert not bool(v.any()), (tag, net + "." + k, "B: a net without a coefficient")
            continue
        spec, sub = c.spec(net), of_net(g, net)
        x = c.feats(net, *where) if isinstance(where, tuple) else c.feats(net, where)
        note(row, "A", onehot_checks_ab(spec, c.params(net), sub, x, (tag, net, where), deltas_nonzero=emu != "fp8_store"))
        if net == "t":
            onehot_latent_rows(sub["time_latents"], int((c.ph[where[0]] if isinstance(where, tuple) else c.ts[where])), (tag, where))
        if emu == "fp8_store":
            continue
        base = TOL if emu == "f32" else BF_FACTOR
        for k, e, at in onehot_factor_errs(spec, sub, of_net(want, net)):
            fl = floor[net + "." + k]
            print(f"C {tag} {net}.{k} at {where}: {e:.3e} (floor {fl:.2e}) worst entry {at}")
            note(row, "C", e)
            note(row, "C/bound", e / max(base, 3 * fl))
            note(row, "floor", fl)
            assert e < max(base, 3 * fl), (tag, net + "." + k, "C: row, column (k-step = column // 16)", at, where, e, fl)


# ------------------------------------------------------------------------------------------ rays: checks A, B, C in every plan
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("case", ONEHOT_RAY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_onehot_rays(dev, case, plan):
    """Each net of the pair is the target at every position (the two one-hots of a launch at different rays), with the default workspace and
    with 24 MB; once alone, the other net's gradient then zero bit for bit and its own the same bits as in the shared launch."""
    c = onehot_rays(*case)
    row = f"rays {c.name} S={c.S} it_d={c.it_d} {plan}"
    for cap in (None, CAP):
        for i in range(len(c.launches)):
            g = run_rays(c, dev, plan, cap, *c.coeffs(i))
            check_abc(c, g, i, plan, (row, "cap", cap, "launch", i), row)
            if i == 0 and cap is None:
                (rs, s_s), (rd, s_d) = c.launches[i]
                for net, r, s in (("s", rs, s_s), ("t", rd, s_d)):
                    alone = run_rays(c, dev, plan, cap, *onehot_coeffs(ONEHOT_R, c.S, net, r, s))
                    check_abc(c, alone, i, plan, (row, "alone", net), row, targets=net)
                    for k, v in of_net(alone, net).items():
                        assert torch.equal(v, g[net + "." + k]), (row, net + "." + k, "the other net's one-hot moved it")


# ------------------------------------------------------------------------------------------ check D
def _q8(x, fmt):
    return O._q8(x.float(), fmt).double()


def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def _is_bf16(x, tag):
    """x (f64 of f32 arithmetic) is a bf16 value up to the f32 roundings of the product and quotient it came from; returns the bf16 value."""
    q = _bf16(x)
    e, at = entry_err(x, q)
    assert e <= EXACT, (tag, "not a bf16 value", at, e)
    return q


@pytest.mark.parametrize("case", ONEHOT_RAY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp8_plan_is_the_bf16_store_plan_quantised(dev, case):
    """Check D.  Both plans share the forward and the bf16 chain, so with (a16, u16) the factors of the bf16-store run of the same one-hot and
    g its dbo, s = 2^(4 - floor(log2 |g|)) (the tile's only non-zero gradient), the 8-bit run must give, per entry to 2^-20:
        dW_l = e5m2(a16 s) / s (x) e4m3(4 u16) / 4, db_l = e5m2(a16 s) / s                           (l < NL - 1)
        dW_{NL-1}[f] = Wo[f] q (x) e4m3(4 u16) / 4, db_{NL-1}[f] = Wo[f] q on on-units, q = e5m2(bf16(g) s) / s
        dWo[f] = q (sum_k bf16(W_{NL-1})[f][k] e4m3(4 u16[k]) / 4 + b_{NL-1}[f]) on on-units, dbo = g
        d time_latents[ph[r*]] = db_0 W_0[:, latent columns]                                        (f32 weights)
    (nca_layout.hpp "The bf16 mode's forward store"; _StagedLinear / _StagedTail of the oracle)."""
    c = onehot_rays(*case)
    row = f"rays {c.name} S={c.S} it_d={c.it_d} fp8_store vs bf16_store"
    for i in range(len(c.launches)):
        coef = c.coeffs(i)
        g16, g8 = run_rays(c, dev, "bf16_store", None, *coef), run_rays(c, dev, "fp8_store", None, *coef)
        for net, (r, s_) in zip("st", c.launches[i]):
            spec, p = c.spec(net), c.params(net)
            a, b = of_net(g16, net), of_net(g8, net)
            tag = (row, net, "launch", i, (r, s_))
            g = a["output_linear.0.bias"].double().reshape(())
            assert torch.equal(b["output_linear.0.bias"], a["output_linear.0.bias"]), tag
            sc = 2.0 ** (4 - (math.frexp(abs(float(g)))[1] - 1))
            q = _q8(_bf16(g) * sc, "e5m2") / sc
            layers = wide_layers(spec)
            for l, (wk, bk, _) in enumerate(layers):
                a16, u16 = rank_one_split(a[wk], a[bk])
                u8 = _q8(4 * _is_bf16(u16, tag + (wk, "u16")), "e4m3") / 4
                if l < len(layers) - 1:
                    a8 = _q8(_is_bf16(a16, tag + (bk, "a16")) * sc, "e5m2") / sc
                else:
                    a8 = p["output_linear.0.weight"].double().reshape(-1) * q * (p[bk] > 0)
                    dWo = q * (p[bk] > 0) * (_bf16(p[wk].double()) @ u8 + p[bk].double())
                    mag = q.abs() * (_bf16(p[wk].double()).abs() @ u8.abs() + p[bk].double().abs())
                    e, at = entry_err(b["output_linear.0.weight"].reshape(-1), dWo, mag)
                    note(row, "D dWo", e)
                    assert e <= EXACT, (tag, "output_linear.0.weight", "D", at, e)
                e, at = entry_err(b[bk], a8)
                note(row, "D db", e)
                assert e <= EXACT, (tag, bk, "D: row", at, e)
                e, at = entry_err(b[wk], a8[:, None] * u8[None, :])
                note(row, "D dW", e)
                assert e <= EXACT, (tag, wk, "D: row, column (k-step = column // 16)", at, e)
                if l == 0 and net == "t":
                    Wl = p[wk].double()[:, -8:]
                    e, at = entry_err(b["time_latents"][int(c.ph[r])], b[bk].double() @ Wl, b[bk].double().abs() @ Wl.abs())
                    note(row, "D latents", e)
                    assert e <= EXACT, (tag, "time_latents", "D", at, e)


# ------------------------------------------------------------------------------------------ check E
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", list(ONEHOT_NETS))
def test_onehots_in_three_wave_tiles_add_up(dev, name, plan):
    """Three one-hots of each net in three different wave tiles -- two rays, and both tiles of one ray (the second ragged) -- give the sum of
    the three single runs, per entry to 2^-20 of the sum of the three |terms|: a sample's contribution depends on other samples only
    through its tile's scale, so this is exact up to f32 summation.  With the default workspace and with 24 MB: the split-slab reduction
    and nca_sum_tile_records, which a single one-hot does not exercise."""
    c = onehot_rays(name)
    row = f"rays {c.name} S={c.S} it_d={c.it_d} {plan}"
    spots = {"s": [(4, 10), (4, 66), (8, 40)], "t": [(0, 69), (0, 33), (5, 64)]}
    for cap in (None, CAP):
        singles = []
        cs_all, cd_all = torch.zeros(ONEHOT_R, c.S), torch.zeros(ONEHOT_R, c.S)
        for j in range(3):
            cp, cs, _ = onehot_coeffs(ONEHOT_R, c.S, "s", *spots["s"][j])
            cd = onehot_coeffs(ONEHOT_R, c.S, "t", *spots["t"][j])[2]
            cs_all += cs
            cd_all += cd
            singles.append(run_rays(c, dev, plan, cap, cp, cs, cd))
        both = run_rays(c, dev, plan, cap, cp, cs_all, cd_all)
        for k, v in both.items():
            assert bool(torch.isfinite(v).all()), (row, k)
            terms = torch.stack([g[k].double() for g in singles])
            scale = terms.abs().sum(0)
            if k == "t.time_latents":
                # an entry of the latents' gradient is itself an f32 contraction over the F units, sum_f d_0[f] W_0[f][latent t] (the one-hot phase
                # columns of the input block times D_0, then the f32 weights: _StagedLinear), and two of the three samples share a ray, so a
                # heart phase: (d_a + d_b) W_0 against d_a W_0 + d_b W_0 rounds at the scale of the products, not of the sums they cancel to
                # (measured at the scale of the three sums: 9.76e-7 .. 2.85e-6 in 8 of the 25 net x plan rows, against 2^-20 = 9.54e-7; at the scale of
                # the products: <= 2.1e-7)
                W = c.pd["early_pts_layers.0.weight"].double()[:, -8:]
                scale = torch.zeros_like(scale)
                for j, g in enumerate(singles):
                    scale[int(c.ph[spots["t"][j][0]])] += g["t.early_pts_layers.0.bias"].double().abs() @ W.abs()
                note(row, "E latents, of the 3 sums", entry_err(v, terms.sum(0), terms.abs().sum(0))[0])
            e, at = entry_err(v, terms.sum(0), scale)
            note(row, "E", e)
            assert e <= EXACT, (row, "cap", cap, k, "E", at, e)


# ------------------------------------------------------------------------------------------ the point kernels and the general kernels
def run_points(c, dev, prec, i, cap=None):
    from nerfca_amd import fused, set_precision
    s, t = models(c, dev)
    set_precision(prec, s, t)
    ns, nd = c.launches[i]
    gs, gd = torch.zeros(c.N, 1), torch.zeros(c.N, 1)
    gs[ns], gd[nd] = 1.0, 1.0
    for m in (s, t):
        m.zero_grad()
    saved = fused.BWD_WORKSPACE_BYTES
    try:
        if cap:
            fused.BWD_WORKSPACE_BYTES = cap
        x = c.x.to(dev)
        ((s(x) * gs.to(dev)).sum() + (t.forward_composite(x, c.ts.to(dev)) * gd.to(dev)).sum()).backward()
    finally:
        fused.BWD_WORKSPACE_BYTES = saved
    g = {"s." + k: p.grad.detach().cpu() for k, p in s.named_parameters()}
    g.update({"t." + k: p.grad.detach().cpu() for k, p in t.named_parameters()})
    return g


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["F32_e1", "F128_e3", "F128_e1_l2"])
def test_onehot_points(dev, name, prec):
    """CPPN.forward / Temporal.forward_composite on 130 points with a one-hot `gout` at n* in {0, 63, 64, 129}: checks A, B, C."""
    c = onehot_points(name, 130)
    row = f"points {c.name} N={c.N} {prec}"
    for i in range(len(c.launches)):
        check_abc(c, run_points(c, dev, prec, i), i, "f32" if prec == "f32" else "recompute", (row, "launch", i), row)


def test_onehot_points_general_kernels(dev):
    """The general kernels (F = 144 > 128 units; f32) on 300 points with a 3 MB workspace (the 384 rows fit it: one chunk of three row tiles and three splits, tests/test_onehot_general_cpu.py), n* in {0, 127, 128, 299}: check A
    (the same 2^-20 of v_mfma_f32_32x32x2_f32: one product per entry), B, and C at 1e-5 -- with the f32 rule's floor, as for the fused
    kernels: without it the first layer's weights measure 4.33e-5 (row 50, column 42: the cosine of band 6), which is the f32 oracle's own
    4.3e-5 from the f64 one -- the reference forms a cosine as sin(fl32(2^k x) + fl32(pi / 2)) (oracle.encode), and so do the kernels and the
    f32 oracle; the f64 oracle does not round that argument.  Every other parameter is under 1e-5 without the floor."""
    from nerfca_amd import _capi
    c = onehot_points("F144_e1", 300)
    s, t = models(c, dev)
    assert _capi.net_is_general(s._binding.net) and _capi.net_is_general(t._binding.net)
    row = f"points {c.name} N={c.N} f32 general"
    for i in range(len(c.launches)):
        g = run_points(c, dev, "f32", i, cap=3 << 20)
        check_abc(c, g, i, "f32", (row, "launch", i), row)
