"""The CPU half of the one-hot gradient checks (tests/test_onehot_grads_gpu.py holds the kernels to them): the nets, the metric and the floors.

The suite's gradient checks are one number per tensor, rel_err = max |a - b| / max |b|, at 1e-5 (f32) or BF_GRAD = 5e-2 (bf16).  An error that
stays under 5 % of a weight tensor's largest entry -- one encoded column of a high band, one row, one latent slot -- passes them.  Here:
  * `decided_params` builds nets whose ReLU masks are decided by their biases (every pre-activation in [-3, -1] u [1, 3]) on every batch the
    GPU module uses, for the f32 and the f64 oracle, with and without bf16 operands;
  * seeded faults in a copy of the oracle's one-hot gradient are each caught by check A (rank one), check B (exact zeros) or check C
    (`scaled_err`) -- and each still passes rel_err < BF_GRAD: the old measure is blind to them;
  * the distance of the f32 emulating oracle from the f64 one in check C's metric is recorded for every plan's emulation: the floor of the
    GPU module's check C.  Measured (worst over launches and parameters; the GPU module writes them beside its own figures into
    profiles/onehot_grad.txt): f32 (nothing emulated) 4e-5 .. 1.6e-4 on the first layer's weights -- the f32 oracle rounds the argument
    2^k x + pi / 2 of a high band's cosine to f32 as the reference does, the f64 oracle does not -- and <= 2e-6 elsewhere; the bf16
    emulations 1e-7 .. 8e-7, but 1.3e-4 where that same f32 rounding moves an encoded feature across a bf16 rounding boundary (F32_e1)."""
import pytest
import torch

from conftest import rel_err
from nca_testlib import (BF_FACTOR, BF_GRAD, ONEHOT_NETS, ONEHOT_POINT_CASES, ONEHOT_RAY_CASES, onehot_checks_ab, onehot_emulations, onehot_factor_errs, onehot_latent_rows, onehot_points,
                         onehot_rays, rank_one_split, wide_layers, wide_preacts)

MARGIN = 1 - 2.0 ** -6          # (the slack: W / max |P| is rounded to f32, then to bf16 again)


@pytest.mark.parametrize("case", [("rays",) + c for c in ONEHOT_RAY_CASES] + [("points",) + c for c in ONEHOT_POINT_CASES], ids=lambda c: "-".join(map(str, c)))
def test_decided_nets_have_the_margin_on_every_batch(case):
    c = onehot_rays(*case[1:]) if case[0] == "rays" else onehot_points(*case[1:])
    for net in "st":
        spec, p = c.spec(net), c.params(net)
        feats = c.feats_s if net == "s" else c.feats_d
        assert min(c.margin_s if net == "s" else c.margin_d) >= MARGIN
        for dt in (torch.float32, torch.float64):
            for emulate in (True, False):          # (f32 mode rounds no operand: the same margin must hold there)
                for (wk, bk, _), z in zip(wide_layers(spec), wide_preacts(p, spec, feats, dt, emulate)):
                    assert float(z.abs().min()) >= MARGIN and float(z.abs().max()) <= 3 + 2.0 ** -6, (net, wk, dt, emulate)
                    on = p[bk] > 0
                    assert bool(((z > 0) == on).all())          # the masks are the biases' signs: mixed, and no rounding can flip one
                    assert 0.25 <= float(on.float().mean()) <= 0.75, (net, bk)


# ------------------------------------------------------------------------------------------ seeded faults
def _target(name="F128_e3", i=2):
    """The dynamic net of launch i of a ray case under the recompute plan's emulation, in f64: (case, spec, params, gradients, the
    sample's input row, its heart phase).  The default: F = 128, 3 hidden layers, s* = 63."""
    c = onehot_rays(name)
    (_, _), (r, s) = c.launches[i]
    g = {k[2:]: v.clone() for k, v in c.oracle(i, "recompute").items() if k[0] == "t"}
    return c, c.sd, c.pd, g, c.feats("t", r, s), int(c.ph[r])


def _first_target(pick):
    """The first (net, launch) of the ray cases at which `pick(gradients, phase)` finds a place for its fault (it returns None elsewhere)."""
    for name in ONEHOT_NETS:
        for i in range(6):
            t = _target(name, i)
            where = pick(t[3], t[5])
            if where is not None:
                return t, where
    raise AssertionError("no launch has a place for this fault")


def _worst_c(spec, got, want):
    return max(e for _, e, _ in onehot_factor_errs(spec, got, want))


def _small(v, lo, hi):
    """Index of the largest |v_i| with lo < |v_i| / max |v| < hi."""
    rel = v.abs() / v.abs().max()
    ok = (rel > lo) & (rel < hi)
    assert bool(ok.any())
    return int(torch.where(ok, rel, torch.zeros_like(rel)).argmax())


def test_the_oracle_itself_passes_every_check():
    c, spec, p, g, x, _ = _target()
    assert onehot_checks_ab(spec, p, g, x, "oracle") <= 2.0 ** -40          # f64: rank one to its own rounding
    assert _worst_c(spec, g, g) == 0.0


@pytest.mark.parametrize("fault", ["column_zeroed", "columns_swapped", "row_doubled", "off_row_filled", "latent_slot_in_next_phase"])
def test_seeded_fault_is_caught_by_the_new_checks_and_missed_by_rel_err(fault):
    c, spec, p, g, x, phase = _target()
    W0, b0 = "early_pts_layers.0.weight", "early_pts_layers.0.bias"
    bad = {k: v.clone() for k, v in g.items()}
    a, u = rank_one_split(g[W0], g[b0])
    if fault == "column_zeroed":
        # the highest encoded column under 4 % of the largest (the raw coordinates are ~4, a band's features at most 1) and above check C's 1 / 256
        rel = u[:75].abs() / u.abs().max()
        key, j = W0, int(torch.nonzero((rel > 2.0 ** -8) & (rel < 0.04)).max())
        assert j >= 3 + 6 * 4, j          # a high band: 4 or above of the 7 the window at iteration 75 000 leaves open
        bad[W0][:, j] = 0
        assert _worst_c(spec, bad, g) >= 0.99 > BF_FACTOR          # the whole column, at its own scale
    elif fault == "columns_swapped":
        # two adjacent encoded columns that are both small against the largest, and different
        d = (u[3:74] - u[4:75]).abs() / u.abs().max()
        both = torch.maximum(u[3:74].abs(), u[4:75].abs()) / u.abs().max()
        ok = (d < 0.04) & (d > 4 * BF_FACTOR * both.clamp_min(2.0 ** -8))
        assert bool(ok.any())
        key, j = W0, 3 + int(torch.where(ok, d, torch.zeros_like(d)).argmax())
        bad[W0][:, [j, j + 1]] = g[W0][:, [j + 1, j]]
        assert _worst_c(spec, bad, g) > 4 * BF_FACTOR
    elif fault == "row_doubled":
        key, f = W0, _small(a, 0, 0.04)
        bad[W0][f] *= 2
        with pytest.raises(AssertionError, match="A: row, column"):
            onehot_checks_ab(spec, p, bad, x, fault)
    elif fault == "off_row_filled":
        key = "early_pts_layers.2.weight"

        def pick(g, phase):
            a1 = g["early_pts_layers.2.bias"]
            return next((f for f in range(1, a1.numel()) if a1[f] == 0 and 0 < abs(a1[f - 1]) < 0.04 * a1.abs().max()), None)
        (c, spec, p, g, x, phase), f = _first_target(pick)
        bad = {k: v.clone() for k, v in g.items()}
        bad[key][f] = g[key][f - 1]
        with pytest.raises(AssertionError, match="B: off-unit rows"):
            onehot_checks_ab(spec, p, bad, x, fault)
    else:
        key = "time_latents"

        def pick(g, phase):
            rel = g[key][phase].abs() / g[key][phase].abs().max()
            return int(rel.argmin()) if float(rel.min()) < 0.04 else None
        (c, spec, p, g, x, phase), t = _first_target(pick)
        bad = {k: v.clone() for k, v in g.items()}
        bad[key][(phase + 1) % 10, t], bad[key][phase, t] = g[key][phase, t], 0
        onehot_latent_rows(g[key], phase, "oracle")
        with pytest.raises(AssertionError, match="B: latent rows"):
            onehot_latent_rows(bad[key], phase, fault)
    for k in g:
        assert rel_err(bad[k], g[k]) < BF_GRAD, (fault, k)          # the old measure does not see it
    assert not torch.equal(bad[key], g[key])


# ------------------------------------------------------------------------------------------ the floors of check C
@pytest.mark.parametrize("case", ONEHOT_RAY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_floor_of_check_c_is_recorded(case):
    """scaled_err of the f32 emulating oracle from the f64 one, per plan's emulation.  The bf16 emulations' floor never widens the 2^-6
    of check C; the f32 floor does widen its 1e-5 on the first layer's weights (the f32 rounding of a high band's argument)."""
    c = onehot_rays(*case)
    for emu in onehot_emulations(c.S):
        worst = {}
        for i in range(len(c.launches)):
            for k, e in c.floor(i, emu).items():
                worst[k] = max(worst.get(k, 0.0), e)
        top = max(worst, key=worst.get)
        print(f"floor {c.name} S={c.S} it_d={c.it_d} {emu}: {worst[top]:.2e} ({top})")
        assert all(e == e and e < float("inf") for e in worst.values())
        if emu != "f32":
            assert 3 * worst[top] < BF_FACTOR
