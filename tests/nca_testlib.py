"""Shared helpers of the suite: the `dev` fixture, net construction, seeded ray batches, the oracle's and the library's gradients of
the scalar every render-parity test differentiates,

    sum(pix * cp) + 50 sum(sigma_s * cs) + 50 sum(sigma_d * cd),

launch counting, the bf16 bounds, the per-entry gradient checks on one-hot upstream gradients (nets with decided ReLU masks, the rank-one
split, `scaled_err`, the ray and point cases with their memoised oracle gradients, the general kernels' cases with the restated launch arithmetic
they are chosen by), what the launch-free tests of the view sections (csrc/view/) share: the `capi` / `lib` fixtures, the
declared-bound-exported check, `refused` and the one list of NcaGrid refusals, and what their GPU tests share: `grid_of`, `same_bits`, `ulp_distance` and the raw launch of a
workspace-taking entry point, `gpu_stack_call`.  Test modules import from here (and from conftest.py), never from one another.  Every helper
draws from the generator it is given in a fixed, documented order: the tolerances of the tests were measured on those draws.
"""
import contextlib
import ctypes as C
import dataclasses
import functools
import math
import os
import re
import socket

import numpy as np
import pytest
import torch

from oracle import nerfca_oracle as O

# bf16 throughput mode against the oracle that rounds what the kernels round (the derivation: tests/test_hip_parity.py, above
# test_bf16_points_vs_emulating_oracle): outputs <= 2e-3 of the max-norm (measured ~1.5e-4), gradients <= 5e-2 (measured 2e-3 .. 2e-2).
BF_OUT, BF_GRAD = 2e-3, 5e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------------------------------ nets
def model_def(F=128, early=4, late=0, pos_enc="free_windowed", L=12, T=0, gauss=None, sigma=2, cin=3, cout=1, device="cpu"):
    """The definition dict the drop-in CPPN / Temporal are built from."""
    d = dict(num_early_layers=early, num_late_layers=late, num_filters=F, num_input_channels=cin, num_output_channels=cout,
             use_bias=True, pos_enc=pos_enc, pos_enc_window_start=1, pos_enc_basis=L, fourier_sigma=sigma,
             fourier_gaussian=gauss, act_func="relu", device=device)
    if T:
        d.update(num_input_times=1, use_time_latents=True, num_time_dim=T)
    return d


def make_static(params, dev, **kw):
    from nerfca_amd.model.CPPN import CPPN
    m = CPPN(model_def(device=dev, **kw))
    m.load_state_dict(params)
    return m.to(dev)


def make_dynamic(params, dev, **kw):
    from nerfca_amd.model.Temporal import Temporal
    m = Temporal(model_def(device=dev, **kw))
    m.load_state_dict(params)
    return m.to(dev)


def grads_of(model):
    return {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


def spec_from(F, early, late, pos_enc="free_windowed", L=12, T=0, start=1, cin=3, cout=1, coef=None):
    return O.NetSpec(num_filters=F, num_early_layers=early, num_late_layers=late, num_input_channels=cin, num_output_channels=cout,
                     pos_enc=pos_enc, pos_enc_basis=L, pos_enc_window_start=start, num_time_dim=T, fourier_coefficients=coef)


def net_pair(F, early, gen, T=8):
    """Oracle specs and seeded parameters of a static / dynamic pair: (ss, sd, ps, pd).  Draws the static net's parameters first."""
    ss = O.NetSpec(num_filters=F, num_early_layers=early, num_time_dim=0)
    sd = O.NetSpec(num_filters=F, num_early_layers=early, num_time_dim=T)
    return ss, sd, O.init_params(ss, gen), O.init_params(sd, gen)


def bf16_pair(dev, ps, pd, F, early, it_d):
    """The pair on the device in bf16 mode, the static net's band window at iteration 75 000 and the dynamic net's at `it_d` (of 150 000)."""
    from nerfca_amd import set_precision
    s = make_static(ps, dev, F=F, early=early, late=0)
    t = make_dynamic(pd, dev, F=F, early=early, late=0, T=8)
    set_precision("bf16", s, t)
    s.update_freq_mask_alpha(75000, 150000)
    t.update_freq_mask_alpha(it_d, 150000)
    return s, t


# ------------------------------------------------------------------------------------------ ray batches
def ray_inputs(R, S, gen, dtype=torch.float64, unit_dirs=True, z="stratified"):
    """A seeded batch on the CPU: (o, d, ph, z, I0, cp, cs, cd).  Draws, in this order: rand(R, 3) origins, rand(R, 3) directions,
    randint phases, the depths, randn(R) / randn(R, S) / randn(R, S) coefficients of pix / sigma_s / sigma_d.  `dtype` is that of
    o, d and cp.  unit_dirs: directions of length 1.001, else as drawn.  z: "stratified" (one jittered depth vector, rand(S)),
    "per_ray" (sorted rand(R, S)) or None (no draw; z is None)."""
    o = (torch.rand(R, 3, generator=gen) * 0.2 + torch.tensor([3.0, -2.0, 2.5])).to(dtype)
    d = (torch.rand(R, 3, generator=gen) - 0.5).to(dtype)
    if unit_dirs:
        d = d / d.norm(dim=-1, keepdim=True) * 1.001
    ph = torch.randint(0, 10, (R,), generator=gen)
    if z == "stratified":
        z = O.stratified_depths(O.depth_values(3.4259, 5.5741, S), torch.rand(S, generator=gen))
    elif z == "per_ray":
        z = torch.sort(3.4259 + (5.5741 - 3.4259) * torch.rand(R, S, generator=gen), -1)[0]
    else:
        assert z is None, z
    I0 = torch.full((R,), 2.15991)
    cp, cs, cd = torch.randn(R, generator=gen).to(dtype), torch.randn(R, S, generator=gen), torch.randn(R, S, generator=gen)
    return o, d, ph, z, I0, cp, cs, cd


# ------------------------------------------------------------------------------------------ the scalar and its gradients
def oracle_render_grads(ps, ss, pd, sd, win, o, d, ph, I0, z, cp, cs, cd, dt=torch.float32, win_d=None, emulate=None, ray_chunk=None):
    """Outputs and all parameter gradients of the oracle evaluated in dtype `dt` (same f32 query points): (pix, a, b, dists, pso, pdo),
    the gradients in pso[k].grad / pdo[k].grad.  win_d: the dynamic net's band window where it differs from `win`.  emulate: NetSpec
    fields replaced in both specs (emulate_bf16, emulate_fp8_stage, emulate_onchip_last, emulate_stage_formats).  Rays are independent,
    so the backward may run over chunks of `ray_chunk` rays (bounded memory) and add up."""
    R, S = o.shape[0], z.shape[0]
    ss, sd = dataclasses.replace(ss, **(emulate or {})), dataclasses.replace(sd, **(emulate or {}))
    pso = {k: v.clone().to(dt).requires_grad_(True) for k, v in ps.items()}
    pdo = {k: v.clone().to(dt).requires_grad_(True) for k, v in pd.items()}
    w_s, w_d = win.to(dt), (win if win_d is None else win_d).to(dt)
    outs = []
    step = ray_chunk or R
    for r0 in range(0, R, step):
        sl = slice(r0, min(R, r0 + step))
        n = sl.stop - sl.start
        pts = O.query_points(o[sl], d[sl], z).to(dt)
        raw_s = O.static_forward(pso, ss, pts, w_s).reshape(n, S, -1)
        raw_d = O.dynamic_forward(pdo, sd, pts, ph[sl][:, None].repeat(1, S).flatten(), w_d).reshape(n, S, -1)
        pix, a, b, dists = O.composite(raw_s, raw_d, I0[sl].to(dt), d[sl], z.to(dt))
        ((pix * cp[sl]).sum() + (a * cs[sl]).sum() * 50 + (b * cd[sl]).sum() * 50).backward()
        outs.append((pix.detach(), a.detach(), b.detach()))
    pix, a, b = (torch.cat([x[i] for x in outs]) for i in range(3))
    return pix, a, b, dists, pso, pdo


def prefixed_grads(pso, pdo):
    """The oracle's gradients under the keys of hip_render_grads: "s." + name, "t." + name."""
    return {**{"s." + k: v.grad for k, v in pso.items()}, **{"t." + k: v.grad for k, v in pdo.items()}}


def hip_render_grads(s, t, dev, o, d, ph, I0, z, dists, cp, cs, cd, want_depth=False):
    """The library's side of oracle_render_grads: (pix, a, b, g) with g["s." + name] / g["t." + name] (and g["depth"])."""
    from nerfca_amd import render_rays
    for m in (s, t):
        m.zero_grad()
    zz = z.to(dev)
    if want_depth:
        zz = zz[None, :].repeat(o.shape[0], 1).clone().requires_grad_(True)
    pix, a, b = render_rays(s, t, o.to(dev), d.to(dev), ph.to(dev), I0.to(dev), zz, dists.to(dev))
    ((pix * cp.to(dev)).sum() + (a * cs.to(dev)).sum() * 50 + (b * cd.to(dev)).sum() * 50).backward()
    g = {"s." + k: p.grad.detach().clone() for k, p in s.named_parameters()}
    g.update({"t." + k: p.grad.detach().clone() for k, p in t.named_parameters()})
    if want_depth:
        g["depth"] = zz.grad.detach().clone()
    return pix.detach(), a.detach(), b.detach(), g


# ------------------------------------------------------------------------------------------ one-hot upstream gradients
# (tests/test_onehot_grads_cpu.py, tests/test_onehot_grads_gpu.py.)  With one coefficient at one sample (r*, s*) of one net every weight
# gradient is the outer product d_l (x) h_{l-1} of that sample: no sum over samples, no cancellation, so every ENTRY can be held to its own
# row and column scale.  With nets whose ReLU masks are decided by their biases no rounding can flip a mask, on the device or in the oracle.
def wide_layers(spec):
    """(weight key, bias key, takes the skip input cat[feats, h]) of every F-wide layer in order."""
    out = [(f"early_pts_layers.{2 * i}.weight", f"early_pts_layers.{2 * i}.bias", False) for i in range(spec.num_early_layers + 1)]
    if spec.num_late_layers > 0:
        out.append(("skip_connection.0.weight", "skip_connection.0.bias", True))
        out += [(f"late_pts_layers.{2 * i}.weight", f"late_pts_layers.{2 * i}.bias", False) for i in range(spec.num_late_layers - 1)]
    return out


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def wide_preacts(params, spec, feats, dt=torch.float64, emulate_bf16=True):
    """The pre-activations [N, F] of every F-wide layer as O.mlp forms them in dtype `dt` (bf16-rounded operands with `emulate_bf16`);
    feats: the encoded batch (with the gathered latents for a dynamic net)."""
    rnd = _bf if emulate_bf16 else (lambda x: x)
    f = feats.to(dt)
    h, out = f, []
    for wk, bk, skip in wide_layers(spec):
        x = torch.cat([f, h], -1) if skip else h
        z = rnd(x) @ rnd(params[wk].to(dt)).t() + params[bk].to(dt)
        out.append(z)
        h = torch.relu(z)
    return out


def decided_params(spec, gen, feats, sign_share=0.25, phases=None):
    """Seeded parameters whose ReLU masks are decided by the biases: O.init_params(spec, gen), then every F-wide layer in order (early
    layers, the skip layer with cat[feats, h], late layers) has W divided by max |bf16(W) bf16(h)| over all rows of `feats` (f64
    accumulation) and bias[f] = +2 or -2 from a seeded draw with at least `sign_share` of the units on each side -- every pre-activation
    lies in [-3, -1] u [1, 3].  feats: the encoded batch; a dynamic net's latents (drawn here) are gathered by `phases` and appended.
    The output layer stays as initialised.  Returns (params, [smallest |pre-activation| of each layer], the full input rows)."""
    p = O.init_params(spec, gen)
    f = feats.double()
    if spec.num_time_dim > 0:
        f = torch.cat([f, p["time_latents"][phases.long()].double()], -1)
    h, margins = f, []
    for wk, bk, skip in wide_layers(spec):
        x = _bf(torch.cat([f, h], -1) if skip else h)
        P = x @ _bf(p[wk]).double().t()
        p[wk] = (p[wk].double() / P.abs().max()).float()
        F = p[wk].shape[0]
        need = int(math.ceil(sign_share * F))
        on = torch.rand(F, generator=gen) < 0.5
        order = torch.randperm(F, generator=gen)
        for want in (True, False):          # too few of one sign: flip the first units of the seeded order that have the other
            lack = need - int((on == want).sum())
            if lack > 0:
                on[order[on[order] != want][:lack]] = want
        p[bk] = torch.where(on, 2.0, -2.0).float()
        z = x @ _bf(p[wk]).double().t() + p[bk].double()
        margins.append(float(z.abs().min()))
        h = torch.relu(z)
    return p, margins, f


def onehot_coeffs(R, S, net, r, s):
    """(cp, cs, cd) of the scalar of oracle_render_grads / hip_render_grads: zero but for 1.0 at [r, s] of the coefficient of `net`
    ("s": sigma_s, "t": sigma_d)."""
    cp, cs, cd = torch.zeros(R, dtype=torch.float64), torch.zeros(R, S), torch.zeros(R, S)
    (cs if net == "s" else cd)[r, s] = 1.0
    return cp, cs, cd


def rank_one_split(dW, db):
    """Factors of a one-sample weight gradient dW = a (x) u: the row factor a = db, the column factor u = dW[f0] / db[f0] at the row
    f0 of largest |db|.  In f64."""
    a = db.detach().double().reshape(-1)
    W = dW.detach().double().reshape(a.numel(), -1)
    f0 = int(a.abs().argmax())
    return a, W[f0] / a[f0]


def entry_err(got, want, scale=None):
    """Largest |got - want| / |scale| over the entries (scale: `want` itself when None), and its index; an entry whose scale is zero must be
    equal bit for bit (else inf)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    sc = (want if scale is None else scale.detach().double().cpu()).abs().expand_as(want)
    diff = (got - want).abs()
    e = torch.where(sc > 0, diff / sc.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, math.inf), torch.zeros_like(diff)))
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, math.inf))
    i = int(e.argmax())
    return float(e.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape)) if e.dim() else ()


def rank_one_err(dW, db):
    """Check A: the largest relative distance of an entry of dW from db[f] u[j] (rank_one_split), and its (row, column)."""
    a, u = rank_one_split(dW, db)
    return entry_err(dW.reshape(a.numel(), -1), a[:, None] * u[None, :])


def scaled_err(got, want, a, c=None):
    """Check C's metric.  A weight gradient [F, K] with the oracle's row factor a and column factor c: per entry
    |got - want| / (max |a| max(|c_j|, 2^-8 max |c|)) -- columns at their own scale down to 1/256 of the largest, rows at the layer's
    largest delta (a delta is a sum with cancellation even for one sample: a per-row relative measure would be noise).  A bias-like
    vector (c None): |got - want| / max |a|.  Returns the maximum and its index."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    amax = float(a.abs().max())
    if c is None:
        den = torch.full_like(want, amax)
    else:
        c = c.detach().double().abs()
        den = (amax * torch.maximum(c, c.max() * 2.0 ** -8))[None, :].expand_as(want.reshape(-1, c.numel())).reshape(want.shape)
    return entry_err(got, want, den)


ONEHOT_R = 9
ONEHOT_NETS = {"F32_e1": (32, 1, 0), "F64_e2": (64, 2, 0), "F128_e3": (128, 3, 0), "F128_e1_l2": (128, 1, 2), "F32_e0_l1": (32, 0, 1)}   # (F, early, late of the static net)
# (net, S, iteration of the dynamic net's band window) of every ray batch of the one-hot tests.  S = 70: two wave tiles per ray, the second
# with 6 samples; 130: three tiles, the last with 2; 30 000: a window of its own for the dynamic net (the input block is not shared)
ONEHOT_RAY_CASES = [(n, 70, 75000) for n in ONEHOT_NETS] + [("F64_e2", 130, 75000), ("F128_e3", 70, 30000)]
ONEHOT_POINT_CASES = [("F32_e1", 130), ("F128_e3", 130), ("F128_e1_l2", 130), ("F144_e1", 300)]          # F = 144: the general kernels
ONEHOT_POINT_NETS = dict(ONEHOT_NETS, F144_e1=(144, 1, 0), F144_e1_l2=(144, 1, 2), F64_e1=(64, 1, 0))
# The general kernels at their tile, split and run seams (tests/test_onehot_general_cpu.py derives every launch shape named here again from
# `general_launch_shapes` and asserts it; tests/test_onehot_general_gpu.py runs them).  Points: name -> (net, N, one-hot positions).
GENERAL_POINT_CASES = {
    "P1024": ("F144_e1", 1024, (0, 255, 320, 447, 512, 703, 831, 1023)),          # 8 row tiles: the remapped tile order, one position per tile
    "P1100": ("F144_e1", 1100, (0, 1023, 1024, 1099)),                            # 9 row tiles: identity order, a last tile of 76 valid rows
    "P16500": ("F144_e1", 16500, (143, 144, 8255, 16415, 16416, 16499)),          # 129 tiles, 128 splits of 144 rows, 13 of them empty
    "PSKIP": ("F144_e1_l2", 300, (0, 127, 128, 299)),                             # the skip layer's two-segment contraction
}
GENERAL_CHANNEL_CASE = dict(cin=2, cout=3, F=48, early=2, late=1, pos_enc="vanilla", L=5, N=200, launches=((0, 0), (127, 2), (128, 1), (199, 2)))          # PCH: (n*, o*)
# Rays: name -> (static net, S, width of the dynamic net when it differs).  RG: both nets on the general kernels; RMIX: one of them on the fused f32 kernels
GENERAL_RAY_CASES = {"RG": ("F144_e1", 70, None), "RMIX_64_144": ("F64_e1", 70, 144), "RMIX_144_64": ("F144_e1", 70, 64)}
BF_FACTOR = 2.0 ** -6          # check C, bf16 operands: one bf16 step is at most 2^-7 of a value, once on each factor


def onehot_launches(S):
    """[((r, s) of the static net's one-hot, (r, s) of the dynamic net's)]: the sample positions are both 32-column halves of a wave tile,
    their edges, the first sample of the ragged tile and its last; the rays 0, R - 1 and 4.  The two nets' one-hots of a launch sit at
    different rays (and samples)."""
    pos = list(zip((0, ONEHOT_R - 1, 4, 0, ONEHOT_R - 1, 4), (0, 31, 32, 63, 64, S - 1)))
    return [(pos[i], pos[(i + 1) % 6]) for i in range(6)]


def onehot_emulations(S):
    """NetSpec fields of the oracle that rounds what each backward plan rounds."""
    return {"f32": {}, "recompute": dict(emulate_bf16=True, emulate_stage_formats=None),
            "bf16_store": dict(emulate_bf16=True, emulate_fp8_stage=S, emulate_stage_formats=("bf16", "bf16")),
            "fp8_store": dict(emulate_bf16=True, emulate_fp8_stage=S)}


def onehot_factor_errs(spec, got, want):
    """Check C over one net: [(parameter name, scaled_err, index)] of every parameter of `got` against the oracle's `want`: weights of the
    F-wide layers with the oracle's row and column factors, biases at the layer's largest delta, the output layer and the latents in
    the vector form at their own largest entry."""
    out = []
    for wk, bk, _ in wide_layers(spec):
        a, c = rank_one_split(want[wk], want[bk])
        out.append((wk,) + scaled_err(got[wk], want[wk], a, c))
        out.append((bk,) + scaled_err(got[bk], want[bk], a))
    for k in want:
        if k.startswith("output_linear") or k == "time_latents":
            out.append((k,) + scaled_err(got[k], want[k], want[k].double()))
    return out


class _OnehotOracle:
    """Memo of the oracle's one-hot gradients of a pair of nets and of check C's floor."""

    def __init__(self):
        self._memo = {}

    def spec(self, net):
        return self.ss if net == "s" else self.sd

    def params(self, net):
        return self.ps if net == "s" else self.pd

    def oracle(self, i, emu, dt=torch.float64):
        """{"s." / "t." + parameter name: gradient} of one-hot launch i, from the oracle with the roundings of plan `emu` in dtype dt."""
        key = (i, emu, dt)
        if key not in self._memo:
            self._memo[key] = self._run(i, emu, dt)
        return self._memo[key]

    def floor(self, i, emu):
        """{prefixed parameter name: scaled_err of the f32 emulating oracle from the f64 one}: the floor of check C."""
        g32, g64 = self.oracle(i, emu, torch.float32), self.oracle(i, emu)
        out = {}
        for net in self.nets:
            sub = lambda g: {k[2:]: v for k, v in g.items() if k[0] == net}          # noqa: E731
            out.update({net + "." + k: e for k, e, _ in onehot_factor_errs(self.spec(net), sub(g32), sub(g64))})
        return out


class OnehotRays(_OnehotOracle):
    """A static / dynamic pair of decided nets on one seeded batch of ONEHOT_R rays x S samples."""
    nets = "st"

    def __init__(self, name, S, it_d, Fd=None):
        super().__init__()
        F, early, late = ONEHOT_POINT_NETS[name]
        self.name, self.S, self.it_d, self.F, self.early, self.late = name, S, it_d, F, early, late
        self.Fd = Fd or F                     # the dynamic net's width (Fd: where it differs from the static net's)
        self.early_d = max(early, 1)          # the dynamic net is plain (a Temporal with late layers has no output in the reference)
        gen = torch.Generator().manual_seed(9100 + 7 * F + 3 * early + late + S + it_d // 1000 + (11 * Fd if Fd else 0))
        self.ss, self.sd = spec_from(F, early, late), spec_from(self.Fd, self.early_d, 0, T=8)
        self.win, self.win_d = O.freq_mask_alpha(12, 75000, 150000, 1)[0], O.freq_mask_alpha(12, it_d, 150000, 1)[0]
        self.o, self.d, self.ph, self.z, self.I0 = ray_inputs(ONEHOT_R, S, gen)[:5]
        self.dists = O.ray_dists(self.z, torch.float64)
        pts = O.query_points(self.o, self.d, self.z)
        self.ps, self.margin_s, self.feats_s = decided_params(self.ss, gen, O.encode(pts, self.ss, self.win))
        self.pd, self.margin_d, self.feats_d = decided_params(self.sd, gen, O.encode(pts, self.sd, self.win_d), phases=self.ph[:, None].repeat(1, S).flatten())
        self.launches = onehot_launches(S)

    def feats(self, net, r, s):
        """The f64 input row (the encoded f32 query point, then the latents) of sample (r, s)."""
        return (self.feats_s if net == "s" else self.feats_d)[r * self.S + s]

    def coeffs(self, i):
        """(cp, cs, cd) of launch i over the whole batch."""
        (rs, s_s), (rd, s_d) = self.launches[i]
        cp, cs, _ = onehot_coeffs(ONEHOT_R, self.S, "s", rs, s_s)
        return cp, cs, onehot_coeffs(ONEHOT_R, self.S, "t", rd, s_d)[2]

    def _run(self, i, emu, dt):
        # the oracle runs on the launch's two rays only: rays are independent and tile scales are per ray
        (rs, s_s), (rd, s_d) = self.launches[i]
        rows = torch.tensor([rs, rd])
        cs, cd = onehot_coeffs(2, self.S, "s", 0, s_s)[1], onehot_coeffs(2, self.S, "t", 1, s_d)[2]
        pso, pdo = oracle_render_grads(self.ps, self.ss, self.pd, self.sd, self.win, self.o[rows], self.d[rows], self.ph[rows], self.I0[rows], self.z,
                                       torch.zeros(2, dtype=torch.float64), cs, cd, dt=dt, win_d=self.win_d, emulate=onehot_emulations(self.S)[emu])[4:]
        return {k: v.detach() for k, v in prefixed_grads(pso, pdo).items()}


class OnehotPoints(_OnehotOracle):
    """Decided nets on N seeded points for CPPN.forward / Temporal.forward_composite; launch i puts the one-hot `gout` at ns[i] (static
    net) and ns[i - 1] (dynamic net: a plain one beside a static net with a skip layer)."""

    def __init__(self, name, N, ns=None):
        super().__init__()
        F, early, late = ONEHOT_POINT_NETS[name]
        self.name, self.N, self.F, self.early, self.late, self.early_d = name, N, F, early, late, max(early, 1)
        gen = torch.Generator().manual_seed(9700 + 7 * F + 3 * early + late + N)
        self.ss, self.sd = spec_from(F, early, late), spec_from(F, self.early_d, 0, T=8)
        self.win = O.freq_mask_alpha(12, 75000, 150000, 1)[0]
        self.x = torch.rand(N, 3, generator=gen) * 2 - 1
        self.ts = torch.randint(0, 10, (N,), generator=gen)
        self.ps, self.margin_s, self.feats_s = decided_params(self.ss, gen, O.encode(self.x, self.ss, self.win))
        self.pd, self.margin_d, self.feats_d = decided_params(self.sd, gen, O.encode(self.x, self.sd, self.win), phases=self.ts)
        self.nets = "st"
        self.ns = list(ns) if ns is not None else ([0, 63, 64, 129] if N == 130 else [0, 127, 128, N - 1])
        self.launches = [(self.ns[i], self.ns[i - 1]) for i in range(len(self.ns))]

    def feats(self, net, n):
        return (self.feats_s if net == "s" else self.feats_d)[n]

    def _run(self, i, emu, dt):
        out = {}
        for net, n in zip("st", self.launches[i]):
            spec = dataclasses.replace(self.spec(net), emulate_bf16=emu != "f32")
            p = {k: v.clone().to(dt).requires_grad_(True) for k, v in self.params(net).items()}
            x = self.x[n:n + 1].to(dt)
            y = O.static_forward(p, spec, x, self.win.to(dt)) if net == "s" else O.dynamic_forward(p, spec, x, self.ts[n:n + 1], self.win.to(dt))
            y.sum().backward()
            out.update({net + "." + k: v.grad.detach() for k, v in p.items()})
        return out


@functools.lru_cache(maxsize=None)
def onehot_rays(name, S=70, it_d=75000):
    return OnehotRays(name, S, it_d)


@functools.lru_cache(maxsize=None)
def onehot_points(name, N):
    return OnehotPoints(name, N)


class OnehotChannels(_OnehotOracle):
    """PCH: one decided static net with other channel counts than 3 -> 1 (GENERAL_CHANNEL_CASE: the shape of test_wide_nets.CHANNEL_CASES[0]) on N seeded
    points; launch i puts the one-hot `gout` at [n*, o*] = launches[i] -- one point AND one output channel."""
    nets = "s"

    def __init__(self):
        super().__init__()
        k = GENERAL_CHANNEL_CASE
        self.name, self.N, self.F, self.early, self.late, self.cin, self.cout = "c2to3", k["N"], k["F"], k["early"], k["late"], k["cin"], k["cout"]
        gen = torch.Generator().manual_seed(9900 + 7 * self.F + self.N)
        self.ss = spec_from(self.F, self.early, self.late, k["pos_enc"], k["L"], cin=self.cin, cout=self.cout)
        self.x = torch.rand(self.N, self.cin, generator=gen) * 2 - 1
        self.ps, self.margin_s, self.feats_s = decided_params(self.ss, gen, O.encode(self.x, self.ss, None))
        self.launches = list(k["launches"])

    def feats(self, net, n):
        return self.feats_s[n]

    def _run(self, i, emu, dt):
        n, o = self.launches[i]
        p = {k: v.clone().to(dt).requires_grad_(True) for k, v in self.ps.items()}
        O.static_forward(p, self.ss, self.x[n:n + 1].to(dt), None)[0, o].backward()
        return {"s." + k: v.grad.detach() for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def general_case(name):
    """The case `name` of GENERAL_POINT_CASES / GENERAL_RAY_CASES, or "PCH"."""
    if name == "PCH":
        return OnehotChannels()
    if name in GENERAL_POINT_CASES:
        net, N, ns = GENERAL_POINT_CASES[name]
        return OnehotPoints(net, N, ns)
    net, S, Fd = GENERAL_RAY_CASES[name]
    return OnehotRays(net, S, 75000, Fd)


def _up(a, b):
    return (a + b - 1) // b * b


def general_layout(F, NL, Kenc, T=0, P=0, cout=1, skip=None):
    """What nca_build_layout_wide (nca_wide.hpp) derives of a net on the general kernels: K0 = Kenc + T, K0p = round_up(K0 + P, 16), the fan-in
    Kp of every layer (layer 0: K0p; the skip layer `skip`: K0p + F; else F) and the floats of the packed image, which is also one split slab:
    sum F Kp | biases NL F | Wo cout F | bo cout, rounded up to 4."""
    K0 = Kenc + T
    K0p = _up(K0 + P, 16)
    Kp = [K0p if j == 0 else (K0p + F if j == skip else F) for j in range(NL)]
    return dict(F=F, NL=NL, K0=K0, K0p=K0p, Kp=Kp, P=P, packed=_up(sum(F * k for k in Kp) + NL * F + cout * F + cout, 4))


def general_plan(y, N, bwd=True, max_bytes=0):
    """wide_plan of nca_api_wide.inc restated: (rows per chunk, nsplit, workspace bytes) of N samples under a workspace of max_bytes (0: no cap).
        rows_all = align_up(N, 128); chunk = min(rows_all, 2^18); tiles = ceil(F / 128)^2; want = max(512 / tiles, 1)
        nsplit = min(want, chunk / 128)
        floats = chunk K0p + chunk F (bwd ? NL : 2) + (bwd ? (NL - 1) (chunk / 128) ceil(F / 128) 512 + 2 chunk F + nsplit packed + F P : 0)
        over max_bytes and chunk > 128: chunk = align_up(chunk / 2, 128), again"""
    F, NL = y["F"], y["NL"]
    chunk = min(_up(N, 128), 1 << 18)
    nt = (F + 127) // 128
    want = max(512 // (nt * nt), 1)
    while True:
        nsplit = min(want, chunk // 128)
        floats = chunk * y["K0p"] + chunk * F * (NL if bwd else 2)
        if bwd:
            floats += (NL - 1) * (chunk // 128) * nt * 512 + 2 * chunk * F + nsplit * y["packed"] + F * y["P"]
        nbytes = _up(floats * 4, 256)
        if max_bytes <= 0 or nbytes <= max_bytes or chunk <= 128:
            return chunk, nsplit, nbytes
        chunk = _up(chunk // 2, 128)


def general_gemm_shape(kind, rows, cols, nsplit=1, ktot=0):
    """The launch arithmetic of nca_wide_gemm (nca_kernels_wide.hip) restated:
        nrt = ceil(rows / 128), nct = ceil(cols / 128); gs = wgrad ? nrt nct : nct (workgroups per group); ng = wgrad ? nsplit : nrt (groups)
        (ng & 7) == 0: the XCD-aware remap  q = lid >> 3, member = q % gs, group = (q / gs) 8 + (lid & 7); else member = lid % gs, group = lid / gs
        wgrad: per = round_up(ceil(ktot / nsplit), 16); split z contracts [z per, min((z + 1) per, ktot)): empty when z per >= ktot
    Returns dict(nrt, nct, gs, ng, remap, per, empty: the number of empty splits, tiles: the (group, member) of every workgroup id)."""
    nrt, nct = (rows + 127) // 128, (cols + 127) // 128
    wgrad = kind == "wgrad"
    gs, ng = (nrt * nct, nsplit) if wgrad else (nct, nrt)
    remap = ng % 8 == 0
    tiles = []
    for lid in range(gs * ng):
        q = lid >> 3
        tiles.append(((q // gs) * 8 + (lid & 7), q % gs) if remap else (lid // gs, lid % gs))
    per = _up((ktot + nsplit - 1) // nsplit, 16) if wgrad else 0
    empty = sum(1 for z in range(nsplit) if z * per >= ktot) if wgrad else 0
    return dict(nrt=nrt, nct=nct, gs=gs, ng=ng, remap=remap, per=per, empty=empty, tiles=tiles)


def general_ray_runs(R, S, need_of_rays, budget):
    """plan_ray_chunks of nca_api_wide.inc restated: rays per run of a backward that recomputes -- rays = min(R, 2^18 / S), halved ((rays + 1) / 2) while the
    regions of a run of `rays` rays (need_of_rays(rays), bytes) exceed `budget` and rays > 1."""
    rays = max(1, min(R, (1 << 18) // S))
    while need_of_rays(rays) > budget and rays > 1:
        rays = (rays + 1) // 2
    return rays


def onehot_latent_rows(tl, phase, tag):
    """Check B on d loss / d time_latents [10, T] of a one-hot at a sample of heart phase `phase`: every other row is zero bit for bit."""
    rest = tl.detach().cpu()[torch.arange(tl.shape[0]) != phase]
    assert not bool(rest.any()), (tag, "time_latents", "B: latent rows", torch.nonzero(rest)[:4].tolist())
    assert bool(tl[phase].detach().cpu().any()), (tag, "time_latents", "the sample's own row is zero")


def onehot_checks_ab(spec, params, g, x, tag, deltas_nonzero=True):
    """Checks A and B on one net's one-hot gradients g = {parameter name: gradient} for the sample with input row x (f64, the oracle's):
    every F-wide layer's weight gradient is db (x) u to 2^-20 per entry (one sample's entry is one product -- at most nine partial products of
    the exact 3-way bf16 split in f32 mode -- so sixteen f32 roundings is generous; a skip layer: over its K0 + F columns); rows of off
    units (the bias is -2), columns whose input is exactly zero (an off unit of the previous layer, an encoded feature that is zero) are
    zero bit for bit; everything is finite.  Returns the worst check-A error."""
    worst = 0.0
    h, f = x, x
    for k, v in g.items():
        assert bool(torch.isfinite(v).all()), (tag, k)
    for wk, bk, skip in wide_layers(spec):
        xin = torch.cat([f, h]) if skip else h
        dW, db = g[wk].cpu(), g[bk].cpu()
        off = params[bk] < 0
        assert off.any() and not off.all()
        assert not bool(db[off].any()) and not bool(dW[off].any()), (tag, wk, "B: off-unit rows", torch.nonzero(dW[off])[:4].tolist())
        assert not deltas_nonzero or bool((db[~off] != 0).all()), (tag, bk, "an on unit without a delta")          # (an e5m2 delta may underflow)
        assert not bool(dW[:, xin == 0].any()), (tag, wk, "B: columns of zero inputs", torch.nonzero(dW[:, xin == 0])[:4].tolist())
        e, at = rank_one_err(dW, db)
        assert e <= 2.0 ** -20, (tag, wk, "A: row, column", at, e)
        worst = max(worst, e)
        h = torch.relu(_bf(xin) @ _bf(params[wk]).double().t() + params[bk].double())          # (only its zeros are used)
    dWo, dbo = g["output_linear.0.weight"].cpu(), g["output_linear.0.bias"].cpu()
    assert not bool(dWo[:, h == 0].any()), (tag, "output_linear.0.weight", "B: columns of off units")
    e, at = rank_one_err(dWo, dbo)
    assert e <= 2.0 ** -20, (tag, "output_linear.0.weight", at, e)
    return max(worst, e)


def onehot_channel_rows(dWo, dbo, o, tag):
    """Check B on the output layer [Cout, F] of a one-hot at output channel o: every other row of dWo and entry of dbo is zero bit for bit (no
    leakage between the output channels), and dbo[o] is the coefficient itself, exactly 1."""
    rest = torch.arange(dbo.numel()) != o
    assert not bool(dWo[rest].any()) and not bool(dbo[rest].any()), (tag, "B: output channels other than o*", torch.nonzero(dWo[rest])[:4].tolist())
    assert float(dbo[o]) == 1.0, (tag, "dbo[o*]", float(dbo[o]))


def oracle_fine_sampler(sig_s, sig_d, z, u, reduce_max=None):
    """fused.fine_depths signature with the oracle's arithmetic (model_helpers.py:131-148, 162-187)."""
    R = sig_s.shape[0]
    tsum = sig_s + sig_d
    w = torch.cat([torch.full((R, 1), 1e-10), (tsum[:, 1:] - tsum[:, :-1]).abs()], -1)
    wmax = w.max().reshape(1).clone()
    if reduce_max is not None:
        reduce_max(wmax)
    w = w / wmax
    zb = z[None, :].repeat(R, 1)
    mid = 0.5 * (zb[:, 1:] + zb[:, :-1])
    return torch.sort(torch.cat([O.sample_pdf(mid, w[:, 1:-1], u), zb], -1), -1)[0]


@contextlib.contextmanager
def count_launches(out, kinds=("fwd", "bwd_dgrad")):
    """Appends to `out` the number of launches of each kind inside the block: a tuple, or the one number when one kind is asked for."""
    from nerfca_amd import _capi
    _capi.timing_reset()
    _capi.timing_enable(True)
    try:
        yield
    finally:
        n = tuple(_capi.timing_read(k)[1] for k in kinds)
        out.append(n if len(n) > 1 else n[0])
        _capi.timing_enable(False)
        _capi.timing_reset()


# ------------------------------------------------------------------------------------------ the view sections' C ABI, without a launch
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
FAKE = 0x1000          # a non-NULL pointer a refused call never reads


@pytest.fixture(scope="module")
def capi():
    from nerfca_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def lib(capi):
    return capi.lib()


def declared_bound_and_exported(capi, names):
    """Every name is declared in include/nerfca_hip.h, bound in _capi.SYMBOLS and exported by the library, at ABI 13.  Returns the header's
    text for the caller's own assertions about it."""
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "nerfca_hip.h")).read()
    declared = set(re.findall(r"\b(nca_[a-z0-9_]+)\s*\(", header))
    raw = C.CDLL(capi.LIB_PATH)
    for name in names:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(raw, name), name
    assert capi.ABI_VERSION == 13 and capi.lib().nca_abi_version() == 13
    assert int(re.search(r"#define NCA_ABI_VERSION (\d+)", header).group(1)) == 13
    return header


def refused(section, capi, lib, rc, *words, code=E_INVALID):
    """The call returned `code`, the section's own message (nca_<section>_last_error) holds every word, and check_<section> raises with it."""
    msg = getattr(lib, f"nca_{section}_last_error")().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    with pytest.raises(capi.NcaError) as e:
        getattr(capi, f"check_{section}")(rc)
    assert msg in str(e.value)


def grid(capi, n=(5, 3, 4), lo=(-1.0, -1.0, -1.0), inv=(2.0, 1.0, 1.5), reserved=0):
    return capi.NcaGrid(lo=(C.c_double * 3)(*lo), inv=(C.c_double * 3)(*inv), n=(C.c_int32 * 3)(*n), reserved=reserved)


def grid_refusals(section, capi, lib, call):
    """Every refusal of a bad NcaGrid, for an entry point of `section`: `call(g, count)` makes the call with the descriptor g and `count`
    volumes or phases (None: the test's own default), everything else valid."""
    def no(g, *words, count=None):
        refused(section, capi, lib, call(g, count), *words)

    for a in range(3):
        for bad in (1, -6):
            n = [5, 3, 4]
            n[a] = bad
            no(grid(capi, n=n), f"n[{a}] = {bad}", "2 nodes")
        for bad, word in ((math.inf, "inf"), (-math.inf, "-inf"), (math.nan, "nan")):
            lo, inv = [-1.0] * 3, [2.0, 1.0, 1.5]
            lo[a] = bad
            no(grid(capi, lo=lo), f"lo[{a}] = {word}", "finite")
            inv[a] = bad
            no(grid(capi, inv=inv), f"inv[{a}] = {word}", "finite")
        for bad, word in ((0.0, "0"), (-0.25, "-0.25"), (-2.0, "-2")):
            inv = [2.0, 1.0, 1.5]
            inv[a] = bad
            no(grid(capi, inv=inv), f"inv[{a}] = {word}", "positive")
    for bad in (3, 7):
        no(grid(capi, reserved=bad), f"reserved = {bad}")
    big = (1 << 31) - 1
    no(grid(capi, n=(big, big, big)), "overflow", str(big))
    no(grid(capi, n=(1 << 20, 1 << 20, 1 << 20)), "overflow", str(1 << 20), count=4)          # 2^60 voxels x 4 x at least 4 bytes


# ------------------------------------------------------------------------------------------ the view sections on the GPU
def grid_of(shape, inv=(1.0, 2.0, 0.5)):
    """The NcaGrid of the raw launches: a lo that is not 0 and, unless given, a spacing of its own on every axis."""
    from nerfca_amd import _capi
    return grid(_capi, n=shape, lo=(0.0, -1.0, 2.0), inv=inv)


def same_bits(got, want):
    """Two f32 numpy arrays of one shape with the same bits (NaN payloads and the sign of zero included)."""
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def ulp_distance(got, want):
    """Whole steps of their format between two f32 or two f64 numpy arrays, entry by entry (as f64; between values of one sign, inf equals inf)."""
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    kind = {4: np.int32, 8: np.int64}[want.dtype.itemsize]
    return np.abs(got.view(kind).astype(np.float64) - want.view(kind).astype(np.float64))


def gpu_stack_call(dev, check, fn, query, g, vol, args, fill, dtype, node_bytes, out_shape=None, query_args=()):
    """The output (numpy) of one raw call `fn(g, vol, n_vol, *args, out, work, work_bytes, stream)` on the f32 stack `vol` [n_vol,n0,n1,n2]: `out`
    (of `dtype`, the stack's shape unless given) is pre-filled with `fill`, so a node the kernels did not write shows; the workspace is exactly as
    large as `query(g, n_vol, *query_args)` says -- at least `node_bytes` per node in whole 256-byte lines, none at all when `node_bytes` is 0 --
    and pre-filled with 0xff bytes."""
    from nerfca_amd import _capi, fused
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    n_vol = vol.shape[0]
    x = torch.tensor(vol).to(dev)
    out = torch.full(vol.shape if out_shape is None else out_shape, fill, dtype=dtype, device=dev)
    nbytes = query(C.byref(g), n_vol, *query_args)
    assert (nbytes >= node_bytes * vol.size and nbytes % 256 == 0) if node_bytes else nbytes == 0
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        check(fn(C.byref(g), _capi.ptr(x), n_vol, *args, _capi.ptr(out), _capi.ptr(work), nbytes, fused._stream()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ graph replay: the input sequences of both halves
# (tests/test_graph_replay_gpu.py replays every captured entry point on these inputs in this order; tests/test_graph_replay_cpu.py proves with
# the numpy references that a clear which did nothing under replay -- a running maximum, a running sum -- would show on every replay after the
# first.)  The order makes stale state visible: the amplitudes fall, so every maximum falls strictly; the threshold stays, so the mask shrinks
# and the components change; every sum moves by far more than its tolerance.
REPLAY_INPUTS = 3                      # inputs per case; the last one is replayed twice
REPLAY_AMPLITUDES = (1.0, 0.7, 0.45)
REPLAY_THRESHOLD = 0.3                 # of the label, edt, city-block and iso-surface cases: 70 %, 57 % and 33 % of the nodes lie above it
REPLAY_TILE_SHAPE = (5, 9, 65)         # one node past the 4 x 8 x 64 tile on every axis
REPLAY_LINE_SHAPE = (3, 5, 65)         # edt and filt: one node past a chunk of 64
REPLAY_ZOOM = ((3, 5, 70), (6, 5, 33))
REPLAY_DRR_SHAPE = (5, 3, 4)
REPLAY_SSIM = (11, (27, 43))           # window 11: 17 x 33 positions, one row and one column past the 16 x 32 tile
REPLAY_VESS_SCALE = 2.25
REPLAY_VESS_SIGMAS = (1.0, 1.5)
REPLAY_LABEL_CAP = 64
REPLAY_MLP = ("F144_e1", 300)          # the one-hot module's general-kernel point case
REPLAY_RAYS = (7, 40)                  # R, S of the render case: both nets general (144 units)


def replay_volumes(shape, k, n_vol=2):
    """Input k of a volume case: f32 [n_vol, n0, n1, n2], uniform in [0, REPLAY_AMPLITUDES[k]); the volumes of a stack differ."""
    rng = np.random.default_rng(4100 + 10 * k + 7 * shape[0] + 3 * shape[1] + shape[2])
    return (rng.random((n_vol,) + tuple(shape)) * REPLAY_AMPLITUDES[k]).astype(np.float32)


def replay_images(k):
    """Input k of the ssim cases: (x, y, range) with x, y f32 [2, H, W] and range f64 [2].  The truth y stays; the prediction x is y under noise
    that grows with k, so every image's sum of S falls by tens from input to input."""
    H, W = REPLAY_SSIM[1]
    y = np.random.default_rng(4200).random((2, H, W)).astype(np.float32)
    noise = np.random.default_rng(4201 + k).random((2, H, W)) - 0.5
    x = np.clip(y + (0.05, 0.3, 0.9)[k] * noise, 0.0, 1.0).astype(np.float32)
    return x, y, np.array([1.0, 1.0])


def replay_drr_rays():
    """(o f64 [64, 3], d f64 [64, 3], z f32 [16], dists f64 [16]): the 8 x 8 detector of the drr tests, from the host geometry."""
    import drr_ref
    _, geo, S = drr_ref.geometries()[0]
    o, d = drr_ref.host_rays(geo, *drr_ref.VIEWS[0])
    z, dists = drr_ref.depths(geo, S)
    return o, d, z, dists


def replay_pixel_gradients(k, R):
    """Input k of the back-projection case: g_pix f64 [2, R], its size falling with REPLAY_AMPLITUDES."""
    return np.random.default_rng(4300 + k).standard_normal((2, R)) * REPLAY_AMPLITUDES[k]


def replay_upstream(k, shape):
    """Input k of the general kernels' cases: an upstream gradient f32 of `shape`."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(4400 + k)) * REPLAY_AMPLITUDES[k]


def replay_phantom_tables(k, P=2, n_ell=3, n_seg=7):
    """Input k of the phantom case: (ell f64 [P, n_ell, 14], seg f64 [P, n_seg, 8])."""
    import phantom_ref
    return (phantom_ref.random_ellipsoids(P, n_ell, phantom_ref.BOUNDS, seed=4500 + k),
            phantom_ref.random_segments(P, n_seg, phantom_ref.BOUNDS, seed=4600 + k, r_max=0.35))


# The tolerances of the outputs summed with floating-point atomics, restated from the GPU tests of their sections (no new number): both halves
# of the replay tests take them from here.
def replay_ssim_tol(want):
    """tests/test_ssim_gpu.py sum_bound: f64 [N] from ssim_ref.ssim_stack's dict."""
    return 2 * want["count"] * 2.0 ** -53 * want["abs_sum"] + 4 * 2.0 ** -52 * want["abs_sum"]


def replay_voltv_tol(want):
    """tests/test_voltv_gpu.py value_bounds: (space, time) from voltv_ref.total_variation's dict."""
    return np.array([2 * want["count_space"] * 2.0 ** -53 * want["abs_space"], 2 * want["count_time"] * 2.0 ** -53 * want["abs_time"]])


def replay_drr_tol(mass, count):
    """tests/test_drr_grad_gpu.py: count 2^-53 mass per node, from drr_adjoint_ref.backproject's mass [n_vol, ...] and count [...]."""
    return count[None] * 2.0 ** -53 * mass


def replay_references():
    """The numpy references of the accumulating outputs over the input sequences, computed once: a dict of lists over the inputs
    norm_max f64 [2]; sizes int32 [2, cap] and counts; ssim (sum [2], tol [2]); voltv (values [2], tol [2]); drr (g_vol, tol) [2, voxels]."""
    return _replay_references()


@functools.lru_cache(maxsize=None)
def _replay_references():
    import drr_adjoint_ref
    import drr_ref
    import label_ref
    import ssim_ref
    import vess_ref
    import voltv_ref
    out = dict(norm_max=[], sizes=[], counts=[], ssim=[], voltv=[], drr=[])
    o, d, z, dists = replay_drr_rays()
    for k in range(REPLAY_INPUTS):
        vol = replay_volumes(REPLAY_TILE_SHAPE, k)
        out["norm_max"].append(vess_ref.norm_max(vol, REPLAY_VESS_SCALE))
        labels, counts = label_ref.label(vol, REPLAY_THRESHOLD, 1)
        out["sizes"].append(label_ref.sizes(labels, REPLAY_LABEL_CAP))
        out["counts"].append(counts)
        x, y, rng = replay_images(k)
        w = ssim_ref.ssim_stack(x, y, rng, ssim_ref.gaussian(REPLAY_SSIM[0]))
        out["ssim"].append((w["sum"], replay_ssim_tol(w)))
        w = voltv_ref.total_variation(vol, voltv_ref.grid_inv(REPLAY_TILE_SHAPE, drr_ref.BOUNDS), voltv_ref.EPS_S, voltv_ref.EPS_T, True)
        out["voltv"].append((np.array([w["space"], w["time"]]), replay_voltv_tol(w)))
        g_vol, mass, count = drr_adjoint_ref.backproject(REPLAY_DRR_SHAPE, 2, o, d, z, dists, replay_pixel_gradients(k, o.shape[0]), drr_ref.BOUNDS)
        out["drr"].append((g_vol.reshape(2, -1), replay_drr_tol(mass.reshape(2, -1), count.reshape(-1))))
    return out


@functools.lru_cache(maxsize=None)
def replay_mlp_case():
    """The general kernels' point case: (spec, parameters, points f32 [300, 3], band window) of a static net of 144 units."""
    F, early, late = ONEHOT_POINT_NETS[REPLAY_MLP[0]]
    gen = torch.Generator().manual_seed(4700)
    spec = spec_from(F, early, late)
    return spec, O.init_params(spec, gen), torch.rand(REPLAY_MLP[1], 3, generator=gen) * 2 - 1, O.freq_mask_alpha(12, 75000, 150000, 1)[0]


@functools.lru_cache(maxsize=None)
def replay_ray_case():
    """The general kernels' ray case, both nets of 144 units at R, S = REPLAY_RAYS: dict(ss, sd, ps, pd, win, o, d, ph, z, dists, I0) on the CPU."""
    R, S = REPLAY_RAYS
    gen = torch.Generator().manual_seed(4800)
    ss, sd = spec_from(144, 1, 0), spec_from(144, 1, 0, T=8)
    ps, pd = O.init_params(ss, gen), O.init_params(sd, gen)
    o, d, ph, z, I0 = ray_inputs(R, S, gen)[:5]
    return dict(ss=ss, sd=sd, ps=ps, pd=pd, win=O.freq_mask_alpha(12, 75000, 150000, 1)[0], o=o, d=d, ph=ph, z=z, dists=O.ray_dists(z, torch.float64), I0=I0)


def replay_ray_upstream(k):
    """Input k of the ray case: (g_pix f64 [R], g_sigma_s f32 [R, S], g_sigma_d f32 [R, S])."""
    R, S = REPLAY_RAYS
    g = replay_upstream(k, (2 * S + 1, R))
    return g[0].double().contiguous(), g[1:S + 1].t().contiguous(), g[S + 1:].t().contiguous()
