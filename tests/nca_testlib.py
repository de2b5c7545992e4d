"""Shared helpers of the suite: the `dev` fixture, net construction, seeded ray batches, the oracle's and the library's gradients of
the scalar every render-parity test differentiates,

    sum(pix * cp) + 50 sum(sigma_s * cs) + 50 sum(sigma_d * cd),

launch counting, the bf16 bounds, and what the launch-free tests of the view sections (csrc/view/) share: the `capi` / `lib` fixtures, the
declared-bound-exported check, `refused` and the one list of NcaGrid refusals.  Test modules import from here (and from conftest.py), never from one another.  Every helper
draws from the generator it is given in a fixed, documented order: the tolerances of the tests were measured on those draws.
"""
import contextlib
import ctypes as C
import dataclasses
import math
import os
import re
import socket

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
