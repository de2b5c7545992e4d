"""Every entry of every parameter gradient of the GENERAL kernels (nca_kernels_wide.hip, host side nca_api_wide.inc) held to the f64 oracle at their tile,
split and run seams, with the one-hot upstream gradients, the decided nets and the checks A, B, C of tests/test_onehot_grads_gpu.py (helpers and
cases: tests/nca_testlib.py; the launch shapes each case is listed for are derived again and asserted in tests/test_onehot_general_cpu.py, which
also holds the seeded faults these checks catch and rel_err does not).

Cases (F = 144: tiles = 4, want = 128, K0p = 80 static / 96 dynamic):
  P1024   rows 1024, 8 row tiles: forward and dgrad in the XCD-remapped tile order with 2 workgroups per group; nsplit = 8, per = 128: wgrad remapped
          with 4 (hidden part) and 2 (encoded part) workgroups per group.  One one-hot per row tile.
  P1100   rows 1152, 9 row tiles and splits: identity order, the last tile with 76 valid rows.
  P16500  rows 16512 = 129 tiles, nsplit = 128, per = 144: the seam 143 | 144 lies inside row tile 1, splits 115 .. 127 are empty and must still be
          written (nca_wide_reduce sums all 128); nca_wide_colsum cuts the same rows at per = 129.  Poisoned buffers.
  PSKIP   a skip layer (j = 2 of 4): the two-segment contraction of the forward, the two-part wgrad, the offset dgrad.
  PCH     2 -> 3 channels, F = 48: the `o` loops of nca_wide_head_bwd / nca_wide_colsum and gsum; a one-hot at one point AND one channel.
  RG      render_bwd_general with both nets on the general kernels: (i) from the general store, (ii) recomputed in one run, (iii) recomputed in runs of
          5 and of 3 whole rays (workspace caps taken from the library's own query).  Poisoned buffers.
  RMIX    one net on the fused f32 kernels beside one on the general kernels, either way round: no store, the fused net's backward last from g_raw.

Checks: A (rank one to 2^-20), B (exact zeros), C (scaled_err within max(1e-5, 3 floor) of the f64 oracle) on every launch, and
  F  placement invariance, exact: with a one-hot upstream gradient every other sample's row of every D_j is an exact zero, so every partial sum of the
     general kernels (MFMA slabs, rowsum, split slabs, nca_wide_reduce, esum -> nca_wide_latgrad, grads += per chunk) adds zeros to one product
     chain, and the forward of a row does not depend on its place in a tile: the gradients are the same BITS under every chunking of the same launch.

Measured on an MI355X (profiles/onehot_general.txt, written by this module when NERFCA_ONEHOT_GENERAL_RECORD names a file; 10 tests, 3 s):
  A  <= 1.2e-7 on the general kernels (1.8e-7 on the fused f32 net of RMIX); dWo[o*] against the f64 oracle's h(n*): 8.5e-8;
  C  the first layer's weights at the f32 oracle's own floor (6.2e-6 .. 2.6e-4: the rounded argument of a high band's cosine), C / bound 0.33 .. 0.36;
     the forward 5.9e-7 and 8.3e-7 of max |y|;
  F  held bit for bit in every comparison: no parameter had to move to the 2^-20 rule.
No check found a kernel wrong.
"""
import ctypes as C
import os

import pytest
import torch

from conftest import rel_err
from nca_testlib import (ONEHOT_R, dev, entry_err, general_case, general_layout, general_plan, general_ray_runs, make_dynamic, make_static,  # noqa: F401
                         onehot_channel_rows, onehot_checks_ab, onehot_coeffs, onehot_factor_errs, onehot_latent_rows, wide_layers, wide_preacts)
from oracle import nerfca_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
EXACT = 2.0 ** -20
CAP_POINTS = 3 << 20
BIG = 40 << 30
RECORD = {}
_MODELS = {}


def note(row, check, value):
    rec = RECORD.setdefault(row, {})
    rec[check] = max(rec.get(check, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def record():
    """Prints the worst value of every check per case and plan when the module is done; NERFCA_ONEHOT_GENERAL_RECORD=<file> keeps them."""
    yield
    lines = [f"{row:<58s} " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(rec.items())) for row, rec in RECORD.items()]
    print("\n" + "\n".join(lines))
    path = os.environ.get("NERFCA_ONEHOT_GENERAL_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture
def poison(monkeypatch):
    """Every scratch buffer handed to the library is filled with NaNs first: an unwritten slab or a stale padded row shows as a NaN."""
    from nerfca_amd import fused
    monkeypatch.setattr(fused, "POISON_BUFFERS", True)


def models(c, dev):
    """{net: the drop-in model} of a case, in f32 mode."""
    from nerfca_amd import set_precision
    if id(c) not in _MODELS:
        if c.nets == "s":
            m = {"s": make_static(c.ps, dev, F=c.F, early=c.early, late=c.late, pos_enc=c.ss.pos_enc, L=c.ss.pos_enc_basis, cin=c.cin, cout=c.cout)}
        else:
            m = {"s": make_static(c.ps, dev, F=c.F, early=c.early, late=c.late), "t": make_dynamic(c.pd, dev, F=getattr(c, "Fd", c.F), early=c.early_d, late=0, T=8)}
            for v in m.values():
                v.update_freq_mask_alpha(75000, 150000)
        set_precision("f32", *m.values())
        _MODELS[id(c)] = m
    return _MODELS[id(c)]


def of_net(g, net):
    return {k[2:]: v for k, v in g.items() if k[0] == net}


def grads(ms):
    return {net + "." + k: p.grad.detach().cpu() for net, m in ms.items() for k, p in m.named_parameters()}


def check_abc(c, g, i, tag, row, targets=None):
    """Checks A, B and C (the f32 rule) on the gradients of launch i: as check_abc of tests/test_onehot_grads_gpu.py."""
    floor, want = c.floor(i, "f32"), c.oracle(i, "f32")
    where_of = dict(zip("st", c.launches[i])) if c.nets == "st" else {"s": c.launches[i][0]}
    for net in c.nets:
        where = where_of[net]
        if targets is not None and net not in targets:
            for k, v in of_net(g, net).items():
                assert not bool(v.any()), (tag, net + "." + k, "B: a net without a coefficient")
            continue
        spec, sub = c.spec(net), of_net(g, net)
        x = c.feats(net, *where) if isinstance(where, tuple) else c.feats(net, where)
        note(row, "A", onehot_checks_ab(spec, c.params(net), sub, x, (tag, net, where)))
        if net == "t":
            onehot_latent_rows(sub["time_latents"], int((c.ph[where[0]] if isinstance(where, tuple) else c.ts[where])), (tag, where))
        for k, e, at in onehot_factor_errs(spec, sub, of_net(want, net)):
            fl = floor[net + "." + k]
            print(f"C {tag} {net}.{k} at {where}: {e:.3e} (floor {fl:.2e}) worst entry {at}")
            note(row, "C", e)
            note(row, "C/bound", e / max(TOL, 3 * fl))
            note(row, "floor", fl)
            assert e < max(TOL, 3 * fl), (tag, net + "." + k, "C: row, column", at, where, e, fl)


def same_bits(a, b, tag):
    """Check F: two runs of one launch gave every gradient the same bits."""
    for k in a:
        assert torch.equal(a[k], b[k]), (tag, k, "F: the chunking moved it", entry_err(a[k], b[k])[:2])


# ------------------------------------------------------------------------------------------ points
def run_points(c, dev, i, cap=None):
    """The gradients (on the CPU) of one-hot launch i of a point case, the workspace capped at `cap` bytes."""
    from nerfca_amd import _capi, fused
    ms = models(c, dev)
    assert all(_capi.net_is_general(m._binding.net) for m in ms.values())
    for m in ms.values():
        m.zero_grad()
    x = c.x.to(dev)
    saved = fused.BWD_WORKSPACE_BYTES
    try:
        if cap:
            fused.BWD_WORKSPACE_BYTES = cap
        if c.nets == "s":
            n, o = c.launches[i]
            ms["s"](x)[n, o].backward()
        else:
            ns, nd = c.launches[i]
            gs, gd = torch.zeros(c.N, 1), torch.zeros(c.N, 1)
            gs[ns], gd[nd] = 1.0, 1.0
            ((ms["s"](x) * gs.to(dev)).sum() + (ms["t"].forward_composite(x, c.ts.to(dev)) * gd.to(dev)).sum()).backward()
    finally:
        fused.BWD_WORKSPACE_BYTES = saved
    return grads(ms)


def chunk_of(c, dev, net, cap, bwd=True):
    """Rows per chunk of a point launch under `cap`, from the restated plan -- whose bytes must be the library's own query's."""
    from nerfca_amd import _capi
    b = models(c, dev)[net]._binding
    dyn = net == "t"
    y = general_layout(c.F, len(wide_layers(c.spec(net))), 75, T=8 if dyn else 0, P=10 if dyn else 0, skip=(c.early + 1) if (c.late and not dyn) else None)
    chunk, nsplit, nbytes = general_plan(y, c.N, bwd, cap)
    query = _capi.lib().nca_mlp_bwd_workspace if bwd else _capi.lib().nca_mlp_fwd_workspace
    assert query(C.byref(b.net), b.prec, c.N, cap) == nbytes, (net, cap, nbytes)
    return chunk


@pytest.mark.parametrize("name", ["P1024", "P1100", "PSKIP"])
def test_onehot_points_at_tile_and_split_seams(dev, name):
    """A, B, C on every launch under the default workspace (one chunk: the launch shapes the case is listed for); F: P1024 and P1100 once more under a
    3 MB workspace -- chunks of 512 rows (4 row tiles and splits) and of 640 (5) -- must give the same bits."""
    c = general_case(name)
    row = f"points {name} {c.name} N={c.N} f32 general"
    assert chunk_of(c, dev, "s", BIG) == chunk_of(c, dev, "t", BIG) == (c.N + 127) // 128 * 128
    capped = name != "PSKIP"
    if capped:
        assert chunk_of(c, dev, "s", CAP_POINTS) == chunk_of(c, dev, "t", CAP_POINTS) == {"P1024": 512, "P1100": 640}[name]          # the cap binds
    for i in range(len(c.launches)):
        g = run_points(c, dev, i)
        check_abc(c, g, i, (row, "launch", i), row)
        if capped:
            g3 = run_points(c, dev, i, cap=CAP_POINTS)
            check_abc(c, g3, i, (row, "3 MB", "launch", i), row + " 3MB")
            same_bits(g, g3, (row, "default vs 3 MB", "launch", i))


def test_onehot_points_split_seam_and_empty_splits(dev, poison):
    """P16500, poisoned buffers: 128 splits of 144 rows over 16 512, the last 13 empty; one-hots on both sides of the first split seam (143 | 144, inside
    row tile 1), in the middle, on both sides of the seam before the last split that holds rows (16415 | 16416) and at the last valid row."""
    c = general_case("P16500")
    row = f"points P16500 {c.name} N={c.N} f32 general poisoned"
    assert chunk_of(c, dev, "s", BIG) == chunk_of(c, dev, "t", BIG) == 16512
    for i in range(len(c.launches)):
        check_abc(c, run_points(c, dev, i), i, (row, "launch", i), row)


def test_onehot_points_other_channel_counts(dev):
    """PCH: a one-hot at point n* and output channel o*.  A, B, C as everywhere (rank_one_err over the 3 x F output layer already demands that the rows
    o != o* are zero bit for bit: their scale is zero); stated on their own: every row o != o* of dWo and entry of dbo is zero bit for bit, dbo[o*] is
    exactly 1, and dWo[o*] is the last hidden layer's output h(n*) of the f64 oracle per entry to 2^-20."""
    c = general_case("PCH")
    row = f"points PCH {c.name} {c.cin}->{c.cout} F={c.F} N={c.N} f32 general"
    for i, (n, o) in enumerate(c.launches):
        g = run_points(c, dev, i)
        check_abc(c, g, i, (row, "launch", i), row)
        dWo, dbo = g["s.output_linear.0.weight"], g["s.output_linear.0.bias"]
        onehot_channel_rows(dWo, dbo, o, (row, "launch", i))
        h = torch.relu(wide_preacts(c.ps, c.ss, c.feats("s", n)[None, :], torch.float64, emulate_bf16=False)[-1])[0]
        e, at = entry_err(dWo[o], h)
        print(f"A {row} launch {i}: dWo[o*] against h(n*) {e:.3e} at {at}")
        note(row, "A dWo vs h", e)
        assert e <= EXACT, (row, i, "A: dWo[o*] against h(n*)", at, e)


@pytest.mark.parametrize("name", ["P1100", "PSKIP"])
def test_general_forward_does_not_depend_on_the_chunking(dev, name):
    """The raw outputs under the default workspace, under 3 MB and under 1 MiB (the smallest the wrapper allows) are the same bits, and every entry is
    within max(1e-5, 3 floor) max |y64| of the f64 oracle (floor: the f32 oracle's distance from the f64 one).  P1100's forward is cut by the 1 MiB
    cap alone (640-row chunks: the second starts in the middle of row tile 5 of the uncut launch); PSKIP's 384 rows fit every cap."""
    from nerfca_amd import fused
    c = general_case(name)
    ms = models(c, dev)
    row = f"forward {name} {c.name} N={c.N} f32 general"
    if name == "P1100":
        assert chunk_of(c, dev, "s", 1 << 20, bwd=False) == chunk_of(c, dev, "t", 1 << 20, bwd=False) == 640
    x, ts = c.x.to(dev), c.ts.to(dev)
    outs = []
    saved = fused.BWD_WORKSPACE_BYTES
    try:
        for cap in (None, CAP_POINTS, 1 << 20):
            if cap:
                fused.BWD_WORKSPACE_BYTES = cap
            with torch.no_grad():
                outs.append((ms["s"](x).cpu(), ms["t"].forward_composite(x, ts).cpu()))
    finally:
        fused.BWD_WORKSPACE_BYTES = saved
    for other in outs[1:]:
        assert torch.equal(other[0], outs[0][0]) and torch.equal(other[1], outs[0][1]), (row, "the chunking moved the forward")
    for k, net in enumerate("st"):
        y = {}
        for dt in (torch.float32, torch.float64):
            p = {n: v.to(dt) for n, v in c.params(net).items()}
            y[dt] = O.static_forward(p, c.ss, c.x.to(dt), c.win.to(dt)) if net == "s" else O.dynamic_forward(p, c.sd, c.x.to(dt), c.ts, c.win.to(dt))
        floor = rel_err(y[torch.float32], y[torch.float64])
        e = rel_err(outs[0][k], y[torch.float64])          # (max over the entries of |y - y64| / max |y64|: every entry is within the bound)
        print(f"{row} {net}: {e:.3e} (floor {floor:.2e})")
        note(row, "C", e)
        note(row, "floor", floor)
        note(row, "C/bound", e / max(TOL, 3 * floor))
        assert bool(torch.isfinite(outs[0][k]).all()) and e < max(TOL, 3 * floor), (row, net, e, floor)


# ------------------------------------------------------------------------------------------ rays
def run_rays(c, dev, coeffs, limit=None, cap=None):
    """(gradients on the CPU, the forward's store kind) of the scalar with these coefficients; limit: fused.STORE_FORWARD_LIMIT_BYTES, cap: the workspace bound."""
    from nerfca_amd import _capi, fused, render_rays
    ms = models(c, dev)
    for m in ms.values():
        m.zero_grad()
    cp, cs, cd = coeffs
    saved = fused.STORE_FORWARD_LIMIT_BYTES, fused.BWD_WORKSPACE_BYTES
    try:
        if limit is not None:
            fused.STORE_FORWARD_LIMIT_BYTES = limit
        if cap:
            fused.BWD_WORKSPACE_BYTES = cap
        pix, a, b = render_rays(ms["s"], ms["t"], c.o.to(dev), c.d.to(dev), c.ph.to(dev), c.I0.to(dev), c.z.to(dev), c.dists.to(dev))
        kind = _capi.last_plan()["fwd_store_format"] & _capi.STORE_KIND_MASK
        ((pix * cp.to(dev)).sum() + (a * cs.to(dev)).sum() * 50 + (b * cd.to(dev)).sum() * 50).backward()
    finally:
        fused.STORE_FORWARD_LIMIT_BYTES, fused.BWD_WORKSPACE_BYTES = saved
    return grads(ms), kind


def rays_per_run(c, dev, cap):
    """(rays per run, the workspace the library asks for) of the recomputing backward of a ray case under `cap`: plan_ray_chunks restated on the restated
    regions, whose sum must be what the library's own query nca_render_bwd_workspace returns."""
    from nerfca_amd import _capi, fused
    ms = models(c, dev)
    batch = fused._RayBatch(c.o.to(dev), c.d.to(dev), c.ph.to(dev), c.I0.to(dev), c.z.to(dev), c.dists.to(dev), "softplus", False, 1e-2)
    desc = batch.desc()
    bs, bd = ms["s"]._binding, ms["t"]._binding
    need = _capi.check(_capi.lib().nca_render_bwd_workspace(C.byref(desc), C.byref(bs.net), C.byref(bd.net), bs.prec, cap))
    lays = [general_layout(c.F, 2, 75), general_layout(c.Fd, 2, 75, T=8, P=10)]
    extra = 4 * ((ONEHOT_R * c.S * 4 + 255) // 256 * 256)

    def need_of(rays):
        return sum(general_plan(y, (rays * c.S + 127) // 128 * 128)[2] for y in lays)

    rays = general_ray_runs(ONEHOT_R, c.S, need_of, cap - extra)
    assert need == need_of(rays) + extra, (cap, rays, need, need_of(rays), extra)
    return rays, need


def test_render_bwd_general_from_store_recomputed_and_in_runs(dev, poison):
    """RG, poisoned buffers.  Plans: (i) from the general store; (ii) recomputed in one run of 9 rays (640 rows, 10 of them padding); (iii) recomputed under
    workspace caps taken from the library's own query -- 3.5 MB: runs of 5 rays (rays 0 .. 4 | 5 .. 8, rows 384 | 384), 2.5 MB: runs of 3 rays (0 .. 2 |
    3 .. 5 | 6 .. 8, 256 rows each, 46 of them padding): the rays 0, 4 and 8 of the launches then lie in three different runs.  A, B, C in every plan; F:
    all four give the same bits."""
    from nerfca_amd import _capi
    c = general_case("RG")
    ms = models(c, dev)
    assert all(_capi.net_is_general(m._binding.net) for m in ms.values())
    whole, U = rays_per_run(c, dev, BIG)
    assert whole == ONEHOT_R
    caps = {}
    for cap, rays in ((3500000, 5), (2500000, 3)):
        got, need = rays_per_run(c, dev, cap)
        assert got == rays and (1 << 20) < need <= cap and need < U, (cap, got, need, U)          # the cap binds, above the wrapper's 1 MiB floor
        caps[f"recompute {rays} rays per run"] = cap
    assert len({r // 3 for r in (0, 4, 8)}) == 3
    plans = {"store": (None, None, _capi.STORE_GENERAL), "recompute": (0, None, _capi.STORE_NONE)}
    plans.update({k: (0, cap, _capi.STORE_NONE) for k, cap in caps.items()})
    for i in range(len(c.launches)):
        first = None
        for plan, (limit, cap, kind) in plans.items():
            g, got = run_rays(c, dev, c.coeffs(i), limit, cap)
            assert got == kind, (plan, got)
            row = f"rays RG {c.name} S={c.S} f32 general {plan}"
            check_abc(c, g, i, (row, "launch", i), row)
            if first is None:
                first = g
            else:
                same_bits(first, g, (row, "against the store plan", "launch", i))


@pytest.mark.parametrize("name", ["RMIX_64_144", "RMIX_144_64"])
def test_render_bwd_general_beside_a_fused_kernel_net(dev, name):
    """RMIX: no store (STORE_NONE); the net on the general kernels and the fused-kernel net beside it both pass A, B, C under the f32 rule at every
    position; once each net alone: the other's gradient is zero bit for bit and its own the same bits as in the shared launch."""
    from nerfca_amd import _capi
    c = general_case(name)
    ms = models(c, dev)
    assert [_capi.net_is_general(ms[n]._binding.net) for n in "st"] == [c.F > 128, c.Fd > 128] and (c.F > 128) != (c.Fd > 128)
    row = f"rays {name} S={c.S} f32 mixed"
    for i in range(len(c.launches)):
        g, kind = run_rays(c, dev, c.coeffs(i))
        assert kind == _capi.STORE_NONE
        check_abc(c, g, i, (row, "launch", i), row)
        if i == 0:
            for net, (r, s) in zip("st", c.launches[i]):
                alone, kind = run_rays(c, dev, onehot_coeffs(ONEHOT_R, c.S, net, r, s))
                assert kind == _capi.STORE_NONE
                check_abc(c, alone, i, (row, "alone", net), row, targets=net)
                for k, v in of_net(alone, net).items():
                    assert torch.equal(v, g[net + "." + k]), (row, net + "." + k, "the other net's one-hot moved it")
