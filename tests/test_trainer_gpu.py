"""GPU tests of CompositeTrainer's step functions against the reference's own trajectories and of its device-side ray
sampler.  The hierarchical loop (run_composite.py:283-312) is checked through BOTH step functions -- the autograd step
(`fused_loss=False`: the drop-in loss functions -- the HIP loss kernel behind `compute_losses` / `weighted_MSELoss` -- on the HIP render) and the graph-free fused step (`step_fused`: HIP loss kernel,
HIP sampler and its HIP backward, manual chain rule through ray 0's interval lengths) -- on tests/golden/full_step_fine.npz.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import rel_err
from nca_testlib import dev, make_dynamic, make_static  # noqa: F401

pytestmark = pytest.mark.gpu


def _golden_data(g, dev):
    """The golden batch as a ray table (train/data_helpers.py:141-165 layout: origin, direction, pixel x3, weight x3)."""
    o, d, gt, w = g["o"], g["d"], g["gt"], g["wpix"]
    table = torch.stack([o, d, gt[:, None].repeat(1, 3), w[:, None].repeat(1, 3)], 1).double()
    geo = dict(near_thresh=3.4259, far_thresh=5.5741, max_pixel_value=float(g["I0"][0]))
    return SimpleNamespace(geo=geo, rays_train=table.to(dev), phases_train=g["ph"].to(dev), var_ray_ids=np.zeros(0, dtype=np.int64),
                           non_var_ray_ids=np.arange(o.shape[0]))


@pytest.mark.parametrize("fused_loss", [True, False])
def test_fine_training_steps_vs_reference(golden, dev, fused_loss):
    """Three steps of the hierarchical loop on the reference's own inputs, weights and random draws: per-step loss and pixel
    losses (1e-5), step-0 gradients of all four nets (fine nets 3e-4: the sampled depths carry the f32 rounding of an inverse
    CDF that divides by increments as small as 1e-5; coarse nets 1e-3: they include the through-depth term, ~1e4 times their
    regular gradient and ill-conditioned through the sampler, see test_trainer_with_fine_pass_vs_oracle), parameters after
    three Adam + LinearLR steps."""
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    g = golden("full_step_fine")
    R, S, NF = g["o"].shape[0], g["z"].shape[0], int(g["n_fine"])
    s = make_static(g.prefixed("init_sp_"), dev, F=64, early=4, late=0)
    t = make_dynamic(g.prefixed("init_dp_"), dev, F=64, early=4, late=0, T=8)
    sf = make_static(g.prefixed("init_sfp_"), dev, F=32, early=4, late=0)
    tf = make_dynamic(g.prefixed("init_dfp_"), dev, F=32, early=4, late=0, T=8)
    cfg = TrainConfig(depth_samples_per_ray_coarse=S, depth_samples_per_ray_fine=NF, img_sample_size=R)
    tr = CompositeTrainer(cfg, s, t, _golden_data(g, dev), dev, seed=0, fused_loss=fused_loss, static_model_fine=sf, temp_model_fine=tf)
    assert torch.equal(tr.depth.cpu(), g["z"])
    base = int(g["base_iter"])
    # the reference's batch and draws instead of the trainer's own
    tr.draw_ray_ids_device = lambda n_iter: torch.arange(R, device=dev)
    tr.draw_jitter = lambda n_iter: g[f"step{n_iter - base}_t_rand"]
    tr.draw_fine_u = lambda n_iter: g[f"step{n_iter - base}_u"]
    for k in range(3):
        loss, pixel, terms = tr.step(base + k)
        assert rel_err(loss.detach().cpu(), g[f"step{k}_loss"]) < 1e-5, k
        assert rel_err(pixel.detach().cpu(), g[f"step{k}_pixel"]) < 1e-5, k
        if fused_loss:
            assert rel_err(tr.last_fine_terms[1].cpu(), g[f"step{k}_pixel_f"]) < 1e-5, k
        if k == 0:
            for m, pre, tol in ((s, "step0_sg_", 1e-3), (t, "step0_dg_", 1e-3), (sf, "step0_sfg_", 3e-4), (tf, "step0_dfg_", 3e-4)):
                got = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
                for n, ref in g.prefixed(pre).items():
                    assert rel_err(got[n], ref) < tol, (pre, n, rel_err(got[n], ref))
    for m, pre in ((s, "final_sp_"), (t, "final_dp_"), (sf, "final_sfp_"), (tf, "final_dfp_")):
        for n, ref in g.prefixed(pre).items():
            assert rel_err(m.state_dict()[n].cpu(), ref) < 2e-3, (pre, n)


def test_fused_fine_step_equals_autograd_fine_step(dev):
    """The two step functions on the trainer's own batches (synthetic data, F = 64 / 32, 3 steps), with and without the
    through-depth gradient: same losses, same parameters after the optimiser steps."""
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    data = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    for dg in (True, False):
        outs = []
        for fused in (False, True):
            torch.manual_seed(9)
            sdef, tdef = synthetic.net_definitions(dev, F=64)
            fsd, ftd = synthetic.net_definitions(dev, F=32)
            nets = [CPPN(sdef).to(dev), Temporal(tdef).to(dev), CPPN(fsd).to(dev), Temporal(ftd).to(dev)]
            cfg = TrainConfig(depth_samples_per_ray_coarse=48, depth_samples_per_ray_fine=16, img_sample_size=256, favor_s_weight_delay_steps=0,
                              l1_weight_start=1e-3, l1_weight_end=1e-3, occl_weight_start=1e-2, dynamic_entro_weight_start=1e-3,
                              favor_s_weight_start=1e-3, entro_mask_thre=1e-6, fine_depth_gradients=dg)
            tr = CompositeTrainer(cfg, nets[0], nets[1], data, dev, seed=5, fused_loss=fused, static_model_fine=nets[2], temp_model_fine=nets[3])
            losses, g0 = [], None
            for it in range(3):
                losses.append(float(tr.step(1000 + it)[0]))
                if it == 0:
                    g0 = torch.cat([p.grad.detach().flatten() for p in tr.params]).double().cpu()
            outs.append((losses, torch.cat([p.detach().flatten() for p in tr.params]).cpu(), g0))
        # Step 0 runs on identical weights: losses to 2e-5 and the two implementations' GRADIENTS to 1e-4 of each other in L2 (measured: 2.3e-6
        # with the through-depth term, 1.9e-9 without).  What follows is the conditioning of the problem, not of the implementations: with the
        # through-depth term (~1e4 times the regular gradient, ill-conditioned through the sampler) three Adam steps turn that 2e-6 into a
        # 2e-3 difference of the parameters (Adam makes a sign flip of a near-zero entry a full learning-rate step; the max-norm of three steps
        # is bounded by 3 lr / max|p| whatever happens), so the later losses and the parameters are only held to 5e-3 there
        g_l2 = float((outs[1][2] - outs[0][2]).norm() / outs[0][2].norm())
        p_l2 = float((outs[1][1] - outs[0][1]).norm() / outs[0][1].norm())
        print(f"[fine step, through-depth gradient {dg}] step-0 gradient L2 difference {g_l2:.3e}, parameters after 3 steps L2 {p_l2:.3e}, max-norm {rel_err(outs[1][1], outs[0][1]):.3e}; "
              f"losses {outs[0][0]} / {outs[1][0]}", flush=True)
        for k, (a, b) in enumerate(zip(outs[0][0], outs[1][0])):
            assert abs(a - b) <= (2e-5 if (k == 0 or not dg) else 5e-3) * abs(a), (dg, outs[0][0], outs[1][0])
        if dg:
            assert g_l2 < 1e-4 and p_l2 < 5e-3, (g_l2, p_l2)
        else:
            assert g_l2 < 1e-7 and rel_err(outs[1][1], outs[0][1]) < 1e-5, (g_l2, rel_err(outs[1][1], outs[0][1]))


def test_device_ray_sampler_counts_and_determinism(dev):
    """draw_ray_ids_device (run_composite.py:250-260 drawn on the GPU): img_sample_size ids, exactly
    int(var_sample_perc / 100 * img_sample_size) of them from the high-variance table and the rest from its complement (both
    with replacement), shuffled; the same seed and iteration give the same ids (every rank draws the same global batch),
    another iteration different ones; var_sample_perc == 0 draws uniformly over all rays."""
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    n_rays = 5000
    rng = np.random.default_rng(0)
    var = np.sort(rng.choice(n_rays, 700, replace=False))
    non = np.setdiff1d(np.arange(n_rays), var)
    data = SimpleNamespace(geo=dict(near_thresh=3.4, far_thresh=5.6, max_pixel_value=2.0), rays_train=torch.zeros(n_rays, 4, 3, dtype=torch.float64, device=dev),
                           phases_train=torch.zeros(n_rays, dtype=torch.int64, device=dev), var_ray_ids=var, non_var_ray_ids=non)
    dummy = SimpleNamespace(parameters=lambda: iter([torch.nn.Parameter(torch.zeros(1, device=dev))]))
    for perc in (50, 12.5, 0):
        cfg = TrainConfig(depth_samples_per_ray_coarse=8, img_sample_size=1024, var_sample_perc=perc)
        tr = CompositeTrainer(cfg, dummy, dummy, data, dev, seed=3, fused_loss=False)
        ids = tr.draw_ray_ids_device(17)
        assert ids.shape == (1024,) and ids.dtype == torch.int64
        assert int(ids.min()) >= 0 and int(ids.max()) < n_rays
        n_var = int(np.isin(ids.cpu().numpy(), var).sum())
        if perc > 0:
            assert n_var == int(perc / 100.0 * 1024), (perc, n_var)
            # shuffled: the variance rays are not all at the tail
            assert bool(np.isin(ids[:512].cpu().numpy(), var).any())
        else:
            assert 60 < n_var < 240                  # ~14 % of a uniform draw
        assert torch.equal(ids, tr.draw_ray_ids_device(17))
        assert not torch.equal(ids, tr.draw_ray_ids_device(18))
        tr2 = CompositeTrainer(cfg, dummy, dummy, data, dev, rank=1, world=2, seed=3, fused_loss=False)
        assert torch.equal(ids, tr2.draw_ray_ids_device(17))


def test_early_stop_flag(dev):
    """run_composite.py:310-312: the loop ends when the dynamic entropy or the favor loss falls below 1e-15 once the frequency
    windows are fully open; the flag is computed on the device and read on demand."""
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    data = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    torch.manual_seed(2)
    sdef, tdef = synthetic.net_definitions(dev, F=32)
    s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
    cfg = TrainConfig(depth_samples_per_ray_coarse=48, img_sample_size=128, static_pos_enc_window_decay_steps=10, temp_pos_enc_window_decay_steps=10)
    tr = CompositeTrainer(cfg, s, t, data, dev, seed=1)
    tr.step(5)
    assert tr.stop_flag is None and tr.early_stop() is False          # windows still opening: the predicate is not evaluated
    tr.step(10)
    assert tr.stop_flag is not None and tr.early_stop() is False      # a live dynamic field: both terms are far above 1e-15
    with torch.no_grad():                                             # a dead dynamic field: sigma_d == 0 exactly -> blend weight 0, entropy 0
        t.output_linear[0].weight.zero_()
        t.output_linear[0].bias.fill_(-1e4)
    tr.step(11)
    assert tr.early_stop() is True


def test_query_time_with_latent_vectors(golden, dev):
    """Temporal.query_time(x, latent_vectors) (model/Temporal.py:113-136) with vectors that are NOT rows of time_latents --
    23 distinct interpolated latents, i.e. three temporary tables -- against the oracle's MLP on cat[posenc(x), latents],
    outputs and weight gradients at 1e-5; with the module's own rows it equals forward_composite."""
    from oracle import nerfca_oracle as O
    g = golden("mlps")
    tag = "F64_e4_l0"
    pd = g.prefixed(f"d_{tag}_p_")
    t = make_dynamic(pd, dev, F=64, early=4, late=0, T=8)
    t.update_freq_mask_alpha(60000, 150000)
    x = g["x"]
    n = x.shape[0]
    gen = torch.Generator().manual_seed(5)
    pool = torch.rand(23, 8, generator=gen)
    pick = torch.randint(0, 23, (n,), generator=gen)
    lat = pool[pick]
    sd = O.NetSpec(num_filters=64, num_time_dim=8)
    win = O.freq_mask_alpha(12, 60000, 150000, 1)[0]
    po = {k: v.clone().requires_grad_(True) for k, v in pd.items()}
    yo = O.mlp(po, sd, torch.cat([O.encode(x, sd, win), lat], -1))
    (yo * g["gout"]).sum().backward()
    y = t.query_time(x.to(dev), lat.to(dev))
    assert tuple(y.shape) == (n, 1) and rel_err(y.cpu(), yo) < 1e-5
    (y * g["gout"].to(dev)).sum().backward()
    for k, p in t.named_parameters():
        if k == "time_latents":
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        else:
            assert rel_err(p.grad.cpu(), po[k].grad) < 1e-5, k
    ts = g["ts"]
    with torch.no_grad():
        assert torch.equal(t.query_time(x.to(dev), t.time_latents[ts.long().to(dev)]), t.forward_composite(x.to(dev), ts.to(dev)))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_query_time_latent_vector_gradients(golden, dev, prec):
    """Gradients with respect to the latent vectors passed to query_time (plain autograd in the reference, Temporal.py:113-136) are
    PER POINT (nca_mlp_bwd's g_latents): a pool of 23 vectors indexed per point, as forward_composite builds its own (:147-149); a
    LEAF with repeated rows (every row its own gradient -- refused until round 3); equal rows that come from two different tensors
    (each source gets its own points' gradient, not the sum -- ADVICE r3); all rows distinct.  Against autograd through the oracle."""
    from oracle import nerfca_oracle as O
    from nerfca_amd import set_precision
    g = golden("mlps")
    pd = g.prefixed("d_F64_e4_l0_p_")
    t = make_dynamic(pd, dev, F=64, early=4, late=0, T=8)
    set_precision(prec, t)
    tol = 1e-5 if prec == "f32" else 3e-2
    t.update_freq_mask_alpha(60000, 150000)
    x = g["x"]
    n = x.shape[0]
    gen = torch.Generator().manual_seed(6)
    pool = torch.rand(23, 8, generator=gen)
    pick = torch.randint(0, 23, (n,), generator=gen)
    sd = O.NetSpec(num_filters=64, num_time_dim=8, emulate_bf16=(prec == "bf16"))
    win = O.freq_mask_alpha(12, 60000, 150000, 1)[0]

    def oracle(lat_rows):
        yo = O.mlp({k: v.clone() for k, v in pd.items()}, sd, torch.cat([O.encode(x[: lat_rows.shape[0]], sd, win), lat_rows], -1))
        (yo * g["gout"][: lat_rows.shape[0]]).sum().backward()
        return yo.detach()

    def hip(lat_rows):
        y = t.query_time(x[: lat_rows.shape[0]].to(dev), lat_rows)
        (y * g["gout"][: lat_rows.shape[0]].to(dev)).sum().backward()
        return y.detach().cpu()

    # (1) an indexed pool
    pool_o = pool.clone().requires_grad_(True)
    yo = oracle(pool_o[pick])
    pool_d = pool.to(dev).requires_grad_(True)
    y = hip(pool_d[pick.to(dev)])
    assert rel_err(y, yo) < (1e-5 if prec == "f32" else 2e-3)
    assert rel_err(pool_d.grad.cpu(), pool_o.grad) < tol
    # (2) a leaf with repeated rows: one gradient row per point
    leaf_o = pool[pick].clone().requires_grad_(True)
    oracle(leaf_o)
    leaf_d = pool[pick].to(dev).requires_grad_(True)
    hip(leaf_d)
    assert rel_err(leaf_d.grad.cpu(), leaf_o.grad) < tol
    # (3) equal rows from two autograd sources: cat([a, a.clone()]) -- each source keeps the gradient of ITS points
    half = n // 2
    a_o, b_o = pool[pick[:half]].clone().requires_grad_(True), pool[pick[:half]].clone().requires_grad_(True)
    oracle(torch.cat([a_o, b_o]))
    a_d, b_d = pool[pick[:half]].to(dev).requires_grad_(True), pool[pick[:half]].to(dev).requires_grad_(True)
    hip(torch.cat([a_d, b_d]))
    assert rel_err(a_d.grad.cpu(), a_o.grad) < tol and rel_err(b_d.grad.cpu(), b_o.grad) < tol
    assert not torch.equal(a_d.grad, b_d.grad)
    # (4) all rows distinct
    m = min(n, 16)
    lat_o = torch.rand(m, 8, generator=gen).requires_grad_(True)
    oracle(lat_o)
    lat_d = lat_o.detach().to(dev).requires_grad_(True)
    hip(lat_d)
    assert rel_err(lat_d.grad.cpu(), lat_o.grad) < tol


def test_magix_shape_full_size_step(dev):
    """BASELINE configs[3]'s shape (MAGIX cone beam DSD 2000 / DSO 600, 512^2 detector, 256 samples per ray, f32): one fused
    step over a full detector runs as ray micro-batches (its forward store would not fit) and is reproducible bit for bit;
    the ray geometry is the preset's (source at DSO, near / far around it)."""
    import nerfca_amd
    from nerfca_amd import fused, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    data = synthetic.make_dataset(512, 256, dev, views=synthetic.TRAIN_VIEWS[:1], n_phases=2, geometry="magix")
    assert abs(float(data.rays_train[0, 0].norm()) - 6.0) < 1e-6 and abs(data.geo["near_thresh"] - 4.7272) < 1e-3
    outs, calls = [], []
    orig = fused.render_forward_raw
    fused.render_forward_raw = lambda *a, **k: (calls.append(a[0].R), orig(*a, **k))[1]
    try:
        for _ in range(2):
            torch.manual_seed(1)
            sdef, tdef = synthetic.net_definitions(dev)
            s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
            tr = CompositeTrainer(TrainConfig(depth_samples_per_ray_coarse=256, img_sample_size=262144), s, t, data, dev, seed=0)
            _, _, terms = tr.step_fused(75000)
            outs.append((terms.clone(), torch.cat([p.grad.flatten() for p in tr.params]).clone()))
            del tr, s, t
            torch.cuda.empty_cache()
    finally:
        fused.render_forward_raw = orig
    assert len(calls) >= 4 and sum(calls) == 2 * 262144              # several micro-batches per step
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][1].abs().max()) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])

    # A 1/256 subsample of that step's rays (MAGIX geometry, 256 samples per ray, f32) against the ORACLE: the loss, the pixel term,
    # every loss term and the first-layer gradients of both nets.  The oracle runs twice: in f32 (the reference's arithmetic) and in
    # f64 (what it approximates); gradients are gated at max(1e-5, 3 x the f32 oracle's own distance from f64), as everywhere
    # (ReLU masks near zero flip under any f32 rounding, tests/test_hip_parity.py).
    from nerfca_amd import _capi
    from oracle import nerfca_oracle as O
    torch.manual_seed(1)
    sdef, tdef = synthetic.net_definitions(dev)
    s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
    R_sub, n_iter = 1024, 75000
    full = CompositeTrainer(TrainConfig(depth_samples_per_ray_coarse=256, img_sample_size=262144), s, t, data, dev, seed=0)
    ids = full.draw_ray_ids_device(n_iter)[::256].contiguous()
    assert ids.shape[0] == R_sub
    tr = CompositeTrainer(TrainConfig(depth_samples_per_ray_coarse=256, img_sample_size=R_sub), s, t, data, dev, seed=0)
    tr.draw_ray_ids_device = lambda it: ids
    terms, grads_s, grads_d = tr.fused_gradients(n_iter)
    got = dict(zip(_capi.TERM_NAMES, terms.cpu().tolist()))
    gs = dict(zip([n for n, _ in s.named_parameters()], s._binding.split_grads(grads_s)))
    gd = dict(zip([n for n, _ in t.named_parameters()], t._binding.split_grads(grads_d)))
    rays, ph = data.rays_train.cpu().index_select(0, ids.cpu()), data.phases_train.cpu().index_select(0, ids.cpu())
    o, d, gt, w = rays[:, 0, :], rays[:, 1, :], rays[:, 2, 0], rays[:, 3, 0]
    I0 = torch.full((R_sub,), float(data.geo["max_pixel_value"]))
    z = O.stratified_depths(O.depth_values(data.geo["near_thresh"], data.geo["far_thresh"], 256), tr.draw_jitter(n_iter).cpu())
    ss, sd = O.NetSpec(num_filters=128), O.NetSpec(num_filters=128, num_time_dim=8)

    def oracle(dt):
        ot = O.OracleTrainer({k: v.detach().cpu().to(dt) for k, v in s.state_dict().items()}, ss, {k: v.detach().cpu().to(dt) for k, v in t.state_dict().items()}, sd)
        loss, pixel, tt = ot.step(n_iter, o, d, ph[:, None].repeat(1, 256), I0, z.to(dt) if dt == torch.float64 else z, gt, w)
        return loss, pixel, tt, ot
    l64, p64, t64, o64 = oracle(torch.float64)
    _, _, _, o32 = oracle(torch.float32)
    ref = {"loss": l64, "pixel": p64, "blendw": t64[0], "favor_s": t64[3], "s_entropy": t64[4], "s_entropy_sum": t64[5], "d_entropy": t64[6],
           "d_entropy_sum": t64[7], "d_occl": t64[8], "s_l1": t64[9], "s_l2": t64[10]}
    for k, v in ref.items():
        v = float(v.detach())
        assert abs(got[k] - v) <= 2e-5 * abs(v) + 1e-12, (k, got[k], v)
    for name, mine, p64s, p32s in (("static", gs, o64.ps, o32.ps), ("dynamic", gd, o64.pd, o32.pd)):
        for key in ("early_pts_layers.0.weight", "early_pts_layers.0.bias"):
            g64, g32 = p64s[key].grad.double(), p32s[key].grad.double()
            # (262 144 samples: measured 1.06e-5 on the static net's first-layer weight -- one more ReLU mask within rounding of zero than
            # torch's f32 run flips on this batch; the floor is 2e-5 here, 1e-5 on the golden-sized batches of tests/test_hip_parity.py)
            tol = max(2e-5, 3 * rel_err(g32, g64))
            assert rel_err(mine[key].cpu().double(), g64) < tol, (name, key, rel_err(mine[key].cpu().double(), g64), tol)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_graph_step_with_fine_pass_matches_fused_step(dev, prec):
    """CompositeTrainer.step_graph with the hierarchical pass on (one rank): the captured graph holds coarse forward -> loss ->
    sampler -> fine forward -> loss -> fine backward with depth gradients -> sampler backward -> coarse backward -> the library's
    Adam over all four nets; ray ids, depth jitter, sample_pdf's uniform draws, the four band windows and the loss weights
    reach it through device memory.  Same loss every step and same parameters as step_fused with torch.optim.Adam."""
    from nerfca_amd import set_precision, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    data = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    outs = []
    for graph in (False, True):
        torch.manual_seed(9)
        sdef, tdef = synthetic.net_definitions(dev, F=64)
        nets = [CPPN(sdef).to(dev), Temporal(tdef).to(dev), CPPN(sdef).to(dev), Temporal(tdef).to(dev)]
        set_precision(prec, *nets)
        cfg = TrainConfig(depth_samples_per_ray_coarse=48, depth_samples_per_ray_fine=16, img_sample_size=256, favor_s_weight_delay_steps=0,
                          l1_weight_start=1e-3, l1_weight_end=1e-5, occl_weight_start=1e-2, occl_weight_end=1e-4,
                          dynamic_entro_weight_start=1e-3, favor_s_weight_start=1e-3, entro_mask_thre=1e-6,
                          hyperparam_decay_steps=40, lr=2e-3, lr_decay_steps=6, lr_end_factor=0.1,
                          static_pos_enc_window_decay_steps=40, temp_pos_enc_window_decay_steps=40)
        tr = CompositeTrainer(cfg, nets[0], nets[1], data, dev, seed=5, fused_loss=True, static_model_fine=nets[2], temp_model_fine=nets[3])
        losses = []
        for it in range(6):
            out = tr.step_graph(3 * it) if graph else tr.step_fused(3 * it)
            losses.append((float(out[0]), float(tr.last_fine_terms[0])))
        outs.append((losses, torch.cat([p.detach().flatten() for p in tr.params]).cpu()))
    # (step 0 agrees to rounding; after that the two optimisers' last-bit differences are amplified step by step through the
    # sampler's ill-conditioned depth gradient -- 2.5e-4 after three steps, 1e-3 after four in f32; a per-step input that did not
    # advance inside the replay -- ids, jitter, uniform draws, windows, weights -- would show as a difference of order one)
    for k, (a, b) in enumerate(zip(*[o[0] for o in outs])):
        tol = (2e-5 if prec == "f32" else 2e-3) if k == 0 else (5e-3 if prec == "f32" else 2e-2)
        assert abs(a[0] - b[0]) <= tol * abs(a[0]) and abs(a[1] - b[1]) <= tol * abs(a[1]), (k, outs[0][0], outs[1][0])
    assert rel_err(outs[1][1], outs[0][1]) < (5e-3 if prec == "f32" else 2e-2)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_trainer_with_odd_widths(dev, prec):
    """CompositeTrainer over nets of 48 units (kernel width 64): the autograd step with torch's fused Adam, the fused step and the
    graph-replayed step all train (parameters are strided views into the padded flat buffers), agree on the first step's loss and
    leave the padding at zero."""
    import nerfca_amd
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    data = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    losses = {}
    for mode in ("autograd", "fused", "graph"):
        torch.manual_seed(5)
        sdef, tdef = synthetic.net_definitions(dev, F=48)
        s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
        nerfca_amd.set_precision(prec, s, t)
        cfg = TrainConfig(depth_samples_per_ray_coarse=48, img_sample_size=160)
        tr = CompositeTrainer(cfg, s, t, data, dev, seed=3, fused_loss=(mode != "autograd"))
        step = tr.step_graph if mode == "graph" else tr.step
        first = None
        for it in range(3):
            loss, _, _ = step(1000 + it)
            first = float(loss.detach()) if first is None else first
        assert torch.isfinite(loss)
        losses[mode] = first
        for m in (s, t):
            bnd = m._binding
            assert bnd.net.F == 64 and m.num_filters == 48 and bnd._is_flat()
            mask = torch.ones_like(bnd.flat, dtype=torch.bool)
            for g in bnd.split_grads(mask):
                g.fill_(False)
            assert bool(mask.any()) and float(bnd.flat[mask].abs().max()) == 0.0
            assert tuple(m.state_dict()["early_pts_layers.2.weight"].shape) == (48, 48)
    tol = 1e-5 if prec == "f32" else 2e-2
    assert abs(losses["fused"] - losses["autograd"]) <= tol * abs(losses["autograd"]), losses
    assert abs(losses["graph"] - losses["fused"]) <= 1e-6 * abs(losses["fused"]), losses
