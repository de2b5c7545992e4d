"""Ray-sharded data parallelism on CPU with gloo, world_size 2.

The trainer's sharding / loss normalisation / all-reduce logic is backend-agnostic; here the
renderer is the CPU oracle (injected -- the product default is the HIP path, which has no CPU
implementation) and the process group is gloo.  Checked: the summed gradient and the parameters
after Adam of a 2-rank step equal the 1-rank step on the same global batch.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nca_testlib import free_port, oracle_fine_sampler  # noqa: E402


def oracle_render(s, t, o, d, ph, I0, z, dists, act="softplus", single=False, scale=1e-2):
    """render_rays signature, CPU oracle arithmetic, autograd into the drop-in modules' parameters."""
    from oracle import nerfca_oracle as O

    def spec_of(m, T):
        return O.NetSpec(num_filters=m.num_filters, num_early_layers=m.num_early_layers, num_late_layers=m.num_late_layers,
                         pos_enc=m.use_pos_enc, pos_enc_basis=m.pos_enc_basis, num_time_dim=T)

    def window(m):
        return m._band_window() if m.use_pos_enc in ("free_windowed", "nerfies_windowed") else None

    R, S = o.shape[0], z.shape[-1]
    pts = O.query_points(o, d, z)
    raw_s = O.static_forward(dict(s.named_parameters()), spec_of(s, 0), pts, window(s)).reshape(R, S, -1)
    phs = ph.reshape(R, -1)[:, :1].repeat(1, S).flatten()
    raw_d = O.dynamic_forward(dict(t.named_parameters()), spec_of(t, t.num_time_dim), pts, phs, window(t)).reshape(R, S, -1)
    if z.dim() == 1:
        pix, a, b, _ = O.composite(raw_s, raw_d, I0, d, z, act)
        return pix, a, b
    # fine pass: per-ray depths, interval lengths of (global) ray 0 as handed over (model_helpers.py:150)
    f = O.activation(act)
    a, b = f(raw_s[..., -1]) * scale, f(raw_d[..., -1]) * scale
    return I0 - ((a + b) * dists).sum(dim=-1), a, b


def build(seed=0):
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import TrainConfig
    from injected_trainer import InjectedTrainer as CompositeTrainer
    dev = torch.device("cpu")
    sdef, tdef = synthetic.net_definitions(dev, F=32, early=2, L=4, T=4)

    def render_pix(s, t, o, d, ph, I0, z, dists):
        return oracle_render(s, t, o, d, ph, I0, z, dists)[0]

    data = synthetic.make_dataset(8, 16, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32, render=render_pix)
    torch.manual_seed(seed)
    s, t = CPPN(sdef), Temporal(tdef)
    cfg = TrainConfig(depth_samples_per_ray_coarse=16, img_sample_size=64, favor_s_weight_delay_steps=0,
                      l1_weight_start=1e-3, l1_weight_end=1e-3, occl_weight_start=1e-2, dynamic_entro_weight_start=1e-3,
                      favor_s_weight_start=1e-3, entro_mask_thre=1e-6)
    return cfg, s, t, data, dev, CompositeTrainer


def run_steps(rank, world, n_steps=2, n_fine=0, depth_grads=False):
    cfg, s, t, data, dev, CompositeTrainer = build()
    kw = {}
    cfg.fine_depth_gradients = depth_grads
    if n_fine:
        from nerfca_amd import synthetic
        from nerfca_amd.model.CPPN import CPPN
        from nerfca_amd.model.Temporal import Temporal
        cfg.depth_samples_per_ray_fine = n_fine
        sdef, tdef = synthetic.net_definitions(dev, F=32, early=1, L=4, T=4)
        torch.manual_seed(11)
        kw = dict(static_model_fine=CPPN(sdef), temp_model_fine=Temporal(tdef), fine_sampler=oracle_fine_sampler)
    tr = CompositeTrainer(cfg, s, t, data, dev, rank=rank, world=world, seed=7, render=oracle_render, fused_adam=False, **kw)
    grads = None
    for it in range(n_steps):
        tr.step(100 + it)
        if it == 0:
            grads = torch.cat([p.grad.flatten() for p in tr.params]).clone()
    params = torch.cat([p.detach().flatten() for p in tr.params]).clone()
    run_steps.global_terms = tr.global_terms(torch.arange(13, dtype=torch.float64) * (rank + 1) + 0.5 * rank)    # (a made-up local vector)
    return grads, params


def _worker(rank, world, port, outdir, n_fine=0, depth_grads=False):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g, p = run_steps(rank, world, n_fine=n_fine, depth_grads=depth_grads)
        torch.save({"g": g, "p": p, "terms": run_steps.global_terms}, os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_step_equals_one_rank_step(tmp_path):
    torch.set_num_threads(2)
    g1, p1 = run_steps(0, 1)
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    # every rank holds the same all-reduced gradient and the same parameters
    assert torch.equal(r0["g"], r1["g"]) and torch.equal(r0["p"], r1["p"])
    # ... and they equal the single-process step up to f32 reduction order
    gerr = float((r0["g"] - g1).abs().max() / g1.abs().max())
    perr = float((r0["p"] - p1).abs().max() / p1.abs().max())
    assert gerr < 1e-5, gerr
    assert perr < 1e-5, perr
    # CompositeTrainer.global_terms: shares summed over the ranks, the two sigma maxima maximised
    loc = [torch.arange(13, dtype=torch.float64) * (r + 1) + 0.5 * r for r in (0, 1)]
    want = loc[0] + loc[1]
    want[3:5] = torch.maximum(loc[0][3:5], loc[1][3:5])
    assert torch.equal(r0["terms"], want) and torch.equal(r1["terms"], want)


@pytest.mark.timeout(300)
def test_two_rank_step_with_fine_pass_equals_one_rank_step(tmp_path):
    """The hierarchical pass under sharding: the weight maximum is all-reduced (MAX), the interval lengths come from ray 0
    of the GLOBAL batch (broadcast), the uniform draws are rows of one global table; four nets in the optimiser."""
    torch.set_num_threads(2)
    g1, p1 = run_steps(0, 1, n_fine=6)
    assert g1.numel() == p1.numel() and float(g1.abs().max()) > 0
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path), 6), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["g"], r1["g"]) and torch.equal(r0["p"], r1["p"])
    gerr = float((r0["g"] - g1).abs().max() / g1.abs().max())
    perr = float((r0["p"] - p1).abs().max() / p1.abs().max())
    assert gerr < 1e-5, gerr
    assert perr < 1e-5, perr


@pytest.mark.timeout(300)
def test_two_rank_step_with_depth_gradients_equals_one_rank_step(tmp_path):
    """fine_depth_gradients (the reference's undetached fine depths) under sharding: the backward of the batch-wide maximum sums
    its upstream gradient over the ranks and hands it to the rank holding the maximum; the gradient of ray 0's depths is summed
    over the ranks and handed to rank 0.  Two ranks = one rank up to f32 reduction order ON THIS PATH, whose terms carry
    2^k cos(2^k p) factors (1e-4; the detached case above stays at 1e-5) -- and the gradient is not the detached one."""
    torch.set_num_threads(2)
    g1, p1 = run_steps(0, 1, n_fine=6, depth_grads=True)
    g0, _ = run_steps(0, 1, n_fine=6, depth_grads=False)
    assert float((g1 - g0).abs().max() / g0.abs().max()) > 1e-2          # the through-depth term is there
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path), 6, True), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["g"], r1["g"]) and torch.equal(r0["p"], r1["p"])
    gerr = float((r0["g"] - g1).abs().max() / g1.abs().max())
    perr = float((r0["p"] - p1).abs().max() / p1.abs().max())
    assert gerr < 1e-4, gerr
    # parameters after two Adam steps: Adam divides by sqrt(v), so the noise of this path on near-zero gradient components
    # moves parameters by O(lr); the bound only guards against a wrong step
    assert perr < 1e-2, perr


def test_shards_partition_the_global_batch():
    cfg, s, t, data, dev, CompositeTrainer = build()
    ids = CompositeTrainer(cfg, s, t, data, dev, seed=3, render=oracle_render, fused_adam=False).draw_ray_ids(5)
    assert len(ids) == cfg.img_sample_size
    for world in (1, 2, 4, 8):
        cuts = [(len(ids) * r) // world for r in range(world + 1)]
        assert cuts[0] == 0 and cuts[-1] == len(ids) and all(b > a for a, b in zip(cuts, cuts[1:]))
    # same seed -> same ids on every rank
    ids2 = CompositeTrainer(cfg, s, t, data, dev, rank=1, world=2, seed=3, render=oracle_render, fused_adam=False).draw_ray_ids(5)
    assert np.array_equal(ids, ids2)


def _fine_trainer(window_steps=10):
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    cfg, s, t, data, dev, CompositeTrainer = build()
    cfg.depth_samples_per_ray_fine = 6
    cfg.fine_depth_gradients = False
    cfg.static_pos_enc_window_decay_steps = cfg.temp_pos_enc_window_decay_steps = window_steps
    sdef, tdef = synthetic.net_definitions(dev, F=32, early=1, L=4, T=4)
    torch.manual_seed(11)
    sf, tf = CPPN(sdef), Temporal(tdef)
    tr = CompositeTrainer(cfg, s, t, data, dev, seed=7, render=oracle_render, fused_adam=False, static_model_fine=sf, temp_model_fine=tf,
                          fine_sampler=oracle_fine_sampler)
    return tr, tf


def test_early_stop_of_the_autograd_step_reads_the_fine_pass():
    """run_composite.py:298-310: with a fine model pair the reference overwrites dynamic_entropy_loss / favor_s_loss with the
    FINE pass's values before its early-stop check.  A dead fine dynamic field (sigma_d == 0 exactly: blend weight 0, entropy 0)
    beside a live coarse one must raise the flag; the other way round (dead coarse, live fine) must not."""
    tr, tf = _fine_trainer()
    tr.step(5)
    assert tr.stop_flag is None and tr.early_stop() is False              # windows still opening
    tr.step(10)
    assert tr.stop_flag is not None and tr.early_stop() is False          # both passes alive
    with torch.no_grad():
        tf.output_linear[0].weight.zero_()
        tf.output_linear[0].bias.fill_(-1e4)
    tr.step(11)
    assert tr.early_stop() is True
    tr2, _ = _fine_trainer()
    with torch.no_grad():                                                 # dead COARSE dynamic field, live fine one
        tr2.t.output_linear[0].weight.zero_()
        tr2.t.output_linear[0].bias.fill_(-1e4)
    tr2.step(12)
    assert tr2.stop_flag is not None and tr2.early_stop() is False


def _stop_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []
        orig = dist.all_reduce
        dist.all_reduce = lambda t, *a, **k: (calls.append(t.numel()), orig(t, *a, **k))[1]
        cfg, s, t, data, dev, CompositeTrainer = build()
        cfg.static_pos_enc_window_decay_steps = cfg.temp_pos_enc_window_decay_steps = 10
        tr = CompositeTrainer(cfg, s, t, data, dev, rank=rank, world=world, seed=7, render=oracle_render, fused_adam=False)
        tr.step(10)
        n_params = sum(p.numel() for p in tr.params)
        torch.save({"flag": bool(tr.stop_flag), "calls": calls, "n_params": n_params}, os.path.join(outdir, f"stop{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_early_stop_scalars_ride_on_the_gradient_all_reduce(tmp_path):
    """Under ray sharding a steady-state step issues ONE collective: the early-stop predicate's two scalars are appended to the
    flat gradient buffer instead of being all-reduced on their own (one all-reduce per step)."""
    mp.spawn(_stop_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in (0, 1):
        rec = torch.load(tmp_path / f"stop{r}.pt")
        assert rec["flag"] is False
        assert rec["calls"] == [rec["n_params"] + 2], rec["calls"]
