"""GPU tests of the static-only loop's fused path (train/run_nerf.py, BASELINE configs[0]): the static loss kernel against an f64
restatement, StaticTrainer.fused_gradients_on against the reference's own three-step trajectory (tests/golden/static_step.npz),
the fused gradient against the autograd step's, the graph-replayed step against the host-launched one, two ray shards against one
rank, and evaluate against the oracle."""
import pytest
import torch

from conftest import rel_err
from nca_testlib import dev, model_def  # noqa: F401
from oracle import nerfca_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _flat_of(model, flat):
    """The flat gradient of the library in ``parameters()`` order and logical shapes (what ``p.grad`` holds)."""
    return torch.cat([g.reshape(-1) for g in model._binding.split_grads(flat)])


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("R,S", [(1, 7), (96, 64), (1000, 48), (257, 192), (64, 500)])
def test_static_loss_kernel_vs_f64(dev, R, S):
    """nca_static_loss_fwd_bwd against run_nerf.py:227-230 restated from the oracle's weighted_mse / occlusion under torch autograd in
    f64.  Terms and g_pix: 1e-10 relative (f64 tree sums of at most 1.3e7 same-sign terms round orders of magnitude below that);
    g_sigma: one f32 rounding of an f64 value, 2^-24 ~ 6e-8 < 1e-7, element-wise."""
    from nerfca_amd.fused import static_losses
    gen = torch.Generator().manual_seed(1000 * R + S)
    sigma = (torch.rand(R, S, generator=gen) * 3 + 1e-3).float()                   # positive f32
    dists = (torch.rand(S, generator=gen, dtype=torch.float64) * 0.05 + 1e-4)      # positive f64
    pix, gt = torch.randn(R, generator=gen, dtype=torch.float64), torch.randn(R, generator=gen, dtype=torch.float64)
    wpix = 1.0 + torch.rand(R, generator=gen, dtype=torch.float64)
    w_occl, reg_perc = 3e-2, 0.2
    for inv_R in (None, 0.5 / R):           # the default (1 / R) and a shard's share of a global batch twice as large
        p = pix.clone().requires_grad_(True)
        sg = sigma.double().requires_grad_(True)
        scale = 1.0 if inv_R is None else inv_R * R
        pixel = O.weighted_mse(p, gt, wpix).mean() * scale
        occl = torch.sum(O.occlusion(sg, dists, reg_perc)) * scale
        loss = pixel + w_occl * occl
        loss.backward()
        args = [t.to(dev) for t in (pix, gt, wpix, sigma, dists)]
        terms, g_pix, g_sigma = static_losses(*args, w_occl, inv_R=inv_R)
        torch.cuda.synchronize()
        assert terms.dtype == torch.float64 and g_pix.dtype == torch.float64 and g_sigma.dtype == torch.float32
        t = terms.cpu()
        errs = {"loss": abs(float(t[0]) - float(loss)) / abs(float(loss)), "pixel": abs(float(t[1]) - float(pixel)) / abs(float(pixel)),
                "occl": abs(float(t[2]) - float(occl)) / abs(float(occl))}
        gp_err = float(((g_pix.cpu() - p.grad).abs() / p.grad.abs().clamp(min=1e-300)).max())
        gs_err = float(((g_sigma.cpu().double() - sg.grad).abs() / sg.grad.abs()).max())
        print(f"R={R} S={S} inv_R={inv_R}: terms {errs} g_pix {gp_err:.2e} g_sigma {gs_err:.2e}")
        assert all(e < 1e-10 for e in errs.values()), errs
        assert float(t[3]) == 0.0
        assert gp_err < 1e-10, gp_err
        assert gs_err < 1e-7, gs_err
        # values only: the same term bits; a second call: identical bits everywhere
        tv, a, b = static_losses(*args, w_occl, inv_R=inv_R, want_grads=False)
        assert a is None and b is None and torch.equal(tv, terms)
        t32 = torch.zeros(4, dtype=torch.float32, device=dev)
        terms2, g_pix2, g_sigma2 = static_losses(*args, w_occl, inv_R=inv_R, terms_f32=t32)
        assert torch.equal(terms2, terms) and torch.equal(g_pix2, g_pix) and torch.equal(g_sigma2, g_sigma)
        assert torch.equal(t32, terms.to(torch.float32))


# ----------------------------------------------------------------------------- 2. the reference's trajectory
def test_static_fused_steps_vs_reference(golden, dev):
    """Three iterations of the static-only loop (train/run_nerf.py:186-231) through StaticTrainer.fused_gradients_on + Adam/LinearLR
    against the reference's own trajectory (tests/golden/static_step.npz): the bounds of test_static_training_steps_vs_reference."""
    from types import SimpleNamespace
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.train.trainer import StaticTrainer, TrainConfig
    g = golden("static_step")
    s = CPPN(model_def(F=64, device=dev))
    s.load_state_dict(g.prefixed("init_sp_"))
    s = s.to(dev)
    R, S = g["o"].shape[0], g["z"].shape[0]
    cfg = TrainConfig(depth_samples_per_ray_coarse=S, img_sample_size=R, occl_weight_start=float(g["occl_weight_start"]),
                      occl_reg_perc=float(g["occl_reg_perc"]))
    geo = {"near_thresh": 3.4259, "far_thresh": 5.5741, "max_pixel_value": float(g["I0"][0])}
    tr = StaticTrainer(cfg, s, SimpleNamespace(geo=geo), dev, fused_adam=False)
    assert torch.equal(tr.depth.cpu(), g["z"])
    o, d, gt, w, I0 = (g[k].to(dev) for k in ("o", "d", "gt", "wpix", "I0"))
    base = int(g["base_iter"])
    for k in range(3):
        n_iter = base + k
        tr.update_window(n_iter)
        terms, flat, pix = tr.fused_gradients_on(n_iter, o, d, I0, gt, w, g[f"step{k}_t_rand"])
        loss, pixel, occl = (float(x) for x in terms[:3].cpu())
        assert pix.dtype == g[f"step{k}_pix"].dtype
        e_pix = rel_err(pix.cpu(), g[f"step{k}_pix"])
        e_loss = abs(loss - float(g[f"step{k}_loss"])) / abs(float(g[f"step{k}_loss"]))
        e_occl = abs(occl - float(g[f"step{k}_occl"])) / abs(float(g[f"step{k}_occl"]))
        print(f"step {k}: pix {e_pix:.2e} loss {e_loss:.2e} occl {e_occl:.2e}")
        assert e_pix < TOL and e_loss <= TOL and e_occl <= TOL
        assert abs(pixel - float(g[f"step{k}_pixel"])) <= TOL * abs(float(g[f"step{k}_pixel"]))
        tr.opt.zero_grad()
        for p, gr in zip(s.parameters(), s._binding.split_grads(flat)):
            p.grad = gr
        if k == 0:
            for name, gr in g.prefixed("step0_sg_").items():
                assert rel_err(dict(s.named_parameters())[name].grad.cpu(), gr) < TOL, name
        tr.opt.step()
        tr.sched.step()
    for name, v in g.prefixed("final_sp_").items():      # Adam amplifies rounding noise of near-zero gradient entries
        assert rel_err(dict(s.named_parameters())[name].detach().cpu(), v) < 1e-4, name


# ----------------------------------------------------------------------------- synthetic trainers
_DATA = {}


def _data(dev):
    from nerfca_amd import synthetic
    if "d" not in _DATA:
        _DATA["d"] = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)
    return _DATA["d"]


def _trainer(dev, prec, rank=0, world=1, model=None, seed=5, **cfg_kw):
    from nerfca_amd import set_precision, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.train.trainer import StaticTrainer, TrainConfig
    if model is None:
        torch.manual_seed(9)
        model = CPPN(synthetic.net_definitions(dev, F=64)[0]).to(dev)
        set_precision(prec, model)
    kw = dict(depth_samples_per_ray_coarse=48, img_sample_size=512, occl_weight_start=1e-2, lr=5e-3, lr_decay_steps=6, lr_end_factor=0.1,
              static_pos_enc_window_decay_steps=40)
    kw.update(cfg_kw)
    return StaticTrainer(TrainConfig(**kw), model, _data(dev), dev, rank=rank, world=world, seed=seed)


# ----------------------------------------------------------------------------- 3. fused gradient == autograd gradient
@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("bf16", 1e-3)])
def test_fused_gradients_equal_autograd_step(dev, prec, tol):
    """Two routes through the same render kernels: ``step``'s body up to ``backward`` (torch loss operations under autograd) and
    ``fused_gradients`` (HIP loss kernel, no autograd graph), same parameters, same iteration."""
    tr = _trainer(dev, prec)
    n_iter = 7
    tr.update_window(n_iter)
    ids = tr.draw_ray_ids_device(n_iter)
    rays = tr.data.rays_train.index_select(0, ids)
    loss, pixel, occl, _ = tr.loss_on(n_iter, rays[:, 0, :], rays[:, 1, :], tr.I0[: len(ids)], rays[:, 2, 0], rays[:, 3, 0], tr.draw_jitter(n_iter))
    tr.opt.zero_grad(set_to_none=True)
    loss.backward()
    auto = torch.cat([p.grad.reshape(-1) for p in tr.s.parameters()]).clone()
    terms, flat, _ = tr.fused_gradients(n_iter)
    fused = _flat_of(tr.s, flat)
    err = rel_err(fused.cpu(), auto.cpu())
    print(f"{prec}: gradient rel_err {err:.2e}; loss {float(terms[0]):.6e} vs {float(loss):.6e}")
    assert float(auto.abs().max()) > 0
    assert err < tol, err
    for got, want in zip(terms[:3].cpu(), (loss, pixel, occl)):
        assert abs(float(got) - float(want)) <= tol * abs(float(want))


# ----------------------------------------------------------------------------- 4. graph vs eager
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_static_graph_step_matches_eager_step(dev, prec, monkeypatch):
    """StaticTrainer.step_graph (captured HIP graph + library Adam/LinearLR, ids / jitter / window made on the device) follows the
    trajectory of step_fused with torch.optim.Adam: same loss at every call (calls at iterations 0, 3, 6, ...: the counter is set
    from the host when a call is not the previous one's successor), same final parameters.  Then 200 consecutive replays: no
    begin_step call from the host after the capture, and the loss ends below where it started."""
    from nerfca_amd import fused
    calls = {"n": 0}
    real = fused.begin_step

    def counting(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(fused, "begin_step", counting)
    outs = []
    for graph in (False, True):
        tr = _trainer(dev, prec)
        losses = []
        for it in range(8):
            out = tr.step_graph(3 * it) if graph else tr.step_fused(3 * it)
            assert len(out) == 3
            losses.append(float(out[0]))
        outs.append((losses, torch.cat([p.detach().flatten() for p in tr.params]).cpu()))
        if graph:
            assert getattr(tr, "_graph", None) is not None, "step_graph did not replay a graph"
    tol = 1e-5 if prec == "f32" else 1e-3
    print(f"{prec}: eager {outs[0][0]}\n      graph {outs[1][0]}\n      params rel_err {rel_err(outs[1][1], outs[0][1]):.2e}")
    for a, b in zip(*[o[0] for o in outs]):
        assert abs(a - b) <= tol * abs(a), (outs[0][0], outs[1][0])
    assert rel_err(outs[1][1], outs[0][1]) < tol
    # 200 consecutive replays on a fresh trainer
    tr = _trainer(dev, prec, lr=2e-3, lr_decay_steps=150000, lr_end_factor=0.01)
    first = float(tr.step_graph(0)[0])
    after_capture = calls["n"]
    assert after_capture >= 1          # (the eager warm-up and the capture itself)
    last = []
    for it in range(1, 200):
        out = tr.step_graph(it)
        if it >= 190:
            last.append(float(out[0]))
    assert calls["n"] == after_capture, "a replay called begin_step from the host"
    assert int(tr._iter_dev.item()) == 200 and int(tr.adam.step_count.item()) == 200
    tr.check_ray_ids()
    end = sum(last) / len(last)
    print(f"{prec}: 200 replays, loss {first:.4e} -> {end:.4e}")
    assert end < first, (first, end)


def test_static_graph_step_routes_without_device_form(dev):
    """nerfies_windowed has no device form: step_graph runs step_fused (no graph is captured) and returns the same triple."""
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd import synthetic
    torch.manual_seed(9)
    m = CPPN(synthetic.net_definitions(dev, F=64, pos_enc="nerfies_windowed")[0]).to(dev)
    m.update_windowed_alpha(1, 40)
    tr = _trainer(dev, "f32", model=m, static_pos_enc="nerfies_windowed")
    out = tr.step_graph(1)
    assert len(out) == 3 and getattr(tr, "_graph", None) is None
    assert torch.isfinite(out[0])
    # a draw method overridden AFTER a graph was captured is followed from then on: the call runs step_fused, which asks the method
    tr2 = _trainer(dev, "f32")
    tr2.step_graph(0)
    assert getattr(tr2, "_graph", None) is not None
    asked = []
    real = tr2.draw_jitter
    tr2.draw_jitter = lambda n: (asked.append(n), real(n))[1]
    out = tr2.step_graph(1)
    assert asked == [1] and torch.isfinite(out[0])


# ----------------------------------------------------------------------------- 5. two shards == one rank
@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("bf16", 1e-3)])
def test_two_static_shards_equal_one_rank(dev, prec, tol):
    """Two StaticTrainer objects of one process, (rank, world) = (0, 2) and (1, 2), same seed and the same net: their flat gradients add
    up to the one-rank gradient (f32 summation order: 1e-5; bf16 rounds the per-shard partial sums differently: 1e-3) and their
    terms -- shares of the global values -- to the one-rank terms within 1e-10."""
    one = _trainer(dev, prec)
    n_iter = 11
    one.update_window(n_iter)
    t1, g1, pix1 = one.fused_gradients(n_iter)
    g1, t1 = g1.clone(), t1.clone()
    shards = [_trainer(dev, prec, rank=r, world=2, model=one.s) for r in range(2)]
    parts = [tr.fused_gradients(n_iter) for tr in shards]
    assert parts[0][2].shape[0] + parts[1][2].shape[0] == pix1.shape[0]
    gsum = parts[0][1].double() + parts[1][1].double()
    tsum = parts[0][0] + parts[1][0]
    err = rel_err(gsum.cpu(), g1.double().cpu())
    terr = [abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(tsum[:3].cpu(), t1[:3].cpu())]
    print(f"{prec}: gradient rel_err {err:.2e}, terms {terr}")
    assert float(g1.abs().max()) > 0
    assert err < tol, err
    # (a forward tile never spans two rays, so a shard's rays render as they do in the whole batch, in bf16 too: only the f64 sums over
    # rays are split differently)
    assert all(e < 1e-10 for e in terr), terr


# ----------------------------------------------------------------------------- 6. evaluate
def test_static_evaluate_vs_oracle(dev):
    """The display_every block of run_nerf.py:254-291 on the 16^2 held-out view against the oracle (predict_static + weighted_mse +
    occlusion), after graph-replayed steps and WITHOUT a manual update_window: evaluate sets iteration n_iter's window itself."""
    tr = _trainer(dev, "f32")
    with torch.no_grad():          # (a default-init net renders an almost constant image: give it contrast, as synthetic.make_dataset does for its teacher)
        tr.s.output_linear[0].weight.mul_(40.0)
        tr.s.output_linear[0].bias.fill_(-1.0)
    for it in range(3):
        tr.step_graph(it)
    assert getattr(tr, "_graph", None) is not None
    n_iter, steps = 20, tr.cfg.static_pos_enc_window_decay_steps
    ev = tr.evaluate(n_iter)
    torch.cuda.synchronize()
    data, c = tr.data, tr.cfg
    ps = {k: v.detach().cpu().clone() for k, v in tr.s.state_dict().items()}
    spec = O.NetSpec(num_filters=64)
    o, d = data.test_origins.cpu(), data.test_directions.cpu()
    R = o.shape[0]
    I0 = torch.full((R,), data.geo["max_pixel_value"])
    zj = O.stratified_depths(tr.depth.cpu(), tr._test_jitter)

    def oracle(window_iter):
        win = O.freq_mask_alpha(12, window_iter, steps, 1)[0]
        with torch.no_grad():
            pix, sig, dists = O.predict_static(ps, spec, win, o, d, I0, zj)
            gt = data.test_image.cpu().to(pix.dtype)
            pixel = O.weighted_mse(pix, gt, torch.ones(R, dtype=pix.dtype)).mean()
            occl = torch.sum(O.occlusion(sig, dists, c.occl_reg_perc))
            loss = pixel + c.occl_weight_start * occl
        return pix, float(loss), float(pixel), float(occl)

    pix, loss, pixel, occl = oracle(n_iter)
    assert ev["pred"].dtype == torch.float32 and ev["pred"].shape == (R,)
    errs = {"pred": rel_err(ev["pred"].cpu(), pix), "loss": abs(float(ev["test_loss"]) - loss) / abs(loss),
            "pixel": abs(float(ev["test_pixel_loss"]) - pixel) / abs(pixel), "occl": abs(float(ev["test_occl_loss"]) - occl) / abs(occl),
            "psnr": abs(float(ev["test_psnr"]) - (-10.0 * torch.log10(torch.tensor(loss)).item())) / abs(-10.0 * torch.log10(torch.tensor(loss)).item())}
    print(f"evaluate vs oracle: {errs}")
    assert all(e < TOL for e in errs.values()), errs
    # the stale window (iteration 0's, which the module still holds after the graph steps) renders an image that the bound above rejects
    stale = oracle(0)[0]
    print(f"stale window vs iteration {n_iter}'s: pred rel_err {rel_err(stale, pix):.2e}")
    assert rel_err(stale, pix) > TOL
    # (the stale-window property is carried by the oracle comparison above.)  What follows checks something else: the graph steps leave
    # nothing behind that evaluate depends on -- a fresh trainer on the same parameters, which never captured a graph, evaluates to the same bits
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd import synthetic
    m = CPPN(synthetic.net_definitions(dev, F=64)[0])
    m.load_state_dict(ps)
    m = m.to(dev)
    fresh = _trainer(dev, "f32", model=m)
    ev2 = fresh.evaluate(n_iter)
    assert torch.equal(ev2["pred"], ev["pred"]) and torch.equal(ev2["test_loss"], ev["test_loss"])
