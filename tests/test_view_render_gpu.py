"""View rendering on the GPU: the kernels of csrc/view/nca_view.hip against their host definitions, and export.render_view /
render_sequence / density_volumes against the composite path they replace."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from nca_testlib import dev  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-5             # the project's f32 bound (tests/test_hip_parity.py)
BF_OUT = 2e-3          # the project's bf16 output bound (tests/test_hip_parity.py)
VIEWS = [(-5, 40), (60, -30), (0, 0), (137.5, -63)]


def geometries():
    from nerfca_amd import synthetic
    xcat = synthetic.xcat_geometry(16)
    return {"xcat16": xcat, "12x20": dict(xcat, nDetector=[12, 20], dDetector=[2.0 / 12, 2.0 / 20], offDetector=[0.013, -0.02])}


def make_pair(dev, F_s, F_d, seed=5):
    from nerfca_amd import synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    torch.manual_seed(seed)
    s = CPPN(synthetic.net_definitions(dev, F=F_s)[0]).to(dev)
    t = Temporal(synthetic.net_definitions(dev, F=F_d)[1]).to(dev)
    for m in (s, t):
        m.update_freq_mask_alpha(75000, 150000)
    return s, t


@torch.no_grad()
def composite_reference(s, t, geo, theta, phi, phase, S, dev):
    """The composite render of one frame on the device-generated rays, and the two single-field images as CompositeTrainer.evaluate
    forms them from its sigmas."""
    from nerfca_amd import export, render_rays
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    W, H = geo["nDetector"]
    o, d = export.view_rays(geo, theta, phi, device=dev)
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], S, dev)
    dists = _interval_lengths(z, d)
    I0 = torch.full((W * H,), geo["max_pixel_value"], dtype=torch.float32, device=dev)
    ph = torch.full((W * H,), phase, dtype=torch.int32, device=dev)
    pix, sig_s, sig_d = render_rays(s, t, o, d, ph, I0, z, dists)
    i0 = I0[0].double()
    return (pix.reshape(W, H), (i0 - (sig_s.double() * dists).sum(-1)).reshape(W, H), (i0 - (sig_d.double() * dists).sum(-1)).reshape(W, H))


# ----------------------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("geo_name", ["xcat16", "12x20"])
def test_rays_match_the_host_function(dev, geo_name):
    from nerfca_amd import export
    from nerfca_amd.train.proj_helpers import get_ray_values_tigre
    geo = geometries()[geo_name]
    W, H = geo["nDetector"]
    for theta, phi in VIEWS:
        ho, hd = get_ray_values_tigre(theta, phi, 0, geo, "cpu")
        ho, hd = torch.from_numpy(np.ascontiguousarray(ho)).reshape(-1, 3), torch.from_numpy(np.ascontiguousarray(hd)).reshape(-1, 3)
        o32, d32 = export.view_rays(geo, theta, phi, device=dev, dtype=torch.float32)
        o64, d64 = export.view_rays(geo, theta, phi, device=dev)
        assert o32.shape == d32.shape == (W * H, 3) and o64.dtype == d64.dtype == torch.float64
        assert torch.equal(o32.cpu(), ho), (theta, phi)
        err = rel_err(d32.cpu(), hd)
        print(f"{geo_name} view ({theta}, {phi}): rel_err(dirs) = {err:.3e}")
        assert err < 1e-6, (theta, phi, err)
        assert torch.equal(o64, o32.double()) and torch.equal(d64, d32.double())
        o_again, d_again = export.view_rays(geo, theta, phi, device=dev, dtype=torch.float32)
        assert torch.equal(o_again, o32) and torch.equal(d_again, d32)
        for dt, (fo, fd) in ((torch.float32, (o32, d32)), (torch.float64, (o64, d64))):
            po, pd = export.view_rays(geo, theta, phi, p0=37, n=101, device=dev, dtype=dt)
            assert po.shape == (101, 3) and torch.equal(po, fo[37:138]) and torch.equal(pd, fd[37:138])
        to, td = export.view_rays(geo, theta, phi, p0=W * H - 1, device=dev)          # n defaults to the rest of the image
        assert to.shape == (1, 3) and torch.equal(td, d64[-1:])


def test_query_points_are_the_render_kernels_points(dev):
    from nerfca_amd import export
    geo = geometries()["12x20"]
    z = torch.linspace(3.4, 5.6, 7, device=dev)
    o, d = export.view_rays(geo, 60, -30, p0=11, n=130, device=dev)
    pts = export._query_points(o, d, z).reshape(130, 7, 3)
    assert torch.equal(pts, (o[:, None, :] + d[:, None, :] * z.double()[None, :, None]).float())
    with pytest.raises(Exception, match="float64 rays"):
        export._query_points(o.float(), d.float(), z)


# ----------------------------------------------------------------------------- 2. compose
@pytest.mark.parametrize("n", [1, 63, 257, 4099])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_compose(dev, n, dt):
    from nerfca_amd import export
    g = torch.Generator().manual_seed(n)
    i0 = 2.15991
    pix_s = (i0 - torch.rand(n, generator=g, dtype=torch.float64)).to(dt).to(dev)
    pix_d = (i0 - 0.3 * torch.rand(n, generator=g, dtype=torch.float64)).to(dt).to(dev)
    pred, pred_s, pred_d = (torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
    export.compose_images(pix_s, pix_d, i0, pred, pred_s, pred_d)
    assert torch.equal(pred, ((pix_s.double() + pix_d.double()) - i0).float())
    assert torch.equal(pred_s, pix_s.float()) and torch.equal(pred_d, pix_d.float())
    pred2, pred_s2, pred_d2 = (torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
    export.compose_images(pix_s, None, i0, pred2, pred_s2, pred_d2)             # a static-only model
    assert torch.equal(pred_s2, pix_s.float()) and torch.equal(pred2, pred_s2)
    assert torch.equal(pred_d2, torch.full((n,), i0, dtype=torch.float64).float().to(dev))


# ----------------------------------------------------------------------------- 3. normalise
@pytest.mark.parametrize("n", [1, 2, 255, 256, 70001])
@pytest.mark.parametrize("n_img", [1, 3])
def test_normalize(dev, n, n_img):
    from nerfca_amd import export
    g = torch.Generator().manual_seed(7 * n + n_img)
    x = torch.randn(n_img, n, generator=g)
    for k in range(n_img):          # the extreme values sit at the first and the last element, in either order
        lo, hi = -7.5 - k, 9.25 + 2 * k
        x[k, 0], x[k, -1] = (lo, hi) if k % 2 == 0 else (hi, lo)
    x = x.to(dev)
    out, mm = export.normalize_images(x)
    assert out.shape == x.shape and mm.shape == (n_img, 2)
    assert torch.equal(mm[:, 0], x.min(dim=1).values) and torch.equal(mm[:, 1], x.max(dim=1).values)
    if n == 1:                      # a constant image: zeros where the reference's expression gives 0 / 0
        assert torch.equal(out, torch.zeros_like(x))
    else:
        lo, hi = x.min(dim=1, keepdim=True).values, x.max(dim=1, keepdim=True).values
        err = float((out.double() - ((x - lo) / (hi - lo)).double()).abs().max())
        print(f"n = {n}, n_img = {n_img}: max |out - (x - min) / (max - min)| = {err:.3e}")
        assert err <= 2.0 ** -23
        assert float(out.min()) == 0.0 and float(out.max()) == 1.0
    out2, mm2 = export.normalize_images(x)
    assert torch.equal(out2, out) and torch.equal(mm2, mm)
    none, mm3 = export.normalize_images(x, want_out=False)
    assert none is None and torch.equal(mm3, mm)
    const = torch.full((n_img, n), -3.25, device=dev)
    out_c, mm_c = export.normalize_images(const)
    assert torch.equal(out_c, torch.zeros_like(const)) and torch.equal(mm_c, torch.full((n_img, 2), -3.25, device=dev))


@pytest.mark.parametrize("where", [0, 300, 70000])
def test_normalize_propagates_nan_as_torch_does(dev, where):
    from nerfca_amd import export
    x = torch.randn(2, 70001, generator=torch.Generator().manual_seed(where)).to(dev)
    x[1, where] = float("nan")
    out, mm = export.normalize_images(x)
    assert torch.equal(mm[0], torch.stack([x[0].min(), x[0].max()])) and not bool(torch.isnan(out[0]).any())
    assert bool(torch.isnan(mm[1]).all()) and bool(torch.isnan(out[1]).all())          # torch.min / torch.max of the image are NaN too
    assert bool(torch.isnan(x[1].min())) and bool(torch.isnan(x[1].max()))


# ----------------------------------------------------------------------------- 4. - 6. one view against the composite path
@pytest.mark.parametrize("widths", [(128, 128), (64, 32), (136, 136)])
def test_render_view_matches_the_composite_render_f32(dev, widths):
    from nerfca_amd import export
    geo, S = geometries()["xcat16"], 48
    s, t = make_pair(dev, *widths)
    theta, phi, phase = 60, -30, 3
    out = export.render_view(s, t, geo, theta, phi, phase, S, chunk_rays=100)
    assert all(out[k].shape == (16, 16) and out[k].dtype == torch.float32 for k in ("pred", "pred_static", "pred_dynamic"))
    ref = composite_reference(s, t, geo, theta, phi, phase, S, dev)
    for k, r in zip(("pred", "pred_static", "pred_dynamic"), ref):
        err = rel_err(out[k], r)
        print(f"widths {widths} {k}: rel_err = {err:.3e}")
        assert err < TOL, (k, err)
    whole = export.render_view(s, t, geo, theta, phi, phase, S, chunk_rays=65536)
    for k in ("pred", "pred_static", "pred_dynamic"):
        assert torch.equal(whole[k], out[k]), k
    other = export.render_view(s, t, geo, theta, phi, 7, S)          # the phase reaches the dynamic field, and only it
    assert torch.equal(other["pred_static"], out["pred_static"]) and not torch.equal(other["pred_dynamic"], out["pred_dynamic"])


def test_render_view_matches_the_composite_render_bf16(dev):
    from nerfca_amd import export, set_precision
    geo, S = geometries()["xcat16"], 48
    s, t = make_pair(dev, 128, 128)
    set_precision("bf16", s, t)
    out = export.render_view(s, t, geo, -5, 40, 2, S, chunk_rays=100)
    ref = composite_reference(s, t, geo, -5, 40, 2, S, dev)
    for k, r in zip(("pred", "pred_static", "pred_dynamic"), ref):
        err = rel_err(out[k], r)
        print(f"bf16 {k}: rel_err = {err:.3e}")
        assert err < BF_OUT, (k, err)
    whole = export.render_view(s, t, geo, -5, 40, 2, S)
    for k in ("pred", "pred_static", "pred_dynamic"):
        assert torch.equal(whole[k], out[k]), k


def test_render_view_static_only_one_sample_and_normalised(dev):
    from nerfca_amd import export, render_rays
    from nerfca_amd.train.data_helpers import create_depth_values
    from nerfca_amd.train.model_helpers import _interval_lengths
    geo = geometries()["12x20"]
    s, t = make_pair(dev, 64, 64)
    i0 = torch.tensor(geo["max_pixel_value"], dtype=torch.float32, device=dev)
    out = export.render_view(s, None, geo, 0, 0, None, 24, chunk_rays=100, normalize=True)
    o, d = export.view_rays(geo, 0, 0, device=dev)
    z = create_depth_values(geo["near_thresh"], geo["far_thresh"], 24, dev)
    with torch.no_grad():
        pix, _ = render_rays(s, None, o, d, None, i0.expand(o.shape[0]), z, _interval_lengths(z, d), single=True)
    assert out["pred"].shape == (12, 20) and torch.equal(out["pred_static"], pix.float().reshape(12, 20))
    assert torch.equal(out["pred"], out["pred_static"]) and torch.equal(out["pred_dynamic"], i0.expand(12, 20))
    lo, hi = out["pred"].min(), out["pred"].max()
    assert torch.equal(out["minmax"]["pred"], torch.stack([lo, hi]))
    assert float((out["pred_norm"] - (out["pred"] - lo) / (hi - lo)).abs().max()) <= 2.0 ** -23
    assert torch.equal(out["pred_dynamic_norm"], torch.zeros(12, 20, device=dev))          # a constant image
    one = export.render_view(s, t, geo, 137.5, -63, 4, 1)                                   # one sample per ray
    ref = composite_reference(s, t, geo, 137.5, -63, 4, 1, dev)
    for k, r in zip(("pred", "pred_static", "pred_dynamic"), ref):
        assert rel_err(one[k], r) < TOL, k


# ----------------------------------------------------------------------------- 7. sequences
def test_render_sequence_is_render_view_per_frame_with_one_static_pass_per_view(dev, monkeypatch):
    from nerfca_amd import export, synthetic
    geo, S = synthetic.xcat_geometry(8), 32
    s, t = make_pair(dev, 32, 32)
    views, phases = [(-5, 40), (60, -30, 0)], [0, 3, 9]
    calls = {"static": 0, "dynamic": 0}
    render_static, render_dynamic = export._render_static_chunk, export._render_dynamic_chunk

    def counted_static(model, *a):
        assert model is s
        calls["static"] += 1
        return render_static(model, *a)

    def counted_dynamic(model, *a):
        assert model is t
        calls["dynamic"] += 1
        return render_dynamic(model, *a)

    monkeypatch.setattr(export, "_render_static_chunk", counted_static)
    monkeypatch.setattr(export, "_render_dynamic_chunk", counted_dynamic)
    seq = export.render_sequence(s, t, geo, views, phases, S, chunk_rays=50, normalize=True)
    chunks = len(export.chunk_plan(64, 50))
    assert chunks == 2 and calls == {"static": 2 * chunks, "dynamic": 2 * 3 * chunks}, calls          # V x chunks, not V x P x chunks
    monkeypatch.undo()
    assert seq["pred"].shape == seq["pred_dynamic"].shape == (2, 3, 8, 8) and seq["pred_static"].shape == (2, 8, 8)
    assert seq["minmax"]["pred"].shape == (2, 3, 2) and seq["minmax"]["pred_static"].shape == (2, 2)
    for v, view in enumerate(views):
        for j, phase in enumerate(phases):
            one = export.render_view(s, t, geo, view[0], view[1], phase, S, chunk_rays=50, normalize=True)
            assert torch.equal(seq["pred"][v, j], one["pred"]) and torch.equal(seq["pred_dynamic"][v, j], one["pred_dynamic"])
            assert torch.equal(seq["pred_static"][v], one["pred_static"])
            assert torch.equal(seq["pred_norm"][v, j], one["pred_norm"]) and torch.equal(seq["minmax"]["pred"][v, j], one["minmax"]["pred"])
            assert torch.equal(seq["pred_static_norm"][v], one["pred_static_norm"])
            assert torch.equal(seq["pred_dynamic_norm"][v, j], one["pred_dynamic_norm"])


# ----------------------------------------------------------------------------- 8. volumes
def test_density_volumes_equal_density_volume_per_phase(dev):
    from nerfca_amd import export
    s, t = make_pair(dev, 64, 64)
    kw = dict(resolution=(5, 4, 3), chunk_points=50)
    sig_s, sig_d = export.density_volumes(s, t, (0, 3), **kw)
    assert sig_s.shape == (5, 4, 3) and sig_d.shape == (2, 5, 4, 3)
    for j, phase in enumerate((0, 3)):
        one_s, one_d = export.density_volume(s, t, phase, **kw)
        assert torch.equal(sig_s, one_s) and torch.equal(sig_d[j], one_d)
    assert not torch.equal(sig_d[0], sig_d[1])
    only_s, none = export.density_volumes(s, None, (), **kw)
    assert none is None and torch.equal(only_s, export.density_volume(s, None, None, **kw)[0])


# ----------------------------------------------------------------------------- 9. command line
def test_render_views_cli_writes_the_sequence(dev, tmp_path):
    from nerfca_amd import export, synthetic
    s, t = make_pair(dev, 32, 32)
    s.save(str(tmp_path / "static.pth"), {})
    t.save(str(tmp_path / "dynamic.pth"), {})
    out_dir = tmp_path / "renders"
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "render_views.py"), "--static", str(tmp_path / "static.pth"),
           "--dynamic", str(tmp_path / "dynamic.pth"), "--geometry", "xcat", "--n-det", "8", "--views", "-5,40;60,-30", "--phases", "1,6",
           "--samples", "16", "--chunk-rays", "50", "--normalize", "--out", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    seq = export.render_sequence(s, t, synthetic.xcat_geometry(8), [(-5, 40), (60, -30)], [1, 6], 16, chunk_rays=50, normalize=True)
    for k in ("pred", "pred_static", "pred_dynamic", "pred_norm", "pred_static_norm", "pred_dynamic_norm"):
        assert np.array_equal(np.load(out_dir / (k + ".npy")), seq[k].cpu().numpy()), k
    manifest = json.load(open(out_dir / "manifest.json"))
    assert manifest["views"] == [[-5.0, 40.0, 0.0], [60.0, -30.0, 0.0]] and manifest["phases"] == [1, 6]
    assert manifest["files"]["pred"]["shape"] == [2, 2, 8, 8] and manifest["files"]["pred_static"]["shape"] == [2, 8, 8]
    assert manifest["minmax"]["pred"] == seq["minmax"]["pred"].cpu().tolist()
