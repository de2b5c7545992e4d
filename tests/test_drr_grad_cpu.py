"""Back-projection (nca_drr_backproject, drr.fit_volumes, tools/fit_volumes.py): everything that can be checked without a launch -- the
C-ABI surface, every refusal (with pointers that are never read), the f64 oracle of the GPU tests (tests/drr_adjoint_ref.py) against
autograd through torch's grid_sample and against the forward oracle's adjoint identity, and the command line's manifest reading."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import drr_adjoint_ref as adj
import drr_ref as ref
import nca_testlib as T
from nca_testlib import FAKE, capi, grid, lib  # noqa: F401

NEW = ("nca_drr_backproject", "nca_drr_set_backproject_runs", "nca_drr_get_backproject_runs")
refused = functools.partial(T.refused, "drr")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    assert header.index("int nca_drr_project(") < header.index("int nca_drr_backproject(") < header.index("nca_drr_last_error(void)")
    import nerfca_amd
    assert nerfca_amd.drr.fit_volumes


def test_backproject_refusals(capi, lib):
    def call(g="default", n_vol=1, R=8, S=4, o=FAKE, d=FAKE, z=FAKE, dists=FAKE, g_pix=FAKE, g_vol=FAKE):
        g = grid(capi) if g == "default" else g
        return lib.nca_drr_backproject(C.byref(g) if g is not None else None, n_vol, R, S, o, d, z, dists, g_pix, g_vol, None)

    refused(capi, lib, call(g=None), "nca_drr_backproject", "grid", "NULL")
    for name in ("o", "d", "z", "dists", "g_pix", "g_vol"):
        refused(capi, lib, call(**{name: None}), "nca_drr_backproject", {"o": "origins", "d": "dirs"}.get(name, name) + " is NULL")
    refused(capi, lib, call(n_vol=0), "n_vol = 0")
    refused(capi, lib, call(n_vol=-2), "n_vol = -2")
    refused(capi, lib, call(R=0), "R = 0")
    refused(capi, lib, call(R=-7), "R = -7")
    refused(capi, lib, call(S=0), "S = 0")
    refused(capi, lib, call(S=-1), "S = -1")
    T.grid_refusals("drr", capi, lib, lambda g, count: call(g=g, n_vol=count or 1))
    refused(capi, lib, call(R=1 << 62), "R = " + str(1 << 62))


def test_structure_switch(capi, lib):
    before = lib.nca_drr_get_backproject_runs()
    assert before in (0, 1)
    try:
        for k in (1, 0):
            assert lib.nca_drr_set_backproject_runs(k) == 0 and lib.nca_drr_get_backproject_runs() == k
        for bad in (2, -1, 4):
            refused(capi, lib, lib.nca_drr_set_backproject_runs(bad), f"runs = {bad}")
            assert lib.nca_drr_get_backproject_runs() == 0          # a refused value changes nothing
    finally:
        lib.nca_drr_set_backproject_runs(before)


def test_fit_volumes_refuses_the_cpu_and_an_empty_list(capi):
    from nerfca_amd import drr, synthetic
    geo = synthetic.xcat_geometry(8)
    with pytest.raises(capi.NcaError):
        drr.fit_volumes([], geo, (5, 3, 4), 8, n_phases=1, steps=1)
    with pytest.raises(capi.NcaError):
        drr.fit_volumes([(0.0, 0.0, 0, torch.zeros(8, 8))], geo, (5, 3, 4), 8, n_phases=1, steps=1)


# ----------------------------------------------------------------------------- the oracle
S, N_VOL, N_RAYS = 37, 3, 96


def aimed_rays(seed):
    """96 f64 rays from a shell of radius 3 aimed at points inside drr_ref.BOUNDS, f32 depths that span the box, positive f64 interval lengths."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((N_RAYS, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = np.stack([rng.uniform(lo, hi, N_RAYS) for lo, hi in ref.BOUNDS], -1)
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    z = np.linspace(1.2, 4.8, S).astype(np.float32)
    dists = (3.6 / (S - 1)) * rng.uniform(0.5, 1.5, S)
    return o, d, z, dists


def grid_sample_gradient(vols, o, d, z, dists, y, bounds):
    """d sum(pix y) / d vols in f64 through grid_sample, pix built as drr_ref.project_grid_sample builds it (i0 drops out)."""
    dt = torch.float64
    v = torch.from_numpy(vols).to(dt).requires_grad_(True)
    lo = torch.tensor([float(b[0]) for b in bounds], dtype=dt)
    hi = torch.tensor([float(b[1]) for b in bounds], dtype=dt)
    p = torch.from_numpy(o)[:, None, :] + torch.from_numpy(d)[:, None, :] * torch.from_numpy(z).to(dt)[None, :, None]
    u = (p - lo) / (hi - lo) * 2 - 1
    sig = torch.nn.functional.grid_sample(v[None], u.flip(-1)[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]
    pix = 1.0 - (sig * torch.from_numpy(dists)).sum(-1)
    (pix * torch.from_numpy(y)).sum().backward()
    return v.grad.numpy()


@pytest.mark.parametrize("shape", ref.GRIDS)
def test_oracle_equals_the_grid_sample_gradient_in_f64(shape):
    """Pins tests/drr_adjoint_ref.backproject to an independent implementation.  The two differ in how g is rounded (grid_sample works
    in [-1, 1] and maps back), not in the sum: a weight is off by at most a few max(n) 2^-52, so per node the difference is bounded by
    8 max(n) 2^-52 gross, gross = sum |g_pix dists_s| over the node's contributions.  Measured worst |diff| / gross: 4.5e-15 at
    17 x 9 x 33, 1.3e-16 at 5 x 3 x 4, 1.6e-16 at 2 x 2 x 2, against a bound of 5.9e-14 at n = 33."""
    o, d, z, dists = aimed_rays(seed=sum(shape))
    y = np.random.default_rng(7).standard_normal((N_VOL, N_RAYS))
    vols = ref.random_volume((N_VOL,) + shape, seed=3)
    want = grid_sample_gradient(vols, o, d, z, dists, y, ref.BOUNDS)
    got, mass, count = adj.backproject(shape, N_VOL, o, d, z, dists, y, ref.BOUNDS)
    gross = adj.gross(shape, N_VOL, o, d, z, dists, y, ref.BOUNDS)
    assert got.shape == want.shape == mass.shape == (N_VOL,) + shape and count.shape == shape and count.dtype == np.int64
    assert count.sum() > 4 * N_RAYS and (mass[:, count == 0] == 0).all() and (got[:, count == 0] == 0).all()
    diff = np.abs(got - want)
    hit = gross > 0
    print(f"oracle vs grid_sample gradient, grid {shape}: worst |diff| / gross = {(diff[hit] / gross[hit]).max():.2e}, "
          f"bound {8 * max(shape) * 2.0 ** -52:.2e}")
    assert (diff <= 8 * max(shape) * 2.0 ** -52 * gross).all()
    one, mass1, count1 = adj.backproject(shape, 1, o, d, z, dists, y[1], ref.BOUNDS)          # one volume, g_pix [R]: the same numbers
    assert np.array_equal(one[0], got[1]) and np.array_equal(mass1[0], mass[1]) and np.array_equal(count1, count)


@pytest.mark.parametrize("shape", ref.GRIDS)
def test_oracles_satisfy_the_adjoint_identity(shape):
    """sum((i0 - project(x)) y) = -sum(x backproject(y)) within 2^-50 sum(|x| mass); measured at most 3e-17 of that sum.  i0 = 0, so that
    i0 - pix is the ray sum exactly."""
    o, d, z, dists = aimed_rays(seed=1 + sum(shape))
    y = np.random.default_rng(8).standard_normal((N_VOL, N_RAYS))
    x = ref.random_volume((N_VOL,) + shape, seed=4)
    for bounds in (ref.BOUNDS, ref.SMALL_BOX):
        pix, _, _ = ref.project(x, o, d, z, dists, 0.0, bounds)
        g_vol, mass, _ = adj.backproject(shape, N_VOL, o, d, z, dists, y, bounds)
        lhs = float(((0.0 - pix) * y).sum())
        rhs = -float((x.astype(np.float64) * g_vol).sum())
        scale = float((np.abs(x).astype(np.float64) * mass).sum())
        print(f"adjoint identity of the oracles, grid {shape}: |lhs - rhs| = {abs(lhs - rhs):.2e} = {abs(lhs - rhs) / scale:.2e} of sum |x| mass")
        assert scale > 0 and abs(lhs - rhs) <= 2.0 ** -50 * scale


# ----------------------------------------------------------------------------- the command line
def test_cli_parses_its_arguments_and_reads_a_manifest(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fit_volumes as fv
        import project_volumes as pv
    finally:
        sys.path.pop(0)
    assert fv.parse_bounds is pv.parse_bounds          # imported, not copied
    assert fv.parse_shape("9, 8,7") == (9, 8, 7)
    for bad in ("", "9,8", "9,8,1", "a,b,c", "9,8,7,6"):
        with pytest.raises(ValueError):
            fv.parse_shape(bad)
    from nerfca_amd import synthetic
    geo = synthetic.xcat_geometry(8)
    views, phases = [[-5.0, 40.0, 0.0], [60.0, -30.0, 0.0]], [0, 2]
    pred = np.random.default_rng(0).standard_normal((2, 2, 8, 8)).astype(np.float32)
    np.save(tmp_path / "pred.npy", pred)
    manifest = {"views": views, "phases": phases, "samples": 24, "bounds": [[-1, 1], [-0.5, 0.75], [0, 2]], "volume_shape": [9, 9, 9], "geometry": geo,
                "files": {"pred": {"file": "pred.npy", "shape": [2, 2, 8, 8]}}}
    path = tmp_path / "manifest.json"
    path.write_text(json.dumps(manifest))
    argv = fv.join_args(["--frames", str(path), "--shape", "9,8,7", "--bounds", "-1,1,-1,1,-0.5,2", "--samples", "16", "--steps", "30", "--lr", "0.05", "--out", "o"])
    assert "--bounds=-1,1,-1,1,-0.5,2" in argv
    args = fv.parser().parse_args(argv)
    assert args.frames == str(path) and args.shape == (9, 8, 7) and args.bounds == ((-1.0, 1.0), (-1.0, 1.0), (-0.5, 2.0))
    assert args.samples == 16 and args.steps == 30 and args.lr == 0.05 and args.out == "o" and args.n_phases is None and not args.allow_negative
    args = fv.parser().parse_args(["--frames", "m.json", "--shape", "4,4,4", "--out", "o"])
    assert args.bounds is None and args.samples is None and args.steps == 200 and args.lr == 1e-2
    got_geo, frames, info = fv.load_frames(str(path))
    assert got_geo == {k: geo[k] for k in got_geo} and set(got_geo) >= {"DSD", "DSO", "nDetector", "max_pixel_value"}
    assert info == {"samples": 24, "bounds": ((-1.0, 1.0), (-0.5, 0.75), (0.0, 2.0)), "n_phases": 3}
    assert [(t, p, ph) for t, p, ph, _ in frames] == [(-5.0, 40.0, 0), (-5.0, 40.0, 2), (60.0, -30.0, 0), (60.0, -30.0, 2)]
    for k, (_, _, _, img) in enumerate(frames):
        assert img.dtype == np.float32 and img.flags["C_CONTIGUOUS"] and np.array_equal(img, pred[k // 2, k % 2])
    # a static-only manifest (render_views without --dynamic): phase 0 of every view, no bounds
    np.save(tmp_path / "pred.npy", pred[:, :1])
    path.write_text(json.dumps(dict(manifest, phases=None, bounds=None, files={"pred": {"file": "pred.npy", "shape": [2, 1, 8, 8]}})))
    _, frames, info = fv.load_frames(str(path))
    assert [f[2] for f in frames] == [0, 0] and info["n_phases"] == 1 and info["bounds"] is None
    # refused: a rolled C-arm, a stack that is not what the manifest says, a manifest of something else
    path.write_text(json.dumps(dict(manifest, views=[[0, 0, 10.0], [1, 1, 0]])))
    with pytest.raises(ValueError, match="larm"):
        fv.load_frames(str(path))
    path.write_text(json.dumps(manifest))
    with pytest.raises(ValueError, match="pred is"):
        fv.load_frames(str(path))
    path.write_text(json.dumps({"views": views}))
    with pytest.raises(ValueError, match="geometry"):
        fv.load_frames(str(path))
