"""Total-variation priors (nca_vol_tv, nca_vol_tv_grad, drr.total_variation, the tv_* arguments of drr.fit_volumes and
tools/fit_volumes.py): everything that can be checked without a launch -- the C-ABI surface, every refusal of both entry points (with
pointers that are never read), the f64 oracle of the GPU tests (tests/voltv_ref.py) against torch autograd in f64, the refusals of the
Python layer and the command line."""
import ctypes as C
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import drr_ref
import voltv_ref as ref
import nca_testlib as T
from nca_testlib import FAKE, capi, grid, lib  # noqa: F401

NEW = ("nca_vol_tv", "nca_vol_tv_grad", "nca_vol_last_error")
refused = functools.partial(T.refused, "vol")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    assert header.index("nca_drr_last_error(void)") < header.index("int nca_vol_tv(") < header.index("int nca_vol_tv_grad(") < header.index("nca_vol_last_error(void)")
    assert callable(capi.check_vol)
    import nerfca_amd
    assert nerfca_amd.drr.total_variation


@pytest.mark.parametrize("entry", ["nca_vol_tv", "nca_vol_tv_grad"])
def test_refusals(capi, lib, entry):
    def call(g="default", vol=FAKE, n_vol=1, eps_s=1e-3, eps_t=1e-3, cyclic=1, out=FAKE, scale=FAKE, g_vol=FAKE):
        g = grid(capi) if g == "default" else g
        gp = C.byref(g) if g is not None else None
        if entry == "nca_vol_tv":
            return lib.nca_vol_tv(gp, vol, n_vol, eps_s, eps_t, cyclic, out, None)
        return lib.nca_vol_tv_grad(gp, vol, n_vol, eps_s, eps_t, cyclic, scale, g_vol, None)

    refused(capi, lib, call(g=None), entry + ":", "grid", "NULL")
    for name in ("vol",) + (("out",) if entry == "nca_vol_tv" else ("scale", "g_vol")):
        refused(capi, lib, call(**{name: None}), entry + ":", name + " is NULL")
    refused(capi, lib, call(n_vol=0), "n_vol = 0")
    refused(capi, lib, call(n_vol=-2), "n_vol = -2")
    for bad in (2, -1, 7):
        refused(capi, lib, call(cyclic=bad), f"cyclic = {bad}")
    for name in ("eps_s", "eps_t"):
        for bad, word in ((0.0, "0"), (-1e-3, "-0.001"), (math.inf, "inf"), (-math.inf, "-inf"), (math.nan, "nan")):
            refused(capi, lib, call(**{name: bad}), f"{name} = {word}", "positive")
    T.grid_refusals("vol", capi, lib, lambda g, count: call(g=g, n_vol=count or 1))
    # 2^50 voxels fit int64 with room to spare, but make 2^39 tiles of 4 x 8 x 64 nodes: more than the 2^31 - 1 blocks of one launch
    refused(capi, lib, call(g=grid(capi, n=(1 << 20, 1 << 20, 1 << 10))), "tiles", "one launch", str(1 << 39))


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("shape", drr_ref.GRIDS)
def test_oracle_equals_torch_autograd_in_f64(shape):
    """Pins tests/voltv_ref.total_variation to autograd through the torch expression of the same functional in f64.  The gathered g_s is
    held within 16 * 2^-53 * mass(i) (mass = the sum of the absolute values of the node's six quotients), g_t within 16 * 2^-53 (its two
    quotients are at most 1 in size), the two values within 1e-14 relative: three times what the transcription was measured at."""
    inv = ref.grid_inv(shape, drr_ref.BOUNDS)
    worst = [0.0, 0.0, 0.0]
    for n_vol in ref.N_VOLS:
        x = drr_ref.random_volume((n_vol,) + shape, seed=40 + n_vol)
        for cyclic in (False, True):
            got = ref.total_variation(x, inv, ref.EPS_S, ref.EPS_T, cyclic)
            assert got["n_pairs"] == len(ref.pairs(n_vol, cyclic)) == (0 if n_vol == 1 else n_vol - 1 + int(cyclic))
            assert got["count_space"] == x.size and got["count_time"] == got["n_pairs"] * x[0].size
            xs = torch.from_numpy(x).double().requires_grad_()
            space, _ = ref.torch_total_variation(xs, inv, ref.EPS_S, ref.EPS_T, cyclic)
            (want_gs,) = torch.autograd.grad(space, xs)
            xt = torch.from_numpy(x).double().requires_grad_()
            _, time = ref.torch_total_variation(xt, inv, ref.EPS_S, ref.EPS_T, cyclic)
            want_gt = torch.autograd.grad(time, xt)[0].numpy() if got["n_pairs"] else np.zeros_like(got["g_t"])
            if n_vol == 2 and cyclic:
                once = ref.total_variation(x, inv, ref.EPS_S, ref.EPS_T, False)["time"]
                assert once > 0 and abs(got["time"] - 2 * once) <= 1e-14 * got["time"]          # n_vol == 2 carries its pair twice
            err_s = np.abs(got["g_s"] - want_gs.numpy())
            err_t = np.abs(got["g_t"] - want_gt)
            assert (got["mass"] > 0).all()
            worst[0] = max(worst[0], float((err_s / (ref.U * got["mass"])).max()))
            worst[1] = max(worst[1], float(err_t.max() / ref.U))
            assert (err_s <= 16 * ref.U * got["mass"]).all(), (n_vol, cyclic)
            assert (err_t <= 16 * ref.U).all(), (n_vol, cyclic)
            for mine, theirs in ((got["space"], float(space.detach())), (got["time"], float(time.detach()))):
                assert abs(mine - theirs) <= 1e-14 * abs(theirs), (n_vol, cyclic, mine, theirs)
                if theirs:
                    worst[2] = max(worst[2], abs(mine - theirs) / abs(theirs))
            if n_vol == 1:
                assert got["time"] == 0.0 and not got["g_t"].any()
    print(f"oracle vs autograd f64, grid {shape}: g_s {worst[0]:.2f} of 2^-53 mass, g_t {worst[1]:.2f} of 2^-53, values {worst[2]:.2e} relative")


def test_oracle_of_a_constant_stack_is_exactly_zero():
    for shape in drr_ref.GRIDS:
        inv = ref.grid_inv(shape, drr_ref.BOUNDS)
        for n_vol in ref.N_VOLS:
            x = np.full((n_vol,) + shape, np.float32(0.7))
            for cyclic in (False, True):
                got = ref.total_variation(x, inv, ref.EPS_S, ref.EPS_T, cyclic)
                assert got["space"] == 0.0 and got["time"] == 0.0 and got["abs_space"] == 0.0 and got["abs_time"] == 0.0
                assert not got["g_s"].any() and not got["g_t"].any() and not got["mass"].any()


def test_the_shared_stack_has_a_flat_row_and_a_flat_pair():
    for shape in ref.GRIDS:
        inv = ref.grid_inv(shape, drr_ref.BOUNDS)
        x = ref.stack(3, shape, seed=1)
        assert x.dtype == np.float32
        d0 = (x[0, 1, 0, 0] - x[0, 0, 0, 0]) * inv[0]
        assert d0 == 0 and x[0, 0, 1, 0] == x[0, 0, 0, 0] == x[0, 0, 0, 1]          # m == eps_s at node (0, 0, 0) of volume 0
        assert np.array_equal(x[0, -1], x[1, -1]) and (shape == (2, 2, 2) or not np.array_equal(x[0], x[1]))          # mt == eps_t on that slab only


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_weights(capi):
    from nerfca_amd import drr, synthetic
    with pytest.raises(capi.NcaError):
        drr.total_variation(torch.zeros(5, 3, 4), bounds=drr_ref.BOUNDS)
    with pytest.raises(capi.NcaError):
        drr.total_variation(torch.zeros(2, 5, 3, 4), bounds=drr_ref.BOUNDS, cyclic=False)
    geo = synthetic.xcat_geometry(8)
    frames = [(0.0, 0.0, 0, torch.zeros(8, 8))]
    with pytest.raises(capi.NcaError):
        drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, tv_space=1e-3, tv_time=1e-3)          # a CPU image, as without the priors
    # bad weights are refused before the frames are looked at (so before anything is allocated): the message names the weight
    for kw, word in (({"tv_space": -1e-3}, "tv_space = -0.001"), ({"tv_time": -2.0}, "tv_time = -2.0"), ({"tv_space": math.nan}, "tv_space = nan"),
                     ({"tv_time": math.inf}, "tv_time = inf"), ({"tv_space": 1.0, "tv_eps": 0.0}, "tv_eps = 0.0"), ({"tv_eps": -1e-3}, "tv_eps = -0.001"),
                     ({"tv_time": 1.0, "tv_eps": math.nan}, "tv_eps = nan")):
        with pytest.raises(capi.NcaError, match=re.escape(word)):
            drr.fit_volumes(frames, geo, (5, 3, 4), 8, n_phases=1, steps=1, **kw)


def test_cli_parses_the_three_flags():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fit_volumes as fv
    finally:
        sys.path.pop(0)
    args = fv.parser().parse_args(["--frames", "m.json", "--shape", "4,4,4", "--out", "o"])
    assert args.tv_space == 0.0 and args.tv_time == 0.0 and args.tv_eps == 1e-3
    args = fv.parser().parse_args(fv.join_args(["--frames", "m.json", "--shape", "4,4,4", "--out", "o", "--tv-space", "1e-3", "--tv-time", "0.25", "--tv-eps",
                                                "1e-4", "--bounds", "-1,1,-1,1,-1,1"]))
    assert args.tv_space == 1e-3 and args.tv_time == 0.25 and args.tv_eps == 1e-4 and args.bounds == ((-1.0, 1.0),) * 3
