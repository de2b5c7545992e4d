"""The Hessian vesselness (nca_vol_hessian_eig, nca_vol_hessian_norm_max, nca_vol_vesselness, ccta.hessian_eigenvalues / vesselness):
everything that can be checked without a launch -- the C-ABI surface, every refusal of the three entry points (with device pointers that
are never read), the numpy transcription of the GPU tests (tests/vess_ref.py) held to LAPACK's eigenvalues on five families of matrices
and to the plain scipy + eigvalsh expression on small volumes, what the filter means on a tube, a ball and a slab, the refusals of the
Python layer and the command lines."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import nca_testlib as T
import vess_ref as ref
from nca_testlib import FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_hessian_eig", "nca_vol_hessian_norm_max", "nca_vol_vesselness", "nca_vess_last_error")
refused = functools.partial(T.refused, "vess")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_label_last_error(void)", "---- vess:", "int nca_vol_hessian_eig(", "int nca_vol_hessian_norm_max(", "int nca_vol_vesselness(", "nca_vess_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert list(capi.SYMBOLS)[-len(NEW):] == list(NEW)          # bound after the "label" section
    assert callable(capi.check_vess)
    from nerfca_amd import ccta
    for name in ("hessian_eigenvalues", "vesselness"):
        assert callable(getattr(ccta, name)), name


# ----------------------------------------------------------------------------- refusals
def _common_refusals(capi, lib, call, who, out_name):
    """What the three entry points share; `call` takes g, s, n_vol, scale, out (the entry point's own output) and grid keywords.  A call
    that passes every check would launch, so a valid call is never made here: the last refusal (the tile count) is the proof of the order."""
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(s=None), who, "s is NULL")
    refused(capi, lib, call(out=None), who, f"{out_name} is NULL")
    refused(capi, lib, call(out=FAKE), who, f"{out_name} is s")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("vess", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    for bad, word in ((0.0, "0"), (-1.0, "-1"), (math.inf, "inf"), (math.nan, "nan")):
        refused(capi, lib, call(scale=bad), f"scale = {word}", "finite and positive")
    # one tile per volume of 2 x 2 x 2; 4 x 8 x 65 is two tiles: 2^30 such volumes are 2^31 tiles, one more than a launch covers
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30), "tiles", "one launch", str(1 << 31))
    # the tiling sets no limit on an axis: 2^20 nodes along each in turn get as far as the tile count
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        refused(capi, lib, call(n=n, n_vol=(1 << 31) - 1), "tiles", "one launch")


def test_hessian_eig_refusals(capi, lib):
    def call(g="default", s=FAKE, n_vol=2, scale=4.0, out=FAKE + 64, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_hessian_eig(g, s, n_vol, scale, out, None)

    _common_refusals(capi, lib, call, "nca_vol_hessian_eig:", "eig")


def test_hessian_norm_max_refusals(capi, lib):
    def call(g="default", s=FAKE, n_vol=2, scale=4.0, out=FAKE + 64, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_hessian_norm_max(g, s, n_vol, scale, out, None)

    _common_refusals(capi, lib, call, "nca_vol_hessian_norm_max:", "norm_max")


def test_vesselness_refusals(capi, lib):
    def call(g="default", s=FAKE, n_vol=2, scale=4.0, alpha=0.5, beta=0.5, c=FAKE + 128, bright=1, scale_index=0, out=FAKE + 64, scale_out=None, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_vesselness(g, s, n_vol, scale, alpha, beta, c, bright, scale_index, out, scale_out, None)

    who = "nca_vol_vesselness:"
    _common_refusals(capi, lib, call, who, "out")
    refused(capi, lib, call(c=None), who, "c is NULL")
    refused(capi, lib, call(scale_out=FAKE), who, "scale_out is s")
    for name in ("alpha", "beta"):
        for bad, word in ((0.0, "0"), (-0.5, "-0.5"), (math.inf, "inf"), (math.nan, "nan")):
            refused(capi, lib, call(**{name: bad}), f"{name} = {word}", "finite and positive")
    for bad in (-1, 2, 7):
        refused(capi, lib, call(bright=bad), f"bright = {bad}", "0 nor 1")
    for bad in (-1, -9):
        refused(capi, lib, call(scale_index=bad), f"scale_index = {bad}", "negative")
    # a NULL scale_out, bright = 0 and a large scale_index are valid: they get as far as the tile count
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30, bright=0, scale_index=(1 << 31) - 1), "tiles", "one launch")


# ----------------------------------------------------------------------------- the transcription against LAPACK
GATE = 2.0 ** -46          # of |H|_F: about nine times the 1.6e-15 measured here, for the handful of roundings of each of 15 rotations


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_jacobi_against_eigvalsh(family):
    m = ref.matrices(family, 200000)
    want = np.linalg.eigvalsh(m)
    got = np.stack(ref.jacobi(*ref.six(m)), axis=-1)
    fro = np.sqrt((m * m).sum(axis=(1, 2)))
    assert np.isfinite(got).all()
    a = np.abs(got)
    assert (a[:, 0] <= a[:, 1]).all() and (a[:, 1] <= a[:, 2]).all()          # sorted by absolute value
    tie = a[:, :-1] == a[:, 1:]
    assert (got[:, :-1][tie] <= got[:, 1:][tie]).all()          # the smaller value first on a tie
    err = np.abs(np.sort(got, axis=-1) - want).max(axis=-1)
    assert (err[fro == 0] == 0).all()
    worst = float((err[fro > 0] / fro[fro > 0]).max())
    raw = ref.jacobi(*ref.six(m), sort=False)
    off = float((np.abs(np.stack(raw[3:], axis=-1)).max(axis=-1)[fro > 0] / fro[fro > 0]).max())
    three = np.sort(np.stack(ref.jacobi(*ref.six(m), sweeps=3), axis=-1), axis=-1)
    worst3 = float((np.abs(three - want).max(axis=-1)[fro > 0] / fro[fro > 0]).max())
    print(f"{family}: 5 sweeps |l - eigvalsh| <= {worst:.3e} |H|_F (gate {GATE:.3e}), off-diagonal <= {off:.3e} |H|_F; 3 sweeps {worst3:.3e}")
    assert worst <= GATE and off <= 1e-80


def test_the_sort_and_the_skipped_pair():
    # a diagonal matrix is left alone by the sweeps (every pair is skipped) and only sorted: ties by the smaller value first
    got = ref.jacobi(*[np.array([x]) for x in (2.0, 0.0, 0.0, -2.0, 0.0, 1.0)])
    assert [float(x[0]) for x in got] == [1.0, -2.0, 2.0]
    got = ref.jacobi(*[np.array([x]) for x in (-0.0, 0.0, 0.0, 0.0, 0.0, -3.0)])
    assert [math.copysign(1.0, float(x[0])) for x in got] == [-1.0, 1.0, -1.0] and float(got[2][0]) == -3.0          # -0 before +0
    # theta = 0 takes sgn = +1: t = 1, a rotation by 45 degrees
    got = ref.jacobi(*[np.array([x]) for x in (1.0, 1.0, 0.0, 1.0, 0.0, 5.0)])
    assert abs(float(got[0][0])) <= 2.0 ** -52 and abs(float(got[1][0]) - 2.0) <= 2.0 ** -51 and float(got[2][0]) == 5.0


# ----------------------------------------------------------------------------- the transcription against the plain expression
@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 8, 11)], ids=str)
def test_transcription_against_scipy_and_eigvalsh(shape):
    worst = 0.0
    for seed in range(3):
        for kind in ("random", "signed"):
            x = ref.volume(shape, kind, seed)
            for sigma in (1.0, 1.7):
                s, scale = ref.smooth(x, sigma), sigma * sigma
                for bright in (True, False):
                    for c in (0.0, 0.05):
                        got = ref.vesselness_scale(s, scale, 0.5, 0.5, c, bright)
                        want64, w = ref.plain_vesselness(s, scale, 0.5, 0.5, c, bright)
                        # a node whose l2 is within the solver's error of 0 may fall on either side of the sign test: none here
                        fro = np.sqrt((w * w).sum(axis=-1))
                        assert (np.abs(w[..., 1]) > 2.0 ** -40 * fro).all()
                        want = want64.astype(np.float32)
                        assert got.dtype == np.float32 and np.array_equal(got == 0, want == 0)
                        worst = max(worst, float(T.ulp_distance(got, want).max()))
                        assert (got > 0).any() or c
    print(f"{shape}: transcription against gaussian_filter + eigvalsh, worst {worst:.0f} f32 steps")
    assert worst <= 1


def test_norm_max_and_merge_of_the_transcription():
    x = np.stack([ref.volume((5, 6, 7), "nonfinite", 0), ref.volume((5, 6, 7), "constant", 0)])
    e = ref.eigenvalues(x, 2.0)
    assert e.shape == (2, 3, 5, 6, 7) and e.dtype == np.float32
    assert np.isnan(e[0]).any() and not np.isnan(e[0]).all() and not e[1].any()          # NaN around the two nodes only; a constant has no curvature
    assert np.array_equal(np.isnan(e[0, 0]), np.isnan(e[0, 2]))
    m = ref.norm_max(x, 2.0)
    assert m.shape == (2,) and m.dtype == np.float64 and m[1] == 0.0 and np.isfinite(m[0]) and m[0] > 0          # a NaN is passed over
    sq = e[0].astype(np.float64) ** 2
    assert m[0] == np.nanmax((sq[0] + sq[1]) + sq[2])
    a, b = np.array([0.0, 0.5, 0.5, 0.25], dtype=np.float32), np.array([0.0, 0.5, 0.75, 0.125], dtype=np.float32)
    out, idx = ref.merge([a, b])
    assert out.tolist() == [0.0, 0.5, 0.75, 0.25] and idx.tolist() == [0, 0, 1, 0] and idx.dtype == np.int32          # a tie keeps the smaller scale


# ----------------------------------------------------------------------------- what the filter means
def test_a_tube_scores_above_a_ball_and_a_slab_scores_nothing():
    h = ref.SIDE // 2
    V, idx = ref.meaning("tube")
    ball, _ = ref.meaning("ball")
    slab, _ = ref.meaning("slab")
    axis = V[h, h, :]
    print(f"tube axis {float(axis.min()):.4f} .. {float(axis.max()):.4f}, ball max {float(ball.max()):.4f}, slab max {float(slab.max()):.4f}")
    assert float(axis.min()) > float(ball.max()) > 0
    assert abs(float(axis.min()) - 0.247) < 1e-3 and abs(float(ball.max()) - 0.094) < 1e-3
    assert not slab.any()
    d, interior = ref.tube_distance()
    assert not V[(d >= 5) & interior].any() and ((d >= 5) & interior).sum() > 5000
    assert (idx[h, h, :] == 1).all()          # radius 2 answers best at sigma 2
    dark, _ = ref.meaning("negated tube")
    assert not dark[ref.tube() > 0].any()
    flipped, fidx = ref.meaning("negated tube", bright=False)          # the dark filter on the negated tube is the bright one on the tube
    assert np.array_equal(flipped.view(np.int32), V.view(np.int32)) and np.array_equal(fidx, idx)
    assert V.min() >= 0 and V.max() <= 1


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_the_cpu_and_bad_arguments(capi):
    from nerfca_amd import ccta
    a = torch.zeros(2, 4, 4, 4)
    for call in (lambda: ccta.vesselness(a), lambda: ccta.vesselness(a.numpy()), lambda: ccta.vesselness(None), lambda: ccta.hessian_eigenvalues(a, 1.0),
                 lambda: ccta.hessian_eigenvalues(None, 1.0)):
        with pytest.raises(capi.NcaError):
            call()
    with pytest.raises(capi.NcaError, match="empty"):
        ccta._vess_sigmas((), "vesselness")
    for bad in ((0.0,), (1.0, -2.0), (math.inf,), (1.0, math.nan)):
        with pytest.raises(capi.NcaError, match="sigma = .* not finite and positive"):
            ccta._vess_sigmas(bad, "vesselness")
    with pytest.raises(capi.NcaError, match="sequence"):
        ccta._vess_sigmas(2.0, "vesselness")
    assert ccta._vess_sigmas((1, 2.5), "x") == [1.0, 2.5] and ccta._vess_sigmas(np.array([3.0]), "x") == [3.0]
    for bad in (-0.1, math.inf, math.nan):
        with pytest.raises(capi.NcaError, match="c = .* non-negative"):
            ccta._vess_param(bad, "c", "vesselness", zero_ok=True)
    assert ccta._vess_param(0, "c", "x", zero_ok=True) == 0.0 and ccta._vess_param(0.5, "alpha", "x") == 0.5
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(capi.NcaError, match="alpha = .* positive"):
            ccta._vess_param(bad, "alpha", "vesselness")
    import inspect
    sig = inspect.signature(ccta.vesselness).parameters
    assert sig["sigmas"].default == (1.0, 2.0, 3.0) and sig["alpha"].default == 0.5 and sig["beta"].default == 0.5 and sig["c"].default is None
    assert sig["bright"].default is True and sig["return_scale"].default is False
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("alpha", "beta", "c", "bright", "return_scale"))
    assert "anisotropic" in ccta.__doc__ and "2-D" in ccta.__doc__


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(tmp_path, capsys):
    vt = _tool("vesselness")
    args = vt.parser().parse_args(["--vol", "v.npy", "--out", "d"])
    assert args.vol == "v.npy" and args.out == "d" and args.sigmas == [1.0, 2.0, 3.0] and args.dark is False and args.c is None
    args = vt.parser().parse_args(["--vol", "v.npy", "--sigmas", "1.5,4", "--dark", "--c", "0.25", "--out", "d"])
    assert args.sigmas == [1.5, 4.0] and args.dark is True and args.c == 0.25
    vb = _tool("vess_bench")
    args = vb.parser().parse_args(["--out", "profiles/vess_bench.txt"])
    assert args.out == "profiles/vess_bench.txt" and args.sides == "128,256" and args.volumes == "1,10" and args.sigmas == [1.0, 2.0, 3.0]
    for tool, argv in ((vt, ["--help"]), (vt, ["--out", "d"]), (vt, ["--vol", "v.npy", "--out", "d", "--sigmas", "1,x"]), (vt, ["--vol", "v.npy", "--out", "d", "--sigmas", ""]),
                       (vt, ["--vol", "v.npy", "--out", "d", "--c", "half"]), (vb, ["--help"]), (vb, ["--nonsense"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    # a volume that is not f32 [.., n0, n1, n2] is refused before a device is asked for
    bad = tmp_path / "flat.npy"
    np.save(bad, np.zeros((4, 4), dtype=np.float32))
    with pytest.raises(SystemExit) as e:
        vt.main(["--vol", str(bad), "--out", str(tmp_path / "o")])
    assert "n0, n1, n2" in str(e.value.code)
    ps = _tool("phantom_study")
    assert ps.parser().parse_args([]).vesselness is False
    args = ps.parser().parse_args(["--distances", "--cldice", "4", "--components", "--vesselness"])
    assert args.vesselness is True and args.vesselness_sigmas == "1,2,3"
    for argv in (["--vesselness"], ["--distances", "--vesselness"], ["--distances", "--cldice", "4", "--vesselness"]):          # the rows need the study they are rows of
        with pytest.raises(SystemExit) as e:
            ps.main(argv)
        assert "--components" in str(e.value.code)
    m = ps.mask_dice(torch.tensor([[[[1.0, 0.0], [1.0, 1.0]]]]), torch.tensor([[[[3.0, 3.0], [0.0, 3.0]]]]), 0.5, 1.0)
    assert abs(m - 2.0 / 3.0) < 1e-15
