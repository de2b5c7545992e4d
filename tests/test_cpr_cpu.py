"""Oblique planes and lumen rays (nca_vol_sample_planes, nca_vol_lumen, nerfca_amd.reformat): everything that can be checked without a
launch -- the C-ABI surface, every refusal of the two entry points in their stated order (with device pointers that are never read), the
refusals of the Python layer, `frames` against geometry and against its transcription, and the numpy transcription of the GPU tests
(tests/cpr_ref.py) held to the mathematics (volume slices, a slab with a closed-form radius, a tube, a narrowing tube) and to
scipy.ndimage.map_coordinates."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import scipy.ndimage
import torch

from conftest import ROOT

import cpr_ref as ref
import nca_testlib as T
import resample_ref
from nca_testlib import E_UNSUPPORTED, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_sample_planes", "nca_vol_lumen", "nca_cpr_last_error")
refused = functools.partial(T.refused, "cpr")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))
BIG = (1 << 31) - 1


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_mesh_last_error(void)", "---- path:", "nca_path_last_error(void)", "---- cpr:", "int nca_vol_sample_planes(", "int nca_vol_lumen(", "nca_cpr_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    names = list(capi.SYMBOLS)
    assert names.index("nca_path_last_error") < names.index("nca_vol_sample_planes") < names.index("nca_cpr_last_error") < names.index("nca_vol_hessian_eig")
    assert callable(capi.check_cpr)
    import nerfca_amd
    from nerfca_amd import reformat
    assert nerfca_amd.reformat is reformat and "reformat" in nerfca_amd.__all__
    for name in ("frames", "to_device", "cross_sections", "lumen_profile", "stenosis", "along", "directions", "Frames", "LumenProfile"):
        assert callable(getattr(reformat, name)), name
    assert (reformat.MAX_ANGLES, reformat.STATUS_CENTRE, reformat.STATUS_OPEN, reformat.STATUS_GRID) == (1024, ref.CENTRE, ref.OPEN, ref.GRID)
    assert "NCA_CPR_MAX_ANGLES = 1024, NCA_CPR_STATUS_CENTRE = 1, NCA_CPR_STATUS_OPEN = 2, NCA_CPR_STATUS_GRID = 4" in header
    assert "$(CSRC)/view/nca_cpr.hip" in open(os.path.join(ROOT, "Makefile")).read()


# ----------------------------------------------------------------------------- refusals of the entry points
# A call that passes every check would launch, so a valid call is never made here: the last refusal (the launch limit) is the proof of the order.
def test_sample_planes_refusals(capi, lib):
    def call(g="default", n_vol=2, src=FAKE, order=1, n_planes=3, origin=FAKE + 64, e1=FAKE + 128, e2=FAKE + 192, nu=5, nv=7, du=0.5, dv=0.25, fill=0.0, out=FAKE + 256, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_sample_planes(g, n_vol, src, order, n_planes, origin, e1, e2, nu, nv, du, dv, fill, out, None)

    who = "nca_vol_sample_planes:"
    limit = dict(n_planes=BIG, nu=17, nv=17)          # four tiles per plane: 2^33 - 4 workgroups
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    for name in ("src", "origin", "e1", "e2", "out"):
        refused(capi, lib, call(**{name: None}), who, f"{name} is NULL")
    refused(capi, lib, call(src=None, out=None), "src is NULL")          # in the order of the arguments
    refused(capi, lib, call(e2=None, n_vol=0), "e2 is NULL")             # pointers before n_vol
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("cpr", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    refused(capi, lib, call(n=(1, 5, 6), order=2), "n[0] = 1")           # the grid before order
    for bad in (2, 4, 5, -1):
        refused(capi, lib, call(order=bad), f"order = {bad}", "0, 1 or 3", code=E_UNSUPPORTED)
    refused(capi, lib, call(order=2, n_planes=0), "order = 2", code=E_UNSUPPORTED)          # order before the counts
    for name in ("n_planes", "nu", "nv"):
        for bad in (0, -4):
            refused(capi, lib, call(**{name: bad}), f"{name} = {bad}", "positive")
    refused(capi, lib, call(n_planes=0, nu=0), "n_planes = 0")
    refused(capi, lib, call(nu=0, nv=0), "nu = 0")
    refused(capi, lib, call(nv=0, du=0.0), "nv = 0")                     # counts before the pixel sizes
    for name in ("du", "dv"):
        for bad, word, why in ((0.0, "0", "positive"), (-0.5, "-0.5", "positive"), (math.inf, "inf", "finite"), (-math.inf, "-inf", "finite"), (math.nan, "nan", "finite")):
            refused(capi, lib, call(**{name: bad}), f"{name} = {word}", why)
    refused(capi, lib, call(du=0.0, dv=0.0), "du = 0")
    refused(capi, lib, call(dv=math.nan, **limit), "dv = nan")           # the pixel sizes before the launch limits
    refused(capi, lib, call(**limit), who, "tiles", "one launch", f"4 x {BIG}")
    refused(capi, lib, call(fill=math.nan, order=0, **limit), "one launch")          # any fill and every order get as far
    refused(capi, lib, call(order=3, **limit), "one launch")
    refused(capi, lib, call(n_vol=BIG, n_planes=BIG, nu=BIG, nv=1), "one launch")    # 2^27 tiles per plane
    refused(capi, lib, call(n_vol=BIG, n_planes=1, nu=(1 << 15) + 16, nv=1 << 15), "overflow int64", str(BIG))          # 2^22 tiles would do; more than 2^30 f32 pixels x (2^31 - 1) volumes do not
    for a in range(3):          # no limit on an axis
        n = [2, 2, 2]
        n[a] = 1 << 20
        refused(capi, lib, call(n=n, **limit), "one launch")


def test_lumen_refusals(capi, lib):
    def call(g="default", n_vol=2, vol=FAKE, n_planes=3, origin=FAKE + 64, e1=FAKE + 128, e2=FAKE + 192, n_ang=64, dirs=FAKE + 256, sin_step=0.1, level=0.5, dr=0.25,
             n_steps=10, radius=FAKE + 320, stats=FAKE + 384, status=FAKE + 448, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_lumen(g, n_vol, vol, n_planes, origin, e1, e2, n_ang, dirs, sin_step, level, dr, n_steps, radius, stats, status, None)

    who = "nca_vol_lumen:"
    limit = dict(n_vol=1 << 16, n_planes=1 << 15)          # 2^31 workgroups
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    for name in ("vol", "origin", "e1", "e2", "dirs", "radius", "stats", "status"):
        refused(capi, lib, call(**{name: None}), who, f"{name} is NULL")
    refused(capi, lib, call(dirs=None, status=None), "dirs is NULL")
    refused(capi, lib, call(status=None, n_vol=0), "status is NULL")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("cpr", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    refused(capi, lib, call(reserved=1, n_planes=0), "reserved = 1")
    for bad in (0, -4):
        refused(capi, lib, call(n_planes=bad), f"n_planes = {bad}", "positive")
    refused(capi, lib, call(n_planes=0, n_ang=5), "n_planes = 0")
    for bad in (5, 63, 2, 0, -2, 3):
        refused(capi, lib, call(n_ang=bad), f"n_ang = {bad}", "even", "at least 4")
    for bad in (1026, 1025, BIG):
        refused(capi, lib, call(n_ang=bad), f"n_ang = {bad}", "NCA_CPR_MAX_ANGLES = 1024", code=E_UNSUPPORTED)
    refused(capi, lib, call(n_ang=6, n_steps=0), "n_steps = 0", "positive")
    refused(capi, lib, call(n_ang=7, n_steps=0), "n_ang = 7")
    refused(capi, lib, call(n_steps=-1, sin_step=math.nan), "n_steps = -1")
    for bad, word in ((math.inf, "inf"), (math.nan, "nan")):
        refused(capi, lib, call(sin_step=bad), f"sin_step = {word}", "finite")
    refused(capi, lib, call(sin_step=math.inf, level=math.nan), "sin_step = inf")
    refused(capi, lib, call(level=math.nan), "level = nan", "not a number")
    refused(capi, lib, call(level=math.nan, dr=0.0), "level = nan")
    for bad, word, why in ((0.0, "0", "positive"), (-0.5, "-0.5", "positive"), (math.inf, "inf", "finite"), (math.nan, "nan", "finite")):
        refused(capi, lib, call(dr=bad), f"dr = {word}", why)
    refused(capi, lib, call(dr=-1.0, **limit), "dr = -1")
    refused(capi, lib, call(**limit), who, "workgroups", "one launch", str(1 << 31))
    # an infinite level, the smallest and the largest fan and one step are valid: they get as far as the launch limit
    refused(capi, lib, call(level=-math.inf, n_ang=4, n_steps=1, **limit), "one launch")
    refused(capi, lib, call(level=math.inf, n_ang=1024, n_steps=BIG, sin_step=-0.0, **limit), "one launch")


def test_python_layer_refusals(capi):
    from nerfca_amd import reformat as R
    cpu = torch.zeros((3, 4, 5))
    fr = R.frames([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])

    def no(fn, *words):
        with pytest.raises(capi.NcaError) as e:
            fn()
        for w in words:
            assert w in str(e.value), str(e.value)

    no(lambda: R.frames([[0.0, 0.0, 0.0]]), "1 distinct points")
    no(lambda: R.frames([[1.0, 2.0, 3.0]] * 4), "1 distinct points")
    no(lambda: R.frames(np.zeros((4, 2))), "[N, 3]")
    no(lambda: R.frames([[0.0, 0.0, 0.0], [1.0, math.nan, 0.0]]), "not finite")
    no(lambda: R.frames(fr.origin, smooth=-1), "smooth = -1")
    no(lambda: R.frames(fr.origin, smooth=1.5), "smooth = 1.5")
    no(lambda: R.frames(fr.origin, step=0.0), "step = 0.0")
    no(lambda: R.frames(fr.origin, step=math.inf), "step = inf")
    no(lambda: R.frames(fr.origin, step=3.0), "fewer than two planes")
    no(lambda: R.frames(fr.origin, up=(2.0, 0.0, 0.0)), "parallel")
    no(lambda: R.frames(fr.origin, up=(1.0, 0.0)), "three finite numbers")
    no(lambda: R.frames([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], step=1.0), "zero tangent")
    for order in (2, -1, 1.5, True):
        no(lambda: R.cross_sections(cpu, None, fr, size=5, spacing=1.0, order=order), f"order = {order!r}")
    no(lambda: R.cross_sections(cpu, None, fr, size=0, spacing=1.0), "size = 0")
    no(lambda: R.cross_sections(cpu, None, fr, size=(3, 4, 5), spacing=1.0), "size")
    no(lambda: R.cross_sections(cpu, None, fr, size=5, spacing=-1.0), "spacing = -1.0")
    no(lambda: R.cross_sections(cpu, None, fr, size=5, spacing=(1.0, math.nan)), "spacing = nan")
    no(lambda: R.cross_sections(cpu, None, fr, size=5, spacing=1.0, fill="x"), "fill")
    no(lambda: R.cross_sections(cpu, None, (fr.origin, fr.e1, fr.e2), size=5, spacing=1.0), "not a Frames")
    no(lambda: R.cross_sections(cpu, None, fr, size=5, spacing=1.0), "GPU")
    no(lambda: R.cross_sections(np.zeros((3, 4, 5)), None, fr, size=5, spacing=1.0), "not a tensor")
    for bad in (5, 2, 0, 1026, 6.0):
        no(lambda: R.lumen_profile(cpu, None, fr, level=0.5, r_max=2.0, n_angles=bad), f"n_angles = {bad}")
    no(lambda: R.lumen_profile(cpu, None, fr, level=math.nan, r_max=2.0), "level = nan")
    no(lambda: R.lumen_profile(cpu, None, fr, level="x", r_max=2.0), "level")
    no(lambda: R.lumen_profile(cpu, None, fr, level=0.5, r_max=0.0), "r_max = 0.0")
    no(lambda: R.lumen_profile(cpu, None, fr, level=0.5, r_max=2.0, dr=-0.1), "dr = -0.1")
    no(lambda: R.lumen_profile(cpu, None, None, level=0.5, r_max=2.0), "not a Frames")
    no(lambda: R.lumen_profile(cpu, None, fr, level=0.5, r_max=2.0), "GPU")
    no(lambda: R.stenosis(None), "not a LumenProfile")
    prof = R.LumenProfile(*(torch.zeros(1) for _ in range(7)))
    no(lambda: R.stenosis(prof, reference="mean"), "median")
    no(lambda: R.stenosis(prof, reference=0.0), "reference = 0.0")
    no(lambda: R.along(cpu, None, None, level=0.5, r_max=2.0, size=5, spacing=1.0), "not a Centreline")
    no(lambda: R.to_device(None, "cpu"), "not a Frames")


# ----------------------------------------------------------------------------- frames
def _helix(radius=2.0, pitch=0.5, turns=2.0, count=400):
    t = np.linspace(0.0, 2.0 * math.pi * turns, count)
    return np.stack([radius * np.cos(t), radius * np.sin(t), pitch * t], axis=1), t[1] - t[0]


def _orthonormal_error(fr):
    dots = [(getattr(fr, a) * getattr(fr, b)).sum(1) - (1.0 if a == b else 0.0) for a, b in
            (("tangent", "tangent"), ("e1", "e1"), ("e2", "e2"), ("tangent", "e1"), ("tangent", "e2"), ("e1", "e2"))]
    right_handed = np.abs(np.cross(fr.tangent, fr.e1) - fr.e2).max()
    return max(float(np.abs(d).max()) for d in dots), float(right_handed)


def test_frames_on_a_helix():
    from nerfca_amd import reformat as R
    radius, pitch = 2.0, 0.5
    pts, dt = _helix(radius, pitch)
    for kw in (dict(step=0.05), dict(), dict(step=0.3, smooth=2), dict(step=0.05, up=(0.3, -0.2, 1.0))):
        fr = R.frames(pts, **kw)
        err, hand = _orthonormal_error(fr)
        assert err <= 1e-12 and hand <= 1e-12, (kw, err, hand)
        for got, want in zip(fr, ref.frames(pts, **kw)):          # the transcription, point by point: the same bits
            assert np.array_equal(got, want), kw
    # The arclength.  The input polyline has N - 1 chords of the helix, each sqrt(4 R^2 sin^2(dt / 2) + (c dt)^2) long: L_poly in closed form.
    # The planes lie `step` apart along that polyline, so the last one is less than a step short of its end; and a chord of a curve of
    # length l whose tangent turns by Theta < pi in all is at least l cos(Theta / 2) long.  Between two planes the polyline turns at no more
    # than step / chord + 1 vertices by kappa_h = the angle between consecutive chords each, which is at most kappa * arc (kappa = R / (R^2 + c^2)).
    step = 0.05
    fr = R.frames(pts, step=step)
    chord = math.sqrt(4.0 * radius ** 2 * math.sin(dt / 2) ** 2 + (pitch * dt) ** 2)
    arc = dt * math.sqrt(radius ** 2 + pitch ** 2)
    l_poly, l_true = (len(pts) - 1) * chord, (len(pts) - 1) * arc
    kappa = radius / (radius ** 2 + pitch ** 2)
    assert l_true * (1.0 - (kappa * arc) ** 2 / 24.0) <= l_poly <= l_true          # the chord error of the input, from its own step
    assert np.allclose(np.diff(fr.s), step, rtol=0, atol=1e-12) and fr.s[0] == 0.0
    assert l_poly - step < fr.s[-1] <= l_poly + 1e-9
    resampled = float(np.sqrt(((fr.origin[1:] - fr.origin[:-1]) ** 2).sum(1)).sum())
    theta = (step / chord + 1.0) * kappa * arc
    assert fr.s[-1] * math.cos(theta / 2.0) <= resampled <= fr.s[-1] * (1.0 + 1e-14)
    assert abs(resampled - l_true) <= l_true * ((kappa * arc) ** 2 / 24.0 + (1.0 - math.cos(theta / 2.0))) + step


def test_frames_on_a_line_and_a_circle():
    from nerfca_amd import reformat as R
    d = np.array([1.0, 2.0, -0.5])
    line = np.array([0.3, -1.0, 2.0]) + np.linspace(0.0, 3.0, 17)[:, None] * d
    fr = R.frames(line, step=0.11)
    err, hand = _orthonormal_error(fr)
    assert err <= 1e-12 and hand <= 1e-12
    for a in (fr.tangent, fr.e1, fr.e2):
        assert np.abs(a - a[0]).max() <= 1e-12          # constant
    assert np.abs(fr.tangent[0] - d / np.linalg.norm(d)).max() <= 1e-15
    start = np.array([0.0, 0.0, 1.0]) - fr.tangent[0][2] * fr.tangent[0]          # from z, the axis least aligned with the tangent
    assert np.abs(fr.e1[0] - start / np.linalg.norm(start)).max() <= 1e-15
    assert len(R.frames(line).s) == 17                     # the default step keeps a uniform polyline's points
    assert np.abs(R.frames(line).origin - line).max() <= 1e-14
    t = np.linspace(0.0, 1.5 * math.pi, 200)
    circle = np.stack([3.0 * np.cos(t), 3.0 * np.sin(t), np.zeros_like(t)], axis=1)
    fr = R.frames(circle, step=0.1, up=(0.0, 0.0, 1.0))
    assert np.abs(fr.e1 - np.array([0.0, 0.0, 1.0])).max() <= 1e-12
    assert np.abs(fr.e2[:, 2]).max() <= 1e-12 and np.abs((fr.e2[:, :2] * fr.origin[:, :2]).sum(1) / 3.0).min() > 0.99          # e2 = t x z: the radial direction
    doubled = np.repeat(circle, 2, axis=0)                 # a repeated point is dropped
    assert all(np.array_equal(a, b) for a, b in zip(R.frames(doubled, step=0.1), R.frames(circle, step=0.1)))
    f32 = R.frames(torch.tensor(circle, dtype=torch.float32), step=0.1)          # a tensor, as Centreline.points holds them
    assert f32.origin.dtype == np.float64 and np.abs(f32.origin - R.frames(circle, step=0.1).origin[:len(f32.s)]).max() < 1e-5


# ----------------------------------------------------------------------------- the transcription against the volume's own slices and scipy
@pytest.mark.parametrize("inv", ref.INVS)
def test_planes_on_nodes_return_the_slices(inv):
    shape = ref.SHAPES[1]
    vol = ref.volumes(shape, 2, seed=1)
    for axis in range(3):
        slices = list(range(shape[axis]))          # the last plane of the axis included
        origin, e1, e2, nu, nv, du, dv = ref.axis_planes(shape, ref.LO, inv, axis, slices)
        want = np.moveaxis(vol, 1 + axis, 1)
        for order in (0, 1):
            got = ref.sample_planes(vol, ref.LO, inv, order, origin, e1, e2, nu, nv, du, dv, np.nan)
            assert T.same_bits(got, np.ascontiguousarray(want)), (axis, order)
        got = ref.sample_planes(vol, ref.LO, inv, 3, origin, e1, e2, nu, nv, du, dv, np.nan)
        assert T.ulp_distance(got, np.ascontiguousarray(want)).max() <= 1.0, axis
    # NaN and infinite nodes at order 0, and a fill with a payload outside the grid
    special = ref.volumes(shape, 1, seed=2, special=True)
    origin, e1, e2, nu, nv, du, dv = ref.axis_planes(shape, ref.LO, inv, 0, [0, shape[0] - 1, shape[0]])
    fill = np.array([0x7FC12345], dtype=np.int32).view(np.float32)[0]
    got = ref.sample_planes(special, ref.LO, inv, 0, origin, e1, e2, nu, nv, du, dv, fill)
    assert T.same_bits(got[:, :2], special[:, [0, shape[0] - 1]]) and (got[:, 2].view(np.int32) == 0x7FC12345).all()


def test_orders_1_and_3_against_map_coordinates():
    """Both sides are f64 evaluations rounded once to f32: they may differ by one f32 step at the magnitude of the largest |vol|, no more.
    The share of differing pixels is printed (DESIGN.md records it), not gated."""
    differing = {1: [0, 0], 3: [0, 0]}
    for shape in ref.SHAPES:
        for inv in ref.INVS:
            vol = ref.volumes(shape, 1, seed=3)
            origin, e1, e2 = ref.oblique_planes(shape, ref.LO, inv, 6, seed=1, spread=0.6)
            nu, nv, du, dv = 9, 9, 0.3, 0.3
            x, inside = ref.world_to_grid(ref.plane_points(origin, e1, e2, nu, nv, du, dv), ref.LO, inv, shape)
            assert inside.mean() > 0.9
            step = float(np.spacing(np.float32(np.abs(vol).max())))
            for order in (1, 3):
                got = ref.sample_planes(vol, ref.LO, inv, order, origin, e1, e2, nu, nv, du, dv, 0.0)[0]
                src = vol[0].astype(np.float64) if order == 1 else resample_ref.spline_filter(vol[0])
                want = scipy.ndimage.map_coordinates(src, x[inside].T, order=order, prefilter=False, mode="mirror").astype(np.float32)
                diff = np.abs(got[inside].astype(np.float64) - want.astype(np.float64))
                assert diff.max() <= step, (shape, inv, order, diff.max(), step)
                assert (got[~inside] == 0.0).all()
                differing[order][0] += int((diff > 0).sum())
                differing[order][1] += diff.size
    for order, (n, total) in differing.items():
        print(f"order {order}: {n} of {total} pixels differ from map_coordinates")


# ----------------------------------------------------------------------------- the lumen of the transcription
SLAB_SHAPE, SLAB_INV, SLAB_W = (5, 41, 41), (1.0, 2.0, 0.5), 3.25          # spacings 1, 0.5, 2: the box is 4 x 20 x 80 from ref.LO


def _slab():
    """w - |x1 - c| with the kink on node plane 20 of axis 1: linear between node planes, so the trilinear value is the field itself"""
    x1 = ref.LO[1] + np.arange(SLAB_SHAPE[1]) / SLAB_INV[1]
    return np.ascontiguousarray(np.broadcast_to((SLAB_W - np.abs(x1 - x1[20]))[None, :, None], SLAB_SHAPE)).astype(np.float32)[None]


def _plane_at(node, e1=(0.0, 1.0, 0.0), e2=(0.0, 0.0, 1.0)):
    return np.array([ref.node_to_world(node, ref.LO, SLAB_INV)]), np.array([e1]), np.array([e2])


def test_lumen_of_a_slab():
    n_ang, dr, n_steps = 64, 0.25, 32          # r_max = 8: the fan stays inside the grid around node (2, 20, 20)
    radius, stats, status, r = ref.lumen(_slab(), ref.LO, SLAB_INV, *_plane_at((2, 20, 20)), n_ang, 0.0, dr, n_steps)
    cos = np.abs(ref.directions(n_ang)[:, 0])
    closed = SLAB_W / np.maximum(cos, 1e-300)
    inside = closed > 8.0                      # the rays that stay inside the slab up to r_max
    assert 0 < inside.sum() < n_ang and status.tolist() == [[ref.OPEN]]
    _, bits = ref.rays(_slab()[0], ref.LO, SLAB_INV, *_plane_at((2, 20, 20)), ref.directions(n_ang), 0.0, dr, n_steps)
    assert np.array_equal(bits[0] == ref.OPEN, inside) and (bits[0][~inside] == 0).all()          # status 2 exactly on those rays
    assert (r[0, 0][inside] == 8.0).all()
    assert np.abs(r[0, 0][~inside] / closed[~inside] - 1.0).max() <= 1e-14                          # r = w / |cos|, to f64 rounding
    assert np.array_equal(radius, r.astype(np.float32))
    assert stats[0, 0, 1] == 2.0 * SLAB_W and stats[0, 0, 2] == 16.0 and stats[0, 0, 3] == pytest.approx(np.minimum(closed, 8.0).mean(), rel=1e-14)
    # a plane near the face of axis 2 (node 39 of 0 .. 40, spacing 2): the rays towards it leave the grid one sample before they would pass it
    radius, stats, status, r = ref.lumen(_slab(), ref.LO, SLAB_INV, *_plane_at((2, 20, 39)), n_ang, 0.0, dr, n_steps)
    _, bits = ref.rays(_slab()[0], ref.LO, SLAB_INV, *_plane_at((2, 20, 39)), ref.directions(n_ang), 0.0, dr, n_steps)
    assert status[0, 0] & ref.GRID and (bits[0] == ref.GRID).any()
    left = bits[0] == ref.GRID
    sin = ref.directions(n_ang)[:, 1]
    assert (sin[left] > 0).all() and np.array_equal(r[0, 0][left], np.floor(2.0 / sin[left] / dr) * dr)          # the last sample inside: 2 world units to the face
    # a centre outside the lumen: every ray has r = 0 and bit 1
    radius, stats, status, r = ref.lumen(_slab(), ref.LO, SLAB_INV, *_plane_at((2, 29, 20)), n_ang, 0.0, dr, n_steps)
    assert status.tolist() == [[ref.CENTRE]] and not r.any() and not stats.any()
    # a centre outside the grid: r = 0 and bit 4
    radius, stats, status, r = ref.lumen(_slab(), ref.LO, SLAB_INV, *_plane_at((2, 20, 41)), n_ang, 0.0, dr, n_steps)
    assert status.tolist() == [[ref.GRID]] and not r.any()


def test_polygon_area_of_a_constant_radius():
    for n_ang in (4, 64, 258, 1024):
        for r in (3.0, 0.625):          # short mantissas: every partial sum is exact, so the sum is n r^2 and one product rounds
            s = ref.ray_stats(np.full(n_ang, r), ref.sin_step(n_ang))
            assert s[0] == (0.5 * ref.sin_step(n_ang)) * (n_ang * r * r) and s[1] == s[2] == 2 * r and s[3] == r
            assert s[0] == pytest.approx((n_ang / 2) * math.sin(2 * math.pi / n_ang) * r * r, rel=4e-16)
    assert ref.ray_stats(np.array([1.0, 2.0, 3.0, 4.0]), 1.0).tolist() == [0.5 * (2 + 6 + 12 + 4), 4.0, 6.0, 2.5]


# |d_eq - 2 rho| of a straight tube of radius rho = 3 sampled as rho - distance on grids of spacing 1 and 0.5, 64 rays, dr = spacing / 2,
# measured with the transcription (the largest over nine planes between nodes).  Two parts: the polygon through 64 ray ends has
# (32 / pi) sin(pi / 32) = 0.99839 of the disc's area, 0.0048 of the diameter at any spacing; the rest is the trilinear interpolation of a
# cone, which lies above the cone's distance (the distance is convex), so the level is crossed early and the lumen reads narrow.
TUBE_D_EQ_ERROR = {1.0: 0.061562626137863674, 0.5: 0.019185382166117648}


def test_tube_diameter_error_shrinks_with_the_spacing():
    rho, errs = 3.0, {}
    for h in (1.0, 0.5):
        n = int(16 / h) + 1
        lo, inv = (0.0, 0.0, 0.0), (1 / h,) * 3
        vol = ref.tube_field((n, n, n), lo, inv, (8.0, 8.0, -5.0), (8.0, 8.0, 21.0), rho)[None]
        k = 9
        origin = np.stack([np.full(k, 8.0), np.full(k, 8.0), 4.0 + np.arange(k) * 0.37], axis=1)
        e1, e2 = np.tile([[1.0, 0.0, 0.0]], (k, 1)), np.tile([[0.0, 1.0, 0.0]], (k, 1))
        _, stats, status, _ = ref.lumen(vol, lo, inv, origin, e1, e2, 64, 0.0, 0.5 * h, int(6 / (0.5 * h)))
        assert not status.any()
        d_eq = 2.0 * np.sqrt(stats[0, :, 0] / math.pi)
        assert (d_eq < 2 * rho).all()
        errs[h] = float(np.abs(d_eq - 2 * rho).max())
        print(f"tube, spacing {h}: max |d_eq - 2 rho| = {errs[h]!r}")
        assert errs[h] == pytest.approx(TUBE_D_EQ_ERROR[h], rel=1e-9)
    assert errs[0.5] < 0.5 * errs[1.0]


def test_stenosis_of_a_narrowing_tube():
    """Radius 4 falling linearly to 2 over z in [10, 16], 2 up to z = 22, back to 4 at z = 28; planes every unit from z = 1"""
    from nerfca_amd import reformat as R
    shape, lo, inv = (17, 17, 81), (0.0, 0.0, 0.0), (1.0, 1.0, 2.0)
    vol = ref.narrowing_tube(shape, lo, inv, (8.0, 8.0), 4.0, (10.0, 16.0))
    k = 39
    z = 1.0 + np.arange(k)
    origin = np.stack([np.full(k, 8.0), np.full(k, 8.0), z], axis=1)
    e1, e2 = np.tile([[1.0, 0.0, 0.0]], (k, 1)), np.tile([[0.0, 1.0, 0.0]], (k, 1))
    wide = np.stack([vol, ref.tube_field(shape, lo, inv, (8.0, 8.0, -9.0), (8.0, 8.0, 50.0), 4.0)])          # the second volume: no narrowing
    radius, stats, status, _ = ref.lumen(wide, lo, inv, origin, e1, e2, 64, 0.0, 0.25, 28)
    assert not status.any()
    d_eq = 2.0 * np.sqrt(stats[..., 0] / math.pi)
    prof = R.LumenProfile(torch.tensor(radius), torch.tensor(stats[..., 0]), torch.tensor(stats[..., 1]), torch.tensor(stats[..., 2]), torch.tensor(d_eq),
                          torch.tensor(status), torch.tensor(z - 1.0))
    narrow, straight = R.stenosis(prof)
    assert narrow["mld_s"] == 15.0 and z[15] == 16.0          # the first plane of the narrowest stretch
    assert narrow["planes"] == k and narrow["excluded"] == 0
    # pinned from the transcription: 3.9096 for the true 4 (the tube test's error at this spacing), the reference 7.9509 for the true 8
    assert narrow["mld"] == pytest.approx(3.909636803297169, rel=1e-12) and narrow["reference"] == pytest.approx(7.950859640539067, rel=1e-12)
    assert narrow["diameter_stenosis"] == pytest.approx(100.0 * (1.0 - 3.909636803297169 / 7.950859640539067), rel=1e-12)
    assert narrow["diameter_stenosis"] == pytest.approx(50.0, abs=1.0)
    assert narrow["area_stenosis"] == pytest.approx(100.0 * (1.0 - (3.909636803297169 / 7.950859640539067) ** 2), rel=1e-12)
    assert abs(straight["diameter_stenosis"]) < 1e-9 and straight["mld"] == pytest.approx(7.950859640539067, rel=1e-9)
    # a reference given by the caller, and planes with a status bit left out and counted
    given = R.stenosis(prof, reference=8.0)[0]
    assert given["reference"] == 8.0 and given["diameter_stenosis"] == pytest.approx(100.0 * (1.0 - 3.909636803297169 / 8.0), rel=1e-12)
    flagged = status.copy()
    flagged[0, 15:22] = ref.OPEN
    some = R.stenosis(prof._replace(status=torch.tensor(flagged)))[0]
    assert some["excluded"] == 7 and some["planes"] == k - 7 and some["mld_s"] in (14.0, 22.0) and some["mld"] > 4.5
    none = R.stenosis(prof._replace(status=torch.full_like(prof.status, ref.GRID)))[0]
    assert none["planes"] == 0 and none["mld"] is None and none["diameter_stenosis"] is None


# ----------------------------------------------------------------------------- the command lines
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_command_lines(tmp_path, capsys):
    rf, cb, ps = _tool("reformat"), _tool("cpr_bench"), _tool("phantom_study")
    args = rf.parser().parse_args(["--vol", "v.npy", "--threshold", "0.3", "--level", "0.25", "--bounds=-1,1,-1,1,-1,1", "--root", "0.5,-0.25,0", "--vtk", "--out", "d"])
    assert args.bounds == ((-1.0, 1.0),) * 3 and args.root == (0.5, -0.25, 0.0) and args.vtk and (args.size, args.order, args.spacing) == (33, 3, None)
    for argv in (["--help"], ["--vol", "v.npy", "--threshold", "0.3", "--out", "d"], ["--vol", "v.npy", "--threshold", "0.3", "--level", "0.2", "--out", "d", "--order", "2"]):
        with pytest.raises(SystemExit) as e:
            rf.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    bad = tmp_path / "stack.npy"
    np.save(bad, np.zeros((2, 4, 4, 4), dtype=np.float32))          # ONE volume: refused before a device is asked for
    with pytest.raises(SystemExit) as e:
        rf.main(["--vol", str(bad), "--threshold", "0.5", "--level", "0.5", "--out", str(tmp_path / "o")])
    assert "n0, n1, n2" in str(e.value.code)
    args = cb.parser().parse_args(["--out", "profiles/cpr_bench.txt"])
    assert (args.sides, args.volumes, args.planes, args.size, args.passes) == ("128,256", "1,10", 512, 65, 3)
    assert ps.parser().parse_args([]).lumen is False and ps.parser().parse_args(["--lumen"]).lumen is True
