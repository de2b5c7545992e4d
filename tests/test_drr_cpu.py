"""Volume projection (drr.project_rays / project_sequence / volume_teacher, csrc/view/nca_drr.hip): everything that can be checked
without a launch -- the C-ABI surface, every refusal (with pointers that are never read), the grid descriptor, the command line of
tools/project_volumes.py, and the f64 oracle of the GPU tests (tests/drr_ref.py) against torch's grid_sample."""
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

import drr_ref as ref
import nca_testlib as T
from nca_testlib import FAKE, capi, grid, lib  # noqa: F401

NEW = ("nca_drr_project", "nca_drr_set_split", "nca_drr_get_split", "nca_drr_last_error")
refused = functools.partial(T.refused, "drr")


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    import nerfca_amd
    assert nerfca_amd.drr.project_rays and nerfca_amd.drr.project_sequence and nerfca_amd.drr.project_view and nerfca_amd.drr.volume_teacher
    assert header.index("nca_view_last_error(void)") < header.index("typedef struct NcaGrid")          # the new section follows the view section


def test_grid_descriptor_size_and_field_order_match_the_header(capi):
    header = open(os.path.join(ROOT, "include", "nerfca_hip.h")).read()
    body = re.search(r"typedef struct NcaGrid \{(.*?)\} NcaGrid;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    widths = {"double": 8, "int32_t": 4}
    size, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, name = decl.split(None, 1)
        assert size % widths[ctype] == 0, decl          # naturally aligned where it stands: no implicit padding
        m = re.search(r"\[(\d+)\]", name)
        size += widths[ctype] * (int(m.group(1)) if m else 1)
        names.append(re.sub(r"\[.*", "", name).strip())
    assert size == 64 == C.sizeof(capi.NcaGrid)
    assert names == ["lo", "inv", "n", "reserved"] == [n for n, _ in capi.NcaGrid._fields_]
    assert [getattr(capi.NcaGrid, n).offset for n in names] == [0, 24, 48, 60]


def test_project_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=1, R=8, S=4, o=FAKE, d=FAKE, z=FAKE, dists=FAKE, pix=FAKE):
        g = grid(capi) if g == "default" else g
        return lib.nca_drr_project(C.byref(g) if g is not None else None, vol, n_vol, R, S, o, d, z, dists, 2.0, pix, None)

    refused(capi, lib, call(g=None), "nca_drr_project", "grid", "NULL")
    for name in ("vol", "o", "d", "z", "dists", "pix"):
        refused(capi, lib, call(**{name: None}), {"o": "origins", "d": "dirs"}.get(name, name) + " is NULL")
    refused(capi, lib, call(n_vol=0), "n_vol = 0")
    refused(capi, lib, call(n_vol=-2), "n_vol = -2")
    refused(capi, lib, call(R=0), "R = 0")
    refused(capi, lib, call(R=-7), "R = -7")
    refused(capi, lib, call(S=0), "S = 0")
    refused(capi, lib, call(S=-1), "S = -1")
    T.grid_refusals("drr", capi, lib, lambda g, count: call(g=g, n_vol=count or 1))
    refused(capi, lib, call(R=1 << 62), "R = " + str(1 << 62))


def test_split_switch(capi, lib):
    before = lib.nca_drr_get_split()
    assert before in (1, 4)
    try:
        for k in (4, 1):
            assert lib.nca_drr_set_split(k) == 0 and lib.nca_drr_get_split() == k
        for bad in (0, 2, 3, 8, -1):
            refused(capi, lib, lib.nca_drr_set_split(bad), f"split = {bad}")
            assert lib.nca_drr_get_split() == 1          # a refused value changes nothing
    finally:
        lib.nca_drr_set_split(before)


def test_grid_desc_reproduces_lo_and_inv_in_f64(capi):
    from nerfca_amd import drr
    for shape in ref.GRIDS + [(128, 64, 256)]:
        for bounds in (ref.BOUNDS, ref.SMALL_BOX, ((-1, 1),) * 3, ((0.1, 0.7), (-3.0, 1e-3), (5, 9.5))):
            g = drr.grid_desc(shape, bounds)
            assert list(g.n) == list(shape) and g.reserved == 0
            assert list(g.lo) == [float(b[0]) for b in bounds]
            assert list(g.inv) == [(n - 1) / (float(b[1]) - float(b[0])) for n, b in zip(shape, bounds)]
    assert list(drr.grid_desc(torch.Size((5, 3, 4)), ref.BOUNDS).n) == [5, 3, 4]
    for shape, bounds in (((5, 3), ref.BOUNDS), ((5, 3, 1), ref.BOUNDS), ((5, 3, 4), ((0, 1), (0, 1))), ((5, 3, 4), ((0, 1), (1, 1), (0, 1))),
                          ((5, 3, 4), ((0, 1), (2, 1), (0, 1))), ((5, 3, 4), ((0, math.inf), (0, 1), (0, 1)))):
        with pytest.raises(capi.NcaError):
            drr.grid_desc(shape, bounds)


def test_projection_refuses_the_cpu(capi):
    from nerfca_amd import drr, synthetic
    vol = torch.zeros(5, 3, 4)
    o, d, z = torch.zeros(6, 3, dtype=torch.float64), torch.ones(6, 3, dtype=torch.float64), torch.linspace(0, 1, 8)
    with pytest.raises(capi.NcaError):
        drr.project_rays(vol, o, d, z, i0=2.0, bounds=ref.BOUNDS)
    with pytest.raises(capi.NcaError):
        drr.project_sequence(vol, None, synthetic.xcat_geometry(8), [(0, 0)], 8)
    with pytest.raises(capi.NcaError):
        drr.project_sequence(vol, vol[None].repeat(2, 1, 1, 1), synthetic.xcat_geometry(8), [(0, 0)], 8)
    with pytest.raises(capi.NcaError):
        drr.project_view(vol, vol, synthetic.xcat_geometry(8), 0, 0, 8)
    with pytest.raises(capi.NcaError):
        drr.volume_teacher(ref.BOUNDS)(vol, vol[None], o, d, torch.zeros(6, dtype=torch.int32), torch.full((6,), 2.0), z, z.double())


def test_cli_parses_its_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import project_volumes as pv
        import render_views as rv
    finally:
        sys.path.pop(0)
    assert pv.parse_views is rv.parse_views and pv.parse_phases is rv.parse_phases and pv.join_views is rv.join_views          # imported, not copied
    assert pv.load_geometry is rv.load_geometry
    assert pv.parse_bounds("-1,1, -0.5,0.75,0,2") == ((-1.0, 1.0), (-0.5, 0.75), (0.0, 2.0))
    for bad in ("", "1,2,3,4,5", "0,1,0,1,1,1", "0,1,0,1,2,1", "a,b,c,d,e,f"):
        with pytest.raises(ValueError):
            pv.parse_bounds(bad)
    argv = pv.join_args(["--static", "vs.npy", "--dynamic", "vd.npy", "--bounds", "-1,1,-1,1,-1,1", "--views", "-5,40;60,-30", "--phases", "0,2", "--out", "o",
                          "--normalize", "--n-det", "64", "--geometry", "magix", "--samples", "96"])
    assert "--bounds=-1,1,-1,1,-1,1" in argv and "--views=-5,40;60,-30" in argv          # lists that start with a minus sign
    args = pv.parser().parse_args(argv)
    assert args.static == "vs.npy" and args.dynamic == "vd.npy" and args.bounds == ((-1.0, 1.0),) * 3
    assert args.views == [(-5.0, 40.0, 0.0), (60.0, -30.0, 0.0)] and args.phases == [0, 2]
    assert args.normalize and args.n_det == 64 and args.geometry == "magix" and args.samples == 96 and args.out == "o"
    args = pv.parser().parse_args(["--static", "vs.npy", "--views=0,0", "--out", "o"])
    assert args.dynamic is None and args.phases is None and args.bounds == ((-1.0, 1.0),) * 3 and args.samples == 192 and args.geometry == "xcat"
    assert not args.normalize


@pytest.mark.parametrize("shape", ref.GRIDS)
def test_oracle_equals_grid_sample_in_f64(shape):
    """Pins tests/drr_ref.project to an independent implementation before the GPU run: 1e-14 of |I0| + sum |term| per ray, at the
    shapes, bounds, views and depths of tests/test_drr_gpu.py (both boxes: the small one puts most samples outside and in the rim)."""
    i0 = float(np.float32(math.log(8.670397)))
    vols = ref.random_volume((3,) + shape, seed=sum(shape))
    worst = 0.0
    for _, geo, S in ref.geometries():
        z, dists = ref.depths(geo, S)
        for theta, phi in ref.VIEWS:
            o, d = ref.host_rays(geo, theta, phi)
            for bounds in (ref.BOUNDS, ref.SMALL_BOX):
                pix, scale, _ = ref.project(vols, o, d, z, dists, i0, bounds)
                want = ref.project_grid_sample(vols, o, d, z, dists, i0, bounds)
                assert pix.shape == want.shape == (3, o.shape[0])
                err = np.abs(pix - want) / scale
                worst = max(worst, float(err.max()))
                assert (err <= 1e-14).all(), (shape, bounds, float(err.max()))
                one, _, _ = ref.project(vols[1], o, d, z, dists, i0, bounds)          # a 3-D volume: the same numbers, [R]
                assert np.array_equal(one, pix[1])
    print(f"oracle vs grid_sample f64, grid {shape}: worst {worst:.2e} of |I0| + sum |term|")
