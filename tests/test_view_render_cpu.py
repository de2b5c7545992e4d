"""View rendering (export.render_view / render_sequence, csrc/view/nca_view.hip): everything that can be checked without a launch --
the C-ABI surface, every refusal (with pointers that are never read), the workspace query, the descriptor packer, the chunk plan and
the command line of tools/render_views.py."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

import nca_testlib as T
from nca_testlib import E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_view_rays", "nca_view_points", "nca_view_compose", "nca_image_normalize_workspace", "nca_image_normalize", "nca_view_last_error")
refused = functools.partial(T.refused, "view")


def view(capi, W=4, H=5):
    return capi.NcaView(pose=(C.c_float * 12)(*range(12)), W=W, H=H, d_det=(C.c_float * 2)(0.5, 0.25), off_det=(C.c_float * 2)(0, 0), dsd=25.0)


def test_new_names_are_declared_bound_and_exported(capi):
    T.declared_bound_and_exported(capi, NEW)


def test_view_descriptor_size_matches_the_header(capi):
    header = open(os.path.join(ROOT, "include", "nerfca_hip.h")).read()
    body = re.search(r"typedef struct NcaView \{(.*?)\} NcaView;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "int32_t"), decl          # four-byte members only: no padding
        for name in names.split(","):
            m = re.search(r"\[(\d+)\]", name)
            size += 4 * (int(m.group(1)) if m else 1)
    assert size == 76 == C.sizeof(capi.NcaView)
    assert [n for n, _ in capi.NcaView._fields_] == ["pose", "W", "H", "d_det", "off_det", "dsd"]


def test_view_rays_refusals(capi, lib):
    v = view(capi)          # 4 x 5 = 20 pixels
    rays = lambda vv, p0, n, o=FAKE, d=FAKE: lib.nca_view_rays(C.byref(vv) if vv is not None else None, p0, n, 1, o, d, None)
    refused(capi, lib, rays(v, 0, 0), "nca_view_rays", "n = 0")
    refused(capi, lib, rays(v, 0, -3), "n = -3")
    refused(capi, lib, rays(v, -1, 4), "p0 = -1")
    refused(capi, lib, rays(v, 17, 4), "20")
    refused(capi, lib, rays(v, 21, 1), "20")
    refused(capi, lib, rays(v, 1, (1 << 63) - 1), "20")       # p0 + n does not wrap
    refused(capi, lib, rays(view(capi, W=0), 0, 1), "0 x 5")
    refused(capi, lib, rays(view(capi, H=-2), 0, 1), "4 x -2")
    refused(capi, lib, rays(v, 0, 20, o=None), "NULL")
    refused(capi, lib, rays(v, 0, 20, d=None), "NULL")
    refused(capi, lib, rays(None, 0, 20), "NULL")


def test_view_points_refusals(capi, lib):
    pts = lambda R, S, o=FAKE, d=FAKE, z=FAKE, out=FAKE: lib.nca_view_points(R, S, o, d, z, out, None)
    refused(capi, lib, pts(0, 8), "nca_view_points", "not positive")
    refused(capi, lib, pts(8, 0), "not positive")
    refused(capi, lib, pts(-1, 8), "not positive")
    refused(capi, lib, pts(8, 8, o=None), "NULL")
    refused(capi, lib, pts(8, 8, d=None), "NULL")
    refused(capi, lib, pts(8, 8, z=None), "NULL")
    refused(capi, lib, pts(8, 8, out=None), "NULL")
    refused(capi, lib, pts(1 << 61, 8), "overflows")
    refused(capi, lib, pts(1 << 40, 8), "one launch")


def test_view_compose_refusals(capi, lib):
    comp = lambda n, s=FAKE, p=FAKE, ps=FAKE, pd=FAKE: lib.nca_view_compose(n, 2.0, s, FAKE, 1, p, ps, pd, None)
    refused(capi, lib, comp(0), "nca_view_compose", "n = 0")
    refused(capi, lib, comp(-5), "n = -5")
    refused(capi, lib, comp(4, s=None), "pix_s is NULL")
    refused(capi, lib, comp(4, p=None), "NULL")
    refused(capi, lib, comp(4, ps=None), "NULL")
    refused(capi, lib, comp(4, pd=None), "NULL")


def test_image_normalize_refusals_and_workspace(capi, lib):
    ws = lib.nca_image_normalize_workspace
    norm = lambda k, n, img=FAKE, mm=FAKE, work=FAKE, wb=1 << 30: lib.nca_image_normalize(k, n, img, None, mm, work, wb, None)
    refused(capi, lib, ws(0), "nca_image_normalize_workspace", "n = 0")
    refused(capi, lib, ws(-7), "n = -7")
    sizes = [ws(n) for n in (1, 2, 255, 256, 257, 2048, 2049, 70001, 1 << 20, 1 << 24, 1 << 31, 1 << 40)]
    assert all(b > 0 and b % 256 == 0 for b in sizes), sizes
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    refused(capi, lib, norm(0, 16), "nca_image_normalize", "n_img = 0")
    refused(capi, lib, norm(-1, 16), "n_img = -1")
    refused(capi, lib, norm(2, 0), "n = 0")
    refused(capi, lib, norm(2, 16, img=None), "img is NULL")
    refused(capi, lib, norm(2, 16, mm=None), "minmax is NULL")
    refused(capi, lib, norm(3, 70001, wb=3 * ws(70001) - 1), str(3 * ws(70001)), code=E_WORKSPACE)
    refused(capi, lib, norm(3, 70001, wb=ws(70001)), "workspace", code=E_WORKSPACE)          # one image's worth for three images
    refused(capi, lib, norm(1, 16, work=None), "workspace", code=E_WORKSPACE)


def test_pack_view_reproduces_the_f32_pose():
    from nerfca_amd import export, synthetic
    from nerfca_amd.train.proj_helpers import source_matrix_tigre
    geo = dict(synthetic.xcat_geometry(16), nDetector=[12, 20], dDetector=[2.0 / 12, 0.1], offDetector=[0.013, -0.02])
    for theta, phi, larm in ((-5, 40, 0), (60, -30, 0), (0, 0, 0), (137.5, -63, 0)):
        v = export.pack_view(geo, theta, phi, larm)
        want = source_matrix_tigre(np.array([0, 0, -geo["DSO"]]), theta, phi, larm).astype(np.float32)[:3, :4]
        assert np.array_equal(np.array(list(v.pose), dtype=np.float32).reshape(3, 4), want)
        assert (v.W, v.H) == (12, 20)
        assert list(v.d_det) == [np.float32(2.0 / 12), np.float32(0.1)] and list(v.off_det) == [np.float32(0.013), np.float32(-0.02)]
        assert v.dsd == 25.0


@pytest.mark.parametrize("n_pixels", [1, 255, 320])
def test_chunk_plan_covers_every_pixel_once(n_pixels):
    from nerfca_amd import export
    plan = export.chunk_plan(n_pixels, 100)
    covered = np.zeros(n_pixels, dtype=np.int64)
    for p0, n in plan:
        assert 0 < n <= 100 and p0 >= 0 and p0 + n <= n_pixels
        covered[p0:p0 + n] += 1
    assert (covered == 1).all()
    assert [p0 for p0, _ in plan] == sorted(p0 for p0, _ in plan) and len(plan) == -(-n_pixels // 100)
    with pytest.raises(ValueError):
        export.chunk_plan(n_pixels, 0)


def test_view_rendering_refuses_the_cpu():
    import torch
    from nerfca_amd import _capi, export, synthetic
    from nerfca_amd.model.CPPN import CPPN
    with pytest.raises(_capi.NcaError):
        export.view_rays(synthetic.xcat_geometry(8), 0, 0, device="cpu")
    with pytest.raises(_capi.NcaError):
        export.render_view(CPPN(synthetic.net_definitions("cpu", F=32)[0]), None, synthetic.xcat_geometry(8), 0, 0, None, 8)
    with pytest.raises(_capi.NcaError):
        export.normalize_images(torch.zeros(2, 8))


def test_cli_parses_its_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import render_views as rv
    finally:
        sys.path.pop(0)
    assert rv.parse_views("-5,40; 60,-30,2.5;") == [(-5.0, 40.0, 0.0), (60.0, -30.0, 2.5)]
    assert rv.parse_phases("0,3, 7") == [0, 3, 7]
    for bad in ("", "1", "1,2,3,4", "a,b"):
        with pytest.raises(ValueError):
            rv.parse_views(bad)
    args = rv.parser().parse_args(["--static", "s.pth", "--views", "0,0;90,0", "--phases", "1,2", "--out", "o", "--normalize", "--precision", "bf16"])
    assert args.views == [(0.0, 0.0, 0.0), (90.0, 0.0, 0.0)] and args.phases == [1, 2] and args.dynamic is None
    assert args.normalize and args.precision == "bf16" and args.samples == 192 and args.geometry == "xcat"
    joined = rv.join_views(["--static", "s.pth", "--views", "-5,40;60,-30", "--out", "o"])          # a list that starts with a minus sign
    assert joined == ["--static", "s.pth", "--views=-5,40;60,-30", "--out", "o"]
    assert rv.parser().parse_args(joined).views == [(-5.0, 40.0, 0.0), (60.0, -30.0, 0.0)]
    geo = rv.load_geometry("magix", 8)
    assert set(rv.GEO_KEYS) <= set(geo) and geo["nDetector"] == [8, 8]
