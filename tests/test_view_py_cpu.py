"""nerfca_amd._view without a GPU: its refusals, word for word as the wrappers have always made them (metrics._check_volume,
drr._check_volumes and the two NaN-threshold refusals lived in the wrappers before), and that it is a leaf: it loads none of the wrappers."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from nca_testlib import capi  # noqa: F401


def test_refusals_word_for_word(capi):
    from nerfca_amd import _view, ccta, drr, metrics

    def refuses(text, fn, *args, **kw):
        with pytest.raises(capi.NcaError) as e:
            fn(*args, **kw)
        assert str(e.value) == text

    on_cpu = "{} must live on the GPU: the fused NeRF-CA path has no CPU implementation (got device cpu)"
    x = torch.zeros(2, 3, 4)
    refuses("zoom: vol is not a tensor", _view.check_volume, [[1.0]], "zoom")
    refuses("prepare_ccta: raw_hu is not a tensor", _view.check_volume, None, "prepare_ccta", "raw_hu")
    refuses(on_cpu.format("vol"), _view.check_volume, x, "zoom")
    refuses(on_cpu.format("truth"), _view.check_volume, x, "mask_distances", "truth")
    refuses(on_cpu.format("vol"), _view.volume_stack, x, "spline_filter")
    refuses("distance_transform: threshold = nan is not a number", _view.finite_threshold, float("nan"), "distance_transform")
    refuses("cityblock_distance: threshold = nan is not a number", _view.finite_threshold, torch.tensor(float("nan")), "cityblock_distance")
    assert _view.finite_threshold(torch.tensor(0.25), "x") == 0.25 and isinstance(_view.finite_threshold(1, "x"), float)
    refuses("project_rays takes contiguous float32 volumes [n0,n1,n2] or [n_vol,n0,n1,n2], got torch.float64 (2, 3, 4)", _view.check_contiguous_volumes, x.double(),
            "project_rays")
    refuses("total_variation takes contiguous float32 volumes [n0,n1,n2] or [n_vol,n0,n1,n2], got torch.float32 (3, 4)", _view.check_contiguous_volumes, x[0],
            "total_variation")
    refuses("project_rays takes contiguous float32 volumes [n0,n1,n2] or [n_vol,n0,n1,n2], got torch.float32 (2, 3, 2) (not contiguous)",
            _view.check_contiguous_volumes, x[:, :, ::2], "project_rays")
    _view.check_contiguous_volumes(x, "project_rays")
    # the wrappers still make them, in the same words
    refuses("gaussian_filter: vol is not a tensor", ccta.gaussian_filter, [[1.0]], 1.0)
    refuses(on_cpu.format("vol"), ccta.cityblock_distance, x, threshold=float("nan"))
    refuses(on_cpu.format("vol"), metrics.distance_transform, x, ((0.0, 1.0),) * 3, threshold=0.5)
    refuses("centreline_coverage: vol is not a tensor", metrics.centreline_coverage, 3, ((0.0, 1.0),) * 3, [], threshold=0.5, tol=1.0)
    refuses(on_cpu.format("volumes"), drr.total_variation, x, bounds=((0.0, 1.0),) * 3)


def test_view_is_a_leaf_module():
    """A fresh interpreter imports nerfca_amd._view under a bare package (the real __init__ imports every wrapper itself): what _view pulls in
    on its own is _capi and fused, and none of the wrappers."""
    code = ("import json, sys, types\n"
            "pkg = types.ModuleType('nerfca_amd')\n"
            f"pkg.__path__ = [{os.path.join(ROOT, 'nerf-ca_amd')!r}]\n"
            "sys.modules['nerfca_amd'] = pkg\n"
            "import nerfca_amd._view\n"
            "print(json.dumps(sorted(m for m in sys.modules if m.startswith('nerfca_amd.'))))\n")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    loaded = json.loads(run.stdout.strip().splitlines()[-1])
    assert {"nerfca_amd._view", "nerfca_amd._capi", "nerfca_amd.fused"} <= set(loaded)
    for wrapper in ("metrics", "ccta", "drr", "export", "phantom"):
        assert "nerfca_amd." + wrapper not in loaded, loaded
