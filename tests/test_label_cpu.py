"""Connected components (nca_vol_label, nca_vol_label_sizes, metrics.label / component_sizes / keep_largest / component_report): everything
that can be checked without a launch -- the C-ABI surface, every refusal of both entry points (with device pointers that are never read),
the workspace query, the numpy oracle of the GPU tests (tests/label_ref.py) held to scipy.ndimage.label, the plain-torch reductions on
hand-made labels, the refusals of the Python layer and the command lines."""
import ctypes as C
import functools
import inspect
import math
import os
import sys

import numpy as np
import pytest
import scipy.ndimage
import torch

from conftest import ROOT

import nca_testlib as T
import label_ref as ref
from nca_testlib import E_UNSUPPORTED, E_WORKSPACE, FAKE, capi, lib  # noqa: F401

NEW = ("nca_vol_label_workspace", "nca_vol_label", "nca_vol_label_sizes", "nca_label_last_error")
refused = functools.partial(T.refused, "label")
grid = functools.partial(T.grid, n=(4, 5, 6), lo=(0.0, 0.0, 0.0), inv=(1.0, 2.0, 3.0))


def test_new_names_are_declared_bound_and_exported(capi):
    header = T.declared_bound_and_exported(capi, NEW)
    order = ["nca_skel_last_error(void)", "size_t nca_vol_label_workspace(", "int nca_vol_label(", "int nca_vol_label_sizes(", "nca_label_last_error(void)"]
    at = [header.index(s) for s in order]
    assert at == sorted(at)
    assert "---- label:" in header and header.index("---- label:") > header.index("---- skel:")
    assert callable(capi.check_label)
    from nerfca_amd import metrics
    for name in ("label", "component_sizes", "keep_largest", "largest_components", "component_report", "component_report_reductions"):
        assert callable(getattr(metrics, name)), name


# ----------------------------------------------------------------------------- refusals
def test_label_refusals(capi, lib):
    def call(g="default", vol=FAKE, n_vol=2, threshold=0.5, connectivity=1, invert=0, labels=FAKE + 64, counts=FAKE + 128, work=FAKE, work_bytes=1 << 62, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_label(g, vol, n_vol, threshold, connectivity, invert, labels, counts, work, work_bytes, None)

    who = "nca_vol_label:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(vol=None), who, "vol is NULL")
    refused(capi, lib, call(labels=None), who, "labels is NULL")
    refused(capi, lib, call(counts=None), who, "counts is NULL")
    refused(capi, lib, call(labels=FAKE), who, "labels is vol")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
    T.grid_refusals("label", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    refused(capi, lib, call(threshold=math.nan), "threshold = nan", "not a number")
    for ok in (math.inf, -math.inf, 0.0):
        assert call(threshold=ok, work=None) == E_WORKSPACE
    for bad in (0, 4, -1, 26):
        refused(capi, lib, call(connectivity=bad), f"connectivity = {bad}", "1, 2 or 3", code=E_UNSUPPORTED)
    for ok in (1, 2, 3):
        assert call(connectivity=ok, work=None) == E_WORKSPACE
    for bad in (2, -1):
        refused(capi, lib, call(invert=bad), f"invert = {bad}", "neither 0 nor 1")
    assert call(invert=1, work=None) == E_WORKSPACE
    # a label is a node index plus one in int32: 2^31 - 2 nodes are labelled, one more is not
    assert call(n=(2, 3, 357913941), n_vol=1, work=None) == E_WORKSPACE          # 6 x 357913941 = 2^31 - 2
    refused(capi, lib, call(n=(2, 1 << 15, 1 << 15), n_vol=1), "2^31 - 2", str(1 << 31), code=E_UNSUPPORTED)
    refused(capi, lib, call(n=(2, 3, 357913941 + 1), n_vol=1), "2^31 - 2", str((1 << 31) + 4), code=E_UNSUPPORTED)
    # no limit on an axis: 2^20 nodes along each in turn get as far as the workspace
    for a in range(3):
        n = [2, 2, 2]
        n[a] = 1 << 20
        assert call(n=n, work=None) == E_WORKSPACE
    # one tile per volume of 2 x 2 x 2: 2^31 - 1 of them are one launch; 2^30 volumes of 4 x 8 x 65 (two tiles, and three blocks of 1024
    # nodes each: the larger of the two launch sizes is named) are not, and neither are 2^30 of 4 x 4 x 128 (two of each)
    assert call(n=(2, 2, 2), n_vol=(1 << 31) - 1, work=None) == E_WORKSPACE
    refused(capi, lib, call(n=(4, 8, 65), n_vol=1 << 30), "tiles", "one launch", str(3 << 30))
    refused(capi, lib, call(n=(4, 4, 128), n_vol=1 << 30), "tiles", "one launch", str(1 << 31))
    g = grid(capi)
    need = lib.nca_vol_label_workspace(C.byref(g), 2)
    assert need == 1024 + 256          # 2 * 120 nodes * 4 bytes = 960 -> 1024, and 2 volumes of one block count, 8 bytes -> 256
    refused(capi, lib, call(work_bytes=need - 1), str(need - 1), str(need), code=E_WORKSPACE)
    refused(capi, lib, call(work=None), "work is NULL", code=E_WORKSPACE)
    refused(capi, lib, call(work_bytes=0), " 0 bytes", code=E_WORKSPACE)


def test_label_sizes_refusals(capi, lib):
    def call(g="default", labels=FAKE, n_vol=2, cap=5, sizes=FAKE + 64, **kw):
        g = C.byref(grid(capi, **kw)) if isinstance(g, str) else g
        return lib.nca_vol_label_sizes(g, labels, n_vol, cap, sizes, None)

    who = "nca_vol_label_sizes:"
    refused(capi, lib, call(g=None), who, "grid", "NULL")
    refused(capi, lib, call(labels=None), who, "labels is NULL")
    refused(capi, lib, call(sizes=None), who, "sizes is NULL")
    for bad in (0, -3):
        refused(capi, lib, call(n_vol=bad), f"n_vol = {bad}", "positive")
        refused(capi, lib, call(cap=bad), f"cap = {bad}", "positive")
    T.grid_refusals("label", capi, lib, lambda g, count: call(g=C.byref(g), n_vol=count or 2))
    refused(capi, lib, call(n=(2, 1 << 15, 1 << 15), n_vol=1), "2^31 - 2", code=E_UNSUPPORTED)
    # a workgroup per 4096 nodes of a volume: more than 2^24 of them are not one launch
    refused(capi, lib, call(n=(2, 2, 2), n_vol=(1 << 24) + 1), "tiles", "one launch", str((1 << 24) + 1))


def test_workspace_query(capi, lib):
    def q(n, n_vol, **kw):
        return lib.nca_vol_label_workspace(C.byref(grid(capi, n=n, **kw)), n_vol)

    def formula(n, n_vol):
        nodes = n[0] * n[1] * n[2]
        return (4 * n_vol * nodes + 255) // 256 * 256 + (4 * n_vol * ((nodes + 1023) // 1024) + 255) // 256 * 256

    assert q((4, 5, 6), 2) == 1280 and q((2, 2, 2), 1) == 512
    for n_vol in (1, 2, 7):
        for n in ((3, 4, 5), (9, 4, 130), (33, 17, 65), (256, 256, 256), (4, 4, 1 << 20)):
            assert q(n, n_vol) == formula(n, n_vol) and q(n, n_vol) % 256 == 0, (n, n_vol)
    assert q((512,) * 3, 64) == formula((512,) * 3, 64) > 1 << 32          # a size_t
    assert lib.nca_vol_label_workspace(None, 1) == 0
    for bad in (((1, 4, 4), 1), ((4, 4, 4), 0), ((4, 4, 4), -1), ((2, 1 << 15, 1 << 15), 1)):
        assert q(*bad) == 0, bad
    assert q((4, 4, 4), 1, reserved=1) == 0 and q((4, 4, 4), 1, inv=(1.0, 0.0, 1.0)) == 0


# ----------------------------------------------------------------------------- the oracle against scipy
@pytest.mark.parametrize("shape", ref.GPU_SHAPES, ids=str)
def test_oracle_equals_scipy(shape):
    names = [c[0] for c in ref.cases(shape)]
    assert {"random 0.3", "random 0.5", "random 0.7", "random 0.5 inverted", "empty", "full", "checkerboard", "nan", "serpentine"} <= set(names)
    assert ("two serpentines" in names) == (shape in ((5, 9, 65), (7, 9, 70), (9, 17, 130)))
    for name, stack, thr, inv in ref.cases(shape):
        for conn in ref.CONNECTIVITIES:
            got_l, got_c = ref.expected(shape, name, conn)
            assert got_l.dtype == np.int32 and got_c.dtype == np.int32 and got_l.shape == stack.shape and got_c.shape == (2,)
            structure = scipy.ndimage.generate_binary_structure(3, conn)
            for v in range(2):
                with np.errstate(invalid="ignore"):
                    m = stack[v] > thr
                want_l, want_c = scipy.ndimage.label(~m if inv else m, structure)
                assert got_c[v] == want_c and np.array_equal(got_l[v], want_l), (name, conn, v)
                alone = ref.label(stack[v:v + 1], thr, conn, inv)
                assert np.array_equal(alone[0][0], got_l[v]) and alone[1][0] == got_c[v]
            if name == "empty":
                assert got_c[0] == 0 and not got_l[0].any()
            if name == "full":
                assert got_c[0] == 1 and (got_l[0] == 1).all()
            if name == "checkerboard":
                N = stack[0].size
                assert tuple(got_c) == (((N + 1) // 2, N // 2) if conn == 1 else (1, 1))
            if name == "serpentine":
                assert got_c[0] == 1 and got_l[0][0, 0, 0] == 1 and got_c[1] in (1, 2)          # the second volume is the path cut once
            if name == "two serpentines":
                assert got_c[0] == (2 if conn == 1 else 1) and got_c[1] == 1
                assert got_l[0][3, 7, 63] == 1 and got_l[0][3, 8, 64] == got_c[0] == got_l[0][4, 8, 64]


def test_the_neighbourhoods_and_the_nan_rule():
    assert [len(ref.forward_offsets(c)) for c in (1, 2, 3)] == [3, 9, 13]
    for c in (1, 2, 3):
        st = scipy.ndimage.generate_binary_structure(3, c)
        offs = ref.forward_offsets(c)
        assert st.sum() == 2 * len(offs) + 1 and all(st[1 + a, 1 + b, 1 + d] for a, b, d in offs)
    x = np.array([np.nan, 0.5, 1.0, -np.inf, np.inf], dtype=np.float32)
    assert ref.mask_of(x, 0.5).tolist() == [False, False, True, False, True]          # a NaN and the threshold itself are not above it
    assert ref.mask_of(x, 0.5, True).tolist() == [True, True, False, True, False]
    lab = np.array([[[0, 1, 1], [2, 0, 7]]], dtype=np.int32)
    assert ref.sizes(lab, 3).tolist() == [[2, 2, 1]] and ref.sizes(lab, 9).tolist() == [[2, 2, 1, 0, 0, 0, 0, 1, 0]]


# ----------------------------------------------------------------------------- the plain-torch parts on hand-made labels
def hand_made():
    """labels [2, 2, 3, 4] and sizes: volume 0 has components of 5, 2, 5, 1 nodes; volume 1 one of 3 nodes."""
    a = np.array([[[1, 1, 1, 0], [1, 1, 0, 2], [0, 0, 0, 2]], [[3, 3, 3, 0], [3, 3, 0, 0], [0, 4, 0, 0]]], dtype=np.int32)
    b = np.zeros((2, 3, 4), dtype=np.int32)
    b[1, 2, 1:] = 1
    labels = np.stack([a, b])
    return torch.from_numpy(labels), torch.from_numpy(ref.sizes(labels, 5).astype(np.int64)), torch.tensor([4, 1])


def test_largest_components_on_hand_made_labels():
    from nerfca_amd import metrics
    labels, sizes, _ = hand_made()
    assert sizes.tolist() == [[11, 5, 2, 5, 1], [21, 3, 0, 0, 0]]
    a = labels[0]
    got = metrics.largest_components(labels, sizes, 1)
    assert got.dtype == torch.bool and got.shape == labels.shape
    assert torch.equal(got[0], a == 1) and torch.equal(got[1], labels[1] == 1)          # 5 against 5: the smaller label
    got = metrics.largest_components(labels, sizes, 2)
    assert torch.equal(got[0], (a == 1) | (a == 3)) and torch.equal(got[1], labels[1] == 1)          # fewer than k: all of them
    assert torch.equal(metrics.largest_components(labels, sizes, 3)[0], (a == 1) | (a == 3) | (a == 2))
    assert torch.equal(metrics.largest_components(labels, sizes, 9), labels > 0)
    got = metrics.largest_components(labels, sizes, min_size=3)
    assert torch.equal(got[0], (a == 1) | (a == 3)) and torch.equal(got[1], labels[1] == 1)
    assert not metrics.largest_components(labels, sizes, min_size=6).any()
    assert torch.equal(metrics.largest_components(labels, sizes, min_size=1), labels > 0)
    assert torch.equal(metrics.largest_components(labels[0], sizes[0], 1), a == 1)          # one volume, no leading shape
    lead = metrics.largest_components(labels.reshape(2, 1, 2, 3, 4), sizes.reshape(2, 1, 5), 1)
    assert lead.shape == (2, 1, 2, 3, 4) and torch.equal(lead.reshape(labels.shape), metrics.largest_components(labels, sizes, 1))
    none = metrics.largest_components(torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.tensor([[8]]), 1)          # the single background column
    assert none.shape == (1, 2, 2, 2) and not none.any()
    for bad in (dict(k=0), dict(k=-1), dict(k=1.5), dict(k=True), dict(k=2, min_size=3), dict(min_size=0), dict(min_size=2.5)):
        with pytest.raises(metrics._capi.NcaError, match="keep_largest"):
            metrics.largest_components(labels, sizes, **bad)
    with pytest.raises(metrics._capi.NcaError, match="belong together"):
        metrics.largest_components(labels, sizes[:1])


def test_component_report_reductions_on_hand_made_sizes():
    from nerfca_amd import metrics
    _, sizes, counts = hand_made()
    truth_sizes, truth_counts = torch.tensor([[20, 4], [24, 0]]), torch.tensor([1, 0])
    got = metrics.component_report_reductions(counts, sizes, truth_counts, truth_sizes)
    assert set(got) == {"components_pred", "components_truth", "betti0_error", "largest_share_pred", "largest_share_truth"}
    assert got["components_pred"].tolist() == [4, 1] and got["components_truth"].tolist() == [1, 0] and got["betti0_error"].tolist() == [3, 1]
    assert all(got[k].dtype == torch.int64 for k in ("components_pred", "components_truth", "betti0_error"))
    assert got["largest_share_pred"].dtype == torch.float64 and got["largest_share_pred"].tolist() == [5.0 / 13.0, 1.0]
    assert float(got["largest_share_truth"][0]) == 1.0 and math.isnan(float(got["largest_share_truth"][1]))          # an empty mask
    only_background = metrics.component_report_reductions(torch.tensor([0]), torch.tensor([[8]]), torch.tensor([0]), torch.tensor([[8]]))
    assert math.isnan(float(only_background["largest_share_pred"][0])) and only_background["betti0_error"].tolist() == [0]
    with pytest.raises(metrics._capi.NcaError, match="belong together"):
        metrics.component_report_reductions(counts, sizes, truth_counts[:1], truth_sizes[:1])


# ----------------------------------------------------------------------------- the Python layer
def test_the_python_layer_refuses_before_anything_touches_a_device(capi, monkeypatch):
    from nerfca_amd import metrics

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library")

    monkeypatch.setattr(metrics._view, "launch", no_launch)
    a = torch.zeros(2, 4, 4, 4)
    lab, cnt = torch.zeros(2, 4, 4, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    calls = [lambda: metrics.label(a, threshold=0.5), lambda: metrics.label(a > 0, threshold=0.5), lambda: metrics.label(a.numpy(), threshold=0.5),
             lambda: metrics.label(None, threshold=0.5), lambda: metrics.keep_largest(a, threshold=0.5), lambda: metrics.keep_largest(a > 0, 2, threshold=0.5),
             lambda: metrics.keep_largest(a, 0, threshold=0.5), lambda: metrics.keep_largest(a, 2, threshold=0.5, min_size=3),
             lambda: metrics.component_report(a, a, threshold=0.5), lambda: metrics.component_report(a, None, threshold=0.5),
             lambda: metrics.component_report(a, a > 0, threshold=0.5), lambda: metrics.component_sizes(lab, cnt),
             lambda: metrics.component_sizes(lab.long(), cnt), lambda: metrics.component_sizes(lab, cnt.int()), lambda: metrics.component_sizes(lab, cnt[:1]),
             lambda: metrics.component_sizes(None, cnt)]
    for i, call in enumerate(calls):
        with pytest.raises(capi.NcaError):
            call()
    with pytest.raises(capi.NcaError, match="k = 0"):
        metrics.keep_largest(a, 0, threshold=0.5)          # the rule is looked at first: before the device of vol
    with pytest.raises(capi.NcaError, match="both given"):
        metrics.keep_largest(a, 2, threshold=0.5, min_size=3)
    for bad in (0, 4, 1.5, True, "1"):
        with pytest.raises((capi.NcaError, ValueError, TypeError)):
            metrics._connectivity(bad, "label")
    assert [metrics._connectivity(c, "label") for c in (1, 2, 3, 2.0)] == [1, 2, 3, 2]
    sig = inspect.signature(metrics.label).parameters
    assert sig["threshold"].kind is inspect.Parameter.KEYWORD_ONLY and sig["threshold"].default is inspect.Parameter.empty
    assert sig["connectivity"].default == 1 and sig["invert"].default is False
    sig = inspect.signature(metrics.keep_largest).parameters
    assert sig["k"].default == 1 and sig["k"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and sig["connectivity"].default == 3 and sig["min_size"].default is None
    assert sig["threshold"].kind is inspect.Parameter.KEYWORD_ONLY and sig["threshold"].default is inspect.Parameter.empty
    sig = inspect.signature(metrics.component_report).parameters
    assert sig["connectivity"].default == 3 and sig["pred_threshold"].default is None and sig["threshold"].default is inspect.Parameter.empty


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_command_lines(capsys):
    cv = _tool("compare_volumes")
    base = ["a", "b", "--bounds", "0,1,0,1,0,1", "--threshold", "3"]
    args = cv.parser().parse_args(cv.join_args(base))
    assert args.components is False and args.connectivity == 3 and args.keep_largest is None
    args = cv.parser().parse_args(cv.join_args(base + ["--components", "--connectivity", "1", "--keep-largest", "2"]))
    assert args.components is True and args.connectivity == 1 and args.keep_largest == 2
    ps = _tool("phantom_study")
    args = ps.parser().parse_args([])
    assert args.components is False and args.keep_largest is None
    args = ps.parser().parse_args(["--distances", "--components", "--keep-largest", "1"])
    assert args.components is True and args.keep_largest == 1
    lb = _tool("label_bench")
    args = lb.parser().parse_args(["--out", "profiles/label_bench.txt"])
    assert args.out == "profiles/label_bench.txt" and args.passes == 3 and args.sides == "128,256" and args.volumes == "1,10" and args.connectivities == "1,3"
    for tool, argv in ((lb, ["--help"]), (lb, ["--passes", "many"]), (lb, ["--nonsense"]), (cv, cv.join_args(base + ["--connectivity", "4"])),
                       (cv, cv.join_args(base + ["--keep-largest", "one"])), (ps, ["--keep-largest"])):
        with pytest.raises(SystemExit) as e:
            tool.parser().parse_args(argv)
        assert (e.value.code == 0) == (argv == ["--help"])
    capsys.readouterr()
    # the columns need the study they are columns of, and the cleanup needs the components: refused before anything runs
    with pytest.raises(SystemExit) as e:
        ps.main(["--components"])
    assert "--distances" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        ps.main(["--distances", "--keep-largest", "1"])
    assert "--components" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cv.main(cv.join_args(base + ["--keep-largest", "1"]))
    assert "--components" in str(e.value.code)
