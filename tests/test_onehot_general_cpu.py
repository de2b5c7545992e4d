"""The CPU half of the general kernels' one-hot checks (tests/test_onehot_general_gpu.py holds the kernels to them): the decided nets of the new cases keep
their margin, the floors of check C, the launch shapes each case is listed for -- derived from a restatement of wide_plan (nca_api_wide.inc) and of
nca_wide_gemm's launch arithmetic (nca_kernels_wide.hip), so that a retuned `want` or tile size says which case lost its purpose -- and seeded faults
of the kind the general kernels could have: each is rejected by check A or B and accepted by rel_err < 1e-5, the bound of tests/test_wide_nets.py."""
import pytest
import torch

from conftest import rel_err
from nca_testlib import (GENERAL_POINT_CASES, GENERAL_RAY_CASES, ONEHOT_R, general_case, general_gemm_shape, general_layout, general_plan, general_ray_runs,
                         onehot_channel_rows, onehot_checks_ab, onehot_factor_errs, rank_one_split, wide_layers, wide_preacts)

MARGIN = 1 - 2.0 ** -6          # as tests/test_onehot_grads_cpu.py
TOL = 1e-5
CASES = list(GENERAL_POINT_CASES) + ["PCH"] + list(GENERAL_RAY_CASES)
KENC = 75                       # 3 (1 + 2 * 12) encoded inputs


def _feats(c, net):
    return c.feats_s if net == "s" else c.feats_d


@pytest.mark.parametrize("name", CASES)
def test_decided_nets_of_the_general_cases_have_the_margin(name):
    c = general_case(name)
    for net in c.nets:
        spec, p = c.spec(net), c.params(net)
        margins = c.margin_s if net == "s" else c.margin_d
        print(f"margin {name} {net}: " + " ".join(f"{m:.4f}" for m in margins))
        assert min(margins) >= MARGIN
        for dt in (torch.float32, torch.float64):
            for (wk, bk, _), z in zip(wide_layers(spec), wide_preacts(p, spec, _feats(c, net), dt, emulate_bf16=False)):          # (the general kernels round no operand)
                assert float(z.abs().min()) >= MARGIN and float(z.abs().max()) <= 3 + 2.0 ** -6, (net, wk, dt)
                on = p[bk] > 0
                assert bool(((z > 0) == on).all())
                assert 0.25 <= float(on.float().mean()) <= 0.75, (net, bk)


@pytest.mark.parametrize("name", CASES)
def test_floor_of_check_c_of_the_general_cases(name):
    """scaled_err of the f32 oracle from the f64 one on every launch, as the GPU half uses it: finite everywhere."""
    c = general_case(name)
    worst = {}
    for i in range(len(c.launches)):
        for k, e in c.floor(i, "f32").items():
            worst[k] = max(worst.get(k, 0.0), e)
    top = max(worst, key=worst.get)
    print(f"floor {name} {c.name}: {worst[top]:.2e} ({top})")
    assert all(e == e and e < float("inf") for e in worst.values())


# ------------------------------------------------------------------------------------------ the case table
# Restated (nca_testlib.general_plan / general_gemm_shape), nca_api_wide.inc wide_plan:
#     const int64_t tiles = ((y.F + 127) / 128) * ((y.F + 127) / 128);  const int64_t want = 512 / tiles > 1 ? 512 / tiles : 1;
#     p->nsplit = (int32_t)(want < chunk / NCA_WIDE_ROWS ? want : chunk / NCA_WIDE_ROWS);
#     if (max_bytes <= 0 || p->bytes <= max_bytes || chunk <= NCA_WIDE_ROWS) return;  chunk = align_up(chunk / 2, NCA_WIDE_ROWS);
# nca_kernels_wide.hip nca_wide_gemm:
#     const int nrt = (int)((a.rows + WG_BM - 1) / WG_BM), nct = (int)((a.cols + WG_BN - 1) / WG_BN);
#     const int gs = KIND == NCA_WG_WGRAD ? nrt * nct : nct;  const int64_t ng = KIND == NCA_WG_WGRAD ? a.nsplit : nrt;
#     if ((ng & 7) == 0) { q = lid >> 3; member = q % gs; group = (q / gs) * 8 + (lid & 7); } else { member = lid % gs; group = lid / gs; }
#     const int64_t per = ((ktot + a.nsplit - 1) / a.nsplit + WG_BK - 1) / WG_BK * WG_BK;  kb = zsplit * per;  ke = min(kb + per, ktot);
# nca_wide_colsum:  const int64_t per = (rows + nsplit - 1) / nsplit;          (rows: the VALID rows)
Y_S = general_layout(144, 2, KENC)
Y_D = general_layout(144, 2, KENC, T=8, P=10)
Y_SKIP = general_layout(144, 4, KENC, skip=2)


def _bijection(g):
    return sorted(g["tiles"]) == [(grp, m) for grp in range(g["ng"]) for m in range(g["gs"])]


def test_layouts():
    assert (Y_S["K0p"], Y_D["K0p"], Y_D["K0"]) == (80, 96, 83) and Y_SKIP["Kp"] == [80, 144, 224, 144]
    assert Y_SKIP["packed"] == (144 * 80 + 144 * 144 + 144 * 224 + 144 * 144 + 4 * 144 + 144 + 1 + 3) // 4 * 4          # (test_wide_nets: the header's own count)


def test_case_p1024_takes_the_remapped_tile_order_with_several_workgroups_per_group():
    _, N, ns = GENERAL_POINT_CASES["P1024"]
    for y in (Y_S, Y_D):
        chunk, nsplit, _ = general_plan(y, N)
        assert (chunk, nsplit) == (1024, 8)
        fwd = general_gemm_shape("fwd", chunk, 144)
        assert fwd["remap"] and (fwd["nrt"], fwd["gs"]) == (8, 2) and _bijection(fwd)          # forward and dgrad: the same arithmetic
        hid = general_gemm_shape("wgrad", 144, 144, nsplit, chunk)
        enc = general_gemm_shape("wgrad", 144, y["K0p"], nsplit, chunk)
        assert hid["remap"] and hid["gs"] == 4 and hid["per"] == 128 and hid["empty"] == 0 and _bijection(hid)
        assert enc["remap"] and enc["gs"] == 2 and enc["nct"] == 1 and _bijection(enc)
    assert sorted(n // 128 for n in ns) == list(range(8))          # one one-hot per row tile
    assert general_plan(Y_S, N, True, 3 << 20)[:2] == (512, 4) and general_plan(Y_D, N, True, 3 << 20)[:2] == (512, 4)          # check F's second chunking


def test_case_p1100_takes_the_identity_order_and_has_a_ragged_last_tile():
    _, N, ns = GENERAL_POINT_CASES["P1100"]
    for y in (Y_S, Y_D):
        chunk, nsplit, _ = general_plan(y, N)
        assert (chunk, nsplit) == (1152, 9)
        assert not general_gemm_shape("fwd", chunk, 144)["remap"] and not general_gemm_shape("wgrad", 144, 144, nsplit, chunk)["remap"]
        assert general_gemm_shape("wgrad", 144, 144, nsplit, chunk)["per"] == 128
        assert general_plan(y, N, True, 3 << 20)[:2] == (640, 5)          # check F's second chunking: 640 + 460 valid rows
        assert general_plan(y, N, False, 3 << 20)[0] == 1152 and general_plan(y, N, False, 1 << 20)[0] == 640          # the forward is cut by 1 MiB alone
    assert N - 1024 == 76 and 1152 - N == 52 and set(ns) == {0, 1023, 1024, N - 1}


def test_case_p16500_has_splits_that_straddle_row_tiles_and_empty_splits():
    _, N, ns = GENERAL_POINT_CASES["P16500"]
    for y in (Y_S, Y_D):
        chunk, nsplit, nbytes = general_plan(y, N)
        assert (chunk, nsplit) == (16512, 128) and chunk // 128 == 129 and 55e6 < nbytes < 65e6
        w = general_gemm_shape("wgrad", 144, 144, nsplit, chunk)
        assert w["per"] == 144 and w["empty"] == 13 and w["remap"] and _bijection(w)
        assert not general_gemm_shape("fwd", chunk, 144)["remap"]
    assert (N + 127) // 128 == 129          # nca_wide_colsum's per: another cut of the same rows
    per = 144
    assert (143 // per, 144 // per) == (0, 1) and 143 // 128 == 144 // 128 == 1          # the first seam lies inside row tile 1
    assert (16415 // per, 16416 // per) == (113, 114) and 114 == 128 - 13 - 1 and 115 * per >= 16512          # ... and the last one before the last split with rows
    assert set(ns) == {143, 144, 8255, 16415, 16416, N - 1}


def test_case_pskip_and_pch_and_the_merged_general_case():
    assert general_plan(Y_SKIP, 300)[:2] == (384, 3)
    k = general_layout(48, 4, 2 + 2 * 2 * 5, cout=3, skip=3)
    assert k["K0"] == 22 and general_plan(k, 200)[:2] == (256, 2)
    # tests/test_onehot_grads_gpu.py::test_onehot_points_general_kernels (F144_e1, N = 300, 3 MB): 384 rows fit 3 MB, so it runs ONE chunk of three row tiles and splits
    for y in (Y_S, Y_D):
        assert general_plan(y, 300, True, 3 << 20)[:2] == (384, 3)


def test_case_rg_is_cut_into_runs_of_whole_rays_above_the_wrappers_floor():
    S = GENERAL_RAY_CASES["RG"][1]
    extra = 4 * ((ONEHOT_R * S * 4 + 255) // 256 * 256)

    def need_of(rays):
        return sum(general_plan(y, (rays * S + 127) // 128 * 128)[2] for y in (Y_S, Y_D))

    assert general_ray_runs(ONEHOT_R, S, need_of, (40 << 30) - extra) == 9
    U = need_of(9) + extra
    for cap, rays in ((3500000, 5), (2500000, 3)):
        assert general_ray_runs(ONEHOT_R, S, need_of, cap - extra) == rays
        assert (1 << 20) < need_of(rays) + extra <= cap < U
    assert [(0 // 3), (4 // 3), (8 // 3)] == [0, 1, 2] and [(0 // 5), (4 // 5), (8 // 5)] == [0, 0, 1]
    print(f"RG: U = {U} bytes, 5 rays per run {need_of(5) + extra}, 3 rays per run {need_of(3) + extra}")


# ------------------------------------------------------------------------------------------ seeded faults
def _static_target(name, i):
    """(case, spec, params, the f64 oracle's gradients of the static net of launch i, the sample's input row)."""
    c = general_case(name)
    g = {k[2:]: v.clone() for k, v in c.oracle(i, "f32").items() if k[0] == "s"}
    where = c.launches[i][0]
    return c, c.ss, c.ps, g, c.feats("s", where)


def _accepted_by_rel_err(bad, g):
    for k in g:
        assert rel_err(bad[k], g[k]) < TOL, k          # the measure of tests/test_wide_nets.py does not see it


@pytest.mark.parametrize("name", ["P1024", "PSKIP", "PCH"])
def test_the_oracle_passes_the_checks(name):
    c, spec, p, g, x = _static_target(name, 1)
    assert onehot_checks_ab(spec, p, g, x, "oracle") <= 2.0 ** -40
    assert max(e for _, e, _ in onehot_factor_errs(spec, g, g)) == 0.0
    if name == "PCH":
        onehot_channel_rows(g["output_linear.0.weight"], g["output_linear.0.bias"], c.launches[1][1], "oracle")


def test_fault_in_the_second_column_tile_is_caught_by_check_a():
    """A relative error of 1e-4 in the small entries of columns 128 .. 143 of a hidden layer's weight gradient: the 16-wide second column tile of the wgrad."""
    c, spec, p, g, x = _static_target("P1024", 3)
    key = "early_pts_layers.2.weight"
    a, u = rank_one_split(g[key], g["early_pts_layers.2.bias"])
    small = (g[key].abs() > 0) & (g[key].abs() < 0.09 * g[key].abs().max())          # (1e-4 of them: under 1e-5 of the largest entry)
    small[:, :128] = False
    assert int(small.sum()) >= 4          # (a hidden layer's inputs are 0 or in [1, 3]: an entry is small where its unit's delta is)
    bad = {k: v.clone() for k, v in g.items()}
    bad[key][small] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="A: row, column"):
        onehot_checks_ab(spec, p, bad, x, "fault")
    _accepted_by_rel_err(bad, g)


def test_fault_in_the_skip_layers_column_map_is_caught_by_check_b():
    """The skip layer's hidden part K0p - K0 = 5 columns off, in the rows of off units.  Those rows are exact zeros, and zeros moved by 5 columns are the
    same zeros: what a wrong column map does to such a row is bring in what lies 5 floats further in the slab -- here an on unit's hidden part, at 1e-6
    of its size (a slab that was not cleared)."""
    c, spec, p, g, x = _static_target("PSKIP", 2)
    key, K0, K0p = "skip_connection.0.weight", Y_SKIP["K0"], Y_SKIP["K0p"]
    assert g[key].shape == (144, K0 + 144) and K0p - K0 == 5
    off = torch.nonzero(p["skip_connection.0.bias"] < 0).flatten()
    src = int(g["skip_connection.0.bias"].abs().argmax())
    bad = {k: v.clone() for k, v in g.items()}
    bad[key][off, K0 + 5:] = 1e-6 * g[key][src, K0:-5]
    assert bool(bad[key][off].any())
    with pytest.raises(AssertionError, match="B: off-unit rows"):
        onehot_checks_ab(spec, p, bad, x, "fault")
    _accepted_by_rel_err(bad, g)


def test_fault_between_output_channels_is_caught_by_check_b():
    """A row o != o* of dWo at 1e-6 of the largest entry."""
    c, spec, p, g, x = _static_target("PCH", 1)
    o = c.launches[1][1]
    bad = {k: v.clone() for k, v in g.items()}
    bad["output_linear.0.weight"][(o + 1) % 3] = 1e-6 * g["output_linear.0.weight"].abs().max()
    with pytest.raises(AssertionError, match="B: output channels other than"):
        onehot_channel_rows(bad["output_linear.0.weight"], bad["output_linear.0.bias"], o, "fault")
    with pytest.raises(AssertionError, match="output_linear.0.weight"):
        onehot_checks_ab(spec, p, bad, x, "fault")          # (rank one over the 3 x F layer: a zero-scale entry must be zero bit for bit)
    _accepted_by_rel_err(bad, g)


def test_fault_of_an_empty_split_that_is_not_cleared_is_caught_by_check_b():
    """One empty split's slab holds a denormal-scale constant: nca_wide_reduce adds it to every entry in f32 -- invisible in an entry that is not zero."""
    c, spec, p, g, x = _static_target("P16500", 4)
    bad = {k: (v.float() + torch.tensor(1e-40)).double() for k, v in g.items()}
    key = "early_pts_layers.2.weight"
    nz = g[key] != 0
    assert torch.equal(bad[key][nz], g[key].float().double()[nz]) and bool((bad[key][~nz] != 0).all())
    with pytest.raises(AssertionError, match="B: off-unit rows"):
        onehot_checks_ab(spec, p, bad, x, "fault")
    _accepted_by_rel_err(bad, g)
