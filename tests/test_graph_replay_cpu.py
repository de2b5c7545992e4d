"""The teeth of tests/test_graph_replay_gpu.py, proved without a GPU.  That module replays every captured entry point on a fixed sequence of
inputs (tests/nca_testlib.py: replay_*) and compares each replay with an eager call.  An output that is cleared and then accumulated into --
a maximum, a histogram, a sum of floating-point atomics, the general kernels' gradients -- goes wrong under replay when the clear does
nothing (docs/DESIGN_rounds1-4.md 4.4).  Here the numpy references of the same operations run over the same sequences, a skipped clear is
modelled (a running maximum, a running sum, a gradient plus the previous one), and the stale value must differ from the clean one on every
replay after the first: by at least 1 for the integer and bitwise outputs, by at least 1000 times the tolerance the GPU half applies for the
toleranced ones.  A condition on the sequences, not a measurement: a sequence that fails it is changed."""
import numpy as np
import torch

from nca_testlib import (REPLAY_AMPLITUDES, REPLAY_INPUTS, FAKE, REPLAY_RAYS, capi, lib,  # noqa: F401
                         REPLAY_TILE_SHAPE, REPLAY_VESS_SIGMAS, oracle_render_grads, prefixed_grads, replay_mlp_case,
                         replay_ray_case, replay_ray_upstream, replay_references, replay_upstream, replay_volumes)
from oracle import nerfca_oracle as O

import vess_ref

REPLAYS = list(range(REPLAY_INPUTS)) + [REPLAY_INPUTS - 1]          # the GPU half's order: every input, then the last one again
FACTOR = 1000.0


def running(values, combine):
    """What an output holds after each replay when its clear does nothing: combine(previous content, this replay's clean result)."""
    out, held = [], None
    for k in REPLAYS:
        held = values[k] if held is None else combine(held, values[k])
        out.append(held)
    return out


def test_the_sequence_is_ordered_as_the_gpu_half_says():
    assert REPLAY_INPUTS >= 3 and len(REPLAY_AMPLITUDES) == REPLAY_INPUTS and REPLAYS[-1] == REPLAYS[-2]
    assert all(a > b > 0 for a, b in zip(REPLAY_AMPLITUDES, REPLAY_AMPLITUDES[1:]))
    vols = [replay_volumes(REPLAY_TILE_SHAPE, k) for k in range(REPLAY_INPUTS)]
    for v in vols:
        assert v.shape == (2,) + REPLAY_TILE_SHAPE and v.dtype == np.float32 and not np.array_equal(v[0], v[1])
    assert all(a.max() > b.max() for a, b in zip(vols, vols[1:]))


def test_a_stale_maximum_shows_in_norm_max_and_in_the_vesselness():
    """The maxima fall strictly, per volume: a running maximum keeps the first input's value, which is not the clean one on any replay after the
    first -- the repeated last input included: what it holds there is still input 0's maximum."""
    clean = replay_references()["norm_max"]
    stale = running(clean, np.maximum)
    for i, k in enumerate(REPLAYS):
        if i:
            if REPLAYS[i - 1] != k:
                assert (clean[k] < clean[REPLAYS[i - 1]]).all(), (k, clean[k], clean[REPLAYS[i - 1]])
            assert (stale[i] == clean[0]).all()
            assert (np.abs(stale[i].view(np.int64) - clean[k].view(np.int64)) >= 1).all(), (i, k)
    # the wrapper's pipeline (ccta.vesselness with Frangi's c, one graph): per scale the maximum of the smoothed volume falls as well, and a
    # stale c changes the bits of the response
    for sigma in REPLAY_VESS_SIGMAS:
        held = None
        for k in range(REPLAY_INPUTS):
            s = vess_ref.smooth(replay_volumes(REPLAY_TILE_SHAPE, k), sigma)
            m = vess_ref.norm_max(s, sigma * sigma)
            if held is not None:
                assert (m < held).all(), (sigma, k)
                c_clean, c_stale = 0.5 * np.sqrt(m), 0.5 * np.sqrt(np.maximum(held, m))
                for v in range(2):
                    a = vess_ref.vesselness_scale(s[v:v + 1], sigma * sigma, 0.5, 0.5, float(c_clean[v]))
                    b = vess_ref.vesselness_scale(s[v:v + 1], sigma * sigma, 0.5, 0.5, float(c_stale[v]))
                    assert (a > 0).any() and not np.array_equal(a.view(np.int32), b.view(np.int32)), (sigma, k, v)
            held = m if held is None else np.maximum(held, m)


def test_stale_component_sizes_show_on_every_replay_after_the_first():
    ref = replay_references()
    clean, counts = ref["sizes"], ref["counts"]
    assert all(not np.array_equal(a, b) for a, b in zip(counts, counts[1:])), counts          # the components change with the mask
    assert all(a[:, 0].sum() < b[:, 0].sum() for a, b in zip(clean, clean[1:]))              # the mask shrinks: the background grows
    stale = running(clean, np.add)
    for i, k in enumerate(REPLAYS):
        if i:
            diff = np.abs(stale[i].astype(np.int64) - clean[k])
            assert (diff.max(axis=1) >= 1).all(), (i, k)
    assert np.array_equal(stale[-1] - stale[-2], clean[REPLAYS[-1]])          # the repeated input: doubled on top of what was there


def _toleranced(name):
    clean = replay_references()[name]
    stale = running([c[0] for c in clean], np.add)
    for i, k in enumerate(REPLAYS):
        value, tol = clean[k]
        assert (tol > 0).any(), (name, k)
        if i:
            gap = np.abs(stale[i] - value) - FACTOR * tol
            # (per node for the back-projection: SOME node must show it -- enough, because the GPU half holds every node to its tolerance, so one node out fails it)
            assert gap.max() > 0, (name, i, k, float(gap.max()))
            if name != "drr":          # scalars per image / per term: every one of them shows
                assert (gap > 0).all(), (name, i, k, gap)
            if REPLAYS[i - 1] != k:    # the clean totals themselves move by far more than the tolerance from input to input
                assert (np.abs(value - clean[REPLAYS[i - 1]][0]) - FACTOR * tol).max() > 0, (name, k)


def test_stale_ssim_sums_show():
    _toleranced("ssim")


def test_stale_total_variation_terms_show():
    _toleranced("voltv")


def test_stale_back_projection_shows():
    _toleranced("drr")
    g, tol = replay_references()["drr"][0]
    assert ((tol > 0) & (np.abs(g) > FACTOR * tol)).sum() >= g.size // 4          # not one lucky node: a quarter of them and more


def _stale_gradients_differ(grads):
    """grads: per input a dict of parameter gradients.  grads[k] + grads[previous] must differ from grads[k] in every parameter tensor."""
    for i, k in enumerate(REPLAYS):
        if i:
            for name, g in grads[k].items():
                prev = grads[REPLAYS[i - 1]][name]
                stale = (g.float() + prev.float())
                assert bool((stale != g.float()).any()), (i, name)
                assert float((stale - g.float()).abs().max()) >= 1e-3 * float(g.float().abs().max()), (i, name)


def test_stale_gradients_of_the_general_point_backward_show():
    spec, params, x, win = replay_mlp_case()
    assert spec.num_filters > 128          # the general kernels
    grads = []
    for k in range(REPLAY_INPUTS):
        p = {n: v.clone().double().requires_grad_(True) for n, v in params.items()}
        y = O.static_forward(p, spec, x.double(), win.double())
        (y * replay_upstream(k, tuple(y.shape)).double()).sum().backward()
        grads.append({n: v.grad.detach() for n, v in p.items()})
    _stale_gradients_differ(grads)


def test_stale_gradients_of_the_general_ray_backward_show():
    c = replay_ray_case()
    grads = []
    for k in range(REPLAY_INPUTS):
        g_pix, g_s, g_d = replay_ray_upstream(k)
        assert g_pix.shape == c["I0"].shape and g_s.shape == g_d.shape == (c["o"].shape[0], c["z"].shape[0])
        pso, pdo = oracle_render_grads(c["ps"], c["ss"], c["pd"], c["sd"], c["win"], c["o"], c["d"], c["ph"], c["I0"], c["z"], g_pix, g_s / 50, g_d / 50,
                                       dt=torch.float64)[4:]
        grads.append(prefixed_grads(pso, pdo))
    _stale_gradients_differ(grads)


def test_backward_workspace_query_without_a_cap_sizes_for_one_ray_per_run(lib, capi):
    """Pins what include/nerfca_hip.h says of nca_render_bwd_workspace with general nets: max_bytes <= 0 is not "no cap" but the smallest plan, one ray per
    run -- less than a backward from the general forward store needs, which takes all its rays' scratch at once and refuses a smaller workspace with
    NCA_E_WORKSPACE.  Callers pass the cap they can afford (fused: at least 1 MiB); the GPU half passes 2^28."""
    import ctypes as C
    R, S = REPLAY_RAYS
    nets = [capi.NcaNet(F=144, n_hidden=1, n_late=0, enc_mode=capi.ENC_BANDS, L=12, T=T, P=10 if T else 0, reserved=0) for T in (0, 8)]
    rays = capi.NcaRays(R=R, S=S, ray_is_f64=1, origins=FAKE, dirs=FAKE, phase=FAKE, phase_stride_r=1, z=FAKE, dists=FAKE, I0=FAKE, act=capi.ACT_SOFTPLUS, single_field=0,
                        scale=1e-2, store_format=capi.STORE_GENERAL)          # (the query reads no device pointer: it only wants them non-NULL)

    def query(cap):
        return lib.nca_render_bwd_workspace(C.byref(rays), C.byref(nets[0]), C.byref(nets[1]), capi.PREC_F32, cap)

    small, capped = query(0), query(1 << 28)
    assert 0 < small < capped and query(1) == small and query(-5) == small, (small, capped)
    assert query(capped) == capped          # a cap that fits the whole batch in one run changes nothing
