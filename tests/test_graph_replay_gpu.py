"""Every captured call must replay to the eager result.  bench.py's default step is replayed from a captured graph, and the worst bug of this
project lived there and nowhere else: a hipMemsetAsync captured into a HIP graph did nothing, and a kernel added whatever the memory held
(docs/DESIGN_rounds1-4.md 4.4).  This module holds every entry point of the view sections (view, drr, voltv, phantom, ssim, edt, filt, resample,
skel, label, vess, mesh) and the general (wide) kernels to their contract under capture, on a side stream, through one table-driven harness:

  1. the test owns static input, output and workspace tensors and runs one eager warm-up call on a side stream (as train/trainer.py does before
     it captures a step);
  2. it captures one call, or one short sequence of calls, into a torch.cuda.graph: one linear stream, no graph-related settings;
  3. for each of three inputs in a fixed order (tests/nca_testlib.py: replay_*; maxima fall strictly, the mask and its components change, every
     sum moves by far more than its tolerance -- tests/test_graph_replay_cpu.py proves that a skipped clear shows on these sequences) it copies
     the input into the static tensor, fills every output and every workspace with the poison words of fused._scratch (0x7FC12345, an f32 NaN)
     eagerly and outside the graph, checks that the poison landed, replays, and compares with an eager call on fresh (equally poisoned) tensors;
  4. it replays the last input a second time: a counter that is never cleared shows as doubled.

Outputs that their section promises bit for bit are compared byte for byte.  The three outputs summed with floating-point atomics (nca_ssim's
sums, nca_vol_tv's terms, nca_drr_backproject) are ADDED INTO by the library and zeroed by the caller: the captured sequence is a fill kernel and
the call, and they are held to the tolerance of their section's own GPU test (nca_testlib.replay_*_tol).  nca_vol_overlap_sums folds per-block
partials from its workspace in a fixed order (no atomics): bit for bit.

The table calls the C entry points through `_capi` with the current stream as their last argument, which is all `_view.launch` does; the wrapper
rows go through `_view.launch` itself.  Every Python wrapper that makes no host read is a row as well (its outputs, its workspace and -- for the
three accumulating entry points -- its own torch.zeros land in the graph's pool): export._query_points, export.normalize_images,
ccta.gaussian_filter, ccta.vesselness, drr.project_rays forward and backward, drr.total_variation, metrics.ssim with a tensor data_range,
metrics.distance_transform, metrics.soft_skeleton, metrics.label.  Wrappers that cannot be captured whole, and the host read that says so:
phantom.voxelize uploads its tables from host arrays (torch.from_numpy(...).to(device): a host-to-device copy, not a read); mesh.isosurface reads nca_vol_iso_count's totals back (totals.cpu().tolist()) to
size the emit's buffers; metrics.component_sizes reads int(counts.max()) to size its table; export.view_rays only packs host geometry around
nca_view_rays, which is a row.

An entry point whose arguments are host values only (nca_view_rays) has no device input: its three replays must reproduce the same rays over
poison.  nca_vol_iso_count and nca_vol_iso_emit are two graphs with the host's read of the totals between them; the emit's workspace is the
count's product, so it is an input there and is made eagerly before every replay.

NERFCA_GRAPH_REPLAY_RECORD=<file> keeps one line per case: the comparison, the worst difference seen and the seconds taken
(profiles/graph_replay.txt is the MI355X run)."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

from conftest import rel_err
from nca_testlib import (REPLAY_DRR_SHAPE, REPLAY_INPUTS, REPLAY_LABEL_CAP, REPLAY_LINE_SHAPE, REPLAY_RAYS, REPLAY_SSIM, REPLAY_THRESHOLD, REPLAY_TILE_SHAPE,
                         REPLAY_VESS_SCALE, REPLAY_VESS_SIGMAS, REPLAY_ZOOM, dev, grid_of, make_dynamic, make_static, replay_drr_rays, replay_images, replay_mlp_case,  # noqa: F401
                         replay_phantom_tables, replay_pixel_gradients, replay_ray_case, replay_ray_upstream, replay_references, replay_upstream, replay_volumes)

import drr_ref
import label_ref
import mesh_ref
import phantom_ref
import ssim_ref
import voltv_ref

pytestmark = pytest.mark.gpu

POISON = 0x7FC12345
ORDER = list(range(REPLAY_INPUTS)) + [REPLAY_INPUTS - 1]
RECORD = {}
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def record():
    """Prints one line per case when the module is done; NERFCA_GRAPH_REPLAY_RECORD=<file> keeps them."""
    yield
    lines = [f"{name:<44s} {kind:<28s} worst {worst:.3e}   {secs:6.2f} s" for name, (kind, worst, secs) in RECORD.items()]
    lines.append(f"{len(RECORD)} cases, {time.time() - T0:.1f} s for the module")
    print("\n" + "\n".join(lines))
    path = os.environ.get("NERFCA_GRAPH_REPLAY_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ----------------------------------------------------------------------------- the harness
def raw_bytes(t):
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


def poison(t):
    raw = raw_bytes(t)
    n4 = raw.numel() // 4 * 4
    raw[:n4].view(torch.int32).fill_(POISON)
    raw[n4:].fill_(0x45)


def is_poisoned(t):
    raw = raw_bytes(t)
    n4 = raw.numel() // 4 * 4
    return bool((raw[:n4].view(torch.int32) == POISON).all()) and bool((raw[n4:] == 0x45).all())


class Call:
    """One row of the table.
    inputs  {name: [REPLAY_INPUTS CPU tensors]}: the device inputs that change from replay to replay
    consts  {name: CPU tensor}: device inputs that stay
    outs    {name: (shape, dtype)}: caller-owned outputs; or None when `run` returns them (a Python wrapper allocates its own)
    works   {name: bytes}
    run(b)  enqueues the call(s) on the current stream; b holds every tensor above by name
    zero    outputs the library ADDS INTO: the sequence zeroes them first, with a fill kernel on the same stream
    tol     {output name: [per input, an array the |difference| must stay within]}; every other output is compared byte for byte
    setup(b, dev)   once per set of buffers; prepare(b, k)   eagerly before every run, outside the graph"""

    def __init__(self, inputs, run, outs=None, consts=None, works=None, zero=(), tol=None, setup=None, prepare=None):
        self.inputs, self.consts, self.outs, self.works = inputs, consts or {}, outs, works or {}
        self.run, self.zero, self.tol, self.setup, self.prepare = run, zero, tol or {}, setup, prepare
        for v in inputs.values():
            assert len(v) == REPLAY_INPUTS

    def buffers(self, dev):
        b = {n: torch.empty_like(v[0], device=dev) for n, v in self.inputs.items()}
        b.update({n: v.to(dev) for n, v in self.consts.items()})
        b.update({n: torch.empty(shape, dtype=dt, device=dev) for n, (shape, dt) in (self.outs or {}).items()})
        b.update({n: torch.empty(max(int(nb), 8), dtype=torch.uint8, device=dev) for n, nb in self.works.items()})
        if self.setup:
            self.setup(b, dev)
        return b

    def scratch_names(self):
        return list(self.outs or {}) + list(self.works)

    def load(self, b, k):
        for n, v in self.inputs.items():
            b[n].copy_(v[k])
        for n in self.scratch_names():
            poison(b[n])
        torch.cuda.synchronize()
        for n in self.scratch_names():
            assert is_poisoned(b[n]), n
        if self.prepare:
            self.prepare(b, k)

    def sequence(self, b):
        for n in self.zero:
            b[n].zero_()
        return self.run(b)


def replay_and_compare(dev, name, call):
    t0 = time.time()
    static = call.buffers(dev)
    call.load(static, 0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # the eager warm-up on a side stream
        call.sequence(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        returned = call.sequence(static)
    torch.cuda.synchronize()
    static_out = returned if call.outs is None else {n: static[n] for n in call.outs}
    assert static_out, name
    worst = 0.0
    for i, k in enumerate(ORDER):
        call.load(static, k)
        if call.outs is None:          # a wrapper's outputs live in the graph's pool: poisoned here like the caller-owned ones
            for t in static_out.values():
                poison(t)
            torch.cuda.synchronize()
            assert all(is_poisoned(t) for t in static_out.values())
        graph.replay()
        torch.cuda.synchronize()
        fresh = call.buffers(dev)
        call.load(fresh, k)
        with torch.cuda.stream(side):
            eager = call.sequence(fresh)
        side.synchronize()
        eager_out = eager if call.outs is None else {n: fresh[n] for n in call.outs}
        assert set(eager_out) == set(static_out)
        for n, want in eager_out.items():
            got = static_out[n]
            assert got.shape == want.shape and got.dtype == want.dtype, (name, n)
            assert not is_poisoned(got) or got.numel() == 0, (name, n, "replay", i, "wrote nothing")
            if n in call.tol:
                tol = torch.as_tensor(np.asarray(call.tol[n][k], dtype=np.float64)).to(dev).reshape(want.shape)
                err = (got.double() - want.double()).abs()
                assert bool(torch.isfinite(got).all()), (name, n, i)
                ratio = float(torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
                print(f"{name} {n} replay {i} (input {k}): worst |replay - eager| / tolerance = {ratio:.3e}")
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, n, "replay", i, "input", k, ratio)
            else:
                differ = int((raw_bytes(got) != raw_bytes(want)).sum())
                worst = max(worst, float(differ))
                assert differ == 0, (name, n, "replay", i, "input", k, f"{differ} bytes differ")
    kind = "tolerance (|d| / tol)" if call.tol and len(call.tol) == len(static_out) else ("bitwise + tolerance" if call.tol else "bitwise (bytes that differ)")
    RECORD[name] = (kind, worst, time.time() - t0)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _volumes(shape):
    return [_t(replay_volumes(shape, k)) for k in range(REPLAY_INPUTS)]


def _stack_call(check, fn_name, query_name, shape, args, out_shape, out_dtype, query_args=()):
    """The raw call fn(g, vol, n_vol, *args, out, work, work_bytes, stream) of a workspace-taking stack entry point (nca_testlib.gpu_stack_call)."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    g = grid_of(shape)
    nbytes = getattr(lib, query_name)(C.byref(g), 2, *query_args) if query_name else 0

    def run(b):
        getattr(_capi, check)(getattr(lib, fn_name)(C.byref(g), b["vol"].data_ptr(), 2, *args, b["out"].data_ptr(), b["work"].data_ptr() if nbytes else None, nbytes, _stream()))

    return Call({"vol": _volumes(shape)}, run, outs={"out": (out_shape, out_dtype)}, works={"work": nbytes} if nbytes else {})


# ----------------------------------------------------------------------------- the table: view
def case_view_rays(dev):
    from nerfca_amd import _capi, export, synthetic
    view = export.pack_view(synthetic.xcat_geometry(8), 60.0, -30.0)
    p0, n = 5, 50

    def run(b):
        _capi.check_view(_capi.lib().nca_view_rays(C.byref(view), p0, n, 1, b["o"].data_ptr(), b["d"].data_ptr(), _stream()))

    return Call({}, run, outs={"o": ((n, 3), torch.float64), "d": ((n, 3), torch.float64)})


def _ray_inputs():
    o, d, z, dists = replay_drr_rays()
    return ({"o": [_t(o + 0.01 * k) for k in range(REPLAY_INPUTS)], "d": [_t(d * (1.0 - 0.1 * k)) for k in range(REPLAY_INPUTS)]},
            {"z": _t(z), "dists": _t(dists)}, o.shape[0], z.shape[0])


def case_view_points(dev, wrapper=False):
    from nerfca_amd import _capi, export
    inputs, consts, R, S = _ray_inputs()

    def run(b):
        _capi.check_view(_capi.lib().nca_view_points(R, S, b["o"].data_ptr(), b["d"].data_ptr(), b["z"].data_ptr(), b["pts"].data_ptr(), _stream()))

    if wrapper:
        return Call(inputs, lambda b: {"pts": export._query_points(b["o"], b["d"], b["z"])}, consts=consts)
    return Call(inputs, run, consts=consts, outs={"pts": ((R * S, 3), torch.float32)})


def _images(n_img, n, dtype, seed):
    return [(2.16 - torch.rand(n_img, n, generator=torch.Generator().manual_seed(seed + k), dtype=torch.float64) * (1.0, 0.7, 0.45)[k]).to(dtype) for k in range(REPLAY_INPUTS)]


def case_view_compose(dev):
    from nerfca_amd import _capi
    n = 257

    def run(b):
        _capi.check_view(_capi.lib().nca_view_compose(n, 2.16, b["pix_s"].data_ptr(), b["pix_d"].data_ptr(), 1, b["pred"].data_ptr(), b["pred_s"].data_ptr(),
                                                      b["pred_d"].data_ptr(), _stream()))

    return Call({"pix_s": [x[0].contiguous() for x in _images(1, n, torch.float64, 10)], "pix_d": [x[0].contiguous() for x in _images(1, n, torch.float64, 20)]}, run,
                outs={k: ((n,), torch.float32) for k in ("pred", "pred_s", "pred_d")})


def case_image_normalize(dev, wrapper=False):
    from nerfca_amd import _capi, export
    n_img, n = 2, 257
    lib = _capi.lib()
    per = _capi.check_view(lib.nca_image_normalize_workspace(n))

    def run(b):
        _capi.check_view(lib.nca_image_normalize(n_img, n, b["img"].data_ptr(), b["out"].data_ptr(), b["minmax"].data_ptr(), b["work"].data_ptr(), per * n_img, _stream()))

    def wrapped(b):
        out, mm = export.normalize_images(b["img"])
        return {"out": out, "minmax": mm}

    inputs = {"img": _images(n_img, n, torch.float32, 30)}          # the maxima fall with the amplitude
    if wrapper:
        return Call(inputs, wrapped)
    return Call(inputs, run, outs={"out": ((n_img, n), torch.float32), "minmax": ((n_img, 2), torch.float32)}, works={"work": per * n_img})


# ----------------------------------------------------------------------------- drr, voltv, phantom, ssim
def case_drr_project(dev):
    from nerfca_amd import _capi
    o, d, z, dists = replay_drr_rays()
    R, S = o.shape[0], z.shape[0]
    desc = _capi.grid_desc(REPLAY_DRR_SHAPE, drr_ref.BOUNDS)

    def run(b):
        _capi.check_drr(_capi.lib().nca_drr_project(C.byref(desc), b["vol"].data_ptr(), 2, R, S, b["o"].data_ptr(), b["d"].data_ptr(), b["z"].data_ptr(), b["dists"].data_ptr(),
                                                    2.16, b["pix"].data_ptr(), _stream()))

    return Call({"vol": _volumes(REPLAY_DRR_SHAPE)}, run, consts={"o": _t(o), "d": _t(d), "z": _t(z), "dists": _t(dists)}, outs={"pix": ((2, R), torch.float64)})


def case_drr_backproject(dev):
    from nerfca_amd import _capi
    o, d, z, dists = replay_drr_rays()
    R, S = o.shape[0], z.shape[0]
    desc = _capi.grid_desc(REPLAY_DRR_SHAPE, drr_ref.BOUNDS)
    voxels = int(np.prod(REPLAY_DRR_SHAPE))

    def run(b):
        _capi.check_drr(_capi.lib().nca_drr_backproject(C.byref(desc), 2, R, S, b["o"].data_ptr(), b["d"].data_ptr(), b["z"].data_ptr(), b["dists"].data_ptr(),
                                                        b["g_pix"].data_ptr(), b["g_vol"].data_ptr(), _stream()))

    return Call({"g_pix": [_t(replay_pixel_gradients(k, R)) for k in range(REPLAY_INPUTS)]}, run, consts={"o": _t(o), "d": _t(d), "z": _t(z), "dists": _t(dists)},
                outs={"g_vol": ((2, voxels), torch.float64)}, zero=("g_vol",), tol={"g_vol": [t for _, t in replay_references()["drr"]]})


def case_vol_tv(dev):
    from nerfca_amd import _capi
    desc = _capi.grid_desc(REPLAY_TILE_SHAPE, drr_ref.BOUNDS)

    def run(b):
        _capi.check_vol(_capi.lib().nca_vol_tv(C.byref(desc), b["vol"].data_ptr(), 2, voltv_ref.EPS_S, voltv_ref.EPS_T, 1, b["out"].data_ptr(), _stream()))

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, outs={"out": ((2,), torch.float64)}, zero=("out",), tol={"out": [t for _, t in replay_references()["voltv"]]})


def case_vol_tv_grad(dev):
    from nerfca_amd import _capi
    desc = _capi.grid_desc(REPLAY_TILE_SHAPE, drr_ref.BOUNDS)

    def run(b):
        _capi.check_vol(_capi.lib().nca_vol_tv_grad(C.byref(desc), b["vol"].data_ptr(), 2, voltv_ref.EPS_S, voltv_ref.EPS_T, 1, b["scale"].data_ptr(), b["g"].data_ptr(), _stream()))

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, consts={"scale": torch.tensor([0.5, -2.0], dtype=torch.float64)}, outs={"g": ((2,) + REPLAY_TILE_SHAPE, torch.float32)})


def case_phantom_voxelize(dev):
    from nerfca_amd import _capi
    desc = _capi.grid_desc(REPLAY_TILE_SHAPE, phantom_ref.BOUNDS)
    tables = [replay_phantom_tables(k) for k in range(REPLAY_INPUTS)]
    n_ell, n_seg = tables[0][0].shape[1], tables[0][1].shape[1]

    def run(b):
        _capi.check_phantom(_capi.lib().nca_phantom_voxelize(C.byref(desc), 2, n_ell, b["ell"].data_ptr(), n_seg, b["seg"].data_ptr(), phantom_ref.RHO_V, 0.11, b["out"].data_ptr(),
                                                             _stream()))

    return Call({"ell": [_t(t[0]) for t in tables], "seg": [_t(t[1]) for t in tables]}, run, outs={"out": ((2,) + REPLAY_TILE_SHAPE, torch.float32)})


def _ssim_inputs():
    K, (H, W) = REPLAY_SSIM
    imgs = [replay_images(k) for k in range(REPLAY_INPUTS)]
    win = ssim_ref.gaussian(K)
    return K, H, W, {"x": [_t(i[0]) for i in imgs]}, {"y": _t(imgs[0][1]), "range": _t(imgs[0][2])}, (C.c_double * K)(*[float(w) for w in win])


def case_ssim(dev):
    from nerfca_amd import _capi
    K, H, W, inputs, consts, cwin = _ssim_inputs()

    def run(b):
        _capi.check_ssim(_capi.lib().nca_ssim(2, H, W, b["x"].data_ptr(), b["y"].data_ptr(), b["range"].data_ptr(), K, cwin, ssim_ref.K1, ssim_ref.K2, b["sum"].data_ptr(),
                                              b["map"].data_ptr(), _stream()))

    return Call(inputs, run, consts=consts, outs={"sum": ((2,), torch.float64), "map": ((2, H - K + 1, W - K + 1), torch.float32)}, zero=("sum",),
                tol={"sum": [t for _, t in replay_references()["ssim"]]})


def case_ssim_grad(dev):
    from nerfca_amd import _capi
    K, H, W, inputs, consts, cwin = _ssim_inputs()
    lib = _capi.lib()
    nbytes = lib.nca_ssim_grad_workspace(2, H, W, K)
    assert nbytes == 24 * 2 * (H - K + 1) * (W - K + 1)

    def run(b):
        _capi.check_ssim(lib.nca_ssim_grad(2, H, W, b["x"].data_ptr(), b["y"].data_ptr(), b["range"].data_ptr(), K, cwin, ssim_ref.K1, ssim_ref.K2, b["scale"].data_ptr(),
                                           b["g"].data_ptr(), b["work"].data_ptr(), nbytes, _stream()))

    return Call(inputs, run, consts=dict(consts, scale=torch.tensor([1.0, -1.5], dtype=torch.float64)), outs={"g": ((2, H, W), torch.float32)}, works={"work": nbytes})


# ----------------------------------------------------------------------------- edt, filt, resample, skel
def case_vol_edt(dev):
    return _stack_call("check_edt", "nca_vol_edt", "nca_vol_edt_workspace", REPLAY_LINE_SHAPE, (REPLAY_THRESHOLD, 0), (2,) + REPLAY_LINE_SHAPE, torch.float32)


def _smooth_args():
    from nerfca_amd import ccta
    halves = [ccta.gaussian_weights(s, r) for s, r in ((1.0, 2), (0.7, 3), (1.5, 4))]
    flat = np.concatenate(halves)
    return (C.c_int32 * 3)(*[len(h) - 1 for h in halves]), (C.c_double * flat.size)(*flat.tolist())


def case_vol_smooth(dev, wrapper=False):
    from nerfca_amd import ccta
    if wrapper:
        return Call({"vol": _volumes(REPLAY_LINE_SHAPE)}, lambda b: {"out": ccta.gaussian_filter(b["vol"], (1.0, 0.7, 1.5), radius=(2, 3, 4))})
    return _stack_call("check_filt", "nca_vol_smooth", "nca_vol_smooth_workspace", REPLAY_LINE_SHAPE, _smooth_args(), (2,) + REPLAY_LINE_SHAPE, torch.float32)


def case_vol_cityblock(dev):
    return _stack_call("check_filt", "nca_vol_cityblock", "nca_vol_cityblock_workspace", REPLAY_LINE_SHAPE, (REPLAY_THRESHOLD, 0, 1), (2,) + REPLAY_LINE_SHAPE, torch.int32)


def case_vol_spline_filter(dev):
    from nerfca_amd import _capi
    shape = REPLAY_ZOOM[0]
    g = grid_of(shape)

    def run(b):
        _capi.check_resample(_capi.lib().nca_vol_spline_filter(C.byref(g), b["vol"].data_ptr(), 2, b["out"].data_ptr(), _stream()))

    return Call({"vol": _volumes(shape)}, run, outs={"out": ((2,) + shape, torch.float64)})


def case_vol_zoom(dev):
    shape, m = REPLAY_ZOOM
    return _stack_call("check_resample", "nca_vol_zoom", "nca_vol_zoom_workspace", shape, ((C.c_int32 * 3)(*m), 3), (2,) + m, torch.float32, query_args=(3,))


def case_vol_softskel(dev):
    return _stack_call("check_skel", "nca_vol_softskel", "nca_vol_softskel_workspace", REPLAY_TILE_SHAPE, (2,), (2,) + REPLAY_TILE_SHAPE, torch.float32)


def case_vol_overlap_sums(dev):
    from nerfca_amd import _capi
    lib = _capi.lib()
    g = grid_of(REPLAY_TILE_SHAPE)
    nbytes = lib.nca_vol_overlap_sums_workspace(C.byref(g), 2)
    vols = _volumes(REPLAY_TILE_SHAPE)

    def run(b):
        _capi.check_skel(lib.nca_vol_overlap_sums(C.byref(g), b["a"].data_ptr(), b["b"].data_ptr(), 2, b["sums"].data_ptr(), b["work"].data_ptr(), nbytes, _stream()))

    return Call({"a": vols, "b": [(v > REPLAY_THRESHOLD).float() for v in vols]}, run, outs={"sums": ((2, 2), torch.float64)}, works={"work": nbytes})


# ----------------------------------------------------------------------------- label, vess, mesh
def case_vol_label(dev):
    from nerfca_amd import _capi
    lib = _capi.lib()
    g = grid_of(REPLAY_TILE_SHAPE)
    nbytes = lib.nca_vol_label_workspace(C.byref(g), 2)

    def run(b):
        _capi.check_label(lib.nca_vol_label(C.byref(g), b["vol"].data_ptr(), 2, REPLAY_THRESHOLD, 1, 0, b["labels"].data_ptr(), b["counts"].data_ptr(), b["work"].data_ptr(), nbytes,
                                            _stream()))

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, outs={"labels": ((2,) + REPLAY_TILE_SHAPE, torch.int32), "counts": ((2,), torch.int32)}, works={"work": nbytes})


def case_vol_label_sizes(dev):
    from nerfca_amd import _capi
    g = grid_of(REPLAY_TILE_SHAPE)
    labels = [_t(label_ref.label(replay_volumes(REPLAY_TILE_SHAPE, k), REPLAY_THRESHOLD, 1)[0]) for k in range(REPLAY_INPUTS)]

    def run(b):
        _capi.check_label(_capi.lib().nca_vol_label_sizes(C.byref(g), b["labels"].data_ptr(), 2, REPLAY_LABEL_CAP, b["sizes"].data_ptr(), _stream()))

    return Call({"labels": labels}, run, outs={"sizes": ((2, REPLAY_LABEL_CAP), torch.int32)})


def _vess_call(fn_name, outs, extra=lambda b: (), consts=None):
    from nerfca_amd import _capi
    g = grid_of(REPLAY_TILE_SHAPE)

    def run(b):
        _capi.check_vess(getattr(_capi.lib(), fn_name)(C.byref(g), b["vol"].data_ptr(), 2, REPLAY_VESS_SCALE, *extra(b), _stream()))

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, outs=outs, consts=consts)


def case_vol_hessian_eig(dev):
    return _vess_call("nca_vol_hessian_eig", {"eig": ((2, 3) + REPLAY_TILE_SHAPE, torch.float32)}, lambda b: (b["eig"].data_ptr(),))


def case_vol_hessian_norm_max(dev):
    return _vess_call("nca_vol_hessian_norm_max", {"norm_max": ((2,), torch.float64)}, lambda b: (b["norm_max"].data_ptr(),))


def case_vol_vesselness(dev):
    return _vess_call("nca_vol_vesselness", {"out": ((2,) + REPLAY_TILE_SHAPE, torch.float32), "index": ((2,) + REPLAY_TILE_SHAPE, torch.int32)},
                      lambda b: (0.5, 0.5, b["c"].data_ptr(), 1, 0, b["out"].data_ptr(), b["index"].data_ptr()), consts={"c": torch.tensor([2.0, 1.5], dtype=torch.float64)})


def case_ccta_vesselness(dev):
    """The whole multi-scale pipeline of the wrapper as ONE graph: per scale a smoothing (three launches), nca_vol_hessian_norm_max, two torch
    kernels for Frangi's c and nca_vol_vesselness.  The wrapper makes no host read."""
    from nerfca_amd import ccta

    def run(b):
        out, index = ccta.vesselness(b["vol"], REPLAY_VESS_SIGMAS, return_scale=True)
        return {"out": out, "index": index}

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run)


def _iso_grid():
    return grid_of(REPLAY_TILE_SHAPE, inv=mesh_ref.INV)


def case_vol_iso_count(dev):
    from nerfca_amd import _capi
    lib = _capi.lib()
    g = _iso_grid()
    nbytes = lib.nca_vol_iso_workspace(C.byref(g), 2)

    def run(b):
        _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), b["vol"].data_ptr(), 2, REPLAY_THRESHOLD, b["totals"].data_ptr(), b["work"].data_ptr(), nbytes, _stream()))

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, outs={"totals": ((2, 2), torch.int64)}, works={"work": nbytes})


def case_vol_iso_emit(dev):
    """The second of the two graphs.  The host reads the totals between them: here once per input, eagerly, before the capture; the capacities the
    emit is captured with are the largest totals of the sequence, so a replay on a smaller mesh leaves the rows past its totals as they were
    (poison, in the replay and in the eager call alike).  The workspace is the count's product: made eagerly before every run."""
    from nerfca_amd import _capi
    lib = _capi.lib()
    g = _iso_grid()
    nbytes = lib.nca_vol_iso_workspace(C.byref(g), 2)
    vols = _volumes(REPLAY_TILE_SHAPE)

    def count(b):
        poison(b["count_work"])
        _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), b["vol"].data_ptr(), 2, REPLAY_THRESHOLD, b["totals"].data_ptr(), b["count_work"].data_ptr(), nbytes, _stream()))
        torch.cuda.synchronize()
        return b["totals"].cpu().numpy()

    caps = np.zeros(2, dtype=np.int64)
    probe = {"vol": torch.empty_like(vols[0], device=dev), "totals": torch.zeros((2, 2), dtype=torch.int64, device=dev), "count_work": torch.empty(nbytes, dtype=torch.uint8, device=dev)}
    seen = []
    for v in vols:
        probe["vol"].copy_(v)
        tot = count(probe)
        seen.append(tot.sum(axis=0))
        caps = np.maximum(caps, tot.sum(axis=0))
    assert (caps > 0).all() and len({tuple(s) for s in seen}) == REPLAY_INPUTS, seen          # meshes of three different sizes
    vert_cap, tri_cap = int(caps[0]), int(caps[1])

    def setup(b, dev):
        b["totals"] = torch.zeros((2, 2), dtype=torch.int64, device=dev)
        b["count_work"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run(b):
        _capi.check_mesh(lib.nca_vol_iso_emit(C.byref(g), b["vol"].data_ptr(), 2, REPLAY_THRESHOLD, b["count_work"].data_ptr(), nbytes, vert_cap, tri_cap, b["verts"].data_ptr(),
                                              b["tris"].data_ptr(), b["normals"].data_ptr(), _stream()))

    return Call({"vol": vols}, run, outs={"verts": ((vert_cap, 3), torch.float32), "tris": ((tri_cap, 3), torch.int32), "normals": ((vert_cap, 3), torch.float32)},
                setup=setup, prepare=lambda b, k: count(b))


# ----------------------------------------------------------------------------- the general kernels
def case_mlp_bwd(dev):
    """nca_mlp_bwd on the one-hot module's general point case (144 units, 300 points): wide_backward clears `grads` and accumulates over chunks."""
    from nerfca_amd import _capi
    spec, params, x, _ = replay_mlp_case()
    model = make_static(params, dev, F=spec.num_filters, early=spec.num_early_layers, late=spec.num_late_layers)
    model.update_freq_mask_alpha(75000, 150000)
    bnd = model._binding
    assert _capi.net_is_general(bnd.net) and bnd.net.F == 144
    lib = _capi.lib()
    N = x.shape[0]
    keep = dict(model=model, packed=bnd.ensure_packed(), enc=model._enc_buffers())
    torch.cuda.synchronize()
    nbytes = _capi.check(lib.nca_mlp_bwd_workspace(C.byref(bnd.net), bnd.prec, N, 0))
    assert nbytes > 0

    def run(b):
        win, four = keep["enc"]
        _capi.check(lib.nca_mlp_bwd(C.byref(bnd.net), bnd.prec, _capi.ptr(keep["packed"]), _capi.ptr(win), _capi.ptr(four), _capi.ptr(bnd.flat), N, b["pts"].data_ptr(), None,
                                    b["g_raw"].data_ptr(), b["grads"].data_ptr(), None, b["work"].data_ptr(), nbytes, _stream()))

    return Call({"g_raw": [replay_upstream(k, (N, 1)).contiguous() for k in range(REPLAY_INPUTS)]}, run, consts={"pts": x.contiguous()},
                outs={"grads": ((bnd.flat.numel(),), torch.float32)}, works={"work": nbytes})


def case_render(dev, store):
    """nca_render_fwd + nca_render_bwd, both nets on the general kernels, as one captured sequence: with the forward store (the backward recomputes
    nothing; the forward copies the raw fields into the store) and without one (what fused.STORE_FORWARD_LIMIT_BYTES = 0 runs: the backward
    recomputes per run of whole rays).  Both clear the gradients and accumulate into them."""
    from nerfca_amd import _capi, fused
    c = replay_ray_case()
    R, S = REPLAY_RAYS
    s = make_static(c["ps"], dev, F=144, early=1, late=0)
    t = make_dynamic(c["pd"], dev, F=144, early=1, late=0, T=8)
    for m in (s, t):
        m.update_freq_mask_alpha(75000, 150000)
    bs, bd = s._binding, t._binding
    assert _capi.net_is_general(bs.net) and _capi.net_is_general(bd.net)
    batch = fused._RayBatch(c["o"].to(dev), c["d"].to(dev), c["ph"].to(dev), c["I0"].to(dev), c["z"].to(dev), c["dists"].to(dev), "softplus", False, 1e-2)
    lib = _capi.lib()
    packed_s, packed_d = fused.FieldBinding.ensure_packed_pair(bs, bd)
    (win_s, four_s), (win_d, four_d) = s._enc_buffers(), t._enc_buffers()
    torch.cuda.synchronize()
    keep = (s, t, batch, packed_s, packed_d, win_s, four_s, win_d, four_d)
    desc = batch.desc()
    fbytes = _capi.check(lib.nca_render_fwd_workspace_nets(C.byref(desc), C.byref(bs.net), C.byref(bd.net), bs.prec, 0))
    sbytes = _capi.check(lib.nca_render_store_bytes(C.byref(desc), C.byref(bs.net), C.byref(bd.net), bs.prec)) if store else 0
    assert fbytes > 0 and (sbytes > 0) == store
    bdesc = batch.desc(store_format=_capi.STORE_GENERAL if store else 0)
    bbytes = _capi.check(lib.nca_render_bwd_workspace(C.byref(bdesc), C.byref(bs.net), C.byref(bd.net), bs.prec, 1 << 28))          # (a byte cap, as fused passes one: all rays in one run)
    p = _capi.ptr

    def run(b):
        assert keep
        fmt = _capi.check(lib.nca_render_fwd(C.byref(desc), bs.prec, C.byref(bs.net), p(packed_s), p(win_s), p(four_s), C.byref(bd.net), p(packed_d), p(win_d), p(four_d), p(bd.flat),
                                             b["pix"].data_ptr(), b["sig_s"].data_ptr(), b["sig_d"].data_ptr(), b["fwork"].data_ptr(), fbytes,
                                             b["store"].data_ptr() if store else None, sbytes, _stream()))
        assert fmt == (_capi.STORE_GENERAL if store else _capi.STORE_NONE), fmt
        _capi.check(lib.nca_render_bwd(C.byref(bdesc), bs.prec, C.byref(bs.net), p(packed_s), p(win_s), p(four_s), p(bs.flat), C.byref(bd.net), p(packed_d), p(win_d), p(four_d),
                                       p(bd.flat), b["g_pix"].data_ptr(), b["g_s"].data_ptr(), b["g_d"].data_ptr(), b["grads_s"].data_ptr(), b["grads_d"].data_ptr(),
                                       b["bwork"].data_ptr(), bbytes, b["store"].data_ptr() if store else None, sbytes, _stream()))

    ups = [replay_ray_upstream(k) for k in range(REPLAY_INPUTS)]
    works = {"fwork": fbytes, "bwork": bbytes}
    if store:
        works["store"] = sbytes
    return Call({"g_pix": [u[0] for u in ups], "g_s": [u[1] for u in ups], "g_d": [u[2] for u in ups]}, run,
                outs={"pix": ((R,), torch.float64), "sig_s": ((R, S), torch.float32), "sig_d": ((R, S), torch.float32), "grads_s": ((bs.flat.numel(),), torch.float32),
                      "grads_d": ((bd.flat.numel(),), torch.float32)}, works=works)


# ----------------------------------------------------------------------------- the Python wrappers of the accumulating and the stack entry points
F32_STEP = 2.0 ** -23          # one step of f32 at a value's own size: what a wrapper's rounding of an f64 result to f32 may add to a difference


def case_drr_project_rays(dev, backward=False):
    """drr.project_rays: the forward launch; or, with `backward`, the autograd path -- forward and backward captured as one sequence, the backward's
    torch.zeros of the f64 buffer and nca_drr_backproject into it, returned as f32: the section's tolerance plus one f32 step of the gradient."""
    from nerfca_amd import drr
    o, d, z, dists = replay_drr_rays()
    R = o.shape[0]
    consts = {"o": _t(o), "d": _t(d), "z": _t(z), "dists": _t(dists)}
    if not backward:
        return Call({"vol": _volumes(REPLAY_DRR_SHAPE)}, lambda b: {"pix": drr.project_rays(b["vol"], b["o"], b["d"], b["z"], b["dists"], i0=2.16, bounds=drr_ref.BOUNDS)},
                    consts=consts)

    def run(b):
        vol = b["vol"].detach().requires_grad_()
        pix = drr.project_rays(vol, b["o"], b["d"], b["z"], b["dists"], i0=2.16, bounds=drr_ref.BOUNDS)
        return {"g_vol": torch.autograd.grad(pix, vol, b["g_pix"])[0].contiguous()}

    refs = replay_references()["drr"]
    tol = [(t + F32_STEP * np.abs(g)).reshape((2,) + REPLAY_DRR_SHAPE) for g, t in refs]
    return Call({"g_pix": [_t(replay_pixel_gradients(k, R)) for k in range(REPLAY_INPUTS)]}, run, consts=dict(consts, vol=_volumes(REPLAY_DRR_SHAPE)[0]), tol={"g_vol": tol})


def case_drr_total_variation(dev):
    """drr.total_variation: torch.zeros(2), nca_vol_tv into it, the two divisions by the counts.  The section's tolerance of the sums over the same
    counts, plus one f64 step of the quotient."""
    from nerfca_amd import drr
    voxels = int(np.prod(REPLAY_TILE_SHAPE))
    counts = np.array([2 * voxels, 2 * voxels], dtype=np.float64)          # two volumes; cyclic with two volumes carries its pair twice
    tol = [t / counts + 2.0 ** -52 * np.abs(v / counts) for v, t in replay_references()["voltv"]]

    def run(b):
        space, time_ = drr.total_variation(b["vol"], bounds=drr_ref.BOUNDS, eps_space=voltv_ref.EPS_S, eps_time=voltv_ref.EPS_T, cyclic=True)
        return {"tv": torch.stack([space, time_])}

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run, tol={"tv": tol})


def case_metrics_ssim(dev):
    """metrics.ssim with a tensor data_range and full=True: torch.zeros(N), nca_ssim into it, the division by the number of positions."""
    from nerfca_amd import metrics
    K, H, W, inputs, consts, _ = _ssim_inputs()
    count = float((H - K + 1) * (W - K + 1))
    tol = [t / count + 2.0 ** -52 * np.abs(v / count) for v, t in replay_references()["ssim"]]

    def run(b):
        mean, smap = metrics.ssim(b["x"], b["y"], data_range=b["range"], win_size=K, full=True)
        return {"mean": mean, "map": smap}

    return Call(inputs, run, consts=consts, tol={"mean": tol})


def case_metrics_stack(dev, which):
    from nerfca_amd import metrics
    if which == "distance_transform":
        return Call({"vol": _volumes(REPLAY_LINE_SHAPE)}, lambda b: {"out": metrics.distance_transform(b["vol"], drr_ref.BOUNDS, threshold=REPLAY_THRESHOLD)})
    if which == "soft_skeleton":
        return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, lambda b: {"out": metrics.soft_skeleton(b["vol"], 2)})

    def run(b):
        labels, counts = metrics.label(b["vol"], threshold=REPLAY_THRESHOLD)
        return {"labels": labels, "counts": counts}

    return Call({"vol": _volumes(REPLAY_TILE_SHAPE)}, run)


CASES = {
    "nca_view_rays": case_view_rays, "nca_view_points": case_view_points, "nca_view_compose": case_view_compose, "nca_image_normalize": case_image_normalize,
    "nca_drr_project": case_drr_project, "nca_drr_backproject": case_drr_backproject, "nca_vol_tv": case_vol_tv, "nca_vol_tv_grad": case_vol_tv_grad,
    "nca_phantom_voxelize": case_phantom_voxelize, "nca_ssim": case_ssim, "nca_ssim_grad": case_ssim_grad, "nca_vol_edt": case_vol_edt, "nca_vol_smooth": case_vol_smooth,
    "nca_vol_cityblock": case_vol_cityblock, "nca_vol_spline_filter": case_vol_spline_filter, "nca_vol_zoom": case_vol_zoom, "nca_vol_softskel": case_vol_softskel,
    "nca_vol_overlap_sums": case_vol_overlap_sums, "nca_vol_label": case_vol_label, "nca_vol_label_sizes": case_vol_label_sizes, "nca_vol_hessian_eig": case_vol_hessian_eig,
    "nca_vol_hessian_norm_max": case_vol_hessian_norm_max, "nca_vol_vesselness": case_vol_vesselness, "nca_vol_iso_count": case_vol_iso_count,
    "nca_vol_iso_emit": case_vol_iso_emit,
    # the Python wrappers that make no host read (their outputs are allocated inside the capture, in the graph's pool)
    "export._query_points": lambda dev: case_view_points(dev, wrapper=True), "export.normalize_images": lambda dev: case_image_normalize(dev, wrapper=True),
    "ccta.gaussian_filter": lambda dev: case_vol_smooth(dev, wrapper=True), "ccta.vesselness (two scales, one graph)": case_ccta_vesselness,
    "drr.project_rays": case_drr_project_rays, "drr.project_rays backward (autograd)": lambda dev: case_drr_project_rays(dev, backward=True),
    "drr.total_variation": case_drr_total_variation, "metrics.ssim (tensor data_range)": case_metrics_ssim,
    "metrics.distance_transform": lambda dev: case_metrics_stack(dev, "distance_transform"), "metrics.soft_skeleton": lambda dev: case_metrics_stack(dev, "soft_skeleton"),
    "metrics.label": lambda dev: case_metrics_stack(dev, "label"),
    # the general (wide) kernels
    "nca_mlp_bwd (144 units, 300 points)": case_mlp_bwd, "nca_render_fwd + nca_render_bwd (general, store)": lambda dev: case_render(dev, True),
    "nca_render_fwd + nca_render_bwd (general, no store)": lambda dev: case_render(dev, False),
}


@pytest.mark.parametrize("name", list(CASES), ids=lambda n: n.replace(" ", "_"))
def test_replay_equals_eager(dev, name):
    with torch.cuda.device(dev):
        replay_and_compare(dev, name, CASES[name](dev))


def test_the_sequences_are_those_of_the_cpu_half(dev):
    """What tests/test_graph_replay_cpu.py proves about the sequences holds for the library too: the eager results of the accumulating outputs ARE
    the references' (bit for bit where they are integers or maxima), so the stale values modelled there are the ones a dead clear would give."""
    ref = replay_references()
    for k in range(REPLAY_INPUTS):
        for name, key, out in (("nca_vol_hessian_norm_max", "norm_max", "norm_max"), ("nca_vol_label_sizes", "sizes", "sizes")):
            call = CASES[name](dev)
            b = call.buffers(dev)
            call.load(b, k)
            with torch.cuda.device(dev):
                call.sequence(b)
            torch.cuda.synchronize()
            assert np.array_equal(b[out].cpu().numpy(), ref[key][k]), (name, k)


# ----------------------------------------------------------------------------- the trainer
def test_trainer_graph_steps_with_general_nets_equal_eager_gradients(dev):
    """CompositeTrainer.step_graph over nets of 136 units (general kernels, width 144), the configuration of test_trainer_steps_with_wide_nets, in the
    manner of test_graph_step_survives_allocator_churn and with every scratch buffer poisoned: before each of four replays a reference trainer's
    eager fused_gradients at the graph trainer's current weights; the replay's loss terms within rel_err < 1e-6 of them (the bound of the churn
    test: the two paths build the interval lengths with different torch ops) -- and, what the loss terms cannot show, the GRADIENTS the replay left
    in the step's flat buffer against the eager ones at rel_err < 1e-5, the project's f32 parity bound (tests/test_hip_parity.py): the same kernels
    sum in the same order on both paths, only the interval lengths differ in their last f32 bit, while gradients that accumulate over replays are
    off by their own size."""
    from nerfca_amd import _capi, fused, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    from nerfca_amd.train.trainer import CompositeTrainer, TrainConfig
    t0 = time.time()
    data = synthetic.make_dataset(16, 48, dev, views=synthetic.TRAIN_VIEWS[:2], n_phases=3, F=32)

    def trainer():
        torch.manual_seed(5)
        sdef, tdef = synthetic.net_definitions(dev, F=136)
        s, t = CPPN(sdef).to(dev), Temporal(tdef).to(dev)
        return CompositeTrainer(TrainConfig(depth_samples_per_ray_coarse=48, img_sample_size=160), s, t, data, dev, seed=3)

    old = fused.POISON_BUFFERS
    fused.POISON_BUFFERS = True
    worst = 0.0
    try:
        tr, ref = trainer(), trainer()
        for m in (tr.s, tr.t):
            assert _capi.net_is_general(m._binding.net) and m._binding.net.F == 144
        n_grad = sum(b.flat.numel() for b in (tr.t._binding, tr.s._binding))
        for it in range(4):
            with torch.no_grad():
                for pr, pg in zip(ref.params, tr.params):
                    pr.copy_(pg)
            terms, gs, gd = ref.fused_gradients(1000 + it)
            want_terms, want_grad = terms.clone(), torch.cat([gd.flatten(), gs.flatten()]).clone()          # the flat buffer's order: self.params, dynamic net first
            got_terms = tr.step_graph(1000 + it)[2].clone()
            got_grad = tr._flat[:n_grad].clone()
            assert want_grad.numel() == n_grad and bool(torch.isfinite(got_terms).all()) and bool(torch.isfinite(got_grad).all()), it
            e_t, e_g = rel_err(got_terms, want_terms), rel_err(got_grad, want_grad)
            print(f"replay {it}: rel_err of the loss terms {e_t:.3e}, of the gradients {e_g:.3e}")
            worst = max(worst, e_t, e_g)
            assert e_t < 1e-6, (it, got_terms, want_terms)
            assert e_g < 1e-5, (it, e_g)
            assert float(want_grad.abs().max()) > 0
    finally:
        fused.POISON_BUFFERS = old
    RECORD["CompositeTrainer.step_graph (136 units)"] = ("rel_err: terms 1e-6, grads 1e-5", worst, time.time() - t0)
