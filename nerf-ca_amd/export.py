"""Checkpoint loading, 4-D field export and view rendering around the fused kernels.

The reference only *saves* checkpoints (``CPPN.save`` / ``Temporal.save``, model/CPPN.py:164-180) and leaves
sampling the trained fields on a grid to downstream scripts; these helpers close that loop for users of the
drop-in modules.  Field evaluation goes through ``fused.eval_points`` (the HIP kernel), in chunks.

``render_view`` / ``render_sequence`` render any C-arm view at any heart phase from a pair of nets alone (no trainer, no
dataset): rays are generated on the device per chunk (``nca_view_rays``), the static field is rendered ONCE per view and
the dynamic field once per (view, phase), and ``nca_view_compose`` turns the two single-field images into the composite /
static / dynamic images the reference's display block logs (train/run_composite.py:361, 405-413).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from . import _view
from . import fused as _fused
from . import mesh as _mesh
from .fused import eval_points


def load_checkpoint(filename, device=None):
    """Rebuild the model a ``save()`` call wrote: returns ``(model, training_information)``.

    The blob holds the constructor dictionary under ``"parameters"`` (with the device it was trained on), the
    state dict under ``"model"`` and, for windowed encodings, ``windowed_alpha`` / ``freq_mask_alpha``.  A blob with a
    ``time_latents`` entry (or ``num_time_dim`` in its parameters) is a ``Temporal``, anything else a ``CPPN``."""
    from .model.CPPN import CPPN
    from .model.Temporal import Temporal
    blob = torch.load(filename, map_location="cpu", weights_only=False)
    params = dict(blob["parameters"])
    if device is not None:
        params["device"] = device
    if params.get("fourier_gaussian") is not None:
        params["fourier_gaussian"] = params["fourier_gaussian"].to("cpu")
    is_temporal = "time_latents" in blob["model"] or "num_time_dim" in params
    model = (Temporal if is_temporal else CPPN)(params)
    model.load_state_dict(blob["model"])
    if "windowed_alpha" in blob:
        model.windowed_alpha = blob["windowed_alpha"]
    if "freq_mask_alpha" in blob:
        model.freq_mask_alpha = blob["freq_mask_alpha"]
    if device is not None:
        model = model.to(device)
    return model, blob.get("training_information", {})


@torch.no_grad()
def density_volume(static_model, temp_model, phase: Optional[int], resolution: Sequence[int] = (128, 128, 128),
                   bounds: Tuple[Tuple[float, float], ...] = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), output_activation: str = "softplus",
                   scale_value: float = 1e-2, chunk_points: int = 1 << 22):
    """Sample the trained fields on a regular grid: returns ``(sigma_static, sigma_dynamic | None)`` as f32
    ``[nx, ny, nz]`` tensors on the models' device, ``sigma = act(raw) * scale_value`` as in
    render_volume_density_composite (model_helpers.py:72-84).  ``phase`` selects the heart phase of the dynamic field
    (one 3-D volume per phase = the 4-D reconstruction); ``temp_model=None`` exports the static field only."""
    dev = next(static_model.parameters()).device
    axes = [torch.linspace(lo, hi, n, device=dev) for (lo, hi), n in zip(bounds, resolution)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    out_s = torch.empty(grid.shape[0], dtype=torch.float32, device=dev)
    out_d = torch.empty_like(out_s) if temp_model is not None else None
    line = 256                                                   # grid points are handed to the compositing kernel as rows of 256
    i0 = torch.zeros(1, dtype=torch.float32, device=dev)
    dz = torch.zeros(line, dtype=torch.float64, device=dev)      # only the activation is wanted here, not the line integral
    for i in range(0, grid.shape[0], chunk_points):
        pts = grid[i:i + chunk_points]
        n = pts.shape[0]
        pad = (-n) % line
        raw_s = torch.nn.functional.pad(eval_points(static_model, pts)[:, 0], (0, pad)).reshape(-1, line)
        if temp_model is not None:
            ph = torch.full((n,), int(phase), dtype=torch.int32, device=dev)
            raw_d = torch.nn.functional.pad(eval_points(temp_model, pts, ph)[:, 0], (0, pad)).reshape(-1, line)
            _, ss, sd = _fused.composite_raw(raw_s, raw_d, i0, dz, output_activation, False, scale_value, False)
            out_d[i:i + n] = sd.reshape(-1)[:n]
        else:                                                    # one field: the kernel's single mode returns sigma un-scaled,
            _, ss, _ = _fused.composite_raw(raw_s, raw_s, i0, dz, output_activation, False, scale_value, False)   # so use the scaled pair mode
        out_s[i:i + n] = ss.reshape(-1)[:n]
    shape = tuple(int(n) for n in resolution)
    return out_s.reshape(shape), (out_d.reshape(shape) if out_d is not None else None)


@torch.no_grad()
def density_volumes(static_model, temp_model, phases: Sequence[int], resolution: Sequence[int] = (128, 128, 128),
                    bounds: Tuple[Tuple[float, float], ...] = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), output_activation: str = "softplus",
                    scale_value: float = 1e-2, chunk_points: int = 1 << 22):
    """``density_volume`` for a list of heart phases with the static field sampled once: returns ``(sigma_static [nx,ny,nz],
    sigma_dynamic [P,nx,ny,nz] | None)``, each volume equal bit for bit to what ``density_volume`` returns for that phase."""
    dev = next(static_model.parameters()).device
    axes = [torch.linspace(lo, hi, n, device=dev) for (lo, hi), n in zip(bounds, resolution)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    phases = [int(p) for p in phases]
    out_s = torch.empty(grid.shape[0], dtype=torch.float32, device=dev)
    out_d = torch.empty((len(phases), grid.shape[0]), dtype=torch.float32, device=dev) if temp_model is not None else None
    line = 256                                                   # as density_volume: rows of 256 for the compositing kernel
    i0 = torch.zeros(1, dtype=torch.float32, device=dev)
    dz = torch.zeros(line, dtype=torch.float64, device=dev)

    def sigma(raw, n):       # act(raw) * scale_value through the compositing kernel's scaled pair mode
        raw = torch.nn.functional.pad(raw[:, 0], (0, (-n) % line)).reshape(-1, line)
        return _fused.composite_raw(raw, raw, i0, dz, output_activation, False, scale_value, False)[1].reshape(-1)[:n]

    for i in range(0, grid.shape[0], chunk_points):
        pts = grid[i:i + chunk_points]
        n = pts.shape[0]
        out_s[i:i + n] = sigma(eval_points(static_model, pts), n)
        if temp_model is not None:
            ph = torch.empty(n, dtype=torch.int32, device=dev)
            for j, phase in enumerate(phases):
                out_d[j, i:i + n] = sigma(eval_points(temp_model, pts, ph.fill_(phase)), n)
    shape = tuple(int(n) for n in resolution)
    return out_s.reshape(shape), (out_d.reshape((len(phases),) + shape) if out_d is not None else None)


@torch.no_grad()
def density_surfaces(static_model, temp_model, phases: Sequence[int], level: float, resolution: Sequence[int] = (128, 128, 128),
                     bounds: Tuple[Tuple[float, float], ...] = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), output_activation: str = "softplus",
                     scale_value: float = 1e-2, chunk_points: int = 1 << 22, *, field: str = "dynamic", normals: bool = False) -> "List[_mesh.Mesh]":
    """The 4-D reconstruction as surfaces: one ``mesh.Mesh`` per heart phase of ``phases``, the iso-surface at ``level`` of the density
    sampled by ``density_volumes`` (same arguments) -- of the dynamic field (``field="dynamic"``, the vessels), of the sum of both fields
    (``"total"``), or, as a list of one, of the static field (``"static"``; ``temp_model`` may then be None).  Vertices are in the
    coordinates of ``bounds``.  One ``density_volumes`` and one ``mesh.isosurface`` over the stack: one host read in all."""
    who = "density_surfaces"
    if field not in ("dynamic", "total", "static"):
        raise _capi.NcaError(f"{who}: field = {field!r} is not 'dynamic', 'total' or 'static'")
    if field != "static" and temp_model is None:
        raise _capi.NcaError(f"{who}: field = {field!r} needs the dynamic model")
    sig_s, sig_d = density_volumes(static_model, temp_model if field != "static" else None, phases, resolution, bounds, output_activation, scale_value, chunk_points)
    stack = sig_s[None] if field == "static" else (sig_d if field == "dynamic" else sig_d + sig_s[None])
    return _mesh.isosurface(stack, level, bounds, normals=normals)


# ----------------------------------------------------------------------------- view rendering
def pack_view(geo: dict, theta: float, phi: float, larm: float = 0) -> "_capi.NcaView":
    """The NcaView of one projection: the f32 3x4 [R | t] of ``source_matrix_tigre([0, 0, -DSO], theta, phi, larm)`` and the
    detector of ``geo`` (the dict ``TrainingData.geo`` / ``synthetic.*_geometry`` use), rounded to f32 where
    ``proj_helpers.get_ray_values_tigre`` rounds."""
    from .train.proj_helpers import source_matrix_tigre
    pose = np.asarray(source_matrix_tigre(np.array([0, 0, -geo["DSO"]]), theta, phi, larm), dtype=np.float64).astype(np.float32)[:3, :4]
    W, H = (int(v) for v in geo["nDetector"])
    return _capi.NcaView(pose=(C.c_float * 12)(*pose.reshape(-1).tolist()), W=W, H=H, d_det=(C.c_float * 2)(*geo["dDetector"]),
                         off_det=(C.c_float * 2)(*geo["offDetector"]), dsd=float(geo["DSD"]))


def chunk_plan(n_pixels: int, chunk_rays: int) -> List[Tuple[int, int]]:
    """``(p0, n)`` pieces of at most ``chunk_rays`` pixels that cover ``[0, n_pixels)`` exactly once, in order."""
    if n_pixels <= 0 or chunk_rays <= 0:
        raise ValueError("n_pixels and chunk_rays must be positive")
    return [(p0, min(chunk_rays, n_pixels - p0)) for p0 in range(0, n_pixels, chunk_rays)]


def _rays_of(view: "_capi.NcaView", p0: int, n: int, device, dtype):
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("rays are float32 or float64")
    origins = torch.empty((n, 3), dtype=dtype, device=device)
    dirs = torch.empty((n, 3), dtype=dtype, device=device)
    _view.launch(_capi.check_view, _capi.lib().nca_view_rays, origins.device, C.byref(view), p0, n, 1 if dtype == torch.float64 else 0, _capi.ptr(origins),
                 _capi.ptr(dirs))
    return origins, dirs


def view_rays(geo: dict, theta: float, phi: float, larm: float = 0, p0: int = 0, n: Optional[int] = None, device="cuda", dtype=torch.float64):
    """Origins and directions ``[n,3]`` of the pixels ``p = w*H + h`` in ``[p0, p0+n)`` of one projection, generated on the device
    (``nca_view_rays``): ``proj_helpers.get_ray_values_tigre`` without the host geometry and the upload.  The values are f32 as
    there; ``dtype=torch.float64`` (the ray table's type) holds the same values widened."""
    view = pack_view(geo, theta, phi, larm)
    device = torch.device(device)
    if device.type != "cuda":
        raise _capi.NcaError("view_rays generates rays on the GPU: device must be a cuda device")
    if n is None:
        n = view.W * view.H - p0
    return _rays_of(view, int(p0), int(n), device, dtype)


def compose_images(pix_s: torch.Tensor, pix_d: Optional[torch.Tensor], i0: float, pred: torch.Tensor, pred_s: torch.Tensor, pred_d: torch.Tensor) -> None:
    """``nca_view_compose`` into caller-owned contiguous f32 ``[n]`` buffers: ``pred = f32((pix_s + pix_d) - i0)`` in f64,
    ``pred_s = f32(pix_s)``, ``pred_d = f32(pix_d)``; ``pix_d=None``: ``pred = pred_s``, ``pred_d = f32(i0)``."""
    _fused._require_cuda(pix_s, "single-field images")
    n = pix_s.numel()
    for t in (pix_s, pix_d, pred, pred_s, pred_d):
        if t is not None and (not t.is_contiguous() or t.numel() != n or t.device != pix_s.device):
            raise _capi.NcaError("compose_images takes contiguous tensors of one length on one device")
    if pix_s.dtype not in (torch.float32, torch.float64) or (pix_d is not None and pix_d.dtype != pix_s.dtype):
        raise _capi.NcaError("pix_s and pix_d are both float32 or both float64")
    if any(t.dtype != torch.float32 for t in (pred, pred_s, pred_d)):
        raise _capi.NcaError("the output images are float32")
    _view.launch(_capi.check_view, _capi.lib().nca_view_compose, pix_s.device, n, float(i0), _capi.ptr(pix_s), _capi.ptr(pix_d),
                 1 if pix_s.dtype == torch.float64 else 0, _capi.ptr(pred), _capi.ptr(pred_s), _capi.ptr(pred_d))


_NORM_IMAGES_PER_CALL = 65535


def normalize_images(img: torch.Tensor, want_out: bool = True):
    """Per-image ``(x - min) / (max - min)`` of f32 ``[n_img, ...]`` images (``nca_image_normalize``): returns ``(normalised |
    None, minmax [n_img, 2])``.  What ``trainer.normalize_image`` does before logging, except that a constant image gives
    zeros, not NaN."""
    _fused._require_cuda(img, "images")
    if img.dtype != torch.float32 or img.dim() < 2 or img.numel() == 0:
        raise _capi.NcaError("normalize_images takes non-empty float32 images [n_img, ...]")
    lib = _capi.lib()
    x = img.contiguous().reshape(img.shape[0], -1)
    n_img, n = x.shape
    out = torch.empty_like(x) if want_out else None
    minmax = torch.empty((n_img, 2), dtype=torch.float32, device=x.device)
    per = _capi.check_view(lib.nca_image_normalize_workspace(n))
    for i in range(0, n_img, _NORM_IMAGES_PER_CALL):
        k = min(_NORM_IMAGES_PER_CALL, n_img - i)
        work = _fused._scratch(per * k, x.device)
        _view.launch(_capi.check_view, lib.nca_image_normalize, x.device, k, n, _capi.ptr(x[i:]), _capi.ptr(out[i:]) if want_out else None, _capi.ptr(minmax[i:]),
                     _capi.ptr(work), per * k)
    return (out.reshape(img.shape) if want_out else None), minmax


def _render_static_chunk(static_model, origins, dirs, I0, z, dists, act: str, scale: float) -> torch.Tensor:
    """pix f64[n] of the static field alone on one ray chunk: the fused single-field render."""
    return _fused.render_rays(static_model, None, origins, dirs, None, I0, z, dists, act=act, single=True, scale=scale)[0]


def _query_points(origins, dirs, z) -> torch.Tensor:
    """f32 ``[R*S,3]`` query points of f64 rays ``[R,3]`` at the depths ``z`` f32 ``[S]`` (``nca_view_points``)."""
    if origins.dtype != torch.float64 or dirs.dtype != torch.float64 or z.dtype != torch.float32:
        raise _capi.NcaError("query points are made from float64 rays and float32 depths")
    R, S = origins.shape[0], z.shape[0]
    pts = torch.empty((R * S, 3), dtype=torch.float32, device=origins.device)
    _view.launch(_capi.check_view, _capi.lib().nca_view_points, origins.device, R, S, _capi.ptr(origins), _capi.ptr(dirs), _capi.ptr(z), _capi.ptr(pts))
    return pts


def _render_dynamic_chunk(temp_model, pts, phase_ids, I0, dists, act: str, scale: float) -> torch.Tensor:
    """pix f64[n] of the dynamic field alone at one phase.  ``nca_render_fwd`` binds time latents to its second net only, so a dynamic
    net does not run there in single-field mode, whatever its width: it is evaluated on the chunk's query points by the point forward
    (fused or general kernels, the model's precision) and summed by the compositing kernel in single-field mode, in place."""
    R = I0.shape[0]
    raw = eval_points(temp_model, pts, phase_ids)
    pix = torch.empty(R, dtype=torch.float64, device=pts.device)
    _capi.check(_capi.lib().nca_composite_fwd(R, raw.shape[0] // R, _fused.act_code(act), 1, float(scale), _capi.ptr(raw), None, _capi.ptr(I0),
                                              _capi.ptr(dists), _capi.ptr(pix), _capi.ptr(raw), None, _fused._stream()))
    return pix


@torch.no_grad()
def render_sequence(static_model, temp_model, geo: dict, views: Sequence[Sequence[float]], phases: Optional[Sequence[int]], samples: int, *,
                    z: Optional[torch.Tensor] = None, output_activation: str = "softplus", scale_value: float = 1e-2, chunk_rays: int = 65536,
                    normalize: bool = False) -> dict:
    """Render every view ``(theta, phi[, larm])`` of ``views`` at every heart phase of ``phases``: f32 images ``pred`` and
    ``pred_dynamic`` ``[V,P,W,H]`` and ``pred_static`` ``[V,W,H]`` on the models' device -- the composite image and the image each
    field renders on its own, un-normalised ``I0 - sum sigma dists`` (run_composite.py:361, 407-413).

    Per view and ray chunk the static field is rendered once and the dynamic field once per phase on the same rays: P + 1 net passes
    where a composite render per frame takes 2 P.  The models are used as they are: their precision (``set_precision``) and their
    encoding windows (``load_checkpoint`` restores them).  ``z`` defaults to the un-jittered ``create_depth_values(near, far,
    samples)``, so the output is deterministic; ``I0 = geo["max_pixel_value"]``.  ``temp_model=None`` renders the static field
    alone (``phases`` is ignored, P = 1, ``pred = pred_static`` and ``pred_dynamic`` is ``I0`` everywhere).  ``normalize=True`` adds
    ``pred_norm`` / ``pred_static_norm`` / ``pred_dynamic_norm`` (per frame, ``normalize_images``) and ``minmax``, a dict of the
    frames' ``(min, max)`` under the three image names."""
    from .train.data_helpers import create_depth_values
    from .train.model_helpers import _interval_lengths
    dev = next(static_model.parameters()).device
    if dev.type != "cuda":
        raise _capi.NcaError("render_sequence needs the models on the GPU")
    views = [tuple(float(a) for a in v) for v in views]
    if not views or any(len(v) not in (2, 3) for v in views):
        raise ValueError("views is a non-empty list of (theta, phi) or (theta, phi, larm)")
    if temp_model is not None:
        phases = [int(p) for p in phases]
        if not phases:
            raise ValueError("phases is empty")
    else:
        phases = [None]
    if temp_model is not None and temp_model._binding.prec != static_model._binding.prec:
        raise _capi.NcaError("static and dynamic networks must use the same precision (see set_precision)")
    W, H = (int(v) for v in geo["nDetector"])
    npix, V, P = W * H, len(views), len(phases)
    if z is None:
        z = create_depth_values(geo["near_thresh"], geo["far_thresh"], int(samples), dev)
    z = z.detach().to(device=dev, dtype=torch.float32).contiguous()
    if z.dim() != 1:
        raise _capi.NcaError("view rendering takes ONE depth vector [S] shared by all rays")
    S = z.shape[0]
    dists = _interval_lengths(z, torch.empty(0, dtype=torch.float64, device=dev)).to(torch.float64).contiguous()
    i0 = float(torch.tensor(geo["max_pixel_value"], dtype=torch.float32))          # the f32 value the kernels start every ray sum from
    pred = torch.empty((V, P, npix), dtype=torch.float32, device=dev)
    pred_d = torch.empty((V, P, npix), dtype=torch.float32, device=dev)
    pred_s = torch.empty((V, npix), dtype=torch.float32, device=dev)
    plan = chunk_plan(npix, int(chunk_rays))
    with torch.cuda.device(dev):
        for v, view in enumerate(views):
            desc = pack_view(geo, *view)
            for p0, n in plan:
                o, d = _rays_of(desc, p0, n, dev, torch.float64)
                I0 = torch.full((n,), i0, dtype=torch.float32, device=dev)
                pix_s = _render_static_chunk(static_model, o, d, I0, z, dists, output_activation, scale_value)
                if temp_model is None:
                    compose_images(pix_s, None, i0, pred[v, 0, p0:p0 + n], pred_s[v, p0:p0 + n], pred_d[v, 0, p0:p0 + n])
                    continue
                pts = _query_points(o, d, z)
                ids = torch.empty(n * S, dtype=torch.int32, device=dev)
                for j, phase in enumerate(phases):
                    pix_d = _render_dynamic_chunk(temp_model, pts, ids.fill_(phase), I0, dists, output_activation, scale_value)
                    compose_images(pix_s, pix_d, i0, pred[v, j, p0:p0 + n], pred_s[v, p0:p0 + n], pred_d[v, j, p0:p0 + n])
    out = {"pred": pred.reshape(V, P, W, H), "pred_static": pred_s.reshape(V, W, H), "pred_dynamic": pred_d.reshape(V, P, W, H)}
    if normalize:
        out["minmax"] = {}
        for k in ("pred", "pred_static", "pred_dynamic"):
            img = out[k]
            norm, mm = normalize_images(img.reshape(-1, W, H))
            out[k + "_norm"], out["minmax"][k] = norm.reshape(img.shape), mm.reshape(img.shape[:-2] + (2,))
    return out


def render_view(static_model, temp_model, geo: dict, theta: float, phi: float, phase: Optional[int], samples: int, *, z: Optional[torch.Tensor] = None,
                larm: float = 0, output_activation: str = "softplus", scale_value: float = 1e-2, chunk_rays: int = 65536, normalize: bool = False) -> dict:
    """One view at one heart phase: ``render_sequence`` for ``[(theta, phi, larm)]`` x ``[phase]`` with the leading axes dropped --
    ``pred``, ``pred_static``, ``pred_dynamic`` as f32 ``[W,H]`` (and, with ``normalize``, the ``*_norm`` images and ``minmax``
    entries ``[2]``)."""
    out = render_sequence(static_model, temp_model, geo, [(theta, phi, larm)], None if temp_model is None else [phase], samples, z=z,
                          output_activation=output_activation, scale_value=scale_value, chunk_rays=chunk_rays, normalize=normalize)
    W, H = out["pred_static"].shape[-2:]
    res = {k: t.reshape(t.shape[-2:]) for k, t in out.items() if k != "minmax"}
    if normalize:
        res["minmax"] = {k: t.reshape(2) for k, t in out["minmax"].items()}
    return res
