"""Comparing image stacks on the device: PSNR and the structural similarity of Wang et al. (csrc/view/nca_ssim.hip).

NeRF-CA reports its 2-D results as PSNR and SSIM.  ``ssim`` is one pass over the two stacks in f64 (``nca_ssim``): Gaussian-windowed
means, variances and the covariance at every window position that lies inside the image (no padding), combined as include/nerfca_hip.h
("ssim") writes it, and averaged per image.  It is differentiable in the prediction (``nca_ssim_grad``: gathered, the same
bits on every run), so ``1 - ssim`` serves as a loss; ``drr.fit_volumes`` takes it with ``ssim_weight``.  ``compare_sequences`` sets the
stacks of ``export.render_sequence`` / ``drr.project_sequence`` side by side.  There is no torch implementation behind ``ssim``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _capi
from . import fused as _fused

MAX_WIN = 11          # NCA_SSIM_MAX_WIN


def gaussian_window(win_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The 1-D window of Wang et al.: ``exp(-d^2 / (2 sigma^2))`` at ``d = -(K-1)/2 .. (K-1)/2``, normalised to sum 1, numpy f64 ``[K]``.
    One half is computed and mirrored, so the window is symmetric bit for bit."""
    K, sigma = int(win_size), float(sigma)
    if K != win_size or K < 1 or K % 2 == 0:
        raise _capi.NcaError(f"gaussian_window: win_size = {win_size} is not an odd positive length")
    if not (math.isfinite(sigma) and sigma > 0):
        raise _capi.NcaError(f"gaussian_window: sigma = {sigma} is not finite and positive")
    h = K // 2
    half = np.exp(-(np.arange(h, -1, -1, dtype=np.float64) ** 2) / (2.0 * sigma * sigma))          # d = -h .. 0
    g = np.concatenate([half, half[-2::-1]])
    g = g / g.sum()
    g[h + 1:] = g[:h][::-1]
    return g


def _c_window(win: np.ndarray):
    win = np.ascontiguousarray(win, dtype=np.float64)
    return (C.c_double * win.size)(*win.tolist())


def _launch_ssim(x, y, rng, win, k1, k2, want_map):
    """(sums f64 [N], map f32 [N,Hv,Wv] or None): one nca_ssim of checked, contiguous stacks [N,H,W] into zeroed sums."""
    N, H, W = x.shape
    K = len(win)
    sums = torch.zeros(N, dtype=torch.float64, device=x.device)
    smap = torch.empty((N, H - K + 1, W - K + 1), dtype=torch.float32, device=x.device) if want_map else None
    with torch.cuda.device(x.device):
        _capi.check_ssim(_capi.lib().nca_ssim(N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), K, win, k1, k2, _capi.ptr(sums), _capi.ptr(smap),
                                              _fused._stream()))
    return sums, smap


class _Ssim(torch.autograd.Function):
    """The per-image mean SSIM with a gradient in the prediction: the forward is one ``nca_ssim``, the backward one ``nca_ssim_grad`` whose
    device ``scale`` holds the upstream gradients over the position count -- nothing is read back.  The map, when asked for, is returned
    without a gradient."""

    @staticmethod
    def forward(ctx, x, y, rng, win, k1, k2, want_map):
        ctx.save_for_backward(x, y, rng)
        ctx.args = (win, k1, k2)
        N, H, W = x.shape
        K = len(win)
        sums, smap = _launch_ssim(x.detach(), y, rng, win, k1, k2, want_map)
        mean = sums / float((H - K + 1) * (W - K + 1))
        if want_map:
            ctx.mark_non_differentiable(smap)
            return mean, smap
        return mean, None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mean, _g_map):
        x, y, rng = ctx.saved_tensors
        win, k1, k2 = ctx.args
        N, H, W = x.shape
        K = len(win)
        dev = x.device
        if g_mean.device != dev:
            raise _capi.NcaError(f"ssim backward: the upstream gradient lives on {g_mean.device}, the images on {dev}")
        scale = (g_mean.to(torch.float64) / float((H - K + 1) * (W - K + 1))).contiguous()
        g_x = torch.empty_like(x)
        lib = _capi.lib()
        nbytes = int(lib.nca_ssim_grad_workspace(N, H, W, K))
        work = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _capi.check_ssim(lib.nca_ssim_grad(N, H, W, _capi.ptr(x), _capi.ptr(y), _capi.ptr(rng), K, win, k1, k2, _capi.ptr(scale), _capi.ptr(g_x),
                                               _capi.ptr(work), nbytes, _fused._stream()))
        return g_x, None, None, None, None, None, None


def _range_vector(data_range, lead, dev) -> torch.Tensor:
    """f64 [N] on the device from a float or a tensor broadcastable to the leading shape; nothing is read back."""
    if isinstance(data_range, torch.Tensor):
        r = data_range.detach().to(device=dev, dtype=torch.float64)
    else:
        r = torch.tensor(float(data_range), dtype=torch.float64, device=dev)
    try:
        r = torch.broadcast_to(r, lead)
    except RuntimeError:
        raise _capi.NcaError(f"data_range of shape {tuple(r.shape)} does not broadcast to the leading shape {tuple(lead)}") from None
    return r.reshape(-1).contiguous()


def _check_pair(pred, truth, who):
    for t, what in ((pred, "pred"), (truth, "truth")):
        if not isinstance(t, torch.Tensor):
            raise _capi.NcaError(f"{who}: {what} is not a tensor")
        _fused._require_cuda(t, what)
    if pred.dtype != torch.float32 or truth.dtype != torch.float32:
        raise _capi.NcaError(f"{who} takes float32 images, got {pred.dtype} and {truth.dtype}")
    if pred.dim() < 2 or pred.shape != truth.shape or pred.numel() == 0:
        raise _capi.NcaError(f"{who} takes two stacks [..., A, B] of one shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise _capi.NcaError(f"{who}: pred lives on {pred.device}, truth on {truth.device}")


def ssim(pred: torch.Tensor, truth: torch.Tensor, *, data_range: Union[float, torch.Tensor], win_size: int = 11, sigma: float = 1.5, k1: float = 0.01,
         k2: float = 0.03, full: bool = False):
    """Mean structural similarity per image of f32 stacks ``pred`` and ``truth`` ``[..., A, B]`` on the device (the last two axes are the
    image), as an f64 device tensor of the leading shape.  ``data_range`` is the dynamic range ``L`` of the images (``C1 = (k1 L)^2``,
    ``C2 = (k2 L)^2``): a float, or a tensor broadcastable to the leading shape -- it stays on the device.  A range that is not finite and
    positive gives NaN for that image.  The window is ``gaussian_window(win_size, sigma)`` on both axes; statistics are taken only where the
    window lies inside the image, so the mean runs over ``(A - K + 1) (B - K + 1)`` positions and both axes must be at least ``win_size``
    (odd, at most 11).  ``full=True`` returns ``(mean, map)`` with the f32 map ``[..., A - K + 1, B - K + 1]`` (no gradient).

    Identical stacks give exactly 1.  The definition, operation by operation, is in include/nerfca_hip.h ("ssim"); the per-image sum is
    f64 atomics over blocks, so its last bits can differ from run to run.

    With grad mode on and ``pred.requires_grad`` the mean carries a gradient in ``pred`` (f32, gathered: the same bits on
    every run); ``truth`` and ``data_range`` get none.  In every other case nothing is recorded."""
    _check_pair(pred, truth, "ssim")
    k1, k2 = float(k1), float(k2)
    win = gaussian_window(win_size, sigma)
    K = len(win)
    A, B = pred.shape[-2:]
    if K > MAX_WIN:
        raise _capi.NcaError(f"ssim: win_size = {K} is larger than {MAX_WIN}")
    if A < K or B < K:
        raise _capi.NcaError(f"ssim: images of {A} x {B} are smaller than the window, win_size = {K}")
    lead = pred.shape[:-2]
    rng = _range_vector(data_range, lead, pred.device)
    cwin = _c_window(win)
    y = truth.detach().reshape(-1, A, B).contiguous()
    if torch.is_grad_enabled() and pred.requires_grad:
        mean, smap = _Ssim.apply(pred.reshape(-1, A, B).contiguous(), y, rng, cwin, k1, k2, bool(full))
    else:
        with torch.no_grad():
            sums, smap = _launch_ssim(pred.detach().reshape(-1, A, B).contiguous(), y, rng, cwin, k1, k2, bool(full))
            mean = sums / float((A - K + 1) * (B - K + 1))
    mean = mean.reshape(lead)
    return (mean, smap.reshape(lead + smap.shape[-2:])) if full else mean


def psnr(pred: torch.Tensor, truth: torch.Tensor, *, data_range: Union[float, torch.Tensor]) -> torch.Tensor:
    """Peak signal-to-noise ratio per image, ``10 log10(range^2 / mse)`` in f64, of stacks ``[..., A, B]``: an f64 tensor of the leading
    shape (``inf`` for identical images).  Plain torch: a handful of reductions."""
    _check_pair(pred, truth, "psnr")
    lead = pred.shape[:-2]
    diff = pred.detach().double() - truth.detach().double()
    mse = (diff * diff).mean(dim=(-2, -1))
    rng = _range_vector(data_range, lead, pred.device).reshape(lead)
    return 10.0 * torch.log10(rng * rng / mse)


def compare_sequences(pred: dict, truth: dict, *, data_range: Optional[Union[float, torch.Tensor]] = None) -> dict:
    """PSNR and SSIM of two sequence dicts as ``export.render_sequence`` / ``drr.project_sequence`` return them.  For every key both hold
    as f32 image stacks of one shape (``pred`` ``[V,P,W,H]``, ``pred_static`` ``[V,W,H]``, ...): ``{"psnr", "ssim"}`` per ``(view, phase)``
    as f64 device tensors of the leading shape, and ``"psnr_mean"``, ``"ssim_mean"`` as 0-d tensors.  ``data_range`` defaults to ``max - min``
    of each TRUTH image, formed in f64 on the device.  A constant truth image (for
    instance the ``pred_dynamic`` of a static scene, ``I0`` everywhere) has range 0: its SSIM is NaN by the kernel's rule and its PSNR
    ``-inf`` or NaN, and so are the means of that stack; pass ``data_range`` to compare such stacks."""
    out = {}
    for key in pred:
        a, b = pred[key], truth.get(key)
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.dim() < 3 or a.shape != b.shape or not a.dtype.is_floating_point:
            continue
        a, b = a.detach().to(torch.float32), b.detach().to(torch.float32)
        rng = b.amax(dim=(-2, -1)).double() - b.amin(dim=(-2, -1)).double() if data_range is None else data_range
        with torch.no_grad():
            p, s = psnr(a, b, data_range=rng), ssim(a, b, data_range=rng)
        out[key] = {"psnr": p, "ssim": s, "psnr_mean": p.mean(), "ssim_mean": s.mean()}
    if not out:
        raise _capi.NcaError("compare_sequences: the two dicts share no image stack of one shape")
    return out
