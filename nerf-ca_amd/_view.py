"""What the Python wrappers of csrc/view/ share (export, drr, metrics, ccta, phantom): the checks of a voxel stack, its grid descriptor,
the workspace of a call and the launch itself -- the counterpart of csrc/view/nca_view_common.hpp on this side.  A leaf module: it imports
``_capi`` and ``fused`` and none of the wrappers.  Every text below is part of the wrappers' behaviour: tests and callers match on it.
"""
from __future__ import annotations

import math

import torch

from . import _capi
from . import fused as _fused


def check_volume(vol, who, what="vol"):
    """An f32 stack ``[..., n0, n1, n2]`` on the device, not empty; ``who`` is the calling function's name, ``what`` the argument's."""
    if not isinstance(vol, torch.Tensor):
        raise _capi.NcaError(f"{who}: {what} is not a tensor")
    _fused._require_cuda(vol, what)
    if vol.dtype != torch.float32:
        raise _capi.NcaError(f"{who} takes float32 volumes, got {vol.dtype}")
    if vol.dim() < 3 or vol.numel() == 0:
        raise _capi.NcaError(f"{who} takes a stack [..., n0, n1, n2], got {tuple(vol.shape)}")


def check_contiguous_volumes(volumes, who):
    """The volume stack ``who`` (an entry point's name) takes: contiguous float32 [n0,n1,n2] or [n_vol,n0,n1,n2], not empty."""
    if volumes.dtype != torch.float32 or volumes.dim() not in (3, 4) or not volumes.is_contiguous() or volumes.numel() == 0:
        raise _capi.NcaError(f"{who} takes contiguous float32 volumes [n0,n1,n2] or [n_vol,n0,n1,n2], got {volumes.dtype} "
                             f"{tuple(volumes.shape)}{'' if volumes.is_contiguous() else ' (not contiguous)'}")


def volume_stack(vol, who, bounds=None, what="vol"):
    """(grid descriptor, the stack as f32 [n_vol, n0, n1, n2] contiguous, n_vol, shape) of a checked f32 volume stack on the device.
    ``bounds=None``: the grid in node units, ``(0, n - 1)`` per axis."""
    check_volume(vol, who, what)
    shape = tuple(vol.shape[-3:])
    desc = _capi.grid_desc(shape, tuple((0.0, float(n - 1)) for n in shape) if bounds is None else bounds)
    x = vol.detach().reshape((-1,) + shape).contiguous()
    return desc, x, x.shape[0], shape


def workspace(nbytes, dev):
    """The workspace of a call whose query returned ``nbytes`` (the call still gets ``nbytes``): never empty, and poisoned under
    ``NERFCA_POISON=1`` like every other scratch buffer."""
    return _fused._scratch(max(int(nbytes), 8), dev)


def launch(check, fn, dev, *args):
    """``check(fn(*args, stream))`` on the device ``dev``: the current stream is the last argument of every view entry point."""
    with torch.cuda.device(dev):
        return check(fn(*args, _fused._stream()))


def finite_threshold(value, who):
    """``float(value)`` of a threshold; NaN is refused (it would compare false with every node)."""
    value = float(value)
    if math.isnan(value):
        raise _capi.NcaError(f"{who}: threshold = nan is not a number")
    return value
