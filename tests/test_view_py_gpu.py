"""nerfca_amd._view on the GPU: the stack it hands to the library, and the workspaces of the view wrappers under NERFCA_POISON.

A view workspace is fused._scratch's, so with fused.POISON_BUFFERS it is filled with a NaN pattern before the call.  Every wrapper below
promises the same bits on every run; a kernel that read a workspace byte it had not written would change them under the pattern.  Shapes: two
volumes of (3, 5, 65), one node past a chunk of 64 along the last axis; two images of 13 x 17, 3 x 7 positions of the 11 x 11 window."""
import pytest
import torch

from nca_testlib import dev  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE = (3, 5, 65)


def test_volume_stack(dev):
    from nerfca_amd import _capi, _view
    base = torch.arange(2 * 3 * 5 * 130, dtype=torch.float32, device=dev).reshape(2, 1, 3, 5, 130)
    vol = base[..., ::2]
    assert vol.shape == (2, 1) + SHAPE and not vol.is_contiguous()
    desc, x, n_vol, shape = _view.volume_stack(vol, "test")
    assert x.is_contiguous() and tuple(x.shape) == (2,) + SHAPE and x.dtype == torch.float32 and x.device == vol.device
    assert torch.equal(x, vol.reshape((2,) + SHAPE)) and n_vol == 2 and shape == SHAPE
    assert tuple(desc.n) == SHAPE and desc.reserved == 0
    assert all(v == 1.0 for v in desc.inv) and all(v == 0.0 for v in desc.lo)          # node units, exactly
    bounds = ((-1.0, 1.5), (0.25, 0.75), (2.0, 9.0))
    placed, y, _, _ = _view.volume_stack(vol, "test", bounds)
    want = _capi.grid_desc(SHAPE, bounds)
    assert tuple(placed.n) == SHAPE and list(placed.lo) == list(want.lo) and list(placed.inv) == list(want.inv)
    assert list(placed.lo) == [-1.0, 0.25, 2.0] and placed.inv[2] == 64 / 7.0
    assert torch.equal(y, x)


def _cases(dev):
    from nerfca_amd import ccta, metrics
    gen = torch.Generator().manual_seed(20)
    vol = torch.rand((2,) + SHAPE, generator=gen).to(dev)
    pred, truth = torch.rand((2, 13, 17), generator=gen).to(dev), torch.rand((2, 13, 17), generator=gen).to(dev)

    def ssim_grad():
        p = pred.clone().requires_grad_()
        metrics.ssim(p, truth, data_range=1.0, win_size=11).sum().backward()
        return p.grad

    return {"distance_transform": lambda: metrics.distance_transform(vol, ((0.0, 1.0), (0.0, 3.0), (0.0, 20.0)), threshold=0.9),
            "gaussian_filter": lambda: ccta.gaussian_filter(vol, (1.2, 2.0, 0.8)),
            "cityblock_distance": lambda: ccta.cityblock_distance(vol, threshold=0.9),
            "zoom": lambda: ccta.zoom(vol, order=3, output_shape=(4, 7, 70)),
            "ssim gradient": ssim_grad}


def test_poisoned_workspaces_change_no_bit(dev, monkeypatch):
    from nerfca_amd import _view, fused
    cases = _cases(dev)
    monkeypatch.setattr(fused, "POISON_BUFFERS", False)
    plain = {k: run() for k, run in cases.items()}
    monkeypatch.setattr(fused, "POISON_BUFFERS", True)
    work = _view.workspace(20, dev)
    assert work.numel() == 20 and (work.view(torch.int32) == 0x7FC12345).all()          # the flag reaches the view workspaces
    poisoned = {k: run() for k, run in cases.items()}
    monkeypatch.setattr(fused, "POISON_BUFFERS", False)
    for k, got in poisoned.items():
        want = plain[k]
        assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in (torch.float32, torch.int32), k
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (k, int((got.view(torch.int32) != want.view(torch.int32)).sum()))
        assert not torch.isnan(got).any(), k
    assert plain["zoom"].shape == (2, 4, 7, 70) and (plain["cityblock_distance"] >= 0).all() and bool(plain["ssim gradient"].any())
