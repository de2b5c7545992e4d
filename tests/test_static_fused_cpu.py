"""CPU tests of the static-only loop's fused path (ABI 13): the two nca_static_loss_* entry points as the header, the ctypes table and
the built library know them, the workspace arithmetic, the argument refusals through the C ABI (pointers that are never read) and the
StaticTrainer surface.  No launch happens here."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_static_loss_symbols_and_abi():
    from nerfca_amd import _capi
    header = open(os.path.join(ROOT, "include", "nerfca_hip.h")).read()
    declared = set(re.findall(r"\b(nca_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in ("nca_static_loss_workspace", "nca_static_loss_fwd_bwd"):
        assert name in declared, f"{name} is not declared in nerfca_hip.h"
        assert name in _capi.SYMBOLS, f"{name} is not in the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported"
    assert int(re.search(r"#define NCA_ABI_VERSION (\d+)", header).group(1)) == 13
    assert _capi.ABI_VERSION == 13 and _capi.lib().nca_abi_version() == 13
    assert _capi.STATIC_TERM_NAMES == ["loss", "pixel", "occl", "reserved"]
    # the descriptor as the header lays it out: i64, 2 x i32, 2 x f64, 4 pointers, 2 x i32
    assert C.sizeof(_capi.NcaStaticLoss) == 8 + 8 + 16 + 32 + 8
    assert re.search(r"NCA_ST_LOSS = 0, NCA_ST_PIXEL, NCA_ST_OCCL, NCA_ST_COUNT = 4", header)


def test_static_loss_workspace():
    from nerfca_amd import _capi
    L = _capi.lib()
    prev = 0
    for R in (1, 3, 4, 5, 96, 257, 1000, 16384, 65536, 1 << 24):
        b = L.nca_static_loss_workspace(R)
        assert b > 0 and b % 256 == 0, (R, b)
        assert b >= prev, (R, b, prev)
        assert b >= 16 * ((R + 3) // 4)            # two f64 partial sums per block of four rays
        prev = b
    assert L.nca_static_loss_workspace(1 << 24) > L.nca_static_loss_workspace(1)
    assert L.nca_static_loss_workspace(0) == -1 and b"empty" in L.nca_last_error()
    assert L.nca_static_loss_workspace(-5) == -1


def test_static_loss_argument_refusals():
    """Every refusal is decided on the host before any launch: the dummy pointers are never read."""
    from nerfca_amd import _capi
    L = _capi.lib()
    dummy = C.c_void_p(0x1000)

    def desc(R=64, S=48, **kw):
        return _capi.NcaStaticLoss(R=R, S=S, reserved=0, w_occl=1e-8, inv_R=1.0 / max(R, 1), terms_f32=None,
                                   ray_part=kw.get("ray_part"), ray_I0=kw.get("ray_I0"), pix_out=None, ray_nchunk=kw.get("ray_nchunk", 0), reserved2=0)

    def call(d, pix=dummy, gt=dummy, wpix=dummy, sigma=dummy, dists=dummy, terms=dummy, g_pix=dummy, g_sigma=dummy, work=dummy, wbytes=None):
        if wbytes is None:
            wbytes = L.nca_static_loss_workspace(max(int(d.R), 1)) if d is not None else 256
        return L.nca_static_loss_fwd_bwd(C.byref(d) if d is not None else None, pix, gt, wpix, sigma, dists, terms, g_pix, g_sigma, work, wbytes, None)

    INVALID, WORKSPACE = -1, -4
    assert call(None) == INVALID and b"descriptor" in L.nca_last_error()
    assert call(desc(R=0)) == INVALID and b"empty" in L.nca_last_error()
    assert call(desc(R=-3)) == INVALID
    assert call(desc(S=0)) == INVALID
    assert call(desc(), pix=None) == INVALID and b"ray_part" in L.nca_last_error()          # NULL pix without ray sums
    assert call(desc(ray_part=dummy), pix=None) == INVALID and b"ray_I0" in L.nca_last_error()   # ray sums without their I0 / chunk count
    assert call(desc(ray_part=dummy, ray_I0=dummy, ray_nchunk=0), pix=None) == INVALID
    assert call(desc(), sigma=None) == INVALID and b"sigma" in L.nca_last_error()
    assert call(desc(), dists=None) == INVALID and b"dists" in L.nca_last_error()
    assert call(desc(), gt=None) == INVALID
    assert call(desc(), wpix=None) == INVALID
    assert call(desc(), terms=None) == INVALID
    assert call(desc(), g_pix=None) == INVALID and b"both gradient outputs" in L.nca_last_error()
    assert call(desc(), g_sigma=None) == INVALID
    need = L.nca_static_loss_workspace(64)
    assert call(desc(), wbytes=need - 1) == WORKSPACE and b"workspace" in L.nca_last_error()
    assert call(desc(), work=None) == WORKSPACE
    assert call(desc(R=1 << 20), wbytes=need) == WORKSPACE


def test_static_trainer_surface():
    import inspect
    from nerfca_amd import fused
    from nerfca_amd.train.trainer import StaticTrainer
    for name in ("step_fused", "step_graph", "evaluate", "fused_gradients", "fused_gradients_on"):
        assert callable(getattr(StaticTrainer, name, None)), name
    assert list(inspect.signature(StaticTrainer.fused_gradients_on).parameters) == ["self", "n_iter", "origins", "directions", "I0", "gt", "w", "t_rand", "share"]
    assert list(inspect.signature(StaticTrainer.evaluate).parameters) == ["self", "n_iter", "chunk_rays"]
    assert list(inspect.signature(fused.static_losses).parameters) == ["pix", "gt", "wpix", "sigma", "dists", "w_occl", "inv_R", "want_grads", "terms_f32", "pix_out"]
    for name in ("nerfies_windowed", "64", "world > 1"):           # the cases step_graph routes to step_fused are named in its docstring
        assert name in StaticTrainer.step_graph.__doc__, name
