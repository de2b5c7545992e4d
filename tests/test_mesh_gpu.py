"""Iso-surfaces on the GPU: nca_vol_iso_count / nca_vol_iso_emit against the numpy transcription of their definition (tests/mesh_ref.py, held
to the mathematics in tests/test_mesh_cpu.py) with np.array_equal on the totals and the triangles and bit equality on the vertices and the
normals in every case, and mesh.isosurface, its measures and export.density_surfaces on top of them.  Output buffers are pre-filled with
0x7f7f7f7f, two rows longer than the totals, and the workspace, exactly as large as the query says, with 0xff bytes: a word the kernels did
not write, or wrote past the end, shows.

The kernels' tile is 4 x 8 x 64 nodes, staged with the next node on every axis.  (2,2,2): one cell; (3,3,3), (4,5,6): one tile; (5,9,65): a
seam of one node on every axis, so cells straddle tiles and use the halo; (9,17,130): three tiles along every axis, and twenty runs of
SCAN_CHUNK = 1024 nodes for the scan.  The scan's second level takes SCAN_BATCH = 256 run sums per round: (3,3,29128) has one node more than
SCAN_CHUNK x SCAN_BATCH / 9 per row, 257 runs, so the carry into a second round is exercised.  Every stack has two volumes that differ, and
the second is also run alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from nca_testlib import dev, grid_of, same_bits  # noqa: F401

import mesh_ref as ref

pytestmark = pytest.mark.gpu

POISON = 0x7f7f7f7f
POISON64 = 0x7f7f7f7f7f7f7f7f
GUARD = 2          # rows past the totals, which must keep their poison


def gpu_iso(dev, stack, level, normals=True, short=0):
    """One nca_vol_iso_count and one nca_vol_iso_emit of a stack [n_vol,n0,n1,n2] on the grid (ref.LO, ref.INV): dict(totals, verts, tris,
    normals) as numpy arrays without the guard rows, which are checked here.  `short`: the capacities handed to the emit are that much below
    the totals (the buffers are not)."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    n_vol = stack.shape[0]
    g = grid_of(stack.shape[1:], inv=ref.INV)
    assert tuple(g.lo) == ref.LO and tuple(g.inv) == ref.INV
    x = torch.tensor(stack).to(dev)
    totals = torch.full((n_vol, 2), POISON64, dtype=torch.int64, device=dev)
    nbytes = lib.nca_vol_iso_workspace(C.byref(g), n_vol)
    assert nbytes >= 10 * stack.size and nbytes % 256 == 0
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), _capi.ptr(x), n_vol, float(level), _capi.ptr(totals), _capi.ptr(work), nbytes, fused._stream()))
    torch.cuda.synchronize(dev)
    tot = totals.cpu().numpy()
    nv, nt = int(tot[:, 0].sum()), int(tot[:, 1].sum())
    assert 0 <= nv <= 7 * stack.size and 0 <= nt <= 12 * stack.size
    verts = torch.full((nv + GUARD, 3), POISON, dtype=torch.int32, device=dev)
    tris = torch.full((nt + GUARD, 3), POISON, dtype=torch.int32, device=dev)
    norm = torch.full((nv + GUARD, 3), POISON, dtype=torch.int32, device=dev) if normals else None
    with torch.cuda.device(dev):
        _capi.check_mesh(lib.nca_vol_iso_emit(C.byref(g), _capi.ptr(x), n_vol, float(level), _capi.ptr(work), nbytes, max(nv - short, 0), max(nt - short, 0), _capi.ptr(verts),
                                              _capi.ptr(tris), _capi.ptr(norm), fused._stream()))
    torch.cuda.synchronize(dev)
    out = dict(totals=tot, verts=verts.cpu().numpy(), tris=tris.cpu().numpy(), normals=None if norm is None else norm.cpu().numpy())
    for key in ("verts", "tris", "normals"):
        if out[key] is not None:
            assert (out[key][len(out[key]) - GUARD:] == POISON).all(), key
            out[key] = out[key][:len(out[key]) - GUARD]
    return out


def check_equal(got, want, tag, v0=0, v1=None, t0=0, t1=None):
    """got (int32 views, from gpu_iso) against rows [v0, v1) and [t0, t1) of want (tests/mesh_ref.py)."""
    assert np.array_equal(got["tris"], want["tris"][t0:t1]), (tag, "tris", got["tris"].shape, want["tris"][t0:t1].shape)
    assert np.array_equal(got["verts"], want["verts"][v0:v1].view(np.int32)), (tag, "verts")
    if got["normals"] is not None:
        assert np.array_equal(got["normals"], want["normals"][v0:v1].view(np.int32)), (tag, "normals")


# ----------------------------------------------------------------------------- the raw entry points
CASES = [(shape, name) for shape in ref.GPU_SHAPES for name in ref.CASE_NAMES] + [(ref.PAST_ONE_SCAN_ROUND, name) for name in ("random", "checkerboard")]


@pytest.mark.parametrize("shape,name", CASES, ids=lambda p: str(p).replace(" ", ""))
def test_iso_equals_the_oracle(dev, shape, name):
    """Two volumes that differ: the oracle's totals, triangles, vertices and normals, the last two bit for bit; a second run; the second
    volume alone; without normals."""
    stack, level = ref.case(shape, name)
    want = ref.expected(shape, name)
    got = gpu_iso(dev, stack, level)
    assert got["totals"].dtype == np.int64 and np.array_equal(got["totals"], want["totals"]), (got["totals"].tolist(), want["totals"].tolist())
    check_equal(got, want, name)
    again = gpu_iso(dev, stack, level)
    for key in ("totals", "verts", "tris", "normals"):
        assert np.array_equal(again[key], got[key]), (name, key)
    v0, t0 = (int(x) for x in want["totals"][0])
    alone = gpu_iso(dev, stack[1:2], level)
    assert np.array_equal(alone["totals"], want["totals"][1:2])
    check_equal(alone, want, name + " alone", v0, None, t0, None)
    bare = gpu_iso(dev, stack, level, normals=False)
    assert bare["normals"] is None
    check_equal(bare, want, name + " without normals")


def test_what_the_cases_cover():
    """Totals of 0, twelve triangles in every cell, and meshes large enough to cross every seam."""
    for shape in ref.GPU_SHAPES:
        cells = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
        assert ref.expected(shape, "empty and full")["totals"].tolist() == [[0, 0], [0, 0]]
        assert ref.expected(shape, "checkerboard")["totals"][:, 1].tolist() == [12 * cells] * 2
        assert (ref.expected(shape, "random")["totals"] > 0).all() and (ref.expected(shape, "nonfinite")["totals"] > 0).all()
    assert (ref.expected((9, 17, 130), "ball")["totals"] > 100).all() and (ref.expected((9, 17, 130), "torus")["totals"] > 100).all()
    n = ref.PAST_ONE_SCAN_ROUND
    assert (n[0] * n[1] * n[2] + ref.SCAN_CHUNK - 1) // ref.SCAN_CHUNK == ref.SCAN_BATCH + 1


@pytest.mark.parametrize("shape", [(4, 5, 6), (9, 17, 130)], ids=str)
def test_capacities_guard_every_store(dev, shape):
    """Capacities one short of the totals: everything below them is written as before, the last vertex, normal and triangle keep their poison."""
    for name in ("random", "checkerboard"):
        stack, level = ref.case(shape, name)
        want = ref.expected(shape, name)
        got = gpu_iso(dev, stack, level, short=1)
        for key in ("verts", "tris", "normals"):
            assert (got[key][-1] == POISON).all(), (name, key)
            got[key] = got[key][:-1]
        check_equal(got, want, name, 0, -1, 0, -1)


def test_nothing_to_write_launches_nothing(dev):
    """Totals of 0: the emit takes NULL outputs and capacities of 0."""
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    g = grid_of((4, 5, 6), inv=ref.INV)
    x = torch.zeros((2, 4, 5, 6), device=dev)
    nbytes = lib.nca_vol_iso_workspace(C.byref(g), 2)
    work = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=dev)
    totals = torch.full((2, 2), POISON64, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), _capi.ptr(x), 2, 0.5, _capi.ptr(totals), _capi.ptr(work), nbytes, fused._stream()))
        assert totals.cpu().tolist() == [[0, 0], [0, 0]]
        assert lib.nca_vol_iso_emit(C.byref(g), _capi.ptr(x), 2, 0.5, _capi.ptr(work), nbytes, 0, 0, None, None, None, fused._stream()) == 0
    torch.cuda.synchronize(dev)


def test_refusal_texts_with_device_pointers(dev):
    from nerfca_amd import _capi, fused
    lib = _capi.lib()
    g = grid_of((4, 5, 6), inv=ref.INV)
    x = torch.zeros((1, 4, 5, 6), device=dev)
    nbytes = lib.nca_vol_iso_workspace(C.byref(g), 1)
    work = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        with pytest.raises(_capi.NcaError, match=r"nca_vol_iso_count: level = inf is not finite"):
            _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), _capi.ptr(x), 1, float("inf"), _capi.ptr(totals), _capi.ptr(work), nbytes, fused._stream()))
        with pytest.raises(_capi.NcaError, match=rf"nca_vol_iso_count: the workspace holds {nbytes - 1} bytes, {nbytes} are needed"):
            _capi.check_mesh(lib.nca_vol_iso_count(C.byref(g), _capi.ptr(x), 1, 0.5, _capi.ptr(totals), _capi.ptr(work), nbytes - 1, fused._stream()))
        with pytest.raises(_capi.NcaError, match=r"nca_vol_iso_emit: tris is NULL"):
            _capi.check_mesh(lib.nca_vol_iso_emit(C.byref(g), _capi.ptr(x), 1, 0.5, _capi.ptr(work), nbytes, 0, 5, None, None, None, fused._stream()))
        with pytest.raises(_capi.NcaError, match=r"nca_vol_iso_emit: vert_cap = -2 is negative"):
            _capi.check_mesh(lib.nca_vol_iso_emit(C.byref(g), _capi.ptr(x), 1, 0.5, _capi.ptr(work), nbytes, -2, 5, None, None, None, fused._stream()))
    torch.cuda.synchronize(dev)


# ----------------------------------------------------------------------------- the Python layer
def bounds_of(shape):
    return tuple((ref.LO[a], ref.LO[a] + (shape[a] - 1) / ref.INV[a]) for a in range(3))


def test_isosurface_and_its_measures(dev):
    from nerfca_amd import mesh
    shape = (12, 20, 20)
    bounds = bounds_of(shape)
    vols = np.stack([ref.torus(shape), ref.ball(shape, 4.3), ref.two_balls(shape), np.full(shape, -1.0, dtype=np.float32)])
    x = torch.from_numpy(vols).to(dev)
    meshes = mesh.isosurface(x, 0.0, bounds, normals=True)
    assert isinstance(meshes, list) and len(meshes) == 4
    for v, (m, chi) in enumerate(zip(meshes, (0, 2, 4, 0))):
        want = ref.mesh(vols[v], 0.0, ref.LO, ref.INV, normals=True)
        assert isinstance(m, mesh.Mesh) and m.verts.device == x.device and m.faces.device == x.device and m.normals.device == x.device
        assert m.verts.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.normals.dtype == torch.float32
        assert same_bits(m.verts.cpu().numpy(), want["verts"]) and np.array_equal(m.faces.cpu().numpy(), want["tris"]) and same_bits(m.normals.cpu().numpy(), want["normals"])
        assert mesh.euler_characteristic(m) == chi == (ref.euler_characteristic(want["tris"]) if len(want["tris"]) else 0)
        area, volume = mesh.surface_area(m), mesh.enclosed_volume(m)
        assert area.device == x.device and area.dtype == torch.float64 and volume.device == x.device and volume.dtype == torch.float64
        if v < 3:
            want_area, want_volume = ref.area(want["verts"], want["tris"]), ref.inside_volume(vols[v], 0.0, bounds)
            assert abs(float(area) - want_area) <= 1e-12 * want_area and abs(float(volume) - want_volume) <= 1e-6 * want_volume
    empty = meshes[3]
    assert empty.verts.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.normals.shape == (0, 3)
    assert float(mesh.surface_area(empty)) == 0.0 and float(mesh.enclosed_volume(empty)) == 0.0
    # one volume: a Mesh, not a list; no normals unless asked for; bounds=None is node units; a leading shape is flattened in stack order
    one = mesh.isosurface(x[1], 0.0, bounds)
    assert isinstance(one, mesh.Mesh) and one.normals is None and torch.equal(one.verts, meshes[1].verts) and torch.equal(one.faces, meshes[1].faces)
    nodes = mesh.isosurface(x[1], 0.0, None)
    want = ref.mesh(vols[1], 0.0, (0.0,) * 3, (1.0,) * 3)
    assert same_bits(nodes.verts.cpu().numpy(), want["verts"]) and torch.equal(nodes.faces, one.faces)
    lead = mesh.isosurface(x.reshape((2, 2) + shape), 0.0, bounds)
    assert len(lead) == 4 and all(torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) for a, b in zip(lead, meshes))
    nothing = mesh.isosurface(x[3], 0.0, bounds, normals=True)
    assert nothing.verts.shape == (0, 3) and nothing.faces.shape == (0, 3) and nothing.normals.shape == (0, 3)
    # an input that is not contiguous
    wide = torch.zeros((12, 20, 40), device=dev)
    wide[..., ::2] = x[0]
    strided = wide[..., ::2]
    sm = mesh.isosurface(strided, 0.0, bounds)
    assert not strided.is_contiguous() and torch.equal(sm.verts, meshes[0].verts) and torch.equal(sm.faces, meshes[0].faces)
    with pytest.raises(mesh._capi.NcaError, match="float32"):
        mesh.isosurface(x.double(), 0.0, bounds)
    with pytest.raises(mesh._capi.NcaError, match="level"):
        mesh.isosurface(x, float("nan"), bounds)
    with pytest.raises(mesh._capi.NcaError, match="bounds"):
        mesh.isosurface(x, 0.0, ((0.0, 1.0), (1.0, 1.0), (0.0, 1.0)))


def test_isosurface_reads_the_host_once(dev, monkeypatch):
    """Exactly one device-to-host copy per call: the totals."""
    from nerfca_amd import mesh
    x = torch.from_numpy(np.stack([ref.ball((8, 9, 10)), ref.random_volume((8, 9, 10), 2)])).to(dev)
    reads = []
    real_cpu, real_tolist = torch.Tensor.cpu, torch.Tensor.tolist

    def cpu(self, *a, **k):
        reads.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    def on_device(name, real):
        def method(self, *a, **k):
            assert not self.is_cuda, f"{name} of a device tensor is a host read"
            return real(self, *a, **k)
        return method

    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    monkeypatch.setattr(torch.Tensor, "tolist", on_device("tolist", real_tolist))
    monkeypatch.setattr(torch.Tensor, "item", on_device("item", torch.Tensor.item))
    meshes = mesh.isosurface(x, 0.25, None, normals=True)
    assert reads == [(2, 2)] and len(meshes) == 2 and meshes[1].faces.shape[0] > 0


def test_density_surfaces(dev):
    from nerfca_amd import export, mesh, synthetic
    from nerfca_amd.model.CPPN import CPPN
    from nerfca_amd.model.Temporal import Temporal
    torch.manual_seed(5)
    s = CPPN(synthetic.net_definitions(dev, F=64)[0]).to(dev)
    t = Temporal(synthetic.net_definitions(dev, F=64)[1]).to(dev)
    for m in (s, t):
        m.update_freq_mask_alpha(75000, 150000)
    kw = dict(resolution=(7, 6, 9), bounds=((-1.0, 1.0), (-0.5, 0.75), (0.0, 1.0)), chunk_points=100)
    sig_s, sig_d = export.density_volumes(s, t, (0, 3), **kw)
    level = float(sig_d.median())
    got = export.density_surfaces(s, t, (0, 3), level, **kw)
    assert isinstance(got, list) and len(got) == 2
    inv = tuple((n - 1) / (hi - lo) for n, (lo, hi) in zip(kw["resolution"], kw["bounds"]))
    for j in range(2):
        want = ref.mesh(sig_d[j].cpu().numpy(), level, tuple(b[0] for b in kw["bounds"]), inv)
        assert want["tris"].shape[0] > 0 and got[j].normals is None
        assert same_bits(got[j].verts.cpu().numpy(), want["verts"]) and np.array_equal(got[j].faces.cpu().numpy(), want["tris"])
    total = export.density_surfaces(s, t, (3,), float((sig_d[1] + sig_s).median()), field="total", normals=True, **kw)
    want = mesh.isosurface(sig_d[1] + sig_s, float((sig_d[1] + sig_s).median()), kw["bounds"], normals=True)
    assert len(total) == 1 and torch.equal(total[0].verts, want.verts) and torch.equal(total[0].faces, want.faces) and torch.equal(total[0].normals, want.normals)
    static = export.density_surfaces(s, None, (), float(sig_s.median()), field="static", **kw)
    want = mesh.isosurface(sig_s, float(sig_s.median()), kw["bounds"])
    assert len(static) == 1 and torch.equal(static[0].verts, want.verts) and torch.equal(static[0].faces, want.faces) and static[0].faces.shape[0] > 0


def test_nothing_existing_changed(dev):
    """metrics.label and ccta.hessian_eigenvalues give the same bits before and after the new entry points have run."""
    from nerfca_amd import ccta, mesh, metrics
    a = torch.from_numpy(np.stack([ref.random_volume((7, 9, 70), s) for s in (0, 1)])).to(dev)

    def existing():
        labels, counts = metrics.label(a, threshold=0.5, connectivity=3)
        return labels.clone(), counts.clone(), ccta.hessian_eigenvalues(a, 1.0).clone()

    before = existing()
    mesh.isosurface(a, 0.5, None, normals=True)
    after = existing()
    for x, y in zip(before, after):
        assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
