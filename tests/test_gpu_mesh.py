"""Isosurface extraction on the device (csrc/mesh.hip through ncnerf_amd.mesh) against the NumPy
restatement of the definition (tests/mesh_ref.py, pinned by tests/test_mesh_host.py): vertices bit for
bit, faces as arrays (their order is part of the contract), at the smallest sizes at which each
mechanism can go wrong."""
import math

import numpy as np
import pytest
import torch

import mesh_ref
from ncnerf_amd import _lib, mesh
from ncnerf_amd.ngp_mt import NGPMT
from oracle import field_ref

pytestmark = pytest.mark.gpu
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
ANISO = ((-0.31, 0.05, -1.7), (0.44, 0.26, 2.9))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_extract(dev, sigma, lo, hi, iso, occupancy=None):
    v, f = mesh.extract_isosurface(torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float32)).to(dev), lo, hi, iso,
                                   occupancy)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    return v.cpu().numpy(), f.cpu().numpy()


def assert_same_mesh(got, want):
    (v, f), (rv, rf) = got, want
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(bits(v), bits(rv))
    assert np.array_equal(f, rf)


def large_res():
    """The smallest (nx, n, n) with two tiles along x whose point count and cell count each span at least
    three scan blocks with a ragged last block."""
    nx = mesh.TILE[0] + 1
    for n in range(1, 4096):
        P, C = (nx + 1) * (n + 1) ** 2, nx * n * n
        if min(mesh.blocks(P), mesh.blocks(C)) >= 3 and P % mesh.SCAN_ELEMS and C % mesh.SCAN_ELEMS:
            return (nx, n, n)


# ---- every sign pattern of one cell ----
def test_all_256_sign_patterns_of_one_cell(dev):
    iso = 0.25
    for pattern in range(256):
        sigma = np.array([iso + 1.0 if (pattern >> d) & 1 else iso - 1.0 for d in range(8)], np.float32).reshape(2, 2, 2)
        got = device_extract(dev, sigma, *ANISO, iso)
        want = mesh_ref.extract(sigma, *ANISO, iso)
        assert_same_mesh(got, want)
        assert np.array_equal(mesh_ref.canonical(got[1]), mesh_ref.canonical(want[1]))


# ---- random lattices ----
@pytest.mark.parametrize("res,box", [((1, 1, 1), BOX), ((2, 3, 4), BOX), ((5, 6, 7), BOX), ((7, 5, 3), ANISO),
                                     (mesh.TILE, BOX), ("large", ANISO)])
def test_random_lattice(dev, res, box):
    res = large_res() if res == "large" else res
    if res[0] > mesh.TILE[0]:
        P, C = (res[0] + 1) * (res[1] + 1) * (res[2] + 1), res[0] * res[1] * res[2]
        assert mesh.blocks(P) >= 3 and mesh.blocks(C) >= 3 and P % mesh.SCAN_ELEMS and C % mesh.SCAN_ELEMS
        assert res[1] + 1 > mesh.TILE[1] and res[2] + 1 > mesh.TILE[2]  # more than one tile on every axis
    rng = np.random.default_rng(sum(res))
    sigma = rng.standard_normal((res[2] + 1, res[1] + 1, res[0] + 1)).astype(np.float32)
    got = device_extract(dev, sigma, *box, 0.1)
    want = mesh_ref.extract(sigma, *box, 0.1)
    assert len(want[0]) > 0 and len(want[1]) > 0
    assert_same_mesh(got, want)


def test_sigma_shape_is_checked_and_a_view_is_accepted(dev):
    with pytest.raises(ValueError, match=r"sigma must be \(Nz\+1, Ny\+1, Nx\+1\)"):
        mesh.extract_isosurface(torch.zeros(3, 3, device=dev), *BOX, 0.0)
    with pytest.raises(ValueError, match=r"sigma must be \(Nz\+1, Ny\+1, Nx\+1\)"):
        mesh.extract_isosurface(torch.zeros(3, 1, 3, device=dev), *BOX, 0.0)
    with pytest.raises(RuntimeError, match="sigma must be torch.float32"):
        mesh.extract_isosurface(torch.zeros(3, 3, 3, device=dev, dtype=torch.float64), *BOX, 0.0)
    rng = np.random.default_rng(5)
    big = torch.from_numpy(rng.standard_normal((6, 5, 8)).astype(np.float32)).to(dev)
    view = big[:, :, ::2]  # not contiguous
    v, f = mesh.extract_isosurface(view, *BOX, 0.0)
    assert_same_mesh((v.cpu().numpy(), f.cpu().numpy()), mesh_ref.extract(view.cpu().numpy(), *BOX, 0.0))


# ---- the scan alone: every path of its two passes ----
@pytest.mark.parametrize("popcount", [0, 1])
def test_scan(dev, popcount):
    E, S = mesh.SCAN_ELEMS, mesh.SCAN_SWEEP
    rng = np.random.default_rng(11)
    for n in (1, 15, 16, 17, E - 1, E, E + 1, 3 * E + 1234, (2 * S + 1) * E + 777):  # the last: three sweeps of the base pass
        a = rng.integers(0, 128 if popcount else 13, n).astype(np.uint8)
        v = np.array([bin(x).count("1") for x in range(128)], np.int64)[a] if popcount else a.astype(np.int64)
        excl = np.cumsum(v) - v
        nb = mesh.blocks(n)
        local = torch.full((n + 32,), -1, dtype=torch.int16, device=dev)
        base = torch.full((nb + 4,), -7, dtype=torch.int64, device=dev)
        total = torch.full((2,), -7, dtype=torch.int64, device=dev)
        _lib.call("ncn_mesh_scan", torch.from_numpy(a).to(dev), n, popcount, local, base, total)
        want_base = excl[::E]
        assert np.array_equal(base.cpu().numpy(), np.concatenate([want_base, [-7] * 4])), n
        assert np.array_equal(total.cpu().numpy(), [v.sum(), -7]), n
        got_local = local.cpu().numpy().view(np.uint16)
        assert np.array_equal(got_local[:n].astype(np.int64), excl - np.repeat(want_base, E)[:n]), n
        assert (got_local[n:] == 0xFFFF).all(), n  # nothing past the n elements


# ---- edge values ----
def test_exact_iso_nan_and_infinities(dev):
    rng = np.random.default_rng(3)
    sigma = rng.standard_normal((6, 7, 8)).astype(np.float32)
    kind = rng.integers(0, 8, sigma.shape)
    iso = np.float32(0.375)
    sigma[kind == 0] = iso  # inside by definition: t = 0 on its crossing edges, degenerate triangles kept
    sigma[kind == 1] = np.nan  # outside
    sigma[kind == 2] = np.inf  # inside
    sigma[kind == 3] = -np.inf
    got = device_extract(dev, sigma, *ANISO, float(iso))
    want = mesh_ref.extract(sigma, *ANISO, float(iso))
    assert np.isfinite(want[0]).all() and len(want[1]) > 100
    assert_same_mesh(got, want)
    # a vertex on an edge with a non-finite end is its midpoint; one owned by an exact-iso point is that point
    pos = mesh_ref.lattice_positions((7, 6, 5), *ANISO)
    assert (got[0][:, None, :] == pos[None, (sigma == iso).reshape(-1), :]).all(-1).any()


@pytest.mark.parametrize("value", [1.0, -1.0, float("nan")])
def test_all_inside_or_all_outside_writes_nothing(dev, value):
    sigma = torch.full((5, 4, 6), value, device=dev)
    ws = mesh.count_and_scan(sigma, *BOX, 0.0)
    assert ws["totals"].tolist() == [0, 0]
    assert not ws["mask"].any() and not ws["nfaces"].any()
    verts = torch.full((16, 3), -123.0, device=dev)
    faces = torch.full((16, 3), -123, dtype=torch.int64, device=dev)
    mesh.emit(sigma, *BOX, 0.0, ws, verts, faces, 0, 0)
    assert (verts == -123.0).all() and (faces == -123).all()
    v, f = mesh.extract_isosurface(sigma, *BOX, 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_nothing_is_written_past_the_counts(dev):
    rng = np.random.default_rng(9)
    s = rng.standard_normal((5, 6, 7)).astype(np.float32)
    sigma = torch.from_numpy(s).to(dev)
    ws = mesh.count_and_scan(sigma, *BOX, 0.0)
    V, F = ws["totals"].tolist()
    rv, rf = mesh_ref.extract(s, *BOX, 0.0)
    assert (V, F) == (len(rv), len(rf))
    verts = torch.full((V + 64, 3), -123.0, device=dev)
    faces = torch.full((F + 64, 3), -123, dtype=torch.int64, device=dev)
    mesh.emit(sigma, *BOX, 0.0, ws, verts, faces, V, F)
    assert_same_mesh((verts[:V].cpu().numpy(), faces[:F].cpu().numpy()), (rv, rf))
    assert (verts[V:] == -123.0).all() and (faces[F:] == -123).all()
    # a caller that hands a smaller count gets that many rows and no more
    verts.fill_(-123.0), faces.fill_(-123)
    mesh.emit(sigma, *BOX, 0.0, ws, verts, faces, V // 2, F // 2)
    assert np.array_equal(bits(verts[:V // 2].cpu().numpy()), bits(rv[:V // 2])) and (verts[V // 2:] == -123.0).all()
    assert np.array_equal(faces[:F // 2].cpu().numpy(), rf[:F // 2]) and (faces[F // 2:] == -123).all()


def test_surface_that_meets_the_box_face(dev):
    res, c = (5, 4, 3), 0.13
    sigma = mesh_ref.sample(lambda x, y, z: c - x, res, *ANISO)
    v, f = device_extract(dev, sigma, *ANISO, 0.0)
    assert_same_mesh((v, f), mesh_ref.extract(sigma, *ANISO, 0.0))
    uses = mesh_ref.undirected_edge_uses(f)
    assert set(uses.values()) == {1, 2} and all(k == 1 for k in mesh_ref.directed_edge_uses(f).values())
    ends = [mesh_ref.axis_positions(res[a], ANISO[0][a], ANISO[1][a])[[0, -1]] for a in range(3)]
    lo, hi = (np.array([e[k] for e in ends], np.float32) for k in range(2))  # the first and last lattice planes
    on_face = lambda i: bool(((v[i, 1:] == lo[1:]) | (v[i, 1:] == hi[1:])).any())
    assert all(on_face(a) and on_face(b) for (a, b), k in uses.items() if k == 1)  # border edges lie on the box
    n = mesh_ref.face_normals_area(v, f)
    assert (n[:, 0] > 0).all() and abs(np.linalg.norm(n, axis=1).sum() - (hi[1] - lo[1]) * (hi[2] - lo[2])) < 1e-5


# ---- topology of the device output ----
def test_sphere(dev):
    res, R, c = (20, 20, 20), 0.3, (0.013, -0.021, 0.007)
    sigma = mesh_ref.sample(mesh_ref.sphere(c, R), res, *BOX)
    v, f = device_extract(dev, sigma, *BOX, 0.0)
    assert_same_mesh((v, f), mesh_ref.extract(sigma, *BOX, 0.0))
    mesh_ref.check_closed_surface(v, f, 2)
    lo_v, hi_v = mesh_ref.sphere_volume_bounds(R, 1.0 / 20)
    assert lo_v <= mesh_ref.signed_volume(v, f) <= hi_v


def test_two_spheres(dev):
    f1, f2 = mesh_ref.sphere((-0.22, 0.0, 0.0), 0.17), mesh_ref.sphere((0.22, 0.05, 0.0), 0.15)
    sigma = mesh_ref.sample(lambda x, y, z: np.maximum(f1(x, y, z), f2(x, y, z)), (24, 16, 16), *BOX)
    v, f = device_extract(dev, sigma, *BOX, 0.0)
    assert_same_mesh((v, f), mesh_ref.extract(sigma, *BOX, 0.0))
    mesh_ref.check_closed_surface(v, f, 4)


def test_torus(dev):
    sigma = mesh_ref.sample(mesh_ref.torus, (24, 24, 12), *BOX)
    v, f = device_extract(dev, sigma, *BOX, 0.0)
    assert_same_mesh((v, f), mesh_ref.extract(sigma, *BOX, 0.0))
    mesh_ref.check_closed_surface(v, f, 0)
    assert mesh_ref.signed_volume(v, f) > 0


# ---- occupancy ----
def _random_occupancy(dev, G, seed):
    occ = np.random.default_rng(seed).random((G, G, G)) < 0.5
    return occ, mesh.Occupancy(torch.from_numpy(mesh_ref.pack_bitfield(occ)).to(dev), G, 0.5)


@pytest.mark.parametrize("box", [BOX, ((-0.7, -0.2, -0.5), (0.3, 0.45, 0.55))])  # the second leaves the grid: clamped
def test_half_set_bitfield(dev, box):
    G, res = 8, (9, 7, 5)
    occ, occupancy = _random_occupancy(dev, G, 21)
    active = mesh_ref.active_cells(res, *box, mesh_ref.pack_bitfield(occ), G, 0.5)
    assert 0.25 < active.mean() < 0.75
    sigma = np.random.default_rng(22).standard_normal((res[2] + 1, res[1] + 1, res[0] + 1)).astype(np.float32)
    got = device_extract(dev, sigma, *box, 0.0, occupancy)
    want = mesh_ref.extract(sigma, *box, 0.0, active)
    full = mesh_ref.extract(sigma, *box, 0.0)
    assert 0 < len(want[1]) < len(full[1]) and len(want[0]) < len(full[0])
    assert_same_mesh(got, want)
    assert len(np.unique(got[1])) == len(got[0])  # no vertex without a face
    # the points the density pass is given: those with an active incident cell, and no others
    P = sigma.size
    xyz = torch.full((P, 3), -9.0, device=dev)
    idx = torch.full((P,), -9, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("ncn_mesh_points", *res, *box[0], *box[1], 0, P, occupancy.bitfield, G, 0.5, xyz, idx, count)
    listed = np.flatnonzero(mesh_ref.points_with_active_cell(active).reshape(-1))
    m = int(count.item())
    got_idx = idx.cpu().numpy()
    assert m == len(listed) and np.array_equal(np.sort(got_idx[:m]), listed) and (got_idx[m:] == -9).all()
    pos = mesh_ref.lattice_positions(res, *box)
    assert np.array_equal(bits(xyz[:m].cpu().numpy()), bits(pos[got_idx[:m]])) and (xyz[m:] == -9.0).all()


def test_all_set_bitfield_equals_no_occupancy(dev):
    G, res = 8, (9, 7, 5)
    occupancy = mesh.Occupancy(torch.full((G ** 3 // 8,), 255, dtype=torch.uint8, device=dev), G, 0.5)
    sigma = torch.from_numpy(np.random.default_rng(23).standard_normal((6, 8, 10)).astype(np.float32)).to(dev)
    a, b = mesh.extract_isosurface(sigma, *BOX, 0.0, occupancy), mesh.extract_isosurface(sigma, *BOX, 0.0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and len(a[1]) > 0
    with pytest.raises(ValueError, match="power of two"):
        mesh.extract_isosurface(sigma, *BOX, 0.0, mesh.Occupancy(occupancy.bitfield, 6, 0.5))
    with pytest.raises(ValueError, match=r"grid_size\*\*3 / 8 = 512 bytes"):
        mesh.extract_isosurface(sigma, *BOX, 0.0, mesh.Occupancy(occupancy.bitfield, 16, 0.5))


def test_points_range(dev):
    """ncn_mesh_points on a range [p0, p0 + n) that starts and ends inside rows."""
    res = (6, 4, 3)
    pos = mesh_ref.lattice_positions(res, *ANISO)
    for p0, n in ((0, len(pos)), (5, 1), (13, 77), (len(pos) - 3, 3)):
        xyz = torch.full((n + 2, 3), -9.0, device=dev)
        _lib.call("ncn_mesh_points", *res, *ANISO[0], *ANISO[1], p0, n, None, 0, 0.0, xyz, None, None)
        assert np.array_equal(bits(xyz[:n].cpu().numpy()), bits(pos[p0:p0 + n])) and (xyz[n:] == -9.0).all()
    with pytest.raises(_lib.NcnError, match=r"must lie in \[0, 140\)"):
        _lib.call("ncn_mesh_points", *res, *ANISO[0], *ANISO[1], 100, 41, None, 0, 0.0, xyz, None, None)


# ---- end to end on a model ----
def _model_from(P, dev):
    m = NGPMT(scale=0.5, grid_size=128).to(dev)
    flat, off = m.flat_params(), m._n_table
    with torch.no_grad():
        flat[:off].copy_(P.table.reshape(-1))
        for W in (P.W1, P.W2, P.W3, P.W4, P.W5):
            flat[off:off + W.numel()].copy_(W.reshape(-1))
            off += W.numel()
    return m


@pytest.fixture(scope="module")
def blob_model(dev):
    """The end-to-end model is not a trained synthetic scene (training one takes longer than a test may):
    it is mesh_ref.blob_params(), a smooth blob in the dense coarsest level with every hashed level zero,
    so that the surface and the oracle's normal share are known.  The hashed levels take part through
    `hashed_model` below."""
    return _model_from(mesh_ref.blob_params()[0], dev)


@pytest.fixture(scope="module")
def hashed_model(dev):
    """Every level of the table drawn from U(-0.5, 0.5), as the field's own tests do: all 16 levels, the
    hashed ones included, shape the density."""
    return _model_from(field_ref.init_params(seed=3, table_init=0.5)[0], dev)


def test_density_lattice_is_model_density_at_the_lattice_points(dev, blob_model):
    res = (24, 24, 24)
    pos = torch.from_numpy(mesh_ref.lattice_positions(res, *BOX)).to(dev)
    with torch.no_grad():
        want = blob_model.density(pos)
    for chunk in (2 ** 22, 5000):  # one chunk; four chunks with a ragged last one
        got = mesh.density_lattice(blob_model, 24, chunk=chunk)
        assert got.shape == (25, 25, 25) and got.dtype == torch.float32
        assert torch.equal(got.reshape(-1).view(torch.int32), want.view(torch.int32)), chunk
    assert float(want.max() / want.min()) > 1.05  # (the blob is there)
    # another box and resolution per axis
    got = mesh.density_lattice(blob_model, (5, 6, 7), lo=(-0.2, -0.3, -0.1), hi=(0.4, 0.1, 0.3))
    pos = torch.from_numpy(mesh_ref.lattice_positions((5, 6, 7), (-0.2, -0.3, -0.1), (0.4, 0.1, 0.3))).to(dev)
    with torch.no_grad():
        assert torch.equal(got.reshape(-1), blob_model.density(pos))


def test_density_lattice_with_every_hashed_level(dev, hashed_model):
    res, lo, hi = (24, 24, 24), *BOX
    pos = torch.from_numpy(mesh_ref.lattice_positions(res, lo, hi)).to(dev)
    with torch.no_grad():
        want = hashed_model.density(pos)
    assert float(want.std() / want.mean()) > 0.05  # (the levels do shape it: 0.09 in the oracle)
    for chunk in (2 ** 22, 5000):
        got = mesh.density_lattice(hashed_model, 24, chunk=chunk)
        assert torch.equal(got.reshape(-1).view(torch.int32), want.view(torch.int32)), chunk
    # the mesh of that rough field is the oracle's on the same lattice, and its normals are unit vectors
    iso = float(want.median())
    v, f, n = mesh.extract_mesh(hashed_model, res=24, iso=iso, normals=True)
    assert_same_mesh((v.cpu().numpy(), f.cpu().numpy()), mesh_ref.extract(got.cpu().numpy(), lo, hi, iso))
    assert len(v) > 10000 and bool(torch.isfinite(n).all())
    assert float((n.norm(dim=1) - 1).abs().max()) < 1e-5


def test_vertex_normals_stay_finite_where_the_density_leaves_the_fp16_range(dev, blob_model):
    """sigma = exp(h): with the blob's features scaled by 600 h reaches 57, by -1500 it reaches -23 (the
    oracle's figures), past TruncExp's clamp at +-15 on either side.  The normals are unit vectors or, where the gradient is zero or
    not finite, the zero vector; never NaN or Inf."""
    flat, n_table = blob_model.flat_params(), blob_model._n_table
    saved = flat[:n_table].clone()
    x = (torch.rand(4099, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) - 0.5) * 0.98
    try:
        for scale in (600.0, -1500.0):
            with torch.no_grad():
                flat[:n_table].copy_(saved * scale)
                s = blob_model.density(x)
            assert float(s.max()) > math.exp(16) or float(s.min()) < math.exp(-16)
            n = mesh.vertex_normals(blob_model, x)
            norm = n.norm(dim=1)
            assert bool(torch.isfinite(n).all())
            assert bool((((norm - 1).abs() < 1e-5) | (norm == 0)).all()) and float((norm > 0).float().mean()) > 0.5
    finally:
        with torch.no_grad():
            flat[:n_table].copy_(saved)
        blob_model._packed_fresh = False


def test_occupancy_never_hands_an_inactive_point_to_the_density_pass(dev, blob_model, monkeypatch):
    occ = np.zeros((128, 128, 128), bool)
    occ[:64] = True  # x < 0
    blob_model.density_bitfield.copy_(torch.from_numpy(mesh_ref.pack_bitfield(occ)).to(dev))
    res = (24, 24, 24)
    active = mesh_ref.active_cells(res, *BOX, mesh_ref.pack_bitfield(occ), 128, 0.5)
    assert active[:, :, :12].all() and not active[:, :, 12:].any()
    listed = mesh_ref.points_with_active_cell(active)
    seen = []
    density = blob_model.density
    monkeypatch.setattr(blob_model, "density", lambda x: (seen.append(x.detach().clone()), density(x))[1])
    lattice = mesh.density_lattice(blob_model, 24, chunk=5000, occupancy=True)
    x = torch.cat(seen).cpu().numpy()
    assert len(x) == int(listed.sum()) == 25 * 25 * 13
    pos = mesh_ref.lattice_positions(res, *BOX)[listed.reshape(-1)]
    order = lambda a: a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
    assert np.array_equal(bits(order(x)), bits(order(pos)))
    monkeypatch.undo()
    full = mesh.density_lattice(blob_model, 24)
    assert torch.equal(lattice[:, :, :13], full[:, :, :13]) and not lattice[:, :, 13:].any()
    # the culled mesh is the oracle's on that lattice: open where the surface leaves the occupied half
    iso = float((full.min() + full.max()) * 0.5)
    v, f = mesh.extract_mesh(blob_model, res=24, iso=iso, occupancy=True)
    want = mesh_ref.extract(lattice.cpu().numpy(), *BOX, iso, active)
    assert_same_mesh((v.cpu().numpy(), f.cpu().numpy()), want)
    assert set(mesh_ref.undirected_edge_uses(want[1]).values()) == {1, 2}
    blob_model.density_bitfield.zero_()


def test_extract_mesh_normals(dev, blob_model):
    """The share of vertices whose unit normal -grad sigma / |grad sigma| has a positive dot with the
    normal of their first incident face.  The oracle pipeline on this input (mesh_ref.oracle_normal_share:
    oracle/field_ref.py's density on the lattice, tests/mesh_ref.py's extraction, central differences of
    that density with step 1e-3 for the gradient) reaches 1756 of 1756 vertices with the fp32 field and
    1750 of 1750 with its fp16 emulation, share 1.000 both times (F = 3508 / 3496, Euler characteristic 2):
    tests/test_mesh_host.py::test_oracle_pipeline_normal_share measures it on the host.  The bound is
    mesh_ref.NORMAL_SHARE_BOUND = 0.99: the device's fp16 field against central differences may turn the
    sign at a sliver."""
    sigma = mesh.density_lattice(blob_model, 24)
    iso = float((sigma.min() + sigma.max()) * 0.5)
    grad_before = blob_model.flat_grad().clone()
    v, f, n = mesh.extract_mesh(blob_model, res=24, iso=iso, normals=True)
    assert torch.equal(blob_model.flat_grad(), grad_before)  # the parameters' gradients are not touched
    assert all(p.requires_grad for p in blob_model.parameters())
    v2, f2 = mesh.extract_mesh(blob_model, res=24, iso=iso)
    assert torch.equal(v, v2) and torch.equal(f, f2)
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy().astype(np.float64)
    assert_same_mesh((v, f), mesh_ref.extract(sigma.cpu().numpy(), *BOX, iso))
    mesh_ref.check_closed_surface(v, f, 2)
    assert 1500 < len(v) < 2000  # (the oracle's own lattice gives 1750 .. 1756)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5
    assert np.isfinite(n).all()
    share = mesh_ref.normal_share(v, f, n)
    print(f"normal share {share:.4f} over {len(v)} vertices")
    assert share >= mesh_ref.NORMAL_SHARE_BOUND


# ---- determinism ----
def test_two_calls_are_bit_identical(dev, blob_model):
    sigma = torch.from_numpy(np.random.default_rng(1).standard_normal((19, 23, 40)).astype(np.float32)).to(dev)
    a, b = mesh.extract_isosurface(sigma, *ANISO, 0.05), mesh.extract_isosurface(sigma, *ANISO, 0.05)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and len(a[1]) > 1000
    x, y = mesh.density_lattice(blob_model, 24, chunk=5000), mesh.density_lattice(blob_model, 24, chunk=5000)
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))
