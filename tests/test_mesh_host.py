"""Isosurface extraction on a host without a GPU: include/ncnerf_mesh.h parses into a table of its own
and binds; ncnerf_amd.mesh refuses wrong arguments before the library is reached and writes a PLY that
reads back; and the NumPy restatement of the definition (tests/mesh_ref.py), the oracle of the GPU
tests, is pinned by closed forms: a plane, a sphere, two spheres, a torus."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import mesh_ref
from ncnerf_amd import _lib, mesh
from ncnerf_amd._lib import F32, I32, I64, P
from test_abi import NAMES as ALL_NAMES, altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ncnerf_mesh.h"
NAMES = ALL_NAMES[HEADER]
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


# ---- the ABI ----
def test_mesh_header_parses_into_a_table_of_its_own():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    assert set(_lib.symbols(HEADER)) == NAMES <= set(_lib.exported_symbols())


def test_known_signatures():
    box = [F32] * 6
    assert _lib.SIGNATURES["ncn_mesh_points"] == [I64, I64, I64] + box + [I64, I64, P, I32, F32, P, P, P, P]
    assert _lib.SIGNATURES["ncn_mesh_count"] == [P, I64, I64, I64] + box + [F32, P, I32, F32, P, P, P]
    assert _lib.SIGNATURES["ncn_mesh_scan"] == [P, I64, I32, P, P, P, P]
    assert _lib.SIGNATURES["ncn_mesh_emit_verts"] == [P, I64, I64, I64] + box + [F32, P, P, P, P, I64, P]
    assert _lib.SIGNATURES["ncn_mesh_emit_faces"] == [P, I64, I64, I64, F32, P, P, P, P, P, P, P, I64, P]
    scan = _lib.ABI["ncn_mesh_scan"][1]
    assert scan[0] == ("ptr", 1, "in") and scan[3] == ("ptr", 2, "local") and scan[4] == ("ptr", 8, "block_base")


def test_library_binds_the_new_names_as_int():
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name]


def test_header_constants_match_the_package():
    text = _lib.read_header(HEADER)
    got = {k: int(v) for k, v in re.findall(r"^#define NCN_MESH_(\w+) (\d+)$", text, flags=re.M)}
    assert got == {"TILE_X": mesh.TILE[0], "TILE_Y": mesh.TILE[1], "TILE_Z": mesh.TILE[2],
                   "SCAN_ELEMS": mesh.SCAN_ELEMS, "SCAN_SWEEP": mesh.SCAN_SWEEP}
    assert mesh.SCAN_ELEMS * 15 < 2 ** 16  # a block's offsets (popcounts <= 7, face counts <= 12) fit uint16
    assert [mesh.blocks(n) for n in (1, mesh.SCAN_ELEMS, mesh.SCAN_ELEMS + 1)] == [1, 1, 2]


def test_a_name_in_two_headers_is_an_error(tmp_path):
    clash = altered_headers(tmp_path, HEADER, "int ncn_mesh_count(int a, void* stream);\n"
                                              "int ncn_geom_loss_fwd(int a, void* stream);\n")
    with pytest.raises(_lib.NcnError, match="ncn_geom_loss_fwd is declared in include/ncnerf_mesh.h and in "
                                            "include/ncnerf_geom.h"):
        _lib.load_headers(clash)
    twice = altered_headers(tmp_path, HEADER, "int ncn_mesh_count(int a, void* stream);\n"
                                              "int ncn_mesh_count(int b, void* stream);\n")
    with pytest.raises(ValueError, match="ncn_mesh_count is declared twice"):
        _lib.load_headers(twice)


def test_missing_mesh_header_names_the_path(tmp_path):
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*isosurface extraction"):
        _lib.load_headers(gone)


# ---- refusals precede the call ----
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    monkeypatch.setattr(_lib, "stream", lambda: P(0x5EED))


def test_entry_points_refuse_host_tensors_and_wrong_widths(no_library):
    d = P(16)
    with pytest.raises(TypeError, match=r"ncn_mesh_count: argument 0 \(sigma\).*CUDA.*float32 cpu tensor"):
        _lib.call("ncn_mesh_count", torch.zeros(8), 1, 1, 1, 0., 0., 0., 1., 1., 1., 0., None, 0, 0., d, d)
    with pytest.raises(TypeError, match=r"ncn_mesh_scan: argument 3 \(local\).*2-byte"):
        _lib.call("ncn_mesh_scan", d, 8, 1, torch.zeros(8, dtype=torch.int32), d, d)
    with pytest.raises(TypeError, match=r"ncn_mesh_scan: takes 6 or 7 arguments, got 2"):
        _lib.call("ncn_mesh_scan", d, 8)
    with pytest.raises(TypeError, match=r"argument 1 \(nx\)"):
        _lib.call("ncn_mesh_emit_faces", d, torch.tensor(1), 1, 1, 0., d, d, d, d, d, d, d, 0)


def _model(**over):
    m = types.SimpleNamespace(density=lambda x: pytest.fail("the model was evaluated"), xyz_min=-torch.ones(1, 3) * 0.5,
                              xyz_max=torch.ones(1, 3) * 0.5, density_bitfield=torch.zeros(64, dtype=torch.uint8),
                              grid_size=8, scale=0.5)
    m.__dict__.update(over)
    return m


def test_mesh_argument_checks(no_library):
    s = torch.zeros(3, 3, 3)
    with pytest.raises(RuntimeError, match="sigma must be a CUDA tensor"):
        mesh.extract_isosurface(s, *BOX, 0.0)
    with pytest.raises(RuntimeError, match="sigma must be a CUDA tensor"):
        mesh.extract_isosurface(np.zeros((3, 3, 3), np.float32), *BOX, 0.0)
    with pytest.raises(ValueError, match="lo < hi"):
        mesh.extract_isosurface(s, (0, 0, 0), (1, 0, 1), 0.0)
    with pytest.raises(ValueError, match="lo must be 3 finite numbers"):
        mesh.extract_isosurface(s, (0, 0), (1, 1, 1), 0.0)
    with pytest.raises(ValueError, match="hi must be 3 finite numbers"):
        mesh.extract_isosurface(s, (0, 0, 0), (1, float("inf"), 1), 0.0)
    for iso in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iso must be finite"):
            mesh.extract_isosurface(s, *BOX, iso)
    for res in (0, (4, 4), (4, 0, 4), (4, 4, 2.5), -3):
        with pytest.raises(ValueError, match="res must be"):
            mesh.density_lattice(_model(), res)
        with pytest.raises(ValueError, match="res must be"):
            mesh.extract_mesh(_model(), res=res)
    with pytest.raises(ValueError, match="iso must be finite"):
        mesh.extract_mesh(_model(), res=4, iso=float("nan"))
    with pytest.raises(ValueError, match="lo < hi"):
        mesh.density_lattice(_model(), 4, lo=(0.6, 0, 0))  # above the model's xyz_max
    with pytest.raises(ValueError, match="chunk"):
        mesh.density_lattice(_model(), 4, chunk=0)
    with pytest.raises(ValueError, match="model must be an NGPMT"):
        mesh.density_lattice(object(), 4)
    # well-formed arguments pass every check and stop at the device
    with pytest.raises(RuntimeError, match="model.xyz_min must be a CUDA tensor"):
        mesh.density_lattice(_model(), (4, 5, 6))
    with pytest.raises(RuntimeError, match="model.xyz_min must be a CUDA tensor"):
        mesh.extract_mesh(_model(), res=4, occupancy=True, normals=True)
    with pytest.raises(RuntimeError, match="verts must be a CUDA tensor"):
        mesh.vertex_normals(_model(), torch.zeros(4, 3))


# ---- PLY ----
def _read_ply(path):
    data = open(path, "rb").read()
    head, payload = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    V = int(re.search(r"element vertex (\d+)", head.decode()).group(1))
    F = int(re.search(r"element face (\d+)", head.decode()).group(1))
    props = re.findall(r"property float (\w+)", head.decode())
    assert "property list uchar int vertex_indices" in lines
    v = np.frombuffer(payload, "<f4", V * len(props)).reshape(V, len(props))
    f = np.frombuffer(payload, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), F, offset=V * len(props) * 4)
    assert len(payload) == V * len(props) * 4 + F * 13
    return props, v, f


@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_round_trip(tmp_path, with_normals):
    g = torch.Generator().manual_seed(3)
    verts = torch.randn(7, 3, generator=g)
    faces = torch.randint(0, 7, (5, 3), generator=g)
    normals = torch.randn(7, 3, generator=g) if with_normals else None
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path, verts, faces, normals)
    props, v, f = _read_ply(path)
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert np.array_equal(v[:, :3], verts.numpy()) and (f["n"] == 3).all() and np.array_equal(f["i"], faces.numpy())
    if with_normals:
        assert np.array_equal(v[:, 3:], normals.numpy())
    mesh.save_ply(path, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))  # the empty mesh
    assert _read_ply(path)[1].shape == (0, 3)
    with pytest.raises(ValueError, match=r"verts must be \(V, 3\)"):
        mesh.save_ply(path, torch.zeros(4, 2), faces)
    with pytest.raises(ValueError, match="normals must be"):
        mesh.save_ply(path, verts, faces, torch.zeros(6, 3))


# ---- the rule of one tetrahedron ----
def test_tet_rule_orients_every_case_toward_the_outside():
    """On a geometric tetrahedron of either sign, with the edge vertices at the midpoints, every
    triangle's normal has a positive dot with (centroid of the outside corners - centroid of the
    inside corners), and the 2-2 quad's two triangles share its diagonal."""
    for perm in mesh_ref.PERMS:
        a, b, c = perm
        e = np.eye(3)
        v = np.array([np.zeros(3), e[a], e[a] + e[b], e[a] + e[b] + e[c]])
        sign = mesh_ref.perm_sign(perm)
        assert np.sign(np.linalg.det(v[1:] - v[0])) == sign
        for bits in range(16):
            inside = [(bits >> k) & 1 for k in range(4)]
            tris = mesh_ref.tet_triangles(inside, sign)
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside)]
            if not tris:
                continue
            out_dir = v[[k for k in range(4) if not inside[k]]].mean(0) - v[[k for k in range(4) if inside[k]]].mean(0)
            for tri in tris:
                assert all(inside[i] != inside[j] and i < j for i, j in tri)
                p = [(v[i] + v[j]) / 2 for i, j in tri]
                assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), out_dir) > 0, (perm, bits, tri)
            if len(tris) == 2:
                assert tris[0][0] == tris[1][0] and len(set(tris[0]) & set(tris[1])) == 2 and len(set(tris[0] + tris[1])) == 4


# ---- closed forms ----
def test_plane():
    """sigma = iso + (c - x): the surface is the box's cross-section x = c, facing +x (lower density).
    Every vertex lies at x = c within one ulp of c in float32 (the linear interpolation of a linear
    function is exact up to its roundings)."""
    res, (lo, hi), c, iso = (5, 4, 3), ((-0.5, -0.4, -0.3), (0.5, 0.6, 0.3)), 0.13, 0.0
    sigma = mesh_ref.sample(lambda x, y, z: iso + (c - x), res, lo, hi)
    verts, faces = mesh_ref.extract(sigma, lo, hi, iso)
    err = np.abs(verts[:, 0].astype(np.float64) - c).max()
    print(f"plane: max |x_v - c| = {err:.3e} = {err / np.spacing(np.float32(c)):.2f} ulp of c")
    assert len(verts) > 0 and err <= np.spacing(np.float32(c))
    n = mesh_ref.face_normals_area(verts, faces)
    area = np.linalg.norm(n, axis=1)
    assert abs(area.sum() - (hi[1] - lo[1]) * (hi[2] - lo[2])) <= 1e-6 * area.sum()
    assert (area > 0).all() and (n[:, 0] / area >= 1 - 1e-6).all()
    # border edges (on the box faces) are used once, interior edges twice
    uses = mesh_ref.undirected_edge_uses(faces)
    assert set(uses.values()) == {1, 2}
    on_face = lambda v: bool((np.isclose(verts[v, 1:], np.array(lo[1:], np.float32))
                              | np.isclose(verts[v, 1:], np.array(hi[1:], np.float32))).any())
    for (a, b), k in uses.items():
        if k == 1:
            assert on_face(a) and on_face(b)


def test_sphere():
    res, R, c = (20, 20, 20), 0.3, (0.013, -0.021, 0.007)
    verts, faces = mesh_ref.extract(mesh_ref.sample(mesh_ref.sphere(c, R), res, *BOX), *BOX, 0.0)
    mesh_ref.check_closed_surface(verts, faces, 2)
    lo_v, hi_v = mesh_ref.sphere_volume_bounds(R, 1.0 / 20)
    vol = mesh_ref.signed_volume(verts, faces)
    assert vol > 0 and lo_v <= vol <= hi_v, (lo_v, vol, hi_v)
    r = np.linalg.norm(verts.astype(np.float64) - np.array(c), axis=1)
    assert r.max() <= R * (1 + 1e-6)


def test_two_spheres():
    f1, f2 = mesh_ref.sphere((-0.22, 0.0, 0.0), 0.17), mesh_ref.sphere((0.22, 0.05, 0.0), 0.15)
    sigma = mesh_ref.sample(lambda x, y, z: np.maximum(f1(x, y, z), f2(x, y, z)), (24, 16, 16), *BOX)
    mesh_ref.check_closed_surface(*mesh_ref.extract(sigma, *BOX, 0.0), 4)


def test_torus():
    verts, faces = mesh_ref.extract(mesh_ref.sample(mesh_ref.torus, (24, 24, 12), *BOX), *BOX, 0.0)
    mesh_ref.check_closed_surface(verts, faces, 0)
    assert mesh_ref.signed_volume(verts, faces) > 0


def test_iso_level_and_anisotropic_box_move_the_sphere_as_they_should():
    """The same sphere at iso = 0.05 is the sphere of radius R - 0.05."""
    res, R = (18, 14, 10), 0.3
    verts, faces = mesh_ref.extract(mesh_ref.sample(mesh_ref.sphere((0, 0, 0), R), res, *BOX), *BOX, 0.05)
    mesh_ref.check_closed_surface(verts, faces, 2)
    r = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert r.max() <= (R - 0.05) * (1 + 1e-6) and r.min() >= R - 0.05 - 3 * 0.1 ** 2 / (2 * (0.25 - math.sqrt(3) * 0.1)) - 1e-6


# ---- the oracle pipeline's own normal share (the source of the device test's bound) ----
@pytest.mark.parametrize("emulate,V,F", [(None, 1756, 3508), ("fp16", 1750, 3496)])
def test_oracle_pipeline_normal_share(emulate, V, F):
    """What tests/test_gpu_mesh.py::test_extract_mesh_normals cites: on the blob the oracle pipeline's
    normals agree with the first incident face at every vertex, comfortably inside the 0.99 asked of the
    device."""
    share, n_verts, n_faces, chi = mesh_ref.oracle_normal_share(emulate=emulate)
    print(f"oracle normal share {share:.4f} over {n_verts} vertices, {n_faces} faces, chi {chi}")
    assert (n_verts, n_faces, chi) == (V, F, 2)
    assert share == 1.0 and share > mesh_ref.NORMAL_SHARE_BOUND
