"""The isosurface definition of include/ncnerf_mesh.h restated in NumPy, independently of csrc/mesh.hip:
the oracle of tests/test_mesh_host.py (which pins it with closed forms) and tests/test_gpu_mesh.py.

Everything that reaches the output is float32 with one rounding per operation, as the header states,
so `extract` is bit for bit what the kernels must give.  The rule that turns a tetrahedron's inside
corners into oriented triangles is evaluated here as written (`tet_triangles`), per case and per
tetrahedron; no table is shared with the library.
"""
import itertools
import math

import numpy as np

F32 = np.float32
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def perm_sign(p):
    inv = sum(1 for i in range(len(p)) for j in range(i + 1, len(p)) if p[i] > p[j])
    return -1 if inv & 1 else 1


def axis_positions(n, lo, hi):
    """lo + (float)i * h, h = (hi - lo) / (float)n, in float32."""
    h = (F32(hi) - F32(lo)) / F32(n)
    return F32(lo) + np.arange(n + 1, dtype=F32) * h


def lattice_positions(res, lo, hi):
    """(P, 3) float32 positions in point order p = (iz (ny+1) + iy)(nx+1) + ix."""
    xs, ys, zs = (axis_positions(res[a], lo[a], hi[a]) for a in range(3))
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3)


def sample(fn, res, lo, hi):
    """fn(x, y, z) (float64 arrays in, anything out) on the lattice -> (nz+1, ny+1, nx+1) float32."""
    p = lattice_positions(res, lo, hi).astype(np.float64)
    return np.asarray(fn(p[:, 0], p[:, 1], p[:, 2])).astype(F32).reshape(res[2] + 1, res[1] + 1, res[0] + 1)


def tet_triangles(inside, sign):
    """Triangles of one tetrahedron: `inside` = 4 bools in path order (v0..v3), sign = the permutation's.
    Each triangle is three edges (i, j), i < j: the vertex on the edge v_i v_j."""
    E = lambda a, b: (min(a, b), max(a, b))
    ins = [v for v in range(4) if inside[v]]
    outs = [v for v in range(4) if not inside[v]]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (i, j), (k, l) = ins, outs
        quad = [E(i, k), E(i, l), E(j, l), E(j, k)]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        o = sign * perm_sign((i, j, k, l))
    else:
        i = ins[0] if len(ins) == 1 else outs[0]
        j, k, l = outs if len(ins) == 1 else ins
        tris = [[E(i, j), E(i, k), E(i, l)]]
        o = sign * perm_sign((i, j, k, l)) * (1 if len(ins) == 1 else -1)
    if o < 0:
        tris = [[t[0], t[2], t[1]] for t in tris]
    return tris


def morton3d(x, y, z):
    def expand(v):
        v = v.astype(np.uint64)
        out = np.zeros_like(v)
        for b in range(10):
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
        return out
    return expand(x) | (expand(y) << np.uint64(1)) | (expand(z) << np.uint64(2))


def active_cells(res, lo, hi, bitfield, grid_size, scale):
    """(nz, ny, nx) bool: the occupancy cell (cascade 0) around the cell's centre is set.  The marcher's
    lookup: n = (int)clamp(0.5 * fma(x, 1 / b, 1) * G, 0, G - 1), b = min(0.5, scale).  The fma is taken
    in float64 (the product of two float32 is exact there) and rounded once to float32."""
    b = min(F32(0.5), F32(scale))
    inv = F32(1.0) / b
    n = []
    for a in range(3):
        h = (F32(hi[a]) - F32(lo[a])) / F32(res[a])
        c = F32(lo[a]) + (np.arange(res[a], dtype=F32) + F32(0.5)) * h
        f = (c.astype(np.float64) * np.float64(inv) + 1.0).astype(F32)
        v = F32(0.5) * f * F32(grid_size)
        n.append(np.clip(v, F32(0), F32(grid_size - 1)).astype(np.int64))
    Z, Y, X = np.meshgrid(n[2], n[1], n[0], indexing="ij")
    idx = morton3d(X, Y, Z).astype(np.int64)
    bits = np.asarray(bitfield, dtype=np.uint8)
    return ((bits[idx >> 3] >> (idx & 7).astype(np.uint8)) & 1).astype(bool)


def points_with_active_cell(active):
    """(nz+1, ny+1, nx+1) bool: the point has at least one active incident cell."""
    nz, ny, nx = active.shape
    out = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        out[dz:dz + nz, dy:dy + ny, dx:dx + nx] |= active
    return out


def extract(sigma, lo, hi, iso, active=None):
    """-> (verts (V, 3) float32, faces (F, 3) int64) of the header's definition."""
    sigma = np.asarray(sigma, dtype=F32)
    nz, ny, nx = (s - 1 for s in sigma.shape)
    iso = F32(iso)
    with np.errstate(invalid="ignore"):
        inside = sigma >= iso
    if active is None:
        active = np.ones((nz, ny, nx), bool)
    A = np.zeros((nz + 2, ny + 2, nx + 2), bool)  # cell c at index c + 1; cells outside the lattice are inactive
    A[1:-1, 1:-1, 1:-1] = active
    pos = [axis_positions(n, lo[a], hi[a]) for a, n in enumerate((nx, ny, nz))]
    P = (nx + 1) * (ny + 1) * (nz + 1)

    # ---- edges: kind d - 1 for the direction d = dx + 2 dy + 4 dz, owned by the lower endpoint ----
    cross = np.zeros((nz + 1, ny + 1, nx + 1, 7), bool)
    for d in range(1, 8):
        dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
        lower = (slice(0, nz + 1 - dz), slice(0, ny + 1 - dy), slice(0, nx + 1 - dx))
        upper = (slice(dz, nz + 1), slice(dy, ny + 1), slice(dx, nx + 1))
        in_cell = np.zeros((nz + 1, ny + 1, nx + 1), bool)  # the edge lies in at least one active cell
        for oz in ((0,) if dz else (0, 1)):
            for oy in ((0,) if dy else (0, 1)):
                for ox in ((0,) if dx else (0, 1)):
                    in_cell |= A[1 - oz:nz + 2 - oz, 1 - oy:ny + 2 - oy, 1 - ox:nx + 2 - ox]
        cross[lower + (d - 1,)] = (inside[lower] != inside[upper]) & in_cell[lower]
    flat = cross.reshape(-1)
    number = (np.cumsum(flat, dtype=np.int64) - flat).reshape(P, 7)  # exclusive scan over (point, kind)
    V = int(flat.sum())
    verts = np.zeros((V, 3), F32)
    iz, iy, ix = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    with np.errstate(all="ignore"):
        for d in range(1, 8):
            sel = cross[..., d - 1]
            if not sel.any():
                continue
            dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
            ax, ay, az = ix[sel], iy[sel], iz[sel]
            sa, sb = sigma[az, ay, ax], sigma[az + dz, ay + dy, ax + dx]
            t = np.where(np.isfinite(sa) & np.isfinite(sb), (iso - sa) / (sb - sa), F32(0.5)).astype(F32)
            n = number.reshape(nz + 1, ny + 1, nx + 1, 7)[..., d - 1][sel]
            for a, (ia, ib) in enumerate(((ax, ax + dx), (ay, ay + dy), (az, az + dz))):
                pa, pb = pos[a][ia], pos[a][ib]
                verts[n, a] = pa + t * (pb - pa)

    # ---- faces: per cell, per tetrahedron, per case ----
    corner_inside = [inside[(d >> 2):(d >> 2) + nz, ((d >> 1) & 1):((d >> 1) & 1) + ny, (d & 1):(d & 1) + nx]
                     for d in range(8)]
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cell = (cz * ny + cy) * nx + cx
    keys, tris_out = [], []
    for t, perm in enumerate(PERMS):
        a, b, _ = perm
        corners = (0, 1 << a, (1 << a) | (1 << b), 7)
        sign = perm_sign(perm)
        case = sum(corner_inside[corners[v]].astype(np.int64) << v for v in range(4))
        for bits in range(1, 15):
            sel = active & (case == bits)
            if not sel.any():
                continue
            tris = tet_triangles([(bits >> v) & 1 for v in range(4)], sign)
            for q, tri in enumerate(tris):
                cols = []
                for (i, j) in tri:
                    o, d = corners[i], corners[j] - corners[i]
                    p = ((cz[sel] + (o >> 2)) * (ny + 1) + cy[sel] + ((o >> 1) & 1)) * (nx + 1) + cx[sel] + (o & 1)
                    assert cross.reshape(P, 7)[p, d - 1].all()
                    cols.append(number[p, d - 1])
                keys.append((cell[sel] * 6 + t) * 2 + q)
                tris_out.append(np.stack(cols, -1))
    if not keys:
        return verts, np.zeros((0, 3), np.int64)
    keys, faces = np.concatenate(keys), np.concatenate(tris_out)
    return verts, faces[np.argsort(keys, kind="stable")].astype(np.int64)


# ---- helpers for the assertions ----
def canonical(faces):
    """Each triangle rotated to start at its smallest index (orientation kept), rows sorted."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return f
    k = np.argmin(f, axis=1)
    rot = np.stack([f[np.arange(len(f)), (k + s) % 3] for s in range(3)], -1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def directed_edge_uses(faces):
    """{(a, b): how many faces run a -> b}."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(uniq, counts)}


def undirected_edge_uses(faces):
    out = {}
    for (a, b), c in directed_edge_uses(faces).items():
        k = (min(a, b), max(a, b))
        out[k] = out.get(k, 0) + c
    return out


def euler(n_verts, faces):
    return n_verts - len(undirected_edge_uses(faces)) + len(faces)


def is_closed_oriented(faces):
    """Every undirected edge in exactly two faces and every directed edge exactly once."""
    return (all(c == 2 for c in undirected_edge_uses(faces).values())
            and all(c == 1 for c in directed_edge_uses(faces).values()))


def face_normals_area(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    return 0.5 * np.cross(b - a, c - a)  # (F, 3): direction = normal, length = area


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- closed forms and what they must satisfy (shared by the host and the device tests) ----
def sphere(c, R):
    return lambda x, y, z: R - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)


def sphere_volume_bounds(R, h):
    """The mesh is the zero set of the piecewise-linear interpolant of f = R - |x - c| over tetrahedra of
    diameter D = sqrt(3) h.  |f - interpolant| <= M D^2 / 2 with M = 1 / (R - D) bounding f's second
    derivatives within D of the sphere, and f has slope 1 along the radius, so the mesh lies between the
    spheres of radius R - e and R + e, e = 3 h^2 / (2 (R - sqrt(3) h)).  f is concave, so every vertex (the
    zero of a chord of f) lies inside the closed ball, and so does the mesh: volume <= 4/3 pi R^3.
    (1e-5 relative for the float32 vertices.)"""
    e = 3 * h * h / (2 * (R - math.sqrt(3) * h))
    return 4 / 3 * math.pi * (R - e) ** 3 * (1 - 1e-5), 4 / 3 * math.pi * R ** 3 * (1 + 1e-5)


def check_closed_surface(verts, faces, chi):
    assert len(faces) > 0 and faces.min() >= 0 and faces.max() == len(verts) - 1
    assert len(np.unique(faces)) == len(verts)  # indexed: no vertex is left unused
    assert is_closed_oriented(faces)
    assert euler(len(verts), faces) == chi


def torus(x, y, z, R=0.3, r=0.12):
    return r - np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z)


def pack_bitfield(occ):
    """(G, G, G) bool occupancy indexed [x][y][z] -> the G^3 / 8 bytes of cascade 0 (bit morton3d(x, y, z))."""
    G = occ.shape[0]
    x, y, z = np.nonzero(occ)
    bits = np.zeros(G ** 3, np.uint8)
    bits[morton3d(x, y, z).astype(np.int64)] = 1
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


# ---- the end-to-end input and the oracle pipeline's normal share ----
NORMAL_SHARE_BOUND = 0.99  # what tests/test_gpu_mesh.py asks of the device; the oracle pipeline reaches 1.000


def blob_params():
    """Oracle field parameters (oracle/field_ref.py) whose density is a smooth blob: every level of the
    table zero but the coarsest, which is dense (16^3 nodes, index x + 16 y + 256 z, node g at
    (g - 0.5) / 15 of the box) and holds a Gaussian in both features.  The encoding is then a non-negative
    multiple of one vector, sigma_net is positively homogeneous, so sigma = exp(k * blob) with one
    constant k (> 0 for this seed): the level sets are those of the trilinearly interpolated blob.  The
    hashed levels take no part in this model."""
    import torch
    from oracle import field_ref
    P, levels = field_ref.init_params(seed=8)
    P.table.zero_()
    g = (torch.arange(16, dtype=torch.float64) - 0.5) / 15.0 - 0.5
    Z, Y, X = torch.meshgrid(g, g, g, indexing="ij")
    f = torch.exp(-((X - 0.03) ** 2 + (Y + 0.02) ** 2 + (Z - 0.01) ** 2) / (2 * 0.2 ** 2)).float().reshape(-1)
    P.table[:4096, 0] = f
    P.table[:4096, 1] = f
    return P, levels


def normal_share(verts, faces, normals):
    """The share of vertices whose normal has a positive dot with the normal of their first incident face
    (first in face order; a degenerate face counts against the share)."""
    first = np.full(len(verts), len(faces))
    for k in range(3):
        np.minimum.at(first, faces[:, k], np.arange(len(faces)))
    dots = (np.asarray(normals, dtype=np.float64) * face_normals_area(verts, faces)[first]).sum(1)
    return float((dots > 0).mean())


def oracle_normal_share(res=24, emulate=None, eps=1e-3):
    """The oracle pipeline on the blob: oracle/field_ref.py's density on the lattice of the box
    [-0.5, 0.5]^3 (emulate: None for fp32, "fp16" for the kernels' operand rounding), iso midway between
    the lattice's extremes, `extract`, and -grad sigma by central differences of the fp32 density with step
    eps.  -> (share, V, F, Euler characteristic)."""
    import torch
    from oracle import field_ref
    P, levels = blob_params()
    lo, hi = (-0.5,) * 3, (0.5,) * 3
    pos = torch.from_numpy(lattice_positions((res,) * 3, lo, hi))
    sigma = field_ref.density(pos, P, levels, emulate=emulate).numpy().reshape(res + 1, res + 1, res + 1)
    iso = float((F32(sigma.min()) + F32(sigma.max())) * F32(0.5))
    verts, faces = extract(sigma, lo, hi, iso)
    x = torch.from_numpy(verts).clone()
    axes = torch.eye(3)
    grad = torch.stack([(field_ref.density(x + eps * axes[a], P, levels) - field_ref.density(x - eps * axes[a], P, levels))
                        / (2 * eps) for a in range(3)], 1).numpy().astype(np.float64)
    normals = -grad / np.maximum(np.linalg.norm(grad, axis=1, keepdims=True), 1e-30)
    return normal_share(verts, faces, normals), len(verts), len(faces), euler(len(verts), faces)
