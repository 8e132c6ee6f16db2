"""Isosurface mesh extraction from the trained density field (csrc/mesh.hip, include/ncnerf_mesh.h).

The reference has no counterpart: the header states the definition (a Kuhn split of every lattice cell
into six tetrahedra, vertices owned by the lower endpoint of their edge and numbered by an ordered
scan, faces in cell order with their normals toward lower density), tests/mesh_ref.py restates it.
The mesh is a function of the lattice alone: two calls give the same bits.

    extract_isosurface(sigma, lo, hi, iso)   any (Nz+1, Ny+1, Nx+1) float32 CUDA lattice -> (verts, faces)
    density_lattice(model, res)              NGPMT.density on the lattice points, chunk by chunk
    extract_mesh(model, res=256, iso=...)    the two above (+ unit vertex normals -grad sigma / |grad sigma|)
    save_ply(path, verts, faces)             binary little-endian PLY

Occupancy culling (`occupancy=`): a lattice cell is active when the occupancy cell (cascade 0) that
contains its centre is set in the model's density bitfield, by the marcher's own lookup.  Inactive cells
emit nothing and points with no active incident cell are never evaluated (their density counts as 0).
This matches what the renderer can see and skips most of the volume, but the surface is left OPEN
where it leaves the occupied region: border edges there are used by one face only.  Off by default.

No CPU fallback: a CPU tensor raises.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._lib import call


_C = _lib.CONSTANTS
TILE = (_C["NCN_MESH_TILE_X"], _C["NCN_MESH_TILE_Y"], _C["NCN_MESH_TILE_Z"])  # points per workgroup of ncn_mesh_count, (x, y, z)
SCAN_ELEMS = _C["NCN_MESH_SCAN_ELEMS"]  # elements per workgroup of ncn_mesh_scan
SCAN_SWEEP = _C["NCN_MESH_SCAN_SWEEP"]  # block sums per sweep of its second pass
DEFAULT_ISO = 10.0  # a level, not a property of the method: pass the one that suits the scene's densities

# (bitfield: uint8 CUDA tensor of grid_size**3 / 8 bytes, cascade 0 first; scale: the model's)
Occupancy = collections.namedtuple("Occupancy", "bitfield grid_size scale")


def model_occupancy(model):
    """The Occupancy of a model's density bitfield (its first cascade is what the lookup reads)."""
    return Occupancy(model.density_bitfield, int(model.grid_size), float(model.scale))


def _vec3(v, name):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    try:
        out = tuple(float(np.float32(x)) for x in np.asarray(v, dtype=np.float64).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be 3 numbers") from None
    if len(out) != 3 or not all(math.isfinite(x) for x in out):
        raise ValueError(f"{name} must be 3 finite numbers (got {v!r})")
    return out


def _box(lo, hi):
    lo, hi = _vec3(lo, "lo"), _vec3(hi, "hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"lo < hi is needed on every axis (got lo {lo}, hi {hi})")
    return lo, hi


def _res(res):
    r = (res,) * 3 if isinstance(res, (int, np.integer)) else tuple(res)
    if len(r) != 3 or not all(isinstance(n, (int, np.integer)) and n >= 1 for n in r):
        raise ValueError(f"res must be an int or (Nx, Ny, Nz), each >= 1 (got {res!r})")
    return tuple(int(n) for n in r)


def _iso(iso):
    iso = float(iso)
    if not math.isfinite(iso):
        raise ValueError(f"iso must be finite (got {iso})")
    return iso


def _occupancy(occupancy):
    """(bitfield, grid_size, scale) as the kernels take them; (None, 0, 0.0) when culling is off."""
    if occupancy is None:
        return None, 0, 0.0
    bitfield, G, scale = occupancy
    _lib.check_input(bitfield, "occupancy.bitfield")
    _lib.check_dtype(bitfield, torch.uint8, "occupancy.bitfield")
    G, scale = int(G), float(scale)
    if G < 2 or G > 1024 or G & (G - 1):
        raise ValueError(f"occupancy.grid_size must be a power of two in [2, 1024] (got {G})")
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError(f"occupancy.scale must be positive (got {scale})")
    if bitfield.numel() < G ** 3 // 8:
        raise ValueError(f"occupancy.bitfield must hold grid_size**3 / 8 = {G ** 3 // 8} bytes (got {bitfield.numel()})")
    return bitfield, G, scale


def _lattice(sigma):
    _lib.check_input(sigma, "sigma")
    _lib.check_dtype(sigma, torch.float32, "sigma")
    if sigma.dim() != 3 or min(sigma.shape) < 2:
        raise ValueError(f"sigma must be (Nz+1, Ny+1, Nx+1) with every N >= 1 (got {tuple(sigma.shape)})")
    nz, ny, nx = (int(s) - 1 for s in sigma.shape)
    return nx, ny, nz


def blocks(n):
    """Scan blocks of n elements: the length of vbase / fbase."""
    return (n + SCAN_ELEMS - 1) // SCAN_ELEMS


def count_and_scan(sigma, lo, hi, iso, occupancy=None):
    """First phase: ncn_mesh_count and the two scans.  Returns the workspace dict {mask, nfaces, vlocal,
    flocal, vbase, fbase, totals} (device tensors, sized as the header states; totals = [V, F] int64)."""
    lo, hi = _box(lo, hi)
    iso = _iso(iso)
    nx, ny, nz = _lattice(sigma)
    bitfield, G, scale = _occupancy(occupancy)
    dev = sigma.device
    P, C = (nx + 1) * (ny + 1) * (nz + 1), nx * ny * nz
    ws = {"mask": torch.empty(P, dtype=torch.uint8, device=dev), "nfaces": torch.empty(C, dtype=torch.uint8, device=dev),
          "vlocal": torch.empty(P, dtype=torch.int16, device=dev), "flocal": torch.empty(C, dtype=torch.int16, device=dev),
          "vbase": torch.empty(blocks(P), dtype=torch.int64, device=dev),
          "fbase": torch.empty(blocks(C), dtype=torch.int64, device=dev),
          "totals": torch.empty(2, dtype=torch.int64, device=dev)}
    call("ncn_mesh_count", sigma, nx, ny, nz, *lo, *hi, iso, bitfield, G, scale, ws["mask"], ws["nfaces"])
    call("ncn_mesh_scan", ws["mask"], P, 1, ws["vlocal"], ws["vbase"], ws["totals"][0:1])
    call("ncn_mesh_scan", ws["nfaces"], C, 0, ws["flocal"], ws["fbase"], ws["totals"][1:2])
    return ws


def emit(sigma, lo, hi, iso, ws, verts, faces, n_verts, n_faces):
    """Second phase: the vertices and faces into caller-sized buffers (n_verts, n_faces: the totals)."""
    nx, ny, nz = _lattice(sigma)
    lo, hi = _box(lo, hi)
    call("ncn_mesh_emit_verts", sigma, nx, ny, nz, *lo, *hi, _iso(iso), ws["mask"], ws["vlocal"], ws["vbase"], verts,
         n_verts)
    call("ncn_mesh_emit_faces", sigma, nx, ny, nz, _iso(iso), ws["mask"], ws["vlocal"], ws["vbase"], ws["nfaces"],
         ws["flocal"], ws["fbase"], faces, n_faces)


def extract_isosurface(sigma, lo, hi, iso, occupancy=None):
    """The indexed mesh of {sigma = iso}: sigma (Nz+1, Ny+1, Nx+1) float32 CUDA over the box [lo, hi]
    (3 floats each) -> (verts (V, 3) float32, faces (F, 3) int64) on the device.  Inside is
    sigma >= iso; every triangle's normal points toward lower density.  occupancy: None or an
    Occupancy (bitfield, grid_size, scale); with it the surface may have open borders (module docstring).
    One host read (V and F) between the two phases: this is an export, not the training step."""
    sigma = sigma if not isinstance(sigma, torch.Tensor) or sigma.is_contiguous() else sigma.contiguous()
    ws = count_and_scan(sigma, lo, hi, iso, occupancy)
    V, F = (int(v) for v in ws["totals"].tolist())
    verts = torch.empty(V, 3, dtype=torch.float32, device=sigma.device)
    faces = torch.empty(F, 3, dtype=torch.int64, device=sigma.device)
    emit(sigma, lo, hi, iso, ws, verts, faces, V, F)
    return verts, faces


def _model_box(model, lo, hi):
    if not hasattr(model, "density") or not hasattr(model, "xyz_min"):
        raise ValueError("model must be an NGPMT (density(), xyz_min, xyz_max)")
    return _box(model.xyz_min if lo is None else lo, model.xyz_max if hi is None else hi)


@torch.no_grad()
def density_lattice(model, res, lo=None, hi=None, chunk=2 ** 22, occupancy=False):
    """model.density at the lattice points of `res` cells over [lo, hi] (default: the model's box), as
    a (Nz+1, Ny+1, Nx+1) float32 lattice.  The points are generated chunk by chunk (ncn_mesh_points:
    the (P, 3) array of the whole lattice never exists).  occupancy=True: only the points with at least
    one active incident cell are evaluated, the others stay 0."""
    nx, ny, nz = _res(res)
    lo, hi = _model_box(model, lo, hi)
    chunk = int(chunk)
    if chunk < 1 or chunk >= 2 ** 31:
        raise ValueError(f"chunk must be in [1, 2^31) (got {chunk})")
    _lib.check_input(model.xyz_min, "model.xyz_min")
    bitfield, G, scale = _occupancy(model_occupancy(model) if occupancy else None)
    dev = model.xyz_min.device
    P = (nx + 1) * (ny + 1) * (nz + 1)
    lattice = torch.zeros(P, dtype=torch.float32, device=dev)
    n_max = min(chunk, P)
    xyz = torch.empty(n_max, 3, dtype=torch.float32, device=dev)
    idx = torch.empty(n_max, dtype=torch.int64, device=dev) if occupancy else None
    count = torch.zeros(1, dtype=torch.int32, device=dev) if occupancy else None
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        if occupancy:
            count.zero_()
        call("ncn_mesh_points", nx, ny, nz, *lo, *hi, p0, n, bitfield, G, scale, xyz, idx, count)
        if not occupancy:
            lattice[p0:p0 + n] = model.density(xyz[:n])
            continue
        m = int(count.item())
        if m:
            lattice[idx[:m]] = model.density(xyz[:m])
    return lattice.view(nz + 1, ny + 1, nx + 1)


def vertex_normals(model, verts, chunk=2 ** 22):
    """Unit normals -grad sigma / |grad sigma| at verts (V, 3), through NGPMT.density's gradient w.r.t. x,
    chunk by chunk.  Only the direction is wanted, so the backward is kept inside the fp16 range whatever
    the densities are: the upstream gradient of vertex i is 1 / sigma_i (grad log sigma has the direction
    of grad sigma) with sigma_i clamped to [exp(-15), exp(15)], the range in which TruncExp's backward
    follows sigma, so that upstream x d sigma / d h is at most 1 for every density, zero included; and an
    internal GradScaler's scale, sized for a training step's ~1e-5 upstream gradients, is 1 meanwhile.
    The parameters are frozen meanwhile too, so their gradient buffer is not touched.  Both are put back on
    the way out.  A vertex whose density is not finite, or whose gradient is zero or not finite, gets the
    zero vector: the result never holds a NaN or an Inf."""
    _lib.check_input(verts, "verts")
    params = [p for p in model.parameters() if p.requires_grad]
    amp_state = getattr(model, "amp_state", None)
    saved_amp = None if amp_state is None else amp_state.clone()
    out = torch.empty_like(verts)
    try:
        for p in params:
            p.requires_grad_(False)
        if amp_state is not None:
            amp_state[0] = 1.0
        for i in range(0, verts.shape[0], chunk):
            x = verts[i:i + chunk].detach().clone().requires_grad_(True)
            with torch.enable_grad():
                sigma = model.density(x)
                s = sigma.detach()
                upstream = torch.where(torch.isfinite(s), 1.0 / s.clamp(math.exp(-15.0), math.exp(15.0)), torch.zeros_like(s))
                g, = torch.autograd.grad(sigma, x, grad_outputs=upstream)
            # (the largest component first, so that the norm of a huge gradient does not overflow)
            g = g / g.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30)
            n = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-30)
            out[i:i + chunk] = torch.where(torch.isfinite(n).all(dim=-1, keepdim=True), n, torch.zeros_like(n))
    finally:
        for p in params:
            p.requires_grad_(True)
        if amp_state is not None:
            amp_state.copy_(saved_amp)
    return out


def extract_mesh(model, res=256, iso=DEFAULT_ISO, normals=False, occupancy=False, lo=None, hi=None, chunk=2 ** 22):
    """The isosurface of the model's density over its box (or [lo, hi]): density_lattice, then
    extract_isosurface.  -> (verts, faces), or (verts, faces, normals) with normals=True: unit vertex
    normals -grad sigma / |grad sigma|.  occupancy=True culls by the model's density bitfield (open
    borders where the surface leaves the occupied region: module docstring)."""
    res, iso = _res(res), _iso(iso)
    lo, hi = _model_box(model, lo, hi)
    sigma = density_lattice(model, res, lo, hi, chunk, occupancy)
    verts, faces = extract_isosurface(sigma, lo, hi, iso, model_occupancy(model) if occupancy else None)
    if not normals:
        return verts, faces
    return verts, faces, vertex_normals(model, verts, chunk)


def save_ply(path, verts, faces, normals=None):
    """Binary little-endian PLY: x y z (and nx ny nz) float32 per vertex, `list uchar int` per face.
    One host copy of each tensor."""
    if not isinstance(verts, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise ValueError("verts and faces must be tensors")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"verts must be (V, 3) and faces (F, 3) (got {tuple(verts.shape)}, {tuple(faces.shape)})")
    if normals is not None and (not isinstance(normals, torch.Tensor) or normals.shape != verts.shape):
        raise ValueError("normals must be a (V, 3) tensor like verts")
    V, F = verts.shape[0], faces.shape[0]
    if V >= 2 ** 31:
        raise ValueError(f"{V} vertices do not fit PLY's int indices")
    cols = [verts.detach().to(torch.float32).cpu().numpy()]
    names = ["x", "y", "z"]
    if normals is not None:
        cols.append(normals.detach().to(torch.float32).cpu().numpy())
        names += ["nx", "ny", "nz"]
    v = np.ascontiguousarray(np.concatenate(cols, axis=1).astype("<f4"))
    f = np.empty(F, dtype=[("n", "u1"), ("i", "<i4", (3,))])
    f["n"] = 3
    f["i"] = faces.detach().cpu().numpy()
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V}"]
    header += [f"property float {n}" for n in names]
    header += [f"element face {F}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())
