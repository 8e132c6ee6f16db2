"""What the isosurface extraction costs, stage by stage.

Per resolution (256^3 and 512^3 cells over the model's box) and with occupancy culling off and on:
  points + density   ncn_mesh_points + NGPMT.density over the whole lattice, chunk by chunk
                     (mesh.density_lattice), on a freshly initialised NGPMT with the synthetic room's
                     bitfield: the densities are not a trained scene's, their cost per point is;
  count              ncn_mesh_count, with its achieved bytes/s against the compulsory traffic (one read
                     of the lattice, one write of the masks and the face counts) and the share of the
                     HBM peak that is;
  scan               both ncn_mesh_scan calls (four launches);
  emit               ncn_mesh_emit_verts + ncn_mesh_emit_faces.
count / scan / emit run on a lattice that has a surface of a scene's size: the synthetic room's
occupancy sampled at the lattice points (20 inside an occupied voxel, 0 outside) at iso 10.  Device
events around `iters` back-to-back calls after a warm-up.  Last, the only other implementation there
is: tests/mesh_ref.py on the host against mesh.extract_isosurface on the same 64^3 lattice (host clock,
the device call ending in a synchronise).  Needs a GPU; there is no fallback.

  python tools/mesh_probe.py --out profiles/mesh/mesh_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, the MI355X's specification
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
ISO = 10.0


def room_lattice(occ, res, dev):
    """The room's occupancy [x][y][z] sampled at the lattice points: (res+1)^3 float32, 20 or 0."""
    G = occ.shape[0]
    i = torch.clamp((torch.arange(res + 1, device=dev) * G) // res, max=G - 1)
    o = torch.from_numpy(occ).to(dev)
    return (o[i[None, None, :], i[None, :, None], i[:, None, None]].float() * 20.0).contiguous()


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_probe needs a GPU")
    import mesh_ref
    from ncnerf_amd import _lib, mesh
    from ncnerf_amd.ngp_mt import NGPMT
    from ncnerf_amd.synthetic import SyntheticScene
    dev = torch.device("cuda:0")
    scene = SyntheticScene()
    torch.manual_seed(0)
    model = NGPMT(scale=0.5, grid_size=128).to(dev)
    model.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    occupancy = mesh.model_occupancy(model)
    med = statistics.median
    rows = []
    for res in args.res:
        sigma = room_lattice(scene.occ, res, dev)
        P, C = (res + 1) ** 3, res ** 3
        for occ_on in (False, True):
            occ = occupancy if occ_on else None
            row = dict(res=res, occupancy=occ_on, points=P, cells=C)
            # points + density (once to warm, then `repeats` timed whole-lattice passes)
            mesh.density_lattice(model, res, occupancy=occ_on)
            torch.cuda.synchronize()
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                mesh.density_lattice(model, res, occupancy=occ_on)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            row["points_density_ms"] = med(t)
            if occ_on:
                pts = mesh_points_listed(mesh, _lib, model, res, dev)
                row["points_evaluated"] = pts
            ws = mesh.count_and_scan(sigma, *BOX, ISO, occ)
            V, F = ws["totals"].tolist()
            row["verts"], row["faces"] = V, F
            bitfield, G, scale = mesh._occupancy(occ)
            count = lambda: _lib.call("ncn_mesh_count", sigma, res, res, res, *BOX[0], *BOX[1], ISO, bitfield, G, scale,
                                      ws["mask"], ws["nfaces"])

            def scan():
                _lib.call("ncn_mesh_scan", ws["mask"], P, 1, ws["vlocal"], ws["vbase"], ws["totals"][0:1])
                _lib.call("ncn_mesh_scan", ws["nfaces"], C, 0, ws["flocal"], ws["fbase"], ws["totals"][1:2])

            verts = torch.empty(V, 3, device=dev)
            faces = torch.empty(F, 3, dtype=torch.int64, device=dev)
            emit = lambda: mesh.emit(sigma, *BOX, ISO, ws, verts, faces, V, F)
            for name, fn in (("count", count), ("scan", scan), ("emit", emit)):
                row[name + "_ms"] = med([events(fn, args.iters, args.warmup) for _ in range(args.repeats)])
            row["count_bytes"] = 4 * P + P + C
            row["count_bytes_per_s"] = row["count_bytes"] / (row["count_ms"] * 1e-3)
            row["count_share_of_hbm_peak"] = row["count_bytes_per_s"] / HBM_PEAK
            row["scan_bytes"] = (1 + 2) * (P + C)
            row["scan_bytes_per_s"] = row["scan_bytes"] / (row["scan_ms"] * 1e-3)
            t = []
            for _ in range(5):  # host clock, with its allocations and the host read; the median of five calls
                t0 = time.perf_counter()
                mesh.extract_isosurface(sigma, *BOX, ISO, occ)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            row["extract_isosurface_wall_ms"] = med(t)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del ws, verts, faces
        del sigma
        torch.cuda.empty_cache()
    # the host restatement at 64^3
    sigma = room_lattice(scene.occ, 64, dev)
    host = sigma.cpu().numpy()
    t0 = time.perf_counter()
    rv, rf = mesh_ref.extract(host, *BOX, ISO)
    host_ms = (time.perf_counter() - t0) * 1e3
    mesh.extract_isosurface(sigma, *BOX, ISO)
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        v, f = mesh.extract_isosurface(sigma, *BOX, ISO)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.cpu().numpy(), rf))
    res = dict(unit="ms", hbm_peak_bytes_per_s=HBM_PEAK, iters=args.iters, repeats=args.repeats, stages=rows,
               host_64=dict(verts=len(rv), faces=len(rf), mesh_ref_ms=host_ms, device_ms=med(t), same_mesh=same))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def mesh_points_listed(mesh, _lib, model, res, dev):
    """How many lattice points occupancy culling hands to the density pass."""
    P = (res + 1) ** 3
    occ = mesh.model_occupancy(model)
    chunk, total = 2 ** 22, 0
    xyz = torch.empty(chunk, 3, device=dev)
    idx = torch.empty(chunk, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    for p0 in range(0, P, chunk):
        count.zero_()
        _lib.call("ncn_mesh_points", res, res, res, *BOX[0], *BOX[1], p0, min(chunk, P - p0), occ.bitfield, occ.grid_size,
                  occ.scale, xyz, idx, count)
        total += int(count.item())
    return total


if __name__ == "__main__":
    main()
