"""What the geometry terms of NeRFMTLoss cost per step.

8192 rays in 8x8 patches (6272 triangles) with depth and normal labels; depth -> normals -> the four
terms (depth L2, GT-normal L1 / dot, RegNeRF) -> backward to the depth, in two forms, alternated in one
process after a warm-up and timed with device events:
  1. node   extract_normals_from_ray_batch + ncnerf_amd.losses.geometry_losses (ncn_geom_loss_fwd /
            ncn_geom_loss_bwd, include/ncnerf_geom.h);
  2. torch  the expressions NeRFMTLoss used before: boolean-mask gathers (each reads the mask's count
            on the host), means, torch.where as the validity filter, autograd through them and
            through the normals node (ncn_normals_bwd).
Needs a GPU; there is no fallback.

  python tools/geom_loss_probe.py --out profiles/geom_loss/geom_loss_probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

W = (0.1, 0.05, 0.02)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=128, help="8x8 patches (128: 8192 rays, 6272 triangles)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geom_loss_probe needs a GPU")
    import geom_ref
    from ncnerf_amd.losses import (GEOM_DEPTH, GEOM_NORM_DOT, GEOM_NORM_L1, GEOM_REG, extract_normals_from_ray_batch,
                                   geometry_losses)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    o, d = geom_ref.patch_rays(rng, args.patches)
    true_depth, n = geom_ref.box_exit(o, d)
    R = len(true_depth)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    depth_gt = true_depth * (1 + 0.002 * rng.standard_normal(R))
    depth_gt[rng.random(R) < 0.2] = 0.0
    normals_gt = n + 0.1 * rng.standard_normal((R, 3))
    normals_gt[rng.random(R) < 0.25] = 0.0
    rays_o, rays_d, depth_gt, normals_gt = t(o), t(d), t(depth_gt), t(normals_gt)
    depth = t(true_depth * (1 + 0.01 * rng.standard_normal(R))).requires_grad_(True)
    x = {k: v.to(dev) for k, v in geom_ref.triangles(R, "all_images_triang_patch").items()}
    terms = GEOM_DEPTH | GEOM_NORM_L1 | GEOM_NORM_DOT | GEOM_REG
    one = torch.ones((), device=dev)
    valid_filter = lambda v: torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    cos = torch.nn.CosineSimilarity(dim=-1)

    def node():
        nd = extract_normals_from_ray_batch(rays_o, rays_d, depth, x)
        vals, _, _ = geometry_losses(depth, x, depth_gt, nd, normals_gt, terms, W, step=1, reg_start=0,
                                     rays=(rays_o, rays_d))
        total = vals[0] + vals[1] + vals[2] + vals[3]
        return total, torch.autograd.grad(total, depth, one)[0]

    def plain():
        nd = extract_normals_from_ray_batch(rays_o, rays_d, depth, x)
        valid = depth_gt > 0
        l_depth = valid_filter(W[0] * ((depth[valid] - depth_gt[valid]) ** 2).mean())
        tgt = normals_gt[x["x1"]]
        valid = tgt.abs().sum(-1) > 0
        l_l1 = valid_filter(W[1] * (nd[valid] - tgt[valid]).abs().sum(-1).mean())
        l_dot = valid_filter(W[2] * (1.0 - cos(nd[valid], tgt[valid])).mean())
        l_reg = valid_filter(((depth[x["x1"]] - depth[x["x2"]]) ** 2 + (depth[x["x1"]] - depth[x["x3"]]) ** 2).mean())
        total = l_depth + l_l1 + l_dot + l_reg
        return total, torch.autograd.grad(total, depth, one)[0]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters  # us per forward + backward

    for fn in (node, plain):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    a, b = node(), plain()
    agree = dict(loss_rel=abs(float(a[0].detach()) - float(b[0].detach())) / abs(float(b[0].detach())),
                 grad_rel_l2=float((a[1] - b[1]).norm() / b[1].norm()))
    runs = {"node": [], "torch": []}
    for _ in range(args.repeats):  # alternating
        runs["node"].append(timed(node))
        runs["torch"].append(timed(plain))
    res = dict(n_rays=R, n_tri=int(x["x1"].numel()), iters=args.iters, repeats=args.repeats, unit="us per forward + backward",
               node_us=runs["node"], torch_us=runs["torch"], node_median_us=statistics.median(runs["node"]),
               torch_median_us=statistics.median(runs["torch"]), agreement=agree)
    res["torch_over_node"] = res["torch_median_us"] / res["node_median_us"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
