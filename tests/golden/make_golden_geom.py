"""Generate tests/golden/geom_losses.npz from the REFERENCE's own NeRFMTLoss.forward (losses.py:244-587).

Runs only where the reference checkout is readable (make_golden.py's container); nothing under tests/
reads the reference at test time.  The reference's native dependencies are stubbed exactly as
make_golden.py stubs them (none of them is on the path the geometry terms take: these are plain torch).

Per sampling strategy one set of inputs; per case the hyper-parameters, the step, every entry of the
returned loss_d and d total / d depth from autograd — in float32, and again with every floating
input cast to float64 (the reference of the tests' bounds).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geom.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as G  # noqa: E402  (the stubs, the path set-up)
from geom_ref import box_exit, patch_offsets, patch_rays  # noqa: E402  (tests/geom_ref.py: the well-conditioned rays)

BASE = dict(G.HPARAMS, loss_opacity_w=0, loss_norm_D_C_ort_dot_w=0, loss_norm_D_C_centr_dot_w=0,
            loss_norm_D_C_centr_L1_w=0, load_norm_gt=True, load_norm_depth_gt=True)
W_DEPTH, W_L1, W_DOT, START = 0.1, 0.05, 0.02, 500
ALL = dict(loss_depth_w=W_DEPTH, loss_norm_depth_L1_w=W_L1, loss_norm_depth_dot_w=W_DOT, loss_reg_depth_w=1.0)
# name -> (hyper-parameter overrides, global_step, input variant)
CASES = {
    "depth": (dict(loss_depth_w=W_DEPTH), 3000, "plain"),
    "norm": (dict(loss_norm_depth_L1_w=W_L1, loss_norm_depth_dot_w=W_DOT), 3000, "plain"),
    "norm_gtdepth": (dict(loss_norm_depth_L1_w=W_L1, loss_norm_depth_dot_w=W_DOT, loss_norm_GT_depth=True), 3000,
                     "plain"),
    "reg_off": (dict(loss_reg_depth_w=1.0), START, "plain"),  # step <= start: the entry is absent
    "reg_on": (dict(loss_reg_depth_w=1.0), START + 1, "plain"),
    "all": (ALL, 3000, "plain"),
    "empty": (ALL, START, "empty"),  # no depth_gt > 0, no non-zero GT normal, RegNeRF not started
    "nan": (ALL, 3000, "nan"),  # one NaN in the predicted depth (nan_ray): every term is filtered
}


def make_inputs(strategy, seed):
    """Four 8x8 patches of rays (R = 256, 196 triangles); for `all_images_triang` 64 triangles of three
    consecutive rays each (R = 192), taken from the patches' own triangles."""
    rng = np.random.default_rng(seed)
    o, d = patch_rays(rng, 4)
    off = patch_offsets(8)
    if strategy == "all_images_triang":
        pick = np.array([[64 * (j // 16) + off[c][3 * (j % 16)] for c in range(3)] for j in range(64)]).reshape(-1)
        o, d = o[pick], d[pick]
    R = o.shape[0]
    true_depth, n = box_exit(o, d)
    depth = true_depth * (1 + 0.01 * rng.standard_normal(R)).astype(np.float32)
    depth_gt = true_depth * (1 + 0.002 * rng.standard_normal(R)).astype(np.float32)
    depth_gt[rng.random(R) < 0.2] = 0.0
    normals = (n + 0.05 * rng.standard_normal((R, 3))).astype(np.float32)  # (not unit: the cosine's norms matter)
    normals_depth = (n + 0.2 * rng.standard_normal((R, 3))).astype(np.float32)
    normals[rng.random(R) < 0.25] = 0.0
    normals_depth[rng.random(R) < 0.25] = 0.0
    out = dict(rays_o=o, rays_d=d, depth=depth.astype(np.float32), rgb_pred=rng.random((R, 3), dtype=np.float32),
               rgb_gt=rng.random((R, 3), dtype=np.float32), depth_gt=depth_gt.astype(np.float32), normals_gt=normals,
               normals_depth_gt=normals_depth)
    if strategy == "all_images_triang_patch":
        out.update(patch_area=np.array(64), x1_offsets_local=off[0], x2_offsets_local=off[1], x3_offsets_local=off[2])
    return out


def nan_ray(strategy, inp):
    """The ray that carries the NaN: the first x1 corner, past the middle of the batch, whose labels are
    all valid, so that the NaN enters every term (a NaN behind a masked label would leave the normal
    terms finite and, in the reference too, put 0 * NaN into the gradient)."""
    R = len(inp["depth"])
    if strategy == "all_images_triang":
        x1 = np.arange(0, R, 3)
    else:
        x1 = (np.arange(0, R, 64)[:, None] + inp["x1_offsets_local"][None]).reshape(-1)
    ok = (inp["depth_gt"] > 0) & (np.abs(inp["normals_gt"]).sum(-1) > 0) & (np.abs(inp["normals_depth_gt"]).sum(-1) > 0)
    return int([r for r in x1 if r > R // 2 and ok[r]][0])


def run_case(losses, strategy, inp, over, step, variant, dtype):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    depth = inp["depth"].copy()
    depth_gt, normals, normals_depth = inp["depth_gt"], inp["normals_gt"], inp["normals_depth_gt"]
    if variant == "empty":
        depth_gt, normals, normals_depth = (np.zeros_like(a) for a in (depth_gt, normals, normals_depth))
    if variant == "nan":
        depth[nan_ray(strategy, inp)] = np.nan
    depth_t = t(depth).requires_grad_(True)
    rays_o, rays_d = t(inp["rays_o"]), t(inp["rays_d"])
    pred = dict(rgb=t(inp["rgb_pred"]).requires_grad_(True), depth=depth_t,
                opacity=torch.zeros(len(depth), dtype=dtype), rays_o=rays_o, rays_d=rays_d, deltas=torch.zeros(1), ts=torch.zeros(1), rays_a=torch.zeros(1, 3, dtype=torch.long),
                ws=torch.zeros(1))
    target = dict(rgb=t(inp["rgb_gt"]), depth=t(depth_gt), normals=t(normals), normals_depth=t(normals_depth))
    if strategy == "all_images_triang_patch":
        target.update(patch_area=int(inp["patch_area"]), x1_offsets_local=inp["x1_offsets_local"],
                      x2_offsets_local=inp["x2_offsets_local"], x3_offsets_local=inp["x3_offsets_local"])
    mod = losses.NeRFMTLoss(dict(BASE, ray_sampling_strategy=strategy, loss_norm_can_start=START, **over))
    ld = mod(pred, target, global_step=step)
    ld["total"].backward()
    grad = np.zeros(len(depth), np.float64) if depth_t.grad is None else depth_t.grad.double().numpy()
    return {k: float(v.detach()) for k, v in ld.items()}, grad


def main():
    G.install_stubs()
    import importlib
    losses = importlib.import_module("losses")
    out = {}
    for si, strategy in enumerate(("all_images_triang", "all_images_triang_patch")):
        tag = "tri" if strategy == "all_images_triang" else "patch"
        inp = make_inputs(strategy, seed=31 + si)
        for k, v in inp.items():
            out[f"{tag}/{k}"] = v
        out[f"{tag}/nan_ray"] = np.array(nan_ray(strategy, inp))
        for name, (over, step, variant) in CASES.items():
            ld32, g32 = run_case(losses, strategy, inp, over, step, variant, torch.float32)
            ld64, g64 = run_case(losses, strategy, inp, over, step, variant, torch.float64)
            assert sorted(ld32) == sorted(ld64), (ld32, ld64)
            pre = f"{tag}/{name}/"
            out[pre + "step"] = np.array(step)
            out[pre + "variant"] = np.array(variant)
            for k in ("loss_depth_w", "loss_norm_depth_L1_w", "loss_norm_depth_dot_w", "loss_reg_depth_w"):
                out[pre + k] = np.array(float(over.get(k, 0)))
            out[pre + "loss_norm_GT_depth"] = np.array(bool(over.get("loss_norm_GT_depth", False)))
            out[pre + "loss_norm_can_start"] = np.array(START)
            out[pre + "keys"] = np.array(sorted(ld32))
            for k in ld32:
                out[pre + "loss_" + k] = np.array(ld32[k], np.float32)
                out[pre + "loss64_" + k] = np.array(ld64[k], np.float64)
            out[pre + "grad_depth"] = g32.astype(np.float32)
            out[pre + "grad_depth64"] = g64
            print(tag, name, {k: round(v, 7) for k, v in ld64.items()}, "|grad|", float(np.abs(g64).sum()))
    np.savez_compressed(os.path.join(HERE, "geom_losses.npz"), **out)


if __name__ == "__main__":
    main()
