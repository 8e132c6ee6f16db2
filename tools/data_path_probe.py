"""What producing one training batch costs, beside the training step itself.

8192 rays as 128 patches of 8x8 from 100 images of 1024x768 (fp32 pixels), three ways:
  1. host     the reference's structure: numpy draws and a gather from the (pinned) host image stack
              (datasets/base.py:142-182), the host-to-device copies, then NeRFSystem.forward's ray
              code in torch ops (train_nerf.py:167-182: poses[img_idxs], directions[pix_idxs], get_rays);
  2. torch    the same with the image stack on the device and torch indexing (the draws stay numpy);
  3. kernels  ncnerf_amd.data.DeviceRayDataset.batch: eager (two launches) and as a captured graph
              (one replay), with fp32 and with uint8 pixels.
Each figure is the median over --iters single batches after --warmup, timed with device events
around everything the path does for one batch — for 1 and 2 that includes the host work, during
which the device idles — after a device synchronise; `wall_us` is the host clock around the same
work ending in a synchronise.  Needs a GPU; there is no fallback.

  python tools/data_path_probe.py --out profiles/data_path/data_path_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters, warmup):
    """Median / min / max of device-event and host-clock times of single calls, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        ev.append(e0.elapsed_time(e1) * 1e3)
    return {"event_us": {"median": statistics.median(ev), "min": min(ev), "max": max(ev)},
            "wall_us": {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--patch", type=int, default=8)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_path", "data_path_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_path_probe needs a GPU")
    from ncnerf_amd.data import DeviceRayDataset
    from ncnerf_amd.synthetic import make_cameras

    dev = torch.device("cuda:0")
    V, H, W, p, R = a.images, a.height, a.width, a.patch, a.rays
    n_p, area = R // (p * p), p * p
    torch.manual_seed(0)
    images_dev = torch.rand(V, H * W, 3, device=dev)
    images_u8 = (images_dev * 255).to(torch.uint8)
    images_host = torch.empty(V, H * W, 3, pin_memory=True)
    images_host.copy_(images_dev)
    poses = torch.from_numpy(make_cameras(V, seed=0)).to(dev)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5)
    d = np.stack([(u - W / 2) / W, (v - H / 2) / W, np.ones_like(u)], -1).reshape(-1, 3)
    directions = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    n_corners = (H - p + 1) * (W - p + 1)
    offsets = np.arange(H * W, dtype=np.int64).reshape(H, W)[:p, :p].reshape(-1)
    rng = np.random.default_rng(0)

    def draws():  # base.py:151-167
        img_idxs = np.repeat(rng.integers(0, V, n_p), area)
        pix_idxs = (rng.integers(0, n_corners, n_p)[:, None] + offsets[None]).reshape(-1)
        return img_idxs, pix_idxs

    def get_rays(img_idxs, pix_idxs):  # train_nerf.py:167-168, 182 (ray_utils.py:45-71)
        c2w = poses[img_idxs]
        rays_d = (directions[pix_idxs][:, None, :] @ c2w[..., :3].transpose(1, 2))[:, 0]
        return c2w[..., 3].expand_as(rays_d), rays_d

    def host_path():
        img_idxs, pix_idxs = draws()
        rgb = images_host[img_idxs, pix_idxs]  # base.py:176-177
        rgb = rgb.to(dev, non_blocking=True)
        ii = torch.from_numpy(img_idxs).to(dev, non_blocking=True)
        pp = torch.from_numpy(pix_idxs).to(dev, non_blocking=True)
        return get_rays(ii, pp) + (rgb,)

    def torch_path():
        img_idxs, pix_idxs = draws()
        ii = torch.from_numpy(img_idxs).to(dev, non_blocking=True)
        pp = torch.from_numpy(pix_idxs).to(dev, non_blocking=True)
        return get_rays(ii, pp) + (images_dev[ii, pp],)

    res = {"config": {"rays": R, "patch": p, "images": V, "width": W, "height": H, "iters": a.iters,
                      "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}}
    res["1_host_gather_h2d_torch_rays"] = timed(host_path, a.iters, a.warmup)
    res["2_device_images_torch_indexing"] = timed(torch_path, a.iters, a.warmup)
    step_dev = torch.zeros((), dtype=torch.int64, device=dev)
    for name, imgs in (("f32", images_dev), ("u8", images_u8)):
        ds = DeviceRayDataset(imgs, poses, directions, (W, H), batch_size=R, patch_size=p)
        out = ds.buffers()
        res[f"3_kernels_eager_{name}"] = timed(lambda: ds.batch(step_dev, out=out), a.iters, a.warmup)
        ds.batch(step_dev, out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ds.batch(step_dev, out=out)
        # the captured pair follows the device counter and writes what the eager call writes
        step_dev.fill_(7)
        g.replay()
        eager = ds.batch(7)
        assert all(torch.equal(out[k], eager[k]) for k in out), "captured batch != eager batch"
        step_dev.zero_()
        res[f"3_kernels_graph_{name}"] = timed(g.replay, a.iters, a.warmup)
        # back to back (no idle device between batches): device time per batch
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        res[f"3_kernels_graph_{name}"]["back_to_back_us"] = e0.elapsed_time(e1) * 1e3 / a.iters
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
