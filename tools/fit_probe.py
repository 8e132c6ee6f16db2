"""What the batch draw and the device log cost inside the captured step.

ms/step of Trainer.fit on a DeviceRayDataset of the bench's image size (100 views of 1024x768,
uint8, random pixels) against Trainer(use_graph=True).step() on one fixed batch: 8192 rays,
defer_optimizer, no grid refresh, two trainers in one process, alternating windows of 30 steps
(five each) after a warm-up, host clock around each window ending in a synchronise; a fit window
includes its one drain of the log ring.  Then the eager two-launch draw alone, for scale.  One JSON
line per window and a summary.  Needs a GPU; there is no fallback.

  python tools/fit_probe.py --out profiles/fit/fit_vs_step.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ncnerf_amd.data import DeviceRayDataset  # noqa: E402
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers  # noqa: E402
from ncnerf_amd.synthetic import IMG_H, IMG_W, SyntheticScene  # noqa: E402
from ncnerf_amd.trainer import Trainer  # noqa: E402

RAYS, WINDOW, N_WIN, WARM = 8192, 30, 5, 12
ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="file for the JSON lines")
args = ap.parse_args()
assert torch.cuda.is_available(), "fit_probe needs a GPU"
dev = torch.device("cuda:0")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


scene = SyntheticScene()
n_views = len(scene.poses)
g = torch.Generator(device=dev).manual_seed(0)
images = torch.randint(0, 256, (n_views, IMG_H * IMG_W, 3), device=dev, dtype=torch.uint8, generator=g)
ds = DeviceRayDataset(images, torch.from_numpy(scene.poses).to(dev), torch.from_numpy(scene.dirs).to(dev),
                      (IMG_W, IMG_H), batch_size=RAYS, seed=3, corner_mode="grid")
emit(what="setup", views=n_views, img_wh=[IMG_W, IMG_H], rays=RAYS, window=WINDOW, windows=N_WIN, warmup=WARM,
     images_mib=round(images.numel() / 2 ** 20, 1))


def trainer():
    torch.manual_seed(7)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    tr = Trainer(m, update_grid=False, use_graph=True, defer_optimizer=True)
    tr._rng_seed = 99
    tr.status_interval = 10 ** 9 + 7
    return tr


fixed = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in ds.batch(7).items()}
t_step, t_fit = trainer(), trainer()
nxt = {"step": 1000, "fit": 1000}


def run_step(n):
    for s in range(nxt["step"], nxt["step"] + n):
        t_step.step(fixed, s)
    nxt["step"] += n
    torch.cuda.synchronize()


def run_fit(n):
    log = t_fit.fit(ds, n, start_step=nxt["fit"], log_capacity=WINDOW)  # (ends with the drain: a device-to-host copy)
    nxt["fit"] += n
    torch.cuda.synchronize()
    return log


run_step(WARM)
run_fit(WARM)
ms = {"step": [], "fit": []}
for w in range(N_WIN):
    for name in ("step", "fit"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = run_step(WINDOW) if name == "step" else run_fit(WINDOW)
        dt = 1e3 * (time.perf_counter() - t0) / WINDOW
        ms[name].append(dt)
        extra = {} if log is None else {"rm_s": round(float(log["rm_s"].mean()), 2), "vr_s": round(float(log["vr_s"].mean()), 2),
                                        "psnr_last": round(float(log["psnr"][-1]), 3)}
        emit(what="window", order=2 * w + (name == "fit"), path=name, ms_per_step=round(dt, 4), **extra)
# the draw alone, eager, for scale: the launches that became nodes of the graph
bufs = ds.buffers()
step_dev = torch.zeros((), dtype=torch.int64, device=dev)
for _ in range(20):
    ds.batch(step_dev, out=bufs)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    ds.batch(step_dev, out=bufs)
torch.cuda.synchronize()
emit(what="eager_draw", us_per_batch=round(1e6 * (time.perf_counter() - t0) / 200, 2))
emit(what="summary", step_ms_median=round(float(np.median(ms["step"])), 4), fit_ms_median=round(float(np.median(ms["fit"])), 4),
     step_ms=[round(x, 4) for x in ms["step"]], fit_ms=[round(x, 4) for x in ms["fit"]],
     rays_per_s_step=round(RAYS / np.median(ms["step"]) * 1e3), rays_per_s_fit=round(RAYS / np.median(ms["fit"]) * 1e3))
