"""What one checkpoint costs at the bench model's size.

The bench's model (NGPMT(scale=0.5, grid_size=128): 11.5 M flat parameters, a 128^3 occupancy grid)
under Trainer(use_graph=True, defer_optimizer=True) after a few steps on 8192 rays, so a deferred
step is pending when the snapshot is taken.  Timed, host clock around work that ends in a device
synchronise: Trainer.state_dict() (the flush and the device clones), checkpoint.save of that
snapshot (the copies to the host, torch.save, the rename), Trainer.save_checkpoint (both), and
Trainer.load_checkpoint into a second trainer.  The file goes to --dir (default: the system's
temporary directory) and is removed.  One JSON line per repetition and a summary.  Needs a GPU;
there is no fallback.

  python tools/checkpoint_probe.py --out profiles/checkpoint/checkpoint_cost.txt
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ncnerf_amd import checkpoint  # noqa: E402
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers  # noqa: E402
from ncnerf_amd.synthetic import SyntheticScene  # noqa: E402
from ncnerf_amd.trainer import Trainer  # noqa: E402

RAYS, WARM, REPS = 8192, 12, 5
ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="file for the JSON lines")
ap.add_argument("--dir", default=None, help="directory for the checkpoint file (default: a temporary one)")
args = ap.parse_args()
assert torch.cuda.is_available(), "checkpoint_probe needs a GPU"
dev = torch.device("cuda:0")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


scene = SyntheticScene()


def trainer(seed):
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    tr = Trainer(m, update_grid=True, use_graph=True, defer_optimizer=True)
    tr.status_interval = 10 ** 9 + 7
    return tr


tr, other = trainer(7), trainer(8)
step = 0
batch = scene.torch_batch(RAYS, seed=1, device=dev)


def train(n):
    global step
    for _ in range(n):
        tr.step(batch, step)
        step += 1


train(WARM)
tmp = tempfile.mkdtemp(dir=args.dir)
path = os.path.join(tmp, "probe.pt")
ms = {"state_dict": [], "save": [], "save_checkpoint": [], "load_checkpoint": []}
try:
    for r in range(REPS + 1):  # (the first repetition warms the allocator and the page cache: not counted)
        train(3)
        assert tr._pending
        t_sd, sd = clock(tr.state_dict)
        t_save, _ = clock(lambda: checkpoint.save(sd, path))
        n_bytes = os.path.getsize(path)
        del sd
        train(3)
        t_both, _ = clock(lambda: tr.save_checkpoint(path))
        t_load, nxt = clock(lambda: other.load_checkpoint(path))
        assert nxt == step and torch.equal(other.model.flat_params(), tr.model.flat_params())
        emit(what="repetition", counted=r > 0, state_dict_ms=round(t_sd, 2), save_ms=round(t_save, 2),
             save_checkpoint_ms=round(t_both, 2), load_checkpoint_ms=round(t_load, 2), file_mib=round(n_bytes / 2 ** 20, 1))
        if r > 0:
            for k, v in zip(ms, (t_sd, t_save, t_both, t_load)):
                ms[k].append(v)
finally:
    if os.path.exists(path):
        os.remove(path)
    os.rmdir(tmp)
emit(what="summary", file_mib=round(n_bytes / 2 ** 20, 1), repetitions=REPS,
     **{k + "_ms_median": round(float(np.median(v)), 2) for k, v in ms.items()},
     **{k + "_ms": [round(x, 2) for x in v] for k, v in ms.items()})
