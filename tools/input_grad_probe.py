"""Measurements of the field's input gradients at the bench batch.

  python tools/input_grad_probe.py kernels   the field forward + backward on the marched samples of
      the 8192-ray synthetic batch, 23 times without and 23 times with input gradients; run it under
      `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run --` and read
      field_bwd_dx_kernel beside field_fwd_kernel, and field_bwd_kernel<.., 3, false> beside
      <.., 3, true> (the direction output) in DIR/run_kernel_stats.csv.
  python tools/input_grad_probe.py eager     the eager Trainer.step at 8192 rays without and with rays
      that require grad (pose refinement), median of 20 steps, two alternations."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT]
import torch
from ncnerf_amd import vren
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import Trainer

mode = sys.argv[1]
dev = torch.device("cuda:0")
scene = SyntheticScene()
torch.manual_seed(0)
m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
batch = scene.torch_batch(8192, seed=1, device=dev)
ITERS = 20

if mode == "kernels":
    ro, rd = batch["rays_o"], batch["rays_d"]
    _, hits_t, _ = vren.ray_aabb_intersect(ro, rd, m.center, m.half_size, 1, near_distance=0.01)
    noise = torch.rand(8192, device=dev)
    rays_a, xyzs, dirs, deltas, ts, counter = vren.raymarching_train(ro, rd, hits_t[:, 0].contiguous(), m.density_bitfield,
                                                                    m.cascades, m.scale, 0.0, noise, m.grid_size, 1024)
    S = xyzs.shape[0]
    print("marched S =", S, flush=True)
    gs = torch.randn(S, device=dev) * 1e-5
    gr = torch.randn(S, 3, device=dev) * 1e-5
    for grads in (False, True):
        for it in range(ITERS + 3):
            x, d = xyzs.clone().requires_grad_(grads), dirs.clone().requires_grad_(grads)
            out = m(x, d)
            torch.autograd.backward([out["sigmas"], out["rgbs"]], [gs, gr])
        torch.cuda.synchronize()
    print("done", flush=True)
else:
    tr = Trainer(m, use_graph=False)
    for grads in (False, True, False, True):
        b = dict(batch)
        if grads:
            b["rays_o"] = batch["rays_o"].clone().requires_grad_(True)
            b["rays_d"] = batch["rays_d"].clone().requires_grad_(True)
        times = []
        for it in range(ITERS + 5):
            if grads:
                b["rays_o"].grad = b["rays_d"].grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(b, 3000)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t = sorted(times[5:])
        extra = ""
        if grads:
            g = b["rays_d"].grad
            extra = f" rays_d.grad finite {bool(torch.isfinite(g).all())} norm {float(g.norm()):.3e} amp {float(m.amp_state[0])}"
        print(f"eager step 8192 rays, ray grads {grads}: median {1e3 * t[len(t) // 2]:.3f} ms min {1e3 * t[0]:.3f} ms "
              f"max {1e3 * t[-1]:.3f} ms ({len(t)} steps){extra}", flush=True)
