"""Cost of the direction gradient in the split backward's rgb part: the plain part 1 of
ncn_field_bwd_mlp_part and ncn_field_bwd_mlp_rgb_din on the same inputs, alternating.

  python tools/heads_input_grad_probe.py run       the marched samples of the 8192-ray synthetic batch
      in fp16; 3 warm-up and 20 timed pairs of launches.  Run it under
      `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run --` (the program after `--`).
  python tools/heads_input_grad_probe.py summary DIR/.../run_kernel_trace.csv
      the median, minimum and maximum kernel time of field_bwd_kernel<_Float16, 1, false> and
      <_Float16, 1, true> over the run's launches (the first 3 of each dropped), and their ratio."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT]
WARMUP, ITERS = 3, 20


def run():
    import torch
    from ncnerf_amd import _lib, vren
    from ncnerf_amd.ngp_mt import NGPMT, N_W, register_grid_buffers
    from ncnerf_amd.synthetic import SyntheticScene

    dev = torch.device("cuda:0")
    scene = SyntheticScene()
    torch.manual_seed(0)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, precision="fp16").to(dev))
    m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    batch = scene.torch_batch(8192, seed=1, device=dev)
    ro, rd = batch["rays_o"], batch["rays_d"]
    _, hits_t, _ = vren.ray_aabb_intersect(ro, rd, m.center, m.half_size, 1, near_distance=0.01)
    noise = torch.rand(8192, device=dev)
    _, xyzs, dirs, _, _, _ = vren.raymarching_train(ro, rd, hits_t[:, 0].contiguous(), m.density_bitfield, m.cascades,
                                                    m.scale, 0.0, noise, m.grid_size, 1024)
    n = xyzs.shape[0]
    print("marched S =", n, flush=True)
    L = _lib.lib()
    _, _, enc, packed, _ = m._field_fwd(xyzs, dirs, None, 0, True)
    gr = torch.randn(n, 3, device=dev) * 1e-5
    f = lambda k: torch.empty(int(k), dtype=torch.float32, device=dev)  # noqa: E731
    nb = int(L.ncn_field_bwd_part_blocks(n, 1))
    slab, dE, lmax, stash = f(nb * N_W), f(L.ncn_field_bwd_dE_floats(n)), f(16 * 256), f(L.ncn_field_bwd_stash_floats(n))
    dd = torch.empty(n, 3, device=dev)
    scale, w_master = m._bwd_loss_scale(), m.flat_params()[m._n_table:]
    for _ in range(WARMUP + ITERS):
        _lib.call("ncn_field_bwd_mlp_part", xyzs, dirs, n, None, None, packed, m._prec, enc, None, None, gr, scale, 1, 0,
                  slab, dE, lmax, stash)
        _lib.call("ncn_field_bwd_mlp_rgb_din", xyzs, dirs, n, None, None, packed, m._prec, enc, gr, scale, 0, slab, dE,
                  lmax, stash, w_master, dd)
    torch.cuda.synchronize()
    print("grid", nb, "dL_ddirs finite", bool(torch.isfinite(dd).all()), "norm", float(dd.norm()), flush=True)


def summary(path):
    times = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            if "field_bwd_kernel" in name:
                times.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    med = {}
    for name, t in sorted(times.items()):
        t = sorted(t[WARMUP:])
        med[name] = t[len(t) // 2]
        print(f"{name}: {len(t)} launches, median {med[name]:.2f} us, min {t[0]:.2f} us, max {t[-1]:.2f} us")
    plain = [v for k, v in med.items() if "1, false" in k or "Li1ELb0" in k]
    din = [v for k, v in med.items() if "1, true" in k or "Li1ELb1" in k]
    if len(plain) == 1 and len(din) == 1:
        print(f"rgb part with the direction gradient / plain rgb part: {din[0] / plain[0]:.3f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        summary(sys.argv[2])
