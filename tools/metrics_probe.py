"""What the metric stage of one validation view costs.

One 1024x768 view (rgb, depth, normals; synthetic images, the cost does not depend on the values),
two forms, alternated in one process after a warm-up and timed with device events:
  1. kernels  ncnerf_amd.metrics.ViewMetrics.update: pointwise errors, the SSIM pass, angles, the
              exact medians, the row (include/ncnerf_metrics.h); also each entry point on its own;
  2. torch    the float32 torch restatement in the reference's structure, ON THE DEVICE
              (tests/metrics_ref.py: dense grouped conv for the three SSIMs, torch.median for the
              medians, masked means for depth).  This flatters the reference, which copies every
              image to the host and runs scikit-image's SSIM there in float64.
The SSIM launch's share of the HBM peak is the bytes it has to move (both images once, the partial
sums) over its time, against 8 TB/s.  Needs a GPU; there is no fallback.

  python tools/metrics_probe.py --out profiles/view_metrics/metrics_probe.json
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

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_probe needs a GPU")
    import metrics_ref as M
    from ncnerf_amd import metrics as NM
    from ncnerf_amd._lib import call
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    n = H * W
    torch.manual_seed(0)
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                          torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(x / 37.0) * torch.cos(y / 23.0)
    rgb_t = torch.stack([base, 0.8 * base + 0.1, 0.6 * base + 0.2], -1).reshape(n, 3).contiguous()
    rgb_p = (rgb_t + 0.03 * torch.randn(n, 3, device=dev)).contiguous()
    dep_t = (2.0 + base.reshape(n)).contiguous()
    dep_t[::17] = 0.0
    dep_p = (dep_t + 0.05 * torch.randn(n, device=dev)).contiguous()
    nrm_t = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1).contiguous()
    nrm_t[::5] = 0.0
    nrm_p = torch.nn.functional.normalize(nrm_t + 0.2 * torch.randn(n, 3, device=dev), dim=-1).contiguous()
    preds = {"rgb": rgb_p, "depth": dep_p, "norm_depth": nrm_p}
    target = {"rgb": rgb_t, "depth": dep_t, "normals": nrm_t}

    vm = NM.ViewMetrics(eval_depth=True, norm_gt=True)
    s = NM._Scratch(H, W, dev)
    row = torch.empty(12, device=dev)

    def kernels():
        vm.reset()
        return vm.update(preds, target, H, W)

    def torch_form():
        mse = ((rgb_p - rgb_t) ** 2).mean()
        out = [-10.0 * torch.log10(mse)] + [m for _, m in M.ssims_torch32(rgb_p, rgb_t, H, W)]
        out += list(M.depth_torch32(dep_p, dep_t)) + list(M.normals_torch32(nrm_p, nrm_t))
        return torch.stack([o.float() for o in out])

    stages = {
        "pointwise": lambda: call("ncn_metrics_pointwise", rgb_p, rgb_t, dep_p, dep_t, n, s.pw_ws, s.pw_ws.numel(),
                                  s.pw_sums, s.depth_count, s.range),
        "ssim": lambda: call("ncn_metrics_ssim", rgb_p, rgb_t, H, W, s.range, s.ssim_ws, s.ssim_ws.numel(), None, s.ssim),
        "angles": lambda: call("ncn_metrics_angles", nrm_p, nrm_t, n, s.angles, s.ang_ws, s.ang_ws.numel(), s.ang_sums,
                               s.ang_counts),
        "select_median": lambda: call("ncn_select_median", s.angles, n, 2, s.ang_counts, s.sel_ws, s.sel_ws.numel(),
                                      s.medians),
        "finalise": lambda: call("ncn_metrics_finalise", s.pw_sums, s.depth_count, 3 * n, s.ssim, s.ang_sums,
                                 s.ang_counts, s.medians, row),
        "torch_ssims": lambda: M.ssims_torch32(rgb_p, rgb_t, H, W),
        "torch_medians": lambda: M.normals_torch32(nrm_p, nrm_t),
    }
    forms = {"kernels": kernels, "torch": torch_form, **stages}
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.iters):  # alternating: every form once per round
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(200000)  # the device is busy while the host issues the launches
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    got, want = kernels().tolist(), torch_form().tolist()
    ssim_bytes = 2 * n * 3 * 4 + 3 * 8 * (-(-W // 64)) * (-(-H // 8)) + 8 + 12
    res = {"width": W, "height": H, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "event_us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "ssim_launch": {"bytes_to_move": ssim_bytes, "box_window": "rides in the same launch (same tile, same loads)",
                           "share_of_hbm_peak": ssim_bytes / (statistics.median(times["ssim"]) * 1e-6) / HBM_PEAK},
           "speedup_median": statistics.median(times["torch"]) / statistics.median(times["kernels"]),
           "row_kernels": got, "row_torch": want[:4] + want[4:6] + [1.0] + [want[6], want[7], want[8], want[9], 1.0]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
