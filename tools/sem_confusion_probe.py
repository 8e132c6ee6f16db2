"""What counting one validation view into the semantic confusion matrix costs.

One 1024x768 view with K = 40 classes, the logits a channel slice of a (n, 3 + 3 + K) render buffer
(row stride 46: the test renderer's layout with both heads), raw labels with 0 = void.  Two forms,
alternated in one process after a warm-up and timed with device events:
  1. kernel  ncn_sem_confusion: one streaming launch, nothing on the host;
  2. torch   the reference's structure (metrics/semantic_metrics.py:23-40) in torch ops ON THE DEVICE:
             the all-void test, argmax on the strided slice, the mask, its host check (`True in
             valid_idx`), the two indexings, bincount(t * K + p) and the add into the state.
The two results are compared (they are integers: equal).  The kernel's bytes/s is what it has to move —
n x (46 x 4 + 8) bytes, the 64-byte-aligned rows whole and the int64 labels — over its time, against
8 TB/s.  Needs a GPU; there is no fallback.

  python tools/sem_confusion_probe.py --out profiles/round13/sem_confusion_probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "normal-clustering-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--lead", type=int, default=6, help="channels of the render buffer in front of the logits")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sem_confusion_probe needs a GPU")
    from ncnerf_amd._lib import call
    dev = torch.device("cuda:0")
    n, K, lead = args.height * args.width, args.classes, args.lead
    torch.manual_seed(0)
    rend = torch.randn(n, lead + K, device=dev)
    logits = rend[:, lead:]
    raw = torch.randint(0, K + 1, (n,), device=dev)
    conf_k = torch.zeros(K, K, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    conf_t = torch.zeros(K, K, dtype=torch.int64, device=dev)

    def kernel():
        call("ncn_sem_confusion", logits, logits.stride(0), raw, -1, -1, n, K, conf_k, counts, None)

    def torch_form():
        target = raw - 1
        if (target == -1).all():
            return
        pred = torch.argmax(logits, dim=1)
        valid = target != -1
        if valid.numel() > 0 and (True in valid):
            p, t = pred[valid], target[valid]
            conf_t.add_(torch.bincount(t * K + p, minlength=K * K).reshape(K, K))

    forms = {"kernel": kernel, "torch": torch_form}
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    conf_k.zero_(), counts.zero_(), conf_t.zero_()
    times = {k: [] for k in forms}
    for _ in range(args.iters):  # alternating: every form once per round
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(200000)  # the device is busy while the host issues the first launch
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    equal = bool(torch.equal(conf_k, conf_t))
    moved = n * ((lead + K) * 4 + 8)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"width": args.width, "height": args.height, "classes": K, "row_stride": lead + K, "iters": args.iters,
           "device": torch.cuda.get_device_name(0),
           "event_us": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
           "results_equal": equal, "counted": int(counts[0]), "bytes_to_move": moved,
           "kernel_bytes_per_s": moved / (med["kernel"] * 1e-6),
           "kernel_share_of_hbm_peak": moved / (med["kernel"] * 1e-6) / HBM_PEAK,
           "speedup_median": med["torch"] / med["kernel"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        raise SystemExit("the kernel's matrix differs from the torch form's")


if __name__ == "__main__":
    main()
