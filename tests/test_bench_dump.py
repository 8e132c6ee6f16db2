"""bench.py --dump-outputs: dump_arrays puts a step's outputs into a layout that does not depend on
the marcher's row order or sample count (per-sample arrays as (rays, K) rows in ray order, zero
behind a ray's last sample, ws zeroed where the compositor writes nothing), and stores a large
array as a fixed sample.  GPU: a plain run writes the arrays and reports only the headline (the
other measurements are behind --full), and a second run writes the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _step_outputs(order):
    """5 rays with 3, 0, 2, 4, 1 samples, placed in `order` in capacity-16 arrays; sample j of ray r
    carries the value 10 r + j; the compositor integrated 2, 0, 2, 1, 1 of them."""
    n = [3, 0, 2, 4, 1]
    rays_a, ts, s = [], torch.full((16,), -1.0), 0
    for r in order:
        rays_a.append([r, s, n[r]])
        ts[s:s + n[r]] = torch.arange(n[r]) + 10.0 * r
        s += n[r]
    per_ray = torch.arange(5.0)
    results = {"rays_a": torch.tensor(rays_a), "total_samples": torch.tensor([2, 0, 2, 1, 1]),
               "vr_samples": torch.tensor(6), "rm_samples": torch.tensor(10), "rgb": per_ray[:, None].expand(5, 3),
               "opacity": per_ray, "depth": per_ray, "deltas": ts.clone(), "ts": ts, "ws": ts.clone()}
    return results, {"total": torch.tensor(1.5), "rgb": torch.tensor(0.5)}


def test_dump_layout_is_independent_of_row_order(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLES_PER_RAY", 3)
    params = torch.arange(10.0)
    a = bench.dump_arrays(*_step_outputs([0, 1, 2, 3, 4]), params)
    b = bench.dump_arrays(*_step_outputs([3, 0, 2, 4, 1]), params)  # (long rays first)
    assert sorted(a) == sorted(b) == sorted(["rgb", "opacity", "depth", "total_samples", "n_samples", "deltas", "ts",
                                            "ws", "loss_total", "loss_rgb", "params"])
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    # (ray 3's fourth sample does not fit the 3 columns)
    assert a["ts"].tolist() == a["deltas"].tolist() == [[0, 1, 2], [0, 0, 0], [20, 21, 0], [30, 31, 32], [40, 0, 0]]
    assert a["ws"].tolist() == [[0, 1, 0], [0, 0, 0], [20, 21, 0], [30, 0, 0], [40, 0, 0]]
    assert a["n_samples"].tolist() == [3, 0, 2, 4, 1] and a["total_samples"].tolist() == [2, 0, 2, 1, 1]
    assert a["loss_total"].tolist() == [1.5] and a["params"].tolist() == list(range(10))


def test_large_array_is_a_fixed_sample(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 4)
    params = torch.arange(10.0)
    a = bench.dump_arrays(*_step_outputs([0, 1, 2, 3, 4]), params)
    b = bench.dump_arrays(*_step_outputs([3, 0, 2, 4, 1]), params)
    for k in ("params", "ts", "ws", "rgb"):
        assert a[k].shape == (4,) and np.array_equal(a[k], b[k]), k
    assert set(a["params"].tolist()) <= set(range(10)) and np.all(np.diff(a["params"]) > 0)
    assert a["loss_total"].tolist() == [1.5]  # (not over the limit: whole)


def _run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_writes_outputs_and_only_the_headline(dev, tmp_path):
    out = _run_bench("--dump-outputs", str(tmp_path / "dump"))
    assert out["steps"] == 3 and out["unit"] == "rays/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(8192 / (1e-3 * out["ms_per_step"]), rel=1e-3)
    for key in ("roofline", "kernels", "other_precision", "opaque_state", "eval_render", "cpu_baseline"):
        assert key not in out, key
    arrays = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert {"rgb", "opacity", "depth", "deltas", "ts", "ws", "loss_total", "params"} <= set(arrays)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for k, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), k
    assert arrays["rgb"].shape == (8192, 3)
    for k in ("deltas", "ts", "ws"):  # (shapes that do not depend on the marched sample count)
        assert arrays[k].shape == (8192, bench.DUMP_SAMPLES_PER_RAY), k
    assert np.count_nonzero(arrays["deltas"]) == np.minimum(arrays["n_samples"], bench.DUMP_SAMPLES_PER_RAY).sum() > 0
    assert arrays["n_samples"].sum() == pytest.approx(8192 * out["rm_samples_per_ray"], rel=0.2)
    # A second run of the same command: the dumped step starts from the seeded state, and everything
    # up to its outputs and losses is computed in a fixed order, so those are equal bit for bit.  The
    # table gradient is summed with float atomics: an entry's sum moves by a few ulp with their order,
    # and Adam's first step, lr * g / (|g| + 1e-15), turns that into ~1e-7 on a parameter except
    # where a sum cancels to rounding level (its sign is then open: up to 2 lr) -- at most a few
    # entries in 10^4.
    _run_bench("--dump-outputs", str(tmp_path / "dump2"))
    for k, a in arrays.items():
        b = np.load(tmp_path / "dump2" / (k + ".npy"))
        assert a.shape == b.shape, k
        if k == "params":
            assert np.mean(np.abs(a - b) > 1e-6) < 1e-4 and np.abs(a - b).max() <= 2.1e-2
        else:
            assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
