"""The semantic metrics and the norm_nn tag on the GPU (include/ncnerf_sem.h, ncnerf_amd.metrics)
against the host restatement (tests/sem_metrics_ref.py).

The confusion matrix, the counts and the predicted labels are integers: EXACTLY equal.  The scores:
the kernel takes each quotient and mean in float64 and rounds once, the restatement works in float32
as the reference, so `ious` and `total_acc` (one float32 rounding on each side; the integers here are
below 2^24, so their conversion is exact) agree to 2^-23 relative, and the three means — a float32
sum of at most K terms, each add within 2^-24 of the partial sum, then a division — to
(K + 2) 2^-24 relative.
"""
import math

import numpy as np
import pytest
import torch

import metrics_ref as M
import sem_metrics_ref as S

pytestmark = pytest.mark.gpu

from ncnerf_amd import _lib  # noqa: E402
from ncnerf_amd import metrics as NM  # noqa: E402

NAN, INF = float("nan"), float("inf")
REL_ONE = 2.0 ** -23


def _strided(logits, pad, dev):
    """logits (n, K) on the device as a channel slice of an (n, K + pad) buffer whose other columns
    hold NaN and huge values (pad 0: the contiguous tensor)."""
    n, K = logits.shape
    if pad == 0:
        return logits.to(dev)
    buf = torch.empty(n, K + pad)
    buf[:, 0::2] = NAN
    buf[:, 1::2] = 3e38
    lo = pad // 2
    buf[:, lo:lo + K] = logits
    view = buf.to(dev)[:, lo:lo + K]
    assert view.stride() == (K + pad, 1)
    return view


def _confusion(logits_dev, raw_labels_dev, K, conf=None, counts=None, shift=-1, ignore=-1):
    n, dev = logits_dev.shape[0], logits_dev.device
    conf = torch.zeros(K, K, dtype=torch.int64, device=dev) if conf is None else conf
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else counts
    pred = torch.full((n,), -7, dtype=torch.int32, device=dev)
    _lib.call("ncn_sem_confusion", logits_dev, logits_dev.stride(0) if n > 1 else K, raw_labels_dev, shift, ignore, n, K,
              conf, counts, pred)
    return conf, counts, pred


def _check(logits, raw, K, pad, dev):
    want_conf, counted, out, want_pred = S.update(torch.zeros(K, K, dtype=torch.int64), logits, raw - 1)
    conf, counts, pred = _confusion(_strided(logits, pad, dev), raw.to(dev), K)
    assert torch.equal(conf.cpu(), want_conf)
    assert counts.tolist() == [counted, out]
    assert torch.equal(pred.cpu().long(), want_pred)
    return conf


# K: 1 and 2 (the LDS row stride K | 1 is K + 1 for even K), 33 and 48 (more than one 16-row tile of the
# head), 64 (the largest: 48.5 KiB of LDS); n_pix: one thread, a wave's edge, and 257 = two 128-row
# tiles and one pixel of a third, more tiles than the grid has workgroups
@pytest.mark.parametrize("pad", [0, 6])
@pytest.mark.parametrize("K", [1, 2, 3, 33, 48, 64])
def test_confusion_matrix_counts_and_labels_are_exact(dev, K, pad):
    for n in (1, 63, 64, 65, 257):
        logits, raw = S.make_case(n, K, seed=1000 * K + n)
        _check(logits, raw, K, pad, dev)


def test_more_pixels_than_the_grid_holds(dev):
    """256 * 1024 + 1 pixels: the grid stops growing at 1024 workgroups, each takes two 128-row tiles
    and the first a third, of one pixel."""
    n, K = 256 * 1024 + 1, 3
    logits, raw = S.make_case(n, K, seed=5)
    conf = _check(logits, raw, K, 0, dev)
    assert int(conf.sum()) == int((raw != 0).sum())


def test_ties_nan_and_equal_rows(dev):
    rows = [[1, 3, 3, 2], [NAN, 5, NAN, 1], [-INF] * 4, [2, NAN, 9, NAN], [INF, INF, 0, NAN]]
    logits = torch.tensor(rows, dtype=torch.float32)
    raw = torch.tensor([1, 2, 3, 4, 1])
    for pad in (0, 6):
        conf, counts, pred = _confusion(_strided(logits, pad, dev), raw.to(dev), 4)
        assert pred.tolist() == [1, 0, 0, 1, 3] == torch.argmax(logits, 1).tolist()
        assert conf.tolist() == [[0, 1, 0, 1], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]] and counts.tolist() == [5, 0]
    flat = torch.full((70, 48), 0.25)  # every class ties: the first wins
    conf, _, pred = _confusion(_strided(flat, 6, dev), torch.full((70,), 48).to(dev), 48)
    assert pred.tolist() == [0] * 70 and conf[47, 0].item() == 70 and int(conf.sum()) == 70


def test_void_and_out_of_range_labels(dev):
    K, n = 5, 300
    logits, raw = S.make_case(n, K, seed=9)
    before = torch.arange(K * K, dtype=torch.int64).reshape(K, K)
    conf, counts, pred = _confusion(logits.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), K,
                                    conf=before.clone().to(dev))
    assert torch.equal(conf.cpu(), before) and counts.tolist() == [0, 0]  # all void: unchanged
    assert torch.equal(pred.cpu().long(), torch.argmax(logits, 1))       # the labels of every pixel all the same
    # K + 1 and -5 after the shift: counted in counts[1], nothing else changes
    odd = raw.clone()
    odd[3], odd[200], odd[201] = K + 2, -4, 2 ** 40
    ref_conf, counted, out, _ = S.update(torch.zeros(K, K, dtype=torch.int64), logits, odd - 1)
    conf, counts, _ = _confusion(logits.to(dev), odd.to(dev), K)
    assert out == 3 and counts.tolist() == [counted, out] and torch.equal(conf.cpu(), ref_conf)
    # another ignore label and no shift, as SemanticMetrics(ignore_label=255) on shifted labels
    shifted = raw - 1
    shifted[shifted < 0] = 255
    ref_conf, counted, out, _ = S.update(torch.zeros(K, K, dtype=torch.int64), logits, shifted, ignore_label=255)
    conf, counts, _ = _confusion(logits.to(dev), shifted.to(dev), K, shift=0, ignore=255)
    assert torch.equal(conf.cpu(), ref_conf) and counts.tolist() == [counted, 0]


def test_accumulation_repeatability_and_bad_class_counts(dev):
    K = 7
    a, ra = S.make_case(500, K, seed=1)
    b, rb = S.make_case(129, K, seed=2)
    conf, counts, _ = _confusion(a.to(dev), ra.to(dev), K)
    first = conf.clone()
    _confusion(b.to(dev), rb.to(dev), K, conf=conf, counts=counts)
    want, ca, _, _ = S.update(torch.zeros(K, K, dtype=torch.int64), a, ra - 1)
    want, cb, _, _ = S.update(want, b, rb - 1)
    assert torch.equal(conf.cpu(), want) and counts.tolist() == [ca + cb, 0] and not torch.equal(first, conf)
    again, _, _ = _confusion(a.to(dev), ra.to(dev), K)
    assert torch.equal(again, first)  # two runs, the same bits
    # NULL pred_labels
    conf2 = torch.zeros(K, K, dtype=torch.int64, device=dev)
    _lib.call("ncn_sem_confusion", a.to(dev), K, ra.to(dev), -1, -1, 500, K, conf2, torch.zeros(2, dtype=torch.int64, device=dev),
              None)
    assert torch.equal(conf2, first)
    # n_cls 0 and 65: an error and no launch (the sentinels stay)
    big = torch.zeros(4, 65, device=dev)
    sentinel = torch.full((65 * 65,), -3, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), -3, dtype=torch.int64, device=dev)
    pred = torch.full((4,), -3, dtype=torch.int32, device=dev)
    for k in (0, 65):
        with pytest.raises(_lib.NcnError, match=r"n_cls = %d" % k):
            _lib.call("ncn_sem_confusion", big, 65, torch.ones(4, dtype=torch.int64, device=dev), -1, -1, 4, k, sentinel, cnt,
                      pred)
        with pytest.raises(_lib.NcnError, match=r"n_cls = %d" % k):
            _lib.call("ncn_sem_finalise", sentinel, k, big)
    with pytest.raises(_lib.NcnError, match="row_stride"):
        _lib.call("ncn_sem_confusion", big, 3, torch.ones(4, dtype=torch.int64, device=dev), -1, -1, 4, 5, sentinel, cnt, pred)
    torch.cuda.synchronize()
    assert (sentinel == -3).all() and (cnt == -3).all() and (pred == -3).all() and (big == 0).all()


# ---------------------------------------------------------------- the scores
def _random_conf():
    g = torch.Generator().manual_seed(48)
    conf = torch.randint(0, 1000, (48, 48), generator=g)
    conf[5] = 0   # two classes the ground truth does not hold; class 5 is still predicted
    conf[31] = 0
    conf[:, 31] = 0  # class 31 appears nowhere: its IoU is 0 / 0
    return conf


@pytest.mark.parametrize("conf", [torch.tensor([[2, 1, 0], [0, 0, 0], [1, 0, 3]]), torch.zeros(3, 3, dtype=torch.int64),
                                  _random_conf()], ids=["worked", "zero", "random48"])
def test_finalise_scores(dev, conf):
    K = conf.shape[0]
    out = torch.full((4 + K,), -7.0, device=dev)
    _lib.call("ncn_sem_finalise", conf.to(dev), K, out)
    out2 = torch.full((4 + K,), -7.0, device=dev)
    _lib.call("ncn_sem_finalise", conf.to(dev), K, out2)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    got, want = NM.sem_dict(out.tolist()), S.compute(conf)
    print({k: (got[k], want[k]) for k in S.KEYS})
    for g, w in zip(got["ious"], want["ious"]):
        assert S.same(g, w, REL_ONE), (g, w)
    assert S.same(got["total_acc"], want["total_acc"], REL_ONE)
    for key in ("miou", "miou_valid_cls", "cls_avg_acc"):
        assert S.same(got[key], want[key], (K + 2) * 2.0 ** -24), (key, got[key], want[key])
    if K == 48:
        assert math.isnan(got["ious"][31]) and got["ious"][5] == 0.0 and not math.isnan(got["miou"])


def test_semantic_metrics_class(dev):
    K, n = 5, 16 * 12
    logits, raw = S.make_case(n, K, seed=3)
    wide = _strided(logits, 6, dev)
    sm = NM.SemanticMetrics(K)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    sm.update(wide, (raw - 1).to(dev), pred_labels=pred)            # int64, already shifted
    sm.update(logits.to(dev), (raw - 1).to(torch.int32).to(dev))    # another integer dtype, contiguous logits
    want, counted, _, want_pred = S.update(torch.zeros(K, K, dtype=torch.int64), logits, raw - 1)
    assert sm.conf_mat.shape == (K, K) and sm.conf_mat.dtype == torch.int64 and sm.conf_mat.is_cuda
    assert torch.equal(sm.conf_mat.cpu(), 2 * want) and sm.counts.tolist() == [2 * counted, 0]
    assert torch.equal(pred.cpu().long(), want_pred)
    got, ref = sm.compute(), S.compute(2 * want)
    assert set(got) == {"miou", "miou_valid_cls", "total_acc", "cls_avg_acc", "ious"} and len(got["ious"]) == K
    for key in S.KEYS:
        assert S.same(got[key], ref[key], (K + 2) * 2.0 ** -24), key
    sm.reset()
    assert int(sm.conf_mat.sum()) == 0 and sm.counts.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="unit channel stride"):
        sm.update(logits.to(dev).T.contiguous().T, (raw - 1).to(dev))
    with pytest.raises(RuntimeError, match="float32"):
        sm.update(logits.double().to(dev), (raw - 1).to(dev))
    with pytest.raises(RuntimeError, match="integer dtype"):
        sm.update(logits.to(dev), (raw - 1).float().to(dev))
    with pytest.raises(RuntimeError, match="CUDA"):
        sm.update(logits.to(dev), raw - 1)
    assert int(sm.conf_mat.sum()) == 0


# ---------------------------------------------------------------- ViewMetrics and evaluate_views
H, W, V, K5 = 16, 12, 2, 5


def _count_host_copies(monkeypatch):
    copies = []
    for name in ("cpu", "numpy", "tolist", "item", "__float__", "__int__", "__bool__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, **k):
            if self.is_cuda:
                copies.append(self.numel())
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    return copies


def test_view_metrics_with_the_new_flags(dev, monkeypatch):
    n = H * W
    g = torch.Generator().manual_seed(11)
    views = []
    for v in range(V):
        rgb = torch.rand(n, 3, generator=g)
        nrm = torch.randn(n, 3, generator=g)
        gt = torch.randn(n, 3, generator=g)
        gt[::4] = 0.0
        logits, raw = S.make_case(n, K5, seed=20 + v)
        rend = torch.cat([rgb, nrm, logits], dim=1).to(dev)  # the test renderer's layout with both heads
        preds = {"rgb": rend[:, :3].contiguous(), "norm_depth": rend[:, 3:6].contiguous(), "norm_nn": rend[:, 3:6],
                 "sem": rend[:, 6:]}
        target = {"rgb": (rgb + 0.05).to(dev), "normals": gt.to(dev), "semantics": raw.to(torch.uint8).to(dev)}
        views.append((preds, target, logits, raw))
    assert views[0][0]["sem"].stride() == (6 + K5, 1)
    plain = NM.ViewMetrics(norm_gt=True)
    full = NM.ViewMetrics(norm_gt=True, pred_norm_nn=True, eval_sem=True, n_sem_cls=K5)
    conf = torch.zeros(K5, K5, dtype=torch.int64)
    for preds, target, logits, raw in views:
        plain.update(preds, target, H, W)
        full.update(preds, target, H, W)
        conf = S.update(conf, logits, raw - 1)[0]
    rows, nn_rows = full.rows(), full.nn_rows()
    assert rows.shape == (V, 12) and nn_rows.shape == (V, 5) and NM.NN_COLUMNS == NM.COLUMNS[7:]
    assert torch.equal(rows.view(torch.int32), plain.rows().view(torch.int32))         # the old row keeps its bits
    assert torch.equal(nn_rows.view(torch.int32), rows[:, 7:].contiguous().view(torch.int32))  # the same tensor, the same numbers
    assert (nn_rows[:, 4] == 1).all() and (nn_rows[:, :4] > 0).all()
    assert torch.equal(full.sem.conf_mat.cpu(), conf)
    old = plain.compute()
    copies = _count_host_copies(monkeypatch)
    logs = full.compute()
    monkeypatch.undo()
    assert copies == [V * 12 + V * 5 + 4 + K5], copies  # ONE copy: the single concatenated tensor
    assert {k: logs[k] for k in old} == old
    want = S.compute(conf)
    assert set(logs) == set(old) | {f"norm_nn/ang_err_{k}" for k in ("mean", "median", "mean_min", "median_min")} | {
        f"sem/{k}" for k in S.KEYS}
    for k in ("mean", "median", "mean_min", "median_min"):
        assert logs[f"norm_nn/ang_err_{k}"] == logs[f"norm_depth/ang_err_{k}"]
    assert S.same(logs["sem/total_acc"], want["total_acc"], REL_ONE)
    for key in ("miou", "miou_valid_cls", "cls_avg_acc"):
        assert S.same(logs[f"sem/{key}"], want[key], (K5 + 2) * 2.0 ** -24), key
    full.reset()
    assert int(full.sem.conf_mat.sum()) == 0
    with pytest.raises(RuntimeError, match="no view yet"):
        full.rows()


def test_evaluate_views_with_sem_gt_and_the_normal_head(dev, monkeypatch):
    import ncnerf_amd.evaluation as Ev
    import ncnerf_amd.rendering as rendering
    from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
    from ncnerf_amd.synthetic import SyntheticScene
    from test_gpu_eval import dir_grid
    scene = SyntheticScene()
    torch.manual_seed(7)
    model = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=K5, pred_norm=True).to(dev))
    with torch.no_grad():
        model.density_grid.copy_(torch.from_numpy(scene.density_grid).to(dev) * 10.0)
        model.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    dirs = torch.from_numpy(np.ascontiguousarray(dir_grid(H, W))).to(dev)
    poses = torch.from_numpy(np.ascontiguousarray(scene.poses[:V])).to(dev)
    n = H * W
    g = torch.Generator().manual_seed(4)
    rgb_gt = torch.rand(V, n, 3, generator=g).to(dev)
    normals_gt = torch.randn(V, n, 3, generator=g)
    normals_gt[:, ::5] = 0.0
    sem_gt = torch.randint(0, K5 + 1, (V, H, W), generator=g)
    seen = []
    orig_render = rendering.render

    def render_spy(*a, **k):
        res = orig_render(*a, **k)
        seen.append((res["sem"].clone(), res["norm_nn"].clone(), res["sem"].stride()))
        return res
    monkeypatch.setattr(rendering, "render", render_spy)
    # (R_ref: the frame's columns are then signed towards it; three raw centroids may be left-handed)
    kw = dict(rgb_gt=rgb_gt, K=10, niter=5, R_ref=torch.eye(3), normals_gt=normals_gt.to(dev), n_sem_cls=K5)
    out = Ev.evaluate_views(model, poses, dirs, (W, H), sem_gt=sem_gt.to(dev), **kw)
    monkeypatch.undo()
    assert len(seen) == V and seen[0][2] == (3 + 3 + K5, 1)  # the slice of the render buffer, as it was scored
    conf = torch.zeros(K5, K5, dtype=torch.int64)
    for v, (sem, _, _) in enumerate(seen):
        conf = S.update(conf, sem.cpu(), sem_gt[v].reshape(-1) - 1)[0]
    assert out["conf_mat"].is_cuda and torch.equal(out["conf_mat"].cpu(), conf) and int(conf.sum()) > 0
    want = S.compute(conf)
    logs = out["metrics"]
    assert S.same(logs["sem/total_acc"], want["total_acc"], REL_ONE)
    for key in ("miou", "miou_valid_cls", "cls_avg_acc"):
        assert S.same(logs[f"sem/{key}"], want[key], (K5 + 2) * 2.0 ** -24), key
    assert len(out["sem_ious"]) == K5 and all(S.same(a, b, REL_ONE) for a, b in zip(out["sem_ious"], want["ious"]))
    # the norm_nn tag against the float64 definition on the rendered norm_nn (tolerances of
    # test_gpu_metrics.test_view_metrics_through_evaluate_views: 1e-3 degrees on a mean, 0.05 on a median)
    cols = ("nn_ang_mean", "nn_ang_median", "nn_ang_mean_min", "nn_ang_median_min", "nn_norm_counted")
    refs = []
    for v, (_, nn, _) in enumerate(seen):
        ref = M.normals_f64(nn.cpu().numpy(), normals_gt[v].numpy())
        refs.append(ref)
        row = out["per_view"][v]
        assert tuple(row) == NM.COLUMNS + cols and ref[4] == 1 == row["nn_norm_counted"]
        for c, r, tol in zip(cols[:4], ref[:4], (1e-3, 0.05, 1e-3, 0.05)):
            assert abs(row[c] - r) <= tol, (v, c, row[c], r)
    for i, name in enumerate(("mean", "median", "mean_min", "median_min")):
        mean = sum(r[i] for r in refs) / V
        assert abs(logs[f"norm_nn/ang_err_{name}"] - mean) <= (1e-3, 0.05)[i % 2]
        assert f"norm_depth/ang_err_{name}" in logs
    assert {"sem/miou", "sem/miou_valid_cls", "sem/total_acc", "sem/cls_avg_acc"} <= set(logs)
    # without n_sem_cls, or with a model without the head: ValueError before anything is rendered
    with pytest.raises(ValueError, match="n_sem_cls"):
        Ev.evaluate_views(model, poses, dirs, (W, H), sem_gt=sem_gt.to(dev), rgb_gt=rgb_gt)
    torch.manual_seed(7)
    bare = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with pytest.raises(ValueError, match="semantic head"):
        Ev.evaluate_views(bare, poses, dirs, (W, H), sem_gt=sem_gt.to(dev), rgb_gt=rgb_gt, n_sem_cls=K5)
