"""The host side of Trainer.fit (no GPU): TrainLog's decoding of the device ring, the rank seed of
the batch draws, and the pose group's learning-rate schedule."""
import math

import numpy as np
import pytest
import torch

from ncnerf_amd import distributed
from ncnerf_amd.optim import POSE_LR, PoseAdam, cosine_factor
from ncnerf_amd.trainer import TrainLog, pose_lr, rank_seed

LOSS_D = {"rgb": 0, "opacity": 0, "norm_D_C_ort_dot": 0, "norm_D_C_centr_dot": 0, "norm_D_C_centr_L1": 0, "total": 0}
COLS = ("step", "total", "rgb", "opacity", "norm_D_C_ort_dot", "norm_D_C_centr_dot", "norm_D_C_centr_L1", "rm_samples",
        "vr_samples")


def _row(step):
    """A row whose every value names its step and column."""
    return [float(step), 10.0 + step, 0.001 * (step + 1)] + [step + 0.125 * c for c in range(3, 7)] + [
        64.0 * step, 32.0 * step]


def _ring(capacity, first, count):
    """The ring as the device leaves it after the steps [first, first + count): step s in row s % capacity."""
    ring = torch.full((capacity, len(COLS)), -1.0)
    for s in range(first, first + count):
        ring[s % capacity] = torch.tensor(_row(s))
    return ring


def test_column_names_put_total_first():
    assert TrainLog.column_names(LOSS_D) == COLS
    assert TrainLog.column_names({"rgb": 0, "total": 0}) == ("step", "total", "rgb", "rm_samples", "vr_samples")


def test_decoding_by_name_psnr_and_per_ray_counts():
    log = TrainLog(n_rays=64)
    log.add_ring(_ring(6, 100, 6), COLS, 100, 6)
    assert len(log) == 6 and log.columns == COLS
    assert log.steps.dtype == torch.int64 and log.steps.tolist() == list(range(100, 106))
    want = torch.tensor([_row(s) for s in range(100, 106)])
    for c, name in enumerate(COLS):
        assert torch.equal(log[name], want[:, c]), name
    assert torch.equal(log["psnr"], -10.0 * torch.log10(want[:, 2]))
    np.testing.assert_allclose(log["psnr"].numpy(), [-10 * math.log10(0.001 * (s + 1)) for s in range(100, 106)],
                               rtol=1e-6)
    assert log["rm_s"].tolist() == [float(s) for s in range(100, 106)]  # 64 s samples over 64 rays
    assert log["vr_s"].tolist() == [0.5 * s for s in range(100, 106)]
    with pytest.raises(KeyError):
        log["depth"]


def test_ring_order_after_wrap_around():
    """Capacity 8, steps 1000..1019 in drains of 8, 8 and 4: 1000 % 8 == 0, but 1016..1019 overwrite
    rows 0..3 only, and a start that is no multiple of the capacity wraps inside one drain."""
    assert TrainLog.ring_rows(1000, 8, 8) == list(range(8))
    assert TrainLog.ring_rows(1003, 8, 8) == [3, 4, 5, 6, 7, 0, 1, 2]
    log = TrainLog(n_rays=64)
    for first, count in ((1003, 8), (1011, 8), (1019, 4)):
        log.add_ring(_ring(8, first, count), COLS, first, count)
    assert log.steps.tolist() == list(range(1003, 1023))
    assert torch.equal(log["total"], torch.tensor([10.0 + s for s in range(1003, 1023)]))
    with pytest.raises(ValueError, match="drained too late"):
        TrainLog.ring_rows(0, 9, 8)
    with pytest.raises(ValueError, match="columns"):
        log.add_ring(torch.zeros(8, 4), COLS, 0, 1)


def test_a_term_that_appears_later_is_nan_before():
    """The eager step's loss dict can gain a term (a schedule that starts): earlier steps hold NaN."""
    log = TrainLog(n_rays=64)
    log.add_ring(torch.tensor([[5.0, 1.0, 1.0, 10.0, 9.0]]), ("step", "total", "rgb", "rm_samples", "vr_samples"), 5, 1)
    log.add_ring(torch.tensor([[6.0, 3.0, 1.0, 2.0, 10.0, 9.0]]),
                 ("step", "total", "rgb", "reg_depth", "rm_samples", "vr_samples"), 6, 1)
    assert log.columns == ("step", "total", "rgb", "rm_samples", "vr_samples", "reg_depth")
    assert log["total"].tolist() == [1.0, 3.0]
    assert math.isnan(log["reg_depth"][0]) and float(log["reg_depth"][1]) == 2.0


def test_rank_seed_is_seed_plus_rank(monkeypatch):
    class DS:
        seed = 21

    assert distributed.rank() == 0 and rank_seed(DS) == 21  # (no process group)
    monkeypatch.setattr(distributed, "rank", lambda: 3)
    assert rank_seed(DS) == 24


def test_pose_group_cosine_factor():
    """CosineAnnealingLR(T_max=30, eta_min=0) holds every group: factor 1, 1/2, 0 at epochs 0, 15, 30."""
    assert cosine_factor(0, 30) == 1.0
    assert abs(cosine_factor(15, 30) - 0.5) < 1e-15
    assert abs(cosine_factor(30, 30)) < 1e-15
    assert POSE_LR == 1e-6
    assert pose_lr(0, 30) == 1e-6 and abs(pose_lr(15, 30) - 0.5e-6) < 1e-20 and abs(pose_lr(30, 30)) < 1e-20
    assert pose_lr(7, None) == 1e-6  # (no schedule)
    # the field's learning rate is the same factor of its base, to the bit of the expression it had
    for e in range(0, 31):
        assert 1e-2 * cosine_factor(e, 30) == 0.5 * 1e-2 * (1 + math.cos(math.pi * e / 30))


def test_pose_adam_on_cpu_tensors():
    """PoseAdam against torch.optim.Adam (lr 1e-6, eps 1e-8) over three steps; a non-finite gradient
    leaves parameters, moments and step count bit-identical."""
    g = torch.Generator().manual_seed(0)
    p0 = [torch.randn(5, 3, generator=g) * 0.02, torch.randn(5, 3, generator=g) * 1e-3]
    mine = [torch.nn.Parameter(p.clone()) for p in p0]
    ref = [torch.nn.Parameter(p.double().clone()) for p in p0]
    opt, ref_opt = PoseAdam(mine), torch.optim.Adam(ref, lr=1e-6, eps=1e-8)
    for k in range(3):
        grads = [torch.randn(5, 3, generator=g) * 1e-3 for _ in p0]
        grads[0][2] = 0.0  # (an image absent from the batch)
        for p, r, gr in zip(mine, ref, grads):
            p.grad, r.grad = gr.clone(), gr.double()
        opt.step(0.75)
        ref_opt.param_groups[0]["lr"] = 0.75e-6
        ref_opt.step()
    for p, r, start in zip(mine, ref, p0):
        # three fp32 roundings of the parameter (2^-24 relative each) and one for the update's own
        # arithmetic (~1e-6 x 1e-6, far below); a wrong step is off by ~lr = 1e-6, a hundred times that
        err = float((p.detach().double() - r.detach()).abs().max())
        assert err <= 4 * 2.0 ** -24 * float(r.detach().abs().max()), err
        assert float((p.detach() - start).abs().max()) > 1e-6
    assert torch.equal(mine[0][2], p0[0][2])  # zero gradient, zero moments: no move
    before = [t.clone() for t in opt.state_tensors()]
    mine[0].grad = torch.full((5, 3), float("inf"))
    mine[1].grad = torch.ones(5, 3)
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, opt.state_tensors())) and float(opt.t) == 3.0
    opt.zero_grad()
    assert mine[0].grad is None and mine[1].grad is None
