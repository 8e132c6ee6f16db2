"""The split backward (ncn_field_bwd_mlp_part, split_step.SplitStep, Trainer(split_backward=True))
against the one-pass field backward and the autograd step on identical inputs.

Tolerances: the rgb + sigma passes on the full grid are bit-identical to ncn_field_bwd_mlp (same
per-sample arithmetic, the rgb part of dL/dh passes through an fp32 stash, each slab tile is
written by exactly one pass); on the bench's grids (rgb pass capped at split_step.SPLIT_BLOCKS, sigma
pass at two workgroups per CU) only the slab-row partition of the weight-gradient sum changes:
rel. 1e-5.  The split step vs the autograd step:
same kernels on the same inputs, so the forward (losses, render) and every per-sample gradient are
bit-identical; the table gradient's float-atomic flush order and the split grids' slab-row
partition differ, so gradients agree to rel. L2 1e-6 (the run-to-run floor is ~5e-8) with the same
set of touched table rows; the graph-captured split step, in lockstep with the autograd graph step,
gives bit-identical losses and one-step parameters within test_gpu_graph's run-to-run bounds."""
import numpy as np
import pytest
import torch

from ncnerf_amd import _lib
from ncnerf_amd.ngp_mt import N_W, NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.split_step import SplitStep, split_eligible
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu


def _model(dev, scene, seed=7, precision="fp16"):
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("n,sort", [(1000, False), (70001, False), (70001, True), (600000, False)])
def test_mlp_parts_equal_one_pass(dev, precision, n, sort):
    """sort: the Morton-window processing order (NGPMT.sort_samples) through both passes."""
    g = torch.Generator(device=dev).manual_seed(n)
    m = NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev)
    m.sort_samples = sort
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-0.3, 0.3, generator=g)
    if m.amp_state is not None:
        m.amp_state[0] = 4.0
    x = (torch.rand(n, 3, device=dev, generator=g) - 0.5) * 0.99
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    n_dev = torch.tensor([n - 7], dtype=torch.int32, device=dev)  # (a device count below capacity)
    with torch.no_grad():
        _, _, enc, packed, order = m._field_fwd(x, d, n_dev, 0, True)
    assert (order is not None) == sort
    dsig = torch.randn(n, device=dev, generator=g) * 1e-2
    drgb = torch.randn(n, 3, device=dev, generator=g) * 1e-2
    L = _lib.lib()
    nb_full = int(L.ncn_field_bwd_blocks(n))
    dE_n = int(L.ncn_field_bwd_dE_floats(n))
    scale = m._bwd_loss_scale()

    def one_pass():
        slab = torch.full((nb_full * N_W,), float("nan"), device=dev)
        dE = torch.zeros(dE_n, device=dev)
        lmax = torch.full((16 * 256,), -1.0, device=dev)
        _lib.call("ncn_field_bwd_mlp", x, d, n, n_dev, order, packed, m._prec, enc, dsig, drgb, scale, slab, dE, lmax)
        return slab, dE, lmax

    def parts(nb1, nb2):
        g1 = nb1 or int(L.ncn_field_bwd_part_blocks(n, 1))
        g2 = nb2 or int(L.ncn_field_bwd_part_blocks(n, 2))
        slab = torch.full((max(g1, g2) * N_W,), float("nan"), device=dev)
        dE = torch.zeros(dE_n, device=dev)
        lmax = torch.full((16 * 256,), -1.0, device=dev)
        stash = torch.empty(int(L.ncn_field_bwd_stash_floats(n)), device=dev)
        for part, ds, nb in ((1, None, nb1), (2, dsig, nb2)):
            _lib.call("ncn_field_bwd_mlp_part", x, d, n, n_dev, order, packed, m._prec, enc, ds, None, drgb, scale,
                      part, nb, slab, dE, lmax, stash)
        w = torch.zeros(N_W, device=dev)
        _lib.call("ncn_field_reduce_wgrad_parts", slab, g2, g1, w)
        return slab, dE, lmax, w

    s0, e0, l0 = one_pass()
    w0 = torch.zeros(N_W, device=dev)
    _lib.call("ncn_field_reduce_wgrad", s0, nb_full, w0)
    s1, e1, l1, _ = parts(nb_full, nb_full)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1)  # every tile written, by one of the two passes, bit for bit
    assert torch.equal(e0, e1)
    assert torch.equal(l0[: 16 * nb_full], l1[: 16 * nb_full])
    # the bench's grids (rgb pass capped as split_step caps it, sigma pass at two workgroups per
    # CU): same dE and per-level maxima, weight sums regrouped over other slab rows
    s2, e2, l2, w2 = parts(min(240, nb_full), 0)
    torch.cuda.synchronize()
    assert torch.equal(e0, e2)
    rows_ref = l0[: 16 * nb_full].view(nb_full, 16).amax(0)
    assert torch.equal(l2[: 16 * nb_full].view(nb_full, 16).amax(0), rows_ref)
    assert float((w2 - w0).norm() / w0.norm()) < 1e-5


def _batch(scene, dev, R, seed):
    b = scene.torch_batch(R, seed=seed, device=dev)
    b["march_noise"] = torch.rand(R, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return b


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_split_step_matches_autograd(dev, precision):
    """One step, no optimizer: SplitStep.run vs render -> NeRFMTLoss -> backward (the Trainer's
    graph body without the split), both on the static-shape path with the same march noise."""
    scene = SyntheticScene()
    b = _batch(scene, dev, 4096, 11)
    step_dev = torch.tensor(1500, dtype=torch.int64, device=dev)  # inside the clustering ramp
    out = []
    for split in (False, True):
        m = _model(dev, scene, precision=precision)
        tr = Trainer(m, update_grid=False, use_graph=False)
        assert split_eligible(tr, b)
        m.flat_grad().zero_()
        if split:
            res, ld = SplitStep(tr).run(b, step_dev)
        else:
            kw = dict(tr.render_kwargs, static_shapes=True, march_noise=b["march_noise"], count_in_loss=True)
            res = render(m, b["rays_o"], b["rays_d"], **kw)
            ld = tr.loss(res, b, global_step=step_dev)
            ld["total"].backward()
        torch.cuda.synchronize()
        out.append(({k: float(v) for k, v in ld.items()}, {k: res[k].detach().clone() for k in ("rgb", "depth", "opacity")},
                    int(res["vr_samples"]), m.flat_grad().clone(), m._n_table))
    (l0, r0, v0, g0, nt), (l1, r1, v1, g1, _) = out
    assert l0 == l1, (l0, l1)  # the forward is the same kernels on the same inputs
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k
    assert v0 == v1 > 0
    t0, t1 = g0[:nt], g1[:nt]
    assert torch.equal(t0 != 0, t1 != 0)  # same touched table rows
    rel_t = float((t1 - t0).norm() / t0.norm())
    rel_w = float((g1[nt:] - g0[nt:]).norm() / g0[nt:].norm())
    print("split vs autograd: rel table", rel_t, "rel weights", rel_w)
    assert rel_t < 1e-6 and rel_w < 1e-6, (rel_t, rel_w)


@pytest.mark.parametrize("defer", [False, True])
def test_split_graph_step_matches_graph_step(dev, defer):
    """Trainer(use_graph=True, split_backward=True) against the autograd graph step in lockstep over
    6 steps (each step starts both from the same parameters and Adam state): the losses are
    bit-identical (the same forward kernels on the same state), and one Adam step apart the
    parameters stay within test_graph_step_matches_eager's bounds for two runs of one path.
    (Free-running comparisons over more steps are chaotic: a k-means label of a borderline normal
    flips on a 1e-7 parameter difference — measured at step 4 in ~1 of 5 pairs of runs of EITHER
    path — and moves ~1e4 table entries by a full lr step.)"""
    scene = SyntheticScene()
    batches = [_batch(scene, dev, 4096, 90 + k) for k in range(3)]
    trs = []
    for split in (False, True):
        m = _model(dev, scene)
        trs.append(Trainer(m, update_grid=False, use_graph=True, defer_optimizer=defer, split_backward=split))
    nt = trs[0].model._n_table
    for k in range(6):
        ls = []
        for tr in trs:
            _, ld = tr.step(batches[k % 3], global_step=1000 + 300 * k)
            tr.flush_optimizer()
            ls.append(float(ld["total"]))
        torch.cuda.synchronize()
        assert (trs[0]._split, trs[1]._split is not None) == (None, True)
        assert ls[0] == ls[1], (k, ls)
        p0, p1 = trs[0].model.flat_params(), trs[1].model.flat_params()
        dt = (p1[:nt] - p0[:nt]).abs()
        frac, big = float((dt > 1e-6).float().mean()), int((dt > 1e-4).sum())
        rel_w = float((p1[nt:] - p0[nt:]).norm() / p0[nt:].norm())
        print(f"step {k}: entries apart >1e-6 {frac:.2e}, >1e-4 {big}; weights rel {rel_w:.2e}")
        assert frac < 1e-3 and big <= 5e-5 * nt and rel_w < 1e-3, (k, frac, big, rel_w)
        for a, b in zip(trs[0].opt.state_tensors(), trs[1].opt.state_tensors()):
            b.copy_(a)  # (lockstep: both continue from the autograd path's state)


def test_split_refused_falls_back_to_autograd_step(dev, monkeypatch):
    """A device that cannot hold the clustering beside the rgb pass (fewer CUs than
    MI355X's 256): SplitStep refuses, and Trainer's captured step runs the autograd backward
    instead of failing; its losses equal a trainer built without the split."""
    from ncnerf_amd import split_step
    scene = SyntheticScene()
    b = _batch(scene, dev, 4096, 21)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    import ctypes
    cap = ctypes.c_int(0)
    assert _lib.lib().ncn_cluster_coresidency(20, 0, ctypes.byref(cap)) == 0
    assert split_step.device_rgb_blocks() == split_step.split_rgb_blocks(cus, cap.value // cus)
    monkeypatch.setattr(split_step, "device_rgb_blocks", lambda: cus)  # every CU busy: no room for the clustering
    res = []
    for split in (True, False):
        tr = Trainer(_model(dev, scene), update_grid=False, use_graph=True, split_backward=split)
        if split:
            with pytest.warns(UserWarning, match="split backward unavailable"):
                _, ld = tr.step(b, global_step=1500)
            assert tr._split is None
        else:
            _, ld = tr.step(b, global_step=1500)
        torch.cuda.synchronize()
        res.append(float(ld["total"]))
    assert res[0] == res[1], res
