"""The static-shape render path and the HIP-graph-captured training step (Trainer(use_graph=True))
against the eager path on identical inputs.

Tolerances: static vs dynamic render bit-exact (same kernels, the field stops at the device count);
graph vs eager training: per-step loss within 1e-4 relative; over 4 Adam steps at most 1e-5 of
the hash-table entries moved by more than 1e-4 and under 0.1% by more than 1e-6 between any two
runs (the table-gradient flush uses float atomics: two runs are equal up to summation order, and
Adam with eps 1e-15 turns a near-zero gradient's sign into a full lr step); MLP weights within 1e-3."""
import numpy as np
import pytest
import torch

from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu


def _model(dev, scene, seed=7):
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


def test_static_shapes_render_matches_dynamic(dev):
    scene = SyntheticScene()
    m = _model(dev, scene)
    b = scene.torch_batch(2048, seed=3, device=dev)
    noise = torch.rand(2048, device=dev)
    kw = dict(near_distance=0.01, max_samples=1024, march_noise=noise)
    with torch.no_grad():
        r0 = render(m, b["rays_o"], b["rays_d"], **kw)
        r1 = render(m, b["rays_o"], b["rays_d"], static_shapes=True, **kw)
    assert int(r0["rm_samples"]) == int(r1["rm_samples"])
    assert r1["ts"].shape[0] == 2048 * 1024  # capacity
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(r0[k], r1[k]), k
    S = int(r0["rm_samples"])
    assert torch.equal(r0["ts"], r1["ts"][:S])


def test_static_shapes_render_matches_dynamic_two_cascades(dev):
    """The same at scale 1.0 (C = 2, a different bitfield per cascade), constant dt: the static-shape
    path takes the one-launch marcher (ncn_march_train_fused at C > 1), the dynamic one the eager
    marcher; 256 rays."""
    import scale_cases as sc
    from ncnerf_amd.rendering import _fused_march_ok
    scene = SyntheticScene()
    torch.manual_seed(7)
    m = register_grid_buffers(NGPMT(scale=1.0, grid_size=128).to(dev))
    assert m.cascades == 2
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(np.array(sc.cascade_bitfield(2))).to(dev))
    n = 256
    b = scene.torch_batch(n, seed=3, device=dev)
    noise = torch.rand(n, device=dev)
    kw = dict(near_distance=0.01, max_samples=1024, march_noise=noise)
    assert _fused_march_ok(m, dict(static_shapes=True, **kw), n) and not _fused_march_ok(m, dict(kw), n)
    with torch.no_grad():
        r0 = render(m, b["rays_o"], b["rays_d"], **kw)
        r1 = render(m, b["rays_o"], b["rays_d"], static_shapes=True, **kw)
    S = int(r0["rm_samples"])
    assert S == int(r1["rm_samples"]) > 20 * n
    assert r1["ts"].shape[0] == n * 1024  # capacity
    for k in ("rgb", "depth", "opacity"):
        assert torch.equal(r0[k], r1[k]), k
    assert torch.equal(r0["ts"], r1["ts"][:S])


def test_graph_step_matches_eager(dev):
    """Two eager runs give the run-to-run floor (float atomics in the table-gradient flush and the
    dW reduction sum in arrival order; Adam's m/sqrt(v) turns a sign flip of a near-zero gradient
    into a full lr step), the graph run must stay within a small multiple of it."""
    scene = SyntheticScene()
    batches = []
    for k in range(4):
        b = scene.torch_batch(4096, seed=50 + k, device=dev)
        b["march_noise"] = torch.rand(4096, device=dev, generator=torch.Generator(device=dev).manual_seed(k))
        batches.append(b)
    losses, params = [], []
    for use_graph in (False, False, True):
        m = _model(dev, scene)
        tr = Trainer(m, update_grid=False, use_graph=use_graph)
        ls = []
        for k, b in enumerate(batches):
            _, ld = tr.step(b, global_step=1000 + 400 * k)  # inside the clustering ramp
            ls.append(float(ld["total"]))
        torch.cuda.synchronize()
        losses.append(np.array(ls))
        params.append(m.flat_params().detach().clone())
    np.testing.assert_allclose(losses[2], losses[0], rtol=1e-4)
    # hash-table entries: the float-atomic summation order differs run to run, and Adam (eps 1e-15)
    # turns the sign of a near-zero gradient into a full +-lr step, so a few hundred of the 11.4M
    # entries (measured: ~150 between two eager runs) may move by ~lr between ANY two runs (eager or
    # graph); everything else agrees
    n_t = _model(dev, scene)._n_table
    for other in (1, 2):
        d = (params[other][:n_t] - params[0][:n_t]).abs()
        big = int((d > 1e-4).sum())
        assert big <= 5e-5 * n_t, (other, big)
        assert float((d > 1e-6).float().mean()) < 1e-3, other
    # the MLP weights (dense, large gradients) agree tightly
    rel_w = float((params[2][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm())
    assert rel_w < 1e-3, rel_w


def test_step_inputs_copy(dev):
    """ncn_step_inputs: every buffer copied byte for byte (16-B chunks, byte tails, unaligned views),
    the device step counter written, in one launch."""
    from ncnerf_amd import _lib
    g = torch.Generator(device=dev).manual_seed(0)
    srcs = [torch.randn(n, device=dev, generator=g) for n in (1, 17, 8192 * 3, 100003)]
    srcs.append(torch.randint(0, 1 << 40, (777,), device=dev, dtype=torch.int64, generator=g))
    base = torch.randn(64, device=dev, generator=g)
    srcs.append(base[1:34])  # (a view at a 4-B offset: byte-copy path)
    dsts = [torch.full_like(s, -7) for s in srcs]
    step = torch.zeros((), dtype=torch.int64, device=dev)
    _lib.step_inputs(srcs, dsts, step, 123456789012)
    torch.cuda.synchronize()
    for s, d in zip(srcs, dsts):
        assert torch.equal(s, d)
    assert int(step) == 123456789012


def test_deferred_optimizer_matches_graph_step(dev):
    """Trainer(defer_optimizer=True): step k's optimizer runs inside graph k+1 beside its marcher
    (gated off when nothing is pending), a grid refresh flushes it first.  Over 20 steps with
    refreshes at 0 and 16 the losses and, after flush_optimizer(), the parameters match the plain
    graph step within the run-to-run floor of test_graph_step_matches_eager; the device step
    counter counts exactly one optimizer step per training step."""
    scene = SyntheticScene()
    batches = []
    for k in range(4):
        b = scene.torch_batch(4096, seed=70 + k, device=dev)
        b["march_noise"] = torch.rand(4096, device=dev, generator=torch.Generator(device=dev).manual_seed(k))
        batches.append(b)
    out = []
    for defer in (False, True):
        m = _model(dev, scene)
        tr = Trainer(m, update_grid=True, use_graph=True, defer_optimizer=defer)
        tr.grid_seed = lambda k: 1000 + k
        ls = []
        for k in range(20):
            _, ld = tr.step(batches[k % 4], global_step=k)
            ls.append(float(ld["total"]))
        tr.flush_optimizer()
        torch.cuda.synchronize()
        assert int(tr.opt.step_dev) == 20
        out.append((np.array(ls), m.flat_params().detach().clone(), m.density_bitfield.clone()))
    np.testing.assert_allclose(out[1][0], out[0][0], rtol=1e-3)
    n_t = _model(dev, scene)._n_table
    d = (out[1][1][:n_t] - out[0][1][:n_t]).abs()
    assert int((d > 1e-4).sum()) <= 5e-5 * n_t
    rel_w = float((out[1][1][n_t:] - out[0][1][n_t:]).norm() / out[0][1][n_t:].norm())
    assert rel_w < 1e-3, rel_w


def test_graph_step_sample_counts(dev):
    """The graph step's sample counts (the loss node's first launch sums the compositor's per-ray
    counts; the bench's device accumulators): vr_samples of each step == the eager render's, and the
    accumulators hold the marched and composited totals of the replayed steps."""
    scene = SyntheticScene()
    m = _model(dev, scene)
    tr = Trainer(m, update_grid=False, use_graph=True)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    tr.render_kwargs["count_acc"] = acc
    want_rm, want_vr = 0, 0
    for k in range(3):
        b = scene.torch_batch(2048, seed=70 + k, device=dev)
        b["march_noise"] = torch.rand(2048, device=dev, generator=torch.Generator(device=dev).manual_seed(k))
        if k == 1:
            acc.zero_()  # (step 0 captured the graph: its warm-up bodies counted too)
        with torch.no_grad():
            r = render(m, b["rays_o"], b["rays_d"], near_distance=0.01, max_samples=1024,
                       march_noise=b["march_noise"], static_shapes=True)
        out, _ = tr.step(b, global_step=1000 + k)
        torch.cuda.synchronize()
        assert int(out["vr_samples"]) == int(r["vr_samples"]) > 0
        if k >= 1:
            want_rm += int(r["rm_samples"])
            want_vr += int(r["vr_samples"])
    assert int(acc[0]) == want_rm and int(acc[1]) == want_vr, (acc.tolist(), want_rm, want_vr)
