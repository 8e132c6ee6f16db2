"""Training from the device ray dataset: Trainer.step_from, Trainer.fit and the device log.

Set-up shared by the tests: the 5-view 24x20 room dataset of tests/test_gpu_data.py, patch 8, 1024
rays (16 patches: the reference loss configuration with its clustering; 128 rays for the pose test),
the model of tests/test_gpu_graph.py, update_grid off unless stated, the trainers' jitter seed
(`_rng_seed`) equal across the runs that are compared.

Bounds: the drawn batch of a replay against DeviceRayDataset.batch of the same step bit for bit
(same kernels, same inputs); dataset-sourced steps against host-batch steps by the acceptance of
tests/test_gpu_graph.py::test_graph_step_matches_eager (two runs differ by the float atomics of the
table-gradient flush, so a second host-batch run gives the floor, and the dataset-sourced run is
held to what that one is held to); the pose step against an fp64 Adam step within 4 ulp of the
fp32 parameter."""
import numpy as np
import pytest
import torch

import data_ref
from ncnerf_amd.data import DeviceRayDataset
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene, make_cameras
from ncnerf_amd.trainer import Trainer, TrainLog, pose_lr, rank_seed

pytestmark = pytest.mark.gpu

V, H, W = 5, 20, 24
RAYS = 1024
TENSORS = ("img_idxs", "pix_idxs", "rays_o", "rays_d", "rgb")
FAR = 10 ** 6 + 3  # a status_interval that no step of these tests is a multiple of


def _room_dataset(dev, batch_size, **kw):
    """tests/test_gpu_data.py::_room_dataset: 5 cameras inside the synthetic room, 24x20 images."""
    images, _, directions = data_ref.small_scene(V, H, W, seed=6)
    poses = make_cameras(V, seed=2)
    return DeviceRayDataset(torch.from_numpy(images).to(dev), torch.from_numpy(poses).to(dev),
                            torch.from_numpy(directions).to(dev), (W, H), batch_size=batch_size, seed=21, **kw)


def _model(dev, scene, seed=7):
    """tests/test_gpu_graph.py::_model."""
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


def _trainer(dev, scene, **kw):
    tr = Trainer(_model(dev, scene), **dict(dict(update_grid=False, use_graph=True), **kw))
    tr._rng_seed = 1234
    return tr


def _host_batch(ds, s):
    """The batch of step s as a dict somebody built: clones, so nothing aliases the dataset's buffers."""
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in ds.batch(s).items()}


# ---- 1. the replayed draw follows the step counter ------------------------------------------------
@pytest.mark.parametrize("labels", [False, True], ids=["rgb", "depth_semantics"])
def test_replayed_draw_follows_the_step_counter(dev, labels):
    """The first step_from captures, the later ones replay; after each, the static buffers hold the
    batch DeviceRayDataset.batch draws for that step from a host step value, bit for bit.  A step baked
    into the capture as a constant would repeat the first batch."""
    kw = {}
    if labels:
        g = torch.Generator().manual_seed(4)
        kw = dict(depth=torch.rand(V, H * W, generator=g).to(dev),
                  semantics=torch.randint(0, 6, (V, H * W), generator=g).to(torch.uint8).to(dev))
    ds = _room_dataset(dev, RAYS, **kw)
    tr = _trainer(dev, SyntheticScene())
    keys = TENSORS + (("depth", "semantics") if labels else ())
    seen = []
    for s in (3000, 3001, 3017):
        tr.step_from(ds, s)
        torch.cuda.synchronize()
        ref = ds.batch(s)
        assert set(keys) <= set(tr.last_batch)
        for k in keys:
            assert torch.equal(tr.last_batch[k], ref[k]), (s, k)
        assert tr.last_batch["patch_area"] == 64
        seen.append({k: tr.last_batch[k].clone() for k in keys})
    assert int(tr._step_dev) == 3017
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for k in ("pix_idxs", "rays_d", "rgb"):
            assert not torch.equal(seen[a][k], seen[b][k]), (a, b, k)


# ---- 2. dataset-sourced step equals host-batch step ------------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "deferred", "eager"])
def test_dataset_step_matches_host_batch_step(dev, mode):
    """Runs (a) and (b): step() fed copies of ds.batch(s); run (c): step_from(ds, s); steps 1000, 1400,
    1800 (inside the clustering ramp).  The acceptance of test_graph_step_matches_eager, (c) against
    (a) held to what (b) against (a) is held to."""
    scene = SyntheticScene()
    ds = _room_dataset(dev, RAYS)
    steps = (1000, 1400, 1800)
    losses, params = [], []
    for run in ("a", "b", "c"):
        tr = _trainer(dev, scene, use_graph=mode != "eager", defer_optimizer=mode == "deferred")
        torch.manual_seed(99)  # (the eager marcher's jitter comes from torch's generator)
        ls = []
        for s in steps:
            _, ld = tr.step_from(ds, s) if run == "c" else tr.step(_host_batch(ds, s), s)
            ls.append(float(ld["total"].detach()))
        tr.flush_optimizer()
        torch.cuda.synchronize()
        assert tr.opt.step_count == len(steps)
        losses.append(np.array(ls))
        params.append(tr.model.flat_params().detach().clone())
        n_t = tr.model._n_table
    print(f"{mode}: losses a {losses[0]}, c - a {losses[2] - losses[0]}, b - a {losses[1] - losses[0]}")
    np.testing.assert_allclose(losses[2], losses[0], rtol=1e-4)
    for other in (1, 2):
        d = (params[other][:n_t] - params[0][:n_t]).abs()
        big, small = int((d > 1e-4).sum()), float((d > 1e-6).float().mean())
        print(f"{mode}: run {'abc'[other]} vs a: {big} table entries moved by > 1e-4, a fraction {small:.2e} by > 1e-6")
        assert big <= 5e-5 * n_t, (other, big)
        assert small < 1e-3, (other, small)
    rel_w = float((params[2][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm())
    assert rel_w < 1e-3, rel_w
    assert not torch.equal(params[0], _model(dev, scene).flat_params())  # (the runs trained)


# ---- 3. a foreign source is refused ------------------------------------------------------------------
def test_foreign_source_is_refused(dev):
    scene = SyntheticScene()
    ds, other = _room_dataset(dev, RAYS), _room_dataset(dev, RAYS)
    tr = _trainer(dev, scene)
    tr.step_from(ds, 1000)
    torch.cuda.synchronize()

    def refused(call, exc=RuntimeError, match="captured step"):
        before = tr.model.flat_params().clone()
        count = tr.opt.step_count
        with pytest.raises(exc, match=match):
            call()
        torch.cuda.synchronize()
        assert torch.equal(before, tr.model.flat_params()) and tr.opt.step_count == count

    host = _host_batch(ds, 1001)
    refused(lambda: tr.step(host, 1001))
    refused(lambda: tr.step_from(other, 1001))
    refused(lambda: tr.fit(other, 2, start_step=1001))
    tr.step_from(ds, 1001)  # (its own source still trains)
    # ... and the other way round: a graph captured from a host batch does not draw
    tr = _trainer(dev, scene)
    tr.step(host, 1001)
    torch.cuda.synchronize()
    refused(lambda: tr.step_from(ds, 1002))
    tr.step(_host_batch(ds, 1002), 1002)


# ---- 4. pose refinement, eager ----------------------------------------------------------------------
def test_pose_refinement_eager(dev):
    """The set-up of test_pose_gradients_through_the_dataset (optimize_ext, 128 rays, loss scale 1, full
    bitfield), one step_from at step 3000 (epoch 3 of 30).  A first Adam step from zero moments is
    p - lr g / (|g| + eps), lr = pose_lr(3, 30), eps = 1e-8: computed in fp64 from the pose gradients
    of a manual ds.batch -> render -> loss -> backward pass over the same state, and compared within
    4 ulp of the fp32 parameter.  Rows of images absent from the batch do not move at all (their
    gradient and moments are exactly zero)."""
    ds = _room_dataset(dev, 128, optimize_ext=True)
    torch.manual_seed(0)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    m.amp_state[0] = 1.0
    m.density_bitfield.fill_(255)
    rng = np.random.default_rng(8)  # a pose correction that is not the origin: |dR| = 0.02, dT ~ 1e-3
    ax = rng.normal(size=(V, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    with torch.no_grad():
        ds.dR.copy_(torch.from_numpy((0.02 * ax).astype(np.float32)).to(dev))
        ds.dT.copy_(torch.from_numpy(rng.uniform(-2e-3, 2e-3, size=(V, 3)).astype(np.float32)).to(dev))
    tr = Trainer(m, update_grid=False, use_graph=False)
    step = 3000
    start = {"dR": ds.dR.detach().clone(), "dT": ds.dT.detach().clone()}
    # the manual pass: the step's own calls, the jitter from the generator state the step will see
    amp = m.amp_state.clone()
    b = ds.batch(step, seed=rank_seed(ds))
    torch.manual_seed(5)
    ld = tr.loss(render(m, b["rays_o"], b["rays_d"], **dict(tr.render_kwargs, global_step=step)), b, global_step=step)
    ld["total"].backward()
    grads = {"dR": ds.dR.grad.double().cpu(), "dT": ds.dT.grad.double().cpu()}
    present = torch.zeros(V, dtype=torch.bool)
    present[b["img_idxs"].cpu()] = True
    assert 0 < int(present.sum()) < V
    assert bool((grads["dR"][~present] == 0).all()) and float(grads["dR"][present].abs().min()) > 0
    with torch.no_grad():
        m.flat_grad().zero_()
        m.amp_state.copy_(amp)
    ds.dR.grad = ds.dT.grad = None
    before = m.flat_params().clone()
    # the step
    torch.manual_seed(5)
    tr.step_from(ds, step)
    torch.cuda.synchronize()
    assert not torch.equal(before, m.flat_params())
    lr = pose_lr(3, 30)
    assert abs(lr - 1e-6 * 0.5 * (1 + np.cos(np.pi * 0.1))) < 1e-20
    for name, p in (("dR", ds.dR), ("dT", ds.dT)):
        got, p0, g = p.detach().cpu(), start[name].cpu(), grads[name]
        assert torch.equal(got[~present], p0[~present]), name
        want = (p0.double() - lr * g / (g.abs() + 1e-8)).float()
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        err = ((got.double() - want.double()).abs() / ulp.double())[present]
        same = torch.equal(p.grad.double().cpu(), g)
        print(f"{name}: worst error {float(err.max()):.2f} ulp; the step's gradient equals the manual pass's: {same}")
        assert float(err.max()) <= 4, name
        assert bool((got != p0)[present].all()), name  # (lr is ~500 ulp of 0.02 and ~8000 ulp of 1e-3)
    assert float(tr.pose_opt.t) == 1.0
    # a non-finite pose gradient: dR, dT and the pose moments stay, the field takes its step
    hook = ds.dR.register_hook(lambda grad: torch.full_like(grad, float("inf")))
    state = [t.detach().clone() for t in tr.pose_opt.state_tensors()]
    before = m.flat_params().clone()
    tr.step_from(ds, step + 1)
    hook.remove()
    torch.cuda.synchronize()
    assert bool(torch.isinf(ds.dR.grad).all()) and bool(torch.isfinite(ds.dT.grad).all())
    for a, t in zip(state, tr.pose_opt.state_tensors()):
        assert torch.equal(a, t.detach())
    assert not torch.equal(before, m.flat_params())
    # the captured step refuses the dataset before it captures or launches anything
    tg = Trainer(m, update_grid=False, use_graph=True)
    before = m.flat_params().clone()
    with pytest.raises(NotImplementedError, match="use_graph=False"):
        tg.step_from(ds, 0)
    with pytest.raises(NotImplementedError, match="use_graph=False"):
        tg.fit(ds, 2)
    torch.cuda.synchronize()
    assert tg.graph is None and torch.equal(before, m.flat_params())
    for a, t in zip(state, tr.pose_opt.state_tensors()):
        assert torch.equal(a, t.detach())


# ---- 5. the log -------------------------------------------------------------------------------------
class _HostReads:
    """Counts the calls that read the device from the host while it is active."""
    NAMES = ("item", "cpu", "tolist", "numpy", "__int__", "__float__", "__bool__", "__index__")

    def __init__(self):
        self.counts = {}

    def _wrap(self, owner, name):
        orig = getattr(owner, name)

        def counted(*a, **k):
            self.counts[name] = self.counts.get(name, 0) + 1
            return orig(*a, **k)

        own = name in vars(owner)  # (an inherited method is put back by removing the wrapper)
        setattr(owner, name, counted)
        return owner, name, orig if own else None

    def __enter__(self):
        self._saved = [self._wrap(torch.Tensor, n) for n in self.NAMES] + [self._wrap(torch.cuda, "synchronize")]
        return self

    def __exit__(self, *exc):
        for owner, name, orig in self._saved:
            if orig is None:
                delattr(owner, name)
            else:
                setattr(owner, name, orig)


def test_fit_log(dev):
    """fit(ds, 20, start_step=1000) on the captured step: 20 rows, steps 1000..1019, `total` the fp32
    sum of the term columns in the loss dict's order (exact: the loss node adds the same operands in
    that order), psnr = -10 log10(rgb), rm_s / vr_s the sample counts a second identical trainer
    returns from step_from, over 1024 rays.  With log_capacity=8 (drains after 8, 16 and at the end)
    the same rows come back: steps and marched counts exactly (they depend on the rays, the jitter and
    the bitfield only), the totals within the 1e-4 of two runs' losses.  The replayed steps of a fit
    read nothing from the device between drains: 20 more steps perform the three drains' .cpu() and
    no other host read."""
    scene = SyntheticScene()
    ds = _room_dataset(dev, RAYS)
    tr = _trainer(dev, scene)
    tr.status_interval = FAR
    log = tr.fit(ds, 20, start_step=1000)
    assert isinstance(log, TrainLog) and len(log) == 20
    assert log.steps.tolist() == list(range(1000, 1020))
    terms = ("rgb", "opacity", "norm_D_C_ort_dot", "norm_D_C_centr_dot", "norm_D_C_centr_L1")
    assert log.columns == ("step", "total") + terms + ("rm_samples", "vr_samples")
    acc = torch.zeros(20)
    for k in terms:
        acc = acc + log[k]
    assert torch.equal(log["total"], acc), (log["total"] - acc)
    assert bool((log["total"] > 0).all()) and bool((log["norm_D_C_centr_L1"] > 0).any())
    assert torch.equal(log["psnr"], -10.0 * torch.log10(log["rgb"])) and bool(torch.isfinite(log["psnr"]).all())
    # the counts of the same steps, read step by step from a second identical trainer
    t2 = _trainer(dev, scene)
    rm, vr = [], []
    for s in range(1000, 1020):
        res, _ = t2.step_from(ds, s)
        rm.append(int(res["rm_samples"]))
        vr.append(int(res["vr_samples"]))
    assert min(vr) > 0 and all(a >= b for a, b in zip(rm, vr))
    assert log["rm_s"].tolist() == [x / 1024 for x in rm]
    assert log["vr_s"].tolist() == [x / 1024 for x in vr]
    # a ring of 8 rows
    t3 = _trainer(dev, scene)
    t3.status_interval = FAR
    log8 = t3.fit(ds, 20, start_step=1000, log_capacity=8)
    assert t3._log_ring.shape[0] == 8 and len(log8) == 20
    assert log8.steps.tolist() == list(range(1000, 1020))
    assert torch.equal(log8["rm_samples"], log["rm_samples"])
    np.testing.assert_allclose(log8["total"].numpy(), log["total"].numpy(), rtol=1e-4)
    # 20 more steps, every one a replay
    with _HostReads() as reads:
        more = t3.fit(ds, 20, start_step=1020, log_capacity=8)
    assert reads.counts == {"cpu": 3}, reads.counts
    assert more.steps.tolist() == list(range(1020, 1040))


def test_fit_callback_runs_after_the_flush(dev):
    """callback(trainer, global_step) is called after the step `global_step` whenever
    (global_step + 1) % callback_every == 0, with the deferred optimizer step applied (fit's
    docstring): under defer_optimizer a step is pending after every graph, so the callback sees none
    pending and the device step counter at the number of steps trained."""
    ds = _room_dataset(dev, RAYS)
    tr = _trainer(dev, SyntheticScene(), defer_optimizer=True)
    assert "(global_step + 1) % callback_every == 0" in Trainer.fit.__doc__
    calls = []
    log = tr.fit(ds, 12, start_step=1003, callback_every=5,
                 callback=lambda t, s: calls.append((t is tr, s, t._pending, int(t.opt.step_dev))))
    assert calls == [(True, 1004, False, 2), (True, 1009, False, 7), (True, 1014, False, 12)]
    assert not tr._pending and int(tr.opt.step_dev) == 12 and len(log) == 12
    calls.clear()
    tr.fit(ds, 3, start_step=1015)  # callback_every = 0: never
    assert calls == []


# ---- 6. grid refresh inside fit -------------------------------------------------------------------
GRID_FLOOR_BYTES = 1  # differing bitfield bytes between two identical step() runs (see the docstring)


def test_fit_refreshes_the_grid(dev):
    """update_grid with a fixed grid_seed, steps 0..33 (refreshes at 0, 16 and 32): fit ends with the
    density bitfield of the step() loop fed ds.batch(s).  Two identical step() loops give the floor
    of differing bitfield bytes (a cell's density near the threshold can fall either side, as the
    parameters differ by the float atomics' summation order): measured on an MI355X, 1 of 262144
    bytes between the two step() loops (fit against the first: 0).  fit may differ by what the floor
    shows, the measured one or this run's, and no more."""
    scene = SyntheticScene()
    ds = _room_dataset(dev, RAYS)
    fields = []
    for run in ("a", "b", "fit"):
        tr = _trainer(dev, scene, update_grid=True)
        tr.grid_seed = lambda k: 1000 + k
        if run == "fit":
            log = tr.fit(ds, 34)
            assert log.steps.tolist() == list(range(34))
        else:
            for s in range(34):
                tr.step(_host_batch(ds, s), s)
        torch.cuda.synchronize()
        fields.append(tr.model.density_bitfield.clone())
    assert not torch.equal(fields[0], torch.from_numpy(scene.bitfield).to(dev))  # (the refreshes ran)
    floor = int((fields[1] != fields[0]).sum())
    got = int((fields[2] != fields[0]).sum())
    print(f"differing bitfield bytes of {fields[0].numel()}: step() vs step() {floor}, fit vs step() {got}")
    assert got <= max(floor, GRID_FLOOR_BYTES), (got, floor)
