"""Trainer checkpoints on the device: state_dict / load_state_dict, save_checkpoint / load_checkpoint
and fit(checkpoint_every=, checkpoint_path=).

Set-up (restated from tests/test_gpu_fit.py): the 5-view 24x20 room dataset, patch 8, 1024 rays (128
for the pose test), the model of tests/test_gpu_graph.py, `status_interval` out of the way.  The
steps are 1005..1010 with update_grid on, so that the refresh at 1008 — whose seed comes from torch's
CPU generator — lies inside; the eager marcher's jitter comes from the device's generator.  A
trainer that loads is built with another model seed, another jitter seed and torch reseeded, so only
the checkpoint can make it continue the saved run.

Bounds.  A state round trip carries no arithmetic: bit for bit.  A continued run against the
uninterrupted one is held to what a second uninterrupted run is held to, the acceptance of
tests/test_gpu_fit.py::test_dataset_step_matches_host_batch_step unchanged (two identical runs
differ by the float atomics of the table-gradient flush): per-step losses within rtol 1e-4, at most
5e-5 n_table table entries moved by more than 1e-4, a fraction below 1e-3 moved by more than 1e-6,
the MLP weights' relative difference below 1e-3."""
import warnings

import numpy as np
import pytest
import torch

import data_ref
from ncnerf_amd import checkpoint
from ncnerf_amd.data import DeviceRayDataset
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene, make_cameras
from ncnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

V, H, W = 5, 20, 24
RAYS = 1024
K = 5
FAR = 10 ** 6 + 3  # a status_interval that no step of these tests is a multiple of
FIRST, N = 1005, 6  # steps 1005..1010
MODES = ["graph", "deferred", "eager"]
SEM_HPARAMS = dict(loss_sem_w=0.1, pred_sem=True, load_sem_gt=True)  # tests/test_gpu_heads_e2e.py


@pytest.fixture(scope="module")
def scene():
    return SyntheticScene()


def _room_dataset(dev, batch_size, views=V, **kw):
    """tests/test_gpu_fit.py::_room_dataset: cameras inside the synthetic room, 24x20 images."""
    images, _, directions = data_ref.small_scene(views, H, W, seed=6)
    poses = make_cameras(views, seed=2)
    return DeviceRayDataset(torch.from_numpy(images).to(dev), torch.from_numpy(poses).to(dev),
                            torch.from_numpy(directions).to(dev), (W, H), batch_size=batch_size, seed=21, **kw)


def _sem_dataset(dev):
    g = torch.Generator().manual_seed(4)
    return _room_dataset(dev, RAYS, semantics=torch.randint(0, K + 1, (V, H * W), generator=g).to(torch.uint8).to(dev))


def _model(dev, scene, seed=7, heads=False, grid_size=128):
    """tests/test_gpu_graph.py::_model (with heads: tests/test_gpu_heads_e2e.py::_model)."""
    torch.manual_seed(seed)
    kw = dict(pred_sem=True, n_sem_cls=K, pred_norm=True) if heads else {}
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=grid_size, **kw).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        if grid_size == 128:
            m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
        else:
            m.density_bitfield.fill_(255)
    return m


def _trainer(dev, scene, mode, seed=7, rng_seed=1234, torch_seed=99, heads=False, update_grid=True, **kw):
    """A trainer in `mode`; torch is seeded last (the model's construction and the Trainer's own
    jitter-seed draw consume the CPU generator)."""
    if heads:
        kw["hparams"] = SEM_HPARAMS
    tr = Trainer(_model(dev, scene, seed, heads), update_grid=update_grid, use_graph=mode != "eager",
                 defer_optimizer=mode == "deferred", **kw)
    tr._rng_seed = rng_seed
    tr.status_interval = FAR
    torch.manual_seed(torch_seed)
    return tr


def _other(dev, scene, mode, **kw):
    """A trainer that shares nothing with the saved one but its configuration."""
    return _trainer(dev, scene, mode, seed=8, rng_seed=999, torch_seed=5, **kw)


def _assert_same(a, b, where="state"):
    """Nested states equal: tensors by torch.equal (dtype and shape included), everything else by ==."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), where
        assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a.cpu(), b.cpu()), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _assert_same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, f"{where}[{i}]")
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def _render_view0(tr, ds):
    o, d, _ = ds.image_rays(0)
    with torch.no_grad():
        res = render(tr.model, o, d, **dict(tr.render_kwargs, test_time=True))
    return {k: res[k] for k in ("rgb", "depth", "opacity")}


def _accept(tag, losses, params, n_t):
    """The acceptance of test_dataset_step_matches_host_batch_step: runs [1:] against run 0."""
    for i in range(1, len(losses)):
        d = (params[i][:n_t] - params[0][:n_t]).abs()
        big, small = int((d > 1e-4).sum()), float((d > 1e-6).float().mean())
        rel_w = float((params[i][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm())
        print(f"{tag}: run {i} vs run 0: losses {losses[i]} - {losses[0]} = {losses[i] - losses[0]}; {big} table "
              f"entries moved by > 1e-4, a fraction {small:.2e} by > 1e-6, MLP weights rel. {rel_w:.2e}")
    for i in range(1, len(losses)):
        np.testing.assert_allclose(losses[i], losses[0], rtol=1e-4)
        d = (params[i][:n_t] - params[0][:n_t]).abs()
        assert int((d > 1e-4).sum()) <= 5e-5 * n_t, i
        assert float((d > 1e-6).float().mean()) < 1e-3, i
        assert float((params[i][n_t:] - params[0][n_t:]).norm() / params[0][n_t:].norm()) < 1e-3, i


def _round_trip(dev, scene, mode, heads=False, path=None):
    """Train A over the steps, snapshot it, load the snapshot (or its file) into an unrelated B."""
    ds = _sem_dataset(dev) if heads else _room_dataset(dev, RAYS)
    A = _trainer(dev, scene, mode, heads=heads)
    start = A.model.flat_params().clone()
    A.fit(ds, N, start_step=FIRST)
    B = _other(dev, scene, mode, heads=heads)
    assert not torch.equal(A.model.flat_params(), B.model.flat_params())
    if path is None:
        sd = A.state_dict()
        assert A._pending is False
        nxt = B.load_state_dict(sd)
    else:
        assert A.save_checkpoint(path) == str(path)
        sd = A.state_dict()
        nxt = B.load_checkpoint(path)
    assert nxt == FIRST + N == sd["next_step"]
    assert sd["optimizer"]["step_count"] == N and int(sd["optimizer"]["step_dev"]) == N
    assert not torch.equal(sd["model"]["flat"], start) and bool(sd["optimizer"]["v"].any())
    assert bool((sd["model"]["density_grid"] != 0).any())  # (the refresh at 1008 ran)
    assert sd["model"]["flat"].is_cuda and sd["model"]["flat"].data_ptr() != A.model.flat_params().data_ptr()
    _assert_same(B.state_dict(), sd)
    assert B._rng_seed == 1234 and B.opt.step_count == N and B._pending is False
    assert not bool(B.model.flat_grad().any())
    ra, rb = _render_view0(A, ds), _render_view0(B, ds)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert float(ra["opacity"].max()) > 0
    return A, B, sd


# ---- 1. state round trip ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_state_round_trip(dev, scene, mode):
    _round_trip(dev, scene, mode)


# ---- 2. file round trip -----------------------------------------------------------------------------
def test_file_round_trip(dev, scene, tmp_path):
    path = tmp_path / "c.pt"
    _round_trip(dev, scene, "graph", path=path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c.pt"]
    state = torch.load(path, weights_only=True)
    assert state["format"] == "ncnerf_amd.trainer" and state["version"] == 1 and state["next_step"] == 1011
    assert not state["model"]["flat"].is_cuda


# ---- 3. continuation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_continuation(dev, scene, mode, tmp_path):
    """(a), (b): fit over 1005..1010 uninterrupted.  (c): fit over 1005..1007 with checkpoint_every=3,
    then an unrelated trainer loads the file and fits 1008..1010.

    The occupancy threshold of these runs is lowered (density_tresh_decay 1e-3: 0.0059 instead of
    5.9), which makes the comparison well conditioned and checks no less.  With the default, the
    refresh at 1008 thresholds at min(mean, 5.9) = the mean density of the cells it sampled, and this
    model's densities lie in a narrow band around that mean (the table is U(-1e-2, 1e-2): sigma is
    close to 1 everywhere), so the low-bit differences two identical runs carry from the float atomics
    of steps 1005..1007 put a few cells on the other side; their samples then give table entries a
    gradient in one run and none in the other, and Adam moves such an entry by about lr.  Measured
    on an MI355X with the default threshold, deferred mode: (c) already differed from (a) by 3e-8 in
    the losses of steps 1006 and 1007, before anything was saved; 3 of 262144 bitfield bytes differed
    after the refresh; 356 table entries moved by more than 1e-4 (allowed: 575) and a fraction 3.1e-3
    by more than 1e-6 (allowed: 1e-3), while (b) against (a) in the same run and all six comparisons
    of another run, with no differing byte, gave fractions of 5e-7 .. 6e-5.  Under the low threshold
    every sampled cell is occupied by a wide margin and every other cell is empty, whatever the low
    bits; which cells are sampled still comes from the refresh's seed, i.e. from torch's CPU
    generator, so a load that did not restore it would occupy other cells.  The bounds are unchanged."""
    ds = _room_dataset(dev, RAYS)
    losses, params, bits = [], [], []
    hp = dict(hparams=dict(density_tresh_decay=1e-3))
    for run in "abc":
        tr = _trainer(dev, scene, mode, **hp)
        if run != "c":
            logs = [tr.fit(ds, N, start_step=FIRST)]
        else:
            path = tmp_path / "run_{step}.pt"
            logs = [tr.fit(ds, 3, start_step=FIRST, checkpoint_every=3, checkpoint_path=path)]
            assert sorted(p.name for p in tmp_path.iterdir()) == ["run_1008.pt"]  # (once: the end is a multiple)
            tr = _other(dev, scene, mode, **hp)
            nxt = tr.load_checkpoint(tmp_path / "run_1008.pt", ds)
            assert nxt == FIRST + 3
            logs.append(tr.fit(ds, 3, start_step=nxt))
            assert logs[0].steps.tolist() == [1005, 1006, 1007] and logs[1].steps.tolist() == [1008, 1009, 1010]
        torch.cuda.synchronize()
        assert tr.opt.step_count == N and int(tr.opt.step_dev) == N and not tr._pending
        losses.append(torch.cat([log["total"] for log in logs]).numpy())
        params.append(tr.model.flat_params().detach().clone())
        bits.append(tr.model.density_bitfield.clone())
        n_t = tr.model._n_table
    print(f"{mode}: differing bitfield bytes of {bits[0].numel()}: b vs a {int((bits[1] != bits[0]).sum())}, "
          f"c vs a {int((bits[2] != bits[0]).sum())}")
    assert not torch.equal(bits[0], torch.from_numpy(scene.bitfield).to(dev))  # (the refresh ran)
    _accept(mode, losses, params, n_t)


def test_fit_saves_every_k_steps_and_at_the_end(dev, scene, tmp_path):
    """fit over 1005..1008 with checkpoint_every=3: a save after 1007 (1008 steps counted from 0) and
    one at the end; with "{step}" a file each, named by next_step, without it one file, replaced."""
    ds = _room_dataset(dev, RAYS)
    tr = _trainer(dev, scene, "deferred", update_grid=False)
    before = tr.model.flat_params().clone()
    for bad in (dict(checkpoint_every=3), dict(checkpoint_every=-1, checkpoint_path=tmp_path / "x.pt")):
        with pytest.raises(ValueError, match="checkpoint_every"):
            tr.fit(ds, 4, start_step=FIRST, **bad)
    assert tr.graph is None and torch.equal(tr.model.flat_params(), before) and list(tmp_path.iterdir()) == []
    tr.fit(ds, 4, start_step=FIRST, checkpoint_every=3, checkpoint_path=tmp_path / "c_{step}.pt")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c_1008.pt", "c_1009.pt"]
    states = [checkpoint.load(tmp_path / f"c_{n}.pt") for n in (1008, 1009)]
    assert [s["next_step"] for s in states] == [1008, 1009]
    assert [s["optimizer"]["step_count"] for s in states] == [3, 4]  # (the pending step was flushed into each)
    assert [int(s["optimizer"]["step_dev"]) for s in states] == [3, 4]
    assert torch.equal(states[1]["model"]["flat"], tr.model.flat_params().cpu())
    assert not torch.equal(states[0]["model"]["flat"], states[1]["model"]["flat"])
    tr.fit(ds, 3, start_step=1009, checkpoint_every=2, checkpoint_path=tmp_path / "last.pt")  # saves after 1009, 1011
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c_1008.pt", "c_1009.pt", "last.pt"]
    assert checkpoint.load(tmp_path / "last.pt")["next_step"] == 1012
    tr.fit(ds, 2, start_step=1012)  # checkpoint_every = 0: nothing is written
    assert checkpoint.load(tmp_path / "last.pt")["next_step"] == 1012 and len(list(tmp_path.iterdir())) == 3


# ---- 4. load into a captured trainer ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "deferred"])
def test_load_into_a_captured_trainer(dev, scene, mode):
    ds = _room_dataset(dev, RAYS)
    tr = _trainer(dev, scene, mode, update_grid=False)
    tr.step_from(ds, 1000)  # (captures)
    sd = tr.state_dict()
    graph = tr.graph
    assert graph is not None

    def ptrs():
        m, o = tr.model, tr.opt
        return [t.data_ptr() for t in (m.flat_params(), o.m, o.v, o.step_dev, o.lr_dev, m.amp_state, m.density_grid,
                                       m.density_bitfield)]

    def two_steps():
        ls = [float(tr.step_from(ds, s)[1]["total"]) for s in (1001, 1002)]
        tr.flush_optimizer()
        torch.cuda.synchronize()
        return np.array(ls), tr.model.flat_params().detach().clone()

    before = ptrs()
    first = two_steps()
    assert tr.opt.step_count == 3 and int(tr.opt.step_dev) == 3
    if mode == "deferred":
        tr.step_from(ds, 1003)  # (leaves an optimizer step pending: the load must drop it)
        assert tr._pending
    assert tr.load_state_dict(sd) == 1001
    assert tr.graph is graph and ptrs() == before
    assert not tr._pending and tr.opt.step_count == 1 and int(tr.opt.step_dev) == 1
    assert torch.equal(tr.model.flat_params(), sd["model"]["flat"]) and torch.equal(tr.opt.m, sd["optimizer"]["m"])
    second = two_steps()
    assert tr.graph is graph and ptrs() == before
    assert tr.opt.step_count == 3 and int(tr.opt.step_dev) == 3
    assert not torch.equal(second[1], sd["model"]["flat"])
    _accept(mode, [first[0], second[0]], [first[1], second[1]], tr.model._n_table)
    # the captured step holds the jitter seed: a checkpoint of another seed is refused, nothing changes
    keep = tr.model.flat_params().clone()
    with pytest.raises(ValueError, match="rng_seed"):
        tr.load_state_dict(dict(sd, rng_seed=77))
    assert torch.equal(tr.model.flat_params(), keep) and tr.opt.step_count == 3


# ---- 5. pose state ----------------------------------------------------------------------------------------
def _pose_setup(dev, seed):
    """tests/test_gpu_fit.py::test_pose_refinement_eager's set-up: loss scale 1, full bitfield."""
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    m.amp_state[0] = 1.0
    m.density_bitfield.fill_(255)
    tr = Trainer(m, update_grid=False, use_graph=False)
    tr.status_interval = FAR
    return tr


def test_pose_state(dev):
    ds = _room_dataset(dev, 128, optimize_ext=True)
    rng = np.random.default_rng(8)
    ax = rng.normal(size=(V, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    with torch.no_grad():
        ds.dR.copy_(torch.from_numpy((0.02 * ax).astype(np.float32)).to(dev))
        ds.dT.copy_(torch.from_numpy(rng.uniform(-2e-3, 2e-3, size=(V, 3)).astype(np.float32)).to(dev))
    start = ds.dR.detach().clone()
    tr = _pose_setup(dev, 0)
    for s in (3000, 3001):
        tr.step_from(ds, s)
    sd = tr.state_dict(ds)
    assert float(sd["pose"]["t"]) == 2.0 and not torch.equal(sd["pose"]["dR"], start)
    assert bool(sd["pose"]["m"][0].any()) and bool(sd["pose"]["v"][1].any())
    assert sd["dataset_signature"]["n_images"] == V and sd["next_step"] == 3002
    # into a new trainer and a new dataset
    ds2 = _room_dataset(dev, 128, optimize_ext=True)
    tr2 = _pose_setup(dev, 1)
    ptr = (ds2.dR.data_ptr(), ds2.dT.data_ptr())
    assert tr2.load_state_dict(sd, ds2) == 3002
    assert (ds2.dR.data_ptr(), ds2.dT.data_ptr()) == ptr and isinstance(ds2.dR, torch.nn.Parameter)
    assert torch.equal(ds2.dR.detach(), ds.dR.detach()) and torch.equal(ds2.dT.detach(), ds.dT.detach())
    for a, b in zip(tr.pose_opt.m + tr.pose_opt.v + [tr.pose_opt.t], tr2.pose_opt.m + tr2.pose_opt.v + [tr2.pose_opt.t]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert tr2.pose_opt.params[0] is ds2.dR and float(tr2.pose_opt.t) == 2.0
    _assert_same(tr2.state_dict(ds2), sd)
    tr2.step_from(ds2, 3002)
    assert float(tr2.pose_opt.t) == 3.0 and not torch.equal(ds2.dR.detach(), sd["pose"]["dR"])
    # without the dataset, or with another one: refused, nothing changes
    tr3 = _pose_setup(dev, 2)
    before = tr3.model.flat_params().clone()
    ds4 = _room_dataset(dev, 128, views=4, optimize_ext=True)
    with pytest.raises(ValueError, match="optimize_ext"):
        tr3.load_state_dict(sd)
    with pytest.raises(ValueError, match="optimize_ext"):
        tr3.load_state_dict(sd, _room_dataset(dev, 128))
    with pytest.raises(ValueError, match="n_images: saved 5, current 4"):
        tr3.load_state_dict(sd, ds4)
    assert torch.equal(tr3.model.flat_params(), before) and tr3.opt.step_count == 0 and int(tr3.opt.step_dev) == 0
    assert not bool(ds4.dR.any()) and not bool(tr3.opt.m.any())


# ---- 6. refusals change nothing -----------------------------------------------------------------------------
def test_refusals_change_nothing(dev, scene):
    ds = _room_dataset(dev, RAYS)
    tr = _trainer(dev, scene, "eager", update_grid=False)
    tr.step_from(ds, 1005)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (tr.model.flat_params(), tr.opt.m, tr.opt.v, tr.model.amp_state, tr.model.density_grid)]
    assert bool(keep[1].any())

    def refused(sd, field):
        with pytest.raises(ValueError, match=field):
            tr.load_state_dict(sd)
        now = (tr.model.flat_params(), tr.opt.m, tr.opt.v, tr.model.amp_state, tr.model.density_grid)
        assert all(torch.equal(a, b) for a, b in zip(keep, now))
        assert tr.opt.step_count == 1 and int(tr.opt.step_dev) == 1 and tr._next_step == 1006

    heads = Trainer(_model(dev, scene, heads=True), update_grid=False).state_dict()
    refused(heads, r"heads: saved \[\['sem_net', 5\], \['norm_net', 3\]\], current \[\]")
    small = Trainer(_model(dev, scene, grid_size=64), update_grid=False).state_dict()
    refused(small, "grid_size: saved 64, current 128")
    own = tr.state_dict()
    refused(dict(own, format="somebody.else"), "format")
    refused(dict(own, version=2), "version")
    refused(dict(own, optimizer=dict(own["optimizer"], m=own["optimizer"]["m"][:-1])), r"optimizer\.m")
    refused(dict(own, model={k: v for k, v in own["model"].items() if k != "amp_state"}), r"model\.amp_state")
    # differing hyper-parameters: a warning that lists them, and the trainer's own stay
    with pytest.warns(UserWarning, match="grad_clip: saved 0.5, current 0.05"):
        tr.load_state_dict(dict(own, hparams=dict(own["hparams"], grad_clip=0.5)))
    assert tr.h["grad_clip"] == 0.05 and tr.opt.max_norm == 0.05
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="hyper-parameters")
        tr.load_state_dict(own)


# ---- 7. heads on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_state_round_trip_with_heads(dev, scene, mode):
    A, B, sd = _round_trip(dev, scene, mode, heads=True)
    m = A.model
    assert sd["model_signature"]["heads"] == [("sem_net", K), ("norm_net", 3)]
    off = m._heads[0][2]
    assert sd["model"]["flat"].numel() == m.flat_params().numel() > off
    assert bool(sd["optimizer"]["v"][off:off + m._heads[0][3]].any())  # (the semantic head trained)


def test_reference_weights_round_trip_on_the_device(dev, scene):
    a, b = _model(dev, scene, seed=3, heads=True), _model(dev, scene, seed=4, heads=True)
    with torch.no_grad():
        a.density_grid.uniform_(0, 1)
    ptr = b.flat_params().data_ptr()
    sd = checkpoint.reference_state_dict(a)
    assert all(not t.is_cuda for t in sd.values()) and "model.sem_net.params" in sd and "model.amp_state" not in sd
    loaded, ignored = checkpoint.load_reference_state_dict(b, sd)
    assert ignored == [] and len(loaded) == len(sd)
    assert torch.equal(a.flat_params(), b.flat_params()) and b.flat_params().data_ptr() == ptr
    assert torch.equal(a.density_grid, b.density_grid) and torch.equal(a.density_bitfield, b.density_bitfield)
    assert b.xyz_encoder.params.data_ptr() == ptr and b._packed_fresh is False
    assert b.norm_net.params.data_ptr() == b.flat_params()[b._heads[1][2]:].data_ptr()
