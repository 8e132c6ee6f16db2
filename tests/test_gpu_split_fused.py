"""The split step's fused loss node (ncn_split_loss_fused, SplitStep(fused=True)) against the
separate entry points it replaces in the step, on identical inputs.

Nothing here has a tolerance of its own: launch 1 runs the compositor backward's own row code with
the dL/dsigma terms compiled out, launch 2 runs the bodies of cluster_kernel and of the rgb pass of
field_bwd_kernel as two roles, so every output is compared bit for bit (torch.equal on the values,
under which -0 equals +0, or on the int32 view where a buffer is prefilled with NaN).  Only the whole
step's flat gradient is compared with the bounds test_gpu_split_step applies between the split and
the autograd step (rel. 1e-6: the table gradient's float-atomic flush order differs between any two
runs), and the captured Trainer steps with test_split_graph_step_matches_graph_step's."""
import ctypes

import pytest
import torch

from ncnerf_amd import _lib, split_step, vren
from ncnerf_amd.losses import N_OUT, _STD_OFFSETS, _cluster_workspace, kmeans_plan
from ncnerf_amd.ngp_mt import N_W, NGPMT, register_grid_buffers
from ncnerf_amd.split_step import SplitStep, _fused_loss
from ncnerf_amd.synthetic import SyntheticScene
from ncnerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

T_THR = 1e-4
W_OP = 1e-3
W_CL = (0.01, 0.02, 0.005)
SCHED = (1000.0, 1000.0)
_MODELS = {}


def _field(dev, precision):
    if precision not in _MODELS:
        g = torch.Generator(device=dev).manual_seed(5)
        m = NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev)
        with torch.no_grad():
            m.flat_params()[: m._n_table].uniform_(-0.3, 0.3, generator=g)
        if m.amp_state is not None:
            m.amp_state[0] = 4.0
        _MODELS[precision] = m
    return _MODELS[precision]


def _bits(t):
    return t.contiguous().view(torch.int32)


class Inputs:
    """One loss node's inputs: `counts[i]` samples in row i of rays_a (rows in the given order, ray
    ids permuted), n_dev = their sum, capacity n = n_dev + pad; `opaque` = {row: sample} makes that
    row's transmittance fall under T_THR at that sample."""

    def __init__(self, dev, precision, counts, opaque=(), pad=37, seed=0, bad_gt=False):
        g = torch.Generator(device=dev).manual_seed(1000 + seed)
        R = len(counts)
        assert R % 64 == 0
        self.R, self.T = R, (R // 64) * 49
        n_dev = int(sum(counts))
        self.n = n = n_dev + pad
        self.m = m = _field(dev, precision)
        starts = torch.tensor([0] + list(counts[:-1]), dtype=torch.int64).cumsum(0)
        ray_ids = torch.randperm(R, generator=torch.Generator().manual_seed(seed))
        self.rays_a = torch.stack([ray_ids, starts, torch.tensor(counts, dtype=torch.int64)], 1).contiguous().to(dev)
        self.n_dev = torch.tensor([n_dev], dtype=torch.int32, device=dev)
        self.xyzs = (torch.rand(n, 3, device=dev, generator=g) - 0.5) * 0.99
        self.dirs = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
        self.deltas = torch.rand(n, device=dev, generator=g) * 0.01 + 0.002
        self.ts = torch.zeros(n, device=dev)
        sig = torch.rand(n, device=dev, generator=g) * 4.0
        for row, c in enumerate(counts):
            s0 = int(starts[row])
            self.ts[s0:s0 + c] = 0.1 + torch.cumsum(self.deltas[s0:s0 + c], 0)
        for row, k in dict(opaque).items():
            sig[int(starts[row]) + k] = 1e5
        self.sigmas = sig
        with torch.no_grad():
            _, self.rgbs, self.enc, self.packed, self.order = m._field_fwd(self.xyzs, self.dirs, self.n_dev, 0, True)
        self.total_s, self.opacity, self.depth, self.rend, self.ws, self.rgb = vren.composite_train_multi_fw(
            self.sigmas, self.rgbs, self.deltas, self.ts, self.rays_a, T_THR, bg=1.0)
        self.rgb_gt = torch.rand(R, 3, device=dev, generator=g)
        if bad_gt:
            self.rgb_gt[3, 1] = float("nan")
        self.rays_d = torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=1)
        pix = torch.arange(R, device=dev).view(-1, 64)
        self.x = [pix[:, torch.as_tensor(o, device=dev)].reshape(-1).contiguous() for o in _STD_OFFSETS]
        self.one = torch.ones((), device=dev)
        self.step = torch.tensor(1500, dtype=torch.int64, device=dev)
        self.dev = dev

    def _outs(self, K):
        dev, T, n = self.dev, self.T, self.n
        L = _lib.lib()
        o = dict(photo=torch.full((4,), -1.0, device=dev), normals=torch.full((T, 3), -2.0, device=dev),
                 cnt=torch.full((), -3, dtype=torch.int64, device=dev), draws=torch.zeros(n, 3, device=dev),
                 out=torch.full((N_OUT,), -4.0, device=dev), labels=torch.full((T,), -5, dtype=torch.int32, device=dev),
                 cents=torch.full((K, 3), -6.0, device=dev), dn=torch.full((3, T, 3), -7.0, device=dev),
                 slab=torch.full((256 * N_W,), float("nan"), device=dev),
                 dE=torch.full((int(L.ncn_field_bwd_dE_floats(n)),), 0.25, device=dev),
                 lmax=torch.full((16 * 256,), -1.0, device=dev),
                 stash=torch.full((int(L.ncn_field_bwd_stash_floats(n)),), 0.5, device=dev))
        return o

    def _status(self, K):
        off = int(_lib.lib().ncn_cluster_status_offset(K))
        return int(_cluster_workspace(self.dev, K).view(torch.int32)[off].item())

    def fused(self, K, nb):
        o = self._outs(K)
        _fused_loss(K, self.m._prec, nb, self.rgb, self.rgb_gt, self.opacity, self.R, W_OP, o["photo"], self.rays_d,
                    self.rays_d, self.depth, *self.x, self.T, o["normals"], self.total_s, None, o["cnt"], None, self.one,
                    self.sigmas, self.deltas, self.rays_a, T_THR, o["draws"], 20, kmeans_plan(self.dev, self.T, K),
                    0.9, W_CL, self.step, SCHED, o["out"], o["labels"], o["cents"], o["dn"],
                    _cluster_workspace(self.dev, K), self.xyzs, self.dirs, self.n, self.n_dev, self.order, self.packed,
                    self.enc, self.m._bwd_loss_scale(), o["slab"], o["dE"], o["lmax"], o["stash"])
        torch.cuda.synchronize()
        o["status"] = self._status(K)
        return o

    def separate(self, K, nb, zero_draws=False):
        """The forked step's calls: photo/normals/count forward, loss backward (rgb part), rgb-only
        compositor backward, ncn_cluster_loss, ncn_field_bwd_mlp_part part 1."""
        o = self._outs(K)
        call, R = _lib.call, self.R
        call("ncn_photo_normals_count_fwd", self.rgb, self.rgb_gt, self.opacity, R, W_OP, o["photo"], self.rays_d,
             self.rays_d, self.depth, *self.x, self.T, o["normals"], self.total_s, R, None, o["cnt"], None)
        drgb, dop = torch.empty_like(self.rgb), torch.empty_like(self.opacity)
        call("ncn_nerf_loss_bwd", self.rgb, self.rgb_gt, self.opacity, R, W_OP, o["photo"], self.rays_d, self.rays_d,
             self.depth, None, self.one, None, drgb, dop, None)
        dsig = torch.zeros(self.n, device=self.dev)
        call("ncn_composite_train_bw_bg", dop, None, drgb, None, self.sigmas, self.rgbs, self.ws, self.deltas, self.ts,
             self.rays_a, R, self.n, 3, self.opacity, self.depth, self.rend, T_THR, 1.0, dsig, o["draws"])
        call("ncn_cluster_loss", o["normals"], self.T, K, 20, kmeans_plan(self.dev, self.T, K), 0.9, *W_CL, None,
             self.step, *SCHED, o["photo"], o["out"], o["labels"], o["cents"], o["dn"], _cluster_workspace(self.dev, K))
        draws = torch.zeros_like(o["draws"]) if zero_draws else o["draws"]
        call("ncn_field_bwd_mlp_part", self.xyzs, self.dirs, self.n, self.n_dev, self.order, self.packed, self.m._prec,
             self.enc, None, None, draws, self.m._bwd_loss_scale(), 1, nb, o["slab"], o["dE"], o["lmax"], o["stash"])
        torch.cuda.synchronize()
        o["status"] = self._status(K)
        return o


FWD = ("photo", "normals", "cnt")
CLUSTER = ("out", "labels", "cents", "dn")
RGB_ROLE = ("slab", "stash", "lmax", "dE")  # dE: the POS_MASK word and the permuted positions; the rest untouched


def _same(a, b, keys):
    for k in keys:
        bitwise = a[k].is_floating_point() and k != "draws"  # (draws: by value, -0 equals +0)
        assert torch.equal(_bits(a[k]) if bitwise else a[k], _bits(b[k]) if bitwise else b[k]), k


def _draw_counts():
    """64 rows, the long rays first as the training step places them: every block shape of the
    compositor backward (1, 2 and 4 rows, the workgroup path up to 1024, the guarded rows beyond)."""
    counts = [1024, 700, 257, 300, 1100, 0, 1, 63, 64, 65, 128, 129, 256, 200, 90, 40]
    counts += [(7 * i) % 97 + 2 for i in range(64 - len(counts))]
    # stops: in a workgroup ray's second wave, past its first wave's rows, in the guarded loop's
    # second block, in the first row of a two-row ray, in a later row of a four-row ray
    opaque = {0: 300, 1: 20, 4: 400, 10: 10, 13: 150, 8: 63}
    return counts, opaque


def test_draws_equal_loss_and_compositor_backward(dev):
    counts, opaque = _draw_counts()
    assert {0, 1, 63, 64, 65, 128, 129, 256, 257, 700, 1024} <= set(counts)
    inp = Inputs(dev, "fp16", counts, opaque)
    nb = min(3, split_step.device_rgb_blocks())
    f, s = inp.fused(20, nb), inp.separate(20, nb)
    assert float(s["photo"][2]) == 1.0 and float(s["photo"][3]) == 1.0
    assert int((inp.total_s < torch.tensor(counts, device=dev)[inp.rays_a[:, 0].argsort()]).sum()) >= 3
    assert torch.equal(f["draws"], s["draws"])
    assert int((s["draws"] != 0).sum()) > 1000
    _same(f, s, FWD)
    _same(f, s, CLUSTER + RGB_ROLE)


def test_non_finite_photometric_loss_feeds_zeros(dev):
    counts, opaque = _draw_counts()
    inp = Inputs(dev, "fp16", counts, opaque, bad_gt=True)
    nb = min(3, split_step.device_rgb_blocks())
    f, s = inp.fused(20, nb), inp.separate(20, nb, zero_draws=True)
    assert float(s["photo"][2]) == 0.0 and float(s["photo"][0]) == 0.0 and float(s["photo"][3]) == 1.0
    _same(f, s, FWD + CLUSTER + RGB_ROLE)
    assert not torch.isnan(f["slab"][: nb * N_W]).all()


def _counts_for(R, n_dev):
    """R rows summing to n_dev, uneven, some of them empty."""
    if n_dev < R:
        return [1 if i < n_dev else 0 for i in range(R)]
    base = [(3 * i) % 5 for i in range(R)]  # weights 0..4: every fifth row is empty
    tot = sum(base)
    counts = [n_dev * b // tot for b in base]
    counts[1] += n_dev - sum(counts)
    return counts


@pytest.mark.parametrize("nb", [1, 3, 0])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("K", [10, 20])
def test_fused_launch_equals_separate_entry_points(dev, K, precision, nb):
    """R = 128 rays (98 triangles), enough samples for several steps of every workgroup of the
    device's grid (8 groups of 16 samples per step); nb = 0: the device's rgb grid."""
    nb = nb or split_step.device_rgb_blocks()
    n_dev = 3 * nb * 128 + 1000 if nb > 3 else 40 * 128 + 9
    inp = Inputs(dev, precision, _counts_for(128, n_dev), seed=K + nb)
    f, s = inp.fused(K, nb), inp.separate(K, nb)
    assert f["status"] == 0 and s["status"] == 0
    assert float(s["out"][3]) >= K  # enough valid normals: the clustering ran
    _same(f, s, FWD + CLUSTER + RGB_ROLE + ("draws",))
    rows = min(nb, int(_lib.lib().ncn_field_bwd_part_blocks(inp.n, 1)))
    written = ~torch.isnan(f["slab"]).view(-1, N_W)  # (the rgb pass writes the rgb_net tiles of its rows only)
    assert written[:rows].any(1).all() and not written[:rows].all(1).any() and not written[rows:].any()


@pytest.mark.parametrize("K,precision", [(20, "fp16"), (10, "bf16")])
@pytest.mark.parametrize("R,n_dev", [(128, 0), (128, 1), (128, 16 * 50 - 7), (704, 5000)])
def test_fused_launch_edge_shapes(dev, K, precision, R, n_dev):
    """No sample at all (device count 0), one, a count that ends inside a group of 16, and 539
    triangles: more than one 512-thread round of the clustering's compaction."""
    inp = Inputs(dev, precision, _counts_for(R, n_dev), seed=R + n_dev)
    for nb in (1, split_step.device_rgb_blocks()):
        f, s = inp.fused(K, nb), inp.separate(K, nb)
        assert f["status"] == 0 and s["status"] == 0
        _same(f, s, FWD + CLUSTER + RGB_ROLE + ("draws",))


def _model(dev, scene, precision="fp16"):
    torch.manual_seed(7)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev))
    with torch.no_grad():
        m.flat_params()[: m._n_table].uniform_(-1e-2, 1e-2)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    return m


def _batch(scene, dev, R, seed):
    b = scene.torch_batch(R, seed=seed, device=dev)
    b["march_noise"] = torch.rand(R, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return b


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_split_step_fused_equals_forked(dev, precision):
    scene = SyntheticScene()
    b = _batch(scene, dev, 2048, 31)
    step_dev = torch.tensor(1500, dtype=torch.int64, device=dev)
    runs = []
    for fused in (False, True):
        m = _model(dev, scene, precision)
        tr = Trainer(m, update_grid=False, use_graph=False)
        m.flat_grad().zero_()
        st = SplitStep(tr, fused=fused)
        assert st.fused == fused and st.cluster_capacity >= 16
        res, ld = st.run(b, step_dev)
        torch.cuda.synchronize()
        labels, cents, out = tr.loss.last_cluster
        runs.append(({k: v.clone() for k, v in ld.items()},
                     {k: res[k].clone() for k in ("rgb", "depth", "opacity", "ws", "total_samples", "vr_samples",
                                                  "rm_samples", "rays_a", "deltas", "ts")},
                     (labels.clone(), cents.clone(), out.clone(), tr.loss.last_normals.clone()), m.flat_grad().clone(),
                     m._n_table))
    (l0, r0, c0, g0, nt), (l1, r1, c1, g1, _) = runs
    for k in l0:
        assert torch.equal(_bits(l0[k]), _bits(l1[k])), k
    n_live = int(r0["rm_samples"])  # (per-sample arrays have the marcher's capacity: rows past the count are unwritten)
    for k in r0:
        per_sample = k in ("ws", "deltas", "ts")
        assert torch.equal(r0[k][:n_live] if per_sample else r0[k], r1[k][:n_live] if per_sample else r1[k]), k
    for a, c in zip(c0, c1):
        assert torch.equal(a, c)
    assert int(r0["vr_samples"]) > 0
    t0, t1 = g0[:nt], g1[:nt]
    assert torch.equal(t0 != 0, t1 != 0)
    rel_t = float((t1 - t0).norm() / t0.norm())
    rel_w = float((g1[nt:] - g0[nt:]).norm() / g0[nt:].norm())
    print("fused vs forked: rel table", rel_t, "rel weights", rel_w)
    assert rel_t < 1e-6 and rel_w < 1e-6, (rel_t, rel_w)


def test_fused_graph_steps_match_forked_graph_steps(dev):
    """Three captured Trainer steps in lockstep (both start every step from the same parameters and
    Adam state), fused against forked: bit-identical losses, parameters within the bounds of
    test_gpu_split_step.test_split_graph_step_matches_graph_step."""
    scene = SyntheticScene()
    batches = [_batch(scene, dev, 4096, 60 + k) for k in range(3)]
    trs = [Trainer(_model(dev, scene), update_grid=False, use_graph=True, split_backward=mode)
           for mode in ("forked", "fused")]
    nt = trs[0].model._n_table
    for k in range(3):
        ls = []
        for tr in trs:
            _, ld = tr.step(batches[k], global_step=1000 + 300 * k)
            tr.flush_optimizer()
            ls.append(float(ld["total"]))
        torch.cuda.synchronize()
        assert (trs[0]._split.fused, trs[1]._split.fused) == (False, True)
        assert ls[0] == ls[1], (k, ls)
        p0, p1 = trs[0].model.flat_params(), trs[1].model.flat_params()
        dt = (p1[:nt] - p0[:nt]).abs()
        frac, big = float((dt > 1e-6).float().mean()), int((dt > 1e-4).sum())
        rel_w = float((p1[nt:] - p0[nt:]).norm() / p0[nt:].norm())
        print(f"step {k}: entries apart >1e-6 {frac:.2e}, >1e-4 {big}; weights rel {rel_w:.2e}")
        assert frac < 1e-3 and big <= 5e-5 * nt and rel_w < 1e-3, (k, frac, big, rel_w)
        for a, b in zip(trs[0].opt.state_tensors(), trs[1].opt.state_tensors()):
            b.copy_(a)


def test_fused_refuses_a_grid_the_device_cannot_hold(dev, monkeypatch):
    """Every CU taken by the rgb role leaves none for the clustering's 16 workgroups: refused by
    count before anything is launched (the call with no rays is the check alone)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    prec = _field(dev, "fp16")._prec
    _fused_loss(20, prec, split_step.device_rgb_blocks())  # the step's own grid passes
    with pytest.raises(_lib.NcnError, match="cannot all be resident"):
        _fused_loss(20, prec, cus)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    tr = Trainer(m, update_grid=False, use_graph=True)
    monkeypatch.setattr(split_step, "device_rgb_blocks", lambda: cus)
    with pytest.raises(_lib.NcnError, match="cannot all be resident"):
        SplitStep(tr)
    cap = ctypes.c_int(0)
    assert _lib.lib().ncn_cluster_coresidency(20, 0, ctypes.byref(cap)) == 0  # (the device itself is fine)
