"""The test-time renderer against an oracle of its loop (oracle/render_test_ref.py), above the pieces the
suite already pins (the test marcher bit-exact, the dense compositor at one shape, the two scans).

The chain that carries the result to a real model:
  oracle loop == the renderer run with the stub field            (C, D here; exact in every integer)
  stub run and real run differ only in the field call            (the field is pinned by its own tests)
  real unfused == real fused, host- and device-driven, bit for bit (E here, test_gpu_render_test.py)

The stub field (tests/render_test_cases.py) has the same bits in numpy and in torch on the device, and
no ray's transmittance comes near T_threshold (test_oracle_render_test.py::test_margin_condition), so
alive sets, iteration counts, N_samples schedules and sample counts are compared exactly.

  A  ncn_test_loop_next alone: the alive compaction (block ranges of one and two chunks) and the loop
     head (N_samples rule and its clamps, the budget stop at equality, the done latch, the resets)
  B  the compositor's three entries (dense, through offsets, A / NS from ctrl) at C = 1, 3, 6, 54:
     bit-identical to each other, the dense one against the oracle at the existing tolerance
  C  the device-driven loop (rendering._test_loop_device) with the stub as its field
  D  render(stub_model, test_time=True): heads off / on up to C = 54, both backgrounds, one and two cascades
  E  a real random-init NGPMT at small and degenerate ray sets: the three loop modes bit-identical

Float bound of C and D, per ray: |x - x64| <= c 2^-24 (n_r + 1) max(1, max|v|) against the oracle's
float64 companion (render_test_cases.bound_ratio); c = GPU_C = max(4, 4 ORACLE_C) = 4, ORACLE_C = 0.5
bounding what the fp32 oracle itself needs (0.309, measured on the CPU).  Each test prints the c it needs.
Measured on an MI355X: the HIP renderer needs c = 0.309 at most (render/*/scale 0.5), the oracle's own
figure; per case it needs what the oracle needs to two digits, but for esf 1/256 at scale 1.0 (0.085
against 0.069) and diag_budget (0.078 against 0.085).  The whole file runs in 5 s.
"""
import json
import types

import numpy as np
import pytest
import torch

import render_test_cases as rc
from oracle import vren_ref
from ncnerf_amd import _lib, ngp_mt, rendering, vren
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a copy: the shared cases are read-only)


# ---- A: ncn_test_loop_next ------------------------------------------------------------------------
def _loop_head(ctrl, total, na, n_rays, max_samples, min_samples):
    """rendering.py's loop head after one iteration, on the control block (include/ncnerf.h)."""
    if ctrl[3]:
        return list(ctrl), total
    total += ctrl[4]
    it, marched, samples = ctrl[6] + 1, ctrl[7] + ctrl[0] * ctrl[1], ctrl[2]
    if na == 0 or samples >= max_samples:
        return [0, ctrl[1], samples, 1, 0, 0, it, marched], total
    ns = max(min(n_rays // na, 64), min_samples)
    return [na, ns, samples + ns, 0, 0, 0, it, marched], total


# block_sum<256> + block_excl_sweep<256> over block ranges: A = 65537 gives ranges of 512, two chunks each
@pytest.mark.parametrize("dead", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("A", [1, 255, 256, 257, 65537])
def test_loop_next(dev, A, dead):
    rng = np.random.default_rng(A)
    rays = rng.permutation(3 * A)[:A].astype(np.int64)
    alive = rays.copy()
    alive[rng.random(A) < dead] = -1
    if dead == 0.25 and A == 1:
        alive[0] = -1
    kept = np.sort(alive[alive >= 0])
    na = len(kept)
    # (n_rays, max_samples, min_samples, samples so far, done): every branch of the loop head
    states = {"above_64": (100 * A + 3, 1024, 1, 10, 0), "below_min_1": (A // 2, 1024, 1, 10, 0),
              "below_min_4": (2 * A, 1024, 4, 12, 0), "between": (7 * A, 1024, 4, 12, 0),
              "at_budget": (3 * A, 40, 1, 40, 0), "one_below_budget": (3 * A, 40, 1, 39, 0),
              "done": (3 * A, 1024, 1, 99, 1)}
    for name, (n_rays, ms, mins, samples, done) in states.items():
        c0 = [0, 7, samples, 1, 0, 0, 5, 1234] if done else [A, 3, samples, 0, 17, 0, 2, 100]
        ctrl = torch.tensor(c0 + [-7], dtype=torch.int32, device=dev)
        total = torch.tensor([1000, -7], dtype=torch.int64, device=dev)
        nxt = torch.full((A + 1,), -7, dtype=torch.int64, device=dev)
        _lib.call("ncn_test_loop_next", T(alive, dev), nxt, A, ctrl, total, n_rays, ms, mins)
        want, want_total = _loop_head(c0, 1000, na, n_rays, ms, mins)
        assert ctrl.cpu().tolist() == want + [-7], (name, ctrl.cpu().tolist(), want)
        assert total.cpu().tolist() == [want_total, -7], name
        got = nxt.cpu().numpy()
        if done:
            assert (got == -7).all(), name  # a done loop has A = 0: nothing is compacted
        else:
            assert np.array_equal(np.sort(got[:na]), kept), name
            assert (got[na:] == -7).all(), name
    if dead < 1.0 and A > 1:  # the states do take different branches
        assert _loop_head([A, 3, 10, 0, 17, 0, 2, 100], 0, na, 100 * A + 3, 1024, 1)[0][1] == 64
        assert _loop_head([A, 3, 12, 0, 17, 0, 2, 100], 0, na, 2 * A, 1024, 4)[0][1] == 4
        assert 4 < _loop_head([A, 3, 12, 0, 17, 0, 2, 100], 0, na, 7 * A, 1024, 4)[0][1] < 64
        assert _loop_head([A, 3, 10, 0, 17, 0, 2, 100], 0, na, A // 2, 1024, 1)[0][1] == 1


# ---- B: the compositor's three entries ------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 6, 54])
@pytest.mark.parametrize("A", [1, 257, 2000])
def test_composite_test_entries(dev, A, C):
    """test_gpu_vren.test_composite_test_parity's inputs at A rays and C channels, starting from non-zero
    opacity / depth / rend, one sample in twenty opaque (sigma 2^15: alpha = 1.0f, the ray stops there;
    every other T stays above 0.2, far from T_threshold)."""
    rng = np.random.default_rng(4)
    N, R, PAD = 8, A + A // 2 + 1, 300
    alive = np.sort(rng.choice(R, A, replace=False)).astype(np.int64)
    sig = np.abs(rng.normal(0, 50, (A, N))).astype(np.float32)
    sig[rng.random((A, N)) < 0.05] = rc.HIGH
    raws = rng.random((A, N, C), dtype=np.float32)
    deltas = np.full((A, N), 1.7e-3, np.float32)
    ts = rng.random((A, N), dtype=np.float32)
    n_eff = rng.integers(0, N + 1, A).astype(np.int32)
    n_eff[0] = N
    if A > 1:
        n_eff[1] = 0
    op = rng.random(R, dtype=np.float32) * 0.5
    de = rng.random(R, dtype=np.float32)
    re = rng.random((R, C), dtype=np.float32)
    # the compacted layout: ray n's n_eff[n] rows from offsets[n], the segments in a shuffled order
    order = rng.permutation(A)
    offsets = np.zeros(A, np.int32)
    offsets[order] = (np.cumsum(n_eff[order]) - n_eff[order]).astype(np.int32)
    total = int(n_eff.sum())
    sig_c = np.full(A * N + 1, np.nan, np.float32)  # (capacity-sized as the renderer's are; NaN past the total)
    raws_c = np.full((A * N + 1, C), np.nan, np.float32)
    for n in range(A):
        sig_c[offsets[n]:offsets[n] + n_eff[n]] = sig[n, :n_eff[n]]
        raws_c[offsets[n]:offsets[n] + n_eff[n]] = raws[n, :n_eff[n]]
    al_r, op_r, de_r, re_r = alive.copy(), op.copy(), de.copy(), re.copy()
    vren_ref.composite_test_multi_fw(sig, raws, deltas, ts, None, al_r, 1e-4, n_eff, op_r, de_r, re_r)
    assert A == 1 or ((al_r < 0) & (n_eff > 0)).any()  # rays stopped by T, not only for want of samples

    def run(entry):
        al = T(np.concatenate([alive, np.full(PAD, -7, np.int64)]), dev)
        ne = T(np.concatenate([n_eff, np.full(PAD, N, np.int32)]), dev)
        o, d, r = T(op, dev), T(de, dev), T(re, dev)
        ctrl = torch.tensor([A, N, N, 0, total, 0, 0, 0], dtype=torch.int32, device=dev)
        if entry == "dense":
            _lib.call("ncn_composite_test_fw", T(sig, dev), T(raws, dev), T(deltas, dev), T(ts, dev), al, A, N, C,
                      1e-4, ne, o, d, r)
        elif entry == "compact":
            _lib.call("ncn_composite_test_fw_compact", T(sig_c, dev), T(raws_c, dev), T(offsets, dev), T(deltas, dev),
                      T(ts, dev), al, A, N, C, 1e-4, ne, o, d, r)
        elif entry == "ctrl":  # what the device-driven loop launches: the (A, NS) layout, A / NS from ctrl
            _lib.call("ncn_test_loop_composite", T(sig, dev), T(raws, dev), None, T(deltas, dev), T(ts, dev), al,
                      A + PAD, ctrl, C, 1e-4, ne, o, d, r)
        else:  # A / NS from ctrl and sigmas / raws through offsets
            _lib.call("ncn_test_loop_composite", T(sig_c, dev), T(raws_c, dev), T(offsets, dev), T(deltas, dev),
                      T(ts, dev), al, A + PAD, ctrl, C, 1e-4, ne, o, d, r)
        assert ctrl.cpu().tolist() == [A, N, N, 0, total, 0, 0, 0]
        return [x.cpu().numpy() for x in (al, o, d, r)]

    dense = run("dense")
    assert np.array_equal(dense[0][:A], al_r) and (dense[0][A:] == -7).all()
    for got, want, name in zip(dense[1:], (op_r, de_r, re_r), ("opacity", "depth", "rend")):
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=name)
    untouched = np.setdiff1d(np.arange(R), alive)
    assert np.array_equal(dense[1][untouched], op[untouched]) and np.array_equal(dense[3][untouched], re[untouched])
    for entry in ("compact", "ctrl", "ctrl_compact"):
        for got, want, name in zip(run(entry), dense, ("alive", "opacity", "depth", "rend")):
            assert np.array_equal(got, want), (entry, name)


# ---- C: the device-driven loop with the stub field ------------------------------------------------
def _grid(dev, scale, full=False):
    return types.SimpleNamespace(density_bitfield=T(rc.bitfield(scale, full), dev), cascades=rc.cascades(scale),
                                 scale=scale, grid_size=rc.G)


def _check_floats(ref, opacity, depth, rend, label):
    c = rc.needed_c(ref, opacity, depth, rend)
    print(f"{label}: needs c = {c:.3f} (allowed {rc.GPU_C})")
    assert c <= rc.GPU_C, (label, c)
    idle = ref["n_comp"] == 0  # nothing composited: exactly zero
    assert not opacity[idle].any() and not depth[idle].any() and not rend[idle].any()


@pytest.mark.parametrize("name", sorted(rc.LOOP_CASES))
def test_device_loop_against_oracle(dev, name):
    R, esf, ms, low_only, kind = rc.LOOP_CASES[name]
    ref = rc.loop_oracle(name, "retire")
    o, d, ht = rc.ray_set(kind, R)
    min_samples = 1 if esf == 0 else 4
    hist = []

    def field(xyzs, dirs, ctrl, idx, sig, rgb):
        hist.append(ctrl.clone())
        s, r = rc.stub_channels(torch, xyzs, dirs, 0.5, 3, low_only)
        sig.copy_(s)
        rgb.copy_(r)

    opacity, depth, rend = (torch.zeros(R, device=dev), torch.zeros(R, device=dev), torch.zeros(R, 3, device=dev))
    alive = torch.arange(R, device=dev)
    stats = {}
    total = rendering._test_loop_device(_grid(dev, 0.5, kind == "diag"), T(o, dev), T(d, dev), T(ht, dev), alive, esf,
                                        ms, min_samples, rc.T_THRESHOLD, opacity, depth, rend, stats, field=field)
    torch.cuda.synchronize()
    trace = ref["trace"]
    ctrl = stats["ctrl"]
    # the fused ending retires the rays of an all-invalid round instead of breaking: the same rounds run
    assert ctrl[6] == len(trace) == stats["iterations"]
    assert ctrl[7] == sum(A * NS for A, NS, _, _ in trace) == stats["samples_marched"]
    assert int(total) == ref["total_samples"]
    assert ctrl[:6] == [0, trace[-1][1], ref["samples"], 1, 0, 0]
    hist = [h.tolist() for h in hist]
    assert len(hist) == stats["launched_iterations"] >= len(trace)
    samples = 0
    for k, (A, NS, n_valid, _) in enumerate(trace):  # the control block every iteration ran on
        samples += NS
        assert hist[k][:5] == [A, NS, samples, 0, n_valid] and hist[k][6] == k, (k, hist[k])
    for h in hist[len(trace):]:  # iterations past the end launch empty
        assert h == ctrl
    last = stats["alive_last"].cpu().numpy()
    assert np.array_equal(np.sort(last[:len(ref["alive"])]), ref["alive"])
    if kind == "diag":  # the budget stop, at equality, with every ray alive
        assert ref["samples"] == ms and len(ref["alive"]) == R
    _check_floats(ref, opacity.cpu().numpy(), depth.cpu().numpy(), rend.cpu().numpy(), name)
    if kind == "miss":
        assert ref["total_samples"] == 0 and ctrl[6] == 1


# ---- D: render() with a stub model ----------------------------------------------------------------
class StubModel:
    """What render_rays_test needs of a model; no _field_fwd, so it takes the reference-structure path."""

    def __init__(self, dev, scale, head):
        self.n_rend, self.pred_norm, K, _ = rc.HEAD_CASES[head]
        self.pred_sem = K is not None
        g = _grid(dev, scale)
        self.density_bitfield, self.cascades, self.scale, self.grid_size = g.density_bitfield, g.cascades, scale, rc.G
        self.center = torch.zeros(1, 3, device=dev)
        self.half_size = torch.full((1, 3), float(scale), device=dev)

    def __call__(self, xyzs, dirs, **kwargs):
        sig, raws = rc.stub_channels(torch, xyzs, dirs, self.scale, self.n_rend)
        return {"sigmas": sig, "rgbs": raws[:, :3], "norms": raws[:, 3:6], "sems": raws[:, 6:]}


def _render_stub(dev, head, esf, scale, o, d):
    K, unit = rc.HEAD_CASES[head][2:]
    kw = dict(near_distance=rc.NEAR, max_samples=1024, test_time=True, exp_step_factor=esf, pred_norm_nn_norm=unit)
    if K is not None:
        kw["n_sem_cls"] = K
    with torch.no_grad():
        res = render(StubModel(dev, scale, head), T(o, dev), T(d, dev), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


@pytest.mark.parametrize("scale", rc.RENDER_SCALES)
@pytest.mark.parametrize("esf", rc.RENDER_ESF)
@pytest.mark.parametrize("head", sorted(rc.HEAD_CASES))
def test_render_stub_model_against_oracle(dev, head, esf, scale):
    n_rend, pred_norm, K, unit = rc.HEAD_CASES[head]
    ref = rc.render_oracle(head, esf, scale)
    o, d, _ = rc.ray_set("image", rc.RENDER_R, scale)
    res = _render_stub(dev, head, esf, scale, o, d)
    assert int(res["total_samples"]) == ref["total_samples"]
    assert set(res) == {"opacity", "depth", "rgb", "total_samples"} | ({"norm_nn"} if pred_norm else set()) | (
        {"sem"} if K is not None else set())
    nc, u = ref["n_comp"], 2.0 ** -24
    bg = 1.0 if esf == 0 else 0.0
    need = [rc.bound_ratio(res["opacity"], ref["opacity64"], nc, 1.0),
            rc.bound_ratio(res["depth"], ref["depth64"], nc, ref["t_absmax"])]
    # rgb = rend + bg (1 - opacity), held to the same bound as every channel (the background adds opacity's
    # error, itself within the bound, and two roundings of values below 2)
    rgb64 = ref["rend64"][:, :3] + bg * (1.0 - ref["opacity64"])[:, None]
    need.append(rc.bound_ratio(res["rgb"], rgb64, nc, ref["raw_absmax"][:3]))
    if pred_norm and not unit:
        need.append(rc.bound_ratio(res["norm_nn"], ref["rend64"][:, 3:6], nc, ref["raw_absmax"][3:6]))
    if pred_norm and unit:
        # normalize(v): |d(v / |v|)| <= 2 |dv| / |v|, and three roundings of values below 1
        v = ref["rend64"][:, 3:6]
        n = np.linalg.norm(v, axis=1, keepdims=True)
        want = v / np.maximum(n, 1e-12)
        lim = 2 * rc.GPU_C * u * (nc + 1.0)[:, None] / np.maximum(n, 1e-12) + 3 * u
        assert (np.abs(res["norm_nn"] - want) <= lim).all()
        assert (np.abs(np.linalg.norm(res["norm_nn"][nc > 0], axis=1) - 1) < 1e-6).all()  # (stub norms = -d: |v| = opacity)
    if K is not None:
        assert res["sem"].shape == (rc.RENDER_R, K)
        need.append(rc.bound_ratio(res["sem"], ref["rend64"][:, 6:], nc, ref["raw_absmax"][6:]))
    print(f"render/{head}/esf{esf:g}/scale{scale}: needs c = {max(need):.3f} (allowed {rc.GPU_C})")
    assert max(need) <= rc.GPU_C, need
    # the integer side of every ray: a ray the oracle stopped is opaque here too (alpha = 1.0f of a HIGH sample)
    stopped = ref["opacity"] > 0.999
    assert np.array_equal(res["opacity"] > 0.999, stopped) and 0.3 < stopped.mean() < 0.95


@pytest.mark.parametrize("esf", rc.RENDER_ESF)
def test_render_stub_model_all_miss(dev, esf):
    """Rays that composite nothing: zeros, and rgb = the background (white at esf 0, else black; quirk q2)."""
    o, d, _ = rc.ray_set("miss", 1025)
    res = _render_stub(dev, "sem48", esf, 0.5, o, d)
    for k in ("opacity", "depth", "norm_nn", "sem"):
        assert not res[k].any(), k
    assert (res["rgb"] == (1.0 if esf == 0 else 0.0)).all() and res["rgb"].shape == (1025, 3)
    assert int(res["total_samples"]) == 0


# ---- E: a real model at small and degenerate ray sets ---------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    torch.manual_seed(0)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.density_bitfield.copy_(T(rc.scene().bitfield, dev))
        m.flat_params()[: m._n_table].mul_(3e4)  # densities of order 1: some rays stop, some march on
    return m


def _three_modes(m, o, d, esf, ms):
    outs = []
    for fused in (False, "host", True):
        st = {}
        with torch.no_grad():
            r = render(m, o, d, near_distance=0.01, max_samples=ms, test_time=True, test_fused=fused,
                       exp_step_factor=esf, loop_stats=st)
        torch.cuda.synchronize()
        outs.append((r, st))
    (a, sa) = outs[0]
    for b, sb in outs[1:]:
        for k in ("opacity", "depth", "rgb"):
            assert torch.equal(a[k], b[k]), k
        assert int(a["total_samples"]) == int(b["total_samples"])
        assert sa.get("iterations", 0) <= sb["iterations"] <= sa.get("iterations", 0) + 1, (sa, sb)
        json.dumps(sb)  # loop_stats stays plain numbers (tools write it out as JSON)
    return a, sa


@pytest.mark.parametrize("esf,ms", [(0.0, 1024), (0.0, 8), (1.0 / 256, 1024), (1.0 / 256, 8), (1.0 / 256, 2)])
@pytest.mark.parametrize("R", [1, 63, 257, 4097])
def test_three_modes_small_ray_sets(dev, model, R, esf, ms):
    """ms = 2 at esf > 0: max_samples below min_samples = 4, one round of 4 samples per ray."""
    o, d, _ = rc.ray_set("image", R)
    a, st = _three_modes(model, T(o, dev), T(d, dev), esf, ms)
    assert a["opacity"].shape == (R,) and a["rgb"].shape == (R, 3) and bool(torch.isfinite(a["rgb"]).all())
    if ms == 1024:
        assert int(a["total_samples"]) > R and float(a["opacity"].max()) > 0
    if ms == 2:
        assert st.get("iterations", 0) <= 1  # (0: a round that yields no sample is not counted)


@pytest.mark.parametrize("esf", [0.0, 1.0 / 256])
def test_three_modes_all_miss(dev, model, esf):
    o, d, _ = rc.ray_set("miss", 257)
    a, st = _three_modes(model, T(o, dev), T(d, dev), esf, 1024)
    assert int(a["total_samples"]) == 0 and not a["opacity"].any() and not a["depth"].any()
    assert bool((a["rgb"] == (1.0 if esf == 0 else 0.0)).all())


@pytest.mark.parametrize("fused", [False, "host", True])
def test_no_rays(dev, model, fused, monkeypatch):
    """R = 0: every output is empty, and the loop calls no kernel entry point."""
    o = torch.zeros(0, 3, device=dev)
    with torch.no_grad():
        r = render(model, o, o.clone(), near_distance=0.01, max_samples=1024, test_time=True, test_fused=fused)
    assert r["opacity"].shape == (0,) and r["depth"].shape == (0,) and r["rgb"].shape == (0, 3)
    assert int(r["total_samples"]) == 0
    calls = []
    real = _lib.call
    count = lambda name, *a: (calls.append(name), real(name, *a))[1]  # noqa: E731
    monkeypatch.setattr(_lib, "call", count)
    monkeypatch.setattr(vren, "call", count)
    monkeypatch.setattr(ngp_mt, "call", count)  # (the weight packing of the fused modes)
    with torch.no_grad():
        r = rendering.render_rays_test(model, o, o.clone(), torch.zeros(0, 1, 2, device=dev), max_samples=1024,
                                       test_time=True, test_fused=fused)
    assert calls == [] and r["rgb"].shape == (0, 3)
