"""The oracle of the test-time render loop (oracle/render_test_ref.py) pinned on the CPU before the GPU
tests (tests/test_gpu_render_test_oracle.py) rely on it, with the stub field and the cases of
tests/render_test_cases.py:

  (a) chunk independence: the loop equals "march every ray once with N_samples = max_samples, then
      composite each ray's samples in the chunks the trace gave it", bit for bit (the marcher resumes
      from hits_t exactly; a ray's result does not depend on its place in the alive list or on the
      other rays).  One composite call over the whole ray is NOT bit-identical to the loop and is not
      asked to be: the loop restarts T = 1 - opacity at every chunk where one call keeps the running
      product; it is held to the float bound below instead.
  (b) the trace obeys the loop head (A = the rays the last round kept, N_samples = max(min(R // A, 64),
      min_samples)) and `samples` stops at the first value >= max_samples: at equality, with every ray
      alive, in the two diag cases.
  (c) an all-miss ray set returns zeros plus the background under both endings.
  (d) the margin condition: for every case the GPU tests use, no ray's float64 transmittance comes
      within 1e-2 (relative) of T_threshold at any composited sample.  No ray is excluded.  This is
      what makes the alive sets, iteration counts and sample counts of an fp32 compositor exact.
  (e) the constant of the float bound |x - x64| <= c 2^-24 (n_r + 1) max(1, max|v|): the smallest c the
      fp32 oracle needs against its float64 companion is measured and must not exceed
      render_test_cases.ORACLE_C (nor fall below half of it: the constant stays a measurement).
      Measured: 0.309 (render/*/scale0.5; the loop cases need 0.30 or less).

CPU time of the oracle per case (one core, seconds; either ending, the run itself without the scene):
  loop cases     r1 0.016   r63_exp_ms16 0.001   r257 0.013   r1025_ms64 0.003   r1025_exp 0.017
                 r1025_miss 0.000   diag_budget 0.016   diag_budget_exp 0.005
  render cases   513 rays, (esf 0, esf 1/256) at scale 0.5 / at scale 1.0:
                 rgb (0.017, 0.019) / (0.093, 0.034)     norm and norm_unit (0.026, 0.018) / (0.052, 0.035)
                 sem1 (0.023, 0.012) / (0.036, 0.024)    sem48 (0.029, 0.021) / (0.056, 0.038)
All 36 runs together: 0.9 s.  The tests themselves: test_chunk_independence marches every ray by max_samples
slots once more and takes 0.01 to 0.7 s per case; the test that runs first (test_chunk_independence[diag_budget])
also builds the synthetic scene and the oracle library's first call, 1.3 s here and up to 3 s on a slower core;
test_margin_condition 0.5 s; the whole file 5 s.
"""
import numpy as np
import pytest

import render_test_cases as rc
from oracle import vren_ref

LOOP = sorted(rc.LOOP_CASES)


def _min_samples(esf):
    return 1 if esf == 0 else 4


@pytest.mark.parametrize("name", LOOP)
def test_chunk_independence(name):
    R, esf, ms, low_only, kind = rc.LOOP_CASES[name]
    ref = rc.loop_oracle(name, "break")
    o, d, ht = rc.ray_set(kind, R)
    bf = rc.bitfield(0.5, kind == "diag")
    X, D, DL, TS, NE = vren_ref.raymarching_test(o, d, ht.copy(), np.arange(R, dtype=np.int64), bf, 1, 0.5, esf, rc.G,
                                                 ms, ms)
    field = rc.np_field(0.5, 3, low_only)
    op, de, re = np.zeros(R, np.float32), np.zeros(R, np.float32), np.zeros((R, 3), np.float32)
    used = np.zeros(R, np.int64)
    alive = np.arange(R, dtype=np.int64)
    for A, NS, n_valid, after in ref["trace"]:
        assert A == len(alive)
        slot = used[alive][:, None] + np.arange(NS)[None, :]
        n_eff = np.clip(NE[alive].astype(np.int64) - used[alive], 0, NS).astype(np.int32)
        ok = np.arange(NS)[None, :] < n_eff[:, None]
        slot = np.where(ok, slot, 0)
        take = lambda a: np.where(ok.reshape(ok.shape + (1,) * (a.ndim - 2)), a[alive[:, None], slot], 0).astype(np.float32)  # noqa: E731
        x, dd, dl, ts = take(X), take(D), take(DL), take(TS)
        assert int(n_eff.sum()) == n_valid
        sig, raws = field(x.reshape(-1, 3), dd.reshape(-1, 3))
        sig = np.where(ok, sig.reshape(A, NS), 0).astype(np.float32)
        raws = np.where(ok[..., None], raws.reshape(A, NS, 3), 0).astype(np.float32)
        if n_valid == 0:
            break
        al = alive.copy()
        vren_ref.composite_test_multi_fw(sig, raws, dl, ts, None, al, rc.T_THRESHOLD, n_eff, op, de, re)
        used[alive] += n_eff
        alive = al[al >= 0]
        assert np.array_equal(np.sort(alive), after)
    assert np.array_equal(op, ref["opacity"]) and np.array_equal(de, ref["depth"]) and np.array_equal(re, ref["rend"])
    # one composite call over each whole ray: the same image within the float bound (see (a) above)
    op1, de1, re1 = np.zeros(R, np.float32), np.zeros(R, np.float32), np.zeros((R, 3), np.float32)
    al = np.arange(R, dtype=np.int64)
    ok = np.arange(ms)[None, :] < NE[:, None]
    sig, raws = field(X.reshape(-1, 3), D.reshape(-1, 3))
    vren_ref.composite_test_multi_fw(np.where(ok, sig.reshape(R, ms), 0).astype(np.float32),
                                     np.where(ok[..., None], raws.reshape(R, ms, 3), 0).astype(np.float32), DL, TS,
                                     None, al, rc.T_THRESHOLD, NE, op1, de1, re1)
    if ref["samples"] < ms or kind == "diag":  # (the budget cut no ray short of its samples)
        assert rc.needed_c(ref, op1, de1, re1) <= rc.GPU_C
        stopped = ref["n_comp"] < NE  # the rays the compositor stopped: the same ones
        assert np.array_equal(al[NE > 0] < 0, stopped[NE > 0])


@pytest.mark.parametrize("name", LOOP)
def test_trace_obeys_the_loop_head(name):
    R, esf, ms, low_only, kind = rc.LOOP_CASES[name]
    for ending in ("break", "retire"):
        ref = rc.loop_oracle(name, ending)
        n_alive, samples, total = R, 0, 0
        for k, (A, NS, n_valid, after) in enumerate(ref["trace"]):
            assert samples < ms and n_alive > 0  # (the loop head let this round run)
            assert A == n_alive and NS == max(min(R // A, 64), _min_samples(esf))
            samples += NS
            total += n_valid
            assert 0 <= n_valid <= A * NS
            if n_valid == 0:  # the all-invalid round is the last one, under either ending
                assert k == len(ref["trace"]) - 1 and len(after) == (A if ending == "break" else 0)
            n_alive = len(after)
        assert samples == ref["samples"] and total == ref["total_samples"]
        assert int(ref["n_comp"].sum()) <= total  # (a stopped ray leaves marched samples uncomposited)
        # the loop ended for one of its three reasons
        last_invalid = bool(ref["trace"]) and ref["trace"][-1][2] == 0
        assert samples >= ms or n_alive == 0 or (ending == "break" and last_invalid)
        assert np.array_equal(ref["alive"], ref["trace"][-1][3])
    if kind == "diag":  # the budget: reached at equality, every ray still alive
        assert ref["samples"] == ms and len(ref["alive"]) == R and ref["total_samples"] == R * ms


@pytest.mark.parametrize("name", LOOP)
def test_endings_agree(name):
    a, b = rc.loop_oracle(name, "break"), rc.loop_oracle(name, "retire")
    for k in ("opacity", "depth", "rend", "rgb", "n_comp", "opacity64", "depth64", "rend64", "margin"):
        assert np.array_equal(a[k], b[k]), k
    assert a["total_samples"] == b["total_samples"] and len(a["trace"]) == len(b["trace"])
    for (A, NS, v, al), (A2, NS2, v2, al2) in zip(a["trace"][:-1], b["trace"][:-1]):
        assert (A, NS, v) == (A2, NS2, v2) and np.array_equal(al, al2)
    assert a["trace"][-1][:3] == b["trace"][-1][:3]


@pytest.mark.parametrize("esf", [0.0, 1.0 / 256])
@pytest.mark.parametrize("ending", ["break", "retire"])
def test_all_miss(esf, ending):
    ref = rc.oracle("miss", 1025, 0.5, esf, 1024, 6, False, ending)
    assert ref["total_samples"] == 0 and len(ref["trace"]) == 1 and ref["trace"][0][:3] == (1025, _min_samples(esf), 0)
    for k in ("opacity", "depth", "rend", "n_comp", "opacity64", "depth64", "rend64"):
        assert not ref[k].any(), k
    assert (ref["rgb"] == (1.0 if esf == 0 else 0.0)).all() and ref["rgb"].shape == (1025, 3)
    assert len(ref["alive"]) == (1025 if ending == "break" else 0)


def test_stub_is_the_same_in_torch():
    """The stub's numpy and torch statements give the same bits (CPU torch here; the GPU tests run the
    torch statement on the device)."""
    import torch
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (4096, 3)).astype(np.float32)
    x[:64] = np.float32([-0.453125, 0.1875, 0.125])  # on the thresholds
    d = rng.normal(size=(4096, 3)).astype(np.float32)
    for scale in (0.5, 1.0):
        for n_rend in (3, 6, 7, 54):
            for low in (False, True):
                s0, r0 = rc.stub_channels(np, x, d, scale, n_rend, low)
                s1, r1 = rc.stub_channels(torch, torch.from_numpy(x), torch.from_numpy(d), scale, n_rend, low)
                assert s0.dtype == r0.dtype == np.float32 and s1.dtype == r1.dtype == torch.float32
                assert np.array_equal(s0, s1.numpy()) and np.array_equal(r0, r1.numpy())
    assert set(np.unique(s0)) == {np.float32(0.25)} and len(np.unique(rc.stub_channels(np, x, d, 1.0, 3)[0])) == 3


def test_cases_exercise_the_loop():
    """What the cases are there for, on the oracle alone."""
    r = rc.loop_oracle("r1025_exp")
    stopped = (r["opacity"] > 0.999).mean()
    assert 0.5 < stopped < 0.9 and (r["n_comp"] > 64).any()  # rays that stop at a surface and rays that run out
    ns = [t[1] for t in r["trace"]]
    assert ns[0] == 4 and 64 in ns and any(4 < n < 64 for n in ns)  # the clamp and the values between
    r = rc.loop_oracle("r1")
    assert all(t[:2] == (1, 1) for t in r["trace"]) and len(r["trace"]) > 64
    r = rc.loop_oracle("r63_exp_ms16")
    assert [t[1] for t in r["trace"]] == [4, 4] and (r["n_comp"] == 0).any()
    for head in rc.HEAD_CASES:  # both cascades composited at scale 1.0
        r = rc.render_oracle(head, 1.0 / 256, 1.0)
        assert r["t_absmax"] > 0.6 and r["n_comp"].max() > 128


def test_margin_condition():
    """(d): a condition, not a measurement.  Cap on excluded rays: zero."""
    for label, ref in rc.all_oracles():
        comp = ref["n_comp"] > 0
        assert np.isinf(ref["margin"][~comp]).all()
        assert (ref["margin"][comp] >= 1e-2).all(), (label, float(ref["margin"][comp].min()))
        # and by construction far more: T stays above 8 T_threshold or drops to (nearly) zero
        assert (ref["margin"][comp] >= 0.99).all(), label


def test_oracle_c():
    worst = 0.0
    for label, ref in rc.all_oracles():
        c = rc.needed_c(ref, ref["opacity"], ref["depth"], ref["rend"])
        print(f"{label}: fp32 oracle against its float64 companion needs c = {c:.3f}")
        worst = max(worst, c)
    print(f"largest: {worst:.3f}; ORACLE_C = {rc.ORACLE_C}, GPU_C = {rc.GPU_C}")
    assert rc.ORACLE_C / 2 <= worst <= rc.ORACLE_C
    assert rc.GPU_C == max(4.0, 4.0 * rc.ORACLE_C)
