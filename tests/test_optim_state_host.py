"""tests/optim_state.py catches a wrong optimizer — shown on the CPU with the apex restatement in
torch and one fault injected at a time (optim_state.restatement), through the functions the device
tests of tests/test_gpu_optim_state.py call; no wrong kernel runs on a GPU.  Also recorded: the
blind spot (the scale, weight-decay and eps faults pass the parameters-only check of
tests/test_gpu_optim.py on that test's own inputs), that the unmutated restatement is
_apex_reference bit for bit, and that a correct optimizer of another rounding (the same arithmetic
carried in fp64) sits well inside every bound.

The f32 powf bias corrections: at step 30000 they are below the bound (1 - 0.999^30000 is 1 - 9e-14:
both forms round to 1.0f, and the mutant's p, m and v are the reference's bit for bit); the mutant is
caught at step 1000, at 3.7 times the parameters' bound (test_late_step_mutant)."""
import pytest
import torch

import optim_state as os_
from optim_state import LR, MAX_NORM
from test_gpu_optim import _apex_reference

CPU = torch.device("cpu")
OLD = dict(n=100003, n0=70001, scale=0.5, gmag=1e-2, steps=3)  # test_adam_step_matches_torch_adamw's first case
WD_VISIBLE = (0.5, 0.25)


def _old_inputs():
    return os_.adamw_case(OLD["n"], OLD["gmag"], OLD["steps"], CPU)


def _fp64(p0, grads, *a, **kw):
    """The restatement's arithmetic carried in fp64 (f32 betas, as apex), rounded to f32 at the end."""
    kw = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    p, m, v, _ = os_.restatement(p0.double(), [g.double() for g in grads], *a, **kw)
    return p.float(), m.float(), v.float()


def test_restatement_is_the_reference():
    p0, grads = _old_inputs()
    p0l, m0, v0, gl = os_.late_state(4099, 1e-2, CPU)
    for a, kw in (((p0, grads, OLD["n0"], OLD["scale"], LR, MAX_NORM), {}),
                  ((p0, grads, OLD["n0"], 1.0, LR, 0.0), dict(wd=WD_VISIBLE)),
                  ((p0l, [gl], 1001, 0.5, LR, MAX_NORM), dict(start_step=999, m0=m0, v0=v0, eps=1e-8))):
        ref = _apex_reference(*a, return_state=True, **kw)
        for x, y in zip(os_.restatement(*a, **kw), ref):
            assert torch.equal(x, y)
        assert torch.equal(ref[0], _apex_reference(*a, **kw))


def test_probe_indices_sit_on_the_boundaries():
    big = 12_587_011
    n4, blocks, stride = os_.prep_geometry(big)
    assert (n4, blocks, stride) == (12 * 256 * 1024 + 1024, 256, 256 * 1024) and big - 4 * n4 == 3
    idx = os_.probe_indices(big)
    sweep2 = 4 * 12 * stride
    for want in (0, big - 1, big - 2, big - 3, 4 * n4 - 1, 4095, 4096, 4 * 255 * 1024, 4 * stride - 1, 4 * stride,
                 4 * 11 * stride - 1, 4 * 11 * stride, sweep2 - 1, sweep2):
        assert want in idx, want
    assert len(idx) == os_.PROBES == len(set(idx))
    assert os_.prep_geometry(4 * 4096 * 7 + 2)[1] == 7 and os_.prep_geometry(4 * 4096 * 7 + 6)[1] == 8
    assert os_.prep_geometry(4 * 4096 * 300 + 1)[1] == 256
    for n in (1, 3, 5):
        assert os_.probe_indices(n) == list(range(n))
    assert max(os_.probe_indices(4099)) == 4098 and os_.prep_geometry(4099)[1] == 1


# ---------------------------------------------------------------------------------- sections 1 and 4
def _state_run(fault, wd, n=OLD["n"], n0=OLD["n0"], fp64=False):
    p0, grads = os_.adamw_case(n, OLD["gmag"], OLD["steps"], CPU)
    a = (p0, grads, n0, OLD["scale"], LR, MAX_NORM)
    ref = _apex_reference(*a, wd=wd, return_state=True)
    got = _fp64(*a, wd=wd) if fp64 else os_.restatement(*a, wd=wd, fault=fault)[:3]
    return got, ref, n


@pytest.mark.parametrize("fault", [{"cf_mul": 3.0}, {"cf_mul": 0.5}, {"norm_unscaled": True}, {"wd_drop": True},
                                   {"eps": 0.0}], ids=str)
def test_blind_spot_of_the_parameters_only_check(fault):
    """The fault passes |p - ref| <= 2e-6 |ref| + 1e-8 on the old inputs with the reference's weight
    decay; the scale faults are caught there by the moments all the same."""
    got, ref, n = _state_run(fault, os_.WD)
    assert os_.params_ratio(got[0], ref[0]) < 1.0
    if "wd_drop" not in fault and "eps" not in fault:
        with pytest.raises(AssertionError):
            os_.check_state(*got, ref, n, str(fault))
        r = os_.state_ratios(*got, ref, n)
        assert r["m"] > 1e4 and r["v"] > 1e4, r


@pytest.mark.parametrize("n,n0", [(100003, 70001), (100003, 70000), (100003, 70002), (4099, 4097)])
def test_correct_runs_pass_the_state_check(n, n0):
    got, ref, _ = _state_run(None, WD_VISIBLE, n, n0)
    assert os_.check_state(*got, ref, n, "unmutated") == {"p": 0.0, "m": 0.0, "v": 0.0, "dead": 0}
    got, ref, _ = _state_run(None, WD_VISIBLE, n, n0, fp64=True)
    r = os_.check_state(*got, ref, n, "fp64 form")
    assert max(r["p"], r["m"], r["v"]) <= 0.5, r


@pytest.mark.parametrize("n,n0,fault", [
    (100003, 70001, {"wd_drop": True}), (100003, 70001, {"n0_shift": 1}), (100003, 70001, {"n0_shift": -1}),
    (100003, 70000, {"n0_shift": 1}), (100003, 70002, {"n0_shift": -1}), (100003, 70001, {"swap_groups": True}),
    (4099, 4097, {"n0_shift": 1}), (4099, 4097, {"n0_shift": -1}), (100003, 70001, {"cf_mul": 3.0}),
], ids=str)
def test_weight_decay_mutants(n, n0, fault):
    got, ref, _ = _state_run(fault, WD_VISIBLE, n, n0)
    with pytest.raises(AssertionError):
        os_.check_state(*got, ref, n, str(fault))


# ---------------------------------------------------------------------------------- section 2
def _probe_run(n, fault=None, **case_kw):
    case = os_.probe_case(n, CPU, **case_kw)
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.1
    n0, wd = n // 2, (0.0, 0.25)
    if fault is not None:  # the faults name a probe by its rank
        fault = {k: (int(case.idx[v]) if k in ("norm_drop", "norm_double") else v) for k, v in fault.items()}
    p, m, v, _ = os_.restatement(p0, [case.g], n0, case.grad_scale, LR, case.max_norm, wd=wd, fault=fault)
    return os_.check_probe(case, p0, p, m, v, n0, wd, LR, f"probe n {n} {case_kw} {fault}")


# (value, grad_scale): the scaled norm sqrt(32) value grad_scale on either side of 0.05, the unscaled
# one above it in all four
SCALED_NORM_CASES = [(2.0 ** -6, 1.0), (2.0 ** -6, 0.25), (2.0 ** -4, 1.0), (2.0 ** -4, 0.25)]


@pytest.mark.parametrize("n", [1, 3, 5, 4099, 4 * 4096 * 7 + 6])
def test_correct_runs_pass_the_probe_check(n):
    _probe_run(n)
    _probe_run(n, max_norm=0.0)
    for value, gs in SCALED_NORM_CASES:
        _probe_run(n, value=value, grad_scale=gs)


def test_scaled_norm_cases_straddle_the_clip():
    clipped = [os_.expected_cf(32, v, gs, MAX_NORM) < gs for v, gs in SCALED_NORM_CASES]
    assert clipped == [True, False, True, True]
    assert all(32 ** 0.5 * v > MAX_NORM for v, _ in SCALED_NORM_CASES)


@pytest.mark.parametrize("n,fault,case_kw", [
    (4099, {"norm_drop": 0}, {}), (4099, {"norm_drop": 31}, {}), (4099, {"norm_double": 17}, {}),
    (4 * 4096 * 7 + 6, {"norm_drop": 5}, {}), (4 * 4096 * 7 + 6, {"norm_double": 30}, {}),
    (4099, {"cf_mul": 3.0}, {}), (4099, {"norm_unscaled": True}, {}),
    (4099, {"norm_unscaled": True}, dict(value=2.0 ** -6, grad_scale=0.25)),
    (4099, {"norm_unscaled": True}, dict(value=2.0 ** -4, grad_scale=0.25)),
    (4099, {"clip_when_off": True}, dict(max_norm=0.0)),
    (4099, {"wd_drop": True}, {}), (4099, {"n0_shift": 1}, {}),
], ids=str)
def test_probe_mutants(n, fault, case_kw):
    with pytest.raises(AssertionError):
        _probe_run(n, fault, **case_kw)


def test_probe_check_sees_a_stray_moment():
    n = 4099
    case = os_.probe_case(n, CPU)
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1)) * 0.1
    p, m, v, _ = os_.restatement(p0, [case.g], n // 2, case.grad_scale, LR, case.max_norm, wd=(0.0, 0.25))
    os_.check_probe(case, p0, p, m, v, n // 2, (0.0, 0.25), LR, "clean")
    m[7] = 1e-30
    with pytest.raises(AssertionError, match="away from the probes"):
        os_.check_probe(case, p0, p, m, v, n // 2, (0.0, 0.25), LR, "stray m")


# ---------------------------------------------------------------------------------- section 5
def _eps_run(fault, wd=os_.WD, fp64=False):
    n, n0 = 100003, 70001
    grads = os_.eps_grads(n, 3, CPU)
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(11)) * 0.1
    a = (p0, grads, n0, 1.0, LR, MAX_NORM)
    ref = _apex_reference(*a, wd=wd, return_state=True)
    got = _fp64(*a, wd=wd) if fp64 else os_.restatement(*a, wd=wd, fault=fault)[:3]
    return got, ref, n, p0


def test_eps_inputs_and_correct_runs():
    grads = os_.eps_grads(100003, 3, CPU)
    norms = [float(g.double().norm()) for g in grads]
    assert max(norms) < 1e-6  # unclipped
    assert all(bool((g[::3] == 0).all()) for g in grads)
    assert sorted(set(torch.stack(grads).flatten().tolist())) == sorted(os_.EPS_VALUES)
    got, ref, n, p0 = _eps_run(None, wd=(0.0, 0.0))
    assert bool(torch.isfinite(torch.stack(ref[:3])).all())
    root = torch.sqrt(ref[2][ref[2] > 0] / (1 - os_.B2 ** 3))
    assert float(root.min()) < os_.EPS < float(root.max())  # sqrt(v^) on either side of eps
    assert float(ref[2][ref[2] > 0].min()) > 1.2e-38  # normal
    assert torch.equal(ref[0][::3], p0[::3]) and not bool(ref[1][::3].any()) and not bool(ref[2][::3].any())
    os_.check_state(*got, ref, n, "eps unmutated")
    got, ref, n, _ = _eps_run(None, fp64=True)
    r = os_.check_state(*got, ref, n, "eps fp64 form")
    assert max(r["p"], r["m"], r["v"]) <= 0.5, r


@pytest.mark.parametrize("fault", [{"eps": 0.0}, {"eps": 1e-8}, {"eps": 1e-14}], ids=str)
def test_eps_mutants(fault):
    got, ref, n, _ = _eps_run(fault)
    with pytest.raises(AssertionError):
        os_.check_state(*got, ref, n, str(fault))


def test_state_check_sees_a_moment_where_no_gradient_arrived():
    got, ref, n, _ = _eps_run(None)
    got[2][3] = 1e-38
    with pytest.raises(AssertionError, match="not exactly 0"):
        os_.check_state(*got, ref, n, "stray v")


# ---------------------------------------------------------------------------------- section 6
def _late_run(start_step, fault, fp64=False):
    n, n0 = 4099, 1001
    p0, m0, v0, g = os_.late_state(n, 1e-2, CPU)
    a = (p0, [g], n0, 0.5, LR, MAX_NORM)
    kw = dict(start_step=start_step, m0=m0, v0=v0)
    ref = _apex_reference(*a, return_state=True, **kw)
    got = _fp64(*a, **kw) if fp64 else os_.restatement(*a, fault=fault, **kw)[:3]
    return got, ref, n


@pytest.mark.parametrize("start_step", [999, 1999, 29999])
def test_late_steps_correct_runs(start_step):
    got, ref, n = _late_run(start_step, None)
    os_.check_state(*got, ref, n, f"late {start_step} unmutated")
    got, ref, n = _late_run(start_step, None, fp64=True)
    r = os_.check_state(*got, ref, n, f"late {start_step} fp64 form")
    assert max(r["p"], r["m"], r["v"]) <= 0.6, r


def test_late_step_mutant():
    """f32 powf bias corrections: caught at step 1000; invisible at 30000, where 1 - beta^step
    rounds to 1.0f in either form (module docstring)."""
    got, ref, n = _late_run(999, {"bc_f32": True})
    with pytest.raises(AssertionError):
        os_.check_state(*got, ref, n, "bc_f32 at 1000")
    got, ref, n = _late_run(29999, {"bc_f32": True})
    assert os_.state_ratios(*got, ref, n) == {"p": 0.0, "m": 0.0, "v": 0.0, "dead": 0}
