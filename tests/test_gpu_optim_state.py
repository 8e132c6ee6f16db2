"""ncn_adam_step's state — the clip factor, m, v — and what the reference's settings hide from a
parameters-only comparison (tests/optim_state.py has the bounds, the probe placement and the
inputs; tests/test_optim_state_host.py shows on the CPU that each check fails when it should).

  test_probe_norm*            every element counted once in adam_prep_kernel's sum of squares: K = 32
                              ones among zeros at the boundaries of the launch (buffer, float4 body,
                              tail, workgroups 0 / 1 / 255 / last, the u = 1 / 11 / 12 boundaries, the
                              second sweep), the clip factor read back from m and v after one step;
                              on a work buffer that another grid width has used; max_norm = 0; the
                              clip acting on the scaled norm.
                              Sizes: n = 4 * 4096 * 7 + 2 has n / 4 = 7 * 4096 exactly and so runs 7
                              full workgroups; 4 * 4096 * 7 + 6 is the one with 8, the last unit of
                              1024 float4 holding a single one.
  test_nonfinite_*            +-inf / NaN at the last tail element, the first element of the second
                              sweep and in workgroup 255 of n = 12 587 011, and a finite gradient whose
                              sum of squares overflows: the step is skipped.
  test_weight_decay_*         weight decay (0.5, 0.25): the decay and the group boundary (either side
                              of a float4, and inside the scalar tail) move p by 2.5e-3 |p| a step.
  test_eps_*                  gradients of 0 and 2^-50 ... 2^-30: sqrt(v^) on either side of eps.
  test_late_step              one step at step 1000, 2000 (with the GradScaler's growth) and 30000.

Measured on an MI355X: 39 cases, about 3 s for the file, the slowest case 0.7 s (the first, which
loads the library).  Worst figure of each bound over the cases of a test, as a share of the bound:
  probes (all 20 cases)   |cf(m) - cf| / cf 1.10e-7 of 16 u = 9.54e-7 (0.12; 0 where the clip is off)
                          |cf^2(v) - cf^2| / cf^2 1.87e-7 of 36 u = 2.15e-6 (0.09)
                          p away from the probes 0.499 of 2^-23 |p0|: the half ulp of the result's
                          one rounding, which is reached among 12.5 M elements; bitwise in group 0
                          m, v away from the probes: 0 non-zero
  non-finite (10 cases)   skipped, p / m / v bitwise, step 5, scale 32768, tracker 0, gradient
                          zeroed; 2 x 2^63 applied
  weight decay            p 0.46   m 0.10   v 0.10   (n0 70000 / 70001 / 70002: 0.42; 4099 / 4097: 0.46)
  eps                     p 0.40   m 0.03   v 0.04   the untouched entries bitwise
  late steps              p 0.11 / 0.09 / 0.14 at step 1000 / 2000 / 30000   m 0.04   v 0.02
  test_gpu_optim.py's     p 0.48 / 0.38 / 0.23 / 0.16   m 0.10 / 0.07 / 0.10 / 0   v 0.10 / 0.04 / 0.09 / 0
  four cases              (the 34 M case is one step: its m and v come out bit for bit)
Every test passed on its first run; no defect in csrc/optim.hip was found.
"""
import functools

import pytest
import torch

import guard_bands as gb
import optim_state as os_
from ncnerf_amd import _lib
from ncnerf_amd.optim import FlatAdam
from optim_state import B1, B2, EPS, LR, MAX_NORM
from test_gpu_guard_bands import _fig
from test_gpu_optim import _Flat, _apex_reference

pytestmark = pytest.mark.gpu

BIG = 12_587_011  # 12 * 256 * 1024 float4 + 1024 float4 + 3: the smallest size class with a second sweep
WIDE = 4 * 4096 * 300 + 1  # the 256-workgroup cap, one partial sweep
PROBE_WD = (0.0, 0.25)  # group 0 must keep p bitwise, group 1 moves by lr wd p


def _work(dev):
    return torch.zeros(int(_lib.lib().ncn_adam_step_work_floats()), device=dev)


def _adam_step(p, g, m, v, n0, step_dev, work, grad_scale=0.5, max_norm=MAX_NORM, wd=os_.WD, zero_grads=0, amp=None):
    _lib.call("ncn_adam_step", p, g, m, v, p.numel(), n0, grad_scale, max_norm, LR, B1, B2, EPS, wd[0], wd[1], None,
              step_dev, work, zero_grads, amp, None)


def _random_step(dev, n, work):
    """One step of a random gradient over n elements on `work` (buffers of its own)."""
    g = torch.Generator(device=dev).manual_seed(n)
    p, gr = (torch.randn(n, device=dev, generator=g) for _ in range(2))
    _adam_step(p, gr, torch.zeros_like(p), torch.zeros_like(p), n // 2, torch.zeros((), dtype=torch.int32, device=dev),
               work)


def _probe_run(dev, n, work=None, tag="", **case_kw):
    case = os_.probe_case(n, dev, **case_kw)
    p0 = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n)) * 0.1
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    step_dev = torch.zeros((), dtype=torch.int32, device=dev)
    _adam_step(p, case.g, m, v, n // 2, step_dev, _work(dev) if work is None else work, case.grad_scale,
               case.max_norm, PROBE_WD)
    torch.cuda.synchronize()
    assert int(step_dev) == 1
    os_.check_probe(case, p0, p, m, v, n // 2, PROBE_WD, LR, f"probe n {n}{tag}", fig=_fig)


# ================================================================================ 2. exact-norm probes
@pytest.mark.parametrize("n", [1, 3, 5, 4099, 4 * 4096 * 7 + 2, 4 * 4096 * 7 + 6, WIDE, BIG])
def test_probe_norm(dev, n):
    _probe_run(dev, n)


@pytest.mark.parametrize("n,n_before", [(4099, WIDE), (BIG, 4099)])
def test_probe_norm_on_a_used_work_buffer(dev, n, n_before):
    """The arrival counter and the partials another grid width left behind are in play."""
    work = _work(dev)
    _random_step(dev, n_before, work)
    _probe_run(dev, n, work, tag=f" after n {n_before}")


@pytest.mark.parametrize("n", [4099, BIG])
def test_probe_norm_without_clipping(dev, n):
    """max_norm = 0: cf == grad_scale."""
    _probe_run(dev, n, tag=" max_norm 0", max_norm=0.0)


# (value, grad_scale): sqrt(32) value is above 0.05 in all four; times grad_scale it is above (clipped)
# in the first, third and fourth and below (cf == grad_scale) in the second
SCALED_NORM_CASES = [(2.0 ** -6, 1.0), (2.0 ** -6, 0.25), (2.0 ** -4, 1.0), (2.0 ** -4, 0.25)]


@pytest.mark.parametrize("value,grad_scale", SCALED_NORM_CASES)
@pytest.mark.parametrize("n", [4099, BIG])
def test_probe_clip_acts_on_the_scaled_norm(dev, n, value, grad_scale):
    _probe_run(dev, n, tag=f" value {value} grad_scale {grad_scale}", value=value, grad_scale=grad_scale)


# ================================================================================ 3. non-finite detection
@functools.lru_cache(maxsize=None)
def _big_state(dev):
    """(p0, m0, v0, g0) at BIG: shared, never written."""
    g = torch.Generator(device=dev).manual_seed(3)
    p0 = torch.randn(BIG, device=dev, generator=g) * 0.1
    m0 = torch.randn(BIG, device=dev, generator=g) * 1e-3
    v0 = torch.rand(BIG, device=dev, generator=g) * 1e-6
    return p0, m0, v0, torch.randn(BIG, device=dev, generator=g) * 1e-3


def _amp_step(dev, grad):
    """One folded step of `grad` from _big_state with a GradScaler state of (65536, 7) at device step 5:
    -> (skipped and everything as the header states it, applied and everything as it states that)."""
    p0, m0, v0, _ = _big_state(dev)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    amp = torch.tensor([65536.0, 7.0], device=dev)
    step_dev = torch.full((), 5, dtype=torch.int32, device=dev)
    _adam_step(p, grad, m, v, BIG // 2, step_dev, _work(dev), zero_grads=1, amp=amp)
    torch.cuda.synchronize()
    assert int(grad.count_nonzero()) == 0  # consumed under the fold, skipped or not
    kept = [gb.same_bits(a, b) for a, b in ((p, p0), (m, m0), (v, v0))]
    skipped = all(kept) and int(step_dev) == 5 and amp.tolist() == [32768.0, 0.0]
    applied = not any(kept) and int(step_dev) == 6 and amp.tolist() == [65536.0, 8.0]
    return skipped, applied


_N4, _, _STRIDE = os_.prep_geometry(BIG)
NONFINITE_AT = {"last tail element": BIG - 1, "first element of the second sweep": 4 * os_.PREP_UNROLL * _STRIDE,
                "workgroup 255": 4 * (255 * os_.PREP_THREADS + 513) + 2}


@pytest.mark.parametrize("where", list(NONFINITE_AT))
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step(dev, bad, where):
    grad = _big_state(dev)[3].clone()
    grad[NONFINITE_AT[where]] = bad
    skipped, applied = _amp_step(dev, grad)
    assert skipped and not applied, (bad, where)


def test_nonfinite_norm_of_a_finite_gradient_skips_the_step(dev):
    """Two entries of 2^64: each square is 2^128, past f32 — "a gradient whose norm is not finite"
    (ncnerf.h).  Two of 2^63 (squares 2^126, sum 2^127) leave it finite: the step applies."""
    for value, want_skip in ((2.0 ** 64, True), (2.0 ** 63, False)):
        grad = _big_state(dev)[3].clone()
        grad[1000] = value
        grad[BIG - 2] = value
        skipped, applied = _amp_step(dev, grad)
        assert (skipped, applied) == (want_skip, not want_skip), value


# ================================================================================ 4. weight decay, the boundary
def _flat_adam_run(dev, p0, grads, n0, scale, wd, tag, start_step=0, m0=None, v0=None, amp=None):
    """FlatAdam over the gradients against the apex restatement: p, m, v within optim_state's bounds."""
    f = _Flat(p0.clone(), n0)
    if amp is not None:
        f.amp_state = amp
    opt = FlatAdam(f, lr=LR, max_norm=MAX_NORM, weight_decay=wd, zero_grad_on_step=True)
    opt.step_dev.fill_(start_step)
    opt.step_count = start_step
    if m0 is not None:
        opt.m.copy_(m0)
        opt.v.copy_(v0)
    for gr in grads:
        f.flat_grad().copy_(gr)
        opt.step(grad_scale=scale)
    torch.cuda.synchronize()
    assert int(opt.step_dev) == start_step + len(grads)
    ref = _apex_reference(p0, grads, n0, scale, LR, MAX_NORM, wd=wd, start_step=start_step, m0=m0, v0=v0,
                          return_state=True)
    got = (f.flat_params(), opt.m, opt.v)
    assert bool(torch.isfinite(torch.stack(got)).all()), tag
    os_.check_state(*got, ref, p0.numel(), tag, fig=_fig)
    return got


@pytest.mark.parametrize("n,n0", [(100003, 70001), (100003, 70000), (100003, 70002), (4099, 4097)])
def test_weight_decay_and_group_boundary(dev, n, n0):
    p0, grads = os_.adamw_case(n, 1e-2, 3, dev)
    _flat_adam_run(dev, p0, grads, n0, 0.5, (0.5, 0.25), f"weight decay n {n} n0 {n0}")


# ================================================================================ 5. eps, untouched entries
@pytest.mark.parametrize("wd", [(0.0, 1e-6), (0.0, 0.0)])
def test_eps_and_untouched_entries(dev, wd):
    n = 100003
    grads = os_.eps_grads(n, 3, dev)
    p0 = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(11)) * 0.1
    p, m, v = _flat_adam_run(dev, p0, grads, 70001, 1.0, wd, f"eps wd {wd}")
    assert not bool(m[::3].any()) and not bool(v[::3].any())  # (check_state's s_m == 0 rule, spelled out)
    if wd == (0.0, 0.0):
        gb.assert_same_bits(p[::3], p0[::3], "p of the entries no gradient reached", "moved without a gradient")


# ================================================================================ 6. late steps
@pytest.mark.parametrize("start_step", [999, 1999, 29999])
def test_late_step(dev, start_step):
    """The bias corrections where the reference trains; at 1999 with the GradScaler's tracker at 1999,
    so the 2000th finite step doubles the scale in the same launch."""
    p0, m0, v0, grad = os_.late_state(4099, 1e-2, dev)
    amp = torch.tensor([65536.0, 1999.0], device=dev) if start_step == 1999 else None
    _flat_adam_run(dev, p0, [grad], 1001, 0.5, os_.WD, f"late step {start_step + 1}", start_step, m0, v0, amp)
    if amp is not None:
        assert amp.tolist() == [131072.0, 0.0]
