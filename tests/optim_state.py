"""The optimizer's state (m, v, the clip factor) checked, not only the parameters.

With the reference's settings (eps 1e-15, weight decay 0 / 1e-6) the update m^ / (sqrt(v^) + eps)
does not depend on the gradient's scale and lr wd p is below the parameters' tolerance, so a wrong
clip factor, a forgotten grad_scale, a dropped weight decay or a moved group boundary all pass a
parameters-only comparison.  This module holds what tests/test_gpu_optim_state.py (on the device)
and tests/test_optim_state_host.py (on the CPU, with faults injected) share:

  bounds      `state_ratios` / `check_state`: p, m, v against the apex restatement
              (test_gpu_optim._apex_reference(return_state=True)):
                p   2e-6 |ref| + 1e-8                 the project's bound
                m   (2e-6 + E) s_m                    s_m = b1 s_m + (1 - b1) |g cf|: m cancels between
                                                      steps, its rounding error does not
                v   (4e-6 + 2 E) |ref|                v carries cf^2 and does not cancel
                E   1/2 (L + 24) 2^-24                first-order worst case of cf from the f32 sum of
                                                      squares: L = 4 ceil(n4 / (prep_blocks 1024)) + 3
                                                      fmas chained by one thread, 24 for the 10 + 4
                                                      levels of the workgroup sum, the sum of the
                                                      partials and sqrt / mul / add / div
              and m == v == 0 exactly where s_m == 0.
  probes      `probe_case` / `check_probe`: a gradient of K ones among zeros has the sum of squares
              K exactly in f32 in any order, and after one step from m = v = 0 every probe's m
              reports the clip factor the kernel used; one probe dropped or counted twice moves it
              by >= 1 / (2 K + 2).  `probe_indices` puts the probes at the boundaries of the prep
              launch (PREP_* below).
  inputs      `adamw_case` (test_adam_step_matches_torch_adamw's), `eps_grads`, `late_state`.
  mutants     `restatement`: _apex_reference's arithmetic with one fault injected (FAULTS).

A plain module: no fixture, marker or pytest setting; works on CPU tensors as on the device.
"""
import math
import types

import torch

LR, MAX_NORM, B1, B2, EPS, WD = 1e-2, 0.05, 0.9, 0.999, 1e-15, (0.0, 1e-6)
U = 2.0 ** -24  # unit roundoff of f32

# The geometry of adam_prep_kernel's launch as adam_step_impl derives it (csrc/optim.hip):
# prep_blocks = min(PREP_BLOCKS, cdiv(n / 4, 4 PREP_THREADS)) workgroups of PREP_THREADS threads, each
# thread PREP_UNROLL float4 per sweep at a stride of prep_blocks * PREP_THREADS float4, the n % 4 tail
# elements in workgroup 0.  A library built with other NCN_ADAM_BLOCKS / NCN_ADAM_UNROLL values leaves
# every test here valid (the expected values do not depend on them) but less aimed: the probes then
# sit beside the boundaries, not on them.
PREP_BLOCKS, PREP_THREADS, PREP_UNROLL = 256, 1024, 12
PROBES = 32

F32_ONE_MINUS_B1 = float(1 - torch.tensor(B1, dtype=torch.float32))  # the kernels' (1.f - b1)
F32_ONE_MINUS_B2 = float(1 - torch.tensor(B2, dtype=torch.float32))


def fig(name, value, bound):
    """The default figure printer (the device tests pass the guard-band module's _fig)."""
    print(f"OS-FIGURE {name} worst {value:.3e} bound {bound:.3e}")


# ================================================================================ geometry
def prep_geometry(n):
    """-> (n4, prep_blocks, stride): float4 count, workgroups, float4 stride between a thread's loads."""
    n4 = n // 4
    blocks = min(PREP_BLOCKS, max(1, -(-n4 // (4 * PREP_THREADS))))
    return n4, blocks, blocks * PREP_THREADS


def cf_error(n):
    """E: the first-order worst-case relative error of the clip factor (module docstring)."""
    n4, blocks, stride = prep_geometry(n)
    chain = 4 * -(-n4 // stride) + 3
    return 0.5 * (chain + 24) * U


def probe_indices(n, k=PROBES):
    """min(k, n) distinct element indices: first and last element of the buffer, of the float4 body,
    each tail element; first element, end of the first chunk and last element of workgroup 0, 1,
    PREP_BLOCKS - 1 and the last one; each side of the u = 1, PREP_UNROLL - 1, PREP_UNROLL boundaries
    (the last is the first element of the second sweep); filled up with evenly spaced elements."""
    n4, blocks, stride = prep_geometry(n)
    cand = [0, n - 1, 4 * n4 - 1] + list(range(4 * n4, n))
    if n4:
        q, r = divmod(n4 - 1, stride)  # the last float4 sits in row q (of stride float4), column r
        for wg in (0, 1, PREP_BLOCKS - 1, blocks - 1):
            first = wg * PREP_THREADS
            if wg >= blocks:
                continue
            last = q * stride + min(r, first + PREP_THREADS - 1) if r >= first else (q - 1) * stride + first + PREP_THREADS - 1
            cand += [4 * first, 4 * (first + PREP_THREADS - 1) + 3, 4 * last + 3]
    for u in (1, PREP_UNROLL - 1, PREP_UNROLL):
        cand += [4 * stride * u - 1, 4 * stride * u]
    want = min(k, n)
    cand += [(i * n) // (want + 1) for i in range(1, want + 1)] + list(range(min(n, 2 * want)))
    out = []
    for c in cand:
        if 0 <= c < n and c not in out and len(out) < want:
            out.append(c)
    assert len(out) == want, (n, len(out))
    return sorted(out)


# ================================================================================ bounds
def params_ratio(p, ref_p):
    """The parameters-only check of tests/test_gpu_optim.py: worst |err| / (2e-6 |ref| + 1e-8)."""
    return float(((p - ref_p).abs() / (2e-6 * ref_p.abs() + 1e-8)).max())


def _worst(err, bound):
    """max err / bound with 0 / 0 = 0 (and x / 0 = inf, NaN kept)."""
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()) if err.numel() else 0.0


def state_ratios(p, m, v, ref, n):
    """(p, m, v) of a run against ref = (p, m, v, s_m) of the restatement -> worst |err| / bound of
    each (module docstring), and the number of elements with s_m == 0 whose m or v is not 0."""
    rp, rm, rv, s_m = ref
    e = cf_error(n)
    live = s_m > 0
    return {
        "p": params_ratio(p, rp),
        "m": _worst((m.double() - rm.double()).abs()[live], (2e-6 + e) * s_m[live]),
        "v": _worst((v.double() - rv.double()).abs()[live], (4e-6 + 2 * e) * rv.double().abs()[live]),
        "dead": int((((m != 0) | (v != 0)) & ~live).sum()),
    }


def check_state(p, m, v, ref, n, tag, fig=fig):
    """Prints every worst ratio, then asserts it (a NaN fails)."""
    r = state_ratios(p, m, v, ref, n)
    for k in "pmv":
        fig(f"{tag}: {k} |err| / bound", r[k], 1.0)
    assert r["dead"] == 0, (tag, "m or v not exactly 0 where no gradient ever arrived", r["dead"])
    for k in "pmv":
        assert r[k] <= 1.0, (tag, k, r[k])
    return r


# ================================================================================ probes
def expected_cf(k, value, grad_scale, max_norm):
    """The clip factor times grad_scale of k entries `value` among zeros, in fp64."""
    clip = min(1.0, max_norm / (math.sqrt(k) * abs(value) * grad_scale + 1e-6)) if max_norm > 0 else 1.0
    return clip * grad_scale


def probe_case(n, device, value=1.0, grad_scale=0.5, max_norm=MAX_NORM):
    """value: a power of two (its square times K is then exact in f32 whatever the order)."""
    assert math.frexp(value)[0] == 0.5
    idx = torch.tensor(probe_indices(n), dtype=torch.int64, device=device)
    g = torch.zeros(n, device=device)
    g[idx] = value
    return types.SimpleNamespace(n=n, idx=idx, g=g, k=idx.numel(), value=value, grad_scale=grad_scale,
                                 max_norm=max_norm, cf=expected_cf(idx.numel(), value, grad_scale, max_norm))


CF_BOUND = 16 * U  # about 8 roundings in the kernel (sqrt, mul, add, div, mul; g cf, (1 - b1) .) and 8 here
V_BOUND = 2 * CF_BOUND + 4 * U  # v = ((1 - b2) gi) gi: cf twice, and two more products


def check_probe(case, p0, p, m, v, n0, wd, lr, tag, fig=fig):
    """After one step from m = v = 0 on case.g: every probe's m (and v) reports the expected clip
    factor; away from the probes m == v == 0 and p has moved by the weight-decay term only (one
    rounding of the result, half an ulp, plus the roundings of a term that is lr wd << 1 of it: one
    ulp in all; bitwise where wd == 0)."""
    idx, cf = case.idx, case.cf
    cf_m = m[idx].double() / (F32_ONE_MINUS_B1 * case.value)
    cf2_v = v[idx].double() / (F32_ONE_MINUS_B2 * case.value * case.value)
    r_m = float(((cf_m - cf).abs() / cf).max())
    r_v = float(((cf2_v - cf * cf).abs() / (cf * cf)).max())
    fig(f"{tag}: |cf(m) - cf| / cf", r_m, CF_BOUND)
    fig(f"{tag}: |cf^2(v) - cf^2| / cf^2", r_v, V_BOUND)
    away = torch.ones(case.n, dtype=torch.bool, device=p.device)
    away[idx] = False
    stray = int((((m != 0) | (v != 0)) & away).sum())
    wdv = torch.full((case.n,), float(wd[1]), dtype=torch.float64, device=p.device)
    wdv[:n0] = wd[0]
    want = p0.double() * (1 - lr * wdv)
    r_p = _worst((p.double() - want).abs()[away], (2 * U * p0.double().abs())[away])
    fig(f"{tag}: |p - p0 (1 - lr wd)| / (2^-23 |p0|), away from the probes", r_p, 1.0)
    kept = bool(torch.equal(p[away & (wdv == 0)], p0[away & (wdv == 0)]))
    assert r_m <= CF_BOUND, (tag, "clip factor seen in m", r_m, float(cf_m.min()), float(cf_m.max()), cf)
    assert r_v <= V_BOUND, (tag, "clip factor seen in v", r_v)
    assert stray == 0, (tag, "m or v non-zero away from the probes", stray)
    assert r_p <= 1.0 and kept, (tag, "p away from the probes moved by more than the weight decay", r_p, kept)
    return r_m, r_v, r_p


# ================================================================================ inputs
def adamw_case(n, gmag, steps, device):
    """The inputs of test_adam_step_matches_torch_adamw: -> (p0, [grads])."""
    g = torch.Generator(device=device).manual_seed(n)
    p0 = torch.randn(n, device=device, generator=g) * 0.1
    return p0, [torch.randn(n, device=device, generator=g) * gmag for _ in range(steps)]


EPS_VALUES = (0.0, 2.0 ** -50, -2.0 ** -47, 2.0 ** -44, -2.0 ** -40, 2.0 ** -30)


def eps_grads(n, steps, device, seed=5):
    """Gradients whose sqrt(v^) sits on either side of eps = 1e-15: every third entry exactly 0 on
    all steps (a hash-table entry no ray touched), the rest drawn from EPS_VALUES.  Unclipped (norm
    < 1e-6); the smallest non-zero v, (1 - b2) 2^-100 = 8e-34, is a normal f32."""
    g = torch.Generator(device=device).manual_seed(seed)
    vals = torch.tensor(EPS_VALUES, device=device)
    grads = []
    for _ in range(steps):
        gr = vals[torch.randint(0, len(EPS_VALUES), (n,), device=device, generator=g)]
        gr[::3] = 0.0
        grads.append(gr)
    return grads


def late_state(n, gmag, device, seed=7):
    """-> (p0, m0, v0, grad): moments of the (clipped) gradient's scale, v0 >= m0^2 as the moments
    of any gradient sequence are up to the bias corrections (Cauchy-Schwarz) — an update
    m^ / sqrt(v^) far above 1, which independent draws of m0 and v0 produce where v0 comes out
    near 0, multiplies the roundings of the quotient past the parameters' absolute bound of 1e-8."""
    g = torch.Generator(device=device).manual_seed(seed)
    p0 = torch.randn(n, device=device, generator=g) * 0.1
    m0 = torch.randn(n, device=device, generator=g) * (0.1 * gmag)
    v0 = m0.square() + (torch.randn(n, device=device, generator=g) * (0.1 * gmag)).square()
    return p0, m0, v0, torch.randn(n, device=device, generator=g) * gmag


# ================================================================================ mutants
FAULTS = ("norm_drop", "norm_double", "norm_unscaled", "cf_mul", "clip_when_off", "wd_drop", "n0_shift",
          "swap_groups", "eps", "bc_f32")


def restatement(p0, grads, n0, scale, lr, max_norm, wd=WD, b1=B1, b2=B2, eps=EPS, start_step=0, m0=None,
                v0=None, fault=None):
    """test_gpu_optim._apex_reference(return_state=True) with the faults of `fault` ({name: value})
    injected; without one, the same bits (tests/test_optim_state_host.py asserts it).
      norm_drop / norm_double: i   element i left out of / counted twice in the sum of squares
      norm_unscaled: True          the clip compares the norm of g, not of g grad_scale
      cf_mul: x                    the clip factor times x
      clip_when_off: True          max_norm <= 0 goes through the clip formula
      wd_drop: True                no weight decay;   swap_groups: True   wd0 and wd1 exchanged
      n0_shift: d                  the group boundary at n0 + d
      eps: x                       another eps (0.0: dropped)
      bc_f32: True                 bias corrections 1 - powf(beta_f32, step) in f32"""
    f = dict(fault or {})
    assert set(f) <= set(FAULTS), f
    if f.get("swap_groups"):
        wd = (wd[1], wd[0])
    if f.get("wd_drop"):
        wd = (0.0, 0.0)
    n0 = n0 + f.get("n0_shift", 0)
    eps = f.get("eps", eps)
    p = p0.clone()
    m = torch.zeros_like(p0) if m0 is None else m0.clone()
    v = torch.zeros_like(p0) if v0 is None else v0.clone()
    s_m = m.double().abs()
    wdv = torch.full_like(p0, wd[1])
    wdv[:n0] = wd[0]
    fb1, fb2 = torch.tensor(b1, dtype=torch.float32), torch.tensor(b2, dtype=torch.float32)
    for st, g in enumerate(grads, start_step + 1):
        gs = g * scale
        src = g if f.get("norm_unscaled") else gs
        norm = float(src.double().norm())
        if "norm_drop" in f:
            norm = math.sqrt(max(norm * norm - float(src[f["norm_drop"]]) ** 2, 0.0))
        if "norm_double" in f:
            norm = math.sqrt(norm * norm + float(src[f["norm_double"]]) ** 2)
        clip = min(1.0, max_norm / (norm + 1e-6)) if (max_norm > 0 or f.get("clip_when_off")) else 1.0
        gi = gs * (clip * f["cf_mul"] if "cf_mul" in f else clip)
        m = fb1 * m + (1 - fb1) * gi
        v = fb2 * v + (1 - fb2) * gi * gi
        s_m = b1 * s_m + (1 - b1) * gi.double().abs()
        if f.get("bc_f32"):
            stf = torch.tensor(float(st), dtype=torch.float32)
            bc1, bc2 = float(1 - torch.pow(fb1, stf)), float(1 - torch.pow(fb2, stf))
        else:
            bc1, bc2 = 1 - b1 ** st, 1 - b2 ** st
        upd = (m / bc1) / (torch.sqrt(v / bc2) + eps) + wdv * p
        p = p - lr * upd
    return p, m, v, s_m
