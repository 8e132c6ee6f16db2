"""Inputs of the test-time renderer's oracle tests, built once on the host and shared:
tests/test_oracle_render_test.py asserts on the oracle alone what the cases are there for (the margin
condition above all), tests/test_gpu_render_test_oracle.py runs the same arrays on the device.

The stub field.  The real field's fp16 arithmetic differs from any CPU restatement by more than the
compositor's rounding, which would flip `T <= T_threshold` decisions; the stub's values are the same
bits in numpy and in torch on the device:
  sigma   piecewise constant, chosen by comparisons of the position with thresholds that are exact
          in fp32: HIGH where x < -0.453125 and y > 0.1875 (deep in the wall image 1 looks at: 72 % of its
          rays stop there), else MID where z > 0.125, else LOW
  rgb     x * 0.5 / scale + 0.5        (scale a power of two: an exact product, then one rounded add,
  norms   -d                            which a contracted fma rounds the same way)
  sems_k  x[k % 3] * 2^-(1 + k // 3 % 3) / scale + (k % 11) / 8 - 0.5
Levels (scale s): LOW 0.25 / s and MID 2 / s bound a ray's optical depth by MID * (2 sqrt(3) s + one
step) < 7.1, so T stays above 8e-4 = 8 T_threshold until a HIGH sample; HIGH = 2^15 gives
sigma * delta >= 55 at the smallest step (sqrt(3) / 1024), so that sample's alpha is 1.0f and T drops to
0 (fp32) / below 1e-24 (f64).  No ray's T comes near T_threshold: |T / T_threshold - 1| >= 0.99 for every
composited sample, by construction and asserted (test_margin_condition).
"""
import functools
import time

import numpy as np

from oracle import render_test_ref, vren_ref

G = 128
HIGH = 32768.0
NEAR = 0.01
T_THRESHOLD = 1e-4


def stub_channels(xp, x, d, scale, n_rend, low_only=False):
    """(sigmas (S), raws (S, n_rend)) of the stub; xp is numpy or torch, x / d (S, 3) f32 of that library.
    n_rend = 3 (rgb), 6 (+ norms) or 6 + K (+ K sems)."""
    f = (lambda v: np.float32(v)) if xp is np else (lambda v: float(v))
    s = float(scale)
    lo = xp.full_like(x[:, 0], 0.25 / s)
    if low_only:
        sig = lo
    else:
        high = (x[:, 0] < f(-0.453125)) & (x[:, 1] > f(0.1875))
        mid = x[:, 2] > f(0.125)
        sig = xp.where(high, xp.full_like(lo, HIGH), xp.where(mid, xp.full_like(lo, 2.0 / s), lo))
    cols = [x[:, i] * f(0.5 / s) + f(0.5) for i in range(3)]
    if n_rend >= 6:
        cols += [-d[:, i] for i in range(3)]
    for k in range(max(n_rend - 6, 0)):
        cols.append(x[:, k % 3] * f(0.5 ** (1 + (k // 3) % 3) / s) + f((k % 11) / 8.0 - 0.5))
    assert len(cols) == n_rend
    return sig, xp.stack(cols, -1)


def np_field(scale, n_rend, low_only=False):
    return lambda x, d: stub_channels(np, x, d, scale, n_rend, low_only)


@functools.lru_cache(maxsize=None)
def scene():
    from ncnerf_amd.synthetic import SyntheticScene
    return SyntheticScene()


@functools.lru_cache(maxsize=None)
def ray_set(kind, R, scale=0.5):
    """R rays -> (o, d, hits_t (R, 2) with render()'s near clamp), read-only.
    "image": spread evenly over image 1 of the synthetic scene (the camera sits in the innermost cascade,
    0.1 to 0.26 from the room's wall it looks at: at scale 1.0 its rays go on through cascade 1).
    "miss": the same with every origin moved 6 half widths along its own direction: outside the box and
    looking away.
    "diag": from outside a corner along the box's diagonal, slightly spread: with an all-occupied bitfield
    the only rays that can yield max_samples samples (the diagonal is max_samples steps long), i.e. that
    reach the loop's sample budget."""
    if kind == "diag":
        rng = np.random.default_rng(R)
        o = (np.float32(-1.4 * scale) + rng.uniform(-0.004, 0.004, (R, 3)) * scale).astype(np.float32)
        tgt = 1.4 * scale + rng.uniform(-0.004, 0.004, (R, 3)) * scale
        d = tgt - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    else:
        ro, rd = scene().image_rays(1)
        step = ro.shape[0] // R
        o = np.ascontiguousarray(ro[::step][:R])
        d = np.ascontiguousarray(rd[::step][:R])
        if kind == "miss":
            o = (d * np.float32(6 * scale)).astype(np.float32)
    ht = hits(o, d, scale)
    miss = kind == "miss"
    assert o.shape == (R, 3) and (ht[:, 0] < 0).all() == miss and (miss or (ht[:, 0] >= 0).all())
    for a in (o, d, ht):
        a.setflags(write=False)
    return o, d, ht


def hits(o, d, scale):
    _, ht, _ = vren_ref.ray_aabb_intersect(o, d, np.zeros((1, 3), np.float32), np.full((1, 3), scale, np.float32), 1)
    ht = ht[:, 0].copy()
    near = (ht[:, 0] >= 0) & (ht[:, 0] < NEAR)  # rendering.py:28
    ht[near, 0] = NEAR
    return ht


@functools.lru_cache(maxsize=None)
def bitfield(scale, full=False):
    if full:
        return np.full(cascades(scale) * G ** 3 // 8, 255, np.uint8)
    if scale == 0.5:
        return scene().bitfield
    import scale_cases as sc
    return np.ascontiguousarray(sc.cascade_bitfield(sc.CASCADES[scale]))


def cascades(scale):
    return max(1 + int(np.ceil(np.log2(2 * scale))), 1)


# The device-driven loop's cases (test C): name -> (R, exp_step_factor, max_samples, low sigma everywhere,
# ray set).  Image 1's rays are at most 0.26 long, about 0.15 max_samples steps: none of them can reach the
# sample budget (r1025_ms64 ends, like the others, when its last rays leave the box, after the schedule
# N_samples = 1, 1, 1, 1, 3, 42).  The two diag cases (all-occupied bitfield, low sigma) are the ones that do:
# samples reaches max_samples exactly, with rays still alive.
LOOP_CASES = {
    "r1": (1, 0.0, 1024, False, "image"),
    "r63_exp_ms16": (63, 1.0 / 256, 16, False, "image"),
    "r257": (257, 0.0, 1024, False, "image"),
    "r1025_ms64": (1025, 0.0, 64, True, "image"),
    "r1025_exp": (1025, 1.0 / 256, 1024, False, "image"),
    "r1025_miss": (1025, 0.0, 1024, False, "miss"),
    "diag_budget": (65, 0.0, 64, True, "diag"),
    "diag_budget_exp": (65, 1.0 / 256, 64, True, "diag"),
}
# render() with the stub model (test D): name -> (n_rend, pred_norm, K or None, normalise norm_nn)
HEAD_CASES = {"rgb": (3, False, None, False), "norm": (6, True, None, False), "sem1": (7, True, 1, False),
              "sem48": (54, True, 48, False), "norm_unit": (6, True, None, True)}
RENDER_R = 513
RENDER_ESF = (0.0, 1.0 / 256)
RENDER_SCALES = (0.5, 1.0)
CPU_SECONDS = {}  # case key -> the oracle's time (filled as the cases are built)


@functools.lru_cache(maxsize=None)
def oracle(kind, R, scale, esf, max_samples, n_rend, low_only=False, ending="break"):
    """render_test_ref.render_test on ray_set(kind, R, scale) with the stub field; computed once, shared,
    never modified."""
    o, d, ht = ray_set(kind, R, scale)
    t0 = time.perf_counter()
    ref = render_test_ref.render_test(o, d, ht, bitfield(scale, kind == "diag"), cascades(scale), scale, esf, G,
                                      max_samples, np_field(scale, n_rend, low_only), n_rend, T_THRESHOLD, ending)
    CPU_SECONDS[(kind, R, scale, esf, max_samples, n_rend, low_only, ending)] = time.perf_counter() - t0
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def loop_oracle(name, ending="retire"):
    R, esf, ms, low_only, kind = LOOP_CASES[name]
    return oracle(kind, R, 0.5, esf, ms, 3, low_only, ending)


def render_oracle(head, esf, scale):
    return oracle("image", RENDER_R, scale, esf, 1024, HEAD_CASES[head][0], False, "break")


def all_oracles():
    """Every oracle run a GPU test compares with: [(label, result)]."""
    out = [(f"loop/{n}/{e}", loop_oracle(n, e)) for n in LOOP_CASES for e in ("retire", "break")]
    out += [(f"render/{h}/esf{esf:g}/scale{s}", render_oracle(h, esf, s))
            for h in HEAD_CASES for esf in RENDER_ESF for s in RENDER_SCALES]
    return out


# ---- the bound of the float comparisons -----------------------------------------------------------
# |x - x64| <= c * 2^-24 * (n_r + 1) * max(1, max|v|) per ray: n_r the ray's composited samples, v the
# values the channel composites (1 for opacity, ts for depth, raws[..., i] for rend[:, i]).  Every alpha
# carries an absolute error of a few 2^-24 (expf / __expf of a non-positive argument, one subtraction),
# so a ray's error grows with its sample count, not with its value.  ORACLE_C: the smallest c the fp32
# oracle itself needs against its float64 companion over all_oracles(), rounded up (measured by
# test_oracle_render_test.py::test_oracle_c, which fails if a case needs more); the HIP compositor
# (__expf, fmaf, the same association) gets four times that and at least 4.
ORACLE_C = 0.5
GPU_C = max(4.0, 4.0 * ORACLE_C)


def bound_ratio(got, ref64, n_comp, vmax):
    """max over rays (and channels) of |got - ref64| / (2^-24 (n_r + 1) max(1, vmax)): the c this needs."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    unit = 2.0 ** -24 * (n_comp + 1.0)
    if got.ndim == 2:
        unit = unit[:, None] * np.maximum(1.0, np.asarray(vmax, np.float64))[None, :]
    else:
        unit = unit * max(1.0, float(vmax))
    return float((np.abs(got - ref64) / unit).max()) if got.size else 0.0


def needed_c(res, opacity, depth, rend):
    """The c that (opacity, depth, rend) need against the oracle result's float64 companion."""
    return max(bound_ratio(opacity, res["opacity64"], res["n_comp"], 1.0),
               bound_ratio(depth, res["depth64"], res["n_comp"], res["t_absmax"]),
               bound_ratio(rend, res["rend64"], res["n_comp"], res["raw_absmax"]))
