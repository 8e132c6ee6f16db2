"""Inputs of the tests at scene scales above 0.5 (more than one cascade, other level tables), built
once on the host and shared: tests/test_scale_cases_host.py asserts on the oracle alone what each
case is there for, the GPU tests (test_gpu_field_scales.py, test_gpu_vren.py) run the same arrays.

Scales: 1.0 (C = 2, extent 2; level 5, res 81, is hashed inside the scatter's unit class 0),
1.5 (C = 3, extent 3: not a power of two), 16.0 (C = 6; level 9, res 1553, lies beyond the scatter's
cell-key range pz < 1023; the finest level has res 32768)."""
import functools

import numpy as np

from oracle import field_ref, vren_ref
from field_level_check import place_edges

CASCADES = {1.0: 2, 1.5: 3, 16.0: 6}  # max(1 + ceil(log2(2 scale)), 1), ngp_mt.py:34
N_FIELD = 4099  # two Morton windows, the second of three samples
G, MAX_SAMPLES = 128, 1024
SQRT3 = np.float32(1.73205080757)
NAMES = ("rays_a", "xyzs", "dirs", "deltas", "ts", "counter")


def edge_rays(rng, n):
    """Random rays plus the reference edge cases: misses, starts inside, axis-parallel (1/d = inf)."""
    o = rng.uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 8, 1:] = 0.0  # parallel to x
    d[n // 8: n // 4, 0] = 0.0  # in the yz plane
    o[n // 4: n // 3] = rng.uniform(-0.2, 0.2, (n // 3 - n // 4, 3))  # inside the box
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


@functools.lru_cache(maxsize=None)
def field_positions(scale, n=N_FIELD, seed=21):
    """(n, 3) f32 world positions: uniform in 0.999 of the box [-scale, scale]^3, with the edge set
    of field_level_check.place_edges for that box (corners, face centres, one ulp inside and outside
    each face, points outside, cell boundaries of levels 0, 5, 10, runs of 600 equal positions) at
    the start and across index 4096.  Read-only (shared)."""
    levels = field_ref.grid_levels(scale)[0]
    rng = np.random.default_rng(seed)
    fill = ((rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.999 * 2 * scale)).astype(np.float32)
    xw, mark = place_edges(fill, levels, scale)
    assert mark[0] and (n <= 4096 or (mark[4095] and mark[4096])) and (~mark).sum() >= n // 4
    xw.setflags(write=False)
    return xw


def x01_f32(xw, scale):
    """(x - xyz_min) / xyz_extent in f32, as the kernels form it."""
    mn, ext = np.float32(-scale), np.float32(scale) - np.float32(-scale)
    return ((np.asarray(xw, np.float32) - mn) / ext).astype(np.float32)


def level_cells(xw, scale, level):
    """The integer cell (n, 3) of each position on one level: floor(fma(scale_l, x01, 0.5))."""
    lv = field_ref.grid_levels(scale)[0][level]
    pos = (x01_f32(xw, scale).astype(np.float64) * np.float64(np.float32(lv["scale"])) + 0.5).astype(np.float32)
    return np.floor(pos).astype(np.int64)


# ---- marcher cases --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _room_bitfield():
    from ncnerf_amd.synthetic import bitfield_np, room_occupancy
    return bitfield_np(room_occupancy())


def cascade_bitfield(C):
    """A different occupancy pattern per cascade: the synthetic room's bitfield, rotated by 1000 c bytes."""
    bf = _room_bitfield()
    return np.concatenate([np.roll(bf, 1000 * c) for c in range(C)])


def march_rays(scale, n, seed, far):
    """n rays for the box [-scale, scale]^3: the first half edge_rays scaled to the box (origins
    within 1.8 half widths: misses, starts inside, axis-parallel), the rest ordinary rays from origins
    at a distance of far[0]..far[1] (world units) aimed at a point of the inner box.  -> (o, d, hits_t
    with render()'s near clamp (rendering.py:28), noise), f32."""
    rng = np.random.default_rng(seed)
    ne = n // 2
    o, d = edge_rays(rng, max(ne, 8))
    o, d = o[:ne] * np.float32(2 * scale), d[:ne]
    k = n - ne
    u = rng.normal(size=(k, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o2 = (u * rng.uniform(far[0], far[1], (k, 1))).astype(np.float32)
    tgt = rng.uniform(-0.8 * scale, 0.8 * scale, (k, 3))
    tgt[: k // 3] *= 0.25  # a third through the innermost cascade
    d2 = tgt - o2
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(np.float32)
    o, d = np.concatenate([o, o2]).astype(np.float32), np.concatenate([d, d2]).astype(np.float32)
    _, ht, _ = vren_ref.ray_aabb_intersect(o, d, np.zeros((1, 3), np.float32), np.full((1, 3), scale, np.float32), 1)
    ht = ht[:, 0].copy()
    near = (ht[:, 0] >= 0) & (ht[:, 0] < 0.01)
    ht[near, 0] = 0.01
    return o, d, ht, rng.random(n, dtype=np.float32)


# (name: scale, exp_step_factor, distance range of the ordinary rays' origins)
TRAIN_CASES = {"c2_const": (1.0, 0.0, (1.8, 4.0)), "c3_const": (1.5, 0.0, (2.7, 6.0)),
               "c3_exp": (1.5, 1.0 / 256, (2.7, 8.0))}
TRAIN_N = (2048, 777, 1)  # several workgroups; not a multiple of 64; a single ray


@functools.lru_cache(maxsize=None)
def train_case(name, n):
    """-> dict(scale, C, esf, o, d, ht, noise, bf, ref): ref = vren_ref.raymarching_train's outputs
    (computed once, shared, never modified)."""
    scale, esf, far = TRAIN_CASES[name]
    C = CASCADES[scale]
    o, d, ht, noise = march_rays(scale, n, 100 + n, far)
    if n == 1:  # the single ray: an ordinary one through the middle of the box
        o, d, ht, noise = (a[1:2].copy() for a in march_rays(scale, 2, 7, far))
    bf = cascade_bitfield(C)
    ref = vren_ref.raymarching_train(o, d, ht, bf, C, scale, esf, noise, G, MAX_SAMPLES)
    for a in (o, d, ht, noise, bf) + tuple(ref):
        a.setflags(write=False)
    return dict(scale=scale, C=C, esf=esf, o=o, d=d, ht=ht, noise=noise, bf=bf, ref=ref)


def mip_from_pos(xyzs, C):
    """raymarching.cu:19-25: min(C - 1, max(0, exponent(max |x|) + 1))."""
    e = np.frexp(np.abs(np.asarray(xyzs, np.float32)).max(axis=1))[1]
    return np.clip(e + 1, 0, C - 1)


def mip_from_dt(dt, C, grid_size=G):
    """raymarching.cu:27-32: min(C - 1, max(0, exponent(dt * G)))."""
    e = np.frexp(np.asarray(dt, np.float32) * np.float32(grid_size))[1]
    return np.clip(e, 0, C - 1)


def dt_clamp(dt_scale, grid_size=G):
    """calc_dt's upper clamp SQRT3 * 2 * scale / G in f32 (raymarching.cu:11-13); the test marcher
    passes the cascade count as that scale (raymarching.cu:370, :399)."""
    return SQRT3 * np.float32(2) * np.float32(dt_scale) / np.float32(grid_size)


QUIRK_ESF = 1.0 / 64  # t / 64 reaches the test marcher's clamp at t = 3.5 (C = 2) / 5.2 (C = 3)
TEST_ESF = (0.0, 1.0 / 256, QUIRK_ESF)
TEST_SCALES = (1.0, 1.5)
TEST_NS = (1, 4, 64)
TEST_RAYS = 1500


@functools.lru_cache(maxsize=None)
def eval_march_case(scale, esf):
    """The test marcher's case: 1500 rays (ordinary origins 2..8 away), every other one alive, three
    calls with N_samples 1, 4, 64 on the same hits_t (mutated by each call).
    -> dict(scale, C, esf, o, d, ht0, alive, bf, refs): refs[i] = (outputs of call i, hits_t after it)."""
    C = CASCADES[scale]
    o, d, ht, _ = march_rays(scale, TEST_RAYS, 300, (2.0 * scale, 8.0))
    alive = np.arange(0, TEST_RAYS, 2, dtype=np.int64)
    bf = cascade_bitfield(C)
    ht_ref = ht.copy()
    refs = []
    for N in TEST_NS:
        out = vren_ref.raymarching_test(o, d, ht_ref, alive, bf, C, scale, esf, G, MAX_SAMPLES, N)
        refs.append((out, ht_ref.copy()))
    for a in (o, d, ht, alive, bf) + tuple(x for out, h in refs for x in out + (h,)):
        a.setflags(write=False)
    return dict(scale=scale, C=C, esf=esf, o=o, d=d, ht0=ht, alive=alive, bf=bf, refs=refs)

