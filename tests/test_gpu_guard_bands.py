"""Guard-band tests: the kernels neither write nor read outside their buffers.

Every buffer a case hands to the C ABI (through _lib.call: the Python wrappers allocate their own
outputs) lies between two 64 KiB bands (tests/guard_bands.py) and has exactly its documented or
queried size: no slack anywhere.  Per case
  - the bands of every buffer are intact afterwards, bytewise;
  - output rows the call must leave alone (rows at or past a device count, rows outside every
    segment) still hold the prefill, bytewise;
  - the case runs twice, the bands and the never-to-be-read rows of every input filled with A and then
    with B (floats: NaN and 1e30; indices and counts: two values valid for that array), and the
    outputs of the two runs are bit-identical (the table scatter accumulates with float atomics: each
    run meets its value test's bound instead);
  - the values meet the check of the entry point's existing value test, helpers and bounds imported
    unchanged (no tolerance is derived here, but for ncn_sumsq, which had no test: see
    test_sumsq_and_adam).
That the helper would catch a wrong kernel is shown on the CPU (tests/test_guard_bands_host.py); no
kernel that overruns is ever run on a GPU.

Two places follow the header where it says something else than "untouched": dL_dxyzs / dL_ddirs rows
[*n_dev, n) are written as zeros (include/ncnerf.h; tests/test_gpu_field_input_grad.py asserts it), so
they are checked to be exactly zero; ncn_segment_csr sums [start[r], start[r + 1]) (the reference's
segment_csr), so its rows come in start order without gaps and only the rows in front of the first
and behind the last segment are never read.

The dE outlier share of test_gpu_field_levels is a share of a level's 2 n elements; at n = 1 and 17 it is
applied to the case's 32 n elements and never excludes a single outlier (_check_dE_share says why).

Measured on an MI355X: 105 cases, 9.7 s for the file, the slowest case 0.5 s (test_adam_step[1-0], the
first launch; the field cases 0.3 - 0.45 s each).  Worst observed value over all cases, next to its
borrowed bound (every figure is printed before it is asserted, as "GB-FIGURE"):
  ncn_adam_step / _packed / ncn_adam vs the apex restatement   0.21 / 0.27 / 0.23 of 2e-6 |ref| + 1e-8
  ncn_sumsq vs the fp64 sum                                     5.2e-4 of (n + 1024) 2^-24 sum (asserted: 2x)
  wire, unpacked gradient, packed fragments, marcher, grid     bit-exact (as their value tests demand)
  compositor fw opacity / depth / rend / ws / rgb_bg            0.070 / 0.054 / 0.053 / 0.031 / 0.047 of 2e-5 + 2e-4 |ref|
  compositor bw dL_dsigmas / dL_draws                           0.018 / 0.006 of 1e-4 max |ref| + 1e-3 |ref|
  extra channels fw / dL_dws / dL_draws                         1.3e-3 of 2 (n - 1) u sum |terms| / 0 / exact
  distortion loss / ws scan / wts scan / dL_dws                 0.069 / 0.073 / 0.076 / 0.006 of their bounds
  segment_csr                                                   within 2 (n - 1) u sum |terms| (asserted per row)
  field fwd sigma / rgb                                         fp16 0.020 / 0.038, bf16 0.010 / 0.032 of TOL
  field dE outlier share, worst level (n = 4099)                fp16 0.012 %, bf16 0 %            (cap 2 %)
  field dE outliers at n = 17 / n = 1                           1 of 544 (fp16, level 4) / 0 of 32  (allowed 10 / 1)
  table scatter vs the serial scatter of the decoded dE         rel-L2 3.6e-8, max |diff| / max 1.3e-7, 0 one-sided
                                                                (bounds 1e-6, 1e-5, 1e-4 of the non-zero entries)
  dL/dx, dL/dd worst column rel-L2                              fp16 3.3e-4, bf16 2.9e-3 (n = 1)  (bounds 2e-2, 5e-2)
No band was found modified, no row written that had to be left alone, and no output depended on a fill.

Found: one defect, in csrc/optim.hip.  test_adam_step_packed at pack_off 2 and 3 (n % 4 = 2, 3):
ncn_adam_step_packed's parameters and second moments differed from ncn_adam_step's by one ulp in the
scalar tail (element 10241 of 10242 / 10243) — the compiler contracted adam_apply_kernel's update
differently in the tail of the packed instances than in the plain one.  The tail now states its fused
operations itself with contraction off: the operations the float4 body compiles to, whose code is
unchanged (the old and the new library are bit-identical on n % 4 == 0, the model's case, in all six
instances).  Nothing else: no overrun, no over-read, no size query too small.
"""
import functools

import numpy as np
import pytest
import torch

import guard_bands as gb
import heads_ref
from ncnerf_amd import _lib
from ncnerf_amd.ngp_mt import ENC_BYTES, N_PACKED_HALVES, N_W
from oracle import losses_ref, vren_ref
from test_gpu_heads import U, _exact_inputs, _ray_of, _segments
from test_gpu_optim import _apex_reference
from test_gpu_vren import _assert_segment_sums, _march_inputs

pytestmark = pytest.mark.gpu

FILLS = gb.FLOAT_FILLS  # A, B for float data
HALF_FILLS = (float("nan"), 65504.0)  # ... for 16-bit float data


def _fig(name, value, bound):
    """Every figure is printed before it is asserted (collected into the docstring's table)."""
    print(f"GB-FIGURE {name} worst {value:.3e} bound {bound:.3e}")


class Pool:
    """The guarded buffers of one run: inp() / out() hand out payloads, check() asserts every band."""

    def __init__(self, dev, fill, int_fill=0):
        self.dev, self.fill, self.int_fill, self.handles = dev, fill, int_fill, []

    def inp(self, array, rows=None, fill=None, misalign=0, name="input"):
        # (numpy arrays are copied: the shared cases are read-only)
        a = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.array(array))
        if fill is None:
            fill = self.fill if a.dtype.is_floating_point else self.int_fill
        t, h = gb.guarded_copy(a, fill, self.dev, rows=rows, misalign=misalign)
        self.handles.append((name, h))
        return t

    def out(self, shape, dtype=torch.float32, misalign=0, name="output"):
        t, h = gb.guarded(shape, dtype, self.dev, misalign=misalign)
        self.handles.append((name, h))
        t.handle = h
        return t

    def ins(self, rows=None, **arrays):
        """name=array, ... -> the input buffers in that order (`rows` as for inp, for all of them)."""
        return [self.inp(a, rows=rows, name=k) for k, a in arrays.items()]

    def outs(self, **shapes):
        """name=shape or name=(shape, dtype), ... -> the output buffers in that order."""
        res = []
        for k, sh in shapes.items():
            typed = len(sh) == 2 and isinstance(sh[1], torch.dtype)
            res.append(self.out(sh[0] if typed else sh, sh[1] if typed else torch.float32, name=k))
        return res

    def check(self):
        torch.cuda.synchronize()
        for name, h in self.handles:
            h.assert_bands_intact(name)


def _ab(dev, run, int_fills=(0, 1), atomic=()):
    """run(pool) -> {name: output tensor} under fill A and under fill B; bands checked, outputs
    compared bitwise (but those named in `atomic`).  -> the outputs of run A."""
    res = []
    for fill, ifill in zip(FILLS, int_fills):
        pool = Pool(dev, fill, ifill)
        outs = run(pool)
        pool.check()
        res.append({k: v.clone() for k, v in outs.items()})
    for k in res[0]:
        if k not in atomic:
            gb.assert_same_bits(res[0][k], res[1][k], k)
    return res[0]


# ================================================================================ optimizer
LR, MAX_NORM, B1, B2, EPS, WD = 1e-2, 0.05, 0.9, 0.999, 1e-15, (0.0, 1e-6)


def _work(pool):
    return pool.inp(torch.zeros(int(_lib.lib().ncn_adam_step_work_floats())), name="work")


def _optim_bad(got, ref):
    """test_gpu_optim's bound against the apex restatement: |err| <= 2e-6 |ref| + 1e-8."""
    err = (got - ref).abs()
    lim = 2e-6 * ref.abs() + 1e-8
    return int((err > lim).sum()), float((err / lim).max())


def _group0(n):
    """n_group0: 0, an odd value inside a float4 (or inside the scalar tail when n < 4), n."""
    return sorted({0, 4 * (n // 8) + 1 if n >= 4 else 1, n})


@pytest.mark.parametrize("zero_grads", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_adam_step(dev, n, zero_grads):
    """ncn_adam_step: plain; with amp_state and lr_dev and one step skipped by a non-finite gradient;
    with amp_state and gate and one step skipped by each.  On a skipped step p, m and v are bytewise
    unchanged and g is zeroed only under the fold."""
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g) * 0.1
    grads = [torch.randn(n, generator=g) * 1e-2 for _ in range(3)]
    worst = 0.0
    for n0 in _group0(n):
        ref = _apex_reference(p0, [grads[0], grads[2]], n0, 0.5, LR, MAX_NORM).to(dev)
        for mode in ("plain", "amp", "amp+gate"):
            def run(pool):
                p, m, v = pool.inp(p0, name="p"), pool.inp(torch.zeros(n), name="m"), pool.inp(torch.zeros(n), name="v")
                gr = pool.inp(torch.zeros(n), name="g")
                step = pool.inp(torch.zeros(1, dtype=torch.int32), name="step_dev")
                work = _work(pool)
                amp = pool.inp(torch.tensor([65536.0, 0.0]), name="amp_state") if mode != "plain" else None
                lr_dev = pool.inp(torch.tensor([LR]), name="lr_dev") if mode == "amp" else None
                gate = pool.inp(torch.ones(1, dtype=torch.int32), name="gate") if mode == "amp+gate" else None

                def step_once(grad, gate_v=1):
                    gr.copy_(grad.to(dev))
                    if gate is not None:
                        gate.fill_(gate_v)
                    _lib.call("ncn_adam_step", p, gr, m, v, n, n0, 0.5, MAX_NORM, 1.0 if lr_dev is not None else LR,
                              B1, B2, EPS, WD[0], WD[1], lr_dev, step, work, zero_grads, amp, gate)

                def skipped(grad, gate_v, amp_want):
                    before = [t.clone() for t in (p, m, v)]
                    step_once(grad, gate_v)
                    torch.cuda.synchronize()
                    for t, b in zip((p, m, v), before):
                        assert gb.same_bits(t, b), (mode, "a skipped step changed p, m or v")
                    if zero_grads:
                        assert int(gr.count_nonzero()) == 0
                    else:
                        assert gb.same_bits(gr, grad.to(dev))
                    assert int(step) == 1 and amp.tolist() == amp_want

                step_once(grads[0])
                if mode != "plain":
                    bad = grads[1].clone()
                    bad[n // 2] = float("inf")
                    if mode == "amp+gate":
                        skipped(grads[1], 0, [65536.0, 1.0])  # gated off: the scaler is not touched
                    skipped(bad, 1, [32768.0, 0.0])
                step_once(grads[2])
                torch.cuda.synchronize()
                assert int(step) == 2
                assert int(gr.count_nonzero()) == (0 if zero_grads else int(grads[2].count_nonzero()))
                return {"p": p, "m": m, "v": v, "g": gr}

            out = _ab(dev, run)
            bad, ratio = _optim_bad(out["p"], ref)
            worst = max(worst, ratio)
            assert bad == 0, (n, n0, mode, bad, ratio)
    _fig(f"adam_step n {n} zero_grads {zero_grads}: |err| / (2e-6 |ref| + 1e-8)", worst, 1.0)


@functools.lru_cache(maxsize=None)
def _pack_inv(dev):
    """pack_inv as NGPMT.pack_target builds it for FlatAdam: (N_W, 2) int32, -1 = none, from ncn_field_pack_map."""
    src = torch.empty(N_PACKED_HALVES, dtype=torch.int32, device=dev)
    _lib.call("ncn_field_pack_map", src)
    s = src.cpu().numpy()
    table = np.full((N_W, 2), -1, np.int32)
    fill = np.zeros(N_W, np.int64)
    for q, w in enumerate(s):
        assert 0 <= w < N_W and fill[w] < 2, (q, w)
        table[w, fill[w]] = q
        fill[w] += 1
    return torch.from_numpy(table)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("pack_off", [0, 1, 2, 3, 5])
def test_adam_step_packed(dev, pack_off, precision):
    """pack_off inside a float4 (the `e + 3 >= poff` branch that straddles one): `packed` is
    bit-identical to ncn_field_pack_weights of the updated weights, the parameters to ncn_adam_step's —
    after a normal, a clipped and an AMP-skipped step (the fragments then rewritten from the unchanged
    weights)."""
    n, prec = pack_off + N_W, 0 if precision == "fp16" else 1
    g = torch.Generator().manual_seed(pack_off)
    p0 = torch.randn(n, generator=g) * 0.05
    grads = [torch.randn(n, generator=g) * mag for mag in (1e-4, 10.0, 1e-3)]
    grads[2][n - 5] = float("inf")
    inv = _pack_inv(dev)

    def run(pool):
        bufs = []
        for _ in range(2):  # the packed step, then the plain one
            bufs.append(dict(p=pool.inp(p0, name="p"), m=pool.inp(torch.zeros(n), name="m"),
                             v=pool.inp(torch.zeros(n), name="v"), g=pool.inp(torch.zeros(n), name="g"),
                             step=pool.inp(torch.zeros(1, dtype=torch.int32), name="step_dev"), work=_work(pool),
                             amp=pool.inp(torch.tensor([65536.0, 0.0]), name="amp_state")))
        pinv = pool.inp(inv, fill=-1 if pool.int_fill == 0 else 0, name="pack_inv")
        packed = pool.out((N_PACKED_HALVES,), torch.float16, name="packed")
        for k, grad in enumerate(grads):
            for b, fused in zip(bufs, (True, False)):
                b["g"].copy_(grad.to(dev))
                args = [b["p"], b["g"], b["m"], b["v"], n, pack_off, 1.0, MAX_NORM, LR, B1, B2, EPS, WD[0], WD[1], None,
                        b["step"], b["work"], 1, b["amp"], None]
                if fused:
                    packed.fill_(0)  # stale: the pass must rewrite every fragment
                    _lib.call("ncn_adam_step_packed", *args, pinv, pack_off, packed, prec)
                else:
                    _lib.call("ncn_adam_step", *args)
            w = pool.inp(bufs[0]["p"][pack_off:], name="w_master")  # (an aligned copy of the master weights)
            want = pool.out((N_PACKED_HALVES,), torch.float16, name="packed (reference)")
            _lib.call("ncn_field_pack_weights", w, want, prec)
            torch.cuda.synchronize()
            assert gb.same_bits(packed, want), (k, "packed != ncn_field_pack_weights of the updated weights")
            for key in ("p", "m", "v", "g", "step", "amp"):
                gb.assert_same_bits(bufs[0][key], bufs[1][key], f"step {k} {key}", "ncn_adam_step_packed != ncn_adam_step")
        assert int(bufs[0]["step"]) == 2 and bufs[0]["amp"].tolist() == [32768.0, 0.0]
        return {"p": bufs[0]["p"], "m": bufs[0]["m"], "v": bufs[0]["v"], "packed": packed}

    out = _ab(dev, run)
    ref = _apex_reference(p0, grads[:2], pack_off, 1.0, LR, MAX_NORM).to(dev)
    bad, ratio = _optim_bad(out["p"], ref)
    _fig(f"adam_step_packed pack_off {pack_off} {precision}: |err| / (2e-6 |ref| + 1e-8)", ratio, 1.0)
    assert bad == 0, (bad, ratio)


F32 = lambda x: float(np.float32(x))  # noqa: E731


@pytest.mark.parametrize("n", [1, 3, 5, 4099])
def test_sumsq_and_adam(dev, n):
    """ncn_sumsq (with step_inc) and ncn_adam at step 1: 1 - powf(b, 1) is exact, so the apex
    restatement with the f32 betas states ncn_adam's f32 bias corrections exactly; clipped and
    unclipped, with lr_dev, with step_dev on its own, and once with all four buffers 4 bytes off a
    16-byte boundary (the scalar path).
    ncn_sumsq's bound (it had no test; from the number formats): each of the n squares is one fma onto a
    partial, the 1024 partials are summed afterwards, all terms >= 0: whatever the order,
    |sum - exact| <= (n + 1024) 2^-24 exact to first order; asserted with 2x for the higher orders."""
    g = torch.Generator().manual_seed(100 + n)
    p0 = torch.randn(n, generator=g) * 0.1
    worst, worst_sq = 0.0, 0.0
    for gmag in (1.0, 1e-4):  # norm >> 0.05: clipped; << 0.05: not
        grad = torch.randn(n, generator=g) * gmag
        ref = _apex_reference(p0, [grad], n, 1.0, LR, MAX_NORM, wd=(1e-6, 1e-6), b1=F32(B1), b2=F32(B2)).to(dev)
        exact = float((grad.double() ** 2).sum())
        for variant in ("host", "lr_dev", "step_dev", "misaligned"):
            mis = 4 if variant == "misaligned" else 0

            def run(pool):
                x = pool.inp(grad, name="x")
                part = pool.out((1024,), name="out_partial")
                inc = pool.inp(torch.tensor([7], dtype=torch.int32), name="step_inc")
                _lib.call("ncn_sumsq", x, n, part, inc)
                p, m, v = (pool.inp(t, misalign=mis, name=k)
                           for k, t in (("p", p0), ("m", torch.zeros(n)), ("v", torch.zeros(n))))
                gr = pool.inp(grad, misalign=mis, name="g")
                assert p.data_ptr() % 16 == mis
                lr_dev = pool.inp(torch.tensor([LR]), name="lr_dev") if variant == "lr_dev" else None
                step_dev = pool.inp(torch.tensor([1], dtype=torch.int32), name="step_dev") if variant == "step_dev" else None
                _lib.call("ncn_adam", p, gr, m, v, n, part, MAX_NORM, 1.0 if lr_dev is not None else LR, B1, B2, EPS, 1e-6,
                          3 if step_dev is not None else 1, lr_dev, step_dev)
                torch.cuda.synchronize()
                assert int(inc) == 8  # incremented once
                assert gb.same_bits(gr, grad.to(dev))
                return {"p": p, "m": m, "v": v, "part": part}

            out = _ab(dev, run)
            got = float(out["part"].double().sum())
            worst_sq = max(worst_sq, abs(got - exact) / ((n + 1024) * 2.0 ** -24 * exact))
            assert abs(got - exact) <= 2 * (n + 1024) * 2.0 ** -24 * exact, (got, exact)
            bad, ratio = _optim_bad(out["p"], ref)
            worst = max(worst, ratio)
            assert bad == 0, (n, gmag, variant, bad, ratio)
    _fig(f"sumsq n {n}: |err| / ((n + 1024) u sum)", worst_sq, 2.0)
    _fig(f"adam n {n}: |err| / (2e-6 |ref| + 1e-8)", worst, 1.0)


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("world", [1, 8])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2049])
def test_grad_pack_unpack(dev, n, world, with_scale):
    """The wire is bit-identical to numpy's two fp16 roundings, the unpacked gradient to float(wire) / S."""
    rng = np.random.default_rng(n)
    grad = (rng.normal(size=n) * rng.choice([1e-6, 1e-2, 30.0], n)).astype(np.float32)
    grad[0] = 70.0  # (x 1024: overflows fp16 -> inf, the step the GradScaler skips)
    s = np.float32(1024.0 if with_scale else 1.0)
    with np.errstate(over="ignore"):
        wire_ref = ((grad * s).astype(np.float16).astype(np.float32) / np.float32(world)).astype(np.float16)
    back_ref = wire_ref.astype(np.float32) * (np.float32(1.0) / s)

    def run(pool):
        half_fill = HALF_FILLS[0] if pool.fill != pool.fill else HALF_FILLS[1]  # (NaN with NaN, 65504 with 1e30)
        gr = pool.inp(grad, name="grad")
        scale = pool.inp(np.array([s]), name="scale") if with_scale else None
        wire = pool.out((n,), torch.float16, name="wire")
        _lib.call("ncn_grad_pack_f16", gr, n, scale, world, wire)
        win = pool.inp(torch.from_numpy(wire_ref), fill=half_fill, name="wire (input)")
        back = pool.out((n,), name="grad (unpacked)")
        _lib.call("ncn_grad_unpack_f16", win, n, scale, back)
        return {"wire": wire, "back": back}

    out = _ab(dev, run)
    assert np.array_equal(out["wire"].view(torch.int16).cpu().numpy(), wire_ref.view(np.int16))
    assert np.array_equal(out["back"].view(torch.int32).cpu().numpy(), back_ref.view(np.int32))
    assert with_scale == bool(np.isinf(wire_ref[0]))


# ================================================================================ segment kernels
SEG_COUNTS = [0, 1, 63, 64, 65, 129, 257, 300, 1025]
N_COOP = 256  # the compositors' workgroups for long rows at the front of the grid


@functools.lru_cache(maxsize=None)
def _seg_layout(layout):
    """-> (rays_a, S, used).  "shuffled": test_gpu_heads._segments as it is (shuffled rows; unused rows
    in front, between two segments and behind); "long_first": its rows with the long rays first, as
    the training step orders them (257 and 300 on the workgroup path); "ray_order": in ray order
    behind 256 short rows, so a short row lies N_COOP rows ahead of every long one and no workgroup
    takes it (the single-wave path, see test_gpu_vren._channel_inputs)."""
    if layout == "ray_order":
        rays_a, S, used = _segments([1, 0] * (N_COOP // 2) + SEG_COUNTS, 21)
        rays_a = rays_a[np.argsort(rays_a[:, 0])]
        long_rows = np.nonzero(rays_a[:, 2] > 256)[0]
        assert (long_rows >= N_COOP).all() and (rays_a[long_rows - N_COOP, 2] <= 256).all()
    else:
        rays_a, S, used = _segments(SEG_COUNTS, 20)
        if layout == "long_first":
            rays_a = np.concatenate([rays_a[rays_a[:, 2] > 256], rays_a[rays_a[:, 2] <= 256]])
    assert used.sum() == rays_a[:, 2].sum() and not used[:3].any() and not used[-37:].any()
    for a in (rays_a, used):
        a.setflags(write=False)
    return rays_a, S, used


LAYOUTS = ["shuffled", "long_first", "ray_order"]


@functools.lru_cache(maxsize=None)
def _composite_case(layout, C):
    """Inputs in the form of test_gpu_vren._channel_inputs (|N(0, 0.2)| keeps T well above 1e-4, so a
    ray stops only at a 1e5 sample: no borderline stop) and the oracle's forward, computed once."""
    rays_a, S, used = _seg_layout(layout)
    rng = np.random.default_rng(30 + C)
    sig = np.abs(rng.normal(0, 0.2, S)).astype(np.float32)
    for ray, s, c in rays_a:
        if c > 8 and ray % 2 == 0:
            sig[s + int(0.7 * c)] = 1e5  # every other longer ray stops early
    raws = rng.random((S, C), dtype=np.float32)
    deltas = np.full(S, 1.7e-3, np.float32)
    ts = (np.arange(S) % 977 * 1.7e-3).astype(np.float32)
    for a in (sig, raws, deltas, ts):
        a[~used] = 0.0
    ref = vren_ref.composite_train_multi_fw(sig, raws, deltas, ts, rays_a, 1e-4)
    R = rays_a.shape[0]
    ups = (rng.normal(size=R).astype(np.float32), rng.normal(size=R).astype(np.float32),
           rng.normal(size=(R, C)).astype(np.float32), np.where(used, rng.normal(size=S), 0).astype(np.float32))
    return sig, raws, deltas, ts, ref, ups


def _close(got, ref, rtol, atol, name, worst):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    lim = atol + rtol * np.abs(ref)
    if got.size:
        worst[name] = max(worst.get(name, 0.0), float((np.abs(got - ref) / lim).max()))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=name)


@pytest.mark.parametrize("C", [1, 3, 6])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_composite_train(dev, layout, C):
    """ncn_composite_train_fw / _fw_bg / _bw / _bw_bg (without and with dL_dws) at test_gpu_vren's bounds:
    forward exact counts, rtol 2e-4 + 2e-5; backward rtol 1e-3 + 1e-4 max |ref|."""
    rays_a, S, used = _seg_layout(layout)
    sig, raws, deltas, ts, ref, ups = _composite_case(layout, C)
    R, unused = rays_a.shape[0], ~used
    tot_r, O, D, RE, ws_r = ref
    worst = {}

    def per_sample(pool):
        return pool.ins(rows=unused, sigmas=sig, raws=raws, deltas=deltas, ts=ts)

    for bg in (None, 0.7):
        def run_fw(pool):
            s_, r_, d_, t_ = per_sample(pool)
            ra = pool.inp(rays_a, name="rays_a")
            tot = pool.out((R,), torch.int64, name="total_samples")
            op, dp, rend, ws = pool.outs(opacity=(R,), depth=(R,), rend=(R, C), ws=(S,))
            outs = {"total": tot, "opacity": op, "depth": dp, "rend": rend, "ws": ws}
            if bg is None:
                _lib.call("ncn_composite_train_fw", s_, r_, d_, t_, ra, R, S, C, 1e-4, tot, op, dp, rend, ws)
            else:
                outs["rgb_bg"] = pool.out((R, C), name="rgb_bg")
                _lib.call("ncn_composite_train_fw_bg", s_, r_, d_, t_, ra, R, S, C, 1e-4, tot, op, dp, rend, ws, bg,
                          outs["rgb_bg"])
            torch.cuda.synchronize()
            ws.handle.assert_untouched(unused, "ws")
            return outs

        out = _ab(dev, run_fw)
        assert np.array_equal(out["total"].cpu().numpy(), tot_r)
        for k, r in (("opacity", O), ("depth", D), ("rend", RE)):
            _close(out[k].cpu().numpy(), r, 2e-4, 2e-5, f"composite fw {k}", worst)
        _close(out["ws"].cpu().numpy()[used], ws_r[used], 2e-4, 2e-5, "composite fw ws", worst)
        if bg is not None:
            rgb_r = RE + np.float32(bg) * (1 - O)[:, None]
            _close(out["rgb_bg"].cpu().numpy(), rgb_r, 2e-4, 2e-5, "composite fw rgb_bg", worst)

    dO, dD, dR, dW = ups
    for dW_, bg in ((None, None), (dW, None), (None, 0.7), (dW, 0.7)):
        def run_bw(pool):
            s_, r_, d_, t_ = per_sample(pool)
            ra = pool.inp(rays_a, name="rays_a")
            w_ = pool.inp(ws_r, rows=unused, name="ws")
            gw = pool.inp(dW_, rows=unused, name="dL_dws") if dW_ is not None else None
            go, gd, gr = pool.inp(dO, name="dL_dopacity"), pool.inp(dD, name="dL_ddepth"), pool.inp(dR, name="dL_drend")
            o_, dd_, re_ = pool.inp(O, name="opacity"), pool.inp(D, name="depth"), pool.inp(RE, name="rend")
            dsig, draws = pool.out((S,), name="dL_dsigmas"), pool.out((S, C), name="dL_draws")
            if bg is None:
                _lib.call("ncn_composite_train_bw", go, gd, gr, gw, s_, r_, w_, d_, t_, ra, R, S, C, o_, dd_, re_, 1e-4,
                          dsig, draws)
            else:
                _lib.call("ncn_composite_train_bw_bg", go, gd, gr, gw, s_, r_, w_, d_, t_, ra, R, S, C, o_, dd_, re_, 1e-4,
                          bg, dsig, draws)
            torch.cuda.synchronize()
            dsig.handle.assert_untouched(unused, "dL_dsigmas")
            draws.handle.assert_untouched(unused, "dL_draws")
            return {"dL_dsigmas": dsig, "dL_draws": draws}

        out = _ab(dev, run_bw)
        dO_ref = dO if bg is None else (dO - np.float32(bg) * dR.sum(1, dtype=np.float32)).astype(np.float32)
        r2 = vren_ref.composite_train_multi_bw(dO_ref, dD, dR, dW_, sig, raws, ws_r, deltas, ts, rays_a, O, D, RE, 1e-4)
        for k, r in zip(("dL_dsigmas", "dL_draws"), r2):
            _close(out[k].cpu().numpy()[used], r[used], 1e-3, 1e-4 * np.abs(r[used]).max(), f"composite bw {k}", worst)
    for k, v in worst.items():
        _fig(f"{k} {layout} C {C}: |err| / (atol + rtol |ref|)", v, 1.0)


@pytest.mark.parametrize("C", [3, 51])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_composite_extra(dev, layout, C):
    """ncn_composite_extra_fw / _bw by test_gpu_heads.test_extra_channels' checks (exact products: the
    forward within the summation-order bound 2 (n - 1) u sum |terms|, dL_draws exact, dL_dws within
    2 (C - 1) u sum |terms|)."""
    rays_a, S, used = _seg_layout(layout)
    R, unused = rays_a.shape[0], ~used
    ws, raws = _exact_inputs(rays_a, S, used, C, 5)
    ws, raws = np.nan_to_num(ws), np.nan_to_num(raws)  # (the unused rows: filled per run below)
    up = (np.random.default_rng(6).integers(-256, 256, (R, C)) / 64.0).astype(np.float32)

    def run(pool):
        (w_, r_), ra = pool.ins(rows=unused, ws=ws, raws=raws), pool.inp(rays_a, name="rays_a")
        rend = pool.out((R, C), name="rend")
        _lib.call("ncn_composite_extra_fw", w_, r_, ra, R, S, C, rend)
        g_ = pool.inp(up, name="dL_drend")
        dws, draws = pool.out((S,), name="dL_dws"), pool.out((S, C), name="dL_draws")
        _lib.call("ncn_composite_extra_bw", g_, w_, r_, ra, R, S, C, dws, draws)
        torch.cuda.synchronize()
        dws.handle.assert_untouched(unused, "dL_dws")
        draws.handle.assert_untouched(unused, "dL_draws")
        return {"rend": rend, "dL_dws": dws, "dL_draws": draws}

    out = _ab(dev, run)
    ref, mag, cnt = heads_ref.composite_extra(ws, raws, rays_a, R)
    got = out["rend"].cpu().numpy().astype(np.float64)
    bound = 2.0 * np.maximum(cnt - 1, 0)[:, None] * U * mag
    assert np.all(np.abs(got - ref) <= bound), float(np.max(np.abs(got - ref) - bound))
    assert np.all(got[cnt == 0] == 0.0)
    dws_ref, draws_ref = heads_ref.composite_extra_bw(up, ws, raws, rays_a)
    dws, draws = out["dL_dws"].cpu().numpy().astype(np.float64), out["dL_draws"].cpu().numpy().astype(np.float64)
    assert np.array_equal(draws[used], draws_ref[used])
    terms = np.abs(raws.astype(np.float64) * up[_ray_of(rays_a, S)].astype(np.float64)).sum(1)
    lim = 2.0 * (C - 1) * U * terms
    assert np.all(np.abs(dws - dws_ref)[used] <= lim[used])
    live = bound > 0
    _fig(f"composite_extra fw {layout} C {C}: |err| / (2 (n - 1) u sum |terms|)",
         float((np.abs(got - ref)[live] / bound[live]).max()) if live.any() else 0.0, 1.0)
    live = used & (lim > 0)
    _fig(f"composite_extra bw dL_dws {layout} C {C}: |err| / (2 (C - 1) u sum |terms|)",
         float((np.abs(dws - dws_ref)[live] / lim[live]).max()) if live.any() else 0.0, 1.0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_distortion(dev, layout):
    """ncn_distortion_loss_fw / _bw at test_gpu_distortion's bounds (loss 1e-4 + 1e-7, scans 1e-5 + 1e-7,
    dL_dws 1e-4 + 1e-8), inputs in its _rays' form."""
    rays_a, S, used = _seg_layout(layout)
    R, unused = rays_a.shape[0], ~used
    rng = np.random.default_rng(40)
    ws = np.where(used, rng.uniform(0, 0.1, S), 0).astype(np.float32)
    deltas = np.where(used, rng.uniform(1e-3, 3e-3, S), 0).astype(np.float32)
    ts = np.zeros(S, np.float32)
    for _, s0, n in rays_a:
        ts[s0:s0 + n] = np.cumsum(deltas[s0:s0 + n]) + rng.uniform(0, 0.5)
    g = rng.uniform(0.5, 1.5, R).astype(np.float32)
    rl, rwsi, rwtsi = losses_ref.distortion_loss_fw(ws, deltas, ts, rays_a)
    ref_bw = losses_ref.distortion_loss_bw(g, rwsi, rwtsi, ws, deltas, ts, rays_a)

    def run(pool):
        w_, d_, t_ = (pool.inp(a, rows=unused, name=k) for k, a in (("ws", ws), ("deltas", deltas), ("ts", ts)))
        ra = pool.inp(rays_a, name="rays_a")
        loss, wsi, wtsi = pool.outs(loss=(R,), ws_inclusive_scan=(S,), wts_inclusive_scan=(S,))
        _lib.call("ncn_distortion_loss_fw", w_, d_, t_, ra, R, loss, wsi, wtsi)
        g_ = pool.inp(g, name="dL_dloss")
        i1, i2 = pool.ins(rows=unused, ws_inclusive_scan_in=rwsi, wts_inclusive_scan_in=rwtsi)
        dws = pool.out((S,), name="dL_dws")
        _lib.call("ncn_distortion_loss_bw", g_, i1, i2, w_, d_, t_, ra, R, dws)
        torch.cuda.synchronize()
        for t in (wsi, wtsi, dws):
            t.handle.assert_untouched(unused)
        return {"loss": loss, "wsi": wsi, "wtsi": wtsi, "dws": dws}

    out = _ab(dev, run)
    worst = {}
    _close(out["loss"].cpu().numpy(), rl, 1e-4, 1e-7, "distortion loss", worst)
    _close(out["wsi"].cpu().numpy()[used], rwsi[used], 1e-5, 1e-7, "distortion ws scan", worst)
    _close(out["wtsi"].cpu().numpy()[used], rwtsi[used], 1e-5, 1e-7, "distortion wts scan", worst)
    _close(out["dws"].cpu().numpy()[used], ref_bw[used], 1e-4, 1e-8, "distortion dL_dws", worst)
    for k, v in worst.items():
        _fig(f"{k} {layout}: |err| / (atol + rtol |ref|)", v, 1.0)


@pytest.mark.parametrize("short_rows", [0, 256])
def test_segment_csr(dev, short_rows):
    """ncn_segment_csr by test_gpu_vren._assert_segment_sums (2 (n - 1) u sum |terms| per row).  Row r sums
    [start[r], start[r + 1]): the rows in start order without gaps; never read: the rows in front of
    the first segment and behind the last."""
    rays_a, S, used = _segments([1, 0] * (short_rows // 2) + SEG_COUNTS, 22, gap=0)
    # (by start, an empty row in front of the row it shares its start with)
    rays_a = rays_a[np.lexsort((rays_a[:, 2] > 0, rays_a[:, 1]))]
    R, unused = rays_a.shape[0], ~used
    assert np.array_equal(rays_a[1:, 1], rays_a[:-1, 1] + rays_a[:-1, 2]) and unused[:3].all() and unused[-37:].all()
    rng = np.random.default_rng(41)
    ts = np.where(used, rng.uniform(0.0, 3.0, S), 0).astype(np.float32)
    gx = np.where(used[:, None], rng.normal(size=(S, 3)), 0).astype(np.float32)
    gd = np.where(used[:, None], rng.normal(size=(S, 3)), 0).astype(np.float32)
    for x, y in ((gx, gd), (gx, None), (None, gd)):
        def run(pool):
            x_ = pool.inp(x, rows=unused, name="dL_dxyzs") if x is not None else None
            y_ = pool.inp(y, rows=unused, name="dL_ddirs") if y is not None else None
            t_, ra = pool.inp(ts, rows=unused, name="ts"), pool.inp(rays_a, name="rays_a")
            d_o, d_d = pool.out((R, 3), name="dL_drays_o"), pool.out((R, 3), name="dL_drays_d")
            _lib.call("ncn_segment_csr", x_, y_, t_, ra, R, d_o, d_d)
            return {"d_o": d_o, "d_d": d_d}

        # (rays_a's band: 0 = an empty range at sample 0, or S - 37 = the end of the last segment)
        out = _ab(dev, run, int_fills=(0, int(rays_a[-1, 1] + rays_a[-1, 2])))
        _assert_segment_sums(rays_a, ts, x, y, out["d_o"].cpu().numpy(), out["d_d"].cpu().numpy())


# ================================================================================ marcher
@functools.lru_cache(maxsize=None)
def _scene():
    from ncnerf_amd.synthetic import SyntheticScene
    return SyntheticScene()


MS = 64
MARCH_NAMES = ("rays_a", "xyzs", "dirs", "deltas", "ts", "counter")


@pytest.mark.parametrize("R", [1, 65, 777])
def test_march_train(dev, R):
    """ncn_march_train_walk -> _scan -> _pack and ncn_march_train_fused at max_samples 64, bit-exact
    against the oracle as in test_gpu_vren; the fused marcher's outputs have the capacity R *
    max_samples, its rows past the count untouched; work has ncn_march_train_fused_work_bytes(R) bytes."""
    scene = _scene()
    o, d, ht, noise = _march_inputs(scene, R, 7 + R, dev)
    ref = vren_ref.raymarching_train(o, d, ht, scene.bitfield, 1, 0.5, 0.0, noise, 128, MS)
    S = int(ref[5][0])
    assert S > 0 or R == 1

    def run_eager(pool):
        o_, d_, h_, n_ = (pool.inp(a, name=k) for k, a in (("rays_o", o), ("rays_d", d), ("hits_t", ht), ("noise", noise)))
        bf = pool.inp(scene.bitfield, fill=0 if pool.int_fill == 0 else 255, name="bitfield")
        counts = pool.out((R,), torch.int32, name="counts")
        sx, st, sd = pool.outs(slab_xyz=(R * MS * 3,), slab_t=(R * MS,), slab_dt=(R * MS,))
        _lib.call("ncn_march_train_walk", o_, d_, h_, n_, R, bf, 1, 0.5, 0.0, 128, MS, counts, sx, st, sd)
        rays_a, counter = pool.out((R, 3), torch.int64, name="rays_a"), pool.out((2,), torch.int32, name="counter")
        _lib.call("ncn_march_train_scan", counts, R, rays_a, counter)
        xyzs, dirs, deltas, ts = pool.outs(xyzs=(S, 3), dirs=(S, 3), deltas=(S,), ts=(S,))
        _lib.call("ncn_march_train_pack", d_, rays_a, R, MS, sx, st, sd, xyzs, dirs, deltas, ts)
        return dict(zip(MARCH_NAMES, (rays_a, xyzs, dirs, deltas, ts, counter)))

    out = _ab(dev, run_eager)
    for name, r in zip(MARCH_NAMES, ref):
        a = out[name].cpu().numpy()
        assert a.shape == r.shape and np.array_equal(a, r), f"eager {name}: {np.argwhere(a != r)[:5]}"

    def run_fused(pool):
        o_, d_, n_ = (pool.inp(a, name=k) for k, a in (("rays_o", o), ("rays_d", d), ("noise", noise)))
        bf = pool.inp(scene.bitfield, fill=0 if pool.int_fill == 0 else 255, name="bitfield")
        sx, st, sd = pool.outs(slab_xyz=(R * MS * 3,), slab_t=(R * MS,), slab_dt=(R * MS,))
        work = pool.out((int(_lib.lib().ncn_march_train_fused_work_bytes(R)),), torch.uint8, name="work")
        rays_a, counter = pool.out((R, 3), torch.int64, name="rays_a"), pool.out((2,), torch.int32, name="counter")
        cap = R * MS
        xyzs, dirs, deltas, ts = pool.outs(xyzs=(cap, 3), dirs=(cap, 3), deltas=(cap,), ts=(cap,))
        _lib.call("ncn_march_train_fused", o_, d_, R, 0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.01, n_, 0, None, bf, 1, 0.5, 128, MS,
                  sx, st, sd, work, rays_a, xyzs, dirs, deltas, ts, counter)
        torch.cuda.synchronize()
        for t in (xyzs, dirs, deltas, ts):
            t.handle.assert_untouched(slice(S, cap))
        return dict(zip(MARCH_NAMES, (rays_a, xyzs, dirs, deltas, ts, counter)))

    out = _ab(dev, run_fused)
    for name, r in zip(MARCH_NAMES, ref):
        a = out[name].cpu().numpy()
        if name == "rays_a":
            a = a[np.argsort(a[:, 0], kind="stable")]
        if name in ("xyzs", "dirs", "deltas", "ts"):
            a = a[:S]
        assert np.array_equal(a, r), f"fused {name}: {np.argwhere(a != r)[:5]}"


@pytest.mark.parametrize("n_samples", [1, 4])
@pytest.mark.parametrize("n_alive", [1, 257])
def test_march_test(dev, n_alive, n_samples):
    """ncn_march_test, bit-exact against the oracle as in test_gpu_vren.test_raymarching_test_bitexact;
    the alive list is longer than n_alive, its tail holding two valid ray indices in turn."""
    scene = _scene()
    R = 600
    o, d, ht, _ = _march_inputs(scene, R, 11, dev)
    alive = np.arange(0, 2 * n_alive, 2, dtype=np.int64)
    ht_ref = ht.copy()
    ref = vren_ref.raymarching_test(o, d, ht_ref, alive, scene.bitfield, 1, 0.5, 0.0, 128, 1024, n_samples)
    tail = 19
    names = ("xyzs", "dirs", "deltas", "ts", "n_eff", "hits_t")

    def run(pool):
        o_, d_, h_ = (pool.inp(a, name=k) for k, a in (("rays_o", o), ("rays_d", d), ("hits_t", ht)))
        bf = pool.inp(scene.bitfield, fill=0 if pool.int_fill == 0 else 255, name="bitfield")
        al = pool.inp(np.concatenate([alive, np.zeros(tail, np.int64)]), rows=slice(n_alive, None), name="alive")
        A, N = n_alive, n_samples
        xyzs, dirs, deltas, ts = pool.outs(xyzs=(A, N, 3), dirs=(A, N, 3), deltas=(A, N), ts=(A, N))
        n_eff = pool.out((A,), torch.int32, name="n_eff")
        _lib.call("ncn_march_test", o_, d_, h_, al, A, bf, 1, 0.5, 0.0, 128, 1024, N, xyzs, dirs, deltas, ts, n_eff)
        return dict(zip(names, (xyzs, dirs, deltas, ts, n_eff, h_)))

    out = _ab(dev, run, int_fills=(0, R - 1))
    for name, r in zip(names, list(ref) + [ht_ref]):
        a = out[name].cpu().numpy()
        assert a.shape == r.shape and np.array_equal(a, r), f"{name}: {np.argwhere(a != r)[:5]}"


# ================================================================================ field
import field_level_check  # noqa: E402
import test_gpu_field_input_grad as ig  # noqa: E402
import test_gpu_field_levels as fl  # noqa: E402
from oracle import field_ref  # noqa: E402
from test_gpu_field import TOL, _inputs, _model_from_oracle  # noqa: E402
from test_gpu_scatter_units import _check as _check_scatter  # noqa: E402

FIELD_CASES = [(1, None), (17, None), (4099, None), (4099, 4092)]  # (n, device count)
FIELD_IDS = ["n1", "n17", "n4099", "n4099_count4092"]


@functools.lru_cache(maxsize=None)
def _field_model(dev, precision, loss_scale):
    return _model_from_oracle(fl._params()[0], dev, precision, loss_scale=loss_scale)


@functools.lru_cache(maxsize=None)
def _field_consts(dev, precision, loss_scale, fill):
    """The model's read-only device inputs between bands, one copy per fill: the table, the packed
    weights, the master weights, the loss scale (None for bf16)."""
    m = _field_model(dev, precision, loss_scale)
    half_fill = HALF_FILLS[0] if fill != fill else HALF_FILLS[1]
    pool = Pool(dev, fill)
    scale = m._bwd_loss_scale()
    return pool, dict(table=pool.inp(m.flat_params()[: m._n_table].detach(), name="table"),
                      packed=pool.inp(m._pack_weights(), fill=half_fill, name="weights_packed"),
                      w_master=pool.inp(m.flat_params()[m._n_table:m._n_table + N_W].detach(), name="w_master"),
                      scale=None if scale is None else pool.inp(scale.detach(), name="loss_scale"))


@functools.lru_cache(maxsize=None)
def _oracle_forward(precision, n):
    P, levels = fl._params()
    x, d = _inputs(n, 2)
    sig, rgb, _ = field_ref.field_forward(x, d, P, levels, emulate=precision)
    return sig.numpy(), rgb.numpy()


def _enc_halves(n):
    return ((n + 15) // 16) * 16 * ENC_BYTES // 2  # test_gpu_field_levels._mlp_pass's size


def _field_order(m, x, n, count, dev):
    """The Morton-window processing order of the first `count` samples (a plain tensor: sort_windows
    is not under test here)."""
    n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    order = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.call("ncn_field_sort_windows", x.to(dev), n, n_dev, m._xyz_min, m._xyz_extent, order)
    torch.cuda.synchronize()
    o = order.cpu().numpy().astype(np.int64)
    nv = n if count is None else count
    assert np.array_equal(np.sort(o[:nv]), np.arange(nv))
    return order.cpu()


def _field_args(pool, dev, x, d, n, count, order, nv):
    """x, d, n_dev, order between bands; rows at or past the count hold the fill (order: a valid index)."""
    past = slice(nv, n)
    x_, d_ = pool.inp(x, rows=past, name="xyzs"), pool.inp(d, rows=past, name="dirs")
    n_dev = None if count is None else pool.inp(torch.tensor([count], dtype=torch.int32), name="n_dev")
    o_fill = 0 if pool.int_fill == 0 else nv - 1
    order_ = None if order is None else pool.inp(order, rows=past, fill=o_fill, name="order")
    return x_, d_, n_dev, order_


def _check_dE_share(dE, ref, precision, tag):
    """test_gpu_field_levels' outlier rule and its cap, a share of 2 % of a level's 2 n elements.  A share
    needs elements to be a share of: below 50 per level a single outlier, which the rule's own docstring
    expects now and then (the oracle against its own fp64 run: up to 0.35 % of the elements), is already
    2.9 % (n = 17) or 50 % (n = 1) of a level.  There the outliers are counted over the case's 32 n
    elements against the same 2 %, and never less than the one outlier that a share cannot exclude; a
    level computed wrongly makes every one of its elements an outlier, at any n."""
    if dE.shape[0] * 2 >= 50:
        share = field_level_check.outlier_share(dE.numpy(), ref, precision)
        _fig(f"field dE outlier share, worst level, {precision} {tag}", float(share.max()), fl.SHARE_CAP)
        fl._check_dE(dE, ref, precision, f"guard bands {tag}")
        return
    bad = field_level_check.outlier_mask(dE.numpy(), ref, precision)
    allowed = max(1, int(fl.SHARE_CAP * bad.size))
    _fig(f"field dE outliers of {bad.size} elements, {precision} {tag}", float(bad.sum()), float(allowed))
    assert int(bad.sum()) <= allowed, (tag, int(bad.sum()), bad.sum(0).tolist())


@pytest.mark.parametrize("with_order", [False, True], ids=["sample_order", "morton_order"])
@pytest.mark.parametrize("n,count", FIELD_CASES, ids=FIELD_IDS)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_field_passes(dev, precision, n, count, with_order):
    """ncn_field_fwd (modes 0, 1 and, without an order, 2), ncn_field_bwd_mlp, ncn_field_bwd_mlp_part
    (parts 1 + 2 on the full grid: bit for bit the one pass) and ncn_field_scatter, by the checks of
    test_gpu_field.py (TOL) and test_gpu_field_levels.py (header, level_max, dE outlier share <= 2 %: see
    _check_dE_share for n < 25; the scatter's criteria against the serial scatter of the decoded dE).
    slab: ncn_field_bwd_blocks(n) x N_W floats, dE_ws: ncn_field_bwd_dE_floats(n), level_max [256][16], stash:
    ncn_field_bwd_stash_floats(n), the encoding cache at _mlp_pass's size."""
    L = _lib.lib()
    m = _field_model(dev, precision, fl.LOSS_SCALE)
    prec, nv = m._prec, n if count is None else count
    x, d = _inputs(n, 2)
    gs, gr = fl._upstream(n)
    order = _field_order(m, x, n, count, dev) if with_order else None
    nb = int(L.ncn_field_bwd_blocks(n))
    n_de, n_st = int(L.ncn_field_bwd_dE_floats(n)), int(L.ncn_field_bwd_stash_floats(n))
    assert int(L.ncn_field_bwd_part_blocks(n, 1)) == nb and int(L.ncn_field_bwd_part_blocks(n, 2)) >= nb
    n_entries = m._n_table // 2
    past = slice(nv, n)

    def run(pool):
        cpool, c = _field_consts(dev, precision, fl.LOSS_SCALE, pool.fill)
        x_, d_, n_dev, order_ = _field_args(pool, dev, x, d, n, count, order, nv)
        geo = (m._levels_ptr, m._xyz_min, m._xyz_extent)
        sig, rgb = pool.out((n,), name="sigmas"), pool.out((n, 3), name="rgbs")
        enc = pool.out((_enc_halves(n),), torch.float16, name="enc_cache")
        _lib.call("ncn_field_fwd", x_, d_, n, n_dev, order_, c["table"], *geo, c["packed"], prec, 0, sig, rgb, enc)
        sig1 = pool.out((n,), name="sigmas (mode 1)")
        _lib.call("ncn_field_fwd", x_, None, n, n_dev, order_, c["table"], *geo, c["packed"], prec, 1, sig1, None, None)
        outs = {"sigmas": sig, "rgbs": rgb, "sigmas1": sig1}
        if order is None:
            sig2 = outs["sigmas2"] = pool.out((n,), name="sigmas (mode 2)")
            enc2 = pool.out((_enc_halves(n),), torch.float16, name="enc_cache (mode 2 scratch)")
            _lib.call("ncn_field_fwd", x_, None, n, n_dev, None, c["table"], *geo, c["packed"], prec, 2, sig2, None, enc2)
        gs_, gr_ = pool.inp(gs, rows=past, name="dL_dsigmas"), pool.inp(gr, rows=past, name="dL_drgbs")

        def workspace():
            w0 = torch.zeros(n_de)
            w0[-32:] = 7.0  # (the unit queue: the MLP pass must zero it)
            return pool.inp(w0, name="dE_ws"), pool.inp(torch.full((256, 16), -1.0), name="level_max")

        slab = pool.out((nb * N_W,), name="slab")
        ws, lmax = workspace()
        _lib.call("ncn_field_bwd_mlp", x_, d_, n, n_dev, order_, c["packed"], prec, enc, gs_, gr_, c["scale"], slab, ws,
                  lmax)
        slab2, stash = pool.out((nb * N_W,), name="slab (parts)"), pool.out((n_st,), name="dh_stash")
        ws2, lmax2 = workspace()
        for part, ds in ((1, None), (2, gs_)):
            _lib.call("ncn_field_bwd_mlp_part", x_, d_, n, n_dev, order_, c["packed"], prec, enc, ds, None, gr_, c["scale"],
                      part, nb, slab2, ws2, lmax2, stash)
        grad = pool.inp(torch.zeros(n_entries, 2, device=dev), name="grad_table")
        _lib.call("ncn_field_scatter", x_, n, n_dev, order_, *geo, ws, lmax, 0, 16, 0, grad)
        torch.cuda.synchronize()
        cpool.check()
        for k, t in outs.items():
            t.handle.assert_untouched(past, k)
        assert gb.same_bits(slab, slab2) and gb.same_bits(ws, ws2) and gb.same_bits(lmax[:nb], lmax2[:nb])
        outs.update(slab=slab, dE_ws=ws, level_max=lmax, grad_table=grad)
        # the table scatter accumulates with float atomics: each run meets the value test's bound
        _, dE, _ = fl._decode(ws, n, precision)
        o = np.arange(n) if order is None else order.numpy().astype(np.int64)
        x01 = (x.numpy()[o[:nv]] + np.float32(0.5)).astype(np.float32)
        ref = fl._serial_scatter(x01, dE[:nv].contiguous(), n_entries)
        _check_scatter(grad.cpu().numpy().astype(np.float64), ref, n, precision, f"guard bands count {count}",
                       order is not None)
        return outs

    out = _ab(dev, run, atomic=("grad_table",))
    t = TOL[precision]
    sig_r, rgb_r = _oracle_forward(precision, n)
    np.testing.assert_allclose(out["sigmas"][:nv].cpu().numpy(), sig_r[:nv], rtol=t["rtol"], atol=t["atol"])
    np.testing.assert_allclose(out["rgbs"][:nv].cpu().numpy(), rgb_r[:nv], atol=t["rgb"])
    np.testing.assert_allclose(out["sigmas1"][:nv].cpu().numpy(), sig_r[:nv], rtol=t["rtol"], atol=t["atol"])
    sig_err = np.abs(out["sigmas"][:nv].cpu().numpy() - sig_r[:nv]) / (t["atol"] + t["rtol"] * np.abs(sig_r[:nv]))
    rgb_err = np.abs(out["rgbs"][:nv].cpu().numpy() - rgb_r[:nv]) / t["rgb"]
    _fig(f"field fwd sigma {precision} n {n}: |err| / (atol + rtol |ref|)", float(sig_err.max()), 1.0)
    _fig(f"field fwd rgb {precision} n {n}: |err| / atol", float(rgb_err.max()), 1.0)
    if order is None:
        assert gb.same_bits(out["sigmas2"][:nv], out["sigmas1"][:nv])  # mode 2 == mode 1, bit for bit
    fl._check_header(out["dE_ws"], precision, 0 if with_order else 3)
    _, dE, pad = fl._decode(out["dE_ws"], n, precision)
    assert float(pad.abs().max()) == 0.0 if pad.numel() else True
    if nv < n:
        assert float(dE[nv:].abs().max()) == 0.0  # (never written: the workspace's zeros)
    fl._check_level_max(out["level_max"], dE, n, nv)
    ref_dE = fl._oracle_dE(precision, n)[:nv]
    if with_order:
        ref_dE = ref_dE[order.numpy().astype(np.int64)[:nv]]
    _check_dE_share(dE[:nv], ref_dE, precision, f"n {n} count {count} order {with_order}")


@pytest.mark.parametrize("with_order", [False, True], ids=["sample_order", "morton_order"])
@pytest.mark.parametrize("n,count", FIELD_CASES, ids=FIELD_IDS)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_field_input_grads(dev, precision, n, count, with_order):
    """ncn_field_bwd_mlp_din and ncn_field_bwd_dx by test_gpu_field_input_grad's check (rel-L2 per column
    <= TOL[precision]["bwd"] against its oracle reference); slab, dE_ws and level_max bit for bit
    ncn_field_bwd_mlp's; rows [count, n) of both outputs exactly zero, as the header documents."""
    L = _lib.lib()
    m = _field_model(dev, precision, 1.0)  # (ig._params() is fl._params(): the same seed)
    prec, nv = m._prec, n if count is None else count
    x, d, gs, gr = ig._case(n, 2)
    order = _field_order(m, x, n, count, dev) if with_order else None
    nb, n_de = int(L.ncn_field_bwd_blocks(n)), int(L.ncn_field_bwd_dE_floats(n))
    past = slice(nv, n)

    def run(pool):
        cpool, c = _field_consts(dev, precision, 1.0, pool.fill)
        x_, d_, n_dev, order_ = _field_args(pool, dev, x, d, n, count, order, nv)
        geo = (m._levels_ptr, m._xyz_min, m._xyz_extent)
        sig, rgb = pool.out((n,), name="sigmas"), pool.out((n, 3), name="rgbs")
        enc = pool.out((_enc_halves(n),), torch.float16, name="enc_cache")
        _lib.call("ncn_field_fwd", x_, d_, n, n_dev, order_, c["table"], *geo, c["packed"], prec, 0, sig, rgb, enc)
        gs_, gr_ = pool.inp(gs, rows=past, name="dL_dsigmas"), pool.inp(gr, rows=past, name="dL_drgbs")
        res = []
        for din in (False, True):
            slab = pool.out((nb * N_W,), name="slab")
            ws, lmax = pool.inp(torch.zeros(n_de), name="dE_ws"), pool.inp(torch.full((256, 16), -1.0), name="level_max")
            if din:
                gd = pool.out((n, 3), name="dL_ddirs")
                _lib.call("ncn_field_bwd_mlp_din", x_, d_, n, n_dev, order_, c["packed"], prec, enc, gs_, gr_, c["scale"],
                          slab, ws, lmax, c["w_master"], gd)
            else:
                _lib.call("ncn_field_bwd_mlp", x_, d_, n, n_dev, order_, c["packed"], prec, enc, gs_, gr_, c["scale"], slab,
                          ws, lmax)
            res.append((slab, ws, lmax))
        gx = pool.out((n, 3), name="dL_dxyzs")
        _lib.call("ncn_field_bwd_dx", x_, n, n_dev, order_, c["table"], *geo, ws, gx)
        torch.cuda.synchronize()
        cpool.check()
        for a, b in zip(*res):
            assert gb.same_bits(a, b)
        return {"dL_dxyzs": gx, "dL_ddirs": gd}

    out = _ab(dev, run)
    gx, gd = out["dL_dxyzs"].cpu(), out["dL_ddirs"].cpu()
    if nv < n:
        assert float(gx[nv:].abs().max()) == 0.0 and float(gd[nv:].abs().max()) == 0.0
        assert gb.same_bits(gx[nv:], torch.zeros(n - nv, 3)) and gb.same_bits(gd[nv:], torch.zeros(n - nv, 3))
    ref_x, ref_d = ig._reference(precision, n, 2)
    ex, ed = ig._col_errors(gx[:nv], ref_x[:nv]), ig._col_errors(gd[:nv], ref_d[:nv])
    _fig(f"field input grads {precision} n {n} count {count} order {with_order}: worst column rel-L2", max(ex + ed),
         TOL[precision]["bwd"])
    ig._check_columns(f"guard bands n {n} count {count} order {with_order}", precision, gx[:nv], gd[:nv], ref_x[:nv],
                      ref_d[:nv])


# ================================================================================ grid refresh
import test_gpu_grid as tg  # noqa: E402


@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "sampled"])
def test_grid_refresh(dev, warmup):
    """ncn_grid_sample -> ncn_field_fwd (mode 2, the device count) -> ncn_grid_apply -> ncn_grid_packbits at
    G = 32 by test_gpu_grid's checks.  The hit list has the capacity N (exactly full in warm-up), work
    ncn_grid_work_bytes() bytes, the bitfield N / 8 bytes.  The list's order depends on the order in
    which the workgroups reserve their slices, so the lists are compared as sets (sorted by cell)."""
    G = 32
    N = G ** 3
    m = tg._model(dev, G)
    old = tg._init_grid(m, np.random.default_rng(1 if warmup else 2))
    thr, decay, seed = (1e4, 0.95, 123) if warmup else (2.0, 0.95, 7)
    s = min(2 ** -1, m.scale)
    hg = s / G
    packed_src = m._pack_weights()
    table_src = m.flat_params()[: m._n_table].detach()
    n_work = int(_lib.lib().ncn_grid_work_bytes())

    def run(pool):
        half_fill = HALF_FILLS[0] if pool.fill != pool.fill else HALF_FILLS[1]
        table, packed = pool.inp(table_src, name="table"), pool.inp(packed_src, fill=half_fill, name="weights_packed")
        dg = pool.inp(old, name="density_grid")
        xyzs, idx, sig = pool.outs(list_xyzs=(N, 3), list_idx=((N,), torch.int32), sigmas=(N,))
        n_list = pool.inp(torch.tensor([5], dtype=torch.int32), name="n_list")
        work = pool.inp(torch.zeros(n_work, dtype=torch.uint8), name="work")
        enc = pool.out((_enc_halves(N),), torch.float16, name="enc_cache (scratch)")
        _lib.call("ncn_grid_sample", dg[0], N, G, s - hg, hg, thr, N // 4, 1 if warmup else 0, seed, decay, None, xyzs, idx,
                  n_list, work)
        _lib.call("ncn_field_fwd", xyzs, None, N, n_list, None, table, m._levels_ptr, m._xyz_min, m._xyz_extent, packed,
                  m._prec, 2, sig, None, enc)
        _lib.call("ncn_grid_apply", dg[0], idx, sig, n_list, N, decay, None)
        bf, thr_out = pool.out((N // 8,), torch.uint8, name="bitfield"), pool.out((1,), name="thr_out")
        _lib.call("ncn_grid_packbits", dg, N, thr, bf, thr_out, work)
        torch.cuda.synchronize()
        n = int(n_list)
        assert n == N if warmup else 0 < n < N
        for t in (xyzs, idx, sig):
            t.handle.assert_untouched(slice(n, N))
        by_cell = torch.argsort(idx[:n].long())
        return {"density_grid": dg, "bitfield": bf, "thr_out": thr_out, "n_list": n_list, "idx": idx[:n][by_cell],
                "xyzs": xyzs[:n][by_cell], "sigmas": sig[:n][by_cell]}

    out = _ab(dev, run)
    n = int(out["n_list"])
    hits = (n, out["idx"].cpu().numpy(), out["xyzs"].cpu().numpy(), out["sigmas"].cpu().numpy())
    new = out["density_grid"].cpu().numpy()
    tg._check_cascade(m, 0, old[0], new[0], hits, thr, decay)
    tg._check_packbits(new, thr, float(out["thr_out"]), out["bitfield"].cpu().numpy())
    if warmup:
        assert np.array_equal(hits[1], np.arange(N))
