"""The semantic / normal heads on the GPU (include/ncnerf_heads.h, csrc/heads.hip) against tests/heads_ref.py:
the head network's forward and backward, the hand-off of its dL/dh through the split backward's stash,
and the compositing of extra channels through the compositor's weights.

Tolerances.
 * Head forward, against heads_ref with the same operand emulation: relative L2 of the output <= the
   field's forward rtol (test_gpu_field.TOL: 2e-3 fp16, 2e-2 bf16), and a max-abs bound measured on
   the CPU for the very inputs of each case: 4 x the largest difference between heads_ref with fp32
   and with fp64 accumulation (the kernel sums in another order again), floored at 4 x TOL[precision]
   ["rgb"] (the accepted error of the equally deep rgb_net behind a sigmoid of slope <= 1/4).
   Measured fp32-vs-fp64 differences of the reference (CPU, these inputs, the largest over the cases):
   fp16 1.6e-4, bf16 1.1e-3 at n = 4099 (9.3e-5 and 1.5e-8 at n <= 17) on outputs of magnitude <= 0.26
   — where an operand rounds the other way under the other accumulation the output moves by far more
   than the order of the sum moves it; 4 x these stays below the floors (8e-3 / 4e-2), which bind.
 * Head backward: relative L2 of every parameter block (table, W1..W5, each head matrix) against
   autograd through heads_ref <= the field's backward bound (2e-2 / 5e-2), also per 16-row tile of the
   head matrices (field_level_check.weight_tile_errors).  The fp16 backward runs at loss scale 1
   (test_gpu_field._model_from_oracle); the reference rounds its gradients at 128 x that.
 * Extra channels: forward within the summation-order bound 2 (n - 1) 2^-24 sum|terms| per element of
   the fp64 sum.  The bound covers the order of the sum alone, so the inputs carry few mantissa bits
   (ws multiples of 2^-10, raws multiples of 2^-8 below 4): every term ws * raws is exact in fp32, as
   tests/test_gpu_geom_loss.py chooses exact addends for a one-term mean.  Backward: products of two
   such values, exact; dL/dws within the same order bound.  Against the existing compositor (6 channels
   directly vs 3 + 3 through the node): test_gpu_vren.test_composite_bw_parity's rtol 1e-3, atol
   1e-4 max|ref|."""
import functools

import numpy as np
import pytest
import torch

import heads_ref
from field_level_check import MAX_SKIPPED_TILES, weight_tile_errors
from ncnerf_amd import _lib
from ncnerf_amd.custom_functions import ExtraChannels, VolumeRenderer
from ncnerf_amd.ngp_mt import NGPMT, N_HEAD_PACKED_HALVES, head_nw
from oracle import field_ref
from test_gpu_field import TOL, _inputs

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
PRECISIONS = ["fp16", "bf16"]


@functools.lru_cache(maxsize=None)
def _field():
    return field_ref.init_params(seed=3, table_init=0.5)  # large table values exercise the encoding


@functools.lru_cache(maxsize=None)
def _head(n_out, seed):
    return heads_ref.init_head(n_out, seed)


def _model(dev, precision, n_out, W_sem, W_norm):
    """A heads-on model (sem_net with n_out classes + norm_net) holding the oracle's parameters; the
    fp16 backward at loss scale 1."""
    P, _ = _field()
    m = NGPMT(scale=0.5, grid_size=128, precision=precision, pred_sem=True, n_sem_cls=n_out, pred_norm=True).to(dev)
    if m.amp_state is not None:
        m.amp_state[0] = 1.0
    with torch.no_grad():
        flat, off = m.flat_params(), 0
        for W in [P.table, P.W1, P.W2, P.W3, P.W4, P.W5] + list(W_sem) + list(W_norm):
            flat[off:off + W.numel()].copy_(W.reshape(-1))
            off += W.numel()
        assert off == flat.numel()
    return m


@functools.lru_cache(maxsize=None)
def _reference_h(n, precision, dtype):
    """The field's reference outputs on the forward inputs, once per (n, precision, accumulation type)."""
    P, levels = _field()
    x, d = _inputs(n, 1)
    Pd = field_ref.FieldParams(*[t.to(dtype) for t in P.tensors()])
    with torch.no_grad():
        return field_ref.field_forward_autograd(x.to(dtype), d.to(dtype), Pd, levels, emulate=precision)


def _reference_out(n, precision, n_out, seed, dtype):
    with torch.no_grad():
        h = _reference_h(n, precision, dtype)[2]
        return heads_ref.head_forward(h, [w.to(dtype) for w in _head(n_out, seed)], n_out, emulate=precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_out", [3, 16, 17, 40])
@pytest.mark.parametrize("n", [1, 17, 4099])
def test_head_forward(dev, n, n_out, precision):
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d = _inputs(n, 1)
    with torch.no_grad():
        out = m(x.to(dev), d.to(dev))
    t = TOL[precision]
    for key, k, seed in (("sems", n_out, 11), ("norms", 3, 12)):
        got = out[key].cpu().double()
        ref32, ref64 = _reference_out(n, precision, k, seed, torch.float32), _reference_out(n, precision, k, seed, torch.float64)
        assert got.shape == (n, k)
        measured = float((ref32.double() - ref64).abs().max())
        bound = max(4 * measured, 4 * t["rgb"])
        err = float((got - ref32.double()).abs().max())
        rel = float((got - ref32.double()).norm() / ref32.double().norm())
        print(f"head forward {key} n {n} n_out {k} {precision}: max-abs {err:.3e} (bound {bound:.3e}, reference "
              f"fp32 vs fp64 {measured:.3e}), rel-L2 {rel:.3e}")
        assert rel <= t["rtol"], (key, rel)
        assert err <= bound, (key, err, bound)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_leave_the_field_outputs_alone(dev, precision):
    """sigmas / rgbs of a heads-on model equal a heads-off model with the same weights bit for bit, and
    density(x, return_feat=True) returns the features h (sigma_net's fp32 accumulators: sigma = exp(h0))."""
    P, _ = _field()
    m = _model(dev, precision, 5, _head(5, 11), _head(3, 12))
    m0 = NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev)
    with torch.no_grad():
        m0.flat_params().copy_(m.flat_params()[:m0.flat_params().numel()])
    x, d = _inputs(4099, 1)
    with torch.no_grad():
        a, b = m(x.to(dev), d.to(dev)), m0(x.to(dev), d.to(dev))
        sig, h = m.density(x.to(dev), return_feat=True)
    assert torch.equal(a["sigmas"], b["sigmas"]) and torch.equal(a["rgbs"], b["rgbs"])
    assert torch.equal(sig, b["sigmas"]) and h.shape == (4099, 16) and h.dtype == torch.float32
    href = _reference_h(4099, precision, torch.float32)[2]
    t = TOL[precision]
    np.testing.assert_allclose(h.cpu().numpy(), href.numpy(), rtol=t["rtol"], atol=4 * t["rgb"])


def _direct_forward(m, x, d, n_dev, n_out, out):
    _, _, enc, packed, _ = m._field_fwd(x, d, n_dev, 0, True)
    _lib.call("ncn_head_fwd", enc, x.shape[0], n_dev, packed, m._head_packed["sem_net"], n_out, m._prec, out)
    return enc, packed


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_forward_device_count(dev, precision):
    """Capacity 4099 with *n_dev = 1000: rows < 1000 equal an n = 1000 run bit for bit, rows >= 1000 keep
    a NaN sentinel."""
    n_out = 17
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d = (t.to(dev) for t in _inputs(4099, 1))
    full = torch.full((4099, n_out), float("nan"), device=dev)
    _direct_forward(m, x, d, torch.tensor([1000], dtype=torch.int32, device=dev), n_out, full)
    part = torch.full((1000, n_out), float("nan"), device=dev)
    _direct_forward(m, x[:1000].contiguous(), d[:1000].contiguous(), None, n_out, part)
    assert torch.isfinite(part).all() and torch.equal(full[:1000], part)
    assert torch.isnan(full[1000:]).all()


def test_head_arguments_out_of_range(dev):
    """n_out outside [1, 48] and an unknown precision are hipErrorInvalidValue (1), before any launch."""
    buf = torch.zeros(N_HEAD_PACKED_HALVES, dtype=torch.float16, device=dev)
    w = torch.zeros(head_nw(48), device=dev)
    for n_out, prec in ((0, 0), (49, 0), (3, 2)):
        with pytest.raises(_lib.NcnError, match=r"hipError 1\)"):
            _lib.call("ncn_head_pack_weights", w, n_out, buf, prec)
        with pytest.raises(_lib.NcnError, match=r"hipError 1\)"):
            _lib.call("ncn_head_fwd", buf, 16, None, buf, buf, n_out, prec, w)
    with pytest.raises(_lib.NcnError, match=r"hipError 1\)"):
        _lib.call("ncn_composite_extra_fw", w, w, torch.zeros(1, 3, dtype=torch.int64, device=dev), 1, 4, 52, w)
    m = NGPMT(scale=0.5, grid_size=128, pred_norm=True).to(dev)
    m.sort_samples = True
    with pytest.raises(NotImplementedError, match="sort_samples"):
        m(torch.zeros(16, 3, device=dev), torch.ones(16, 3, device=dev))


def _blocks(m, n_out):
    """(name, shape) of every parameter block of the flat buffers, in their order."""
    P, _ = _field()
    blocks = [(n, tuple(t.shape)) for n, t in zip(("table", "W1", "W2", "W3", "W4", "W5"), P.tensors())]
    for head, k in (("sem", n_out), ("norm", 3)):
        blocks += [(f"{head}.{w}", s) for w, s in zip(("Wa", "Wb", "Wc"), heads_ref.head_shapes(k))]
    return blocks


def _run_backward(m, x, d, ups, dev):
    m.flat_grad().zero_()
    out = m(x.to(dev), d.to(dev))
    loss = None
    for key, g in ups.items():
        if g is not None:
            term = (out[key] * g.to(dev)).sum()
            loss = term if loss is None else loss + term
    loss.backward()
    torch.cuda.synchronize()
    return m.flat_grad().detach().cpu().clone()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_out", [3, 17, 40])
@pytest.mark.parametrize("n", [17, 4099])
def test_head_backward(dev, n, n_out, precision):
    P, levels = _field()
    W_sem, W_norm = _head(n_out, 11), _head(3, 12)
    m = _model(dev, precision, n_out, W_sem, W_norm)
    x, d = _inputs(n, 2)
    g = torch.Generator().manual_seed(9)
    ups = {"sigmas": torch.randn(n, generator=g), "rgbs": torch.randn(n, 3, generator=g),
           "sems": torch.randn(n, n_out, generator=g), "norms": torch.randn(n, 3, generator=g)}
    gflat = _run_backward(m, x, d, ups, dev)
    # the reference: autograd through heads_ref, the gradients rounded at the chain's scale
    Pt = field_ref.FieldParams(*[t.clone().requires_grad_(True) for t in P.tensors()])
    Ws = [[w.clone().requires_grad_(True) for w in W] for W in (W_sem, W_norm)]
    sig, rgb, (sems, norms) = heads_ref.forward_with_heads(x, d, Pt, levels, [(Ws[0], n_out), (Ws[1], 3)], emulate=precision,
                                                           bwd_scale=128.0 if precision == "fp16" else 1.0)
    ((sig * ups["sigmas"]).sum() + (rgb * ups["rgbs"]).sum() + (sems * ups["sems"]).sum()
     + (norms * ups["norms"]).sum()).backward()
    refs = [t.grad for t in Pt.tensors()] + [w.grad for W in Ws for w in W]
    bound, off, errs = TOL[precision]["bwd"], 0, {}
    for (name, shape), ref in zip(_blocks(m, n_out), refs):
        k = ref.numel()
        got = gflat[off:off + k].reshape(ref.shape)
        off += k
        errs[name] = float((got - ref).norm() / ref.norm().clamp_min(1e-12))
        if "." in name:  # a head matrix: the same bound per 16-row tile
            tiles, skipped = weight_tile_errors(got.numpy(), ref.numpy())
            print(f"head backward n {n} n_out {n_out} {precision} {name} rel-L2 per 16-row tile:",
                  " ".join(f"{t_}:{e:.2e}" for t_, e in tiles.items()), "skipped:", skipped)
            assert len(skipped) <= MAX_SKIPPED_TILES, (name, skipped)
            assert all(e <= bound for e in tiles.values()), (name, tiles)
    assert off == gflat.numel()
    print(f"head backward n {n} n_out {n_out} {precision} rel-L2 per block:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e <= bound for e in errs.values()), errs
    # rows >= n_out of the last head matrices: parameters without a gradient
    sem_off = m._heads[0][2] + 5120
    wc = gflat[sem_off:sem_off + 64 * 16 * ((n_out + 15) // 16)].reshape(-1, 64)
    assert float(wc[:n_out].abs().max()) > 0
    assert wc.shape[0] == n_out or float(wc[n_out:].abs().max()) == 0.0
    norm_wc = gflat[m._heads[1][2] + 5120:].reshape(16, 64)
    assert float(norm_wc[3:].abs().max()) == 0.0 and float(norm_wc[:3].abs().max()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_gradient_reaches_the_field_through_the_stash(dev, precision):
    """With no upstream gradient on sigma and rgb, the gradients of W3..W5 are exactly 0 while the table's,
    W1's and W2's are not: the heads' dL/dh arrives through the stash between the two MLP parts.  The
    heads' own gradients of two runs are bit-identical."""
    n, n_out = 4099, 17
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d = _inputs(n, 2)
    g = torch.Generator().manual_seed(10)
    ups = {"sems": torch.randn(n, n_out, generator=g), "norms": torch.randn(n, 3, generator=g)}
    runs = [_run_backward(m, x, d, ups, dev) for _ in range(2)]
    nt = m._n_table
    g0 = runs[0]
    assert float(g0[nt + 3072:nt + 10240].abs().max()) == 0.0  # W3, W4, W5
    for a, b in ((0, nt), (nt, nt + 2048), (nt + 2048, nt + 3072)):  # table, W1, W2
        assert float(g0[a:b].abs().max()) > 0 and torch.isfinite(g0[a:b]).all()
    # (the heads' own blocks only: the table's gradient is flushed with float atomics, and W1 / W2, which
    # receive the hand-off through part 2, leave through the field's slab reduction, whose chunk
    # partials are added with float atomics too: equal up to summation order, as between any two runs)
    assert torch.equal(runs[0][nt + 10240:], runs[1][nt + 10240:])
    # the hand-off alone: against the reference with the same upstream gradients
    P, levels = _field()
    Pt = field_ref.FieldParams(*[t.clone().requires_grad_(True) for t in P.tensors()])
    _, _, (sems, norms) = heads_ref.forward_with_heads(x, d, Pt, levels, [(_head(n_out, 11), n_out), (_head(3, 12), 3)],
                                                       emulate=precision, bwd_scale=128.0 if precision == "fp16" else 1.0)
    ((sems * ups["sems"]).sum() + (norms * ups["norms"]).sum()).backward()
    for name, a, b, ref in (("table", 0, nt, Pt.table.grad), ("W1", nt, nt + 2048, Pt.W1.grad),
                            ("W2", nt + 2048, nt + 3072, Pt.W2.grad)):
        rel = float((g0[a:b] - ref.reshape(-1)).norm() / ref.norm())
        print(f"stash hand-off {precision} {name}: rel-L2 {rel:.2e}")
        assert rel <= TOL[precision]["bwd"], (name, rel)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_backward_kernel_is_deterministic(dev, precision):
    """ncn_head_bwd twice on copies of one stash: the slab rows and the stash are bit-identical, and the
    groups past the device count are left alone."""
    n, n_dev, n_out = 4099, 3000, 40
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d = (t.to(dev) for t in _inputs(n, 2))
    L = _lib.lib()
    cnt = torch.tensor([n_dev], dtype=torch.int32, device=dev)
    _, _, enc, packed, _ = m._field_fwd(x, d, cnt, 0, True)
    g = torch.Generator(device=dev).manual_seed(3)
    stash0 = torch.zeros(int(L.ncn_field_bwd_stash_floats(n)), device=dev)
    stash0[-16 * ((n + 15) // 16):] = torch.randn(16 * ((n + 15) // 16), device=dev, generator=g)
    up = torch.randn(n, n_out, device=dev, generator=g)
    nb, n_w = int(L.ncn_head_bwd_blocks(n)), head_nw(n_out)
    res = []
    for _ in range(2):
        stash, slab = stash0.clone(), torch.full((nb * n_w,), float("nan"), device=dev)
        _lib.call("ncn_head_bwd", enc, n, cnt, packed, m._head_packed["sem_net"], n_out, m._prec, up, m._bwd_loss_scale(),
                  slab, stash)
        res.append((stash, slab))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])
    stash, slab = res[0]
    assert torch.isfinite(slab).all()  # every element of every slab row is written
    groups, live = (n + 15) // 16, (n_dev + 15) // 16
    tiles = stash[:128 * groups].view(groups, 128)
    assert float(tiles[:live].abs().max()) > 0 and float(tiles[live:].abs().max()) == 0.0
    h0, h0_before = stash[128 * groups:].view(groups, 16), stash0[128 * groups:].view(groups, 16)
    assert torch.equal(h0[live:], h0_before[live:]) and not torch.equal(h0[:live], h0_before[:live])


# ---------------------------------------------------------------- extra channels
def _segments(counts, seed, lead=3, gap=5, tail=37):
    """Hand-built rays: `counts` samples each, in shuffled row order, `lead` unused rows in front, a gap of
    unused rows between two segments and a capacity tail behind the last.  -> rays_a (R, 3) int64, the row
    count S, the used mask."""
    rng = np.random.default_rng(seed)
    R = len(counts)
    rays_a, start = np.zeros((R, 3), np.int64), lead
    for ray in rng.permutation(R):
        rays_a[ray] = (ray, start, counts[ray])
        start += counts[ray] + gap
    S = start + tail
    used = np.zeros(S, bool)
    for _, s, c in rays_a:
        used[s:s + c] = True
    return rays_a[rng.permutation(R)], S, used


def _exact_inputs(rays_a, S, used, C, seed):
    """ws multiples of 2^-10 in [0, 1) with a zero tail in every longer ray (early termination), raws
    multiples of 2^-8 in [-4, 4): every product is exact in fp32.  Unused rows are NaN."""
    rng = np.random.default_rng(seed)
    ws = (rng.integers(0, 1024, S) / 1024.0).astype(np.float32)
    raws = (rng.integers(-1024, 1024, (S, C)) / 256.0).astype(np.float32)
    for _, s, c in rays_a:
        if c > 8:
            ws[s + int(0.7 * c):s + c] = 0.0
    ws[~used], raws[~used] = np.nan, np.nan
    return ws, raws


COUNTS = [0, 1, 63, 65, 300, 64, 700, 0, 2, 129]


@pytest.mark.parametrize("C", [1, 3, 43, 51])
@pytest.mark.parametrize("counts", [COUNTS, [40], [0]], ids=["ragged", "one_ray", "one_empty_ray"])
def test_extra_channels(dev, counts, C):
    rays_a, S, used = _segments(counts, 4)
    ws, raws = _exact_inputs(rays_a, S, used, C, 5)
    R = len(counts)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ws_d, raws_d = T(ws).requires_grad_(True), T(raws).requires_grad_(True)
    rend = ExtraChannels.apply(ws_d, raws_d, T(rays_a))
    ref, mag, cnt = heads_ref.composite_extra(ws, raws, rays_a, R)
    got = rend.detach().cpu().numpy().astype(np.float64)
    assert got.shape == (R, C) and np.isfinite(got).all()  # NaN rows outside every ray change nothing
    bound = 2.0 * np.maximum(cnt - 1, 0)[:, None] * U * mag
    assert np.all(np.abs(got - ref) <= bound), float(np.max(np.abs(got - ref) - bound))
    assert np.all(got[cnt == 0] == 0.0)
    # backward: upstream multiples of 2^-6 (exact products again)
    rng = np.random.default_rng(6)
    up = (rng.integers(-256, 256, (R, C)) / 64.0).astype(np.float32)
    rend.backward(T(up))
    dws_ref, draws_ref = heads_ref.composite_extra_bw(up, np.nan_to_num(ws), np.nan_to_num(raws), rays_a)
    dws, draws = ws_d.grad.cpu().numpy().astype(np.float64), raws_d.grad.cpu().numpy().astype(np.float64)
    assert np.all(dws[~used] == 0.0) and np.all(draws[~used] == 0.0)
    assert np.array_equal(draws[used], draws_ref[used])
    terms = np.abs(np.nan_to_num(raws).astype(np.float64) * up[_ray_of(rays_a, S)].astype(np.float64)).sum(1)
    assert np.all(np.abs(dws - dws_ref)[used] <= (2.0 * (C - 1) * U * terms)[used])
    # two runs are bit-identical
    again = ExtraChannels.apply(ws_d.detach(), raws_d.detach(), T(rays_a))
    assert torch.equal(again, rend.detach())


def _ray_of(rays_a, S):
    ray = np.zeros(S, np.int64)
    for r, s, c in rays_a:
        ray[s:s + c] = r
    return ray


@pytest.mark.parametrize("with_dws", [False, True])
def test_extra_channels_against_the_compositor(dev, with_dws):
    """6 channels composited directly by VolumeRenderer (forward and backward, dL/dws included) against 3
    through it plus 3 through the node: rend, dL/dsigma and dL/draws agree."""
    counts = [0, 1, 63, 65, 300, 17, 700, 5, 128, 256, 31, 90]
    rays_a, S, used = _segments(counts, 7, lead=0, gap=0, tail=0)  # (the compositor writes every row it is given)
    rng = np.random.default_rng(8)
    R = len(counts)
    scale = np.where(np.arange(R) % 2 == 0, 400.0, 20.0)[_ray_of(rays_a, S)]  # every other ray terminates early
    sig = np.abs(rng.normal(0, 1, S) * scale).astype(np.float32)
    raws = rng.random((S, 6), dtype=np.float32)
    deltas = np.full(S, 1.7e-3, np.float32)
    ts = np.zeros(S, np.float32)
    for _, s, c in rays_a:
        ts[s:s + c] = 0.05 + 1.7e-3 * np.arange(c)
    ups = [rng.normal(size=R).astype(np.float32), rng.normal(size=R).astype(np.float32),
           rng.normal(size=(R, 6)).astype(np.float32), rng.normal(size=S).astype(np.float32) if with_dws else None]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ra, de, tt = T(rays_a), T(deltas), T(ts)

    def run(split):
        s, r = T(sig).requires_grad_(True), T(raws).requires_grad_(True)
        if split:
            _, op, dep, rend3, ws = VolumeRenderer.apply(s, r[:, :3].contiguous(), de, tt, ra, 1e-4)
            rend = torch.cat((rend3, ExtraChannels.apply(ws, r[:, 3:].contiguous(), ra)), dim=-1)
        else:
            _, op, dep, rend, ws = VolumeRenderer.apply(s, r, de, tt, ra, 1e-4)
        loss = (op * T(ups[0])).sum() + (dep * T(ups[1])).sum() + (rend * T(ups[2])).sum()
        if with_dws:
            loss = loss + (ws * T(ups[3])).sum()
        loss.backward()
        return [t.detach().cpu().numpy() for t in (rend, ws, s.grad, r.grad)]

    direct, split = run(False), run(True)
    assert float(np.mean(direct[1] == 0)) > 0.2  # (early termination: a zero tail of ws)
    for a, r, name in zip(split, direct, ("rend", "ws", "dL_dsigmas", "dL_draws")):
        np.testing.assert_allclose(a, r, rtol=1e-3, atol=1e-4 * np.abs(r).max(), err_msg=name)
