"""The field backward per level and at the faces of the scene box.

1. The MLP pass (ncn_field_bwd_mlp) against the emulating oracle (oracle/field_ref.py with the
   backward's rounding at the kernel's scale, bwd_scale = 128 x the loss scale; 1 for bf16): the
   encoding gradient dE decoded from the workspace the scatter reads, per level, by the outlier rule
   of tests/field_level_check.py (|got - ref| > 8 u |ref| + 0.08 u rms_l), outlier share <= 2 % on
   every level.  The cap is a condition, not a measurement: ~6x the reference's own fp32-against-fp64
   share (<= 0.35 %, tests/test_oracle_field_levels.py; the kernel's fp32 accumulation order and fast
   exp / sigmoid differ from both oracle runs) and 50x below what a 1 % (fp16) / 5 % (bf16) error on
   a level produces.  level_max equals the maximum of the stored values bit for bit (it sets the
   scatter's 64-bit fixed-point scale: too small overflows silently, too large loses bits), samples
   past the device count touch nothing, and the header is {1 / S, operand type, class mask 3 (0 in
   a processing order), 0} with the unit queue zeroed.
2. Composition: ncn_field_scatter on the workspace the MLP pass really wrote (header mask 3: the
   coarse classes read the permuted positions, the fine ones the strided ones) against the oracle's
   serial scatter of the decoded dE, by test_gpu_scatter_units._check's criteria (rel-L2 <= 1e-6,
   max |diff| <= 1e-5 of the largest entry, non-zero sets equal to 1e-4), on interior positions and on
   the edge set E (field_level_check.place_edges: the box's corners and face centres, one ulp inside
   and outside every face, 0.1 outside — a negative floor, px = 0xFFFFFFFF, the scatter's
   out-of-key-range branch — cell boundaries of levels 0, 5 and 10, and runs of 600 equal positions),
   and the scatter alone (test_gpu_scatter_units.scatter_case) on E in both layouts and in a
   processing order.
3. The forward on E: NGPMT.forward / .density against the oracle (test_gpu_field.TOL), the
   level-split density mode 2 equal to mode 1 bit for bit, ncn_field_sort_windows against the host's
   clipped Morton keys.

4. Finding (fixed in csrc/field_scatter.h sc_push_run): the cell key of (2047, 2047, 1023) equalled the LDS
   table's empty marker; test_scatter_cell_whose_key_is_the_empty_marker is its regression.

Measured (profiles/round7/field_levels_test.log), worst over the cases, next to the bound:
  dE outlier share, worst level     fp16 0.02 %   bf16 0.02 %                      (cap 2 %)
  composition, interior             rel-L2 5.0e-8, max |diff| / max 2.0e-7, 0 one-sided non-zeros
  composition, edge set             rel-L2 5.1e-7, max |diff| / max 1.1e-6, 11 of 566 683 one-sided
  scatter alone, edge set           rel-L2 4.2e-7, max |diff| / max 9.1e-7, 4 of 443 946 one-sided
                                    (bounds: 1e-6, 1e-5, 1e-4 of the non-zero entries)
(the edge set's one-sided entries: corners whose trilinear weight is a product of two one-ulp
fractions, ~2^-48 — below the fixed-point scale's last bit, kept by the oracle's f32 sum; the
oracle's own f32 serial sum is 4.2e-7 / 1.6e-6 away from an f64 sum on these positions.)
Each of the statements the edge set is there for (the dense `% params` corner in encode_level,
sc_corner_entry and sc_corner_entries, the scatter's out-of-key-range adds, level_max) was changed on
its own in a scratch build: the tests of that path here fail.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import field_ref
from field_level_check import outlier_mask, outlier_share, place_edges
from ncnerf_amd import _lib
from ncnerf_amd.ngp_mt import ENC_BYTES, N_W
from test_gpu_field import TOL, _inputs, _model_from_oracle, check_window_order
from test_gpu_scatter_units import _check, _ray_samples, scatter_case

pytestmark = pytest.mark.gpu

LOSS_SCALE = 4.0  # fp16: a GradScaler scale other than 1 (S = 4 x 128 in the kernel's chain)
SHARE_CAP = 0.02
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _bwd_scale(precision):
    return LOSS_SCALE * 128.0 if precision == "fp16" else 1.0


def _upstream(n):
    g = torch.Generator().manual_seed(9)
    return torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


@functools.lru_cache(maxsize=None)
def _params():
    return field_ref.init_params(seed=5, table_init=0.5)


@functools.lru_cache(maxsize=None)
def _oracle_dE(precision, n):
    """dL/denc (n, 32) of the emulating oracle at the section's inputs (computed once per case)."""
    P, levels = _params()
    x, d = _inputs(n, 2)
    gs, gr = _upstream(n)
    sig, rgb, _, enc = field_ref.field_forward_autograd(x, d, P, levels, emulate=precision,
                                                        bwd_scale=_bwd_scale(precision), return_enc=True)
    ((sig * gs).sum() + (rgb * gr).sum()).backward()
    g = enc.grad.numpy().copy()
    g.setflags(write=False)
    return g


def _model(dev, precision):
    return _model_from_oracle(_params()[0], dev, precision, loss_scale=LOSS_SCALE)


def _sort_windows(m, x):
    n = x.shape[0]
    order = torch.empty(n, dtype=torch.int32, device=x.device)
    assert _lib.call("ncn_field_sort_windows", x, n, None, m._xyz_min, m._xyz_extent, order) == 0
    return order


def _mlp_pass(m, x, d, dsig, drgb, n_dev=None, order=None, ws=None):
    """ncn_field_fwd (mode 0, with the encoding cache) then ncn_field_bwd_mlp on device tensors.
    Returns (the dE workspace, level_max [256][16] with untouched rows at -1, sigmas, rgbs)."""
    n = x.shape[0]
    dev = x.device
    L = _lib.lib()
    packed = m._pack_weights()
    table = m.flat_params()[: m._n_table]
    sig = torch.zeros(n, device=dev)
    rgb = torch.zeros(n, 3, device=dev)
    enc = torch.zeros(((n + 15) // 16) * 16 * ENC_BYTES // 2, dtype=torch.float16, device=dev)
    _lib.call("ncn_field_fwd", x, d, n, n_dev, order, table, m._levels_ptr,
              m._xyz_min, m._xyz_extent, packed, m._prec, 0, sig, rgb, enc)
    nb = int(L.ncn_field_bwd_blocks(n))
    slab = torch.empty(nb * N_W, device=dev)
    if ws is None:
        ws = torch.zeros(int(L.ncn_field_bwd_dE_floats(n)), device=dev)
        ws[-32:] = 7.0  # (the unit queue: the MLP pass must zero it)
    lmax = torch.full((256, 16), -1.0, device=dev)
    _lib.call("ncn_field_bwd_mlp", x, d, n, n_dev, order, packed, m._prec, enc,
              dsig, drgb, m._bwd_loss_scale(), slab, ws, lmax)
    torch.cuda.synchronize()
    return ws, lmax, sig, rgb


def _decode(ws, n, precision):
    """The workspace as the scatter reads it (csrc/field_de_ws.h; field_bwd_mlp.h field_bwd_kernel / field_scatter.h ScDE): a header of 4
    floats {1 / S, operand type, class mask, -}, then [16][n_stride] pairs of the operand type,
    n_stride = (n + 3) & ~3; the pairs times 1 / S (a power of two: exact).
    -> (header (4,) f32, dE (n, 32) f32 level-major pairs, the padding pairs (16, n_stride - n, 2))."""
    w = ws.cpu()
    n_stride = (n + 3) & ~3
    hdr = w[:4].clone()
    pairs = w[4:4 + 16 * n_stride].view(TDT[precision]).view(16, n_stride, 2).float() * hdr[0]
    return hdr, pairs[:, :n].permute(1, 0, 2).reshape(n, 32).contiguous(), pairs[:, n:]


def _check_header(ws, precision, mask):
    hdr = ws[:4].cpu()
    assert float(hdr[0]) == 1.0 / _bwd_scale(precision)  # exactly: S is a power of two
    assert float(hdr[1]) == (0.0 if precision == "fp16" else 1.0)
    assert float(hdr[2]) == float(mask)
    assert int(ws[-32:].view(torch.int32).abs().sum()) == 0  # the scatter's unit queue


def _check_level_max(lmax, dE, n, n_valid=None):
    """amax over the launched workgroups' rows == max |decoded dE| per level, bit for bit; rows past
    the launched grid untouched."""
    nb = int(_lib.lib().ncn_field_bwd_blocks(n))
    lm = lmax.cpu()
    assert bool((lm[:nb] >= 0).all()) and bool((lm[nb:] == -1.0).all())
    want = dE[:n_valid].reshape(-1, 16, 2).abs().amax(dim=(0, 2))
    got = lm[:nb].amax(0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got, want)
    assert bool(torch.isfinite(got).all()) and bool((got > 0).all())
    return got


def _check_dE(dE, ref, precision, tag):
    share = outlier_share(dE.numpy(), ref, precision)
    print(f"dE outlier share per level (%) {tag} {precision}:", " ".join(f"{100 * s:.2f}" for s in share),
          f"| worst {100 * share.max():.2f}")
    if share.max() > SHARE_CAP:  # which elements: a whole level / feature would be a bug, not rounding
        bad = outlier_mask(dE.numpy(), ref, precision)
        print("  outliers per feature column:", bad.sum(0).tolist())
        print("  samples with > 8 outliers:", np.nonzero(bad.sum(1) > 8)[0][:32].tolist())
    assert share.max() <= SHARE_CAP, share


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_mlp_pass_dE_and_level_max_vs_oracle(dev, precision):
    n = 3000
    m = _model(dev, precision)
    x, d = _inputs(n, 2)
    gs, gr = _upstream(n)
    x, d, gs, gr = x.to(dev), d.to(dev), gs.to(dev), gr.to(dev)
    ref = _oracle_dE(precision, n)
    ws, lmax, sig, rgb = _mlp_pass(m, x, d, gs, gr)
    _check_header(ws, precision, 3)
    hdr, dE, pad = _decode(ws, n, precision)
    assert float(pad.abs().max()) == 0.0 if pad.numel() else True
    _check_level_max(lmax, dE, n)
    _check_dE(dE, ref, precision, f"n {n}")

    # a device count below the capacity: the samples past it are neither read nor written
    nv = n - 7
    n_dev = torch.tensor([nv], dtype=torch.int32, device=dev)
    ws1, lmax1, _, _ = _mlp_pass(m, x, d, gs, gr, n_dev=n_dev)
    _check_header(ws1, precision, 3)
    _, dE1, _ = _decode(ws1, n, precision)
    assert float(dE1[nv:].abs().max()) == 0.0  # (never written: the workspace's zeros)
    assert torch.equal(dE1[:nv], dE[:nv])  # (a sample's arithmetic does not depend on the count)
    lm1 = _check_level_max(lmax1, dE1, n, nv)
    _check_dE(dE1[:nv], ref[:nv], precision, f"n {n} n_dev {nv}")
    gs_p, gr_p = gs.clone(), gr.clone()
    gs_p[nv:] = 1e4
    gr_p[nv:] = 1e4
    ws2, lmax2, _, _ = _mlp_pass(m, x, d, gs_p, gr_p, n_dev=n_dev)
    _, dE2, _ = _decode(ws2, n, precision)
    assert torch.equal(dE2, dE1)
    assert torch.equal(_check_level_max(lmax2, dE2, n, nv), lm1)
    assert torch.equal(lmax2, lmax1)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_mlp_pass_in_processing_order(dev, precision):
    """n = 4099 (two Morton windows): dE is written in the processing order, so position p holds
    sample order[p]'s gradient; the header's class mask is 0 (the scatter gathers the positions
    itself), also on a workspace whose last call ran without an order (mask 3)."""
    n = 4099
    m = _model(dev, precision)
    x, d = _inputs(n, 2)
    gs, gr = _upstream(n)
    x, d, gs, gr = x.to(dev), d.to(dev), gs.to(dev), gr.to(dev)
    ref = _oracle_dE(precision, n)
    ws, lmax, sig0, rgb0 = _mlp_pass(m, x, d, gs, gr)
    _check_header(ws, precision, 3)
    _, dE0, _ = _decode(ws, n, precision)
    _check_level_max(lmax, dE0, n)
    _check_dE(dE0, ref, precision, f"n {n}")
    order = _sort_windows(m, x)
    o = order.cpu().numpy().astype(np.int64)
    check_window_order(o, x.cpu().numpy(), m._xyz_min, m._xyz_extent)
    assert not np.array_equal(o, np.arange(n))
    ws[-32:] = 7.0
    ws1, lmax1, sig1, rgb1 = _mlp_pass(m, x, d, gs, gr, order=order, ws=ws)  # (the same workspace)
    assert ws1.data_ptr() == ws.data_ptr()
    _check_header(ws1, precision, 0)
    _, dE1, _ = _decode(ws1, n, precision)
    assert torch.equal(sig0, sig1) and torch.equal(rgb0, rgb1)  # (the outputs stay in sample order)
    assert torch.equal(dE1, dE0[torch.from_numpy(o)])  # (the same per-sample arithmetic, permuted)
    _check_level_max(lmax1, dE1, n)
    _check_dE(dE1, ref[o], precision, f"n {n} order")


def _edge_positions(n, seed=11):
    levels = field_ref.grid_levels(0.5)[0]
    fill = (_ray_samples(n, seed=seed) - np.float32(0.5)).astype(np.float32)
    xw, mark = place_edges(fill, levels)
    assert mark[0] and mark[n - 1] and (n <= 4096 or (mark[4095] and mark[4096]))
    return xw


def _serial_scatter(x01, dE, n_table):
    ctx = type("Ctx", (), {"saved_tensors": (torch.from_numpy(x01),), "levels": field_ref.grid_levels(0.5)[0],
                           "n_table": (n_table, 2)})()
    return field_ref._HashEncodeC.backward(ctx, dE)[1].numpy().astype(np.float64)


@pytest.mark.parametrize("positions", ["interior", "edges"])
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_scatter_on_the_mlp_pass_workspace(dev, precision, positions):
    n = 2 * 4096 + 5
    m = _model(dev, precision)
    x, d = _inputs(n, 2)
    if positions == "edges":
        x = torch.from_numpy(_edge_positions(n))
    gs, gr = _upstream(n)
    xd, d, gs, gr = x.to(dev), d.to(dev), gs.to(dev), gr.to(dev)
    ws, lmax, sig, rgb = _mlp_pass(m, xd, d, gs, gr)
    assert bool(torch.isfinite(sig).all()) and bool(torch.isfinite(rgb).all())
    _check_header(ws, precision, 3)  # the coarse classes' permuted positions, as the training step's pass writes
    _, dE, _ = _decode(ws, n, precision)
    _check_level_max(lmax, dE, n)
    grad = torch.zeros(m._n_table // 2, 2, device=dev)
    rc = _lib.call("ncn_field_scatter", xd, n, None, None, m._levels_ptr, m._xyz_min,
                   m._xyz_extent, ws, lmax, 0, 16, 0, grad)
    assert rc == 0, _lib.lib().ncn_last_error()
    torch.cuda.synchronize()
    assert float(ws[2]) == 3.0
    assert int(ws[-32:].view(torch.int32).abs().sum()) == 0  # the unit queue is left zero
    x01 = (x.numpy() + np.float32(0.5)).astype(np.float32)  # (x - xyz_min) * (1 / extent), extent 1
    ref = _serial_scatter(x01, dE, m._n_table // 2)
    _check(grad.cpu().numpy().astype(np.float64), ref, n, precision, f"mlp-pass workspace, {positions}", "mask 3")


@pytest.mark.parametrize("op,with_order,mode", [("fp16", False, "unit"), ("bf16", False, "unit"), ("fp16", True, "unit"),
                                                ("fp16", False, "inf")])
def test_scatter_alone_on_the_edge_set(dev, op, with_order, mode):
    """test_scatter_matches_serial_oracle's body (a fabricated workspace, header masks 0 and 15; or a
    processing order) with the edge set as positions.  mode "inf": an overflowed pair on level 0 —
    the whole level then goes straight to global memory through sc_add, the only caller of the dense
    form of sc_corner_entries (the levels sc_add otherwise serves are hashed), here with its boundary
    corner."""
    n = 2 * 4096 + 5
    scatter_case(dev, n, op, mode, xw=_edge_positions(n), with_order=with_order, inf_level=0)


def test_scatter_cell_whose_key_is_the_empty_marker(dev):
    """The coarse levels key a run by its cell, px | py << 11 | pz << 22, and 0xFFFFFFFF marks an empty
    way of the LDS table: cell (2047, 2047, 1023) — 16 box widths outside on level 9, 136 on level 0 —
    must not be keyed (it would be "found" in any empty way: its sums added to a slot that is never
    flushed, lost, and left behind for the slot's next owner).  A run of four samples in that cell
    of every coarse level, twice; the criteria of the scatter test (before the fix: rel-L2 3.7e-2, 48
    entries on one side only)."""
    n = 2 * 4096 + 5
    levels = field_ref.grid_levels(0.5)[0]
    xw = (_ray_samples(n, seed=3) - np.float32(0.5)).astype(np.float32)
    for l in range(10):
        s = float(np.float32(levels[l]["scale"]))
        p = (np.array([2047.3, 2047.3, 1023.3]) / s - 0.5).astype(np.float32)
        pos = np.float32(s) * (p + np.float32(0.5)) + np.float32(0.5)
        assert np.array_equal(np.floor(pos), [2047, 2047, 1023])
        for at in (64 + 8 * l, 4090 + 8 * l):
            xw[at:at + 4] = p
    scatter_case(dev, n, "fp16", "unit", xw=xw)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_forward_on_the_edge_set(dev, precision):
    n = 4099
    P, levels = _params()
    m = _model(dev, precision)
    x = torch.from_numpy(_edge_positions(n))
    _, d = _inputs(n, 1)
    with torch.no_grad():
        out = m(x.to(dev), d.to(dev))
        sig_d = m.density(x.to(dev))
    sig, rgb, _ = field_ref.field_forward(x, d, P, levels, emulate=precision)
    t = TOL[precision]
    np.testing.assert_allclose(out["sigmas"].cpu().numpy(), sig.numpy(), rtol=t["rtol"], atol=t["atol"])
    np.testing.assert_allclose(out["rgbs"].cpu().numpy(), rgb.numpy(), atol=t["rgb"])
    np.testing.assert_allclose(sig_d.cpu().numpy(), sig.numpy(), rtol=t["rtol"], atol=t["atol"])
    # the level-split density pass (mode 2) == the sample-major one (mode 1), bit for bit, at the
    # capacity and with a device count below it (in the form of test_density_level_split_mode_bitexact)
    xd = x.to(dev)
    packed = m._pack_weights()
    table = m.flat_params()[: m._n_table]
    for count in (n, n - 13):
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        res = []
        for mode in (1, 2):
            s = torch.full((n,), -7.0, device=dev)
            enc = torch.empty(((n + 15) // 16) * 16 * 32, dtype=torch.float16, device=dev) if mode == 2 else None
            _lib.call("ncn_field_fwd", xd, None, n, n_dev, None, table, m._levels_ptr,
                      m._xyz_min, m._xyz_extent, packed, m._prec, mode, s, None, enc)
            res.append(s)
        torch.cuda.synchronize()
        assert torch.equal(res[0], res[1]), (precision, count)
        assert bool((res[1][count:] == -7.0).all()) and bool(torch.isfinite(res[1][:count]).all())
        assert torch.equal(res[0][:count], sig_d[:count])
    # the Morton windows of the same points: the clipped keys of the points outside the box
    check_window_order(_sort_windows(m, xd).cpu().numpy().astype(np.int64), x.numpy(), m._xyz_min, m._xyz_extent)
