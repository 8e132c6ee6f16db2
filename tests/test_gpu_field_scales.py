"""The field at scene scales other than 0.5: xyz_extent != 1 and the level tables of other scales.

At scale 0.5 the box extent is 1, so every `/ xyz_extent`, `* (1 / xyz_extent)` and the scatter's two
normalisation branches coincide; the scatter's unit classes (levels 0-5, 6-9, 10-14, 15) are exactly
the dense / coarse hashed / fine hashed levels; and every cell of a coarse level fits the scatter's
32-bit cell key.  Here: scale 1.0 (extent 2; level 5, res 81, is hashed inside class 0), 1.5 (extent 3:
the scatter divides instead of multiplying by an exact reciprocal), 16.0 (extent 32; level 9 has res
1553, so in-box cells with pz >= 1023 take sc_push_run's out-of-key-range branch; the finest level
has res 32768: 15 integer bits of the f32 position).  tests/test_scale_cases_host.py asserts these
facts and the share of such positions (48 % of the scale-16 samples) on the host.

Inputs: n = 4099 positions (tests/scale_cases.py field_positions: uniform in the box plus the edge
set of field_level_check.place_edges for that box), parameters field_ref.init_params(5, scale=s,
table_init=0.5).  References and bounds are the project's existing ones, unchanged:
  forward        field_ref.field_forward(scale=s, emulate=precision), test_gpu_field.TOL; mode 2 == mode 1 bitwise
  backward       autograd through the emulating oracle: rel-L2 per block, per table level and per 16-row
                 weight tile <= TOL["bwd"]; rows lost <= 1e-3; dE per level by field_level_check's outlier
                 rule, share <= 2 % (test_gpu_field_levels.SHARE_CAP)
  scatter alone  test_gpu_scatter_units.scatter_case / _check: rel-L2 <= 1e-6, max |diff| <= 1e-5 max, one-sided
                 non-zeros <= 1e-4
  input grads    oracle dE contracted with the host Jacobian / extent (world coordinates) and autograd's dL/dd:
                 rel-L2 per column <= TOL["bwd"]; a second backward bit-identical
  sort windows   test_gpu_field.check_window_order's host keys

Found: no defect; every check holds at the existing bounds (no tolerance was re-derived for a scale).

Measured on an MI355X, worst over the cases (1.0 fp16, 1.5 fp16, 1.5 bf16, 16.0 fp16), next to the bound:
  forward |dsigma| / (rtol |sigma| + atol)   0.020 fp16 / 0.008 bf16                  (1)
  forward |drgb|                             7.7e-5 fp16 / 2.6e-4 bf16                (2e-3 / 1e-2)
  backward rel-L2, worst block               4.0e-4 fp16 / 2.6e-3 bf16                (2e-2 / 5e-2)
  backward rel-L2, worst table level         5.9e-4 fp16 / 3.9e-3 bf16; rows lost <= 2 of 17 653
  backward rel-L2, worst 16-row weight tile  4.3e-4 fp16 / 2.5e-3 bf16; no tile skipped
  dE outlier share, worst level              0.06 % fp16 / 0.00 % bf16                (cap 2 %)
  scatter alone, edge set                    rel-L2 4.1e-7, max |diff| / max 1.2e-6, 2 of 324 540 one-sided
  scatter alone, ray samples, scale 16       rel-L2 1.2e-7, max |diff| / max 9.6e-7, 0 of 4 565 524 one-sided
                                             (bounds: 1e-6, 1e-5, 1e-4 of the non-zero entries)
  dL/dx rel-L2, worst column                 4.1e-5 fp16 / 1.0e-7 bf16                (2e-2 / 5e-2)
  dL/dd rel-L2, worst column                 2.3e-4 fp16 / 1.7e-3 bf16                (2e-2 / 5e-2)
Each of these was also run against a scratch build with one statement changed: the scatter's dividing
normalisation replaced by the multiplication with the rounded reciprocal (test_scatter_alone_at_scale at
1.5 fails: rel-L2 1.3e-4, 10 one-sided entries), `/ xyz_extent` dropped from ncn_field_bwd_dx's out_scale
(test_input_grads_at_scale fails: dL/dx rel-L2 2.0 at scale 1.5, 31 at scale 16).
"""
import functools

import numpy as np
import pytest
import torch

import scale_cases as sc
from oracle import field_ref
from field_input_grad_check import enc_jacobian
from field_level_check import MAX_SKIPPED_TILES, table_level_errors, weight_tile_errors
from ncnerf_amd import _lib
from test_gpu_field import TOL, _inputs, _model_from_oracle, check_window_order
from test_gpu_field_levels import LOSS_SCALE, _bwd_scale, _check_dE, _check_level_max, _decode, _mlp_pass, _upstream
from test_gpu_scatter_units import scatter_case

pytestmark = pytest.mark.gpu

N = sc.N_FIELD
CASES = [(1.0, "fp16"), (1.5, "fp16"), (1.5, "bf16"), (16.0, "fp16")]


@functools.lru_cache(maxsize=None)
def _params(scale):
    return field_ref.init_params(seed=5, scale=scale, table_init=0.5)


@functools.lru_cache(maxsize=None)
def _xd(scale):
    """(positions (N, 3), directions with |d| != 1 (N, 3)), shared and never modified."""
    x = torch.from_numpy(np.array(sc.field_positions(scale)))
    d = _inputs(N, 1)[1]
    d = d * (0.5 + torch.rand(N, 1, generator=torch.Generator().manual_seed(101)))
    return x, d


@functools.lru_cache(maxsize=None)
def _oracle_forward(scale, precision):
    P, levels = _params(scale)
    x, d = _xd(scale)
    sig, rgb, _ = field_ref.field_forward(x, d, P, levels, scale=scale, emulate=precision)
    return sig.numpy(), rgb.numpy()


@pytest.mark.parametrize("scale,precision", CASES)
def test_forward_at_scale(dev, scale, precision):
    P, levels = _params(scale)
    m = _model_from_oracle(P, dev, precision, scale=scale)
    assert m._xyz_extent == 2 * scale and m.cascades == sc.CASCADES[scale]
    x, d = _xd(scale)
    xd, dd = x.to(dev), d.to(dev)
    with torch.no_grad():
        out = m(xd, dd)
        sig_d = m.density(xd)
    sig, rgb = _oracle_forward(scale, precision)
    t = TOL[precision]
    got_s, got_r = out["sigmas"].cpu().numpy(), out["rgbs"].cpu().numpy()
    print(f"forward scale {scale} {precision}: max |dsigma| / (rtol |sigma| + atol) "
          f"{np.max(np.abs(got_s - sig) / (t['rtol'] * np.abs(sig) + t['atol'])):.3f}, max |drgb| {np.abs(got_r - rgb).max():.2e} "
          f"(bound {t['rgb']:.0e})")
    np.testing.assert_allclose(got_s, sig, rtol=t["rtol"], atol=t["atol"])
    np.testing.assert_allclose(got_r, rgb, atol=t["rgb"])
    np.testing.assert_allclose(sig_d.cpu().numpy(), sig, rtol=t["rtol"], atol=t["atol"])
    # the level-split density pass (mode 2) == the sample-major one (mode 1), bit for bit, at the
    # capacity and with a device count below it
    packed = m._pack_weights()
    table = m.flat_params()[: m._n_table]
    for count in (N, N - 13):
        n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
        res = []
        for mode in (1, 2):
            s = torch.full((N,), -7.0, device=dev)
            enc = torch.empty(((N + 15) // 16) * 16 * 32, dtype=torch.float16, device=dev) if mode == 2 else None
            _lib.call("ncn_field_fwd", xd, None, N, n_dev, None, table, m._levels_ptr,
                      m._xyz_min, m._xyz_extent, packed, m._prec, mode, s, None, enc)
            res.append(s)
        torch.cuda.synchronize()
        assert torch.equal(res[0], res[1]), (scale, precision, count)
        assert bool((res[1][count:] == -7.0).all()) and bool(torch.isfinite(res[1][:count]).all())
        assert torch.equal(res[0][:count], sig_d[:count])


@functools.lru_cache(maxsize=None)
def _oracle_backward(scale, precision):
    """(parameter gradients of the emulating oracle, as test_field_backward forms them)."""
    P, levels = _params(scale)
    x, d = _xd(scale)
    gs, gr = _upstream(N)
    Pt = field_ref.FieldParams(*[t.clone().requires_grad_(True) for t in P.tensors()])
    sig, rgb, _ = field_ref.field_forward_autograd(x, d, Pt, levels, scale=scale, emulate=precision)
    ((sig * gs).sum() + (rgb * gr).sum()).backward()
    return [t.grad for t in Pt.tensors()]


@functools.lru_cache(maxsize=None)
def _oracle_dE_dd(scale, precision):
    """(dL/denc (N, 32) as the grid backward receives it, dL/dd) of the emulating oracle with the
    backward's rounding at the kernel's scale."""
    P, levels = _params(scale)
    x, d = _xd(scale)
    gs, gr = _upstream(N)
    dr = d.clone().requires_grad_(True)
    sig, rgb, _, enc = field_ref.field_forward_autograd(x, dr, P, levels, scale=scale, emulate=precision,
                                                        bwd_scale=_bwd_scale(precision), return_enc=True)
    ((sig * gs).sum() + (rgb * gr).sum()).backward()
    return enc.grad.clone(), dr.grad.double()


@pytest.mark.parametrize("scale,precision", CASES)
def test_backward_at_scale(dev, scale, precision):
    """test_field_backward's checks at this scale (loss scale 1), then the MLP pass's dE per level
    against the oracle with the backward's rounding (loss scale 4, as test_gpu_field_levels)."""
    P, levels = _params(scale)
    m = _model_from_oracle(P, dev, precision, scale=scale)
    x, d = _xd(scale)
    gs, gr = _upstream(N)
    xd, dd, gsd, grd = x.to(dev), d.to(dev), gs.to(dev), gr.to(dev)
    out = m(xd, dd)
    (out["sigmas"] * gsd).sum().add_((out["rgbs"] * grd).sum()).backward()
    gflat = m.flat_grad().cpu()
    ref = _oracle_backward(scale, precision)
    bound = TOL[precision]["bwd"]
    off, errs = 0, {}
    for name, r in zip(("table", "W1", "W2", "W3", "W4", "W5"), ref):
        k = r.numel()
        errs[name] = float((gflat[off:off + k].reshape(r.shape) - r).norm() / r.norm().clamp_min(1e-12))
        off += k
    print(f"backward scale {scale} {precision} rel-L2 per block:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e < bound for e in errs.values()), errs
    assert float(gflat[-16 * 64:].reshape(16, 64)[3:].abs().max()) == 0.0  # padded output rows
    nt = m._n_table
    lv_errs = table_level_errors(gflat[:nt].numpy(), ref[0].numpy(), levels)
    print(f"backward scale {scale} {precision} table rel-L2 per level:", " ".join(f"{e[0]:.2e}" for e in lv_errs),
          "| rows lost / rows:", " ".join(f"{e[1]}/{e[2]}" for e in lv_errs))
    for l, (rel, lost, nz) in enumerate(lv_errs):
        assert nz > 0 and rel <= bound, (l, rel)
        assert lost <= 1e-3 * nz, (l, lost, nz)
    off = nt
    for name, r in zip(("W1", "W2", "W3", "W4", "W5"), ref[1:]):
        k = r.numel()
        tiles, skipped = weight_tile_errors(gflat[off:off + k].reshape(r.shape).numpy(), r.numpy())
        off += k
        print(f"backward scale {scale} {precision} {name} worst 16-row tile rel-L2 {max(tiles.values()):.2e}, skipped {skipped}")
        assert len(skipped) <= MAX_SKIPPED_TILES, (name, skipped)
        assert all(e <= bound for e in tiles.values()), (name, tiles)
    # the MLP pass alone: dE decoded from the workspace, per level
    if m.amp_state is not None:
        m.amp_state[0] = LOSS_SCALE
    ws, lmax, _, _ = _mlp_pass(m, xd, dd, gsd, grd)
    _, dE, pad = _decode(ws, N, precision)
    assert pad.numel() == 0 or float(pad.abs().max()) == 0.0
    _check_level_max(lmax, dE, N)
    _check_dE(dE, _oracle_dE_dd(scale, precision)[0].numpy(), precision, f"scale {scale} n {N}")


@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("scale,op", CASES)
def test_scatter_alone_at_scale(dev, scale, op, with_order):
    """The table scatter on a fabricated workspace (both position layouts, or a processing order)
    against the oracle's serial scatter.  Scale 1.5 runs the dividing normalisation, scale 16 real
    runs beyond the cell key range (level 9, pz >= 1023), scale 1.0 a hashed level in unit class 0."""
    scatter_case(dev, N, op, "unit", xw=np.array(sc.field_positions(scale)), with_order=with_order, scale=scale)


@pytest.mark.parametrize("n", [40960])
def test_scatter_ray_samples_at_scale_16(dev, n):
    """Samples on rays inside the scale-16 box (long runs of equal coarse cells across several units
    of every level, a third of them beyond the cell key range on level 9)."""
    scatter_case(dev, n, "fp16", "unit", scale=16.0)


def _col_errors(got, ref):
    return [float((got[:, k].double() - ref[:, k]).norm() / ref[:, k].norm().clamp_min(1e-30)) for k in range(3)]


@pytest.mark.parametrize("scale,precision", [(1.5, "fp16"), (1.5, "bf16"), (16.0, "fp16")])
def test_input_grads_at_scale(dev, scale, precision):
    """dL/dx (ncn_field_bwd_dx) and dL/dd against the oracle in world coordinates: the encoding
    gradient contracted with the host Jacobian d enc / d x01, times d x01 / d x = 1 / extent."""
    P, levels = _params(scale)
    m = _model_from_oracle(P, dev, precision, loss_scale=LOSS_SCALE, scale=scale)
    x, d = _xd(scale)
    gs, gr = _upstream(N)
    dE, ref_d = _oracle_dE_dd(scale, precision)
    extent = 2.0 * scale
    x01 = (x - (-scale)) / extent
    J = enc_jacobian(x01, P.table, levels, torch.float32)  # (N, 32, 3) fp64
    ref_x = torch.einsum("nf,nfk->nk", dE.double(), J) / extent

    def run():
        xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
        out = m(xg, dg)
        (out["sigmas"] * gs.to(dev)).sum().add_((out["rgbs"] * gr.to(dev)).sum()).backward()
        return xg.grad.cpu(), dg.grad.cpu()

    gx, gd = run()
    ex, ed = _col_errors(gx, ref_x), _col_errors(gd, ref_d)
    print(f"input grads scale {scale} {precision} rel-L2 dL/dx {' '.join(f'{e:.3e}' for e in ex)} | "
          f"dL/dd {' '.join(f'{e:.3e}' for e in ed)}")
    bound = TOL[precision]["bwd"]
    assert all(e <= bound for e in ex + ed), (ex, ed)
    gx2, gd2 = run()
    assert torch.equal(gx, gx2) and torch.equal(gd, gd2)


@pytest.mark.parametrize("scale", [1.5, 16.0])
def test_sort_windows_at_scale(dev, scale):
    """ncn_field_sort_windows multiplies by 1 / extent: the order against the host's clipped Morton
    keys, on the edge set (points outside the box clip) and on 8195 uniform positions."""
    m = _model_from_oracle(_params(scale)[0], dev, scale=scale)
    for x in (torch.from_numpy(np.array(sc.field_positions(scale))), _inputs(8195, 3, scale=scale)[0]):
        n = x.shape[0]
        xd = x.to(dev)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        assert _lib.call("ncn_field_sort_windows", xd, n, None, m._xyz_min, m._xyz_extent, order) == 0
        o = order.cpu().numpy().astype(np.int64)
        check_window_order(o, x.numpy(), m._xyz_min, m._xyz_extent)
        assert not np.array_equal(o, np.arange(n))
