"""Occupancy-grid refresh on the device (csrc/grid.hip via NGPMT.update_density_grid) against the
numpy restatement of ngp_mt.py:305-368 (oracle/vren_ref.py: density_grid_update, packbits).

What is exact: the hit cells' positions lie in their cell's jitter box (ngp_mt.py:318-319), their
densities are the field's density mode at those positions (bit-equal to NGPMT.density), the update
where(grid < 0, grid, max(grid*decay, tmp)) of every cell, the bitfield (packbits against
min(mean, threshold): the device threshold is within 1e-6 of the oracle's f64 mean, the bitfield is
packbits of the updated grid against it).
What is statistical (the sampling is random in the reference too): the fraction of cells hit vs the
marginal probability of M uniform + M occupied draws with replacement (5 sigma).

More than one cascade (scale 1.0: C = 2, scale 1.5: C = 3; test_grid_refresh_cascades_*): the workspace
holds one cascade's hit list, so _drive_cascades runs update_density_grid's loop one cascade at a time
through the C ABI on a copy of the grid and checks each cascade as above (jitter box
s = min(2^(c-1), scale), count_grid[c] under erode, the rows still to come untouched), then the mean and
packbits over C * N cells; the model's own call from the same grid and seed must give that grid and
bitfield bit for bit (so the cascade term of its seed, the reuse of the workspace, the reset of the
list count and the `beside` side stream on c == 0 are held to the driven result).  Found: no defect.
With the cascade term dropped from update_density_grid's seed in a scratch copy, all five fail.
"""
import numpy as np
import pytest
import torch

from oracle import vren_ref
from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers

pytestmark = pytest.mark.gpu


def _model(dev, G, seed=0, scale=0.5):
    torch.manual_seed(seed)
    m = register_grid_buffers(NGPMT(scale=scale, grid_size=G).to(dev))
    with torch.no_grad():  # a table with structure: densities spread over ~[0.1, 20]
        m.flat_params()[: m._n_table].mul_(3e4)
    return m


def _init_grid(m, rng, frac_neg=0.05):
    N = m.grid_size ** 3
    g = rng.exponential(3.0, (m.cascades, N)).astype(np.float32)
    g[rng.random((m.cascades, N)) < 0.5] = 0.0
    g[rng.random((m.cascades, N)) < frac_neg] = -1.0  # cells marked invisible (mark_invisible_cells)
    with torch.no_grad():
        m.density_grid.copy_(torch.from_numpy(g))
    return g


def _hits(m):
    ws = m._gws
    n = int(ws["scal"][0].item())
    return n, ws["idx"][:n].cpu().numpy(), ws["xyzs"][:n].cpu().numpy(), ws["sigmas"][:n].cpu().numpy()


def _check_cascade(m, c, old_row, new_row, hits, thr, decay, cnt_row=None):
    """One cascade's refresh: `hits` = (n, idx, xyz, sig) of its hit list, old_row / new_row its grid
    row before / after.  Every hit cell once, positions in the cascade's jitter box
    (s = min(2^(c-1), scale), ngp_mt.py:316-319), densities == NGPMT.density bit for bit, the update
    rule == the oracle's on this row (with erode: within 1e-6, the device's powf)."""
    G = m.grid_size
    n, idx, xyz, sig = hits
    # each hit cell once
    assert len(np.unique(idx)) == n
    # positions inside the cell's jitter box
    centre, hg = vren_ref.grid_cell_positions(idx, G, min(2 ** (c - 1), m.scale))
    assert np.all(np.abs(xyz - centre) <= hg * (1 + 1e-5) + 1e-7)
    # densities = the density mode of the field at those positions
    with torch.no_grad():
        ref_sig = m.density(torch.from_numpy(xyz).to(m.density_grid.device)).cpu().numpy()
    np.testing.assert_array_equal(sig, ref_sig)
    new_ref, _, _ = vren_ref.density_grid_update(old_row, idx, sig, decay, thr, count_grid=cnt_row)
    if cnt_row is None:
        np.testing.assert_array_equal(new_row, new_ref)
    else:
        np.testing.assert_allclose(new_row, new_ref, rtol=1e-6, atol=0)


def _check_packbits(new, thr, thr_dev, bf):
    """The threshold min(mean of the positive cells of every cascade, thr) within 1e-6 of the f64 mean,
    the bitfield == packbits of the whole grid against the device's threshold (NaN: cleared, q12)."""
    pos = new[new > 0]
    mean = np.float32(pos.astype(np.float64).mean()) if pos.size else np.float32(np.nan)
    thr_ref = min(float(mean), thr)
    if np.isnan(thr_ref):
        assert np.isnan(thr_dev)
        assert int(bf.sum()) == 0
        return
    assert abs(thr_dev - thr_ref) <= 1e-6 * abs(thr_ref)
    np.testing.assert_array_equal(bf, vren_ref.packbits(new, thr_dev))


def _drive_cascades(m, old, thr, warmup, seed, decay=0.95, erode=False):
    """update_density_grid's cascades one at a time through the C ABI, on a copy of the grid (the
    workspace holds one cascade's hit list, so after the model's own call only the last one could be
    inspected): per cascade ncn_grid_sample (the seed update_density_grid derives: the cascade folded
    in) -> density pass (ncn_field_fwd mode 2 on the device count) -> ncn_grid_apply, each checked by
    _check_cascade; then ncn_grid_packbits over C * N cells, checked by _check_packbits.
    -> (grid (C, N) device tensor, bitfield device tensor, [hit cell indices per cascade])."""
    from ncnerf_amd._lib import call
    G, C = m.grid_size, m.cascades
    N = G ** 3
    dev = m.density_grid.device
    dg = torch.from_numpy(old).to(dev).contiguous()
    cnt = m.count_grid.float().contiguous() if erode else None
    ws = m._grid_ws()
    n_list = ws["scal"][0:1]
    packed = m._pack_weights()
    hit_cells = []
    for c in range(C):
        s = min(2 ** (c - 1), m.scale)
        hg = s / G
        cc = cnt[c] if erode else None
        call("ncn_grid_sample", dg[c], N, G, s - hg, hg, thr, N // 4, 1 if warmup else 0,
             (seed + 0x9E3779B97F4A7C15 * c) % 2 ** 64, decay, cc, ws["xyzs"], ws["idx"], n_list, ws["work"])
        call("ncn_field_fwd", ws["xyzs"], None, N, n_list, None, m.xyz_encoder.params, m._levels_ptr, m._xyz_min,
             m._xyz_extent, packed, m._prec, 2, ws["sigmas"], None, ws["enc"])
        call("ncn_grid_apply", dg[c], ws["idx"], ws["sigmas"], n_list, N, decay, cc)
        hits = _hits(m)
        _check_cascade(m, c, old[c], dg[c].cpu().numpy(), hits, thr, decay, None if cnt is None else cnt[c].cpu().numpy())
        hit_cells.append(hits[1])
        if c + 1 < C:  # the rows of the cascades still to come are untouched
            assert np.array_equal(dg[c + 1:].cpu().numpy(), old[c + 1:])
    bf = torch.full_like(m.density_bitfield, 0x5A)
    thr_out = ws["scal"][1:2].view(torch.float32)
    call("ncn_grid_packbits", dg, C * N, thr, bf, thr_out, ws["work"])
    _check_packbits(dg.cpu().numpy(), thr, float(thr_out.item()), bf.cpu().numpy())
    return dg, bf, hit_cells


def _check_update(m, old, thr, decay=0.95, warmup=None, seed=None, erode=False, **kw):
    """After m.update_density_grid(thr, ...) on the grid `old`.  One cascade: the workspace holds its
    hit list, checked in place -> (n, idx).  More: the cascades are driven one at a time with the same
    warmup / seed / erode (_drive_cascades, every cascade checked), and the model's own call, repeated
    from `old` with that seed, must give that grid and bitfield bit for bit -> the hit cells per cascade."""
    C = m.cascades
    if C == 1:
        hits = _hits(m)
        new = m.density_grid.cpu().numpy()
        _check_cascade(m, 0, old[0], new[0], hits, thr, decay)
        thr_dev = float(m._gws["scal"][1:2].view(torch.float32).item())
        _check_packbits(new, thr, thr_dev, m.density_bitfield.cpu().numpy())
        return hits[0], hits[1]
    got = m.density_grid.clone(), m.density_bitfield.clone()
    dg, bf, hit_cells = _drive_cascades(m, old, thr, warmup, seed, decay, erode)
    assert torch.equal(got[0], dg) and torch.equal(got[1], bf)
    with torch.no_grad():
        m.density_grid.copy_(torch.from_numpy(old))
        m.density_bitfield.fill_(0xA5)
    m.update_density_grid(thr, warmup=warmup, decay=decay, erode=erode, seed=seed, **kw)
    assert torch.equal(m.density_grid, dg) and torch.equal(m.density_bitfield, bf)
    return hit_cells


@pytest.mark.parametrize("G", [32, 128])
def test_grid_refresh_warmup_all_cells(dev, G):
    m = _model(dev, G)
    rng = np.random.default_rng(1)
    old = _init_grid(m, rng)
    m.update_density_grid(1e4, warmup=True, seed=123)  # threshold above the mean: min(mean, thr) = mean
    n, idx = _check_update(m, old, 1e4)
    assert n == G ** 3
    assert np.array_equal(np.sort(idx), np.arange(G ** 3))


def test_grid_refresh_sampled(dev):
    G = 128
    m = _model(dev, G)
    rng = np.random.default_rng(2)
    old = _init_grid(m, rng)
    thr = 0.01 * 1024 / 3 ** 0.5
    m.update_density_grid(thr, warmup=False, seed=7)
    n, idx = _check_update(m, old, thr)
    N = G ** 3
    occ = old[0] > thr
    p_u, p_o = vren_ref.grid_hit_probabilities(N, N // 4, int(occ.sum()))
    hit = np.zeros(N, bool)
    hit[idx] = True
    for mask, p in ((~occ, p_u), (occ, 1 - (1 - p_u) * (1 - p_o))):
        k = int(mask.sum())
        f = hit[mask].mean()
        assert abs(f - p) <= 5 * np.sqrt(p * (1 - p) / k), (f, p, k)


def test_grid_refresh_deterministic_and_seeded(dev):
    m = _model(dev, 64)
    old = _init_grid(m, np.random.default_rng(3))
    thr = 2.0
    outs = []
    for seed in (11, 11, 12):
        with torch.no_grad():
            m.density_grid.copy_(torch.from_numpy(old))
        m.update_density_grid(thr, warmup=False, seed=seed)
        outs.append((m.density_grid.clone(), m.density_bitfield.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])


def test_grid_refresh_empty_grid_clears_bitfield(dev):
    """Quirk q12 (ngp_mt.py:365-368): no cell > 0 -> mean NaN -> packbits against NaN -> all zero."""
    m = _model(dev, 32)
    with torch.no_grad():
        m.density_grid.fill_(-1.0)
        m.density_bitfield.fill_(255)
    m.update_density_grid(0.5, warmup=True, seed=5)
    assert torch.all(m.density_grid == -1.0)
    assert int(m.density_bitfield.sum().item()) == 0


def test_grid_refresh_erode(dev):
    m = _model(dev, 32)
    rng = np.random.default_rng(4)
    old = _init_grid(m, rng, frac_neg=0.0)
    cnt = rng.integers(0, 4, old.shape).astype(np.float32)
    m.count_grid = torch.from_numpy(cnt).to(dev)
    m.update_density_grid(1e4, warmup=True, erode=True, seed=9)
    n, idx, xyz, sig = _hits(m)
    new_ref, _, _ = vren_ref.density_grid_update(old, idx, sig, 0.95, 1e4, count_grid=cnt)
    np.testing.assert_allclose(m.density_grid.cpu().numpy(), new_ref, rtol=1e-6, atol=0)


def test_grid_refresh_cascades_warmup(dev):
    """Scale 1.0 (C = 2), warm-up at G = 32: every cell of every cascade is hit; the per-cascade loop
    (jitter box s = min(2^(c-1), scale), one workspace reused, the list count reset, mean and packbits
    over C * N cells) by _check_update."""
    G = 32
    m = _model(dev, G, scale=1.0)
    assert m.cascades == 2
    old = _init_grid(m, np.random.default_rng(11))
    m.update_density_grid(1e4, warmup=True, seed=123)
    hit_cells = _check_update(m, old, 1e4, warmup=True, seed=123)
    for idx in hit_cells:
        assert np.array_equal(np.sort(idx), np.arange(G ** 3))


def test_grid_refresh_cascades_sampled(dev):
    """Scale 1.5 (C = 3; the third cascade's box is clipped to the scale: s = 0.5, 1, 1.5), sampled at
    G = 64: _check_update, and per cascade the fraction of cells hit against the marginal probability
    of M uniform + M occupied draws (5 sigma), the occupied cells counted on that cascade's row."""
    G = 64
    m = _model(dev, G, scale=1.5)
    assert m.cascades == 3
    old = _init_grid(m, np.random.default_rng(12))
    thr = 2.0
    m.update_density_grid(thr, warmup=False, seed=7)
    hit_cells = _check_update(m, old, thr, warmup=False, seed=7)
    N = G ** 3
    for c, idx in enumerate(hit_cells):
        occ = old[c] > thr
        p_u, p_o = vren_ref.grid_hit_probabilities(N, N // 4, int(occ.sum()))
        hit = np.zeros(N, bool)
        hit[idx] = True
        for mask, p in ((~occ, p_u), (occ, 1 - (1 - p_u) * (1 - p_o))):
            k = int(mask.sum())
            f = hit[mask].mean()
            assert abs(f - p) <= 5 * np.sqrt(p * (1 - p) / k), (c, f, p, k)


def test_grid_refresh_cascades_erode(dev):
    """C = 2 with erode: the per-cell decay reads count_grid[c] (rows that differ between the cascades)."""
    m = _model(dev, 32, scale=1.0)
    rng = np.random.default_rng(13)
    old = _init_grid(m, rng, frac_neg=0.0)
    cnt = rng.integers(0, 4, old.shape).astype(np.float32)
    cnt[1] = 3 - cnt[0]  # no cell has the same count in both cascades
    m.count_grid = torch.from_numpy(cnt).to(dev)
    m.update_density_grid(1e4, warmup=True, erode=True, seed=9)
    _check_update(m, old, 1e4, warmup=True, seed=9, erode=True)
    # and sampled (the decay of the cells that are not hit, in ncn_grid_sample)
    m.density_grid.copy_(torch.from_numpy(old))
    m.update_density_grid(2.0, warmup=False, erode=True, seed=10)
    _check_update(m, old, 2.0, warmup=False, seed=10, erode=True)


def test_grid_refresh_cascades_beside(dev):
    """C = 2 with `beside`: the first cascade's sampling runs on the side stream (c == 0 only) while the
    callable's work is issued on the current one; the result equals the run without it bit for bit."""
    m = _model(dev, 32, scale=1.0)
    old = _init_grid(m, np.random.default_rng(14))
    thr = 2.0
    calls = []
    acc = torch.zeros(1 << 20, device=dev)

    def beside():
        calls.append(1)
        for _ in range(4):
            acc.add_(1.0)

    m.update_density_grid(thr, warmup=False, seed=21, beside=beside)
    torch.cuda.synchronize()
    assert calls == [1] and bool((acc == 4.0).all())
    with_beside = m.density_grid.clone(), m.density_bitfield.clone()
    _check_update(m, old, thr, warmup=False, seed=21)  # (drives the cascades, then the model's call without `beside`)
    assert torch.equal(m.density_grid, with_beside[0]) and torch.equal(m.density_bitfield, with_beside[1])
    _check_update(m, old, thr, warmup=False, seed=21, beside=beside)  # (and with it again)
    assert calls == [1, 1]


def test_grid_refresh_cascade_is_in_the_seed(dev):
    """Two cascades with equal grid rows draw different cells: the cascade is folded into the seed
    (the same row under the same seed would repeat the draw, as cascade 0 does run to run)."""
    G = 32
    m = _model(dev, G, scale=1.0)
    old = _init_grid(m, np.random.default_rng(15))
    old[1] = old[0]
    with torch.no_grad():
        m.density_grid.copy_(torch.from_numpy(old))
    thr = 2.0
    m.update_density_grid(thr, warmup=False, seed=33)
    h0, h1 = (set(h.tolist()) for h in _check_update(m, old, thr, warmup=False, seed=33))
    again = _drive_cascades(m, old, thr, False, 33)[2]
    assert set(again[0].tolist()) == h0 and set(again[1].tolist()) == h1
    # independent draws with the same per-cell probabilities p (p_u, or 1 - (1 - p_u)(1 - p_o) on the
    # occupied cells): a cell is in both hit sets with probability p^2 (5 sigma)
    N = G ** 3
    occ = old[0] > thr
    p_u, p_o = vren_ref.grid_hit_probabilities(N, N // 4, int(occ.sum()))
    p = np.where(occ, 1 - (1 - p_u) * (1 - p_o), p_u)
    both, want = len(h0 & h1), float((p ** 2).sum())
    assert h0 != h1 and abs(both - want) <= 5 * np.sqrt(float((p ** 2 * (1 - p ** 2)).sum())), (both, want, len(h0), len(h1))


@pytest.mark.parametrize("branch", ["pinhole", "ndc"])
def test_mark_invisible_cells_golden(dev, branch):
    """NGPMT.mark_invisible_cells vs the reference's own (tests/golden/invisible_cells.npz, made by
    tests/golden/make_golden.py from models/ngp_mt.py:274-337 on a 32^3 grid, 20 synthetic poses):
    the 0 / -1 marks and the per-cell camera counts.  The projections run as fp32 matmuls on the
    device (the fixture: torch CPU), so a cell projecting within rounding of an image border or of
    the near plane may flip: at most 0.05 % of the cells."""
    import os
    from ncnerf_amd import synthetic
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "invisible_cells.npz"))
    G, n_cams = int(f["G"]), int(f["n_cams"])
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=G).to(dev))
    scene = synthetic.SyntheticScene()
    poses = torch.from_numpy(scene.poses[:n_cams].astype(np.float32)).to(dev)
    K = torch.from_numpy(f["K"]) if branch == "pinhole" else (torch.from_numpy(f["M_ndc"]), torch.from_numpy(f["M_uv"]),
                                                              [0.0, 0.0, 0.0], float(f["ndc_scale"]))
    m.mark_invisible_cells(K, dev, poses, (synthetic.IMG_W, synthetic.IMG_H), float(f["near"]), chunk=5000)
    dens = m.density_grid.cpu().numpy()
    cnt = np.rint(m.count_grid.cpu().numpy() * n_cams).astype(np.int64)
    bad_d = int((dens != f[branch + "_density"].astype(np.float32)).sum())
    bad_c = int((cnt != f[branch + "_count"].astype(np.int64)).sum())
    assert set(np.unique(dens).tolist()) <= {0.0, -1.0}
    assert bad_d <= 0.0005 * dens.size and bad_c <= 0.0005 * dens.size, (bad_d, bad_c)
