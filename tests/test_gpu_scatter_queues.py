"""The table scatter's unit queue (field_scatter_kernel): ncn_field_scatter against the oracle's
serial scatter (oracle/hashgrid_ref.c hashgrid_bwd) by test_gpu_scatter_units' criteria (rel-L2 <=
1e-6, every entry within 1e-5 of the largest, the same non-zero set), at the sizes and grids where
a queue's bookkeeping can go wrong.  (Written for the per-XCD queues of round 7, which were measured
and removed; the cases hold for any unit order and any number of queues, and for
eight queues of 32768-sample spans they are the edges named in the brackets.)

 * fewer units than workgroups (n = 5: one unit per level) [seven of eight queues empty from the start];
 * one unit plus one sample on the C = 2 level (n = 2049), on the C = 4 levels (n = 4097) and on the
   coarse levels (n = 32769: a second span that holds a single sample);
 * n = 70001 (two full spans of the longest unit and a ragged one) on grids of 1, 7, 9 and 256
   workgroups [three queues own a span, five own none and steal from the first unit on];
 * the levels [10, 16) then [0, 10) as two launches (each range's own queue words);
 * levels whose maximum is 0 (units skipped, drawn past without a barrier), a cell level that opens
   every span and a fine one;
 * the `order` (Morton window) path.

Every case launches at least twice on one workspace without touching its queue words in between and
checks them zero after each launch, so a launch that left a counter behind would hand the next one
the wrong units.  Two launches on identical inputs differ only in the f32 flush order: they must
agree within the same bounds as a launch and the oracle (the unit sums are exact integers)."""
import numpy as np
import pytest
import torch

from oracle import field_ref
from ncnerf_amd import _lib
from ncnerf_amd.ngp_mt import NGPMT
from test_gpu_scatter_units import _check, _ray_samples

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(dev, n, op="fp16", with_order=False, zero_levels=()):
    """Inputs, workspace and the oracle's table gradient of one case (built once, never changed
    except for the workspace's position copies and queue words, which the launches own)."""
    key = (n, op, with_order, tuple(zero_levels))
    if key in _CASES:
        return _CASES[key]
    m = NGPMT(scale=0.5, grid_size=128).to(dev)
    levels = field_ref.grid_levels(0.5)[0]
    xw = (_ray_samples(n, seed=n) - np.float32(0.5)).astype(np.float32)
    xyzs = torch.from_numpy(xw).to(dev)
    order = None
    if with_order:
        order = torch.empty(n, dtype=torch.int32, device=dev)
        assert _lib.call("ncn_field_sort_windows", xyzs, n, None, m._xyz_min, m._xyz_extent, order) == 0
    x01 = (xw + np.float32(0.5)).astype(np.float32)
    rng = np.random.default_rng(n + 1)
    tdt = torch.float16 if op == "fp16" else torch.bfloat16
    gt_ = torch.from_numpy(rng.uniform(-1, 1, (n, 16, 2)).astype(np.float32)).to(tdt)
    gt_[torch.from_numpy(rng.random((n, 16)) < 0.2)] = 0
    gt_[n // 3: n // 3 + 500] = 0
    for l in zero_levels:
        gt_[:, l] = 0
    g = gt_.float().numpy()
    n_stride = (n + 3) & ~3
    ws = torch.zeros(int(_lib.lib().ncn_field_bwd_dE_floats(n)), dtype=torch.float32)
    ws[0] = 1.0
    ws[1] = 0.0 if op == "fp16" else 1.0
    pairs = torch.zeros(16, n_stride, 2, dtype=tdt)
    pairs[:, :n] = gt_.permute(1, 0, 2)
    ws[4:4 + 16 * n_stride] = pairs.contiguous().view(torch.float32).reshape(-1)
    lmax = torch.zeros(int(_lib.lib().ncn_field_bwd_blocks(n)), 16, dtype=torch.float32)
    lmax[0] = torch.from_numpy(np.abs(g).max(axis=(0, 2)))
    for l in zero_levels:
        assert float(lmax[0, l]) == 0.0
    g_samples = g.reshape(n, 32)
    if with_order:
        o = order.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(o), np.arange(n))
        g_samples = np.empty_like(g_samples)
        g_samples[o] = g.reshape(n, 32)

    def oracle(lo, hi):  # the serial f32 scatter of the levels [lo, hi)
        gl = np.zeros_like(g_samples).reshape(n, 16, 2)
        gl[:, lo:hi] = g_samples.reshape(n, 16, 2)[:, lo:hi]
        return field_ref._HashEncodeC.backward(
            type("Ctx", (), {"saved_tensors": (torch.from_numpy(x01),), "levels": levels,
                             "n_table": (m._n_table, 2)})(),
            torch.from_numpy(np.ascontiguousarray(gl.reshape(n, 32))))[1].numpy().astype(np.float64)

    c = dict(m=m, n=n, op=op, xyzs=xyzs, order=order, ws=ws.to(dev), lmax=lmax.to(dev), ref=oracle(0, 16), oracle=oracle)
    _CASES[key] = c
    return c


def _scatter(c, grad, lo=0, hi=16, max_blocks=0):
    m = c["m"]
    rc = _lib.call("ncn_field_scatter", c["xyzs"], c["n"], None, c["order"], m._levels_ptr, m._xyz_min, m._xyz_extent,
                   c["ws"], c["lmax"], lo, hi, max_blocks, grad)
    assert rc == 0, _lib.lib().ncn_last_error()
    torch.cuda.synchronize()
    # every launch leaves the queue words (the workspace's last 32) zero: the next one draws from them
    assert int(c["ws"][-32:].view(torch.int32).abs().sum()) == 0


def _run(c, dev, **kw):
    grad = torch.zeros(c["m"]._n_table, 2, dtype=torch.float32, device=dev)
    _scatter(c, grad, **kw)
    return grad.cpu().numpy().astype(np.float64)


def _permute_positions(c):
    assert _lib.call("ncn_field_scatter_positions", c["xyzs"], c["n"], None, c["ws"]) == 0


@pytest.mark.parametrize("n", [5, 2049, 4097, 32769])
def test_few_units(dev, n):
    """Sizes just past one unit of a class: the sample-ordered positions, then (same workspace) the
    permuted ones."""
    c = _case(dev, n)
    _check(_run(c, dev), c["ref"].copy(), n, "fp16", "unit", False)
    _permute_positions(c)
    _check(_run(c, dev), c["ref"].copy(), n, "fp16", "unit", True)
    c["ws"][2] = 0.0  # (back to the sample-ordered positions for a later user of the case)


@pytest.mark.parametrize("max_blocks", [1, 7, 9, 0])
def test_grid_sizes(dev, max_blocks):
    """Grids of 1, 7 and 9 workgroups and the full 256 (max_blocks 0) on three spans of the longest
    unit: every unit drawn by one workgroup, by a few, and more workgroups than coarse units."""
    c = _case(dev, 70001, "bf16")
    _permute_positions(c)
    a = _run(c, dev, max_blocks=max_blocks)
    b = _run(c, dev, max_blocks=max_blocks)
    _check(a, c["ref"].copy(), 70001, "bf16", "unit", True)
    _check(b, c["ref"].copy(), 70001, "bf16", "unit", True)
    # two launches on identical inputs: the f32 flush order alone differs
    rel = np.linalg.norm(a - b) / np.linalg.norm(a)
    print(f"two launches, max_blocks {max_blocks}: rel-L2 {rel:.2e}, max |diff| / max {np.abs(a - b).max() / np.abs(a).max():.2e}")
    assert rel <= 1e-6
    assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max()
    c["ws"][2] = 0.0


def test_level_ranges(dev):
    """The deferred scatter's two launches: the levels [10, 16), then [0, 10), into one table
    gradient; each range alone against the oracle's scatter of those levels, and twice over."""
    c = _case(dev, 70001, "bf16")
    for rep in range(2):
        grad = torch.zeros(c["m"]._n_table, 2, dtype=torch.float32, device=dev)
        _scatter(c, grad, lo=10, hi=16)
        hi_part = grad.cpu().numpy().astype(np.float64)
        _scatter(c, grad, lo=0, hi=10)
        _check(grad.cpu().numpy().astype(np.float64), c["ref"].copy(), 70001, "bf16", "unit", False)
        if rep == 0:
            _check(hi_part, c["oracle"](10, 16), 70001, "bf16", "unit", False)
            _check(_run(c, dev, lo=0, hi=10), c["oracle"](0, 10), 70001, "bf16", "unit", False)


def test_zero_levels(dev):
    """Levels 0 (the unit that opens every span), 7 and 12 carry no gradient: their units are skipped
    and the next ones drawn without a barrier."""
    c = _case(dev, 40961, zero_levels=(0, 7, 12))
    _permute_positions(c)
    for rep in range(2):
        got = _run(c, dev)
        off = [int(lv["offset"]) for lv in c["m"].levels] + [c["m"]._n_table]
        for l in (0, 7, 12):
            assert not got[off[l]:off[l + 1]].any()
        _check(got, c["ref"].copy(), 40961, "fp16", "unit", True)
    c["ws"][2] = 0.0


def test_order_path(dev):
    """The gradient stored in the Morton-window processing order, the positions gathered through it."""
    c = _case(dev, 70001, with_order=True)
    for rep in range(2):
        _check(_run(c, dev), c["ref"].copy(), 70001, "fp16", "unit", False)
