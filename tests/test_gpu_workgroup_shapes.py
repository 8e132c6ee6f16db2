"""The boundary shapes of the shared workgroup primitives (csrc/workgroup.h) through the entry points that
sit on them: one thread, one lane short of / past a wave, one past a workgroup, one past a sweep (where
the running carry matters), and a 64-bit total whose high word must travel through the wave sum.
Integer results are exact; the one float sum has the textbook bound."""
import numpy as np
import pytest
import torch

from ncnerf_amd import _lib

pytestmark = pytest.mark.gpu


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def counts_with_zeros(rng, n, hi):
    c = rng.integers(0, hi + 1, n).astype(np.int32)
    c[rng.random(n) < 0.25] = 0
    return c


# block_excl_sweep<1024> over 4 counts per thread: 4096 counts per sweep
@pytest.mark.parametrize("R", [1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_march_train_scan(dev, R):
    c = counts_with_zeros(np.random.default_rng(R), R, 1024)
    rays_a = torch.full((R + 1, 3), -7, dtype=torch.int64, device=dev)
    counter = torch.full((3,), -7, dtype=torch.int32, device=dev)
    _lib.call("ncn_march_train_scan", to_dev(c, dev), R, rays_a, counter)
    c64 = c.astype(np.int64)
    want = np.stack([np.arange(R), np.cumsum(c64) - c64, c64], 1)
    assert np.array_equal(rays_a.cpu().numpy(), np.concatenate([want, [[-7, -7, -7]]]))
    assert counter.cpu().tolist() == [int(c64.sum()), R, -7]


# block_excl_scan<256>, one workgroup per 256 rays, the workgroups' order in the output arbitrary
@pytest.mark.parametrize("A", [1, 63, 65, 255, 256, 257, 513])
def test_test_compact(dev, A):
    NS = 5
    rng = np.random.default_rng(A)
    n_eff = rng.integers(0, NS + 1, A).astype(np.int32)
    xyzs = rng.standard_normal((A, NS, 3)).astype(np.float32)
    dirs = rng.standard_normal((A, NS, 3)).astype(np.float32)
    offsets = torch.full((A + 1,), -7, dtype=torch.int32, device=dev)
    xyz_c = torch.full((A * NS, 3), np.nan, device=dev)
    dir_c = torch.full((A * NS, 3), np.nan, device=dev)
    count = torch.full((2,), -7, dtype=torch.int32, device=dev)
    _lib.call("ncn_test_compact", to_dev(xyzs, dev), to_dev(dirs, dev), to_dev(n_eff, dev), A, NS, offsets, xyz_c,
              dir_c, count)
    total = int(n_eff.sum())
    assert count.cpu().tolist() == [total, -7]
    off = offsets.cpu().numpy()
    assert off[A] == -7
    off = off[:A].astype(np.int64)
    order = np.lexsort((n_eff, off))  # (an empty segment shares its start with its successor: it goes first)
    ends = off[order] + n_eff[order]
    assert off[order][0] == 0 and np.array_equal(ends[:-1], off[order][1:]) and ends[-1] == total
    rows = np.concatenate([off[n] + np.arange(n_eff[n]) for n in range(A)]).astype(np.int64)
    src = np.concatenate([np.arange(n_eff[n]) + n * NS for n in range(A)]).astype(np.int64)
    got_x, got_d = xyz_c.cpu().numpy(), dir_c.cpu().numpy()
    assert np.array_equal(got_x[rows], xyzs.reshape(-1, 3)[src]) and np.array_equal(got_d[rows], dirs.reshape(-1, 3)[src])
    assert np.isnan(got_x[total:]).all() and np.isnan(got_d[total:]).all()


# block_sum<256> + block_excl_sweep<256> over a block range: A = 65537 gives ranges of 512, two chunks each
@pytest.mark.parametrize("A", [1, 255, 256, 257, 65537])
def test_test_loop_index(dev, A):
    NS = 3
    n_eff = np.random.default_rng(A).integers(0, NS + 1, A).astype(np.int32)
    total = int(n_eff.sum())
    ctrl = torch.tensor([A, NS, NS, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
    idx = torch.full((A * NS + 1,), -7, dtype=torch.int32, device=dev)
    _lib.call("ncn_test_loop_index", to_dev(n_eff, dev), A, ctrl, idx)
    assert ctrl.cpu().tolist() == [A, NS, NS, 0, total, 0, 0, 0]
    got = idx.cpu().numpy()
    want = np.concatenate([n * NS + np.arange(n_eff[n]) for n in range(A)]).astype(np.int32)
    assert np.array_equal(np.sort(got[:total]), want) and (got[total:] == -7).all()


# block_sum<1024> of long long
@pytest.mark.parametrize("R", [1, 64, 1023, 1024, 1025])
def test_count_samples_carries_the_high_word(dev, R):
    rng = np.random.default_rng(R)
    t = (2**31 - rng.integers(0, 1000, R)).astype(np.int64)
    t[::7] += 2**33  # (high words that differ between lanes)
    out = torch.full((2,), -7, dtype=torch.int64, device=dev)
    acc = torch.tensor([1.0, 2.0], dtype=torch.float64, device=dev)
    counter = torch.tensor([5, 9], dtype=torch.int32, device=dev)
    _lib.call("ncn_count_samples", to_dev(t, dev), R, counter, out, acc)
    want = int(t.sum())
    assert R < 3 or want > 2**32
    assert out.cpu().tolist() == [want, -7]
    assert acc.cpu().tolist() == [6.0, 2.0 + float(want)]  # (want < 2^53: exact in f64)


# block_sum<256> of float, 1024 workgroups: n / 4 float4 loads, the tail by workgroup 0
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 262151])
def test_sumsq(dev, n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    part = torch.full((1025,), -7.0, device=dev)
    _lib.call("ncn_sumsq", to_dev(x, dev), n, part, None)
    p = part.cpu().numpy()
    assert p[1024] == -7.0
    got = np.float32(0.0)
    for v in p[:1024]:
        got = np.float32(got + v)
    want = float((x.astype(np.float64) ** 2).sum())
    # an f32 sum of n non-negative terms, in any order
    assert abs(float(got) - want) <= (n + 1) * 2.0**-24 * want, (float(got), want)
