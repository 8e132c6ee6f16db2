"""tests/guard_bands.py catches a wrong kernel — shown on CPU tensors with small "kernels" written
in torch, so no wrong kernel ever runs on a GPU.  A kernel gets the payload tensor only, as the HIP
entry points get its pointer; the wrong ones reach past it through as_strided, which is what an
index off by one does.  Also the helper's geometry: band size, payload alignment, misalign = 4."""
import numpy as np
import pytest
import torch

import guard_bands as gb

N = 37  # rows of the output; the "device count" below is COUNT
COUNT = 29
CPU = torch.device("cpu")


def _past_end(t, k=1):
    """t's flat elements plus k behind them."""
    return t.as_strided((t.numel() + k,), (1,), t.storage_offset())


def _before_start(t, k=1):
    return t.as_strided((t.numel() + k,), (1,), t.storage_offset() - k)


def k_correct(x, out, count):
    out[:count] = 2 * x[:count]


def k_writes_past_end(x, out, count):
    k_correct(x, out, count)
    _past_end(out)[-1] = 1.0


def k_writes_before_start(x, out, count):
    k_correct(x, out, count)
    _before_start(out)[0] = 1.0


def k_writes_row_past_count(x, out, count):
    out[:count + 1] = 2 * x[:count + 1]


def k_sum_correct(x, out, count):
    out[0] = x.sum()


def k_sum_reads_past_end(x, out, count):
    out[0] = _past_end(x).sum()


def _run(kernel, fill, n_out=N, dtype=torch.float32):
    x = np.arange(N, dtype=np.float32) + 1
    xd, hx = gb.guarded_copy(x, fill, CPU)
    out, ho = gb.guarded((n_out,), dtype, CPU)
    kernel(xd, out, COUNT)
    return out, ho, hx


def test_geometry():
    assert gb.BAND == 64 * 1024 and gb.BAND % 512 == 0 and gb.BAND == 4 * 1024 * 16
    for dtype in (torch.float32, torch.float16, torch.int64, torch.uint8):
        t, h = gb.guarded((5, 3), dtype, CPU)
        assert t.is_contiguous() and t.shape == (5, 3) and t.dtype == dtype
        assert t.data_ptr() - h.raw.data_ptr() == gb.BAND  # exactly one band in front ...
        assert h.raw.numel() == 2 * gb.BAND + t.numel() * t.element_size()  # ... one behind, no slack
        assert h.raw.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0  # the allocator's alignment, kept
        assert bool((h.raw[:gb.BAND] == gb.BAND_BYTE).all()) and bool((h.raw[h.hi:] == gb.BAND_BYTE).all())
        assert bool((h.raw[h.lo:h.hi] == gb.PAYLOAD_BYTE).all())
    a, ha = gb.guarded((7,), torch.float32, CPU)
    b, hb = gb.guarded((7,), torch.float32, CPU, misalign=4)
    assert (b.data_ptr() - hb.raw.data_ptr()) - (a.data_ptr() - ha.raw.data_ptr()) == 4
    assert b.data_ptr() % 16 == 4 and hb.raw.numel() == ha.raw.numel() + 4
    with pytest.raises(AssertionError):
        gb.guarded((7,), torch.float32, CPU, misalign=8)
    c, hc = gb.guarded_copy(np.arange(6, dtype=np.int64).reshape(3, 2), 5, CPU, rows=[1])
    assert c.tolist() == [[0, 1], [5, 5], [4, 5]]
    assert bool((hc.raw[:gb.BAND].view(torch.int64) == 5).all()) and bool((hc.raw[hc.hi:].view(torch.int64) == 5).all())
    d, hd = gb.guarded_copy(np.ones(3, np.float32), float("nan"), CPU, misalign=4)
    assert d.data_ptr() % 16 == 4 and d.tolist() == [1.0, 1.0, 1.0]
    assert bool(torch.isnan(hd.raw[4:hd.lo].view(torch.float32)).all())
    e, he = gb.guarded((0, 3), torch.float32, CPU)  # an empty payload: two bands back to back
    assert e.shape == (0, 3)
    he.assert_bands_intact()
    he.assert_untouched(slice(0, 0))


def test_correct_kernel_passes():
    outs = []
    for fill in gb.FLOAT_FILLS:
        out, ho, hx = _run(k_correct, fill)
        ho.assert_bands_intact()
        hx.assert_bands_intact()
        ho.assert_untouched(slice(COUNT, N))
        ho.assert_untouched(torch.arange(N) >= COUNT)
        assert out[:COUNT].tolist() == [2.0 * (i + 1) for i in range(COUNT)]
        outs.append(out)
    gb.assert_same_bits(*outs)
    sums = [_run(k_sum_correct, fill, n_out=1)[0] for fill in gb.FLOAT_FILLS]
    gb.assert_same_bits(*sums)


def test_write_past_the_end_fails_the_band_check():
    out, ho, _ = _run(k_writes_past_end, 1e30)
    with pytest.raises(AssertionError, match="0 B past the end"):
        ho.assert_bands_intact()


def test_write_before_the_start_fails_the_band_check():
    out, ho, _ = _run(k_writes_before_start, 1e30)
    with pytest.raises(AssertionError, match="4 B before the start"):
        ho.assert_bands_intact()
    out, ho, _ = _run(k_writes_before_start, 1e30, dtype=torch.float16)  # (a narrower element all the same)
    with pytest.raises(AssertionError, match="2 B before the start"):
        ho.assert_bands_intact()


def test_row_past_the_count_fails_assert_untouched():
    out, ho, _ = _run(k_writes_row_past_count, 1e30)
    ho.assert_bands_intact()  # (inside the payload: only the row check sees it)
    with pytest.raises(AssertionError, match=f"the first row {COUNT}"):
        ho.assert_untouched(slice(COUNT, N))
    ho.assert_untouched(slice(COUNT + 1, N))


def test_read_past_the_end_fails_the_ab_comparison():
    a, ho, hx = _run(k_sum_reads_past_end, gb.FLOAT_FILLS[0], n_out=1)
    b, _, _ = _run(k_sum_reads_past_end, gb.FLOAT_FILLS[1], n_out=1)
    ho.assert_bands_intact()
    hx.assert_bands_intact()  # (a read leaves no trace: only the two fills tell)
    with pytest.raises(AssertionError, match="depends on the fill"):
        gb.assert_same_bits(a, b)
    # index data: two valid values, a gather that reads one index too many
    idx = np.array([2, 0, 1], np.int64)
    src = torch.tensor([10.0, 20.0, 30.0])
    res = []
    for fill in (0, 2):
        i, _ = gb.guarded_copy(idx, fill, CPU)
        res.append(src[_past_end(i)].sum().reshape(1))
    with pytest.raises(AssertionError, match="depends on the fill"):
        gb.assert_same_bits(*res)


def test_same_bits_is_bytewise():
    nan = torch.tensor([float("nan")])
    gb.assert_same_bits(nan, nan.clone())  # NaN == NaN here
    with pytest.raises(AssertionError):
        gb.assert_same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not gb.same_bits(torch.zeros(2), torch.zeros(3))
