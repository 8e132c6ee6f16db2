"""The host Jacobian of the hash-grid encoding (tests/field_input_grad_check.py), which the GPU tests
hold ncn_field_bwd_dx to, checked on its own: against central differences of an fp64 encoding built
from the same pieces, and that encoding against the oracle's hash_encode."""
import torch

from field_input_grad_check import enc_jacobian, encode, near_boundary
from oracle import field_ref

N, H = 512, 1e-7


def _setup():
    P, levels = field_ref.init_params(seed=11, table_init=0.5)
    g = torch.Generator().manual_seed(12)
    x01 = torch.rand(N, 3, generator=g)  # fp32 values: exact in fp64, and hash_encode sees the same points
    return P.table, levels, x01


def test_jacobian_matches_central_differences():
    """Inside a cell the encoding is linear along each axis, so a central difference is exact up to
    fp64 rounding: ~2^-53 * 8 corners * max|T| per encode and the rounding of x +- h (2^-53 / h
    relative), both far below the bound 1e-6 * scale_l * max|T| per level — while a wrong sign, weight
    or corner is an error of order scale_l * max|T|.  Samples with a cell boundary within h along any
    axis on any level (the difference straddles a kink) are left out: 6 h sum_l scale_l = 0.25 %
    expected, at most 2 %."""
    table, levels, x01 = _setup()
    xd = x01.double()
    near = near_boundary(xd, levels, H)
    share = float(near.float().mean())
    expected = 6 * H * sum(lv["scale"] for lv in levels)
    print(f"left out: {share:.4%} (expected {expected:.4%})")
    assert share <= 0.02
    J = enc_jacobian(xd, table, levels, torch.float64)[~near]
    assert J.shape == (int((~near).sum()), 32, 3)
    tmax = float(table.abs().max())
    tol = torch.tensor([1e-6 * lv["scale"] * tmax for lv in levels], dtype=torch.float64).repeat_interleave(2)
    worst = 0.0
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[k] = H
        fd = (encode(xd + e, table, levels, torch.float64) - encode(xd - e, table, levels, torch.float64)) / (2 * H)
        err = (J[..., k] - fd[~near]).abs()
        worst = max(worst, float((err / tol[None]).max()))
        assert bool((err <= tol[None]).all()), (k, float((err / tol[None]).max()))
    assert float(J.abs().max()) > 1.0  # (not vacuous: the finest level's slopes are ~ scale * |T|)
    print(f"worst |J - FD| / bound: {worst:.3e}")


def test_fp64_encode_matches_oracle():
    """The fp64 encoding differs from field_ref.hash_encode (fp32 position and weights) by the
    rounding of the position (half an ulp of pos < 1024: 2^-14, moving each of three weight factors)
    over eight corners: 24 * 2^-14 * max|T|."""
    table, levels, x01 = _setup()
    ref = field_ref.hash_encode(x01, table, levels).double()
    got = encode(x01.double(), table, levels, torch.float64)
    err = float((got - ref).abs().max())
    bound = 24 * 2.0 ** -14 * float(table.abs().max())
    print(f"max |enc64 - hash_encode| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # the fp32-position form (the cell and weights the kernel sees) agrees as closely
    got32 = encode(x01.double(), table, levels, torch.float32)
    assert float((got32 - ref).abs().max()) <= bound
