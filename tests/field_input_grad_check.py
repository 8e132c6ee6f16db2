"""Host reference of the hash-grid encoding's input Jacobian (the check of ncn_field_bwd_dx).

The encoding of oracle/field_ref.py is, per level, a trilinear interpolation of the 8 table entries
at the corners of the cell floor(scale * x01 + 0.5); inside a cell it is linear along each axis, so
  d enc[l, f] / d x01_k = scale_l * sum over the 4 corner pairs of the other two axes of
                          w_other * (T[hi_k]_f - T[lo_k]_f),
piecewise constant along k.  Everything here is fp64 arithmetic on the oracle's own pieces
(`field_ref._grid_index`, the `levels` list); `pos_dtype` chooses how the cell position is formed:
torch.float32 rounds scale * x01 + 0.5 to fp32 as the kernels' fmaf does (the cell and the weights
the kernel sees), torch.float64 keeps it in fp64 (for finite differences)."""
import torch

from oracle import field_ref

_CORNER = torch.tensor([[(c >> dim) & 1 for dim in range(3)] for c in range(8)], dtype=torch.int64)  # (8, 3)


def level_parts(x01, lv, pos_dtype):
    """(frac (N,3) fp64, table row index (N,8) int64) of one level, corner bit d -> +1 along dim d."""
    pos = x01.double() * lv["scale"] + 0.5  # (an fp32 x01 times the fp32 scale is exact in fp64)
    if pos_dtype == torch.float32:
        pos = pos.float()
    fl = torch.floor(pos)
    frac = (pos - fl).double()
    pg = fl.to(torch.int64) & 0xFFFFFFFF
    pc = (pg[:, None, :] + _CORNER[None]) & 0xFFFFFFFF
    return frac, field_ref._grid_index(pc, lv["res"], lv["params"]) + lv["offset"]


def encode(x01, table, levels, pos_dtype):
    """(N, 32) fp64 encoding, level-major, from the pieces the Jacobian uses."""
    tab = table.double()
    out = []
    for lv in levels:
        frac, idx = level_parts(x01, lv, pos_dtype)
        wd = torch.where(_CORNER[None].bool(), frac[:, None, :], 1 - frac[:, None, :])  # (N,8,3)
        w = wd[..., 0] * wd[..., 1] * wd[..., 2]
        out.append((w[..., None] * tab[idx]).sum(1))
    return torch.cat(out, 1)


def enc_jacobian(x01, table, levels, pos_dtype):
    """(N, 32, 3) fp64: d enc / d x01."""
    tab = table.double()
    sign = (2 * _CORNER - 1).double()  # (8,3): +1 on the hi corner of a dim, -1 on the lo one
    out = []
    for lv in levels:
        frac, idx = level_parts(x01, lv, pos_dtype)
        wd = torch.where(_CORNER[None].bool(), frac[:, None, :], 1 - frac[:, None, :])  # (N,8,3)
        v = tab[idx]  # (N,8,2)
        cols = []
        for k in range(3):
            a, b = [j for j in range(3) if j != k]
            w = wd[..., a] * wd[..., b] * sign[None, :, k]  # (N,8)
            cols.append((w[..., None] * v).sum(1) * lv["scale"])  # (N,2)
        out.append(torch.stack(cols, -1))  # (N,2,3)
    return torch.cat(out, 1)


def near_boundary(x01, levels, h):
    """(N,) bool: a cell boundary of some level lies within h (in x01) of the point along some axis."""
    near = torch.zeros(x01.shape[0], dtype=torch.bool)
    for lv in levels:
        frac, _ = level_parts(x01, lv, torch.float64)
        m = h * lv["scale"]
        near |= ((frac <= m) | (frac >= 1 - m)).any(1)
    return near
