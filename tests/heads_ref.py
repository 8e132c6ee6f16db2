"""Reference of the semantic / normal heads and of the extra-channel compositing (test infrastructure).

sem_net / norm_net (the reference's models/ngp_mt.py:116-140, 222-227) restated on top of
oracle.field_ref: a tcnn FullyFusedMLP(16 -> 64 -> 64 -> n_out), ReLU, no output activation, no biases,
in tcnn's padded shapes Wa (64, 16), Wb (64, 64), Wc (16 ceil(n_out / 16), 64), on the 16 features h that
field_ref.field_forward_autograd returns.  Same operand emulation as the field's reference: the
operands of every layer (weights, h, the two hidden activations) are rounded to the MFMA operand
type in the forward (field_ref._rounder, straight-through in the backward), and with `bwd_scale` the
upstream gradient and the two pre-ReLU gradients are rounded where csrc/heads.hip rounds them
(field_ref._grad_rounder).  The head's dL/dh flows into h, whose own gradient rounder (inside
field_forward_autograd) rounds the sum of every consumer's contribution once.  Differentiable with
torch autograd; the tensors' dtype is kept (fp64 tensors: the same rounding points, fp64 accumulation).

The extra-channel compositing is restated in fp64 NumPy.
"""
import math

import numpy as np
import torch

from oracle import field_ref


def head_shapes(n_out):
    return ((64, 16), (64, 64), (16 * ((n_out + 15) // 16), 64))


def init_head(n_out, seed):
    """Xavier-uniform (Wa, Wb, Wc) in tcnn's padded shapes."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(o, i, generator=g) * 2 - 1) * math.sqrt(6.0 / (o + i)) for o, i in head_shapes(n_out)]


def head_forward(h, W, n_out, emulate=None, bwd_scale=None):
    """(N, 16) features -> (N, n_out) outputs: the unrounded accumulators of the last layer."""
    Wa, Wb, Wc = W
    q = field_ref._rounder(False, emulate)
    rg = field_ref._grad_rounder(emulate, bwd_scale)
    a = torch.relu(rg(q(h) @ q(Wa).t()))
    b = torch.relu(rg(q(a) @ q(Wb).t()))
    return rg(q(b) @ q(Wc).t())[:, :n_out]


def forward_with_heads(x, d, P, levels, heads, emulate=None, bwd_scale=None):
    """field_ref.field_forward_autograd and every head of `heads` = [(W, n_out), ...] on its h
    -> (sigmas, rgbs, [head outputs])."""
    sig, rgb, h = field_ref.field_forward_autograd(x, d, P, levels, emulate=emulate, bwd_scale=bwd_scale)
    return sig, rgb, [head_forward(h, W, n_out, emulate, bwd_scale) for W, n_out in heads]


def composite_extra(ws, raws, rays_a, n_rays):
    """rend[r][c] = sum over ray r's samples of ws[s] raws[s][c] in fp64 -> (rend (R, C) f64, the sums of
    the terms' magnitudes (R, C) f64, the sample counts (R)).  Rows outside every ray's range are not read."""
    C = raws.shape[1]
    rend, mag, cnt = np.zeros((n_rays, C)), np.zeros((n_rays, C)), np.zeros(n_rays, np.int64)
    for ray, start, n in np.asarray(rays_a, np.int64):
        t = ws[start:start + n, None].astype(np.float64) * raws[start:start + n].astype(np.float64)
        rend[ray], mag[ray], cnt[ray] = t.sum(0), np.abs(t).sum(0), n
    return rend, mag, cnt


def composite_extra_bw(dL_drend, ws, raws, rays_a):
    """-> (dL_dws (S), dL_draws (S, C)) in fp64; zero outside every ray's range."""
    dws, draws = np.zeros(ws.shape[0]), np.zeros(raws.shape)
    for ray, start, n in np.asarray(rays_a, np.int64):
        g = dL_drend[ray].astype(np.float64)
        sl = slice(start, start + n)
        draws[sl] = g[None, :] * ws[sl, None].astype(np.float64)
        dws[sl] = (raws[sl].astype(np.float64) * g[None, :]).sum(1)
    return dws, draws
