"""Input gradients of the field, dL/dx (ncn_field_bwd_dx) and dL/dd (ncn_field_bwd_mlp_din), against
the torch CPU oracle (oracle/field_ref.py) in both MFMA operand precisions.

Reference: field_ref.field_forward_autograd with the kernel's rounding points (emulate=precision,
bwd_scale = 128 for fp16 at loss scale 1, 1 for bf16, return_enc=True).  `d.grad` is the reference
of dL/dd; `enc0.grad` (dL/denc as the grid backward receives it) contracted with the host Jacobian of
the encoding at the fp32 cell positions (tests/field_input_grad_check.py, itself checked against
finite differences in tests/test_field_input_jacobian.py), divided by the box extent, is the
reference of dL/dx.  Parameters: field_ref.init_params(seed, table_init=0.5) copied into NGPMT, as
tests/test_gpu_field.py does; upstream gradients randn.

Bound: rel-L2 of each of the six columns <= the project's backward bound TOL[precision]["bwd"]
(2e-2 fp16, 5e-2 bf16: the bound on the table gradient, which is formed from the same dE).
Measured worst column (profiles/round7/input_grad_tests.log; the tests print every figure before
asserting): dL/dx 1.6e-5 (fp16) / 2.7e-5 (bf16), dL/dd 3.3e-4 / 2.9e-3 (the n = 1 case), density
dL/dx 6.3e-6 / 9.8e-8; table gradient with vs without input gradients 2e-8.

Further: two backwards are bit-identical; with input gradients on, the weight gradients are
bit-identical to the run without and the table gradient agrees within rel-L2 2e-4 (the f32-atomics
bound of test_field_morton_window_order); with every parameter frozen the input gradients are the
same bit for bit and the flat gradient buffer stays zero; a static-capacity call (device count 3001
of 4099) leaves rows >= 3001 exactly zero and rows < 3001 bit-identical to the plain n = 3001 run;
density(x) differentiates into x (the sigma-only chain)."""
import functools

import pytest
import torch

from field_input_grad_check import enc_jacobian
from oracle import field_ref
from test_gpu_field import TOL, _inputs, _model_from_oracle

pytestmark = pytest.mark.gpu

SEED_P = 5
EXTENT = 1.0  # xyz_max - xyz_min at scale 0.5


@functools.lru_cache(maxsize=None)
def _params():
    return field_ref.init_params(seed=SEED_P, table_init=0.5)


@functools.lru_cache(maxsize=None)
def _case(n, seed):
    x, d = _inputs(n, seed)
    d = d * (0.5 + torch.rand(n, 1, generator=torch.Generator().manual_seed(seed + 100)))  # |d| != 1: the normalisation
    g = torch.Generator().manual_seed(seed + 7)
    return x, d, torch.randn(n, generator=g), torch.randn(n, 3, generator=g)


def _dx_from_enc_grad(x, enc_grad, P, levels):
    x01 = (x - (-0.5)) / EXTENT
    J = enc_jacobian(x01, P.table, levels, torch.float32)  # (N,32,3) fp64
    return torch.einsum("nf,nfk->nk", enc_grad.double(), J) / EXTENT


@functools.lru_cache(maxsize=None)
def _reference(precision, n, seed):
    """(dL/dx, dL/dd) fp64 of the oracle, computed once per case and shared (never modified)."""
    P, levels = _params()
    x, d, gs, gr = _case(n, seed)
    dr = d.clone().requires_grad_(True)
    sig, rgb, _, enc0 = field_ref.field_forward_autograd(x, dr, P, levels, emulate=precision,
                                                         bwd_scale=128 if precision == "fp16" else 1, return_enc=True)
    ((sig * gs).sum() + (rgb * gr).sum()).backward()
    return _dx_from_enc_grad(x, enc0.grad, P, levels), dr.grad.double()


@functools.lru_cache(maxsize=None)
def _reference_density(precision, n, seed):
    """dL/dx of the sigma-only chain: field_forward_autograd's sigma_net part with its rounding points."""
    P, levels = _params()
    x, _, gs, _ = _case(n, seed)
    q = field_ref._rounder(False, precision)
    rg = field_ref._grad_rounder(precision, 128 if precision == "fp16" else 1)
    x01 = (x - (-0.5)) / EXTENT
    enc0 = field_ref.hash_encode(x01, P.table, levels).requires_grad_(True)
    h = rg(q(torch.relu(rg(q(rg(enc0)) @ q(P.W1).t()))) @ q(P.W2).t())
    sig = field_ref._TruncExp.apply(h[:, 0])
    (sig * gs).sum().backward()
    return _dx_from_enc_grad(x, enc0.grad, P, levels)


def _run(m, dev, x, d, gs, gr, grads=True, n_dev=None):
    """One forward + backward on the device -> (x.grad, d.grad) on the host (None without grads)."""
    xd, dd = x.to(dev).requires_grad_(grads), d.to(dev).requires_grad_(grads)
    kw = {} if n_dev is None else {"n_samples_dev": torch.tensor([n_dev], dtype=torch.int32, device=dev)}
    out = m(xd, dd, **kw)
    (out["sigmas"] * gs.to(dev)).sum().add_((out["rgbs"] * gr.to(dev)).sum()).backward()
    if not grads:
        return None, None
    return xd.grad.cpu(), dd.grad.cpu()


def _col_errors(got, ref):
    return [float((got[:, k].double() - ref[:, k]).norm() / ref[:, k].norm().clamp_min(1e-30)) for k in range(3)]


def _check_columns(tag, precision, gx, gd, ref_x, ref_d):
    ex, ed = _col_errors(gx, ref_x), (_col_errors(gd, ref_d) if gd is not None else [])
    print(f"{tag} {precision} rel-L2 dL/dx {' '.join(f'{e:.3e}' for e in ex)} | dL/dd {' '.join(f'{e:.3e}' for e in ed)}")
    bound = TOL[precision]["bwd"]
    assert all(e <= bound for e in ex + ed), (tag, ex, ed)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 17, 4099])
def test_input_grads(dev, precision, n):
    P, _ = _params()
    m = _model_from_oracle(P, dev, precision)
    x, d, gs, gr = _case(n, 2)
    gx, gd = _run(m, dev, x, d, gs, gr)
    ref_x, ref_d = _reference(precision, n, 2)
    assert gx.shape == (n, 3) and gd.shape == (n, 3) and gx.dtype == torch.float32
    _check_columns(f"input grads n {n}", precision, gx, gd, ref_x, ref_d)
    gx2, gd2 = _run(m, dev, x, d, gs, gr)  # no atomics: bit-identical run to run
    assert torch.equal(gx, gx2) and torch.equal(gd, gd2)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_input_grads_morton_windows(dev, precision):
    """n = 8195 with sort_samples: three Morton windows, the last one partial; dE is in processing
    order, the outputs in sample order."""
    n = 8195
    P, _ = _params()
    m = _model_from_oracle(P, dev, precision)
    m.sort_samples = True
    x, d, gs, gr = _case(n, 3)
    gx, gd = _run(m, dev, x, d, gs, gr)
    ref_x, ref_d = _reference(precision, n, 3)
    _check_columns(f"input grads sorted n {n}", precision, gx, gd, ref_x, ref_d)
    gx2, gd2 = _run(m, dev, x, d, gs, gr)
    assert torch.equal(gx, gx2) and torch.equal(gd, gd2)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_input_grads_device_count(dev, precision):
    """Capacity 4099 with a device count of 3001: rows >= 3001 exactly zero, rows < 3001 bit-identical
    to the plain n = 3001 run (the arithmetic is per sample)."""
    cap, cnt = 4099, 3001
    P, _ = _params()
    m = _model_from_oracle(P, dev, precision)
    x, d, gs, gr = _case(cap, 2)
    gx, gd = _run(m, dev, x, d, gs, gr, n_dev=cnt)
    assert gx.shape == (cap, 3) and gd.shape == (cap, 3)
    assert float(gx[cnt:].abs().max()) == 0.0 and float(gd[cnt:].abs().max()) == 0.0
    px, pd = _run(m, dev, x[:cnt].contiguous(), d[:cnt].contiguous(), gs[:cnt].contiguous(), gr[:cnt].contiguous())
    assert torch.equal(gx[:cnt], px) and torch.equal(gd[:cnt], pd)
    assert float(px.abs().max()) > 0 and float(pd.abs().max()) > 0


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_input_grads_leave_parameter_grads(dev, precision):
    """With input gradients on, the weight gradients are bit-identical to the run without and the
    table gradient agrees within the atomics bound; with every parameter frozen the input gradients
    are the same bit for bit and the flat gradient stays zero."""
    n = 4099
    P, _ = _params()
    m = _model_from_oracle(P, dev, precision)
    x, d, gs, gr = _case(n, 2)
    nt = m._n_table
    _run(m, dev, x, d, gs, gr, grads=False)
    g0 = m.flat_grad().clone()
    m.flat_grad().zero_()
    gx, gd = _run(m, dev, x, d, gs, gr)
    g1 = m.flat_grad().clone()
    assert float(g0[nt:].abs().max()) > 0
    assert torch.equal(g0[nt:], g1[nt:])
    rel = float((g1[:nt] - g0[:nt]).norm() / g0[:nt].norm())
    print(f"table gradient with vs without input grads {precision}: rel-L2 {rel:.3e}")
    assert rel <= 2e-4
    m.flat_grad().zero_()
    for p in m.parameters():
        p.requires_grad_(False)
    fx, fd = _run(m, dev, x, d, gs, gr)
    assert torch.equal(fx, gx) and torch.equal(fd, gd)
    assert float(m.flat_grad().abs().max()) == 0.0


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [17, 4099])
def test_density_input_grad(dev, precision, n):
    P, _ = _params()
    m = _model_from_oracle(P, dev, precision)
    x, _, gs, _ = _case(n, 2)
    xd = x.to(dev).requires_grad_(True)
    (m.density(xd) * gs.to(dev)).sum().backward()
    assert xd.grad is not None and xd.grad.shape == (n, 3)
    _check_columns(f"density n {n}", precision, xd.grad.cpu(), None, _reference_density(precision, n, 2), None)
    x2 = x.to(dev).requires_grad_(True)
    (m.density(x2) * gs.to(dev)).sum().backward()
    assert torch.equal(xd.grad, x2.grad)
