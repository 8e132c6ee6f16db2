"""The split MLP backward (ncn_field_bwd_mlp_part parts 1 + 2: the rgb pass, then the sigma pass
with sigma_net's K=32 fragments held in registers) against the one-pass ncn_field_bwd_mlp at the
shapes where the sigma pass's step loop changes path, bit for bit in fp16 and bf16:

 * n = 1, 15, 17: one partial group; one sample past a full group;
 * n = 129: one group past a full 8-group step (a step with a single group: phase 2 pairs it with
   zeros);
 * n = 16 * 8 * 3 + 5 = 389 (25 groups) on sigma-pass grids of 1, 2 and 3 workgroups: the last step
   of a workgroup has an odd group count (1 group on grid 1, 1 group on the second workgroup of
   grid 2).  The one-pass grid of these sizes is one workgroup (ncn_field_bwd_blocks) and the entry
   point caps the sigma pass at twice that, so a request for 3 runs 2: the case checks the cap;
 * a device count n_dev = n - 7 below the capacity, and n_dev = 0 (no group at all);
 * an fp16 overflow of the encoding gradient: the level maximum is inf in both forms.

On a grid equal to the one-pass grid the slab tiles, the dE workspace and the level_max rows are
the same bits (NaN payloads included: compared as integers).  On the two-workgroup grids the dW
tiles are split over two slab rows, so dE and the level maxima are compared bit for bit and the
reduced weight gradient to 1e-5 (test_gpu_split_step's bound for regrouped slab rows)."""
import pytest
import torch

from ncnerf_amd import _lib
from ncnerf_amd.ngp_mt import N_W, NGPMT

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(dev, precision):
    if precision not in _MODELS:
        g = torch.Generator(device=dev).manual_seed(3)
        m = NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev)
        with torch.no_grad():
            m.flat_params()[: m._n_table].uniform_(-0.3, 0.3, generator=g)
        if m.amp_state is not None:
            m.amp_state[0] = 4.0
        _MODELS[precision] = m
    return _MODELS[precision]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _compare(dev, precision, n, count, grid2, overflow=False):
    """count: the device count (None = the capacity n); grid2: the sigma pass's requested grid."""
    m = _model(dev, precision)
    g = torch.Generator(device=dev).manual_seed(1000 * n + (count or 0))
    x = (torch.rand(n, 3, device=dev, generator=g) - 0.5) * 0.99
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    with torch.no_grad():
        _, _, enc, packed, order = m._field_fwd(x, d, n_dev, 0, True)
    assert order is None
    dsig = torch.randn(n, device=dev, generator=g) * 1e-2
    drgb = torch.randn(n, 3, device=dev, generator=g) * 1e-2
    if overflow:
        dsig[n // 2] = 3e4  # times the chain's scale (4 x 128): past fp16's range
    L = _lib.lib()
    nb_full = int(L.ncn_field_bwd_blocks(n))
    assert nb_full == 1
    dE_n = int(L.ncn_field_bwd_dE_floats(n))
    scale = m._bwd_loss_scale()

    s0 = torch.full((nb_full * N_W,), float("nan"), device=dev)
    e0 = torch.zeros(dE_n, device=dev)
    l0 = torch.full((16 * 256,), -1.0, device=dev)
    _lib.call("ncn_field_bwd_mlp", x, d, n, n_dev, order, packed, m._prec, enc, dsig, drgb, scale, s0, e0, l0)
    w0 = torch.zeros(N_W, device=dev)
    _lib.call("ncn_field_reduce_wgrad", s0, nb_full, w0)

    g2 = min(grid2, int(L.ncn_field_bwd_part_blocks(n, 2)))
    assert g2 == min(grid2, 2)
    s1 = torch.full((max(nb_full, g2) * N_W,), float("nan"), device=dev)
    e1 = torch.zeros(dE_n, device=dev)
    l1 = torch.full((16 * 256,), -1.0, device=dev)
    stash = torch.empty(int(L.ncn_field_bwd_stash_floats(n)), device=dev)
    for part, ds, nb in ((1, None, nb_full), (2, dsig, grid2)):
        _lib.call("ncn_field_bwd_mlp_part", x, d, n, n_dev, order, packed, m._prec, enc, ds, None, drgb, scale,
                  part, nb, s1, e1, l1, stash)
    w1 = torch.zeros(N_W, device=dev)
    _lib.call("ncn_field_reduce_wgrad_parts", s1, g2, nb_full, w1)
    torch.cuda.synchronize()

    assert torch.equal(_bits(e0), _bits(e1))
    assert torch.equal(_bits(l0[:16]), _bits(l1[:16]))
    if g2 == nb_full:
        assert torch.equal(_bits(s0), _bits(s1))
    elif count == 0:
        assert not w0.any() and not w1.any()
    elif not overflow:
        assert float((w1 - w0).norm() / w0.norm()) < 1e-5
    if overflow:
        assert torch.isinf(l0[:16]).any() and torch.isinf(l1[:16]).any()
    else:
        assert torch.isfinite(l0[:16]).all()
        live = n if count is None else count
        assert (live == 0) == (float(l0[:16].max()) == 0.0)
    return l0[:16]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 15, 17, 129])
def test_partial_groups_and_steps(dev, precision, n):
    _compare(dev, precision, n, None, 1)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("grid2", [1, 2, 3])
def test_odd_group_count_on_small_grids(dev, precision, grid2):
    _compare(dev, precision, 16 * 8 * 3 + 5, None, grid2)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("n,count,grid2", [(389, 382, 1), (389, 382, 2), (129, 122, 1), (389, 0, 1), (389, 0, 2)])
def test_device_count(dev, precision, n, count, grid2):
    _compare(dev, precision, n, count, grid2)


@pytest.mark.parametrize("grid2", [1, 2])
def test_fp16_overflow_keeps_inf_level_max(dev, grid2):
    _compare(dev, "fp16", 389, None, grid2, overflow=True)
