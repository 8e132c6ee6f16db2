"""Input gradients (dL/dx, dL/dd) of a model with the semantic / normal heads: pose refinement with
the semantic and normal terms on.  dL/dd leaves the split backward's rgb part
(ncn_field_bwd_mlp_rgb_din, include/ncnerf_input_grad.h), dL/dx is ncn_field_bwd_dx over the encoding
gradient the sigma part left, which carries every head's dL/dh.

Reference (tests/test_gpu_field_input_grad.py's, with the heads of tests/heads_ref.py on its h):
field_ref.field_forward_autograd with the kernel's rounding points (emulate=precision, bwd_scale = 128
for fp16 at loss scale 1, 1 for bf16, return_enc=True) and heads_ref.head_forward on the returned h;
`d.grad` is the reference of dL/dd, `enc0.grad` contracted with the host Jacobian of the encoding
(tests/field_input_grad_check.enc_jacobian, computed once per n) and divided by the box extent is the
reference of dL/dx.  Parameters: tests/test_gpu_heads.py's (_field, _head, _model); inputs with
|d| != 1; upstream gradients randn.

Bound: rel-L2 of each of the six columns <= the project's backward bound TOL[precision]["bwd"] (2e-2
fp16, 5e-2 bf16), as tests/test_gpu_field_input_grad.py for the same quantities.  Every figure is
printed before it is asserted.
Measured worst columns (profiles/heads_input_grad/gpu_tests.txt): dL/dx 9.0e-3 (fp16; n = 1, n_out
17) / 1.4e-2 (bf16; n = 1, n_out 40), at n = 4099 5.0e-4 / 3.9e-3; dL/dd 2.8e-4 / 2.3e-3 (n = 17), at
n = 4099 2.1e-4 / 1.7e-3; the heads' gradient alone, dL/dx 5.1e-4 / 4.1e-3; table gradient with vs
without input gradients 1.5e-8.  End to end the semantic term (weight 0.1, freshly initialised heads)
moves |dR.grad| = 1.5e-3 by 8.2e-7 and |dT.grad| = 1.4e-5 by 4.0e-6; two runs without it are bit-identical.

Further: two backwards are bit-identical; with upstream gradients on the heads alone dL/dx is
non-zero and within the bound, dL/dd exactly zero; with a loss on sigmas and rgbs alone both
gradients equal the heads-off model's bit for bit; the entry point's dL_ddirs equals
ncn_field_bwd_mlp_din's and its slab / stash / level_max equal part 1's bit for bit; a static-capacity
call leaves rows past the device count exactly zero; with input gradients on the weight gradients
are bit-identical to the run without (the table's within the f32-atomics bound 2e-4), and with every
parameter frozen the input gradients are unchanged and the flat gradient stays zero; end to end,
the semantic term reaches the pose of a DeviceRayDataset(optimize_ext=True, semantics=...)."""
import functools

import pytest
import torch

import heads_ref
from field_input_grad_check import enc_jacobian
from ncnerf_amd import _lib
from ncnerf_amd.data import DeviceRayDataset
from ncnerf_amd.losses import NeRFMTLoss
from ncnerf_amd.ngp_mt import NGPMT, N_W
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import make_cameras
from ncnerf_amd.trainer import HYPERSIM_HPARAMS
from oracle import field_ref
from test_gpu_field import TOL, _inputs
from test_gpu_field_input_grad import _col_errors
from test_gpu_heads import _field, _head, _model

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp16", "bf16"]
EXTENT = 1.0  # xyz_max - xyz_min at scale 0.5
SEED = 2


@functools.lru_cache(maxsize=None)
def _case(n, n_out):
    """x, d with |d| != 1 (tests/test_gpu_field_input_grad._case), upstream gradients of the four outputs."""
    x, d = _inputs(n, SEED)
    d = d * (0.5 + torch.rand(n, 1, generator=torch.Generator().manual_seed(SEED + 100)))
    g = torch.Generator().manual_seed(SEED + 7)
    ups = {"sigmas": torch.randn(n, generator=g), "rgbs": torch.randn(n, 3, generator=g),
           "sems": torch.randn(n, n_out, generator=g), "norms": torch.randn(n, 3, generator=g)}
    return x, d, ups


@functools.lru_cache(maxsize=None)
def _jacobian(n):
    """d enc / d x01 at the case's positions, (n, 32, 3) fp64: once per n, shared by every reference."""
    P, levels = _field()
    x, _ = _inputs(n, SEED)
    return enc_jacobian((x - (-0.5)) / EXTENT, P.table, levels, torch.float32)


@functools.lru_cache(maxsize=None)
def _reference(precision, n, n_out, keys):
    """(dL/dx, dL/dd) fp64 of the oracle for the upstream gradients named by `keys`; computed once per
    case and never modified."""
    P, levels = _field()
    x, d, ups = _case(n, n_out)
    scale = 128 if precision == "fp16" else 1
    dr = d.clone().requires_grad_(True)
    sig, rgb, h, enc0 = field_ref.field_forward_autograd(x, dr, P, levels, emulate=precision, bwd_scale=scale,
                                                         return_enc=True)
    outs = {"sigmas": sig, "rgbs": rgb,
            "sems": heads_ref.head_forward(h, _head(n_out, 11), n_out, emulate=precision, bwd_scale=scale),
            "norms": heads_ref.head_forward(h, _head(3, 12), 3, emulate=precision, bwd_scale=scale)}
    sum((outs[k] * ups[k]).sum() for k in keys).backward()
    dx = torch.einsum("nf,nfk->nk", enc0.grad.double(), _jacobian(n)) / EXTENT
    dd = dr.grad.double() if dr.grad is not None else torch.zeros(n, 3, dtype=torch.float64)
    return dx, dd


ALL = ("sigmas", "rgbs", "sems", "norms")


def _run(m, dev, x, d, ups, keys=ALL, grads=True, n_dev=None):
    """One forward + backward on the device -> (x.grad, d.grad) on the host (None without grads)."""
    xd, dd = x.to(dev).requires_grad_(grads), d.to(dev).requires_grad_(grads)
    kw = {} if n_dev is None else {"n_samples_dev": torch.tensor([n_dev], dtype=torch.int32, device=dev)}
    out = m(xd, dd, **kw)
    sum((out[k] * ups[k].to(dev)).sum() for k in keys).backward()
    torch.cuda.synchronize()
    if not grads:
        return None, None
    return xd.grad.cpu(), dd.grad.cpu()


def _check_columns(tag, precision, gx, gd, ref_x, ref_d):
    ex, ed = _col_errors(gx, ref_x), (_col_errors(gd, ref_d) if ref_d is not None else [])
    print(f"{tag} {precision} rel-L2 dL/dx {' '.join(f'{e:.3e}' for e in ex)} | dL/dd {' '.join(f'{e:.3e}' for e in ed)}")
    bound = TOL[precision]["bwd"]
    assert all(e <= bound for e in ex + ed), (tag, ex, ed)


# ---------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n_out", [3, 17, 40])
@pytest.mark.parametrize("n", [1, 17, 4099])
def test_input_grads_with_heads(dev, n, n_out, precision):
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d, ups = _case(n, n_out)
    gx, gd = _run(m, dev, x, d, ups)
    ref_x, ref_d = _reference(precision, n, n_out, ALL)
    assert gx.shape == (n, 3) and gd.shape == (n, 3) and gx.dtype == gd.dtype == torch.float32
    _check_columns(f"heads input grads n {n} n_out {n_out}", precision, gx, gd, ref_x, ref_d)
    gx2, gd2 = _run(m, dev, x, d, ups)  # no atomics on the way to x and d: bit-identical run to run
    assert torch.equal(gx, gx2) and torch.equal(gd, gd2)


# ---------------------------------------------------------------- 2. the heads' gradient alone
@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_gradient_alone_reaches_x_not_d(dev, precision):
    """Upstream gradients on sems and norms only: dL/dx arrives through h -> sigma_net -> encoding,
    dL/dd is exactly zero (the heads read h, never d)."""
    n, n_out = 4099, 17
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d, ups = _case(n, n_out)
    gx, gd = _run(m, dev, x, d, ups, keys=("sems", "norms"))
    ref_x, ref_d = _reference(precision, n, n_out, ("sems", "norms"))
    assert float(ref_d.abs().max()) == 0.0 and float(ref_x.abs().max()) > 0
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    _check_columns(f"heads alone n {n} n_out {n_out}", precision, gx, None, ref_x, None)
    assert gd.shape == (n, 3) and float(gd.abs().max()) == 0.0


# ---------------------------------------------------------------- 3. against the heads-off model
@pytest.mark.parametrize("precision", PRECISIONS)
def test_field_gradients_equal_the_heads_off_model(dev, precision):
    """A loss on sigmas and rgbs alone: x.grad and d.grad of the heads-on model (the split backward)
    equal the heads-off model's (the one-pass backward) bit for bit."""
    n, n_out = 4099, 5
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    m0 = NGPMT(scale=0.5, grid_size=128, precision=precision).to(dev)
    if m0.amp_state is not None:
        m0.amp_state[0] = 1.0
    with torch.no_grad():
        m0.flat_params().copy_(m.flat_params()[:m0.flat_params().numel()])
    x, d, ups = _case(n, n_out)
    gx, gd = _run(m, dev, x, d, ups, keys=("sigmas", "rgbs"))
    hx, hd = _run(m0, dev, x, d, ups, keys=("sigmas", "rgbs"))
    assert float(hx.abs().max()) > 0 and float(hd.abs().max()) > 0
    assert torch.equal(gx, hx) and torch.equal(gd, hd)


# ---------------------------------------------------------------- 4. the entry point directly
def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,n_blocks", [(4099, 0), (17, 1)])
def test_entry_point_against_din_and_part_1(dev, precision, n, n_blocks):
    L = _lib.lib()
    m = _model(dev, precision, 5, _head(5, 11), _head(3, 12))
    x, d, ups = _case(n, 5)
    xd, dd, gr = x.to(dev), d.to(dev), ups["rgbs"].to(dev)
    _, _, enc, packed, _ = m._field_fwd(xd, dd, None, 0, True)
    scale, w_master = m._bwd_loss_scale(), m.flat_params()[m._n_table:]
    n_de, n_st = int(L.ncn_field_bwd_dE_floats(n)), int(L.ncn_field_bwd_stash_floats(n))
    rows = int(L.ncn_field_bwd_part_blocks(n, 1))
    grid = min(n_blocks, rows) if n_blocks > 0 else rows
    nan = float("nan")
    full = lambda k, v: torch.full((k,), v, dtype=torch.float32, device=dev)  # noqa: E731
    # the one-pass form's direction gradient
    din = torch.full((n, 3), nan, device=dev)
    _lib.call("ncn_field_bwd_mlp_din", xd, dd, n, None, None, packed, m._prec, enc, None, gr, scale,
              full(int(L.ncn_field_bwd_blocks(n)) * N_W, nan), full(n_de, 0.0), full(16 * 256, nan), w_master, din)
    # part 1, and the new entry point, on the same grid and on equally prefilled outputs
    a = dict(slab=full(rows * N_W, nan), dE=full(n_de, 0.0), lmax=full(16 * 256, nan), stash=full(n_st, nan))
    _lib.call("ncn_field_bwd_mlp_part", xd, dd, n, None, None, packed, m._prec, enc, None, None, gr, scale, 1, n_blocks,
              a["slab"], a["dE"], a["lmax"], a["stash"])
    b = dict(slab=full(rows * N_W, nan), dE=full(n_de, 0.0), lmax=full(16 * 256, nan), stash=full(n_st, nan))
    got = torch.full((n, 3), nan, device=dev)
    _lib.call("ncn_field_bwd_mlp_rgb_din", xd, dd, n, None, None, packed, m._prec, enc, gr, scale, n_blocks,
              b["slab"], b["dE"], b["lmax"], b["stash"], w_master, got)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert torch.equal(_bits(got), _bits(din))
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    # (what part 1 writes: the tiles of W3..W5 in the grid's slab rows, the whole stash, the level_max rows)
    slab = a["slab"].view(rows, N_W)
    assert bool(torch.isfinite(slab[:grid, 3072:]).all()) and bool(torch.isnan(slab[:grid, :3072]).all())
    assert bool(torch.isfinite(a["stash"][:144 * ((n + 15) // 16)]).all())
    assert float(a["lmax"][:16 * int(L.ncn_field_bwd_blocks(n))].abs().max()) == 0.0
    # dirs == NULL: hipErrorInvalidValue, nothing launched, the outputs untouched
    c = dict(slab=full(rows * N_W, 7.0), dE=full(n_de, 7.0), lmax=full(16 * 256, 7.0), stash=full(n_st, 7.0))
    out = torch.full((n, 3), 7.0, device=dev)
    with pytest.raises(_lib.NcnError, match=r"hipError 1\).*dirs"):
        _lib.call("ncn_field_bwd_mlp_rgb_din", xd, None, n, None, None, packed, m._prec, enc, gr, scale, n_blocks,
                  c["slab"], c["dE"], c["lmax"], c["stash"], w_master, out)
    with pytest.raises(_lib.NcnError, match=r"hipError 1\).*dL_ddirs"):
        _lib.call("ncn_field_bwd_mlp_rgb_din", xd, dd, n, None, None, packed, m._prec, enc, gr, scale, n_blocks,
                  c["slab"], c["dE"], c["lmax"], c["stash"], w_master, None)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in list(c.values()) + [out])


# ---------------------------------------------------------------- 5. device count
@pytest.mark.parametrize("precision", PRECISIONS)
def test_input_grads_with_heads_device_count(dev, precision):
    """Capacity 4099 with a device count of 3001: rows >= 3001 of both gradients exactly zero, rows
    < 3001 bit-identical to the plain n = 3001 run (the arithmetic is per sample)."""
    cap, cnt, n_out = 4099, 3001, 17
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d, ups = _case(cap, n_out)
    gx, gd = _run(m, dev, x, d, ups, n_dev=cnt)
    assert gx.shape == (cap, 3) and gd.shape == (cap, 3)
    assert float(gx[cnt:].abs().max()) == 0.0 and float(gd[cnt:].abs().max()) == 0.0
    px, pd = _run(m, dev, x[:cnt].contiguous(), d[:cnt].contiguous(), {k: v[:cnt].contiguous() for k, v in ups.items()})
    assert torch.equal(gx[:cnt], px) and torch.equal(gd[:cnt], pd)
    assert float(px.abs().max()) > 0 and float(pd.abs().max()) > 0


# ---------------------------------------------------------------- 6. gradients for the weights
@pytest.mark.parametrize("precision", PRECISIONS)
def test_input_grads_with_heads_leave_parameter_grads(dev, precision):
    """With input gradients on, every weight-gradient block (W1..W5, both heads' matrices) is
    bit-identical to the run without and the table gradient agrees within the atomics bound; with
    every parameter frozen the input gradients are the same bit for bit and flat_grad stays zero."""
    n, n_out = 4099, 17
    m = _model(dev, precision, n_out, _head(n_out, 11), _head(3, 12))
    x, d, ups = _case(n, n_out)
    nt = m._n_table
    m.flat_grad().zero_()
    _run(m, dev, x, d, ups, grads=False)
    g0 = m.flat_grad().clone()
    m.flat_grad().zero_()
    gx, gd = _run(m, dev, x, d, ups)
    g1 = m.flat_grad().clone()
    bounds = [nt, nt + 2048, nt + 3072, nt + 5120, nt + 9216, nt + N_W, m._heads[1][2], g0.numel()]
    for name, lo, hi in zip(("W1", "W2", "W3", "W4", "W5", "sem_net", "norm_net"), bounds[:-1], bounds[1:]):
        assert float(g0[lo:hi].abs().max()) > 0, name
        assert torch.equal(g0[lo:hi], g1[lo:hi]), name
    rel = float((g1[:nt] - g0[:nt]).norm() / g0[:nt].norm())
    print(f"heads: table gradient with vs without input grads {precision}: rel-L2 {rel:.3e}")
    assert rel <= 2e-4
    m.flat_grad().zero_()
    for p in m.parameters():
        p.requires_grad_(False)
    fx, fd = _run(m, dev, x, d, ups)
    assert torch.equal(fx, gx) and torch.equal(fd, gd)
    assert float(m.flat_grad().abs().max()) == 0.0


# ---------------------------------------------------------------- 7. end to end
R, K = 128, 5


@pytest.fixture(scope="module")
def e2e(dev):
    """128 rays (two 8x8 patches) of 5 cameras inside the synthetic room (tests/test_gpu_data.py's
    _room_dataset) with a label plane, a heads-on model with every occupancy bit set (as
    tests/test_gpu_pose_grad.py), injected march noise."""
    import data_ref
    V, H, W = 5, 20, 24
    images, _, directions = data_ref.small_scene(V, H, W, seed=6)
    labels = torch.randint(0, K + 1, (V, H * W), generator=torch.Generator().manual_seed(4)).to(torch.uint8)  # 0 = void
    ds = DeviceRayDataset(torch.from_numpy(images).to(dev), torch.from_numpy(make_cameras(V, seed=2)).to(dev),
                          torch.from_numpy(directions).to(dev), (W, H), batch_size=R, seed=21, optimize_ext=True,
                          semantics=labels.to(dev))
    with torch.no_grad():  # a pose correction that is not the origin
        g = torch.Generator().manual_seed(8)
        ds.dR.copy_((0.02 * torch.randn(V, 3, generator=g)).to(dev))
        ds.dT.copy_((0.02 * torch.randn(V, 3, generator=g)).to(dev))
    torch.manual_seed(0)
    m = NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=K, pred_norm=True).to(dev)
    m.amp_state[0] = 1.0  # (upstream gradients of order 1e-3: no need for the GradScaler's 2^16)
    m.density_bitfield.fill_(255)
    noise = torch.rand(R, generator=torch.Generator().manual_seed(3)).to(dev)
    kw = dict(near_distance=0.01, max_samples=256, test_time=False, random_bg=False, anneal_strategy="none",
              anneal_steps=0, march_noise=noise, global_step=3000, n_sem_cls=K)
    return ds, m, kw


def _pose_grads(ds, m, kw, sem_w):
    hp = dict(HYPERSIM_HPARAMS, loss_sem_w=sem_w, pred_sem=True, load_sem_gt=True)
    loss = NeRFMTLoss(hp)
    ds.dR.grad = ds.dT.grad = None
    m.flat_grad().zero_()
    b = ds.batch(3000)
    assert b["rays_d"].requires_grad and b["semantics"].dtype == torch.int64 and int(b["semantics"].max()) > 0
    res = render(m, b["rays_o"], b["rays_d"], **kw)
    assert res["sem"].shape == (R, K) and res["sem"].requires_grad
    loss_d = loss(res, b, global_step=3000)
    assert loss.last_cluster is not None and "norm_D_C_ort_dot" in loss_d  # the clustering terms are on
    assert ("sem" in loss_d) == (sem_w > 0)
    loss_d["total"].backward()
    torch.cuda.synchronize()
    return ds.dR.grad.clone(), ds.dT.grad.clone()


def test_semantic_term_reaches_the_pose(dev, e2e):
    ds, m, kw = e2e
    gR, gT = _pose_grads(ds, m, kw, 0.1)
    for g in (gR, gT):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    zR, zT = _pose_grads(ds, m, kw, 0.0)
    print(f"heads e2e: |dR.grad| = {float(gR.norm()):.3e} (sem_w 0: {float(zR.norm()):.3e}), "
          f"|dT.grad| = {float(gT.norm()):.3e} (sem_w 0: {float(zT.norm()):.3e})")
    assert bool(torch.isfinite(zR).all()) and bool(torch.isfinite(zT).all())
    assert not torch.equal(gR, zR) and not torch.equal(gT, zT)
    # the difference is the semantic term's, not the order of the loss backward's float atomics: a
    # second run without the term gives that floor, and the term moves the gradients by over 10 x it
    yR, yT = _pose_grads(ds, m, kw, 0.0)
    print(f"heads e2e: moved by the semantic term {float((gR - zR).norm()):.3e} / {float((gT - zT).norm()):.3e}, "
          f"run to run {float((yR - zR).norm()):.3e} / {float((yT - zT).norm()):.3e}")
    assert float((gR - zR).norm()) > 10 * float((yR - zR).norm())
    assert float((gT - zT).norm()) > 10 * float((yT - zT).norm())


def test_static_shapes_still_refuse_ray_gradients_with_heads(dev, e2e):
    ds, m, kw = e2e
    b = ds.batch(3000)
    with pytest.raises(RuntimeError, match="require grad"):
        render(m, b["rays_o"], b["rays_d"], static_shapes=True, **kw)
