"""NGPMT field of the reference models/ngp_mt.py:10-368 on the fused gfx950 kernels.

Surface kept: `NGPMT(scale, grid_size, rgb_act='Sigmoid', pred_sem=False, pred_norm=False, **kw)`,
attributes read by render() (center, half_size, density_bitfield, cascades, scale, grid_size,
pred_norm, pred_sem), `forward(x, d) -> {'sigmas', 'rgbs'}`, `density(x, return_feat)`, and the
occupancy-grid maintenance (get_all_cells, sample_uniform_and_occupied_cells,
update_density_grid, mark_invisible_cells).  Parameter names keep tcnn's `<module>.params`
(xyz_encoder.params / sigma_net.params / rgb_net.params) so the reference's optimizer grouping
('xyz_encoder' in name -> no weight decay, train_nerf.py:262-274) applies unchanged.

Memory layout (MI355X): all parameters live in ONE flat fp32 buffer
  [hash table (n_entries x 2) | W1 (64,32) | W2 (16,64) | W3 (64,32) | W4 (64,64) | W5 (16,64)]
(tcnn's padded rgb_net: 19 inputs cat[d/|d|, h] + 13 constant-1 inputs, 3 outputs + 13 unused rows)
and their gradients in a second flat buffer of the same layout, so the gradient all-reduce is a
single RCCL call and the optimizer a single pass.  The backward accumulates straight into
`param.grad` (views of the flat gradient buffer): hash-table gradients by f32 atomics, weight
gradients through a fixed-order slab reduction.

Input gradients: `forward(x, d)` and `density(x)` are also differentiable w.r.t. x and d (tcnn's
dL/dinput): the reference's --optimize_ext run (train_nerf.py:177-180, 244-249) makes the rays
require grad, and RayMarcher.backward folds dL/dxyzs and dL/ddirs into them; d sigma / d x is the
analytic normal.  dL/dd leaves the MLP backward, dL/dx is one more hash-grid gather
(ncn_field_bwd_mlp_din / ncn_field_bwd_dx, no atomics: bit-identical run to run).  Under the
internal fp16 GradScaler an overflowed backward leaves non-finite input gradients (the step the
optimizer skips): the caller skips its pose update too.

Heads (ngp_mt.py:116-140, 222-227): `NGPMT(..., pred_sem=True, n_sem_cls=K, pred_norm=True)` adds
sem_net / norm_net, tcnn FullyFusedMLP(16 -> 64 -> 64 -> K / 3) on the 16 sigma_net features h
(include/ncnerf_heads.h, csrc/heads.hip).  Their parameters `sem_net.params` / `norm_net.params` are
appended to the flat buffers behind W5 (every existing offset stays), `forward` also returns 'sems'
(N, K) / 'norms' (N, 3), and the backward runs the split MLP pass with each head's backward between
its two parts: the head adds its dL/dh into the stash the sigma part consumes.  With both heads off
every path is what it was.  Input gradients with a head (the reference lists --pred_sem beside
--optimize_ext): dL/dd leaves the rgb part (ncn_field_bwd_mlp_rgb_din; the heads read h, never d),
dL/dx is ncn_field_bwd_dx over the sigma part's encoding gradient, which carries the heads' dL/dh.
Not with a head: sort_samples.

Not provided (off in every reference config, hyperparameters.py:26-30): rgb_act='None' exposure
tonemappers.
"""
import math

import numpy as np
import torch
from einops import rearrange
from torch import nn

from . import _lib, vren
from ._lib import CONSTANTS as _C, call  # (the header's #define NCN_* values)

L_LEVELS, F_PER_LEVEL, LOG2_T, N_MIN = 16, 2, 19, 16  # ngp_mt.py:40
# tcnn's padded shapes (ngp_mt.py:83-113 through tcnn.Network): sigma_net W1 (64,32) W2 (16,64);
# rgb_net's 19 inputs padded to 32 with 1.0, 3 outputs padded to 16: W3 (64,32) W4 (64,64) W5 (16,64)
MLP_SHAPES = ((64, 32), (16, 64), (64, 32), (64, 64), (16, 64))
N_W = sum(o * i for o, i in MLP_SHAPES)  # NCN_FIELD_NW (10240: sigma_net 3072 + rgb_net 7168)
PRECISIONS = {"fp16": _C["NCN_PREC_F16"], "bf16": _C["NCN_PREC_BF16"]}
N_PACKED_HALVES = _C["NCN_FIELD_PACKED_HALVES"]
ENC_BYTES = _C["NCN_ENC_BYTES_PER_SAMPLE"]
SORT_MIN_SAMPLES = 8192  # training batches at least this large are evaluated in Morton-window order
W_SIGMA = 64 * 32 + 16 * 64
W_RGB = N_W - W_SIGMA
HEAD_MAX_OUT = _C["NCN_HEAD_MAX_OUT"]  # three 16-row output tiles
N_HEAD_PACKED_HALVES = _C["NCN_HEAD_PACKED_HALVES"]


def head_shapes(n_out):
    """tcnn's padded shapes of a head FullyFusedMLP(16 -> 64 -> 64 -> n_out): the output rows padded
    to a multiple of 16 (NCN_HEAD_NW(n_out) = 1024 + 4096 + 64 * 16 * ceil(n_out / 16) weights)."""
    if not isinstance(n_out, int) or isinstance(n_out, bool) or not 1 <= n_out <= HEAD_MAX_OUT:
        raise ValueError(f"a head has 1..{HEAD_MAX_OUT} outputs (got {n_out!r})")
    return ((64, 16), (64, 64), (16 * ((n_out + 15) // 16), 64))


def head_nw(n_out):
    return sum(o * i for o, i in head_shapes(n_out))


def grid_levels(scale, n_levels=L_LEVELS, log2_T=LOG2_T, n_min=N_MIN):
    """Per-level tcnn geometry: b = exp(ln(2048*scale/N_min)/(L-1)) (ngp_mt.py:41);
    grid_scale = exp2(l*log2(b))*N_min - 1 (fp32), resolution = ceil(scale)+1,
    params = min(next_multiple(res^3, 8), 2^log2_T).  Returns (levels, n_entries)."""
    b = math.exp(math.log(2048 * scale / n_min) / (n_levels - 1))
    log2_pls = np.float32(np.log2(np.float32(b)))
    levels, offset = [], 0
    for l in range(n_levels):
        s = np.float32(np.float32(np.exp2(np.float32(l) * log2_pls)) * np.float32(n_min) - np.float32(1.0))
        res = int(math.ceil(float(s))) + 1
        params = min(((res ** 3 + 7) // 8) * 8, 1 << log2_T)
        levels.append(dict(scale=float(s), res=res, params=params, offset=offset))
        offset += params
    return levels, offset


def level_words(levels):
    """16 x {scale f32 bits, res, params, offset} as a host uint32 array (the C ABI `levels`)."""
    w = np.zeros(64, np.uint32)
    for l, lv in enumerate(levels):
        w[4 * l] = np.frombuffer(np.float32(lv["scale"]).tobytes(), np.uint32)[0]
        w[4 * l + 1], w[4 * l + 2], w[4 * l + 3] = lv["res"], lv["params"], lv["offset"]
    return w


class _ParamHolder(nn.Module):
    """Stands in for a tcnn module: exposes `.params` (a view of the model's flat buffer)."""

    def __init__(self, flat_view):
        super().__init__()
        self.params = nn.Parameter(flat_view)


class _FieldFunction(torch.autograd.Function):
    """Fused hash-grid + sigma_net + TruncExp + rgb_net (ncn_field_fwd / ncn_field_bwd).

    Differentiable w.r.t. the three parameters (accumulated into the flat gradient buffer) and
    w.r.t. the inputs x and d (camera pose refinement, density normals): dL/dd leaves the MLP pass
    (ncn_field_bwd_mlp_din), dL/dx is a second hash-grid gather over the encoding gradient the MLP
    pass left in its workspace (ncn_field_bwd_dx).  With every parameter frozen only the MLP pass
    and the input kernels run: no table scatter, no weight-gradient reduction, flat_grad untouched.
    (A model with heads takes _FieldHeadsFunction, which gives the same input gradients out of the
    split backward.)"""

    @staticmethod
    def forward(ctx, x, d, table, w_sigma, w_rgb, model, mode, n_dev=None):
        need_grad = any(ctx.needs_input_grad[:5])  # grad mode is off inside Function.forward
        sigmas, rgbs, enc, packed, order = model._field_fwd(x, d, n_dev, mode, need_grad)
        if need_grad:
            need_in = ctx.needs_input_grad[0] or (d is not None and ctx.needs_input_grad[1])
            ctx.save_for_backward(x, d, enc, packed, n_dev, order, table if need_in else None)
            ctx.model = model
        if mode != 0:
            ctx.mark_non_differentiable(rgbs)
        ctx.set_materialize_grads(False)
        return sigmas, rgbs

    @staticmethod
    def backward(ctx, dL_dsigmas, dL_drgbs):
        x, d, enc, packed, n_dev, order, table = ctx.saved_tensors
        model = ctx.model
        n = x.shape[0]
        dev = x.device
        need_x = ctx.needs_input_grad[0]
        need_d = d is not None and ctx.needs_input_grad[1]
        need_param = any(ctx.needs_input_grad[2:5])
        L = _lib.lib()
        dE_ws = torch.empty(int(L.ncn_field_bwd_dE_floats(n)), dtype=torch.float32, device=dev)
        c = lambda t: None if t is None else t.contiguous().float()
        dsig, drgb = c(dL_dsigmas), c(dL_drgbs)
        scale = model._bwd_loss_scale()
        g_table, g_w = model._grad_views() if need_param else (None, None)
        dL_dx = dL_dd = None
        if d is None:
            # density mode (no directions): the sigma part alone on a zero stash, dL/dh = TruncExp'(h0) dL/dsigma
            nb = int(L.ncn_field_bwd_part_blocks(n, 2))
            slab = torch.empty(nb * N_W, dtype=torch.float32, device=dev)
            stash = torch.zeros(int(L.ncn_field_bwd_stash_floats(n)), dtype=torch.float32, device=dev)
            lmax = model._level_max()
            lmax.zero_()  # (the sigma part max-reduces into the rows the rgb part would have zeroed)
            dE_ws[:4].zero_()  # (header: no permuted positions in this workspace)
            call("ncn_field_bwd_mlp_part", x, None, n, n_dev, order, packed, model._prec, enc, dsig, None, None, scale,
                 2, 0, slab, dE_ws, lmax, stash)
            if need_param:
                model._scatter(x, n, n_dev, order, dE_ws, lmax, g_table)
                call("ncn_field_reduce_wgrad_parts", slab, nb, 0, g_w)
        else:
            nb = L.ncn_field_bwd_blocks(n)
            slab = torch.empty(nb * N_W, dtype=torch.float32, device=dev)
            lmax = model._level_max()
            if need_param and not (need_x or need_d) and model.scatter_split is None:
                call("ncn_field_bwd", x, d, n, n_dev, order, model._levels_ptr, model._xyz_min, model._xyz_extent,
                     packed, model._prec, enc, dsig, drgb, scale, g_table, slab, dE_ws, lmax)
            else:
                if need_d:
                    dL_dd = torch.empty(n, 3, dtype=torch.float32, device=dev)  # (the kernel zeroes rows >= *n_dev)
                    call("ncn_field_bwd_mlp_din", x, d, n, n_dev, order, packed, model._prec, enc, dsig, drgb, scale,
                         slab, dE_ws, lmax, model._flat[model._n_table:], dL_dd)
                else:
                    call("ncn_field_bwd_mlp", x, d, n, n_dev, order, packed, model._prec,
                         enc, dsig, drgb, scale, slab, dE_ws, lmax)
                if need_param:
                    model._scatter(x, n, n_dev, order, dE_ws, lmax, g_table)
            if need_param:
                call("ncn_field_reduce_wgrad", slab, nb, g_w)
        if need_x:
            dL_dx = torch.empty(n, 3, dtype=torch.float32, device=dev)  # (the kernel zeroes rows >= *n_dev)
            call("ncn_field_bwd_dx", x, n, n_dev, order, table, model._levels_ptr,
                 model._xyz_min, model._xyz_extent, dE_ws, dL_dx)
        return dL_dx, dL_dd, None, None, None, None, None, None


class _FieldHeadsFunction(torch.autograd.Function):
    """_FieldFunction of a model with heads: ncn_field_fwd, then ncn_head_fwd per head on the encoding
    cache -> (sigmas, rgbs, one (N, n_out) output per head in the model's head order).  Backward:
    ncn_field_bwd_mlp_part part 1 (rgb_net, its dL/dh into the stash), ncn_head_bwd per head (weight
    gradients; its dL/dh added into the stash), part 2 (TruncExp, sigma_net, the encoding gradient),
    the table scatter and the weight-gradient reductions.

    Differentiable w.r.t. x and d as _FieldFunction is (camera pose refinement with the semantic /
    normal terms on): dL/dd leaves part 1 (ncn_field_bwd_mlp_rgb_din: the heads read h, never d),
    dL/dx is ncn_field_bwd_dx over the encoding gradient part 2 left, which carries rgb_net's, every
    head's and TruncExp's dL/dh through sigma_net.  With every parameter frozen only the MLP parts,
    the head backwards and the input kernels run: no table scatter, no weight-gradient reduction
    (the heads' included), flat_grad untouched."""

    @staticmethod
    def forward(ctx, x, d, n_dev, model, *params):
        need_in = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_grad = need_in or any(ctx.needs_input_grad[4:])
        # (the encoding cache is the heads' input: needed as scratch at inference too)
        sigmas, rgbs, enc, packed, _ = model._field_fwd(x, d, n_dev, 0, True)
        n = x.shape[0]
        outs = []
        for name, n_out, _, _ in model._heads:
            o = torch.empty(n, n_out, dtype=torch.float32, device=x.device)
            if n > 0:
                call("ncn_head_fwd", enc, n, n_dev, packed, model._head_packed[name], n_out, model._prec, o)
            outs.append(o)
        if need_grad:
            ctx.save_for_backward(x, d, enc, packed, n_dev, model.xyz_encoder.params if need_in else None,
                                  *[model._head_packed[h[0]] for h in model._heads])
            ctx.model = model
        ctx.set_materialize_grads(False)
        return (sigmas, rgbs) + tuple(outs)

    @staticmethod
    def backward(ctx, dL_dsigmas, dL_drgbs, *dL_dheads):
        x, d, enc, packed, n_dev, table, *head_packed = ctx.saved_tensors
        model = ctx.model
        n, dev = x.shape[0], x.device
        need_x, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_param = any(ctx.needs_input_grad[4:])
        none = (None,) * (2 + 3 + len(model._heads))
        if n == 0:
            return (torch.zeros_like(x) if need_x else None, torch.zeros_like(d) if need_d else None) + none
        L = _lib.lib()
        c = lambda t: None if t is None else t.contiguous().float()
        scale = model._bwd_loss_scale()
        g_table, g_w = model._grad_views() if need_param else (None, None)
        nb = (int(L.ncn_field_bwd_part_blocks(n, 1)), int(L.ncn_field_bwd_part_blocks(n, 2)))
        slab = torch.empty(max(nb) * N_W, dtype=torch.float32, device=dev)
        dE_ws = torch.empty(int(L.ncn_field_bwd_dE_floats(n)), dtype=torch.float32, device=dev)
        stash = torch.empty(int(L.ncn_field_bwd_stash_floats(n)), dtype=torch.float32, device=dev)
        lmax = model._level_max()
        dL_dx = dL_dd = None
        if need_d:
            dL_dd = torch.empty(n, 3, dtype=torch.float32, device=dev)  # (the kernel zeroes rows >= *n_dev)
            call("ncn_field_bwd_mlp_rgb_din", x, d, n, n_dev, None, packed, model._prec, enc, c(dL_drgbs), scale, nb[0],
                 slab, dE_ws, lmax, stash, model._flat[model._n_table:], dL_dd)
        else:
            call("ncn_field_bwd_mlp_part", x, d, n, n_dev, None, packed, model._prec, enc, None, None, c(dL_drgbs),
                 scale, 1, nb[0], slab, dE_ws, lmax, stash)
        nbh = int(L.ncn_head_bwd_blocks(n))
        for (name, n_out, off, n_w), hp, g in zip(model._heads, head_packed, dL_dheads):
            if g is None:
                continue
            hslab = torch.empty(nbh * n_w, dtype=torch.float32, device=dev)
            call("ncn_head_bwd", enc, n, n_dev, packed, hp, n_out, model._prec, c(g), scale, hslab, stash)
            if need_param:
                call("ncn_head_reduce_wgrad", hslab, nbh, n_w, model._flat_grad[off:off + n_w])
        call("ncn_field_bwd_mlp_part", x, d, n, n_dev, None, packed, model._prec, enc, c(dL_dsigmas), None, None, scale,
             2, nb[1], slab, dE_ws, lmax, stash)
        if need_param:
            model._scatter(x, n, n_dev, None, dE_ws, lmax, g_table, wgrad=(slab, nb[1], nb[0], g_w))
        if need_x:
            dL_dx = torch.empty(n, 3, dtype=torch.float32, device=dev)  # (the kernel zeroes rows >= *n_dev)
            call("ncn_field_bwd_dx", x, n, n_dev, None, table, model._levels_ptr, model._xyz_min, model._xyz_extent,
                 dE_ws, dL_dx)
        return (dL_dx, dL_dd) + none


class NGPMT(nn.Module):
    def _bwd_loss_scale(self):
        """The field backward's loss_scale operand (ncn_field_bwd): the internal GradScaler's scale,
        a device 1.0 under external AMP, None for bf16."""
        return self.amp_state if self.amp_state is not None else self._amp_unit

    def _level_max(self):
        """ncn_field_bwd's per-level max |dE| workspace: 16 floats per MLP-pass workgroup (<= 256).
        The scatter reads it as each level's fixed-point scale, so with scatter_split set (a backward
        whose coarse levels are scattered later, run_deferred_scatter) every backward gets its own:
        a shared buffer would hand the earlier pending scatters the LAST backward's maxima
        (overflowing 64-bit sums, or a level dropped when its maximum there is 0)."""
        dev = self._flat.device
        if self.scatter_split is not None:
            return torch.empty(16 * 256, dtype=torch.float32, device=dev)
        if getattr(self, "_lmax", None) is None or self._lmax.device != dev:
            self._lmax = torch.empty(16 * 256, dtype=torch.float32, device=dev)
        return self._lmax

    def __init__(self, scale, grid_size, rgb_act="Sigmoid", pred_sem=False, pred_norm=False, seed=1337,
                 precision="fp16", amp="internal", **kwargs):
        """precision: MFMA operand type of the MLPs, "fp16" (tcnn's FullyFusedMLP, the reference's AMP
        run) or "bf16" (config #3); parameters, table and accumulation stay fp32.
        amp (fp16 only): "internal" — the model keeps its own GradScaler state (`amp_state`, updated by
        FlatAdam / ncn_adam_step) and the field backward applies it at the MLP's boundary, so the
        caller's loss is unscaled (the Trainer path); "external" — the caller runs AMP itself
        (train_nerf.py's PL precision=16 + GradScaler, or torch.cuda.amp.GradScaler): the upstream
        gradient arrives already scaled, the backward applies only tcnn's own fp16 module scale
        (x128 in, /128 out, NCN_TCNN_LOSS_SCALE) and the gradients leave in the caller's scale, as
        tcnn's do; any optimizer (torch.optim.Adam(W), apex FusedAdam) then steps them."""
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        if amp not in ("internal", "external"):
            raise ValueError("amp must be 'internal' or 'external'")
        self.amp = amp
        self.precision = precision
        self._prec = PRECISIONS[precision]
        if rgb_act != "Sigmoid":
            raise NotImplementedError("rgb_act='None' (exposure tonemappers) is off in every reference config")
        pred_sem, pred_norm = bool(pred_sem), bool(pred_norm)
        heads = []  # (module name, outputs) in the reference's module order (ngp_mt.py:116-140)
        if pred_sem:
            if kwargs.get("n_sem_cls") is None:
                raise NotImplementedError("pred_sem=True needs the class count: pass n_sem_cls (the reference reads "
                                          "kwargs['n_sem_cls'], ngp_mt.py:119)")
            head_shapes(kwargs["n_sem_cls"])  # (ValueError outside 1..48)
            heads.append(("sem_net", kwargs["n_sem_cls"]))
            self.n_sem_cls = kwargs["n_sem_cls"]
        if pred_norm:
            heads.append(("norm_net", 3))
        self.pred_sem, self.pred_norm, self.rgb_act = pred_sem, pred_norm, rgb_act
        self.scale = scale
        self.register_buffer("center", torch.zeros(1, 3))
        self.register_buffer("xyz_min", -torch.ones(1, 3) * scale)
        self.register_buffer("xyz_max", torch.ones(1, 3) * scale)
        self.register_buffer("half_size", (self.xyz_max - self.xyz_min) / 2)
        # the scene box as host floats for the one-launch marcher (no device read per step)
        self._aabb = (tuple(float(v) for v in self.center[0]), tuple(float(v) for v in self.half_size[0]))
        self.cascades = max(1 + int(np.ceil(np.log2(2 * scale))), 1)  # ngp_mt.py:34
        self.grid_size = grid_size
        self.register_buffer("density_bitfield", torch.zeros(self.cascades * grid_size ** 3 // 8, dtype=torch.uint8))
        self.levels, self.n_entries = grid_levels(scale)
        self._level_words = level_words(self.levels)
        self._levels_ptr = self._level_words.ctypes.data_as(_lib.P)
        self._xyz_min = float(np.float32(-scale))
        self._xyz_extent = float(np.float32(scale) - np.float32(-scale))
        n_table = self.n_entries * F_PER_LEVEL
        self._n_table = n_table
        # heads behind W5: (module name, outputs, offset in the flat buffer, weights)
        self._heads, off = [], n_table + N_W
        for name, n_out in heads:
            self._heads.append((name, n_out, off, head_nw(n_out)))
            off += head_nw(n_out)
        flat = torch.zeros(off)
        g = torch.Generator().manual_seed(seed)
        flat[:n_table] = (torch.rand(n_table, generator=g) * 2 - 1) * 1e-4  # tcnn grid init U(-1e-4, 1e-4)
        off = n_table
        for o, i in MLP_SHAPES:  # Xavier-uniform MLP weights (tcnn initialises the padded matrices)
            a = math.sqrt(6.0 / (o + i))
            flat[off:off + o * i] = (torch.rand(o * i, generator=g) * 2 - 1) * a
            off += o * i
        for _, n_out, _, _ in self._heads:  # (drawn after W1..W5: the field's initialisation is the heads-off one)
            for o, i in head_shapes(n_out):
                a = math.sqrt(6.0 / (o + i))
                flat[off:off + o * i] = (torch.rand(o * i, generator=g) * 2 - 1) * a
                off += o * i
        self._flat = flat
        self.xyz_encoder = _ParamHolder(flat[:n_table])
        self.sigma_net = _ParamHolder(flat[n_table:n_table + W_SIGMA])
        self.rgb_net = _ParamHolder(flat[n_table + W_SIGMA:n_table + N_W])
        for name, _, off, n_w in self._heads:
            setattr(self, name, _ParamHolder(flat[off:off + n_w]))
        self._flat_grad = None
        self._packed = None
        self._head_packed = {}
        # AMP GradScaler state {scale, growth tracker} of the fp16 MLP (the reference trains with
        # precision=16, train_nerf.py:954: the scaled loss keeps tcnn's fp16 backward from
        # underflowing): the field backward multiplies its upstream gradients by the scale and
        # divides its outputs by it; ncn_adam_step skips non-finite steps and grows / backs off the
        # scale.  bf16 operands (fp32's exponent range) run unscaled, as PL's bf16 mode does.
        f16 = precision == "fp16"
        self.register_buffer("amp_state", torch.tensor([_lib.AMP_INIT_SCALE, 0.0]) if f16 and amp == "internal" else None)
        # external AMP: the backward's loss-scale operand is a constant 1 (only tcnn's x128 remains)
        self.register_buffer("_amp_unit", torch.ones(1) if f16 and amp == "external" else None, persistent=False)
        # None: the backward scatters every level.  An int L (data-parallel step): levels [L, 16)
        # are scattered in the backward, [0, L) by run_deferred_scatter() (grad_buckets(L)).
        self.scatter_split = None
        # Morton-window processing order (ncn_field_sort_windows) for training batches: off by default
        # (measured: forward 88 -> 72 us, but sort 40 us + MLP backward +6 us + scatter +9 us)
        self.sort_samples = False
        self._deferred = []  # pending coarse-level scatters of the split data-parallel step (eager backwards)
        self._deferred_graph = []  # the captured step's coarse-level scatters (Trainer._capture), every replay

    # -- flat buffers --------------------------------------------------------------------------
    def _param_slices(self):
        """(parameter, start, end) of every parameter in the flat buffers, in their order."""
        n_table = self._n_table
        return ([(self.xyz_encoder.params, 0, n_table), (self.sigma_net.params, n_table, n_table + W_SIGMA),
                 (self.rgb_net.params, n_table + W_SIGMA, n_table + N_W)]
                + [(getattr(self, name).params, off, off + n_w) for name, _, off, n_w in self._heads])

    def _apply(self, fn, recurse=True):
        # keep the parameters as views of one flat buffer across .to()/.cuda()
        super()._apply(fn, recurse)
        flat = fn(self._flat)
        for p, a, b in self._param_slices():
            flat[a:b].copy_(p.data)
        self._flat = flat
        for p, a, b in self._param_slices():
            p.data = flat[a:b]
        self._flat_grad = None
        self._packed = None
        self._head_packed = {}
        return self

    def flat_params(self):
        return self._flat

    def flat_grad(self):
        """The flat gradient buffer; every parameter's .grad is a view of it."""
        self._grad_views()
        return self._flat_grad

    def _grad_views(self):
        if self._flat_grad is None or self._flat_grad.device != self._flat.device:
            self._flat_grad = torch.zeros_like(self._flat)
        fg, n_table = self._flat_grad, self._n_table
        for p, a, b in self._param_slices():
            v = fg[a:b]
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                if p.grad is not None:
                    v.copy_(p.grad)
                else:
                    v.zero_()
                p.grad = v
        return fg[:n_table], fg[n_table:n_table + N_W]

    def grad_buckets(self, split):
        """The flat gradient as (levels [split, 16) of the table + the MLP weights, levels [0, split)):
        two contiguous views, the all-reduce buckets of the split data-parallel step."""
        fg = self.flat_grad()
        cut = 2 * self.levels[split]["offset"]
        return fg[cut:], fg[:cut]

    def run_deferred_scatter(self, max_blocks=0, graph=False):
        """Scatter of the levels [0, scatter_split) left by the field backwards: graph=False — the
        eager backwards since the last call (then cleared); graph=True — the captured step's entries
        (Trainer._capture moves them to _deferred_graph: they name the graph's static buffers, refilled
        by every replay, and are run after each replay)."""
        entries = self._deferred_graph if graph else self._deferred
        if not entries:
            raise RuntimeError("run_deferred_scatter: no deferred scatter (scatter_split unset or no backward yet)")
        for x, n, n_dev, order, dE_ws, lmax, g_table in entries:
            call("ncn_field_scatter", x, n, n_dev, order, self._levels_ptr, self._xyz_min, self._xyz_extent, dE_ws,
                 lmax, 0, self.scatter_split, max_blocks, g_table)
        if not graph:
            self._deferred = []

    def prepare_weights(self):
        """Pack the MLP weights now (after the optimizer step) so the next forward reuses them.
        The packed fragments are reused by the next forward while `_packed_fresh` is set (FlatAdam's
        packed step sets it: its Adam pass writes the fragments of the weights it updates).  A caller
        that changes the parameters any other way (an in-place edit, a copy from another model, a
        broadcast) must call prepare_weights() afterwards; load_state_dict clears the flag itself."""
        self._pack_weights()
        self._packed_fresh = True

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._packed_fresh = False  # (the loaded weights: the next forward packs them)

    def _take_packed(self):
        if getattr(self, "_packed_fresh", False) and self._packed is not None:
            self._packed_fresh = False
            return self._packed
        return self._pack_weights()

    def pack_target(self):
        """(pack_inv, pack_off, packed, precision) for ncn_adam_step_packed: the optimizer refreshes
        the packed MLP fragments itself (no pack launch between it and the next forward).  pack_inv
        (NCN_FIELD_NW x 2 int32, -1 = none) lists each master weight's packed elements, from
        ncn_field_pack_map; built once.  The packed buffer is allocated (and packed) if needed."""
        if self._heads:
            raise RuntimeError("pack_target: ncn_adam_step_packed refreshes the field's fragments only; a model with "
                               "heads takes ncn_adam_step and packs explicitly (FlatAdam does)")
        if self._packed is None or self._packed.device != self._flat.device:
            self._pack_weights()
        inv = getattr(self, "_pack_inv", None)
        if inv is None or inv.device != self._flat.device:
            src = torch.empty(N_PACKED_HALVES, dtype=torch.int32, device=self._flat.device)
            call("ncn_field_pack_map", src)
            s = src.cpu().numpy()
            table = np.full((N_W, 2), -1, np.int32)
            fill = np.zeros(N_W, np.int64)
            for q, w in enumerate(s):
                assert 0 <= w < N_W and fill[w] < 2, (q, w)
                table[w, fill[w]] = q
                fill[w] += 1
            inv = self._pack_inv = torch.from_numpy(table).to(self._flat.device)
        return inv, self._n_table, self._packed, self._prec

    def _pack_weights(self):
        if self._packed is None or self._packed.device != self._flat.device:
            self._packed = torch.empty(N_PACKED_HALVES, dtype=torch.float16, device=self._flat.device)
        call("ncn_field_pack_weights", self._flat[self._n_table:], self._packed, self._prec)
        for name, n_out, off, n_w in self._heads:
            hp = self._head_packed.get(name)
            if hp is None or hp.device != self._flat.device:
                hp = self._head_packed[name] = torch.empty(N_HEAD_PACKED_HALVES, dtype=torch.float16,
                                                           device=self._flat.device)
            call("ncn_head_pack_weights", self._flat[off:off + n_w], n_out, hp, self._prec)
        return self._packed

    # -- field -----------------------------------------------------------------------------------
    def _field_fwd(self, x, d, n_dev, mode, need_grad):
        """ncn_field_fwd on x (N,3) / d (N,3) fp32 contiguous (capacity N when n_dev, a device int32
        count, is given) -> (sigmas, rgbs, enc_cache, packed weights, order); enc_cache and order
        (None unless sort_samples) are the backward's inputs, None without need_grad."""
        n = x.shape[0]
        dev = x.device
        sigmas = torch.empty(n, dtype=torch.float32, device=dev)
        rgbs = torch.empty(n, 3, dtype=torch.float32, device=dev) if mode == 0 else sigmas.new_empty(0, 3)
        enc = None
        if need_grad:
            enc = torch.empty(((n + 15) // 16) * 16 * ENC_BYTES // 2, dtype=torch.float16, device=dev)
        packed = self._take_packed()
        order = None
        if self._heads and self.sort_samples:
            raise NotImplementedError("sort_samples (the Morton-window processing order) is not supported with a "
                                      "pred_sem / pred_norm head")
        if need_grad and self.sort_samples and n >= SORT_MIN_SAMPLES:
            # processing order: Morton-sorted windows of 4096 samples (ncn_field_sort_windows); the
            # encoding cache and the backward's dE are kept in it, the outputs stay in sample order
            order = torch.empty(n, dtype=torch.int32, device=dev)
            call("ncn_field_sort_windows", x, n, n_dev, self._xyz_min, self._xyz_extent, order)
        call("ncn_field_fwd", x, d if mode == 0 else None, n, n_dev, order, self.xyz_encoder.params, self._levels_ptr,
             self._xyz_min, self._xyz_extent, packed, self._prec, mode, sigmas, rgbs if mode == 0 else None, enc)
        return sigmas, rgbs, enc, packed, order

    def _scatter(self, x, n, n_dev, order, dE_ws, lmax, g_table, wgrad=None):
        """Table scatter after the MLP pass: every level (scatter_split None), else the levels
        [scatter_split, 16) now and [0, scatter_split) queued for run_deferred_scatter() — the
        data-parallel step scatters them while the all-reduce of the first bucket is in flight.
        wgrad = (slab, sigma-pass rows, rgb-pass rows, grad_w): the split backward's weight-gradient
        reduction, folded into this launch (ncn_field_scatter_wgrad)."""
        split = self.scatter_split
        lo = 0 if split is None else split
        slab, nb_s, nb_r, g_w = wgrad if wgrad is not None else (None, 0, 0, None)
        call("ncn_field_scatter_wgrad", x, n, n_dev, order, self._levels_ptr, self._xyz_min, self._xyz_extent, dE_ws,
             lmax, lo, 16, 0, g_table, slab, nb_s, nb_r, g_w)
        if split is not None:
            # (a list: a step with two field backwards — e.g. density() with grad and forward() —
            # leaves two pending coarse-level scatters, both run by run_deferred_scatter)
            self._deferred.append((x, n, n_dev, order, dE_ws, lmax, g_table))

    def density(self, x, return_feat=False):
        """ngp_mt.py:157-171 (density-only kernel mode).  Differentiable w.r.t. the parameters and
        w.r.t. x (-d sigma / d x is the analytic normal): the sigma part of the MLP backward alone."""
        _lib.check_input(x, "x")
        if return_feat:
            return self._density_feat(x.float().contiguous())
        sigmas, _ = _FieldFunction.apply(x.float().contiguous(), None, self.xyz_encoder.params,
                                         self.sigma_net.params, self.rgb_net.params, self, 1)
        return sigmas

    @torch.no_grad()
    def _density_feat(self, x):
        """density(x, return_feat=True) -> (sigmas (N), h (N, 16) fp32), for inference and inspection
        (no gradient): h, sigma_net's fp32 accumulators, is recomputed from the forward's encoding cache
        with the field's own sigma_net code (ncn_head_feat): the h whose row 0 the kernel exponentiates."""
        n = x.shape[0]
        sigmas, _, enc, packed, _ = self._field_fwd(x, None, None, 1, True)
        h = torch.empty(n, 16, dtype=torch.float32, device=x.device)
        if n > 0:
            call("ncn_head_feat", enc, n, None, packed, self._prec, h)
        return sigmas, h

    def forward(self, x, d, **kwargs):
        """ngp_mt.py:196-229 -> {'sigmas': (N,), 'rgbs': (N,3)} (fp32).

        kwargs['n_samples_dev'] (extension): a device int32 sample count <= len(x); x/d are then
        static-capacity buffers and only the first *n_samples_dev rows are evaluated."""
        x = x.float().contiguous()
        d = d.float().contiguous()
        _lib.check_input(x, "x")
        _lib.check_input(d, "d")
        n_dev = kwargs.get("n_samples_dev")
        if self._heads:
            sigmas, rgbs, *outs = _FieldHeadsFunction.apply(x, d, n_dev, self, *[p for p, _, _ in self._param_slices()])
            output = {"sigmas": sigmas, "rgbs": rgbs}
            for (name, _, _, _), o in zip(self._heads, outs):
                output["sems" if name == "sem_net" else "norms"] = o
            return output
        sigmas, rgbs = _FieldFunction.apply(x, d, self.xyz_encoder.params, self.sigma_net.params,
                                            self.rgb_net.params, self, 0, n_dev)
        return {"sigmas": sigmas, "rgbs": rgbs}

    # -- occupancy grid maintenance (ngp_mt.py:231-368) --------------------------------------------
    @torch.no_grad()
    def get_all_cells(self):
        indices = vren.morton3D(self.grid_coords).long()
        return [(indices, self.grid_coords)] * self.cascades

    @torch.no_grad()
    def sample_uniform_and_occupied_cells(self, M, density_threshold):
        cells = []
        for c in range(self.cascades):
            coords1 = torch.randint(self.grid_size, (M, 3), dtype=torch.int32, device=self.density_grid.device)
            indices1 = vren.morton3D(coords1).long()
            indices2 = torch.nonzero(self.density_grid[c] > density_threshold)[:, 0]
            if len(indices2) > 0:
                rand_idx = torch.randint(len(indices2), (M,), device=self.density_grid.device)
                indices2 = indices2[rand_idx]
            coords2 = vren.morton3D_invert(indices2.int().contiguous())
            cells += [(torch.cat([indices1, indices2]), torch.cat([coords1, coords2]))]
        return cells

    @torch.no_grad()
    def mark_invisible_cells(self, K, dev, poses, img_wh, near_distance, chunk=64 ** 3):
        """ngp_mt.py:274-337 (pinhole K (3,3) tensor branch and the Hypersim NDC tuple branch)."""
        N_cams = poses.shape[0]
        self.count_grid = torch.zeros_like(self.density_grid)
        w2c_R = rearrange(poses[:, :3, :3], "n a b -> n b a")
        w2c_T = -w2c_R @ poses[:, :3, 3:]
        cells = self.get_all_cells()
        if isinstance(K, torch.Tensor):
            K = K.to(dev)
        elif isinstance(K, tuple):
            M_ndc_from_cam, M_uv_from_ndc = K[0].to(dev), K[1].to(dev)
            k_scale = K[3]
        else:
            raise AssertionError
        for c in range(self.cascades):
            indices, coords = cells[c]
            for i in range(0, len(indices), chunk):
                xyzs = coords[i:i + chunk] / (self.grid_size - 1) * 2 - 1
                s = min(2 ** (c - 1), self.scale)
                half_grid_size = s / self.grid_size
                xyzs_w = (xyzs * (s - half_grid_size)).T
                xyzs_c = w2c_R @ xyzs_w + w2c_T
                if isinstance(K, torch.Tensor):
                    uvd = K @ xyzs_c
                    uv = uvd[:, :2] / uvd[:, 2:]
                else:
                    xyzs_c *= 2 * k_scale
                    xyzs_c = torch.cat((xyzs_c, torch.ones_like(xyzs_c)[:, :1, :]), 1)
                    xyz_clip = M_ndc_from_cam @ xyzs_c
                    xyz_ndc = xyz_clip / xyz_clip[:, 3:]
                    uvd = M_uv_from_ndc @ xyz_ndc
                    uv = uvd[:, :2]
                in_image = (uvd[:, 2] >= 0) & (uv[:, 0] >= 0) & (uv[:, 0] < img_wh[0]) & (uv[:, 1] >= 0) & \
                           (uv[:, 1] < img_wh[1])
                covered_by_cam = (uvd[:, 2] >= near_distance) & in_image
                self.count_grid[c, indices[i:i + chunk]] = count = covered_by_cam.sum(0) / N_cams
                too_near_to_cam = (uvd[:, 2] < near_distance) & in_image
                valid_mask = (count > 0) & (~too_near_to_cam.any(0))
                self.density_grid[c, indices[i:i + chunk]] = torch.where(valid_mask, 0., -1.)

    def _grid_side_stream(self):
        if getattr(self, "_grid_side", None) is None:
            self._grid_side = torch.cuda.Stream(device=self.density_grid.device)
        return self._grid_side

    def _grid_ws(self):
        """Device workspace of the grid refresh: hit list (positions, cell indices, densities) of one
        cascade's capacity, the list count, the effective threshold and the reduction scratch."""
        dev, N = self.density_grid.device, self.grid_size ** 3
        ws = getattr(self, "_gws", None)
        if ws is None or ws["xyzs"].device != dev or ws["idx"].numel() != N:
            nbytes = int(_lib.lib().ncn_grid_work_bytes())
            ws = {"xyzs": torch.empty(N, 3, device=dev), "idx": torch.empty(N, dtype=torch.int32, device=dev),
                  "sigmas": torch.empty(N, device=dev), "scal": torch.zeros(4, dtype=torch.int32, device=dev),
                  # the density pass's encodings (ncn_field_fwd mode 2 scratch: 64 B per point)
                  "enc": torch.empty(((N + 15) // 16) * 16 * ENC_BYTES // 2, dtype=torch.float16, device=dev),
                  "work": torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.float32, device=dev)}
            self._gws = ws
        return ws

    @torch.no_grad()
    def update_density_grid(self, density_threshold, warmup=False, decay=0.95, erode=False, seed=None, beside=None):
        """ngp_mt.py:340-368 on the device (csrc/grid.hip): per cascade ncn_grid_sample -> density
        pass (ncn_field_fwd mode 2 over the hit list, device count) -> ncn_grid_apply, then
        ncn_grid_packbits.  Cells hit: all of them in warmup (get_all_cells), else each cell with the
        marginal probability of the reference's M uniform + M occupied draws with replacement
        (sample_uniform_and_occupied_cells, M = G^3/4) — the documented sampling deviation of
        grid.hip.  The density grid is updated in place (the reference rebinds it to the same values).
        Quirk q12: with no cell > 0 the mean is NaN and the bitfield is cleared — reproduced.
        No host synchronisation; `seed` (default: drawn from torch's CPU generator) fixes the draw.
        beside (optional callable): work issued on the current stream while the first cascade's cell
        sampling — which reads the density grid only, not the parameters — runs on a side stream
        (Trainer: the optimizer step the refresh waits for); joined before the density pass."""
        G, C = self.grid_size, self.cascades
        N = G ** 3
        dg = self.density_grid
        if not (dg.is_cuda and dg.is_contiguous() and dg.dtype == torch.float32 and dg.shape == (C, N)):
            raise RuntimeError("density_grid must be a contiguous CUDA float32 (cascades, grid_size**3) tensor")
        cnt = None
        if erode:
            cnt = self.count_grid.float().contiguous()
        ws = self._grid_ws()
        n_list = ws["scal"][0:1]
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        table = self.xyz_encoder.params
        packed = None
        for c in range(C):
            s = min(2 ** (c - 1), self.scale)
            half_grid_size = s / G
            dgc = dg[c]
            cc = cnt[c] if cnt is not None else None

            def sample():
                call("ncn_grid_sample", dgc, N, G, s - half_grid_size, half_grid_size, density_threshold, N // 4,
                     1 if warmup else 0, (seed + 0x9E3779B97F4A7C15 * c) % 2 ** 64, decay, cc, ws["xyzs"], ws["idx"],
                     n_list, ws["work"])

            if c == 0 and beside is not None:
                cur = torch.cuda.current_stream(dg.device)
                side = self._grid_side_stream()
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    sample()
                beside()
                cur.wait_stream(side)
            else:
                sample()
            if packed is None:
                packed = self._take_packed()  # (after `beside`: the optimizer may have refreshed the fragments)
            # density pass, mode 2: the hash-grid encoding split by level over the XCDs into the
            # scratch ws["enc"] (each L2 serves two levels' tables), then sigma_net from it
            call("ncn_field_fwd", ws["xyzs"], None, N, n_list, None, table, self._levels_ptr, self._xyz_min,
                 self._xyz_extent, packed, self._prec, 2, ws["sigmas"], None, ws["enc"])
            call("ncn_grid_apply", dgc, ws["idx"], ws["sigmas"], n_list, N, decay, cc)
        thr_out = ws["scal"][1:2].view(torch.float32)
        call("ncn_grid_packbits", dg, C * N, density_threshold, self.density_bitfield, thr_out, ws["work"])


def register_grid_buffers(model):
    """What train_nerf.py:153-157 does: density_grid (C, G^3) and grid_coords (G^3, 3) buffers."""
    G = model.grid_size
    model.register_buffer("density_grid", torch.zeros(model.cascades, G ** 3, device=model.center.device))
    r = torch.arange(G, dtype=torch.int32, device=model.center.device)
    zz, yy, xx = torch.meshgrid(r, r, r, indexing="ij")  # kornia create_meshgrid3d: index (d,h,w) -> (w,h,d)
    coords = torch.stack([xx, yy, zz], -1).reshape(-1, 3)
    model.register_buffer("grid_coords", coords.contiguous())
    return model
