"""One training step of the reference NeRFSystem (train_nerf.py:165-358) on the HIP hot path:
render (intersect -> march -> field -> composite) -> NeRFMTLoss (rgb + opacity + normal
clustering) -> backward -> [RCCL gradient all-reduce] -> clip + Adam, plus the occupancy-grid
refresh every 16 steps (train_nerf.py:314-320) when `update_grid` is on, and the per-epoch cosine
learning rate (CosineAnnealingLR(T_max=num_epochs), train_nerf.py:286-288; an epoch is the
training set's 1000 items, base.py:78-81, split over the ranks by DDP's DistributedSampler).

Hyper-parameters default to the Hypersim config (experiments/hypersim/hyperparameters.py);
preset="scannet_manhattan" selects config #5's (experiments/scannet_man/hyperparameters.py).

The training loop (the reference's trainer.fit(system)): Trainer.step_from(dataset, global_step) is
the step with its batch drawn from a data.DeviceRayDataset — in the captured step the draw, the
rays and the gathers are nodes of the graph that read the device step counter, so a replay copies
no batch — and Trainer.fit(dataset, n_steps) runs it over a step range, steps the dataset's pose
corrections dR / dT (eager step, optimize_ext), and keeps the per-step log (losses, sample counts)
in a device ring that is read once per drain (TrainLog).

Checkpoints (the reference's ModelCheckpoint / --ckpt_path): Trainer.state_dict / load_state_dict
snapshot and restore everything a step depends on, save_checkpoint / load_checkpoint put a file
around them (checkpoint.py), and fit(checkpoint_every=, checkpoint_path=) saves inside the loop."""
import math
import os
import warnings

import torch

from . import _lib, checkpoint, distributed
from .losses import NeRFMTLoss, check_cluster_status
from .optim import POSE_LR, FlatAdam, PoseAdam, cosine_factor
from .rendering import march_train_fused, render

HYPERSIM_HPARAMS = dict(
    scale=0.5, grid_size=128, rend_max_samples=1024, rend_near_dist=0.01, density_tresh_decay=1.0,
    loss_opacity_w=1e-3, loss_distortion_w=0, loss_depth_w=0, loss_norm_depth_dot_w=0, loss_norm_depth_L1_w=0,
    loss_reg_depth_w=0, loss_sem_w=0, loss_manhattan_nerf_w=0,
    loss_norm_D_C_ort_dot_w=2e-3, loss_norm_D_C_centr_dot_w=2e-3, loss_norm_D_C_centr_L1_w=2e-3,
    loss_norm_D_C_can_dot_w=0, loss_norm_D_C_can_L1_w=0, loss_norm_can_tres=0.01, loss_norm_can_start=500,
    loss_norm_can_end=-1, loss_norm_can_grow=2500, lr=1e-2, num_epochs=30, batch_size=8192,
    ray_sampling_strategy="all_images_triang_patch", grad_clip=0.05, pred_norm_depth=True)

# config #5 (experiments/scannet_man/hyperparameters.py): the Hypersim settings with the three
# normal-clustering weights at 1e-2 (:45-47); scale, grid, samples, lr, batch and clip are equal (:21-24)
SCANNET_HPARAMS = dict(HYPERSIM_HPARAMS, loss_norm_D_C_ort_dot_w=1e-2, loss_norm_D_C_centr_dot_w=1e-2,
                       loss_norm_D_C_centr_L1_w=1e-2)

PRESETS = {"hypersim": HYPERSIM_HPARAMS, "scannet_manhattan": SCANNET_HPARAMS}


def hparams_for(preset):
    """The hyper-parameter dict of a dataset preset (train_nerf.py --dataset_name)."""
    if preset not in PRESETS:
        raise ValueError(f"unknown preset {preset!r}; one of {sorted(PRESETS)}")
    return dict(PRESETS[preset])


_HOST_BATCH = "batch"  # Trainer._source of a graph captured from step()'s host-built dict


def rank_seed(dataset):
    """The seed this rank draws its batches with: the dataset's plus the rank (every rank of a
    data-parallel run draws its own 8192 rays, base.py:94-171 under DDP's per-rank workers)."""
    return dataset.seed + distributed.rank()


def pose_lr(epoch, num_epochs):
    """The learning rate of the pose group [dR, dT] in `epoch`: the hard-coded 1e-6 (train_nerf.py:
    275-277) under the scheduler's per-epoch cosine factor (:286-288), which holds every group."""
    return POSE_LR * (cosine_factor(epoch, num_epochs) if num_epochs else 1.0)


class TrainLog:
    """The per-step log of Trainer.fit, decoded on the host.  Rows come from the device ring
    (`add_ring`): float32 columns `step`, `total`, the loss terms in the order of the step's loss
    dict, `rm_samples`, `vr_samples` (exact in float32 below 2^24).  log[name] is the column as a
    float32 tensor in step order (NaN where a step had no such term); derived columns, as the
    reference logs them: `psnr` = -10 log10(rgb) (train/psnr: PSNR at data range 1 of the step's
    batch, train_nerf.py:348,353), `rm_s` / `vr_s` = marched / composited samples per ray
    (train_nerf.py:350-352).  log.steps: the step column as int64."""

    HEAD, TAIL = ("step", "total"), ("rm_samples", "vr_samples")

    def __init__(self, n_rays):
        self.n_rays = int(n_rays)
        self._segments = []  # (column names, (n, n_cols) float32 CPU rows)

    @classmethod
    def column_names(cls, loss_d):
        """The ring's columns for a step whose loss dict is `loss_d` (`total` moved to the front)."""
        return cls.HEAD + tuple(k for k in loss_d if k != "total") + cls.TAIL

    @staticmethod
    def ring_rows(first_step, count, capacity):
        """Ring rows of the steps [first_step, first_step + count), in step order: step s is at s % capacity."""
        if count > capacity:
            raise ValueError(f"{count} steps do not fit a ring of {capacity} rows: drained too late")
        return [(first_step + i) % capacity for i in range(count)]

    def add_ring(self, ring, columns, first_step, count):
        """Append the rows of `count` steps from `first_step` on out of a host copy of the ring."""
        ring = torch.as_tensor(ring, dtype=torch.float32, device="cpu")
        if ring.dim() != 2 or ring.shape[1] != len(columns):
            raise ValueError(f"ring {tuple(ring.shape)} does not hold the {len(columns)} columns {tuple(columns)}")
        if count > 0:
            self._segments.append((tuple(columns), ring[self.ring_rows(first_step, count, ring.shape[0])].clone()))

    def __len__(self):
        return sum(rows.shape[0] for _, rows in self._segments)

    @property
    def columns(self):
        """Every stored column name, in first-seen order."""
        names = []
        for cols, _ in self._segments:
            names += [c for c in cols if c not in names]
        return tuple(names)

    def __getitem__(self, name):
        if name == "psnr":
            return -10.0 * torch.log10(self["rgb"])
        if name in ("rm_s", "vr_s"):
            return self[name[:2] + "_samples"] / float(self.n_rays)
        if name not in self.columns:
            raise KeyError(name)
        parts = [rows[:, cols.index(name)] if name in cols else torch.full((rows.shape[0],), float("nan"))
                 for cols, rows in self._segments]
        return torch.cat(parts) if parts else torch.empty(0)

    @property
    def steps(self):
        return self["step"].to(torch.int64) if self._segments else torch.empty(0, dtype=torch.int64)


class Trainer:
    warmup_steps = 256
    update_interval = 16

    epoch_items = 1000  # base.py:78-81 (training "epoch" = 1000 batches)

    def __init__(self, model, hparams=None, update_grid=False, use_graph=False, scatter_split=None,
                 defer_optimizer=False, preset="hypersim", split_backward=True):
        """hparams: overrides of the preset's hyper-parameters (PRESETS: "hypersim" = configs #1-#4,
        "scannet_manhattan" = config #5).  split_backward (graph step; taken when the loss is the
        reference configuration, split_step.split_eligible): the step runs as split_step.SplitStep —
        the photometric backward overlaps the normal clustering, every per-sample value as the
        autograd backward computes it — instead of render -> loss -> autograd backward.  True or
        "fused": the clustering and the rgb pass in one launch; "forked": on two streams
        (SplitStep's `fused`)."""
        self.h = dict(hparams_for(preset), **(hparams or {}))
        self.model = model
        self.loss = NeRFMTLoss(self.h)
        # the Adam pass zeroes the gradient it consumed: no zero_grad fill in the step
        self.opt = FlatAdam(model, lr=self.h["lr"], max_norm=self.h["grad_clip"], num_epochs=self.h["num_epochs"],
                            zero_grad_on_step=True)
        self.world = distributed.world_size()
        self.steps_per_epoch = math.ceil(self.epoch_items / self.world)  # DistributedSampler split
        # data-parallel step: all-reduce the gradient in two buckets, the table levels
        # [scatter_split, 16) + MLP weights while the levels [0, scatter_split) are scattered
        if self.world > 1:
            model.scatter_split = distributed.DEFAULT_SCATTER_SPLIT if scatter_split is None else scatter_split
        self.update_grid = update_grid
        self.render_kwargs = dict(near_distance=self.h["rend_near_dist"], max_samples=self.h["rend_max_samples"],
                                  test_time=False, random_bg=False, anneal_strategy="none", anneal_steps=0)
        # a model with heads: the render slices its channels by these (rendering.py:120-148, 203-224)
        if getattr(model, "pred_sem", False):
            self.render_kwargs["n_sem_cls"] = model.n_sem_cls
        if getattr(model, "pred_norm", False):
            self.render_kwargs["pred_norm_nn_norm"] = bool(self.h.get("pred_norm_nn_norm", False))
        self.use_graph = use_graph
        self.split_backward = bool(split_backward) and use_graph
        self.split_fused = split_backward != "forked"
        self._split = None  # the SplitStep of the captured graph (split_backward and split_eligible)
        self.graph = None
        # defer_optimizer (graph step): the optimizer step of step k runs inside graph k+1 on a side
        # stream, concurrently with step k+1's marcher (which reads no parameter), and joins before
        # the field forward; a refresh of the occupancy grid, or flush_optimizer(), applies a pending
        # step first.  Parameters read between steps are one step behind until flush_optimizer() is
        # called.  N > 1: the gradient all-reduce of step k (eager, after graph k) is ordered before
        # graph k+1 on the same stream, so the deferred step reads the reduced gradient; DDP's
        # 1/world goes in as the step's grad_scale on the fp32 wire (the fp16 wire divides before
        # the sum, as DDP does: grad_scale 1).
        self.defer = bool(defer_optimizer) and use_graph
        self._grad_scale = distributed.grad_scale_after_reduce(model, self.world)
        self._pending = False
        self._rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # marcher jitter stream (CPU generator)
        # optional seed of each grid refresh (global_step -> int); default: drawn from torch's CPU generator
        self.grid_seed = None
        self.last_batch = None  # the dict the last step trained on (graph step: the static buffers)
        # what the captured graph takes its batch from: None (not captured), _HOST_BATCH (step(): copies
        # of a host-built dict) or the DeviceRayDataset whose draw is captured (step_from())
        self._source = None
        self.pose_opt = None  # PoseAdam of the dataset's dR / dT (eager step_from, optimize_ext)
        self._pose_ds = None
        self._log_ring = self._log_buf = self._log_cols = self._log_step = None  # fit()'s device log
        self._log_capacity = self.log_capacity
        self._next_step = 0  # the last step passed to step() / step_from() plus one (a checkpoint's `next_step`)

    log_capacity = 1024  # rows of the log ring when a step_from() captures the graph before any fit()

    def flush_optimizer(self):
        """Apply the deferred optimizer step (defer_optimizer) now, if one is pending."""
        if self._pending:
            self.opt.step(grad_scale=self._grad_scale)
            self._pending = False

    def _maybe_update_grid(self, global_step):
        m = self.model
        if self.update_grid and global_step % self.update_interval == 0:
            thr = 0.01 * self.h["rend_max_samples"] / 3 ** 0.5 * self.h["density_tresh_decay"]
            seed = self.grid_seed(global_step) if self.grid_seed is not None else None
            # the pending optimizer step first (the density pass reads the parameters), issued beside
            # the refresh's cell sampling, which reads only the density grid
            m.update_density_grid(thr, warmup=global_step < self.warmup_steps, seed=seed, beside=self.flush_optimizer)
            distributed.broadcast_occupancy(m)

    # -- graph-captured step ---------------------------------------------------------------------
    # The whole step (zero_grad, render with static shapes, losses, backward, [optimizer]) is one
    # HIP graph: the marcher's sample count stays on the device (static_shapes), the loss-weight
    # schedule and Adam's step/lr are device scalars, so nothing in the step reads the host.  A
    # replay costs one launch instead of ~150 Python-driven ones.  Inputs are copied into the
    # graph's static batch buffers (step()), or drawn into them by the graph's own first nodes
    # (step_from(): DeviceRayDataset.batch on the device step counter, and the log row behind the
    # body); the occupancy-grid refresh and the RCCL all-reduce (N > 1) run eagerly around it.
    def _body(self, batch, step_dev, with_opt):
        m = self.model
        if self._source is not _HOST_BATCH:
            # the draw, the rays and the gathers as nodes of the graph, reading the device step counter;
            # on the main stream, ahead of the fork below (the marcher beside the optimizer reads the rays)
            batch = self._source.batch(step_dev, out=batch, seed=self._seed)
        kw = dict(self.render_kwargs, global_step=0, static_shapes=True)
        kw["count_in_loss"] = True  # vr_samples summed by the loss node's first launch (no launch of its own)
        if "march_noise" in batch:
            kw["march_noise"] = batch["march_noise"]
        else:  # jitter drawn on the device from the step counter: no torch RNG node in the graph
            kw["march_rng"] = (self._rng_seed, step_dev)
        if self.defer:
            # the previous step's optimizer (gated: skipped when nothing is pending) beside this step's
            # marcher; joined before the field forward reads the parameters
            cur = torch.cuda.current_stream()
            side = self._side_stream()
            side.wait_stream(cur)

            def optimizer():
                self.opt.step(gated=True, grad_scale=self._grad_scale)
                if not self.opt.pack_fused:
                    m._pack_weights()  # the MLP's fp16 fragments of the updated weights, also beside the marcher
                m._packed_fresh = True  # (pack_fused: the Adam pass has written them)

            def marcher(out=None):
                return march_train_fused(m, batch["rays_o"], batch["rays_d"], kw["near_distance"], kw["max_samples"],
                                         kw.get("march_noise"), kw.get("march_rng"), out=out)

            # (the optimizer on the main stream and the marcher on the side one measured the same:
            # DESIGN.md §7, rounds 4 and 6)
            with torch.cuda.stream(side):
                optimizer()
            kw["premarched"] = marcher()
            cur.wait_stream(side)
        if self._split is not None:
            results, loss_d = self._split.run(batch, step_dev, premarched=kw.get("premarched"))
        else:
            results = render(m, batch["rays_o"], batch["rays_d"], **kw)
            loss_d = self.loss(results, batch, global_step=step_dev)
            # (a constant upstream gradient: no ones_like fill node per step)
            torch.autograd.backward(loss_d["total"], grad_tensors=self._unit(loss_d["total"].device))
        if with_opt and not self.defer:
            self.opt.step()
        if self._source is not _HOST_BATCH:  # (the log row directly behind the body: captured with it)
            self._log_row(results, loss_d, step_dev)
        return results, loss_d

    def _log_row(self, results, loss_d, step_dev):
        """One row of the device log: (step, total, the loss terms, rm_samples, vr_samples) as float32
        into row step % capacity of the ring, by device ops that read the step's outputs and the
        device step counter (capturable: no host value, nothing allocated after the first call)."""
        cols = TrainLog.column_names(loss_d)
        if self._log_ring is None or cols != self._log_cols:
            f = dict(dtype=torch.float32, device=step_dev.device)
            self._log_ring, self._log_buf, self._log_cols = torch.zeros(self._log_capacity, len(cols), **f), torch.zeros(
                len(cols), **f), cols
        with torch.no_grad():
            row, n = self._log_buf, len(cols)
            # the float terms in one launch; the three integers (int64, int32, int64) by a converting copy each
            torch.stack([loss_d["total"]] + [loss_d[k] for k in cols[2:-2]], out=row[1:n - 2])
            row[0].copy_(step_dev)
            row[n - 2].copy_(results["rm_samples"])
            row[n - 1].copy_(results["vr_samples"])
            at = torch.remainder(step_dev, self._log_ring.shape[0]).reshape(1)
            self._log_ring.index_copy_(0, at, row.reshape(1, n))

    def _unit(self, dev):
        """A device fp32 1.0: the upstream gradient of the total loss."""
        if getattr(self, "_one", None) is None or self._one.device != dev:
            self._one = torch.ones((), dtype=torch.float32, device=dev)
        return self._one

    def _side_stream(self):
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.model.flat_params().device)
        return self._side

    def _capture(self, batch, dataset=None):
        """Capture the step.  batch: a host-built dict, cloned into the static buffers that every
        replay's inputs are copied into; or dataset: the static buffers are its buffers() plus the
        constant entries, and the body begins with its draw."""
        if self.render_kwargs.get("anneal_steps", 0) > 0:
            raise NotImplementedError("ray-range annealing is step-dependent host control flow")
        if dataset is not None:
            dev = dataset.device
            self._static = dict(dataset.buffers(), patch_area=dataset.patch_size * dataset.patch_size,
                                x1_offsets_local=dataset.x1_off, x2_offsets_local=dataset.x2_off,
                                x3_offsets_local=dataset.x3_off)
            self._seed = rank_seed(dataset)
        else:
            dev = batch["rays_o"].device
            self._static = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        self._source = _HOST_BATCH if dataset is None else dataset
        from .split_step import SplitStep, split_eligible
        self._split = None
        if self.split_backward and split_eligible(self, self._static):
            try:
                self._split = SplitStep(self, fused=self.split_fused)
            except _lib.NcnError as e:  # the clustering cannot stay resident beside the rgb pass
                warnings.warn(f"split backward unavailable on this device, using the autograd step: {e}")
        self._step_dev = torch.zeros((), dtype=torch.int64, device=dev)
        # the optimizer is in the graph unless the gradient is reduced (or its scatter finished) outside
        self._with_opt = not distributed.is_distributed() and self.model.scatter_split is None
        state = self.opt.state_tensors()
        saved = [t.clone() for t in state]  # warm-up steps must not advance training
        saved_count = self.opt.step_count
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._body(self._static, self._step_dev, self._with_opt)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.model._deferred = []  # (the warm-ups' deferred scatters are dropped with their gradients)
        # the warm-ups' optimizer steps also refreshed the packed MLP fragments (FlatAdam.pack_fused):
        # the captured forward packs for itself unless the deferred optimizer in the body does it
        self.model._packed_fresh = False
        self.graph = torch.cuda.CUDAGraph()
        # No cyclic garbage collection while the capture is open: a dead cycle that holds an earlier
        # Trainer's CUDA graph and its memory pool is destroyed wherever the collector happens to run,
        # and destroying a graph (or freeing its pool) on a capturing thread aborts the process.
        # torch.cuda.graph no longer collects before it begins, so it is done here.
        import gc
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(self.graph):
                self._out = self._body(self._static, self._step_dev, self._with_opt)
        finally:
            if gc_was_on:
                gc.enable()
        # the captured backward's deferred scatter names the graph's static buffers: every replay's
        # reduce_gradients(graph=True) runs that same entry; eager backwards keep their own list
        self.model._deferred_graph = self.model._deferred
        self.model._deferred = []
        for t, v in zip(state, saved):
            t.copy_(v)
        if hasattr(self.model, "prepare_weights"):
            self.model.prepare_weights()  # (the fragments of the restored parameters)
        self.opt.step_count = saved_count
        self.model.flat_grad().zero_()  # (the warm-ups without the optimizer left gradients behind)

    def _graph_step(self, batch, global_step, dataset=None):
        """batch: the host-built dict to copy into the static buffers; or dataset (batch None): the
        captured draw fills them, and the replay's only inputs are the step counter and the gate."""
        if self.graph is None:
            self._capture(batch, dataset)
        self.last_batch = self._static
        dst, src = [], []
        for k, v in ({} if batch is None else batch).items():
            if k in self._static and hasattr(v, "copy_") and v is not self._static[k]:
                dst.append(self._static[k])
                src.append(v)
        fast = len(dst) <= 8 and all(
            s.is_cuda and s.is_contiguous() and d.is_contiguous() and s.dtype == d.dtype and s.shape == d.shape
            for s, d in zip(src, dst))
        gate = 1 if self._pending else 0  # (defer: the previous step's gradient awaits its optimizer step)
        if fast:  # the batch copies, the device step counter and the gate in one launch (ncn_step_inputs)
            _lib.step_inputs(src, dst, self._step_dev, global_step, self.opt.gate if self.defer else None, gate)
        else:
            if dst:
                torch._foreach_copy_(dst, src, non_blocking=True)  # one launch for the whole batch
            self._step_dev.fill_(global_step)
            if self.defer:
                self.opt.gate.fill_(gate)
        self.graph.replay()
        scale = distributed.reduce_gradients(self.model, graph=True) if not self._with_opt else 1.0
        if self.defer:  # (the next graph's side stream applies it, after the reduction above)
            self.opt.step_count += gate
            self._pending = True
        elif not self._with_opt:
            self.opt.step(grad_scale=scale)
        else:
            self.opt.step_count += 1
        return self._out

    status_interval = 100  # steps between reads of the clustering kernel's error word

    def _check_source(self, dataset):
        """One captured graph serves one source.  dataset: None for step()'s host-built batch.  Raises
        before anything is launched."""
        if not self.use_graph:
            return
        if dataset is not None and dataset.optimize_ext:
            raise NotImplementedError(
                "Trainer(use_graph=True) cannot refine the poses of a dataset with optimize_ext: the captured step "
                "renders with static shapes, and that render refuses rays that require grad (rendering.render; "
                "RayMarcher.backward has no static-capacity ray gradient).  Use Trainer(use_graph=False).")
        want = _HOST_BATCH if dataset is None else dataset
        if self._source is None or self._source is want:
            return
        have = ("a host-built batch (step())" if self._source is _HOST_BATCH
                else "the DeviceRayDataset of its first step_from(): the draw is part of the graph")
        raise RuntimeError(f"the captured step takes its batch from {have}; it cannot train on "
                           f"{'a host-built batch' if dataset is None else 'another source'}.  "
                           "Use one Trainer per source.")

    def _prologue(self, global_step):
        """What surrounds every step: the cluster status word, the grid refresh, the epoch's learning rate."""
        if global_step % self.status_interval == 0:
            check_cluster_status(self.model.flat_params().device)  # (raises if an earlier launch timed out)
        self._maybe_update_grid(global_step)
        epoch = global_step // self.steps_per_epoch
        if epoch != self.opt.epoch:
            self.flush_optimizer()  # (a pending step belongs to the previous epoch's learning rate)
        self.opt.set_epoch(epoch)

    def _eager_step(self, batch, global_step):
        m = self.model
        self.last_batch = batch
        kw = dict(self.render_kwargs, global_step=global_step)
        if "march_noise" in batch:
            kw["march_noise"] = batch["march_noise"]
        results = render(m, batch["rays_o"], batch["rays_d"], **kw)
        loss_d = self.loss(results, batch, global_step=global_step)
        loss_d["total"].backward()
        self.opt.step(grad_scale=distributed.reduce_gradients(m))
        return results, loss_d

    def step(self, batch, global_step):
        self._check_source(None)
        self._prologue(global_step)
        out = self._graph_step(batch, global_step) if self.use_graph else self._eager_step(batch, global_step)
        self._next_step = int(global_step) + 1
        return out

    def step_from(self, dataset, global_step):
        """step() with the batch of `global_step` drawn from `dataset` (a data.DeviceRayDataset) with
        this rank's seed (rank_seed); same return value.  Graph step: the first call captures the draw
        with the step (see _capture), a replay copies no batch; the graph then serves this dataset
        only.  Eager step: with dataset.optimize_ext the pose corrections dR / dT take their Adam step
        too (optim.PoseAdam at pose_lr of the epoch; their gradients are cleared before every step, and
        a step with a non-finite pose gradient leaves them and their moments untouched)."""
        self._check_source(dataset)
        pose = None
        if dataset.optimize_ext:
            if self.world > 1:
                raise NotImplementedError("pose refinement is single-process: the pose gradients are not all-reduced")
            pose = self._pose_adam(dataset)
        self._prologue(global_step)
        if self.use_graph:
            out = self._graph_step(None, global_step, dataset)
        else:
            if pose is not None:
                pose.zero_grad()
            out = self._eager_step(dataset.batch(global_step, seed=rank_seed(dataset)), global_step)
            if pose is not None:
                pose.step(cosine_factor(self.opt.epoch, self.h["num_epochs"]) if self.h.get("num_epochs") else 1.0)
        self._next_step = int(global_step) + 1
        return out

    def _pose_adam(self, dataset):
        """The PoseAdam of `dataset`'s dR / dT (optimize_ext): made, with zero moments, the first time
        the dataset is seen."""
        if self._pose_ds is not dataset:
            self.pose_opt, self._pose_ds = PoseAdam([dataset.dR, dataset.dT]), dataset
        return self.pose_opt

    # -- checkpoints -------------------------------------------------------------------------------
    # What a resumed run needs (DESIGN.md §7 lists every buffer that survives a step as state or
    # scratch): the flat parameters, the occupancy grid behind the bitfield, the GradScaler state, the
    # optimizer's moments with its device step counter and learning rate and their host mirrors, the
    # jitter seed, torch's CPU generator (grid-refresh seeds) and the device's (the eager marcher's
    # jitter), the pose corrections with their Adam state, and the next step.  A load writes into the
    # existing tensors: a captured graph names them by address.
    def _state_tensors(self, dataset=None):
        """{name: tensor} of every device tensor a checkpoint holds, under the names of its sections."""
        m, opt = self.model, self.opt
        t = {"model.flat": m.flat_params(), "model.density_bitfield": m.density_bitfield}
        for k in ("density_grid", "amp_state"):
            if getattr(m, k, None) is not None:
                t["model." + k] = getattr(m, k)
        t.update({"optimizer.m": opt.m, "optimizer.v": opt.v, "optimizer.step_dev": opt.step_dev,
                  "optimizer.lr_dev": opt.lr_dev})
        if dataset is not None and dataset.optimize_ext:
            pose = self._pose_adam(dataset)
            t.update({"pose.dR": dataset.dR, "pose.dT": dataset.dT, "pose.t": pose.t})
            for i in range(len(pose.params)):
                t[f"pose.m.{i}"], t[f"pose.v.{i}"] = pose.m[i], pose.v[i]
        return t

    def state_dict(self, dataset=None):
        """A snapshot of the training state (fresh clones on the device; checkpoint.save moves them to
        the CPU): see the section comment above.  A pending deferred optimizer step is applied first
        (flush_optimizer), so it is never part of a checkpoint.  dataset: the DeviceRayDataset the run
        draws from; its signature is recorded, and under optimize_ext its dR / dT and their PoseAdam
        state are saved.  `hparams` is recorded only (a load warns where it differs).  The device log
        is not state: a TrainLog covers one fit call."""
        self.flush_optimizer()
        dev = self.model.flat_params().device
        state = {"format": checkpoint.FORMAT, "version": checkpoint.VERSION,
                 "model_signature": checkpoint.model_signature(self.model), "hparams": dict(self.h),
                 "model": {}, "optimizer": {"step_count": int(self.opt.step_count), "epoch": int(self.opt.epoch),
                                            "lr": float(self.opt.lr)},
                 "rng_seed": int(self._rng_seed), "torch_rng_state": torch.get_rng_state().clone(),
                 "next_step": int(self._next_step)}
        if dev.type == "cuda":
            state["cuda_rng_state"] = torch.cuda.get_rng_state(dev).clone()
        if dataset is not None:
            state["dataset_signature"] = checkpoint.dataset_signature(dataset)
        for name, t in self._state_tensors(dataset).items():
            node, *path = name.split(".")
            if node == "pose" and len(path) == 2:  # pose.m.i / pose.v.i: lists in parameter order
                state.setdefault("pose", {}).setdefault(path[0], []).append(t.detach().clone())
            else:
                state.setdefault(node, {})[path[0]] = t.detach().clone()
        return state

    @staticmethod
    def _state_lookup(state, name):
        """The entry of `state` that _state_tensors calls `name`, or None."""
        node = state
        for k in name.split("."):
            if isinstance(node, dict):
                node = node.get(k)
            elif isinstance(node, (list, tuple)) and k.isdigit() and int(k) < len(node):
                node = node[int(k)]
            else:
                return None
        return node

    def load_state_dict(self, state, dataset=None):
        """Continue from `state` (state_dict(), or checkpoint.load of a file).  Everything is checked
        before anything changes — the format, the model's signature, with pose state in `state` the
        dataset (needed then, with optimize_ext and the checkpoint's signature), every tensor's shape
        and dtype — and a refusal (ValueError) leaves the trainer as it was.  Hyper-parameters that
        differ from the recorded ones are listed in a warning, and so is a dataset whose signature
        differs when no pose state depends on it; the trainer's own values stay.

        The load copies into the existing tensors (no tensor is rebound, so a captured graph replays
        on the loaded state), drops a pending deferred optimizer step, zeroes the flat gradient,
        restores the optimizer's host mirrors, the jitter seed and both generators, and packs the MLP
        fragments of the loaded weights (prepare_weights).  The captured step holds the jitter seed as
        a constant: a trainer that has captured takes a checkpoint of the same seed only (its own
        snapshots); load into a new Trainer otherwise.  Returns `next_step`."""
        checkpoint.check_header(state, "the state")
        m, opt = self.model, self.opt
        checkpoint.check_signature(state.get("model_signature", {}), checkpoint.model_signature(m), "model")
        has_pose = "pose" in state
        if has_pose:
            if dataset is None or not dataset.optimize_ext:
                raise ValueError("the checkpoint holds pose corrections (dR / dT and their Adam state): load it with "
                                 "the DeviceRayDataset(optimize_ext=True) they belong to")
            checkpoint.check_signature(state.get("dataset_signature", {}), checkpoint.dataset_signature(dataset),
                                       "dataset")
        targets = self._state_tensors(dataset if has_pose else None)
        problems, plan = [], []
        for name, dst in targets.items():
            src = self._state_lookup(state, name)
            if not isinstance(src, torch.Tensor):
                problems.append(f"{name}: missing")
            elif tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                problems.append(f"{name}: {tuple(src.shape)} {src.dtype}, the trainer's is {tuple(dst.shape)} {dst.dtype}")
            else:
                plan.append((dst, src))
        for k in ("density_grid", "amp_state"):
            if isinstance(state.get("model", {}).get(k), torch.Tensor) and "model." + k not in targets:
                problems.append(f"model.{k}: in the checkpoint, but the model has none")
        for k, kind in (("step_count", int), ("epoch", int), ("lr", float)):
            if not isinstance(state.get("optimizer", {}).get(k), kind):
                problems.append(f"optimizer.{k}: missing")
        for k in ("rng_seed", "next_step"):
            if not isinstance(state.get(k), int):
                problems.append(f"{k}: missing")
        rng = [("torch_rng_state", True)] + [("cuda_rng_state", m.flat_params().is_cuda)]
        for k, needed in rng:
            if needed and not (isinstance(state.get(k), torch.Tensor) and state[k].dtype == torch.uint8):
                problems.append(f"{k}: missing")
        if self.graph is not None and isinstance(state.get("rng_seed"), int) and state["rng_seed"] != self._rng_seed:
            problems.append("rng_seed: this trainer's captured step holds its own jitter seed as a constant; load the "
                            "checkpoint into a new Trainer, before its first step")
        if problems:
            raise ValueError("the checkpoint does not fit this trainer (nothing was loaded): " + "; ".join(problems))
        diff = checkpoint.signature_diff(state.get("hparams", {}), self.h)
        if diff:
            warnings.warn("hyper-parameters differ from the checkpoint's (the trainer's own are used): " + "; ".join(diff))
        if not has_pose and dataset is not None and "dataset_signature" in state:
            diff = checkpoint.signature_diff(state["dataset_signature"], checkpoint.dataset_signature(dataset))
            if diff:
                warnings.warn("the dataset differs from the checkpoint's (its draws will not continue the saved run): "
                              + "; ".join(diff))
        # ---- nothing has changed up to here ----
        with torch.no_grad():
            for dst, src in plan:
                dst.copy_(src)
            m.flat_grad().zero_()
        self._pending = False  # (a pending step's gradient belonged to the state that was replaced)
        if has_pose:
            self.pose_opt.zero_grad()
        o = state["optimizer"]
        opt.step_count, opt.epoch, opt.lr = o["step_count"], o["epoch"], o["lr"]
        self._rng_seed = state["rng_seed"]
        torch.set_rng_state(state["torch_rng_state"].cpu())
        if m.flat_params().is_cuda:
            torch.cuda.set_rng_state(state["cuda_rng_state"].cpu(), m.flat_params().device)
        m.prepare_weights()
        self._next_step = state["next_step"]
        return self._next_step

    def save_checkpoint(self, path, dataset=None):
        """checkpoint.save(self.state_dict(dataset), path): rank 0 writes, the other ranks (which hold
        the same parameters) only flush their pending optimizer step and return None.  The generator
        states in the file are rank 0's."""
        if distributed.rank() != 0:
            self.flush_optimizer()
            return None
        return checkpoint.save(self.state_dict(dataset), path)

    def load_checkpoint(self, path, dataset=None):
        """load_state_dict of the file (every rank loads it); returns its `next_step`, the
        `start_step` of the fit that continues the run."""
        return self.load_state_dict(checkpoint.load(path, map_location=self.model.flat_params().device), dataset)

    def fit(self, dataset, n_steps, start_step=0, callback=None, callback_every=0, log_capacity=None,
            checkpoint_every=0, checkpoint_path=None):
        """Train on `dataset` for the steps [start_step, start_step + n_steps) (step_from each) and
        return their TrainLog.

        After every step one row (TrainLog's columns) goes into a device ring at row step % capacity,
        written by device ops — in the graph step captured once, directly behind the body, so a replay
        logs with no Python work.  log_capacity (default n_steps) is the ring's rows; the ring is read
        back ("drained", one copy) every log_capacity steps and at the end, and between drains fit
        reads nothing from the device but the cluster status word every `status_interval` steps.  The
        ring belongs to the captured graph: a later fit on the same trainer keeps its rows and drains
        at least that often.

        callback(trainer, global_step), callback_every > 0: called after the step `global_step`
        whenever (global_step + 1) % callback_every == 0, i.e. each time the total number of steps
        trained reaches a multiple of callback_every; flush_optimizer() has run, so the model holds
        the parameters after that step (a validation render, evaluation.evaluate_views, goes here).
        At the end a pending deferred optimizer step is flushed.

        checkpoint_every > 0 with checkpoint_path: save_checkpoint(path, dataset) after the step
        `global_step` whenever (global_step + 1) % checkpoint_every == 0, and at the end (once, if the
        last step has just been saved).  A "{step}" in the path is replaced by the file's `next_step`
        (global_step + 1: the steps trained, counted from step 0), one file per save; otherwise the
        one file is replaced.  The run continues in another process with
        fit(dataset, n, start_step=trainer.load_checkpoint(path, dataset)).  With checkpoint_every = 0
        nothing is saved and the loop issues what it would without these arguments."""
        n_steps, start_step = int(n_steps), int(start_step)
        capacity = n_steps if log_capacity is None else int(log_capacity)
        if n_steps < 1 or capacity < 1:
            raise ValueError(f"fit: n_steps {n_steps} and log_capacity {capacity} must be at least 1")
        checkpoint_every = int(checkpoint_every)
        if checkpoint_every < 0 or (checkpoint_every > 0 and checkpoint_path is None):
            raise ValueError(f"fit: checkpoint_every {checkpoint_every} needs to be >= 0, and a checkpoint_path when > 0")
        self._check_source(dataset)
        if self.graph is None:  # (a captured graph keeps the ring it was captured with)
            self._log_capacity = capacity
            self._log_ring = None
        log = TrainLog(dataset.batch_size)
        first = start_step  # the first step whose row is still on the device only
        for s in range(start_step, start_step + n_steps):
            results, loss_d = self.step_from(dataset, s)
            if not self.use_graph:
                if self._log_step is None:
                    self._log_step = torch.zeros((), dtype=torch.int64, device=dataset.device)
                self._log_step.fill_(s)
                cols = TrainLog.column_names(loss_d)
                if self._log_ring is not None and cols != self._log_cols and s > first:
                    self._drain(log, first, s - first)  # (a term switched on: the ring changes its columns)
                    first = s
                self._log_row(results, loss_d, self._log_step)
            if s + 1 - first == min(capacity, self._log_ring.shape[0]):
                self._drain(log, first, s + 1 - first)
                first = s + 1
            if callback is not None and callback_every > 0 and (s + 1) % callback_every == 0:
                self.flush_optimizer()
                callback(self, s)
            if checkpoint_every > 0 and (s + 1) % checkpoint_every == 0:
                self._save_numbered(checkpoint_path, dataset)
        self.flush_optimizer()
        self._drain(log, first, start_step + n_steps - first)
        if checkpoint_every > 0 and (start_step + n_steps) % checkpoint_every != 0:
            self._save_numbered(checkpoint_path, dataset)
        return log

    def _save_numbered(self, path, dataset):
        """save_checkpoint under `path` with "{step}" replaced by the next step."""
        return self.save_checkpoint(os.fspath(path).replace("{step}", str(self._next_step)), dataset)

    def _drain(self, log, first_step, count):
        """The ring's rows of `count` steps into the host log: one device-to-host copy."""
        if count > 0:
            log.add_ring(self._log_ring.cpu(), self._log_cols, first_step, count)
