"""Optimizer step of the reference training loop on the flat parameter buffer.

Reference: apex FusedAdam (AdamW mode, eps 1e-15) with two groups — hash-grid features (weight
decay 0) and MLP weights (weight decay 1e-6) — (train_nerf.py:262-285), gradient clipping by global
L2 norm 0.05 (train_nerf.py:955), CosineAnnealingLR(T_max=num_epochs, eta_min=0) stepped once per
epoch (:286-288; `set_epoch`).  Two launches per step (ncn_adam_step: sum of squares whose last
workgroup forms the clip factor and step scalars, then Adam of both groups); the clip factor never
leaves the device.  With `zero_grad_on_step` the Adam pass also zeroes the gradient it consumed, so
the next step needs no zero_grad fill (PL's zero_grad before every backward, folded in).
"""
import math

import torch

from . import _lib
from ._lib import call


def cosine_factor(epoch, num_epochs):
    """CosineAnnealingLR(T_max=num_epochs, eta_min=0) after `epoch` scheduler steps, as a factor of
    the base learning rate (train_nerf.py:286-288): (1 + cos(pi * epoch / num_epochs)) / 2.  The
    scheduler holds every parameter group of the optimizer, the pose group included."""
    return 0.5 * (1 + math.cos(math.pi * epoch / num_epochs))


POSE_LR = 1e-6  # train_nerf.py:275-277 ("learning rate is hard-coded")


class PoseAdam:
    """The reference's third parameter group, [dR, dT] (train_nerf.py:275-277): Adam at lr 1e-6, weight
    decay 0, default betas, and the optimizer's default eps 1e-8 (the group sets none), on a few
    (V, 3) tensors with torch ops: an eager group beside the captured field step.  A step whose
    gradients are not all finite (the fp16 overflow step that ncn_adam_step skips for the field)
    leaves parameters, moments and step count as they are; the test is a device select, not a host
    read.  The gradients are not clipped."""

    def __init__(self, params, lr=POSE_LR, betas=(0.9, 0.999), eps=1e-8):
        self.params = list(params)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        # applied steps, on the device: a skipped step does not count (fp64: 1 - beta^t without loss)
        self.t = torch.zeros((), dtype=torch.float64, device=self.params[0].device)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def state_tensors(self):
        return self.params + self.m + self.v + [self.t]

    @torch.no_grad()
    def step(self, lr_factor=1.0):
        """One Adam step at lr * lr_factor from the parameters' .grad (a missing one: zeros)."""
        grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in self.params]
        ok = torch.stack([torch.isfinite(g).all() for g in grads]).all()
        b1, b2 = self.betas
        t = self.t + 1
        c1, c2 = (1 - b1 ** t).float(), (1 - b2 ** t).float()
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            m_new = b1 * m + (1 - b1) * g
            v_new = b2 * v + (1 - b2) * g * g
            p_new = p - (self.lr * lr_factor) * (m_new / c1) / ((v_new / c2).sqrt() + self.eps)
            p.copy_(torch.where(ok, p_new, p))
            m.copy_(torch.where(ok, m_new, m))
            v.copy_(torch.where(ok, v_new, v))
        self.t.copy_(torch.where(ok, t, self.t))


class FlatAdam:
    def __init__(self, model, lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=(0.0, 1e-6), max_norm=0.05,
                 num_epochs=None, zero_grad_on_step=False):
        self.model = model
        self.base_lr = self.lr = lr
        self.betas, self.eps, self.wd, self.max_norm = betas, eps, weight_decay, max_norm
        flat = model.flat_params()
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.part = torch.empty(1024, dtype=torch.float32, device=flat.device)
        self.work = torch.zeros(int(_lib.lib().ncn_adam_step_work_floats()), dtype=torch.float32, device=flat.device)
        self.step_count = 0
        # device-side step counter and learning rate: the step kernels read them, so the optimizer
        # step can sit inside a captured HIP graph (the counter is bumped by the sum-of-squares kernel)
        self.step_dev = torch.zeros((), dtype=torch.int32, device=flat.device)
        self.lr_dev = torch.full((), float(lr), dtype=torch.float32, device=flat.device)
        self.num_epochs = num_epochs
        self.n_table = model._n_table
        self.zero_grad_on_step = zero_grad_on_step
        self.epoch = 0
        # gate of a deferred step inside a captured graph (Trainer(defer_optimizer=True)): 0 = no
        # gradient pending, the step is skipped
        self.gate = torch.ones((), dtype=torch.int32, device=flat.device)
        # refresh the model's packed MLP fragments inside the Adam pass (models with pack_target).  A model
        # with heads has more weights behind the field's than ncn_adam_step_packed maps (it requires
        # n - pack_off == NCN_FIELD_NW): it takes the plain step and packs explicitly.
        self.pack_fused = hasattr(model, "pack_target") and not getattr(model, "_heads", None)
        if self.pack_fused:
            model.pack_target()  # (the map is built here, eagerly: a later first call may be inside a capture)

    def zero_grad(self):
        self.model.flat_grad().zero_()

    def set_epoch(self, epoch):
        """CosineAnnealingLR(T_max=num_epochs, eta_min=0) stepped per epoch (train_nerf.py:286-288):
        lr(e) = base_lr * (1 + cos(pi * e / T_max)) / 2.  Writes the device lr the step kernels read
        (also inside a captured graph); a no-op when the epoch is unchanged."""
        if self.num_epochs and epoch != self.epoch:
            self.epoch = epoch
            self.lr = self.base_lr * cosine_factor(epoch, self.num_epochs)  # (x 0.5 is exact: the value as before)
            self.lr_dev.fill_(self.lr)

    def step(self, grad_scale=1.0, gated=False):
        """grad_scale: the gradient used is flat_grad * grad_scale (1/world after an all-reduce SUM).
        gated: the step runs only if the device gate is 1 (a deferred step in a captured graph)."""
        self.step_count += 1
        p = self.model.flat_params()
        g = self.model.flat_grad()
        b1, b2 = self.betas
        args = [p, g, self.m, self.v, p.numel(), self.n_table, grad_scale, self.max_norm, self.lr, b1, b2, self.eps,
                self.wd[0], self.wd[1], self.lr_dev, self.step_dev, self.work, 1 if self.zero_grad_on_step else 0,
                getattr(self.model, "amp_state", None), self.gate if gated else None]
        if self.pack_fused:
            # the field's packed MLP fragments refreshed by the Adam pass itself (ncn_adam_step_packed):
            # afterwards they match the parameters whether the step applied or was skipped
            inv, off, packed, prec = self.model.pack_target()
            call("ncn_adam_step_packed", *args, inv, off, packed, prec)
            self.model._packed_fresh = True
        else:
            call("ncn_adam_step", *args)
            if getattr(self.model, "_heads", None):
                self.model.prepare_weights()  # (the field's and the heads' fragments of the updated weights)

    def state_tensors(self):
        """Every tensor the step mutates (parameters, moments, device counters)."""
        st = [self.model.flat_params(), self.m, self.v, self.step_dev, self.lr_dev]
        amp = getattr(self.model, "amp_state", None)
        return st + ([amp] if amp is not None else [])
