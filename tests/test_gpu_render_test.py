"""The fused test-time render iteration (rendering.render_rays_test; default: driven from the device,
ncn_test_loop_*; test_fused="host": one host read of the alive count per iteration) against the loop
in the reference's structure (test_fused=False: valid mask, host-synced count, masked field evaluation,
scatter back into zero-filled sigmas / rgbs; rendering.py:45-149): opacity, depth, rgb and
total_samples bit-identical, on a random-init model (no ray terminates: the loop runs to the
sample budget) and on a model whose densities were fitted to the room's occupancy (rays stop at the
first surface), for full-image-shaped ray sets.

Where this sits in the chain that pins the test-time image:
  oracle loop == the renderer run with a stub field   tests/test_gpu_render_test_oracle.py (C, D), exact
                                                      in every integer, float bound per ray
  stub run and real run differ only in the field      the field has its own parity tests
  real unfused == real fused (host, device)           here (image-sized ray sets) and part E of that
                                                      file (R = 1 ... 4097, all-miss, R = 0), bit for bit"""
import os
import sys

import pytest
import torch

from ncnerf_amd.ngp_mt import NGPMT, register_grid_buffers
from ncnerf_amd.rendering import render
from ncnerf_amd.synthetic import SyntheticScene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(dev, scene, opaque):
    torch.manual_seed(0)
    m = register_grid_buffers(NGPMT(scale=0.5, grid_size=128).to(dev))
    with torch.no_grad():
        m.density_grid.copy_(torch.from_numpy(scene.density_grid).to(dev) * 10.0)
        m.density_bitfield.copy_(torch.from_numpy(scene.bitfield).to(dev))
    if opaque:
        sys.path.insert(0, ROOT)
        from bench import distill_opaque
        from ncnerf_amd.trainer import Trainer
        distill_opaque(m, Trainer(m, update_grid=False), scene, dev, steps=150)
    return m


@pytest.mark.parametrize("opaque,esf", [(False, 0.0), (True, 0.0), (False, 1.0 / 256)])
def test_fused_test_render_bit_identical(dev, opaque, esf):
    """esf > 0: exponential stepping, where the loop's minimum samples per ray is 4 (rendering.py:65)."""
    scene = SyntheticScene()
    m = _model(dev, scene, opaque)
    ro, rd = scene.image_rays(1, device=dev)
    n = ro.shape[0] // (4 if not opaque else 1)  # (the random model marches the whole budget)
    o, d = ro[:n].contiguous(), rd[:n].contiguous()
    outs = []
    for fused in (False, "host", True):
        st = {}
        with torch.no_grad():
            r = render(m, o, d, near_distance=0.01, max_samples=1024, test_time=True, test_fused=fused,
                       exp_step_factor=esf, loop_stats=st)
        torch.cuda.synchronize()
        outs.append((r, st))
    (a, sa) = outs[0]
    for b, sb in outs[1:]:
        for k in ("opacity", "depth", "rgb"):
            assert torch.equal(a[k], b[k]), k
        assert int(a["total_samples"]) == int(b["total_samples"])
        assert sa["iterations"] <= sb["iterations"] <= sa["iterations"] + 1, (sa, sb)
    if opaque:
        assert float(a["opacity"].mean()) > 0.9  # the fitted model's rays do stop


def test_fused_test_render_two_cascades(dev):
    """The same at scale 1.0 (C = 2: march_test_kernel<false> and the device-driven loop at C > 1, the
    field at extent 2), exponential stepping, a different bitfield per cascade, 4096 rays spread over
    one image (the oracle's test marcher puts 83 % / 17 % of their first 64 samples in cascade 0 / 1):
    the three loop modes bit-identical, iteration counts related as above."""
    import numpy as np
    import scale_cases as sc
    scene = SyntheticScene()
    torch.manual_seed(0)
    m = register_grid_buffers(NGPMT(scale=1.0, grid_size=128).to(dev))
    assert m.cascades == 2
    with torch.no_grad():
        m.density_bitfield.copy_(torch.from_numpy(np.array(sc.cascade_bitfield(2))).to(dev))
        m.flat_params()[: m._n_table].mul_(3e4)  # densities of order 1: some rays stop, some march the budget
    ro, rd = scene.image_rays(1, device=dev)
    step = ro.shape[0] // 4096
    o, d = ro[::step][:4096].contiguous(), rd[::step][:4096].contiguous()
    outs = []
    for fused in (False, "host", True):
        st = {}
        with torch.no_grad():
            r = render(m, o, d, near_distance=0.01, max_samples=1024, test_time=True, test_fused=fused,
                       exp_step_factor=1.0 / 256, loop_stats=st)
        torch.cuda.synchronize()
        outs.append((r, st))
    (a, sa) = outs[0]
    assert int(a["total_samples"]) > 4096 and sa["iterations"] > 1
    assert 0.0 < float(a["opacity"].mean()) and bool(torch.isfinite(a["rgb"]).all())
    for b, sb in outs[1:]:
        for k in ("opacity", "depth", "rgb"):
            assert torch.equal(a[k], b[k]), k
        assert int(a["total_samples"]) == int(b["total_samples"])
        assert sa["iterations"] <= sb["iterations"] <= sa["iterations"] + 1, (sa, sb)
