"""Host side of the semantic / normal heads (include/ncnerf_heads.h): the binding, the refusals that
precede the library, the model's parameters and flat buffers, the loss constructor.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from ncnerf_amd import _lib, ngp_mt
from ncnerf_amd.losses import NeRFMTLoss
from ncnerf_amd.ngp_mt import NGPMT
from ncnerf_amd.trainer import HYPERSIM_HPARAMS
from test_abi import NAMES as ALL_NAMES, altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ncnerf_heads.h"
NAMES = ALL_NAMES[HEADER]


def test_header_parses_into_its_own_table():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    assert set(_lib.symbols(HEADER)) == NAMES
    fwd = _lib.ABI["ncn_head_fwd"][1]
    assert fwd[0] == ("ptr", 2, "enc_cache") and fwd[-1] == ("ptr", 0, "stream")


def test_name_clash_with_another_header_is_an_error(tmp_path):
    clash = altered_headers(tmp_path, HEADER,
                            "int ncn_morton3D(const int32_t* coords, int64_t n, int32_t* out, void* stream);\n")
    with pytest.raises(_lib.NcnError, match="ncn_morton3D is declared in include/ncnerf_heads.h and in include/ncnerf.h"):
        _lib.load_headers(clash)
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*semantic / normal heads"):
        _lib.load_headers(gone)


def test_every_name_binds_with_int_restype():
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name], name
    assert L.ncn_head_packed_halves(5) == ngp_mt.N_HEAD_PACKED_HALVES == L.ncn_head_packed_halves(48)
    assert L.ncn_head_packed_halves(0) == -1 and L.ncn_head_packed_halves(49) == -1
    assert L.ncn_head_bwd_blocks(4099) == L.ncn_field_bwd_blocks(4099)


def test_refusals_precede_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda: _lib.P(0x5EED))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    dev_like = _lib.P(16)
    host_f16, host_f32 = torch.zeros(64, dtype=torch.float16), torch.zeros(64)
    with pytest.raises(TypeError, match=r"ncn_head_fwd: argument 0 \(enc_cache\).*CUDA.*cpu tensor"):
        _lib.call("ncn_head_fwd", host_f16, 16, None, dev_like, dev_like, 3, 0, dev_like)
    with pytest.raises(TypeError, match=r"ncn_head_fwd: argument 0 \(enc_cache\).*2-byte"):  # a wrong width
        _lib.call("ncn_head_fwd", host_f32, 16, None, dev_like, dev_like, 3, 0, dev_like)
    with pytest.raises(TypeError, match=r"ncn_head_bwd: argument 7 \(dL_dout\)"):
        _lib.call("ncn_head_bwd", dev_like, 16, None, dev_like, dev_like, 3, 0, host_f32, None, dev_like, dev_like)
    with pytest.raises(TypeError, match=r"ncn_composite_extra_fw: argument 2 \(rays_a\).*8-byte"):
        _lib.call("ncn_composite_extra_fw", dev_like, dev_like, torch.zeros(3, dtype=torch.int32), 1, 4, 3, dev_like)
    with pytest.raises(TypeError, match=r"ncn_head_pack_weights: argument 1 \(n_out\)"):
        _lib.call("ncn_head_pack_weights", dev_like, 3.0, dev_like, 0)


def test_extra_channels_refuses_host_tensors():
    from ncnerf_amd.custom_functions import ExtraChannels
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ExtraChannels.apply(torch.zeros(4), torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int64))


def test_model_with_heads_on_cpu():
    m = NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=5, pred_norm=True)
    names = dict(m.named_parameters())
    assert list(names) == ["xyz_encoder.params", "sigma_net.params", "rgb_net.params", "sem_net.params",
                           "norm_net.params"]
    # tcnn's counts: 1024 + 4096 + 64 * 16 * ceil(n_out / 16)
    assert names["sem_net.params"].numel() == names["norm_net.params"].numel() == 1024 + 4096 + 1024 == ngp_mt.head_nw(5)
    assert ngp_mt.head_nw(16) == 6144 and ngp_mt.head_nw(17) == 7168 and ngp_mt.head_nw(48) == 8192
    assert names["rgb_net.params"].numel() == ngp_mt.W_RGB and names["sigma_net.params"].numel() == ngp_mt.W_SIGMA
    # all five are consecutive views of ONE flat buffer, the heads behind W5 (every existing offset stays)
    flat = m.flat_params()
    assert flat.numel() == m._n_table + ngp_mt.N_W + 2 * 6144
    off = 0
    for p in names.values():
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == flat.numel()
    # Xavier-initialised, and the field's initialisation is the heads-off model's
    sem = names["sem_net.params"].detach()
    assert 0 < float(sem[:1024].abs().max()) <= (6.0 / 80) ** 0.5 and float(sem[5120:].abs().max()) <= (6.0 / 80) ** 0.5
    m0 = NGPMT(scale=0.5, grid_size=128)
    assert torch.equal(m0.flat_params(), flat[:m0.flat_params().numel()])
    # the gradients are views of one flat buffer too, and the all-reduce buckets cover all of it
    fg = m.flat_grad()
    off = 0
    for p in names.values():
        assert p.grad.data_ptr() == fg.data_ptr() + 4 * off
        off += p.numel()
    hi, lo = m.grad_buckets(4)
    assert lo.data_ptr() == fg.data_ptr() and hi.data_ptr() == fg.data_ptr() + 4 * lo.numel()
    assert lo.numel() + hi.numel() == fg.numel() == flat.numel()
    with pytest.raises(RuntimeError, match="heads"):  # the packed Adam step maps the field's weights only
        m.pack_target()


def test_model_head_arguments():
    for bad in (0, 49):
        with pytest.raises(ValueError, match="1..48"):
            NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=bad)
    with pytest.raises(NotImplementedError, match="n_sem_cls"):
        NGPMT(scale=0.5, grid_size=128, pred_sem=True)
    m = NGPMT(scale=0.5, grid_size=128, pred_norm=True)
    assert [n for n, _ in m.named_parameters()][-1] == "norm_net.params" and not m.pred_sem and m.pred_norm
    assert NGPMT(scale=0.5, grid_size=128, pred_sem=True, n_sem_cls=48).sem_net.params.numel() == 8192


def test_loss_constructor_with_the_semantic_term():
    loss = NeRFMTLoss(dict(HYPERSIM_HPARAMS, loss_sem_w=1e-3, pred_sem=True, load_sem_gt=True))
    assert loss.sem_w == 1e-3
    # the fused reference-configuration node has no semantic term: never taken with it
    assert not loss.reference_config(64, 64, 64, {"x1": [], "x2": [], "x3": []}, False)
    with pytest.raises(NotImplementedError, match="pred_sem"):
        NeRFMTLoss(dict(HYPERSIM_HPARAMS, loss_sem_w=1e-3))
    for bad in (dict(), dict(load_sem_gt=True, load_sem_WF_gt=True)):  # the reference's asserts, losses.py:235-236
        with pytest.raises(ValueError, match="load_sem_gt"):
            NeRFMTLoss(dict(HYPERSIM_HPARAMS, loss_sem_w=1e-3, pred_sem=True, **bad))
    with pytest.raises(NotImplementedError):  # unreachable in the reference too (losses.py:227-231)
        NeRFMTLoss(dict(HYPERSIM_HPARAMS, loss_manhattan_nerf_w=1e-3, pred_sem=True))
