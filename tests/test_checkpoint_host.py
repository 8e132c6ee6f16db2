"""ncnerf_amd.checkpoint on the host: the reference's weight file (export, import, the reference's
own load recipe), the trainer checkpoint file (atomic write, rank 0 only, weights_only, the refusals)
and the signatures.  NGPMT lives on the CPU here; nothing is launched.

State round trips carry no arithmetic: every comparison is bit for bit."""
import os

import pytest
import torch

from ncnerf_amd import checkpoint, distributed
from ncnerf_amd.ngp_mt import NGPMT, head_nw, register_grid_buffers

G = 16  # a small occupancy grid: the checkpoint code does not depend on its size
BOX = ("center", "xyz_min", "xyz_max", "half_size")
FIELD = ("xyz_encoder.params", "sigma_net.params", "rgb_net.params")


def _model(heads=False, grid=True, **kw):
    if heads:
        kw = dict(kw, pred_sem=True, n_sem_cls=5, pred_norm=True)
    m = NGPMT(scale=0.5, grid_size=G, **kw)
    return register_grid_buffers(m) if grid else m


def _distinct(shape, base, dtype=torch.float32):
    """fp32: base + i, distinct and exact below 2^24.  fp16: base + (i % 1024) / 8, exact in fp16 (below
    256 in steps of 1/8), so a cast to fp32 gives the same numbers whichever side performs it."""
    n = int(torch.tensor(shape).prod()) if len(shape) else 1
    i = torch.arange(n, dtype=torch.float32)
    assert n < 2 ** 24
    return (i + base if dtype == torch.float32 else (i % 1024) / 8 + base).reshape(shape).to(dtype)


# ---- 1. reference export ---------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [False, True], ids=["field", "heads"])
def test_reference_export_keys_shapes_values(heads):
    m = _model(heads)
    with torch.no_grad():
        m.flat_params().copy_(torch.arange(m.flat_params().numel(), dtype=torch.float32))
        m.density_grid.uniform_(0, 1)
        m.density_bitfield.fill_(37)
    names = FIELD + (("sem_net.params", "norm_net.params") if heads else ())
    base = set(names) | set(BOX) | {"density_bitfield"}
    sd = checkpoint.reference_state_dict(m)
    assert set(sd) == {"model." + k for k in base | {"density_grid", "grid_coords"}}
    slim = checkpoint.reference_state_dict(m, slim=True)
    assert set(slim) == {"model." + k for k in base}
    assert set(checkpoint.reference_state_dict(m, prefix="")) == base | {"density_grid", "grid_coords"}
    assert "model.amp_state" not in sd and m.amp_state is not None
    n_t = 2 * m.n_entries
    want = {"xyz_encoder.params": (0, n_t), "sigma_net.params": (n_t, n_t + 3072),
            "rgb_net.params": (n_t + 3072, n_t + 3072 + 7168)}
    if heads:
        a = n_t + 10240
        want["sem_net.params"] = (a, a + head_nw(5))
        want["norm_net.params"] = (a + head_nw(5), a + head_nw(5) + head_nw(3))
        assert m.flat_params().numel() == a + head_nw(5) + head_nw(3)
    flat = m.flat_params()
    for k, (a, b) in want.items():
        t = sd["model." + k]
        assert t.shape == (b - a,) and t.dtype == torch.float32 and t.device.type == "cpu", k
        assert torch.equal(t, flat[a:b]), k
        assert t.data_ptr() != flat[a:b].data_ptr(), k  # (a copy, not a view of the live buffer)
    assert torch.equal(sd["model.density_bitfield"], m.density_bitfield)
    assert sd["model.density_bitfield"].data_ptr() != m.density_bitfield.data_ptr()
    assert torch.equal(sd["model.density_grid"], m.density_grid) and torch.equal(sd["model.grid_coords"], m.grid_coords)
    for k in BOX:
        assert torch.equal(sd["model." + k], getattr(m, k))


# ---- 2. reference import ---------------------------------------------------------------------------
def _lightning_dict(m, dtype=torch.float32):
    """A Lightning-style state_dict around distinct model values, in the reference's key order."""
    sd = {"directions": torch.zeros(7, 3), "poses": torch.zeros(2, 3, 4)}
    for i, k in enumerate(FIELD):
        sd["model." + k] = _distinct(tuple(m.state_dict()[k].shape), 1.0 + i, dtype)
    sd["model.dir_encoder.params"] = torch.zeros(0, dtype=dtype)
    sd["model.density_bitfield"] = torch.full_like(m.density_bitfield, 5)
    sd["model.density_grid"] = _distinct(tuple(m.density_grid.shape), 9.0)
    sd["val_lpips.net.x"] = torch.ones(3)
    return sd


def _flat_of(sd, prefix="model."):
    return torch.cat([sd[prefix + k].float() for k in FIELD])


def test_reference_import_lightning_slim_and_plain():
    m = _model()
    ptr = m.flat_params().data_ptr()
    inner = _lightning_dict(m)
    loaded, ignored = checkpoint.load_reference_state_dict(m, {"state_dict": inner, "epoch": 3})
    assert ignored == ["directions", "poses", "model.dir_encoder.params", "val_lpips.net.x"]
    assert loaded == ["model." + k for k in FIELD] + ["model.density_bitfield", "model.density_grid"]
    assert torch.equal(m.flat_params(), _flat_of(inner))
    assert torch.equal(m.density_grid, inner["model.density_grid"]) and bool((m.density_bitfield == 5).all())
    named = dict(m.named_parameters())
    assert named["xyz_encoder.params"].data_ptr() == m.flat_params().data_ptr() == ptr
    assert named["sigma_net.params"].data_ptr() == m.flat_params()[2 * m.n_entries:].data_ptr()
    assert m._packed_fresh is False
    # the slim form: no grid, nothing but the model's keys
    m2 = _model()
    grid_before = m2.density_grid.clone().fill_(0.25)
    with torch.no_grad():
        m2.density_grid.fill_(0.25)
    slim = {k: v for k, v in inner.items() if k.startswith("model.") and k != "model.density_grid"}
    m2._packed_fresh = True
    loaded, ignored = checkpoint.load_reference_state_dict(m2, slim)
    assert ignored == ["model.dir_encoder.params"] and "model.density_grid" not in loaded
    assert torch.equal(m2.flat_params(), _flat_of(inner)) and torch.equal(m2.density_grid, grid_before)
    assert m2._packed_fresh is False
    # un-prefixed keys, with the system's own entries beside them
    m3 = _model()
    plain = {k[len("model."):] if k.startswith("model.") else k: v for k, v in inner.items()}
    loaded, ignored = checkpoint.load_reference_state_dict(m3, plain)
    assert ignored == ["directions", "poses", "dir_encoder.params", "val_lpips.net.x"]
    assert torch.equal(m3.flat_params(), _flat_of(inner))


def test_reference_import_from_a_file(tmp_path):
    m = _model()
    inner = _lightning_dict(m)
    torch.save({"state_dict": inner}, tmp_path / "epoch=29.ckpt")
    loaded, _ = checkpoint.load_reference_state_dict(m, tmp_path / "epoch=29.ckpt")
    assert len(loaded) == 5 and torch.equal(m.flat_params(), _flat_of(inner))


def test_reference_import_casts_fp16():
    m = _model()
    inner = _lightning_dict(m, torch.float16)
    assert inner["model.xyz_encoder.params"].dtype == torch.float16
    checkpoint.load_reference_state_dict(m, inner)
    assert m.flat_params().dtype == torch.float32
    assert torch.equal(m.flat_params(), _flat_of(inner))  # (the values are exact in fp16)
    assert float(m.flat_params().max()) > 100


def test_reference_import_refuses_a_wrong_shape_before_copying():
    m = _model()
    before = m.flat_params().clone()
    bits = m.density_bitfield.clone()
    inner = _lightning_dict(m)
    # the bad key comes last of the parameters: the ones before it must not have been copied
    inner["model.rgb_net.params"] = torch.zeros(7168 + 16)
    with pytest.raises(ValueError, match=r"model\.rgb_net\.params"):
        checkpoint.load_reference_state_dict(m, inner)
    assert torch.equal(m.flat_params(), before) and torch.equal(m.density_bitfield, bits)
    # a head's weights into a model without that head: named, nothing copied
    inner = _lightning_dict(m)
    inner["model.sem_net.params"] = torch.zeros(head_nw(5))
    with pytest.raises(ValueError, match=r"model\.sem_net\.params"):
        checkpoint.load_reference_state_dict(m, inner)
    assert torch.equal(m.flat_params(), before)


def test_reference_export_loads_back_with_heads():
    a, b = _model(heads=True, seed=1), _model(heads=True, seed=2)
    with torch.no_grad():
        a.density_grid.uniform_(0, 1)
        a.density_bitfield.fill_(129)
    assert not torch.equal(a.flat_params(), b.flat_params())
    loaded, ignored = checkpoint.load_reference_state_dict(b, checkpoint.reference_state_dict(a))
    assert ignored == [] and len(loaded) == len(a.state_dict()) - 1  # (all but amp_state)
    assert torch.equal(a.flat_params(), b.flat_params())
    assert torch.equal(a.density_grid, b.density_grid) and torch.equal(a.density_bitfield, b.density_bitfield)
    assert dict(b.named_parameters())["norm_net.params"].data_ptr() == b.flat_params()[b._heads[1][2]:].data_ptr()


# ---- 3. the reference's own recipe --------------------------------------------------------------------
def test_reference_recipe_keeps_the_parameters_views():
    """utils.py:21-26: d = model.state_dict(); d.update(stripped); model.load_state_dict(d)."""
    m = _model()
    inner = _lightning_dict(m)
    stripped = {k[len("model."):]: v for k, v in inner.items() if k.startswith("model.") and v.numel() > 0}
    m._packed_fresh = True
    d = m.state_dict()
    d.update(stripped)
    m.load_state_dict(d)
    assert torch.equal(m.flat_params(), _flat_of(inner))
    off = 0
    for name, p in m.named_parameters():
        assert p.data_ptr() == m.flat_params()[off:].data_ptr(), name
        off += p.numel()
    assert off == m.flat_params().numel() and m._packed_fresh is False
    # ... and it reads what reference_state_dict writes
    src = _model(seed=5)
    d = m.state_dict()
    d.update({k[len("model."):]: v for k, v in checkpoint.reference_state_dict(src).items()})
    m.load_state_dict(d)
    assert torch.equal(m.flat_params(), src.flat_params())


# ---- 4. the file ---------------------------------------------------------------------------------------
def _state():
    return {"format": checkpoint.FORMAT, "version": checkpoint.VERSION,
            "model": {"flat": torch.arange(12, dtype=torch.float32)}, "optimizer": {"step_count": 6, "lr": 1e-2},
            "hparams": {"ray_sampling_strategy": "all_images_triang_patch", "pred_norm_depth": True},
            "model_signature": {"heads": [("sem_net", 5)]}, "pose": {"m": [torch.zeros(2, 3), torch.ones(2, 3)]},
            "t": torch.tensor(2.0, dtype=torch.float64), "next_step": 1011}


def test_save_is_atomic_and_loads_weights_only(tmp_path, monkeypatch):
    path = tmp_path / "c.pt"
    path.write_bytes(b"an older file")
    seen = {}
    real_replace = os.replace

    def replace(src, dst):
        # the complete file exists under the temporary name while `path` still holds the old one
        seen["tmp"] = src
        seen["old"] = open(dst, "rb").read()
        seen["tmp_loads"] = torch.load(src, weights_only=True)["next_step"]
        real_replace(src, dst)

    monkeypatch.setattr(os, "replace", replace)
    assert checkpoint.save(_state(), path) == str(path)
    assert seen == {"tmp": str(path) + ".tmp", "old": b"an older file", "tmp_loads": 1011}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c.pt"]
    raw = torch.load(path, weights_only=True)  # (no pickled class inside)
    got = checkpoint.load(path)
    want = _state()
    for st in (raw, got):
        assert torch.equal(st["model"]["flat"], want["model"]["flat"])
        assert st["t"].dtype == torch.float64 and st["t"].item() == 2.0
        assert st["optimizer"] == want["optimizer"] and st["hparams"] == want["hparams"] and st["next_step"] == 1011
        assert st["model_signature"]["heads"] == [["sem_net", 5]]  # (tuples come back as lists)
        assert torch.equal(st["pose"]["m"][1], torch.ones(2, 3))


def test_a_failed_write_leaves_the_old_file(tmp_path, monkeypatch):
    path = tmp_path / "c.pt"
    path.write_bytes(b"an older file")

    def broken(obj, f):
        open(f, "wb").write(b"half")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", broken)
    with pytest.raises(OSError):
        checkpoint.save(_state(), path)
    assert path.read_bytes() == b"an older file"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c.pt"]


def test_only_rank_zero_writes(tmp_path, monkeypatch):
    monkeypatch.setattr(distributed, "rank", lambda: 1)
    assert checkpoint.save(_state(), tmp_path / "c.pt") is None
    assert list(tmp_path.iterdir()) == []


# ---- 5. refusals -----------------------------------------------------------------------------------------
def test_load_refuses_foreign_and_newer_files(tmp_path):
    torch.save(dict(_state(), format="somebody.else"), tmp_path / "foreign.pt")
    with pytest.raises(ValueError, match="format"):
        checkpoint.load(tmp_path / "foreign.pt")
    torch.save({"state_dict": {}}, tmp_path / "lightning.pt")
    with pytest.raises(ValueError, match="format"):
        checkpoint.load(tmp_path / "lightning.pt")
    torch.save(dict(_state(), version=2), tmp_path / "newer.pt")
    with pytest.raises(ValueError, match="version 2"):
        checkpoint.load(tmp_path / "newer.pt")
    torch.save(dict(_state(), cls=os.stat_result), tmp_path / "pickled.pt")  # (a pickled class reference)
    with pytest.raises(ValueError, match="plain values"):
        checkpoint.load(tmp_path / "pickled.pt")


def test_save_refuses_what_is_not_plain(tmp_path):
    class Thing:
        pass

    for bad, where in ((dict(_state(), loss=Thing()), "loss"), (dict(_state(), model={"flat": [Thing()]}), "flat"),
                       (dict(_state(), hparams={3: 1}), "hparams")):
        with pytest.raises(TypeError, match=where):
            checkpoint.save(bad, tmp_path / "c.pt")
    with pytest.raises(ValueError, match="format"):
        checkpoint.save({"model": {}}, tmp_path / "c.pt")
    assert list(tmp_path.iterdir()) == []


# ---- 6. signatures -----------------------------------------------------------------------------------------
def test_model_signature_fields():
    m = _model(heads=True)
    sig = checkpoint.model_signature(m)
    assert sig == dict(scale=0.5, grid_size=G, cascades=1, n_entries=m.n_entries, n_flat=m.flat_params().numel(),
                       precision="fp16", amp="internal", heads=[("sem_net", 5), ("norm_net", 3)])
    checkpoint.check_signature(sig, checkpoint.model_signature(_model(heads=True, seed=3)), "model")
    # through a file: lists for tuples, still equal
    checkpoint.check_signature(checkpoint._to_file_form(sig, "sig"), sig, "model")


def test_check_signature_names_every_differing_field():
    a = checkpoint.model_signature(NGPMT(scale=0.5, grid_size=64))
    b = checkpoint.model_signature(NGPMT(scale=0.5, grid_size=128, precision="bf16", pred_norm=True))
    with pytest.raises(ValueError) as e:
        checkpoint.check_signature(a, b, "model")
    msg = str(e.value)
    assert "model" in msg
    assert "grid_size: saved 64, current 128" in msg
    assert "precision: saved 'fp16', current 'bf16'" in msg
    assert "heads: saved [], current [['norm_net', 3]]" in msg
    assert "n_flat" in msg  # (the head's weights lengthen the flat buffer)
    for same in ("scale", "cascades", "n_entries", "amp"):
        assert same + ":" not in msg
    # one field alone
    with pytest.raises(ValueError, match="heads") as e:
        checkpoint.check_signature(a, dict(a, heads=[("sem_net", 5)]), "model")
    assert "grid_size" not in str(e.value)


class _FakeDataset:
    n_images, H, W, batch_size, patch_size = 5, 20, 24, 1024, 8
    ray_sampling_strategy, corner_mode, seed, optimize_ext = "all_images_triang_patch", 0, 21, True


def test_dataset_signature():
    sig = checkpoint.dataset_signature(_FakeDataset())
    assert sig == dict(n_images=5, H=20, W=24, batch_size=1024, patch_size=8, strategy="all_images_triang_patch",
                       corner_mode=0, seed=21, optimize_ext=True)
    other = _FakeDataset()
    other.n_images, other.seed = 4, 22
    with pytest.raises(ValueError, match="n_images: saved 5, current 4.*seed: saved 21, current 22"):
        checkpoint.check_signature(sig, checkpoint.dataset_signature(other), "dataset")
