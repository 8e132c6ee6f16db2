"""Checkpoint files of the training loop, and the reference's weight files.

The reference has three entry points (train_nerf.py:260, 885-898, 960; utils.py): PL's
ModelCheckpoint (a file per `num_epochs`), `--ckpt_path` (resume) and `--weight_path` / `--val_only`
(`load_ckpt`: the model's weights alone).  Here:

* a trainer checkpoint (`save` / `load`; Trainer.save_checkpoint / load_checkpoint build and consume
  the state): one nested dict of tensors, ints, floats, strings, lists and dicts under `format`
  "ncnerf_amd.trainer", `version` 1.  It holds no pickled class, so it loads under
  `torch.load(weights_only=True)`; it is written to `path + ".tmp"` and renamed over `path`, so a
  process killed while it writes never leaves a half-written `path`; only rank 0 writes.
* the reference's weight file (`reference_state_dict` / `load_reference_state_dict`): the keys
  `model.xyz_encoder.params`, `model.sigma_net.params`, `model.rgb_net.params` (and the heads'), the
  density bitfield, the box buffers and the grid, as `slim_ckpt` returns and `load_ckpt` reads them.
  The element order of the parameters is what ngp_mt.py's docstring states (tcnn's padded row-major
  matrices, level-major table); it has not been confirmed against a checkpoint written by tcnn.
* signatures (`model_signature`, `dataset_signature`, `check_signature`): what must agree between
  the saved and the loading side for a load to make sense, compared before anything is written.

Everything here is host code: torch's copies do the work."""
import os
import pickle

import torch

from . import distributed

FORMAT = "ncnerf_amd.trainer"
VERSION = 1

_SCALARS = (bool, int, float, str, type(None))


# ---- signatures ------------------------------------------------------------------------------------
def model_signature(model):
    """What a model must share with a checkpoint's: the scene box and grid (scale, grid_size,
    cascades), the hash table (n_entries), the flat buffer's element count, the MLPs' operand type
    and AMP mode, and the heads as [(module name, outputs), ...] in the flat buffer's order."""
    return dict(scale=float(model.scale), grid_size=int(model.grid_size), cascades=int(model.cascades),
                n_entries=int(model.n_entries), n_flat=int(model.flat_params().numel()),
                precision=str(model.precision), amp=str(model.amp),
                heads=[(str(name), int(n_out)) for name, n_out, _, _ in model._heads])


def dataset_signature(ds):
    """What a DeviceRayDataset must share with a checkpoint's for its pose state to apply and its
    draws to continue: the views, the draw's geometry and seed, and whether it refines the poses."""
    return dict(n_images=int(ds.n_images), H=int(ds.H), W=int(ds.W), batch_size=int(ds.batch_size),
                patch_size=int(ds.patch_size), strategy=str(ds.ray_sampling_strategy),
                corner_mode=int(ds.corner_mode), seed=int(ds.seed), optimize_ext=bool(ds.optimize_ext))


def _plain(v):
    """Lists and tuples compare as lists (a file gives back lists for the tuples that went in)."""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def signature_diff(saved, current):
    """The differing fields of two signatures as ["field: saved X, current Y", ...]."""
    saved, current = _plain(dict(saved)), _plain(dict(current))
    missing = "(absent)"
    return [f"{k}: saved {saved.get(k, missing)!r}, current {current.get(k, missing)!r}"
            for k in list(saved) + [k for k in current if k not in saved]
            if k not in saved or k not in current or saved[k] != current[k]]


def check_signature(saved, current, what):
    """Raise ValueError naming every field in which the checkpoint's signature of `what` ("model",
    "dataset") differs from the current one."""
    diff = signature_diff(saved, current)
    if diff:
        raise ValueError(f"the checkpoint's {what} does not match the current {what}: " + "; ".join(diff))


# ---- trainer checkpoint files -------------------------------------------------------------------------
def _to_file_form(v, where):
    """`v` with every tensor detached on the CPU and every tuple a list; anything but tensors, ints,
    floats, strings, None, lists and dicts with string keys raises TypeError naming its place."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, _SCALARS):
        return v
    if isinstance(v, (list, tuple)):
        return [_to_file_form(x, f"{where}[{i}]") for i, x in enumerate(v)]
    if isinstance(v, dict):
        for k in v:
            if not isinstance(k, str):
                raise TypeError(f"checkpoint state: the key {k!r} of {where} is not a string")
        return {k: _to_file_form(x, f"{where}[{k!r}]") for k, x in v.items()}
    raise TypeError(f"checkpoint state: {where} is a {type(v).__name__}; a checkpoint holds tensors, ints, floats, "
                    "strings, lists and dicts only (it must load with weights_only=True)")


def check_header(state, where):
    """Raise ValueError unless `state` is a dict of this format and of a version this code reads."""
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        got = state.get("format") if isinstance(state, dict) else type(state).__name__
        raise ValueError(f"{where} is not a trainer checkpoint: format {got!r}, expected {FORMAT!r}")
    version = state.get("version")
    if not isinstance(version, int) or isinstance(version, bool) or not 1 <= version <= VERSION:
        raise ValueError(f"{where} has checkpoint version {version!r}; this code reads versions up to {VERSION}")


def save(state, path):
    """Write `state` (Trainer.state_dict()) to `path`; returns the path, or None on a rank other than
    0 (every rank holds the same parameters; there is no collective in here, so the ranks need not
    call it together).  Tensors are copied to the CPU; the file appears under its name only when it is
    complete (`path + ".tmp"`, then os.replace)."""
    check_header(state, "the state")
    plain = _to_file_form(state, "state")  # (refused before the rank test: every rank sees the error)
    if distributed.rank() != 0:
        return None
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        torch.save(plain, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load(path, map_location="cpu"):
    """Read a trainer checkpoint (weights_only: nothing but tensors and plain values is unpickled).
    `format` and `version` are checked before anything else: a foreign file or one written by a
    newer version raises ValueError."""
    path = os.fspath(path)
    try:
        state = torch.load(path, map_location=map_location, weights_only=True)
    except pickle.UnpicklingError as e:
        raise ValueError(f"{path} is not a trainer checkpoint: it holds more than tensors and plain values ({e})")
    check_header(state, path)
    return state


# ---- the reference's weight file ------------------------------------------------------------------------
GRID_KEYS = ("density_grid", "grid_coords")  # what slim_ckpt pops (utils.py:32)
# the system's own entries of a Lightning state_dict (train_nerf.py:239-249 and its metric modules)
_SYSTEM_KEYS = ("directions", "poses", "random_poses", "dR", "dT", "dR_glob_norm_coded", "theta_WF")
_SYSTEM_PREFIXES = ("val_lpips", "train_psnr", "val_psnr", "val_ssim")


def reference_state_dict(model, prefix="model.", slim=False):
    """The model as the reference's weight file holds it: `<prefix><module>.params` of the hash table,
    sigma_net, rgb_net and the heads that are on, `density_bitfield`, the box buffers (center, xyz_min,
    xyz_max, half_size), and `density_grid` / `grid_coords` unless slim (slim_ckpt drops them) — CPU
    copies.  The model's GradScaler state `amp_state` is not part of it: the reference's model has none
    (PL keeps the scaler)."""
    out = {}
    for k, v in model.state_dict().items():
        if k == "amp_state" or (slim and k in GRID_KEYS):
            continue
        out[prefix + k] = v.detach().to("cpu", copy=True)
    return out


def _is_system_key(k):
    return k in _SYSTEM_KEYS or any(k.startswith(p) for p in _SYSTEM_PREFIXES)


def load_reference_state_dict(model, sd_or_path, prefix="model."):
    """The reference's load_ckpt (utils.py:21-26) for this model: `sd_or_path` is a Lightning
    checkpoint ({"state_dict": ...}), a slim dict (slim_ckpt's return value), a dict of un-prefixed
    model keys, or the path of a file that holds one of them as tensors and plain values (a file with
    pickled objects in it — PL's hyper-parameters — is for the caller to torch.load and pass on).

    Keys under `prefix` are the model's; every other key of a prefixed dict, the system's own entries
    of an un-prefixed one (directions, poses, dR, dT, val_lpips*, train_psnr*) and the empty
    `dir_encoder.params` tcnn registers are ignored.  fp16 or fp32 values are cast to the model's
    fp32.  A key the model does not have, or one of another shape, raises ValueError naming it before
    anything is copied.  The copies are in place — the parameters stay views of the flat buffer — and
    the packed MLP fragments are marked stale.  A key that is absent keeps the model's value
    (load_ckpt fills it from the model's own state_dict).  Returns (loaded_keys, ignored_keys), the
    keys as they stand in the dict."""
    sd = sd_or_path
    if isinstance(sd, (str, os.PathLike)):
        try:
            sd = torch.load(os.fspath(sd), map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as e:
            raise ValueError(f"{os.fspath(sd_or_path)} holds more than tensors and plain values ({e}); torch.load it "
                             "yourself if you trust it and pass the dict")
    if not isinstance(sd, dict):
        raise ValueError(f"a state dict is needed (got {type(sd).__name__})")
    if isinstance(sd.get("state_dict"), dict):  # a pytorch-lightning checkpoint (utils.py:7-8)
        sd = sd["state_dict"]
    prefixed = bool(prefix) and any(isinstance(k, str) and k.startswith(prefix) for k in sd)
    target = model.state_dict()  # (detached aliases of the parameters and buffers)
    plan, loaded, ignored, problems = [], [], [], []
    for key, v in sd.items():
        if prefixed and not key.startswith(prefix):
            ignored.append(key)
            continue
        k = key[len(prefix):] if prefixed else key
        if not isinstance(v, torch.Tensor):
            problems.append(f"{key}: not a tensor ({type(v).__name__})")
        elif k in target:
            dst = target[k]
            if tuple(v.shape) != tuple(dst.shape):
                problems.append(f"{key}: shape {tuple(v.shape)}, the model's is {tuple(dst.shape)}")
            elif v.is_floating_point() != dst.is_floating_point():
                problems.append(f"{key}: dtype {v.dtype}, the model's is {dst.dtype}")
            else:
                plan.append((key, dst, v))
        elif (k == "dir_encoder.params" and v.numel() == 0) or (not prefixed and _is_system_key(k)):
            ignored.append(key)
        else:
            problems.append(f"{key}: the model has no such parameter or buffer")
    if problems:
        raise ValueError("the state dict does not fit the model (nothing was loaded): " + "; ".join(problems))
    with torch.no_grad():
        for key, dst, v in plan:
            dst.copy_(v)  # (casts fp16 to the fp32 master copy, moves to the model's device)
            loaded.append(key)
    model._packed_fresh = False  # (the next forward packs the loaded weights)
    return loaded, ignored
