"""Geometry supervision on a host without a GPU: include/ncnerf_geom.h parses into a table of its
own beside the two-header table, its entry points bind with an int restype and refuse wrong arguments
before the library is reached; DeviceRayDataset checks its label planes; and the float64 torch
restatement of the four terms (tests/geom_ref.py), the reference of the GPU tests' bounds, reproduces
the reference's own float64 results in tests/golden/geom_losses.npz."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import geom_ref
from ncnerf_amd import _lib
from ncnerf_amd._lib import F32, I32, I64, P
from test_abi import NAMES as ALL_NAMES, altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "geom_losses.npz")
HEADER = "ncnerf_geom.h"
NAMES = ALL_NAMES[HEADER]
CASES = ("depth", "norm", "norm_gtdepth", "reg_off", "reg_on", "all", "empty", "nan")


# ---- the ABI ----
def test_geom_header_parses_into_a_table_of_its_own():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    assert set(_lib.symbols(HEADER)) == NAMES <= set(_lib.exported_symbols())


def test_known_signatures():
    assert _lib.SIGNATURES["ncn_geom_loss_fwd"] == [P, P, I64, P, P, P, P, P, I64, I32, F32, F32, F32, P, I64, I64, P,
                                                    I64, P, P, P]
    assert _lib.SIGNATURES["ncn_geom_loss_bwd"] == [P, P, I64, P, P, P, P, P, I64, P, P, I32, F32, F32, F32, P, P, P, P,
                                                    P]
    assert _lib.SIGNATURES["ncn_batch_labels_fw"] == [P, P, I64, P, P, P, I32, I64, P, P, P, P]
    fwd = _lib.ABI["ncn_geom_loss_fwd"][1]
    assert fwd[16] == ("ptr", 8, "ws") and fwd[19] == ("ptr", 8, "counts") and fwd[13] == ("ptr", 8, "step_dev")


def test_library_binds_the_new_names_as_int():
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name]


def test_header_constants_match_the_package():
    from ncnerf_amd import losses
    text = _lib.read_header(HEADER)
    got = {k: int(v) for k, v in re.findall(r"^#define NCN_GEOM_(\w+) (\d+)$", text, flags=re.M)}
    assert got == {"DEPTH": losses.GEOM_DEPTH, "NORM_L1": losses.GEOM_NORM_L1, "NORM_DOT": losses.GEOM_NORM_DOT,
                   "REG": losses.GEOM_REG} == {"DEPTH": 1, "NORM_L1": 2, "NORM_DOT": 4, "REG": 8}
    # the workspace formula of the header: 6 * min(ceil(n / 256), 1024)
    assert [losses.geom_workspace_doubles(r, t) for r, t in ((0, 0), (64, 49), (256, 196), (257, 0), (8192, 6272),
                                                             (262144, 0), (262145, 7), (10, 10 ** 7))] == [
        6, 6, 6, 12, 192, 6144, 6144, 6144]


def test_a_name_in_two_headers_is_an_error(tmp_path):
    clash = altered_headers(tmp_path, HEADER, "int ncn_geom_loss_fwd(int a, void* stream);\nint ncn_version(void);\n")
    with pytest.raises(_lib.NcnError, match="ncn_version is declared in include/ncnerf_geom.h and in include/ncnerf.h"):
        _lib.load_headers(clash)


def test_missing_geom_header_names_the_path(tmp_path):
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*geometry supervision"):
        _lib.load_headers(gone)


# ---- refusals precede the call ----
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    monkeypatch.setattr(_lib, "stream", lambda: P(0x5EED))


def _fwd_args(**over):
    d = P(16)
    a = dict(depth=d, depth_gt=d, n_rays=64, normals=d, normals_gt=d, x1=d, x2=d, x3=d, n_tri=49, terms=15,
             w_depth=0.1, w_l1=0.1, w_dot=0.1, step_dev=None, step=3, reg_start=0, ws=d, ws_doubles=6, out=d,
             counts=d)
    a.update(over)
    return tuple(a.values())


def test_host_tensor_wrong_width_and_wrong_count_are_refused(no_library):
    assert len(_lib.marshal("ncn_geom_loss_fwd", _fwd_args())) == 21  # (the stream appended)
    with pytest.raises(TypeError, match=r"ncn_geom_loss_fwd: argument 0 \(depth\).*CUDA.*float32 cpu tensor"):
        _lib.call("ncn_geom_loss_fwd", *_fwd_args(depth=torch.zeros(64)))
    with pytest.raises(TypeError, match=r"ncn_geom_loss_fwd: argument 16 \(ws\).*8-byte"):
        _lib.call("ncn_geom_loss_fwd", *_fwd_args(ws=torch.zeros(6)))  # float32 for the double workspace
    with pytest.raises(TypeError, match=r"ncn_geom_loss_fwd: argument 5 \(x1\).*8-byte"):
        _lib.call("ncn_geom_loss_fwd", *_fwd_args(x1=torch.zeros(49, dtype=torch.int32)))
    with pytest.raises(TypeError, match=r"argument 14 \(step\)"):
        _lib.call("ncn_geom_loss_fwd", *_fwd_args(step=torch.tensor(3)))  # a tensor for the host step
    with pytest.raises(TypeError, match=r"ncn_geom_loss_fwd: takes 20 or 21 arguments, got 19.*reg_start"):
        _lib.call("ncn_geom_loss_fwd", *_fwd_args()[:-1])
    with pytest.raises(TypeError, match=r"ncn_geom_loss_bwd: takes 19 or 20 arguments, got 2"):
        _lib.call("ncn_geom_loss_bwd", P(16), 3)
    with pytest.raises(TypeError, match=r"ncn_batch_labels_fw: argument 0 \(img_idxs\).*8-byte"):
        _lib.call("ncn_batch_labels_fw", torch.zeros(4, dtype=torch.int32), P(16), 4, None, None, None, 1, 4, None, None,
                  None)
    with pytest.raises(TypeError, match=r"ncn_batch_labels_fw: argument 3 \(depth\).*CUDA.*cpu tensor"):
        _lib.call("ncn_batch_labels_fw", P(16), P(16), 4, torch.zeros(1, 4), None, None, 1, 4, P(16), None, None)


def test_geometry_losses_refuses_host_tensors(no_library):
    from ncnerf_amd.losses import GEOM_DEPTH, geometry_losses
    d = torch.zeros(64)
    with pytest.raises(RuntimeError, match="depth must be a CUDA tensor"):
        geometry_losses(d, None, d, terms=GEOM_DEPTH)
    with pytest.raises(ValueError, match="terms 16"):
        geometry_losses(d, terms=16)


# ---- the dataset's label planes ----
def _dataset_args(V=2, H=8, W=9):
    return dict(images=torch.zeros(V, H * W, 3), poses=torch.zeros(V, 3, 4), directions=torch.zeros(H * W, 3),
                img_wh=(W, H), batch_size=64, patch_size=8)


def test_dataset_checks_the_planes_before_the_device():
    from ncnerf_amd.data import DeviceRayDataset, LABEL_PLANES
    assert LABEL_PLANES == ("depth", "normals", "normals_depth")
    a = _dataset_args()
    with pytest.raises(RuntimeError, match="depth must be a CUDA tensor"):
        DeviceRayDataset(**a, depth=np.zeros((2, 72), np.float32))  # not a tensor
    with pytest.raises(RuntimeError, match=r"normals must be torch.float32 \(got torch.float64\)"):
        DeviceRayDataset(**a, normals=torch.zeros(2, 72, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"depth must be \(2, 72\) for img_wh \(9, 8\) \(got \(2, 72, 1\)\)"):
        DeviceRayDataset(**a, depth=torch.zeros(2, 72, 1))
    with pytest.raises(ValueError, match=r"normals_depth must be \(2, 72, 3\)"):
        DeviceRayDataset(**a, normals_depth=torch.zeros(2, 72))
    with pytest.raises(ValueError, match=r"normals must be \(2, 72, 3\)"):
        DeviceRayDataset(**a, normals=torch.zeros(3, 72, 3))  # another number of views
    # well-formed planes (flat or (V, H, W[, 3])) pass every check and stop at the device, like the images
    for planes in (dict(depth=torch.zeros(2, 72)), dict(depth=torch.zeros(2, 8, 9), normals=torch.zeros(2, 8, 9, 3),
                                                        normals_depth=torch.zeros(2, 72, 3))):
        with pytest.raises(RuntimeError, match="images must be a CUDA tensor"):
            DeviceRayDataset(**a, **planes)


# ---- the restatement against the reference's float64 results ----
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_every_case(golden):
    for tag, R in (("tri", 192), ("patch", 256)):
        assert golden[f"{tag}/depth"].shape == (R,) and golden[f"{tag}/normals_gt"].shape == (R, 3)
        assert (golden[f"{tag}/depth_gt"] == 0).any() and (golden[f"{tag}/depth_gt"] > 0).any()
        for k in ("normals_gt", "normals_depth_gt"):
            zero = np.abs(golden[f"{tag}/{k}"]).sum(-1) == 0
            assert zero.any() and not zero.all()
        for name in CASES:
            assert f"{tag}/{name}/grad_depth64" in golden.files, (tag, name)
    assert geom_ref.triangles(256, "all_images_triang_patch")["x1"].numel() == 196
    c = geom_ref.FixtureCase(golden, "patch", "reg_off")
    assert "reg_depth" not in c.keys and c.step <= c.start
    assert "reg_depth" in geom_ref.FixtureCase(golden, "patch", "reg_on").keys
    for tag in ("tri", "patch"):
        c = geom_ref.FixtureCase(golden, tag, "nan")
        assert int(torch.isnan(c.depth).sum()) == 1 and all(c.loss64[k] == 0.0 for k in c.expected_keys())
        assert not c.grad64.any()
        c = geom_ref.FixtureCase(golden, tag, "empty")
        assert c.keys == ["depth", "norm", "rgb", "total"] and c.loss64["depth"] == 0.0 and c.loss64["norm"] == 0.0
        assert c.expected_keys() == {"depth", "norm_D_L1", "norm_D_dot"}


@pytest.mark.parametrize("tag", ["tri", "patch"])
@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(golden, tag, name):
    """Same float64 expressions: the terms to 1e-13 relative, d sum / d depth to 1e-11 (rel. L2)."""
    c = geom_ref.FixtureCase(golden, tag, name, torch.float64)
    terms, grad = c.restated()
    assert set(terms) == c.expected_keys()
    for k, (loss, _scale, _addends) in terms.items():
        want = c.loss64["norm" if k not in c.loss64 else k]
        assert abs(float(loss.detach()) - want) <= 1e-13 * abs(want), (k, float(loss.detach()), want)
    want = torch.from_numpy(c.grad64)
    if not c.grad64.any():
        assert not grad.any() and bool(torch.isfinite(grad).all())
    else:
        assert float((grad - want).norm() / want.norm()) < 1e-11
