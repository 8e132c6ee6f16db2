"""The host restatement of the semantic metrics (tests/sem_metrics_ref.py) against a worked case and
torch's argmax rule, the sixth ABI header, and the host side of the new arguments.  No GPU."""
import math
import os
import re

import pytest
import torch

import sem_metrics_ref as S
from ncnerf_amd import _lib
from ncnerf_amd import metrics as NM
from test_abi import NAMES as ALL_NAMES, altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ncnerf_sem.h"
NAMES = ALL_NAMES[HEADER]
NAN, INF = float("nan"), float("inf")
ARGMAX_ROWS = [([1, 3, 3, 2], 1), ([NAN, 5, NAN, 1], 0), ([-INF] * 4, 0), ([2, NAN, 9, NAN], 1), ([INF, INF, 0, NAN], 3)]


def test_worked_case():
    """Class 1 is absent from the ground truth but predicted once: its IoU is 0, not NaN, and it is
    left out of miou_valid_cls and cls_avg_acc."""
    got = S.compute(torch.tensor([[2, 1, 0], [0, 0, 0], [1, 0, 3]]))
    assert got["ious"] == [0.5, 0.0, 0.75]
    assert abs(got["miou"] - 1.25 / 3) < 1e-6 and got["miou_valid_cls"] == 0.625
    assert abs(got["total_acc"] - 5 / 7) < 1e-6 and abs(got["cls_avg_acc"] - (2 / 3 + 3 / 4) / 2) < 1e-6


def test_empty_matrix_is_nan_everywhere():
    got = S.compute(torch.zeros(3, 3, dtype=torch.int64))
    assert all(math.isnan(got[k]) for k in S.KEYS) and all(math.isnan(v) for v in got["ious"])


def test_argmax_rule():
    """A NaN beats every number (+inf too), the first NaN wins, otherwise the first maximum."""
    for row, want in ARGMAX_ROWS:
        assert torch.argmax(torch.tensor([row], dtype=torch.float32), dim=1).item() == want, row


def test_update_is_the_confusion_matrix():
    logits = torch.tensor([[0.0, 1, 0], [2, 0, 0], [0, 0, 3], [0, 5, 0], [1, 0, 0], [0, 0, 1]])
    target = torch.tensor([1, 0, 2, -1, 7, -5])  # one void, two out of range
    conf, counted, out, pred = S.update(torch.zeros(3, 3, dtype=torch.int64), logits, target)
    assert pred.tolist() == [1, 0, 2, 1, 0, 2] and (counted, out) == (3, 2)
    assert conf.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    conf, counted, _, _ = S.update(conf, logits[:2], torch.tensor([2, 2]))  # rows the target, columns the prediction
    assert conf.tolist() == [[1, 0, 0], [0, 1, 0], [1, 1, 1]] and counted == 2
    same, counted, _, _ = S.update(conf, logits, torch.full((6,), -1))
    assert torch.equal(same, conf) and counted == 0


# ---------------------------------------------------------------- the sixth header
def test_sem_header_parses_into_its_own_table():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    sixth = _lib.parse_header(_lib.read_header(HEADER))
    assert set(_lib.symbols(HEADER)) == NAMES == set(sixth)
    P, I64, I32 = _lib.P, _lib.I64, _lib.I32
    assert _lib.SIGNATURES["ncn_sem_confusion"] == [P, I64, P, I32, I32, I64, I32, P, P, P, P]
    assert _lib.SIGNATURES["ncn_sem_finalise"] == [P, I32, P, P]
    assert _lib.SIGNATURES["ncn_batch_semantics_fw"] == [P, P, I64, P, I32, I32, I64, P, P]
    conf = sixth["ncn_sem_confusion"][1]
    assert conf[0] == ("ptr", 4, "logits") and conf[2] == ("ptr", 8, "labels") and conf[7] == ("ptr", 8, "conf")
    assert conf[9] == ("ptr", 4, "pred_labels")
    assert sixth["ncn_batch_semantics_fw"][1][3] == ("ptr", 0, "plane")  # void*: uint8, int32 or int64
    assert _lib.declaration("ncn_sem_finalise") == sixth["ncn_sem_finalise"]


def test_library_exports_the_semantic_entry_points():
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is _lib.I32 and list(fn.argtypes) == _lib.SIGNATURES[name]


def test_name_clash_and_missing_header(tmp_path):
    clash = altered_headers(tmp_path, HEADER, "int ncn_select_median(const float* vals, void* stream);\n")
    with pytest.raises(_lib.NcnError, match="ncn_select_median is declared in include/ncnerf_sem.h and in "
                                            "include/ncnerf_metrics.h"):
        _lib.load_headers(clash)
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*semantic metrics"):
        _lib.load_headers(gone)


def test_refusals_precede_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda: _lib.P(0x5EED))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was entered"))
    d = _lib.P(16)
    with pytest.raises(TypeError, match=r"ncn_sem_confusion: argument 0 \(logits\).*CUDA.*cpu tensor"):
        _lib.call("ncn_sem_confusion", torch.zeros(4, 3), 3, d, -1, -1, 4, 3, d, d, None)
    with pytest.raises(TypeError, match=r"ncn_sem_confusion: argument 2 \(labels\).*8-byte"):
        _lib.call("ncn_sem_confusion", d, 3, torch.zeros(4, dtype=torch.int32), -1, -1, 4, 3, d, d, None)
    with pytest.raises(TypeError, match=r"ncn_sem_confusion: argument 6 \(n_cls\)"):
        _lib.call("ncn_sem_confusion", d, 3, d, -1, -1, 4, 3.0, d, d, None)
    with pytest.raises(TypeError, match=r"ncn_batch_semantics_fw: argument 3 \(plane\).*CUDA.*cpu tensor"):
        _lib.call("ncn_batch_semantics_fw", d, d, 4, torch.zeros(1, 4, dtype=torch.uint8), 1, 1, 4, d)


# ---------------------------------------------------------------- the Python surface, host side
ROWS = [[20.0, 0.9, 0.8, 0.7, 1.0, 0.5, 1, 10.0, 8.0, 6.0, 4.0, 1],
        [30.0, 0.7, 0.6, 0.5, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0]]


def test_logs_from_rows_old_arguments_old_keys():
    assert NM.COLUMNS[7:] == NM.NN_COLUMNS and len(NM.COLUMNS) == 12
    old = NM.logs_from_rows(ROWS, True, True)
    assert list(old) == ["rgb/psnr", "rbg/ssim", "rbg/ssim_n", "rbg/ssim_n_sck", "depth/rmse", "depth/abs",
                         "norm_depth/ang_err_mean", "norm_depth/ang_err_median", "norm_depth/ang_err_mean_min",
                         "norm_depth/ang_err_median_min"]
    assert set(NM.logs_from_rows(ROWS, False, False)) == {"rgb/psnr", "rbg/ssim", "rbg/ssim_n", "rbg/ssim_n_sck"}
    nn_rows = [[12.0, 9.0, 7.0, 5.0, 1], [0.0, 0.0, 0.0, 0.0, 0]]
    sem = [0.4, 0.6, 0.7, 0.65, 0.5, 0.0, 0.75]
    new = NM.logs_from_rows(ROWS, True, True, nn_rows=nn_rows, sem=sem)
    assert {k: v for k, v in new.items() if k in old} == old
    assert set(new) - set(old) == {"norm_nn/ang_err_mean", "norm_nn/ang_err_median", "norm_nn/ang_err_mean_min",
                                   "norm_nn/ang_err_median_min", "sem/miou", "sem/miou_valid_cls", "sem/total_acc",
                                   "sem/cls_avg_acc"}
    assert new["norm_nn/ang_err_mean"] == 12.0 and new["norm_nn/ang_err_median_min"] == 5.0  # one view counted
    assert [new[f"sem/{k}"] for k in S.KEYS] == sem[:4] and NM.SEM_KEYS == S.KEYS
    none = NM.logs_from_rows(ROWS[1:], False, False, nn_rows=nn_rows[1:])
    assert math.isnan(none["norm_nn/ang_err_mean"])  # 0 / 0, as the depth tag


def test_host_tensors_and_bad_arguments_are_refused():
    sm = NM.SemanticMetrics(3)
    assert sm.n_classes == 3 and sm.ignore_label == -1
    with pytest.raises(RuntimeError, match="CUDA"):
        sm.update(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no update yet"):
        sm.compute()
    for k in (0, 65, 3.0, None):
        with pytest.raises(ValueError, match="1..64"):
            NM.SemanticMetrics(k)
    with pytest.raises(ValueError, match="n_sem_cls"):
        NM.ViewMetrics(eval_sem=True)
    vm = NM.ViewMetrics(norm_gt=False, pred_norm_nn=True)
    assert not vm.pred_norm_nn  # the reference's condition: pred_norm_nn and load_norm_gt
    vm = NM.ViewMetrics()
    assert (vm.eval_depth, vm.norm_gt, vm.pred_norm_nn, vm.eval_sem, vm.sem) == (False, False, False, False, None)
    assert NM.sem_dict([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]) == {"miou": 0.1, "miou_valid_cls": 0.2, "total_acc": 0.3,
                                                          "cls_avg_acc": 0.4, "ious": [0.5, 0.6]}


def test_dataset_checks_the_semantics_plane_on_the_host():
    from ncnerf_amd.data import LABEL_PLANES, DeviceRayDataset
    assert LABEL_PLANES == ("depth", "normals", "normals_depth")
    V, H, W = 2, 8, 8
    images, poses, dirs = torch.zeros(V, H * W, 3), torch.zeros(V, 3, 4), torch.zeros(H * W, 3)
    kw = dict(batch_size=64, patch_size=8)
    with pytest.raises(RuntimeError, match="semantics must be torch.uint8, torch.int32 or torch.int64"):
        DeviceRayDataset(images, poses, dirs, (W, H), semantics=torch.zeros(V, H * W), **kw)
    with pytest.raises(ValueError, match="semantics must be"):
        DeviceRayDataset(images, poses, dirs, (W, H), semantics=torch.zeros(V, H * W + 1, dtype=torch.uint8), **kw)
    with pytest.raises(RuntimeError, match="semantics must be a CUDA tensor"):
        DeviceRayDataset(images, poses, dirs, (W, H), semantics=[1, 2], **kw)
