"""The host restatement of the validation metrics (tests/metrics_ref.py) against closed forms and
against itself, and the second ABI header.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as M
from ncnerf_amd import _lib
from test_abi import NAMES as ALL_NAMES, altered_headers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ncnerf_metrics.h"
NAMES = ALL_NAMES[HEADER]
BOUND0 = 2.0 ** -20


def test_identical_images_give_one():
    _, gt = M.noise_case(13, 17)
    for form in (M.ssims_f64, M.ssims_torch32, M.ssim_separable32):
        for m, mean in form(gt, gt, 13, 17):
            assert abs(float(mean) - 1.0) <= 1e-6 and np.abs(np.asarray(m, np.float64) - 1.0).max() <= 1e-5


def test_constant_images_closed_form():
    """sigma = 0, so S = (2ab + c1) / (a^2 + b^2 + c1): exactly for the box window; for the Gaussian
    one up to (a - b)^2 eps / c2, because its float32 weights sum to 1 + eps (|eps| ~ 1e-7)."""
    h, w, a, b = 12, 15, 0.75, 0.5
    pred = np.full((h * w, 3), a, np.float32)
    gt = np.full((h * w, 3), b, np.float32)
    gt[0, 0] = pred[0, 0] = 0.25  # one pixel sets the data range of ssim_n and ssim_n_sck: R = 0.25
    R = M.data_range(gt)
    assert R == 0.25
    res = M.ssims_f64(pred, gt, h, w)
    for (m, _), r, rad in zip(res, (1.0, R, R), (5, 5, 3)):
        c1 = (0.01 * r) ** 2
        inner = m[1:, 1:] if rad == 5 else m[4:, 4:]  # the windows that do not hold pixel (0, 0)
        np.testing.assert_allclose(inner, (2 * a * b + c1) / (a * a + b * b + c1), rtol=0, atol=2e-4 if rad == 5 else 1e-12)
    # the Gaussian taps are float32 and sum to 1 + eps: with eps accounted for, the form is exact
    eps = float(M.window32().double().sum()) - 1.0
    c1, c2 = 1e-4, 9e-4
    mp, mt = a * (1 + eps), b * (1 + eps)
    vp, vt, vpt = a * a * (1 + eps) - mp * mp, b * b * (1 + eps) - mt * mt, a * b * (1 + eps) - mp * mt
    exact = ((2 * mp * mt + c1) * (2 * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    np.testing.assert_allclose(res[0][0][1:, 1:], exact, rtol=0, atol=1e-12)


def test_one_box_window_hand_formula():
    pred, gt = M.noise_case(7, 7, seed=3)
    R = M.data_range(gt)
    m, mean = M.ssim_box_f64(pred, gt, 7, 7, R)
    assert m.shape == (1, 1, 3)
    p, t = pred.astype(np.float64).reshape(49, 3), gt.astype(np.float64).reshape(49, 3)
    mp, mt = p.mean(0), t.mean(0)
    vp = (49 / 48) * ((p * p).mean(0) - mp * mp)
    vt = (49 / 48) * ((t * t).mean(0) - mt * mt)
    vpt = (49 / 48) * ((p * t).mean(0) - mp * mt)
    np.testing.assert_allclose(vp, p.var(0, ddof=1), rtol=1e-12)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    hand = ((2 * mp * mt + c1) * (2 * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    np.testing.assert_allclose(m[0, 0], hand, rtol=1e-12)
    assert abs(mean - hand.mean()) <= 1e-14


@pytest.mark.parametrize("case", ["noise", "flat"])
@pytest.mark.parametrize("hw", [(11, 11), (12, 29), (37, 53), (70, 131)])
def test_float32_forms_agree_with_float64(case, hw):
    """The dense float32 torch form is the yardstick E; the separable, centred float32 form (the
    kernel's arithmetic) is held to the criterion of the GPU tests: 4 E + 2^-20."""
    h, w = hw
    pred, gt = (M.noise_case if case == "noise" else M.flat_case)(h, w)
    ref, t32, sep = M.ssims_f64(pred, gt, h, w), M.ssims_torch32(pred, gt, h, w), M.ssim_separable32(pred, gt, h, w)
    for k, name in enumerate(("ssim", "ssim_n", "ssim_n_sck")):
        E = np.abs(t32[k][0].double().numpy() - ref[k][0]).max()
        Em = abs(float(t32[k][1]) - ref[k][1])
        G = np.abs(sep[k][0].astype(np.float64) - ref[k][0]).max()
        Gm = abs(sep[k][1] - ref[k][1])
        print(f"{case} {h}x{w} {name}: torch32 map {E:.2e} mean {Em:.2e}; separable32 map {G:.2e} mean {Gm:.2e}")
        assert E <= (1e-5 if case == "noise" else 1e-2), "the dense float32 form left the definition"
        assert G <= 4 * E + BOUND0 and Gm <= 4 * Em + BOUND0


def test_small_image_raises():
    pred, gt = M.noise_case(10, 12)
    for form in (M.ssims_f64, M.ssims_torch32, M.ssim_separable32):
        with pytest.raises(ValueError):
            form(pred, gt, 10, 12)


def test_median_is_the_lower_middle():
    assert M.median_lower([3, 1, 2, 4]) == 2
    assert M.median_lower([3.0, 1.0, 2.0]) == 2.0 and M.median_lower([5.0]) == 5.0
    x = np.random.default_rng(0).random(1000).astype(np.float32)
    assert M.median_lower(x) == torch.median(torch.from_numpy(x)).item()
    assert M.median_lower(x) == torch.kthvalue(torch.from_numpy(x), (1000 - 1) // 2 + 1).values.item()


def test_angles():
    gt = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 2, 0]], np.float32)
    pred = np.array([[0, 0, 0], [0, 0, -3], [0, 1, 1], [1, 0, 0], [0, 1, 0]], np.float32)
    valid, a, m = M.angles_f64(pred, gt)
    assert valid.tolist() == [True, True, True, False, True]
    # (the 1e-8 in x / (|x| + 1e-8) keeps parallel unit vectors' dot product just below 1, where
    # acos is steep: 0.0099 degrees instead of 0)
    assert a[0] == 90.0 and m[0] == 90.0  # a zero predicted normal: exactly 90 degrees
    np.testing.assert_allclose(a, [90.0, 180.0, 45.0, 0.0], atol=0.02)
    np.testing.assert_allclose(m, [90.0, 0.0, 45.0, 0.0], atol=0.02)
    a32, m32 = M.angles_torch32(pred, gt)
    np.testing.assert_allclose(a32.numpy(), a, atol=0.05)
    np.testing.assert_allclose(m32.numpy(), m, atol=0.05)
    mean, med, mean_min, med_min, counted = M.normals_f64(pred, gt)
    assert counted == 1 and abs(med - 45.0) < 1e-5 and abs(med_min - 0.0) < 0.02  # lower middle of 4
    assert abs(mean - 78.75) < 0.01
    # one NaN prediction on a valid pixel: four NaNs, still counted; no valid pixel: not counted
    bad = pred.copy()
    bad[2, 1] = np.nan
    row = M.normals_f64(bad, gt)
    assert all(math.isnan(v) for v in row[:4]) and row[4] == 1
    t32 = M.normals_torch32(bad, gt)
    assert all(math.isnan(float(v)) for v in t32)
    bad = pred.copy()
    bad[3, 0] = np.nan  # on an invalid pixel: ignored
    assert M.normals_f64(bad, gt) == M.normals_f64(pred, gt)
    assert M.normals_f64(pred, np.zeros_like(gt)) == (0.0, 0.0, 0.0, 0.0, 0)


def test_depth_rules():
    gt = np.array([2.0, 0.0, -1.0, np.nan, 4.0], np.float32)
    pred = np.array([1.0, 9.0, 9.0, 9.0, 7.0], np.float32)
    rmse, ab, counted = M.depth_f64(pred, gt)
    assert counted == 1 and abs(rmse - math.sqrt((1 + 9) / 2)) < 1e-12 and abs(ab - 2.0) < 1e-12
    r32, a32 = M.depth_torch32(pred, gt)
    assert abs(float(r32) - rmse) < 1e-6 and abs(float(a32) - ab) < 1e-6
    assert M.depth_f64(pred, np.array([0.0, -1.0, np.nan, 0.0, 0.0], np.float32)) == (0.0, 0.0, 0)


def test_compute_counts_only_the_views_that_counted():
    rows = [[20.0, 0.9, 0.8, 0.7, 1.0, 0.5, 1, 10.0, 8.0, 6.0, 4.0, 1],
            [30.0, 0.7, 0.6, 0.5, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0],
            [40.0, 0.5, 0.4, 0.3, 3.0, 1.5, 1, 0.0, 0.0, 0.0, 0.0, 0]]
    logs = M.compute_from_rows(rows, True, True)
    assert logs["rgb/psnr"] == 30.0 and abs(logs["rbg/ssim"] - 0.7) < 1e-12
    assert logs["depth/rmse"] == 2.0 and logs["depth/abs"] == 1.0
    assert logs["norm_depth/ang_err_mean"] == 10.0 and logs["norm_depth/ang_err_median_min"] == 4.0
    assert set(M.compute_from_rows(rows, False, False)) == {"rgb/psnr", "rbg/ssim", "rbg/ssim_n", "rbg/ssim_n_sck"}
    none = M.compute_from_rows([rows[1]], True, True)
    assert math.isnan(none["depth/rmse"]) and math.isnan(none["norm_depth/ang_err_mean"]) and none["rgb/psnr"] == 30.0
    # the package's own averaging is the same function of the rows
    from ncnerf_amd.metrics import COLUMNS, logs_from_rows
    assert COLUMNS == M.COLUMNS
    for r in (rows, [rows[1]], [rows[0], [float("nan")] * 4 + rows[0][4:7] + [float("nan")] * 4 + [1]]):
        a, b = logs_from_rows(r, True, True), M.compute_from_rows(r, True, True)
        assert set(a) == set(b)
        for k in a:
            assert (math.isnan(a[k]) and math.isnan(b[k])) or abs(a[k] - b[k]) < 1e-12, k


# ---------------------------------------------------------------- the second header
def test_metrics_header_parses_into_the_one_table():
    """(what every header shares, its names among it, is in test_abi.py)"""
    assert _lib.header_path(HEADER) == os.path.join(ROOT, "include", HEADER)
    assert set(_lib.symbols(HEADER)) == NAMES
    P, I64, I32 = _lib.P, _lib.I64, _lib.I32
    assert _lib.SIGNATURES["ncn_select_median"] == [P, I64, I32, P, P, I64, P, P]
    assert _lib.ABI["ncn_metrics_ssim"][1][5] == ("ptr", 8, "ws")


def test_header_taps_are_torchs_float32_taps():
    """NCN_SSIM_TAPS, bit for bit the restatement's taps (the window's weight sum depends on them)."""
    text = _lib.read_header(HEADER)
    body = re.search(r"^#define NCN_SSIM_TAPS \{([^}]*)\}$", text, flags=re.M).group(1)
    taps = np.array([float.fromhex(t.strip().rstrip("f")) for t in body.split(",")])
    g = M.gaussian_taps32().numpy()
    assert taps.shape == (6,) and np.array_equal(taps.astype(np.float32), g[5:]) and np.array_equal(taps, g[5:].astype(np.float64))
    assert np.array_equal(g[:5], g[:5:-1])
    assert abs(float(M.window32().double().sum()) - 1.0 + 9.3e-8) < 1e-9


def test_library_exports_the_metric_entry_points():
    L = _lib.lib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is _lib.I32 and list(fn.argtypes) == _lib.SIGNATURES[name]


def test_missing_metrics_header_names_the_path(tmp_path):
    gone = altered_headers(tmp_path, HEADER)
    with pytest.raises(_lib.NcnError, match=re.escape(os.path.join(gone, HEADER)) + ".*validation metrics"):
        _lib.load_headers(gone)


def test_metric_calls_are_marshalled_like_the_others():
    """Refused before anything is launched: a CPU tensor, a tensor of the wrong width, a float for n."""
    f32, f64, i64 = torch.zeros(4), torch.zeros(4, dtype=torch.float64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(TypeError, match=r"ncn_select_median: argument 0 \(vals\).*CUDA.*cpu tensor"):
        _lib.call("ncn_select_median", f32, 4, 1, i64, torch.zeros(5120, dtype=torch.int32), 5120, f32)
    with pytest.raises(TypeError, match=r"ncn_metrics_ssim: argument 2 \(H\)"):
        _lib.marshal("ncn_metrics_ssim", (_lib.P(16), _lib.P(16), 11.0, 11, _lib.P(16), _lib.P(16), 3, None, _lib.P(16),
                                          _lib.P(0)))
    with pytest.raises(TypeError, match=r"ncn_metrics_angles: argument 4 \(ws\)"):
        _lib.marshal("ncn_metrics_angles", (_lib.P(16), _lib.P(16), 4, _lib.P(16), f32, 4, f64, i64, _lib.P(0)))


def test_view_metrics_refuses_host_tensors():
    from ncnerf_amd.metrics import ViewMetrics, select_median, ssim_view
    pred, gt = (torch.from_numpy(x) for x in M.noise_case(11, 11))
    with pytest.raises(RuntimeError, match="CUDA"):
        ViewMetrics().update({"rgb": pred}, {"rgb": gt}, 11, 11)
    with pytest.raises(RuntimeError, match="CUDA"):
        ssim_view(pred, gt, 11, 11)
    with pytest.raises(RuntimeError, match="CUDA"):
        select_median(torch.zeros(4), torch.ones(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="11x11"):
        ViewMetrics().update({"rgb": pred}, {"rgb": gt}, 10, 12)
