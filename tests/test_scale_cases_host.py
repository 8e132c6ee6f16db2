"""Scene scales above 0.5 on the host: the level table at every scale, and the input conditions of
the GPU cases at scales 1.0 / 1.5 / 16.0 (tests/scale_cases.py), asserted on the oracle alone — what
each GPU case is there for is verified here without a GPU, so a change to the level rule, to a
case's rays or to its positions cannot silently empty it.

Measured (this file's prints): scale-16 positions in a level-9 cell with pz >= 1023: 47.8 % (bound
5 %); samples per mip of the 2048-ray marcher cases: c2_const 101 k / 252 k, c3_const 78 k / 202 k /
274 k, c3_exp 10 k / 27 k / 43 k, of which 12.6 k have their mip from dt; test marcher, esf 1/64:
2378 (C = 2) / 1625 (C = 3) samples at the upper clamp."""
import numpy as np
import pytest

from oracle import field_ref
from ncnerf_amd.ngp_mt import NGPMT, grid_levels
import scale_cases as sc

ALL_SCALES = (0.25, 0.5, 1.0, 1.5, 2.0, 4.0, 8.0, 16.0)


@pytest.mark.parametrize("scale", ALL_SCALES)
def test_level_table_matches_oracle_at_scale(scale):
    lv, n = grid_levels(scale)
    lo, no = field_ref.grid_levels(scale)
    assert n == no and len(lv) == len(lo) == 16
    for a, b in zip(lv, lo):
        assert np.float32(a["scale"]).tobytes() == np.float32(b["scale"]).tobytes()  # the scale's bits
        assert (a["res"], a["params"], a["offset"]) == (b["res"], b["params"], b["offset"])
    assert lv[-1]["offset"] + lv[-1]["params"] == n


def test_level_table_facts_the_gpu_cases_rely_on():
    assert {s: field_ref.grid_levels(s)[1] for s in (0.5, 1.0, 16.0)} == {0.5: 5722520, 1.0: 6098120, 16.0: 6811592}
    l05, l1, l16 = (field_ref.grid_levels(s)[0] for s in (0.5, 1.0, 16.0))
    # scale 0.5: the scatter's unit class 0 (levels 0-5) is exactly the dense levels
    assert [lv["hashed"] for lv in l05] == [False] * 6 + [True] * 10
    # scale 1.0: level 5 is hashed inside class 0
    assert l1[5]["res"] == 81 and l1[5]["hashed"] and not l1[4]["hashed"]
    # scale 16: level 9 is beyond the scatter's cell key range (pz < 1023), the finest res is 32768
    assert l16[9]["res"] == 1553 and l16[9]["res"] > 1024 and l16[8]["res"] <= 1024
    assert l16[15]["res"] == 32768
    for s, C in sc.CASCADES.items():  # (ngp_mt.py:34; no device needed to build the model)
        m = NGPMT(scale=s, grid_size=8)
        assert m.cascades == C and m._xyz_extent == 2 * s and m._n_table == 2 * field_ref.grid_levels(s)[1]
    ext = np.float32(3.0)  # scale 1.5: the extent is not a power of two (the scatter's dividing branch)
    assert (ext.view(np.uint32) & 0x807FFFFF) != 0
    for s in (1.0, 16.0):
        assert (np.float32(2 * s).view(np.uint32) & 0x807FFFFF) == 0


@pytest.mark.parametrize("scale", sorted(sc.CASCADES))
def test_field_positions_hold_the_edges(scale):
    xw = sc.field_positions(scale)
    assert xw.shape == (sc.N_FIELD, 3) and xw.dtype == np.float32
    x01 = sc.x01_f32(xw, scale)
    assert (x01 == 0).any() and (x01 == 1).any() and (x01 < 0).any() and (x01 > 1).any()
    assert (np.abs(xw) == np.float32(scale)).all(axis=1).sum() >= 8  # the corners
    inside = ((x01 >= 0) & (x01 <= 1)).all(axis=1)
    assert inside.mean() > 0.95
    for l in (0, 5, 10):  # cell-boundary pairs: neighbouring cells of the level
        lv = field_ref.grid_levels(scale)[0][l]
        pos = np.float32(lv["scale"]) * x01[:, 0] + np.float32(0.5)
        assert (np.abs(pos - np.round(pos)) < 2e-3 * max(1.0, lv["scale"] / 256)).sum() >= 6


def test_scale16_positions_leave_the_cell_key_range():
    cells = sc.level_cells(sc.field_positions(16.0), 16.0, 9)
    x01 = sc.x01_f32(sc.field_positions(16.0), 16.0)
    inside = ((x01 >= 0) & (x01 <= 1)).all(axis=1)
    share = float(((cells[:, 2] >= 1023) & inside).mean())
    print(f"scale 16: samples in a level-9 cell with pz >= 1023: {100 * share:.1f} %")
    assert share >= 0.05
    fill = cells[~_edge_mark(16.0)]  # the uniform part alone: in-box cells, not fabricated positions
    assert float((fill[:, 2] >= 1023).mean()) >= 0.05
    cells15 = sc.level_cells(sc.field_positions(16.0), 16.0, 15)
    assert cells15.max() >= 1 << 14  # 15 integer bits of the f32 position


def _edge_mark(scale):
    from field_level_check import place_edges
    return place_edges(np.zeros((sc.N_FIELD, 3), np.float32), field_ref.grid_levels(scale)[0], scale)[1]


@pytest.mark.parametrize("name", sorted(sc.TRAIN_CASES))
@pytest.mark.parametrize("n", [n for n in sc.TRAIN_N if n > 1])
def test_train_marcher_cases_reach_every_mip(name, n):
    case = sc.train_case(name, n)
    C = case["C"]
    rays_a, xyzs, dirs, deltas, ts, counter = case["ref"]
    S = int(counter[0])
    assert S == xyzs.shape[0] > 20 * n
    mp = sc.mip_from_pos(xyzs, C)
    per_mip = np.bincount(mp, minlength=C)
    md = sc.mip_from_dt(deltas, C)
    by_dt = int((md > mp).sum())
    print(f"{name} n {n}: C {C}, {S} samples, per mip (from xyzs) {per_mip.tolist()}, mip decided by dt: {by_dt}")
    assert (per_mip >= 50).all(), per_mip
    assert (rays_a[:, 2] == 0).any() and (rays_a[:, 2] > 256).any()  # misses, and rays on the long path
    if case["esf"] > 0:
        assert by_dt >= 1
    else:
        assert by_dt == 0  # constant dt = sqrt(3) / max_samples: mip_from_dt is 0


def test_single_ray_cases_have_samples():
    for name in sc.TRAIN_CASES:
        assert int(sc.train_case(name, 1)["ref"][5][0]) > 0


@pytest.mark.parametrize("scale", sc.TEST_SCALES)
@pytest.mark.parametrize("esf", sc.TEST_ESF)
def test_test_marcher_cases(scale, esf):
    case = sc.eval_march_case(scale, esf)
    C = case["C"]
    hi_test, hi_train = sc.dt_clamp(C), sc.dt_clamp(scale)
    assert hi_test > hi_train
    xyz = np.concatenate([r[0][0].reshape(-1, 3) for r in case["refs"]])
    dt = np.concatenate([r[0][2].reshape(-1) for r in case["refs"]])
    valid = dt > 0
    per_mip = np.bincount(sc.mip_from_pos(xyz[valid], C), minlength=C)
    at_clamp = int((dt == hi_test).sum())
    print(f"test marcher scale {scale} esf {esf:.5f}: samples per mip {per_mip.tolist()}, at the upper clamp {at_clamp}, "
          f"above the training clamp {int((dt > hi_train).sum())}")
    assert (per_mip >= 50).all(), per_mip
    for (out, ht_after), N in zip(case["refs"], sc.TEST_NS):
        assert out[4].max() == N  # some ray fills every slot
    assert not np.array_equal(case["refs"][0][1], case["ht0"])  # hits_t moves
    if esf == sc.QUIRK_ESF:
        # the quirk case: dt at the test marcher's clamp sqrt(3) 2 C / G, above the training clamp
        assert at_clamp >= 1 and (dt.max() == hi_test)
    if esf == 0:
        assert (dt[valid] == sc.SQRT3 / np.float32(sc.MAX_SAMPLES)).all()
