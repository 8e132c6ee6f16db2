"""Per-level comparison helpers of the field backward (tests/test_oracle_field_levels.py on the CPU,
tests/test_gpu_field_levels.py and tests/test_gpu_field.py on the GPU) and the edge set of positions
at and around the faces of the scene box.

Outlier rule for the encoding gradient dL/denc (N, 32, level-major pairs): an element of level l is
an outlier when |got - ref| > 8 u |ref| + 0.08 u rms_l, u the unit roundoff of the MLP operand type
(2^-11 fp16, 2^-8 bf16) and rms_l the RMS of ref on that level; a level's outlier share is the
fraction of its 2 N elements that are outliers.  The element's own term allows a few roundings of
the stored value (dE leaves the MLP pass in the operand type), the level's term covers elements
that cancel to far below the level's size, whose absolute error is set by their addends.  A
systematic error on a level (a scaling by 1 % in fp16, 5 % in bf16: bf16's window 8 u is 3.1 %)
puts more than half of the level outside (test_oracle_field_levels.py)."""
import numpy as np

U_ROUND = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
N_LEVELS = 16


def outlier_mask(got, ref, precision):
    """(N, 32) bool: the outliers of got against ref (float64 arithmetic)."""
    got = np.asarray(got, np.float64).reshape(-1, N_LEVELS, 2)
    ref = np.asarray(ref, np.float64).reshape(-1, N_LEVELS, 2)
    u = U_ROUND[precision]
    rms = np.sqrt((ref ** 2).mean(axis=(0, 2)))  # per level
    bad = np.abs(got - ref) > 8 * u * np.abs(ref) + 0.08 * u * rms[None, :, None]
    return bad.reshape(-1, 2 * N_LEVELS)


def outlier_share(got, ref, precision):
    """Per level: the fraction of the level's elements that are outliers (16 floats)."""
    return outlier_mask(got, ref, precision).reshape(-1, N_LEVELS, 2).mean(axis=(0, 2))


def table_level_errors(got, ref, levels):
    """The table gradient (n_entries, 2) split by level: [(rel-L2, rows the reference gives a
    gradient and `got` leaves zero, rows the reference gives a gradient)] per level."""
    got = np.asarray(got, np.float64).reshape(-1, 2)
    ref = np.asarray(ref, np.float64).reshape(-1, 2)
    out = []
    for lv in levels:
        a, b = got[lv["offset"]:lv["offset"] + lv["params"]], ref[lv["offset"]:lv["offset"] + lv["params"]]
        nz = np.any(b != 0, axis=1)
        lost = nz & ~np.any(a != 0, axis=1)
        out.append((float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)), int(lost.sum()), int(nz.sum())))
    return out


TILE_SKIP = 1e-3  # a 16-row tile whose reference norm is below this share of its matrix's norm is not judged
MAX_SKIPPED_TILES = 2


def weight_tile_errors(got, ref):
    """A weight gradient (rows, cols) by 16-row tile: (rel-L2 per judged tile {tile: rel}, skipped
    tiles [tile]).  A tile whose reference norm is below TILE_SKIP of the matrix's is skipped (its
    relative error says nothing: W5's padded rows 3..15 share tile 0 with the live rows, so no tile
    of the model's matrices is empty by construction)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and ref.shape[0] % 16 == 0
    whole = np.linalg.norm(ref)
    errs, skipped = {}, []
    for t in range(ref.shape[0] // 16):
        a, b = got[16 * t:16 * t + 16], ref[16 * t:16 * t + 16]
        nb = np.linalg.norm(b)
        if nb < TILE_SKIP * whole:
            skipped.append(t)
        else:
            errs[t] = float(np.linalg.norm(a - b) / nb)
    return errs, skipped


# ---- the edge set E: positions at, just inside, just outside and well outside the faces of the
# world box [-scale, scale]^3 (scale 0.5: x01 = x + 0.5), on cell boundaries of three levels, and
# maximal runs (one position repeated).  The in-box constants below are those of the unit box,
# multiplied by the box's width 2 * scale (1.0, exactly, at the default) ----
REPEAT = 600


def _f32(v):
    return np.float32(v)


def edge_points(levels, scale=0.5):
    """(special points (k, 3) f32, the repeated interior point (3,), the repeated face point (3,)),
    world coordinates of the box [-scale, scale]^3 (`levels`: that scale's level table)."""
    w = 2.0 * scale  # the box's width: 1.0 at scale 0.5, so every product below is the constant itself
    lo, hi = _f32(-scale), _f32(scale)
    pts = []
    for cx in (lo, hi):  # the 8 corners, exactly
        for cy in (lo, hi):
            for cz in (lo, hi):
                pts.append((cx, cy, cz))
    inner = (_f32(0.13 * w), _f32(-0.21 * w))  # the in-face coordinates of the off-centre face points
    for axis in range(3):
        for side, face in ((-1.0, lo), (1.0, hi)):
            def put(v, others=(_f32(0.0), _f32(0.0))):
                p = [None, None, None]
                p[axis] = _f32(v)
                p[(axis + 1) % 3], p[(axis + 2) % 3] = others
                pts.append(tuple(p))
            put(face)  # the face centre, exactly
            put(np.nextafter(face, _f32(0.0)), inner)  # one ulp inside
            put(np.nextafter(face, _f32(2.0 * side * w)), inner)  # one ulp outside
            put(_f32(side * 0.7 * w), inner)  # 0.1 outside: x01 = -0.2 / 1.2
            put(_f32(side * 0.7 * w), (_f32(side * 0.62 * w), _f32(side * 0.58 * w)))  # all three outside (low side: every floor < 0)
            put(_f32(side * 0.7 * w), (_f32(-side * 0.62 * w), _f32(side * 0.58 * w)))  # outside on both sides at once
    # cell boundaries of levels 0, 5 and 10 (pos = scale x01 + 0.5 crosses an integer at
    # x01 = (k - 0.5) / scale): the floats just below and just above, on one axis and on all three
    for l in (0, 5, 10):
        s = float(np.float32(levels[l]["scale"]))
        res = levels[l]["res"]
        for k in (1, res // 2, res - 1):
            exact = ((k - 0.5) / s - 0.5) * w  # world
            w0 = _f32(exact)
            below = w0 if float(w0) <= exact else np.nextafter(w0, _f32(-w))
            above = np.nextafter(below, _f32(w))
            for v in (below, above):
                pts.append((v, _f32(0.05 * w), _f32(-0.3 * w)))
            pts.append((below, above, below))
    spec = np.array(pts, dtype=np.float32)
    rep_in = np.array([0.2113 * w, -0.0371 * w, 0.3307 * w], dtype=np.float32)
    rep_face = np.array([-0.5 * w, 0.17 * w, -0.08 * w], dtype=np.float32)  # x01 == 0 on x
    return spec, rep_in, rep_face


def place_edges(fill, levels, scale=0.5):
    """fill (n, 3) f32 world positions -> a copy with the edge set (edge_points(levels, scale): the
    box [-scale, scale]^3 and its level table) at the start of the array
    ([special, interior x 600, face x 600]), across index 4096 ([interior x 600, special, face x 600],
    the special points straddling 4096) and at the tail ([face x 600, special], as far as it does
    not overlap the block before), and the indices that hold an edge point."""
    x = np.array(fill, dtype=np.float32, copy=True)
    n = x.shape[0]
    spec, rep_in, rep_face = edge_points(levels, scale)
    r_in, r_face = np.tile(rep_in, (REPEAT, 1)), np.tile(rep_face, (REPEAT, 1))
    mark = np.zeros(n, bool)

    def put(at, block):
        at = max(at, 0)
        k = min(len(block), n - at)
        if k > 0:
            x[at:at + k] = block[:k]
            mark[at:at + k] = True
        return at + max(k, 0)

    end = put(0, np.concatenate([spec, r_in, r_face]))
    at = 4096 - REPEAT - len(spec) // 2
    if at >= end:
        end = put(at, np.concatenate([r_in, spec, r_face]))
    tail = np.concatenate([r_face, spec])
    k = min(len(tail), n - end)
    if k > 0:
        put(n - k, tail[len(tail) - k:])
    return x, mark
