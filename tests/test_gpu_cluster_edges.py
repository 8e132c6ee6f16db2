"""The clustering kernel (cluster_kernel<K> behind ncn_cluster_loss, csrc/loss.hip) at the sizes and
corners the parity tests of test_gpu_loss.py do not reach: K = 10, n_tri > 8192 (the gather path) up
to the maximum 16384 with a workgroup's whole 1024-point chunk in one cluster, nv at the subsample
cap, nv == K and K + 1, niter in {0, 1, 30}, the three gradient rows one by one against float64, the
device schedule / weights / total and the refusals through the C ABI, and the launch-sequence wrap
of the Lloyd tags.  Reference throughout: oracle/losses_ref.py (general in K, n and niter).

Every parity case asserts from the oracle's own result that it is non-vacuous (three non-empty
selected clusters, a flipped label unless the data has none by construction).  DESIGN.md §7
"Round 10" holds the case table and the measured figures."""
import numpy as np
import pytest
import torch

from oracle import losses_ref
from ncnerf_amd import _lib
from ncnerf_amd import losses as L

pytestmark = pytest.mark.gpu

W = (2e-3, 3e-3, 5e-3)
KM_BLOCKS = 16  # the kernel's co-resident workgroups: chunk = ceil(nv / 16) consecutive ranks each
_AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
_P = np.array([0.3, 0.05, 0.25, 0.1, 0.25, 0.05])


def _normals(n, seed, noise=0.05, ordered=False, frame=None, invalid=0, scale=1.0):
    """Manhattan-style normals as in test_gpu_loss.py.  ordered: the points sorted by generating axis
    before the noise is added (the ranks of one cluster are then contiguous, as the triangles of a wall
    are in a patch-ordered batch).  frame: 3x3, its rows replace the three axes.  invalid: that many
    all-zero rows spread evenly over the whole index range (first and last row included), one of them
    a NaN row and one an Inf row instead."""
    rng = np.random.default_rng(seed)
    axes = _AXES if frame is None else (_AXES @ np.asarray(frame, np.float64)).astype(np.float32)
    g = rng.choice(6, n, p=_P)
    if ordered:
        g = np.sort(g)
    x = axes[g] + rng.normal(0, noise, (n, 3)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = (x * np.float32(scale)).astype(np.float32)
    if invalid:
        assert invalid >= 4
        idx = np.unique(np.linspace(0, n - 1, invalid).astype(np.int64))
        assert len(idx) == invalid
        x[idx] = 0.0
        x[idx[1]] = (0.5, np.nan, 0.5)
        x[idx[-2]] = (np.inf, 0.0, -np.inf)
    return x


def _degenerate_normals(n, seed):
    """test_gpu_loss._degenerate_normals: three exact directions (+ 50 noisy points), so the init
    picks repeat points and the Lloyd rounds take faiss's split walk."""
    rng = np.random.default_rng(seed)
    x = _AXES[::2][rng.choice(3, n)].astype(np.float32)
    x[:50] += rng.normal(0, 0.05, (50, 3)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def _oracle(X, K, niter, need_negative=True):
    valid = losses_ref.valid_normals_mask(torch.from_numpy(X)).numpy()
    Xv = X[valid]
    C, a = losses_ref.spherical_kmeans(Xv, K=K, niter=niter, seed=1234)
    lab, _ = losses_ref.cluster_select(C, a, 0.99)
    for k in (1, 2, 3):  # non-vacuous: the three selected clusters have members
        assert (np.abs(lab) == k).any(), f"selected cluster {k} is empty"
    if need_negative:
        assert (lab < 0).any(), "no flipped label"
    return valid, Xv, C, a, lab


def _status_clean(dev, K):
    """The sticky status word of the (dev, K) workspace is clear; a set word is cleared before the
    assertion fails so that it cannot make the launches of later tests drop their terms."""
    ws = L._WS[(str(dev), K)]
    off = int(_lib.lib().ncn_cluster_status_offset(K))
    word = int(ws.view(torch.int32)[off].item())
    if word:
        ws.view(torch.int32)[off] = 0
    assert word == 0, f"cluster status word = {word}"


# (id, K, n_tri, dict(niter, invalid, ordered, degenerate, scale, full_chunk, seed)); the data seed is
# n_tri + K unless given (k10-nv=K+1: with seed 28 the oracle's second selected cluster is empty)
_CASES = [
    ("k10-2000", 10, 2000, {}), ("k10-6272", 10, 6272, {}),
    # nv exactly at / one past the subsample cap K * 256, directly and through compaction
    ("k10-cap", 10, 2560, {}), ("k10-cap+1", 10, 2561, {}), ("k20-cap", 20, 5120, {}), ("k20-cap+1", 20, 5121, {}),
    ("k10-cap-inv", 10, 2565, dict(invalid=5)), ("k10-cap+1-inv", 10, 2566, dict(invalid=5)),
    ("k20-cap-inv", 20, 5125, dict(invalid=5)), ("k20-cap+1-inv", 20, 5126, dict(invalid=5)),
    # the last size of the register-resident compaction, the first of the gather path (one-thread last round)
    ("k20-8192", 20, 8192, {}), ("k20-8193", 20, 8193, {}),
    # the 16384-ray batch: 37 invalid rows over all 25 rounds
    ("k20-12544", 20, 12544, dict(invalid=37)), ("k10-12544", 10, 12544, dict(invalid=37)),
    # the maximum: full count scan, chunk = KM_CHUNK_MAX
    ("k20-16384", 20, 16384, {}), ("k10-16384", 10, 16384, {}),
    # ... with a workgroup's whole chunk in one cluster (the value-field overflow of the Lloyd words)
    ("k20-16384-ordered", 20, 16384, dict(ordered=True, full_chunk=True)),
    ("k10-16384-ordered", 10, 16384, dict(ordered=True, full_chunk=True)),
    # (4 invalid rows: chunk still 1024, the last one short; no chunk of this set is uniform)
    ("k20-16380-ordered", 20, 16384, dict(ordered=True, invalid=4)),
    ("k20-niter1", 20, 6272, dict(niter=1)), ("k20-niter30", 20, 6272, dict(niter=30)),
    ("k10-niter30", 10, 2000, dict(niter=30)),
    # the split walk at K = 10 and on the gather path
    ("k10-degenerate", 10, 6272, dict(degenerate=True)), ("k20-degenerate-12544", 20, 12544, dict(degenerate=True)),
    # faiss's copy corner nv == K (centroids = the points, unnormalised, in order) and nv == K + 1
    ("k10-nv=K", 10, 17, dict(invalid=7, scale=2.0)), ("k10-nv=K+1", 10, 18, dict(invalid=7, scale=2.0, seed=1)),
    ("k20-nv=K", 20, 27, dict(invalid=7, scale=2.0)), ("k20-nv=K+1", 20, 28, dict(invalid=7, scale=2.0)),
    # no Lloyd round: the renormalised init picks and the final search
    ("k20-niter0", 20, 2000, dict(niter=0)),
]
# Cases whose centroids are not bit-equal to the oracle's but agree to 1e-5 with equal labels (none).
_NOT_BIT_EQUAL = ()


@pytest.mark.parametrize("cid,K,n,opt", _CASES, ids=[c[0] for c in _CASES])
def test_parity_matrix(dev, cid, K, n, opt):
    """k-means, selection and losses against the oracle.  Labels equal (-9 on invalid rows), raw[3] ==
    nv, centroids BIT-EQUAL (np.array_equal: the oracle restates the kernel's arithmetic; no case
    needed the 1e-5 fallback of _NOT_BIT_EQUAL), weighted terms within rtol 1e-4 / atol 1e-8 (the
    bound of test_cluster_loss_parity), gradient rows of invalid normals exactly zero per term.
    niter = 0: faiss's Clustering::train calls post_process_centroids (the spherical renormalisation)
    on the init picks before its iteration loop, so the picks are renormalised also when the loop
    runs zero times — the oracle did that, the kernel skipped it (`if (niter_eff > 0)`) and was
    changed; the nv == K cases pin the one exception (faiss returns the copied points untouched, in
    order), with points of length 2 so that a renormalisation would show."""
    niter = opt.get("niter", 20)
    invalid = opt.get("invalid", 0)
    if opt.get("degenerate"):
        X = _degenerate_normals(n, seed=5)
    else:
        X = _normals(n, seed=opt.get("seed", n + K), ordered=opt.get("ordered", False), invalid=invalid, scale=opt.get("scale", 1.0))
    valid, Xv, C, a, lab = _oracle(X, K, niter, need_negative=not opt.get("degenerate"))
    nv = len(Xv)
    assert nv == n - invalid
    if cid.endswith("nv=K"):
        assert nv == K and np.array_equal(C, Xv[:K])
    chunk = -(-nv // KM_BLOCKS)
    if n == 16384:
        assert chunk == 1024  # KM_CHUNK_MAX
    if opt.get("full_chunk"):  # the case keeps covering the overflow: a full chunk with one k-means label
        assert max(np.bincount(a[b * chunk:(b + 1) * chunk]).max() for b in range(KM_BLOCKS)) == 1024
    ort, cdot, cl1 = losses_ref.cluster_losses(torch.from_numpy(Xv), torch.from_numpy(lab))
    Xd = torch.from_numpy(X).to(dev).requires_grad_(True)
    terms, labels, cents, raw = L.cluster_losses(Xd, K=K, niter=niter, t_similar=0.99, w=W)
    dn = [torch.autograd.grad(terms[q], Xd, retain_graph=True)[0] for q in range(3)]
    _status_clean(dev, K)
    lab_d = labels.cpu().numpy()
    cen_d = cents.cpu().numpy()
    diff = float(np.abs(cen_d - C).max())
    print(f"{cid}: nv={nv} centroid max|d|={diff:.3e} bit-equal={np.array_equal(cen_d, C)} "
          f"labels equal={np.array_equal(lab_d[valid], lab)}")
    assert np.array_equal(lab_d[valid], lab)
    assert np.all(lab_d[~valid] == -9)
    assert float(raw[3]) == nv
    if cid in _NOT_BIT_EQUAL:
        np.testing.assert_allclose(cen_d, C, rtol=0, atol=1e-5)
    else:
        assert np.array_equal(cen_d, C), diff
    np.testing.assert_allclose(terms.detach().cpu().numpy(), [W[0] * ort.item(), W[1] * cdot.item(), W[2] * cl1.item()],
                               rtol=1e-4, atol=1e-8)
    inv_rows = torch.from_numpy(~valid).to(dev)
    for q in range(3):
        assert torch.isfinite(dn[q]).all()
        assert float(dn[q][inv_rows].abs().sum()) == 0.0
        assert float(dn[q].abs().sum()) > 0.0


# ---- 2. the three gradient rows against float64 ---------------------------------------------------
def _frame80():
    """Three unit axes pairwise 80 degrees apart (e_i + t (1,1,1), t from cos 80 = (2t + 3t^2) /
    (1 + 2t + 3t^2)), in a fixed generic rotation: |c_i . c_j| ~ 0.17, far from the ort term's kink."""
    s = np.cos(np.deg2rad(80.0))
    s = s / (1.0 - s)
    t = (-2.0 + np.sqrt(4.0 + 12.0 * s)) / 6.0
    f = np.eye(3) + t
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    q, _ = np.linalg.qr(np.random.default_rng(80).normal(size=(3, 3)))
    return f @ q


def _term_grads(Xv, lab, dtype):
    x = torch.from_numpy(Xv).to(dtype).requires_grad_(True)
    terms = losses_ref.cluster_losses(x, torch.from_numpy(lab))
    return [torch.autograd.grad(W[q] * terms[q], x, retain_graph=True)[0].double().numpy() for q in range(3)]


@pytest.mark.parametrize("K,n,invalid", [(20, 6272, 37), (10, 2000, 0), (20, 12544, 0)])
def test_term_gradients_vs_float64(dev, K, n, invalid):
    """dL_dnormals row q alone (terms[q].backward()) against the float64 autograd of W[q] * term q of
    losses_ref.cluster_losses on the oracle's labels.  Yardstick: e32, the rel-L2 error of the same
    expression in float32 torch on the CPU; the device row must lie within 4 * e32 + 1e-6 (another
    summation order, its own f32 centroid; the floor covers a tiny e32).  Kinks kept out: a frame with
    |c_i . c_j| >= 0.05 (asserted), and the L1 row's components with |x - c| < 1e-6 dropped (at most
    0.1 % of them, asserted).  Per selected cluster c and term q the sum over the members of
    sg * dn[q] — as a vector, N * G[q][c] plus the direct parts, and projected on the unit centroid —
    is held to the same bound relative to the sum of the members' |row| (the sum itself cancels: for
    the ort row its projection is 0).  terms.sum().backward() equals (dn[0] + dn[1]) + dn[2] bit for bit.
    Measured on one MI355X, e32 / device rel-L2 (ort; dot; L1), L1 components dropped:
      (20, 6272, 37 invalid)  5.7e-8 / 1.4e-7;  3.9e-8 / 1.2e-7;  4.2e-8 / 6.5e-8;  0
      (10, 2000)              9.7e-8 / 9.1e-8;  1.2e-7 / 7.5e-8;  7.2e-8 / 5.4e-8;  0
      (20, 12544)             8.1e-8 / 9.4e-8;  1.2e-7 / 7.8e-8;  4.9e-8 / 5.8e-8;  1
    and the per-cluster sums: f32 at most 1.8e-7, device at most 2.0e-7 of their scale."""
    X = _normals(n, seed=n + K + 1, frame=_frame80(), invalid=invalid)
    valid, Xv, C, a, lab = _oracle(X, K, 20)
    v_ort, v_l1, cc = losses_ref.kink_values(Xv, lab)
    assert np.abs(v_ort).min() >= 0.05, v_ort
    g64 = _term_grads(Xv, lab, torch.float64)
    g32 = _term_grads(Xv, lab, torch.float32)
    Xd = torch.from_numpy(X).to(dev).requires_grad_(True)
    terms, labels, cents, raw = L.cluster_losses(Xd, K=K, niter=20, t_similar=0.99, w=W)
    rows = [torch.autograd.grad(terms[q], Xd, retain_graph=True)[0] for q in range(3)]
    (total,) = torch.autograd.grad(terms.sum(), Xd)
    _status_clean(dev, K)
    assert np.array_equal(labels.cpu().numpy()[valid], lab)
    assert torch.equal(total, (rows[0] + rows[1]) + rows[2])
    gd = [r.cpu().numpy().astype(np.float64) for r in rows]
    for q in range(3):
        assert not gd[q][~valid].any()
    gd = [g[valid] for g in gd]
    # the L1 row's kink components
    keep = np.ones_like(g64[2], dtype=bool)
    sel = lab != 0
    la = np.abs(lab[sel])
    near = np.zeros((int(sel.sum()), 3), bool)
    for k in range(3):
        near[la == k + 1] = np.abs(v_l1[k]) < 1e-6
    keep[sel] = ~near
    dropped = int((~keep).sum())
    assert dropped <= 1e-3 * keep.size, dropped
    sg = np.where(lab < 0, -1.0, 1.0)[:, None]
    for q, name in enumerate(("ort", "dot", "L1")):
        m = keep if q == 2 else np.ones_like(keep)
        den = np.linalg.norm(g64[q][m])
        e32 = np.linalg.norm((g32[q] - g64[q])[m]) / den
        edev = np.linalg.norm((gd[q] - g64[q])[m]) / den
        print(f"K={K} n={n} term {name}: e32={e32:.3e} device={edev:.3e} (L1 components dropped: {dropped})")
        assert edev <= 4 * e32 + 1e-6, (name, edev, e32)
        for k in range(3):
            mem = np.abs(lab) == k + 1
            mk = mem[:, None] & m
            scale = np.linalg.norm(g64[q][mem], axis=1).sum()
            s64, s32, sd = ((sg * g * mk)[mem].sum(0) for g in (g64[q], g32[q], gd[q]))
            ev32, evd = np.linalg.norm(s32 - s64) / scale, np.linalg.norm(sd - s64) / scale
            ep32, epd = abs((s32 - s64) @ cc[k]) / scale, abs((sd - s64) @ cc[k]) / scale
            print(f"    cluster {k + 1}: sum e32={ev32:.3e} device={evd:.3e}; on the centroid e32={ep32:.3e} "
                  f"device={epd:.3e}")
            assert evd <= 4 * ev32 + 1e-6, (name, k, evd, ev32)
            assert epd <= 4 * ep32 + 1e-6, (name, k, epd, ep32)


# ---- 3. schedule, device weights, total and refusals through the C ABI ----------------------------
SENT = -12345.5


def _buffers(dev, T, K):
    return (torch.full((L.N_OUT,), SENT, device=dev), torch.full((T,), -77, dtype=torch.int32, device=dev),
            torch.full((K, 3), SENT, device=dev), torch.full((3, T, 3), SENT, device=dev))


def _launch(dev, Xd, K, niter=20, w=W, w_dev=None, step=None, start=0.0, grow=1.0, photo=None, plan=None):
    """ncn_cluster_loss through _lib.call on sentinel-filled outputs -> (out, labels, cents, dn)."""
    T = Xd.shape[0]
    bufs = _buffers(dev, T, K)
    if plan is None:
        plan = L.kmeans_plan(dev, T, K)
    ws = L._cluster_workspace(dev, K)
    _lib.call("ncn_cluster_loss", Xd, T, K, niter, plan, 0.99, float(w[0]), float(w[1]), float(w[2]), w_dev, step,
              float(start), float(grow), photo, *bufs, ws)
    return bufs


@pytest.fixture(scope="module")
def abi_set(dev):
    X = _normals(2000, seed=2020)
    _oracle(X, 20, 20)
    Xd = torch.from_numpy(X).to(dev)
    return Xd, [b.clone() for b in _launch(dev, Xd, 20)]


def _sched32(w, step, start, grow):
    """losses_ref.w_sched in the kernel's f32 operation order: ds = (float)step - start;
    max(0, min(w, ds * (w / grow)))."""
    w, ds = np.float32(w), np.float32(np.float32(step) - np.float32(start))
    return np.float32(max(np.float32(0), min(w, np.float32(ds * np.float32(w / np.float32(grow))))))


@pytest.mark.parametrize("step", [0, 499, 500, 501, 1750, 3000, 3001, 10 ** 6])
def test_device_schedule_and_total(dev, abi_set, step):
    """out_losses[7..9] = the f32 schedule exactly (clamp below the start, the corner step == start,
    the ramp, saturation), [4..6] = [7..9] * [0..2], [10] = the f32 running sum photo[0] + photo[1] +
    [4] + [5] + [6]; at steps <= start every gradient is exactly zero; labels, centroids and the
    unweighted terms do not depend on the step."""
    Xd, (out0, lab0, cen0, dn0) = abi_set
    photo = torch.tensor([0.0123, 0.0045, 1.0, 1.0], device=dev)
    sd = torch.tensor(step, dtype=torch.int64, device=dev)
    out, lab, cen, dn = _launch(dev, Xd, 20, step=sd, start=500.0, grow=2500.0, photo=photo)
    _status_clean(dev, 20)
    o = out.cpu().numpy()
    want = [_sched32(w, step, 500.0, 2500.0) for w in W]
    assert [np.float32(v) for v in o[7:10]] == want, (o[7:10], want)
    assert abs(float(want[0]) - losses_ref.w_sched(W[0], step)) <= 1e-6 * W[0]  # (the f32 restatement is w_sched)
    assert np.array_equal(o[4:7], o[7:10] * o[0:3])
    tot = np.float32(0)
    for v in (np.float32(0.0123), np.float32(0.0045), o[4], o[5], o[6]):
        tot = np.float32(tot + v)
    assert o[10] == tot
    assert torch.equal(lab, lab0) and torch.equal(cen, cen0) and torch.equal(out[:4], out0[:4])
    assert float(o[0]) > 0 and float(o[3]) == 2000
    if step <= 500:
        assert want == [0, 0, 0] and float(dn.abs().sum()) == 0.0
    else:
        assert float(dn.abs().sum()) > 0.0
    if step > 3000:  # saturated: (step - start) * (w / grow) > w
        assert want == [np.float32(w) for w in W] and torch.equal(dn, dn0)


def test_device_weights_replace_host_weights(dev, abi_set):
    """w_dev replaces (w_ort, w_dot, w_l1): host weights passed as NaN leak into no output.  With
    photo_loss NULL out_losses[10] is left as the caller set it."""
    Xd, ref = abi_set
    nan = float("nan")
    got = _launch(dev, Xd, 20, w=(nan, nan, nan), w_dev=torch.tensor(W, dtype=torch.float32, device=dev))
    _status_clean(dev, 20)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    assert float(got[0][10]) == SENT and bool(torch.isfinite(got[0][:10]).all()) and bool(torch.isfinite(got[3]).all())


def test_entry_point_refusals(dev, abi_set):
    """n_tri = 16385, K = 15, niter = 31 and a NULL plan return an error with its message and launch
    nothing: the sentinel-filled outputs stay as they were."""
    Xd, _ = abi_set
    plan = L.kmeans_plan(dev, 2000, 20)
    big = torch.zeros(16385, 3, device=dev)
    for kw, msg in ((dict(Xd=big, K=20, plan=plan), "exceeds 16384"), (dict(Xd=Xd, K=15, plan=plan), "K must be 10 or 20"),
                    (dict(Xd=Xd, K=20, niter=31, plan=plan), r"niter must be in \[0, 30\]"),
                    (dict(Xd=Xd, K=20, plan=None), "kmeans_plan required")):
        T = kw["Xd"].shape[0]
        bufs = _buffers(dev, T, 20)
        args = (kw["Xd"], T, kw["K"], kw.get("niter", 20), kw["plan"], 0.99, 1.0, 1.0, 1.0, None, None, 0.0, 1.0, None,
                *bufs, L._cluster_workspace(dev, 20))
        rc = _lib.lib().ncn_cluster_loss(*_lib.marshal("ncn_cluster_loss", args))
        assert rc != 0 and _lib.lib().ncn_last_error().decode()
        with pytest.raises(_lib.NcnError, match=msg):
            _lib.call("ncn_cluster_loss", *args)
        assert all(bool((b == s).all()) for b, s in zip(bufs, (SENT, -77, SENT, SENT)))
    _status_clean(dev, 20)


def test_mismatched_plan_sets_status(dev, abi_set):
    """A plan built for another (n_tri, K) sets the status word to 3 and check_cluster_status raises;
    the launch drops its cluster terms.  The word is cleared afterwards (it is sticky)."""
    Xd, _ = abi_set
    ws = L._cluster_workspace(dev, 20)
    off = int(_lib.lib().ncn_cluster_status_offset(20))
    try:
        for other in ((2001, 20), (2000, 10)):
            out, lab, cen, dn = _launch(dev, Xd, 20, plan=L.kmeans_plan(dev, *other))
            assert int(ws.view(torch.int32)[off].item()) == 3
            with pytest.raises(_lib.NcnError):
                L.check_cluster_status(dev)
            assert float(out[:3].abs().sum()) == 0.0 and float(out[4:7].abs().sum()) == 0.0 and float(dn.abs().sum()) == 0.0
            ws.view(torch.int32)[off] = 0
    finally:
        ws.view(torch.int32)[off] = 0
    L.check_cluster_status(dev)
    got = _launch(dev, Xd, 20)  # and the next launch is whole again
    assert all(torch.equal(g, r) for g, r in zip(got, abi_set[1]))


# ---- 4. the launch-sequence wrap of the Lloyd tags ------------------------------------------------
def test_sequence_wrap_and_launch_mixing(dev):
    """One workspace, 1100 launches cycling A (512 points, niter 20), B (12 points: unclustered, void
    tags), C (nv == K: no Lloyd round, void tags in buffer 1), A with niter 1 (one round per buffer)
    and A: the sequence field of the tags (8 bits) wraps four times.  In the windows 500-530 and
    1010-1040 and over the last cycle every launch reproduces the outputs its kind gave first (all four
    buffers, compared on the device, ONE synchronisation per window); the status word stays clear."""
    A = torch.from_numpy(_normals(512, seed=512)).to(dev)
    B = torch.from_numpy(_normals(12, seed=12)).to(dev)
    Cx = torch.from_numpy(_normals(20, seed=20, scale=2.0)).to(dev)
    kinds = {"A": (A, 20), "B": (B, 20), "C": (Cx, 20), "A1": (A, 1)}
    first = {k: _launch(dev, x, 20, niter=ni) for k, (x, ni) in kinds.items()}
    # what the recorded outputs are: A is the oracle's clustering, B is empty, C the points themselves
    Xa = A.cpu().numpy()
    _, _, Ca, _, lab_a = _oracle(Xa, 20, 20)
    assert np.array_equal(first["A"][2].cpu().numpy(), Ca) and np.array_equal(first["A"][1].cpu().numpy(), lab_a)
    assert float(first["B"][0][3]) == 12 and float(first["B"][3].abs().sum()) == 0.0
    assert torch.equal(first["C"][2], Cx) and float(first["C"][0][3]) == 20
    assert not torch.equal(first["A1"][2], first["A"][2])
    cycle = ("A", "B", "C", "A1", "A")
    windows = ((500, 530), (1010, 1040), (1095, 1100))
    pending, checked = [], 0
    for i in range(1100):
        k = cycle[i % len(cycle)]
        x, ni = kinds[k]
        got = _launch(dev, x, 20, niter=ni)
        w = next((w for w in windows if w[0] <= i < w[1]), None)
        if w is not None:
            pending.append(torch.stack([(g == r).all() for g, r in zip(got, first[k])]).all())
            if i == w[1] - 1:
                assert bool(torch.stack(pending).all()), f"launches {w[0]}-{w[1]} differ from their first run"
                checked += len(pending)
                pending = []
    assert checked == 65
    _status_clean(dev, 20)
