"""The k-variate normal over row groups of one ring (ops/csrc/mvn_groups.hip,
``kernels.mvn_groups``) against the fp64 reference (models/multivariate_normal.py), in the
shape of test_bivariate_pairs_gpu.py.

The reference of every case is built on the CPU, in float64, from the values as the ring
stores them (bf16-rounded, then upcast).  ``test_reference_keeps_clear_of_the_lines`` checks,
without a GPU, that no finite d2 lies within 1 % of q_k(thr) and that on the anomalous slots
no contribution lies within 1 % of d2 of the naming line d2 / k, so that demanding exact
counts, verdicts and blame masks of the kernel is fair.

The metrics of a group share a latent load (pairwise correlation ~0.5), which gives an 8 x 8
covariance a condition number around 10 (measured by the CPU test: below 30).  Near-collinear
inputs are kept out of the numeric bounds; the duplicated-row group runs with the visible
``EPS`` of the pair test.

Bound on mean / cov / d2 / contrib / score: the larger of the pair test's ``D2_TOL`` and
4 x D, D the distance between the reference formulas run in float32 and in float64 on the
CPU (docs/SCORING.md), measured per k here and printed."""

import functools

import numpy as np
import pytest
import torch

from foremast_amd.ingest.ringbuffer import HistoryRing
from foremast_amd.models import bivariate as biv_ref
from foremast_amd.models import multivariate_normal as mvn

SEED = 1
N, R, W, WIDE = 40, 1003, 5, 67
MIN_VALID = 10
EPS = 1e-3    # as in test_bivariate_pairs_gpu.py: the duplicated row is singular under 1e-9
D2_TOL = dict(rtol=2e-3, atol=1e-3)   # tests/test_bivariate_pairs_gpu.py
GROUPS = [
    (1, 0),                             # 0  k = 2, descending; spikes in row 1 only
    (4, 3, 2),                          # 1  k = 3, descending; rows 2 and 4 move against their correlation
    (5, 6, 7, 8, 9),                    # 2  k = 5; shares rows 5, 6, 9 with the next (both flagged by row 6)
    (5, 6, 9),                          # 3
    (10, 11, 12, 13, 14, 15, 16, 17),   # 4  k = 8; row 12 alone in one slot, rows 15 / 16 in another
    (18, 18, 19),                       # 5  a duplicated row
    (20, 21, 22),                       # 6  isolated NaNs in row 20, a 60-point outage in row 21
    (23, 24, 25),                       # 7  all-NaN row 24: verdict -1
    (33, 32, 31, 30, 29, 28, 27, 26),   # 8  k = 8, descending, healthy
    (34, 35),                           # 9  row 35 NaN in window slot 2: d2 NaN, not counted
    (36, 37),                           # 10 all-NaN window of row 36: verdict -1
    (38, 39),                           # 11 fewer jointly valid points than MIN_VALID: verdict -1
    (10, 11, 12, 13, 14),               # 12 k = 5 on rows of group 4
]
KS = [len(g) for g in GROUPS]
LATENT = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 2] + [3] * 8 + [4] * 5 + [5] * 3 + [6] * 8 + [7, 7, 8, 8, 9, 9])
SPIKES = ((1, (1, 3), 9.0), (2, (2,), 7.0), (4, (2,), -7.0), (6, (0, 2, 4), 12.0), (12, (4,), 10.0),
          (15, (1,), 7.0), (16, (1,), -7.0), (18, (0,), 8.0))
RINGS = [(0, R), (517, R), (1002, R), (600, 700), (37, 100)]   # (head, len)
CASES = [(dt, head, ln, P, W) for dt in ("bf16", "fp32") for head, ln in RINGS for P in (1, 3)]
CASES.append(("bf16", 517, R, 3, WIDE))    # more slots than lanes


def table():
    t = np.full((len(GROUPS), 8), -1, dtype=np.int32)
    for q, g in enumerate(GROUPS):
        t[q, :len(g)] = g
    return t


@functools.lru_cache(maxsize=None)
def world():
    """Physical ring values [N, R], per-row thresholds and the windows [N, P, WIDE] for P = 1, 3
    (a case with W slots takes the first W)."""
    assert len(LATENT) == N
    g = np.random.default_rng(SEED)
    lvl, sig = g.uniform(5, 50, N), g.uniform(0.5, 3, N)
    sig[18] = 1.0
    z = g.standard_normal((LATENT.max() + 1, R + WIDE))[LATENT]       # the rows of a block share a latent load
    v = lvl[:, None] + sig[:, None] * (0.7 * z + 0.7 * g.standard_normal((N, R + WIDE)))
    hist = v[:, :R].astype(np.float32)
    hist[20, g.choice(R, 20, replace=False)] = np.nan
    hist[21, 400:460] = np.nan
    hist[24] = np.nan
    keep = hist[38, 40:46].copy()
    hist[38] = np.nan
    hist[38, 40:46] = keep
    slot = v[:, R:].copy()                                            # [N, WIDE]
    for r, cols, k in SPIKES:
        slot[r, list(cols)] += k * sig[r]
    wins = {}
    for P in (1, 3):
        c = slot[:, None, :] + 0.1 * sig[:, None, None] * g.standard_normal((N, P, WIDE))
        if P == 3:
            c[1, 1, 1] = c[6, 0, 2] = c[12, 2, 0] = c[12, 0, 0] = np.nan   # a pod missing in some slots
        c[35, :, 2] = np.nan
        c[36] = np.nan
        wins[P] = c.astype(np.float32)
    thr = (3.0 + np.arange(N) % 3).astype(np.float32)
    return hist, thr, wins


def stored(dtype):
    h = torch.from_numpy(world()[0])
    return h.bfloat16().float() if dtype == "bf16" else h


def thr2_of(groups=GROUPS):
    thr = world()[1]
    return torch.tensor([mvn.chi2_threshold(float(thr[g[0]]), len(g)) for g in groups], dtype=torch.float32)


def score_groups(h, cm, groups, thr2, eps, dt):
    """The reference over ``groups`` in dtype ``dt`` (float64: the reference; float32: the same
    formulas, for D), padded like the kernel's outputs.  ``h [N, T]``, ``cm [N, W]`` pod means."""
    Ng, Wn = len(groups), cm.shape[1]
    o = dict(mean=torch.zeros(Ng, 8, dtype=dt), cov=torch.zeros(Ng, 36, dtype=dt), nvalid=torch.zeros(Ng),
             d2=torch.full((Ng, Wn), float("nan"), dtype=dt), contrib=torch.zeros(Ng, Wn, 8, dtype=dt),
             count=torch.zeros(Ng, dtype=torch.int32), verdict=torch.zeros(Ng, dtype=torch.int8),
             blame=torch.zeros(Ng, dtype=torch.int32), flag=torch.zeros(Ng, Wn, dtype=torch.bool),
             names=torch.zeros(Ng, Wn, 8, dtype=torch.bool), x=torch.zeros(Ng, Wn, 8))
    for k in sorted({len(g) for g in groups}):
        sel = torch.tensor([q for q, g in enumerate(groups) if len(g) == k])
        rows = torch.tensor([groups[q] for q in sel.tolist()])                 # [n, k]
        fit = mvn.fit_mvn(h[rows].permute(0, 2, 1).double())
        fit = mvn.MvnFit(fit.mean.to(dt), fit.cov.to(dt), fit.count)
        x = cm[rows].permute(0, 2, 1)
        s = mvn.score_mvn(fit, x.to(dt), thr2[sel].to(dt), MIN_VALID, eps=eps)
        o["mean"][sel, :k], o["cov"][sel, :k * (k + 1) // 2], o["nvalid"][sel] = fit.mean, fit.cov, fit.count.float()
        o["d2"][sel], o["contrib"][sel, :, :k], o["count"][sel], o["verdict"][sel] = s.d2, s.contrib, s.count, s.verdict
        o["blame"][sel], o["flag"][sel], o["names"][sel, :, :k], o["x"][sel, :, :k] = s.blame, s.flag, s.names, x
    valid = ~torch.isnan(o["d2"])
    o["score"] = torch.where(valid, o["d2"].clamp(min=0).sqrt(), torch.zeros_like(o["d2"])).amax(1)
    return o


@functools.lru_cache(maxsize=None)
def reference(dtype, head, length, P, Wn=W, eps=EPS):
    """fp64 fit on the gathered logical rows, nanmean over pods, the verdict and attribution rules;
    ``D``: per k and output, the largest distance of the float32 run of the same formulas."""
    _, _, wins = world()
    idx = (head + torch.arange(length)) % R
    h = stored(dtype)[:, idx]
    cm = torch.nanmean(torch.from_numpy(wins[P][:, :, :Wn]), 1)
    thr2 = thr2_of()
    ref = score_groups(h, cm, GROUPS, thr2, eps, torch.float64)
    f32 = score_groups(h, cm, GROUPS, thr2, eps, torch.float32)
    ref["thr2"] = thr2
    ref["D"] = {}
    scored = ref["nvalid"] >= MIN_VALID
    for k in sorted(set(KS)):
        sel = torch.tensor([q for q, kk in enumerate(KS) if kk == k and scored[q]])
        ref["D"][k] = {}
        for name in ("mean", "cov", "d2", "contrib", "score"):
            e = (f32[name][sel].double() - ref[name][sel]).abs()
            ref["D"][k][name] = float(e[torch.isfinite(e)].max())
    return ref


def test_reference_keeps_clear_of_the_lines():
    """No finite d2 of any case within 1 % of q_k(thr), no contribution of an anomalous slot
    within 1 % of d2 of the line d2 / k (a seed that fails here would hide, or fake, a count
    or blame mismatch on the GPU), and the cases hold what they are there for."""
    for case in CASES:
        ref = reference(*case)
        d2, thr2 = ref["d2"], ref["thr2"].double()[:, None].expand_as(ref["d2"])
        fin = torch.isfinite(d2)
        assert ((d2[fin] - thr2[fin]).abs() > 0.01 * thr2[fin]).all(), case
        for q, k in enumerate(KS):
            f = ref["flag"][q]
            c, line = ref["contrib"][q, f, :k], d2[q, f] / k
            assert ((c - line[:, None]).abs() > 0.01 * d2[q, f][:, None]).all(), (case, q)
        v = ref["verdict"].tolist()
        assert v[7] == -1 and v[10] == -1 and v[11] == -1, case          # all-NaN row, no window, few points
        assert torch.isnan(d2[9, 2]) and torch.isnan(d2[10]).all() and ref["count"][9] == 0, case
        assert torch.isfinite(d2[11]).all() and 0 < ref["nvalid"][11] < MIN_VALID
        if case[2] == R:
            blame = ref["blame"].tolist()
            assert [v[q] for q in (0, 1, 2, 3, 4, 5, 12)] == [1] * 7 and v[8] == 0 and v[6] in (0, 1), case
            assert blame[0] == 0b01                   # (1, 0): row 1 is metric 0 -- exactly one metric
            assert blame[1] == 0b101                  # (4, 3, 2): rows 4 and 2 -- two metrics
            assert blame[2] == 0b00010 and blame[3] == 0b010 and blame[12] == 0b00100
            assert blame[4] == 0b01100100             # row 12 in slot 4, rows 15 and 16 in slot 1
            assert blame[5] == 0b011                  # both copies of the duplicated row
            assert R - 80 <= ref["nvalid"][6] < R - 60
    # the condition number the numeric bounds assume
    ref = reference("fp32", 0, R, 1)
    for q in (4, 8):
        full = np.zeros((8, 8))
        for i in range(8):
            for j in range(i + 1):
                full[i, j] = full[j, i] = float(ref["cov"][q, mvn.tri_index(i, j)])
        cond = np.linalg.cond(full / np.sqrt(np.outer(np.diag(full), np.diag(full))))
        print("group", q, "condition number of the 8 x 8 correlation matrix", cond)
        assert cond < 30


def device_inputs(dtype, P, Wn=W):
    dev = torch.device("cuda:0")
    hist, thr, wins = world()
    ring = HistoryRing(N, R, torch.bfloat16 if dtype == "bf16" else torch.float32, dev)
    assert ring.ld == (1008 if dtype == "bf16" else 1004)   # the vector path, then a 3-column scalar tail
    ring.data.copy_(torch.from_numpy(hist))
    cur = torch.from_numpy(np.ascontiguousarray(wins[P][:, :, :Wn])).reshape(N, P * Wn).to(dev)
    return dev, ring, cur, torch.from_numpy(thr).to(dev)


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


def within(got, ref, D, what, q):
    """|got - ref| <= max(D2_TOL, 4 D) elementwise; NaNs in the same places."""
    got, ref = got.double(), ref.double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, q)
    fin = torch.isfinite(ref)
    err = (got - ref).abs()[fin]
    tol = torch.clamp(D2_TOL["atol"] + D2_TOL["rtol"] * ref.abs()[fin], min=4 * D)
    assert (err <= tol).all(), (what, q, float(err.max()), float(tol.min()))
    return float(err.max()) if err.numel() else 0.0


SENTINEL = {torch.float32: -12345.0, torch.int32: -77, torch.int8: -7}


def guarded_outputs(K, Ng, Wn, dev):
    """Output buffers with one more row, filled with a sentinel; the views handed to the kernel."""
    shapes = {"mean": ((Ng, 8), torch.float32), "cov": ((Ng, 36), torch.float32), "nvalid": ((Ng,), torch.float32),
              "d2": ((Ng, Wn), torch.float32), "count": ((Ng,), torch.int32), "verdict": ((Ng,), torch.int8),
              "score": ((Ng,), torch.float32), "blame": ((Ng,), torch.int32), "contrib": ((Ng, Wn, 8), torch.float32)}
    full = {k: torch.full((s[0] + 1,) + s[1:], SENTINEL[dt], dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    return full, {k: v[:Ng] for k, v in full.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,head,length,P,Wn", CASES)
def test_groups_match_reference(K, dtype, head, length, P, Wn):
    dev, ring, cur, thr = device_inputs(dtype, P, Wn)
    Ng = len(GROUPS)
    full, views = guarded_outputs(K, Ng, Wn, dev)
    out = K.mvn_groups(ring.data, head, length, table(), cur, P, Wn, thr, min_valid=MIN_VALID, eps=EPS,
                       contrib=True, out=views)
    pairs = K.bivariate_pairs(ring.data, head, length, np.array([GROUPS[0]], dtype=np.int32), cur, P, Wn, thr,
                              min_valid=MIN_VALID, eps=EPS)
    torch.cuda.synchronize()
    assert all(out[k].data_ptr() == views[k].data_ptr() for k in views)      # written in place
    for k, v in full.items():                                                # the row behind every output
        assert (v[Ng] == SENTINEL[v.dtype]).all(), k
    ref = reference(dtype, head, length, P, Wn)
    got = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(got["nvalid"], ref["nvalid"])
    assert torch.equal(got["count"], ref["count"])
    assert torch.equal(got["verdict"], ref["verdict"])
    assert torch.equal(got["blame"], ref["blame"])
    worst = {}
    for q, k in enumerate(KS):
        tri = k * (k + 1) // 2
        assert (got["mean"][q, k:] == 0).all() and (got["cov"][q, tri:] == 0).all()
        assert (got["contrib"][q, :, k:] == 0).all()
        if ref["nvalid"][q] == 0:
            continue
        D = ref["D"][k]
        e = {"mean": within(got["mean"][q, :k], ref["mean"][q, :k], D["mean"], "mean", q),
             "cov": within(got["cov"][q, :tri], ref["cov"][q, :tri], D["cov"], "cov", q)}
        if ref["nvalid"][q] >= MIN_VALID:
            e["d2"] = within(got["d2"][q], ref["d2"][q], D["d2"], "d2", q)
            e["contrib"] = within(got["contrib"][q, :, :k], ref["contrib"][q, :, :k], D["contrib"], "contrib", q)
            e["score"] = within(got["score"][q], ref["score"][q], D["score"], "score", q)
        for name, val in e.items():
            worst.setdefault(k, {}).setdefault(name, 0.0)
            worst[k][name] = max(worst[k][name], val)
    for k in sorted(worst):
        print(f"k={k} D (fp32 formulas vs fp64) {ref['D'][k]}  kernel max error {worst[k]}")
    assert torch.isnan(got["d2"][9, 2]) and torch.isnan(got["d2"][10]).all()
    # a k = 2 group against the pair kernel on the same pair
    torch.testing.assert_close(got["d2"][0], pairs["d2"][0].cpu(), equal_nan=True, **D2_TOL)


@pytest.mark.gpu
def test_large_level_error_against_the_pair_kernel(K):
    """fp32 ring of 10,080 points at level 1e4 with sigma 1, k = 4: the shifted sums and the
    relative merge keep d2 as close to the fp64 reference as the pair kernel keeps it on two
    of the same rows.  The factor 2 is test_large_level_error_against_k8's allowance for the
    summation order of fp32 sums of the same length; it is not a measured property."""
    dev = torch.device("cuda:0")
    n, r, k = 16, 10080, 4
    g = np.random.default_rng(5)
    z = g.standard_normal((n // k, r + W))[np.arange(n) // k]
    v = 1e4 + 0.7 * z + 0.7 * g.standard_normal((n, r + W))
    v[:, r:] += g.uniform(-4, 4, (n, W))
    ring = HistoryRing(n, r, torch.float32, dev)
    ring.data.copy_(torch.from_numpy(v[:, :r].astype(np.float32)))
    cur = torch.from_numpy(v[:, r:].astype(np.float32)).to(dev)
    groups = np.arange(n, dtype=np.int32).reshape(-1, k)
    thr = torch.full((n,), 3.0, device=dev)
    out = K.mvn_groups(ring.data, 3, r, groups, cur, 1, W, thr)
    pr = K.bivariate_pairs(ring.data, 3, r, np.ascontiguousarray(groups[:, :2]), cur, 1, W, thr)
    torch.cuda.synchronize()
    h64, c64 = ring.data.cpu().double(), cur.cpu().double()
    gi = torch.from_numpy(groups).long()
    want = mvn.mahalanobis2_mvn(mvn.fit_mvn(h64[gi].permute(0, 2, 1)), c64[gi].permute(0, 2, 1))
    want2 = biv_ref.mahalanobis2(biv_ref.fit_bivariate(h64[gi[:, :2]].permute(0, 2, 1)), c64[gi[:, :2]].permute(0, 2, 1))
    assert want.dtype == torch.float64 and want2.dtype == torch.float64
    err_new = float((out["d2"].cpu().double() - want).abs().max())
    err_pair = float((pr["d2"].cpu().double() - want2).abs().max())
    print(f"level 1e4: max |d2 - fp64|  mvn k=4 {err_new:.3e}  pair kernel {err_pair:.3e}  "
          f"(max d2 {float(want.max()):.1f} / {float(want2.max()):.1f})")
    assert err_new <= 2 * err_pair + D2_TOL["atol"], (err_new, err_pair)


def named_rows(ref):
    """Rows of the metrics named by the flagged groups."""
    return sorted({GROUPS[q][i] for q in range(len(GROUPS)) for i in range(KS[q]) if int(ref["blame"][q]) >> i & 1})


@pytest.mark.gpu
def test_state_effects(K):
    """A flagged group raises the row verdict of every named metric; the per-app anomalous
    counter moves once per row and tick, and not for a row the per-row pass flagged already."""
    dev, ring, cur, thr = device_inputs("bf16", 3)
    ref = reference("bf16", 517, R, 3)
    rows = named_rows(ref)
    assert rows == [1, 2, 4, 6, 12, 15, 16, 18]       # 6 and 12 named by two groups each, 18 twice by one
    before = torch.zeros(N, dtype=torch.int8)
    before[3::4] = -1
    before[rows[0]] = 1        # flagged by the per-row pass already: not counted again
    before[39] = 1             # in no flagged group
    before[5] = 0              # in two flagged groups, never named: stays
    app_id = (torch.arange(N) % 3).int()
    stats = torch.zeros((3, 2), dtype=torch.int32)
    stats[:, 0] = torch.bincount(app_id[before == 1].long(), minlength=3).int()
    stats[:, 1] = 777
    verdict, stats_d = before.to(dev), stats.to(dev)
    out = K.mvn_groups(ring.data, 517, R, table(), cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS,
                       verdict=verdict, app_id=app_id.to(dev), app_stats=stats_d)
    torch.cuda.synchronize()
    assert torch.equal(out["verdict"].cpu(), ref["verdict"]) and torch.equal(out["blame"].cpu(), ref["blame"])
    after = before.clone()
    after[rows] = 1
    assert torch.equal(verdict.cpu(), after) and after[5] == 0
    want = torch.bincount(app_id[after == 1].long(), minlength=3).int()
    assert torch.equal(stats_d.cpu()[:, 0], want) and int(want.sum()) == int(stats[:, 0].sum()) + len(rows) - 1
    assert (stats_d.cpu()[:, 1] == 777).all()


@pytest.mark.gpu
def test_anomaly_list(K):
    dev, ring, cur, thr = device_inputs("fp32", 3)
    ref = reference("fp32", 517, R, 3)
    q, slot, i = np.nonzero(ref["names"].numpy())
    want = sorted(zip([GROUPS[a][b] for a, b in zip(q, i)], slot.tolist(), ref["x"].numpy()[q, slot, i].tolist()))
    assert len(want) >= 12 and len(set(w[:2] for w in want)) < len(want)    # shared and duplicated rows repeat
    ab = K.AnomalyBuffer(64, dev)
    ab.reset()
    K.mvn_groups(ring.data, 517, R, table(), cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS, anomalies=ab)
    s, c, v, overflow = ab.fetch()
    assert not overflow and int(ab.count.item()) == len(want)
    got = sorted(zip(s.tolist(), c.tolist(), v.tolist()))
    assert [g[:2] for g in got] == [w[:2] for w in want]
    np.testing.assert_allclose([g[2] for g in got], [w[2] for w in want], rtol=1e-6)
    # a list shorter than the anomalies: the count goes on, nothing is written past cap
    ab.cap = 3
    ab.reset()
    ab.series.fill_(-7)
    ab.col.fill_(-7)
    ab.val.fill_(-7.0)
    K.mvn_groups(ring.data, 517, R, table(), cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS, anomalies=ab)
    assert int(ab.count.item()) == len(want)
    assert (ab.series[3:] == -7).all() and (ab.col[3:] == -7).all() and (ab.val[3:] == -7.0).all()
    head = list(zip(ab.series[:3].tolist(), ab.col[:3].tolist()))
    assert set(head) <= {w[:2] for w in want}


@pytest.mark.gpu
def test_empty_table_and_rejections(K):
    dev, ring, cur, thr = device_inputs("bf16", 1)
    out = K.mvn_groups(ring.data, 0, R, np.zeros((0, 8), dtype=np.int32), cur, 1, W, thr, contrib=True)
    assert out["d2"].shape == (0, W) and out["mean"].shape == (0, 8) and out["cov"].shape == (0, 36)
    assert out["contrib"].shape == (0, W, 8)
    assert all(out[k].shape == (0,) for k in ("nvalid", "count", "verdict", "score", "blame"))
    with pytest.raises(K.KernelShapeError):
        K.mvn_groups(ring.data, 0, R, np.array([[0, 1, N, -1, -1, -1, -1, -1]]), cur, 1, W, thr)
    with pytest.raises(K.KernelShapeError):
        K.mvn_groups(ring.data, 0, R, [list(range(9))], cur, 1, W, thr)
    with pytest.raises(K.KernelShapeError):
        K.mvn_groups(ring.data, 0, R, np.arange(9)[None], cur, 1, W, thr)
    with pytest.raises(K.KernelShapeError):     # a device table carries no thresholds of its own
        K.mvn_groups(ring.data, 0, R, torch.from_numpy(table()).to(dev), cur, 1, W, thr)
    # a device table is not range-checked on the host: the kernel reports such groups unscored
    # (NaN outputs, verdict -1, nothing read) beside the groups it scores
    t = np.full((4, 8), -1, dtype=np.int32)
    t[0, :2] = (1, 0)
    t[1, :3] = (2, N, 3)        # a row outside the ring
    t[2, :1] = (5,)             # fewer than two rows
    t[3, :3] = (4, 3, 2)
    thr2 = torch.tensor([mvn.chi2_threshold(float(world()[1][1]), 2), 9.0, 9.0,
                         mvn.chi2_threshold(float(world()[1][4]), 3)], device=dev)
    full, views = guarded_outputs(K, 4, W, dev)
    out = K.mvn_groups(ring.data, 0, R, torch.from_numpy(t).to(dev), cur, 1, W, thr, thr2=thr2, min_valid=MIN_VALID,
                       eps=EPS, contrib=True, out=views)
    torch.cuda.synchronize()
    ref = reference("bf16", 0, R, 1)
    for q in (1, 2):
        assert torch.isnan(out["d2"][q]).all() and torch.isnan(out["mean"][q]).all() and torch.isnan(out["cov"][q]).all()
        assert torch.isnan(out["contrib"][q]).all()
        assert (out["verdict"][q], out["count"][q], out["blame"][q], out["nvalid"][q]) == (-1, 0, 0, 0)
    for q, g in ((0, 0), (3, 1)):
        assert out["verdict"][q] == ref["verdict"][g] and out["blame"][q] == ref["blame"][g]
        within(out["d2"][q].cpu(), ref["d2"][g], ref["D"][KS[g]]["d2"], "d2", q)
    for k, v in full.items():
        assert (v[4] == SENTINEL[v.dtype]).all(), k
