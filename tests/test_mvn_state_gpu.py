"""The resident state form of the k-variate normal (ops/csrc/mvn_state.hip:
``kernels.mvn_fit_state`` at admission, ``kernels.mvn_state_detect`` every tick) against the
fp64 reference (models/multivariate_normal.py ``fit_mvn`` + ``mvn_state`` + ``score_state``),
and against ``kernels.mvn_groups`` on the same ring and window.

The reference of every case is built on the CPU, in float64, from the values as the ring
stores them (bf16-rounded, then upcast).  ``test_reference_keeps_clear_of_the_lines`` checks,
without a GPU, that no finite d2 of a scored group lies within 1 % of q_k(thr) and that on
the anomalous slots no contribution lies within 1 % of d2 of the naming line d2 / k, so that
demanding exact counts, verdicts, blame masks and anomaly lists of the kernel is fair.
SEED = 3 passes it (1 and 2 do not).

Bound on mean / cov / chol / d2 / contrib / score: the larger of the ``mvn_groups`` test's
tolerance (2e-3 relative + 1e-3) and 4 x D, D the distance between the reference formulas run
in float32 and in float64 on the CPU, measured per k and printed.  The same bound holds
between fit_state + state_detect and ``kernels.mvn_groups``."""

import functools

import numpy as np
import pytest
import torch

from foremast_amd.ingest.ringbuffer import HistoryRing
from foremast_amd.models import multivariate_normal as mvn

SEED = 3      # seeds 1 and 2 put a d2 within 1 % of a line (test_reference_keeps_clear_of_the_lines)
N, R, WIDE = 44, 1003, 17
MIN_VALID = 10
EPS = 1e-3
D2_TOL = dict(rtol=2e-3, atol=1e-3)   # tests/test_mvn_groups_gpu.py
BASE = [
    (1, 0),                             # 0  k = 2, descending; spikes in row 1 only
    (4, 3, 2),                          # 1  k = 3; rows 2 and 4 move against their correlation
    (5, 6, 7, 8, 9),                    # 2  k = 5; row 6 spikes
    (10, 11, 12, 13, 14, 15, 16, 17),   # 3  k = 8; row 12 alone, rows 15 / 16 in another slot
    (20, 21, 22),                       # 4  2 % NaN in every row
    (23, 24, 25),                       # 5  all-NaN row 24: nvalid 0
    (33, 32, 31, 30, 29, 28, 27, 26),   # 6  k = 8, descending, healthy
    (34, 35),                           # 7  row 35 has no pod in window slots 0 and 2: d2 NaN there
    (36, 37),                           # 8  exactly MIN_VALID jointly valid points; row 36 spikes: flagged
    (38, 39),                           # 9  one fewer: the same spike, verdict -1
    (5, 6, 9),                          # 10 shares rows with group 2
    (18,),                              # 11 a padded group of one row: NaN state, nothing read
    (2, N, 3),                          # 12 a row outside the ring: the same
    (40, 41, 19),                       # 13 row 19's window is empty: no slot scorable, verdict -1
]
LATENT = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 2] + [3] * 8 + [4, 4] + [5] * 3 + [6] * 3 + [7] * 8
                  + [8, 8, 9, 9, 10, 10, 11, 11, 4, 4])
SPIKES = ((1, (0, 3), 9.0), (2, (0, 2), 7.0), (4, (2,), -7.0), (6, (0, 2, 4), 12.0), (12, (0, 4), 10.0),
          (15, (1,), 7.0), (16, (1,), -7.0), (36, (0,), 9.0), (38, (0,), 9.0))
LENS = (R, R - 1, R - 37, 1)
HEADS = (0, 77, R - 5)


def groups_of(Ng):
    """``Ng`` groups cycling BASE, each with its window length: the lengths cycle LENS (13 and 4
    are coprime: over 67 groups nearly every base group meets every length); the two groups
    that pin nvalid at MIN_VALID keep the whole ring."""
    gs = [BASE[q % len(BASE)] for q in range(Ng)]
    ls = [R if q % len(BASE) in (8, 9) else LENS[q % 4] for q in range(Ng)]
    return gs, ls


def table(groups):
    t = np.full((len(groups), 8), -1, dtype=np.int32)
    for q, g in enumerate(groups):
        t[q, :len(g)] = g
    return t


def usable(g):
    return len(g) >= 2 and all(0 <= r < N for r in g)


@functools.lru_cache(maxsize=None)
def world():
    """Physical ring values [N, R], per-row thresholds and the windows [N, P, WIDE] for P = 1, 3."""
    assert len(LATENT) == N
    g = np.random.default_rng(SEED)
    lvl, sig = g.uniform(5, 50, N), g.uniform(0.5, 3, N)
    z = g.standard_normal((LATENT.max() + 1, R + WIDE))[LATENT]
    v = lvl[:, None] + sig[:, None] * (0.7 * z + 0.7 * g.standard_normal((N, R + WIDE)))
    hist = v[:, :R].astype(np.float32)
    for r in (20, 21, 22):
        hist[r, g.choice(R, R // 50, replace=False)] = np.nan
    hist[24] = np.nan
    for r, n in ((36, MIN_VALID), (38, MIN_VALID - 1)):
        keep = hist[r, 500:500 + n].copy()
        hist[r] = np.nan
        hist[r, 500:500 + n] = keep
    slot = v[:, R:].copy()
    for r, cols, k in SPIKES:
        slot[r, list(cols)] += k * sig[r]
    wins = {}
    for P in (1, 3):
        c = slot[:, None, :] + 0.1 * sig[:, None, None] * g.standard_normal((N, P, WIDE))
        if P == 3:
            c[1, 1, 0] = c[6, 0, 2] = c[12, 2, 0] = c[12, 0, 0] = np.nan   # a pod missing in some slots
        c[35, :, 0] = c[35, :, 2] = np.nan
        c[19] = np.nan
        wins[P] = c.astype(np.float32)
    thr = (3.0 + np.arange(N) % 3).astype(np.float32)
    return hist, thr, wins


def stored(dtype):
    h = torch.from_numpy(world()[0])
    return h.bfloat16().float() if dtype == "bf16" else h


def thr2_of(groups):
    thr = world()[1]
    return torch.tensor([mvn.chi2_threshold(float(thr[g[0]]), max(len(g), 1)) if usable(g) else 9.0 for g in groups],
                        dtype=torch.float32)


def fit_groups(dtype, head, groups, lens, dt):
    """The state of every group in ``dt``: fit in float64 on the logical window, cast, factorise."""
    Ng = len(groups)
    h = stored(dtype)
    o = dict(mean=torch.full((Ng, 8), float("nan"), dtype=dt), cov=torch.full((Ng, 36), float("nan"), dtype=dt),
             chol=torch.full((Ng, 36), float("nan"), dtype=dt), nvalid=torch.zeros(Ng))
    for q, (g, ln) in enumerate(zip(groups, lens)):
        if not usable(g):
            continue
        k = len(g)
        idx = (head + torch.arange(ln)) % R
        fit = mvn.fit_mvn(h[list(g)][:, idx].T[None].double())
        fit = mvn.MvnFit(fit.mean.to(dt), fit.cov.to(dt), fit.count)
        for name in ("mean", "cov", "chol"):
            o[name][q] = 0
        o["mean"][q, :k], o["cov"][q, :k * (k + 1) // 2] = fit.mean[0], fit.cov[0]
        o["chol"][q] = mvn.mvn_state(fit, EPS)[0]
        o["nvalid"][q] = float(fit.count[0])
    return o


def score_groups(st, groups, cm, thr2, dt):
    """``score_state`` of every group's state on the pod means ``cm [N, W]`` in ``dt``, padded like
    the kernel's outputs."""
    Ng, Wn = len(groups), cm.shape[1]
    o = dict(d2=torch.full((Ng, Wn), float("nan"), dtype=dt), contrib=torch.full((Ng, Wn, 8), float("nan"), dtype=dt),
             count=torch.zeros(Ng, dtype=torch.int32), verdict=torch.full((Ng,), -1, dtype=torch.int8),
             blame=torch.zeros(Ng, dtype=torch.int32), flag=torch.zeros(Ng, Wn, dtype=torch.bool),
             names=torch.zeros(Ng, Wn, 8, dtype=torch.bool), x=torch.zeros(Ng, Wn, 8))
    for q, g in enumerate(groups):
        if not usable(g):
            continue
        k = len(g)
        x = cm[list(g)].T[None]
        s = mvn.score_state(st["mean"][q:q + 1, :k].to(dt), st["chol"][q:q + 1].to(dt), st["nvalid"][q:q + 1],
                            x.to(dt), thr2[q:q + 1].to(dt), MIN_VALID)
        o["contrib"][q] = 0
        o["d2"][q], o["contrib"][q, :, :k], o["count"][q], o["verdict"][q] = s.d2[0], s.contrib[0], s.count[0], s.verdict[0]
        o["blame"][q], o["flag"][q], o["names"][q, :, :k], o["x"][q, :, :k] = s.blame[0], s.flag[0], s.names[0], x[0]
    valid = ~torch.isnan(o["d2"])
    o["score"] = torch.where(valid, o["d2"].clamp(min=0).sqrt(), torch.zeros_like(o["d2"])).amax(1)
    return o


@functools.lru_cache(maxsize=None)
def reference(dtype, head, Ng, uniform_len=None, P=1, Wn=WIDE):
    """fp64 state and scores of ``groups_of(Ng)`` (``uniform_len``: every group that length), and
    ``D``: per k and output, the largest distance of the float32 run of the same formulas over
    the groups with at least MIN_VALID points."""
    groups, lens = groups_of(Ng)
    if uniform_len is not None:
        lens = [uniform_len] * Ng
    cm = torch.nanmean(torch.from_numpy(world()[2][P][:, :, :Wn]), 1)
    thr2 = thr2_of(groups)
    ref = fit_groups(dtype, head, groups, lens, torch.float64)
    f32 = fit_groups(dtype, head, groups, lens, torch.float32)
    ref.update(score_groups(ref, groups, cm, thr2, torch.float64))
    f32.update(score_groups(f32, groups, cm, thr2, torch.float32))
    ref.update(groups=groups, lens=lens, thr2=thr2, D={})
    for k in sorted({len(g) for g in groups if usable(g)}):
        sel = torch.tensor([q for q, g in enumerate(groups)
                            if usable(g) and len(g) == k and ref["nvalid"][q] >= MIN_VALID], dtype=torch.long)
        ref["D"][k] = {}
        for name in ("mean", "cov", "chol", "d2", "contrib", "score"):
            e = (f32[name][sel].double() - ref[name][sel]).abs()
            e = e[torch.isfinite(e)]
            ref["D"][k][name] = float(e.max()) if e.numel() else 0.0
    return ref


FIT_CASES = [(dt, head, 67) for dt in ("fp32", "bf16") for head in HEADS] + [("bf16", 77, 1), ("fp32", 77, 5)]
DETECT_CASES = [(dt, Wn, P, ln) for dt, ln in (("fp32", R - 37), ("bf16", R)) for Wn in (1, 10, 17) for P in (1, 3)]


def test_reference_keeps_clear_of_the_lines():
    seen_k, seen_len = set(), set()
    for dt, Wn, P, ln in DETECT_CASES:
        ref = reference(dt, 77, 67, ln, P, Wn)
        scored = ref["nvalid"] >= MIN_VALID
        d2, thr2 = ref["d2"], ref["thr2"].double()[:, None].expand_as(ref["d2"])
        fin = torch.isfinite(d2) & scored[:, None]
        assert ((d2[fin] - thr2[fin]).abs() > 0.01 * thr2[fin]).all(), (dt, Wn, P)
        for q, g in enumerate(ref["groups"]):
            f = ref["flag"][q]
            c, line = ref["contrib"][q, f, :len(g)], d2[q, f] / len(g)
            assert ((c - line[:, None]).abs() > 0.01 * d2[q, f][:, None]).all(), (dt, Wn, P, q)
        v, nv = ref["verdict"].tolist(), ref["nvalid"].tolist()
        assert [v[q] for q in (0, 1, 2, 3, 8, 10)] == [1] * 6 and v[6] == 0 and v[4] == 0
        assert [v[q] for q in (5, 9, 11, 12, 13)] == [-1] * 5
        assert nv[5] == 0 and nv[8] == MIN_VALID and nv[9] == MIN_VALID - 1 and nv[11] == 0 and nv[12] == 0
        assert ref["blame"][0] == 0b01 and ref["blame"][3] & 0b100 and ref["blame"][8] & 0b01
        assert torch.isnan(d2[7, 0]) and torch.isnan(d2[13]).all() and torch.isfinite(d2[9]).all()
        if Wn >= 3:
            assert torch.isnan(d2[7, 2]) and torch.isfinite(d2[7, 1]) and ref["blame"][1] == 0b101
    for dt, head, Ng in FIT_CASES:
        ref = reference(dt, head, Ng)
        for g, ln in zip(ref["groups"], ref["lens"]):
            if usable(g):
                seen_k.add(len(g))
                seen_len.add(ln)
    assert seen_k == {2, 3, 5, 8} and seen_len == set(LENS)


def ring_of(dtype, dev, pad=None):
    """The ring on the device: a HistoryRing (rows padded to 16 bytes: the vector walk and its
    tail), or with ``pad`` extra columns per row a store whose rows are mostly unaligned."""
    hist = torch.from_numpy(world()[0])
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    if pad is None:
        ring = HistoryRing(N, R, tdt, dev)
        assert ring.ld == (1008 if dtype == "bf16" else 1004)
        ring.data.copy_(hist)
        return ring.data
    store = torch.full((N, R + pad), float("nan"), dtype=tdt, device=dev)
    store[:, :R].copy_(hist)
    data = store[:, :R]
    assert (data.stride(0) * data.element_size()) % 16 != 0
    return data


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


STATE_FILL = -12345.0
SENTINEL = {torch.float32: -12345.0, torch.int32: -77, torch.int8: -7}


def guarded_state(K, S, dev):
    """State tables of S + 1 rows filled with a sentinel, and the [:S] views handed to the kernels."""
    full = {k: torch.full((S + 1, w) if w else (S + 1,), STATE_FILL, device=dev) for k, w in K.MVN_STATE.items()}
    return full, {k: v[:S] for k, v in full.items()}


def dst_of(Ng):
    """A permutation with gaps: Ng distinct rows of 2 Ng + 3."""
    S = 2 * Ng + 3
    return S, np.random.default_rng(Ng).permutation(S)[:Ng].astype(np.int64)


def check_fit(got, ref, dst, S, full, worst):
    at = torch.from_numpy(dst)
    untouched = torch.ones(S + 1, dtype=torch.bool)
    untouched[at] = False
    for k, v in full.items():   # rows outside dst, and the row behind the tables, keep their bits
        assert (v.cpu()[untouched] == STATE_FILL).all(), k
    assert torch.equal(got["nvalid"][at], ref["nvalid"])
    for q, g in enumerate(ref["groups"]):
        d = int(dst[q])
        if not usable(g):
            assert all(torch.isnan(got[n][d]).all() for n in ("mean", "cov", "chol")) and got["nvalid"][d] == 0
            continue
        k = len(g)
        tri = k * (k + 1) // 2
        assert (got["mean"][d, k:] == 0).all() and (got["cov"][d, tri:] == 0).all() and (got["chol"][d, tri:] == 0).all()
        if ref["nvalid"][q] == 0:
            continue
        D = ref["D"][k]
        e = {"mean": within(got["mean"][d, :k], ref["mean"][q, :k], D["mean"], "mean", q),
             "cov": within(got["cov"][d, :tri], ref["cov"][q, :tri], D["cov"], "cov", q)}
        if ref["nvalid"][q] >= MIN_VALID:
            e["chol"] = within(got["chol"][d, :tri], ref["chol"][q, :tri], D["chol"], "chol", q)
        for name, val in e.items():
            worst.setdefault(k, {}).setdefault(name, 0.0)
            worst[k][name] = max(worst[k][name], val)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,head,Ng", FIT_CASES)
def test_fit_state_matches_reference(K, dtype, head, Ng):
    dev = torch.device("cuda:0")
    ref = reference(dtype, head, Ng)
    S, dst = dst_of(Ng)
    full, state = guarded_state(K, S, dev)
    out = K.mvn_fit_state(ring_of(dtype, dev), head, table(ref["groups"]), np.asarray(ref["lens"]), dst, state, eps=EPS)
    torch.cuda.synchronize()
    assert all(out[k].data_ptr() == state[k].data_ptr() for k in state)
    worst = {}
    check_fit({k: v.cpu() for k, v in state.items()}, ref, dst, S, full, worst)
    for k in sorted(worst):
        print(f"fit {dtype} head={head} k={k} D {({n: ref['D'][k][n] for n in ('mean', 'cov', 'chol')})}  "
              f"kernel max error {worst[k]}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,pad", [("fp32", 2), ("bf16", 2)])
def test_fit_state_on_unaligned_rows(K, dtype, pad):
    """Rows that do not start on 16 bytes take the scalar walk whatever their length; a group
    whose rows all happen to be aligned still takes the vector walk.  Device index tensors."""
    dev = torch.device("cuda:0")
    Ng, head = 67, 77
    ref = reference(dtype, head, Ng)
    S, dst = dst_of(Ng)
    full, state = guarded_state(K, S, dev)
    K.mvn_fit_state(ring_of(dtype, dev, pad), head, torch.from_numpy(table(ref["groups"])).to(dev),
                    torch.tensor(ref["lens"], dtype=torch.int32, device=dev),
                    torch.from_numpy(dst.astype(np.int32)).to(dev), state, eps=EPS)
    torch.cuda.synchronize()
    check_fit({k: v.cpu() for k, v in state.items()}, ref, dst, S, full, {})


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,Wn,P,length", DETECT_CASES)
def test_state_detect_matches_reference_and_mvn_groups(K, dtype, Wn, P, length):
    dev = torch.device("cuda:0")
    Ng, head = 67, 77
    ref = reference(dtype, head, Ng, length, P, Wn)
    groups = ref["groups"]
    S, dst = dst_of(Ng)
    full, state = guarded_state(K, S, dev)
    ring = ring_of(dtype, dev)
    K.mvn_fit_state(ring, head, table(groups), length, dst, state, eps=EPS)
    cur = torch.from_numpy(np.ascontiguousarray(world()[2][P][:, :, :Wn])).reshape(N, P * Wn).to(dev)
    rows = np.full((S, 8), -1, dtype=np.int32)
    rows[dst] = table(groups)
    thr2 = torch.full((S,), 1e-6)          # a live group reading another row's threshold would flag everything
    thr2[torch.from_numpy(dst)] = ref["thr2"]
    sel = np.array([q for q in range(Ng) if q % 5 != 3])[::-1].copy()     # a strict subset, out of order
    active = dst[sel]
    n = len(active)
    shapes = {"d2": ((n, Wn), torch.float32), "count": ((n,), torch.int32), "verdict": ((n,), torch.int8),
              "score": ((n,), torch.float32), "blame": ((n,), torch.int32), "contrib": ((n, Wn, 8), torch.float32)}
    guard = {k: torch.full((s[0] + 1,) + s[1:], SENTINEL[dt], dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    views = {k: v[:n] for k, v in guard.items()}
    before = {k: v.clone() for k, v in full.items()}
    ab = K.AnomalyBuffer(8 * n * Wn + 1, dev)
    ab.reset()
    ab.series.fill_(-7)
    out = K.mvn_state_detect(state, rows, thr2.to(dev), active, cur, P, Wn, min_valid=MIN_VALID, anomalies=ab,
                             contrib=True, out=views)
    # the fused launch on the same ring and window (a device table: rows are not range-checked)
    fused = K.mvn_groups(ring, head, length, torch.from_numpy(table([groups[q] for q in sel])).to(dev), cur, P, Wn,
                         torch.zeros(N, device=dev), thr2=ref["thr2"][torch.from_numpy(sel)].to(dev),
                         min_valid=MIN_VALID, eps=EPS, contrib=True)
    torch.cuda.synchronize()
    assert all(out[k].data_ptr() == views[k].data_ptr() for k in views)
    for k, v in guard.items():
        assert (v[n] == SENTINEL[v.dtype]).all(), k
    for k, v in full.items():   # the detect reads the state, it never writes it (bits: unusable groups hold NaN)
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
    got = {k: v.cpu() for k, v in out.items()}
    fz = {k: v.cpu() for k, v in fused.items()}
    qs = torch.from_numpy(sel)
    assert torch.equal(got["count"], ref["count"][qs]) and torch.equal(got["verdict"], ref["verdict"][qs])
    assert torch.equal(got["blame"], ref["blame"][qs])
    assert torch.equal(got["count"], fz["count"]) and torch.equal(got["verdict"], fz["verdict"])
    assert torch.equal(got["blame"], fz["blame"])
    worst = {}
    for j, q in enumerate(sel.tolist()):
        g = groups[q]
        if not usable(g):
            assert torch.isnan(got["d2"][j]).all() and torch.isnan(got["contrib"][j]).all() and got["score"][j] == 0
            continue
        k = len(g)
        assert (got["contrib"][j, :, k:] == 0).all()
        if ref["nvalid"][q] < MIN_VALID:
            assert torch.equal(torch.isnan(got["d2"][j]), torch.isnan(ref["d2"][q]))
            continue
        D = ref["D"][k]
        e = {"d2": within(got["d2"][j], ref["d2"][q], D["d2"], "d2", q),
             "contrib": within(got["contrib"][j, :, :k], ref["contrib"][q, :, :k], D["contrib"], "contrib", q),
             "score": within(got["score"][j], ref["score"][q], D["score"], "score", q),
             "d2 vs mvn_groups": within(got["d2"][j], fz["d2"][j], D["d2"], "d2 vs mvn_groups", q),
             "contrib vs mvn_groups": within(got["contrib"][j, :, :k], fz["contrib"][j, :, :k], D["contrib"],
                                             "contrib vs mvn_groups", q),
             "score vs mvn_groups": within(got["score"][j], fz["score"][j], D["score"], "score vs mvn_groups", q)}
        for name, val in e.items():
            worst.setdefault(k, {}).setdefault(name, 0.0)
            worst[k][name] = max(worst[k][name], val)
    for k in sorted(worst):
        print(f"detect {dtype} W={Wn} P={P} len={length} k={k} "
              f"D {({n_: ref['D'][k][n_] for n_ in ('d2', 'contrib', 'score')})}  kernel max error {worst[k]}")
    # the K9 list: one entry per anomalous slot and named metric, the metric's own row and pod mean
    names = ref["names"][qs].numpy()
    j, slot, i = np.nonzero(names)
    want = sorted(zip([groups[sel[a]][b] for a, b in zip(j, i)], slot.tolist(), ref["x"][qs].numpy()[j, slot, i].tolist()))
    s, c, v, overflow = ab.fetch()
    assert not overflow and int(ab.count.item()) == len(want) and len(want) >= 6
    gl = sorted(zip(s.tolist(), c.tolist(), v.tolist()))
    assert [a[:2] for a in gl] == [w[:2] for w in want]
    np.testing.assert_allclose([a[2] for a in gl], [w[2] for w in want], rtol=1e-6)
    assert (ab.series[len(want):] == -7).all()


@pytest.mark.gpu
def test_rejections_and_empty_launches(K):
    dev = torch.device("cuda:0")
    ring = ring_of("bf16", dev)
    state = K.mvn_state_tables(8, dev)
    t = table([BASE[0], BASE[1]])
    with pytest.raises(K.KernelShapeError):      # dst outside the tables
        K.mvn_fit_state(ring, 0, t, R, np.array([0, 8]), state)
    with pytest.raises(K.KernelShapeError):      # one dst per group
        K.mvn_fit_state(ring, 0, t, R, np.array([0]), state)
    with pytest.raises(K.KernelShapeError):      # a window longer than the ring
        K.mvn_fit_state(ring, 0, t, np.array([R, R + 1]), np.array([0, 1]), state)
    with pytest.raises(K.KernelShapeError):
        K.mvn_fit_state(ring, R, t, R, np.array([0, 1]), state)
    with pytest.raises(K.KernelShapeError):      # a group of nine rows
        K.mvn_fit_state(ring, 0, [list(range(9))], R, np.array([0]), state)
    with pytest.raises(K.KernelShapeError):      # int64 device indices
        K.mvn_fit_state(ring, 0, t, R, torch.tensor([0, 1], device=dev), state)
    with pytest.raises(K.KernelShapeError):      # a table missing
        K.mvn_fit_state(ring, 0, t, R, np.array([0, 1]), {k: v for k, v in state.items() if k != "chol"})
    with pytest.raises(K.KernelShapeError):      # a CPU table
        K.mvn_fit_state(ring, 0, t, R, np.array([0, 1]), dict(state, cov=state["cov"].cpu()))
    with pytest.raises(K.KernelShapeError):      # a strided table
        K.mvn_fit_state(ring, 0, t, R, np.array([0, 1]), dict(state, nvalid=torch.zeros(16, device=dev)[::2]))
    assert all(bool((v == 0).all()) for v in state.values())
    K.mvn_fit_state(ring, 0, np.zeros((0, 8), dtype=np.int32), R, np.zeros(0, dtype=np.int64), state)
    cur = torch.zeros((N, 3 * 5), device=dev)
    rows = np.full((8, 8), -1, dtype=np.int32)
    thr2 = torch.ones(8, device=dev)
    with pytest.raises(K.KernelShapeError):      # active outside the tables
        K.mvn_state_detect(state, rows, thr2, np.array([8]), cur, 3, 5)
    with pytest.raises(K.KernelShapeError):
        K.mvn_state_detect(state, rows, thr2, np.array([-1]), cur, 3, 5)
    with pytest.raises(K.KernelShapeError):      # one group row per state row
        K.mvn_state_detect(state, rows[:7], thr2, np.array([0]), cur, 3, 5)
    with pytest.raises(K.KernelShapeError):      # cur is [N, P * W]
        K.mvn_state_detect(state, rows, thr2, np.array([0]), cur, 3, 4)
    with pytest.raises(K.KernelShapeError):
        K.mvn_state_detect(state, rows, thr2[:7], np.array([0]), cur, 3, 5)
    with pytest.raises(K.KernelShapeError):
        K.mvn_state_detect(state, rows, thr2.double(), np.array([0]), cur, 3, 5)
    out = K.mvn_state_detect(state, rows, thr2, np.zeros(0, dtype=np.int64), cur, 3, 5, contrib=True)
    assert out["d2"].shape == (0, 5) and out["contrib"].shape == (0, 5, 8) and out["verdict"].shape == (0,)
    # a live state row without a group: unscored, nothing read
    out = K.mvn_state_detect(state, rows, thr2, np.array([3]), cur, 3, 5)
    torch.cuda.synchronize()
    assert torch.isnan(out["d2"]).all() and out["verdict"].tolist() == [-1] and out["count"].tolist() == [0]
