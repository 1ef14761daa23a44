"""The bivariate normal over row pairs of one ring (ops/csrc/bivariate_pairs.hip,
``kernels.bivariate_pairs``) against the fp64-accumulating reference (models/bivariate.py)
and against K8 (``kernels.bivariate``) on gathered copies of the same rows.

The reference of every case is built on the CPU from the values as the ring stores them
(bf16-rounded, then upcast); ``test_reference_keeps_clear_of_the_threshold`` checks, without
a GPU, that no finite d2 lies within 1 % of thr^2, so that demanding exact counts and
verdicts of the kernel is fair."""

import functools

import numpy as np
import pytest
import torch

from foremast_amd.ingest.ringbuffer import HistoryRing
from foremast_amd.models import bivariate as biv_ref

SEED = 11
N, R, W = 37, 1003, 5
MIN_VALID = 10
# (r, r) is singular under the default eps (1e-9 vanishes against an fp32 variance): the
# cases with that pair regularise the covariance visibly; the large-level test runs the default
EPS = 1e-3
D2_TOL = dict(rtol=2e-3, atol=1e-3)   # tests/test_kernels_gpu.py::test_bivariate_kernel
PAIRS = np.array([
    (0, 1), (3, 2),            # row0 > row1
    (4, 5), (4, 6),            # two pairs share row0 (both flagged)
    (7, 7),                    # (r, r)
    (8, 9),                    # isolated NaNs in one metric, a 60-point outage in the other
    (10, 11),                  # all-NaN row: verdict -1
    (12, 13),                  # fewer jointly valid points than min_valid: verdict -1
    (14, 15),                  # one metric NaN in a window slot: d2 NaN, not counted
    (16, 17),                  # all-NaN window
    (18, 19), (20, 21), (22, 23), (24, 25), (26, 27), (28, 29), (30, 31), (32, 33),
    (36, 34),
], dtype=np.int32)
RINGS = [(0, R), (1, R), (517, R), (1002, R), (600, 700), (37, 100)]   # (head, len)
CASES = [(dt, head, ln, P) for dt in ("bf16", "fp32") for head, ln in RINGS for P in (1, 3)]


@functools.lru_cache(maxsize=None)
def world():
    """Physical ring values [N, R], per-row thresholds and the windows [N, P, W] for P = 1, 3."""
    g = np.random.default_rng(SEED)
    lvl, sig = g.uniform(5, 50, N), g.uniform(0.5, 3, N)
    sig[7] = 1.0
    z = g.standard_normal((N // 2 + 1, R + W))[np.arange(N) // 2]     # rows 2k, 2k + 1 share a latent load
    v = lvl[:, None] + sig[:, None] * (0.7 * z + 0.7 * g.standard_normal((N, R + W)))
    hist = v[:, :R].astype(np.float32)
    hist[8, g.choice(R, 20, replace=False)] = np.nan
    hist[9, 400:460] = np.nan
    hist[10] = np.nan
    keep = hist[12, 40:46].copy()
    hist[12] = np.nan
    hist[12, 40:46] = keep
    slot = v[:, R:].copy()                                            # [N, W]
    for r, cols, k in ((0, (1, 3), 9.0), (4, (0, 2, 4), 12.0), (3, (2,), -9.0), (7, (0,), 8.0), (20, (4,), 10.0),
                       (36, (1,), 9.0)):
        slot[r, list(cols)] += k * sig[r]
    wins = {}
    for P in (1, 3):
        c = slot[:, None, :] + 0.1 * sig[:, None, None] * g.standard_normal((N, P, W))
        if P == 3:
            c[0, 1, 1] = c[5, 0, 2] = c[22, 2, 0] = c[22, 0, 0] = np.nan   # a pod missing in some slots
        c[14, :, 2] = np.nan
        c[16] = np.nan
        wins[P] = c.astype(np.float32)
    thr = (3.0 + np.arange(N) % 3).astype(np.float32)
    return hist, thr, wins


def stored(dtype):
    h = torch.from_numpy(world()[0])
    return h.bfloat16().float() if dtype == "bf16" else h


@functools.lru_cache(maxsize=None)
def reference(dtype, head, length, P, eps=EPS, pairs=None):
    """fp64-accumulating fit on the gathered logical rows, nanmean over pods, the verdict rule."""
    pr = torch.from_numpy(PAIRS if pairs is None else np.array(pairs, dtype=np.int32)).long()
    _, thr, wins = world()
    idx = (head + torch.arange(length)) % R
    h = stored(dtype)[:, idx]
    fit = biv_ref.fit_bivariate(torch.stack([h[pr[:, 0]], h[pr[:, 1]]], 2))
    cm = torch.nanmean(torch.from_numpy(wins[P]), 1)
    x = torch.stack([cm[pr[:, 0]], cm[pr[:, 1]]], 2)
    d2 = biv_ref.mahalanobis2(fit, x, eps=eps)
    thr2 = torch.from_numpy(thr)[pr[:, 0]] ** 2
    ok = fit.count >= MIN_VALID
    valid = ~torch.isnan(d2)
    flag = valid & ok[:, None] & (d2 > thr2[:, None])
    count = flag.sum(1).int()
    verdict = torch.where(count > 0, 1, torch.where(valid.any(1) & ok, 0, -1)).to(torch.int8)
    return dict(mean=fit.mean, cov=fit.cov, nvalid=fit.count, d2=d2, count=count, verdict=verdict, flag=flag,
                thr2=thr2, x0=x[..., 0])


def test_reference_keeps_clear_of_the_threshold():
    """No finite d2 of any case within 1 % of thr^2 (a seed that fails here would hide, or
    fake, a count mismatch on the GPU), and the cases hold what they are there for."""
    for case in CASES:
        ref = reference(*case)
        d2, thr2 = ref["d2"], ref["thr2"][:, None].expand_as(ref["d2"])
        fin = torch.isfinite(d2)
        assert ((d2[fin] - thr2[fin]).abs() > 0.01 * thr2[fin]).all(), case
        v = ref["verdict"].tolist()
        assert v[6] == -1 and v[7] == -1 and v[9] == -1, case                 # all-NaN row, few points, no window
        assert torch.isnan(d2[8, 2]) and torch.isnan(d2[9]).all(), case
        if case[2] == R:
            assert v[2] == 1 and v[3] == 1 and v[0] == 1 and v[8] in (0, 1), case
            assert R - 80 <= ref["nvalid"][5] < R - 60 and 0 < ref["nvalid"][7] < MIN_VALID


def device_inputs(dtype, P):
    dev = torch.device("cuda:0")
    hist, thr, wins = world()
    ring = HistoryRing(N, R, torch.bfloat16 if dtype == "bf16" else torch.float32, dev)
    assert ring.ld == (1008 if dtype == "bf16" else 1004)
    ring.data.copy_(torch.from_numpy(hist))
    cur = torch.from_numpy(wins[P]).reshape(N, P * W).to(dev)
    return dev, ring, cur, torch.from_numpy(thr).to(dev)


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,head,length,P", CASES)
def test_pairs_match_reference_and_k8(K, dtype, head, length, P):
    dev, ring, cur, thr = device_inputs(dtype, P)
    pairs = torch.from_numpy(PAIRS).to(dev)
    out = K.bivariate_pairs(ring.data, head, length, pairs, cur, P, W, thr, min_valid=MIN_VALID, eps=EPS)
    # K8 on gathered copies of the same rows (same padded stride) and the packed pod means
    hx = ring._store[pairs[:, 0].long()][:, :R]
    hy = ring._store[pairs[:, 1].long()][:, :R]
    cm = torch.nanmean(cur.view(N, P, W), 1)
    packed = torch.stack([cm[pairs[:, 0].long()], cm[pairs[:, 1].long()]], 2).contiguous()
    k8 = K.bivariate(hx, hy, head, length, packed, thr[pairs[:, 0].long()].contiguous(), min_valid=MIN_VALID, eps=EPS)
    torch.cuda.synchronize()
    ref = reference(dtype, head, length, P)
    got = {k: v.cpu() for k, v in out.items()}
    assert torch.equal(got["nvalid"], ref["nvalid"])
    ok = ref["nvalid"] > 0
    d2_err = (got["d2"] - ref["d2"]).abs()
    print("max |d2 - ref|", float(d2_err[torch.isfinite(d2_err)].max()), "max ref d2",
          float(ref["d2"][torch.isfinite(ref["d2"])].max()))
    torch.testing.assert_close(got["mean"][ok], ref["mean"][ok], **D2_TOL)
    torch.testing.assert_close(got["cov"][ok], ref["cov"][ok], **D2_TOL)
    torch.testing.assert_close(got["d2"][ok], ref["d2"][ok], equal_nan=True, **D2_TOL)
    assert torch.isnan(got["d2"][8, 2]) and torch.isnan(got["d2"][9]).all()
    assert torch.equal(got["count"], ref["count"])
    assert torch.equal(got["verdict"], ref["verdict"])
    score = torch.where(torch.isnan(ref["d2"]), torch.zeros(()), ref["d2"].clamp(min=0).sqrt()).amax(1)
    torch.testing.assert_close(got["score"][ok], score[ok], **D2_TOL)
    assert torch.equal(k8["verdict"].cpu(), got["verdict"]) and torch.equal(k8["count"].cpu(), got["count"])


@pytest.mark.gpu
def test_large_level_error_against_k8(K):
    """fp32 ring at level 1e4 with sigma 1: the shifted sums and the relative merge keep d2 as
    close to the fp64 reference as K8 does.  The factor 2 allows for the different summation
    order of two fp32 sums of the same length; it is not a measured property."""
    dev = torch.device("cuda:0")
    n, r = 16, 10080
    g = np.random.default_rng(5)
    z = g.standard_normal((n // 2, r + W))[np.arange(n) // 2]
    v = 1e4 + 0.7 * z + 0.7 * g.standard_normal((n, r + W))
    v[:, r:] += g.uniform(-4, 4, (n, W))
    ring = HistoryRing(n, r, torch.float32, dev)
    ring.data.copy_(torch.from_numpy(v[:, :r].astype(np.float32)))
    cur = torch.from_numpy(v[:, r:].astype(np.float32)).to(dev)
    pairs = torch.arange(n, dtype=torch.int32, device=dev).view(-1, 2)
    thr = torch.full((n,), 3.0, device=dev)
    out = K.bivariate_pairs(ring.data, 3, r, pairs, cur, 1, W, thr)
    packed = torch.stack([cur[0::2], cur[1::2]], 2).contiguous()
    k8 = K.bivariate(ring._store[0::2][:, :r], ring._store[1::2][:, :r], 3, r, packed, thr[0::2].contiguous())
    torch.cuda.synchronize()
    h64 = ring.data.cpu().double()
    fit = biv_ref.fit_bivariate(torch.stack([h64[0::2], h64[1::2]], 2))
    want = biv_ref.mahalanobis2(fit, packed.cpu().double())
    assert want.dtype == torch.float64
    err_new = float((out["d2"].cpu().double() - want).abs().max())
    err_k8 = float((k8["d2"].cpu().double() - want).abs().max())
    print(f"level 1e4: max |d2 - fp64|  pairs kernel {err_new:.3e}  K8 {err_k8:.3e}  (max d2 {float(want.max()):.1f})")
    assert err_new <= 2 * err_k8 + D2_TOL["atol"], (err_new, err_k8)


@pytest.mark.gpu
def test_state_effects(K):
    """A flagged pair raises its first row's verdict; the per-app anomalous counter moves once
    per row and tick, and not for a row the per-row pass flagged already."""
    dev, ring, cur, thr = device_inputs("bf16", 3)
    ref = reference("bf16", 517, R, 3)
    flagged = sorted({int(PAIRS[q, 0]) for q in np.nonzero(ref["verdict"].numpy() == 1)[0]})
    assert 4 in flagged and ref["verdict"][2] == 1 and ref["verdict"][3] == 1   # the shared row0, both pairs
    before = torch.zeros(N, dtype=torch.int8)
    before[1::4] = -1
    before[flagged[0]] = 1     # flagged by the per-row pass already: not counted again
    before[35] = 1             # no pair's first row
    assert before[4] == 0 and len(flagged) >= 4
    app_id = (torch.arange(N) % 3).int()
    stats = torch.zeros((3, 2), dtype=torch.int32)
    stats[:, 0] = torch.bincount(app_id[before == 1].long(), minlength=3).int()
    stats[:, 1] = 777
    verdict, stats_d = before.to(dev), stats.to(dev)
    out = K.bivariate_pairs(ring.data, 517, R, PAIRS, cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS,
                            verdict=verdict, app_id=app_id.to(dev), app_stats=stats_d)
    torch.cuda.synchronize()
    assert torch.equal(out["verdict"].cpu(), ref["verdict"])
    after = before.clone()
    after[flagged] = 1
    assert torch.equal(verdict.cpu(), after)
    want = torch.bincount(app_id[after == 1].long(), minlength=3).int()
    assert torch.equal(stats_d.cpu()[:, 0], want) and int(want.sum()) == int(stats[:, 0].sum()) + len(flagged) - 1
    assert (stats_d.cpu()[:, 1] == 777).all()


@pytest.mark.gpu
def test_anomaly_list(K):
    dev, ring, cur, thr = device_inputs("fp32", 3)
    ref = reference("fp32", 1, R, 3)
    q, slot = np.nonzero(ref["flag"].numpy())
    want = sorted(zip(PAIRS[q, 0].tolist(), slot.tolist(), ref["x0"].numpy()[q, slot].tolist()))
    assert len(want) >= 8
    ab = K.AnomalyBuffer(64, dev)
    ab.reset()
    K.bivariate_pairs(ring.data, 1, R, PAIRS, cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS, anomalies=ab)
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
    K.bivariate_pairs(ring.data, 1, R, PAIRS, cur, 3, W, thr, min_valid=MIN_VALID, eps=EPS, anomalies=ab)
    assert int(ab.count.item()) == len(want)
    assert (ab.series[3:] == -7).all() and (ab.col[3:] == -7).all() and (ab.val[3:] == -7.0).all()
    head = set(zip(ab.series[:3].tolist(), ab.col[:3].tolist()))
    assert len(head) == 3 and head <= {w[:2] for w in want}


@pytest.mark.gpu
def test_no_pairs_no_launch(K):
    dev, ring, cur, thr = device_inputs("bf16", 1)
    out = K.bivariate_pairs(ring.data, 0, R, np.zeros((0, 2), dtype=np.int32), cur, 1, W, thr)
    assert out["d2"].shape == (0, W) and out["mean"].shape == (0, 2) and out["cov"].shape == (0, 3)
    assert all(out[k].shape == (0,) for k in ("nvalid", "count", "verdict", "score"))
    with pytest.raises(K.KernelShapeError):
        K.bivariate_pairs(ring.data, 0, R, np.array([[0, N]]), cur, 1, W, thr)
