"""The k-variate normal scorer (models/multivariate_normal.py) on the CPU: the chi^2_k
threshold against scipy, k = 2 against the bivariate reference, the additive attribution,
the fit against numpy, the pivot floor, and the dispatch of ``ML_ALGORITHM=multivariate_normal``."""

import math

import numpy as np
import pytest
import torch

from foremast_amd.api import crd
from foremast_amd.api import rest as r
from foremast_amd.brain import plans as P
from foremast_amd.controller import queries
from foremast_amd.models import bivariate as biv_ref
from foremast_amd.models import multivariate_normal as mvn
from foremast_amd.service import app as svc
from foremast_amd.store import MemoryJobStore
from foremast_amd.utils.config import ALGORITHMS
from foremast_amd.utils.timeutil import format_rfc3339


def series(g, G, T, k, rho=0.7):
    """[G, T, k] float64: a shared latent load per group, correlation ~0.5 between metrics."""
    z = g.standard_normal((G, T, 1))
    lvl, sig = g.uniform(5, 50, (G, 1, k)), g.uniform(0.5, 3, (G, 1, k))
    return torch.from_numpy(lvl + sig * (rho * z + rho * g.standard_normal((G, T, k))))


@pytest.mark.parametrize("thr", [1, 2, 3, 5, 10])
@pytest.mark.parametrize("k", range(1, 9))
def test_chi2_threshold_against_scipy(thr, k):
    """1e-8 relative: the bisection runs until the float64 interval stops halving."""
    chi2 = pytest.importorskip("scipy.stats").chi2
    want = chi2.isf(math.erfc(thr / math.sqrt(2.0)), k)
    assert mvn.chi2_threshold(thr, k) == pytest.approx(want, rel=1e-8)


def test_chi2_threshold_reference_values():
    assert mvn.chi2_threshold(3, 1) == pytest.approx(9.0, rel=1e-8)
    assert mvn.chi2_threshold(3, 2) == pytest.approx(11.8292, abs=5e-5)
    assert mvn.chi2_threshold(3, 8) == pytest.approx(23.5746, abs=5e-5)
    # the threshold grows with k: the plain d^2 > thr^2 rule would not
    q = [mvn.chi2_threshold(3, k) for k in range(1, 9)]
    assert all(b > a for a, b in zip(q, q[1:]))


def test_k2_equals_the_bivariate_reference():
    g = np.random.default_rng(0)
    h = series(g, 6, 400, 2)
    h[1, 5:30, 0] = float("nan")
    h[2, 100, 1] = float("nan")
    x = h[:, :9] + torch.from_numpy(g.uniform(-6, 6, (6, 9, 2)))
    x[3, 4, 1] = float("nan")
    a, b = mvn.fit_mvn(h), biv_ref.fit_bivariate(h)
    assert a.mean.dtype == torch.float64
    torch.testing.assert_close(a.mean, b.mean, rtol=0, atol=0)
    torch.testing.assert_close(a.cov, b.cov, rtol=0, atol=0)
    torch.testing.assert_close(a.count, b.count, rtol=0, atol=0)
    d2, want = mvn.mahalanobis2_mvn(a, x), biv_ref.mahalanobis2(b, x)
    assert torch.isnan(d2[3, 4]) and torch.isnan(want[3, 4])
    torch.testing.assert_close(d2, want, rtol=1e-9, atol=0, equal_nan=True)
    # float32 windows come back as float32, like fit_bivariate
    assert mvn.fit_mvn(h.float()).cov.dtype == torch.float32
    assert mvn.mahalanobis2_mvn(mvn.fit_mvn(h.float()), x.float()).dtype == torch.float32


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_fit_against_numpy_cov(k):
    g = np.random.default_rng(k)
    h = series(g, 4, 300, k)
    h[0, g.choice(300, 25, replace=False), 0] = float("nan")
    h[1, 40:90, k - 1] = float("nan")
    h[2] = float("nan")
    fit = mvn.fit_mvn(h)
    assert fit.cov.shape == (4, k * (k + 1) // 2)
    for q in range(4):
        rows = h[q][~torch.isnan(h[q]).any(1)].numpy()
        assert fit.count[q] == len(rows)
        if not len(rows):
            assert (fit.mean[q] == 0).all() and (fit.cov[q] == 0).all()
            continue
        cov = np.cov(rows, rowvar=False, bias=True)
        np.testing.assert_allclose(fit.mean[q].numpy(), rows.mean(0), rtol=1e-12)
        packed = [cov[i, j] for i in range(k) for j in range(i + 1)]     # lower triangle, row-major
        np.testing.assert_allclose(fit.cov[q].numpy(), packed, rtol=1e-10, atol=1e-12)
    assert mvn.tri_index(0, 0) == 0 and mvn.tri_index(1, 0) == 1 and mvn.tri_index(7, 7) == 35
    with pytest.raises(ValueError):
        mvn.fit_mvn(h[..., :1])
    with pytest.raises(ValueError):
        mvn.fit_mvn(torch.zeros(1, 10, 9))


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_contributions_sum_to_d2_and_follow_a_permutation(k):
    g = np.random.default_rng(10 + k)
    h = series(g, 5, 500, k)
    x = h[:, :7] + torch.from_numpy(g.uniform(-8, 8, (5, 7, k)))
    x[1, 2, k - 1] = float("nan")
    fit = mvn.fit_mvn(h)
    d2, c = mvn.mahalanobis2_mvn(fit, x), mvn.contributions(fit, x)
    assert c.shape == (5, 7, k) and torch.isnan(c[1, 2]).all() and torch.isnan(d2[1, 2])
    torch.testing.assert_close(c.sum(2), d2, rtol=1e-12, atol=1e-12, equal_nan=True)
    # against the textbook formula on the full matrix
    q = 3
    full = torch.zeros(k, k, dtype=torch.float64)
    for i in range(k):
        for j in range(i + 1):
            full[i, j] = full[j, i] = fit.cov[q, mvn.tri_index(i, j)]
    dev = x[q] - fit.mean[q]
    w = torch.linalg.solve(full + 1e-9 * torch.eye(k, dtype=torch.float64), dev.T).T
    torch.testing.assert_close(c[q], dev * w, rtol=1e-9, atol=1e-12)
    perm = torch.from_numpy(g.permutation(k))
    fp = mvn.fit_mvn(h[..., perm])
    torch.testing.assert_close(mvn.mahalanobis2_mvn(fp, x[..., perm]), d2, rtol=1e-10, atol=1e-12, equal_nan=True)
    torch.testing.assert_close(mvn.contributions(fp, x[..., perm]), c[..., perm], rtol=1e-9, atol=1e-10,
                               equal_nan=True)


def test_pivot_floor_on_a_duplicated_row():
    """(r, r, s) without regularisation: the second pivot cancels to ~0 and is floored at
    1e-20, so d2 stays finite and non-negative; with a visible eps it is the regularised
    distance, equal for both copies."""
    g = np.random.default_rng(3)
    h3 = series(g, 2, 300, 2)
    h = torch.stack([h3[..., 0], h3[..., 0], h3[..., 1]], 2)
    x = h[:, :4] + 5.0
    fit = mvn.fit_mvn(h)
    L, inv = mvn.cholesky_packed(fit.cov, 3, 0.0)
    assert (L[1][1] <= 1e-7).all() and (L[1][1] >= math.sqrt(mvn.PIVOT_FLOOR) * (1 - 1e-12)).all()
    d2 = mvn.mahalanobis2_mvn(fit, x, eps=0.0)
    assert torch.isfinite(d2).all() and (d2 >= 0).all()
    d2r, c = mvn.mahalanobis2_mvn(fit, x, eps=1e-3), mvn.contributions(fit, x, eps=1e-3)
    assert torch.isfinite(d2r).all()
    torch.testing.assert_close(c[..., 0], c[..., 1], rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(c.sum(2), d2r, rtol=1e-10, atol=1e-10)


def test_verdict_and_attribution_rules():
    g = np.random.default_rng(4)
    k = 4
    h = series(g, 3, 600, k)
    fit = mvn.fit_mvn(h)
    sd = torch.stack([fit.cov[:, mvn.tri_index(i, i)].sqrt() for i in range(k)], 1)
    x = fit.mean[:, None, :].repeat(1, 3, 1)
    x[0, 1, 2] += 12 * sd[0, 2]                       # one metric only
    x[1, 0, 0] += 6 * sd[1, 0]
    x[1, 0, 3] -= 6 * sd[1, 3]                        # two metrics against their correlation
    x[2, 2, 1] = float("nan")
    thr2 = torch.full((3,), mvn.chi2_threshold(3, k))
    s = mvn.score_mvn(fit, x, thr2, min_valid=10)
    assert s.verdict.tolist() == [1, 1, 0] and s.count.tolist() == [1, 1, 0]
    assert s.blame.tolist() == [1 << 2, (1 << 0) | (1 << 3), 0]
    assert s.names[0, 1].tolist() == [False, False, True, False] and not s.names[0, 0].any()
    # too few points: unscored whatever the distance
    assert mvn.score_mvn(fit, x, thr2, min_valid=601).verdict.tolist() == [-1, -1, -1]
    # the largest contribution is always named, ties go to the first
    c = torch.tensor([[[1.0, 1.0, 1.0, 1.0]], [[0.2, 0.2, 0.5, 0.1]]])
    assert mvn.named(c, c.sum(2)).tolist() == [[[True] * 4], [[False, False, True, False]]]
    assert mvn.named(torch.tensor([[3.0, -1.0, 3.0, -1.0]]), torch.tensor([4.0])).tolist() == [[True, False, True, False]]


# ---------------------------------------------------------------------------- dispatch
def test_joint_kind_for_every_algorithm():
    assert "multivariate_normal" in ALGORITHMS and "multivariate_normal" in P.JOINT_ALGORITHMS
    assert "mvn" not in P.JOINT_SERVED
    for n in range(1, 10):
        assert P.joint_kind("multivariate_normal", n) == ("mvn" if n >= 2 else None)
        assert P.joint_kind("bivariate_normal", n) == ("biv" if n >= 2 else None)
        assert P.joint_kind("lstm", n) == ("lstm" if n >= 2 else None)
        assert P.joint_kind("auto", n) == (None if n < 2 else "biv" if n == 2 else "lstm")
        for algo in P.UNIVARIATE:
            assert P.joint_kind(algo, n) is None


T0 = 1_700_000_040.0
EP = "http://prometheus:9090/api/v1/"
METRICS = (("http_server_requests_error_5xx", "error5xx"), ("http_server_requests_latency", "latency"),
           ("http_server_requests_count", "count"))


def rollout_docs():
    store = MemoryJobStore()
    out = []
    for i, n in enumerate((1, 2, 3)):
        mets = crd.Metrics(data_source_type="prometheus", endpoint=EP,
                           monitoring=[crd.Monitoring(metric_name=m, metric_alias=a) for m, a in METRICS[:n]])
        app = f"mvn-app-{i}"
        info = queries.create_metrics_info("ns", app, [[f"{app}-v2-0"], [f"{app}-v1-0"]], mets, 10, "canary", now=T0)
        req = r.ApplicationHealthAnalyzeRequest(app_name=app, start_time=format_rfc3339(T0),
                                                end_time=format_rfc3339(T0 + 600), metrics=info,
                                                strategy="canary").to_dict()
        code, resp = svc.register(store, req)
        assert code == 200
        out.append(store.get(resp["jobId"]))
    return out


def test_plan_many_leaves_mvn_jobs_to_the_worker():
    docs = rollout_docs()
    got = P.plan_many(docs, "multivariate_normal")
    assert got[0] is not None and got[0].n == 1      # one metric: no joint model, the engine keeps it
    assert got[1] is None and got[2] is None         # "mvn" is not served by the resident engine
    assert all(p is not None for p in P.plan_many(docs, "bivariate_normal"))
