"""The state form of the k-variate normal (models/multivariate_normal.py ``mvn_state`` /
``score_state``) against ``score_mvn`` in float64, the ``FOREMAST_ROLLOUT_MVN`` switch, and the
``joint_served`` keyword of the rollout plans."""

import numpy as np
import pytest
import torch

from foremast_amd.api import crd
from foremast_amd.api import rest as r
from foremast_amd.brain import plans as P
from foremast_amd.controller import queries
from foremast_amd.deploy import manifests
from foremast_amd.models import multivariate_normal as mvn
from foremast_amd.service import app as svc
from foremast_amd.store import MemoryJobStore
from foremast_amd.utils.config import BrainConfig, reference_default_env
from foremast_amd.utils.timeutil import format_rfc3339


def series(g, G, T, k, rho=0.7):
    """[G, T, k] float64: a shared latent load per group, correlation ~0.5 between metrics."""
    z = g.standard_normal((G, T, 1))
    lvl, sig = g.uniform(5, 50, (G, 1, k)), g.uniform(0.5, 3, (G, 1, k))
    return torch.from_numpy(lvl + sig * (rho * z + rho * g.standard_normal((G, T, k))))


def assert_same(a: mvn.MvnScore, b: mvn.MvnScore):
    """d2 and contrib to 1e-12 relative, flags, names, counts, verdict and blame exactly."""
    torch.testing.assert_close(a.d2, b.d2, rtol=1e-12, atol=0.0, equal_nan=True)
    torch.testing.assert_close(a.contrib, b.contrib, rtol=1e-12, atol=0.0, equal_nan=True)
    assert torch.equal(a.flag, b.flag) and torch.equal(a.names, b.names)
    assert torch.equal(a.count, b.count) and torch.equal(a.verdict, b.verdict) and torch.equal(a.blame, b.blame)


def points(g, fit, k, C=6):
    """Current points around the mean: some inside, some far out, one with a missing coordinate."""
    sd = torch.stack([fit.cov[:, mvn.tri_index(i, i)].sqrt() for i in range(k)], 1)
    x = fit.mean[:, None, :] + sd[:, None, :] * torch.from_numpy(g.standard_normal((fit.mean.shape[0], C, k)))
    x[:, 1, 0] += 9 * sd[:, 0]
    x[:, 2, k - 1] -= 7 * sd[:, k - 1]
    x[0, 3, k // 2] = float("nan")
    return x


@pytest.mark.parametrize("k", range(2, 9))
def test_score_state_equals_score_mvn(k):
    g = np.random.default_rng(100 + k)
    h = series(g, 5, 400, k)
    h[1, ::7, 0] = float("nan")
    fit = mvn.fit_mvn(h)
    assert fit.mean.dtype == torch.float64
    x = points(g, fit, k)
    thr2 = torch.full((5,), mvn.chi2_threshold(3, k), dtype=torch.float64)
    chol = mvn.mvn_state(fit)
    assert chol.shape == (5, 36) and chol.dtype == torch.float64
    tri = k * (k + 1) // 2
    assert (chol[:, tri:] == 0).all()
    L, inv = mvn.cholesky_packed(fit.cov, k, 1e-9)
    for i in range(k):
        assert torch.equal(chol[:, mvn.tri_index(i, i)], inv[i])
        for j in range(i):
            assert torch.equal(chol[:, mvn.tri_index(i, j)], L[i][j])
    want = mvn.score_mvn(fit, x, thr2, min_valid=10)
    assert want.verdict.tolist() == [1] * 5 and want.count.min() >= 2   # the far points are flagged
    # the mean may arrive padded to 8 columns, as the engine's state tables keep it
    mean8 = torch.zeros((5, 8), dtype=torch.float64)
    mean8[:, :k] = fit.mean
    for mean in (fit.mean, mean8):
        assert_same(mvn.score_state(mean, chol, fit.count, x, thr2, 10), want)


def test_score_state_below_min_valid_is_unscored():
    g = np.random.default_rng(7)
    k = 4
    h = series(g, 3, 120, k)
    h[1, 59:] = float("nan")             # 59 jointly valid points: one below min_valid
    h[2, 60:] = float("nan")             # 60: exactly at it
    fit = mvn.fit_mvn(h)
    assert fit.count.tolist() == [120, 59, 60]
    x = points(g, fit, k)
    thr2 = torch.full((3,), mvn.chi2_threshold(3, k), dtype=torch.float64)
    want = mvn.score_mvn(fit, x, thr2, min_valid=60)
    got = mvn.score_state(fit.mean, mvn.mvn_state(fit), fit.count, x, thr2, 60)
    assert_same(got, want)
    assert got.verdict.tolist() == [1, -1, 1] and got.count[1] == 0 and got.blame[1] == 0
    assert torch.isfinite(got.d2[1]).all()   # the distance is still reported


def test_score_state_on_a_duplicated_row_and_at_the_pivot_floor():
    g = np.random.default_rng(3)
    h3 = series(g, 2, 300, 2)
    h = torch.stack([h3[..., 0], h3[..., 0], h3[..., 1]], 2)
    x = h[:, :4] + 5.0
    fit = mvn.fit_mvn(h)
    thr2 = torch.full((2,), mvn.chi2_threshold(3, 3), dtype=torch.float64)
    # a visible eps: the regularised distance
    chol = mvn.mvn_state(fit, eps=1e-3)
    assert_same(mvn.score_state(fit.mean, chol, fit.count, x, thr2, 10), mvn.score_mvn(fit, x, thr2, 10, eps=1e-3))
    # no regularisation: the second pivot cancels and is floored, the state holds 1 / sqrt(floor)
    chol0 = mvn.mvn_state(fit, eps=0.0)
    L, inv = mvn.cholesky_packed(fit.cov, 3, 0.0)
    assert (L[1][1] <= 1e-7).all()
    assert torch.equal(chol0[:, mvn.tri_index(1, 1)], inv[1]) and torch.isfinite(chol0).all()
    got = mvn.score_state(fit.mean, chol0, fit.count, x, thr2, 10)
    assert_same(got, mvn.score_mvn(fit, x, thr2, 10, eps=0.0))
    assert torch.isfinite(got.d2).all() and (got.d2 >= 0).all()


def test_score_state_rejects_k_outside_2_to_8():
    with pytest.raises(ValueError):
        mvn.score_state(torch.zeros(1, 8), torch.zeros(1, 36), torch.ones(1), torch.zeros(1, 2, 1), torch.ones(1), 0)


# ---------------------------------------------------------------------------- the switch
def test_rollout_mvn_switch_parses_and_is_listed():
    env = reference_default_env()
    assert BrainConfig.from_env(env).rollout_mvn is False
    assert BrainConfig.from_env(dict(env, FOREMAST_ROLLOUT_MVN="0")).rollout_mvn is False
    assert BrainConfig.from_env(dict(env, FOREMAST_ROLLOUT_MVN="1")).rollout_mvn is True
    for bad in ("2", "true", "yes", "on"):
        with pytest.raises(ValueError, match="FOREMAST_ROLLOUT_MVN"):
            BrainConfig.from_env(dict(env, FOREMAST_ROLLOUT_MVN=bad))
    envs = manifests.brain()[0]["spec"]["template"]["spec"]["containers"][0]["env"]
    assert {"name": "FOREMAST_ROLLOUT_MVN", "value": "0"} in envs


# ---------------------------------------------------------------------------- plans
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


def test_plans_serve_mvn_jobs_only_when_asked():
    docs = rollout_docs()
    assert "mvn" not in P.JOINT_SERVED
    served = P.JOINT_SERVED + ("mvn",)
    # asked first: the memo must not remember the wider filter
    got = P.plan_many(docs, "multivariate_normal", joint_served=served)
    assert [p.n for p in got] == [1, 2, 3]
    got = P.plan_many(docs, "multivariate_normal")
    assert got[0] is not None and got[0].n == 1
    assert got[1] is None and got[2] is None
    assert all(p is not None for p in P.plan_many(docs, "multivariate_normal", joint_served=served))
    assert P.plan_rollout(docs[2], "multivariate_normal") is None
    assert P.plan_rollout(docs[2], "multivariate_normal", joint_served=served).n == 3
    # the switch selects the filter
    env = reference_default_env()
    off = BrainConfig.from_env(dict(env, ML_ALGORITHM="multivariate_normal"))
    on = BrainConfig.from_env(dict(env, ML_ALGORITHM="multivariate_normal", FOREMAST_ROLLOUT_MVN="1"))
    assert P.joint_served_for(off) == P.JOINT_SERVED and P.joint_served_for(on) == served
