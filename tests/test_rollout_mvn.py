"""Multi-metric canary jobs under ``ML_ALGORITHM=multivariate_normal`` on the resident engine
(``FOREMAST_ROLLOUT_MVN=1``; brain/rollout.py ``_fit_mvn`` / ``_score_mvn``): the k x k state is
fitted once at admission on the resident history and scored every tick on the pod-mean current
values; verdicts and named aliases equal the per-job BrainWorker's on the same data.

The world: metric j of an app is ``10 + 5 j + 3 u(t) + 0.05 noise_j(t)`` with one latent load u
shared by the app's metrics; u is hash noise before T0 and alternates +1.5 / -1.5 per minute
from T0 on, so every metric alone stays within 1.5 sigma of its own history.  On the new pods
of a broken app one metric moves against the load (``-3 u``) from BREAK_AT on: d² jumps from
single digits to > 2e4 and the broken metric carries half of it, the others well below 1/k
(k >= 3).  At k = 2 the two shares are 0.499 / 0.501, so only "some alias is named" is checked."""

import asyncio
import functools
import json
import logging

import httpx
import numpy as np
import pytest
import torch

from foremast_amd.api import crd
from foremast_amd.api import rest as r
from foremast_amd.brain.batch import BatchScorer
from foremast_amd.brain.rollout import RolloutMonitor, is_rollout_keyable
from foremast_amd.brain.worker import BrainWorker
from foremast_amd.controller import queries
from foremast_amd.promql.client import PromClient
from foremast_amd.promql.fake import FakePrometheus
from foremast_amd.promql.synth import _hash_noise
from foremast_amd.service import app as svc
from foremast_amd.store import MemoryJobStore
from foremast_amd.utils.config import BrainConfig, reference_default_env
from foremast_amd.utils.metrics import BrainMetrics
from foremast_amd.utils.timeutil import format_rfc3339

T0 = 1_700_000_040.0
NS = "ns"
EP = "http://prometheus:9090/api/v1/"
BREAK_AT = T0 + 180
TICKS = (T0 + 120, T0 + 240, T0 + 360, T0 + 660)


def metrics(n):
    return tuple((f"http_server_signal_{j}", f"sig{j}") for j in range(n))


# app -> (number of metrics, index of the broken sorted alias or None)
APPS = {"m3": (3, 2), "m4": (4, 0), "m9": (9, 7), "m2": (2, 1), "ok3": (3, None), "one": (1, None)}


class Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def request(app, new, old, mets, strategy="canary"):
    m = crd.Metrics(data_source_type="prometheus", endpoint=EP,
                    monitoring=[crd.Monitoring(metric_name=n, metric_alias=a) for n, a in mets])
    info = queries.create_metrics_info(NS, app, [list(new), list(old)], m, 10, strategy, now=T0)
    return r.ApplicationHealthAnalyzeRequest(app_name=app, start_time=format_rfc3339(T0),
                                             end_time=format_rfc3339(T0 + 600), metrics=info,
                                             strategy=strategy).to_dict()


def load(ts, seed):
    """The app's latent load: hash noise before T0, then +1.5 / -1.5 alternating per minute."""
    alt = np.where(np.round((ts - T0) / 60.0).astype(np.int64) % 2 == 0, 1.5, -1.5)
    return np.where(ts < T0, _hash_noise(ts, seed), alt)


def signal(seed, j, flip_after=None, pod_seed=0):
    def f(ts):
        ts = np.asarray(ts, dtype=np.float64)
        u = load(ts, seed)
        sign = np.where(ts >= flip_after, -1.0, 1.0) if flip_after is not None else 1.0
        return 10.0 + 5.0 * j + 3.0 * sign * u + 0.05 * _hash_noise(ts, seed + 1000 * (j + 1) + pod_seed)
    return f


def world():
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    store = MemoryJobStore()
    ids = {}
    for i, (app, (n, broken)) in enumerate(APPS.items()):
        new, old = [f"{app}-v2-{k}" for k in range(2)], [f"{app}-v1-{k}" for k in range(3)]
        for j, (m, _a) in enumerate(metrics(n)):
            prom.add("namespace_app_per_pod:" + m, {"namespace": NS, "app": app}, signal(100 * i, j))
            for k, pod in enumerate(new + old):
                brk = BREAK_AT if (broken == j and pod in new) else None
                prom.add("namespace_pod:" + m, {"namespace": NS, "pod": pod}, signal(100 * i, j, brk, pod_seed=k + 1))
        ids[app] = svc.register(store, request(app, new, old, metrics(n)))[1]["jobId"]
    return clock, prom, store, ids


def config(switch="1"):
    env = reference_default_env()
    env.update(MIN_HISTORICAL_DATA_POINT_TO_MEASURE="10", ML_ALGORITHM="multivariate_normal",
               ML_PAIRWISE_ALGORITHM="none", threshold="4", threshold0="4", threshold1="4", threshold2="4",
               FOREMAST_ROLLOUT_MVN=switch)
    return BrainConfig.from_env(env)


def _run_resident(device):
    clock, prom, store, ids = world()
    cfg = config()
    assert all(is_rollout_keyable(store.get(j), cfg) for j in ids.values())
    mon = RolloutMonitor(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                         device=torch.device(device), metrics=BrainMetrics(), window=10, pods=5, clock=clock,
                         ring_len=2880, min_capacity=4)
    assert mon.mvn
    seen = {}

    async def go():
        mon.sync()
        await mon.tick()
        seen["groups"] = int((mon.mvn_k > 0).sum())
        seen["k"] = sorted(mon.mvn_k[mon.mvn_k > 0].tolist())
        for t in TICKS:
            clock.t = t
            mon.sync()
            await mon.tick()
    asyncio.run(go())
    return {app: store.get(j) for app, j in ids.items()}, mon, seen


@functools.lru_cache(maxsize=None)
def resident_cpu():
    return _run_resident("cpu")


@functools.lru_cache(maxsize=None)
def worker_docs():
    clock, prom, store, ids = world()
    cfg = config()
    w = BrainWorker(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                    scorer=BatchScorer(cfg, device=torch.device("cpu")), worker_id="w", clock=clock)

    async def go():
        for t in TICKS:
            clock.t = t
            await w.cycle()
    asyncio.run(go())
    return {app: store.get(j) for app, j in ids.items()}


def named(doc):
    return set(json.loads(doc["anomalyInfo"])) if doc.get("anomalyInfo") else set()


def test_switch_off_leaves_multi_metric_jobs_to_the_worker():
    _clock, _prom, store, ids = world()
    off = config("0")
    assert not off.rollout_mvn
    for app, (n, _b) in APPS.items():
        assert is_rollout_keyable(store.get(ids[app]), off) == (n == 1), app
    mon = RolloutMonitor(store, off, prom=PromClient(transport=httpx.ASGITransport(app=FakePrometheus().asgi_app())),
                         device=torch.device("cpu"), metrics=BrainMetrics(), window=10, pods=5, clock=Clock(T0),
                         ring_len=2880, min_capacity=4)
    assert not mon.mvn
    assert mon._claimable_many([store.get(ids[a]) for a in APPS]) == [n == 1 for n, _b in APPS.values()]


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_mvn_rollout_matches_worker(device, caplog):
    if device == "cpu":
        resident_cpu.cache_clear()
        with caplog.at_level(logging.WARNING, logger="foremast.rollout"):
            docs, mon, seen = resident_cpu()
    else:
        with caplog.at_level(logging.WARNING, logger="foremast.rollout"):
            docs, mon, seen = _run_resident(device)
    ref = worker_docs()
    # one group per multi-metric job, the 9-metric job truncated to its first 8 sorted aliases
    assert seen["groups"] == 5 and seen["k"] == [2, 3, 3, 4, 8]
    warned = [rec.getMessage() for rec in caplog.records
              if rec.name == "foremast.rollout" and "multivariate_normal models the first 8" in rec.getMessage()]
    assert len(warned) == 1 and "has 9 metrics" in warned[0] and "sig8" not in warned[0].split("(")[-1]
    for app, (n, broken) in APPS.items():
        d = docs[app]
        assert "resident engine" in d["processingContent"], app
        if broken is None:
            assert d["status"] == r.ST_COMPLETED_HEALTH, (app, d.get("reason"))
            continue
        assert d["status"] == r.ST_COMPLETED_UNHEALTH, (app, d.get("reason"))
        info = json.loads(d["anomalyInfo"])
        if n >= 3:
            assert set(info) == {f"sig{broken}"}, (app, sorted(info))
        else:
            assert len(info) >= 1 and set(info) <= {"sig0", "sig1"}
        for alias, a in info.items():
            assert a["tags"] == "" and min(a["values"][0::2]) >= BREAK_AT, (app, alias)
    # the per-job worker on the same world
    for app in APPS:
        assert docs[app]["status"] == ref[app]["status"], app
        assert "resident engine" not in (ref[app].get("processingContent") or "")
        if APPS[app][0] != 2:
            assert named(docs[app]) == named(ref[app]), app
        got, want = json.loads(docs[app].get("anomalyInfo") or "{}"), json.loads(ref[app].get("anomalyInfo") or "{}")
        for alias in set(got) & set(want):
            gv, wv = np.array(got[alias]["values"]), np.array(want[alias]["values"])
            # the worker scores at its own cycle times: the resident points are the ones it saw
            gp = dict(zip(gv[0::2].tolist(), gv[1::2].tolist()))
            wp = dict(zip(wv[0::2].tolist(), wv[1::2].tolist()))
            common = sorted(set(gp) & set(wp))
            assert common, (app, alias)
            np.testing.assert_allclose([gp[t] for t in common], [wp[t] for t in common], rtol=1e-5)
    if device != "cpu":   # GPU and CPU engines agree
        cpu_docs, _mon, _seen = resident_cpu()
        for app in APPS:
            assert docs[app]["status"] == cpu_docs[app]["status"], app
            if APPS[app][0] != 2:
                assert named(docs[app]) == named(cpu_docs[app]), app
    # nothing is left behind
    assert not mon.jobs and not (mon.mvn_k > 0).any() and (mon.mvn_rows_h < 0).all()
    assert bool((mon.mvn_rows < 0).all())


def test_world_separates_the_joint_model_from_the_per_metric_rows():
    """The fp64 reference on the world itself (2880 history points, the 10 slots, the mean of
    the 2 new pods, threshold 4): healthy slots far below q_k(4), broken slots far above, the
    broken metric with half of d² and every other at least 2 % of d² under the naming line
    d²/k (k >= 3), and no metric alone beyond 2 sigma of its own history, half the threshold."""
    from foremast_amd.models import multivariate_normal as mvn
    hts = T0 - 60.0 * np.arange(2880, 0, -1)
    cts = T0 + 60.0 * np.arange(1, 11)
    brk = cts >= BREAK_AT
    for i, (app, (n, broken)) in enumerate(APPS.items()):
        k = min(n, 8)
        if k < 2:
            continue
        h = np.stack([signal(100 * i, j)(hts) for j in range(k)], 1)
        x = np.stack([np.mean([signal(100 * i, j, BREAK_AT if broken == j else None, pod_seed=p + 1)(cts)
                               for p in range(2)], 0) for j in range(k)], 1)
        fit = mvn.fit_mvn(torch.from_numpy(h)[None])
        q = mvn.chi2_threshold(4.0, k)
        s = mvn.score_mvn(fit, torch.from_numpy(x)[None], torch.tensor([q], dtype=torch.float64), 10)
        d2, c = s.d2[0].numpy(), s.contrib[0].numpy()
        sd = np.sqrt([float(fit.cov[0, mvn.tri_index(j, j)]) for j in range(k)])
        assert (np.abs(x - fit.mean[0].numpy()) / sd).max() < 2.0, app
        healthy = d2 if broken is None else d2[~brk]
        assert healthy.max() < 0.5 * q, (app, healthy.max(), q)
        if broken is None:
            continue
        assert d2[brk].min() > 1e4 > 100 * q, (app, d2[brk].min())
        share = c[brk] / d2[brk][:, None]
        assert np.abs(share[:, broken] - 0.5).max() < 0.05, app
        if k >= 3:
            assert np.delete(share, broken, 1).max() < 1.0 / k - 0.02, app
            assert s.names[0].numpy()[brk].tolist() == [[j == broken for j in range(k)]] * int(brk.sum()), app
