"""The three-app rollout scenario of tests/test_rollout.py as a helper (a copy of its small
world / config functions, with the engine's ring length and the algorithm as parameters):
apps ``a`` (canary, its new pods' error rate jumps at ``spike_at``), ``b`` (rollingUpdate)
and ``c`` (canary) on a fake Prometheus, registered as jobs in a memory store."""

from __future__ import annotations

import asyncio

import httpx
import torch

from foremast_amd.api import crd
from foremast_amd.api import rest as r
from foremast_amd.brain.batch import BatchScorer
from foremast_amd.brain.rollout import RolloutMonitor
from foremast_amd.brain.worker import BrainWorker
from foremast_amd.controller import queries
from foremast_amd.promql import synth
from foremast_amd.promql.client import PromClient
from foremast_amd.promql.fake import FakePrometheus
from foremast_amd.service import app as svc
from foremast_amd.store import MemoryJobStore
from foremast_amd.utils.config import BrainConfig, reference_default_env
from foremast_amd.utils.metrics import BrainMetrics
from foremast_amd.utils.timeutil import format_rfc3339

T0 = 1_700_000_040.0  # aligned to the minute
NS = "ns"
METRICS = (("http_server_requests_error_5xx", "error5xx"), ("http_server_requests_latency", "latency"))


class Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def request(app, new_pods, old_pods, strategy, now=T0, metrics=METRICS):
    mets = crd.Metrics(data_source_type="prometheus", endpoint="http://prometheus:9090/api/v1/",
                       monitoring=[crd.Monitoring(metric_name=m, metric_alias=a) for m, a in metrics])
    info = queries.create_metrics_info(NS, app, [list(new_pods), list(old_pods)], mets, 10, strategy, now=now)
    return r.ApplicationHealthAnalyzeRequest(app_name=app, start_time=format_rfc3339(now),
                                             end_time=format_rfc3339(now + 600), metrics=info,
                                             strategy=strategy).to_dict()


def world(spike_app="a", spike_at=T0 + 120, metrics=METRICS):
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    apps = {"a": "canary", "b": "rollingUpdate", "c": "canary"}
    pods = {}
    for i, app in enumerate(apps):
        new, old = [f"{app}-v2-{k}" for k in range(2)], [f"{app}-v1-{k}" for k in range(3)]
        pods[app] = (new, old)
        for j, (m, _a) in enumerate(metrics):
            base = 0.3 + 0.1 * i + j
            prom.add("namespace_app_per_pod:" + m, {"namespace": NS, "app": app},
                     synth.error_rate(base=base, spread=0.05, seed=10 * i + j))
            for k, pod in enumerate(new + old):
                gen = synth.error_rate(base=base, spread=0.05, seed=100 + 10 * i + k + 50 * j)
                if app == spike_app and pod in new and j == 0:
                    gen = synth.step_change(gen, at=spike_at, factor=0.0, add=40.0)
                prom.add("namespace_pod:" + m, {"namespace": NS, "pod": pod}, gen)
    store = MemoryJobStore()
    ids = {app: svc.register(store, request(app, *pods[app], strategy))[1]["jobId"] for app, strategy in apps.items()}
    return clock, prom, store, ids


def config(algorithm="moving_average_all"):
    env = reference_default_env()
    env.update(MIN_HISTORICAL_DATA_POINT_TO_MEASURE="10", threshold0="4", threshold1="4", ML_ALGORITHM=algorithm)
    return BrainConfig.from_env(env)


def client(prom):
    return PromClient(transport=httpx.ASGITransport(app=prom.asgi_app()))


def monitor(store, prom, clock, device, cfg, ring_len=2880, **kw):
    return RolloutMonitor(store, cfg, prom=client(prom), device=torch.device(device),
                          metrics=kw.pop("metrics", BrainMetrics()), window=10, pods=5, clock=clock,
                          ring_len=ring_len, min_capacity=4, **kw)


def run_monitor(device, algorithm, ring_len=2880, ticks=(T0 + 120, T0 + 300)):
    """The scenario on the resident engine: ticks at T0 (admission), ``ticks``, and T0 + 660
    (every job past its end).  Returns (statuses written per tick, final documents per app,
    job ids, the monitor, history queries right after admission and at the end)."""
    clock, prom, store, ids = world()
    mon = monitor(store, prom, clock, device, config(algorithm), ring_len=ring_len)
    out, hq = {}, {}

    async def go():
        assert mon.sync() == 3
        w = await mon.tick()
        assert w == {} and len(mon.jobs) == 3 and mon.n_live == 6
        hq["admitted"] = mon.history.history_queries
        for t in ticks:
            clock.t = t
            out[t] = dict(await mon.tick())
        clock.t = T0 + 660
        out["end"] = dict(await mon.tick())
        hq["end"] = mon.history.history_queries
    asyncio.run(go())
    docs = {app: store.get(j) for app, j in ids.items()}
    return out, docs, ids, mon, hq


def run_worker(algorithm):
    """The same jobs and data through the per-job BrainWorker + BatchScorer on the CPU."""
    clock, prom, store, ids = world()
    cfg = config(algorithm)
    worker = BrainWorker(store, cfg, prom=client(prom), scorer=BatchScorer(cfg, device=torch.device("cpu")),
                         worker_id="w", clock=clock)

    async def go():
        for t in (T0 + 120, T0 + 300, T0 + 660):
            clock.t = t
            await worker.cycle()
    asyncio.run(go())
    return {app: store.get(j) for app, j in ids.items()}
