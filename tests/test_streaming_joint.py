"""Continuous two-metric jobs on the streaming engine (brain/streaming.py pair table,
brain/engine.py ``set_pairs``, ops/csrc/bivariate_pairs.hip): under ``ML_ALGORITHM``
bivariate_normal / auto the job keeps its per-metric rows (moving_average_all) and gets
the joint bivariate normal of ``docs/guides/design.md:78`` over the rows of its first two
aliases, refitted from the ring and scored on the pod-mean window every tick."""

import asyncio
import json

import httpx
import numpy as np
import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.brain.batch import BatchScorer
from foremast_amd.brain.streaming import StreamingMonitor
from foremast_amd.brain.worker import BrainWorker
from foremast_amd.models import bivariate as biv_ref
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
FAMILY = "namespace_app_per_pod:"
M2 = (("http_server_requests_error_5xx", "error5xx"), ("http_server_requests_latency", "latency"))
M3 = M2 + (("http_server_requests_error_4xx", "error4xx"),)
APPS = {"a": M2, "b": M2, "c": M2[:1], "d": M3}   # a: correlation breaks; b: healthy; c: 1 metric; d: 3
BREAK_AT = T0 + 180
END = T0 + 600
TICKS = (T0, T0 + 120, T0 + 240, T0 + 360, T0 + 660)
R, W = 2880, 5
D2_TOL = dict(rtol=2e-3, atol=1e-3)  # tests/test_kernels_gpu.py::test_bivariate_kernel


class Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def correlated(seed, j, flip_after=None):
    """Metric j of an app: a shared latent load u(t) drives every metric (error rate
    10 + 3u, latency 20 + 6u, ...), with a little independent noise.  After
    ``flip_after`` the latency moves against the load (20 - 6u): each metric alone
    stays inside its usual range, the pair does not."""
    lvl, amp = (10.0, 3.0) if j == 0 else (20.0 + 5 * j, 6.0)

    def f(ts):
        ts = np.asarray(ts, dtype=np.float64)
        u = _hash_noise(ts, seed)
        v = lvl + amp * u + 0.05 * _hash_noise(ts, seed + 1000 * (j + 1))
        if flip_after is not None and j == 1:
            v = np.where(ts >= flip_after, lvl - amp * u + 0.05 * _hash_noise(ts, seed + 77), v)
        return v
    return f


def generator(app, j):
    i = sorted(APPS).index(app) if app in APPS else 4 + ord(app) - ord("e")
    return correlated(10 * i, j, BREAK_AT if app == "a" else None)


def job(name, app, mets, end=END):
    cur, hist = {}, {}
    for m, alias in mets:
        params = {"endpoint": EP, "query": f'{FAMILY}{m}{{namespace="{NS}",app="{app}"}}', "step": 60}
        cur[alias] = {"dataSourceType": "prometheus", "parameters": dict(params, start=int(T0), end=int(end))}
        hist[alias] = {"dataSourceType": "prometheus",
                       "parameters": dict(params, start=int(T0 - 2 * 86400), end=int(T0))}
    return {"appName": name, "startTime": format_rfc3339(T0), "endTime": format_rfc3339(end),
            "strategy": "continuous", "metrics": {"current": cur, "historical": hist}}


def world(extra_apps=()):
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    store = MemoryJobStore()
    ids = {}
    for app, mets in list(APPS.items()) + [(a, M2) for a in extra_apps]:
        for j, (m, _alias) in enumerate(mets):
            prom.add(FAMILY + m, {"namespace": NS, "app": app}, generator(app, j))
    for app, mets in APPS.items():
        ids[app] = svc.register(store, job(app, app, mets))[1]["jobId"]
    ids["a2"] = svc.register(store, job("a-again", "a", M2))[1]["jobId"]   # a second job on a's two series
    assert len(set(ids.values())) == len(ids)
    return clock, prom, store, ids


def config(algorithm):
    env = reference_default_env()
    env.update(MIN_HISTORICAL_DATA_POINT_TO_MEASURE="10", ML_ALGORITHM=algorithm, ML_PAIRWISE_ALGORITHM="none",
               threshold="4", threshold0="4", threshold1="4", threshold2="4")
    return BrainConfig.from_env(env)


def monitor(store, prom, clock, device, algorithm, worker="s", min_capacity=64):
    return StreamingMonitor(store, config(algorithm), worker_id=worker, clock=clock, device=torch.device(device),
                            prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                            metrics=BrainMetrics(), ring_len=R, window=W, min_capacity=min_capacity)


def run(device, algorithm, probe=None):
    """Tick the monitor at TICKS; returns the statuses written per tick, the final docs and
    what ``probe(mon, t, ids)`` returned after each tick."""
    clock, prom, store, ids = world()
    mon = monitor(store, prom, clock, device, algorithm)
    written, seen = [], []

    async def go():
        for t in TICKS:
            clock.t = t
            mon.sync()
            w = await mon.tick()
            written.append({name: w.get(j) for name, j in ids.items()})
            seen.append(probe(mon, t, ids) if probe else None)
    asyncio.run(go())
    return written, {name: store.get(j) for name, j in ids.items()}, seen, mon


def row_of(mon, app, j):
    return mon.rows[(EP, FAMILY + M3[j][0], NS, app)]


def pair_of(mon, name, ids):
    return mon.job_pair.get(ids[name])


def reference_d2(app, t_last, bf16):
    """biv_ref on the fake Prometheus values themselves: R history points ending W steps
    before ``t_last`` (as the ring stores them: bf16 on the GPU), the window's last W."""
    ts_h = t_last - 60.0 * (W + R - 1 - np.arange(R))
    ts_w = t_last - 60.0 * (W - 1 - np.arange(W))
    h = torch.tensor(np.stack([generator(app, j)(ts_h) for j in (0, 1)], 1), dtype=torch.float32)[None]
    if bf16:
        h = h.bfloat16().float()
    x = torch.tensor(np.stack([generator(app, j)(ts_w) for j in (0, 1)], 1), dtype=torch.float32)[None]
    return biv_ref.mahalanobis2(biv_ref.fit_bivariate(h), x)[0], ts_w


DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("device", DEVICES)
def test_broken_correlation_fails_the_continuous_job(device):
    written, docs, _, _ = run(device, "bivariate_normal")
    for name in ("a", "a2"):
        assert [w[name] for w in written[:3]] == [r.ST_PREPROCESS_INPROGRESS] * 2 + [r.ST_COMPLETED_UNHEALTH], name
        info = json.loads(docs[name]["anomalyInfo"])
        assert set(info) == {"error5xx"} and info["error5xx"]["tags"] == ""
        assert "error5xx" in docs[name]["reason"]
        vals = info["error5xx"]["values"]
        assert vals and min(vals[0::2]) >= BREAK_AT and max(vals[0::2]) <= T0 + 240
        np.testing.assert_allclose(vals[1::2], generator("a", 0)(np.array(vals[0::2])), rtol=1e-5)
    for name in ("b", "c"):
        assert [w[name] for w in written] == [r.ST_PREPROCESS_INPROGRESS] * 4 + [r.ST_COMPLETED_HEALTH], name
    # the per-metric scorer alone sees nothing: the scenario isolates the joint model
    alone, docs1, _, _ = run(device, "moving_average_all")
    for name in ("a", "a2", "b", "c"):
        assert [w[name] for w in alone] == [r.ST_PREPROCESS_INPROGRESS] * 4 + [r.ST_COMPLETED_HEALTH], name
    if device != "cpu":  # the GPU monitor and the CPU monitor write the same statuses on every tick
        assert run("cpu", "bivariate_normal")[0] == written
        assert run("cpu", "moving_average_all")[0] == alone


@pytest.mark.parametrize("algorithm,paired", [
    ("auto", {"a", "a2", "b"}), ("bivariate_normal", {"a", "a2", "b", "d"}), ("lstm", set()), ("holt_winters", set()),
])
def test_pair_dispatch(algorithm, paired):
    clock, prom, store, ids = world()
    mon = monitor(store, prom, clock, "cpu", algorithm)
    mon.sync()
    asyncio.run(mon.tick())
    assert {n for n in ids if pair_of(mon, n, ids) is not None} == paired
    if not paired:
        assert mon.pairs == [] and mon.shard.pairs is None
        return
    assert pair_of(mon, "a", ids) == pair_of(mon, "a2", ids)   # identical pairs are one pair
    assert len(mon.pairs) == len(paired) - 1
    assert mon.shard.pairs.tolist() == [list(p) for p in mon.pairs]
    # first two aliases in sorted order: (error5xx, latency); with three, (error4xx, error5xx)
    assert mon.pairs[pair_of(mon, "a", ids)] == (row_of(mon, "a", 0), row_of(mon, "a", 1))
    if "d" in paired:
        assert mon.pairs[pair_of(mon, "d", ids)] == (row_of(mon, "d", 2), row_of(mon, "d", 0))


@pytest.mark.parametrize("device", DEVICES)
def test_joint_d2_matches_the_reference_on_the_source_values(device):
    def probe(mon, t, ids):
        if t != T0 + 240:
            return None
        q = mon.job_pair[ids["a"]]   # the table of this tick (a's jobs finished in it)
        col = (mon.shard.cur.ticks - 1) % W
        order = [(col - (W - 1 - k)) % W for k in range(W)]    # slots, oldest first
        names, counts = mon.app_table()   # the counters are rewritten every tick: keep a copy
        return (mon.shard.out["joint_d2"][q].float().cpu()[order], (names, counts.clone()),
                mon.shard.out["joint_verdict"].cpu().clone())
    _, _, seen, _ = run(device, "bivariate_normal", probe)
    d2, (names, counts), jv = seen[2]
    want, ts_w = reference_d2("a", T0 + 240, bf16=device != "cpu")
    print("joint d2", d2.tolist(), "reference", want.tolist())
    torch.testing.assert_close(d2, want, **D2_TOL)
    assert (want[torch.tensor(ts_w >= BREAK_AT)] > 16).all() and (want[torch.tensor(ts_w < BREAK_AT)] < 16).all()
    # health table: one anomalous series for a (the pair's shared first row, counted once)
    stats = dict(zip(names, counts.cpu().tolist()))
    assert stats[(NS, "a")] == [1, 2] and stats[(NS, "b")] == [0, 2]
    assert sorted(jv.tolist()) == [0, 0, 1]


def test_terminal_statuses_match_the_per_job_worker():
    written, docs, _, _ = run("cpu", "bivariate_normal")
    clock, prom, store, ids = world()
    cfg = config("bivariate_normal")
    w = BrainWorker(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                    scorer=BatchScorer(cfg, device=torch.device("cpu")), worker_id="w", clock=clock)

    async def go():
        for t in TICKS:
            clock.t = t
            await w.cycle()
    asyncio.run(go())
    for name in ("a", "b"):
        assert store.get(ids[name])["status"] == docs[name]["status"], name
    assert docs["a"]["status"] == r.ST_COMPLETED_UNHEALTH and docs["b"]["status"] == r.ST_COMPLETED_HEALTH


@pytest.mark.parametrize("device", DEVICES)
def test_pair_membership_and_growth(device):
    clock, prom, store, ids = world(extra_apps=("e", "f", "g"))
    mon = monitor(store, prom, clock, device, "auto", min_capacity=8)

    def check():
        for jid, q in mon.job_pair.items():
            s = mon.jobs[jid].series
            a0, a1 = sorted(s)[:2]
            assert (mon.keys[mon.pairs[q][0]], mon.keys[mon.pairs[q][1]]) == (s[a0], s[a1])
        assert (mon.shard.pairs.tolist() if mon.pairs else None) == ([list(p) for p in mon.pairs] or None)

    async def go():
        for t in TICKS[:3]:
            clock.t = t
            mon.sync()
            await mon.tick()
        assert ids["a"] not in mon.jobs and ids["a2"] not in mon.jobs   # failed at T0 + 240
        clock.t = T0 + 300
        b_pair = mon.pairs[mon.job_pair[ids["b"]]]
        later = svc.register(store, job("b-again", "b", M2))[1]["jobId"]
        mon.sync()
        await mon.tick()                       # a's rows are freed: its pair is gone
        assert (EP, FAMILY + M2[0][0], NS, "a") not in mon.rows
        assert mon.pairs == [b_pair] and mon.job_pair == {ids["b"]: 0, later: 0}
        check()
        assert mon.shard.spec.n_series == 8
        for app in ("e", "f", "g"):            # 8 live rows + 6: the shard doubles
            svc.register(store, job(app, app, M2))
        clock.t = T0 + 360
        mon.sync()
        w = await mon.tick()
        assert mon.shard.spec.n_series == 16 and len(mon.pairs) == 4 and len(mon.job_pair) == 5
        check()
        assert set(w.values()) == {r.ST_PREPROCESS_INPROGRESS}
        assert mon.shard.out["joint_verdict"].cpu().tolist() == [0, 0, 0, 0]
    asyncio.run(go())


def test_pairs_are_rebuilt_after_a_snapshot_restore(tmp_path):
    clock, prom, store, ids = world()
    snap = str(tmp_path / "stream.safetensors")

    async def go():
        m1 = monitor(store, prom, clock, "cpu", "bivariate_normal", worker="w1")
        m1.sync()
        await m1.tick()
        clock.t = T0 + 120
        await m1.tick()
        assert m1.save_snapshot(snap)
        m2 = monitor(store, prom, clock, "cpu", "bivariate_normal", worker="w1")   # the same worker, restarted
        m2.jobs = dict(m1.jobs)
        assert m2.pairs == [] and m2.restore_snapshot(snap)
        m2.sync()
        assert m2.pairs == m1.pairs and m2.job_pair == m1.job_pair and len(m2.pairs) == 3
        assert m2.shard.pairs.tolist() == m1.shard.pairs.tolist()
        clock.t = T0 + 240
        docs = {}
        for m in (m1, m2):   # both hold the lease as "w1": each writes the same documents
            w = await m.tick()
            docs[m] = (w, {j: (store.get(j)["status"], store.get(j).get("anomalyInfo")) for j in ids.values()})
            for j in ids.values():   # hand the finished jobs back so the second monitor's writes land too
                store.update(j, {"claimed_by": "w1"})
        assert docs[m1] == docs[m2]
        assert docs[m1][0][ids["a"]] == r.ST_COMPLETED_UNHEALTH and docs[m1][0][ids["b"]] == r.ST_PREPROCESS_INPROGRESS
        torch.testing.assert_close(m1.shard.out["joint_d2"], m2.shard.out["joint_d2"], rtol=0, atol=0, equal_nan=True)
    asyncio.run(go())
