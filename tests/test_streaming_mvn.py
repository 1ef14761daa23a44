"""Continuous jobs with three or more metrics under ``ML_ALGORITHM=multivariate_normal``
(brain/streaming.py group table, brain/engine.py ``set_groups``, ops/csrc/mvn_groups.hip):
the job keeps its per-metric rows (moving_average_all) and gets the k-variate normal of
models/multivariate_normal.py over the rows of all its aliases in sorted order, refitted
from the ring and scored on the pod-mean window every tick."""

import asyncio
import json
import logging

import httpx
import numpy as np
import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.brain.batch import BatchScorer
from foremast_amd.brain.streaming import StreamingMonitor
from foremast_amd.brain.worker import BrainWorker
from foremast_amd.models import multivariate_normal as mvn
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
M3 = (("http_server_requests_error_5xx", "error5xx"), ("http_server_requests_latency", "latency"),
      ("http_server_requests_error_4xx", "error4xx"))
M9 = tuple((f"custom_metric_{j}", f"a{j}") for j in range(9))
# x: latency, the third alias in sorted order, breaks its relation to the other two; y: healthy;
# z: one metric; w: nine metrics
APPS = {"x": M3, "y": M3, "z": M3[:1], "w": M9}
SORTED3 = (2, 0, 1)             # error4xx, error5xx, latency as indices into M3
BREAK_AT = T0 + 180
END = T0 + 600
TICKS = (T0, T0 + 120, T0 + 240, T0 + 360, T0 + 660)
R, W = 2880, 5
THR = 4.0
D2_TOL = dict(rtol=2e-3, atol=1e-3)  # tests/test_bivariate_pairs_gpu.py


class Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def correlated(seed, j, flip_after=None):
    """Metric j of an app: a shared latent load u(t) drives every metric with the same
    amplitude (level 10 (j + 1), 3 u) beside independent noise of sigma 0.2.  After
    ``flip_after`` the latency (j = 1) moves against the load: each metric alone stays inside
    its usual range, and so does the pair of the other two."""
    lvl, amp = 10.0 * (j + 1), 3.0

    def f(ts):
        ts = np.asarray(ts, dtype=np.float64)
        u = _hash_noise(ts, seed)
        v = lvl + amp * u + 0.2 * _hash_noise(ts, seed + 1000 * (j + 1))
        if flip_after is not None and j == 1:
            v = np.where(ts >= flip_after, lvl - amp * u + 0.2 * _hash_noise(ts, seed + 77), v)
        return v
    return f


def generator(app, j):
    i = sorted(APPS).index(app) if app in APPS else 4 + ord(app) - ord("e")
    return correlated(10 * i + 7, j, BREAK_AT if app == "x" else None)


def job(name, app, mets, end=END):
    cur, hist = {}, {}
    for m, alias in mets:
        params = {"endpoint": EP, "query": f'{FAMILY}{m}{{namespace="{NS}",app="{app}"}}', "step": 60}
        cur[alias] = {"dataSourceType": "prometheus", "parameters": dict(params, start=int(T0), end=int(end))}
        hist[alias] = {"dataSourceType": "prometheus",
                       "parameters": dict(params, start=int(T0 - 2 * 86400), end=int(T0))}
    return {"appName": name, "startTime": format_rfc3339(T0), "endTime": format_rfc3339(end),
            "strategy": "continuous", "metrics": {"current": cur, "historical": hist}}


def world(apps=("x", "y", "z"), extra_apps=()):
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    store = MemoryJobStore()
    ids = {}
    for app, mets in [(a, APPS[a]) for a in apps] + [(a, M3) for a in extra_apps]:
        for j, (m, _alias) in enumerate(mets):
            prom.add(FAMILY + m, {"namespace": NS, "app": app}, generator(app, j))
    for app in apps:
        ids[app] = svc.register(store, job(app, app, APPS[app]))[1]["jobId"]
    if "x" in apps:
        ids["x2"] = svc.register(store, job("x-again", "x", M3))[1]["jobId"]   # a second job on x's series
    assert len(set(ids.values())) == len(ids)
    return clock, prom, store, ids


def config(algorithm):
    env = reference_default_env()
    env.update(MIN_HISTORICAL_DATA_POINT_TO_MEASURE="10", ML_ALGORITHM=algorithm, ML_PAIRWISE_ALGORITHM="none",
               threshold=str(int(THR)), threshold0=str(int(THR)), threshold1=str(int(THR)), threshold2=str(int(THR)))
    return BrainConfig.from_env(env)


def monitor(store, prom, clock, device, algorithm, worker="s", min_capacity=64):
    return StreamingMonitor(store, config(algorithm), worker_id=worker, clock=clock, device=torch.device(device),
                            prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                            metrics=BrainMetrics(), ring_len=R, window=W, min_capacity=min_capacity)


def run(device, algorithm, probe=None, apps=("x", "y", "z")):
    """Tick the monitor at TICKS; returns the statuses written per tick, the final docs and
    what ``probe(mon, t, ids)`` returned after each tick."""
    clock, prom, store, ids = world(apps)
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


def row_of(mon, app, metric):
    return mon.rows[(EP, FAMILY + metric, NS, app)]


def check_groups(mon):
    """Every job's group holds the rows of its aliases in sorted order (at most 8)."""
    for jid, q in mon.job_group.items():
        if jid not in mon.jobs:   # finished in this tick: the table is rebuilt at the next
            continue
        s = mon.jobs[jid].series
        assert [mon.keys[row] for row in mon.groups[q]] == [s[a] for a in sorted(s)[:8]]
    table = mon.shard.groups
    if not mon.groups:
        assert table is None
        return
    assert table.shape == (len(mon.groups), 8)
    for q, g in enumerate(mon.groups):
        assert table[q, :len(g)].tolist() == list(g) and (table[q, len(g):] == -1).all()


def reference_d2(app, t_last, bf16):
    """The reference on the fake Prometheus values themselves: R history points ending W steps
    before ``t_last`` (as the ring stores them: bf16 on the GPU), the window's last W; the
    metrics in the sorted order of their aliases."""
    ts_h = t_last - 60.0 * (W + R - 1 - np.arange(R))
    ts_w = t_last - 60.0 * (W - 1 - np.arange(W))
    h = torch.tensor(np.stack([generator(app, j)(ts_h) for j in SORTED3], 1), dtype=torch.float32)[None]
    if bf16:
        h = h.bfloat16().float()
    x = torch.tensor(np.stack([generator(app, j)(ts_w) for j in SORTED3], 1), dtype=torch.float32)[None]
    fit = mvn.fit_mvn(h)
    return mvn.mahalanobis2_mvn(fit, x)[0], mvn.contributions(fit, x)[0], ts_w


DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
HEALTHY = [r.ST_PREPROCESS_INPROGRESS] * 4 + [r.ST_COMPLETED_HEALTH]


@pytest.mark.parametrize("device", DEVICES)
def test_broken_relation_fails_the_job_and_names_the_metric(device):
    written, docs, _, _ = run(device, "multivariate_normal")
    for name in ("x", "x2"):
        assert [w[name] for w in written[:3]] == [r.ST_PREPROCESS_INPROGRESS] * 2 + [r.ST_COMPLETED_UNHEALTH], name
        info = json.loads(docs[name]["anomalyInfo"])
        assert set(info) == {"latency"} and info["latency"]["tags"] == ""       # that alias only
        assert "latency" in docs[name]["reason"]
        vals = info["latency"]["values"]
        assert vals and min(vals[0::2]) >= BREAK_AT and max(vals[0::2]) <= T0 + 240
        np.testing.assert_allclose(vals[1::2], generator("x", 1)(np.array(vals[0::2])), rtol=1e-5)
    for name in ("y", "z"):
        assert [w[name] for w in written] == HEALTHY, name
    # every per-metric band stays quiet: the scenario isolates the joint model
    alone, _, _, _ = run(device, "moving_average_all")
    # and the bivariate normal models (error4xx, error5xx) only: the gap this model closes
    two, _, _, mon2 = run(device, "bivariate_normal")
    for name in ("x", "x2", "y", "z"):
        assert [w[name] for w in alone] == HEALTHY, name
        assert [w[name] for w in two] == HEALTHY, name
    if device != "cpu":  # the GPU monitor and the CPU monitor write the same statuses on every tick
        assert run("cpu", "multivariate_normal")[0] == written


@pytest.mark.parametrize("algorithm,grouped", [
    ("multivariate_normal", {"x", "x2", "y"}), ("bivariate_normal", set()), ("auto", set()), ("lstm", set()),
    ("holt_winters", set()),
])
def test_group_dispatch(algorithm, grouped):
    clock, prom, store, ids = world()
    mon = monitor(store, prom, clock, "cpu", algorithm)
    mon.sync()
    asyncio.run(mon.tick())
    assert {n for n in ids if mon.job_group.get(ids[n]) is not None} == grouped
    check_groups(mon)
    if not grouped:
        assert mon.groups == [] and mon.shard.groups is None
        return
    assert mon.pairs == [] and mon.shard.pairs is None
    assert mon.job_group[ids["x"]] == mon.job_group[ids["x2"]]   # jobs on the same series share one group
    assert len(mon.groups) == 2
    assert mon.groups[mon.job_group[ids["x"]]] == tuple(row_of(mon, "x", M3[j][0]) for j in SORTED3)


@pytest.mark.parametrize("device", DEVICES)
def test_joint_d2_matches_the_reference_on_the_source_values(device):
    def probe(mon, t, ids):
        if t != T0 + 240:
            return None
        q = mon.job_group[ids["x"]]   # the table of this tick (x's jobs finished in it)
        col = (mon.shard.cur.ticks - 1) % W
        order = [(col - (W - 1 - k)) % W for k in range(W)]    # slots, oldest first
        names, counts = mon.app_table()   # the counters are rewritten every tick: keep a copy
        out = mon.shard.out
        d2 = out["joint_d2"][q].float().cpu()[order]
        c = out["joint_contrib"][q].float().cpu()[order]
        blame, verdict = out["joint_blame"].cpu().clone(), out["joint_verdict"].cpu().clone()
        return d2, c, blame, verdict, q, (names, counts.clone())
    _, _, seen, _ = run(device, "multivariate_normal", probe)
    d2, c, blame, jv, q, (names, counts) = seen[2]
    want, want_c, ts_w = reference_d2("x", T0 + 240, bf16=device != "cpu")
    thr2 = mvn.chi2_threshold(THR, 3)
    print("joint d2", d2.tolist(), "reference", want.tolist(), "q_3(thr)", thr2)
    print("contributions / d2", (want_c / want[:, None]).tolist())
    torch.testing.assert_close(d2, want, **D2_TOL)
    torch.testing.assert_close(c[:, :3], want_c, **D2_TOL)
    after = torch.tensor(ts_w >= BREAK_AT)
    assert (want[~after] < thr2).all() and (want[after] > thr2).any()
    # the scenario's attribution keeps clear of the naming line d2 / 3
    flagged = want > thr2
    assert ((want_c[flagged] / want[flagged, None] - 1 / 3).abs() > 0.03).all()
    assert blame[q] == 0b100 and sorted(jv.tolist()) == [0, 1]
    # health table: one anomalous series for x (latency alone is raised), none for y
    stats = dict(zip(names, counts.cpu().tolist()))
    assert stats[(NS, "x")] == [1, 3] and stats[(NS, "y")] == [0, 3]


def test_terminal_statuses_and_named_aliases_match_the_per_job_worker():
    written, docs, _, _ = run("cpu", "multivariate_normal")
    clock, prom, store, ids = world()
    cfg = config("multivariate_normal")
    w = BrainWorker(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                    scorer=BatchScorer(cfg, device=torch.device("cpu")), worker_id="w", clock=clock)

    async def go():
        for t in TICKS:
            clock.t = t
            await w.cycle()
    asyncio.run(go())
    for name in ("x", "y", "z"):
        assert store.get(ids[name])["status"] == docs[name]["status"], name
    assert docs["x"]["status"] == r.ST_COMPLETED_UNHEALTH and docs["y"]["status"] == r.ST_COMPLETED_HEALTH
    assert set(json.loads(store.get(ids["x"])["anomalyInfo"])) == set(json.loads(docs["x"]["anomalyInfo"])) == {"latency"}


@pytest.mark.gpu
def test_per_job_worker_on_the_gpu_names_the_same_aliases():
    """BatchScorer.score_mvn through kernels.mvn_groups (fp32 rows, head 0, one pod)."""
    found = {}
    for device in ("cpu", "cuda"):
        clock, prom, store, ids = world()
        cfg = config("multivariate_normal")
        w = BrainWorker(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                        scorer=BatchScorer(cfg, device=torch.device(device)), worker_id="w", clock=clock)

        async def go():
            for t in TICKS:
                clock.t = t
                await w.cycle()
        asyncio.run(go())
        found[device] = {n: (store.get(j)["status"], sorted(json.loads(store.get(j).get("anomalyInfo") or "{}")))
                         for n, j in ids.items()}
    assert found["cuda"] == found["cpu"]
    assert found["cuda"]["x"] == (r.ST_COMPLETED_UNHEALTH, ["latency"])


@pytest.mark.parametrize("device", DEVICES)
def test_group_membership_and_growth(device):
    clock, prom, store, ids = world(apps=("x", "y"), extra_apps=("e", "f"))
    mon = monitor(store, prom, clock, device, "multivariate_normal", min_capacity=8)

    async def go():
        for t in TICKS[:3]:
            clock.t = t
            mon.sync()
            await mon.tick()
            check_groups(mon)
        assert ids["x"] not in mon.jobs and ids["x2"] not in mon.jobs   # failed at T0 + 240
        clock.t = T0 + 300
        y_group = mon.groups[mon.job_group[ids["y"]]]
        later = svc.register(store, job("y-again", "y", M3))[1]["jobId"]
        mon.sync()
        await mon.tick()                       # x's rows are freed: its group is gone
        assert (EP, FAMILY + M3[0][0], NS, "x") not in mon.rows
        assert mon.groups == [y_group] and mon.job_group == {ids["y"]: 0, later: 0}
        check_groups(mon)
        assert mon.shard.spec.n_series == 8
        for app in ("e", "f"):                 # 3 live rows + 6: the shard doubles
            svc.register(store, job(app, app, M3))
        clock.t = T0 + 360
        mon.sync()
        w = await mon.tick()
        assert mon.shard.spec.n_series == 16 and len(mon.groups) == 3 and len(mon.job_group) == 4
        check_groups(mon)
        assert set(w.values()) == {r.ST_PREPROCESS_INPROGRESS}
        assert mon.shard.out["joint_verdict"].cpu().tolist() == [0, 0, 0]
    asyncio.run(go())


def test_groups_are_rebuilt_after_a_snapshot_restore(tmp_path):
    clock, prom, store, ids = world()
    snap = str(tmp_path / "stream.safetensors")

    async def go():
        m1 = monitor(store, prom, clock, "cpu", "multivariate_normal", worker="w1")
        m1.sync()
        await m1.tick()
        clock.t = T0 + 120
        await m1.tick()
        assert m1.save_snapshot(snap)
        from safetensors import safe_open
        with safe_open(snap, framework="pt") as f:     # derived state: never in the snapshot
            assert not [k for k in f.keys() if "group" in k or "pair" in k]
        m2 = monitor(store, prom, clock, "cpu", "multivariate_normal", worker="w1")   # the same worker, restarted
        m2.jobs = dict(m1.jobs)
        assert m2.groups == [] and m2.restore_snapshot(snap)
        m2.sync()
        assert m2.groups == m1.groups and m2.job_group == m1.job_group and len(m2.groups) == 2
        assert m2.shard.groups.tolist() == m1.shard.groups.tolist()
        check_groups(m2)
        clock.t = T0 + 240
        docs = {}
        for m in (m1, m2):   # both hold the lease as "w1": each writes the same documents
            w = await m.tick()
            docs[m] = (w, {j: (store.get(j)["status"], store.get(j).get("anomalyInfo")) for j in ids.values()})
            for j in ids.values():   # hand the finished jobs back so the second monitor's writes land too
                store.update(j, {"claimed_by": "w1"})
        assert docs[m1] == docs[m2]
        assert docs[m1][0][ids["x"]] == r.ST_COMPLETED_UNHEALTH and docs[m1][0][ids["y"]] == r.ST_PREPROCESS_INPROGRESS
        torch.testing.assert_close(m1.shard.out["joint_d2"], m2.shard.out["joint_d2"], rtol=0, atol=0, equal_nan=True)
    asyncio.run(go())


@pytest.mark.parametrize("device", DEVICES)
def test_a_job_with_nine_metrics_models_its_first_eight(device, caplog):
    clock, prom, store, ids = world(apps=("w", "y"))
    mon = monitor(store, prom, clock, device, "multivariate_normal")

    async def go():
        with caplog.at_level(logging.WARNING):
            for t in TICKS[:2]:
                clock.t = t
                mon.sync()
                await mon.tick()
    asyncio.run(go())
    q = mon.job_group[ids["w"]]
    assert mon.groups[q] == tuple(row_of(mon, "w", f"custom_metric_{j}") for j in range(8))   # a0 .. a7
    check_groups(mon)
    assert mon.shard.group_k.tolist() == [len(g) for g in mon.groups] and sorted(mon.shard.group_k.tolist()) == [3, 8]
    warned = [rec for rec in caplog.records if "models the first 8" in rec.getMessage()]
    assert len(warned) == 1                          # once per job, not once per tick
    jv = mon.shard.out["joint_verdict"].cpu().tolist()
    assert jv == [0, 0]
    assert torch.isfinite(mon.shard.out["joint_d2"]).all()
    assert (mon.shard.out["joint_mean"][q, :8] != 0).all() and mon.shard.out["joint_cov"].shape == (2, 36)
