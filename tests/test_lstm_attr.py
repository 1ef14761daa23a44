"""Per-feature attribution of the joint LSTM-AE verdict, on the CPU: the reference
functions (models/lstm_ae.py), the shard's CPU scoring path, the snapshot, the
configuration switch, and the job documents of the resident LSTM monitor and the
rollout engine (FOREMAST_LSTM_ATTRIBUTION=1 names only the metric that broke)."""

import asyncio
import json

import httpx
import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.brain import checkpoint as ck
from foremast_amd.brain.lstm_engine import LstmShard
from foremast_amd.brain.lstm_monitor import LstmMonitor
from foremast_amd.brain.rollout import RolloutMonitor
from foremast_amd.models.lstm_ae import LSTMAutoencoder, attribute
from foremast_amd.promql import synth
from foremast_amd.promql.client import PromClient
from foremast_amd.promql.fake import FakePrometheus
from foremast_amd.service import app as svc
from foremast_amd.store import MemoryJobStore
from foremast_amd.utils.config import BrainConfig, reference_default_env
from foremast_amd.utils.metrics import BrainMetrics
from foremast_amd.utils.timeutil import format_rfc3339
from tests.test_rollout_joint import M3, NS, T0, Clock, request

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------- reference functions
def test_recon_error_features_mean_is_recon_error():
    torch.manual_seed(0)
    m = LSTMAutoencoder(3, 16)
    x = torch.randn(9, 12, 3)
    with torch.no_grad():
        ef, e = m.recon_error_features(x), m.recon_error(x)
        want = ((m(x) - x) ** 2).mean(1)
    assert ef.shape == (9, 3)
    torch.testing.assert_close(ef, want, rtol=0, atol=0)
    torch.testing.assert_close(ef.mean(1), e, rtol=1e-6, atol=1e-7)


def _cal(mu, inv, n, F):
    return torch.tensor([mu, inv]).repeat(n, F, 1)


def test_attribute_threshold_and_level_bits():
    err = torch.tensor([[1.0, 6.0, 1.0],     # z = 0, 5, 0   -> feature 1
                        [6.0, 1.0, 7.0],     # z = 5, 0, 6   -> features 0 and 2
                        [1.0, 1.0, 1.0],     # healthy error, level term on feature 2
                        [9.0, 9.0, 9.0]])    # verdict 0 -> nothing
    zl = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 5.0, -7.0], [9.0, 9.0, 9.0]])
    v = torch.tensor([1, 1, 1, 0], dtype=torch.int8)
    got = attribute(err, _cal(1.0, 1.0, 4, 3), 4.0, zl, 6.0, v)
    assert got.dtype == torch.int32 and got.tolist() == [0b010, 0b101, 0b100, 0]
    # a threshold per row, no level term
    got = attribute(err, _cal(1.0, 1.0, 4, 3), torch.tensor([4.0, 5.5, 4.0, 4.0]), verdict=v)
    assert got.tolist() == [0b010, 0b100, 0b001, 0]   # row 2: fallback (all z equal: the lowest f)


def test_attribute_fallback_ties_nan_and_padding():
    cal = _cal(1.0, 1.0, 6, 3)
    err = torch.tensor([[2.0, 3.0, 3.0],     # nothing above 4: the largest z, the tie goes to feature 1
                        [NAN, 2.0, 1.5],     # NaN counts as -inf
                        [NAN, NAN, NAN],     # every z NaN: feature 0
                        [2.0, 3.0, 50.0],    # feature 2 is padding (n_feat 2): never named
                        [1.0, 1.0, 50.0],    # padding again: the fallback picks among the real ones
                        [2.0, 9.0, 1.0]])
    v = torch.ones(6, dtype=torch.int8)
    nf = torch.tensor([3, 3, 3, 2, 2, 0], dtype=torch.int32)
    assert attribute(err, cal, 4.0, verdict=v, n_feat=nf).tolist() == [0b010, 0b010, 0b001, 0b010, 0b001, 0]
    # without a verdict every row counts as flagged; without n_feat every feature is real
    assert attribute(err[3:5], cal[3:5], 4.0).tolist() == [0b100, 0b100]
    # a level z on a padded feature is not named either
    zl = torch.tensor([[0.0, 0.0, 99.0]])
    assert attribute(err[:1], cal[:1], 4.0, zl, 5.0, v[:1], torch.tensor([2], dtype=torch.int32)).tolist() == [0b010]
    # NaN level z never sets a bit; +inf z does
    assert attribute(torch.tensor([[INF, 1.0]]), _cal(1.0, 1.0, 1, 2), 4.0, torch.tensor([[0.0, NAN]]), 5.0).tolist() == [1]


# ---------------------------------------------------------------------- shard (CPU path)
def _history(n, L, F, seed=0):
    """Noise-dominated series (a small shared daily wave): per-series, per-feature noise scale 0.1 .. 0.3."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float32)
    scale = 0.1 + 0.2 * torch.rand(n, 1, F, generator=g)
    base = torch.sin(2 * torch.pi * t / 48.0)[None, :, None] * 0.05 + 10.0
    return base + scale * torch.randn(n, L, F, generator=g), scale[:, 0]


def _shard(attribution, n=12, F=3, **kw):
    sh = LstmShard(n, 480, F, window=16, hidden=16, device="cpu", train_batch=32, seed=3, dtype=torch.float32,
                   cal_windows=8, season=48, level_threshold=None, attribution=attribution, **kw)
    hist, scale = _history(n, 408, F)
    sh.load_history(hist[:, :400])
    for _ in range(30):
        sh.train_step()
    return sh, hist[:, 400:], scale


def test_shard_cpu_attribution_names_the_regressed_feature():
    on, ticks, scale = _shard(True)
    off, _, _ = _shard(False)
    on.calibrate(64)
    off.calibrate(64)
    assert on.cal_feat is not None and on.cal_feat.shape == (12, 3, 2) and off.cal_feat is None
    torch.testing.assert_close(on.cal, off.cal, rtol=0, atol=0)   # the entity's own calibration is untouched
    # mu_f: mean without the largest of the 8 windows; the spread is relative: inv_f = 1 / (rho1 mu_f)
    torch.testing.assert_close(on.cal_feat[..., 0] * on.cal_feat[..., 1],
                               torch.full((12, 3), 1.0 / on.rho1), rtol=1e-5, atol=0)
    cf0 = on.cal_feat.clone()
    for k in range(8):   # the next 8 minutes; series 5: feature 1 rises by 8 of its own noise sigmas
        x = ticks[:, k].clone()
        x[5, 1] += 8.0 * scale[5, 1]
        o_on, o_off = on.tick(x.clone(), train=False), off.tick(x.clone(), train=False)
    for k in ("err", "zscore", "verdict"):
        torch.testing.assert_close(o_on[k], o_off[k], rtol=0, atol=0)
    assert "blame" not in o_off and o_on["blame"].dtype == torch.int32
    assert int(o_on["verdict"][5]) == 1 and int(o_on["blame"][5]) == 0b010
    assert bool(((o_on["verdict"] == 0) == (o_on["blame"] == 0)).all())
    # healthy rows' per-feature levels tracked their errors; the flagged row kept its bits
    assert torch.equal(on.cal_feat[5], cf0[5])
    healthy = (o_on["verdict"] == 0).nonzero().flatten()
    assert len(healthy) and not torch.equal(on.cal_feat[healthy], cf0[healthy])


def test_shard_without_feature_calibration_names_every_real_feature():
    sh, ticks, _ = _shard(True)
    sh.calibrate(64)
    sh.cal_feat = None                       # as after loading a snapshot written without it
    sh.n_feat[7] = 2
    sh.threshold = -1e9                      # every row flagged
    out = sh.tick(ticks[:, 0].clone(), train=False)
    want = [0b111] * 12
    want[7] = 0b011
    assert out["blame"].tolist() == want
    # rows= calibration of a grown shard extends the per-feature table
    sh.calibrate(64)
    sh.grow(16)
    assert sh.cal_feat.shape == (16, 3, 2) and sh.n_feat.tolist()[12:] == [3] * 4
    before = sh.cal_feat.clone()
    sh.calibrate(64, rows=torch.tensor([2, 3]))
    changed = (sh.cal_feat != before).flatten(1).any(1).nonzero().flatten().tolist()
    assert set(changed) <= {2, 3}            # only the rows asked for are rewritten


def test_checkpoint_round_trip_and_old_snapshot(tmp_path):
    sh, _, _ = _shard(True)
    sh.calibrate(64)
    sh.n_feat[1] = 2
    p = str(tmp_path / "lstm.ckpt")
    ck.save_lstm_shard(sh, p)
    back = ck.load_lstm_shard(p)
    assert back.attribution is True and back.rho1 == pytest.approx(sh.rho1)
    assert torch.equal(back.cal_feat, sh.cal_feat) and torch.equal(back.n_feat, sh.n_feat)
    # a snapshot written before the attribution existed: no cal_feat / n_feat / rho1 / flag
    meta, tensors = ck._read(p, "cpu")
    for k in ("cal_feat", "n_feat"):
        tensors.pop(k)
    meta.pop("rho1")
    meta["args"].pop("attribution")
    old = str(tmp_path / "old.ckpt")
    ck._atomic_save(tensors, meta, old)
    legacy = ck.load_lstm_shard(old)
    assert legacy.attribution is False and legacy.cal_feat is None and legacy.rho1 == 1.0
    assert legacy.n_feat.tolist() == [3] * 12 and torch.equal(legacy.cal, sh.cal)
    legacy.attribution = True                # switched on over an old snapshot: every feature, then calibrate()
    legacy.threshold = -1e9
    assert legacy.score()["blame"].tolist() == [0b111] * 12
    legacy.calibrate(64)
    assert legacy.cal_feat is not None


# ---------------------------------------------------------------------- configuration
def test_config_flag():
    env = reference_default_env()
    assert BrainConfig.from_env(env).lstm_attribution is False
    assert BrainConfig.from_env(dict(env, FOREMAST_LSTM_ATTRIBUTION="0")).lstm_attribution is False
    assert BrainConfig.from_env(dict(env, FOREMAST_LSTM_ATTRIBUTION="1")).lstm_attribution is True
    for bad in ("2", "true", "on", "-1"):
        with pytest.raises(ValueError, match="FOREMAST_LSTM_ATTRIBUTION"):
            BrainConfig.from_env(dict(env, FOREMAST_LSTM_ATTRIBUTION=bad))
    from foremast_amd.deploy.manifests import brain
    envs = brain()[0]["spec"]["template"]["spec"]["containers"][0]["env"]
    assert {"name": "FOREMAST_LSTM_ATTRIBUTION", "value": "0"} in envs


# ---------------------------------------------------------------------- resident monitor
METRICS = (("namespace_app_per_pod:http_server_requests_latency", "latency"),
           ("namespace_app_per_pod:http_server_requests_error_5xx", "error5xx"),
           ("namespace_app_per_pod:cpu_usage_seconds_total", "cpu"))
NOISE = 0.2


def job(app, endpoint="http://prometheus:9090/api/v1/", now=T0, end=T0 + 3600):
    cur, hist = {}, {}
    for m, alias in METRICS:
        q = f'{m}{{namespace="ns",app="{app}"}}'
        p = {"endpoint": endpoint, "query": q, "step": 60}
        cur[alias] = {"dataSourceType": "prometheus", "parameters": dict(p, start=int(now), end=int(end))}
        hist[alias] = {"dataSourceType": "prometheus", "parameters": dict(p, start=int(now - 86400), end=int(now))}
    return {"appName": app, "startTime": format_rfc3339(now), "endTime": format_rfc3339(end),
            "strategy": "continuous", "metrics": {"current": cur, "historical": hist}}


def shifted(gen, at, by):
    def f(ts):
        import numpy as np
        ts = np.asarray(ts, dtype=np.float64)
        return gen(ts) + np.where(ts >= at, by, 0.0)
    return f


def run_monitor(attribution):
    """Six three-metric continuous jobs; app2's latency (and only it) rises by 40 of its
    noise sigmas from minute 5 on, for the rest of the run (more than a 16-minute window)."""
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    apps = [f"app{i}" for i in range(6)]
    for i, app in enumerate(apps):
        for j, (m, alias) in enumerate(METRICS):
            gen = synth.seasonal(level=10.0 + i + 5 * j, amp=2.0, noise=NOISE, seed=10 * i + j)
            if app == "app2" and alias == "latency":
                gen = shifted(gen, T0 + 5 * 60, 40 * NOISE)
            prom.add(m, {"namespace": "ns", "app": app}, gen)
    store = MemoryJobStore()
    ids = {a: svc.register(store, job(a))[1]["jobId"] for a in apps}
    env = reference_default_env()
    env.update(ML_ALGORITHM="lstm", ML_LSTM_THRESHOLD="4", FOREMAST_LSTM_ATTRIBUTION=attribution)
    cfg = BrainConfig.from_env(env)
    client = PromClient(transport=httpx.ASGITransport(app=prom.asgi_app()))
    mon = LstmMonitor(store, cfg, prom=client, device=torch.device("cpu"), ring_len=2880, window=16, hidden=16,
                      min_capacity=4, clock=clock)

    async def go():
        assert mon.sync() == 6
        written = {}
        for k in range(24):
            clock.t = T0 + 60 * k
            written.update(await mon.tick())
            if ids["app2"] in written:   # fail fast: the verdict ends the run
                break
        return written
    written = asyncio.run(go())
    return mon, store, ids, written


def test_monitor_names_only_the_regressed_metric():
    """The test that fails without the attribution: with the flag on the job document of
    the app whose latency regressed names latency alone."""
    mon, store, ids, written = run_monitor("1")
    assert mon.shard.attribution and mon.shard.cal_feat is not None
    # sorted aliases are the features: cpu, error5xx, latency -> three real features per entity
    assert written.get(ids["app2"]) == "completed_unhealth", written
    d = store.get(ids["app2"])
    info = json.loads(d["anomalyInfo"])
    assert set(info) == {"latency"}, info
    assert info["latency"]["tags"] == "lstm" and len(info["latency"]["values"]) == 2
    assert d["reason"] == "anomaly detected in latency (lstm)"
    assert all(written.get(ids[a]) is None for a in ids if a != "app2"), written


def test_monitor_flag_off_names_every_metric():
    mon, store, ids, written = run_monitor("0")
    assert not mon.shard.attribution and mon.shard.cal_feat is None
    assert written.get(ids["app2"]) == "completed_unhealth", written
    d = store.get(ids["app2"])
    assert set(json.loads(d["anomalyInfo"])) == {"latency", "error5xx", "cpu"}
    assert d["reason"] == "anomaly detected in cpu,error5xx,latency (lstm)"


# ---------------------------------------------------------------------- rollout engine
def run_rollout(attribution, monkeypatch):
    """Four 3-metric canary jobs under ML_ALGORITHM=lstm; the new pods of d3 triple their
    latency (only) from the third minute on.  Per-metric rows cannot fire (threshold 1000)."""
    monkeypatch.setenv("FOREMAST_LSTM_PRETRAIN", "40")
    monkeypatch.setenv("FOREMAST_LSTM_PRETRAIN_PER_TICK", "40")
    clock = Clock(T0)
    prom = FakePrometheus(clock=clock)
    store = MemoryJobStore()
    ids = {}
    for i in range(4):
        app = f"d{i}"
        new, old = [f"{app}-v2-{k}" for k in range(2)], [f"{app}-v1-{k}" for k in range(3)]
        for j, (m, alias) in enumerate(M3):
            base = synth.seasonal(level=10.0 + i + 5 * j, amp=2.0, noise=0.2, seed=10 * i + j)
            prom.add("namespace_app_per_pod:" + m, {"namespace": NS, "app": app}, base)
            for k, pod in enumerate(new + old):
                g = synth.seasonal(level=10.0 + i + 5 * j, amp=2.0, noise=0.2, seed=10 * i + j + 100 * (k + 1))
                if app == "d3" and pod in new and alias == "latency":
                    g = synth.step_change(g, at=T0 + 120, factor=3.0)
                prom.add("namespace_pod:" + m, {"namespace": NS, "pod": pod}, g)
        ids[app] = svc.register(store, request(app, new, old, M3))[1]["jobId"]
    env = reference_default_env()
    env.update(MIN_HISTORICAL_DATA_POINT_TO_MEASURE="10", ML_ALGORITHM="lstm", ML_PAIRWISE_ALGORITHM="none",
               threshold="1000", threshold0="1000", threshold1="1000", threshold2="1000", ML_LSTM_THRESHOLD="4",
               FOREMAST_LSTM_WINDOW="8", FOREMAST_LSTM_HIDDEN="16", FOREMAST_LSTM_ATTRIBUTION=attribution)
    cfg = BrainConfig.from_env(env)
    mon = RolloutMonitor(store, cfg, prom=PromClient(transport=httpx.ASGITransport(app=prom.asgi_app())),
                         device=torch.device("cpu"), metrics=BrainMetrics(), window=10, pods=5, clock=clock,
                         ring_len=2880, min_capacity=4)
    written = {}

    async def go():
        for k in range(12):
            clock.t = T0 + 60 * k
            mon.sync()
            written.update(await mon.tick())
    asyncio.run(go())
    return store, ids, written


def test_rollout_names_only_the_regressed_metric(monkeypatch):
    store, ids, written = run_rollout("1", monkeypatch)
    assert written.get(ids["d3"]) == r.ST_COMPLETED_UNHEALTH, written
    d = store.get(ids["d3"])
    assert set(json.loads(d["anomalyInfo"])) == {"latency"}
    assert d["reason"] == "anomaly detected in latency"
    assert all(written.get(ids[a]) == r.ST_COMPLETED_HEALTH for a in ("d0", "d1", "d2")), written


def test_rollout_flag_off_names_every_metric(monkeypatch):
    store, ids, written = run_rollout("0", monkeypatch)
    assert written.get(ids["d3"]) == r.ST_COMPLETED_UNHEALTH, written
    assert set(json.loads(store.get(ids["d3"])["anomalyInfo"])) == {a for _m, a in M3}
