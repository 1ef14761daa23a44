"""robust_average / robust_average_all: the median / MAD reference model and its wiring
through the configuration, the plans and the CPU paths of the engines."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from foremast_amd.api import rest as r

from foremast_amd.brain import plans
from foremast_amd.brain.batch import BatchScorer, MetricTask
from foremast_amd.brain.engine import ShardSpec, StreamingShard, synthetic_history
from foremast_amd.models import detect as det_ref
from foremast_amd.models import moving_average as ma_ref
from foremast_amd.models import robust_average as rb_ref
from foremast_amd.utils import config as config_mod
from foremast_amd.utils.config import BrainConfig, reference_default_env

NAMES = ("robust_average_all", "robust_average")


def _helper(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rw = _helper("rollout_world")
NAN = float("nan")


def _sorted_reference(row):
    """Plain sort in numpy: lower median, lower median of the fp32 |y - centre|, fp64 std."""
    v = np.sort(row[~np.isnan(row)])
    n = len(v)
    if n == 0:
        return NAN, NAN, NAN, 0
    c = v[(n - 1) // 2]
    d = np.sort(np.abs(v.astype(np.float32) - np.float32(c)))
    return float(c), float(d[(n - 1) // 2]), float(v.astype(np.float64).std()), n


ROWS = {
    "odd": [5.0, 1.0, 9.0, 3.0, 7.0],
    "even": [4.0, 8.0, 2.0, 6.0, NAN],            # n = 4: the LOWER of 4 and 6
    "one": [NAN, 2.5, NAN, NAN, NAN],
    "all_nan": [NAN] * 5,
    "ties": [3.0, 3.0, 1.0, 3.0, 7.0],
    "mixed_signs": [-2.0, 0.5, -0.25, 3.0, -7.0],
    "zeros": [0.0, -0.0, 1.0, -1.0, 0.0],
}


def test_reference_matches_a_plain_sort():
    y = np.array(list(ROWS.values()), dtype=np.float32)
    st = rb_ref.robust_stats(torch.tensor(y))
    for i, name in enumerate(ROWS):
        c, mad, std, n = _sorted_reference(y[i])
        assert float(st.count[i]) == n, name
        if n == 0:
            assert all(bool(torch.isnan(t[i])) for t in (st.center, st.mad, st.sigma, st.std)), name
            continue
        assert float(st.center[i]) == c and float(st.mad[i]) == mad, name
        assert float(st.std[i]) == pytest.approx(std, rel=1e-5, abs=1e-6), name
        want = float(np.float32(1.4826) * np.float32(mad)) if mad > 0 else std
        assert float(st.sigma[i]) == pytest.approx(want, rel=1e-5 if mad == 0 else 0, abs=1e-6 if mad == 0 else 0), name
    assert float(st.center[1]) == 4.0       # never the average of the two middle values
    assert float(st.mad[2]) == 0.0 and float(st.sigma[2]) == 0.0   # one sample: mad 0, std 0


def test_reference_on_random_rows_and_window():
    rng = np.random.default_rng(5)
    y = rng.normal(0, 3, (40, 37)).astype(np.float32)
    y[rng.random(y.shape) < 0.1] = np.nan
    for window in (None, 16, 36):
        st = rb_ref.robust_stats(torch.tensor(y), window)
        yw = y if window is None else y[:, -window:]
        for i in range(y.shape[0]):
            c, mad, _std, n = _sorted_reference(yw[i])
            assert (float(st.center[i]), float(st.mad[i]), float(st.count[i])) == (c, mad, n)


def test_contamination_moves_std_not_the_robust_band():
    """An earlier incident (48 points at x3, 400 points before the window's end) widens the
    std band on every series and leaves the median / MAD band where it was."""
    T = 2016
    clean = synthetic_history(256, T, 288, "cpu", seed=0)
    dirty = clean.clone()
    dirty[:, T - 448:T - 400] *= 3
    a, b = rb_ref.robust_stats(clean), rb_ref.robust_stats(dirty)
    r_rob = b.sigma / a.sigma
    r_std = b.std / a.std
    shift = (b.center - a.center).abs() / a.sigma
    print(f"robust ratio {float(r_rob.min()):.3f}..{float(r_rob.max()):.3f}  std ratio "
          f"{float(r_std.min()):.3f}..{float(r_std.max()):.3f}  centre shift max {float(shift.max()):.3f} sigma")
    assert bool((a.mad > 0).all() and (b.mad > 0).all())
    assert bool((r_rob <= 1.15).all())
    assert bool((r_rob < r_std).all())
    assert bool((shift <= 0.2).all())


def test_fallback_to_std_when_more_than_half_the_samples_are_equal():
    g = torch.Generator().manual_seed(3)
    y = torch.where(torch.rand(16, 500, generator=g) < 0.3, torch.rand(16, 500, generator=g) * 5 + 0.5,
                    torch.zeros(16, 500))
    st = rb_ref.robust_stats(y)
    assert bool((st.mad == 0).all()) and bool((st.center == 0).all())
    assert torch.equal(st.sigma, ma_ref.window_stats(y).std) and bool((st.sigma > 0.5).all())


# ------------------------------------------------------------------ wiring
@pytest.mark.parametrize("name", NAMES)
def test_names_are_configuration_values(name):
    assert name in config_mod.ALGORITHMS and name in plans.UNIVARIATE and name in plans.ALGORITHMS
    assert name not in plans.JOINT_ALGORITHMS
    cfg = BrainConfig.from_env(dict(reference_default_env(), ML_ALGORITHM=name.upper(), FOREMAST_MA_WINDOW="48"))
    assert cfg.algorithm == name and cfg.ma_window == 48


def _history(N, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    y = 40 + 6 * torch.sin(torch.arange(T) / 9.0)[None] + torch.randn(N, T, generator=g)
    y[:, :T // 2] += 25.0          # the older half sits higher: the last-window statistics differ
    y[1, 5:40] = NAN
    y[2] = torch.where(torch.rand(T, generator=g) < 0.3, torch.ones(T) * 4, torch.zeros(T))  # mad == 0
    return y


def _cfg(name, ma_window=50):
    cfg = BrainConfig()
    cfg.algorithm = name
    cfg.min_historical_points = 10
    cfg.ma_window = ma_window
    return cfg


@pytest.mark.parametrize("name", NAMES)
def test_cpu_streaming_shard_scores_the_reference(name):
    N, T, W = 6, 160, 4
    y = _history(N, T)
    cur = y[:, -W:].clone() + 0.1
    cur[3, 2] += 60.0
    cfg = _cfg(name)
    sh = StreamingShard(ShardSpec(n_series=N, ring_len=T, season=24, pods=1, window=W, algorithm=name,
                                  pairwise="NONE", dtype=torch.float32), cfg, device="cpu")
    sh.load_history(y)
    for c in range(W):
        sh.ingest_tick(cur[:, c:c + 1].contiguous())
    out = sh.score()
    hist = sh.hist.logical().float()
    st = rb_ref.robust_stats(hist, cfg.ma_window if name == "robust_average" else None)
    f = st.center[:, None].expand(-1, W)
    d = det_ref.detect(f, st.sigma, sh.cur.data, sh.thr_full, sh.bound, sh.min_lower,
                       pairwise_scale=cfg.pairwise_scale, model_ok=st.count >= cfg.min_historical_points,
                       threshold_low=sh.thr_low, pw_min_points=cfg.pairwise_min_points)
    assert torch.equal(out["verdict"], d.verdict) and torch.equal(out["count"], d.count)
    assert torch.equal(out["upper"], d.upper) and torch.equal(out["lower"], d.lower)
    for k, t in (("center", st.center), ("sigma", st.sigma), ("mad", st.mad)):
        assert torch.equal(out[k], t), k
    assert int(out["verdict"][3]) == 1 and float(out["mad"][2]) == 0.0
    # FOREMAST_MA_WINDOW: the windowed scorer sees only the last 50 points, all of the lower half
    rows = [0, 1, 3, 4, 5]
    whole = rb_ref.robust_stats(hist)
    if name == "robust_average":
        assert bool((out["center"][rows] < whole.center[rows]).all()) and bool((st.count == 50).all())
    else:
        assert torch.equal(out["center"], whole.center)


@pytest.mark.parametrize("name", NAMES)
def test_streaming_monitor_keeps_the_name(name):
    from foremast_amd.brain.streaming import StreamingMonitor
    from foremast_amd.store.jobstore import MemoryJobStore
    brain = StreamingMonitor(MemoryJobStore(), cfg=_cfg(name), device="cpu", ring_len=192, step=1800.0, window=4)
    assert brain._new_shard(4).algorithm == name


@pytest.mark.parametrize("name", NAMES)
def test_cpu_batch_scorer_scores_the_reference(name):
    N, T, C = 6, 160, 5
    y = _history(N, T, seed=2)
    cur = (y[:, -C:] + 0.1).numpy().astype(np.float32)
    cur[4, 1] += 80.0
    cfg = _cfg(name)
    tasks = [MetricTask(job_id="j", alias=f"m{i}", metric=f"m{i}", namespace="ns", app="a", step=60.0,
                        hist=y[i].numpy().astype(np.float32), hist_end=0.0,
                        cur_ts=60.0 * (1 + np.arange(C, dtype=np.float64)), cur_vals=cur[i], threshold=3.0, bound=3)
             for i in range(N)]
    res = BatchScorer(cfg, device=torch.device("cpu")).score(tasks)
    st = rb_ref.robust_stats(y, cfg.ma_window if name == "robust_average" else None)
    thr_f, thr_l = det_ref.effective_thresholds(torch.full((N,), 3.0), torch.full((N,), 3, dtype=torch.int8),
                                                torch.full((N,), float(C), dtype=torch.float64),
                                                cfg.pairwise_scale, cfg.window_correction)
    d = det_ref.detect(st.center[:, None].expand(N, C), st.sigma, torch.from_numpy(cur), thr_f,
                       torch.full((N,), 3, dtype=torch.int8), torch.zeros(N),
                       pairwise_scale=cfg.pairwise_scale, model_ok=st.count >= cfg.min_historical_points,
                       threshold_low=thr_l, pw_min_points=cfg.pairwise_min_points,
                       shift_threshold=cfg.pairwise_shift, shift_min_points=cfg.pairwise_shift_min_points,
                       shift_sigma=st.sigma if cfg.pairwise_shift_one_step else None)
    assert [r.verdict for r in res] == d.verdict.tolist() and res[4].verdict == 1
    assert all(r.model == name for r in res)
    for i, r in enumerate(res):
        np.testing.assert_array_equal(r.upper, d.upper[i].numpy())
        np.testing.assert_array_equal(r.lower, d.lower[i].numpy())


@pytest.mark.parametrize("name", NAMES)
def test_cpu_rollout_fit_state(name):
    from foremast_amd.brain.rollout import HB, RolloutMonitor
    from foremast_amd.store.jobstore import MemoryJobStore
    N, R, head, length = 6, 200, 150, 160     # the window wraps
    y = _history(N, length, seed=4)
    ring = torch.full((N, R), 7.0)
    ring[:, (head + torch.arange(length)) % R] = y
    cfg = _cfg(name)
    mon = RolloutMonitor(MemoryJobStore(), cfg=cfg, device="cpu")
    assert mon._algo_for(length) == name
    s = mon._fit_state(ring, head, length)
    st = rb_ref.robust_stats(y, cfg.ma_window if name == "robust_average" else None)
    assert set(s) == {"level", "trend", "season_hb", "sigma", "nvalid", "best"}
    assert torch.equal(s["level"], st.center) and torch.equal(s["sigma"], st.sigma)
    assert torch.equal(s["nvalid"], st.count) and bool((s["best"] == -1).all())
    assert not s["trend"].any() and not s["season_hb"].any() and s["season_hb"].shape == (N, HB)


@pytest.mark.parametrize("name", NAMES)
def test_rollout_jobs_are_planned(name):
    clock, prom, store, ids = rw.world()
    docs = [store.get(ids[app]) for app in ids]
    got = plans.plan_many(docs, name)
    assert [p.app for p in got] == [(rw.NS, app) for app in ids]
    assert plans.plan_rollout(dict(docs[0], id="other"), name).n == 2
    assert plans.plan_many([dict(d, id="x" + d["id"]) for d in docs], "robust") == [None] * 3   # no such name


@pytest.mark.parametrize("name", NAMES)
def test_cpu_rollout_engine_admits_and_scores_like_the_worker(name):
    """The three-app scenario of tests/test_rollout.py: admission fits the median / MAD state,
    the spike at T0 + 120 fails app a's canary, the others finish healthy; the per-job
    worker with the batch scorer reaches the same statuses."""
    out, docs, ids, mon, _hq = rw.run_monitor("cpu", name)
    assert out[rw.T0 + 120] == {ids["a"]: r.ST_COMPLETED_UNHEALTH}, out
    assert out["end"] == {ids["b"]: r.ST_COMPLETED_HEALTH, ids["c"]: r.ST_COMPLETED_HEALTH}
    worker = rw.run_worker(name)
    assert {a: d["status"] for a, d in worker.items()} == {a: d["status"] for a, d in docs.items()}
