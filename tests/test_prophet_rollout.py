"""ML_ALGORITHM=prophet on the resident rollout engine, CPU side: the harmonic forecast state
(models/prophet_lite.py window_state / forecast_state) against the window-scaled model it is
derived from, the plan, the three-app scenario of tests/test_rollout.py on the engine's CPU
path, and the bound of the kernel-table cache."""

import importlib.util
import json
import os

import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.brain import plans
from foremast_amd.models import prophet_lite as pl


def _helper(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pc = _helper("prophet_cases")
rw = _helper("rollout_world")

M = 24
STATE_TOL = 1e-10   # of the row's level scale (fp64: the identity is exact up to rounding)


def _horizons(m):
    return torch.tensor([1, 2, 16, 17, 64, 65, m - 1, m, m + 1, 7 * m, 7 * m + 1, 10 ** 5], dtype=torch.int64)


# T - 1 just below and exactly at 2 m (daily terms) and 14 m (weekly terms)
@pytest.mark.parametrize("T,P", [(2 * M, 12), (2 * M + 1, 20), (14 * M, 20), (14 * M + 1, 26)])
def test_state_equals_window_forecast(T, P):
    y, pat = pc.make_rows(T, M, 2 * len(pc.PATTERNS), seed=3, bf16=False)
    assert "dense" in pat and "miss60" in pat and "outage20" in pat
    fit = pl.fit_prophet_window(y, M)
    assert fit.beta.shape[1] == P
    level, slope, harm = pl.window_state(fit)
    assert level.dtype == torch.float64 and harm.shape == (y.shape[0], 14)
    if P < 26:
        assert not bool(harm[:, 8:].any())      # weekly terms the window does not enable
    if P < 20:
        assert not bool(harm.any())
    hz = _horizons(M)
    got = pl.forecast_state(level, slope, harm, M, hz)
    # forecast_window's arithmetic without its cast to fp32
    XH = pl._window_features(float(T - 1) + hz.double(), T, M, fit.n_changepoints, fit.cp_range)
    want = fit.beta @ XH.T
    scale = torch.nan_to_num(y.double(), nan=0.0).abs().max(1).values.clamp(min=1e-30)
    err = ((got - want).abs().max(1).values / scale).max()
    print(f"T={T} P={P}: worst |state - window| = {float(err):.2e} of the level scale")
    assert float(err) <= STATE_TOL
    assert torch.equal(pl.forecast_window(fit, hz), want.float())
    # per-row horizons give the same values
    rows = hz[None, :].expand(y.shape[0], -1).contiguous()
    assert torch.equal(pl.forecast_state(level, slope, harm, M, rows), got)


def test_state_needs_changepoints_inside_the_window():
    y, _ = pc.make_rows(2 * M + 1, M, 3, seed=3, bf16=False)
    fit = pl.fit_prophet_window(y, M, cp_range=1.0)
    with pytest.raises(ValueError):
        pl.window_state(fit)
    pl.window_state(pl.fit_prophet_window(y, M, cp_range=0.99))


def test_prophet_jobs_are_planned():
    clock, prom, store, ids = rw.world()
    for app in ids:
        p = plans.plan_rollout(store.get(ids[app]), "prophet")
        assert p is not None and p.app == (rw.NS, app)
    assert "prophet" in plans.UNIVARIATE


_RUNS = {}


def _engine_run(device):
    if device not in _RUNS:
        _RUNS[device] = rw.run_monitor(device, "prophet", ring_len=4320)   # 3 days of minutes: daily terms
    return _RUNS[device]


def _check_scenario(out, docs, ids, mon, hq):
    T0 = rw.T0
    assert mon.prophet and mon.state["harm"].shape[1] == 14
    # the spike starts at T0+120: the tick that ingests that minute fails the canary job of app a
    assert out[T0 + 120] == {ids["a"]: r.ST_COMPLETED_UNHEALTH}, out
    info = json.loads(docs["a"]["anomalyInfo"])
    assert set(info) == {"error5xx"}
    vals = info["error5xx"]["values"]
    assert vals[1] > 30 and vals[0] >= T0 + 120
    assert out[T0 + 300] == {}
    assert out["end"] == {ids["b"]: r.ST_COMPLETED_HEALTH, ids["c"]: r.ST_COMPLETED_HEALTH}
    assert hq["admitted"] > 0 and hq["end"] == hq["admitted"]      # resident: never refetched


def test_rollout_monitor_prophet_cpu():
    out, docs, ids, mon, hq = _engine_run("cpu")
    _check_scenario(out, docs, ids, mon, hq)
    # a 4320-minute ring enables the daily terms: the state carries them
    assert mon.history.R - 1 >= 2 * mon.season


def test_rollout_monitor_prophet_matches_brain_worker():
    _out, docs, ids, _mon, _hq = _engine_run("cpu")
    ref = rw.run_worker("prophet")
    for app in ids:
        assert ref[app]["status"] == docs[app]["status"], app


def test_table_cache_is_bounded():
    from foremast_amd.ops import kernels as K
    bound = K.PROPHET_TABLES_MAX
    assert 1 <= bound <= 16
    cpu = torch.device("cpu")

    def held():
        return [k for k in K._PROPHET_TABLES if k[-2] == "cpu"]
    first = K.prophet_tables(50, M, cpu)
    for T in range(51, 51 + bound + 3):
        K.prophet_tables(T, M, cpu)
        K.prophet_tables(50, M, cpu)                    # in use every time: never the one evicted
        assert len(held()) <= bound
    assert len(held()) == bound
    assert K.prophet_tables(50, M, cpu) is first
    assert K.prophet_tables(51 + bound + 2, M, cpu)["state"].shape == (26,)
    assert not any(k[0] == 51 for k in held())          # the least recently used geometry left
