"""Window-scaled prophet reference (models/prophet_lite.py fit_prophet_window) and its
use by the streaming engines on the CPU."""

import importlib.util
import math
import os

import pytest
import torch

from foremast_amd.models import detect as det_ref
from foremast_amd.models import prophet_lite as pl

_spec = importlib.util.spec_from_file_location(
    "prophet_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "prophet_cases.py"))
pc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pc)

HZ = torch.arange(1, 11)


@pytest.mark.parametrize("T,m,step", [(704, 288, 300.0), (720, 48, 1800.0)])
def test_window_fit_matches_batch_fit_when_the_window_ends_are_valid(T, m, step):
    """Rows whose first and last samples are valid: time scaled by the window is time
    scaled by the series, so the two models coincide (up to the Fourier phase origin)."""
    y, pat = pc.make_rows(T, m, 12, seed=3, bf16=False, patterns=("dense", "miss1", "outage20"))
    assert not torch.isnan(y[:, 0]).any() and not torch.isnan(y[:, -1]).any()
    N = y.shape[0]
    end = torch.full((N,), 1.7e9 + 123.0, dtype=torch.float64)
    old = pl.fit_prophet(y, end, torch.full((N,), step, dtype=torch.float64))
    f_old = pl.forecast(old, end[:, None] + HZ[None].double() * step).double()
    new = pl.fit_prophet_window(y, m)
    # compare in fp64: the float32 forecasts the public functions return round at 6e-8 of the level
    XH = pl.design_window(T, m, 10)[1]
    f_new = new.beta @ XH.T
    assert torch.allclose(pl.forecast_window(new, HZ).double(), f_new, rtol=1e-6, atol=0)
    err = (f_new - f_old).abs().max(1).values / new.sigma.double()
    print("window vs batch fit, worst forecast difference / sigma:", float(err.max()))
    # f_old is float32: allow its rounding (6e-8 of the level, sigma is ~2e-2 of it)
    assert float(err.max()) < 1e-4
    assert torch.equal(new.n_valid, old.n_valid)
    assert torch.allclose(new.sigma, old.sigma, rtol=1e-5)


def test_fourier_phase_origin_is_free():
    T, m = 720, 48
    y, _ = pc.make_rows(T, m, 10, seed=4, bf16=False, patterns=("dense", "miss1", "outage20", "lead_third", "trail7"))
    a = pl.fit_prophet_window(y, m)
    b = pl.fit_prophet_window(y, m, phase=17.3)
    XHa = pl.design_window(T, m, 10)[1]
    XHb = pl.design_window(T, m, 10, phase=17.3)[1]
    fa, fb = a.beta @ XHa.T, b.beta @ XHb.T
    err = (fa - fb).abs().max(1).values / a.sigma.double()
    assert float(err.max()) < 1e-6
    assert torch.allclose(a.sigma, b.sigma, rtol=1e-6)
    assert torch.allclose(pl.forecast_window(b, HZ).double(), fb, rtol=1e-6, atol=0)


def test_term_count_at_the_season_boundaries():
    m = 48
    for T, P in ((2 * m, 12), (2 * m + 1, 20), (14 * m, 20), (14 * m + 1, 26)):
        X, XH, reg, A = pl.design_window(T, m, 3)
        assert X.shape == (T, P) and XH.shape == (3, P) and reg.shape == (P,) and A.shape == (P, P)
        assert pl.fit_prophet_window(torch.ones(1, T), m).beta.shape == (1, P)
        assert pc.n_terms(T, m) == P
    X, XH, reg, A = pl.design_window(97, 48, 2)
    assert torch.equal(reg[2:12], torch.full((10,), 10.0, dtype=torch.float64))
    assert float(reg[0]) == 1e-4 and float(reg[-1]) == 1e-4
    assert torch.allclose(A, X.T @ X + torch.diag(reg))
    # the horizon rows continue the window: XH[h-1] is the feature row of logical index T-1+h
    X2 = pl.design_window(99, 48, 1)[0]
    s_scale = 98.0 / 96.0  # scaled time of the longer window, in units of the shorter one
    assert math.isclose(float(XH[1, 1]), float(X2[98, 1]) * s_scale, rel_tol=1e-12)


def test_per_series_horizons_and_degenerate_rows():
    T, m = 704, 288
    y, pat = pc.make_rows(T, m, 18, seed=5, bf16=True)
    fit = pl.fit_prophet_window(y, m)
    g = torch.Generator().manual_seed(0)
    hz = torch.randint(1, 17, (18, 6), generator=g)
    f = pl.forecast_window(fit, hz)
    for i in (0, 7, 13):
        assert torch.equal(f[i], pl.forecast_window(fit, hz[i])[i])
    assert torch.isfinite(fit.beta).all() and torch.isfinite(fit.sigma).all()
    i = pat.index("all_nan")
    assert int(fit.n_valid[i]) == 0 and float(fit.sigma[i]) == 0 and not fit.beta[i].any()
    i = pat.index("exact_p")
    assert int(fit.n_valid[i]) == fit.beta.shape[1]


@pytest.mark.parametrize("T,m,bf16,N", [(704, 288, True, 36), (720, 48, False, 36), (10080, 1440, True, 18)])
def test_fp32_emulation_of_the_kernel_stays_within_margin(T, m, bf16, N):
    """fp32 tables, fp32 accumulation (sequential over the window, the pessimistic order: the
    kernel sums 32-sample partials per wave), fp32 Cholesky, both forms of the normal
    matrix.  The GPU test's tolerances (5e-3 sigma, 1e-3) are ten times the worst case the
    issue measured; this keeps that margin reproducible."""
    y, pat = pc.make_rows(T, m, N, seed=1, bf16=bf16)
    ref = pl.fit_prophet_window(y, m)
    fr = pl.forecast_window(ref, HZ)
    s = ref.sigma.clamp(min=1e-30)
    for down in (None, True, False):
        if down is False and T > 5000:
            continue  # summing 10,080 outer products per row on the CPU: covered at the short windows
        # a forced form only on the issue's five patterns (a window that is mostly missing
        # leaves nothing of A_dense to downdate from: the kernel takes the smaller side there)
        rows = [i for i, p in enumerate(pat)
                if down is None or p in ("dense", "miss1", "outage20", "lead_third", "trail7")]
        fc, sg, be, fails = pc.emulate_fp32(y[rows], m, HZ, downdate=down)
        assert fails == 0
        ef = (fc - fr[rows]).abs().max(1).values / s[rows]
        es = (sg - ref.sigma[rows]).abs() / s[rows]
        print(f"T={T} downdate={down}: forecast {float(ef.max()):.2e} sigma, sigma {float(es.max()):.2e}")
        assert float(ef.max()) <= 1e-3
        assert float(es.max()) <= 2e-4
        assert torch.isfinite(fc).all() and torch.isfinite(sg).all()


def _shard(algorithm, N, T, m, W, y, cur):
    from foremast_amd.brain.engine import ShardSpec, StreamingShard
    from foremast_amd.utils.config import BrainConfig
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    sh = StreamingShard(ShardSpec(n_series=N, ring_len=T, season=m, pods=1, window=W, algorithm=algorithm,
                                  pairwise="NONE", dtype=torch.float32), cfg, device="cpu")
    sh.load_history(y)
    for c in range(W):
        sh.ingest_tick(cur[:, c:c + 1].contiguous())
    return sh, cfg


def test_cpu_shard_scores_the_prophet_model():
    T, m, W, N = 192, 48, 4, 8
    t = torch.arange(T + 2 * W, dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    full = 50 + 20 * torch.sin(2 * math.pi * t / m)[None] + torch.randn(N, T + 2 * W, generator=g)
    y, cur = full[:, :T].clone(), full[:, T:T + W].clone()
    y[1, 30:50] = float("nan")
    cur[2, 1] += 40.0
    sh, cfg = _shard("prophet", N, T, m, W, y, cur)
    out = sh.score()
    hist = sh.hist.logical().float()
    fit = pl.fit_prophet_window(hist, m)
    f = pl.forecast_window(fit, sh.horizons.long())
    d = det_ref.detect(f, fit.sigma, sh.cur.data, sh.thr_full, sh.bound, sh.min_lower,
                       pairwise_scale=cfg.pairwise_scale, model_ok=fit.n_valid >= cfg.min_historical_points,
                       threshold_low=sh.thr_low, pw_min_points=cfg.pairwise_min_points)
    assert torch.equal(out["verdict"], d.verdict) and torch.equal(out["count"], d.count)
    assert torch.equal(out["forecast"], f) and torch.equal(out["upper"], d.upper)
    assert torch.equal(out["sigma"], fit.sigma)
    assert int(out["verdict"][2]) == 1
    ma, _ = _shard("moving_average_all", N, T, m, W, y, cur)
    # a daily swing of +-20 around 50: the moving average's forecast is flat, the model's is not
    assert float((out["forecast"] - ma.score()["forecast"]).abs().max()) > 5.0


def test_streaming_monitor_serves_prophet():
    from foremast_amd.brain.streaming import StreamingMonitor
    from foremast_amd.store.jobstore import MemoryJobStore
    from foremast_amd.utils.config import BrainConfig
    cfg = BrainConfig()
    cfg.algorithm = "prophet"
    brain = StreamingMonitor(MemoryJobStore(), cfg=cfg, device="cpu", ring_len=192, step=1800.0, window=4)
    sh = brain._new_shard(4)
    assert sh.algorithm == "prophet" and sh.spec.season == 48
