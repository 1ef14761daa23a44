"""Holt-Winters variant 5 on float32 rings (hw_scan.hip: ``hw_d_kernel``, ``hw_q_kernel`` and
``hw_dg_kernel`` instantiated for an fp32 ring element).  Only the staging reads the ring, so
every check is the one the bf16 tests already apply against the fp64 reference fitted on the
ring's own values (tests/test_hw_gaps.py), plus the dispatch, the fp32 aligned staging at a
16-mod-32 row base, the bf16-representable twin and the case fp32 rings are for: a steady
gauge at a level where bf16's step exceeds the noise."""

import numpy as np
import pytest
import torch

from foremast_amd.models import smoothing as sm_ref
from tests.test_hw_gaps import _GEOMETRY, GRID, _gapped
from tests.test_kernels_gpu import _assert_near_optimal, _ref_detect, _ring, _series
from tests.test_ring_dtype import steady_gauge

pytestmark = pytest.mark.gpu

F32 = torch.float32
KEYS = ("best", "level", "trend", "sigma", "verdict", "count", "forecast")


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


def _spec(K, y, N, C, hz, dev, scale=1.05):
    cur = torch.tensor(np.nan_to_num(y[:, -C:], nan=20.0) * scale, device=dev)
    return cur, K.DetectSpec(horizons=hz.to(dev), threshold=torch.full((N,), 2.0, device=dev),
                             bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                             min_lower=torch.full((N,), -1e30, device=dev), cur=cur, max_horizon=int(hz.max()))


def _fit(K, ring, head, T, m, spec, **kw):
    o = K.smoothing_fit(ring, head, T, sm_ref.MODE_HW, m, GRID.to(ring.device), spec, variant=5, **kw)
    torch.cuda.synchronize()
    assert K.last_hw_variant == 5
    return {k: v.clone() for k, v in o.items()}


def _fit_both_prunes(K, monkeypatch, ring, head, T, m, spec):
    """The fit with the branch and bound on and off: bit-identical; returns the first."""
    outs = []
    for prune in ("1", "0"):
        monkeypatch.setenv("FOREMAST_HW_PRUNE", prune)
        outs.append(_fit(K, ring, head, T, m, spec))
    monkeypatch.delenv("FOREMAST_HW_PRUNE")
    for key in KEYS:
        assert torch.equal(outs[0][key], outs[1][key]), key
    return outs[0]


def _check_against_reference(out, yl, m, hz, cur, tag):
    """The bounds of the bf16 tests against the fp64 reference on the ring's own values."""
    ref = sm_ref.fit_smoothing(torch.tensor(yl, dtype=torch.float64), sm_ref.MODE_HW, GRID.double(), m=m)
    kb = out["best"].cpu().long()
    same = (kb == ref.best).numpy()
    sig = out["sigma"].cpu().numpy()
    print(f"{tag}: same {same.mean():.3f} sigma rel err {np.abs(sig / ref.sigma.numpy() - 1).max():.2e}")
    assert same.mean() >= 0.75
    # where the kernel chose the reference's grid point its SSE is the optimum: the per-point
    # fp64 fits of _assert_near_optimal are needed only for the series where it did not
    if not same.all():
        _assert_near_optimal(yl[~same], GRID, sm_ref.MODE_HW, m, kb[torch.tensor(~same)])
    np.testing.assert_allclose(sig, ref.sigma.numpy(), rtol=5e-3)
    np.testing.assert_allclose(out["level"].cpu().numpy()[same], ref.level.numpy()[same], rtol=2e-3, atol=5e-3)
    np.testing.assert_allclose(out["trend"].cpu().numpy()[same], ref.trend.numpy()[same], rtol=2e-2, atol=2e-4)
    f_ref = sm_ref.forecast(ref, hz.long())
    np.testing.assert_allclose(out["forecast"].cpu().numpy()[same], f_ref.numpy()[same], rtol=5e-3, atol=2e-2)
    d = _ref_detect(out, GRID, sm_ref.MODE_HW, m, hz, cur)
    assert torch.equal(d.count, out["count"].cpu())
    assert torch.equal(d.verdict, out["verdict"].cpu())
    return ref


# ---- case 1: dispatch ---------------------------------------------------------------------
@pytest.mark.parametrize("m,T,quad", [(1440, 10080, "1"), (288, 2016, "1"), (288, 2016, "0")],
                         ids=["60s", "300s-quad", "300s-pair"])
def test_fp32_ring_is_fitted_by_variant5(K, m, T, quad, monkeypatch):
    """An fp32 ring at the 60 s and 300 s steps takes variant 5 (it fell to variant 3), on the
    quad path and, with FOREMAST_HW_QUAD=0, on the pair path at K = 9."""
    dev = torch.device("cuda:0")
    N = 6
    monkeypatch.setenv("FOREMAST_HW_QUAD", quad)
    y = _series(N, T, m, seed=5)
    hz = torch.tensor([1, 2, 1, 2], dtype=torch.int32)
    cur, spec = _spec(K, y, N, 4, hz, dev)
    K.hw_clear_gap_flags()
    out = K.smoothing_fit(torch.tensor(y, device=dev), 0, T, sm_ref.MODE_HW, m, GRID.to(dev), spec)
    torch.cuda.synchronize()
    assert K.last_hw_variant == 5
    assert torch.isfinite(out["sigma"]).all()


# ---- case 2: parity at m = 1440 -----------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "miss1e-3", "outage30", "boundary", "season"])
def test_fp32_ring_matches_reference_at_60s(K, case, monkeypatch):
    dev = torch.device("cuda:0")
    m, N, T = 1440, 18, 10080
    R, head = T + 64, 1064                             # aligned ring, head mid-ring: chunked staging
    y = _gapped(case, N, T, seed=len(case) * 13)       # "dense" is no case of _gapped: no gaps
    ring = torch.tensor(_ring(y, R, head), device=dev)
    assert ring.dtype == F32 and R % 8 == 0 and ring.stride(0) % 8 == 0 and ring.data_ptr() % 16 == 0
    yl = ring.cpu().numpy()[:, (head + np.arange(T)) % R]
    hz = torch.arange(1, 11, dtype=torch.int32).repeat(5)
    cur, spec = _spec(K, y, N, 50, hz, dev)
    K.hw_clear_gap_flags()
    before = K.hw_deferred_total(dev)
    out = _fit(K, ring, head, T, m, spec)
    gapped_pairs = int(np.isnan(yl[:, m:]).reshape(N // 2, -1).any(1).sum())
    assert (gapped_pairs > 0) == (case != "dense")
    assert K.hw_deferred_total(dev) - before == gapped_pairs
    # the next fit of the same data: flagged pairs go straight to the gapped kernel, same bits
    again = _fit(K, ring, head, T, m, spec)
    for key in KEYS:
        assert torch.equal(again[key], out[key]), key
    # the branch and bound is exact (the gap flags of the fits above stay: same kernels per pair)
    monkeypatch.setenv("FOREMAST_HW_PRUNE", "0")
    full = _fit(K, ring, head, T, m, spec)
    for key in KEYS:
        assert torch.equal(full[key], out[key]), key
    _check_against_reference(out, yl, m, hz, cur, f"60s-{case}")


# ---- case 3: staging geometry -------------------------------------------------------------
def _base16_ring(y, R, head, dev):
    """A ring whose rows are 32-byte multiples but whose base is 16 mod 32: the fp32 aligned
    path's two 16-byte loads per season must not assume a 32-byte chunk address."""
    N = y.shape[0]
    assert R % 8 == 0
    buf = torch.empty(N * R + 4, dtype=F32, device=dev)  # allocations are 32-byte aligned
    ring = buf[4:].view(N, R)
    ring.copy_(torch.tensor(_ring(y, R, head)))
    assert ring.data_ptr() % 32 == 16 and ring.stride(0) == R
    return ring


def _strided_ring(y, R, head, dev):
    """Rows of stride R + 4 (not a multiple of 8) over an R that is: the per-element path."""
    N = y.shape[0]
    buf = torch.full((N, R + 4), 7.0, dtype=F32, device=dev)
    ring = buf[:, :R]
    ring.copy_(torch.tensor(_ring(y, R, head)))
    assert ring.stride(0) % 8 != 0 and ring.stride(1) == 1
    return ring


_FP32_GEOMETRY = [g + ("plain",) for g in _GEOMETRY] + [
    # R = 1072 = 8 x 134, phi = 4 (as chunk_wrap), base 16 mod 32; then an unaligned row stride
    ("base16",       288,  9, 3 * 288 + 100, 108, 1000, False, "base16"),
    ("base16",       1440, 5, 2 * 1440 + 100, 28, 1000, True,  "base16"),
    ("row_stride",   288,  9, 3 * 288 + 100, 108, 1000, False, "stride"),
    ("row_stride",   1440, 5, 2 * 1440 + 100, 28, 1000, True,  "stride")]


@pytest.mark.parametrize("case,m,N,T,extra,head,outage,layout", _FP32_GEOMETRY,
                         ids=[f"{g[0]}-{g[1]}" for g in _FP32_GEOMETRY])
def test_fp32_staging_geometry_matches_reference(K, case, m, N, T, extra, head, outage, layout, monkeypatch):
    """The geometry cases of the bf16 staging with fp32 rings, and the two that are new with
    them: a row base of 16 mod 32 on the aligned path and a row stride that is no multiple of
    8 (per-element loads), each on the quad kernel (m = 288) and on the pair kernel with a
    gapped pair (m = 1440)."""
    dev = torch.device("cuda:0")
    R = T + extra
    y = _series(N, T, m, seed=51 + len(case))
    if outage:
        y[::3, 2 * m + 17:2 * m + 23] = np.nan            # 6 points past season 0
    make = {"plain": lambda: torch.tensor(_ring(y, R, head), device=dev),
            "base16": lambda: _base16_ring(y, R, head, dev),
            "stride": lambda: _strided_ring(y, R, head, dev)}[layout]
    ring = make()
    assert ring.dtype == F32
    aligned = R % 8 == 0 and ring.stride(0) % 8 == 0 and ring.data_ptr() % 16 == 0
    assert aligned == (case in ("chunk_wrap", "two_seasons", "base16"))
    yl = ring.cpu().numpy()[:, (head + np.arange(T)) % R]
    hz = torch.tensor([1, 2, 1, 2, 1, 2, 1, 2], dtype=torch.int32)
    cur, spec = _spec(K, y, N, 8, hz, dev)
    K.hw_clear_gap_flags()
    before = K.hw_deferred_total(dev)
    out = _fit_both_prunes(K, monkeypatch, ring, head, T, m, spec)
    assert (K.hw_deferred_total(dev) > before) == outage
    _check_against_reference(out, yl, m, hz, cur, f"{case}-{m}")


# ---- case 4: the bf16-representable twin --------------------------------------------------
@pytest.mark.parametrize("m,N", [(1440, 18), (288, 23)])
def test_fp32_ring_of_bf16_values_matches_the_bf16_ring(K, m, N):
    """The same bf16-representable values from a bf16 and from an fp32 ring: the arithmetic
    after staging is the same source, so verdict and count are equal and the parameters agree
    bit for bit unless -ffp-contract=fast contracted the two instantiations differently; then
    within the bounds the project accepts between two variant-5 kernels
    (test_quad_kernel_matches_pair_kernel_at_300s).  docs/PERF.md records which it was."""
    dev = torch.device("cuda:0")
    T = 7 * m
    y = _series(N, T, m, seed=43)
    y[::4, 2 * m + 100:2 * m + 106] = np.nan              # some pairs through the gapped kernel too
    r16 = torch.tensor(y, device=dev).to(torch.bfloat16)
    r32 = r16.float()
    C = 8
    hz = torch.arange(1, C + 1, dtype=torch.int32)
    cur, spec = _spec(K, y, N, C, hz, dev)
    K.hw_clear_gap_flags()
    o16 = _fit(K, r16, 0, T, m, spec)
    K.hw_clear_gap_flags()
    o32 = _fit(K, r32, 0, T, m, spec)
    assert torch.equal(o16["verdict"], o32["verdict"]) and torch.equal(o16["count"], o32["count"])
    exact = {k: bool(torch.equal(o16[k], o32[k])) for k in ("best", "level", "trend", "sigma", "forecast")}
    print(f"twin m={m}: bit-equal {exact}")
    if all(exact.values()):
        return
    same = (o16["best"] == o32["best"]).cpu().numpy()
    assert same.mean() >= 0.95
    np.testing.assert_allclose(o32["sigma"].cpu().numpy(), o16["sigma"].cpu().numpy(), rtol=1e-3)
    np.testing.assert_allclose(o32["level"].cpu().numpy()[same], o16["level"].cpu().numpy()[same],
                               rtol=1e-4, atol=1e-3)


# ---- case 5: the quality case -------------------------------------------------------------
def test_fp32_ring_halves_the_band_of_a_steady_gauge(K):
    """A gauge at level 3000 with daily amplitude 10 and noise 1: bf16's step there is 16, so
    the bf16 ring's sigma is rounding noise.  The fp32-ring fit matches the reference, and
    every series' bf16-ring sigma exceeds 1.9 x its fp32-ring sigma (the reference alone gives
    >= 1.96 for this seed, tests/test_ring_dtype.py; both kernels are within 5e-3 of it)."""
    dev = torch.device("cuda:0")
    m, N = 288, 16
    T = 7 * m
    y = steady_gauge()
    assert y.shape == (N, T)
    hz = torch.arange(1, 9, dtype=torch.int32)
    cur, spec = _spec(K, y, N, 8, hz, dev, scale=1.0)
    r32 = torch.tensor(y, device=dev)
    K.hw_clear_gap_flags()
    o32 = _fit(K, r32, 0, T, m, spec)
    _check_against_reference(o32, y, m, hz, cur, "gauge-fp32")
    o16 = _fit(K, r32.to(torch.bfloat16), 0, T, m, spec)
    ratio = (o16["sigma"] / o32["sigma"]).cpu().numpy()
    print(f"gauge: fp32 sigma {o32['sigma'].min():.3f}..{o32['sigma'].max():.3f} "
          f"bf16 sigma {o16['sigma'].min():.3f}..{o16['sigma'].max():.3f} ratio min {ratio.min():.3f}")
    assert (ratio > 1.9).all(), ratio


# ---- case 6: graph tick -------------------------------------------------------------------
def test_fp32_shard_graph_tick_matches_eager():
    """A float32 shard reaches the graph tick (variant 5 reads the ring head from the device)
    and its replays equal the eager shard bit for bit, through the ring wrap."""
    from foremast_amd.brain.engine import ShardSpec, StreamingShard, synthetic_history
    from foremast_amd.ingest.ringbuffer import RingState
    from foremast_amd.ops import _native
    from foremast_amd.utils.config import BrainConfig
    _native.require()
    dev = torch.device("cuda:0")
    n, R, m, P, W = 64, 2880, 1440, 3, 6
    cfg = BrainConfig()
    cfg.min_historical_points = 0
    shards = []
    hist = synthetic_history(n, R + 40, m, dev, seed=3)
    for _ in range(2):
        sh = StreamingShard(ShardSpec(n_series=n, ring_len=R, season=m, pods=P, window=W, n_apps=8, dtype=F32),
                            cfg, dev, app_id=(torch.arange(n, device=dev) % 8).int())
        sh.load_history(hist[:, :R])
        sh.hist.state = RingState(head=R - 12, length=R)   # the head wraps during the run
        sh.set_baseline(hist[:, R - W:R].repeat(1, P).float())
        shards.append(sh)
    eager, graph = shards
    assert eager.hist.data.dtype == F32
    newv = torch.empty((n, P), device=dev)
    replays = 0
    for k in range(20):
        newv.copy_(hist[:, R + k:R + k + 1].repeat(1, P).float() * (1.0 + 0.3 * (k % 7 == 3)))
        eager.ingest_tick(newv)
        oe = {key: v.clone() for key, v in eager.score().items()}
        se = eager.app_stats.clone()
        replays += graph._graph is not None
        og = graph.tick_graph(newv)
        torch.cuda.synchronize()
        assert eager._hw_variant == 5
        for key in ("verdict", "sigma", "level", "trend", "best", "forecast", "count"):
            assert torch.equal(oe[key], og[key]), (k, key)
        assert torch.equal(se, graph.app_stats), k
        assert eager.hist.head == graph.hist.head and eager.cur.ticks == graph.cur.ticks
    assert graph.graph_ready()
    assert graph._graph is not None and replays >= 10
    assert torch.equal(eager.hist.data, graph.hist.data) and torch.equal(eager.cur.data, graph.cur.data)
