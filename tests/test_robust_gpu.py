"""The robust_stats kernel (ops/csrc/robust.hip) against models/robust_average.py: the
order statistics bit for bit, the std within the window_stats tolerance, verdicts, band and
anomaly list against models/detect.py, and the engines that dispatch the two names."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.models import detect as det_ref
from foremast_amd.models import robust_average as rb_ref

pytestmark = pytest.mark.gpu



def _helper(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rw = _helper("rollout_world")
NAN = float("nan")
THR, C = 2.0, 6
PATTERNS = 9
K_IN = np.array([0.0, 0.5, -0.6, 0.3, -0.75, 0.75])     # band edges are at +-1 (units of thr * sigma)
K_OUT = np.array([0.0, 1.5, -0.6, -1.4, 0.75, 1.25])
MARGIN = 0.2


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


def _bf16(r):
    return torch.tensor(r, dtype=torch.float32).bfloat16().float().numpy()


def _rows(N, L, seed, first=0):
    """Row i holds pattern (first + i) % 9: 5 % NaN, all NaN, one valid sample, all equal, more
    than half equal, heavy ties, mixed signs with both zeros, eight decades, one outlier."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    y = np.empty((N, L), np.float32)
    for i in range(N):
        p = (first + i) % PATTERNS
        if p == 0:    # 5 % NaN
            r = 20 + 5 * np.sin(2 * np.pi * t / 24 + i) + rng.normal(0, 0.5, L)
            r[rng.random(L) < 0.05] = NAN
        elif p == 1:  # all NaN
            r = np.full(L, NAN)
        elif p == 2:  # a single valid sample
            r = np.full(L, NAN)
            r[rng.integers(L)] = 3.25 + i
        elif p == 3:  # all values equal
            r = np.full(L, 41.5 + i)
        elif p == 4:  # more than half equal: mad == 0, the std fallback
            r = rng.uniform(0.5, 5.0, L)
            r[rng.permutation(L)[:max(L // 2 + 1, int(0.7 * L))]] = 0.0
        elif p == 5:  # heavy ties: level 3000 in bf16 steps of 16
            r = _bf16(3000 + rng.normal(0, 30, L))
        elif p == 6:  # mixed signs around 0, with +0 and -0
            r = rng.normal(0, 1, L)
            r[::7] = 0.0
            r[3::7] = -0.0
        elif p == 7:  # 1e-3 .. 1e5 in one row
            r = 10.0 ** rng.uniform(-3, 5, L)
        else:         # one large outlier
            r = 10 + rng.normal(0, 1, L)
            r[rng.integers(L)] = 1e6
        y[i] = r
    return y


def _cur_for(st):
    """Current points a fixed fraction of thr * sigma from the reference centre, at least
    MARGIN * thr * sigma from both band edges; rows with a zero-width band get points on
    the centre and a clear distance away."""
    N = st.center.shape[0]
    c = st.center.double().numpy()
    s = st.sigma.double().numpy()
    cur = np.empty((N, C), np.float64)
    for i in range(N):
        if not np.isfinite(c[i]):
            cur[i] = [1.0, NAN, -3.0, 0.0, 2.0, NAN]
        elif s[i] == 0:
            d = max(2.0, abs(c[i]) * 0.01)
            cur[i] = [c[i], c[i] + d, c[i], NAN, c[i], c[i] - d] if i % 2 else [c[i]] * C
        else:
            cur[i] = c[i] + (K_IN if i % 3 == 0 else K_OUT) * THR * s[i]
            if i % 4 == 1:
                cur[i, 2] = NAN
    return torch.tensor(cur, dtype=torch.float32)


def _assert_margin(st, cur):
    """The reference alone keeps every valid point MARGIN * thr * sigma from the band edges."""
    f, s = st.center[:, None].double(), st.sigma[:, None].double()
    x = cur.double()
    wide = (s > 0).expand_as(x) & ~torch.isnan(x)
    for edge in (f + THR * s, f - THR * s):
        assert bool((((x - edge).abs() >= MARGIN * THR * s) | ~wide).all())
    flat = (s == 0).expand_as(x) & ~torch.isnan(x)
    assert bool((((x == f) | ((x - f).abs() >= 1.0)) | ~flat).all())


def _eq(a, b):
    """Equal as values (+0 == -0), NaN matching NaN."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


SENT_F = -12345.678
SENT_I = 0x5A5A5A5A
SENT_B = 0x5A


def _sentinel_out(N, dev):
    """Outputs as views of buffers one row longer; returns (out, check)."""
    bufs = {}
    for k in ("center", "sigma", "mad", "std", "count_hist", "score"):
        bufs[k] = torch.full((N + 1,), SENT_F, device=dev)
    for k in ("forecast", "upper", "lower"):
        bufs[k] = torch.full((N + 1, C), SENT_F, device=dev)
    bufs["count"] = torch.full((N + 1,), SENT_I, dtype=torch.int32, device=dev)
    bufs["verdict"] = torch.full((N + 1,), SENT_B, dtype=torch.int8, device=dev)
    out = {k: b[:N] for k, b in bufs.items()}

    def check():
        for k, b in bufs.items():
            want = {torch.float32: SENT_F, torch.int32: SENT_I, torch.int8: SENT_B}[b.dtype]
            assert bool((b[N:] == torch.tensor(want, dtype=b.dtype, device=dev)).all()), k
    return out, check


def _run_case(K, y, R, head, dtype, ld=None):
    dev = torch.device("cuda:0")
    N, L = y.shape
    ld = R if ld is None else ld
    store = torch.full((N, ld), 7.0)
    store[:, (head + torch.arange(L)) % R] = torch.tensor(y)
    store = store.to(dtype)
    ring = store.to(dev)[:, :R]
    logical = store[:, :R].float()[:, (head + torch.arange(L)) % R]
    st = rb_ref.robust_stats(logical)
    cur = _cur_for(st)
    _assert_margin(st, cur)
    min_valid = min(2, L)
    buf = K.AnomalyBuffer(N * C + 8, dev)
    spec = K.DetectSpec(horizons=torch.arange(1, C + 1, dtype=torch.int32, device=dev),
                        threshold=torch.full((N,), THR, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur.to(dev), min_valid=min_valid,
                        anomalies=buf)
    out, check_sentinels = _sentinel_out(N, dev)
    got = K.robust_stats(ring, head, L, spec, out=out)
    torch.cuda.synchronize()
    check_sentinels()
    o = {k: v.cpu() for k, v in got.items()}

    # exactness
    assert _eq(o["center"], st.center), "center"
    assert _eq(o["mad"], st.mad), "mad"
    assert torch.equal(o["count_hist"], st.count), "count"
    exact = st.mad > 0
    assert torch.equal(o["sigma"][exact], st.sigma[exact]), "sigma where mad > 0"
    fb = ~exact
    for k, ref in (("std", st.std), ("sigma", st.sigma)):
        np.testing.assert_allclose(o[k][fb].numpy(), ref[fb].numpy(), rtol=1e-4, atol=1e-4, equal_nan=True, err_msg=k)

    # verdicts, band and list against detect() on the reference statistics
    f = st.center[:, None].expand(N, C)
    d = det_ref.detect(f, st.sigma, cur, torch.full((N,), THR), torch.full((N,), 3, dtype=torch.int8),
                       torch.full((N,), -1e30), model_ok=st.count >= min_valid)
    assert torch.equal(o["verdict"], d.verdict) and torch.equal(o["count"], d.count)
    assert _eq(o["forecast"], f)
    mag = f.abs() + THR * st.sigma[:, None].abs()
    # Not torch.equal: the shared epilogue is compiled with fused multiply-add, so f + thr * sigma
    # is rounded once where detect() rounds twice.  Both lie within half an ulp of the exact
    # value, hence within one ulp (2^-23 <= 1.2e-7 of the larger operand) of each other; rows
    # on the std fallback carry the 1e-4 tolerance of their sigma.
    tol = torch.where(exact[:, None], 1.5e-7 * mag, 2e-4 * mag + 1e-4)
    some = st.count > 0
    for k, ref in (("upper", d.upper), ("lower", d.lower)):
        assert not bool(torch.isnan(o[k][some]).any()), k
        bad = (o[k] - ref).abs() > tol
        assert not bool(bad[some].any()), k
    # no valid sample: NaN centre and sigma, no verdict (the shared epilogue's lower edge is then
    # fmaxf(NaN, min_lower) = min_lower, as for window_stats, where torch.maximum keeps the NaN)
    assert bool(torch.isnan(o["upper"][~some]).all()) and bool((o["verdict"][~some] == -1).all())
    s, c, v, over = buf.fetch()
    ws, wc = np.nonzero(d.anomaly.numpy())
    assert not over and s.tolist() == ws.tolist() and c.tolist() == wc.tolist()
    assert v.tolist() == cur.numpy()[ws, wc].tolist()
    return st, d


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("head,L", [(1000, 1000), (1001, 60)])
def test_wrapping_windows(K, dtype, head, L):
    st, d = _run_case(K, _rows(67, L, seed=L), 1024, head, dtype)
    # the cases mean something: fallback rows, exact rows, every verdict
    assert bool((st.mad == 0).any()) and bool((st.mad > 0).any())
    assert {-1, 0, 1} <= set(d.verdict.tolist())


def test_full_week_ring_bf16(K):
    _run_case(K, _rows(130, 10080, seed=7), 10080, 1000, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65])
def test_short_lengths(K, dtype, L):
    _run_case(K, _rows(67, L, seed=100 + L), 1024, 1000, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_series_counts_below_a_workgroup(K, dtype):
    for first in range(PATTERNS):              # N = 1: every pattern on its own
        _run_case(K, _rows(1, 1000, seed=first, first=first), 1024, 1000, dtype)
    for first in (0, 4):                       # N = 5: patterns 0-4 and 4-8
        _run_case(K, _rows(5, 1000, seed=20 + first, first=first), 1024, 1000, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_stride_larger_than_the_ring(K, dtype):
    _run_case(K, _rows(67, 1000, seed=31), 1024, 1000, dtype, ld=1040)


@pytest.mark.parametrize("dtype,R", [(torch.float32, 16384), (torch.bfloat16, 32768)])
def test_windows_too_long_to_stage(K, dtype, R):
    """64 KiB of samples: past the LDS staging limit, the passes read the ring in place."""
    _run_case(K, _rows(PATTERNS, R, seed=41), R, 5003, dtype)
    _run_case(K, _rows(PATTERNS, R - 5, seed=42), R, R - 3, dtype)


# ------------------------------------------------------------------ engines
def _history(N, T, seed=1):
    g = torch.Generator().manual_seed(seed)
    y = 40 + 6 * torch.sin(torch.arange(T) / 9.0)[None] + torch.randn(N, T, generator=g)
    y[:, :T // 2] += 25.0
    y[1, 5:40] = NAN
    y[2] = torch.where(torch.rand(T, generator=g) < 0.3, torch.ones(T) * 4, torch.zeros(T))
    return y


def _cfg(name):
    from foremast_amd.utils.config import BrainConfig
    cfg = BrainConfig()
    cfg.algorithm = name
    cfg.min_historical_points = 10
    cfg.ma_window = 48
    return cfg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["robust_average_all", "robust_average"])
def test_gpu_streaming_shard_equals_its_cpu_twin(K, name, dtype):
    from foremast_amd.brain.engine import ShardSpec, StreamingShard
    N, T, W = 70, 160, 4
    y = _history(N, T)
    cur = y[:, -W:].clone() + 0.1
    cur[3::5, 2] += 200.0
    outs = {}
    for dev in ("cpu", "cuda"):
        sh = StreamingShard(ShardSpec(n_series=N, ring_len=T, season=24, pods=1, window=W, algorithm=name,
                                      pairwise="NONE", dtype=dtype), _cfg(name), device=dev)
        sh.load_history(y)
        for c in range(W):
            sh.ingest_tick(cur[:, c:c + 1].contiguous().to(sh.device))
        outs[dev] = {k: v.cpu() for k, v in sh.score().items()}
    a, b = outs["cpu"], outs["cuda"]
    assert torch.equal(a["verdict"], b["verdict"]) and torch.equal(a["count"], b["count"])
    assert _eq(a["center"], b["center"]) and _eq(a["mad"], b["mad"])
    assert int(a["verdict"][3]) == 1 and int(a["verdict"][0]) == 0


@pytest.mark.parametrize("name", ["robust_average_all", "robust_average"])
def test_gpu_rollout_fit_state_equals_the_cpu_path(K, name):
    """_fit_state, the model fit of an admission, on a wrapped bf16 ring."""
    from foremast_amd.brain.rollout import RolloutMonitor
    from foremast_amd.store.jobstore import MemoryJobStore
    N, R, head, length = 9, 200, 150, 160
    y = _history(N, length, seed=4)
    ring = torch.full((N, R), 7.0)
    ring[:, (head + torch.arange(length)) % R] = y
    ring = ring.bfloat16()
    cpu = RolloutMonitor(MemoryJobStore(), cfg=_cfg(name), device="cpu", ring_len=2880,
                         min_capacity=4)._fit_state(ring, head, length)
    gpu = RolloutMonitor(MemoryJobStore(), cfg=_cfg(name), device="cuda", ring_len=2880,
                         min_capacity=4)._fit_state(ring.cuda(), head, length)
    torch.cuda.synchronize()
    gpu = {k: v.cpu() for k, v in gpu.items()}
    logical = ring.float()[:, (head + torch.arange(length)) % R]
    st = rb_ref.robust_stats(logical, 48 if name == "robust_average" else None)
    assert set(gpu) == set(cpu)
    assert _eq(gpu["level"], cpu["level"]) and _eq(gpu["level"], st.center)
    exact = st.mad > 0                         # sigma = 1.4826 mad there: an exact sigma is an exact mad
    assert bool(exact.any()) and bool((~exact).any())
    assert torch.equal(gpu["sigma"][exact], cpu["sigma"][exact])
    np.testing.assert_allclose(gpu["sigma"][~exact].numpy(), cpu["sigma"][~exact].numpy(), rtol=1e-4, atol=1e-4)
    assert torch.equal(gpu["nvalid"], cpu["nvalid"]) and torch.equal(gpu["best"].int(), cpu["best"].int())
    assert not gpu["trend"].any() and not gpu["season_hb"].any()


@pytest.mark.parametrize("name", ["robust_average_all", "robust_average"])
def test_gpu_rollout_admission_equals_the_cpu_engine(K, name):
    """Jobs admitted and scored by the resident engine on the GPU (the scenario of
    tests/test_rollout.py): the same statuses tick by tick as the engine on the CPU, and the
    same centre per row up to the ring's precision."""
    gout, gdocs, gids, gmon, _ = rw.run_monitor("cuda", name, ticks=(rw.T0 + 120,))
    cout, cdocs, cids, cmon, _ = rw.run_monitor("cpu", name, ticks=(rw.T0 + 120,))
    assert gout[rw.T0 + 120] == {gids["a"]: r.ST_COMPLETED_UNHEALTH}
    assert gout["end"] == {gids["b"]: r.ST_COMPLETED_HEALTH, gids["c"]: r.ST_COMPLETED_HEALTH}
    assert {a: d["status"] for a, d in gdocs.items()} == {a: d["status"] for a, d in cdocs.items()}
    g = {k: v.cpu() for k, v in gmon.state.items()}
    c = cmon.state
    # the GPU ring is bf16 and the CPU ring fp32: rounding is monotone, so the median of the
    # rounded samples is the rounded median, within half a bf16 ulp (2^-9) of the fp32 one
    # (the exact comparison, on one bf16 ring, is the _fit_state test above)
    np.testing.assert_allclose(g["level"][:6].numpy(), c["level"][:6].numpy(), rtol=2.0 ** -8, atol=0)
    assert torch.equal(g["nvalid"][:6], c["nvalid"][:6]) and bool((c["nvalid"][:6] > 0).all())
    assert bool((g["sigma"][:6] > 0).all())


@pytest.mark.parametrize("name", ["robust_average_all", "robust_average"])
def test_gpu_batch_scorer_equals_the_cpu_scorer(K, name):
    from foremast_amd.brain.batch import BatchScorer, MetricTask
    N, T, Cc = 8, 160, 5
    y = _history(N, T, seed=2)
    cur = (y[:, -Cc:] + 0.1).numpy().astype(np.float32)
    cur[4, 1] += 200.0
    tasks = [MetricTask(job_id="j", alias=f"m{i}", metric=f"m{i}", namespace="ns", app="a", step=60.0,
                        hist=y[i].numpy().astype(np.float32), hist_end=0.0,
                        cur_ts=60.0 * (1 + np.arange(Cc, dtype=np.float64)), cur_vals=cur[i], threshold=3.0, bound=3)
             for i in range(N)]
    a = BatchScorer(_cfg(name), device=torch.device("cpu")).score(tasks)
    b = BatchScorer(_cfg(name), device=torch.device("cuda")).score(tasks)
    assert [x.verdict for x in a] == [x.verdict for x in b] and a[4].verdict == 1 and a[0].verdict == 0
    assert all(x.model == name for x in b)
    for x, z in zip(a, b):
        assert [p[:2] for p in x.anomalies] == [p[:2] for p in z.anomalies]
        np.testing.assert_allclose(z.upper, x.upper, rtol=2e-4, atol=1e-4)
        np.testing.assert_allclose(z.lower, x.lower, rtol=2e-4, atol=1e-4)
