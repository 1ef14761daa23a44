"""The prophet forecast state on the GPU (prophet.hip: kernels.prophet_fit_state,
kernels.prophet_state_detect) and ML_ALGORITHM=prophet on the resident rollout engine.

Bounds:

* fit: ``beta`` / ``sigma`` / ``nvalid`` of ``prophet_fit_state`` are the bits of ``prophet_score``.
* the new kernels alone (state from the kernel's own beta, forecast from it at every horizon up
  to 2^20): about 40 fp32 roundings, so <= 1e-5 x the sum of the absolute values of the terms
  (the terms of ``beta . x(h)`` for the forecast).
* end to end against the fp64 model (``window_state(fit_prophet_window(...))``): at horizons
  <= 64 the bounds of tests/test_prophet_gpu.py (forecast 5e-3 sigma, sigma 1e-3 sigma); beyond,
  4x the worst error of the CPU fp32 emulation (helpers/prophet_state_cases.py) on the same
  inputs (worst row of the geometry, per horizon range), in units of the row's sigma.  These bounds are in units of the
  residual sigma, so they apply to rows with at least as many valid samples as the model has
  terms (an underdetermined row interpolates its samples: its sigma is ~1e-5 of its level and
  measures nothing); every row is covered by the two checks above.
  Measured (worst row, sigma; emulation / kernel): 1.7e-3 / 2.2e-4 up to h = 7 m + 1, 0.23 / 0.12
  up to h = 1e5 and 2.4 / 1.2 at h = 2^20 -- the fit's fp32 error in the slope, extrapolated
  over h / (T - 1) windows (docs/SCORING.md).
* verdict / count / row record / per-app counters / anomaly list: exact against models/detect.py
  on the fp64 forecast on every row with no point within EDGE = 1e-2 sigma of a band edge (at
  most 5 % of the rows with a model are excluded, asserted on the reference alone).  These
  tests draw horizons up to 7 m + 1: past that the forecast error above is larger than EDGE,
  so no placement of points keeps a verdict independent of it.
"""

import ctypes
import importlib.util
import json
import os

import pytest
import torch

from foremast_amd.api import rest as r
from foremast_amd.models import detect as det_ref
from foremast_amd.models import prophet_lite as pl

pytestmark = pytest.mark.gpu


def _helper(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


psc = _helper("prophet_state_cases")
pc = psc.pc
rw = _helper("rollout_world")

F_TOL, S_TOL, EDGE = 5e-3, 1e-3, 1e-2
ROUND_TOL = 1e-5          # ~40 fp32 roundings
EMU_HEADROOM = 4.0
THR, THR_LOW, SHIFT = 3.0, 1.5, 4.0
CMAX = 55
EMU_FROM = {"n1": "t49_bf16", "n17": "t337_fp32"}

#        name        T     m     bf16   N
CASES = {"t48_bf16": (48, 24, True, 27), "t48_fp32": (48, 24, False, 27),
         "t49_bf16": (49, 24, True, 27), "t49_fp32": (49, 24, False, 27),
         "t337_bf16": (337, 24, True, 27), "t337_fp32": (337, 24, False, 27),
         "n1": (49, 24, True, 1), "n17": (337, 24, False, 17),
         "days3": (4320, 1440, True, 16)}


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


_CACHE = {}


def _case(name):
    """Inputs, the fp64 reference and the fp32 emulation of a case, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    T, m, bf16, N = CASES[name]
    y, pat = pc.make_rows(T, m, N, seed=11, bf16=bf16)
    ref = pl.fit_prophet_window(y, m)
    state = pl.window_state(ref)
    hz = psc.draw_horizons(m, N, CMAX, seed=5)                       # every horizon, 2^20 included
    hz_near = psc.draw_horizons(m, N, CMAX, seed=6, hmax=7 * m + 1)  # the verdict tests
    fr = pl.forecast_state(*state, m, hz.long())
    emu_f, emu_s, _ = psc.emulate_state_fp32(y, m, hz)
    P = ref.beta.shape[1]
    c = dict(T=T, m=m, bf16=bf16, N=N, R=T + 5, head=3, y=y, pat=pat, ref=ref, state=state, hz=hz,
             hz_near=hz_near, fr=fr, emu_f=emu_f, emu_s=emu_s, P=P, determined=ref.n_valid >= P,
             min_valid=pc.min_valid_of(T))
    _CACHE[name] = c
    return c


def _ring(c, dev):
    return pc.to_ring(c["y"], c["R"], c["head"], torch.bfloat16 if c["bf16"] else torch.float32, dev)


_FITS = {}


def _fit(K, name):
    """``prophet_fit_state`` of a case on the GPU, once (outputs on the host too)."""
    if name not in _FITS:
        c = _case(name)
        out = K.prophet_fit_state(_ring(c, torch.device("cuda")), c["head"], c["T"], c["m"], want_beta=True)
        torch.cuda.synchronize()
        _FITS[name] = out, {k: out[k].cpu() for k in ("level", "slope", "harm", "sigma", "nvalid", "beta")}
    return _FITS[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_args_struct_sizes(K):
    from foremast_amd.ops import _native
    lib = _native.require()
    assert ctypes.sizeof(K.ProphetStateOut) == lib.fm_prophet_state_out_size()
    assert ctypes.sizeof(K.ProphetStateArgs) == lib.fm_prophet_state_args_size()
    assert ctypes.sizeof(K.ProphetArgs) == lib.fm_prophet_args_size()


@pytest.mark.parametrize("name", list(CASES))
def test_fit_bits_equal_prophet_score(K, name):
    c, dev = _case(name), torch.device("cuda")
    N = c["N"]
    _, fit = _fit(K, name)
    spec = K.DetectSpec(horizons=torch.arange(1, 11, dtype=torch.int32, device=dev),
                        threshold=torch.full((N,), THR, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.zeros(N, device=dev), max_horizon=16)
    sc = K.prophet_score(_ring(c, dev), c["head"], c["T"], c["m"], spec, want_beta=True)
    torch.cuda.synchronize()
    assert fit["beta"].shape == (N, c["P"])
    for k in ("beta", "sigma", "nvalid"):
        assert torch.equal(_bits(sc[k].cpu()), _bits(fit[k])), k
    assert torch.equal(fit["nvalid"].double(), c["ref"].n_valid.double())


@pytest.mark.parametrize("name", list(CASES))
def test_state_kernels_against_their_own_beta(K, name):
    """level / slope / harm and the forecast of the detect kernel against the fp64 formulas
    applied to the kernel's beta, at every horizon including 2^20 (a wrong phase reduction
    shows here)."""
    c, dev = _case(name), torch.device("cuda")
    T, m, N = c["T"], c["m"], c["N"]
    out, fit = _fit(K, name)
    b = fit["beta"].double()
    level, slope, harm = pl.state_from_beta(b, T, m)
    omc, cos, sin, on = pl.state_rotation(T, m)
    d = b[:, 2:12].abs()
    l_abs = b[:, 0].abs() + b[:, 1].abs() + (d * omc[None, :]).sum(1)
    s_abs = (b[:, 1].abs() + d.sum(1)) / (T - 1)
    h_abs = torch.zeros_like(harm)
    src, dst, j = 12, 0, 0
    for _days, order in pl.STATE_SEASONS:
        if bool(on[j]):
            a_s, a_c = b[:, src:src + order].abs(), b[:, src + order:src + 2 * order].abs()
            cc, ss = cos[None, j:j + order].abs(), sin[None, j:j + order].abs()
            h_abs[:, dst:dst + order] = a_s * cc + a_c * ss
            h_abs[:, dst + order:dst + 2 * order] = a_s * ss + a_c * cc
            src += 2 * order
        dst += 2 * order
        j += order
    for nm, got, want, mag in (("level", fit["level"], level, l_abs), ("slope", fit["slope"], slope, s_abs),
                               ("harm", fit["harm"], harm, h_abs)):
        err = (got.double() - want).abs()
        print(f"{nm}: worst {float((err / mag.clamp(min=1e-300)).max()):.2e} of the terms")
        assert bool((err <= ROUND_TOL * mag).all()), nm
    # the forecast the detect kernel writes, C in {55, 17, 10, 1} columns of per-row horizons
    for C in (CMAX, 17, 10, 1):
        hz = c["hz"][:, :C].contiguous()
        spec = K.DetectSpec(horizons=hz.to(dev), threshold=torch.full((N,), THR, device=dev),
                            bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                            min_lower=torch.zeros(N, device=dev))
        res = K.prophet_state_detect(out, m, spec)
        torch.cuda.synchronize()
        f = res["forecast"].cpu().double()
        assert f.shape == (N, C)
        want = pl.forecast_state(level, slope, harm, m, hz.long())
        XH = pl._window_features(float(T - 1) + hz.double(), T, m, 10, 0.8)
        mag = (XH * b[:, None, :]).abs().sum(-1)
        err = (f - want).abs()
        far = hz == psc.HZ_MAX
        print(f"C={C}: forecast worst {float((err / mag.clamp(min=1e-300)).max()):.2e} of the terms"
              f" ({int(far.sum())} points at 2^20)")
        assert bool((err <= ROUND_TOL * mag).all())
        if C == CMAX:
            assert bool(far.any())


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_against_the_fp64_model(K, name):
    c, dev = _case(name), torch.device("cuda")
    N, m = c["N"], c["m"]
    out, fit = _fit(K, name)
    ref = c["ref"]
    s = ref.sigma.double()
    sc = s.clamp(min=1e-300)
    det = c["determined"]
    spec = K.DetectSpec(horizons=c["hz"].to(dev), threshold=torch.full((N,), THR, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev), min_lower=torch.zeros(N, device=dev))
    f = K.prophet_state_detect(out, m, spec)["forecast"].cpu().double()
    assert torch.isfinite(f).all() and torch.isfinite(fit["sigma"]).all()
    err = (f - c["fr"]).abs() / sc[:, None]
    near = c["hz"] <= 64
    es = (fit["sigma"].double() - s).abs()
    print(f"sigma: worst {float((es / sc)[det].max()) if bool(det.any()) else 0.0:.2e} sigma; "
          f"forecast h <= 64: {float(err[det][near[det]].max()) if bool(near[det].any()) else 0.0:.2e} sigma")
    assert bool((es <= S_TOL * s)[det].all())
    assert bool((err <= F_TOL)[det[:, None] & near].all())
    # beyond 64: 4x the emulation's worst error over the rows of this geometry (the cases of a
    # few rows hold the first rows of the 27-row case of their geometry, and take its figure)
    ce = _case(EMU_FROM.get(name, name))
    emu = ((ce["emu_f"].double() - ce["fr"]).abs() / ce["ref"].sigma.double().clamp(min=1e-300)[:, None])
    for lo, hi in ((65, 7 * m + 1), (7 * m + 2, 10 ** 5), (10 ** 5 + 1, psc.HZ_MAX)):
        sel = (c["hz"] >= lo) & (c["hz"] <= hi) & det[:, None]
        sel_e = (ce["hz"] >= lo) & (ce["hz"] <= hi) & ce["determined"][:, None]
        if not bool(sel.any()):
            continue
        e_k, e_e = float(err[sel].max()), float(emu[sel_e].max())
        print(f"h in [{lo}, {hi}]: kernel {e_k:.2e} sigma, emulation {e_e:.2e} sigma")
        assert e_k <= EMU_HEADROOM * e_e


# ---- detection ----------------------------------------------------------------------------

def _detect_inputs(c, C, seed):
    """Window of ``C`` columns at per-row horizons <= 7 m + 1: the fp64 forecast + z sigma with z
    at least 0.2 sigma from every threshold in play, a 3x spike in a third of the rows, a
    missing point in a fifth, and the per-row parameters of every epilogue feature."""
    N, m = c["N"], c["m"]
    ref = c["ref"]
    g = torch.Generator().manual_seed(seed)
    hz = c["hz_near"][:, :C].contiguous()
    fr = pl.forecast_state(*c["state"], m, hz.long()).float()
    zs = torch.tensor([-2.2, -1.0, -0.3, 0.4, 0.9, 2.0])
    z = zs[torch.randint(0, len(zs), (N, C), generator=g)]
    z[1::6] = z[1::6].clamp(-1.0, 0.9)    # the mean-shift rows: inside the lowered band
    x = fr + z * ref.sigma[:, None]
    for i in range(0, N, 3):
        x[i, i % C] = 3.0 * fr[i, i % C] + 10.0 * ref.sigma[i]
    if C > 2:
        for i in range(1, N, 5):
            x[i, 2] = float("nan")
    lut_n = C + 1
    k = torch.arange(lut_n, dtype=torch.float32)
    lut = torch.stack([torch.stack([THR + 0.05 * (k % 3), THR_LOW + 0.05 * (k % 3)]),
                       torch.stack([THR + 0.1 - 0.05 * (k % 2), THR_LOW + 0.1 - 0.05 * (k % 2)])])
    cls = (torch.arange(N) % 2).to(torch.int16)
    npts = (~torch.isnan(x)).sum(1)
    kk = npts.clamp(max=lut_n - 1)
    # rows that differ: the mean-shift rule sees a baseline mean 10 sigma below the window on
    # every third of them (far beyond the shift threshold), none on the others
    differs = torch.tensor([i % 2 for i in range(N)], dtype=torch.uint8)
    base_mean = torch.full((N,), float("nan"))
    for i in range(1, N, 6):
        base_mean[i] = float(fr[i].min()) - 10.0 * float(ref.sigma[i])
    return dict(C=C, hz=hz, fr=fr, x=x, lut=lut, cls=cls, npts=npts,
                thr_lut=lut[cls.long(), 0, kk], low_lut=lut[cls.long(), 1, kk],
                thr=torch.full((N,), THR), low=torch.full((N,), THR_LOW), differs=differs, base_mean=base_mean,
                bound=torch.tensor([(3, 1, 2)[i % 3] for i in range(N)], dtype=torch.int8),
                min_lower=torch.tensor([0.0 if i % 4 == 0 else -1e30 for i in range(N)]),
                ok=ref.n_valid >= c["min_valid"])


def _clear_rows(c, d, thresholds, shift=False):
    """Rows whose verdict cannot depend on an error below EDGE sigma, from the reference alone:
    every valid point (and, with the mean-shift rule, the mean deviation) at least EDGE sigma
    from every band edge in play.  Rows without a model are trivially clear."""
    f, x = d["fr"].double(), d["x"].double()
    s = c["ref"].sigma.double()[:, None]
    valid = ~torch.isnan(x)
    dist = torch.full((c["N"],), float("inf"), dtype=torch.float64)
    edges = []
    for t in thresholds:
        edges += [f + t.double()[:, None] * s, torch.maximum(f - t.double()[:, None] * s, d["min_lower"].double()[:, None])]
    if shift:
        bm = d["base_mean"].double()[:, None]
        edges += [(bm + SHIFT * s).expand_as(f), torch.maximum(bm - SHIFT * s, d["min_lower"].double()[:, None]).expand_as(f)]
        z = torch.where(valid, (x - bm) / s.clamp(min=1e-12), torch.zeros_like(x)).sum(1) / valid.sum(1).clamp(min=1)
        dist = torch.minimum(dist, torch.nan_to_num(torch.minimum((z - SHIFT).abs(), (z + SHIFT).abs()), nan=float("inf")))
    for e in edges:
        de = torch.where(valid & ~torch.isnan(e), (x - e).abs() / s.clamp(min=1e-300), torch.full_like(x, float("inf")))
        dist = torch.minimum(dist, de.min(1).values)
    clear = (dist >= EDGE) | ~d["ok"]
    n_model = int(d["ok"].sum())
    n_out = int((~clear).sum())
    print(f"rows excluded (a point within {EDGE} sigma of an edge): {n_out} of {n_model} with a model")
    assert n_out <= 0.05 * n_model
    return clear


def _spec(K, d, dev, **kw):
    args = dict(horizons=d["hz"].to(dev), threshold=d["thr"].to(dev), bound=d["bound"].to(dev),
                min_lower=d["min_lower"].to(dev), cur=d["x"].to(dev))
    for k, v in kw.items():
        args[k] = v.to(dev) if isinstance(v, torch.Tensor) else v
    return K.DetectSpec(**args)


def _band_tol(c, d, thr, edge):
    """What the forecast and sigma bounds allow an edge to move (sigma of the row)."""
    sc = c["ref"].sigma.double().clamp(min=1e-300)
    det = c["determined"]
    sel = (c["hz"] > 64) & (c["hz"] <= 7 * c["m"] + 1) & det[:, None]
    emu = ((c["emu_f"].double() - c["fr"]).abs() / sc[:, None])[sel]
    f_tol = max(F_TOL, EMU_HEADROOM * float(emu.max())) if emu.numel() else F_TOL
    return (f_tol + float(thr) * S_TOL) * c["ref"].sigma[:, None] + 1e-6 * edge.abs()


def _compare(c, d, res, want, clear, thr_max):
    assert torch.equal(res["verdict"].cpu()[clear], want.verdict[clear])
    assert torch.equal(res["count"].cpu()[clear], want.count[clear])
    rows = clear & c["determined"]
    for k, e in (("upper", want.upper), ("lower", want.lower)):
        assert bool(((res[k].cpu() - e).abs() <= _band_tol(c, d, thr_max, e))[rows].all()), k


@pytest.mark.parametrize("C", [CMAX, 17, 10, 1])
@pytest.mark.parametrize("name", ["t49_bf16", "t337_fp32", "n1", "n17", "days3"])
def test_verdict_count_band(K, name, C):
    c, dev = _case(name), torch.device("cuda")
    out, _ = _fit(K, name)
    d = _detect_inputs(c, C, seed=21)
    clear = _clear_rows(c, d, [d["thr"]])
    want = det_ref.detect(d["fr"], c["ref"].sigma, d["x"], d["thr"], d["bound"], d["min_lower"], model_ok=d["ok"])
    if c["N"] >= 17 and C >= 10:
        assert int((want.verdict == 1).sum()) > 0 and int((want.verdict == 0).sum()) > 0 \
            and int((want.verdict == -1).sum()) > 0
    res = K.prophet_state_detect(out, c["m"], _spec(K, d, dev, min_valid=c["min_valid"]))
    torch.cuda.synchronize()
    _compare(c, d, res, want, clear, THR)
    own = det_ref.detect(res["forecast"].cpu(), out["sigma"].cpu(), d["x"], d["thr"], d["bound"], d["min_lower"],
                         model_ok=d["ok"])
    assert torch.allclose(res["upper"].cpu(), own.upper, rtol=1e-6, atol=0)
    assert torch.allclose(res["lower"].cpu(), own.lower, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["t49_bf16", "t337_fp32"])
def test_tabulated_thresholds_lowered_band_and_shift_rule(K, name):
    """thr_lut / thr_cls, ``differs`` with the lowered band, and the mean-shift rule."""
    c, dev = _case(name), torch.device("cuda")
    out, _ = _fit(K, name)
    d = _detect_inputs(c, 10, seed=22)
    sig = c["ref"].sigma
    common = dict(model_ok=d["ok"])
    # tabulated thresholds (class, valid points) with the lowered band where rows differ
    clear = _clear_rows(c, d, [d["thr_lut"], d["low_lut"]])
    want = det_ref.detect(d["fr"], sig, d["x"], d["thr_lut"], d["bound"], d["min_lower"], differs=d["differs"],
                          threshold_low=d["low_lut"], pw_min_points=2, **common)
    plain = det_ref.detect(d["fr"], sig, d["x"], d["thr_lut"], d["bound"], d["min_lower"], **common)
    assert not torch.equal(want.count, plain.count)      # the lowered band is in force somewhere
    res = K.prophet_state_detect(out, c["m"], _spec(K, d, dev, min_valid=c["min_valid"], differs=d["differs"],
                                                    pw_min_points=2, thr_lut=d["lut"], thr_cls=d["cls"]))
    torch.cuda.synchronize()
    _compare(c, d, res, want, clear, THR + 0.1)
    # per-row thresholds, lowered band and the mean-shift rule (one-step sigma)
    clear = _clear_rows(c, d, [d["thr"], d["low"]], shift=True)
    kw = dict(differs=d["differs"], threshold_low=d["low"], pw_min_points=2, shift_threshold=SHIFT,
              base_mean=d["base_mean"], shift_min_points=2)
    want = det_ref.detect(d["fr"], sig, d["x"], d["thr"], d["bound"], d["min_lower"], shift_sigma=sig, **kw, **common)
    noshift = det_ref.detect(d["fr"], sig, d["x"], d["thr"], d["bound"], d["min_lower"], differs=d["differs"],
                             threshold_low=d["low"], pw_min_points=2, **common)
    assert not torch.equal(want.count, noshift.count)    # the shift rule is in force somewhere
    res = K.prophet_state_detect(out, c["m"], _spec(K, d, dev, min_valid=c["min_valid"], shift_one_step=True, **kw))
    torch.cuda.synchronize()
    _compare(c, d, res, want, clear, max(THR, SHIFT))


def test_row_record_app_stats_and_anomaly_list(K):
    c, dev = _case("t337_bf16"), torch.device("cuda")
    out, _ = _fit(K, "t337_bf16")
    N, C, ncol = c["N"], 17, 4
    d = _detect_inputs(c, C, seed=23)
    clear = _clear_rows(c, d, [d["thr"]])
    assert bool(clear.all())                 # the counters and the list are compared whole
    want = det_ref.detect(d["fr"], c["ref"].sigma, d["x"], d["thr"], d["bound"], d["min_lower"], model_ok=d["ok"])
    app = torch.arange(N, dtype=torch.int32) % 5
    stats = torch.zeros((5, 2), dtype=torch.int32, device=dev)
    buf = K.AnomalyBuffer(N * C, dev)
    start = (torch.arange(N, dtype=torch.int32) % 7)
    tick = torch.tensor([5], dtype=torch.int32, device=dev)
    rec = torch.zeros((N, 4), device=dev)
    spec = _spec(K, d, dev, min_valid=c["min_valid"], app_id=app, app_stats=stats, anomalies=buf, row_out=rec,
                 start_min=start, tick_min=tick, last_ncol=ncol)
    res = K.prophet_state_detect(out, c["m"], spec)
    torch.cuda.synchronize()
    assert torch.equal(res["verdict"].cpu(), want.verdict)
    want_stats = torch.zeros((5, 2), dtype=torch.int32)
    for i in range(N):
        want_stats[app[i], 0] += int(want.verdict[i] == 1)
        want_stats[app[i], 1] += int(want.verdict[i] >= 0)
    assert torch.equal(stats.cpu(), want_stats)
    s, col, val, over = buf.fetch()
    rs, rc = torch.nonzero(want.anomaly & (want.verdict == 1)[:, None], as_tuple=True)
    assert not over and len(rs) > 0
    assert s.tolist() == rs.tolist() and col.tolist() == rc.tolist()
    assert val.tolist() == d["x"][rs, rc].tolist()
    rec = rec.cpu()
    last = (5 - start.long()).clamp(0, ncol - 1)
    assert torch.equal(rec[:, 0], want.verdict.float())
    assert torch.equal(rec[:, 1], d["npts"].float())
    assert torch.equal(rec[:, 2], res["upper"].cpu().gather(1, last[:, None])[:, 0])
    assert torch.equal(rec[:, 3], res["lower"].cpu().gather(1, last[:, None])[:, 0])
    # without the band outputs: the same verdicts and record
    rec2 = torch.zeros((N, 4), device=dev)
    stats.zero_()
    buf.reset()
    spec2 = _spec(K, d, dev, min_valid=c["min_valid"], app_id=app, app_stats=stats, anomalies=buf, row_out=rec2,
                  start_min=start, tick_min=tick, last_ncol=ncol, want_band=False)
    res2 = K.prophet_state_detect(out, c["m"], spec2)
    torch.cuda.synchronize()
    assert "forecast" not in res2 and "upper" not in res2
    assert torch.equal(res2["verdict"].cpu(), want.verdict) and torch.equal(rec2.cpu(), rec)


# ---- the engine ---------------------------------------------------------------------------

def test_rollout_monitor_prophet_on_the_gpu():
    """The three-app scenario of tests/test_rollout.py, minute by minute (so the engine captures
    its tick graph and replays it): the statuses of the CPU engine."""
    T0 = rw.T0
    ticks = tuple(T0 + 60 * k for k in range(1, 6))
    runs = {dev: rw.run_monitor(dev, "prophet", ring_len=4320, ticks=ticks) for dev in ("cuda", "cpu")}
    out, docs, ids, mon, hq = runs["cuda"]
    out_c, docs_c, ids_c, _mon_c, _hq_c = runs["cpu"]
    assert mon.prophet and mon.gpu
    assert out[T0 + 120] == {ids["a"]: r.ST_COMPLETED_UNHEALTH}, out
    assert out["end"] == {ids["b"]: r.ST_COMPLETED_HEALTH, ids["c"]: r.ST_COMPLETED_HEALTH}
    assert {a: docs[a]["status"] for a in ids} == {a: docs_c[a]["status"] for a in ids_c}
    got = json.loads(docs["a"]["anomalyInfo"])["error5xx"]["values"]
    want = json.loads(docs_c["a"]["anomalyInfo"])["error5xx"]["values"]
    assert got[0::2] == want[0::2]
    assert hq["end"] == hq["admitted"]
    if mon.graph_on:
        assert mon.graph_replays > 0


# ---- argument errors (raised on the host: no launch) ------------------------------------

def test_bad_arguments(K):
    c, dev = _case("t49_bf16"), torch.device("cuda")
    ring = _ring(c, dev)
    T, m, N = c["T"], c["m"], c["N"]
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring, c["head"], T, 1)                          # m < 2
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring, c["head"], 1, m)                          # one sample
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring[:, 1:], c["head"], T, m)                   # rows off the 16-byte grid
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring.cpu(), c["head"], T, m)
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring, c["head"], T, m, cp_range=1.0)            # a hinge past the window
    with pytest.raises(K.KernelShapeError):
        K.prophet_fit_state(ring, c["head"], T, m, out={"harm": torch.zeros((N, 13), device=dev)})
    f32 = dict(dtype=torch.float32, device=dev)
    good = {"level": torch.zeros(N, **f32), "slope": torch.zeros(N, **f32), "harm": torch.zeros((N, 14), **f32),
            "sigma": torch.ones(N, **f32), "nvalid": torch.ones(N, **f32)}
    spec = K.DetectSpec(horizons=torch.ones((N, 3), dtype=torch.int32, device=dev), threshold=torch.ones(N, **f32),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev), min_lower=torch.zeros(N, **f32))
    for bad in ({"harm": torch.zeros((N, 16), **f32)}, {"harm": torch.zeros((N, 14), dtype=torch.float64, device=dev)},
                {"level": torch.zeros((N, 1), **f32)}, {"slope": torch.zeros(N + 1, **f32)},
                {"sigma": torch.ones(N, **f32).cpu()}, {"nvalid": torch.ones(N, dtype=torch.int32, device=dev)}):
        with pytest.raises(K.KernelShapeError):
            K.prophet_state_detect(dict(good, **bad), m, spec)
    with pytest.raises(K.KernelShapeError):
        K.prophet_state_detect({k: v for k, v in good.items() if k != "harm"}, m, spec)
    with pytest.raises(K.KernelShapeError):
        K.prophet_state_detect(good, 1, spec)
    with pytest.raises(K.KernelShapeError):
        K.prophet_state_detect(good, 86401, spec)
    spec.max_horizon = (1 << 20) + 1
    with pytest.raises(K.KernelShapeError):
        K.prophet_state_detect(good, m, spec)
