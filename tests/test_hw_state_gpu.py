"""The cached Holt-Winters kernels (ops/csrc/hw_state.hip: kernels.hw_state,
kernels.hw_update_detect) against the fp64 oracle of tests/helpers/hw_state_cases.py.

Bounds (helpers/hw_state_cases.py, docs/SCORING.md): level / trend / season / forecast errors
are normalised by ``max|y|`` of the series and held to 4 x D, D being the distance of the fp32
CPU recursion from the same oracle on the same inputs (tests/test_hw_cache.py measures it).
``nvalid``, verdicts, counts, the anomaly list and the per-app counters are exact; phases an
update does not touch keep their bits.  ``upper`` / ``lower`` are compared with
``models/detect.py`` on the kernel's own forecast within 16 fp32 roundings of ``|f| + thr s``
(the h-step factor is ~10 fp32 operations and a square root, the band one multiply-add).

Every per-series buffer of the update tests is the head of a longer allocation whose spare
rows hold a sentinel: a row processed past N changes them.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from foremast_amd.models import detect as det_ref
from foremast_amd.models import smoothing as sm

pytestmark = pytest.mark.gpu


def _helper(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hc = _helper("hw_state_cases")
EPS32 = float(np.finfo(np.float32).eps)
SENT = 777.0
THR, MIN_VALID, PW_MIN = 3.0, 10, 2


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native
    from foremast_amd.ops import kernels
    _native.require()
    return kernels


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------
# hw_state
# ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_hw_state_matches_the_fp64_oracle(K, dev, name):
    b = hc.build(name)
    c = b["case"]
    R, head, ld = hc.ring_layout(c)
    grid = b["grid"].to(dev)
    # N == 1: one launch per row, so every dedicated row runs as the only live thread
    launches = [slice(i, i + 1) for i in range(c.n_rows)] if c.N == 1 else [slice(0, c.N)]
    for rows in launches:
        ring = hc.ring_of(c, b["y"], rows).to(dev)[:, :R]
        assert ring.stride(0) == ld and ring.shape[1] == R
        best = b["best"][rows].to(dev)
        st = K.hw_state(ring, head, c.T, c.m, grid, best)
        torch.cuda.synchronize()
        assert st["Tp"] == c.Tp
        assert st["season"].shape == (c.m, ring.shape[0])
        unit = b["unit"][rows]
        for key in ("level", "trend", "season"):
            got = st[key].cpu().T if key == "season" else st[key].cpu()
            err = hc.norm_err(got, b["ref"][key][rows], unit)
            print(f"{name} rows {rows.start}:{rows.stop} {key}: kernel vs fp64 {err.max():.3e} (row {err.argmax()})")
            assert err.max() <= hc.BOUND[key], (key, err.max(), rows.start + int(err.argmax()))
        assert np.array_equal(st["nvalid"].cpu().double().numpy(), b["ref"]["nvalid"][rows])
        k = hc.K_ALL - rows.start
        if 0 <= k < ring.shape[0]:
            assert st["level"][k] == 0 and st["trend"][k] == 0 and st["nvalid"][k] == 0
            assert not st["season"][:, k].any()
        # a reused state dict keeps its storage and is rewritten in full
        first = {key: st[key].clone() for key in ("level", "trend", "season", "nvalid")}
        ptrs = {key: st[key].data_ptr() for key in first}
        for key in first:
            st[key].fill_(SENT)
        st2 = K.hw_state(ring, head, c.T, c.m, grid, best, state=st)
        torch.cuda.synchronize()
        assert st2 is st and st2["Tp"] == c.Tp
        for key in first:
            assert st2[key].data_ptr() == ptrs[key], key
            assert torch.equal(st2[key], first[key]), key


def test_hw_state_rejects_bad_shapes(K, dev):
    m, n = 128, 4
    ring = torch.zeros((n, 3 * m), device=dev)
    grid = hc.default_grid().to(dev)
    best = torch.zeros(n, dtype=torch.int32, device=dev)
    K.hw_state(ring, 0, 2 * m, m, grid, best)   # the accepted minimum
    with pytest.raises(K.KernelShapeError):
        K.hw_state(torch.zeros((n, 3 * 127), device=dev), 0, 2 * 127, 127, grid, best)
    with pytest.raises(K.KernelShapeError):
        K.hw_state(ring, 0, m, m, grid, best)   # one season
    with pytest.raises(K.KernelShapeError):
        K.hw_state(ring, 0, 2 * m, m, grid, best.long())
    with pytest.raises(K.KernelShapeError):
        K.hw_state(ring, 0, 2 * m, m, grid, best[:n - 1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------
# hw_update_detect
# ---------------------------------------------------------------------------------

def _guarded(t: torch.Tensor, dev, fill=SENT):
    """(buffer, view): ``t`` as the first rows of a device buffer with ``hc.GUARD`` spare rows."""
    buf = torch.full((t.shape[0] + hc.GUARD,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    buf[:t.shape[0]] = t
    buf = buf.to(dev)
    return buf, buf[:t.shape[0]]


def _guard_intact(buf: torch.Tensor, n: int, fill=SENT) -> bool:
    return bool((buf[n:] == fill).all())


def _detect_inputs(u, hz: torch.Tensor, C: int, rng):
    """``cur`` placed around the oracle's forecast so that every rule has rows on each side,
    no point nearer than 0.2 thr s to a band edge (the forecast bound is < 1e-2 s)."""
    N, m = u["N"], u["case"].m
    n = np.arange(N)
    factor = det_ref.horizon_sigma_factor(u["params"], sm.MODE_HW, m, hz).double().numpy()
    factor = np.broadcast_to(factor, (N, C))
    sigma = (0.3 + u["unit"] * rng.uniform(1e-3, 2e-3, N)).astype(np.float32)
    s_h = sigma[:, None].astype(np.float64) * factor
    bound = np.array([1, 2, 3, 3], dtype=np.int8)[n % 4]
    side = np.where(bound == 2, -1.0, 1.0)            # an enabled side of the band
    role = n % 6
    z = rng.uniform(-0.3, 0.3, (N, C)) * THR          # inside the lowered band (0.5 thr)
    spike_col = rng.integers(0, C, N)
    z[role == 1, spike_col[role == 1]] = (1.6 * THR * side)[role == 1]        # outside the full band
    z[role == 2] = (0.75 * THR * side)[role == 2, None]                       # between the two bands
    z[role == 5, spike_col[role == 5]] = (-1.6 * THR * side)[role == 5]       # the other side
    cur = hc.oracle_forecast(u["ref"], hz.numpy()) + z * s_h
    cur[(role == 3)[:, None] & (rng.random((N, C)) < 0.3)] = np.nan
    cur[role == 4] = np.nan
    differs = ((n // 6) % 2).astype(np.uint8)
    return {"sigma": torch.from_numpy(sigma), "s_h": torch.from_numpy(s_h).float(),
            "bound": torch.from_numpy(bound), "cur": torch.from_numpy(cur).float(),
            "differs": torch.from_numpy(differs), "app_id": torch.from_numpy((n % 3).astype(np.int32))}


def _run_update(K, dev, u, C: int, per_series: bool, seen: set):
    c, N, npts, m = u["case"], u["N"], u["npts"], u["case"].m
    rng = np.random.default_rng(u["seed"] + 13 * C + per_series)
    R = 2 * m + 7 if m == 130 else 2 * m
    col0 = R - max(1, (npts + 1) // 2)                 # the points cross the ring's end
    dt = torch.bfloat16 if c.bf16 else torch.float32
    # ring: values of the series' scale everywhere (a wrong column is a wrong value), the new
    # points at col0 .. (mod R)
    ring = u["start"]["level"].double()[:, None] * torch.from_numpy(rng.uniform(0.5, 1.5, (N, R)))
    ring[:, (col0 + torch.arange(npts)) % R] = torch.from_numpy(u["ynew"])
    ring_buf, ring_v = _guarded(ring.to(dt), dev, fill=1.0)

    lvl_buf, lvl = _guarded(u["start"]["level"], dev)
    trd_buf, trd = _guarded(u["start"]["trend"], dev)
    sea_buf = torch.full((m * N + hc.GUARD,), SENT)
    sea_buf[:m * N] = u["start"]["season"].T.reshape(-1)
    sea_buf = sea_buf.to(dev)
    state = {"level": lvl, "trend": trd, "season": sea_buf[:m * N].view(m, N)}
    season0 = state["season"].clone()

    hz = hc.config_horizons(u, C, per_series)
    di = _detect_inputs(u, hz, C, rng)
    best_buf, best = _guarded(u["best"], dev, fill=0)
    sig_buf, sigma = _guarded(di["sigma"], dev)
    nv_buf, nvalid = _guarded(torch.from_numpy(u["nvalid"]).float(), dev)
    thr_buf, thr = _guarded(torch.full((N,), THR), dev)
    bnd_buf, bound = _guarded(di["bound"], dev, fill=3)
    ml_buf, min_lower = _guarded(torch.full((N,), -1e9), dev)
    dif_buf, differs = _guarded(di["differs"], dev, fill=1)
    app_buf, app_id = _guarded(di["app_id"], dev, fill=0)
    cur_buf, cur = _guarded(di["cur"], dev)
    hz_dev = _guarded(hz, dev, fill=1)[1] if per_series else hz.to(dev)
    app_stats = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    bufs = {k: torch.full((N + hc.GUARD, C), SENT, device=dev) for k in ("forecast", "upper", "lower")}
    bufs["count"] = torch.full((N + hc.GUARD,), 77, dtype=torch.int32, device=dev)
    bufs["verdict"] = torch.full((N + hc.GUARD,), 77, dtype=torch.int8, device=dev)
    bufs["score"] = torch.full((N + hc.GUARD,), SENT, device=dev)
    out = {k: v[:N] for k, v in bufs.items()}
    spec = K.DetectSpec(horizons=hz_dev, threshold=thr, bound=bound, min_lower=min_lower, cur=cur, differs=differs,
                        pw_scale=0.5, pw_min_points=PW_MIN, min_valid=MIN_VALID, app_id=app_id, app_stats=app_stats,
                        anomalies=K.AnomalyBuffer(N * C + 8, dev), horizon_variance=True)
    res = K.hw_update_detect(ring_v, col0, npts, u["t_last"], m, u["grid"].to(dev), best, state, sigma, nvalid,
                             spec, out=out)
    torch.cuda.synchronize()
    assert res is out
    tag = f"{c.name} N={N} npts={npts} C={C} per_series={per_series}"

    # state
    ref = u["ref"]
    got = {"level": lvl.cpu(), "trend": trd.cpu(), "season": state["season"].cpu().T}
    for key in ("level", "trend", "season"):
        err = hc.norm_err(got[key], ref[key], u["unit"])
        print(f"{tag} {key}: kernel vs fp64 {err.max():.3e}")
        assert err.max() <= hc.BOUND_UPD[key], (tag, key, err.max(), int(err.argmax()))
    touched = torch.zeros(m, dtype=torch.bool)
    touched[(u["t_last"] + 1 + torch.arange(npts)) % m] = True
    assert torch.equal(state["season"][~touched.to(dev)], season0[~touched.to(dev)]), tag
    if npts == 0:
        assert torch.equal(lvl.cpu(), u["start"]["level"]) and torch.equal(trd.cpu(), u["start"]["trend"]), tag
    # nothing written past row N
    assert _guard_intact(lvl_buf, N) and _guard_intact(trd_buf, N) and _guard_intact(sea_buf, m * N), tag
    for k, fill in (("forecast", SENT), ("upper", SENT), ("lower", SENT), ("count", 77), ("verdict", 77),
                    ("score", SENT)):
        assert _guard_intact(bufs[k], N, fill), (tag, k)

    # forecast
    f = out["forecast"].cpu()
    err = hc.norm_err(f, hc.oracle_forecast(ref, hz.numpy()), u["unit"])
    print(f"{tag} forecast: kernel vs fp64 {err.max():.3e}")
    assert err.max() <= hc.BOUND_UPD["forecast"], (tag, err.max(), int(err.argmax()))

    # band, verdict, count, anomaly list, per-app counters: models/detect.py on the kernel's forecast
    thr_c = torch.full((N,), THR)
    ok = torch.from_numpy(u["nvalid"] >= MIN_VALID)
    d = det_ref.detect(f, di["s_h"], di["cur"], thr_c, di["bound"], torch.full((N,), -1e9), differs=di["differs"],
                       pairwise_scale=0.5, model_ok=ok, pw_min_points=PW_MIN)
    assert torch.equal(out["verdict"].cpu(), d.verdict), tag
    assert torch.equal(out["count"].cpu(), d.count), tag
    tol = 16 * EPS32 * (f.abs() + THR * di["s_h"])
    for key, want in (("upper", d.upper), ("lower", d.lower)):
        assert bool(((out[key].cpu() - want).abs() <= tol).all()), (tag, key)
    s_, c_, v_, overflow = spec.anomalies.fetch()
    exp = d.anomaly.nonzero().numpy()
    assert not overflow and len(exp) == len(s_) and (exp[:, 0] == s_).all() and (exp[:, 1] == c_).all(), tag
    assert (v_ == di["cur"].numpy()[exp[:, 0], exp[:, 1]]).all(), tag
    stats = torch.zeros((3, 2), dtype=torch.int32)
    stats[:, 0] = torch.bincount(di["app_id"][d.verdict == 1].long(), minlength=3)
    stats[:, 1] = torch.bincount(di["app_id"][d.verdict >= 0].long(), minlength=3)
    assert torch.equal(app_stats.cpu(), stats), tag
    seen.update(int(v) for v in d.verdict)
    low = di["differs"].bool() & (d.count > 0) & (torch.arange(N) % 6 == 2)
    if bool(low.any()):
        seen.add("low")
    if bool(((torch.arange(N) % 6 == 2) & ~di["differs"].bool() & (d.verdict == 0)).any()):
        seen.add("not_low")


def _update_case(K, dev, name, N, npts):
    u = hc.update_inputs(name, N, npts)
    seen = set()
    for C, per_series in hc.CONFIGS:
        _run_update(K, dev, u, C, per_series, seen)
    if N >= 17:
        # anomalous, healthy and unknown (no model / no point) rows; the lowered band fired
        # where the pods differ and did not where they do not
        assert {1, 0, -1, "low", "not_low"} <= seen, seen
        assert int((u["nvalid"] < MIN_VALID).sum()) >= 2


@pytest.mark.parametrize("npts", hc.NPTS(130))
@pytest.mark.parametrize("N", [1, 17, 67])
@pytest.mark.parametrize("name", ["u130_fp32", "u130_bf16"])
def test_hw_update_detect_matches_the_fp64_oracle(K, dev, name, N, npts):
    _update_case(K, dev, name, N, npts)


def test_hw_update_detect_production_season(K, dev):
    _update_case(K, dev, "u1440_bf16", 33, 3)
