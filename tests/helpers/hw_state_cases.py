"""Shared inputs of the cached Holt-Winters tests (tests/test_hw_state_gpu.py and the CPU
test in tests/test_hw_cache.py): an fp64 oracle of the recursion in models/smoothing.py
(``hw_run``, ``hw_update``, ``hw_state_forecast``), the case table, the series and rings of
every case, and the error bounds.

Bounds.  Errors are normalised per series by ``max|y|`` of its window (an all-NaN series must
be exactly 0).  ``D_*`` is the largest normalised distance of the fp32 CPU recursion
(``models/smoothing.py``) from the fp64 oracle over the case table below; the kernels are
another fp32 evaluation of the same recursion (contracted multiply-adds, sequential season
means where torch sums pairwise), so they are held to ``4 x D``.  A phase, padding, column or
NaN error is of the order of the seasonal amplitude (0.03 to 0.4 of the level here), 1e4 times
larger.  The CPU test (tests/test_hw_cache.py) holds the fp32 CPU recursion to ``2 x D``: torch's summation order, and
with it the last bits of the season means, depends on the host's vector width.
"""

from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

# D: the fp32 CPU recursion against the fp64 oracle, worst series, in units of max|y|
# (docs/SCORING.md has the per-case figures).  Two sets, since the two kernels do different work:
# the state after a window (sm.hw_run over CASES), and the state and forecast after an update
# from the oracle's own state (sm.hw_update / sm.hw_state_forecast over UPDATE_CASES, every N,
# npts and horizon set of the GPU tests).  The update's level figure comes from the rows whose
# m + 5 new points are all NaN: 135 uncorrected ``level + trend`` additions, whose roundings add up.
D_LEVEL = 6.97e-7        # measured 6.97e-7 (m191_k4_pad64)
D_TREND = 1.90e-8        # measured 1.90e-8 (m130_k3_pad129)
D_SEASON = 7.13e-7       # measured 7.13e-7 (m1440_k3_pad7)
D_UPD_LEVEL = 3.72e-6    # measured 3.72e-6 (u130_fp32, N = 17, npts = 135)
D_UPD_TREND = 2.08e-8    # measured 2.08e-8 (u130_fp32, npts = 135)
D_UPD_SEASON = 1.40e-7   # measured 1.40e-7 (u130_bf16, N = 67, npts = 135)
D_FORECAST = 5.46e-6     # measured 5.46e-6 (u130_fp32, npts = 135; horizons up to 2 m + 1)
KERNEL_HEADROOM = 4.0
BOUND = {"level": KERNEL_HEADROOM * D_LEVEL, "trend": KERNEL_HEADROOM * D_TREND,
         "season": KERNEL_HEADROOM * D_SEASON}
BOUND_UPD = {"level": KERNEL_HEADROOM * D_UPD_LEVEL, "trend": KERNEL_HEADROOM * D_UPD_TREND,
             "season": KERNEL_HEADROOM * D_UPD_SEASON, "forecast": KERNEL_HEADROOM * D_FORECAST}
CPU_HEADROOM = 2.0

NOISE = 0.3
NAN_FRAC = 0.02
GUARD = 16     # spare rows behind every per-series buffer of the update tests
# kinds of the dedicated rows (row i of a case has kind i; later rows have random 2 % NaN)
KINDS = ("dense", "season0_nan", "season1_nan", "all_nan", "last_only", "edges")
K_DENSE, K_S0, K_S1, K_ALL, K_LAST, K_EDGES = range(6)


class Case(NamedTuple):
    name: str
    m: int
    seasons: int     # Tp / m
    pad: int         # front padding: T = Tp - pad
    N: int           # series per launch
    ring: str        # ring layout, see ring_layout()
    bf16: bool
    rows: int = 0    # series built (>= N; N == 1 launches once per row): default max(N, 8)

    @property
    def Tp(self) -> int:
        return self.seasons * self.m

    @property
    def T(self) -> int:
        return self.Tp - self.pad

    @property
    def n_rows(self) -> int:
        return self.rows or max(self.N, 8)


CASES = (
    # minimum season and window: pass 2 runs only the `first` branch; one live thread
    Case("m128_k2_n1", 128, 2, 0, 1, "slack50_head77", False),
    # 2-step partial chunks, phase wrap mid-chunk, one valid season-0 sample, block + 1 row, full ring
    Case("m130_k3_pad129", 130, 3, 129, 129, "full_wrap5", False),
    # odd season (63-step partial chunk), pad equal to one chunk
    Case("m191_k4_pad64", 191, 4, 64, 64, "plus1_head0", True),
    # ld != ring_len, bf16 rows at odd element offsets, fewer rows than a wave
    Case("m192_k3_strided", 192, 3, 1, 63, "strided", True),
    # the production season
    Case("m1440_k3_pad7", 1440, 3, 7, 130, "full_head1000", True),
)
# the update / detect tests start from the oracle's state of these windows advanced by
# UPDATE_AHEAD more points (t_last = Tp - 1 + UPDATE_AHEAD), on the first N rows
UPDATE_AHEAD = 17
UPDATE_CASES = (
    Case("u130_fp32", 130, 3, 5, 67, "none", False),
    Case("u130_bf16", 130, 3, 5, 67, "none", True),
    Case("u1440_bf16", 1440, 2, 0, 33, "none", True),
)
ALL_CASES = CASES + UPDATE_CASES
CASE_BY_NAME = {c.name: c for c in ALL_CASES}


def ring_layout(c: Case):
    """(R, head, ld): ring length, physical column of logical t = 0, row stride."""
    T = c.T
    if c.ring == "slack50_head77":
        return T + 50, 77, T + 50
    if c.ring == "full_wrap5":
        return T, T - 5, T
    if c.ring == "plus1_head0":
        return T + 1, 0, T + 1
    if c.ring == "strided":
        return T + 6, T - 100, T + 6 + 11
    if c.ring == "full_head1000":
        return T, 1000, T
    raise ValueError(c.ring)


def default_grid() -> torch.Tensor:
    """The 64-point default grid (utils/config.py hw_alpha x hw_beta x hw_gamma), fp32 [64, 3]."""
    rows = [(a, b, g) for a in (0.1, 0.3, 0.5, 0.8) for b in (0.0, 0.01, 0.05, 0.1) for g in (0.05, 0.1, 0.3, 0.5)]
    return torch.tensor(rows, dtype=torch.float32)


def make_series(n: int, m: int, Tp: int, pad: int, extra: int, seed: int, bf16: bool) -> Dict[str, np.ndarray]:
    """``n`` series over padded times ``pad .. Tp + extra - 1``: a level drawn from 5 .. 5000,
    a small slope, an independent random value per phase (a one-phase slip is as large as the
    profile), noise 0.3; rounded to the ring's dtype.  ``y [n, Tp - pad + extra]`` float64 (the
    rounded values), without NaN."""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.uniform(np.log(5.0), np.log(5000.0), n))
    slope = level * rng.uniform(-2e-5, 2e-5, n)
    amp = level * rng.uniform(0.03, 0.4, n)
    prof = amp[:, None] * rng.uniform(-1.0, 1.0, (n, m))
    tp = np.arange(pad, Tp + extra)
    y = level[:, None] + slope[:, None] * tp[None, :] + prof[:, tp % m] + NOISE * rng.standard_normal((n, len(tp)))
    t = torch.from_numpy(y).float()
    t = t.bfloat16().float() if bf16 else t
    return {"y": t.double().numpy(), "level": level, "prof": prof}


def apply_kinds(y: np.ndarray, m: int, Tp: int, pad: int, seed: int) -> np.ndarray:
    """NaN patterns of the window ``y [n, T]`` (in place): the dedicated rows, then random 2 %."""
    n, T = y.shape
    rng = np.random.default_rng(seed + 7919)

    def cols(lo, hi):  # logical columns of padded steps [lo, hi)
        return slice(max(lo - pad, 0), max(hi - pad, 0))
    for i in range(n):
        k = i if i < len(KINDS) else -1
        if k == K_DENSE:
            continue
        if k == K_S0:
            y[i, cols(0, m)] = np.nan
        elif k == K_S1:
            y[i, cols(m, 2 * m)] = np.nan
        elif k == K_ALL:
            y[i, :] = np.nan
        elif k == K_LAST:
            y[i, :T - 1] = np.nan
        elif k == K_EDGES:
            for tp in (63, 64, m - 1, m, 2 * m - 1, 2 * m, Tp - 1, pad):
                if pad <= tp < Tp:
                    y[i, tp - pad] = np.nan
        else:
            y[i, rng.random(T) < NAN_FRAC] = np.nan
    return y


# ---------------------------------------------------------------------------------
# fp64 oracle (plain numpy; never calls the fp32 model code)
# ---------------------------------------------------------------------------------

def _nanmean0(x: np.ndarray) -> np.ndarray:
    """Row means over the valid samples; 0 for a row with none."""
    v = ~np.isnan(x)
    cnt = v.sum(1)
    s = np.where(v, x, 0.0).sum(1)
    return np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)


def _params64(params) -> np.ndarray:
    return np.asarray(params.numpy() if torch.is_tensor(params) else params, dtype=np.float64)


def oracle_run(y: np.ndarray, params, m: int, Tp: int) -> Dict[str, object]:
    """State after padded step ``Tp - 1`` of ``y [N, T]`` float64 front-padded with NaN to ``Tp``:
    ``l0`` / ``b0`` from the means of seasons 0 and 1 (0 when empty), ``s[p] = y[p] - l0`` (0
    where missing), then the error-correction recursion over steps ``m .. Tp - 1`` with a NaN
    point imputed by the forecast.  ``nvalid``: valid points of those steps."""
    y = np.asarray(y, dtype=np.float64)
    N, T = y.shape
    assert Tp % m == 0 and Tp // m >= 2 and 0 < T <= Tp
    yp = np.concatenate([np.full((N, Tp - T), np.nan), y], axis=1)
    p = _params64(params)
    al, ab, g1a = p[:, 0], p[:, 0] * p[:, 1], p[:, 2] * (1.0 - p[:, 0])
    s0 = yp[:, :m]
    l0 = _nanmean0(s0)
    lvl = l0.copy()
    trd = (_nanmean0(yp[:, m:2 * m]) - l0) / m
    season = np.where(np.isnan(s0), 0.0, s0 - l0[:, None])
    for t in range(m, Tp):
        ph = t % m
        yt = yp[:, t]
        e = np.where(np.isnan(yt), 0.0, yt - season[:, ph] - lvl - trd)
        lvl = lvl + trd + al * e
        trd = trd + ab * e
        season[:, ph] = season[:, ph] + g1a * e
    return {"level": lvl, "trend": trd, "season": season, "t_last": Tp - 1, "m": m,
            "nvalid": (~np.isnan(yp[:, m:])).sum(1).astype(np.float64)}


def oracle_update(st: Dict[str, object], ynew: np.ndarray, params) -> Dict[str, object]:
    """A copy of ``st`` advanced by the points ``ynew [N, k]`` (oldest first, NaN imputed)."""
    p = _params64(params)
    al, ab, g1a = p[:, 0], p[:, 0] * p[:, 1], p[:, 2] * (1.0 - p[:, 0])
    lvl, trd, season, t, m = st["level"].copy(), st["trend"].copy(), st["season"].copy(), st["t_last"], st["m"]
    ynew = np.asarray(ynew, dtype=np.float64)
    for j in range(ynew.shape[1]):
        t += 1
        ph = t % m
        yt = ynew[:, j]
        e = np.where(np.isnan(yt), 0.0, yt - season[:, ph] - lvl - trd)
        lvl = lvl + trd + al * e
        trd = trd + ab * e
        season[:, ph] = season[:, ph] + g1a * e
    return {**st, "level": lvl, "trend": trd, "season": season, "t_last": t}


def oracle_forecast(st: Dict[str, object], horizons: np.ndarray) -> np.ndarray:
    """``[N, C]`` forecasts ``level + h trend + season[(t_last + h) mod m]``; ``horizons [C]`` or ``[N, C]``."""
    h = np.asarray(horizons, dtype=np.int64)
    N = st["level"].shape[0]
    h = np.broadcast_to(h if h.ndim == 2 else h[None, :], (N, h.shape[-1]))
    ph = (st["t_last"] + h) % st["m"]
    return st["level"][:, None] + h * st["trend"][:, None] + np.take_along_axis(st["season"], ph, axis=1)


def unit_of(y: np.ndarray) -> np.ndarray:
    """``max|y|`` per row over its valid samples (1 for an all-NaN row, whose state must be 0)."""
    a = np.where(np.isnan(y), 0.0, np.abs(y)).max(1)
    return np.where(a > 0, a, 1.0)


def norm_err(got, ref: np.ndarray, unit: np.ndarray) -> np.ndarray:
    """Per-series largest ``|got - ref| / unit`` (``got``: tensor or array, ``[N]`` or ``[N, k]``)."""
    g = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    d = np.abs(g - ref)
    d = d.reshape(d.shape[0], -1).max(1) if d.size else np.zeros(d.shape[0])
    return d / unit


# ---------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------

def horizon_values(m: int, t: int, npts: int) -> List[int]:
    """Horizons every forecast test covers, for a state at padded time ``t`` whose last
    ``npts`` phases were just written: 1; the wrap of ``(t + h) % m`` (phases m - 1 and 0);
    ``h = m - j`` for the applied points ``j`` (j = 0: the last one, phase of ``t``); ``m + 3``
    and ``2 m + 1`` (seasonal-lag term of the h-step variance)."""
    wrap = m - (t % m)
    hs = [1, wrap, wrap - 1 if wrap > 1 else m + wrap - 1, m, m - 1, m - 2, m + 3, 2 * m + 1, 2, 7]
    assert all(h >= 1 for h in hs)
    return hs


def draw_horizons(m: int, t: int, npts: int, N: int, C: int, per_series: bool, seed: int) -> torch.Tensor:
    """int32 ``[C]`` or ``[N, C]``: the values of :func:`horizon_values` first (rotated by the
    row, so with C = 1 every row has another), then random values in ``1 .. m + 10``."""
    hs = horizon_values(m, t, npts)
    rng = np.random.default_rng(seed)
    rows = N if per_series else 1
    hz = rng.integers(1, m + 11, (rows, C))
    for r in range(rows):
        k = min(C, len(hs))
        hz[r, :k] = np.roll(hs, -(r + seed))[:k]
    t_ = torch.from_numpy(hz.astype(np.int32))
    return t_ if per_series else t_[0].contiguous()


@functools.lru_cache(maxsize=None)
def build(name: str) -> Dict[str, object]:
    """Everything the tests of one case share (do not modify): ``y`` (window ``[rows, T]``
    float64 as the ring holds it, NaN patterns applied), ``best`` int32, ``params`` fp32
    ``[rows, 3]``, ``unit``, the oracle state ``ref`` and the ``ahead`` points after the window
    with the oracle state ``ref_ahead`` after them (the update tests start there)."""
    c = CASE_BY_NAME[name]
    seed = 1000 + [k.name for k in ALL_CASES].index(name)
    n = c.n_rows
    s = make_series(n, c.m, c.Tp, c.pad, UPDATE_AHEAD, seed, c.bf16)
    y = apply_kinds(s["y"][:, :c.T].copy(), c.m, c.Tp, c.pad, seed)
    ahead = s["y"][:, c.T:].copy()
    rng = np.random.default_rng(seed + 1)
    ahead[rng.random(ahead.shape) < 0.05] = np.nan
    grid = default_grid()
    best = torch.from_numpy(rng.integers(0, grid.shape[0], n).astype(np.int32))
    params = grid[best.long()]
    ref = oracle_run(y, params, c.m, c.Tp)
    return {"case": c, "y": y, "ahead": ahead, "grid": grid, "best": best, "params": params,
            "unit": unit_of(y), "ref": ref, "ref_ahead": oracle_update(ref, ahead, params), "seed": seed}


def ring_of(c: Case, y: np.ndarray, rows: Optional[slice] = None) -> torch.Tensor:
    """The window ``y[rows]`` laid into the case's ring (CPU tensor of the ring's dtype, shape
    ``[n, R]``, row stride ``ld``); columns outside the window hold a large finite value, so a
    read outside the window shows."""
    R, head, ld = ring_layout(c)
    yy = y if rows is None else y[rows]
    wide = torch.full((yy.shape[0], ld), 3.0e4, dtype=torch.float64)
    idx = (torch.arange(c.T) + head) % R
    wide[:, idx] = torch.from_numpy(yy)
    return wide.to(torch.bfloat16 if c.bf16 else torch.float32)


def new_points(b: Dict[str, object], npts: int, all_nan_row: Optional[int]) -> np.ndarray:
    """``npts`` points per series after ``ref_ahead`` (float64, rounded to the ring's dtype):
    the series continued from its level and seasonal state, 10 % NaN, one row all NaN."""
    c, st = b["case"], b["ref_ahead"]
    n = st["level"].shape[0]
    rng = np.random.default_rng(b["seed"] + 31 * npts + 5)
    t = st["t_last"] + 1 + np.arange(npts)
    y = st["level"][:, None] + st["season"][:, t % c.m] + NOISE * rng.standard_normal((n, npts))
    tt = torch.from_numpy(y).float()
    y = (tt.bfloat16().float() if c.bf16 else tt).double().numpy()
    y[rng.random(y.shape) < 0.10] = np.nan
    if all_nan_row is not None and npts:
        y[all_nan_row] = np.nan
    return y


def NPTS(m: int):
    """New points per update; m + 5: five phases are read again after the update wrote them."""
    return (0, 1, 3, m + 5)


# (C, per-series horizons) of the forecasts taken after every update
CONFIGS = ((1, False), (10, True), (16, False), (17, True), (40, False),
           (1, True), (10, False), (16, True), (17, False), (40, True))


@functools.lru_cache(maxsize=None)
def update_inputs(name: str, N: int, npts: int) -> Dict[str, object]:
    """Inputs and oracle of one update (do not modify): the first ``N`` rows of the case's
    oracle state after ``UPDATE_AHEAD`` points, cast to fp32 (``level`` / ``trend`` ``[N]``,
    ``season [N, m]``: what the kernel and ``sm.hw_update`` start from), ``ynew [N, npts]``
    (float64, row ``N - 1`` all NaN when N > 1), the oracle state ``ref`` after them starting
    from that same fp32 state, and ``unit`` = max|y| over the window and every applied point."""
    b = build(name)
    c = b["case"]
    st = b["ref_ahead"]
    ynew = new_points(b, npts, N - 1 if N > 1 else None)[:N]
    f32 = {k: torch.from_numpy(st[k][:N]).float() for k in ("level", "trend", "season")}
    start = {**st, **{k: v.double().numpy() for k, v in f32.items()}, "nvalid": st["nvalid"][:N]}
    params = b["params"][:N]
    seen = np.concatenate([b["y"][:N], b["ahead"][:N], ynew], axis=1)
    return {"case": c, "N": N, "npts": npts, "t_last": st["t_last"], "start": f32, "ynew": ynew,
            "params": params, "best": b["best"][:N], "grid": b["grid"], "nvalid": st["nvalid"][:N],
            "ref": oracle_update(start, ynew, params), "unit": unit_of(seen), "seed": b["seed"] + 101 * N + npts}


def config_horizons(u: Dict[str, object], C: int, per_series: bool) -> torch.Tensor:
    c = u["case"]
    return draw_horizons(c.m, u["t_last"] + u["npts"], u["npts"], u["N"], C, per_series, u["seed"] + C)
