"""Batched Prophet-style additive model (``ML_ALGORITHM=prophet``).

The reference brain lists Prophet among its univariate models
(``docs/guides/design.md:68-72``; ``foremast-brain/README.md:14-20``).  Prophet
fits  y(t) = g(t) + s(t) + e  with a piecewise-linear trend g (changepoints
in the first 80 % of the history, sparse slope changes) and Fourier-series
seasonalities s (daily, weekly), by MAP optimisation per series.

Here the same model family is fit for *all* series of a batch at once as a
weighted ridge regression — one batched ``[B, P, P]`` normal-equation solve
on the GPU (rocBLAS/rocSOLVER via torch) instead of B independent L-BFGS
runs:

* features per series: intercept, scaled time, ``n_changepoints`` hinge
  terms ``max(0, t - c_k)`` (L2-penalised slope changes — the Laplace prior's
  ridge analogue), daily Fourier terms (order 4) when the history spans >= 2
  days, weekly (order 3) when >= 2 weeks — Prophet's auto-enable rules;
* NaN gaps get zero weight;
* the band is ``forecast ± threshold * sigma`` with sigma the residual
  standard deviation (Prophet samples trend uncertainty; the reference
  thresholds the interval the same way, design decision in docs/SCORING.md).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import torch

DAY = 86400.0
WEEK = 7 * DAY


@dataclass
class ProphetFit:
    beta: torch.Tensor        # [B, P]
    sigma: torch.Tensor       # [B]
    n_valid: torch.Tensor     # [B]
    t0: torch.Tensor          # [B] first timestamp
    span: torch.Tensor        # [B] history span (s)
    cps: torch.Tensor         # [B, K] changepoints in scaled time
    yscale: torch.Tensor      # [B]
    seasons: Tuple[Tuple[float, int], ...]


def _features(ts: torch.Tensor, t0: torch.Tensor, span: torch.Tensor, cps: torch.Tensor,
              seasons) -> torch.Tensor:
    """ts [B, T] seconds → X [B, T, P]."""
    s = (ts - t0[:, None]) / span[:, None]
    hinge = torch.clamp(s[:, :, None] - cps[:, None, :], min=0.0)  # trend slope changes
    parts = [torch.stack([torch.ones_like(s), s], 2), hinge]
    for period, order in seasons:
        k = torch.arange(1, order + 1, dtype=ts.dtype, device=ts.device)
        ang = 2 * math.pi * (ts[:, :, None] / period) * k  # absolute time: phase-consistent across series
        parts += [torch.sin(ang), torch.cos(ang)]
    return torch.cat(parts, 2)


def fit_prophet(hist: torch.Tensor, hist_end: torch.Tensor, step: torch.Tensor, n_changepoints: int = 10,
                cp_range: float = 0.8, ridge_cp: float = 10.0, ridge: float = 1e-4) -> ProphetFit:
    """``hist [B, T]`` (NaN = missing; last sample at ``hist_end``, spacing ``step``)."""
    B, T = hist.shape
    dev = hist.device
    dt = torch.float64
    y = hist.to(dt)
    w = (~torch.isnan(y)).to(dt)
    y = torch.nan_to_num(y, nan=0.0)
    j = torch.arange(T, dtype=dt, device=dev)
    ts = hist_end.to(dt)[:, None] - (T - 1 - j)[None, :] * step.to(dt)[:, None]
    # first/last valid timestamps per series
    big = torch.tensor(float("inf"), dtype=dt, device=dev)
    t0 = torch.where(w > 0, ts, big).min(1).values
    t1 = torch.where(w > 0, ts, -big).max(1).values
    ok = torch.isfinite(t0) & (t1 > t0)
    t0 = torch.where(ok, t0, ts[:, 0])
    span = torch.where(ok, t1 - t0, torch.full_like(t0, 1.0))
    cps = (torch.arange(1, n_changepoints + 1, dtype=dt, device=dev) / (n_changepoints + 1) * cp_range)
    cps = cps[None, :].expand(B, -1).contiguous()
    span_max = float(span.max()) if B else 0.0
    seasons: List[Tuple[float, int]] = []
    if span_max >= 2 * DAY:
        seasons.append((DAY, 4))
    if span_max >= 2 * WEEK:
        seasons.append((WEEK, 3))
    X = _features(ts, t0, span, cps, seasons)  # [B, T, P]
    P = X.shape[2]
    ysc = torch.where(w > 0, y.abs(), torch.zeros_like(y)).max(1).values.clamp(min=1e-12)
    yn = y / ysc[:, None]
    Xw = X * w[:, :, None]
    A = Xw.transpose(1, 2) @ X  # [B, P, P]
    reg = torch.full((P,), ridge, dtype=dt, device=dev)
    reg[2:2 + n_changepoints] = ridge_cp
    A = A + torch.diag(reg)[None]
    rhs = (Xw.transpose(1, 2) @ yn[:, :, None])  # [B, P, 1]
    beta = torch.linalg.solve(A, rhs)[:, :, 0]
    r = (yn - (X @ beta[:, :, None])[:, :, 0]) * w
    n = w.sum(1)
    sigma = torch.sqrt((r * r).sum(1) / (n - P).clamp(min=1.0)) * ysc
    return ProphetFit(beta=beta, sigma=sigma.to(hist.dtype), n_valid=n.to(torch.int32), t0=t0, span=span,
                      cps=cps, yscale=ysc, seasons=tuple(seasons))


def forecast(fit: ProphetFit, ts: torch.Tensor) -> torch.Tensor:
    """``ts [B, C]`` absolute timestamps → forecast ``[B, C]``."""
    X = _features(ts.to(torch.float64), fit.t0, fit.span, fit.cps, fit.seasons)
    return ((X @ fit.beta[:, :, None])[:, :, 0] * fit.yscale[:, None]).to(torch.float32)


# ---------------------------------------------------------------------------------
# Window-scaled variant (streaming shards, ops/csrc/prophet.hip)
# ---------------------------------------------------------------------------------
#
# Every series of a ring shares the step and the window, so with time scaled by the
# WINDOW (logical index t = 0 .. T-1, s = t / (T-1)) instead of by each series' first and
# last valid sample, the design matrix X [T, P] is the same for all of them: the fit is
# rhs = X' (w y) per series against one shared table.  The seasons are decided by the
# window as well (daily iff T-1 >= 2m, weekly iff T-1 >= 14m, m = samples per day).  The
# Fourier phase origin is the window's first sample: the ridge is isotropic on each
# (sin k, cos k) pair, so the origin changes neither forecasts nor residuals.

@dataclass
class ProphetWindowFit(ProphetFit):
    T: int = 0
    m: int = 0
    n_changepoints: int = 10
    cp_range: float = 0.8
    phase: float = 0.0


def window_seasons(T: int, m: int) -> Tuple[Tuple[float, int], ...]:
    """``((period in samples, order), ...)`` of a window of ``T`` samples, ``m`` per day."""
    seasons: List[Tuple[float, int]] = []
    if T - 1 >= 2 * m:
        seasons.append((float(m), 4))
    if T - 1 >= 14 * m:
        seasons.append((float(7 * m), 3))
    return tuple(seasons)


def _window_features(t: torch.Tensor, T: int, m: int, n_changepoints: int, cp_range: float,
                     phase: float = 0.0) -> torch.Tensor:
    """Logical sample indices ``t [...]`` (fp64) → features ``[..., P]``; ``phase``
    shifts the Fourier origin (in samples)."""
    s = t / float(T - 1)
    cps = torch.arange(1, n_changepoints + 1, dtype=t.dtype, device=t.device) / (n_changepoints + 1) * cp_range
    parts = [torch.stack([torch.ones_like(s), s], -1), torch.clamp(s[..., None] - cps, min=0.0)]
    for period, order in window_seasons(T, m):
        k = torch.arange(1, order + 1, dtype=t.dtype, device=t.device)
        ang = 2 * math.pi * ((t[..., None] + phase) / period) * k
        parts += [torch.sin(ang), torch.cos(ang)]
    return torch.cat(parts, -1)


def design_window(T: int, m: int, hmax: int, n_changepoints: int = 10, cp_range: float = 0.8,
                  ridge_cp: float = 10.0, ridge: float = 1e-4, phase: float = 0.0):
    """Shared tables of a ``T``-sample window (fp64): ``X [T, P]``, the horizon rows
    ``XH [hmax, P]`` (features of logical index ``T-1+h``, h = 1..hmax), the ridge vector
    ``reg [P]`` and the gap-free normal matrix ``A_dense = X'X + diag(reg)``."""
    if T < 2 or m < 2:
        raise ValueError("design_window needs T >= 2 and m >= 2")
    dt = torch.float64
    X = _window_features(torch.arange(T, dtype=dt), T, m, n_changepoints, cp_range, phase)
    XH = _window_features(torch.arange(T, T + hmax, dtype=dt), T, m, n_changepoints, cp_range, phase)
    P = X.shape[1]
    reg = torch.full((P,), ridge, dtype=dt)
    reg[2:2 + n_changepoints] = ridge_cp
    return X, XH, reg, X.T @ X + torch.diag(reg)


def fit_prophet_window(hist: torch.Tensor, m: int, n_changepoints: int = 10, cp_range: float = 0.8,
                       ridge_cp: float = 10.0, ridge: float = 1e-4, phase: float = 0.0) -> ProphetWindowFit:
    """Window-scaled fit of ``hist [N, T]`` (NaN = missing) in fp64, in data units
    (``beta`` is :func:`fit_prophet`'s ``beta * yscale``; the fit is linear in y)."""
    N, T = hist.shape
    dev, dt = hist.device, torch.float64
    X, _, reg, _ = design_window(T, m, 1, n_changepoints, cp_range, ridge_cp, ridge, phase)
    X, reg = X.to(dev), reg.to(dev)
    P = X.shape[1]
    y = hist.to(dt)
    w = (~torch.isnan(y)).to(dt)
    y = torch.nan_to_num(y, nan=0.0)
    XX = (X[:, :, None] * X[:, None, :]).reshape(T, P * P)
    A = (w @ XX).reshape(N, P, P) + torch.diag(reg)[None]
    rhs = y @ X  # y is 0 where missing
    beta = torch.linalg.solve(A, rhs[:, :, None])[:, :, 0]
    r = (y - beta @ X.T) * w
    n = w.sum(1)
    sigma = torch.sqrt((r * r).sum(1) / (n - P).clamp(min=1.0))
    cps = (torch.arange(1, n_changepoints + 1, dtype=dt, device=dev) / (n_changepoints + 1) * cp_range)
    return ProphetWindowFit(beta=beta, sigma=sigma.to(torch.float32), n_valid=n.to(torch.int32),
                            t0=torch.zeros(N, dtype=dt, device=dev),
                            span=torch.full((N,), float(T - 1), dtype=dt, device=dev),
                            cps=cps[None, :].expand(N, -1).contiguous(),
                            yscale=torch.ones(N, dtype=dt, device=dev), seasons=window_seasons(T, m),
                            T=T, m=m, n_changepoints=n_changepoints, cp_range=cp_range, phase=phase)


def forecast_window(fit: ProphetWindowFit, horizons: torch.Tensor) -> torch.Tensor:
    """``horizons [C]`` or ``[N, C]`` (steps past the window's last sample, >= 1) → ``[N, C]``."""
    h = horizons.to(fit.beta.device, torch.float64)
    XH = _window_features(float(fit.T - 1) + h, fit.T, fit.m, fit.n_changepoints, fit.cp_range, fit.phase)
    if h.dim() == 1:
        return (fit.beta @ XH.T).to(torch.float32)
    return (XH * fit.beta[:, None, :]).sum(-1).to(torch.float32)


# ---------------------------------------------------------------------------------
# Harmonic forecast state (resident rollout engine, ops/csrc/prophet.hip)
# ---------------------------------------------------------------------------------
#
# The rollout engine fits a row once, at admission, and scores it every tick at horizons
# that grow with the job.  Past the window every hinge is active (cp_range < 1 puts every
# changepoint inside it), so the model collapses to a line plus the Fourier terms with
# their phase moved to the window's last sample:
#
#   f(h) = level + slope h + sum_j [ A_j sin(w_j h) + B_j cos(w_j h) ],   h = steps past T-1
#   level = b0 + b1 + sum_k d_k (1 - c_k),   slope = (b1 + sum_k d_k) / (T - 1)
#   w = 2 pi k / p,  th = w (T - 1 + phase):   A = a_s cos th - a_c sin th,  B = a_s sin th + a_c cos th
#
# A row of any window length has the same 16-float state, so rows fitted at different
# geometries share one table and one scoring kernel.

STATE_SEASONS = ((1, 4), (7, 3))     # (period in days, order): the seasons a window can enable
STATE_HARM = 2 * sum(o for _, o in STATE_SEASONS)   # 14: daily A_1..4, B_1..4, weekly A_1..3, B_1..3


def state_rotation(T: int, m: int, n_changepoints: int = 10, cp_range: float = 0.8, phase: float = 0.0):
    """fp64 constants of :func:`window_state` for a (T, m) geometry: ``one_minus_c
    [n_changepoints]``, and per harmonic (4 daily, 3 weekly) ``cos th`` / ``sin th`` ``[7]``
    and whether its season is enabled ``[7]`` (bool)."""
    if not cp_range < 1.0:
        raise ValueError(f"cp_range {cp_range}: the forecast state needs every changepoint inside the window "
                         "(cp_range < 1)")
    if T < 2 or m < 2:
        raise ValueError("the forecast state needs T >= 2 and m >= 2")
    dt = torch.float64
    cps = torch.arange(1, n_changepoints + 1, dtype=dt) / (n_changepoints + 1) * cp_range
    enabled = {int(round(p)) for p, _ in window_seasons(T, m)}
    cos, sin, on = [], [], []
    for days, order in STATE_SEASONS:
        p = days * m
        for k in range(1, order + 1):
            # th = 2 pi k (T - 1 + phase) / p, reduced before the multiplication by 2 pi
            frac = math.fmod(k * (float(T - 1) + phase), float(p)) / float(p)
            cos.append(math.cos(2 * math.pi * frac))
            sin.append(math.sin(2 * math.pi * frac))
            on.append(p in enabled)
    return 1.0 - cps, torch.tensor(cos, dtype=dt), torch.tensor(sin, dtype=dt), torch.tensor(on)


def state_from_beta(beta: torch.Tensor, T: int, m: int, n_changepoints: int = 10, cp_range: float = 0.8,
                    phase: float = 0.0):
    """``beta [N, P]`` of a window-scaled fit → ``level [N]``, ``slope [N]``, ``harm [N, 14]``
    in fp64 (``harm``: daily ``A_1..4, B_1..4`` then weekly ``A_1..3, B_1..3``; zeros for a
    season the window does not enable)."""
    omc, cos, sin, on = state_rotation(T, m, n_changepoints, cp_range, phase)
    b = beta.to(torch.float64)
    dev = b.device
    omc, cos, sin = omc.to(dev), cos.to(dev), sin.to(dev)
    K = n_changepoints
    delta = b[:, 2:2 + K]
    level = b[:, 0] + b[:, 1] + (delta * omc[None, :]).sum(1)
    slope = (b[:, 1] + delta.sum(1)) / float(T - 1)
    harm = torch.zeros((b.shape[0], STATE_HARM), dtype=torch.float64, device=dev)
    src, dst, j = 2 + K, 0, 0
    for _days, order in STATE_SEASONS:
        if bool(on[j]):
            a_s, a_c = b[:, src:src + order], b[:, src + order:src + 2 * order]
            c, s = cos[None, j:j + order], sin[None, j:j + order]
            harm[:, dst:dst + order] = a_s * c - a_c * s
            harm[:, dst + order:dst + 2 * order] = a_s * s + a_c * c
            src += 2 * order
        dst += 2 * order
        j += order
    return level, slope, harm


def window_state(fit: ProphetWindowFit):
    """Forecast state of a window-scaled fit: ``level [N]``, ``slope [N]`` (per sample),
    ``harm [N, 14]`` in fp64.  ``forecast_state`` on it equals ``forecast_window(fit, h)``
    for every ``h >= 0``.  Raises when ``fit.cp_range >= 1`` (a hinge would start past the
    window and the trend would not be a line there)."""
    return state_from_beta(fit.beta, fit.T, fit.m, fit.n_changepoints, fit.cp_range, fit.phase)


def forecast_state(level: torch.Tensor, slope: torch.Tensor, harm: torch.Tensor, m: int,
                   horizons: torch.Tensor) -> torch.Tensor:
    """``level + slope h + sum_j [A_j sin(w_j h) + B_j cos(w_j h)]`` for ``horizons [C]`` or
    ``[N, C]`` → ``[N, C]``, evaluated in fp64 and returned in ``level``'s dtype.  Integer
    horizons have their phase reduced in integers (``(k h) mod p``), so the result does not
    lose accuracy as ``h`` grows."""
    dt = torch.float64
    dev = level.device
    h = horizons.to(dev)
    if h.dim() == 1:
        h = h[None, :]
    exact = not (h.is_floating_point() or h.is_complex())
    hf = h.to(dt)
    out = level.to(dt)[:, None] + slope.to(dt)[:, None] * hf
    hm = harm.to(dt)
    dst = 0
    for days, order in STATE_SEASONS:
        p = days * int(m)
        for k in range(1, order + 1):
            if exact:
                ang = (2 * math.pi / p) * torch.remainder(h.long() * k, p).to(dt)
            else:
                ang = (2 * math.pi * k / p) * hf
            out = out + hm[:, dst + k - 1, None] * torch.sin(ang) + hm[:, dst + order + k - 1, None] * torch.cos(ang)
        dst += 2 * order
    return out.to(level.dtype)
