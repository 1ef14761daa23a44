"""Multivariate normal scorer (k metrics, 2 <= k <= 8): the closed-form generalisation
of ``models/bivariate.py``.

Per group of k series (the metrics of one job): fit the k-D mean and covariance on the
jointly valid points of the historical window, score current points by squared
Mahalanobis distance ``d²`` through the Cholesky factor of ``Σ + eps·I``.  A point is
anomalous when ``d² > q_k(thr)``, the χ²_k quantile whose upper tail equals the two-sided
normal tail of ``thr`` (``chi2_threshold``): the bivariate rule ``d² > thr²`` widened to k
metrics would fire on a third of all points at k = 8.  ``d²`` splits exactly into one
contribution per metric (``contributions``), which names the metrics behind a verdict.
Reference semantics for the ``mvn_groups`` kernel (``ops/csrc/mvn_groups.hip``).
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Tuple

import torch

MAX_K = 8
PIVOT_FLOOR = 1e-20


@dataclass
class MvnFit:
    mean: torch.Tensor   # [G, k]
    cov: torch.Tensor    # [G, k (k + 1) / 2] packed lower triangle, row-major
    count: torch.Tensor  # [G]

    @property
    def k(self) -> int:
        return self.mean.shape[1]


def tri_index(i: int, j: int) -> int:
    """Position of ``Σ[i, j]`` (i >= j) in the packed lower triangle."""
    return i * (i + 1) // 2 + j


def fit_mvn(h: torch.Tensor) -> MvnFit:
    """``h``: ``[G, T, k]``; a time point is used only if all k coordinates are valid.

    The mean and the biased covariance are accumulated in float64 whatever the input type
    and returned in the promoted type of the input, as ``fit_bivariate`` does."""
    k = h.shape[2]
    if not 2 <= k <= MAX_K:
        raise ValueError(f"fit_mvn takes 2..{MAX_K} metrics, got {k}")
    dt = torch.promote_types(h.dtype, torch.float32)
    h = h.double()
    valid = ~torch.isnan(h).any(2)
    n = valid.sum(1).double()
    nn = n.clamp(min=1)
    z = torch.where(valid[..., None], h, torch.zeros_like(h))
    mean = z.sum(1) / nn[:, None]
    d = torch.where(valid[..., None], h - mean[:, None, :], torch.zeros_like(h))
    cov = [(d[..., i] * d[..., j]).sum(1) / nn for i in range(k) for j in range(i + 1)]
    return MvnFit(mean=mean.to(dt), cov=torch.stack(cov, 1).to(dt), count=n.to(dt))


def _promoted(fit: MvnFit, x: torch.Tensor) -> torch.dtype:
    return torch.promote_types(torch.promote_types(fit.mean.dtype, fit.cov.dtype),
                               torch.promote_types(x.dtype, torch.float32))


def cholesky_packed(cov: torch.Tensor, k: int, eps: float) -> Tuple[list, list]:
    """Cholesky factor of ``Σ + eps·I`` from the packed covariance ``[G, k (k + 1) / 2]``:
    ``L[i][j]`` (j < i) and the reciprocal diagonal, as lists of ``[G]`` tensors.  A pivot
    below ``PIVOT_FLOOR`` is replaced by it (the determinant floor of the bivariate code)."""
    L = [[None] * k for _ in range(k)]
    inv = [None] * k
    for j in range(k):
        for i in range(j, k):
            s = cov[:, tri_index(i, j)]
            if i == j:
                s = s + eps
            for m in range(j):
                s = s - L[i][m] * L[j][m]
            if i == j:
                s = torch.where(s < PIVOT_FLOOR, torch.full_like(s, PIVOT_FLOOR), s)
                L[j][j] = s.sqrt()
                inv[j] = 1.0 / L[j][j]
            else:
                L[i][j] = s * inv[j]
    return L, inv


def _solve_factor(mean: torch.Tensor, L: list, inv: list, x: torch.Tensor, want_contrib: bool):
    """The two triangular solves of a point block ``x [G, C, k]`` against the factor
    (``L[i][j]``, ``inv[i] = 1 / L[i][i]``, lists of ``[G]`` tensors): ``d2 [G, C]`` and, when
    wanted, the contributions ``[G, C, k]``; NaN where a coordinate is missing."""
    k = x.shape[2]
    d = [x[..., i] - mean[:, None, i] for i in range(k)]
    z = []
    for i in range(k):   # z = L^-1 (x - mean)
        s = d[i]
        for m in range(i):
            s = s - L[i][m][:, None] * z[m]
        z.append(s * inv[i][:, None])
    d2 = z[0] * z[0]
    for i in range(1, k):
        d2 = d2 + z[i] * z[i]
    missing = torch.isnan(x).any(2)
    d2 = torch.where(missing, torch.full_like(d2, float("nan")), d2)
    if not want_contrib:
        return d2, None
    w = [None] * k
    for i in reversed(range(k)):   # w = L^-T z = Σ_reg^-1 (x - mean)
        s = z[i]
        for m in range(i + 1, k):
            s = s - L[m][i][:, None] * w[m]
        w[i] = s * inv[i][:, None]
    c = torch.stack([d[i] * w[i] for i in range(k)], 2)
    return d2, torch.where(missing[..., None], torch.full_like(c, float("nan")), c)


def _solve(fit: MvnFit, x: torch.Tensor, eps: float, want_contrib: bool):
    dt = _promoted(fit, x)
    x = x.to(dt)
    mean, cov = fit.mean.to(dt), fit.cov.to(dt)
    L, inv = cholesky_packed(cov, fit.k, eps)
    return _solve_factor(mean, L, inv, x, want_contrib)


def mahalanobis2_mvn(fit: MvnFit, x: torch.Tensor, eps: float = 1e-9) -> torch.Tensor:
    """``x``: ``[G, C, k]`` -> ``d2 [G, C]`` (NaN where any coordinate of the point is
    missing), in the promoted type of the fit and ``x`` (at least float32)."""
    return _solve(fit, x, eps, False)[0]


def contributions(fit: MvnFit, x: torch.Tensor, eps: float = 1e-9) -> torch.Tensor:
    """``[G, C, k]``: ``c_i = (x − μ)_i · (Σ_reg⁻¹ (x − μ))_i``.  They sum to ``d²`` and a
    metric's share does not depend on the order of the metrics."""
    return _solve(fit, x, eps, True)[1]


@functools.lru_cache(maxsize=None)
def chi2_threshold(thr: float, k: int) -> float:
    """``q_k(thr)``: ``P(χ²_k > q) = erfc(thr / √2)``, by bisection on the regularised upper
    incomplete gamma function in float64 (``q_1(thr) = thr²``)."""
    thr, k = float(thr), int(k)
    if k < 1:
        raise ValueError("chi2_threshold needs k >= 1")
    if not thr > 0:
        return 0.0
    p = math.erfc(thr / math.sqrt(2.0))
    a = torch.tensor(0.5 * k, dtype=torch.float64)

    def sf(q: float) -> float:
        return float(torch.special.gammaincc(a, torch.tensor(0.5 * q, dtype=torch.float64)))

    lo, hi = 0.0, thr * thr + 4.0 * k + 16.0
    while sf(hi) > p:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):   # far past float64 resolution: the interval stops halving first
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if sf(mid) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def named(c: torch.Tensor, d2: torch.Tensor) -> torch.Tensor:
    """Attribution rule on ``c [..., k]`` / ``d2 [...]``: metric i is named iff
    ``c_i >= d²/k``; the largest ``c_i`` is always named (ties: the first).  Bool
    ``[..., k]``, False where the point is missing."""
    k = c.shape[-1]
    ok = ~torch.isnan(d2)
    cz = torch.where(ok[..., None], c, torch.zeros_like(c))
    out = cz >= (torch.where(ok, d2, torch.zeros_like(d2)) / k)[..., None]
    top = torch.zeros_like(out)
    top.scatter_(-1, cz.argmax(-1, keepdim=True), True)
    return (out | top) & ok[..., None]


@dataclass
class MvnScore:
    d2: torch.Tensor       # [G, C]
    contrib: torch.Tensor  # [G, C, k]
    flag: torch.Tensor     # [G, C] bool: anomalous slots
    names: torch.Tensor    # [G, C, k] bool: metrics named on the anomalous slots
    count: torch.Tensor    # [G] int32
    verdict: torch.Tensor  # [G] int8: 1 anomalous, 0 healthy, -1 unscored
    blame: torch.Tensor    # [G] int32 bit mask of the named metrics


def _verdict(d2, c, count, thr2, min_valid: int) -> MvnScore:
    k = c.shape[2]
    ok = count >= min_valid
    valid = ~torch.isnan(d2)
    flag = valid & ok[:, None] & (d2 > thr2.to(d2.dtype)[:, None])
    names = named(c, d2) & flag[..., None]
    n = flag.sum(1).int()
    verdict = torch.where(n > 0, 1, torch.where(valid.any(1) & ok, 0, -1)).to(torch.int8)
    bits = (1 << torch.arange(k)).int().to(d2.device)
    blame = (names.any(1).int() * bits).sum(1).int()
    return MvnScore(d2=d2, contrib=c, flag=flag, names=names, count=n, verdict=verdict, blame=blame)


def score_mvn(fit: MvnFit, x: torch.Tensor, thr2: torch.Tensor, min_valid: int, eps: float = 1e-9) -> MvnScore:
    """The verdict and attribution rules: a slot is anomalous iff the model is ok (jointly
    valid points >= ``min_valid``) and ``d² > thr2`` (``thr2 [G]`` = ``q_k(thr)``)."""
    d2, c = _solve(fit, x, eps, True)
    return _verdict(d2, c, fit.count, thr2, min_valid)


STATE_TRI = MAX_K * (MAX_K + 1) // 2   # 36: a state row holds the packed factor of an 8 x 8 matrix


def mvn_state(fit: MvnFit, eps: float = 1e-9) -> torch.Tensor:
    """The scoring state of a fit: ``chol [G, 36]`` packed like ``cov``.  Entries below the
    diagonal hold ``L[i][j]``, diagonal slots hold ``1 / L[i][i]`` (``L Lᵀ = Σ + eps·I``, the
    factor and pivot floor of ``cholesky_packed``), unused entries are 0.  With ``mean`` and
    ``count`` it is all ``score_state`` needs: the fit is made once, the state scored every
    tick (``ops/csrc/mvn_state.hip``)."""
    k = fit.k
    dt = torch.promote_types(torch.promote_types(fit.mean.dtype, fit.cov.dtype), torch.float32)
    L, inv = cholesky_packed(fit.cov.to(dt), k, eps)
    chol = torch.zeros((fit.cov.shape[0], STATE_TRI), dtype=dt, device=fit.cov.device)
    for i in range(k):
        for j in range(i):
            chol[:, tri_index(i, j)] = L[i][j]
        chol[:, tri_index(i, i)] = inv[i]
    return chol


def score_state(mean: torch.Tensor, chol: torch.Tensor, count: torch.Tensor, x: torch.Tensor, thr2: torch.Tensor,
                min_valid: int) -> MvnScore:
    """``score_mvn`` from the state: ``mean [G, >= k]``, ``chol [G, 36]`` (``mvn_state``),
    ``count [G]`` and the points ``x [G, C, k]``.  The same solves, ``named`` rule, verdict and
    blame; only the factorisation is not repeated."""
    k = x.shape[2]
    if not 2 <= k <= MAX_K:
        raise ValueError(f"score_state takes 2..{MAX_K} metrics, got {k}")
    dt = torch.promote_types(torch.promote_types(mean.dtype, chol.dtype), torch.promote_types(x.dtype, torch.float32))
    mean, chol, x = mean.to(dt), chol.to(dt), x.to(dt)
    L = [[chol[:, tri_index(i, j)] if j < i else None for j in range(k)] for i in range(k)]
    inv = [chol[:, tri_index(i, i)] for i in range(k)]
    d2, c = _solve_factor(mean, L, inv, x, True)
    return _verdict(d2, c, count, thr2, min_valid)
