"""Bivariate normal scorer (two metrics; ``docs/guides/design.md:78``).

Per series pair (e.g. latency and error rate of one app): fit the 2-D mean
and covariance on the historical window, score current points by squared
Mahalanobis distance ``d²``.  A point is anomalous when ``d² > thr²``
(``thr`` in sigma units, the same ``threshold`` env as the univariate
models).  Reference semantics for the ``bivariate`` kernel (K8).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class BivariateFit:
    mean: torch.Tensor   # [N, 2]
    cov: torch.Tensor    # [N, 3] (sxx, sxy, syy)
    count: torch.Tensor  # [N]


def fit_bivariate(h: torch.Tensor) -> BivariateFit:
    """``h``: ``[N, T, 2]``; a time point is used only if both coordinates are valid.

    The mean and the centred moments are accumulated in float64 whatever the input
    type (an fp32 sum of T values at level L loses ~T ulp(L) of the mean, and the
    centred moments inherit it); the fit is returned in the promoted type of the
    input: float32 for fp32 / bf16 windows, float64 for fp64 windows."""
    dt = torch.promote_types(h.dtype, torch.float32)
    h = h.double()
    valid = ~torch.isnan(h).any(2)
    n = valid.sum(1).double()
    nn = n.clamp(min=1)
    z = torch.where(valid[..., None], h, torch.zeros_like(h))
    mean = z.sum(1) / nn[:, None]
    d = torch.where(valid[..., None], h - mean[:, None, :], torch.zeros_like(h))
    sxx = (d[..., 0] * d[..., 0]).sum(1) / nn
    sxy = (d[..., 0] * d[..., 1]).sum(1) / nn
    syy = (d[..., 1] * d[..., 1]).sum(1) / nn
    return BivariateFit(mean=mean.to(dt), cov=torch.stack([sxx, sxy, syy], 1).to(dt), count=n.to(dt))


def mahalanobis2(fit: BivariateFit, x: torch.Tensor, eps: float = 1e-9) -> torch.Tensor:
    """``x``: ``[N, C, 2]`` -> ``d2 [N, C]`` (NaN where x is missing), in the promoted type
    of the fit and ``x`` (at least float32)."""
    dt = torch.promote_types(torch.promote_types(fit.mean.dtype, fit.cov.dtype),
                             torch.promote_types(x.dtype, torch.float32))
    x = x.to(dt)
    mean, cov = fit.mean.to(dt), fit.cov.to(dt)
    sxx, sxy, syy = cov[:, 0] + eps, cov[:, 1], cov[:, 2] + eps
    det = sxx * syy - sxy * sxy
    det = torch.where(det.abs() < 1e-20, torch.full_like(det, 1e-20), det)
    dx = x[..., 0] - mean[:, None, 0]
    dy = x[..., 1] - mean[:, None, 1]
    return (syy[:, None] * dx * dx - 2 * sxy[:, None] * dx * dy + sxx[:, None] * dy * dy) / det[:, None]
