"""Median / MAD band (``ML_ALGORITHM=robust_average_all`` / ``robust_average``).

Reference semantics for the ``robust_stats`` kernel (``ops/csrc/robust.hip``).
The moving-average pair estimates its spread by least squares, so an earlier
incident that still sits in the history widens the band; here both the centre
and the spread are order statistics, which up to half of the samples cannot move
far.  Over the ``n`` non-NaN samples of the window:

* ``center`` — the lower median: the order statistic of 0-based rank
  ``(n - 1) // 2`` (``torch.nanmedian``).  The two middle values are never
  averaged, so the centre is always a sample and the kernel matches it bit for bit;
* ``mad`` — the lower median of ``|y - center|`` (each difference in fp32) over the
  same samples;
* ``sigma`` — ``1.4826 * mad`` (the normal-consistent scale) when ``mad > 0``,
  otherwise the population standard deviation of the window
  (:func:`~.moving_average.window_stats`): a metric that is zero more than half of
  the time (``error5xx``) has ``mad == 0`` and would get a zero-width band;
* ``count`` — ``n``; with ``n == 0`` centre and sigma are NaN.

The forecast is ``center`` at every horizon with no horizon factor; band and
verdict are :mod:`foremast_amd.models.detect` unchanged.

* ``robust_average_all`` — statistics over the whole history;
* ``robust_average``     — statistics over the last ``window`` positions.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import moving_average as ma_ref

MAD_SCALE = 1.4826  # 1 / Phi^-1(3/4): MAD -> sigma of a normal sample


@dataclass
class RobustStats:
    center: torch.Tensor  # [N] lower median
    sigma: torch.Tensor   # [N] the band's spread
    mad: torch.Tensor     # [N] lower median of |y - center| (0: sigma is std)
    std: torch.Tensor     # [N] population standard deviation
    count: torch.Tensor   # [N]


def robust_stats(y: torch.Tensor, window: Optional[int] = None) -> RobustStats:
    y = y.float()
    if window is not None and window < y.shape[1]:
        y = y[:, -window:]
    if y.shape[1] == 0:
        nan = torch.full((y.shape[0],), float("nan"), device=y.device)
        return RobustStats(center=nan, sigma=nan.clone(), mad=nan.clone(), std=nan.clone(),
                           count=torch.zeros_like(nan))
    ws = ma_ref.window_stats(y)
    center = torch.nanmedian(y, dim=1).values
    mad = torch.nanmedian((y - center[:, None]).abs(), dim=1).values
    sigma = torch.where(mad > 0, torch.tensor(MAD_SCALE, dtype=torch.float32, device=y.device) * mad, ws.std)
    return RobustStats(center=center, sigma=sigma, mad=mad, std=ws.std, count=ws.count)
