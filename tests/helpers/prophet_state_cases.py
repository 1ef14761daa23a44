"""Shared inputs of the prophet forecast-state tests (tests/test_prophet_state_gpu.py): the
cases' rings, horizons and fp64 reference, and an fp32 emulation of the state kernels on
the CPU (``prophet_cases.emulate_fp32``'s beta reduced to the state and evaluated in fp32
arithmetic, with the phase reduced in integers as the kernel does)."""

from __future__ import annotations

import importlib.util
import math
import os

import numpy as np
import torch

from foremast_amd.models import prophet_lite as pl

_spec = importlib.util.spec_from_file_location(
    "prophet_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "prophet_cases.py"))
pc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pc)

HZ_MAX = 1 << 20


def horizon_set(m: int, far: bool = True):
    """The CPU test's horizons, plus the kernel's largest with ``far``."""
    hs = [1, 2, 16, 17, 64, 65, m - 1, m, m + 1, 7 * m, 7 * m + 1, 10 ** 5]
    return sorted(set(hs + ([HZ_MAX] if far else [])))


def draw_horizons(m: int, N: int, C: int, seed: int, hmax: int = HZ_MAX) -> torch.Tensor:
    """Per-row horizons ``[N, C]`` int32 drawn from :func:`horizon_set` (values <= ``hmax``);
    the first columns of row 0 walk the whole set so that every value appears."""
    hs = torch.tensor([h for h in horizon_set(m) if h <= hmax], dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    hz = hs[torch.randint(0, len(hs), (N, C), generator=g)]
    flat = hz.view(-1)
    k = min(len(hs), flat.numel())
    flat[:k] = hs[:k]
    return hz.contiguous()


def emulate_state_fp32(y: torch.Tensor, m: int, horizons: torch.Tensor):
    """fp32 emulation of ``prophet_fit_state`` + the state kernel's forecast: the beta of
    ``prophet_cases.emulate_fp32`` reduced to (level, slope, harm) with fp32 tables and
    sequential fp32 arithmetic, then ``level + slope h + sum [A sin + B cos]`` in fp32 with
    sin / cos of the exactly reduced phase rounded to fp32.  Returns (forecast ``[N, C]``,
    sigma ``[N]``, (level, slope, harm))."""
    N, T = y.shape
    _, sig, beta, _ = pc.emulate_fp32(y, m, torch.tensor([1]))
    f32 = np.float32
    b = beta.numpy().astype(f32)
    omc, cos, sin, on = pl.state_rotation(T, m)
    omc, cos, sin = (v.numpy().astype(f32) for v in (omc, cos, sin))
    K = len(omc)
    level = (b[:, 0] + b[:, 1]).astype(f32)
    ds = b[:, 1].copy()
    for k in range(K):
        level = (level + b[:, 2 + k] * omc[k]).astype(f32)
        ds = (ds + b[:, 2 + k]).astype(f32)
    slope = (ds * f32(1.0 / (T - 1))).astype(f32)
    harm = np.zeros((N, pl.STATE_HARM), f32)
    src, dst, j = 2 + K, 0, 0
    for _days, order in pl.STATE_SEASONS:
        if bool(on[j]):
            a_s, a_c = b[:, src:src + order], b[:, src + order:src + 2 * order]
            c, s = cos[None, j:j + order], sin[None, j:j + order]
            harm[:, dst:dst + order] = (a_s * c - a_c * s).astype(f32)
            harm[:, dst + order:dst + 2 * order] = (a_s * s + a_c * c).astype(f32)
            src += 2 * order
        dst += 2 * order
        j += order
    hz = horizons.numpy().astype(np.int64)
    hz = np.broadcast_to(hz if hz.ndim == 2 else hz[None, :], (N, hz.shape[-1]))
    fc = (level[:, None] + slope[:, None] * hz.astype(f32)).astype(f32)
    dst = 0
    for days, order in pl.STATE_SEASONS:
        p = days * m
        for k in range(1, order + 1):
            ang = 2 * math.pi * ((hz * k) % p).astype(np.float64) / p
            fc = (fc + harm[:, dst + k - 1, None] * np.sin(ang).astype(f32)).astype(f32)
            fc = (fc + harm[:, dst + order + k - 1, None] * np.cos(ang).astype(f32)).astype(f32)
        dst += 2 * order
    return torch.from_numpy(fc.copy()), sig, (torch.from_numpy(level), torch.from_numpy(slope),
                                              torch.from_numpy(harm))
