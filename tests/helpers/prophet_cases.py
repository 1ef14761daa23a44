"""Shared inputs of the window-scaled prophet tests (tests/test_prophet_window.py,
tests/test_prophet_gpu.py): synthetic rings with the gap patterns the kernel has a path
for, and an fp32 emulation of the kernel's arithmetic on the CPU."""

from __future__ import annotations

import math

import numpy as np
import torch

from foremast_amd.models import prophet_lite as pl

PATTERNS = ("dense", "miss1", "outage20", "lead_third", "trail7", "miss60", "exact_p", "below_min", "all_nan")
LEVELS = (1e-2, 1e-1, 1.0, 10.0, 1e2, 1e3, 1e4, 1e5)


def n_terms(T: int, m: int) -> int:
    return 12 + sum(2 * o for _, o in pl.window_seasons(T, m))


def min_valid_of(T: int) -> int:
    """``min_valid`` of the cases: an eighth of the window (a row of the ``below_min``
    pattern has one sample fewer, still far more than the model has terms)."""
    return T // 8


def make_rows(T: int, m: int, N: int, seed: int, bf16: bool, patterns=PATTERNS):
    """``[N, T]`` float32 series (bf16-representable values with ``bf16``), NaN = missing;
    row ``i`` has pattern ``patterns[i % len(patterns)]`` and a level from ``LEVELS``."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)
    P = n_terms(T, m)
    y = torch.empty((N, T), dtype=torch.float64)
    pat = []
    for i in range(N):
        lvl = LEVELS[(i // len(patterns) + i) % len(LEVELS)]
        ph = torch.rand(2, generator=g, dtype=torch.float64) * 2 * math.pi
        s = (1.0 + 0.2 * torch.sin(2 * math.pi * t / m + ph[0]) + 0.05 * torch.sin(2 * math.pi * t / (7 * m) + ph[1])
             + 0.1 * t / T + 0.03 * torch.randn(T, generator=g, dtype=torch.float64))
        row = lvl * s
        p = patterns[i % len(patterns)]
        pat.append(p)
        nan = torch.zeros(T, dtype=torch.bool)
        if p == "miss1":
            nan = torch.rand(T, generator=g) < 0.01
            nan[0] = nan[-1] = False
        elif p == "outage20":
            a = int(torch.randint(1, T - T // 5 - 1, (1,), generator=g))
            nan[a:a + T // 5] = True
        elif p == "lead_third":
            nan[:T // 3] = True
        elif p == "trail7":
            nan[T - 7:] = True
        elif p == "miss60":
            nan = torch.rand(T, generator=g) < 0.6
        elif p == "exact_p":
            keep = torch.linspace(0, T - 1, P).round().long()
            nan[:] = True
            nan[keep] = False
        elif p == "below_min":
            keep = torch.randperm(T, generator=g)[:min_valid_of(T) - 1]
            nan[:] = True
            nan[keep] = False
        elif p == "all_nan":
            nan[:] = True
        row = torch.where(nan, torch.full_like(row, float("nan")), row)
        y[i] = row
    y = y.float()
    if bf16:
        y = y.bfloat16().float()
    return y, pat


def to_ring(y: torch.Tensor, ring_len: int, head: int, dtype, device, fill: float = 12345.0) -> torch.Tensor:
    """Physical ring ``[N, ring_len]`` (a view of a 16-byte-aligned store) holding the
    logical window ``y`` from column ``head``; the columns outside the window hold ``fill``
    (finite garbage the scorer must not read)."""
    N, T = y.shape
    per16 = 8 if dtype == torch.bfloat16 else 4
    ld = (ring_len + per16 - 1) // per16 * per16
    store = torch.full((N, ld), fill, dtype=dtype)
    cols = (head + torch.arange(T)) % ring_len
    store[:, cols] = y.to(dtype)
    return store.to(device)[:, :ring_len]


def emulate_fp32(y: torch.Tensor, m: int, horizons: torch.Tensor, downdate=None):
    """The kernel's arithmetic on the CPU: fp32 tables, sequential fp32 accumulation of the
    rhs and of the normal matrix (``downdate``: from ``A_dense`` by the missing samples;
    False: ``reg`` + the valid samples; None: whichever side is smaller, as the kernel
    chooses), fp32 Cholesky and solves, a second fp32 pass for the residuals.  Returns
    (forecast ``[N, C]``, sigma ``[N]``, beta ``[N, P]``, Cholesky failures)."""
    N, T = y.shape
    hmax = int(horizons.max())
    X64, XH64, reg64, A64 = pl.design_window(T, m, hmax)
    X, XH, reg, A = (v.numpy().astype(np.float32) for v in (X64, XH64, reg64, A64))
    P = X.shape[1]
    yv = y.numpy().astype(np.float32)
    ok = ~np.isnan(yv)
    y0 = np.where(ok, yv, np.float32(0))
    rhs = np.zeros((N, P), np.float32)
    for t in range(T):
        rhs += X[t][None, :] * y0[:, t:t + 1]
    fc = np.zeros((N, horizons.shape[-1]), np.float32)
    sig = np.zeros(N, np.float32)
    beta = np.zeros((N, P), np.float32)
    fails = 0
    hz = horizons.numpy()
    for i in range(N):
        n = int(ok[i].sum())
        down = (2 * n >= T) if downdate is None else downdate
        acc = np.zeros((P, P), np.float32)
        for t in np.nonzero(~ok[i] if down else ok[i])[0]:
            acc += np.outer(X[t], X[t])
        An = (A - acc) if down else (np.diag(reg) + acc)
        try:
            L = np.linalg.cholesky(An)
        except np.linalg.LinAlgError:
            fails += 1
            continue
        z = np.zeros(P, np.float32)
        for k in range(P):
            z[k] = (rhs[i, k] - np.dot(L[k, :k], z[:k])) / L[k, k]
        b = np.zeros(P, np.float32)
        for k in range(P - 1, -1, -1):
            b[k] = (z[k] - np.dot(L[k + 1:, k], b[k + 1:])) / L[k, k]
        r = np.where(ok[i], yv[i] - X @ b, np.float32(0)).astype(np.float32)
        ss = np.cumsum(r * r, dtype=np.float32)[-1]
        sig[i] = np.sqrt(ss / np.float32(max(n - P, 1)))
        beta[i] = b
        h = hz if hz.ndim == 1 else hz[i]
        fc[i] = XH[h - 1] @ b
    return torch.from_numpy(fc), torch.from_numpy(sig), torch.from_numpy(beta), fails
