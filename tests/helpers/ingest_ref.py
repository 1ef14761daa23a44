"""Host model of the ring and window ingest kernels (ops/csrc/ingest.hip, the ring append
of ops/csrc/window.hip), written from their documented semantics in plain numpy: float64
accumulation, int64 integers, explicit loops where the definition is a loop.

Arrays go in as numpy arrays or CPU torch tensors and are never modified; float32 numpy
arrays come out.  A history ring is the one exception: numpy has no bf16, so a ring passed
as a torch tensor comes back as a torch tensor of the same dtype, and a value written to a
bf16 ring is ``torch.from_numpy(x).to(torch.bfloat16)`` (round to nearest even, NaN stays
NaN)."""

import numpy as np
import torch


def _f32(a):
    """A fresh float32 numpy copy of a numpy array or a CPU tensor (bf16 widens exactly)."""
    if isinstance(a, torch.Tensor):
        return a.detach().float().contiguous().numpy().copy()
    return np.array(a, dtype=np.float32, copy=True)


def _i64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().to(torch.int64).contiguous().numpy().copy()
    return np.array(a, dtype=np.int64, copy=True)


def _is_bf16(ring) -> bool:
    return isinstance(ring, torch.Tensor) and ring.dtype == torch.bfloat16


def stored(x: np.ndarray, bf16: bool) -> np.ndarray:
    """float32 values as a ring of the given dtype keeps them (as float32, exact)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not bf16:
        return x.copy()
    return torch.from_numpy(x.copy()).to(torch.bfloat16).float().numpy()


def _ring_out(like, a: np.ndarray):
    if isinstance(like, torch.Tensor):
        return torch.from_numpy(a).to(like.dtype)  # exact: every value is representable already
    return a


# ---------------------------------------------------------------------------------
# test data shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------
def window_values(rng, shape, exact: bool) -> np.ndarray:
    """``exact``: 12*k with integer k in [-20, 20], so the mean of any 1..4 of them is an
    integer of magnitude <= 240 (exact in float32 and in bf16); else normals scaled by 1e3."""
    if exact:
        return (12 * rng.integers(-20, 21, size=shape)).astype(np.float32)
    return (1e3 * rng.standard_normal(shape)).astype(np.float32)


def punch_slot(cur: np.ndarray, base: np.ndarray, P: int, W: int, slot: int) -> None:
    """NaN holes in the slot about to be evicted, by row number mod 7: none; one pod in both
    windows; two pods in both; every pod in both; every pod of ``cur`` only; every pod of
    ``base`` only; one pod of ``base`` only.  One more hole outside the slot on every third
    row (it must survive the tick)."""
    nan = np.float32("nan")
    for n in range(cur.shape[0]):
        q, p1 = n % 7, n % P
        col = lambda p: (p % P) * W + slot  # noqa: E731
        if q == 1:
            cur[n, col(p1)] = base[n, col(p1)] = nan
        elif q == 2:
            for p in (p1, p1 + 1):
                cur[n, col(p)] = base[n, col(p)] = nan
        elif q == 3:
            for p in range(P):
                cur[n, col(p)] = base[n, col(p)] = nan
        elif q == 4:
            for p in range(P):
                cur[n, col(p)] = nan
        elif q == 5:
            for p in range(P):
                base[n, col(p)] = nan
        elif q == 6:
            base[n, col(p1)] = nan
        if n % 3 == 0 and W > 1:
            cur[n, p1 * W + (slot + 1) % W] = nan


def new_values(rng, N: int, P: int, exact: bool) -> np.ndarray:
    """``[N, P]`` values of a tick, about one in eight NaN."""
    v = window_values(rng, (N, P), exact)
    v[rng.random((N, P)) < 0.125] = np.float32("nan")
    return v


def ring_append_ref(dst, col0, src, col_dev=None):
    """``dst[n, (col0 + col_dev + j) % R] = src[n, j]`` for every row n and j < S."""
    out = _f32(dst)
    v = stored(_f32(src), _is_bf16(dst))
    N, R = out.shape
    S = v.shape[1]
    assert v.shape[0] == N and S <= R
    first = int(col0) + (0 if col_dev is None else int(_i64(col_dev).reshape(-1)[0]))
    for j in range(S):
        out[:, (first + j) % R] = v[:, j]
    return _ring_out(dst, out)


def tick_ingest_ref(hist, hist_col, cur, P, W, slot, newv, graduate, base=None, newb=None):
    """One streaming tick.  The slot being overwritten holds the oldest points; the mean of
    its non-NaN pods graduates into ``hist[:, hist_col]`` (the baseline window's slot when a
    baseline streams, else the current window's; NaN when no pod has a value), then the new
    per-pod values take the slot, NaN included.  Returns ``(hist, cur, base, mean)`` with
    ``mean`` the float64 graduating mean per row (computed whether or not it graduates)."""
    h = _f32(hist)
    c = _f32(cur)
    b = None if base is None else _f32(base)
    nv = _f32(newv)
    N = c.shape[0]
    assert c.shape == (N, P * W) and nv.shape == (N, P) and 0 <= slot < W and 0 <= hist_col < h.shape[1]
    cols = [p * W + slot for p in range(P)]
    evicted = (b if b is not None else c)[:, cols].astype(np.float64)
    mean = np.full(N, np.nan, dtype=np.float64)
    for n in range(N):
        ok = ~np.isnan(evicted[n])
        if ok.any():
            mean[n] = evicted[n][ok].sum() / int(ok.sum())
    if b is not None:
        nb = _f32(newb)
        assert b.shape == c.shape and nb.shape == nv.shape
        b[:, cols] = nb
    c[:, cols] = nv
    if graduate:
        h[:, hist_col] = stored(mean.astype(np.float32), _is_bf16(hist))
    return _ring_out(hist, h), c, b, mean


def tick_advance_ref(state, R, W, h_table=None):
    """One steady-state tick of the record ``{hist_col, slot, graduate, head}`` of a full
    ring: the graduating point overwrites the oldest column (at ``head``), ``head`` moves on
    by one, the window slot cycles mod W.  Returns the new record and the horizon row in
    force after the tick, row ``(new slot + 1) % W`` of ``h_table`` (None without one)."""
    if isinstance(state, dict):
        head, slot = int(state["head"]), int(state["slot"])
    else:
        s = _i64(state).reshape(-1)
        head, slot = int(s[3]), int(s[1])
    new_slot = (slot + 1) % W
    rec = {"hist_col": head, "slot": new_slot, "graduate": 1, "head": (head + 1) % R}
    row = None
    if h_table is not None:
        row = _i64(h_table)[(new_slot + 1) % W].copy()
    return rec, row


def rollout_scatter_ref(win, P, Wc, src, col0, srcmap=None):
    """``win[n, p*Wc + col0[n] + j] = src[srcmap[n*P + p], j]`` (``srcmap`` None: source row
    ``n*P + p``).  A point is dropped when its column is outside ``[0, Wc)``, when its pod
    maps to no source row (``< 0`` or ``>= S``) or when its value is NaN."""
    out = _f32(win)
    s = _f32(src)
    c0 = _i64(col0)
    sm = None if srcmap is None else _i64(srcmap)
    N = out.shape[0]
    S, k = s.shape
    assert out.shape[1] == P * Wc and c0.shape == (N,)
    for n in range(N):
        for p in range(P):
            r = n * P + p if sm is None else int(sm[n * P + p])
            if r < 0 or r >= S:
                continue
            for j in range(k):
                c = int(c0[n]) + j
                if c < 0 or c >= Wc:
                    continue
                v = s[r, j]
                if np.isnan(v):
                    continue
                out[n, p * Wc + c] = v
    return out
