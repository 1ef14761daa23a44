"""The host model of the ingest kernels (helpers/ingest_ref.py) against the project's own
CPU paths, so that the model the GPU tests compare with (test_ingest_kernels_gpu.py) rests
on two independent statements of the semantics: the ring classes and the CPU branch of
``StreamingShard._ingest_tick`` for the streaming kernels, a vectorised torch formulation of
the rollout scatter for the one-shot windows.

Data is "exact tier" wherever equality is bit for bit (window values 12*k, |k| <= 20: every
mean of 1..4 valid pods is an integer <= 240 in magnitude, exact in float32 and bf16, however
it is summed); the general tier uses the bound of a sequential float32 sum and one division,
``(P + 1) * 2^-24 * sum|x| / c``, plus half a bf16 ulp on a bf16 ring."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from foremast_amd.brain.engine import ShardSpec, StreamingShard
from foremast_amd.ingest.ringbuffer import HistoryRing, WindowRing

_spec = importlib.util.spec_from_file_location(
    "ingest_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ingest_ref.py"))
ir = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ir)

DTYPES = [torch.float32, torch.bfloat16]


def _same(got: torch.Tensor, ref, what: str) -> None:
    """Bit equality with NaN compared by position."""
    ref = torch.as_tensor(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN positions differ"
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    g = torch.where(gn, torch.zeros_like(got), got).contiguous().view(bits)
    r = torch.where(rn, torch.zeros_like(ref), ref).contiguous().view(bits)
    assert torch.equal(g, r), f"{what}: {int((g != r).sum())} cells differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_base", [False, True], ids=["cur", "base"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_tick_ingest_ref_matches_cpu_engine(dtype, with_base, exact):
    N, R, W = 23, 7, 4
    P = 3 if exact else 5
    rng = np.random.default_rng(11 + 2 * with_base + exact)
    sh = StreamingShard(ShardSpec(n_series=N, ring_len=R, season=2, pods=P, window=W, dtype=dtype), device="cpu")
    sh.load_history(torch.from_numpy(ir.window_values(rng, (N, 4), True)))  # fills up, then wraps
    hist, cur, base = sh.hist.data.clone(), sh.cur.data.numpy().copy(), sh.base.numpy().copy()
    graduated = 0
    for t in range(3 * W):
        newv = ir.new_values(rng, N, P, exact)
        newb = ir.new_values(rng, N, P, exact) if with_base else None
        if t % 3 == 1:  # rows whose evicted slot is all-NaN by the time it comes round
            newv[t % N], newv[(t + 5) % N] = np.nan, np.nan
            if with_base:
                newb[(t + 9) % N] = np.nan
        col, slot, grad = sh.hist.next_col(), sh.cur.slot(), sh.cur.ticks >= W
        assert grad == (t >= W)
        old_hist = hist.clone()
        src = base if with_base else cur
        evicted = src[:, [p * W + slot for p in range(P)]].astype(np.float64)
        hist, cur, b2, mean = ir.tick_ingest_ref(hist, col, cur, P, W, slot, newv, grad,
                                                 base if with_base else None, newb)
        base = b2 if with_base else base
        sh.ingest_tick(torch.from_numpy(newv), None if newb is None else torch.from_numpy(newb))
        _same(sh.cur.data, cur, f"cur after tick {t}")
        _same(sh.base, base, f"base after tick {t}")
        if not grad:
            _same(hist, old_hist, f"model hist must not move before the window is warm (tick {t})")
        if exact or not grad:
            _same(sh.hist.data, hist, f"hist after tick {t}")
            continue
        graduated += 1
        keep = torch.ones(R, dtype=torch.bool)
        keep[col] = False
        _same(sh.hist.data[:, keep], hist[:, keep], f"hist outside column {col} after tick {t}")
        got = sh.hist.data[:, col].double().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(mean)), f"tick {t}: all-NaN slots graduate NaN"
        ok = ~np.isnan(mean)
        cnt = (~np.isnan(evicted)).sum(1)
        bound = (P + 1) * 2.0 ** -24 * np.nansum(np.abs(evicted), axis=1) / np.maximum(cnt, 1)
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * np.abs(mean)
        assert (np.abs(got - mean)[ok] <= bound[ok]).all(), f"tick {t}"
        hist = sh.hist.data.clone()  # the next ticks start from the engine's rounding of this one
    if not exact:
        assert graduated == 2 * W
    assert torch.isnan(sh.hist.data).any() and not torch.isnan(sh.hist.data).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_ring_append_ref_matches_history_ring(dtype):
    N, R = 5, 7
    rng = np.random.default_rng(3)
    ring = HistoryRing(N, R, dtype, "cpu")
    ring.load(torch.from_numpy(rng.standard_normal((N, 5)).astype(np.float32)))
    model = ring.data.clone()
    for S in (1, 4, 7, 3):  # grows to full, wraps, a whole turn, wraps again
        v = (rng.standard_normal((N, S)) * 2.0 ** rng.integers(-6, 7, size=(N, S))).astype(np.float32)
        v[rng.random((N, S)) < 0.2] = np.nan
        col0 = ring.next_col()
        model = ir.ring_append_ref(model, col0, v)
        # the same append through the device-side column offset
        split = ir.ring_append_ref(ring.data.clone(), col0 - 2 if col0 >= 2 else col0, v,
                                   col_dev=np.array([2 if col0 >= 2 else 0, 99]))
        ring.append_(torch.from_numpy(v))
        _same(ring.data, model, f"ring after S={S}")
        _same(ring.data, split, f"ring after S={S} with col_dev")
    assert ring.length == R and ring.head == (5 + 1 + 4 + 7 + 3 - R) % R
    assert torch.isnan(ring._store[:, R:]).all()


@pytest.mark.parametrize("R,W,head,ticks", [(5, 3, 0, 3), (5, 3, 4, 5), (37, 4, 35, 4), (1, 1, 0, 1), (6, 1, 2, 9)])
def test_tick_advance_ref_matches_ring_classes(R, W, head, ticks):
    P = 2
    hist = HistoryRing(1, R, torch.float32, "cpu")
    hist.load(torch.zeros(1, R))
    hist.state.head = head  # a full ring some way round
    cur = WindowRing(1, P, W, "cpu")
    cur.ticks = ticks  # warm window: every tick graduates
    # the per-slot horizon table, built the way StreamingShard._refresh_horizons builds it
    table = np.stack([cur.horizons(W + s) for s in range(W)])
    # the record of the previous tick, as StreamingShard.tick_graph writes it before a replay
    state = {"hist_col": 0, "slot": (cur.slot() - 1) % W, "graduate": 1, "head": hist.next_col()}
    for _ in range(2 * R * W + 1):
        want_col, want_slot = hist.next_col(), cur.slot()
        state, row = ir.tick_advance_ref(state, R, W, table)
        hist.advance(1)
        cur.ticks += 1
        assert state == {"hist_col": want_col, "slot": want_slot, "graduate": 1, "head": hist.head}
        assert hist.head == hist.next_col()  # full ring: the next point overwrites the oldest
        assert np.array_equal(row, cur.horizons(cur.ticks))
    rec, row = ir.tick_advance_ref([7, state["slot"], 0, state["head"]], R, W)
    assert row is None and rec["hist_col"] == state["head"] and rec["graduate"] == 1


def _scatter_torch(win, P, Wc, src, col0, srcmap):
    """Per-minute masked write (torch.where + nonzero), independent of the triple loop."""
    N = win.shape[0]
    S, k = src.shape
    out = win.clone().view(N, P, Wc)
    sm = (torch.arange(N * P) if srcmap is None else srcmap.long()).view(N, P)
    for j in range(k):
        c = col0.long() + j
        ok = ((c >= 0) & (c < Wc))[:, None] & (sm >= 0) & (sm < S)
        vals = torch.where(ok, src[sm.clamp(0, S - 1), j], torch.full(sm.shape, float("nan")))
        rr, pp = torch.nonzero(ok & ~torch.isnan(vals), as_tuple=True)
        out[rr, pp, c[rr]] = vals[rr, pp]
    return out.view(N, P * Wc)


@pytest.mark.parametrize("N,P,Wc,k", [(1, 1, 1, 1), (7, 3, 5, 4), (7, 3, 5, 9), (40, 3, 30, 4), (33, 2, 30, 1)])
@pytest.mark.parametrize("mapped", [True, False], ids=["srcmap", "identity"])
def test_rollout_scatter_ref_matches_vectorised_torch(N, P, Wc, k, mapped):
    rng = np.random.default_rng(N * 100 + k)
    S = N * P + 3
    wide = torch.from_numpy(rng.standard_normal((S, k + 3)).astype(np.float32))
    wide[torch.from_numpy(rng.random((S, k + 3)) < 0.2)] = float("nan")
    src = wide[:, 2:2 + k]
    col0 = torch.from_numpy(rng.integers(-k - 2, Wc + 3, size=N).astype(np.int32))
    srcmap = torch.from_numpy(rng.integers(-1, S + 2, size=N * P).astype(np.int32)) if mapped else None
    win = torch.arange(N * P * Wc, dtype=torch.float32).view(N, P * Wc) + 1000.0
    ref = ir.rollout_scatter_ref(win, P, Wc, src, col0, srcmap)
    _same(_scatter_torch(win, P, Wc, src, col0, srcmap), ref, "scatter")
    assert torch.equal(win, torch.arange(N * P * Wc, dtype=torch.float32).view(N, P * Wc) + 1000.0)
    assert not np.isnan(ref).any()  # a NaN never overwrites a value
    if N >= 7:
        assert (ref != win.numpy()).any() and (ref == win.numpy()).any()
