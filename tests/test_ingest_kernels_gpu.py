"""The ring and window ingest kernels (ops/csrc/ingest.hip, ring_append of ops/csrc/window.hip)
against the fp64 host model of helpers/ingest_ref.py, which test_ingest_ref.py ties to the
ring classes and the CPU engine.

These kernels move data exactly, apart from one float32 mean, so every comparison is bit for
bit (NaN by position, bf16 through its int16 bits) and on the WHOLE tensor: every output
starts from a recognisable pattern (a ramp or 7.0 for floats, 5 for int32), and untouched
cells, the pad columns of a ring's backing store and the guard elements around every sliced
argument must come back unchanged.

The graduating mean has two tiers.  Exact: P <= 4 and window values 12*k, |k| <= 20, so the
mean of any 1..4 valid pods is an integer of magnitude <= 240, exact in float32 and in bf16
whatever the summation order (the tests first check this on the model's own means).
General (P = 5, normals scaled by 1e3): a sequential float32 sum of c <= P terms and one
division err by at most (P + 1) * 2^-24 * sum|x| / c, and a bf16 ring adds half a bf16 ulp,
2^-8 * |mean|.

Nothing here passes an out-of-range slot or column to a kernel, and the doorbell is only
launched already rung."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from foremast_amd.ingest.ringbuffer import HistoryRing

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "ingest_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ingest_ref.py"))
ir = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ir)

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


def _same(got: torch.Tensor, ref, what: str) -> None:
    """Bit equality of a (CPU copy of a) result with the model, NaN compared by position."""
    got = got.detach().cpu()
    ref = torch.as_tensor(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    if not got.dtype.is_floating_point:
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} cells differ"
        return
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN positions differ in {int((gn != rn).sum())} cells"
    bits = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    g = torch.where(gn, torch.zeros_like(got), got).contiguous().view(bits)
    r = torch.where(rn, torch.zeros_like(ref), ref).contiguous().view(bits)
    assert torch.equal(g, r), f"{what}: {int((g != r).sum())} cells differ"


def _ramp(n: int, m: int) -> torch.Tensor:
    """Small integers (exact in bf16), different in neighbouring cells and rows."""
    return ((torch.arange(n * m, dtype=torch.float32) % 199) - 99).view(n, m)


def _ring(n: int, R: int, dtype) -> HistoryRing:
    """The padded-stride ring the engines use (ld != R), data region holding a ramp."""
    ring = HistoryRing(n, R, dtype, DEV)
    assert ring.data.stride(0) == ring.ld and ring.ld != R
    ring.data.copy_(_ramp(n, R))
    return ring


def _store_with(before_store: torch.Tensor, data, R: int) -> torch.Tensor:
    """The backing store expected after a kernel: the model's data region, pads as before (NaN)."""
    exp = before_store.clone()
    exp[:, :R] = torch.as_tensor(data).to(exp.dtype)
    assert exp.shape[1] > R and torch.isnan(exp[:, R:]).all()
    return exp


def _guard(n_before: int, n: int, n_after: int = 4):
    """An int32 tensor of 5s and the slice of it a kernel may write."""
    g = torch.full((n_before + n + n_after,), 5, dtype=torch.int32, device=DEV)
    return g, g[n_before:n_before + n]


def _guard_ok(g: torch.Tensor, n_before: int, n: int, inner, what: str) -> None:
    exp = torch.full((g.numel(),), 5, dtype=torch.int32)
    exp[n_before:n_before + n] = torch.as_tensor(inner, dtype=torch.int32)
    _same(g, exp, what)


# ---------------------------------------------------------------------------------
# ring_append
# ---------------------------------------------------------------------------------
def _scaled_normals(rng, shape) -> np.ndarray:
    v = (rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 7, size=shape)).astype(np.float32)
    v[rng.random(shape) < 0.1] = np.nan
    return v


def _append_case(K, dtype, N, R, col0, S, col_dev=None, lead=2, tail=3, seed=0):
    rng = np.random.default_rng(seed + 1000 * S + N)
    ring = _ring(N, R, dtype)
    before = ring._store.cpu()
    wide = torch.from_numpy(_scaled_normals(rng, (N, lead + S + tail))).to(DEV)
    src = wide[:, lead:lead + S]
    assert src.stride(0) != S
    cd = cd_before = None
    if col_dev is not None:
        cd = torch.tensor(col_dev, dtype=torch.int32, device=DEV)
        cd_before = cd.cpu()
    K.ring_append(ring.data, col0, src, cd)
    torch.cuda.synchronize()
    ref = ir.ring_append_ref(before[:, :R], col0, src.cpu(), None if cd is None else cd_before)
    _same(ring._store, _store_with(before, ref, R), f"ring N={N} col0={col0} S={S} col_dev={col_dev}")
    if cd is not None:
        _same(cd, cd_before, "col_dev is read-only")
    return ring


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [1, 255, 257])
def test_ring_append_columns(K, dtype, N):
    R = 37
    for col0, S in [(0, 1), (36, 1), (35, 5), (0, 37), (20, 37), (37 + 3, 5), (-2, 5), (-2, 1)]:
        _append_case(K, dtype, N, R, col0, S)
    # one feature column of a wider block, as the LSTM engine appends it
    _append_case(K, dtype, N, R, 36, 1, lead=3, tail=2)
    _append_case(K, dtype, N, R, 0, 1, lead=0, tail=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("N", [1, 255, 257])
def test_ring_append_col_dev(K, dtype, N):
    R = 37
    _append_case(K, dtype, N, R, 30, 5, col_dev=[9])        # 30 + 9 >= R
    _append_case(K, dtype, N, R, 30, 1, col_dev=[9])
    _append_case(K, dtype, N, R, 30, 37, col_dev=[9])
    _append_case(K, dtype, N, R, 30, 5, col_dev=[0])
    _append_case(K, dtype, N, R, 30, 9, col_dev=[0])        # wraps without the offset's help
    _append_case(K, dtype, N, R, 35, 5, col_dev=[36, 1000, 3, 7])  # element 0 of a longer tensor
    _append_case(K, dtype, N, R, 0, 1, col_dev=[36, 0])


def _conversion_row() -> np.ndarray:
    f = np.float32
    special = [0.0, -0.0, np.inf, -np.inf, np.nan,
               1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23,        # a tie (down), a tie (up), just above
               -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 - 2.0 ** -23,  # and just below a tie
               float(np.finfo(f).max), -float(np.finfo(f).max),                     # round to +-inf
               2.0 ** -126, 2.0 ** -127, 2.0 ** -133 + 2.0 ** -149, 2.0 ** -149, -1e-40]
    rng = np.random.default_rng(5)
    rnd = rng.standard_normal(1000) * 2.0 ** rng.integers(-40, 41, size=1000)
    with np.errstate(over="ignore"):
        return np.concatenate([np.array(special, dtype=np.float64), rnd]).astype(f)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_ring_append_conversion_is_round_to_nearest_even(K, dtype):
    row = _conversion_row()
    S, R, N = row.size, row.size + 19, 3
    vals = np.stack([row, -row, np.roll(row, 7)])
    ring = _ring(N, R, dtype)
    before = ring._store.cpu()
    src = torch.from_numpy(vals).to(DEV)
    K.ring_append(ring.data, 11, src)
    torch.cuda.synchronize()
    got = ring._store.cpu()
    # against the conversion itself ...
    want = torch.from_numpy(vals).to(dtype)
    _same(got[:, 11:11 + S], want, "converted values")
    assert torch.equal(torch.isinf(got[:, 11:11 + S]), torch.isinf(want))
    if dtype == torch.bfloat16:
        w = want[0].float()
        assert w[5] == 1.0 and w[6] == 1 + 2.0 ** -6 and w[7] == 1 + 2.0 ** -7 and w[10] == 1.0  # the ties went to even
        assert torch.isinf(w[11]) and torch.isinf(w[12])
    # ... and, whole store, against the model
    _same(got, _store_with(before, ir.ring_append_ref(before[:, :R], 11, vals), R), "store")


def test_ring_append_grid_stride(K):
    """2,107,400 elements: more than the 8192 blocks x 256 threads of one pass."""
    N, S, R = 8200, 257, 300
    assert N * S > 8192 * 256
    rng = np.random.default_rng(8)
    ring = HistoryRing(N, R, torch.bfloat16, DEV)
    ring.data.fill_(7.0)
    before = ring._store.cpu()
    vals = rng.standard_normal((N, S)).astype(np.float32)
    vals[::13, ::5] = np.nan
    K.ring_append(ring.data, 100, torch.from_numpy(vals).to(DEV))
    torch.cuda.synchronize()
    _same(ring._store, _store_with(before, ir.ring_append_ref(before[:, :R], 100, vals), R), "store")


# ---------------------------------------------------------------------------------
# tick_ingest
# ---------------------------------------------------------------------------------
R_HIST = 37


def _slot_means(win: np.ndarray, P: int, W: int, slot: int) -> np.ndarray:
    ev = win[:, [p * W + slot for p in range(P)]].astype(np.float64)
    ok = ~np.isnan(ev)
    cnt = ok.sum(1)
    return np.where(cnt > 0, np.where(ok, ev, 0.0).sum(1) / np.maximum(cnt, 1), np.nan)


def _windows(rng, N, P, W, slot, exact):
    """Independent current and baseline windows with the NaN patterns of punch_slot, redrawn
    until the two evicted-slot means differ in every row where either has one."""
    cur = ir.window_values(rng, (N, P * W), exact)
    base = ir.window_values(rng, (N, P * W), exact)
    ir.punch_slot(cur, base, P, W, slot)
    cols = [p * W + slot for p in range(P)]
    for _ in range(200):
        mc, mb = _slot_means(cur, P, W, slot), _slot_means(base, P, W, slot)
        clash = np.nonzero(mc == mb)[0]
        if clash.size == 0:
            break
        for n in clash:
            live = [c for c in cols if not np.isnan(base[n, c])]
            base[n, live] = ir.window_values(rng, (len(live),), exact)
    mc, mb = _slot_means(cur, P, W, slot), _slot_means(base, P, W, slot)
    assert not (mc == mb).any(), "test data: current and baseline slot means must differ"
    return cur, base


def _ingest_case(K, dtype, with_base, form, P, W, slot, N, hist_col, nz, graduate=True, exact=None):
    exact = P <= 4 if exact is None else exact
    assert not exact or P <= 4
    rng = np.random.default_rng(7 * N + 31 * P + W + slot + (1000 if with_base else 0))
    C = P * W
    cols = [p * W + slot for p in range(P)]
    rest = [c for c in range(C) if c not in cols]
    ring = _ring(N, R_HIST, dtype)
    store0 = ring._store.cpu()
    cur0, base0 = _windows(rng, N, P, W, slot, exact)
    newv0, newb0 = ir.new_values(rng, N, P, exact), ir.new_values(rng, N, P, exact)
    cur = torch.from_numpy(cur0).to(DEV)
    base = torch.from_numpy(base0).to(DEV)  # the decoy when no baseline streams
    wide = torch.full((N, 2 * P + 1), 7.0, device=DEV)
    wide[:, :P] = torch.from_numpy(newv0).to(DEV)
    wide[:, P:2 * P] = torch.from_numpy(newb0).to(DEV)
    newv, newb = wide[:, :P], wide[:, P:2 * P]
    wide0 = wide.cpu()
    g = zero = None
    if nz is not None:
        g, zero = _guard(3, nz)
    kw = dict(base=base, newb=newb) if with_base else {}
    if form == "state":
        rec = [hist_col, slot, int(graduate), 123]  # the 4-element record the engine keeps
        state = torch.tensor(rec, dtype=torch.int32, device=DEV)
        # scalars that differ from the record (and are valid) must be ignored
        K.tick_ingest(ring.data, (hist_col + 5) % R_HIST, cur, P, W, (slot + 1) % W, newv,
                      graduate=not graduate, state=state, zero=zero, **kw)
    else:
        K.tick_ingest(ring.data, hist_col, cur, P, W, slot, newv, graduate=graduate, zero=zero, **kw)
    torch.cuda.synchronize()
    tag = f"{form} P={P} W={W} slot={slot} N={N} col={hist_col} nz={nz} grad={graduate}"
    if form == "state":
        _same(state, torch.tensor(rec, dtype=torch.int32), f"state is read-only ({tag})")
    _same(wide, wide0, f"the tick's values are read-only ({tag})")

    hist_ref, cur_ref, base_ref, mean = ir.tick_ingest_ref(
        store0[:, :R_HIST], hist_col, cur0, P, W, slot, newv0, graduate,
        base0 if with_base else None, newb0 if with_base else None)
    other = _slot_means(cur0 if with_base else base0, P, W, slot)
    assert not (mean == other).any()  # graduating the other window's mean cannot pass

    # windows: the model bit for bit, only the P slot columns moved
    got_cur = cur.cpu()
    _same(got_cur, cur_ref, f"cur ({tag})")
    _same(got_cur[:, rest], cur0[:, rest], f"cur outside the slot ({tag})")
    _same(got_cur[:, cols], newv0, f"cur slot holds the new values, NaN included ({tag})")
    if with_base:
        _same(base, base_ref, f"base ({tag})")
        _same(base.cpu()[:, rest], base0[:, rest], f"base outside the slot ({tag})")
        _same(base.cpu()[:, cols], newb0, f"base slot ({tag})")
    else:
        _same(base, base0, f"decoy baseline untouched ({tag})")

    # history: at most one column moved, pads stay NaN
    got_store = ring._store.cpu()
    keep = [c for c in range(ring.ld) if c != hist_col]
    _same(got_store[:, keep], store0[:, keep], f"hist outside column {hist_col} ({tag})")
    if not graduate:
        _same(got_store, store0, f"nothing graduates ({tag})")
    elif exact:
        ok = ~np.isnan(mean)
        assert (mean[ok] == np.rint(mean[ok])).all() and (np.abs(mean[ok]) <= 240).all(), \
            "exact tier precondition: every model mean is an integer of magnitude <= 240"
        _same(got_store, _store_with(store0, hist_ref, R_HIST), f"hist ({tag})")
    else:
        got = got_store[:, hist_col].double().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(mean)), f"all-NaN slots graduate NaN ({tag})"
        ev = (base0 if with_base else cur0)[:, cols].astype(np.float64)
        cnt = (~np.isnan(ev)).sum(1)
        bound = (P + 1) * 2.0 ** -24 * np.nansum(np.abs(ev), axis=1) / np.maximum(cnt, 1)
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * np.abs(mean)
        ok = ~np.isnan(mean)
        err = np.abs(got - mean)
        print(f"{tag}: worst error / bound = {np.max(err[ok] / bound[ok]):.3f}")
        assert (err[ok] <= bound[ok]).all(), f"graduated mean ({tag})"
    if N >= 7 and graduate:  # the NaN patterns are all there
        assert np.isnan(mean).any() and (~np.isnan(mean)).any()
    if g is not None:
        _guard_ok(g, 3, nz, 0, f"zeroed counters and their guards ({tag})")


#             form     (P, W, slot)  N     col nz    graduate
INGEST = [("scalar", (1, 1, 0), 1, 0, None, True),
          ("state", (3, 2, 1), 255, 17, 1, True),
          ("scalar", (4, 10, 0), 256, 36, 33, True),
          ("state", (4, 10, 9), 257, 0, None, True),
          ("scalar", (5, 10, 3), 1000, 17, 33, True),
          ("state", (5, 10, 3), 257, 36, 1, True),
          ("scalar", (3, 2, 1), 5, 17, 700, True),      # the zeroing loop spans blocks past N
          ("state", (4, 10, 0), 5, 36, 700, True),
          ("scalar", (4, 10, 9), 255, 0, None, False),  # graduate=False
          ("state", (3, 2, 1), 256, 17, 33, False),     # state[2] = 0
          ("state", (1, 1, 0), 1000, 36, 1, True),
          ("scalar", (4, 10, 9), 1, 17, 1, True),
          ("state", (5, 10, 3), 255, 0, 33, False)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("with_base", [False, True], ids=["cur", "base"])
@pytest.mark.parametrize("case", INGEST,
                         ids=lambda c: "%s-P%dW%ds%d-N%d-c%d-z%s-g%d" % (c[0], *c[1], c[2], c[3], c[4], c[5]))
def test_tick_ingest(K, dtype, with_base, case):
    form, (P, W, slot), N, col, nz, grad = case
    _ingest_case(K, dtype, with_base, form, P, W, slot, N, col, nz, grad)


def test_tick_ingest_case_table_covers_every_axis():
    assert {c[0] for c in INGEST} == {"scalar", "state"}
    assert {c[1] for c in INGEST} == {(1, 1, 0), (3, 2, 1), (4, 10, 0), (4, 10, 9), (5, 10, 3)}
    assert {c[2] for c in INGEST} >= {1, 255, 256, 257, 1000}
    assert {c[3] for c in INGEST} == {0, 17, 36}
    assert {c[4] for c in INGEST} == {None, 1, 33, 700}
    assert all(c[2] == 5 for c in INGEST if c[4] == 700)
    assert {(c[0], c[5]) for c in INGEST} == {("scalar", True), ("scalar", False), ("state", True), ("state", False)}


# ---------------------------------------------------------------------------------
# tick_advance, alone and feeding tick_ingest
# ---------------------------------------------------------------------------------
def _run_advance(K, R, W, head, slot, steps, nh=None):
    """``steps`` launches from the record {5, slot, 0, head}; the record (and the horizon
    buffer) after every launch goes to a stream-ordered device log, read after one sync."""
    g, state = _guard(2, 4)
    state.copy_(torch.tensor([5, slot, 0, head], dtype=torch.int32))
    table = hg = hbuf = None
    if nh is not None:
        table = (torch.arange(W * nh, dtype=torch.int32) * 3 + 7).view(W, nh).to(DEV)
        hg, hbuf = _guard(4, nh)
    log, hlog = [], []
    for _ in range(steps):
        K.tick_advance(state, R, W, table, hbuf)
        log.append(state.clone())
        if hg is not None:
            hlog.append(hg.clone())
    torch.cuda.synchronize()
    rec = {"hist_col": 5, "slot": slot, "graduate": 0, "head": head}
    for i in range(steps):
        rec, row = ir.tick_advance_ref(rec, R, W, None if table is None else table.cpu())
        want = [rec["hist_col"], rec["slot"], rec["graduate"], rec["head"]]
        assert log[i].tolist() == want, f"R={R} W={W} step {i}: {log[i].tolist()} != {want}"
        assert 0 <= want[0] < R and 0 <= want[1] < W and 0 <= want[3] < R
        if hg is not None:
            assert row.tolist() == table.cpu()[(rec["slot"] + 1) % W].tolist()
            _guard_ok(hlog[i], 4, nh, row, f"h_buf and its guards, R={R} W={W} nh={nh} step {i}")
    _guard_ok(g, 2, 4, log[-1].cpu(), "the record's guards")
    if table is not None:
        _same(table, (torch.arange(W * nh, dtype=torch.int32) * 3 + 7).view(W, nh), "h_table is read-only")


@pytest.mark.parametrize("R,W,head,slot", [(5, 3, 0, 0), (5, 3, 4, 2), (5, 3, 2, 1), (5, 1, 3, 0), (1, 3, 0, 1)])
def test_tick_advance_record(K, R, W, head, slot):
    _run_advance(K, R, W, head, slot, 2 * R * W)


@pytest.mark.parametrize("nh", [1, 300])
def test_tick_advance_horizon_row(K, nh):
    _run_advance(K, 5, 3, 4, 2, 2 * 5 * 3, nh=nh)
    _run_advance(K, 5, 1, 0, 0, 3, nh=nh)


def test_tick_advance_without_table_leaves_h_buf(K):
    state = torch.tensor([5, 2, 0, 4], dtype=torch.int32, device=DEV)
    hg, hbuf = _guard(4, 300)
    K.tick_advance(state, 5, 3, None, hbuf)
    torch.cuda.synchronize()
    assert state.tolist() == [4, 0, 1, 0]
    _guard_ok(hg, 4, 300, 5, "decoy h_buf")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("with_base", [False, True], ids=["cur", "base"])
def test_tick_advance_drives_tick_ingest(K, dtype, with_base):
    """A full ring in steady state: every tick is tick_advance then tick_ingest reading the
    record, against the host model of the one driving the host model of the other."""
    N, R, W, P, head0 = 70, R_HIST, 4, 3, 35
    ticks = 2 * R + 3
    rng = np.random.default_rng(21 + with_base)
    ring = HistoryRing(N, R, dtype, DEV)
    ring.load(torch.from_numpy(ir.window_values(rng, (N, R), True)).to(DEV))
    ring.state.head = head0
    assert ring.length == R
    store0 = ring._store.cpu()
    cur0, base0 = _windows(rng, N, P, W, 0, True)
    cur, base = torch.from_numpy(cur0).to(DEV), torch.from_numpy(base0).to(DEV)
    vals0 = np.stack([np.concatenate([ir.new_values(rng, N, P, True), ir.new_values(rng, N, P, True)], axis=1)
                      for _ in range(ticks)])
    for t in (ticks - 17, ticks - 16, ticks - 15):  # all-NaN slots that graduate late enough to stay in the ring
        vals0[t, 3] = np.nan
    vals = torch.from_numpy(vals0).to(DEV)
    state = torch.tensor([0, W - 1, 1, ring.next_col()], dtype=torch.int32, device=DEV)
    for t in range(ticks):
        K.tick_advance(state, R, W)
        K.tick_ingest(ring.data, 0, cur, P, W, 0, vals[t, :, :P], state=state,
                      **(dict(base=base, newb=vals[t, :, P:]) if with_base else {}))
    torch.cuda.synchronize()

    rec = {"hist_col": 0, "slot": W - 1, "graduate": 1, "head": head0}
    hist_m, cur_m, base_m = store0[:, :R], cur0, base0 if with_base else None
    for t in range(ticks):
        rec, _ = ir.tick_advance_ref(rec, R, W)
        hist_m, cur_m, base_m, mean = ir.tick_ingest_ref(
            hist_m, rec["hist_col"], cur_m, P, W, rec["slot"], vals0[t, :, :P], rec["graduate"],
            base_m, vals0[t, :, P:] if with_base else None)
        ok = ~np.isnan(mean)
        assert (mean[ok] == np.rint(mean[ok])).all(), "exact tier precondition"
    assert rec["head"] == (head0 + ticks) % R
    assert state.tolist() == [rec["hist_col"], rec["slot"], 1, (head0 + ticks) % R]
    _same(ring._store, _store_with(store0, hist_m, R), "hist")
    _same(cur, cur_m, "cur")
    _same(base, base_m if with_base else base0, "base")
    assert torch.isnan(ring.data[3]).any() and not torch.isnan(ring.data[3]).all()


def test_tick_advance_doorbell_already_rung(K):
    bell = torch.zeros(1, dtype=torch.int32).pin_memory()
    bell[0] = 3
    bg, bell_dev = _guard(1, 2)
    bell_dev.copy_(torch.tensor([2, 0], dtype=torch.int32))
    state = torch.tensor([5, 2, 0, 4], dtype=torch.int32, device=DEV)
    K.tick_advance(state, 5, 3, bell=bell, bell_dev=bell_dev)
    torch.cuda.synchronize()
    _guard_ok(bg, 1, 2, [3, 0], "bell_dev after the first tick")
    assert state.tolist() == [4, 0, 1, 0]
    bell[0] = 4
    K.tick_advance(state, 5, 3, bell=bell, bell_dev=bell_dev)
    torch.cuda.synchronize()
    _guard_ok(bg, 1, 2, [4, 0], "bell_dev after the second tick")
    assert state.tolist() == [0, 1, 1, 1]
    assert bell.tolist() == [4]


# ---------------------------------------------------------------------------------
# rollout_scatter / rollout_tick_scatter
# ---------------------------------------------------------------------------------
T0 = 28_333_334  # a tick's first minute (minutes since the epoch)


def _placements(col0, k, Wc):
    out = set()
    for c in col0.tolist():
        if c + k <= 0:
            out.add("left")
        elif c >= Wc:
            out.add("right")
        elif c < 0:
            out.add("straddles 0")
        elif c + k > Wc:
            out.add("straddles Wc")
        else:
            out.add("inside")
    return out


def _scatter_inputs(N, P, Wc, k, mapping, seed=0):
    rng = np.random.default_rng(seed + 97 * N + k)
    S = {"srcmap": N * P + 3, "exact": N * P, "more": N * P + 4}[mapping]
    wide = rng.standard_normal((S, k + 3)).astype(np.float32)
    wide[rng.random(wide.shape) < 0.2] = np.nan
    col0 = rng.integers(-k - 2, Wc + 3, size=N).astype(np.int32)
    want = set()
    if N >= 5:
        col0[:5] = [-k - 1, -1, 0, Wc - 1, Wc + 1]
        want = {"left", "right"} | ({"straddles 0", "straddles Wc"} if k >= 2 else set()) \
            | ({"inside"} if k <= Wc else set())
        assert want <= _placements(col0, k, Wc)
    assert col0.min() >= -k - 2 and col0.max() <= Wc + 2
    srcmap = None
    if mapping == "srcmap":
        srcmap = rng.integers(-1, S + 2, size=N * P).astype(np.int32)
        if N * P >= 6:
            srcmap[:6] = [2, 2, -1, S, S + 1, 0]  # two pods reading one row, unmapped, past the block
            assert {-1, S}.issubset(srcmap.tolist())
    return wide, col0, srcmap, want


SCATTER = [(1, 1, 1, 1), (7, 3, 5, 4), (7, 3, 5, 9), (300, 3, 30, 4), (33, 2, 30, 1)]
#           zero tensors of the tick scatter per shape: none, one and two, short and long
ZEROS = {(1, 1, 1, 1): (5000, 1), (7, 3, 5, 4): (33,), (7, 3, 5, 9): (), (300, 3, 30, 4): (1, 33),
         (33, 2, 30, 1): (1, 5000)}


@pytest.mark.parametrize("shape", SCATTER, ids=lambda s: "N%d-P%d-Wc%d-k%d" % s)
@pytest.mark.parametrize("mapping", ["srcmap", "exact", "more"])
def test_rollout_scatter(K, shape, mapping):
    N, P, Wc, k = shape
    wide0, col0, srcmap0, _ = _scatter_inputs(N, P, Wc, k, mapping)
    win0 = torch.arange(N * P * Wc, dtype=torch.float32).view(N, P * Wc) + 1000.0
    wide = torch.from_numpy(wide0).to(DEV)
    src = wide[:, 2:2 + k]
    assert src.stride(0) > k
    srcmap = None if srcmap0 is None else torch.from_numpy(srcmap0).to(DEV)
    ref = ir.rollout_scatter_ref(win0, P, Wc, wide0[:, 2:2 + k], col0, srcmap0)
    assert not np.isnan(ref).any()
    if N >= 7:
        assert (ref != win0.numpy()).any() and (ref == win0.numpy()).any()

    win = win0.to(DEV)
    K.rollout_scatter(win, P, Wc, src, torch.from_numpy(col0).to(DEV), srcmap)
    torch.cuda.synchronize()
    _same(win, ref, "rollout_scatter")

    # the tick form: the column is tick[0] - start_min[n], the counters are zeroed on the way
    win_t = win0.to(DEV)
    tick = torch.tensor([T0, 999, -4], dtype=torch.int32, device=DEV)
    start_min = torch.from_numpy((T0 - col0.astype(np.int64)).astype(np.int32)).to(DEV)
    guards = [_guard(3 + i, n) for i, n in enumerate(ZEROS[shape])]
    if ZEROS[shape] and max(ZEROS[shape]) == 5000:
        assert N * P * k < 5000
    K.rollout_tick_scatter(win_t, P, Wc, src, start_min, tick, srcmap, tuple(z for _, z in guards))
    torch.cuda.synchronize()
    _same(win_t, ref, "rollout_tick_scatter")
    for i, (g, _z) in enumerate(guards):
        _guard_ok(g, 3 + i, ZEROS[shape][i], 0, f"zero tensor {i} of {ZEROS[shape]}")
    _same(tick, torch.tensor([T0, 999, -4], dtype=torch.int32), "tick is read-only")
    _same(wide, wide0, "src is read-only")
    if srcmap is not None:
        _same(srcmap, srcmap0, "srcmap is read-only")


def test_rollout_scatter_cases_place_the_block_everywhere():
    seen = set()
    for N, P, Wc, k in SCATTER:
        _, col0, _, want = _scatter_inputs(N, P, Wc, k, "srcmap")
        seen |= want
    assert seen == {"left", "straddles 0", "inside", "straddles Wc", "right"}
    assert sorted(len(z) for z in ZEROS.values()) == [0, 1, 2, 2, 2]


def test_rollout_tick_scatter_idle_tick(K):
    """The call of a tick without new minutes: no rows, only the zeroing."""
    P, Wc = 3, 5
    decoy0 = torch.arange(7 * P * Wc, dtype=torch.float32).view(7, P * Wc) + 1000.0
    decoy = decoy0.to(DEV)
    start_min = torch.full((7,), T0, dtype=torch.int32, device=DEV)
    src = torch.full((1, 1), 7.0, device=DEV)
    tick = torch.tensor([T0], dtype=torch.int32, device=DEV)
    (ga, za), (gb, zb) = _guard(3, 33), _guard(2, 1)
    K.rollout_tick_scatter(decoy[:0], P, Wc, src, start_min[:0], tick[0:1], None, (za, zb))
    torch.cuda.synchronize()
    _guard_ok(ga, 3, 33, 0, "first zero tensor")
    _guard_ok(gb, 2, 1, 0, "second zero tensor")
    _same(decoy, decoy0, "decoy window")
    _same(src, torch.full((1, 1), 7.0), "src")


def test_rollout_scatter_wrappers_validate(K):
    N, P, Wc, k = 7, 3, 5, 4
    win = torch.full((N, P * Wc), 7.0, device=DEV)
    src = torch.zeros((N * P, k), device=DEV)
    col0 = torch.zeros(N, dtype=torch.int32, device=DEV)
    tick = torch.tensor([T0], dtype=torch.int32, device=DEV)
    srcmap = torch.zeros(N * P, dtype=torch.int32, device=DEV)
    z = [_guard(1, 2)[1] for _ in range(3)]
    E = K.KernelShapeError
    for w in (win.double(), torch.full((N, P * Wc + 1), 7.0, device=DEV)):
        with pytest.raises(E):
            K.rollout_scatter(w, P, Wc, src, col0)
        with pytest.raises(E):
            K.rollout_tick_scatter(w, P, Wc, src, col0, tick)
    with pytest.raises(E):
        K.rollout_scatter(win, P, Wc, src, col0, srcmap[:-1])
    with pytest.raises(E):
        K.rollout_tick_scatter(win, P, Wc, src, col0, tick, srcmap[:-1])
    with pytest.raises(E):
        K.rollout_tick_scatter(win, P, Wc, src, col0, tick, srcmap, tuple(z))
    torch.cuda.synchronize()
    _same(win, torch.full((N, P * Wc), 7.0), "nothing launched")
    for t in z:
        assert t.tolist() == [5, 5]
