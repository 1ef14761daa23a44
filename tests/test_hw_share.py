"""Holt-Winters variant 5, season 1 shared across gammas (hw_scan.hip ``hw_d_kernel``, ``QuadQueue``):
on a grid whose rows 4q .. 4q + 3 carry the same (alpha, beta), the first grid pair of a quad walks
season 1 and the second replays it from the saved errors.  ``FOREMAST_HW_SHARE=0`` keeps the pair
queue; both paths of one build must agree bit for bit, on every queue shape (hint pairs alone,
quads, siblings last; whole blocks and split-tail halves) and on grids without quads (fallback)."""

import numpy as np
import pytest
import torch

from foremast_amd.models import smoothing as sm_ref
from tests.test_kernels_gpu import _ref_detect, _series

pytestmark = pytest.mark.gpu

M = 1440
HMAX = 10
AL, BE, GA = (0.1, 0.3, 0.5, 0.8), (0.0, 0.01, 0.05, 0.1), (0.05, 0.1, 0.3, 0.5)
# name -> (grid, quads expected).  Kept alive for the module: the kernels' per-grid caches are
# keyed by the device pointer.
_GRID_SPECS = {
    "default64": (sm_ref.make_grid(sm_ref.MODE_HW, AL, BE, GA), True),
    "4x4x3": (sm_ref.make_grid(sm_ref.MODE_HW, AL, BE, GA[:3]), False),   # G = 48: gamma runs of three
    "2x2x2": (sm_ref.make_grid(sm_ref.MODE_HW, AL[:2], BE[1:3], GA[:2]), False),  # G % 4 == 0, rows share in twos
    "3x1x2": (sm_ref.make_grid(sm_ref.MODE_HW, AL[:3], BE[1:2], GA[:2]), False),  # G = 6
    "1x1x4": (sm_ref.make_grid(sm_ref.MODE_HW, AL[1:2], BE[2:3], GA), True),      # a single quad
}
_DEV_GRIDS = {}
KEYS = ("level", "trend", "sigma", "best", "season_hb", "forecast", "upper", "lower", "verdict", "count")


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


def _grid(name, dev):
    if name not in _DEV_GRIDS:
        _DEV_GRIDS[name] = _GRID_SPECS[name][0].to(dev).contiguous()
    return _DEV_GRIDS[name]


def _spec(K, y, dev):
    N = y.shape[0]
    hz = torch.arange(1, 11, dtype=torch.int32).repeat(2)
    cur = torch.tensor(np.nan_to_num(y[:, -20:], nan=20.0) * 1.04, device=dev)
    return K.DetectSpec(horizons=hz.to(dev), threshold=torch.full((N,), 2.0, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur, max_horizon=HMAX), hz, cur


def _fit(K, ring, T, grid, spec, best):
    """One fit with deferred detection (season_hb is an output) from the hints in ``best``."""
    N = ring.shape[0]
    out = {"best": best.clone()}
    out = K.smoothing_fit(ring, 0, T, sm_ref.MODE_HW, M, grid, spec, variant=5, out=out, defer_detect=True)
    assert K.last_hw_variant == 5 and K.last_detect_deferred
    K.hw_detect_deferred(out, spec, T, M, grid=grid)
    torch.cuda.synchronize()
    assert out["best"].shape[0] == N
    res = {k: out[k].clone() for k in KEYS}
    res["season_hb"] = res["season_hb"][:, :HMAX]   # the fit writes the forecast's phases only
    return res


def _hints(kind, N, G, dev):
    """out["best"] before the fit: the previous winners the kernel takes as hint pairs."""
    b = torch.full((N,), -1, dtype=torch.int32, device=dev)      # none: a first fit
    if kind == "same":
        b[:] = G // 2 + 1                                          # both series: one hint pair
    elif kind == "quads":
        b[0::2], b[1::2] = 1, G - 2                                # hint pairs in different quads (G >= 8)
    elif kind == "siblings":
        b[0::2], b[1::2] = 4 * (G // 8), 4 * (G // 8) + 2          # the two pairs of one quad
    return b


@pytest.mark.parametrize("T", [2880, 4320, 10080])  # nseg = 2: no fused season; 3: exactly one; 7: the product
@pytest.mark.parametrize("gname", list(_GRID_SPECS))
def test_shared_season1_equals_pair_queue_bitwise(K, gname, T, monkeypatch):
    dev = torch.device("cuda:0")
    grid = _grid(gname, dev)
    G = grid.shape[0]
    assert K.grid_has_quads(grid) == _GRID_SPECS[gname][1]
    K.hw_clear_gap_flags()
    before = K.hw_deferred_total(dev)
    lib = K.nat.require()
    slots = K._split_workspace(dev)[1]
    for N in (1, 2, 5, 9):
        assert lib.fm_hw_d_split_plan((N + 1) // 2, slots, K.SPLIT_MAX) > 0   # split "1": halves occur
        y = _series(N, T, M, seed=100 + N)
        y[N // 2] = 7.0                                            # a constant series: every SSE ties at 0
        ring = torch.tensor(y, device=dev).to(torch.bfloat16)
        spec = _spec(K, y, dev)[0]
        for split in ("1", "0"):                                   # split-tail halves / whole blocks
            monkeypatch.setenv("FOREMAST_HW_SPLIT", split)
            for prune in ("1", "0"):
                monkeypatch.setenv("FOREMAST_HW_PRUNE", prune)
                for kind in ("none", "same", "quads", "siblings"):
                    best = _hints(kind, N, G, dev)
                    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
                    shared = _fit(K, ring, T, grid, spec, best)
                    monkeypatch.setenv("FOREMAST_HW_SHARE", "0")
                    pairs = _fit(K, ring, T, grid, spec, best)
                    for key in KEYS:
                        assert torch.equal(shared[key], pairs[key]), (key, N, split, prune, kind)
    assert K.hw_deferred_total(dev) == before                     # every pair stayed in the dense kernel


@pytest.mark.parametrize("T", [4320, 10080])
def test_shared_season1_equals_pair_queue_on_many_series(K, T, monkeypatch):
    """A difference in the last bit of a sum shows on a few series in a hundred (a replayed
    season whose SSE was summed in another order did, on 2 % of them): 600 series, whole blocks
    and the split tail of the same launch, exhaustive and pruned."""
    dev = torch.device("cuda:0")
    N = 600
    grid = _grid("default64", dev)
    y = _series(N, T, M, seed=21)
    ring = torch.tensor(y, device=dev).to(torch.bfloat16)
    spec = _spec(K, y, dev)[0]
    K.hw_clear_gap_flags()
    none = _hints("none", N, 64, dev)
    monkeypatch.setenv("FOREMAST_HW_SHARE", "0")
    monkeypatch.setenv("FOREMAST_HW_PRUNE", "0")
    ref = _fit(K, ring, T, grid, spec, none)
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    for prune, best in (("0", none), ("1", none), ("1", ref["best"])):
        monkeypatch.setenv("FOREMAST_HW_PRUNE", prune)
        got = _fit(K, ring, T, grid, spec, best)
        for key in KEYS:
            assert torch.equal(got[key], ref[key]), (key, prune)


@pytest.mark.parametrize("T", [4320, 10080])
def test_shared_season1_matches_fp64_reference(K, T, monkeypatch):
    """The shared path against models/smoothing.fit_smoothing in fp64 (tolerances of test_hw_gaps.py)."""
    dev = torch.device("cuda:0")
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    N = 5
    grid = _grid("default64", dev)
    gcpu = _GRID_SPECS["default64"][0]
    y = _series(N, T, M, seed=77)
    ring = torch.tensor(y, device=dev).to(torch.bfloat16)
    yl = ring.float().cpu().numpy()
    spec, hz, cur = _spec(K, y, dev)
    K.hw_clear_gap_flags()
    out = _fit(K, ring, T, grid, spec, _hints("none", N, 64, dev))
    y64 = torch.tensor(yl, dtype=torch.float64)
    ref = sm_ref.fit_smoothing(y64, sm_ref.MODE_HW, gcpu.double(), m=M)
    kb = out["best"].cpu().long()
    same = (kb == ref.best).numpy()
    assert same.mean() >= 0.75
    for n in np.nonzero(~same)[0]:   # a flipped near-tie must be within 1e-3 of the best fp64 SSE
        chosen = sm_ref.fit_smoothing(y64[n:n + 1], sm_ref.MODE_HW, gcpu[kb[n]:kb[n] + 1].double(), m=M).sse[0]
        assert chosen <= ref.sse[n] * (1 + 1e-3) + 1e-6
    np.testing.assert_allclose(out["sigma"].cpu().numpy(), ref.sigma.numpy(), rtol=5e-3)
    np.testing.assert_allclose(out["level"].cpu().numpy()[same], ref.level.numpy()[same], rtol=2e-3, atol=5e-3)
    np.testing.assert_allclose(out["trend"].cpu().numpy()[same], ref.trend.numpy()[same], rtol=2e-2, atol=2e-4)
    f_ref = sm_ref.forecast(ref, hz.long())
    np.testing.assert_allclose(out["forecast"].cpu().numpy()[same], f_ref.numpy()[same], rtol=5e-3, atol=2e-2)
    d = _ref_detect(out, gcpu, sm_ref.MODE_HW, M, hz, cur)
    assert torch.equal(d.count, out["count"].cpu())
    assert torch.equal(d.verdict, out["verdict"].cpu())


def test_gapped_series_still_goes_to_the_gapped_kernel(K, monkeypatch):
    """One NaN past season 0: its series pair is handed to hw_dg_kernel, the other series are
    what they are without it."""
    dev = torch.device("cuda:0")
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    N, T = 5, 10080
    grid = _grid("default64", dev)
    y = _series(N, T, M, seed=78)
    spec = _spec(K, y, dev)[0]
    none = _hints("none", N, 64, dev)
    K.hw_clear_gap_flags()
    before = K.hw_deferred_total(dev)
    clean = _fit(K, torch.tensor(y, device=dev).to(torch.bfloat16), T, grid, spec, none)
    assert K.hw_deferred_total(dev) == before
    yg = y.copy()
    yg[3, 2 * M + 17] = np.nan
    gapped = _fit(K, torch.tensor(yg, device=dev).to(torch.bfloat16), T, grid, spec, none)
    assert K.hw_deferred_total(dev) == before + 1                 # the pair of series 2 and 3
    K.hw_clear_gap_flags()
    keep = torch.tensor([0, 1, 4], device=dev)
    for key in KEYS:
        assert torch.equal(gapped[key][keep], clean[key][keep]), key
    assert torch.isfinite(gapped["sigma"]).all()
