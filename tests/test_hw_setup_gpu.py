"""Holt-Winters variant 5, per-pair set-up (hw_scan.hip ``GridPair``, ``lane_powers``): a
lane's Bj = B^(lane & 15) comes from a table section the device fills once per grid, and a
quad's two pairs share one set-up.  None of it may move a bit: the outputs are held to those of
the commit before the change (``tests/golden/hw_parent_bits.npz``, written by
``scripts/hw_golden_bits.py``), the pruned fit to the exhaustive one (also with the bound and
the SSEs at the ends of the fp32 range), and the table section to its definition."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.test_hw_share import _GRID_SPECS, _hints

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec_ = importlib.util.spec_from_file_location("hw_golden_bits", os.path.join(ROOT, "scripts", "hw_golden_bits.py"))
gb = importlib.util.module_from_spec(_spec_)
_spec_.loader.exec_module(gb)


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "hw_parent_bits.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _same_bits(a, b):
    return all(torch.equal(gb.bits(a[k]), gb.bits(b[k])) for k in gb.ARRAYS)


@pytest.mark.parametrize("gname", gb.GRIDS)
@pytest.mark.parametrize("case", gb.CASES, ids=[c[0] for c in gb.CASES])
def test_outputs_are_the_parent_commits_bitwise(K, golden, case, gname, monkeypatch):
    name, m, T, hmax, quad = case
    dev = torch.device("cuda:0")
    grid = gb.dev_grid(gname, dev)
    G = grid.shape[0]
    assert K.grid_has_quads(grid) == _GRID_SPECS[gname][1]
    monkeypatch.setenv("FOREMAST_HW_PRUNE", "1")
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    monkeypatch.setenv("FOREMAST_HW_QUAD", quad)
    before = K.hw_deferred_total(dev)
    for N in gb.NS:
        K.hw_clear_gap_flags()
        y = gb.series(N, T, m)
        ring = torch.tensor(y, device=dev).to(torch.bfloat16)
        spec = gb.detect_spec(K, y, dev, hmax)
        base = f"{name}|{gname}|N{N}"
        r0 = gb.rows()[(name, gname, N)]
        for split, kind in gb.settings():
            monkeypatch.setenv("FOREMAST_HW_SPLIT", split)
            got = gb.fit(K, ring, T, m, grid, spec, _hints(kind, N, G, dev), hmax)
            for k in gb.ARRAYS:
                own = f"{base}|split{split}|{kind}|{k}"
                want = golden[own] if own in golden else golden[k][r0:r0 + N]
                if k == "season_hb":
                    want = want[:, :hmax]
                assert torch.equal(gb.bits(got[k]), want), (k, N, split, kind)
    assert K.hw_deferred_total(dev) == before                     # every pair stayed in the dense kernels


# the prune bound and the SSEs near the bottom of the normal range and far up it
@pytest.mark.parametrize("scale", [1.0, 1e-18, 1e15])
@pytest.mark.parametrize("case", gb.CASES, ids=[c[0] for c in gb.CASES])
def test_pruned_fit_equals_exhaustive_bitwise(K, case, scale, monkeypatch):
    name, m, T, hmax, quad = case
    dev = torch.device("cuda:0")
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    monkeypatch.setenv("FOREMAST_HW_QUAD", quad)
    for gname in gb.GRIDS:
        grid = gb.dev_grid(gname, dev)
        G = grid.shape[0]
        for N in gb.NS:
            K.hw_clear_gap_flags()
            y = gb.series(N, T, m, scale)
            ring = torch.tensor(y, device=dev).to(torch.bfloat16)
            assert torch.isfinite(ring.float()).all() and bool((ring.float() != 0).all())
            spec = gb.detect_spec(K, y, dev, hmax)
            for split, kind in (("1", "none"), ("0", "same"), ("1", "siblings")):
                monkeypatch.setenv("FOREMAST_HW_SPLIT", split)
                best = _hints(kind, N, G, dev)
                monkeypatch.setenv("FOREMAST_HW_PRUNE", "1")
                pruned = gb.fit(K, ring, T, m, grid, spec, best, hmax)
                monkeypatch.setenv("FOREMAST_HW_PRUNE", "0")
                full = gb.fit(K, ring, T, m, grid, spec, best, hmax)
                assert _same_bits(pruned, full), (gname, N, split, kind)
                assert torch.isfinite(pruned["sigma"]).all()


@pytest.mark.parametrize("k", [45, 9, 18])
def test_lane_power_section(K, k):
    """Entry j of a pair is B^j: the identity, the table's own B^1 (both bitwise), and within
    1e-5, relative to its largest entry, of the fp64 power (plus 2e-38 where a contracting B's
    power leaves the fp32 normal range).  A sanity bound: at most three chained fp32 products
    of the table's rounded B^1 .. B^8, about 5e-6 on this grid when the same products are
    rounded on the host; the bits themselves are the golden test's business."""
    dev = torch.device("cuda:0")
    grid = gb.dev_grid("default64", dev)
    gcpu = _GRID_SPECS["default64"][0].double().numpy()
    G = gcpu.shape[0]
    npairs = (G + 1) // 2
    size, pw0, lp0, total = K.pair_table_sections(G, k)
    t = K.pair_table(grid, k)
    torch.cuda.synchronize()
    tab = t.cpu()
    assert tab.numel() == total
    host = torch.from_numpy(K.pair_table_host(gcpu, k))
    assert torch.equal(tab[:lp0].view(torch.int32), host[:lp0].view(torch.int32))   # the device wrote its section only
    lp = tab[lp0:].view(npairs, 16, 4, 2)
    rows = tab[:pw0].view(npairs, size)
    ident = torch.tensor([1.0, 0.0, 0.0, 1.0]).view(4, 1).expand(4, 2).contiguous()
    for p in range(npairs):
        assert torch.equal(lp[p, 0].contiguous().view(torch.int32), ident.view(torch.int32)), p
        b1 = rows[p, 6 + 4 * k:6 + 4 * k + 8].view(4, 2)
        assert torch.equal(lp[p, 1].contiguous().view(torch.int32), b1.contiguous().view(torch.int32)), p
        for comp in range(2):
            al, be, _ga = gcpu[2 * p + comp]
            c2 = al * be
            c1 = al + c2
            B = np.linalg.matrix_power(np.array([[1 - c1, 1.0], [-c2, 1.0]]), k)
            for j in range(16):
                want = np.linalg.matrix_power(B, j).reshape(4)
                got = lp[p, j, :, comp].double().numpy()
                assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() + 2e-38, (p, comp, j)


def test_a_fresh_grid_object_fits_to_the_same_bits(K, monkeypatch):
    """A grid tensor created after the first fit (the per-grid caches miss: a new table, a
    new fill) gives the bits of the first."""
    dev = torch.device("cuda:0")
    monkeypatch.setenv("FOREMAST_HW_PRUNE", "1")
    monkeypatch.setenv("FOREMAST_HW_SHARE", "1")
    m, T, hmax, N = 1440, 10080, 10, 5
    grid = gb.dev_grid("default64", dev)
    y = gb.series(N, T, m)
    ring = torch.tensor(y, device=dev).to(torch.bfloat16)
    spec = gb.detect_spec(K, y, dev, hmax)
    K.hw_clear_gap_flags()
    best = _hints("none", N, grid.shape[0], dev)
    first = gb.fit(K, ring, T, m, grid, spec, best, hmax)
    fresh = _GRID_SPECS["default64"][0].to(dev).contiguous()
    assert fresh.data_ptr() != grid.data_ptr()
    for cache in (K._PAIR_TAB_CACHE, K._GRID_QUADS_CACHE):         # an entry of a freed tensor at this address
        for key in [key for key in cache if key[0] == fresh.data_ptr()]:
            del cache[key]
    again = gb.fit(K, ring, T, m, fresh, spec, best, hmax)
    assert any(key[0] == fresh.data_ptr() for key in K._PAIR_TAB_CACHE)
    assert _same_bits(first, again)
