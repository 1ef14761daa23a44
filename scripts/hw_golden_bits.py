#!/usr/bin/env python3
"""Bits of the Holt-Winters variant-5 fit, for ``tests/golden/hw_parent_bits.npz``.

    python scripts/hw_golden_bits.py [--out tests/golden/hw_parent_bits.npz]

writes what the library this checkout loads computes (level, trend, sigma, best, the
forecast's seasonal phases and the verdict) on the cases of ``tests/test_hw_setup_gpu.py``:
the inputs are ``tests.test_kernels_gpu._series``, so the file holds outputs only.  Run it
from a checkout of the reference commit built in place (copy this file into its ``scripts/``):
the script imports the package and the test helpers of the checkout it lies in.  A library of
the reference commit in ``FOREMAST_HIP_LIB`` under this checkout's Python does not load once
an entry point was added since (``fm_hw_lane_powers`` was).  The test then holds a later
build to these bits; ``profiles/hw_setup/README.md`` records how the committed file was made.

A case is (season, window, grid, N); its outputs do not depend on the hint pairs or on the
split tail (the branch and bound is exact in any order), so they are stored once per case and
the script checks that every (hints, split) setting gave them.  A setting that did not is
stored under its own key, which the test prefers.  The file holds one array per output, the
cases' series stacked in the order of ``rows()`` (season_hb padded to 10 columns).
"""

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from foremast_amd.models import smoothing as sm_ref  # noqa: E402
from tests.test_hw_share import _GRID_SPECS, _hints  # noqa: E402
from tests.test_kernels_gpu import _series  # noqa: E402

# (name, season, window, max horizon, FOREMAST_HW_QUAD).  1440: hw_d_kernel<45> with no fused
# season, one, and the product's six; 288: hw_q_kernel<18> (its gapped pairs at K = 9), and
# hw_d_kernel<9> with the quad layout off (hmax <= K there)
CASES = (
    ("m1440_T2880", 1440, 2880, 10, "1"),
    ("m1440_T4320", 1440, 4320, 10, "1"),
    ("m1440_T10080", 1440, 10080, 10, "1"),
    ("m288_T2016", 288, 2016, 10, "1"),
    ("m288_T2016_k9", 288, 2016, 9, "0"),
)
GRIDS = ("default64", "4x4x3")
NS = (1, 2, 5, 9)
HINTS = ("none", "same", "quads", "siblings")
SPLITS = ("1", "0")
ARRAYS = ("level", "trend", "sigma", "best", "season_hb", "verdict")
_DEV_GRIDS = {}


def dev_grid(name, dev):
    """One device tensor per grid for the process: the kernels' per-grid caches are keyed by
    the device pointer."""
    if name not in _DEV_GRIDS:
        _DEV_GRIDS[name] = _GRID_SPECS[name][0].to(dev).contiguous()
    return _DEV_GRIDS[name]


def series(N, T, m, scale=1.0):
    y = _series(N, T, m, seed=100 + N)
    y[N // 2] = 7.0                                    # a constant series: every SSE ties at 0
    return (y * np.float32(scale)).astype(np.float32)


def detect_spec(K, y, dev, hmax):
    N = y.shape[0]
    hz = torch.arange(1, hmax + 1, dtype=torch.int32).repeat(2)
    cur = torch.tensor(np.nan_to_num(y[:, -2 * hmax:], nan=20.0) * 1.04, device=dev)
    return K.DetectSpec(horizons=hz.to(dev), threshold=torch.full((N,), 2.0, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur, max_horizon=hmax)


def fit(K, ring, T, m, grid, spec, best, hmax):
    """One variant-5 fit with deferred detection from the hints in ``best``; the arrays of
    ARRAYS as they left the device (season_hb: the phases the fit writes)."""
    out = {"best": best.clone()}
    out = K.smoothing_fit(ring, 0, T, sm_ref.MODE_HW, m, grid, spec, variant=5, out=out, defer_detect=True)
    assert K.last_hw_variant == 5 and K.last_detect_deferred
    K.hw_detect_deferred(out, spec, T, m, grid=grid)
    torch.cuda.synchronize()
    res = {k: out[k].clone() for k in ARRAYS}
    res["season_hb"] = res["season_hb"][:, :hmax].contiguous()
    return res


def bits(t):
    """The raw bits of a result tensor (floats as int32: a NaN or a signed zero counts)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def rows():
    """(case name, grid name, N) -> first row of the case in the stacked arrays."""
    at, r = {}, 0
    for case in CASES:
        for gname in GRIDS:
            for N in NS:
                at[(case[0], gname, N)] = r
                r += N
    return at


def settings():
    for split in SPLITS:
        for kind in HINTS:
            yield split, kind


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hw_parent_bits.npz"))
    args = ap.parse_args()
    from foremast_amd.ops import _native, kernels as K
    _native.require()
    dev = torch.device("cuda:0")
    os.environ["FOREMAST_HW_PRUNE"] = "1"
    os.environ["FOREMAST_HW_SHARE"] = "1"
    stack = {k: [] for k in ARRAYS}
    store = {}
    odd = 0
    for name, m, T, hmax, quad in CASES:
        os.environ["FOREMAST_HW_QUAD"] = quad
        for gname in GRIDS:
            grid = dev_grid(gname, dev)
            G = grid.shape[0]
            for N in NS:
                K.hw_clear_gap_flags()
                y = series(N, T, m)
                ring = torch.tensor(y, device=dev).to(torch.bfloat16)
                spec = detect_spec(K, y, dev, hmax)
                base = f"{name}|{gname}|N{N}"
                first = None
                for split, kind in settings():
                    os.environ["FOREMAST_HW_SPLIT"] = split
                    res = fit(K, ring, T, m, grid, spec, _hints(kind, N, G, dev), hmax)
                    if first is None:
                        first = res
                        for k in ARRAYS:
                            b = bits(res[k]).numpy()
                            if k == "season_hb":
                                b = np.pad(b, ((0, 0), (0, 10 - b.shape[1])))
                            stack[k].append(b)
                    elif not all(torch.equal(bits(res[k]), bits(first[k])) for k in ARRAYS):
                        odd += 1
                        for k in ARRAYS:
                            store[f"{base}|split{split}|{kind}|{k}"] = bits(res[k]).numpy()
    store.update({k: np.concatenate(v) for k, v in stack.items()})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **store)
    print(f"{args.out}: {len(store)} arrays, {os.path.getsize(args.out)} bytes, "
          f"{odd} settings that differ from their case's first")


if __name__ == "__main__":
    main()
