"""Timing of the median / MAD scorer's kernel (``ops/csrc/robust.hip``).

``python -m foremast_amd.benchmarks.robust OUT.json [--series N ...] [--calls K]``

Per ``--series`` N, ring type and ``--lengths`` L: ``robust_stats`` over the last L samples of a
seeded synthetic ring of N x 10,080 samples (W = 10, band and verdicts attached), against ``window_stats`` (K1, which
reads the same bytes once and does no selection) on the same ring, alternated in the same
process: median over ``--rounds`` of the time per call from device events around ``--calls``
calls after warm-up.  The kernel stages a window of these lengths in LDS, so it reads each
window from HBM once: ``window_bytes`` is its HBM read traffic by construction (no counter
run here).

Needs a GPU (exit status 2 without one).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Callable, Dict

import torch

T, M, W = 10080, 1440, 10
SEED = 20241


def _timed(fn: Callable[[], None], calls: int) -> float:
    """Milliseconds per call: device events around ``calls`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _shape(K, N: int, dtype, L: int, calls: int, warmup: int, rounds: int, dev) -> Dict:
    from ..brain.engine import synthetic_history
    ring = synthetic_history(N, T, M, dev, seed=SEED, dtype=dtype)
    cur = ring[:, T - W:].float().contiguous()
    spec = K.DetectSpec(horizons=torch.arange(1, W + 1, dtype=torch.int32, device=dev),
                        threshold=torch.full((N,), 3.0, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur, min_valid=60)
    out_w: Dict[str, torch.Tensor] = {}
    out_r: Dict[str, torch.Tensor] = {}

    def k1():
        K.window_stats(ring, T - L, L, spec, out=out_w)

    def rb():
        K.robust_stats(ring, T - L, L, spec, out=out_r)
    for _ in range(warmup):
        k1()
        rb()
    torch.cuda.synchronize()
    w_ms, r_ms = [], []
    for _ in range(rounds):
        w_ms.append(_timed(k1, calls))
        r_ms.append(_timed(rb, calls))
    w, r = sorted(w_ms)[rounds // 2], sorted(r_ms)[rounds // 2]
    row = L * ring.element_size()   # bytes of a row's window
    res = {"series": N, "dtype": str(dtype).split(".")[-1], "T": T, "window": L, "W": W, "rounds": rounds,
           "calls_per_round": calls, "window_stats_ms": w, "robust_stats_ms": r, "ratio": r / w,
           "window_row_bytes": row, "window_bytes": N * row,
           "window_stats_gb_per_s": N * row / w * 1e-6, "robust_stats_gb_per_s": N * row / r * 1e-6,
           "window_stats_ms_all": w_ms, "robust_stats_ms_all": r_ms,
           "fallback_rows": int((out_r["mad"] == 0).sum())}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out", help="path of the JSON result")
    p.add_argument("--series", type=int, nargs="+", default=[100_000, 12_500])
    p.add_argument("--lengths", type=int, nargs="+", default=[T, 60],
                   help="window lengths: the whole ring (robust_average_all) and FOREMAST_MA_WINDOW's default")
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("foremast_amd.benchmarks.robust needs a GPU", file=sys.stderr)
        return 2
    from ..ops import build
    from ..ops import kernels as K
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.basename(build.lib_path()),
           "shapes": [_shape(K, n, dt, ln, max(args.calls, 1), args.warmup, args.rounds, dev)
                      for n in args.series for dt in (torch.bfloat16, torch.float32) for ln in args.lengths]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
