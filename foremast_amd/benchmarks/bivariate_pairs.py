"""Timing of the streaming shard's joint bivariate launch (``ops/csrc/bivariate_pairs.hip``).

``python -m foremast_amd.benchmarks.bivariate_pairs OUT.json [--series N ...] [--calls K]``

Per ``--series`` N: ``bivariate_pairs`` over N / 2 disjoint row pairs of a seeded synthetic
bf16 ring of N x 10,080 samples (full ring, W = 10, P = 1, with the shard's verdicts, per-app
counters and anomaly list attached), against ``window_stats`` (K1, which reads the same
bytes once) on the same ring, alternated in the same process: median over ``--rounds`` of
the time per call from device events around ``--calls`` calls after warm-up.

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


def _shape(K, N: int, calls: int, warmup: int, rounds: int, dev) -> Dict:
    from ..brain.engine import synthetic_history
    ring = synthetic_history(N, T, M, dev, seed=SEED, dtype=torch.bfloat16)
    cur = ring[:, T - W:].float().contiguous()
    thr = torch.full((N,), 3.0, device=dev)
    spec = K.DetectSpec(horizons=torch.arange(1, W + 1, dtype=torch.int32, device=dev), threshold=thr,
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur, min_valid=60)
    pairs = torch.arange(N - N % 2, dtype=torch.int32, device=dev).view(-1, 2)
    verdict = torch.zeros(N, dtype=torch.int8, device=dev)
    app_id = (torch.arange(N, device=dev) % 1024).int()
    stats = torch.zeros((1024, 2), dtype=torch.int32, device=dev)
    ab = K.AnomalyBuffer(4 * N, dev)
    out_w: Dict[str, torch.Tensor] = {}
    out_j: Dict[str, torch.Tensor] = {}

    def k1():
        K.window_stats(ring, 0, T, spec, out=out_w)

    def joint():
        K.bivariate_pairs(ring, 0, T, pairs, cur, 1, W, thr, min_valid=60, verdict=verdict, app_id=app_id,
                          app_stats=stats, anomalies=ab, out=out_j)
    for _ in range(warmup):
        k1()
        joint()
    torch.cuda.synchronize()
    w_ms, j_ms = [], []
    for _ in range(rounds):
        w_ms.append(_timed(k1, calls))
        j_ms.append(_timed(joint, calls))
    w, j = sorted(w_ms)[rounds // 2], sorted(j_ms)[rounds // 2]
    nbytes = N * T * 2
    res = {"series": N, "pairs": int(pairs.shape[0]), "T": T, "W": W, "P": 1, "rounds": rounds, "calls_per_round": calls,
           "window_stats_ms": w, "bivariate_pairs_ms": j, "ratio": j / w, "ring_bytes": nbytes,
           "window_stats_gb_per_s": nbytes / w * 1e-6, "bivariate_pairs_gb_per_s": nbytes / j * 1e-6,
           "window_stats_ms_all": w_ms, "bivariate_pairs_ms_all": j_ms,
           "pair_verdicts": [int((out_j["verdict"] == v).sum()) for v in (1, 0, -1)]}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out", help="path of the JSON result")
    p.add_argument("--series", type=int, nargs="+", default=[100_000, 12_500])
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("foremast_amd.benchmarks.bivariate_pairs needs a GPU", file=sys.stderr)
        return 2
    from ..ops import build
    from ..ops import kernels as K
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.basename(build.lib_path()),
           "shapes": [_shape(K, n, max(args.calls, 1), args.warmup, args.rounds, dev) for n in args.series]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
