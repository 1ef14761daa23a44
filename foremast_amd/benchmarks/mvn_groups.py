"""Timing of the streaming shard's k-variate normal launch (``ops/csrc/mvn_groups.hip``).

``python -m foremast_amd.benchmarks.mvn_groups OUT.json [--groups G] [--k K ...] [--calls C]``

Per ring dtype (bf16, fp32): ``mvn_groups`` over G disjoint groups of k consecutive rows of a
seeded synthetic ring of 8 G x 10,080 samples (full ring, W = 10, P = 1, with the shard's
verdicts, per-app counters and anomaly list attached) at every ``--k``, against
``bivariate_pairs`` on the G pairs that are the k = 2 groups, alternated round by round in
the same process.  Per kernel: the time per call from device events around ``--calls`` calls
after warm-up, as median, minimum and maximum over ``--rounds`` (the run-to-run spread), and
the ring bytes the groups read over the median.

Needs a GPU (exit status 2 without one).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Callable, Dict, List

import torch

T, M, W = 10080, 1440, 10
SEED = 20241
MAXK = 8


def _timed(fn: Callable[[], None], calls: int) -> float:
    """Milliseconds per call: device events around ``calls`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _stats(ms: List[float], nbytes: int) -> Dict:
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"ms": med, "ms_min": s[0], "ms_max": s[-1], "ms_all": ms, "ring_bytes": nbytes,
            "gb_per_s": nbytes / med * 1e-6}


def _dtype(K, ring_dtype: str, G: int, ks: List[int], calls: int, warmup: int, rounds: int, dev) -> Dict:
    from ..brain.engine import synthetic_history
    from ..models.multivariate_normal import chi2_threshold
    dtype = torch.bfloat16 if ring_dtype == "bf16" else torch.float32
    N = MAXK * G
    ring = synthetic_history(N, T, M, dev, seed=SEED, dtype=dtype)
    cur = ring[:, T - W:].float().contiguous()
    thr = torch.full((N,), 3.0, device=dev)
    verdict = torch.zeros(N, dtype=torch.int8, device=dev)
    app_id = (torch.arange(N, device=dev) % 1024).int()
    stats = torch.zeros((1024, 2), dtype=torch.int32, device=dev)
    ab = K.AnomalyBuffer(4 * N, dev)
    elem = ring.element_size()
    pairs = torch.arange(2 * G, dtype=torch.int32, device=dev).view(-1, 2)
    out_p: Dict[str, torch.Tensor] = {}

    def pair():
        K.bivariate_pairs(ring, 0, T, pairs, cur, 1, W, thr, min_valid=60, verdict=verdict, app_id=app_id,
                          app_stats=stats, anomalies=ab, out=out_p)
    fns = {"bivariate_pairs": pair}
    nbytes = {"bivariate_pairs": 2 * G * T * elem}
    outs: Dict[int, Dict[str, torch.Tensor]] = {}
    for k in ks:
        table = torch.full((G, MAXK), -1, dtype=torch.int32)
        table[:, :k] = torch.arange(k * G, dtype=torch.int32).view(G, k)
        table = table.to(dev)
        thr2 = torch.full((G,), chi2_threshold(3.0, k), device=dev)
        outs[k] = {}

        def group(table=table, thr2=thr2, k=k):
            K.mvn_groups(ring, 0, T, table, cur, 1, W, thr, thr2=thr2, kmask=1 << k, min_valid=60, verdict=verdict,
                         app_id=app_id, app_stats=stats, anomalies=ab, out=outs[k])
        fns[f"mvn_groups_k{k}"] = group
        nbytes[f"mvn_groups_k{k}"] = k * G * T * elem
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms: Dict[str, List[float]] = {name: [] for name in fns}
    for _ in range(rounds):     # alternated: every kernel once per round
        for name, fn in fns.items():
            ab.reset()
            ms[name].append(_timed(fn, calls))
    res = {"dtype": ring_dtype, "groups": G, "T": T, "W": W, "P": 1, "rounds": rounds, "calls_per_round": calls,
           "kernels": {name: _stats(v, nbytes[name]) for name, v in ms.items()},
           "verdicts": {f"k{k}": [int((outs[k]["verdict"] == v).sum()) for v in (1, 0, -1)] for k in ks},
           "pair_verdicts": [int((out_p["verdict"] == v).sum()) for v in (1, 0, -1)]}
    if 2 in ks:   # the same pairs under both kernels: the distances agree
        a, b = outs[2]["d2"], out_p["d2"]
        res["k2_vs_pairs_max_rel_d2"] = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
    print(json.dumps(res), flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out", help="path of the JSON result")
    p.add_argument("--groups", type=int, default=10_000)
    p.add_argument("--k", type=int, nargs="+", default=[2, 4, 8])
    p.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"], choices=["bf16", "fp32"])
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=7)
    args = p.parse_args(argv)
    if any(not 2 <= k <= MAXK for k in args.k):
        p.error(f"--k takes values in 2..{MAXK}")
    if not torch.cuda.is_available():
        print("foremast_amd.benchmarks.mvn_groups needs a GPU", file=sys.stderr)
        return 2
    from ..ops import build
    from ..ops import kernels as K
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(dev), "library": os.path.basename(build.lib_path()),
           "results": [_dtype(K, d, args.groups, args.k, max(args.calls, 1), args.warmup, args.rounds, dev)
                       for d in args.dtypes]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
