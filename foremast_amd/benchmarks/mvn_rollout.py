"""Timing of the rollout engine's k-variate normal kernels (``ops/csrc/mvn_state.hip``).

``python -m foremast_amd.benchmarks.mvn_rollout OUT.json [--groups G] [--k K ...] [--calls C]``

Per ring dtype (bf16, fp32) and ``--k``: G disjoint groups of k consecutive rows of a seeded
synthetic ring of 8 G x 10,080 samples, windows of P = 5 pods x Wc = 11 slots.

(a) ``mvn_state_detect`` over the G fitted states per call, against ``mvn_groups`` on the same
    groups, ring and windows: what scoring a tick costs from the state, and what refitting the
    week every tick would cost.
(b) ``mvn_fit_state`` with three distinct window lengths (R, R - 1, R - 2: jobs started over
    three minutes) in one launch, against one ``mvn_groups`` launch per distinct length over
    the groups of that length (the per-length loop of the engine's other admission fits).

The compared launches are alternated round by round in one process.  Per kernel: the time per
call from device events around ``--calls`` calls after warm-up, as median, minimum and maximum
over ``--rounds``, and the bytes the kernel reads over the median.

Needs a GPU (exit status 2 without one).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Callable, Dict, List

import torch

T, M, P, WC = 10080, 1440, 5, 11
SEED = 20242
MAXK = 8
STATE_WORDS = 8 + 36 + 1 + 1 + 8   # mean, chol, nvalid, thr2 and the group's rows, per state row


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
    return {"ms": med, "ms_min": s[0], "ms_max": s[-1], "ms_all": ms, "bytes_read": nbytes,
            "gb_per_s": nbytes / med * 1e-6}


def _dtype(K, ring_dtype: str, G: int, ks: List[int], calls: int, warmup: int, rounds: int, dev) -> Dict:
    from ..brain.engine import synthetic_history
    from ..models.multivariate_normal import chi2_threshold
    dtype = torch.bfloat16 if ring_dtype == "bf16" else torch.float32
    N = MAXK * G
    ring = synthetic_history(N, T, M, dev, seed=SEED, dtype=dtype)
    g = torch.Generator(device="cpu").manual_seed(SEED)
    last = ring[:, T - WC:].float()
    cur = (last[:, None, :] * (1.0 + 0.01 * torch.randn((1, P, 1), generator=g).to(dev))).reshape(N, P * WC).contiguous()
    thr = torch.full((N,), 3.0, device=dev)
    elem = ring.element_size()
    lens3 = (T, T - 1, T - 2)
    fns: Dict[str, Callable[[], None]] = {}
    nbytes: Dict[str, int] = {}
    keep: Dict[int, Dict] = {}
    for k in ks:
        table = torch.full((G, MAXK), -1, dtype=torch.int32)
        table[:, :k] = torch.arange(k * G, dtype=torch.int32).view(G, k)
        table = table.to(dev)
        thr2 = torch.full((G,), chi2_threshold(3.0, k), device=dev)
        ident = torch.arange(G, dtype=torch.int32, device=dev)
        state = K.mvn_state_tables(G, dev)
        full = torch.full((G,), T, dtype=torch.int32, device=dev)
        mixed = torch.tensor(lens3, dtype=torch.int32, device=dev)[ident.long() % 3].contiguous()
        parts = [(ln, table[(ident % 3) == j].contiguous(), thr2[(ident % 3) == j].contiguous())
                 for j, ln in enumerate(lens3)]
        K.mvn_fit_state(ring, 0, table, full, ident, state, kmask=1 << k)
        o_det: Dict[str, torch.Tensor] = {}
        o_grp: Dict[str, torch.Tensor] = {}
        o_part: List[Dict[str, torch.Tensor]] = [{} for _ in parts]
        scratch = K.mvn_state_tables(G, dev)

        def detect(state=state, table=table, thr2=thr2, ident=ident, k=k, o=o_det):
            K.mvn_state_detect(state, table, thr2, ident, cur, P, WC, min_valid=60, kmask=1 << k, out=o)

        def refit(table=table, thr2=thr2, k=k, o=o_grp):
            K.mvn_groups(ring, 0, T, table, cur, P, WC, thr, thr2=thr2, kmask=1 << k, min_valid=60, out=o)

        def fit3(table=table, mixed=mixed, ident=ident, scratch=scratch, k=k):
            K.mvn_fit_state(ring, 0, table, mixed, ident, scratch, kmask=1 << k)

        def loop3(parts=parts, k=k, outs=o_part):
            for (ln, tb, t2), o in zip(parts, outs):
                K.mvn_groups(ring, 0, ln, tb, cur, P, WC, thr, thr2=t2, kmask=1 << k, min_valid=60, out=o)
        win_bytes = k * G * P * WC * 4
        fns.update({f"state_detect_k{k}": detect, f"mvn_groups_k{k}": refit, f"fit_state_3len_k{k}": fit3,
                    f"mvn_groups_per_len_k{k}": loop3})
        nbytes.update({f"state_detect_k{k}": win_bytes + G * STATE_WORDS * 4,
                       f"mvn_groups_k{k}": k * G * T * elem + win_bytes,
                       f"fit_state_3len_k{k}": sum(k * len(tb) * ln * elem for ln, tb, _ in parts),
                       f"mvn_groups_per_len_k{k}": sum(k * len(tb) * ln * elem + k * len(tb) * P * WC * 4
                                                       for ln, tb, _ in parts)})
        keep[k] = {"det": o_det, "grp": o_grp}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms: Dict[str, List[float]] = {name: [] for name in fns}
    for _ in range(rounds):     # alternated: every launch once per round
        for name, fn in fns.items():
            ms[name].append(_timed(fn, calls))
    res = {"dtype": ring_dtype, "groups": G, "T": T, "Wc": WC, "P": P, "lens": list(lens3), "rounds": rounds,
           "calls_per_round": calls, "kernels": {name: _stats(v, nbytes[name]) for name, v in ms.items()}, "agree": {}}
    for k in ks:   # the state scored what the fused launch scored
        a, b = keep[k]["det"], keep[k]["grp"]
        res["agree"][f"k{k}"] = {
            "max_rel_d2": float(((a["d2"] - b["d2"]).abs() / b["d2"].abs().clamp(min=1.0)).max()),
            "verdicts_equal": bool((a["verdict"] == b["verdict"]).all()),
            "verdicts": [int((a["verdict"] == v).sum()) for v in (1, 0, -1)]}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out", help="path of the JSON result")
    p.add_argument("--groups", type=int, default=20_000)
    p.add_argument("--k", type=int, nargs="+", default=[2, 3, 8])
    p.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"], choices=["bf16", "fp32"])
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--rounds", type=int, default=7)
    args = p.parse_args(argv)
    if any(not 2 <= k <= MAXK for k in args.k):
        p.error(f"--k takes values in 2..{MAXK}")
    if not torch.cuda.is_available():
        print("foremast_amd.benchmarks.mvn_rollout needs a GPU", file=sys.stderr)
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
