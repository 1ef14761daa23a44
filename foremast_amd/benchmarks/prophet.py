"""Timing of the window-scaled prophet scorer (``ops/csrc/prophet.hip``).

``python -m foremast_amd.benchmarks.prophet OUT.json [--series N] [--calls K]``

* the product shape: ``prophet_score`` over a seeded synthetic bf16 ring of N x 10,080
  samples (m = 1440, 10 current points) for a dense ring, i.i.d. misses at 1e-3 and one
  contiguous 20 % outage per series: time per call from device events around ``--calls``
  calls (after warm-up, one synchronise at the end), with the HBM bytes and VALU FMAs per
  second that the shapes imply;
* against the torch path (``models/prophet_lite.py`` ``fit_prophet`` + ``forecast`` +
  ``models/detect.py`` ``detect`` on the GPU, the only device path this model had) at
  B = 2048 x 10,080, alternated with ``prophet_score`` at the same B in the same process.

* ``--admission``: ``prophet_fit_state`` (the resident rollout engine's admission fit: the
  same launches without the detection epilogue, plus the forecast-state kernel) against
  ``prophet_score`` on the same rows, alternated.

Needs a GPU (exit status 2 without one).
"""

from __future__ import annotations

import argparse
import json
import sys
from typing import Callable, Dict, List

import torch

T, M, C = 10080, 1440, 10
SEED = 20240


def _ring(N: int, kind: str, dev) -> torch.Tensor:
    """Seeded synthetic ring ``[N, T]`` bf16: ``dense``, ``miss`` (i.i.d. 1e-3) or ``outage``
    (every series loses one contiguous fifth of the window)."""
    from ..brain.engine import synthetic_history
    ring = synthetic_history(N, T, M, dev, seed=SEED, dtype=torch.bfloat16)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED + 1)
    nan = torch.tensor(float("nan"), dtype=torch.bfloat16, device=dev)
    for s in range(0, N, 8192):
        e = min(N, s + 8192)
        if kind == "miss":
            ring[s:e] = torch.where(torch.rand((e - s, T), generator=g, device=dev) < 1e-3, nan, ring[s:e])
        elif kind == "outage":
            a = torch.randint(0, T - T // 5, (e - s, 1), generator=g, device=dev)
            t = torch.arange(T, device=dev)[None]
            ring[s:e] = torch.where((t >= a) & (t < a + T // 5), nan, ring[s:e])
    return ring


def _spec(K, N: int, dev, cur: torch.Tensor):
    return K.DetectSpec(horizons=torch.arange(1, C + 1, dtype=torch.int32, device=dev),
                        threshold=torch.full((N,), 3.0, device=dev),
                        bound=torch.full((N,), 3, dtype=torch.int8, device=dev),
                        min_lower=torch.full((N,), -1e30, device=dev), cur=cur, min_valid=60, max_horizon=C)


def _timed(fn: Callable[[], None], calls: int) -> float:
    """Milliseconds per call: device events around ``calls`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _product(K, N: int, calls: int, warmup: int, dev) -> List[Dict]:
    rows = []
    for kind in ("dense", "miss", "outage"):
        ring = _ring(N, kind, dev)
        cur = ring[:, T - C:].float().contiguous()
        spec = _spec(K, N, dev, cur)
        out: Dict[str, torch.Tensor] = {}

        def tick():
            K.prophet_score(ring, 0, T, M, spec, out=out)
        for _ in range(warmup):
            tick()
        torch.cuda.synchronize()
        ms = _timed(tick, calls)
        PP = out["_beta"].shape[1]
        gapped = float((out["nvalid"] < T).float().mean())
        hbm = N * T * 2 * 2 + N * out["_mask"].shape[1] * 4 * (1 + gapped)  # two ring passes + the mask
        fma = N * T * PP * 2                                               # rhs + residual pass
        rows.append({"input": kind, "series": N, "T": T, "m": M, "terms": PP, "ms_per_call": ms,
                     "us_per_series": 1e3 * ms / N, "gapped_frac": gapped, "hbm_bytes": hbm,
                     "hbm_gb_per_s": hbm / ms * 1e-6, "fma": fma, "tfma_per_s": fma / ms * 1e-9,
                     "verdicts": [int((out["verdict"] == v).sum()) for v in (1, 0, -1)]})
        print(json.dumps(rows[-1]), flush=True)
        del ring, cur, spec, out
        torch.cuda.empty_cache()
    return rows


def _versus_torch(K, B: int, calls: int, warmup: int, rounds: int, dev) -> Dict:
    from ..models import detect as det_ref
    from ..models import prophet_lite as pl
    ring = _ring(B, "dense", dev)
    cur = ring[:, T - C:].float().contiguous()
    spec = _spec(K, B, dev, cur)
    out: Dict[str, torch.Tensor] = {}
    step = torch.full((B,), 60.0, device=dev)
    end = torch.full((B,), 1.7e9, device=dev, dtype=torch.float64)
    ts = end[:, None] + torch.arange(1, C + 1, device=dev, dtype=torch.float64)[None] * 60.0
    hist = ring.float()

    def kernel():
        K.prophet_score(ring, 0, T, M, spec, out=out)

    def torch_path():
        fit = pl.fit_prophet(hist, end, step)
        f = pl.forecast(fit, ts)
        return det_ref.detect(f, fit.sigma, cur, spec.threshold, spec.bound, spec.min_lower,
                              model_ok=fit.n_valid >= spec.min_valid)
    for _ in range(warmup):
        kernel()
    d = torch_path()
    torch.cuda.synchronize()
    agree = float((d.verdict == out["verdict"]).float().mean())
    k_ms, t_ms = [], []
    for _ in range(rounds):  # alternate the two paths
        t_ms.append(_timed(torch_path, 1))
        k_ms.append(_timed(kernel, calls))
    k, t = sorted(k_ms)[len(k_ms) // 2], sorted(t_ms)[len(t_ms) // 2]
    res = {"series": B, "T": T, "rounds": rounds, "kernel_calls_per_round": calls,
           "kernel_ms": k, "torch_ms": t, "kernel_us_per_series": 1e3 * k / B, "torch_us_per_series": 1e3 * t / B,
           "speedup": t / k, "kernel_ms_all": k_ms, "torch_ms_all": t_ms, "verdict_agreement": agree}
    print(json.dumps(res), flush=True)
    return res


def _admission(K, N: int, calls: int, warmup: int, rounds: int, dev) -> List[Dict]:
    """The rollout engine's admission fit (``prophet_fit_state``: fit + forecast state, no
    detection) against ``prophet_score`` on the same rows, alternated in one process."""
    rows = []
    for kind in ("dense", "miss", "outage"):
        ring = _ring(N, kind, dev)
        cur = ring[:, T - C:].float().contiguous()
        spec = _spec(K, N, dev, cur)
        out_s: Dict[str, torch.Tensor] = {}
        out_f: Dict[str, torch.Tensor] = {}

        def score():
            K.prophet_score(ring, 0, T, M, spec, out=out_s)

        def fit_state():
            K.prophet_fit_state(ring, 0, T, M, out=out_f)
        for _ in range(warmup):
            score()
            fit_state()
        torch.cuda.synchronize()
        s_ms, f_ms = [], []
        for _ in range(rounds):
            s_ms.append(_timed(score, calls))
            f_ms.append(_timed(fit_state, calls))
        same = all(torch.equal(out_s[k].view(torch.int32), out_f[k].view(torch.int32))
                   for k in ("_beta", "sigma", "nvalid"))
        rows.append({"input": kind, "series": N, "T": T, "m": M, "rounds": rounds, "calls_per_round": calls,
                     "prophet_score_ms": sorted(s_ms)[rounds // 2], "prophet_fit_state_ms": sorted(f_ms)[rounds // 2],
                     "prophet_score_ms_all": s_ms, "prophet_fit_state_ms_all": f_ms, "same_bits": same})
        print(json.dumps(rows[-1]), flush=True)
        del ring, cur, spec, out_s, out_f
        torch.cuda.empty_cache()
    return rows


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("out", help="path of the JSON result")
    p.add_argument("--series", type=int, default=100_000)
    p.add_argument("--batch", type=int, default=2048, help="series of the comparison with the torch path")
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--skip-product", action="store_true")
    p.add_argument("--skip-torch", action="store_true")
    p.add_argument("--admission", action="store_true",
                   help="also time prophet_fit_state (the rollout engine's admission fit) against prophet_score "
                        "on --series rows, alternated")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        print("foremast_amd.benchmarks.prophet needs a GPU", file=sys.stderr)
        return 2
    from ..ops import kernels as K
    dev = torch.device("cuda")
    res: Dict[str, object] = {"device": torch.cuda.get_device_name(dev), "calls": args.calls, "warmup": args.warmup}
    if not args.skip_product:
        rows = _product(K, args.series, max(args.calls, 1), args.warmup, dev)
        res["product"] = rows
        dense = next(r for r in rows if r["input"] == "dense")["ms_per_call"]
        res["miss_over_dense"] = next(r for r in rows if r["input"] == "miss")["ms_per_call"] / dense
        res["outage_over_dense"] = next(r for r in rows if r["input"] == "outage")["ms_per_call"] / dense
    if not args.skip_torch:
        res["versus_torch"] = _versus_torch(K, args.batch, max(args.calls, 1), args.warmup, args.rounds, dev)
    if args.admission:
        res["admission"] = _admission(K, args.series, max(args.calls, 1), args.warmup, args.rounds, dev)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
