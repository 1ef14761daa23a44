"""FOREMAST_DTYPE: ``BrainConfig.ring_dtype``, the engines that take their ring dtype from it,
and the case fp32 rings are for, on the fp64 reference alone: a steady gauge whose level
puts bf16's step above its noise (the numbers of docs/SCORING.md "Ring precision" are this
test's printout)."""

import numpy as np
import pytest
import torch

from foremast_amd.models import smoothing as sm_ref
from foremast_amd.utils.config import BrainConfig

GRID = sm_ref.make_grid(sm_ref.MODE_HW, (0.1, 0.3, 0.5, 0.8), (0.0, 0.01, 0.05, 0.1), (0.05, 0.1, 0.3, 0.5))
GAUGE_SEED = 11


def steady_gauge(level=3000.0, amp=10.0, noise=1.0, m=288, seasons=7, N=16, seed=GAUGE_SEED, extra=0,
                 clean=False):
    """N series at ``level`` with a daily sine of amplitude ``amp`` and N(0, noise) noise,
    float32 [N, seasons * m + extra]; ``clean``: the same without the noise (float64)."""
    rng = np.random.default_rng(seed)
    T = seasons * m + extra
    t = np.arange(T)
    phase = rng.uniform(0, 2 * np.pi, (N, 1))
    sig = level + amp * np.sin(2 * np.pi * t / m + phase)
    eps = rng.normal(0, noise, (N, seasons * m + 64))[:, :T]
    return sig if clean else (sig + eps).astype(np.float32)


def test_ring_dtype_table():
    cfg = BrainConfig()
    assert cfg.dtype == "bf16"
    assert cfg.ring_dtype("cuda:0") == torch.bfloat16 and cfg.ring_dtype(torch.device("cuda")) == torch.bfloat16
    assert cfg.ring_dtype("cpu") == torch.float32
    cfg.dtype = "fp32"
    assert cfg.ring_dtype("cuda:0") == torch.float32 and cfg.ring_dtype("cpu") == torch.float32
    cfg.dtype = "fp16"
    with pytest.raises(ValueError):
        cfg.ring_dtype("cpu")


def test_from_env_parses_and_rejects_dtype():
    assert BrainConfig.from_env({}).dtype == "bf16"
    assert BrainConfig.from_env({"FOREMAST_DTYPE": "fp32"}).ring_dtype("cuda") == torch.float32
    assert BrainConfig.from_env({"FOREMAST_DTYPE": " BF16 "}).ring_dtype("cuda") == torch.bfloat16
    for bad in ("fp16", "float32", "fp8"):
        with pytest.raises(ValueError, match="FOREMAST_DTYPE"):
            BrainConfig.from_env({"FOREMAST_DTYPE": bad})


class _Float64Rings(BrainConfig):
    """On the CPU both settings give float32: a config whose ring dtype is one no engine
    defaults to shows that the engines ask the config."""

    def ring_dtype(self, device):
        return torch.float64


@pytest.mark.parametrize("cfg,want", [(BrainConfig(), torch.float32), (BrainConfig(dtype="fp32"), torch.float32),
                                      (_Float64Rings(), torch.float64)], ids=["bf16", "fp32", "asks-config"])
def test_engines_take_the_ring_dtype_from_the_config(cfg, want):
    from foremast_amd.brain.lstm_monitor import LstmMonitor
    from foremast_amd.brain.rollout import RolloutMonitor
    from foremast_amd.brain.streaming import StreamingMonitor
    from foremast_amd.store import MemoryJobStore
    prom = object()  # never queried
    sm = StreamingMonitor(MemoryJobStore(), cfg, prom=prom, device="cpu", ring_len=2880, min_capacity=4)
    shard = sm._new_shard(4)
    assert shard.spec.dtype == want and shard.hist.data.dtype == want
    ro = RolloutMonitor(MemoryJobStore(), cfg, prom=prom, device="cpu", ring_len=2880, min_capacity=4)
    assert ro.history.dtype == want
    lm = LstmMonitor(MemoryJobStore(), cfg, prom=prom, device="cpu", ring_len=2880, min_capacity=4)
    assert lm.history.dtype == want


def test_restored_snapshot_keeps_its_ring_dtype(tmp_path, caplog):
    """A shard that is already resident (a restored snapshot) keeps its ring dtype when the
    monitor grows it, whatever FOREMAST_DTYPE says now."""
    from foremast_amd.brain.streaming import StreamingMonitor
    from foremast_amd.store import MemoryJobStore
    sm = StreamingMonitor(MemoryJobStore(), _Float64Rings(), prom=object(), device="cpu", ring_len=2880,
                          min_capacity=4)
    sm._grow(4)
    assert sm.shard.spec.dtype == torch.float64
    sm.cfg = BrainConfig()                               # the configured dtype changes (float32 on the CPU)
    sm._grow(8)
    assert sm.shard.spec.dtype == torch.float64 and sm.shard.hist.data.dtype == torch.float64


def _reference_on(y, clean_next, m):
    """(sigma [N], worst |forecast - noiseless truth| over the next 8 steps [N]) of the fp64
    reference fitted on the values y."""
    ref = sm_ref.fit_smoothing(torch.tensor(y, dtype=torch.float64), sm_ref.MODE_HW, GRID.double(), m=m)
    f = sm_ref.forecast(ref, torch.arange(1, 9)).numpy()
    return ref.sigma.numpy(), np.abs(f - clean_next).max(1)


@pytest.mark.parametrize("level,amp,noise,floor", [(3000.0, 10.0, 1.0, 1.96), (1000.0, 5.0, 0.5, None)],
                         ids=["level3000", "level1000"])
def test_bf16_rounding_doubles_sigma_of_a_steady_gauge(level, amp, noise, floor):
    """bf16 carries 8 significant bits: its step is 16 at 3000 and 4 at 1000 (a rounding
    error of std step / sqrt(12) = 4.6 and 1.2), above the gauge's own noise.  The reference
    fitted on the rounded values reports a sigma about twice the one on the fp32 values and
    forecasts several true sigmas off.  tests/test_hw_fp32_ring_gpu.py asserts a ratio of 1.9
    between the two kernels at level 3000: the reference must give >= 1.96 for the seed."""
    m = 288
    y = steady_gauge(level, amp, noise)
    nxt = steady_gauge(level, amp, noise, extra=8, clean=True)[:, -8:]
    yb = torch.tensor(y).to(torch.bfloat16).float().numpy()
    s32, e32 = _reference_on(y, nxt, m)
    s16, e16 = _reference_on(yb, nxt, m)
    ratio = s16 / s32
    print(f"level {level:g} amp {amp:g} noise {noise:g}: fp32 sigma {s32.min():.2f}..{s32.max():.2f} "
          f"worst 8-step error {e32.max():.1f}; bf16 sigma {s16.min():.2f}..{s16.max():.2f} "
          f"worst 8-step error {e16.max():.1f}; sigma ratio {ratio.min():.2f}..{ratio.max():.2f}")
    assert (s32 < 1.35 * noise).all()                    # the fp32 values: sigma is the noise (G = 64 grid)
    if floor is not None:
        assert ratio.min() >= floor
    else:
        assert ratio.min() > 1.3                         # step 4 at 1000: rounding std 1.15 on noise 0.5
    assert e16.max() > 2 * e32.max()
