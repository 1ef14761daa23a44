"""The fused LSTM-AE training pass (ops/csrc/lstm_train.hip: variant 0, one wave per 32
windows, and variant 1, two waves with a double-buffered LDS exchange; host half in
ops/lstm_train.py) against the fp64 model of helpers/lstm_bf16_ref.py, which rounds to bf16
exactly where the kernels do and which test_lstm_ref.py ties to autograd.

Every buffer the kernel leaves is compared element by element -- err, dy, the dgates of both
LSTMs, the h / x operand blocks -- and then the seven parameter gradients, on the smallest
shapes that take every branch: one group and an odd number of groups, T = 1 (backward takes
the c0 branch, enc_w_hh.grad is exactly zero), odd and even T (variant 1's exchange buffers
are indexed by t & 1), F = 1 and F = 7 (inputs at k = 64..70, next to the bias at k = 71).

Bounds (helpers/lstm_bf16_ref.py; both sides of each come from the model, never the kernel):
mean |kernel - model| <= 0.1 x mean |model(rounded) - model(unrounded)|, the 99.9th percentile
<= 0.25 x that gap's; bf16-stored buffers: no element further than 2 bf16 ulps (2^-6) plus
BF16_FLOOR x the tensor's median magnitude; gradients: ||kernel - model|| / ||model|| <= 0.25 x
the relative quantisation gap of the parameter.  Every output buffer is a leading view of a
larger one whose tail must come back untouched.

Measured on the MI355X, kernel to model as a share of the quantisation gap (mean / p99.9; the
bounds are 0.1 / 0.25), the two variants within a few percent of each other everywhere:

  shape (B, T, F)   err            dy             g_enc          g_dec          h_enc          h_dec
  (32, 1, 1)        7.5e-4/1.4e-3  1.2e-3/5.9e-3  2.7e-4/0       1.7e-4/0       0/0            6.5e-4/5.3e-3
  (32, 2, 7)        2.0e-3/8.5e-3  4.6e-4/2.9e-3  1.9e-3/7.7e-3  2.4e-3/3.3e-3  1.5e-8/0       6.6e-4/2.4e-3
  (64, 5, 3)        2.4e-3/9.1e-3  3.2e-3/4.0e-2  5.2e-3/3.6e-2  1.1e-3/4.5e-3  6.5e-5/0       1.8e-3/2.1e-2
  (96, 5, 7)        2.2e-3/7.8e-3  8.8e-4/1.1e-2  2.4e-3/2.3e-2  2.2e-4/1.7e-4  1.6e-7/0       5.6e-4/4.0e-3
  (96, 12, 2)       6.4e-3/2.7e-2  4.8e-3/3.4e-2  2.5e-2/9.1e-2  3.5e-3/1.1e-2  9.4e-4/3.9e-3  1.6e-3/2.7e-2
  (64, 5, 3) after the x1.5 weight update: g_enc 9.9e-3/1.1e-1, every other quantity below the rows above
  (64, 5, 3) ring input (fp32, bf16 rings): every buffer <= 3.3e-3/3.4e-2, gradients <= 2.1e-2

  parameter gradients (bound 0.25), largest over the seven: 4.3e-3 (T = 1), 3.9e-2 (32, 2, 7),
  1.8e-2 (64, 5, 3), 8.6e-3 (96, 5, 7), 4.4e-2 (96, 12, 2); out_b alone <= 2.9e-3
  bf16 element bound, largest excess over 2^-6 |model| in medians of the tensor: g_enc 0.197 at
  (96, 12, 2), 0.078 after the weight update, 0.030 at (64, 5, 3), below 0.02 elsewhere; g_dec
  0.015, h_enc 1.0e-3, h_dec 5.9e-4.  BF16_FLOOR = 0.4 is twice the largest (see the helper for
  where that excess comes from)
  variant 0 against variant 1: <= 3.2e-3/2.3e-2 elementwise, <= 1.0e-2 on the gradients, excess 0.039

No ratio had to be raised, and the tests found no kernel or host bug.
"""

import copy
import functools
import importlib.util
import os

import pytest
import torch

from foremast_amd.ops.lstm import BIAS_K, H, KAUG, RingSource

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "lstm_bf16_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lstm_bf16_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

GRID = [(32, 1, 1), (32, 2, 7), (64, 5, 3), (96, 5, 7), (96, 12, 2)]   # (B, T, F)
GRID_IDS = [f"B{b}-T{t}-F{f}" for b, t, f in GRID]
HOST_SHAPE = (64, 5, 3)
PAD = 259                       # sentinel elements behind every buffer
SENT = {torch.float32: -12345.5, torch.bfloat16: -768.0}
GUARDED = ("err", "dy", "g_enc", "g_dec", "h_enc", "h_dec", "scratch")


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(model, x, rounded model, unrounded model) of a grid shape: computed once, never modified."""
    m, x = R.make_case(*shape)
    p = R.params_of(m)
    return m, x, R.reference(p, x, rounding=True), R.reference(p, x, rounding=False)


def _guard(fg):
    """Replace the launcher's buffers by leading views of larger ones with a sentinel tail (the
    launcher reads data_ptr() per call).  The outputs start from the sentinel too, so a cell the
    kernel skips cannot pass; h_enc / h_dec keep the host's zero fill and their row of ones."""
    whole = {}
    for name in GUARDED:
        t = getattr(fg, name)
        w = torch.full((t.numel() + PAD,), SENT[t.dtype], dtype=t.dtype, device=t.device)
        v = w[:t.numel()].view(t.shape)
        if name in ("h_enc", "h_dec"):
            v.copy_(t)
        setattr(fg, name, v)
        whole[name] = w
    return whole


def _tails_intact(whole):
    for name, w in whole.items():
        tail = w[-PAD:]
        assert torch.equal(tail, torch.full_like(tail, SENT[w.dtype])), f"{name}: written behind its end"


def _collect(fg, model, loss):
    """The kernel's buffers and the gradients on the CPU, in the layout of R.reference."""
    F = fg.F
    torch.cuda.synchronize()
    he, hd = fg.h_enc.float().cpu(), fg.h_dec.float().cpu()
    for name, hb in (("h_enc", he), ("h_dec", hd)):
        lo = H + F if name == "h_enc" else H      # the decoder has no input rows
        assert float(hb[lo:BIAS_K].abs().max() if lo < BIAS_K else 0.0) == 0.0, f"{name}: rows {lo}..70 not zero"
        assert float(hb[BIAS_K + 1:KAUG].abs().max()) == 0.0, f"{name}: rows 72..79 not zero"
        assert bool((hb[BIAS_K] == 1.0).all()), f"{name}: row 71 is not all ones"
    return {"err": fg.err.double().cpu(), "dy": fg.dy.double().cpu(), "g_enc": fg.g_enc.double().cpu(),
            "g_dec": fg.g_dec.double().cpu(), "h_enc": he[:H + F].double(), "h_dec": hd[:H].double(),
            "grads": {n: getattr(model, n).grad.detach().double().cpu().clone() for n in R.PARAMS},
            "loss": float(loss), "loss_bits": loss.detach().cpu().clone()}


def _launch(shape, variant, model=None, x=None, ring=None, batched=True):
    from foremast_amd.ops.lstm_train import FusedLstmGrad
    B, T, F = shape
    dev = _dev()
    if model is None:
        model = copy.deepcopy(_case(shape)[0]).to(dev)
    if x is None and ring is None:
        x = _case(shape)[1].to(dev).contiguous()
    fg = FusedLstmGrad(B, T, F, dev, variant=variant)
    fg.batched_gemm = batched
    whole = _guard(fg)
    loss = fg.grads(model, x, ring)
    got = _collect(fg, model, loss)
    _tails_intact(whole)
    assert torch.equal(loss.cpu(), fg.err.mean().cpu()), "the returned loss is not err.mean()"
    return got, fg, model


@functools.lru_cache(maxsize=None)
def _kernel(shape, variant):
    """One run of a grid case, shared by the tests that look at it."""
    return _launch(shape, variant)[0]


def _check(got, rnd, unr, what):
    res = R.measure(got, rnd, unr)
    print(f"{what}: {R.fmt(res)}")
    bad = R.violations(res)
    assert not bad, f"{what}: {bad}"
    return res


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
def test_training_pass_matches_bf16_model(shape, variant):
    B, T, F = shape
    _, _, rnd, unr = _case(shape)
    got = _kernel(shape, variant)
    _check(got, rnd, unr, f"v{variant} {shape}")
    # all T + 1 blocks of h_dec were compared (block 0: the encoder's final h)
    assert got["h_dec"].shape == rnd["h_dec"].shape == (H, (T + 1) * B)
    if T == 1:
        assert float(got["grads"]["enc_w_hh"].abs().max()) == 0.0    # h_{-1} = 0: bit-exactly zero
        assert float(got["h_enc"][:H].abs().max()) == 0.0


@pytest.mark.parametrize("shape", GRID, ids=GRID_IDS)
def test_variants_agree(shape):
    """One wave and two waves per 32 windows sum the h k-steps in a different order: not
    bitwise, but within the bounds either has against the model."""
    _, _, rnd, unr = _case(shape)
    res = R.measure_pair(_kernel(shape, 0), _kernel(shape, 1), rnd, unr)
    print(f"v0 vs v1 {shape}: {R.fmt(res)}")
    bad = R.violations(res)
    assert not bad, bad


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ring_dtype", [torch.float32, torch.bfloat16], ids=["ring_fp32", "ring_bf16"])
def test_ring_input_matches_dense_and_model(ring_dtype, variant):
    """Windows read straight from the rings (row-padded storage, a non-zero device head,
    win_start in [0, 3R), eight windows that wrap) equal the dense run on the host-gathered,
    z-scored windows, and meet the model of those windows."""
    B, T, F = HOST_SHAPE
    dev = _dev()
    n, Rl, head = 40, 37, 11
    g = torch.Generator().manual_seed(21)
    store = [(torch.randn(n, 48, generator=g) * (f + 1) + f).to(ring_dtype) for f in range(F)]
    mean = torch.randn(n, F, generator=g) * 0.1
    rstd = 1.0 / (0.5 + torch.rand(n, F, generator=g))
    si = torch.randint(0, n, (B,), generator=g, dtype=torch.int32)
    st = torch.randint(0, 3 * Rl, (B,), generator=g, dtype=torch.int32)
    st[:8] = (Rl - 3 - head) % Rl + Rl * torch.arange(8, dtype=torch.int32).remainder(3)   # physical start R - 3
    cols = (head + st.long()[:, None] + torch.arange(T)[None]) % Rl
    assert int((cols[:, 0] > cols[:, -1]).sum()) >= 8
    x = torch.stack([s[:, :Rl][si.long()[:, None], cols].float() for s in store], 2)
    x = ((x - mean[si.long()][:, None]) * rstd[si.long()][:, None]).contiguous()
    m = _case(HOST_SHAPE)[0]
    p = R.params_of(m)
    rnd, unr = R.reference(p, x, rounding=True), R.reference(p, x, rounding=False)
    dense, _, _ = _launch(HOST_SHAPE, variant, x=x.to(dev))
    rings = [s.to(dev)[:, :Rl] for s in store]
    src = RingSource(rings=rings, mean=mean.to(dev), rstd=rstd.to(dev), win_series=si.to(dev), win_start=st.to(dev),
                     head_dev=torch.tensor([head], dtype=torch.int32, device=dev))
    ring, _, _ = _launch(HOST_SHAPE, variant, ring=src)
    torch.testing.assert_close(ring["err"], dense["err"], rtol=1e-5, atol=1e-6)
    assert abs(ring["loss"] - dense["loss"]) <= 1e-5 * abs(dense["loss"])
    for name in R.PARAMS:
        torch.testing.assert_close(ring["grads"][name], dense["grads"][name], rtol=1e-4, atol=1e-6)
    _check(ring, rnd, unr, f"ring v{variant} {ring_dtype}")
    _check(dense, rnd, unr, f"dense v{variant} {ring_dtype}")


def test_unbatched_gemm_meets_the_same_bounds():
    _, _, rnd, unr = _case(HOST_SHAPE)
    got, _, _ = _launch(HOST_SHAPE, 1, batched=False)
    _check(got, rnd, unr, "batched_gemm=False")


def test_cached_packer_and_scatter_follow_a_weight_update():
    """A second grads() on the same FusedLstmGrad after every parameter changed in place and the
    gradients were dropped (zero_grad(set_to_none=True)) matches the model of the NEW weights:
    neither the cached packer nor the cached scatter may hold on to anything stale."""
    _, x, rnd0, unr0 = _case(HOST_SHAPE)
    got, fg, model = _launch(HOST_SHAPE, 1)
    _check(got, rnd0, unr0, "before the update")
    with torch.no_grad():
        for prm in model.parameters():
            prm.mul_(1.5)
    model.zero_grad(set_to_none=True)
    assert all(prm.grad is None for prm in model.parameters())
    loss = fg.grads(model, x.to(_dev()).contiguous())
    got = _collect(fg, model, loss)
    p = {n: getattr(model, n).detach().cpu() for n in R.PARAMS}
    rnd, unr = R.reference(p, x, rounding=True), R.reference(p, x, rounding=False)
    _check(got, rnd, unr, "after the update")
    assert R.violations(R.measure(got, rnd0, unr0))    # and it is not the old weights' result


def test_split_launch_equals_grads():
    """pack(), launch(pack=False), finish() give the bits of grads()."""
    _, x, _, _ = _case(HOST_SHAPE)
    ref, fg, model = _launch(HOST_SHAPE, 1)
    bits = {n: getattr(model, n).grad.clone() for n in R.PARAMS}
    bufs = {n: getattr(fg, n).clone() for n in GUARDED if n != "scratch"}
    model.zero_grad(set_to_none=True)
    for n in ("err", "dy", "g_enc", "g_dec"):
        getattr(fg, n).fill_(SENT[getattr(fg, n).dtype])
    fg.pack(model)
    fg.launch(model, x.to(_dev()).contiguous(), pack=False)
    loss = fg.finish(model)
    torch.cuda.synchronize()
    assert torch.equal(loss.cpu(), ref["loss_bits"])
    for n, b in bufs.items():
        assert torch.equal(getattr(fg, n).view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), n
    for n, b in bits.items():
        assert torch.equal(getattr(model, n).grad.view(torch.int32), b.view(torch.int32)), n
