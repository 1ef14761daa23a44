"""The fp64 host model of the bf16 LSTM kernels (helpers/lstm_bf16_ref.py) is right, and the
bounds the GPU tests apply with it (test_lstm_train_gpu.py, test_lstm.py) can tell things apart.

* Without rounding the hand-written backward equals autograd of models/lstm_ae.py.
* Every compared quantity has a non-zero quantisation gap (rounded against unrounded model):
  the bounds are shares of that gap.
* Three known ways of being subtly wrong -- one rounding dropped, two gate rows of one hidden
  unit swapped, the error taken against the rounded x -- each move a compared quantity past
  its bound, while the same model run in fp32 (what a correct kernel differs by: accumulation
  noise and the rounding flips it causes) stays inside every one of them."""

import functools
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location(
    "lstm_bf16_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lstm_bf16_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

SHAPES = [(32, 1, 1), (64, 12, 3), (96, 5, 7)]   # (B, T, F)
IDS = ["B32-T1-F1", "B64-T12-F3", "B96-T5-F7"]


@functools.lru_cache(maxsize=None)
def _models(shape):
    """(params, x, rounded, unrounded), computed once per shape and never modified."""
    B, T, F = shape
    m, x = R.make_case(B, T, F)
    p = R.params_of(m)
    return m, x, R.reference(p, x, rounding=True), R.reference(p, x, rounding=False)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unrounded_model_equals_autograd(shape):
    m, x, _, unr = _models(shape)
    md = type(m)(m.F, m.H).double()
    md.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    xd = x.double()
    err = md.recon_error(xd)
    ref = torch.autograd.grad(err.mean(), list(md.parameters()))
    torch.testing.assert_close(unr["y"], md(xd).detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(unr["err"], err.detach(), rtol=1e-12, atol=1e-14)
    for (name, _), g in zip(md.named_parameters(), ref):
        got = unr["grads"][name].view_as(g)
        rel = float((got - g).norm() / g.norm()) if float(g.norm()) > 0 else float(got.norm())
        assert rel <= 1e-5, (name, rel)
    # fp32 autograd, the reference the older GPU test uses, is no further than its own rounding
    loss = m.recon_error(x).mean()
    for (name, _), g in zip(m.named_parameters(), torch.autograd.grad(loss, list(m.parameters()))):
        got = unr["grads"][name].view_as(g)
        rel = float((got - g.double()).norm() / g.double().norm()) if float(g.norm()) > 0 else float(got.norm())
        assert rel <= 1e-5, (name, rel)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_compared_quantity_has_a_quantisation_gap(shape):
    B, T, F = shape
    _, _, rnd, unr = _models(shape)
    for q in R.ELEMENTWISE + ("y",):
        assert rnd[q].shape == unr[q].shape
        assert float((rnd[q] - unr[q]).abs().mean()) > 0, q
    assert rnd["dy"].shape == (F, T * B) and rnd["g_enc"].shape == rnd["g_dec"].shape == (4 * R.H, T * B)
    assert rnd["h_enc"].shape == (R.H + F, T * B) and rnd["h_dec"].shape == (R.H, (T + 1) * B)
    for n in R.PARAMS:
        gap = float((rnd["grads"][n] - unr["grads"][n]).norm())
        if n == "enc_w_hh" and T == 1:   # h_{-1} = 0: identically zero, rounded or not
            assert gap == 0 and float(rnd["grads"][n].abs().max()) == 0
        else:
            assert gap > 0, n
    # the layout: block 0 of h_dec is the encoder's final h, the h rows of h_enc's block 0 are zero
    assert float(rnd["h_enc"][:R.H, :B].abs().max()) == 0
    if T > 1:
        assert float(rnd["h_enc"][:R.H, B:2 * B].abs().mean()) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fp32_run_of_the_model_stays_inside_every_bound(shape):
    m, x, rnd, unr = _models(shape)
    f32 = R.reference(R.params_of(m), x, rounding=True, dtype=torch.float32)
    res = R.measure(f32, rnd, unr)
    print(R.fmt(res))
    assert R.violations(res) == []
    assert abs(f32["loss"] - rnd["loss"]) <= 1e-5 * abs(rnd["loss"])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mutated_model_misses_a_bound(shape, mutation):
    B, T, F = shape
    m, x, rnd, unr = _models(shape)
    mut = R.reference(R.params_of(m), x, rounding=True, mutate=mutation)
    bad = R.violations(R.measure(mut, rnd, unr))
    print(mutation, shape, [(q, k, f"{v:.3g}") for q, k, v, _ in bad])
    if mutation == "swap_gate_rows" and T == 1:
        # W_hh of the encoder multiplies h_{-1} = 0 only: nothing to see at T = 1 (the GPU grid
        # has T = 2, 5 and 12 for it)
        assert bad == []
        return
    assert bad, f"{mutation} at {shape} passes every bound"
    # the forward-only subset that the scoring test compares (y and err) sees the two forward mutations
    if mutation != "no_dgate_round":
        fwd = R.violations(R.measure(mut, rnd, unr, names=("y", "err"), grads=False))
        assert fwd, f"{mutation} at {shape} passes the scoring bounds"
