"""fp64 host model of the bf16 LSTM-autoencoder kernels (ops/csrc/lstm.hip, the bf16
instantiations; ops/csrc/lstm_train.hip, both variants; the GEMM half in ops/lstm_train.py).

Plain torch: the forward of models/lstm_ae.py and a hand-written backward through time.  With
``rounding=True`` a value is rounded to bf16 (round to nearest even, ``.float().to(bfloat16)``)
exactly where the kernels round it, and nowhere else:

* forward (``fwd_phase`` / ``run_phase``): the augmented weights ``[W_hh | W_ih | b]`` of both
  LSTMs are bf16 MFMA A fragments (the bias is a bf16 weight times an input of 1); ``h_{t-1}``
  and ``x_t`` are packed to bf16 as they enter the gate product (``pack8`` / ``make_b_bf16``).
  Gates, cell, ``h``, the read-out ``y = h W_out^T + b_out`` (unrounded ``h``, fp32 read-out
  weights) and the error against the unrounded ``x`` are fp32: not rounded here;
* backward (``bwd_phase``): ``dh_t += dy_t W_out`` unrounded; the dgates are rounded once, for
  the stored ``g_enc`` / ``g_dec`` and for the B operand of ``dh_{t-1} = bf16(W_hh)^T
  bf16(dgates_t)`` alike; the decoder's ``(dh, dc)`` after its step 0 seed the encoder's
  backward; ``dy = (y - x) * 2 / (B T F)``;
* host half: ``dW_aug = bf16(G) bf16([h_{t-1}; x_t; 1])^T`` per LSTM, ``dW_out = bf16(dy)
  bf16(h_dec[t + 1])^T`` and ``db_out = sum dy`` (unrounded), sums in high precision.

Layouts are the kernels': column ``t * B + b``, dgates in PyTorch gate-row order
(``gate * 64 + unit``, gates i, f, g, o).

``dtype=torch.float32`` runs the same model in fp32: a stand-in for a correct kernel's
accumulation noise and the rounding flips that follow from it.  ``mutate`` breaks the model in
one of three known ways (tests/test_lstm_ref.py proves the bounds below tell each from the
model itself).

The bounds of the GPU tests live here too, so the CPU test of this model and the GPU tests
apply the very same ones; the measured kernel-to-model ratios are recorded in
tests/test_lstm_train_gpu.py."""

from typing import Dict, Optional

import numpy as np
import torch

H = 64
PARAMS = ("enc_w_ih", "enc_w_hh", "enc_b", "dec_w_hh", "dec_b", "out_w", "out_b")
MUTATIONS = ("no_dgate_round", "swap_gate_rows", "rounded_x_err")

# kernel-to-model distance as a share of the model's own quantisation gap (rounded against
# unrounded): the two ratios of test_fp8_kernel_matches_emulated_fp8_reference
MEAN_RATIO = 0.1
P999_RATIO = 0.25
GRAD_RATIO = 0.25
# bf16-stored buffers: no element further from the model than two bf16 ulps of it (8-bit
# significand: 2^-6 relative) plus BF16_FLOOR x the tensor's median magnitude for the values
# near zero.  BF16_FLOOR is twice the largest excess over the rtol part measured on the MI355X:
# 0.197, on g_enc at (B, T, F) = (96, 12, 2) (tests/test_lstm_train_gpu.py).  That excess is no
# kernel error: where fp32 noise flips one bf16 rounding (an h of the last decoder steps, a
# dgate), every dgate of that window further down the backward recurrence moves by a share of
# the quantisation gap, and the dgates are sums of products that cancel, so the small ones move
# by far more than two of their own ulps.  The fp32 run of this model on the CPU has the same
# excess at the same shape (0.21), and 0.030 at (64, 5, 3) where the MI355X has 0.030 too.  The
# bound is for what the mean and the percentile cannot see, a few wrong cells: a stale scratch
# slot or a wrong row is off by many medians.
BF16_RTOL = 2.0 ** -6
BF16_FLOOR = 0.4

ELEMENTWISE = ("err", "dy", "g_enc", "g_dec", "h_enc", "h_dec")
BF16_STORED = ("g_enc", "g_dec", "h_enc", "h_dec")


def bf16(v: torch.Tensor) -> torch.Tensor:
    return v.float().to(torch.bfloat16).to(v.dtype)


def params_of(model) -> Dict[str, torch.Tensor]:
    return {n: getattr(model, n).detach().cpu().clone() for n in PARAMS}


def make_case(B: int, T: int, F: int, seed: int = 0):
    """A model with a trained-like spread of weights (some blocks far from the others, a
    read-out large enough that y really depends on h: the spread of
    test_fp8_kernel_matches_emulated_fp8_reference) and windows ``x [B, T, F]`` float32, a
    quarter of them with a +4 excursion."""
    from foremast_amd.models import lstm_ae
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7919 * seed + 101 * F + 13 * T + B)
        m = lstm_ae.LSTMAutoencoder(F, H)
        with torch.no_grad():
            m.enc_w_hh[:, :32] *= 3.0
            m.dec_w_hh[64:128] *= 0.05
            m.enc_b[::5] *= 6.0
            m.out_w *= 8.0
            m.out_b.uniform_(-0.5, 0.5)
        x = torch.randn(B, T, F)
        x[: B // 4, T // 2:] += 4.0
    return m, x.contiguous()


def _cell(gates, c):
    i, f, g, o = gates.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    cn = f * c + i * g
    tc = torch.tanh(cn)
    return o * tc, cn, (i, f, g, o, c, tc)


def _cell_backward(saved, dh, dc):
    i, f, g, o, cp, tc = saved
    dcu = dc + dh * o * (1 - tc * tc)
    dg = torch.cat([dcu * g * i * (1 - i), dcu * cp * f * (1 - f), dcu * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
    return dg, dcu * f


def reference(params: Dict[str, torch.Tensor], x: torch.Tensor, rounding: bool = True, dtype=torch.float64,
              mutate: Optional[str] = None, backward: bool = True) -> Dict[str, object]:
    """``x [B, T, F]`` (as the kernel gets it: float32) → ``y [B, T, F]``, ``err [B]``, ``loss``
    and, with ``backward``: ``dy [F, T B]``, ``g_enc`` / ``g_dec [256, T B]``, ``h_enc
    [64 + F, T B]`` (rows 0..63 ``h_{t-1}``, then ``x_t``), ``h_dec [64, (T + 1) B]`` (block 0 the
    encoder's final h, block t + 1 the decoder's ``h_t``) and ``grads`` (the seven parameter
    gradients of ``loss = err.mean()``).  Everything float64 on the CPU."""
    assert mutate is None or mutate in MUTATIONS
    P = {n: params[n].detach().cpu().to(dtype) for n in PARAMS}
    x = x.detach().cpu().to(dtype)
    B, T, F = x.shape
    rd = bf16 if rounding else (lambda v: v)
    if mutate == "swap_gate_rows":  # gates i and f of hidden unit 5, as a wrong fragment row map would
        w = P["enc_w_hh"].clone()
        w[[5, H + 5]] = w[[H + 5, 5]]
        P["enc_w_hh"] = w
    whe, wie, be = rd(P["enc_w_hh"]), rd(P["enc_w_ih"]), rd(P["enc_b"])
    whd, bd = rd(P["dec_w_hh"]), rd(P["dec_b"])
    wo, bo = P["out_w"], P["out_b"]
    xr = rd(x)
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    enc_saved, enc_in = [], []
    for t in range(T):
        hp = rd(h)
        h, c, s = _cell(hp @ whe.t() + xr[:, t] @ wie.t() + be, c)
        enc_saved.append(s)
        enc_in.append(hp)
    dec_saved, hdec, ys = [], [rd(h)], []
    for t in range(T):
        h, c, s = _cell(hdec[-1] @ whd.t() + bd, c)
        dec_saved.append(s)
        ys.append(h @ wo.t() + bo)
        hdec.append(rd(h))
    y = torch.stack(ys, 1)
    d = y - (xr if mutate == "rounded_x_err" else x)
    err = (d * d).mean(dim=(1, 2))
    out = {"y": y.double(), "err": err.double(), "loss": float(err.double().mean())}
    if not backward:
        return out
    dy = d * (2.0 / (B * T * F))  # [B, T, F]

    def bptt(saved, w, dh, dc, dec):
        gs = [None] * T
        for t in range(T - 1, -1, -1):
            if dec:
                dh = dh + dy[:, t] @ wo
            dg, dc = _cell_backward(saved[t], dh, dc)
            gs[t] = rd(dg)
            dh = (dg if mutate == "no_dgate_round" else gs[t]) @ w
        return gs, dh, dc
    g_dec, dh, dc = bptt(dec_saved, whd, x.new_zeros(B, H), x.new_zeros(B, H), True)
    g_enc, dh, dc = bptt(enc_saved, whe, dh, dc, False)
    dyr = rd(dy)
    one = x.new_ones(B)
    grads = {
        "enc_w_hh": sum(g_enc[t].t() @ enc_in[t] for t in range(T)),
        "enc_w_ih": sum(g_enc[t].t() @ xr[:, t] for t in range(T)),
        "enc_b": sum(g_enc[t].t() @ one for t in range(T)),
        "dec_w_hh": sum(g_dec[t].t() @ hdec[t] for t in range(T)),
        "dec_b": sum(g_dec[t].t() @ one for t in range(T)),
        "out_w": sum(dyr[:, t].t() @ hdec[t + 1] for t in range(T)),
        "out_b": dy.sum(dim=(0, 1)),
    }

    def cols(blocks):  # list of [B, rows] per block -> [rows, blocks * B]
        return torch.cat([b.t() for b in blocks], 1).double()
    out.update({
        "dy": cols([dy[:, t] for t in range(T)]),
        "g_enc": cols(g_enc), "g_dec": cols(g_dec),
        "h_enc": cols([torch.cat([enc_in[t], xr[:, t]], 1) for t in range(T)]),
        "h_dec": cols(hdec),
        "grads": {n: g.double() for n, g in grads.items()},
    })
    return out


# ------------------------------------------------------------------ the bounds
def _abs(a, b) -> np.ndarray:
    return (torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().flatten().numpy()


def ratios(got, rounded, unrounded) -> Dict[str, float]:
    """Distance of ``got`` from the rounded model over the model's quantisation gap: the mean
    and the 99.9th percentile.  Both denominators come from the model alone."""
    dk, dq = _abs(got, rounded), _abs(rounded, unrounded)
    qm, qp = float(dq.mean()), float(np.percentile(dq, 99.9))
    return {"mean": float(dk.mean()) / qm if qm > 0 else (0.0 if float(dk.mean()) == 0 else float("inf")),
            "p999": float(np.percentile(dk, 99.9)) / qp if qp > 0 else (0.0 if float(dk.max()) == 0 else float("inf")),
            "gap_mean": qm, "gap_p999": qp}


def bf16_excess(got, rounded) -> float:
    """Largest ``|got - model| - 2^-6 |model|`` over the tensor, in units of the model's median
    magnitude (0 when that median is 0 and nothing exceeds the rtol part)."""
    m = torch.as_tensor(rounded).double().flatten()
    ex = float(((torch.as_tensor(got).double().flatten() - m).abs() - BF16_RTOL * m.abs()).max())
    med = float(m.abs().median())
    if ex <= 0:
        return 0.0
    return ex / med if med > 0 else float("inf")


def grad_ratio(got, rounded, unrounded) -> float:
    r, u = torch.as_tensor(rounded).double(), torch.as_tensor(unrounded).double()
    gap = float((r - u).norm() / u.norm())
    dist = float((torch.as_tensor(got).double() - r).norm() / r.norm()) if float(r.norm()) > 0 else \
        float(torch.as_tensor(got).double().norm())
    return dist / gap if gap > 0 else (0.0 if dist == 0 else float("inf"))


def measure(got: Dict[str, object], rounded: Dict[str, object], unrounded: Dict[str, object],
            names=ELEMENTWISE, grads: bool = True) -> Dict[str, Dict[str, float]]:
    """Every figure the bounds are about, for ``got`` (a kernel's buffers, or another run of the
    model) in the layout of :func:`reference`."""
    res = {}
    for q in names:
        res[q] = ratios(got[q], rounded[q], unrounded[q])
        if q in BF16_STORED:
            res[q]["excess"] = bf16_excess(got[q], rounded[q])
    if grads:
        for n in PARAMS:
            res["grad." + n] = {"norm": grad_ratio(got["grads"][n], rounded["grads"][n], unrounded["grads"][n])}
    return res


def measure_pair(a: Dict[str, object], b: Dict[str, object], rounded: Dict[str, object],
                 unrounded: Dict[str, object]) -> Dict[str, Dict[str, float]]:
    """Two runs against each other (the two kernel variants) on the scale of the same bounds:
    their distance over the MODEL's quantisation gap."""
    res = {}
    for q in ELEMENTWISE:
        d, gap = _abs(a[q], b[q]), ratios(rounded[q], rounded[q], unrounded[q])
        res[q] = {"mean": float(d.mean()) / gap["gap_mean"], "p999": float(np.percentile(d, 99.9)) / gap["gap_p999"]}
        if q in BF16_STORED:
            res[q]["excess"] = bf16_excess(a[q], b[q])
    for n in PARAMS:
        ga, gb = torch.as_tensor(a["grads"][n]).double(), torch.as_tensor(b["grads"][n]).double()
        r, u = rounded["grads"][n], unrounded["grads"][n]
        gap = float((r - u).norm() / u.norm())
        dist = float((ga - gb).norm() / gb.norm()) if float(gb.norm()) > 0 else float(ga.norm())
        res["grad." + n] = {"norm": dist / gap if gap > 0 else (0.0 if dist == 0 else float("inf"))}
    return res


def violations(m: Dict[str, Dict[str, float]]) -> list:
    """The (quantity, figure, value, bound) of every bound that ``measure``'s result misses."""
    bad = []
    for q, r in m.items():
        for key, bound in (("mean", MEAN_RATIO), ("p999", P999_RATIO), ("excess", BF16_FLOOR), ("norm", GRAD_RATIO)):
            if key in r and not r[key] <= bound:
                bad.append((q, key, r[key], bound))
    return bad


def fmt(m: Dict[str, Dict[str, float]]) -> str:
    return "  ".join(q + " " + "/".join(f"{r[k]:.2e}" for k in ("mean", "p999", "excess", "norm") if k in r)
                     for q, r in m.items())
