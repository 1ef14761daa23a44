"""Per-feature attribution in the fused LSTM-AE kernel's epilogue (csrc/lstm.hip, the
ATTR instantiations) against the reference semantics of models/lstm_ae.py:
``recon_error_features`` (fp8: the per-feature errors of ``fp8_emulated_forward``'s
reconstruction) and ``attribute``.  Every other output of a call with ``attr`` is
bit-equal to the same call without it."""

import functools

import numpy as np
import pytest
import torch

from foremast_amd.brain.lstm_engine import CAL_GATE
from foremast_amd.models import lstm_ae
from foremast_amd.ops import lstm as L
from foremast_amd.ops.lstm import RingSource

pytestmark = pytest.mark.gpu

T = 24
NMAX = 300
THR, THR_LEVEL, EWMA = 4.0, 5.5, 0.05
RHO = 0.3          # relative spread the constructed calibrations use (the chi^2 spread of a 24-step error)
PAD = 3            # sentinel rows behind row N of every buffer
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _model(F):
    torch.manual_seed(100 + F)
    return lstm_ae.LSTMAutoencoder(F, 64)


@functools.lru_cache(maxsize=None)
def _windows(F):
    """300 windows with a series-specific noise scale 0.5 .. 1.5; rows 6, 16, 26, ... carry a NaN step."""
    g = torch.Generator().manual_seed(7 + F)
    x = (0.5 + torch.rand(NMAX, 1, 1, generator=g)) * torch.randn(NMAX, T, F, generator=g)
    x[6::10, 5, :] = NAN
    return x


def _ref_features(m, x, fp8):
    with torch.no_grad():
        if fp8:
            y, _ = L.fp8_emulated_forward(m, x)
            return ((y - x) ** 2).mean(1)
        return m.recon_error_features(x)


@functools.lru_cache(maxsize=None)
def _reference(F, fp8):
    """Reference per-feature errors [300, F] of _windows(F), computed once and never modified."""
    return _ref_features(_model(F), _windows(F), fp8)


def _case_tables(F, fp8):
    """Calibrations, level z and n_feat built from the REFERENCE errors so that known rows
    (by row % 10) take every path of the attribution:

    0  AE verdict, feature (row // 10) % F alone beyond the threshold (z ~ 6.7)
    1  AE verdict, no feature beyond it (z within +-1): the fallback names the largest
    2  level verdict alone: |level z| = 9 on one feature
    3  AE verdict, feature 0's calibration NaN (z NaN: -inf for the fallback)
    4  AE verdict, the last feature is padding (n_feat = F - 1) with a huge z
    5  healthy for the verdict but beyond CAL_GATE (z ~ 3): the calibrations keep their bits
    6  NaN window: no verdict, nothing refreshed
    7, 8, 9  healthy: mask 0, the calibrations track the errors
    """
    ef = _reference(F, fp8).clone()
    ef = torch.where(torch.isfinite(ef), ef, torch.ones_like(ef))
    e = ef.mean(1)
    g = torch.Generator().manual_seed(31 + F)
    rows = torch.arange(NMAX)
    k = rows % 10
    mu_f = ef * (0.85 + 0.3 * torch.rand(NMAX, F, generator=g))        # z_f within +-0.6
    mu = e.clone() * (0.9 + 0.2 * torch.rand(NMAX, generator=g))       # zs within +-0.4
    flagged = (k == 0) | (k == 1) | (k == 3) | (k == 4)
    mu[flagged] = e[flagged] / 3.0                                      # zs = 2 / RHO = 6.7
    mu[k == 5] = e[k == 5] / 1.9                                        # zs = 0.9 / RHO = 3
    f_hot = (rows // 10) % F
    hot = k == 0
    mu_f[rows[hot], f_hot[hot]] = ef[rows[hot], f_hot[hot]] / 3.0
    mu_f[k == 4, F - 1] = ef[k == 4, F - 1] / 10.0
    cal = torch.stack([mu, 1.0 / (RHO * mu)], 1)
    cal_feat = torch.stack([mu_f, 1.0 / (RHO * mu_f)], 2)
    cal_feat[k == 3, 0, 0] = NAN
    zlvl = 0.5 * torch.randn(NMAX, F, generator=g)
    lv = k == 2
    zlvl[rows[lv], f_hot[lv]] = torch.where(rows[lv] % 20 < 10, 9.0, -9.0)
    n_feat = torch.full((NMAX,), F, dtype=torch.int32)
    n_feat[k == 4] = max(F - 1, 1)
    return cal.contiguous(), cal_feat.contiguous(), zlvl.contiguous(), n_feat


def _padded(t, dev):
    """A device buffer with PAD sentinel rows behind t's rows; returns (whole, view of the first rows)."""
    n = t.shape[0]
    if t.dtype.is_floating_point:
        fill = torch.full((PAD,) + tuple(t.shape[1:]), -12345.5, dtype=t.dtype)
    else:
        fill = torch.full((PAD,) + tuple(t.shape[1:]), 77, dtype=t.dtype)
    whole = torch.cat([t, fill]).to(dev)
    return whole, whole[:n]


def _sentinels_intact(whole):
    tail = whole[-PAD:]
    want = torch.full_like(tail, -12345.5 if whole.dtype.is_floating_point else 77)
    return torch.equal(tail, want)


def _score(p, N, F, dev, tables, x=None, ring=None, attr=True, level=None, zlvl_in=True, ewma=EWMA):
    """One scoring call over buffers with sentinel rows; returns the outputs on the CPU."""
    cal0, cal_feat0, zlvl, n_feat = (t[:N].clone() for t in tables)
    bufs = {"err": torch.zeros(N), "zscore": torch.zeros(N), "verdict": torch.zeros(N, dtype=torch.int8),
            "cal": cal0, "cal_feat": cal_feat0, "blame": torch.full((N,), -1, dtype=torch.int32),
            "err_feat": torch.zeros(N, F), "zfeat": torch.zeros(N, F), "zlvl": zlvl, "n_feat": n_feat}
    whole, view = {}, {}
    for k, t in bufs.items():
        whole[k], view[k] = _padded(t, dev)
    app_id = (torch.arange(N, dtype=torch.int32) % 5).to(dev)
    app_stats = torch.zeros((5, 2), dtype=torch.int32, device=dev)
    out = {k: view[k] for k in ("err", "zscore", "verdict")}
    a = None
    if attr:
        a = {"cal": view["cal_feat"], "blame": view["blame"], "err_feat": view["err_feat"], "zfeat": view["zfeat"],
             "n_feat": view["n_feat"]}
    L.lstm_score(p, None if x is None else x[:N].to(dev).contiguous(), mu=0.0, sigma=1e-6, thr_default=THR,
                 app_id=app_id, app_stats=app_stats, out=out, ring=ring, T=T, cal=view["cal"], cal_ewma=ewma,
                 zlvl=view["zlvl"] if zlvl_in else None, thr_level=THR_LEVEL, level=level, attr=a)
    torch.cuda.synchronize()
    for k, w in whole.items():
        assert _sentinels_intact(w), f"{k}: rows behind row N were written"
    res = {k: v.cpu() for k, v in view.items()}
    res["app_stats"] = app_stats.cpu()
    return res


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_attribution(res, plain, tables, N, F, ref, fp8, zl=None):
    cal0, cal_feat0, zlvl, n_feat = (t[:N] for t in tables)
    zl = zlvl if zl is None else zl
    # every other output is bit-equal with and without attribution
    for k in ("err", "zscore", "verdict", "cal", "app_stats"):
        assert torch.equal(_bits(res[k]), _bits(plain[k])), k
    # per-feature errors against the reference, at the project's own bounds for err
    tol = dict(rtol=1e-2, atol=1e-5) if fp8 else dict(rtol=5e-2, atol=1e-3)
    np.testing.assert_allclose(res["err_feat"].numpy(), ref[:N].numpy(), equal_nan=True, **tol)
    ok = torch.isfinite(res["err"])
    torch.testing.assert_close(res["err_feat"].mean(1)[ok], res["err"][ok], rtol=1e-5, atol=0)
    assert bool(torch.isnan(res["err_feat"][~ok]).all())
    zf = (res["err_feat"] - cal_feat0[..., 0]) * cal_feat0[..., 1]
    torch.testing.assert_close(res["zfeat"], zf, rtol=1e-6, atol=1e-6, equal_nan=True)
    # blame == attribute() of the kernel's own err_feat, calibration, level z and verdict, on
    # every row that is not within 1e-3 of a threshold (at most 1 % of the rows)
    want = lstm_ae.attribute(res["err_feat"], cal_feat0, THR, zl, THR_LEVEL, res["verdict"], n_feat)
    near = ((zf - THR).abs() < 1e-3).any(1) | ((zl.abs() - THR_LEVEL).abs() < 1e-3).any(1)
    assert int(near.sum()) <= 0.01 * N
    assert torch.equal(res["blame"][~near], want[~near])
    return zf, want


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("F", [1, 2, 3, 7])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 129, 300])
def test_attribution_x_input(N, F, fp8):
    """x input at the lane-half (1), wave (31 / 32 / 33) and workgroup (129) edges: err_feat,
    bit equality of the other outputs, blame on every path of the rule, the calibration
    refresh and its gate, sentinel rows untouched."""
    dev = torch.device("cuda:0")
    m, x, ref = _model(F), _windows(F), _reference(F, fp8)
    tables = _case_tables(F, fp8)
    cal0, cal_feat0, zlvl, n_feat = (t[:N] for t in tables)
    # the reference inputs leave no row within 1e-3 of a threshold (checked on the CPU reference)
    zf_ref = (ref[:N] - cal_feat0[..., 0]) * cal_feat0[..., 1]
    assert not bool(((zf_ref - THR).abs() < 1e-3).any()) and not bool(((zlvl.abs() - THR_LEVEL).abs() < 1e-3).any())
    p = L.pack(m, fp8=fp8, device=dev)
    res = _score(p, N, F, dev, tables, x=x, attr=True)
    plain = _score(p, N, F, dev, tables, x=x, attr=False)
    zf, want = _check_attribution(res, plain, tables, N, F, ref, fp8)
    rows = torch.arange(N)
    k = rows % 10
    v, blame = res["verdict"], res["blame"]
    f_hot = ((rows // 10) % F).to(torch.int32)
    one = torch.ones(N, dtype=torch.int32)
    # the constructed rows take the paths they were built for
    assert bool((v[(k <= 4)] == 1).all()) and bool((v[k >= 5] == 0).all())
    assert torch.equal(blame[k == 0], (one << f_hot)[k == 0])                       # AE term, one feature
    assert torch.equal(blame[k == 2], (one << f_hot)[k == 2])                       # level term alone
    assert bool(((zf[k == 1] <= THR) | torch.isnan(zf[k == 1])).all())              # fallback rows: nothing above
    fb = torch.where(torch.isnan(zf), torch.full_like(zf, -float("inf")), zf).argmax(1).to(torch.int32)
    assert torch.equal(blame[k == 1], (one << fb)[k == 1])
    if F > 1:
        assert bool(((blame[k == 3] & 1) == 0).all())                                 # the NaN feature is not named
        assert bool((((blame[k == 4] >> (F - 1)) & 1) == 0).all())                    # padding is not named
        assert bool((zf[k == 4, F - 1] > THR).all()) and bool((blame[k == 4] != 0).all())
    else:
        assert bool((blame[k == 3] == 1).all())                                     # every z NaN: feature 0
    assert bool((blame[k >= 5] == 0).all())                                         # healthy / gated / NaN: mask 0
    # calibration refresh: healthy rows by the formula from the kernel's err_feat; flagged rows,
    # rows beyond CAL_GATE and NaN rows keep their bits
    zs = (res["err"] - cal0[:, 0]) * cal0[:, 1]
    upd = (v == 0) & torch.isfinite(res["err"]) & (zs <= CAL_GATE)
    assert bool((upd == (k >= 7)).all())
    mu0, inv0 = cal_feat0[..., 0], cal_feat0[..., 1]
    nmu = mu0 + EWMA * (res["err_feat"] - mu0)
    torch.testing.assert_close(res["cal_feat"][upd][..., 0], nmu[upd], rtol=1e-6, atol=0)
    torch.testing.assert_close(res["cal_feat"][upd][..., 1], (inv0 * (mu0 / nmu))[upd], rtol=1e-6, atol=0)
    assert torch.equal(_bits(res["cal_feat"][~upd]), _bits(cal_feat0[~upd]))
    # without the optional outputs and n_feat: the same blame where no padding is involved
    blame2 = torch.full((N,), -1, dtype=torch.int32, device=dev)
    L.lstm_score(p, x[:N].to(dev).contiguous(), mu=0.0, sigma=1e-6, thr_default=THR, T=T, cal=cal0.to(dev),
                 zlvl=zlvl.to(dev), thr_level=THR_LEVEL, attr={"cal": cal_feat0.to(dev), "blame": blame2})
    torch.cuda.synchronize()
    assert torch.equal(blame2.cpu()[k != 4], blame[k != 4])


def _rings(N, F, R, dtype, dev, m_season, newest_col, seed):
    """Rings whose newest sample sits at physical column ``newest_col`` (the scored window
    wraps around the ring's end), noise sigma 1 around a per-feature level; rows 2, 12, ..
    carry a +6 shift of feature (row // 10) % F over the newest 8 points."""
    g = torch.Generator().manual_seed(seed)
    logical = [50.0 + 10.0 * f + torch.randn(N, R, generator=g) for f in range(F)]
    rows = torch.arange(N)
    for r_ in rows[rows % 10 == 2].tolist():
        logical[(r_ // 10) % F][r_, -8:] += 6.0
    stored = [torch.roll(v, newest_col + 1, dims=1).to(dtype) for v in logical]
    vals = torch.stack([torch.roll(s.float(), -(newest_col + 1), dims=1) for s in stored], 2)   # [N, R, F] as stored
    mean, std = vals.mean(1), vals.std(1, unbiased=False)
    xw = (vals[:, -T:] - mean[:, None]) * (1.0 / std)[:, None]
    return [s.to(dev).contiguous() for s in stored], mean.contiguous(), (1.0 / std).contiguous(), xw.contiguous()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("ring_dtype", [torch.bfloat16, torch.float32], ids=["ring_bf16", "ring_fp32"])
@pytest.mark.parametrize("N", [33, 129])
def test_attribution_ring_input_and_fused_level(N, ring_dtype, fp8):
    """Ring input with a head that makes the window wrap, bf16 and fp32 rings; the level z
    computed by the kernel itself (fused_level_z) yields the mask the zlvl input path
    yields from the same z."""
    dev = torch.device("cuda:0")
    F, R, season, newest = 3, 192, 48, 10
    m = _model(F)
    rings, mean, rstd, xw = _rings(N, F, R, ring_dtype, dev, season, newest, seed=5)
    assert (newest - T + 1) % R + T > R   # the window wraps
    ref = _ref_features(m, xw, fp8)
    ef = ref.clone()
    e = ef.mean(1)
    g = torch.Generator().manual_seed(9)
    rows = torch.arange(N)
    k = rows % 10
    mu = e * (0.9 + 0.2 * torch.rand(N, generator=g))
    mu_f = ef * (0.85 + 0.3 * torch.rand(N, F, generator=g))
    hot = k == 0
    mu[hot] = e[hot] / 3.0
    mu_f[rows[hot], (rows[hot] // 10) % F] = ef[rows[hot], (rows[hot] // 10) % F] / 3.0
    tables = (torch.stack([mu, 1.0 / (RHO * mu)], 1).contiguous(),
              torch.stack([mu_f, 1.0 / (RHO * mu_f)], 2).contiguous(), torch.zeros(N, F),
              torch.full((N,), F, dtype=torch.int32))
    p = L.pack(m, fp8=fp8, device=dev)

    def src():
        return RingSource(rings=rings, start_col=(newest - T + 1) % R, mean=mean.to(dev), rstd=rstd.to(dev))
    lvl_out = torch.full((N, F), NAN, device=dev)
    # the statistic's own spread: an 8-point mean minus 3 days' 8-point means extrapolated, sqrt((1 + 21/9) / 8)
    sig = torch.full((N, F), 0.65, device=dev)
    level = {"sig": sig, "m": season, "newest": newest, "avail": R, "E": 0, "out": lvl_out}
    res = _score(p, N, F, dev, tables, ring=src(), attr=True, level=level, zlvl_in=False)
    zl = lvl_out.cpu().clone()
    plain = _score(p, N, F, dev, tables, ring=src(), attr=False, level=dict(level, out=None), zlvl_in=False)
    _check_attribution(res, plain, tables, N, F, ref, fp8, zl=zl)
    f_hot = ((rows // 10) % F).to(torch.int32)
    one = torch.ones(N, dtype=torch.int32)
    assert bool((zl[rows[k == 2], f_hot[k == 2].long()].abs() > THR_LEVEL).all())
    assert bool((res["verdict"][(k == 0) | (k == 2)] == 1).all())
    assert bool((((res["blame"][k == 2] >> f_hot[k == 2]) & 1) == 1).all())         # the shifted feature is named
    assert torch.equal(res["blame"][k == 0] & (one << f_hot)[k == 0], (one << f_hot)[k == 0])
    # the separate zlvl input path, fed the kernel's own level z, gives the same mask
    tables_z = tables[:2] + (zl.contiguous(),) + tables[3:]
    res_z = _score(p, N, F, dev, tables_z, ring=src(), attr=True, level=None, zlvl_in=True)
    assert torch.equal(res_z["blame"], res["blame"]) and torch.equal(res_z["verdict"], res["verdict"])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("F,hit", [(2, (0,)), (3, (1,)), (7, (2, 5))])
def test_attribution_names_the_perturbed_features(F, hit, fp8):
    """Meaning: cal_feat calibrated by the kernel from 8 healthy windows per series (noise scale
    0.5 .. 1.5), then +6 own sigmas on steps 10..13 of the chosen features of every window:
    every perturbed feature is named in every window, an unperturbed one in at most 3 %."""
    dev = torch.device("cuda:0")
    N, K = NMAX, 8
    m = _model(F)
    p = L.pack(m, fp8=fp8, device=dev)
    g = torch.Generator().manual_seed(50 + F)
    scale = 0.5 + torch.rand(N, 1, 1, generator=g)
    healthy = (scale * torch.randn(K, N, T, F, generator=g)).view(K * N, T, F)
    ones = torch.ones((K * N, F, 2), device=dev)
    ekf = torch.empty((K * N, F), device=dev)
    o = L.lstm_score(p, healthy.to(dev).contiguous(), thr_default=float("inf"),
                     attr={"cal": ones, "blame": torch.empty(K * N, dtype=torch.int32, device=dev), "err_feat": ekf})
    torch.cuda.synchronize()
    ekf, ek = ekf.cpu().view(K, N, F), o["err"].cpu().view(K, N)

    def level_spread(e):   # the shard's rule: mean without the largest, pooled relative spread
        mu = e.sort(0).values[:-1].mean(0)
        return mu, float((e / mu[None] - 1.0).std(unbiased=False))
    mu, rho = level_spread(ek)
    mu_f, rho1 = level_spread(ekf)
    x = scale * torch.randn(N, T, F, generator=g)
    for f in hit:
        x[:, 10:14, f] += 6.0 * scale[:, 0]
    blame = torch.zeros(N, dtype=torch.int32, device=dev)
    o = L.lstm_score(p, x.to(dev).contiguous(), mu=0.0, sigma=1e-6, thr_default=THR,
                     cal=torch.stack([mu, 1.0 / (rho * mu)], 1).to(dev).contiguous(),
                     attr={"cal": torch.stack([mu_f, 1.0 / (rho1 * mu_f)], 2).to(dev).contiguous(), "blame": blame})
    torch.cuda.synchronize()
    blame = blame.cpu()
    assert bool((o["verdict"].cpu() == 1).all())
    for f in range(F):
        named = float(((blame >> f) & 1).float().mean())
        print(f"F={F} fp8={fp8} feature {f}: named in {100 * named:.1f} % of windows (rho1 {rho1:.3f})")
        if f in hit:
            assert named == 1.0, (f, named)
        else:
            assert named <= 0.03, (f, named)


def _toy_history(n, R, F, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(R, dtype=torch.float32)
    return [10.0 + 2.0 * torch.sin(2 * np.pi * t / 60.0)[None, :] + (0.5 + torch.rand(n, 1, generator=g))
            * torch.randn(n, R, generator=g) for _ in range(F)]


def test_shard_blame_eager_graph_and_snapshot(monkeypatch, tmp_path):
    """LstmShard on the GPU, 64 entities x 3 features: calibrate(), then ticks eagerly and as
    graph replays give equal blame; a snapshot round trip keeps cal_feat."""
    from foremast_amd.brain import checkpoint as ck
    from foremast_amd.brain.lstm_engine import LstmShard
    dev = torch.device("cuda:0")
    n, R, F = 64, 300, 3

    def make(graph):
        monkeypatch.setenv("FOREMAST_LSTM_GRAPH", "1" if graph else "0")
        sh = LstmShard(n, R, F, window=16, device=dev, train_batch=64, lr=1e-2, restat_every=8, seed=3,
                       attribution=True)
        sh.load_history([h.to(dev) for h in _toy_history(n, R, F)])
        for _ in range(3):
            sh.train_step()
        sh.calibrate(256)
        return sh
    a, b = make(False), make(True)
    assert a.cal_feat is not None and a.cal_feat.shape == (n, F, 2) and bool((a.cal_feat[..., 0] > 0).all())
    torch.testing.assert_close(a.cal_feat, b.cal_feat, rtol=0, atol=0)
    xa, xb = torch.empty((n, F), device=dev), torch.empty((n, F), device=dev)
    g = torch.Generator().manual_seed(5)
    seen = 0
    for k in range(6):
        x = torch.randn(n, F, generator=g) + 10.0
        x[:8, 1] += 12.0          # entities 0..7: feature 1 leaves its range
        xa.copy_(x)
        xb.copy_(x)
        oa, ob = a.tick(xa), b.tick(xb)
        torch.cuda.synchronize()
        assert torch.equal(oa["verdict"], ob["verdict"]) and torch.equal(oa["blame"], ob["blame"]), k
        assert bool(((oa["blame"] != 0) == (oa["verdict"] == 1)).all())
        seen += int(((oa["blame"][:8] & 2) != 0).sum())
    assert b.graph_replays >= 2 and a.graph_replays == 0
    assert seen >= 8 * 2          # the regressed feature is named on the regressed entities
    path = str(tmp_path / "lstm.ckpt")
    ck.save_lstm_shard(a, path)
    back = ck.load_lstm_shard(path, device=dev)
    assert back.attribution and torch.equal(back.cal_feat, a.cal_feat) and back.rho1 == pytest.approx(a.rho1)


def test_attr_arguments_are_validated():
    """lstm_score rejects attribution buffers of the wrong shape, dtype, layout or device
    before anything is launched."""
    from foremast_amd.ops.kernels import KernelShapeError
    dev = torch.device("cuda:0")
    N, F = 33, 3
    p = L.pack(_model(F), device=dev)
    x = _windows(F)[:N].to(dev).contiguous()

    def good():
        return {"cal": torch.ones(N, F, 2, device=dev), "blame": torch.zeros(N, dtype=torch.int32, device=dev),
                "err_feat": torch.zeros(N, F, device=dev), "zfeat": torch.zeros(N, F, device=dev),
                "n_feat": torch.full((N,), F, dtype=torch.int32, device=dev)}
    L.lstm_score(p, x, attr=good())
    bad = {"cal": [torch.ones(N, F, device=dev), torch.ones(N, F, 2, device=dev, dtype=torch.float64),
                   torch.ones(N, 2, F, device=dev).transpose(1, 2), torch.ones(N, F, 2), None],
           "blame": [torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int64, device=dev),
                     None],
           "err_feat": [torch.zeros(N, F + 1, device=dev), torch.zeros(N, F, dtype=torch.float16, device=dev)],
           "zfeat": [torch.zeros(F, N, device=dev).t(), torch.zeros(N, F)],
           "n_feat": [torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N - 1, dtype=torch.int32, device=dev)]}
    for key, values in bad.items():
        for v in values:
            a = good()
            a[key] = v
            with pytest.raises(KernelShapeError):
                L.lstm_score(p, x, attr=a)
    with pytest.raises(KernelShapeError):
        L.lstm_score(p, x, attr=dict(good(), recon=torch.zeros(N, device=dev)))
    torch.cuda.synchronize()
