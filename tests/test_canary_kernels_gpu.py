"""The canary kernels (rank tests, Friedman, bivariate scorer) against fp64 references.

Every reference is computed in float64 on exactly the values the kernel sees: the fp32
windows, or for bf16 rings the bf16-rounded values widened back.  Decisions are compared
exactly; a row is left out only where a reference p-value of a test that ran lies within
the kernel's p tolerance of alpha, and at most 2 % of a case's rows may be left out so.
"""

import functools
import math
import warnings

import numpy as np
import pytest
import torch

from foremast_amd.models import bivariate as biv_ref
from foremast_amd.models import pairwise as pw_ref

pytestmark = pytest.mark.gpu

P_RTOL, P_ATOL = 2e-3, 1e-5     # the tolerance the project holds the rank kernel's p-values to
MAX_EXCLUDED = 0.02             # share of a case's rows the margin rule may leave out
SEED = 11
ALPHAS = (0.05, 0.01)
GATES = ((20, 20, 5), (1, 1, 1))


@pytest.fixture(scope="module")
def K():
    from foremast_amd.ops import _native, kernels
    _native.require()
    return kernels


# ---- rank tests --------------------------------------------------------------------------

def _rank_inputs(N, nb, nc, nan_frac=0.05, shift=0.5, seed=SEED):
    """Seeded fp32 windows: normal rows, alternate rows with a shifted canary; the first
    quarter rounded to halves (ties), the next eighth 0/1 error counters (baseline 10 %
    ones, canary 20 %), NaN scattered over both windows, and from the last row backwards
    (as far as N allows, never more than half the rows): an all-NaN canary, an all-NaN
    baseline, a row with +inf / -inf samples, a row whose aligned pairs are all equal (no
    Wilcoxon pairs), an all-tied row."""
    rng = np.random.default_rng([seed, N, nb, nc])
    k = min(nb, nc)
    b = rng.normal(0, 1, (N, nb))
    c = rng.normal(0, 1, (N, nc))
    c[1::2] += shift
    q, e = N // 4, N // 8
    b[:q] = np.round(b[:q] * 2) / 2
    c[:q] = np.round(c[:q] * 2) / 2
    b[q:q + e] = rng.random((e, nb)) < 0.1
    c[q:q + e] = rng.random((e, nc)) < 0.2
    b[rng.random((N, nb)) < nan_frac] = np.nan
    c[rng.random((N, nc)) < nan_frac] = np.nan

    def nan_canary(r):
        c[r] = np.nan

    def nan_baseline(r):
        b[r] = np.nan

    def infs(r):
        b[r, 0] = np.inf
        c[r, nc - 1] = -np.inf
        if k > 2:                 # inf - inf: counted in both windows, no Wilcoxon pair
            b[r, 1] = c[r, 1] = np.inf

    def no_pairs(r):
        c[r, :k] = b[r, :k]

    def all_tied(r):
        b[r] = 2.0
        c[r] = 2.0

    for i, special in enumerate((nan_canary, nan_baseline, infs, no_pairs, all_tied)):
        if i >= N // 2:
            break
        special(N - 1 - i)
    return b.astype(np.float32), c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rank_case(N, nb, nc, pods=None, nan_frac=0.05, shift=0.5):
    """Inputs and the fp64 reference of one geometry (computed once, never modified)."""
    b, c = _rank_inputs(N, nb, nc, nan_frac, shift)
    tb, tc = torch.tensor(b), torch.tensor(c)
    ref = pw_ref.rank_tests(tb.double(), tc.double(), pods=pods)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the all-NaN baseline's mean is NaN
        bmean = np.nanmean(b.astype(np.float64), 1)
    return tb, tc, ref, bmean


def _near(p, alpha):
    return (p - alpha).abs() <= P_RTOL * alpha + P_ATOL


def _margin_rows(ref, mode, alpha, gate, min_friedman=5):
    """Rows where a reference p-value of a test that ran (and that ``mode`` reads) lies
    within the p tolerance of alpha: the only rows whose decision may differ."""
    n_small = torch.minimum(ref.n_base, ref.n_cur)
    mw = (n_small >= gate[0]) & _near(ref.p_mw, alpha)
    w = (ref.n_pairs >= gate[1]) & _near(ref.p_wilcoxon, alpha)
    kw = (n_small >= gate[2]) & _near(ref.p_kruskal, alpha)
    none = torch.zeros_like(mw)
    if mode == pw_ref.PW_FRIEDMAN:
        return (ref.n_blocks >= min_friedman) & _near(ref.p_friedman, alpha)
    return {pw_ref.PW_NONE: none, pw_ref.PW_ALL: mw | w | kw, pw_ref.PW_ANY: mw | w | kw,
            pw_ref.PW_MANN_WHITE: mw, pw_ref.PW_WILCOXON: w, pw_ref.PW_KRUSKAL: kw}[mode]


def _assert_decisions(differs, ref, mode, alpha, gate, min_friedman=5, what=""):
    """Exact outside the margin; returns (rows left out, reference rejections)."""
    N = differs.shape[0]
    dref = pw_ref.pairwise_differs(ref, mode, alpha, *gate, min_friedman=min_friedman)
    skip = _margin_rows(ref, mode, alpha, gate, min_friedman)
    n_skip = int(skip.sum())
    assert n_skip <= MAX_EXCLUDED * N, f"{what}: {n_skip} of {N} rows within the p margin of alpha"
    got = differs.cpu().bool()
    bad = torch.nonzero((got != dref) & ~skip).flatten().tolist()
    assert not bad, f"{what}: decisions differ from the fp64 reference on rows {bad[:10]}"
    return n_skip, int(dref.sum())


def _assert_pvals_counts(out, ref, bmean):
    cnt = out["counts"].cpu().double().numpy()
    np.testing.assert_array_equal(cnt[:, 0], ref.n_base.numpy())
    np.testing.assert_array_equal(cnt[:, 1], ref.n_cur.numpy())
    np.testing.assert_array_equal(cnt[:, 2], ref.n_pairs.numpy())
    p = out["pvals"].cpu().double().numpy()
    np.testing.assert_allclose(p[:, 0], ref.p_mw.numpy(), rtol=P_RTOL, atol=P_ATOL)
    np.testing.assert_allclose(p[:, 1], ref.p_wilcoxon.numpy(), rtol=P_RTOL, atol=P_ATOL)
    np.testing.assert_allclose(p[:, 2], ref.p_kruskal.numpy(), rtol=P_RTOL, atol=P_ATOL)
    np.testing.assert_allclose(out["base_mean"].cpu().numpy(), bmean, rtol=1e-5, atol=1e-6)


RANK_GEOMETRIES = [
    # small path (one key per lane)
    (257, 5, 5), (257, 1, 64), (257, 64, 1), (3, 55, 55),
    # sweep path: just over the switch, a k4 tail on a lopsided pair, an odd pooled length,
    # several outer-loop trips, exactly the LDS budget
    (257, 65, 64), (257, 64, 65), (257, 130, 3), (129, 129, 257), (61, 300, 200), (5, 1344, 1344),
]


@pytest.mark.parametrize("N,nb,nc", RANK_GEOMETRIES)
def test_rank_tests_all_modes_vs_fp64(K, N, nb, nc):
    """Modes 0-5 x alpha {0.05, 0.01} x gates {(20, 20, 5), (1, 1, 1)} x {p-value branch,
    decisions-only branch}: counts exact, base_mean and p-values at the kernel's tolerance,
    decisions exact outside the p margin."""
    dev = torch.device("cuda:0")
    tb, tc, ref, bmean = _rank_case(N, nb, nc)
    gb, gc = tb.to(dev), tc.to(dev)
    runs = {}
    for mode in range(6):
        for alpha in ALPHAS:
            for gate in GATES:
                for pv in (True, False):
                    runs[mode, alpha, gate, pv] = K.rank_tests(gb, gc, mode, alpha, *gate, want_pvals=pv)
    torch.cuda.synchronize()
    skipped, spread = set(), False
    for (mode, alpha, gate, pv), out in runs.items():
        what = f"({N}, {nb}, {nc}) mode {mode} alpha {alpha} gates {gate} pvals {pv}"
        if pv:
            _assert_pvals_counts(out, ref, bmean)
        else:
            assert "pvals" not in out and "counts" not in out
            np.testing.assert_allclose(out["base_mean"].cpu().numpy(), bmean, rtol=1e-5, atol=1e-6)
        n_skip, n_rej = _assert_decisions(out["differs"], ref, mode, alpha, gate, what=what)
        got = int(out["differs"].sum())
        spread = spread or (0 < n_rej < N and 0 < got < N)
        if n_skip:
            skipped.add((mode, alpha, gate, n_skip))
    print(f"rank case ({N}, {nb}, {nc}): margin exclusions (mode, alpha, gates, rows) {sorted(skipped)}")
    assert spread, "no (mode, gate) pair with 0 < differs.sum() < N: a constant output would pass"


@pytest.mark.parametrize("N,nb,nc", [(257, 5, 5), (257, 65, 64), (61, 300, 200)])
def test_rank_tests_row_stride_exceeds_window(K, N, nb, nc):
    """base / cur as column slices of wider tensors (the engine passes views): identical to
    the contiguous windows, whatever lies outside them."""
    dev = torch.device("cuda:0")
    tb, tc, ref, bmean = _rank_case(N, nb, nc)
    wb = torch.full((N, nb + 9), 1e30)
    wc = torch.full((N, nc + 6), -1e30)
    wb[:, 3:3 + nb] = tb
    wc[:, 5:5 + nc] = tc
    wb, wc = wb.to(dev), wc.to(dev)
    vb, vc = wb[:, 3:3 + nb], wc[:, 5:5 + nc]
    assert vb.stride(0) > nb and vc.stride(0) > nc
    for pv in (True, False):
        view = K.rank_tests(vb, vc, pw_ref.PW_ALL, 0.05, want_pvals=pv)
        flat = K.rank_tests(tb.to(dev), tc.to(dev), pw_ref.PW_ALL, 0.05, want_pvals=pv)
        torch.cuda.synchronize()
        for key in flat:
            assert torch.equal(view[key].cpu().view(torch.uint8), flat[key].cpu().view(torch.uint8)), key
    _assert_pvals_counts(K.rank_tests(vb, vc, pw_ref.PW_ALL, 0.05), ref, bmean)


def test_rank_tests_rejects_windows_over_the_lds_budget(K):
    dev = torch.device("cuda:0")
    ok = K.rank_tests(torch.zeros(1, 1344, device=dev), torch.ones(1, 1344, device=dev), pw_ref.PW_ALL, 0.05)
    torch.cuda.synchronize()
    assert ok["counts"].cpu().tolist() == [[1344.0, 1344.0, 1344.0]]
    with pytest.raises(K.KernelShapeError):
        K.rank_tests(torch.zeros(1, 1345, device=dev), torch.ones(1, 1344, device=dev), pw_ref.PW_ALL, 0.05)


# ---- Friedman geometries -----------------------------------------------------------------

FRIEDMAN_CASES = [
    # pods_b, pods_c, Wb, Wc
    (1, 1, 40, 40),     # k = 2, dof 1
    (2, 3, 12, 12),     # dof 4: chi2_sf's even branch
    (3, 4, 20, 12),     # Wb != Wc
    (5, 5, 11, 11),     # the product's 55 per side
    (32, 32, 2, 2),     # k = 64 on the small path
    (1, 1, 100, 100),   # 100 blocks: the sweep path, a second trip of the block loop
    (2, 2, 80, 80),     # sweep path
]


@pytest.mark.parametrize("pb,pc,Wb,Wc", FRIEDMAN_CASES)
def test_friedman_geometries_vs_fp64(K, pb, pc, Wb, Wc):
    """Complete-block counts exact, p at the kernel's tolerance, mode-6 decisions exact
    outside the p margin with the block gate met and not met, and the other tests'
    outputs bit-identical when Friedman rides along.

    NaNs are scattered at min(5 %, 0.3 / k) per sample, so that about a quarter of the
    blocks are incomplete at every k; the all-NaN canary row has no complete block."""
    dev = torch.device("cuda:0")
    N, k = 257, pb + pc
    nb, nc, nbk = pb * Wb, pc * Wc, min(Wb, Wc)
    tb, tc, ref, _ = _rank_case(N, nb, nc, pods=(pb, pc), nan_frac=min(0.05, 0.3 / k), shift=1.0)
    gb, gc = tb.to(dev), tc.to(dev)
    nblk = ref.n_blocks
    assert int(nblk.min()) == 0 and int(nblk.max()) > 0 and int((nblk < nbk).sum()) > N // 8
    runs = {}
    for alpha in ALPHAS:
        for mf in (1, 5, nbk + 1):
            runs[alpha, mf] = K.rank_tests(gb, gc, pw_ref.PW_FRIEDMAN, alpha, pods=(pb, pc), min_friedman=mf)
    ride = K.rank_tests(gb, gc, pw_ref.PW_ALL, 0.05, pods=(pb, pc), want_friedman=True)
    ride_d = K.rank_tests(gb, gc, pw_ref.PW_ALL, 0.05, pods=(pb, pc), want_friedman=True, want_pvals=False)
    plain = K.rank_tests(gb, gc, pw_ref.PW_ALL, 0.05)
    plain_d = K.rank_tests(gb, gc, pw_ref.PW_ALL, 0.05, want_pvals=False)
    torch.cuda.synchronize()
    skipped, spread = set(), False
    for (alpha, mf), out in runs.items():
        fr = out["friedman"].cpu().double().numpy()
        np.testing.assert_array_equal(fr[:, 1], nblk.numpy())
        np.testing.assert_allclose(fr[:, 0], ref.p_friedman.numpy(), rtol=P_RTOL, atol=P_ATOL)
        what = f"pods ({pb}, {pc}) W ({Wb}, {Wc}) alpha {alpha} min_friedman {mf}"
        n_skip, n_rej = _assert_decisions(out["differs"], ref, pw_ref.PW_FRIEDMAN, alpha, GATES[0], mf, what)
        if mf > nbk:
            assert n_rej == 0 and int(out["differs"].sum()) == 0   # the block gate abstains
        spread = spread or 0 < n_rej < N
        if n_skip:
            skipped.add((alpha, mf, n_skip))
    print(f"friedman case pods ({pb}, {pc}) W ({Wb}, {Wc}): margin exclusions (alpha, min_friedman, rows) "
          f"{sorted(skipped)}")
    # two blocks of 64 treatments reach p < 0.05 only when both blocks rank alike (chi2 <= 2 k - 2)
    assert spread or nbk < 5
    for a, b_ in ((ride, plain), (ride_d, plain_d)):
        for key in b_:
            assert torch.equal(a[key].cpu().view(torch.uint8), b_[key].cpu().view(torch.uint8)), key
        assert torch.equal(a["friedman"].cpu().view(torch.uint8), runs[0.05, 5]["friedman"].cpu().view(torch.uint8))


@pytest.mark.parametrize("pods", [(1, 1), (2, 2)])
def test_friedman_balanced_rows_give_p_one(K, pods):
    """Rows whose treatments collect equal rank sums: chi^2 is exactly 0 and p exactly 1.  The
    textbook form 12 / (n k (k + 1)) sum R^2 - 3 n (k + 1) cancels two terms of ~3 n (k + 1);
    with one dof p ~ 1 - 0.8 sqrt(chi), so an fp32 residue of 3e-5 (n = 104) already costs
    5e-3 of p.  Block counts on the small path (<= 64 per side) and on the sweep path."""
    dev = torch.device("cuda:0")
    P = pods[0]
    k = 2 * P
    rng = np.random.default_rng([SEED, k])
    for W in (4, 12, 28, 40, 52, 56, 60, 64, 88, 100, 104, 120):
        j = np.arange(W)
        # value of treatment t in block j: a rotation, so every treatment takes every rank W / k times
        g = np.stack([(t + j) % k for t in range(k)], 0).astype(np.float64)      # [k, W]
        rows = [g, g[:, ::-1], g * 0.37 - 1.0, g + 10.0 * rng.normal(0, 1, W)[None, :]]
        holes = g.copy()
        holes[0, :k] = np.nan                 # one whole rotation (k blocks) less: still balanced
        rows.append(holes)
        x = np.stack(rows, 0).astype(np.float32)                                  # [N, k, W]
        tb = torch.tensor(x[:, :P].reshape(len(rows), P * W))
        tc = torch.tensor(x[:, P:].reshape(len(rows), P * W))
        ref = pw_ref.rank_tests(tb.double(), tc.double(), pods=pods)
        assert ref.n_blocks.tolist() == [W] * 4 + [W - k] and torch.all(ref.p_friedman == 1.0)
        out = K.rank_tests(tb.to(dev), tc.to(dev), pw_ref.PW_FRIEDMAN, 0.05, pods=pods)
        torch.cuda.synchronize()
        fr = out["friedman"].cpu().double().numpy()
        np.testing.assert_array_equal(fr[:, 1], ref.n_blocks.numpy())
        np.testing.assert_allclose(fr[:, 0], 1.0, rtol=P_RTOL, atol=P_ATOL, err_msg=f"pods {pods}, {W} blocks")
        assert int(out["differs"].sum()) == 0


# ---- bivariate scorer --------------------------------------------------------------------

BIV_N, BIV_R, BIV_MIN_VALID, BIV_EPS, BIV_SENTINEL = 37, 1024, 20, 1e-9, -12345.0
RADII = (0.3, 0.8, 0.95, 1.05, 1.5, 4.0)   # x the row's effective threshold: >= 5 % from it
ROW_NAN_X, ROW_NAN_Y, ROW_FEW, ROW_NONE, ROW_CONST_X, ROW_NAN_CUR = 3, 4, 5, 6, 7, 8


def _fit64(v):
    """fp64 mean / biased covariance over jointly valid points; v: [N, T, 2] float64."""
    N = v.shape[0]
    mean, cov, cnt = np.zeros((N, 2)), np.zeros((N, 3)), np.zeros(N, dtype=np.int64)
    for n in range(N):
        p = v[n][~np.isnan(v[n]).any(1)]
        cnt[n] = len(p)
        if len(p):
            mean[n] = p.mean(0)
            d = p - mean[n]
            cov[n] = (d[:, 0] ** 2).mean(), (d[:, 0] * d[:, 1]).mean(), (d[:, 1] ** 2).mean()
    return mean, cov, cnt


def _d2_64(mean, cov, cur, eps=BIV_EPS):
    """The scorer's formula in float64 (models/bivariate.mahalanobis2 on an fp64 fit)."""
    fit = biv_ref.BivariateFit(mean=torch.tensor(mean, dtype=torch.float64),
                               cov=torch.tensor(cov, dtype=torch.float64), count=None)
    return biv_ref.mahalanobis2(fit, torch.tensor(cur, dtype=torch.float64), eps=eps).numpy()


@functools.lru_cache(maxsize=None)
def _biv_case(length, head, dtype, level, rho, C):
    """History (as the kernel sees it, widened to fp64), its fp64 fit, the rings, and current
    points placed at RADII x the effective threshold around the fp64 fit."""
    N, R = BIV_N, BIV_R
    rng = np.random.default_rng([SEED, length, head, int(level), int(rho * 100), C])
    h = rng.multivariate_normal([0, 0], [[1.0, rho * math.sqrt(2.0)], [rho * math.sqrt(2.0), 2.0]], size=(N, length))
    h = h + [level + 1.0, -level - 2.0]
    h[ROW_CONST_X, :, 0] = level + 2.5
    h[ROW_NAN_X, 1::4, 0] = np.nan
    h[ROW_NAN_Y, 2::5, 1] = np.nan
    h[ROW_FEW, 10:, 0] = np.nan            # 10 jointly valid points < min_valid
    h[ROW_NONE, 0::2, 0] = np.nan          # no jointly valid point
    h[ROW_NONE, 1::2, 1] = np.nan
    seen = torch.tensor(h, dtype=torch.float32).to(dtype)      # what the ring holds
    v = seen.double().numpy()
    mean, cov, cnt = _fit64(v)
    cols = (head + np.arange(length)) % R
    rings = []
    for j in (0, 1):
        ring = torch.full((N, R), BIV_SENTINEL, dtype=dtype)
        ring[:, cols] = seen[:, :, j]
        rings.append(ring)
    thr = (2.0 + np.arange(N) % 3).astype(np.float32)
    differs = (np.arange(N) % 2).astype(np.uint8)
    pw_scale = 0.5
    thr_eff = thr * np.where(differs > 0, np.float32(pw_scale), np.float32(1.0))
    # x = mean + L (r u), L the Cholesky factor of the covariance the scorer inverts (cov + eps)
    a, b, c = cov[:, 0] + BIV_EPS, cov[:, 1], cov[:, 2] + BIV_EPS
    l11 = np.sqrt(a)
    l21 = b / l11
    l22 = np.sqrt(c - l21 * l21)
    kk = np.arange(C)
    # rows 2, 6, 10, ... keep every point inside the threshold (verdict 0)
    inside = (np.arange(N) % 4 == 2)[:, None]
    fac = np.where(inside, np.array(RADII)[kk % 3][None, :], np.array(RADII)[kk % len(RADII)][None, :])
    theta = 0.7 * np.arange(N)[:, None] + 1.3 * kk[None, :]
    theta[ROW_CONST_X] = np.pi / 2 * (1 + 2 * (kk % 2))         # u = (0, +-1): dx = 0 exactly
    ux, uy = np.cos(theta), np.sin(theta)
    ux[ROW_CONST_X] = 0.0
    r = fac * thr_eff[:, None].astype(np.float64)
    cur = np.stack([mean[:, None, 0] + l11[:, None] * r * ux,
                    mean[:, None, 1] + l21[:, None] * r * ux + l22[:, None] * r * uy], 2)
    if C > 256:                                                # some missing current points
        cur[:, 3::7, 0] = np.nan
        cur[:, 5::11, 1] = np.nan
    cur[ROW_NAN_CUR] = np.nan
    cur = cur.astype(np.float32)
    cur_ok = ~np.isnan(cur).any(2)
    model_ok = cnt >= BIV_MIN_VALID
    count = np.where(model_ok, (cur_ok & (fac > 1.0)).sum(1), 0).astype(np.int32)
    verdict = np.where(count > 0, 1, np.where(cur_ok.any(1) & model_ok, 0, -1)).astype(np.int8)
    app_id = (np.arange(N) % 5).astype(np.int32)
    stats = np.zeros((5, 2), dtype=np.int32)
    np.add.at(stats[:, 0], app_id, verdict == 1)
    np.add.at(stats[:, 1], app_id, verdict >= 0)
    return dict(v=v, mean=mean, cov=cov, cnt=cnt, rings=rings, thr=thr, differs=differs, pw_scale=pw_scale,
                cur=cur, cur_ok=cur_ok, count=count, verdict=verdict, app_id=app_id, stats=stats)


BIV_CASES = [
    # length, head, dtype, level, rho, C, well conditioned at level 0 (d2 also vs the full fp64 fit)
    pytest.param(700, 1001, torch.float32, 0.0, 0.6, 12, True, id="wrap-fp32"),
    pytest.param(700, 1001, torch.bfloat16, 0.0, 0.6, 12, True, id="wrap-bf16"),
    pytest.param(60, 1001, torch.float32, 0.0, 0.6, 12, True, id="len60-fp32"),
    pytest.param(60, 1001, torch.bfloat16, 0.0, 0.6, 12, True, id="len60-bf16"),
    pytest.param(257, 900, torch.float32, 0.0, 0.6, 12, True, id="len257-fp32"),
    pytest.param(257, 900, torch.bfloat16, 0.0, 0.6, 12, True, id="len257-bf16"),
    pytest.param(700, 1001, torch.float32, 1e4, 0.6, 12, False, id="level1e4-fp32"),
    # 1 / (1 - rho^2) = 50 amplifies the fp32 moments' ~1e-6 error to ~5e-5 of d2: within 2e-3
    pytest.param(700, 333, torch.float32, 0.0, 0.99, 12, True, id="rho0.99-fp32"),
    pytest.param(700, 1001, torch.float32, 0.0, 0.6, 300, True, id="C300-fp32"),
    pytest.param(1024, 517, torch.bfloat16, 0.0, 0.6, 300, True, id="fullring-C300-bf16"),
]


@pytest.mark.parametrize("length,head,dtype,level,rho,C,well", BIV_CASES)
def test_bivariate_kernel_vs_fp64_fit(K, length, head, dtype, level, rho, C, well):
    """Fit (mean, cov) against the fp64 fit of the values in the ring; d2 against the fp64
    formula on the kernel's own fit (and on the fp64 fit where well conditioned); count,
    verdict, score and app_stats exact by construction of the current points."""
    dev = torch.device("cuda:0")
    cs = _biv_case(length, head, dtype, level, rho, C)
    N = BIV_N
    hx, hy = (r.to(dev) for r in cs["rings"])
    stats = torch.zeros((5, 2), dtype=torch.int32, device=dev)
    out = K.bivariate(hx, hy, head, length, torch.tensor(cs["cur"], device=dev), torch.tensor(cs["thr"], device=dev),
                      differs=torch.tensor(cs["differs"], device=dev), pw_scale=cs["pw_scale"],
                      min_valid=BIV_MIN_VALID, eps=BIV_EPS, app_id=torch.tensor(cs["app_id"], device=dev),
                      app_stats=stats)
    torch.cuda.synchronize()
    mean_k = out["mean"].cpu().double().numpy()
    cov_k = out["cov"].cpu().double().numpy()
    d2_k = out["d2"].cpu().double().numpy()
    # -- fit: one fp32 ulp of |mean| plus 1e-6 sigma; cov at window_stats' rtol, 0 stays 0
    sigma = np.sqrt(cs["cov"][:, [0, 2]])
    ulp = np.spacing(np.abs(cs["mean"]).astype(np.float32)).astype(np.float64)
    err = np.abs(mean_k - cs["mean"])
    print(f"bivariate fit: worst mean error {float((err / (ulp + 1e-6 * sigma)).max()):.3f} of its bound, "
          f"worst cov error {float(np.abs(cov_k - cs['cov']).max()):.3g}")
    assert (err <= ulp + 1e-6 * sigma).all(), (np.argwhere(err > ulp + 1e-6 * sigma)[:5], err.max())
    assert cs["cov"][ROW_CONST_X, 0] == 0.0 and cs["cov"][ROW_CONST_X, 1] == 0.0
    np.testing.assert_allclose(cov_k[ROW_CONST_X, :2], 0.0, rtol=0, atol=1e-8)
    np.testing.assert_allclose(cov_k[ROW_NONE], 0.0, rtol=0, atol=1e-8)
    live = np.ones((N, 3), dtype=bool)
    live[ROW_CONST_X, :2] = False
    live[ROW_NONE] = False
    np.testing.assert_allclose(cov_k[live], cs["cov"][live], rtol=1e-4)
    # -- scoring
    assert np.array_equal(np.isnan(d2_k), ~cs["cur_ok"])
    ok = cs["cur_ok"]
    own = _d2_64(mean_k, cov_k, cs["cur"])
    np.testing.assert_allclose(d2_k[ok], own[ok], rtol=2e-3, atol=1e-3)
    if well:
        rows = np.ones(N, dtype=bool)
        rows[[ROW_NONE]] = False      # no fit to compare with
        full = _d2_64(cs["mean"], cs["cov"], cs["cur"])
        m = ok & rows[:, None]
        np.testing.assert_allclose(d2_k[m], full[m], rtol=2e-3, atol=1e-3)
    np.testing.assert_array_equal(out["count"].cpu().numpy(), cs["count"])
    np.testing.assert_array_equal(out["verdict"].cpu().numpy(), cs["verdict"])
    score = np.sqrt(np.where(ok, own, 0.0).max(1))
    np.testing.assert_allclose(out["score"].cpu().numpy(), score, rtol=2e-3)
    np.testing.assert_array_equal(stats.cpu().numpy(), cs["stats"])
    # the case holds every verdict, rows over and rows under the threshold
    assert set(cs["verdict"].tolist()) == {-1, 0, 1} and 0 < (cs["count"] > 0).sum() < N
