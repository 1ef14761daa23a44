// The k-variate normal over row groups of one ring (2 <= k <= 8): the joint model of a
// streaming shard's jobs with three or more metrics, and bivariate_pairs.hip generalised.
//
// Semantics: foremast_amd/models/multivariate_normal.py.  The k metrics of a group are rows
// of ONE [N, ld] history ring; the current values are the pod means of the [N, P*W] window
// ring (column p * W + slot).  One wave per group: the k rows are streamed once with shifted
// moment sums over the jointly valid points (k sums, k (k + 1) / 2 products per lane), the
// lane means are merged relative to a wave-common centre (bivariate.hip explains why never
// as absolute values), the covariance + eps I is factorised (Cholesky, pivot floor 1e-20),
// then every window slot is scored: z = L^-1 (x - mean), d^2 = |z|^2, and the additive
// attribution c_i = (x - mean)_i (L^-T z)_i.  Anomaly iff the model is ok and d^2 > thr2,
// thr2 = q_k(thr) the chi^2_k quantile computed by the host.  On an anomalous slot metric i
// is named iff c_i >= d^2 / k, the largest c_i always (ties: the first).
//
// k is a template parameter: every accumulator and factor array is indexed by unrolled
// constants and stays in registers.  The host launches one instantiation per k present in
// the table (MvnGroupArgs::kmask); a wave whose group has another k leaves at once.
//
// A full ring (len == ring_len: every streaming tick) is walked in physical order 0..R-1 with
// 16-byte loads, the moments do not depend on the order; a partial or wrapped window takes
// the scalar path.  A flagged group raises the row verdict of every NAMED metric and counts
// each row once in the per-app table (groups may share a row: the first to exchange
// raised[row] does it), and appends (row, slot, pod mean) per anomalous slot and named
// metric to the K9 list.
#include "mvn_common.h"

#ifndef FM_MVN_WAVES
#define FM_MVN_WAVES 4   // groups (waves) per workgroup
#endif
constexpr int kMvnBlock = FM_MVN_WAVES * FM_WAVE;

template <typename TIN, bool FULL, int K>
__global__ __launch_bounds__(kMvnBlock) void mvn_groups_kernel(const MvnGroupArgs a, const int kfirst) {
  constexpr int TRI = K * (K + 1) / 2;
  constexpr int UNR = MvnUnroll<K>::value;
  const int q = blockIdx.x * FM_MVN_WAVES + wave_id();
  if (q >= a.Ng) return;  // wave-uniform
  const int lane = lane_id();
  const int* g = a.groups + (long long)q * FM_MVN_MAXK;
  const int k = mvn_group_k(g);
  // the launch of the smallest k present also reports the groups with fewer than two rows
  if (k != K && !(k < 2 && K == kfirst)) return;
  int r[K];
  bool inside = k == K;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    r[i] = inside ? g[i] : 0;
    inside = inside && (unsigned)r[i] < (unsigned)a.N;
  }
  if (!inside) {
    // fewer than two rows, or a row outside the ring: nothing is read, the group is unscored
    for (int j = lane; j < a.W; j += FM_WAVE) a.d2[(long long)q * a.W + j] = fm_nan();
    if (a.contrib) {
      for (int j = lane; j < a.W * FM_MVN_MAXK; j += FM_WAVE) a.contrib[(long long)q * a.W * FM_MVN_MAXK + j] = fm_nan();
    }
    if (lane < FM_MVN_MAXK) a.mean[(long long)q * FM_MVN_MAXK + lane] = fm_nan();
    if (lane < FM_MVN_TRI) a.cov[(long long)q * FM_MVN_TRI + lane] = fm_nan();
    if (lane == 0) { a.nvalid[q] = 0.f; a.count[q] = 0; a.verdict[q] = -1; a.score[q] = 0.f; a.blame[q] = 0; }
    return;
  }
  const TIN* row[K];
#pragma unroll
  for (int i = 0; i < K; ++i) row[i] = (const TIN*)a.hist + (long long)r[i] * a.ld;
  MvnAcc<K> s;
  if (FULL) {
    mvn_acc_full<TIN, K, UNR>(row, a.ring_len, lane, s);
  } else {
    mvn_acc_wrapped<TIN, K>(row, a.ring_len, a.head, a.len, lane, s);
  }
  float mean[K], v[TRI], N;
  mvn_merge<K>(s, mean, v, N);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < FM_MVN_MAXK; ++i) a.mean[(long long)q * FM_MVN_MAXK + i] = i < K ? mean[i] : 0.f;
#pragma unroll
    for (int i = 0; i < FM_MVN_TRI; ++i) a.cov[(long long)q * FM_MVN_TRI + i] = i < TRI ? v[i] : 0.f;
    a.nvalid[q] = N;
  }
  float il[K];
  mvn_cholesky<K>(v, il, a.eps);
  const float thr2 = a.thr2[q];
  const bool model_ok = N >= (float)a.min_valid;
  const float* cur[K];
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = a.cur + (long long)r[i] * a.ld_cur;
  float cnt = 0.f, anyv = 0.f, sc = 0.f;
  int blame = 0;
  for (int slot = lane; slot < a.W; slot += FM_WAVE) {
    // pod means over the pods present in the slot (NaN: none)
    float x[K], ci[K];
    const bool present = mvn_pod_means<K>(cur, a.P, a.W, slot, x);
    float d2 = fm_nan();
#pragma unroll
    for (int i = 0; i < K; ++i) ci[i] = fm_nan();
    if (present) {
      d2 = mvn_solve<K>(x, mean, v, il, ci);
      anyv = 1.f;
      sc = fmaxf(sc, sqrtf(fmaxf(d2, 0.f)));
      if (model_ok && d2 > thr2) {
        cnt += 1.f;
        const int names = mvn_names<K>(ci, d2);
        blame |= names;
        if (a.anom_count) mvn_append<K>(names, r, slot, x, a.anom_count, a.anom_cap, a.anom_series, a.anom_col, a.anom_val);
      }
    }
    a.d2[(long long)q * a.W + slot] = d2;
    if (a.contrib) {
      float* co = a.contrib + ((long long)q * a.W + slot) * FM_MVN_MAXK;
#pragma unroll
      for (int i = 0; i < FM_MVN_MAXK; ++i) co[i] = i < K ? ci[i] : 0.f;
    }
  }
  cnt = wave_sum(cnt);
  anyv = wave_max(anyv);
  sc = wave_max(sc);
  blame = wave_or(blame);
  if (lane == 0) {
    const int ic = (int)cnt;
    const int vd = ic > 0 ? 1 : ((anyv > 0.f && model_ok) ? 0 : -1);
    a.count[q] = ic;
    a.verdict[q] = (signed char)vd;
    a.score[q] = sc;
    a.blame[q] = blame;
    if (vd == 1 && a.row_verdict) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        if ((blame & (1 << i)) && atomicExch(&a.raised[r[i]], 1) == 0) {
          // the one claimer of the row this tick: nobody else writes its verdict
          if (a.row_verdict[r[i]] != 1) {
            a.row_verdict[r[i]] = 1;
            if (a.app_id) atomicAdd(&a.app_stats[2 * a.app_id[r[i]]], 1);
          }
        }
      }
    }
  }
}

template <int K>
static void mvn_launch(const MvnGroupArgs& a, int bf16, bool full, int kfirst, hipStream_t st) {
  const dim3 grid((a.Ng + FM_MVN_WAVES - 1) / FM_MVN_WAVES), block(kMvnBlock);
  if (bf16) {
    if (full) hipLaunchKernelGGL((mvn_groups_kernel<bf16_t, true, K>), grid, block, 0, st, a, kfirst);
    else hipLaunchKernelGGL((mvn_groups_kernel<bf16_t, false, K>), grid, block, 0, st, a, kfirst);
  } else {
    if (full) hipLaunchKernelGGL((mvn_groups_kernel<float, true, K>), grid, block, 0, st, a, kfirst);
    else hipLaunchKernelGGL((mvn_groups_kernel<float, false, K>), grid, block, 0, st, a, kfirst);
  }
}

extern "C" int fm_mvn_groups(const MvnGroupArgs* a, int bf16, hipStream_t st) {
  if (a->Ng <= 0) return 0;
  if (a->len < 0 || a->len > a->ring_len || a->head < 0 || a->head >= a->ring_len)
    return (int)hipErrorInvalidValue;
  if (a->N <= 0 || a->W < 0 || a->P < 1 || a->ld < a->ring_len) return (int)hipErrorInvalidValue;
  if (!a->groups || !a->thr2 || !a->blame) return (int)hipErrorInvalidValue;
  if (a->row_verdict && !a->raised) return (int)hipErrorInvalidValue;
  if (a->app_id && !a->app_stats) return (int)hipErrorInvalidValue;
  const int vec = bf16 ? 8 : 4;
  const bool full = a->len == a->ring_len && a->ld % vec == 0 && ((uintptr_t)a->hist % 16) == 0;
  constexpr int all = 0x1fc;   // k = 2..8
  int mask = a->kmask & all;
  if (!mask) mask = all;
  const int kfirst = __builtin_ctz(mask);
  if (mask & (1 << 2)) mvn_launch<2>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 3)) mvn_launch<3>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 4)) mvn_launch<4>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 5)) mvn_launch<5>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 6)) mvn_launch<6>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 7)) mvn_launch<7>(*a, bf16, full, kfirst, st);
  if (mask & (1 << 8)) mvn_launch<8>(*a, bf16, full, kfirst, st);
  return (int)hipGetLastError();
}
