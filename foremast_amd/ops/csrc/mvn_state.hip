// The k-variate normal as a resident state (2 <= k <= 8): the joint model of the rollout
// engine's multi-metric jobs under ML_ALGORITHM=multivariate_normal.  mvn_groups.hip fits and
// scores in one launch because a streaming shard's history moves every tick; a rollout job's
// history ends at its start, so its model is fitted ONCE at admission and only the k x k
// solves run per tick.
//
// Semantics: foremast_amd/models/multivariate_normal.py (mvn_state / score_state).  The
// arithmetic is mvn_groups.hip's (mvn_common.h): shifted moment sums over the jointly valid
// points, wave-common-centre merge, Cholesky of cov + eps I with the pivot floor, z = L^-1 d,
// d^2 = |z|^2, c_i = d_i (L^-T z)_i, named iff c_i >= d^2 / k (the largest always).
//
// fm_mvn_fit_state: one wave per group.  The k rows of a group are rows of the resident ring,
// read in place; every group has its own window length (a job's history ends at its start:
// len = R - the ring's newer points), so one launch serves an admission batch whatever its
// start times.  len == R and 16-byte aligned rows take the physical-order 16-byte walk, the
// rest the wrapped one-element walk (wave-uniform).
// The state is written at row dst[q] of the tables: mean, cov, the packed factor (L below the
// diagonal, 1 / L[i][i] on it) and nvalid.
//
// fm_mvn_state_detect: 16 lanes per group, four groups per wave.  A window has W = 11 slots by
// default: a whole wave per group would idle 53 lanes.  Every lane of a group holds the
// group's state in registers and scores the slots sub, sub + 16, ...; count, score and blame
// are reduced over the group's own 16 lanes (xor shuffles of 8, 4, 2, 1 stay inside them).
// The groups of a wave may differ in k: a launch of another k masks those lanes off.
#include "mvn_common.h"

#ifndef FM_MVN_WAVES
#define FM_MVN_WAVES 4   // groups (waves) per workgroup of the fit
#endif
constexpr int kFitBlock = FM_MVN_WAVES * FM_WAVE;
constexpr int kSub = 16;                         // lanes per group of the detect
constexpr int kDetBlock = 256;
constexpr int kDetGroups = kDetBlock / kSub;     // groups per workgroup

template <typename TIN, int K>
__global__ __launch_bounds__(kFitBlock) void mvn_fit_state_kernel(const MvnFitStateArgs a, const int kfirst) {
  constexpr int TRI = K * (K + 1) / 2;
  const int q = blockIdx.x * FM_MVN_WAVES + wave_id();
  if (q >= a.Ng) return;  // wave-uniform, as every branch below
  const int lane = lane_id();
  const int d = a.dst[q];
  if ((unsigned)d >= (unsigned)a.S) return;
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
  float* om = a.mean + (long long)d * FM_MVN_MAXK;
  float* oc = a.cov + (long long)d * FM_MVN_TRI;
  float* ol = a.chol + (long long)d * FM_MVN_TRI;
  if (!inside) {
    // fewer than two rows, or a row outside the ring: nothing is read, the state is unusable
    if (lane < FM_MVN_MAXK) om[lane] = fm_nan();
    if (lane < FM_MVN_TRI) { oc[lane] = fm_nan(); ol[lane] = fm_nan(); }
    if (lane == 0) a.nvalid[d] = 0.f;
    return;
  }
  const TIN* row[K];
  bool aligned = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    row[i] = (const TIN*)a.hist + (long long)r[i] * a.ld;
    aligned = aligned && ((uintptr_t)row[i] & 15) == 0;
  }
  const int len = min(max(a.len[q], 0), a.ring_len);
  MvnAcc<K> s;
  if (len == a.ring_len && aligned) {
    mvn_acc_full<TIN, K, MvnUnroll<K>::value>(row, a.ring_len, lane, s);
  } else {
    mvn_acc_wrapped<TIN, K>(row, a.ring_len, a.head, len, lane, s);
  }
  float mean[K], v[TRI], N;
  mvn_merge<K>(s, mean, v, N);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < FM_MVN_MAXK; ++i) om[i] = i < K ? mean[i] : 0.f;
#pragma unroll
    for (int i = 0; i < FM_MVN_TRI; ++i) oc[i] = i < TRI ? v[i] : 0.f;
    a.nvalid[d] = N;
  }
  float il[K];
  mvn_cholesky<K>(v, il, a.eps);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) ol[MVN_TRI(i, j)] = i == j ? il[i] : v[MVN_TRI(i, j)];
    }
#pragma unroll
    for (int i = TRI; i < FM_MVN_TRI; ++i) ol[i] = 0.f;
  }
}

__device__ __forceinline__ float sub_sum(float v) {
#pragma unroll
  for (int o = kSub / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kSub);
  return v;
}
__device__ __forceinline__ float sub_max(float v) {
#pragma unroll
  for (int o = kSub / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kSub));
  return v;
}
__device__ __forceinline__ int sub_or(int v) {
#pragma unroll
  for (int o = kSub / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, kSub);
  return v;
}

template <int K>
__global__ __launch_bounds__(kDetBlock) void mvn_state_detect_kernel(const MvnStateDetectArgs a, const int kfirst) {
  constexpr int TRI = K * (K + 1) / 2;
  const int sub = threadIdx.x & (kSub - 1);
  const int q = blockIdx.x * kDetGroups + threadIdx.x / kSub;
  if (q >= a.Ng) return;   // uniform over a group's 16 lanes, as every branch before the slot loop
  const int srow = a.active[q];
  const bool live = (unsigned)srow < (unsigned)a.S;
  const int* g = a.groups + (long long)(live ? srow : 0) * FM_MVN_MAXK;
  const int k = live ? mvn_group_k(g) : 0;
  if (k != K && !(k < 2 && K == kfirst)) return;
  int r[K];
  bool inside = k == K;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    r[i] = inside ? g[i] : 0;
    inside = inside && (unsigned)r[i] < (unsigned)a.N;
  }
  if (!inside) {
    // no such state row, fewer than two rows, or a row outside the table: unscored
    for (int j = sub; j < a.W; j += kSub) a.d2[(long long)q * a.W + j] = fm_nan();
    if (a.contrib) {
      for (int j = sub; j < a.W * FM_MVN_MAXK; j += kSub) a.contrib[(long long)q * a.W * FM_MVN_MAXK + j] = fm_nan();
    }
    if (sub == 0) { a.count[q] = 0; a.verdict[q] = -1; a.score[q] = 0.f; a.blame[q] = 0; }
    return;
  }
  float mean[K], v[TRI], il[K];
  const float* sm = a.mean + (long long)srow * FM_MVN_MAXK;
  const float* sl = a.chol + (long long)srow * FM_MVN_TRI;
#pragma unroll
  for (int i = 0; i < K; ++i) mean[i] = sm[i];
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const float t = sl[MVN_TRI(i, j)];
      if (i == j) { il[i] = t; v[MVN_TRI(i, j)] = 0.f; } else { v[MVN_TRI(i, j)] = t; }
    }
  }
  const float thr2 = a.thr2[srow];
  const bool model_ok = a.nvalid[srow] >= (float)a.min_valid;
  const float* cur[K];
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = a.cur + (long long)r[i] * a.ld_cur;
  float cnt = 0.f, anyv = 0.f, sc = 0.f;
  int blame = 0;
  for (int slot = sub; slot < a.W; slot += kSub) {
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
  cnt = sub_sum(cnt);
  anyv = sub_max(anyv);
  sc = sub_max(sc);
  blame = sub_or(blame);
  if (sub == 0) {
    const int ic = (int)cnt;
    a.count[q] = ic;
    a.verdict[q] = (signed char)(ic > 0 ? 1 : ((anyv > 0.f && model_ok) ? 0 : -1));
    a.score[q] = sc;
    a.blame[q] = blame;
  }
}

template <int K>
static void fit_launch(const MvnFitStateArgs& a, int bf16, int kfirst, hipStream_t st) {
  const dim3 grid((a.Ng + FM_MVN_WAVES - 1) / FM_MVN_WAVES), block(kFitBlock);
  if (bf16) hipLaunchKernelGGL((mvn_fit_state_kernel<bf16_t, K>), grid, block, 0, st, a, kfirst);
  else hipLaunchKernelGGL((mvn_fit_state_kernel<float, K>), grid, block, 0, st, a, kfirst);
}

template <int K>
static void detect_launch(const MvnStateDetectArgs& a, int kfirst, hipStream_t st) {
  const dim3 grid((a.Ng + kDetGroups - 1) / kDetGroups), block(kDetBlock);
  hipLaunchKernelGGL((mvn_state_detect_kernel<K>), grid, block, 0, st, a, kfirst);
}

static int mvn_kmask(int kmask) {
  constexpr int all = 0x1fc;   // k = 2..8
  const int mask = kmask & all;
  return mask ? mask : all;
}

extern "C" int fm_mvn_fit_state(const MvnFitStateArgs* a, int bf16, hipStream_t st) {
  if (a->Ng <= 0) return 0;
  if (a->ring_len < 1 || a->head < 0 || a->head >= a->ring_len) return (int)hipErrorInvalidValue;
  if (a->N <= 0 || a->S <= 0 || a->ld < a->ring_len) return (int)hipErrorInvalidValue;
  if (!a->hist || !a->groups || !a->len || !a->dst) return (int)hipErrorInvalidValue;
  if (!a->mean || !a->cov || !a->chol || !a->nvalid) return (int)hipErrorInvalidValue;
  const int mask = mvn_kmask(a->kmask);
  const int kfirst = __builtin_ctz(mask);
  if (mask & (1 << 2)) fit_launch<2>(*a, bf16, kfirst, st);
  if (mask & (1 << 3)) fit_launch<3>(*a, bf16, kfirst, st);
  if (mask & (1 << 4)) fit_launch<4>(*a, bf16, kfirst, st);
  if (mask & (1 << 5)) fit_launch<5>(*a, bf16, kfirst, st);
  if (mask & (1 << 6)) fit_launch<6>(*a, bf16, kfirst, st);
  if (mask & (1 << 7)) fit_launch<7>(*a, bf16, kfirst, st);
  if (mask & (1 << 8)) fit_launch<8>(*a, bf16, kfirst, st);
  return (int)hipGetLastError();
}

extern "C" int fm_mvn_state_detect(const MvnStateDetectArgs* a, hipStream_t st) {
  if (a->Ng <= 0) return 0;
  if (a->N <= 0 || a->S <= 0 || a->W < 1 || a->P < 1 || a->ld_cur < (long long)a->P * a->W)
    return (int)hipErrorInvalidValue;
  if (!a->mean || !a->chol || !a->nvalid || !a->thr2 || !a->groups || !a->active || !a->cur)
    return (int)hipErrorInvalidValue;
  if (!a->d2 || !a->count || !a->verdict || !a->score || !a->blame) return (int)hipErrorInvalidValue;
  if (a->anom_count && (!a->anom_series || !a->anom_col || !a->anom_val)) return (int)hipErrorInvalidValue;
  const int mask = mvn_kmask(a->kmask);
  const int kfirst = __builtin_ctz(mask);
  if (mask & (1 << 2)) detect_launch<2>(*a, kfirst, st);
  if (mask & (1 << 3)) detect_launch<3>(*a, kfirst, st);
  if (mask & (1 << 4)) detect_launch<4>(*a, kfirst, st);
  if (mask & (1 << 5)) detect_launch<5>(*a, kfirst, st);
  if (mask & (1 << 6)) detect_launch<6>(*a, kfirst, st);
  if (mask & (1 << 7)) detect_launch<7>(*a, kfirst, st);
  if (mask & (1 << 8)) detect_launch<8>(*a, kfirst, st);
  return (int)hipGetLastError();
}
