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
#include "common.h"
#include "args.h"

#ifndef FM_MVN_WAVES
#define FM_MVN_WAVES 4   // groups (waves) per workgroup
#endif
constexpr int kMvnBlock = FM_MVN_WAVES * FM_WAVE;
constexpr float kMvnPivotFloor = 1e-20f;

#define MVN_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))   // i >= j

template <int K>
struct MvnAcc {
  static constexpr int TRI = K * (K + 1) / 2;
  float s[K], a[K], p[TRI];
  float c = 0.f;
  bool has = false;
  __device__ __forceinline__ MvnAcc() {
#pragma unroll
    for (int i = 0; i < K; ++i) { s[i] = 0.f; a[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < TRI; ++i) p[i] = 0.f;
  }
  __device__ __forceinline__ void add(const float (&x)[K]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < K; ++i) ok = ok && (x[i] == x[i]);
    // branch-free: a point with a missing coordinate adds exact zeros; the first jointly
    // valid point of the lane becomes its shift
    const bool first = ok && !has;
    has = has || ok;
    float d[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      s[i] = first ? x[i] : s[i];
      d[i] = ok ? x[i] - s[i] : 0.f;
      a[i] += d[i];
    }
    c += ok ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) p[MVN_TRI(i, j)] += d[i] * d[j];
    }
  }
};

// Physical columns [0, R) of the K rows: 16-byte loads, UNR per row in flight (clamped index,
// no branch before the loads), scalar tail of R % VEC columns.
template <typename TIN, int K, int UNR>
__device__ __forceinline__ void mvn_acc_full(const TIN* const (&row)[K], int R, int lane, MvnAcc<K>& s) {
  constexpr int VEC = 16 / sizeof(TIN);
  const int nvec = R / VEC;
  for (int v0 = lane; v0 < nvec; v0 += FM_WAVE * UNR) {
    uint4 q[UNR][K];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int v = min(v0 + u * FM_WAVE, nvec - 1);
#pragma unroll
      for (int i = 0; i < K; ++i) q[u][i] = *(const uint4*)(row[i] + (long long)v * VEC);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (v0 + u * FM_WAVE >= nvec) break;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        unsigned word[K];
#pragma unroll
        for (int i = 0; i < K; ++i) word[i] = w == 0 ? q[u][i].x : (w == 1 ? q[u][i].y : (w == 2 ? q[u][i].z : q[u][i].w));
        float x[K];
        if (sizeof(TIN) == 2) {
#pragma unroll
          for (int i = 0; i < K; ++i) x[i] = __uint_as_float(word[i] << 16);
          s.add(x);
#pragma unroll
          for (int i = 0; i < K; ++i) x[i] = __uint_as_float(word[i] & 0xffff0000u);
          s.add(x);
        } else {
#pragma unroll
          for (int i = 0; i < K; ++i) x[i] = __uint_as_float(word[i]);
          s.add(x);
        }
      }
    }
  }
  for (int t = nvec * VEC + lane; t < R; t += FM_WAVE) {
    float x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = to_f32<TIN>(row[i][t]);
    s.add(x);
  }
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, FM_WAVE);
  return v;
}

// leading non-negative entries of a group's row table
__device__ __forceinline__ int mvn_group_k(const int* g) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < FM_MVN_MAXK; ++i) {
    if (k == i && g[i] >= 0) k = i + 1;
  }
  return k;
}

template <typename TIN, bool FULL, int K>
__global__ __launch_bounds__(kMvnBlock) void mvn_groups_kernel(const MvnGroupArgs a, const int kfirst) {
  constexpr int TRI = K * (K + 1) / 2;
  constexpr int UNR = K <= 2 ? 5 : (K == 3 ? 3 : (K <= 5 ? 2 : 1));
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
    for (int t = lane; t < a.len; t += FM_WAVE) {
      int p = a.head + t;
      if (p >= a.ring_len) p -= a.ring_len;
      float x[K];
#pragma unroll
      for (int i = 0; i < K; ++i) x[i] = to_f32<TIN>(row[i][p]);
      s.add(x);
    }
  }
  // per-lane centred moments, merged about a wave-common centre (see bivariate.hip)
  const float c = s.c;
  const float rc = c > 0.f ? 1.f / c : 0.f;
  const float N = wave_sum(c);
  const float rN = N > 0.f ? 1.f / N : 0.f;
  float mean[K], dm[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const float m0 = wave_sum(c > 0.f ? c * (s.s[i] + s.a[i] * rc) : 0.f) * rN;
    const float u_t = c > 0.f ? (s.s[i] - m0) + s.a[i] * rc : 0.f;
    const float u = wave_sum(c * u_t) * rN;
    mean[i] = m0 + u;
    dm[i] = u_t - u;
  }
  const float inv = 1.f / fmaxf(N, 1.f);
  float v[TRI];
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const float cij = c > 0.f ? s.p[MVN_TRI(i, j)] - s.a[i] * s.a[j] * rc : 0.f;
      v[MVN_TRI(i, j)] = wave_sum(cij + c * dm[i] * dm[j]) * inv;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < FM_MVN_MAXK; ++i) a.mean[(long long)q * FM_MVN_MAXK + i] = i < K ? mean[i] : 0.f;
#pragma unroll
    for (int i = 0; i < FM_MVN_TRI; ++i) a.cov[(long long)q * FM_MVN_TRI + i] = i < TRI ? v[i] : 0.f;
    a.nvalid[q] = N;
  }
  // Cholesky factor of cov + eps I in place: v[(i, j)] = L[i][j] (j < i), il[i] = 1 / L[i][i]
  float il[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int i = j; i < K; ++i) {
      float t = v[MVN_TRI(i, j)] + (i == j ? a.eps : 0.f);
#pragma unroll
      for (int m = 0; m < j; ++m) t -= v[MVN_TRI(i, m)] * v[MVN_TRI(j, m)];
      if (i == j) {
        if (t < kMvnPivotFloor) t = kMvnPivotFloor;
        il[j] = 1.f / sqrtf(t);
      } else {
        v[MVN_TRI(i, j)] = t * il[j];
      }
    }
  }
  const float thr2 = a.thr2[q];
  const bool model_ok = N >= (float)a.min_valid;
  const float* cur[K];
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = a.cur + (long long)r[i] * a.ld_cur;
  float cnt = 0.f, anyv = 0.f, sc = 0.f;
  int blame = 0;
  for (int slot = lane; slot < a.W; slot += FM_WAVE) {
    // pod means over the pods present in the slot (NaN: none)
    float sp[K], np[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { sp[i] = 0.f; np[i] = 0.f; }
    for (int p = 0; p < a.P; ++p) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float x = cur[i][p * a.W + slot];
        if (x == x) { sp[i] += x; np[i] += 1.f; }
      }
    }
    bool present = true;
#pragma unroll
    for (int i = 0; i < K; ++i) present = present && np[i] > 0.f;
    float d2 = fm_nan();
    float x[K], ci[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { x[i] = fm_nan(); ci[i] = fm_nan(); }
    if (present) {
      float d[K], z[K], w[K];
#pragma unroll
      for (int i = 0; i < K; ++i) { x[i] = sp[i] / np[i]; d[i] = x[i] - mean[i]; }
      d2 = 0.f;
#pragma unroll
      for (int i = 0; i < K; ++i) {   // z = L^-1 d
        float t = d[i];
#pragma unroll
        for (int m = 0; m < i; ++m) t -= v[MVN_TRI(i, m)] * z[m];
        z[i] = t * il[i];
        d2 += z[i] * z[i];
      }
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {   // w = L^-T z
        float t = z[i];
#pragma unroll
        for (int m = i + 1; m < K; ++m) t -= v[MVN_TRI(m, i)] * w[m];
        w[i] = t * il[i];
        ci[i] = d[i] * w[i];
      }
      anyv = 1.f;
      sc = fmaxf(sc, sqrtf(fmaxf(d2, 0.f)));
      if (model_ok && d2 > thr2) {
        cnt += 1.f;
        const float line = d2 * (1.f / K);
        int top = 0;
        float best = ci[0];
        int names = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
          if (i > 0 && ci[i] > best) { best = ci[i]; top = i; }
          if (ci[i] >= line) names |= 1 << i;
        }
        names |= 1 << top;
        blame |= names;
        if (a.anom_count) {
#pragma unroll
          for (int i = 0; i < K; ++i) {
            if (names & (1 << i)) {
              const int at = atomicAdd(a.anom_count, 1);
              if (at < a.anom_cap) {
                a.anom_series[at] = r[i];
                a.anom_col[at] = slot;
                a.anom_val[at] = x[i];
              }
            }
          }
        }
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
