// The k-variate normal's shared device code (2 <= k <= 8): the shifted moment accumulator, the
// 16-byte ring walk, the wave-common-centre merge, the in-register Cholesky factor and the
// per-slot solve / attribution / naming.  Used by mvn_groups.hip (fit + score in one launch,
// streaming shard) and mvn_state.hip (fit once at admission, score every tick; rollout engine).
// Semantics: foremast_amd/models/multivariate_normal.py.
//
// k is a template parameter everywhere: every accumulator and factor array is indexed by
// unrolled constants and stays in registers.
#pragma once

#include "common.h"
#include "args.h"

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

// rows in flight per lane of the 16-byte walk, by k (register budget)
template <int K>
struct MvnUnroll {
  static constexpr int value = K <= 2 ? 5 : (K == 3 ? 3 : (K <= 5 ? 2 : 1));
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

// The logical window [head, head + len) of a ring of R columns, one element per load.
template <typename TIN, int K>
__device__ __forceinline__ void mvn_acc_wrapped(const TIN* const (&row)[K], int R, int head, int len, int lane,
                                                MvnAcc<K>& s) {
  for (int t = lane; t < len; t += FM_WAVE) {
    int p = head + t;
    if (p >= R) p -= R;
    float x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = to_f32<TIN>(row[i][p]);
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

// Per-lane centred moments merged about a wave-common centre (bivariate.hip explains why
// never as absolute values): the mean, the packed biased covariance and the jointly valid
// count N, in every lane.
template <int K>
__device__ __forceinline__ void mvn_merge(const MvnAcc<K>& s, float (&mean)[K], float (&v)[K * (K + 1) / 2], float& N) {
  const float c = s.c;
  const float rc = c > 0.f ? 1.f / c : 0.f;
  N = wave_sum(c);
  const float rN = N > 0.f ? 1.f / N : 0.f;
  float dm[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const float m0 = wave_sum(c > 0.f ? c * (s.s[i] + s.a[i] * rc) : 0.f) * rN;
    const float u_t = c > 0.f ? (s.s[i] - m0) + s.a[i] * rc : 0.f;
    const float u = wave_sum(c * u_t) * rN;
    mean[i] = m0 + u;
    dm[i] = u_t - u;
  }
  const float inv = 1.f / fmaxf(N, 1.f);
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const float cij = c > 0.f ? s.p[MVN_TRI(i, j)] - s.a[i] * s.a[j] * rc : 0.f;
      v[MVN_TRI(i, j)] = wave_sum(cij + c * dm[i] * dm[j]) * inv;
    }
  }
}

// Cholesky factor of cov + eps I in place: v[(i, j)] = L[i][j] (j < i), il[i] = 1 / L[i][i]
// (the diagonal slots of v keep the covariance and are not read again).
template <int K>
__device__ __forceinline__ void mvn_cholesky(float (&v)[K * (K + 1) / 2], float (&il)[K], float eps) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int i = j; i < K; ++i) {
      float t = v[MVN_TRI(i, j)] + (i == j ? eps : 0.f);
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
}

// Pod means of one window slot over the pods present (column p * W + slot of each row);
// false when some metric has no pod in the slot.
template <int K>
__device__ __forceinline__ bool mvn_pod_means(const float* const (&cur)[K], int P, int W, int slot, float (&x)[K]) {
  float sp[K], np[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { sp[i] = 0.f; np[i] = 0.f; }
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const float y = cur[i][p * W + slot];
      if (y == y) { sp[i] += y; np[i] += 1.f; }
    }
  }
  bool present = true;
#pragma unroll
  for (int i = 0; i < K; ++i) present = present && np[i] > 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) x[i] = present ? sp[i] / np[i] : fm_nan();
  return present;
}

// One point: z = L^-1 (x - mean), d^2 = |z|^2, and the additive attribution
// c_i = (x - mean)_i (L^-T z)_i.
template <int K>
__device__ __forceinline__ float mvn_solve(const float (&x)[K], const float (&mean)[K],
                                           const float (&v)[K * (K + 1) / 2], const float (&il)[K], float (&ci)[K]) {
  float d[K], z[K], w[K];
#pragma unroll
  for (int i = 0; i < K; ++i) d[i] = x[i] - mean[i];
  float d2 = 0.f;
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
  return d2;
}

// Metrics named on an anomalous point: c_i >= d^2 / k, the largest c_i always (ties: the first).
template <int K>
__device__ __forceinline__ int mvn_names(const float (&ci)[K], float d2) {
  const float line = d2 * (1.f / K);
  int top = 0;
  float best = ci[0];
  int names = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    if (i > 0 && ci[i] > best) { best = ci[i]; top = i; }
    if (ci[i] >= line) names |= 1 << i;
  }
  return names | (1 << top);
}

// K9 list: (row of a named metric, slot, that metric's pod mean) per named metric.
template <int K>
__device__ __forceinline__ void mvn_append(int names, const int (&r)[K], int slot, const float (&x)[K], int* anom_count,
                                           int anom_cap, int* anom_series, int* anom_col, float* anom_val) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    if (names & (1 << i)) {
      const int at = atomicAdd(anom_count, 1);
      if (at < anom_cap) {
        anom_series[at] = r[i];
        anom_col[at] = slot;
        anom_val[at] = x[i];
      }
    }
  }
}
