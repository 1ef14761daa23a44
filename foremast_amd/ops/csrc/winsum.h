// Shifted window sums and their Chan merge, shared by the kernels that need a window's
// mean / population variance from a ring row (window.hip K1, robust.hip).
#pragma once
#include "common.h"

// Accumulate shifted sums over physical range [p0, p1) of a row; vector body
// of 16-byte loads, scalar head/tail.
template <typename TIN, int UNR = 6>
__device__ __forceinline__ void acc_range(const TIN* row, int p0, int p1, float& shift, bool& has_shift,
                                          float& n, float& s1, float& s2, int tid, int nt) {
  constexpr int VEC = 16 / sizeof(TIN);
  auto add = [&](float v) {
    if (v == v) {
      if (!has_shift) { shift = v; has_shift = true; }
      const float d = v - shift;
      n += 1.f; s1 += d; s2 += d * d;
    }
  };
  int a0 = p0 + ((VEC - (p0 % VEC)) % VEC);
  if (a0 > p1) a0 = p1;
  for (int i = p0 + tid; i < a0; i += nt) add(to_f32<TIN>(row[i]));
  const int nvec = (p1 - a0) / VEC;
  // UNR 16-byte loads of a thread in flight at once (clamped index, no branch before the
  // loads), then the accumulation: one memory latency per UNR vectors instead of one each
  for (int v0 = tid; v0 < nvec; v0 += nt * UNR) {
    uint4 q[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) q[u] = *(const uint4*)(row + a0 + min(v0 + u * nt, nvec - 1) * VEC);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (v0 + u * nt >= nvec) break;
      if (sizeof(TIN) == 2) {
        const unsigned w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          add(__uint_as_float(w[k] << 16));
          add(__uint_as_float(w[k] & 0xffff0000u));
        }
      } else {
        add(__uint_as_float(q[u].x)); add(__uint_as_float(q[u].y));
        add(__uint_as_float(q[u].z)); add(__uint_as_float(q[u].w));
      }
    }
  }
  for (int i = a0 + nvec * VEC + tid; i < p1; i += nt) add(to_f32<TIN>(row[i]));
}

// (count, mean, sum of squared deviations) of a wave's samples
struct WaveMoments {
  float N, mean, M2;
};

// per-lane (n, mean, M2) -> Chan merge about the count-weighted mean of the lane means
__device__ __forceinline__ WaveMoments chan_merge_wave(float shift, float cnt, float s1, float s2) {
  const float mean_t = cnt > 0.f ? shift + s1 / cnt : 0.f;
  const float m2_t = cnt > 0.f ? fmaxf(s2 - s1 * s1 / cnt, 0.f) : 0.f;
  const float N = wave_sum(cnt);
  const float sm = wave_sum(cnt * mean_t);
  const float ref = N > 0.f ? sm / N : 0.f;
  const float dm = mean_t - ref;
  const float M2 = wave_sum(m2_t + cnt * dm * dm);
  WaveMoments w;
  w.N = N; w.mean = ref; w.M2 = M2;
  return w;
}
