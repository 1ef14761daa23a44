// K8 over row pairs of one ring: the bivariate normal of a streaming shard's two-metric jobs.
//
// Semantics: foremast_amd/models/bivariate.py (the same as bivariate.hip).  Both metrics of a
// pair are rows of ONE [N, ld] history ring; the current values are the pod means of the
// [N, P*W] window ring (column p * W + slot).  One wave per pair: the two rows are streamed
// once with shifted moment sums over the jointly valid points, the lane means are merged
// relative to a wave-common centre (bivariate.hip explains why never as absolute values),
// then every window slot is scored by squared Mahalanobis distance; anomaly iff the model is
// ok and d^2 > thr^2, thr the raw threshold of the pair's first row.
//
// A full ring (len == ring_len: every streaming tick) is walked in physical order 0..R-1 with
// 16-byte loads, the moments do not depend on the order; a partial or wrapped window takes
// the scalar path.  A flagged pair raises its first row's verdict and counts the row once in
// the per-app table (several pairs may share a row: the first to exchange raised[row] does
// it), and appends its anomalous slots to the K9 list.
#include "common.h"
#include "args.h"

#ifndef FM_BIVP_WAVES
#define FM_BIVP_WAVES 4   // pairs (waves) per workgroup
#endif
constexpr int kBivpBlock = FM_BIVP_WAVES * FM_WAVE;

struct BivAcc {
  float sx = 0.f, sy = 0.f, c = 0.f, ax = 0.f, ay = 0.f, axx = 0.f, axy = 0.f, ayy = 0.f;
  bool has = false;
  __device__ __forceinline__ void add(float x, float y) {
    if (x == x && y == y) {
      if (!has) { sx = x; sy = y; has = true; }
      const float dx = x - sx, dy = y - sy;
      c += 1.f; ax += dx; ay += dy; axx += dx * dx; axy += dx * dy; ayy += dy * dy;
    }
  }
};

// Physical columns [0, R) of both rows: 16-byte loads, UNR per row in flight (clamped index,
// no branch before the loads), scalar tail of R % VEC columns.
template <typename TIN, int UNR>
__device__ __forceinline__ void bivp_acc_full(const TIN* rx, const TIN* ry, int R, int lane, BivAcc& s) {
  constexpr int VEC = 16 / sizeof(TIN);
  const int nvec = R / VEC;
  for (int v0 = lane; v0 < nvec; v0 += FM_WAVE * UNR) {
    uint4 qx[UNR], qy[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int v = min(v0 + u * FM_WAVE, nvec - 1);
      qx[u] = *(const uint4*)(rx + (long long)v * VEC);
      qy[u] = *(const uint4*)(ry + (long long)v * VEC);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (v0 + u * FM_WAVE >= nvec) break;
      const unsigned wx[4] = {qx[u].x, qx[u].y, qx[u].z, qx[u].w};
      const unsigned wy[4] = {qy[u].x, qy[u].y, qy[u].z, qy[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (sizeof(TIN) == 2) {
          s.add(__uint_as_float(wx[k] << 16), __uint_as_float(wy[k] << 16));
          s.add(__uint_as_float(wx[k] & 0xffff0000u), __uint_as_float(wy[k] & 0xffff0000u));
        } else {
          s.add(__uint_as_float(wx[k]), __uint_as_float(wy[k]));
        }
      }
    }
  }
  for (int i = nvec * VEC + lane; i < R; i += FM_WAVE) s.add(to_f32<TIN>(rx[i]), to_f32<TIN>(ry[i]));
}

template <typename TIN, bool FULL>
__global__ __launch_bounds__(kBivpBlock) void bivariate_pairs_kernel(const BivPairArgs a) {
  const int q = blockIdx.x * FM_BIVP_WAVES + wave_id();
  if (q >= a.Np) return;  // wave-uniform
  const int lane = lane_id();
  const int r0 = a.pairs[2 * (long long)q], r1 = a.pairs[2 * (long long)q + 1];
  if ((unsigned)r0 >= (unsigned)a.N || (unsigned)r1 >= (unsigned)a.N) {
    // a row outside the ring: nothing is read, the pair is reported unscored
    for (int k = lane; k < a.W; k += FM_WAVE) a.d2[(long long)q * a.W + k] = fm_nan();
    if (lane < 2) a.mean[2 * (long long)q + lane] = fm_nan();
    if (lane < 3) a.cov[3 * (long long)q + lane] = fm_nan();
    if (lane == 0) { a.nvalid[q] = 0.f; a.count[q] = 0; a.verdict[q] = -1; a.score[q] = 0.f; }
    return;
  }
  const TIN* rx = (const TIN*)a.hist + (long long)r0 * a.ld;
  const TIN* ry = (const TIN*)a.hist + (long long)r1 * a.ld;
  BivAcc s;
  if (FULL) {
    bivp_acc_full<TIN, 5>(rx, ry, a.ring_len, lane, s);
  } else {
    for (int i = lane; i < a.len; i += FM_WAVE) {
      int p = a.head + i;
      if (p >= a.ring_len) p -= a.ring_len;
      s.add(to_f32<TIN>(rx[p]), to_f32<TIN>(ry[p]));
    }
  }
  const float c = s.c;
  // per-lane centred moments, merged about a wave-common centre (see bivariate.hip)
  const float cxx_t = c > 0.f ? s.axx - s.ax * s.ax / c : 0.f;
  const float cxy_t = c > 0.f ? s.axy - s.ax * s.ay / c : 0.f;
  const float cyy_t = c > 0.f ? s.ayy - s.ay * s.ay / c : 0.f;
  const float N = wave_sum(c);
  float mx0 = wave_sum(c > 0.f ? c * (s.sx + s.ax / c) : 0.f);
  float my0 = wave_sum(c > 0.f ? c * (s.sy + s.ay / c) : 0.f);
  mx0 = N > 0.f ? mx0 / N : 0.f;
  my0 = N > 0.f ? my0 / N : 0.f;
  const float ux_t = c > 0.f ? (s.sx - mx0) + s.ax / c : 0.f;
  const float uy_t = c > 0.f ? (s.sy - my0) + s.ay / c : 0.f;
  float ux = wave_sum(c * ux_t), uy = wave_sum(c * uy_t);
  ux = N > 0.f ? ux / N : 0.f;
  uy = N > 0.f ? uy / N : 0.f;
  const float mx = mx0 + ux, my = my0 + uy;
  const float dmx = ux_t - ux, dmy = uy_t - uy;
  const float Sxx = wave_sum(cxx_t + c * dmx * dmx);
  const float Sxy = wave_sum(cxy_t + c * dmx * dmy);
  const float Syy = wave_sum(cyy_t + c * dmy * dmy);
  const float inv = 1.f / fmaxf(N, 1.f);
  const float vxx = Sxx * inv + a.eps, vxy = Sxy * inv, vyy = Syy * inv + a.eps;
  float det = vxx * vyy - vxy * vxy;
  if (fabsf(det) < 1e-20f) det = 1e-20f;
  if (lane == 0) {
    a.mean[2 * (long long)q] = mx;
    a.mean[2 * (long long)q + 1] = my;
    a.cov[3 * (long long)q] = vxx - a.eps;
    a.cov[3 * (long long)q + 1] = vxy;
    a.cov[3 * (long long)q + 2] = vyy - a.eps;
    a.nvalid[q] = N;
  }
  const float thr = a.threshold[r0];
  const float thr2 = thr * thr;
  const bool model_ok = N >= (float)a.min_valid;
  const float* cx = a.cur + (long long)r0 * a.ld_cur;
  const float* cy = a.cur + (long long)r1 * a.ld_cur;
  float cnt = 0.f, anyv = 0.f, sc = 0.f;
  for (int k = lane; k < a.W; k += FM_WAVE) {
    // pod means over the pods present in the slot (NaN: none)
    float sxp = 0.f, syp = 0.f, nx = 0.f, ny = 0.f;
    for (int p = 0; p < a.P; ++p) {
      const float x = cx[p * a.W + k], y = cy[p * a.W + k];
      if (x == x) { sxp += x; nx += 1.f; }
      if (y == y) { syp += y; ny += 1.f; }
    }
    float d2 = fm_nan();
    if (nx > 0.f && ny > 0.f) {
      const float x = sxp / nx, y = syp / ny;
      const float dx = x - mx, dy = y - my;
      d2 = (vyy * dx * dx - 2.f * vxy * dx * dy + vxx * dy * dy) / det;
      anyv = 1.f;
      sc = fmaxf(sc, sqrtf(fmaxf(d2, 0.f)));
      if (model_ok && d2 > thr2) {
        cnt += 1.f;
        if (a.anom_count) {
          const int slot = atomicAdd(a.anom_count, 1);
          if (slot < a.anom_cap) {
            a.anom_series[slot] = r0;
            a.anom_col[slot] = k;
            a.anom_val[slot] = x;
          }
        }
      }
    }
    a.d2[(long long)q * a.W + k] = d2;
  }
  cnt = wave_sum(cnt);
  anyv = wave_max(anyv);
  sc = wave_max(sc);
  if (lane == 0) {
    const int ic = (int)cnt;
    const int v = ic > 0 ? 1 : ((anyv > 0.f && model_ok) ? 0 : -1);
    a.count[q] = ic;
    a.verdict[q] = (signed char)v;
    a.score[q] = sc;
    if (v == 1 && a.row_verdict && atomicExch(&a.raised[r0], 1) == 0) {
      // the one claimer of the row this tick: nobody else writes its verdict
      if (a.row_verdict[r0] != 1) {
        a.row_verdict[r0] = 1;
        if (a.app_id) atomicAdd(&a.app_stats[2 * a.app_id[r0]], 1);
      }
    }
  }
}

extern "C" int fm_bivariate_pairs(const BivPairArgs* a, int bf16, hipStream_t st) {
  if (a->Np <= 0) return 0;
  if (a->len < 0 || a->len > a->ring_len || a->head < 0 || a->head >= a->ring_len)
    return (int)hipErrorInvalidValue;
  if (a->N <= 0 || a->W < 0 || a->P < 1 || a->ld < a->ring_len) return (int)hipErrorInvalidValue;
  if (a->row_verdict && !a->raised) return (int)hipErrorInvalidValue;
  if (a->app_id && !a->app_stats) return (int)hipErrorInvalidValue;
  const int vec = bf16 ? 8 : 4;
  const bool full = a->len == a->ring_len && a->ld % vec == 0 && ((uintptr_t)a->hist % 16) == 0;
  const dim3 grid((a->Np + FM_BIVP_WAVES - 1) / FM_BIVP_WAVES), block(kBivpBlock);
  if (bf16) {
    if (full) hipLaunchKernelGGL((bivariate_pairs_kernel<bf16_t, true>), grid, block, 0, st, *a);
    else hipLaunchKernelGGL((bivariate_pairs_kernel<bf16_t, false>), grid, block, 0, st, *a);
  } else {
    if (full) hipLaunchKernelGGL((bivariate_pairs_kernel<float, true>), grid, block, 0, st, *a);
    else hipLaunchKernelGGL((bivariate_pairs_kernel<float, false>), grid, block, 0, st, *a);
  }
  return (int)hipGetLastError();
}
