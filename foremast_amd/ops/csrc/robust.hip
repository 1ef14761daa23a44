// robust_average / robust_average_all: lower median, MAD and std of a ring window, with
// the fused detection epilogue.  One 256-thread workgroup per series.
//
// Semantics: foremast_amd/models/robust_average.py.
//
// The window is read from HBM once, with 16-byte loads, into LDS (10,080 points: 20 KB
// bf16, 40 KB fp32), and every later pass runs from there: the shifted sums of the std
// (winsum.h, as K1), the median and the MAD.  A window too long to stage
// (kRobustStageBytes) runs the same passes from the ring itself, element by element.
//
// Both order statistics come from one exact radix select (rb_select) on order-preserving
// unsigned keys: the sign-transformed bits of the sample (16 bits for a bf16 ring, 32 for
// fp32), and the raw bits of |y - centre|, a non-negative fp32.  A pass counts one digit of
// up to 8 bits into a 256-bin LDS histogram with ds_add, a block scan finds the bin that
// holds the wanted rank, and the next pass looks only at the keys of that bin.
//
// Hot bins.  Metric rows live in a narrow range, so the top digits of their keys agree
// and a select that started at bit 31 would send every sample of the row to ONE bin:
// same-address LDS atomics are served one lane at a time, 64 cycles for a wave where
// 64 distinct banks take 2.  Of the two remedies, this kernel takes the row's min and max
// key first (one pass over LDS, wave reductions) and starts the select at the highest
// bit where they differ, rather than keeping a private histogram per lane group:
//  - the first digit then spans the row's actual range, so the samples spread over the
//    bins as their distribution does, and the digits that every key shares cost no pass
//    at all: a bf16 row at level 3000 has 5-6 open bits and is done in ONE pass where
//    the full key needs two, an fp32 row in two or three instead of four;
//  - a constant row (min == max), the worst case for the atomics, needs no pass;
//  - private copies only divide the serialisation by their number and multiply the LDS
//    and the scan; they do nothing about the passes spent on shared digits.
// What the min/max start does NOT remove:
//  - the MAD select.  The centre is a sample, so the smallest |y - centre| is 0, its key is
//    0, and the select always starts at the top set bit of the largest deviation: the first
//    digit is the fp32 exponent byte (typically bits 30..23).  A bell-shaped row puts about
//    a third of its samples into one exponent bin and most of the rest into three or four,
//    on every row, so that pass serialises its ds_add heavily;
//  - a row with an outlier several octaves away (the incident case): min and max keys then
//    differ in the exponent bits and the median's first digit is all exponent as well;
//  - real ties (a row rounded to a few bf16 values).
// Each such ds_add wave-instruction serialises over at most its 64 lanes.  The cost of these
// passes has not been measured on its own; privatised counts for the exponent pass are the
// known next step if the kernel's time (docs/PERF.md) needs it.
#include "common.h"
#include "detect.h"
#include "args.h"
#include "winsum.h"

constexpr int kRobustBlock = 256;
constexpr int kRobustWaves = kRobustBlock / FM_WAVE;
constexpr int kRobustStageBytes = 60 * 1024;  // with RbScratch: inside the 64 KiB a launch gets unasked
constexpr int kRobustPad = 64;                // LDS bytes beyond the window: alignment pads (3 vectors)

extern __shared__ uint4 rb_stage[];

struct RbScratch {
  int hist[256];
  int wtot[kRobustWaves];
  unsigned lo[kRobustWaves], hi[kRobustWaves];
  int cnt[kRobustWaves];
  WaveMoments wm[kRobustWaves];
  int sel, selk;
};

// order-preserving unsigned key of a sample and its inverse (bf16: 16 bits)
template <typename TIN> __device__ __forceinline__ unsigned rb_key(float v);
template <> __device__ __forceinline__ unsigned rb_key<float>(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
template <> __device__ __forceinline__ unsigned rb_key<bf16_t>(float v) {
  const unsigned u = __float_as_uint(v) >> 16;
  return u ^ ((u & 0x8000u) ? 0xffffu : 0x8000u);
}
template <typename TIN> __device__ __forceinline__ float rb_val(unsigned k);
template <> __device__ __forceinline__ float rb_val<float>(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
template <> __device__ __forceinline__ float rb_val<bf16_t>(unsigned k) {
  const unsigned u = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xffffu);
  return __uint_as_float(u << 16);
}

// The window's samples: staged in LDS (pads are NaN), or read from the ring in place.
template <typename TIN, bool STAGED>
struct RbSrc {
  const TIN* p;
  int total, head, R;
  __device__ __forceinline__ float get(int i) const {
    if (STAGED) return to_f32<TIN>(p[i]);
    int c = head + i;
    if (c >= R) c -= R;
    return to_f32<TIN>(p[c]);
  }
};

// Copy physical range [pa, pb) of a row to st[p + delta]; delta keeps 16-byte alignment.
template <typename TIN>
__device__ __forceinline__ void rb_stage_range(const TIN* row, int pa, int pb, TIN* st, int delta, int tid) {
  constexpr int VEC = 16 / sizeof(TIN);
  constexpr int UNR = 4;
  int a0 = pa + ((VEC - (pa % VEC)) % VEC);
  if (a0 > pb) a0 = pb;
  for (int i = pa + tid; i < a0; i += kRobustBlock) st[i + delta] = row[i];
  const int nvec = (pb - a0) / VEC;
  for (int v0 = tid; v0 < nvec; v0 += kRobustBlock * UNR) {
    uint4 q[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      q[u] = *(const uint4*)(row + a0 + min(v0 + u * kRobustBlock, nvec - 1) * VEC);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int v = v0 + u * kRobustBlock;
      if (v < nvec) *(uint4*)(st + a0 + delta + v * VEC) = q[u];
    }
  }
  for (int i = a0 + nvec * VEC + tid; i < pb; i += kRobustBlock) st[i + delta] = row[i];
}

__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, FM_WAVE));
  return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, FM_WAVE));
  return v;
}

// Smallest and largest key and the number of keys.  key(i, k) sets k and returns whether
// slot i holds a sample.
template <typename KeyFn>
__device__ __forceinline__ void rb_minmax(KeyFn key, int total, RbScratch& s, unsigned& kmin, unsigned& kmax,
                                          int& cnt) {
  unsigned lo = 0xffffffffu, hi = 0u;
  int c = 0;
  for (int i = threadIdx.x; i < total; i += kRobustBlock) {
    unsigned k;
    if (key(i, k)) { lo = min(lo, k); hi = max(hi, k); ++c; }
  }
  lo = wave_min_u(lo);
  hi = wave_max_u(hi);
  c = wave_allsum_i(c);
  if (lane_id() == 0) { s.lo[wave_id()] = lo; s.hi[wave_id()] = hi; s.cnt[wave_id()] = c; }
  __syncthreads();
  kmin = s.lo[0]; kmax = s.hi[0]; cnt = s.cnt[0];
#pragma unroll
  for (int w = 1; w < kRobustWaves; ++w) { kmin = min(kmin, s.lo[w]); kmax = max(kmax, s.hi[w]); cnt += s.cnt[w]; }
  __syncthreads();
}

// The key of 0-based rank k (k < number of keys) among keys in [kmin, kmax].  Every
// argument but `key` is the same in all threads, so every barrier is reached by all.
template <typename KeyFn>
__device__ __forceinline__ unsigned rb_select(KeyFn key, int total, int k, unsigned kmin, unsigned kmax,
                                              RbScratch& s) {
  if (kmin == kmax) return kmin;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  int nrem = 32 - __clz((int)(kmin ^ kmax));  // open bits; the ones above are common to every key
  unsigned prefix = nrem >= 32 ? 0u : ((kmin >> nrem) << nrem);
  while (nrem > 0) {
    const int shift = nrem > 8 ? nrem - 8 : 0;
    const unsigned mask = (1u << (nrem - shift)) - 1u;  // at most 8 bits: bins 0 .. 255
    s.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < total; i += kRobustBlock) {
      unsigned kk;
      if (key(i, kk) && (nrem >= 32 || ((kk ^ prefix) >> nrem) == 0u)) atomicAdd(&s.hist[(kk >> shift) & mask], 1);
    }
    __syncthreads();
    // exclusive scan of the 256 bins, one per thread
    const int c = s.hist[tid];
    int inc = c;
#pragma unroll
    for (int o = 1; o < FM_WAVE; o <<= 1) {
      const int t = __shfl_up(inc, o, FM_WAVE);
      if (lane >= o) inc += t;
    }
    if (lane == FM_WAVE - 1) s.wtot[wave] = inc;
    __syncthreads();
    int excl = inc - c;
    for (int w = 0; w < wave; ++w) excl += s.wtot[w];
    if (c > 0 && k >= excl && k < excl + c) { s.sel = tid; s.selk = k - excl; }
    __syncthreads();
    prefix |= (unsigned)s.sel << shift;
    k = s.selk;
    nrem = shift;
  }
  return prefix;
}

template <typename TIN, bool STAGED>
__global__ __launch_bounds__(kRobustBlock) void robust_stats_kernel(const RobustArgs a) {
  __shared__ RbScratch s;
  constexpr int VEC = 16 / sizeof(TIN);
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const TIN* row = (const TIN*)a.hist + (long long)n * a.ld;
  const int R = a.ring_len;
  const int p0 = a.head, p1 = a.head + a.len;
  const int endA = p1 < R ? p1 : R;       // first physical range [p0, endA)
  const int lenB = p1 > R ? p1 - R : 0;   // wrapped range [0, lenB)

  float shift = 0.f, cnt = 0.f, s1 = 0.f, s2 = 0.f;
  bool has = false;
  RbSrc<TIN, STAGED> src;
  src.head = p0;
  src.R = R;
  if (STAGED) {
    // LDS image: [pad | range A | pad][range B | pad], both ranges at the 16-byte phase
    // they have in the row, pads NaN (every pass skips NaN); order does not matter to a
    // selection nor to the sums
    TIN* st = (TIN*)rb_stage;
    const int baseA = p0 - p0 % VEC;
    const int offB = (endA - baseA + VEC - 1) / VEC * VEC;
    const int total = offB + (lenB + VEC - 1) / VEC * VEC;
    const TIN nan = from_f32<TIN>(fm_nan());
    if (tid < VEC) {
      for (int i = tid; i < p0 - baseA; i += VEC) st[i] = nan;
      for (int i = endA - baseA + tid; i < offB; i += VEC) st[i] = nan;
      for (int i = offB + lenB + tid; i < total; i += VEC) st[i] = nan;
    }
    rb_stage_range<TIN>(row, p0, endA, st, -baseA, tid);
    if (lenB > 0) rb_stage_range<TIN>(row, 0, lenB, st, offB, tid);
    __syncthreads();
    src.p = st;
    src.total = total;
    acc_range<TIN, 4>(st, 0, total, shift, has, cnt, s1, s2, tid, kRobustBlock);
  } else {
    src.p = row;
    src.total = a.len;
    acc_range<TIN, 4>(row, p0, endA, shift, has, cnt, s1, s2, tid, kRobustBlock);
    if (lenB > 0) acc_range<TIN, 4>(row, 0, lenB, shift, has, cnt, s1, s2, tid, kRobustBlock);
  }

  // std: the waves' Chan merges, merged once more about their count-weighted mean
  const WaveMoments wmo = chan_merge_wave(shift, cnt, s1, s2);
  if (lane == 0) s.wm[wave] = wmo;
  __syncthreads();
  float N = 0.f, sm = 0.f;
#pragma unroll
  for (int w = 0; w < kRobustWaves; ++w) { N += s.wm[w].N; sm += s.wm[w].N * s.wm[w].mean; }
  const float ref = N > 0.f ? sm / N : 0.f;
  float M2 = 0.f;
#pragma unroll
  for (int w = 0; w < kRobustWaves; ++w) {
    const float dm = s.wm[w].mean - ref;
    M2 += s.wm[w].M2 + s.wm[w].N * dm * dm;
  }
  const float sd = N > 0.f ? sqrtf(fmaxf(M2 / N, 0.f)) : fm_nan();

  // centre: lower median of the samples
  auto key = [&](int i, unsigned& k) {
    const float v = src.get(i);
    k = rb_key<TIN>(v);
    return v == v;
  };
  unsigned kmin, kmax;
  int nv;
  rb_minmax(key, src.total, s, kmin, kmax, nv);
  float center = fm_nan(), mad = fm_nan();
  if (nv > 0) {  // block-uniform
    const int rank = (nv - 1) / 2;
    center = rb_val<TIN>(rb_select(key, src.total, rank, kmin, kmax, s));
    // mad: lower median of |y - centre|, whose fp32 bits order as the values do
    auto dkey = [&](int i, unsigned& k) {
      const float v = src.get(i);
      k = __float_as_uint(fabsf(v - center));
      return v == v;
    };
    int nd;
    rb_minmax(dkey, src.total, s, kmin, kmax, nd);
    mad = __uint_as_float(rb_select(dkey, src.total, rank, kmin, kmax, s));
  }
  const float sigma = mad > 0.f ? 1.4826f * mad : sd;
  if (tid == 0) {
    a.center[n] = center;
    a.mad[n] = mad;
    a.stdv[n] = sd;
    a.sigma[n] = sigma;
    a.count[n] = N;
  }
  if (wave == 0) detect_epilogue_wave(a.det, n, sigma, N, [center](int) { return center; });
}

extern "C" int fm_robust_stats(const RobustArgs* a, int bf16, hipStream_t st) {
  if (a->N <= 0) return 0;
  if (a->len < 0 || a->len > a->ring_len || a->head < 0 || a->head >= a->ring_len || a->ring_len > (1 << 30))
    return (int)hipErrorInvalidValue;
  if (bf16 && (a->ld % 8) != 0) return (int)hipErrorInvalidValue;
  if (!bf16 && (a->ld % 4) != 0) return (int)hipErrorInvalidValue;
  const size_t bytes = (size_t)a->len * (bf16 ? 2 : 4) + kRobustPad;
  const bool staged = bytes <= (size_t)kRobustStageBytes;
  const dim3 grid((unsigned)a->N), block(kRobustBlock);
  if (bf16) {
    if (staged) hipLaunchKernelGGL((robust_stats_kernel<bf16_t, true>), grid, block, bytes, st, *a);
    else hipLaunchKernelGGL((robust_stats_kernel<bf16_t, false>), grid, block, 0, st, *a);
  } else {
    if (staged) hipLaunchKernelGGL((robust_stats_kernel<float, true>), grid, block, bytes, st, *a);
    else hipLaunchKernelGGL((robust_stats_kernel<float, false>), grid, block, 0, st, *a);
  }
  return (int)hipGetLastError();
}
