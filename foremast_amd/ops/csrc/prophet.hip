// Window-scaled Prophet scorer (ML_ALGORITHM=prophet on streaming shards).
//
// Model: foremast_amd/models/prophet_lite.py fit_prophet_window.  Every series of a ring
// shares the design matrix X [T, P] (time scaled by the window), so the fit is a ridge
// regression against shared tables:
//
//   rhs = sum_valid x_t y_t,   A_n = A_dense - sum_missing x_t x_t'   (A_dense = X'X + reg),
//   beta = A_n^-1 rhs,   sigma = sqrt(sum_valid (y_t - x_t beta)^2 / max(n - P, 1)).
//
// Four launches:
//   1. prophet_fit_kernel     lane = series, the window split over the waves of a workgroup:
//                             rhs with the X rows as wave-uniform (scalar) operands, the
//                             missing-sample bit mask, and for a gap-free series the solve
//                             with the shared Cholesky factor.  A gapped series leaves its
//                             rhs and is appended to a device-side list.
//   2. prophet_gapped_kernel  one wave per listed series: A_n from the mask (downdate from
//                             A_dense, or reg + sum_valid when more than half the window is
//                             missing; whole 32-sample words from a prefix table of x x'),
//                             Cholesky with one matrix row per lane, solve.
//   3. prophet_resid_kernel   lane = series: second pass over the window for sum r^2.
//   4. prophet_detect_kernel  band / verdict epilogue, one 16-lane row per series.
//
// The resident rollout engine fits once per job and scores every tick at growing horizons:
//   fm_prophet_fit_state     launches 1-3, then prophet_state_kernel (lane = series): the
//                            forecast state level / slope / harm[14] from beta.
//   fm_prophet_state_detect  prophet_state_detect_kernel: the band / verdict epilogue with the
//                            forecast evaluated from the state at any horizon in 1..2^20.
//
// The tables are padded from P to PP in {12, 20, 26, 32} columns (zero features, unit
// diagonal): the padded coefficients are exactly 0 and the inner loops unroll over PP.
#include "args.h"
#include "detect.h"

struct ProphetArgs {
  const void* hist;     // [N, ld] ring (bf16 or fp32)
  long long ld;
  int ring_len;
  int head;             // physical column of logical t = 0
  int T;                // logical window length
  int N;
  int bf16;
  int P;                // model terms
  int PP;               // padded terms (table row stride)
  int hmax;             // rows of XH: every horizon is in 1..hmax
  const float* X;       // [T, PP]
  const float* XH;      // [hmax, PP] features of logical index T-1+h
  const float* A;       // [PP, PP] A_dense
  const float* L;       // [PP, PP] lower Cholesky factor of A_dense, diagonal replaced by 1 / L[k][k]
  const float* LT;      // [PP, PP] its transpose
  const float* reg;     // [PP] ridge
  const float* XXp;     // [T + 1, PP (PP + 1) / 2] prefix sums of x_t x_t' (lower triangle, row-major)
  float* beta;          // [N, PP]
  float* sigma;         // [N]
  float* nvalid;        // [N]
  unsigned* mask;       // [N, ceil(ring_len / 32)] missing in-window samples by physical column
  int* defer;           // [N + 1] count (zero between calls), gapped series
  int S;                // waves per workgroup of the two streaming kernels
  int _pad;
  DetectArgs det;
};

extern __shared__ __attribute__((aligned(16))) char fm_pr_smem[];

namespace {

// tables in the constant address space: wave-uniform reads become scalar loads
typedef const __attribute__((address_space(4))) float* CF;
__device__ __forceinline__ CF as_const(const float* p) { return (CF)(unsigned long long)p; }

template <typename TIN> struct Raw8;
template <> struct Raw8<bf16_t> {
  uint4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *(const uint4*)p; }
  __device__ __forceinline__ void load_part(const bf16_t* p, int cnt) {  // cnt < 8 columns exist
    unsigned e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = i < cnt ? (unsigned)p[i] : 0u;
    v = uint4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
  }
  __device__ __forceinline__ void zero() { v = uint4{0u, 0u, 0u, 0u}; }
  __device__ __forceinline__ float get(int j) const {
    const unsigned u = (j >> 1) == 0 ? v.x : ((j >> 1) == 1 ? v.y : ((j >> 1) == 2 ? v.z : v.w));
    return __uint_as_float((j & 1) ? (u & 0xffff0000u) : (u << 16));
  }
};
template <> struct Raw8<float> {
  v4f a, b;
  __device__ __forceinline__ void load(const float* p) { a = *(const v4f*)p; b = *(const v4f*)(p + 4); }
  __device__ __forceinline__ void load_part(const float* p, int cnt) {
    float e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = i < cnt ? p[i] : 0.f;
    a = v4f{e[0], e[1], e[2], e[3]};
    b = v4f{e[4], e[5], e[6], e[7]};
  }
  __device__ __forceinline__ void zero() { a = b = v4f{0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ float get(int j) const {
    const v4f q = j < 4 ? a : b;
    return (j & 3) == 0 ? q.x : ((j & 3) == 1 ? q.y : ((j & 3) == 2 ? q.z : q.w));
  }
};

// the 32 physical columns of quad q (four 16-byte groups); columns past the ring read as 0
template <typename TIN>
__device__ __forceinline__ void load_quad(const TIN* row, int q, int R, Raw8<TIN>* raw) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int p0 = 32 * q + 8 * g;  // wave-uniform
    if (p0 + 8 <= R) raw[g].load(row + p0);
    else if (p0 < R) raw[g].load_part(row + p0, R - p0);
    else raw[g].zero();
  }
}

// Walks the quads [q0, q1) of one ring row: sample(t, bit, y) for every in-window column
// (t, bit wave-uniform; y may be NaN), end_quad(q) after each quad.  The next quad's loads
// are issued before the current one is consumed.
template <typename TIN, typename FS, typename FQ>
__device__ __forceinline__ void walk_window(const TIN* row, int q0, int q1, int R, int head, int T, FS sample,
                                            FQ end_quad) {
  const int e1 = min(head + T, R), e2 = head + T - R;  // the window: columns [head, e1) and [0, e2)
  Raw8<TIN> nxt[4];
  if (q0 < q1) load_quad<TIN>(row, q0, R, nxt);
  for (int q = q0; q < q1; ++q) {
    Raw8<TIN> cur[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) cur[g] = nxt[g];
    if (q + 1 < q1) load_quad<TIN>(row, q + 1, R, nxt);
    const int p0 = 32 * q;
    int t0 = -1;  // >= 0: the quad lies inside the window, logical t0 .. t0 + 31
    if (p0 >= head && p0 + 32 <= e1) t0 = p0 - head;
    else if (p0 + 32 <= e2) t0 = p0 + R - head;
    if (t0 >= 0) {  // no per-sample branch: the table rows of the quad are loaded in batches
#pragma unroll
      for (int i = 0; i < 32; ++i) sample(t0 + i, i, cur[i >> 3].get(i & 7));
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int p = p0 + 8 * g + j;
          int t = p - head;
          t += t < 0 ? R : 0;
          if (p < R && t < T) sample(t, 8 * g + j, cur[g].get(j));
        }
      }
    }
    end_quad(q);
  }
}

// ---- 1. rhs, mask, dense solve ----------------------------------------------------------
template <typename TIN, int PP>
__global__ __launch_bounds__(512) void prophet_fit_kernel(const ProphetArgs a) {
  const int S = blockDim.x >> 6;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  const int n = blockIdx.x * FM_WAVE + lane;
  const bool live = n < a.N;
  const int R = a.ring_len, Q = (R + 31) >> 5;
  const TIN* row = (const TIN*)a.hist + (long long)(live ? n : a.N - 1) * a.ld;
  unsigned* mrow = a.mask + (long long)(live ? n : a.N - 1) * Q;
  const CF X = as_const(a.X);
  float acc[PP], loc[PP];
#pragma unroll
  for (int k = 0; k < PP; ++k) acc[k] = loc[k] = 0.f;
  int nmiss = 0;
  unsigned mw = 0u;
  const int q0 = (int)((long long)w * Q / S), q1 = (int)((long long)(w + 1) * Q / S);
  walk_window<TIN>(
      row, q0, q1, R, a.head, a.T,
      [&](int t, int bit, float y) {
        const bool ok = y == y;
        const float yv = ok ? y : 0.f;
        mw |= ok ? 0u : (1u << bit);
        const CF xr = X + (long long)t * PP;
#pragma unroll
        for (int k = 0; k < PP; ++k) loc[k] = fmaf(xr[k], yv, loc[k]);
      },
      [&](int q) {
#pragma unroll
        for (int k = 0; k < PP; ++k) {  // two-level sum: the rounding error grows with 32 + quads, not T
          acc[k] += loc[k];
          loc[k] = 0.f;
        }
        if (live) mrow[q] = mw;
        nmiss += __popc(mw);
        mw = 0u;
      });
  // sum the waves' partial rhs (wave 0 finishes the series)
  float* red = (float*)fm_pr_smem;  // [S - 1][PP + 1][64]
  if (w > 0) {
    float* r = red + (long long)(w - 1) * (PP + 1) * FM_WAVE + lane;
#pragma unroll
    for (int k = 0; k < PP; ++k) r[k * FM_WAVE] = acc[k];
    r[PP * FM_WAVE] = (float)nmiss;
  }
  __syncthreads();
  if (w > 0) return;
  float fm = (float)nmiss;
  for (int v = 1; v < S; ++v) {
    const float* r = red + (long long)(v - 1) * (PP + 1) * FM_WAVE + lane;
#pragma unroll
    for (int k = 0; k < PP; ++k) acc[k] += r[k * FM_WAVE];
    fm += r[PP * FM_WAVE];
  }
  if (!live) return;
  a.nvalid[n] = (float)a.T - fm;
  float* bo = a.beta + (long long)n * PP;
  if (fm > 0.f) {  // gapped: leave the rhs, the per-series kernel solves it
#pragma unroll
    for (int k = 0; k < PP; ++k) bo[k] = acc[k];
    const int slot = atomicAdd(a.defer, 1);
    if (slot < a.N) a.defer[1 + slot] = n;
    return;
  }
  // gap-free: L z = rhs, L' beta = z with the shared factor (scalar operands; the diagonals
  // hold 1 / L[k][k], and the backward sweep reads the transposed copy row-wise)
  const CF L = as_const(a.L), LT = as_const(a.LT);
#pragma unroll
  for (int k = 0; k < PP; ++k) {
    float z = acc[k];
#pragma unroll
    for (int j = 0; j < k; ++j) z = fmaf(-L[k * PP + j], acc[j], z);
    acc[k] = z * L[k * PP + k];
  }
#pragma unroll
  for (int k = PP - 1; k >= 0; --k) {
    float z = acc[k];
#pragma unroll
    for (int i = k + 1; i < PP; ++i) z = fmaf(-LT[k * PP + i], acc[i], z);
    acc[k] = z * LT[k * PP + k];
  }
#pragma unroll
  for (int k = 0; k < PP; ++k) bo[k] = acc[k];
}

// ---- 2. gapped series: per-series normal matrix, Cholesky, solve -------------------------
__device__ __forceinline__ float lane_bcast(float v, int src) {  // src wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// bits of word q (physical columns 32q .. 32q+31) inside [lo, hi)
__device__ __forceinline__ unsigned range_bits(int q, int lo, int hi) {
  const int b0 = max(lo - 32 * q, 0), b1 = min(hi - 32 * q, 32);
  if (b1 <= b0) return 0u;
  const unsigned upto1 = b1 >= 32 ? 0xffffffffu : ((1u << b1) - 1u);
  return upto1 & ~((1u << b0) - 1u);  // b0 < 32 here
}

template <int PP>
__global__ __launch_bounds__(256) void prophet_gapped_kernel(const ProphetArgs a) {
  constexpr int NE = PP * (PP + 1) / 2, KE = (NE + FM_WAVE - 1) / FM_WAVE;
  constexpr int U = KE <= 4 ? 4 : 2;  // samples accumulated per round
  const int lane = lane_id(), wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  float* As = (float*)fm_pr_smem + wv * PP * PP;  // this wave's matrix
  const int R = a.ring_len, Q = (R + 31) >> 5, T = a.T, head = a.head;
  // lower-triangle entries owned by this lane: e = lane + 64 k  ->  (i, j), j <= i
  int ei[KE], ej[KE];
#pragma unroll
  for (int k = 0; k < KE; ++k) {
    const int e = lane + FM_WAVE * k;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    ei[k] = e < NE ? i : 0;
    ej[k] = e < NE ? e - i * (i + 1) / 2 : 0;
  }
  // the window as physical column ranges [head, e1) and [0, e2)
  const int e1 = min(head + T, R), e2 = max(head + T - R, 0);
  const int cnt = min(a.defer[0], a.N);
  for (int li = blockIdx.x * nw + wv; li < cnt; li += gridDim.x * nw) {
    const int n = __builtin_amdgcn_readfirstlane(a.defer[1 + li]);
    const unsigned* mrow = a.mask + (long long)n * Q;
    const float nv = a.nvalid[n];
    const bool use_valid = 2.f * nv < (float)T;  // fewer valid than missing samples: sum the valid side
    float acc[KE];
#pragma unroll
    for (int k = 0; k < KE; ++k) acc[k] = 0.f;
    for (int qb = 0; qb < Q; qb += FM_WAVE) {
      const int q = qb + lane;
      unsigned word = q < Q ? mrow[q] : 0u;
      if (use_valid) word = q < Q ? (~word & (range_bits(q, head, e1) | range_bits(q, 0, e2))) : 0u;
      // a word whose 32 columns are consecutive in-window samples, all set: runs of such
      // words come from the prefix table of x x' (two table rows per run, not 32 samples
      // per word) -- an outage costs what a handful of isolated misses cost
      int t0 = -1;
      if (q < Q) {
        const int p0 = 32 * q;
        if (p0 >= head && p0 + 32 <= e1) t0 = p0 - head;
        else if (p0 + 32 <= e2) t0 = p0 + R - head;
      }
      const bool full = t0 >= 0 && word == 0xffffffffu;
      const unsigned pword = __shfl_up(word, 1, FM_WAVE);
      const int pt0 = __shfl_up(t0, 1, FM_WAVE);
      const bool start = full && !(lane > 0 && pword == 0xffffffffu && pt0 >= 0 && pt0 + 32 == t0);
      const unsigned long long fmk = __ballot(full);
      unsigned long long smk = __ballot(start);
      if (full) word = 0u;
      while (smk) {
        const int s = __builtin_ctzll(smk);
        smk &= smk - 1;
        int e = s + 1;  // the run ends at the next word that is not full or starts another run
        while (e < FM_WAVE && ((fmk >> e) & 1ull) && !((smk >> e) & 1ull)) ++e;
        const int ts = __builtin_amdgcn_readlane(t0, s), te = ts + 32 * (e - s);
        const float* pa = a.XXp + (long long)ts * NE;
        const float* pb = a.XXp + (long long)te * NE;
#pragma unroll
        for (int k = 0; k < KE; ++k)
          if (lane + FM_WAVE * k < NE) acc[k] += pb[lane + FM_WAVE * k] - pa[lane + FM_WAVE * k];
      }
      unsigned long long bal = __ballot(word != 0u);
      while (bal) {
        const int src = __builtin_ctzll(bal);
        bal &= bal - 1;
        unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)word, src);
        while (bits) {
          // U samples per round: their table reads are all in flight before the first FMA
          // (a round short of samples re-reads its first one and skips the FMAs)
          float xi[U][KE], xj[U][KE];
          bool has[U];
          int tf = 0;
#pragma unroll
          for (int u = 0; u < U; ++u) {
            has[u] = bits != 0u;
            const int b = has[u] ? __builtin_ctz(bits) : 0;
            bits = has[u] ? (bits & (bits - 1)) : 0u;
            int t = 32 * (qb + src) + b - head;
            t += t < 0 ? R : 0;
            if (u == 0) tf = t;
            const float* xr = a.X + (long long)(has[u] ? t : tf) * PP;
#pragma unroll
            for (int k = 0; k < KE; ++k) {
              xi[u][k] = xr[ei[k]];
              xj[u][k] = xr[ej[k]];
            }
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (has[u]) {  // wave-uniform
#pragma unroll
              for (int k = 0; k < KE; ++k) acc[k] = fmaf(xi[u][k], xj[u][k], acc[k]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KE; ++k) {
      if (lane + FM_WAVE * k < NE) {
        const int i = ei[k], j = ej[k];
        const float v = use_valid ? ((i == j ? a.reg[i] : 0.f) + acc[k]) : (a.A[i * PP + j] - acc[k]);
        As[i * PP + j] = v;
        As[j * PP + i] = v;
      }
    }
    // the matrix is private to this wave: order its LDS writes before the row reads
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // lane i holds row i (lanes >= PP: zeros)
    float Ar[PP];
#pragma unroll
    for (int j = 0; j < PP; ++j) Ar[j] = lane < PP ? As[lane * PP + j] : 0.f;
    float z = lane < PP ? a.beta[(long long)n * PP + lane] : 0.f;  // rhs
    const float dfl = lane < PP ? a.reg[lane] : 1.f;
#pragma unroll
    for (int k = 0; k < PP; ++k) {
      float akk = lane_bcast(Ar[k], k);
      // a non-positive pivot (rounding of a nearly singular matrix): fall back to the ridge
      if (!(akk > 0.f)) akk = lane_bcast(dfl, k);
      const float rinv = 1.f / sqrtf(akk);
      const float lik = Ar[k] * rinv;  // L[i][k] for lanes i >= k
      Ar[k] = lane == k ? akk * rinv : lik;
#pragma unroll
      for (int j = k + 1; j < PP; ++j) Ar[j] = fmaf(-lik, lane_bcast(lik, j), Ar[j]);
    }
    // forward: L y = rhs (column sweep)
#pragma unroll
    for (int k = 0; k < PP; ++k) {
      const float zk = lane_bcast(z, k) / lane_bcast(Ar[k], k);
      z = lane == k ? zk : (lane > k ? fmaf(-Ar[k], zk, z) : z);
    }
    // backward: L' x = y (x_k needs the lanes above k)
    float x = 0.f;
#pragma unroll
    for (int k = PP - 1; k >= 0; --k) {
      const float s = wave_allsum(lane > k ? Ar[k] * x : 0.f);
      const float xk = (lane_bcast(z, k) - s) / lane_bcast(Ar[k], k);
      x = lane == k ? xk : x;
    }
    if (lane < PP) a.beta[(long long)n * PP + lane] = x;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- 3. residual pass ------------------------------------------------------------------
template <typename TIN, int PP>
__global__ __launch_bounds__(512) void prophet_resid_kernel(const ProphetArgs a) {
  const int S = blockDim.x >> 6;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
  const int n = blockIdx.x * FM_WAVE + lane;
  const bool live = n < a.N;
  const int R = a.ring_len, Q = (R + 31) >> 5;
  // the gapped kernel has drained the list: clear its count for the next call
  if (blockIdx.x == 0 && threadIdx.x == 0) a.defer[0] = 0;
  const TIN* row = (const TIN*)a.hist + (long long)(live ? n : a.N - 1) * a.ld;
  const CF X = as_const(a.X);
  float b[PP];
  {
    const float* bi = a.beta + (long long)(live ? n : a.N - 1) * PP;
#pragma unroll
    for (int k = 0; k < PP; ++k) b[k] = bi[k];
  }
  float ss = 0.f;
  const int q0 = (int)((long long)w * Q / S), q1 = (int)((long long)(w + 1) * Q / S);
  walk_window<TIN>(
      row, q0, q1, R, a.head, a.T,
      [&](int t, int, float y) {
        const CF xr = X + (long long)t * PP;
        float f0 = 0.f, f1 = 0.f;  // two chains
#pragma unroll
        for (int k = 0; k + 1 < PP; k += 2) {
          f0 = fmaf(xr[k], b[k], f0);
          f1 = fmaf(xr[k + 1], b[k + 1], f1);
        }
        const float r = y - (f0 + f1);
        ss += (y == y) ? r * r : 0.f;
      },
      [&](int) {});
  float* red = (float*)fm_pr_smem;  // [S][64]
  red[w * FM_WAVE + lane] = ss;
  __syncthreads();
  if (w > 0 || !live) return;
  float tot = 0.f;
  for (int v = 0; v < S; ++v) tot += red[v * FM_WAVE + lane];
  const float dof = fmaxf(a.nvalid[n] - (float)a.P, 1.f);
  a.sigma[n] = sqrtf(tot / dof);
}

// ---- 4. band / verdict -------------------------------------------------------------------
__global__ __launch_bounds__(256) void prophet_detect_kernel(const ProphetArgs a) {
  const int n = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
  if (n >= a.N) return;  // row-uniform
  const float* be = a.beta + (long long)n * a.PP;
  const float* XH = a.XH;
  const int PP = a.PP, hm = a.hmax;
  detect_epilogue_row(a.det, n, a.sigma[n], a.nvalid[n], [&](int hz) {
    const float* xh = XH + (long long)(min(max(hz, 1), hm) - 1) * PP;  // the host guarantees 1 <= hz <= hmax
    float f = 0.f;
    for (int k = 0; k < PP; ++k) f = fmaf(xh[k], be[k], f);
    return f;
  });
}

// ---- 5. harmonic forecast state (resident rollout engine) --------------------------------
// Past the window every hinge is active, so the model is a line plus the Fourier terms with
// their phase moved to the window's last sample (models/prophet_lite.py window_state):
//   f(h) = level + slope h + sum_j [A_j sin(w_j h) + B_j cos(w_j h)].
// A row of any window length has the same state, so rows fitted at different geometries are
// scored by one launch.
constexpr int PS_NH = 7;         // harmonics: 4 daily, 3 weekly
constexpr int PS_HARM = 14;      // A_1..4, B_1..4 (daily), A_1..3, B_1..3 (weekly)
constexpr int PS_TAB_CP = 16;    // table: [0] 1 / (T - 1), [1..7] cos th_j, [8..14] sin th_j, [16 + k] 1 - c_k
constexpr int PS_HZ_MAX = 1 << 20;

struct ProphetStateOut {
  const float* tab;     // [16 + ncp] rotation table of the (T, m) geometry (fp64 on the host, cast)
  float* level;         // [N]
  float* slope;         // [N]
  float* harm;          // [N, 14]
  int ncp;              // changepoints
  int nd;               // daily order in beta (4 or 0)
  int nw;               // weekly order in beta (3 or 0)
  int _pad;
};

struct ProphetStateArgs {
  const float* level;   // [N]
  const float* slope;   // [N]
  const float* harm;    // [N, 14]
  const float* sigma;   // [N]
  const float* nvalid;  // [N]
  int N;
  int m;                // samples per day
  DetectArgs det;
};

// lane = series: the rotation constants are wave-uniform (scalar) operands
__global__ __launch_bounds__(256) void prophet_state_kernel(const float* __restrict__ beta, int PP, int N,
                                                            const ProphetStateOut s) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const CF tab = as_const(s.tab);
  const float* b = beta + (long long)n * PP;
  const int K = s.ncp;
  float lv = b[0] + b[1], ds = b[1];
  for (int k = 0; k < K; ++k) {
    const float d = b[2 + k];
    lv = fmaf(d, tab[PS_TAB_CP + k], lv);
    ds += d;
  }
  s.level[n] = lv;
  s.slope[n] = ds * tab[0];
  float* ho = s.harm + (long long)n * PS_HARM;
  int src = 2 + K;
  // daily (order 4) then weekly (order 3): beta holds sin 1..order, cos 1..order of an enabled season
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int order = q == 0 ? 4 : 3, on = q == 0 ? s.nd : s.nw, j0 = q == 0 ? 0 : 4, dst = q == 0 ? 0 : 8;
#pragma unroll
    for (int k = 0; k < order; ++k) {
      float A = 0.f, B = 0.f;
      if (on) {  // wave-uniform
        const float as = b[src + k], ac = b[src + order + k];
        const float c = tab[1 + j0 + k], sn = tab[1 + PS_NH + j0 + k];
        A = fmaf(as, c, -(ac * sn));
        B = fmaf(as, sn, ac * c);
      }
      ho[dst + k] = A;
      ho[dst + order + k] = B;
    }
    src += on ? 2 * order : 0;
  }
}

// sum_k [A_k sin(2 pi k h / p) + B_k cos(2 pi k h / p)], k = 1..ORDER, with the phase reduced in
// integers: r_k = (k h) mod p by repeated addition of r_1 (h <= 2^20, p <= 7 * 86400: every
// value fits 32 bits and converts to fp32 exactly), so the accuracy does not decay with h
template <int ORDER>
__device__ __forceinline__ float harm_sum(const float* hc, unsigned h, unsigned p) {
  const unsigned r1 = h % p;
  const float ip2 = 2.f / (float)p;
  unsigned r = 0u;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < ORDER; ++k) {
    r += r1;
    r -= r >= p ? p : 0u;
    float sn, cs;
    sincospif((float)r * ip2, &sn, &cs);
    acc = fmaf(hc[k], sn, acc);
    acc = fmaf(hc[ORDER + k], cs, acc);
  }
  return acc;
}

// band / verdict from the cached state, one 16-lane row per series (as prophet_detect_kernel)
__global__ __launch_bounds__(256) void prophet_state_detect_kernel(const ProphetStateArgs a) {
  const int n = blockIdx.x * (blockDim.x / 16) + (threadIdx.x >> 4);
  if (n >= a.N) return;  // row-uniform
  const float lv = a.level[n], sl = a.slope[n];
  float hc[PS_HARM];
  const float* hp = a.harm + (long long)n * PS_HARM;
  float dmag = 0.f, wmag = 0.f;
#pragma unroll
  for (int k = 0; k < PS_HARM; ++k) {
    hc[k] = hp[k];
    if (k < 8) dmag += fabsf(hc[k]);
    else wmag += fabsf(hc[k]);
  }
  // a season the row's window did not enable holds zeros (row-uniform: one series per row)
  const bool daily = dmag != 0.f, weekly = wmag != 0.f;
  const unsigned m = (unsigned)a.m;
  detect_epilogue_row(a.det, n, a.sigma[n], a.nvalid[n], [&](int hz) {
    const unsigned h = (unsigned)min(max(hz, 1), PS_HZ_MAX);
    float f = fmaf(sl, (float)h, lv);
    if (daily) f += harm_sum<4>(hc, h, m);
    if (weekly) f += harm_sum<3>(hc + 8, h, 7u * m);
    return f;
  });
}

template <typename TIN, int PP>
int launch_prophet(const ProphetArgs* a, hipStream_t st) {
  const int S = a->S;
  const int blocks = (a->N + FM_WAVE - 1) / FM_WAVE;
  const size_t lds1 = (size_t)(S - 1) * (PP + 1) * FM_WAVE * sizeof(float);
  hipLaunchKernelGGL((prophet_fit_kernel<TIN, PP>), dim3(blocks), dim3(S * FM_WAVE), lds1, st, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // grid-stride over the device-side list (its length is only known on the device)
  const int gw = 4, ggrid = min((a->N + gw - 1) / gw, 2048);
  hipLaunchKernelGGL((prophet_gapped_kernel<PP>), dim3(ggrid), dim3(gw * FM_WAVE), gw * PP * PP * sizeof(float), st,
                     *a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((prophet_resid_kernel<TIN, PP>), dim3(blocks), dim3(S * FM_WAVE), S * FM_WAVE * sizeof(float),
                     st, *a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (a->det.C > 0) hipLaunchKernelGGL(prophet_detect_kernel, dim3((a->N + 15) / 16), dim3(256), 0, st, *a);
  return (int)hipGetLastError();
}

template <typename TIN>
int launch_prophet_pp(const ProphetArgs* a, hipStream_t st) {
  switch (a->PP) {
    case 12: return launch_prophet<TIN, 12>(a, st);
    case 20: return launch_prophet<TIN, 20>(a, st);
    case 26: return launch_prophet<TIN, 26>(a, st);
    case 32: return launch_prophet<TIN, 32>(a, st);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace

extern "C" long long fm_prophet_args_size() { return (long long)sizeof(ProphetArgs); }

static bool prophet_fit_args_ok(const ProphetArgs* a) {
  const int per16 = a->bf16 ? 8 : 4;
  return !(a->T < 2 || a->T > a->ring_len || a->head < 0 || a->head >= a->ring_len || a->P < 1 || a->P > a->PP ||
           a->S < 1 || a->S > 8 || a->ld < a->ring_len || a->ld % per16 != 0 ||
           (((unsigned long long)a->hist) & 15ull) != 0 || !a->X || !a->A || !a->L || !a->LT || !a->reg ||
           !a->XXp || !a->beta || !a->sigma || !a->nvalid || !a->mask || !a->defer);
}

extern "C" int fm_prophet_score(const ProphetArgs* a, hipStream_t st) {
  if (a->N <= 0) return 0;
  if (!prophet_fit_args_ok(a) || a->hmax < 1 || a->hmax > 64 || !a->XH) return (int)hipErrorInvalidValue;
  return a->bf16 ? launch_prophet_pp<bf16_t>(a, st) : launch_prophet_pp<float>(a, st);
}

extern "C" long long fm_prophet_state_out_size() { return (long long)sizeof(ProphetStateOut); }
extern "C" long long fm_prophet_state_args_size() { return (long long)sizeof(ProphetStateArgs); }

// The fit, gapped and residual launches of fm_prophet_score with no detection epilogue
// (beta / sigma / nvalid are the same bits), then the forecast state of every series.
extern "C" int fm_prophet_fit_state(const ProphetArgs* a, const ProphetStateOut* s, hipStream_t st) {
  if (a->N <= 0) return 0;
  if (!prophet_fit_args_ok(a) || a->det.C != 0 || !s->tab || !s->level || !s->slope || !s->harm || s->ncp < 0 ||
      !(s->nd == 0 || s->nd == 4) || !(s->nw == 0 || s->nw == 3) || 2 + s->ncp + 2 * (s->nd + s->nw) != a->P)
    return (int)hipErrorInvalidValue;
  const int rc = a->bf16 ? launch_prophet_pp<bf16_t>(a, st) : launch_prophet_pp<float>(a, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(prophet_state_kernel, dim3((a->N + 255) / 256), dim3(256), 0, st, a->beta, a->PP, a->N, *s);
  return (int)hipGetLastError();
}

extern "C" int fm_prophet_state_detect(const ProphetStateArgs* a, hipStream_t st) {
  if (a->N <= 0 || a->det.C <= 0) return 0;
  if (!a->level || !a->slope || !a->harm || !a->sigma || !a->nvalid || a->m < 2 || a->m > 86400)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(prophet_state_detect_kernel, dim3((a->N + 15) / 16), dim3(256), 0, st, *a);
  return (int)hipGetLastError();
}
