// K16: fused k-means Lloyd step for MANY k-means runs at once — assignment + SSE + centroid
// partial sums in ONE pass over the data, then a deterministic device reduction and a device
// centroid update, so an iteration is three launches and one 4-byte-per-run host read
// (CDNA4, gfx950).
//
// Reference: KmeansCluster (J/cluster/KmeansCluster.java, one MR job per iteration: mapper
// assigns each record to its nearest centroid (ClusterMapper.map :154-172), reducer averages
// (ClusterReducer.reduce :233-297)) and the Spark job that runs many (numClusters, initGroup)
// instances keyed by group (S/cluster/KmeansCluster.scala:103-156).
//
// Centroid layout ("pair layout"): the centroids of all R runs are concatenated, every run padded
// to an even count with dummy centroids (norm = +inf, never chosen), and stored interleaved in
// pairs: C2[j/2][d][j&1].  That lets one v_pk_fma_f32 score a row against TWO centroids, with the
// centroid pair arriving as one 64-bit SGPR operand (wave-uniform -> scalar loads, constant cache).
//
// kmeans_mfma_kernel: each lane owns one data row of a 64-row wave tile (the next tile's row is
// prefetched into registers while the current one is scored), keeps it in registers and scores it
// against every centroid pair of every run with packed FMAs.  The per-run argmin goes to a
// wave-private LDS strip and the centroid partial sums become a GEMM on the matrix cores:
//     sums[c][d] += sum_r onehot[c][r] * x[r][d]
// issued as v_mfma_f32_16x16x4_f32 with A = one-hot(assignments) (16 centroids x 4 rows) and
// B = the staged row tile (4 rows x 16 dims), accumulating in registers over the wave's rows.
// Counts are one LDS integer atomic per row and run.  Workgroup partials [grid, K, D + 1].
// kmeans_step_kernel (fallback, more than 16 centroid x dim blocks of 16): centroids and
// accumulators in LDS, per-row ds_add.
// kmeans_reduce_kernel: fixed-order fp64 sum of the workgroup partials (deterministic).
// kmeans_update_kernel: new centroids (mean, or unchanged when empty / run frozen), their norms,
// and the per-run maximum centroid movement (the reference's convergence test).
// D in {2,4,8,16,32,64} (host pads with zeros), R <= 16 runs per launch.
//
// Measured (MI355X, 16.7 M rows x 16 dims, k = 16): 384 us per pass; the same kernel with the
// scoring and the MFMAs removed streams the data in 182 us (5.9 TB/s), so the pass is bound by the
// f32 scoring VALU work (16 packed FMAs + argmin per centroid pair per row), not by HBM.
#include <cstdlib>
#include <string>

#include "avenir_common.h"
#include "avenir_kernels.h"

namespace {

constexpr int KB = 256;
constexpr int MAX_RUNS = 16;  // per-run SSE lives in (statically indexed) registers
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// split-bf16 helpers of the kmeans_score_kernel SB variants (see there): RNE pack of two floats
// (v_cvt_pk_bf16_f32) and the values of a packed pair back in fp32
__device__ __forceinline__ unsigned km_pack(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2v));
}
__device__ __forceinline__ float km_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float km_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }
// 4 floats -> T bf16 terms, term t as two packed u32 (dims 0,1 | 2,3)
template <int T>
__device__ __forceinline__ void km_split4(float v0, float v1, float v2, float v3, unsigned (&o)[T][2]) {
  float r[4] = {v0, v1, v2, v3};
#pragma unroll
  for (int t = 0; t < T; ++t) {
    o[t][0] = km_pack(r[0], r[1]);
    o[t][1] = km_pack(r[2], r[3]);
    if (t + 1 < T) {
      r[0] -= km_lo(o[t][0]); r[1] -= km_hi(o[t][0]);
      r[2] -= km_lo(o[t][1]); r[3] -= km_hi(o[t][1]);
    }
  }
}
__device__ __forceinline__ bf16x8 km_frag(unsigned a0, unsigned a1, unsigned b0, unsigned b1) {
  return __builtin_bit_cast(bf16x8, (u32x4){a0, a1, b0, b1});
}

__device__ __forceinline__ float pair_at(const float* C2, int D, int j, int d) {
  return C2[(long long)(j >> 1) * 2 * D + 2 * d + (j & 1)];
}

template <int D>
__device__ __forceinline__ void load_row(const float* __restrict__ X, long long row, bool ok, float (&x)[D]) {
  if constexpr (D % 4 == 0) {
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const float4 v = ok ? *reinterpret_cast<const float4*>(X + row * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = ok ? X[row * D + d] : 0.f;
  }
}

// Score x against the pair-layout centroids [j0, j1) (both even): best squared distance - ||x||^2.
// Two packed-FMA chains (even / odd dims) so consecutive FMAs do not depend on each other.
template <int D>
__device__ __forceinline__ void score_run(const float (&x)[D], const float* __restrict__ C2,
                                          const float* __restrict__ Cn, int j0, int j1, float& best, int& bj) {
  best = INFINITY;
  bj = j0;
  for (int j = j0; j < j1; j += 2) {
    const f32x2* c = reinterpret_cast<const f32x2*>(C2 + (long long)j * D);  // wave-uniform: s_load
    const f32x2 cn = *reinterpret_cast<const f32x2*>(Cn + j);
    f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
    for (int d = 0; d < D; d += 2) {
      a0 = __builtin_elementwise_fma((f32x2){x[d], x[d]}, c[d], a0);
      if (d + 1 < D) a1 = __builtin_elementwise_fma((f32x2){x[d + 1], x[d + 1]}, c[d + 1], a1);
    }
    const f32x2 acc = a0 + a1;
    const float d0 = cn.x - 2.f * acc.x, d1 = cn.y - 2.f * acc.y;
    if (d0 < best) { best = d0; bj = j; }
    if (d1 < best) { best = d1; bj = j + 1; }
  }
}

template <int D>
__global__ __launch_bounds__(KB) void kmeans_step_kernel(const float* __restrict__ X, long long n,
                                                         const float* __restrict__ C2, const float* __restrict__ Cn,
                                                         const int* __restrict__ roff, int R,
                                                         int* __restrict__ assign, float* __restrict__ partial,
                                                         double* __restrict__ sse_partial) {
  extern __shared__ float lds[];
  __shared__ int s_off[MAX_RUNS + 1];
  __shared__ double red[KB / 64][MAX_RUNS];
  for (int i = threadIdx.x; i <= R; i += KB) s_off[i] = roff[i];
  __syncthreads();
  const int K = s_off[R];
  float* cen = lds;                 // [K][D]
  float* cnorm = cen + K * D;       // [K]
  float* acc = cnorm + K;           // [K][D + 1]
  for (int i = threadIdx.x; i < K * D; i += KB) cen[i] = pair_at(C2, D, i / D, i % D);
  for (int i = threadIdx.x; i < K; i += KB) cnorm[i] = Cn[i];
  for (int i = threadIdx.x; i < K * (D + 1); i += KB) acc[i] = 0.f;
  __syncthreads();
  double sse[MAX_RUNS];
#pragma unroll
  for (int r = 0; r < MAX_RUNS; ++r) sse[r] = 0.0;
  const long long stride = (long long)gridDim.x * KB;
  for (long long row = (long long)blockIdx.x * KB + threadIdx.x; row < n; row += stride) {
    float x[D];
    load_row<D>(X, row, true, x);
    float xn = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) xn = fmaf(x[d], x[d], xn);
#pragma unroll
    for (int r = 0; r < MAX_RUNS; ++r) {
      if (r < R) {   // a guard, not a break: the loop unrolls fully (sse[] stays in registers)
        float best = INFINITY;
        int bj = s_off[r];
        for (int j = s_off[r]; j < s_off[r + 1]; ++j) {
          float dot = 0.f;
#pragma unroll
          for (int d = 0; d < D; ++d) dot = fmaf(x[d], cen[j * D + d], dot);
          const float dist = cnorm[j] - 2.f * dot;
          if (dist < best) { best = dist; bj = j; }
        }
        if (assign) assign[(long long)r * n + row] = bj - s_off[r];
        sse[r] += (double)fmaxf(best + xn, 0.f);
        float* a = acc + bj * (D + 1);
#pragma unroll
        for (int d = 0; d < D; ++d) atomicAdd(&a[d], x[d]);
        atomicAdd(&a[D], 1.f);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < MAX_RUNS; ++r) {
    if (r < R) {
      const double v = av::wave_sum(sse[r]);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][r] = v;
    }
  }
  __syncthreads();
  float* out = partial + (long long)blockIdx.x * K * (D + 1);
  for (int i = threadIdx.x; i < K * (D + 1); i += KB) out[i] = acc[i];
  for (int r = threadIdx.x; r < R; r += KB) {
    double s = 0.0;
    for (int q = 0; q < KB / 64; ++q) s += red[q][r];
    sse_partial[(long long)blockIdx.x * R + r] = s;
  }
}

template <int D, int KBLK>
__global__ __launch_bounds__(KB) void kmeans_mfma_kernel(const float* __restrict__ X, long long n,
                                                         const float* __restrict__ C2, const float* __restrict__ Cn,
                                                         const int* __restrict__ roff, int R, int K,
                                                         int* __restrict__ assign, float* __restrict__ partial,
                                                         double* __restrict__ sse_partial) {
  constexpr int DP = D < 16 ? 16 : D;  // staged row width (zero padded to one 16-wide block)
  constexpr int DB = DP / 16;
  extern __shared__ float lds[];
  float* xs_all = lds;                                                 // [4 waves][64][DP]
  int* asg_all = reinterpret_cast<int*>(xs_all + 4 * 64 * DP);         // [4 waves][64][R]
  unsigned* cnt = reinterpret_cast<unsigned*>(asg_all + 4 * 64 * R);   // [K]
  float* red = reinterpret_cast<float*>(cnt + K);                      // [K][D]
  __shared__ double sred[4][MAX_RUNS];
  for (int i = threadIdx.x; i < K; i += KB) cnt[i] = 0u;
  for (int i = threadIdx.x; i < K * D; i += KB) red[i] = 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* xs = xs_all + w * 64 * DP;
  int* asg = asg_all + w * 64 * R;
  // A operand: lane l supplies A[i = l & 15][k = l >> 4] of centroid block cb
  // (centroid ids as floats are exact; -1 never matches an assignment: centroid lanes past K)
  float a_centf[KBLK];
  int a_runc[KBLK];
#pragma unroll
  for (int cb = 0; cb < KBLK; ++cb) {
    const int c = cb * 16 + (lane & 15);
    int rr = -1;
    for (int r = 0; r < R; ++r)
      if (c >= roff[r] && c < roff[r + 1]) rr = r;
    a_centf[cb] = rr >= 0 ? (float)c : -2.f;
    a_runc[cb] = rr >= 0 ? rr : 0;
  }
  f32x4 acc[2][KBLK][DB];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
      for (int db = 0; db < DB; ++db) acc[h][cb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  double sse[MAX_RUNS];
#pragma unroll
  for (int r = 0; r < MAX_RUNS; ++r) sse[r] = 0.0;
  const long long ntiles = (n + 63) / 64;
  const long long gw = (long long)blockIdx.x * 4 + w, nw = (long long)gridDim.x * 4;
  float xnext[D];
  if (gw < ntiles) load_row<D>(X, gw * 64 + lane, gw * 64 + lane < n, xnext);
  for (long long t = gw; t < ntiles; t += nw) {
    const long long row = t * 64 + lane;
    const bool ok = row < n;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = xnext[d];
    {  // prefetch the next tile's row: its HBM latency hides behind this tile's scoring
      const long long nrow = (t + nw) * 64 + lane;
      if (t + nw < ntiles) load_row<D>(X, nrow, nrow < n, xnext);
    }
    float xn = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) xn = fmaf(x[d], x[d], xn);
#pragma unroll
    for (int r = 0; r < MAX_RUNS; ++r) {
      if (r < R) {   // a guard, not a break: the loop unrolls fully (sse[] stays in registers)
        const int j0 = __builtin_amdgcn_readfirstlane(roff[r]), j1 = __builtin_amdgcn_readfirstlane(roff[r + 1]);
        float best;
        int bj;
        score_run<D>(x, C2, Cn, j0, j1, best, bj);
        if (ok) {
          if (assign) assign[(long long)r * n + row] = bj - j0;
          sse[r] += (double)fmaxf(best + xn, 0.f);
          atomicAdd(&cnt[bj], 1u);
        }
        asg[lane * R + r] = ok ? bj : -1;
      }
    }
    float xp[DP];  // zero-padded copy (compile-time indices: stays in registers)
#pragma unroll
    for (int d = 0; d < DP; ++d) xp[d] = d < D ? x[d < D ? d : 0] : 0.f;
#pragma unroll
    for (int d = 0; d < DP; d += 4)
      *reinterpret_cast<float4*>(xs + lane * DP + d) = make_float4(xp[d], xp[d + 1], xp[d + 2], xp[d + 3]);
    // wave-private strip: LDS executes one wave's instructions in order, so the reads below see
    // these writes without a waitcnt (a full s_waitcnt(0) here would also drain the prefetch)
    __builtin_amdgcn_wave_barrier();
    // 16 MFMA k-steps of 4 rows; operands of 4 steps are read from LDS back to back (one wait),
    // and even / odd steps feed two accumulator sets so consecutive MFMAs are independent
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += 4) {
      float a[4][KBLK], b[4][DB];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 4 * (s0 + q) + (lane >> 4);
#pragma unroll
        for (int cb = 0; cb < KBLK; ++cb) a[q][cb] = (float)asg[rr * R + a_runc[cb]];
#pragma unroll
        for (int db = 0; db < DB; ++db) b[q][db] = xs[rr * DP + db * 16 + (lane & 15)];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cb = 0; cb < KBLK; ++cb) {
          const float av = a[q][cb] == a_centf[cb] ? 1.f : 0.f;
#pragma unroll
          for (int db = 0; db < DB; ++db)
            acc[q & 1][cb][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[q][db], acc[q & 1][cb][db], 0, 0, 0);
        }
    }
    __builtin_amdgcn_wave_barrier();
  }
  // combine the 4 waves' accumulators in LDS: lane holds D[i = 4 (l >> 4) + q][j = l & 15]
#pragma unroll
  for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cb * 16 + 4 * (lane >> 4) + q, d = db * 16 + (lane & 15);
        if (c < K && d < D) atomicAdd(&red[c * D + d], acc[0][cb][db][q] + acc[1][cb][db][q]);
      }
#pragma unroll
  for (int r = 0; r < MAX_RUNS; ++r) {
    if (r < R) {   // a guard, not a break: the loop unrolls fully (sse[] stays in registers)
      const double v = av::wave_sum(sse[r]);
      if (lane == 0) sred[w][r] = v;
    }
  }
  __syncthreads();
  float* out = partial + (long long)blockIdx.x * K * (D + 1);
  for (int i = threadIdx.x; i < K * (D + 1); i += KB) {
    const int c = i / (D + 1), d = i - c * (D + 1);
    out[i] = d < D ? red[c * D + d] : (float)cnt[c];
  }
  for (int r = threadIdx.x; r < R; r += KB) {
    double s = 0.0;
    for (int q = 0; q < 4; ++q) s += sred[q][r];
    sse_partial[(long long)blockIdx.x * R + r] = s;
  }
}

// kmeans_score_kernel: the same pass with the SCORING on the matrix cores too (one run, R = 1: the
// job's k-means; batched runs keep kmeans_mfma_kernel).  A wave owns a 64-row tile; lane l = 16 g + c
// loads rows r0 + 16 s + c, dims 16 b + 4 g .. +3 as one float4 per (16-row sub-tile s, 16-dim
// block b) — each load instruction reads 16 contiguous rows (1 KiB), fully coalesced.  Per tile:
//   * scoring: those registers ARE the B operand of v_mfma_f32_16x16x4_f32 for x . c over a
//     permuted reduction index (step m of block b sums dims 16 b + 4 k + m; the A operand holds the
//     centroids in the same order).  The accumulators START at -||c||^2 / 2, so each MFMA chain
//     yields s'(x, c) = x . c - ||c||^2 / 2 = -(||c||^2 - 2 x.c) / 2 with no epilogue arithmetic; 4
//     sub-tiles x centroid blocks are independent chains issued back to back;
//   * a 4 x 4 register transpose across the row groups — 8 v_permlane32_swap + 8 v_permlane16_swap
//     per 16 centroids, no copies — leaves lane l holding ALL the centroid scores of ITS row
//     r0 + l in a fixed register order (register 4 j + q = centroid 16 cb + 4 j + q);
//   * the argmax of s' is then a strict-> scan in ascending centroid order inside the lane (ties go
//     to the lower centroid, as a sequential scan); the row's squared distance to it is -2 s' + ||x||^2
//     (SSE adds the tile's ||x||^2 once);
//   * partial sums: the one-hot MFMA of kmeans_mfma_kernel with reduction step s over rows 16 g + s,
//     so the one-hot operand of 4 steps is ONE 16-byte LDS read of the assignments, and the
//     row-major staging tile is padded (row stride DP + 4, 16 floats per 16-row group) against
//     LDS bank conflicts.
// Three register tiles rotate (no copies) so the next two tiles' loads are in flight during this
// one's work.
// NBUF register tiles in rotation: 2 (the default) keeps one tile of loads ahead at 4 waves / SIMD
// (120 VGPRs), 3 keeps two ahead at 3 waves / SIMD (162 VGPRs; AVMI_KMEANS_NBUF=3).  Measured at
// 16.7 M x 16, k = 16: 253.5 vs 263.6 us per pass (profiles/r5_kmeans_nbuf_ab.txt); 5 waves spill.
// SB (split-bf16 variant, D in {16, 32}): the fp32 MFMAs become v_mfma_f32_16x16x32_bf16 over
// split operands.  CDNA4's fp32 MFMA runs at 1/16 of the bf16 rate, so the 32 fp32 MFMAs of a tile
// (1,024 cycles) were the matrix half of the pass's issue-bound budget.
//   scoring: the lane's float4 (row 16 sb + col, dims 16 b + 4 g ..+3) is split into 3 bf16 terms
//     x0 + x1 + x2 and a fragment's 8 k-slots hold two terms of those 4 dims, the centroid
//     fragment the matching terms: [x0|x1].[c0|c0] + [x0|x1].[c1|c1] + [x0|x2].[c2|c0] = the 6
//     cross products of fp32-level accuracy (SB = 3) in 3 MFMAs per 16 rows x 16 dims; SB = 2
//     keeps [x0|x1].[c0|c0] + [x0|x1].[c1|0] (2 MFMAs, ~2^-17 per product);
//   partial sums: the one-hot is exact in bf16 and the staged rows go in as all three terms, whose
//     sum IS the fp32 value (3 x 8 significand bits, RNE remainders): [x0|x1] over 4 rows per row
//     group (16 rows per MFMA, 4 per tile) plus [x2|x2] over 8 rows per row group (32 rows per MFMA,
//     2 per tile) instead of 16 fp32 MFMAs.  Every product is exact and the accumulation is fp32,
//     so in every mode (SB = 0, 2, 3) the workgroup partial sums are fp32 sums of the fp32 data;
//     only the SCORES differ by mode (fp32; ~2^-17 per product for SB = 2; fp32-level for SB = 3).
//     Two terms would not do: they keep 16-17 significand bits, and a feature that is nearly
//     constant within a cluster (cents, epoch seconds) loses the SAME low bits in every row, an
//     error that does not average out and that kmeans_update_kernel divides into the centroids.
// Per tile 12 + 6 bf16 MFMAs of 16 cycles (288) instead of 32 fp32 ones of 32 (1,024).
template <int D, int KBLK, int NBUF, int SB = 0>
__global__ __launch_bounds__(KB, (KBLK == 1 && D <= 16) ? (NBUF == 2 ? 4 : 3) : 2) void kmeans_score_kernel(const float* __restrict__ X, long long n,
                                                          const float* __restrict__ C2, const float* __restrict__ Cn,
                                                          const int* __restrict__ roff, int R, int K,
                                                          int* __restrict__ assign, float* __restrict__ partial,
                                                          double* __restrict__ sse_partial) {
  static_assert(D % 4 == 0, "kmeans_score_kernel: rows of whole float4s (D in {4, 8, 16, 32})");
  constexpr int DP = D < 16 ? 16 : D;  // staged row width of the partial-sum tile
  constexpr int DB = DP / 16;          // 16-dim blocks
  constexpr int RS = DP + 4;           // padded row stride of the staging tile
  constexpr int XS = 64 * RS + 64;     // floats per wave
  extern __shared__ float lds[];
  float* xs_all = lds;                                                 // [4 waves][XS]
  int* asg_all = reinterpret_cast<int*>(xs_all + 4 * XS);              // [4 waves][64]
  unsigned* cnt = reinterpret_cast<unsigned*>(asg_all + 4 * 64);       // [K]
  float* red = reinterpret_cast<float*>(cnt + K);                      // [K][D]
  __shared__ double sred[4];
  for (int i = threadIdx.x; i < K; i += KB) cnt[i] = 0u;
  for (int i = threadIdx.x; i < K * D; i += KB) red[i] = 0.f;
  __syncthreads();
  // the wave index read into a scalar register: the tile loop below is then uniform per wave (a
  // VGPR loop counter made it an exec-masked loop, with a full vmcnt(0) wait at its head)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), grp = lane >> 4,
            col = lane & 15;
  float* xs = xs_all + w * XS;
  int* asg = asg_all + w * 64;
  // scoring A operand: centroid 16 cb + col, dim 16 b + 4 grp + m; accumulator start -||c||^2 / 2 of
  // the lane's 4 result rows (centroids 16 cb + 4 grp + q; -inf past K: never the argmax)
  float ac[KBLK][DB][4];
  f32x4 cinit[KBLK];
#pragma unroll
  for (int cb = 0; cb < KBLK; ++cb) {
    const int c = cb * 16 + col;
#pragma unroll
    for (int b = 0; b < DB; ++b)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int d = b * 16 + 4 * grp + m;
        ac[cb][b][m] = (c < K && d < D) ? pair_at(C2, D, c, d) : 0.f;
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cq = cb * 16 + 4 * grp + q;
      cinit[cb][q] = cq < K ? -0.5f * Cn[cq] : -INFINITY;
    }
  }
  static_assert(SB == 0 || ((D == 16 || D == 32) && (SB == 2 || SB == 3)), "split-bf16 scoring: D 16 / 32, SB 2 / 3");
  // split-bf16 centroid fragments: [term pair][cb][b], slots j < 4 / j >= 4 = the two terms of
  // dims 16 b + 4 grp + (j & 3) of centroid 16 cb + col
  bf16x8 cfr[SB == 0 ? 1 : SB][KBLK][DB];
  if constexpr (SB != 0) {
#pragma unroll
    for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        unsigned ct[3][2];
        km_split4<3>(ac[cb][b][0], ac[cb][b][1], ac[cb][b][2], ac[cb][b][3], ct);
        cfr[0][cb][b] = km_frag(ct[0][0], ct[0][1], ct[0][0], ct[0][1]);                  // [c0|c0]
        if constexpr (SB == 3) {
          cfr[1][cb][b] = km_frag(ct[1][0], ct[1][1], ct[1][0], ct[1][1]);                // [c1|c1]
          cfr[2][cb][b] = km_frag(ct[2][0], ct[2][1], ct[0][0], ct[0][1]);                // [c2|c0]
        } else {
          cfr[1][cb][b] = km_frag(ct[1][0], ct[1][1], 0u, 0u);                            // [c1|0]
        }
      }
  }
  // partial-sum A operand: lane supplies one-hot[centroid 16 cb + col][row]
  int a_cent[KBLK];
#pragma unroll
  for (int cb = 0; cb < KBLK; ++cb) a_cent[cb] = cb * 16 + col < K ? cb * 16 + col : -2;
  f32x4 acc[2][KBLK][DB];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
      for (int db = 0; db < DB; ++db) acc[h][cb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  double sse = 0.0, xsq = 0.0;
  const long long ntiles = (n + 63) / 64;
  const long long gw = (long long)blockIdx.x * 4 + w, nw = (long long)gridDim.x * 4;
  // branch-free raw loads: rows past n read the last row, dims past D read dims 0..3 — never
  // masked here (a select right after the load made the waitcnt pass wait for it at once, and loads
  // under per-lane branches made it wait for ALL outstanding loads before each tile's MFMAs).  The
  // extra values are harmless: padded dims meet zero centroid coordinates in the scoring MFMAs and
  // are never summed (red[] keeps d < D), padded rows have no assignment (-1: a zero one-hot
  // row) — only ||x||^2 masks them, in body().
  auto load_tile = [&](long long t, f32x4 (&v)[4][DB]) {
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const long long row = t * 64 + sb * 16 + col;
      const long long rr = row < n ? row : n - 1;
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        const int d = b * 16 + 4 * grp;
        const int dd = d < D ? d : 0;
        const float4 u = *reinterpret_cast<const float4*>(X + rr * D + dd);
        v[sb][b] = f32x4{u.x, u.y, u.z, u.w};
      }
    }
  };
  auto body = [&](long long t, f32x4 (&xv)[4][DB]) {
    float xs2 = 0.f;  // ||x||^2 of the tile's valid rows and dims
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const bool rin = t * 64 + sb * 16 + col < n;
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        float q = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) q = fmaf(xv[sb][b][m], xv[sb][b][m], q);
        xs2 += (rin && b * 16 + 4 * grp < D) ? q : 0.f;
      }
    }
    xsq += (double)xs2;
    // s'(row 16 sb + col, centroid 16 cb + 4 grp + q) in dot[sb][cb][q]
    f32x4 dot[4][KBLK];
    if constexpr (SB == 0) {
#pragma unroll
      for (int b = 0; b < DB; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
            for (int sb = 0; sb < 4; ++sb)
              dot[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[cb][b][m], xv[sb][b][m],
                                                                 (b == 0 && m == 0) ? cinit[cb] : dot[sb][cb], 0, 0, 0);
    } else {
#pragma unroll
      for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) dot[sb][cb] = cinit[cb];
      // one 16-row sub-tile at a time (its fragments die before the next one's split: the x6
      // fragments of all four sub-tiles at once spilled at 4 waves / SIMD); smallest products first
#pragma unroll
      for (int sb = 0; sb < 4; ++sb)
#pragma unroll
        for (int b = 0; b < DB; ++b) {
          unsigned xt[3][2];
          km_split4<SB>(xv[sb][b][0], xv[sb][b][1], xv[sb][b][2], xv[sb][b][3],
                        reinterpret_cast<unsigned (&)[SB][2]>(xt));
          const bf16x8 f01 = km_frag(xt[0][0], xt[0][1], xt[1][0], xt[1][1]);                  // [x0|x1]
#pragma unroll
          for (int cb = 0; cb < KBLK; ++cb) {
            if constexpr (SB == 3) {
              const bf16x8 f02 = km_frag(xt[0][0], xt[0][1], xt[2][0], xt[2][1]);              // [x0|x2]
              dot[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cfr[2][cb][b], f02, dot[sb][cb], 0, 0, 0);
            }
            dot[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cfr[1][cb][b], f01, dot[sb][cb], 0, 0, 0);
            dot[sb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cfr[0][cb][b], f01, dot[sb][cb], 0, 0, 0);
          }
        }
    }
    // transpose: afterwards dot[j][cb][q] = s'(row 16 grp + col, centroid 16 cb + 4 j + q)
#pragma unroll
    for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int lo = 0; lo < 2; ++lo) {  // row groups g <-> g ^ 2: pairs (0, 2), (1, 3)
          const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(dot[lo][cb][q]),
                                                          __float_as_uint(dot[lo + 2][cb][q]), false, false);
          dot[lo][cb][q] = __uint_as_float(r[0]);
          dot[lo + 2][cb][q] = __uint_as_float(r[1]);
        }
#pragma unroll
        for (int lo = 0; lo < 4; lo += 2) {  // row groups g <-> g ^ 1: pairs (0, 1), (2, 3)
          const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(dot[lo][cb][q]),
                                                          __float_as_uint(dot[lo + 1][cb][q]), false, false);
          dot[lo][cb][q] = __uint_as_float(r[0]);
          dot[lo + 1][cb][q] = __uint_as_float(r[1]);
        }
      }
    float best = dot[0][0][0];
    int bi = 0;
#pragma unroll
    for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (cb == 0 && j == 0 && q == 0) continue;
          const float v = dot[j][cb][q];
          const bool gt = v > best;
          best = gt ? v : best;
          bi = gt ? cb * 16 + 4 * j + q : bi;
        }
    const long long row = t * 64 + lane;
    const bool ok = row < n;
    if (ok) {
      if (assign) assign[row] = bi;
      sse += (double)(-2.f * best);
      atomicAdd(&cnt[bi], 1u);
    }
    asg[lane] = ok ? bi : -1;
    // stage the tile row-major (padded) for the partial-sum MFMAs: lane writes its 4-dim pieces
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        const int d = b * 16 + 4 * grp;
        *reinterpret_cast<float4*>(xs + (sb * 16 + col) * RS + 16 * sb + d) =
            make_float4(xv[sb][b][0], xv[sb][b][1], xv[sb][b][2], xv[sb][b][3]);
      }
    // wave-private strip: LDS executes one wave's instructions in order
    __builtin_amdgcn_wave_barrier();
    const float* xr = xs + 16 * grp * RS + 16 * grp + col;  // row 16 grp, dim col
    // split-bf16: the third terms (and one-hot halves) of the even steps wait for the odd ones
    unsigned x2k[DB][2], ohk[KBLK][2];
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += 4) {
      const int4 a4 = *reinterpret_cast<const int4*>(asg + 16 * grp + s0);
      const int a[4] = {a4.x, a4.y, a4.z, a4.w};
      float bb[4][DB];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int db = 0; db < DB; ++db) bb[q][db] = xr[(s0 + q) * RS + db * 16];
      if constexpr (SB == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int cb = 0; cb < KBLK; ++cb) {
            const float av = a[q] == a_cent[cb] ? 1.f : 0.f;
#pragma unroll
            for (int db = 0; db < DB; ++db)
              acc[q & 1][cb][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bb[q][db], acc[q & 1][cb][db], 0, 0, 0);
          }
      } else {
        // [x0|x1] MFMA, k-slot 8 grp + j: row 16 grp + s0 + (j & 3), term j >> 2 (one-hot repeated:
        // exact in bf16).  x0 + x1 + x2 IS the fp32 value (three RNE bf16 terms hold 24 significand
        // bits), so the third terms go in too: [x2 of the previous step's 4 rows|x2 of this step's]
        // every second step, k-slot j: row 16 grp + s0 - 4 + j.
        bf16x8 xb[DB], x2b[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          unsigned xt[3][2];
          km_split4<3>(bb[0][db], bb[1][db], bb[2][db], bb[3][db], xt);
          xb[db] = km_frag(xt[0][0], xt[0][1], xt[1][0], xt[1][1]);
          if ((s0 >> 2) & 1) {
            x2b[db] = km_frag(x2k[db][0], x2k[db][1], xt[2][0], xt[2][1]);
          } else {
            x2k[db][0] = xt[2][0];
            x2k[db][1] = xt[2][1];
          }
        }
#pragma unroll
        for (int cb = 0; cb < KBLK; ++cb) {
          const unsigned one = 0x3F80u;  // bf16 1.0
          const unsigned h0 = (a[0] == a_cent[cb] ? one : 0u) | ((a[1] == a_cent[cb] ? one : 0u) << 16);
          const unsigned h1 = (a[2] == a_cent[cb] ? one : 0u) | ((a[3] == a_cent[cb] ? one : 0u) << 16);
          const bf16x8 oh = km_frag(h0, h1, h0, h1);
#pragma unroll
          for (int db = 0; db < DB; ++db)
            acc[(s0 >> 2) & 1][cb][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oh, xb[db], acc[(s0 >> 2) & 1][cb][db], 0, 0, 0);
          if ((s0 >> 2) & 1) {
            const bf16x8 oh2 = km_frag(ohk[cb][0], ohk[cb][1], h0, h1);
#pragma unroll
            for (int db = 0; db < DB; ++db)
              acc[(s0 >> 3) & 1][cb][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oh2, x2b[db], acc[(s0 >> 3) & 1][cb][db], 0, 0, 0);
          } else {
            ohk[cb][0] = h0;
            ohk[cb][1] = h1;
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  // register tiles in rotation: with three, the loads of the next TWO tiles are in flight during
  // this one's work (one tile ahead left HBM at ~3.9 TB/s at 3 waves / SIMD)
  f32x4 xa[4][DB], xb[4][DB], xc[4][DB];
  long long t = gw;
  if constexpr (NBUF == 3) {
    if (t < ntiles) load_tile(t, xa);
    if (t + nw < ntiles) load_tile(t + nw, xb);
    while (t < ntiles) {
      if (t + 2 * nw < ntiles) load_tile(t + 2 * nw, xc);
      body(t, xa);
      t += nw;
      if (t >= ntiles) break;
      if (t + 2 * nw < ntiles) load_tile(t + 2 * nw, xa);
      body(t, xb);
      t += nw;
      if (t >= ntiles) break;
      if (t + 2 * nw < ntiles) load_tile(t + 2 * nw, xb);
      body(t, xc);
      t += nw;
    }
  } else {
    // the prefetch is unconditional (past the last tile it re-reads the last tile): a prefetch
    // under a branch made the waitcnt pass assume it might be missing and wait for part of it
    // before the current tile's MFMAs
    const long long last = ntiles - 1;
    if (t < ntiles) load_tile(t, xa);
    while (t < ntiles) {
      load_tile(t + nw < ntiles ? t + nw : last, xb);
      __builtin_amdgcn_sched_barrier(0);  // issue the prefetch before this tile's work
      body(t, xa);
      t += nw;
      if (t >= ntiles) break;
      load_tile(t + nw < ntiles ? t + nw : last, xa);
      __builtin_amdgcn_sched_barrier(0);
      body(t, xb);
      t += nw;
    }
  }
#pragma unroll
  for (int cb = 0; cb < KBLK; ++cb)
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cb * 16 + 4 * grp + q, d = db * 16 + col;
        if (c < K && d < D) atomicAdd(&red[c * D + d], acc[0][cb][db][q] + acc[1][cb][db][q]);
      }
  const double v = av::wave_sum(sse) + av::wave_sum(xsq);
  if (lane == 0) sred[w] = v;
  __syncthreads();
  float* out = partial + (long long)blockIdx.x * K * (D + 1);
  for (int i = threadIdx.x; i < K * (D + 1); i += KB) {
    const int c = i / (D + 1), d = i - c * (D + 1);
    out[i] = d < D ? red[c * D + d] : (float)cnt[c];
  }
  if (threadIdx.x == 0) sse_partial[blockIdx.x] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
}

// out[o] = sum_g partial[g][o] (o < KD1) and out[KD1 + r] = sum_g ssep[g][r]: 16 outputs x 64
// grid slices per workgroup (4 independent partial sums per lane keep 4 loads in flight), slices
// combined in a fixed order: deterministic.
constexpr int RD_O = 16, RD_S = 64;
__global__ __launch_bounds__(RD_O * RD_S) void kmeans_reduce_kernel(const float* __restrict__ partial,
                                                                    const double* __restrict__ ssep, int grid,
                                                                    int KD1, int R, double* __restrict__ out) {
  __shared__ double red[RD_S][RD_O];
  const int oi = threadIdx.x % RD_O, sl = threadIdx.x / RD_O;
  const int o = blockIdx.x * RD_O + oi;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (o < KD1) {
    int g = sl;
    for (; g + 3 * RD_S < grid; g += 4 * RD_S) {
      s0 += (double)partial[(long long)g * KD1 + o];
      s1 += (double)partial[(long long)(g + RD_S) * KD1 + o];
      s2 += (double)partial[(long long)(g + 2 * RD_S) * KD1 + o];
      s3 += (double)partial[(long long)(g + 3 * RD_S) * KD1 + o];
    }
    for (; g < grid; g += RD_S) s0 += (double)partial[(long long)g * KD1 + o];
  } else if (o < KD1 + R) {
    for (int g = sl; g < grid; g += RD_S) s0 += ssep[(long long)g * R + (o - KD1)];
  }
  red[sl][oi] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && o < KD1 + R) {
    double t = 0.0;
    for (int q = 0; q < RD_S; ++q) t += red[q][oi];
    out[o] = t;
  }
}

__global__ __launch_bounds__(1024) void kmeans_update_kernel(const double* __restrict__ flat, int K, int D, int R,
                                                             const int* __restrict__ run_of,
                                                             const unsigned char* __restrict__ frozen,
                                                             float* __restrict__ C2, float* __restrict__ Cn,
                                                             float* __restrict__ moves) {
  extern __shared__ float mv2[];  // [K]
  __shared__ unsigned mx[MAX_RUNS];
  __shared__ float ss[MAX_RUNS];  // per run: sum over centroids of the squared shift (sklearn's tol)
  for (int c = threadIdx.x; c < K; c += 1024) mv2[c] = 0.f;
  if (threadIdx.x < MAX_RUNS) {
    mx[threadIdx.x] = 0u;
    ss[threadIdx.x] = 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * D; i += 1024) {
    const int c = i / D, d = i - c * D;
    const int r = run_of[c];
    if (r < 0 || frozen[r]) continue;
    const double cnt = flat[(long long)c * (D + 1) + D];
    float* p = C2 + (long long)(c >> 1) * 2 * D + 2 * d + (c & 1);
    const float old = *p;
    const float nw = cnt > 0.0 ? (float)(flat[(long long)c * (D + 1) + d] / cnt) : old;
    *p = nw;
    const float df = nw - old;
    atomicAdd(&mv2[c], df * df);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < K; c += 1024) {
    const int r = run_of[c];
    if (r < 0 || frozen[r]) continue;
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
      const float v = C2[(long long)(c >> 1) * 2 * D + 2 * d + (c & 1)];
      s = fmaf(v, v, s);
    }
    Cn[c] = s;
    atomicMax(&mx[r], __float_as_uint(sqrtf(mv2[c])));  // non-negative floats order like their bits
    atomicAdd(&ss[r], mv2[c]);
  }
  __syncthreads();
  if (threadIdx.x < R) {
    moves[threadIdx.x] = __uint_as_float(mx[threadIdx.x]);  // max centroid shift (Java criterion)
    moves[R + threadIdx.x] = ss[threadIdx.x];               // total squared shift
  }
}

// Kernel variant for (D, K, R): the MFMA kernel when its accumulators fit (<= 16 blocks of 16
// centroids x 16 dims), else the LDS kernel.  Returns nullptr when neither fits.
struct KmVariant {
  const void* fn;
  size_t lds;
  bool mfma;
};

KmVariant km_variant(int D, int K, int R) {
  const int DP = D < 16 ? 16 : D;
  int KBt = 1;
  while (KBt * 16 < K) KBt *= 2;
  static const bool nbuf2 = [] {
    const char* e = std::getenv("AVMI_KMEANS_NBUF");
    return !(e && e[0] == '3');
  }();
  static const bool valu_score = [] {
    const char* e = std::getenv("AVMI_KMEANS_SCORE");
    return e && (e[0] == 'v' || e[0] == 'V');  // "valu": the packed-FMA scoring kernel (A/B)
  }();
  // AVMI_KMEANS_MFMA = f32 | bf16x3 (default) | bf16x6: the arithmetic of kmeans_score_kernel.
  // Scoring accuracy by mode: f32 = fp32 products and sums; x3 ~2^-17 relative per product (passes
  // the fp64 oracle with its fp32 tie tolerance); x6 fp32-level.  The partial sums are fp32 sums of
  // the fp32 data in ALL modes (three bf16 terms in the one-hot MFMA; the cross-workgroup reduce is
  // fp64), and integer data that fits one bf16 term is reproduced bit for bit by every mode
  // (tests/test_kmeans_kernels.py).
  // At 16.7 M x 16, k = 16, kernel time: f32 253.5 us, x3 199.6 us, x6 217.1 us per pass with
  // two-term sums (profiles/r6_kmeans_split_bf16.jsonl).  The third term, as kmeans_assign call
  // time (median of 1000 warm passes, device events): x3 193.4 -> 201.2 us (+4 %), x6 211.4 ->
  // 229.2 us (+8 %) (profiles/kmeans_exact_sums_pass_times.jsonl); f32 is unchanged.
  static const int sbm = [] {
    const char* e = std::getenv("AVMI_KMEANS_MFMA");
    if (e == nullptr) return 2;
    const std::string v(e);
    return v == "f32" ? 0 : (v == "bf16x6" ? 3 : 2);
  }();
  // one run (R = 1: the job's k-means; batched runs keep the packed-FMA kernel, whose registers
  // grow less with R) and up to 2 blocks of 16 centroids x 16 dims of accumulators
  if (!valu_score && R == 1 && D >= 4 && KBt * (DP / 16) <= 2) {
    const size_t lds = sizeof(float) * (4 * (64 * (size_t)(DP + 4) + 64) + 4 * 64 + K + (size_t)K * D);
#define AVK_KMSB(DD, KK) \
  if (D == DD && KBt == KK && sbm != 0)                                                       \
    return {sbm == 3 ? (const void*)kmeans_score_kernel<DD, KK, 2, 3> : (const void*)kmeans_score_kernel<DD, KK, 2, 2>, lds, true};
    AVK_KMSB(16, 1) AVK_KMSB(16, 2) AVK_KMSB(32, 1)
#undef AVK_KMSB
#define AVK_KMS(DD, KK) \
  if (D == DD && KBt == KK)                                                                   \
    return {nbuf2 ? (const void*)kmeans_score_kernel<DD, KK, 2> : (const void*)kmeans_score_kernel<DD, KK, 3>, lds, true};
    AVK_KMS(4, 1) AVK_KMS(4, 2)
    AVK_KMS(8, 1) AVK_KMS(8, 2)
    AVK_KMS(16, 1) AVK_KMS(16, 2)
    AVK_KMS(32, 1)
#undef AVK_KMS
  }
  if (KBt * (DP / 16) <= 16) {
    const size_t lds = sizeof(float) * (4 * 64 * (size_t)DP + 4 * 64 * (size_t)R + K + (size_t)K * D);
#define AVK_KMM(DD, KK) \
  if (D == DD && KBt == KK) return {(const void*)kmeans_mfma_kernel<DD, KK>, lds, true};
    AVK_KMM(2, 1) AVK_KMM(2, 2) AVK_KMM(2, 4) AVK_KMM(2, 8) AVK_KMM(2, 16)
    AVK_KMM(4, 1) AVK_KMM(4, 2) AVK_KMM(4, 4) AVK_KMM(4, 8) AVK_KMM(4, 16)
    AVK_KMM(8, 1) AVK_KMM(8, 2) AVK_KMM(8, 4) AVK_KMM(8, 8) AVK_KMM(8, 16)
    AVK_KMM(16, 1) AVK_KMM(16, 2) AVK_KMM(16, 4) AVK_KMM(16, 8) AVK_KMM(16, 16)
    AVK_KMM(32, 1) AVK_KMM(32, 2) AVK_KMM(32, 4) AVK_KMM(32, 8)
    AVK_KMM(64, 1) AVK_KMM(64, 2) AVK_KMM(64, 4)
#undef AVK_KMM
    return {nullptr, 0, true};
  }
  const size_t lds = sizeof(float) * ((size_t)K * D + K + (size_t)K * (D + 1));
  switch (D) {
    case 2: return {(const void*)kmeans_step_kernel<2>, lds, false};
    case 4: return {(const void*)kmeans_step_kernel<4>, lds, false};
    case 8: return {(const void*)kmeans_step_kernel<8>, lds, false};
    case 16: return {(const void*)kmeans_step_kernel<16>, lds, false};
    case 32: return {(const void*)kmeans_step_kernel<32>, lds, false};
    case 64: return {(const void*)kmeans_step_kernel<64>, lds, false};
    default: return {nullptr, 0, false};
  }
}

}  // namespace

namespace avk {

int kmeans_grid(long long n, int D, int K, int R) {
  // ~16K rows per workgroup, between 256 and 4096 workgroups, but never more than are resident at
  // once (a second partial round of workgroups runs at lower occupancy)
  long long g = std::max(256LL, std::min((n + 16383) / 16384, 4096LL));
  const KmVariant v = km_variant(D, K, R);
  if (v.fn && v.lds <= 160 * 1024) {
    if (v.lds > 64 * 1024)
      AV_HIP_CHECK(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds));
    g = std::min<long long>(g, av::resident_blocks(v.fn, KB, v.lds));
  }
  return (int)g;
}

void kmeans_assign(const float* X, long long n, int D, const float* C2, const float* Cn, const int* roff, int R, int K,
                   int* assign, float* partial, double* sse_partial, int grid, hipStream_t stream) {
  if (R < 1 || R > MAX_RUNS) throw std::runtime_error("kmeans_assign: 1 <= runs <= 16");
  if (K & 1) throw std::runtime_error("kmeans_assign: padded centroid count must be even");
  const KmVariant v = km_variant(D, K, R);
  if (!v.fn) throw std::runtime_error("kmeans_assign: D must be 2, 4, 8, 16, 32 or 64");
  if (v.lds > (v.mfma ? 160 : 64) * 1024) throw std::runtime_error("kmeans_assign: LDS budget exceeded");
  if (v.lds > 64 * 1024)
    AV_HIP_CHECK(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds));
  void* args[] = {(void*)&X, (void*)&n, (void*)&C2, (void*)&Cn, (void*)&roff, (void*)&R, (void*)&K,
                  (void*)&assign, (void*)&partial, (void*)&sse_partial};
  void* args_lds[] = {(void*)&X, (void*)&n, (void*)&C2, (void*)&Cn, (void*)&roff, (void*)&R,
                      (void*)&assign, (void*)&partial, (void*)&sse_partial};
  AV_HIP_CHECK(hipLaunchKernel(v.fn, dim3(grid), dim3(KB), v.mfma ? args : args_lds, v.lds, stream));
}

void kmeans_reduce(const float* partial, const double* sse_partial, int grid, int K, int D, int R, double* out,
                   hipStream_t stream) {
  const int KD1 = K * (D + 1);
  const int blocks = (KD1 + R + RD_O - 1) / RD_O;
  kmeans_reduce_kernel<<<blocks, RD_O * RD_S, 0, stream>>>(partial, sse_partial, grid, KD1, R, out);
  AV_HIP_CHECK(hipGetLastError());
}

void kmeans_update(const double* flat, int K, int D, int R, const int* run_of, const unsigned char* frozen, float* C2,
                   float* Cn, float* moves, hipStream_t stream) {
  if (R < 1 || R > MAX_RUNS) throw std::runtime_error("kmeans_update: 1 <= runs <= 16");
  const size_t lds = sizeof(float) * (size_t)K;
  if (lds > 64 * 1024) throw std::runtime_error("kmeans_update: too many centroids");
  kmeans_update_kernel<<<1, 1024, lds, stream>>>(flat, K, D, R, run_of, frozen, C2, Cn, moves);
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace avk
