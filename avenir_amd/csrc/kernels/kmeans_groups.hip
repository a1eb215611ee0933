// K16g: many independent small-to-medium k-means fits in ONE launch (CDNA4, gfx950).
//
// K16 (cluster.hip) streams one big table through a grid and leaves the Lloyd loop on the host:
// three launches and one host read per iteration.  The kMeansPlusPlusCluster job has the opposite
// shape (S/cluster/KMeansPlusPlusCluster.scala: one model per key group, every k, several
// restarts): thousands of cheap fits whose whole cost is launches and host round trips.  Here ONE
// workgroup owns ONE run (group, k, restart) from its initial centroids to convergence: no host
// involvement, no grid-wide sync, no dependence between workgroups.
//
// Run record (8 x int64, host-validated): row offset, rows n, k, centroid offset, group, run id,
// convergence threshold (the bits of a double), accumulator replicas.  Per run the workgroup
//   * takes the group's max |x| (a workgroup max over the |x| bit patterns: NaN and inf order above
//     every finite value, so one compare finds non-finite data -> status[group] = 1, run skipped);
//   * loads its centroids into LDS and loops: every lane keeps one row in registers (float4 loads,
//     the next row in flight during the scoring; after the first pass the rows come from L2),
//     scores it against the LDS centroids with broadcast reads, adds the row to its cluster's sums,
//     then the workgroup updates the centroids, tests convergence and goes round again;
//   * runs one more assignment pass for the final SSE and counts.
//
// Arithmetic (the contract of models/kmeans_groups.py::kmeans_groups_twin, bit for bit):
//   distance  acc = 0; for d in order: t = x_d - c_jd; acc = acc + t * t   (fp32, product and sum
//             rounded separately; zero-padded dims add exact zeros); argmin: lowest index on ties.
//   sums      exact and order-independent: with max |x| < 2^e as frexp gives it (e = 0 for an
//             all-zero group), scale = 2^(40 - e), q = (long long)rint((double)x * scale), added
//             with 64-bit integer LDS atomics; |q| <= 2^40 and n <= 2^22 rows: no overflow.  The
//             atomics go to lane-indexed replicas of the table (odd stride), summed afterwards:
//             with k = 2 a single table would serialise 64 lanes on two addresses.
//   update    new = (float)((double)S / ((double)cnt * scale)); an empty cluster keeps its centroid.
//   shift     sh_c = sum_d (new - old)^2 in fp32, in d order, uncontracted.
//   converged "shift": (double)max_c sh_c <= thr (thr = tol^2); "sklearn": (double)sum_c sh_c <= thr
//             (thr = tol_eff), summed in c order.  No sqrtf.
//   SSE       fp64 sum of (double)best in a FIXED order that depends on the row index and the
//             workgroup size T only: thread t adds rows t, t + T, t + 2 T, ... in that order; the 64
//             lanes of a wave are combined by the xor butterfly 32, 16, 8, 4, 2, 1 (both partners
//             of a step compute the same commutative sum, so all lanes agree); the waves' values
//             are added in wave order 0, 1, 2, ...  No float atomics, nothing timing dependent, and
//             T is a function of the run's own group size (kmeans_groups_threads), never of what
//             else is in the launch.
#include <stdexcept>

#include "avenir_common.h"
#include "avenir_kernels.h"

namespace {

constexpr int KG_REC = 8;  // int64 words per run record

template <int DP>
__device__ __forceinline__ void kg_load_row(const float* __restrict__ X, long long row, float (&x)[DP]) {
  if constexpr (DP == 2) {
    const float2 v = *reinterpret_cast<const float2*>(X + row * 2);
    x[0] = v.x; x[1] = v.y;
  } else {
#pragma unroll
    for (int d = 0; d < DP; d += 4) {
      const float4 v = *reinterpret_cast<const float4*>(X + row * DP + d);
      x[d] = v.x; x[d + 1] = v.y; x[d + 2] = v.z; x[d + 3] = v.w;
    }
  }
}

// squared distance of x to the LDS centroid c (wave-uniform address: broadcast reads)
template <int DP>
__device__ __forceinline__ float kg_dist(const float (&x)[DP], const float* c) {
#pragma clang fp contract(off)  // the twin rounds t * t and the add separately
  float acc = 0.f;
  if constexpr (DP == 2) {
    const float2 v = *reinterpret_cast<const float2*>(c);
    const float t0 = x[0] - v.x, t1 = x[1] - v.y;
    acc = acc + t0 * t0;
    acc = acc + t1 * t1;
  } else {
#pragma unroll
    for (int d = 0; d < DP; d += 4) {
      const float4 v = *reinterpret_cast<const float4*>(c + d);
      const float t0 = x[d] - v.x, t1 = x[d + 1] - v.y, t2 = x[d + 2] - v.z, t3 = x[d + 3] - v.w;
      acc = acc + t0 * t0;
      acc = acc + t1 * t1;
      acc = acc + t2 * t2;
      acc = acc + t3 * t3;
    }
  }
  return acc;
}

template <int DP, int T>
__global__ __launch_bounds__(T) void kmeans_groups_kernel(
    const float* __restrict__ X, const long long* __restrict__ tab, int D, int max_iter, int mode,
    float* __restrict__ C, int* __restrict__ counts, double* __restrict__ sse_out, int* __restrict__ iters,
    int* __restrict__ conv, double* __restrict__ hist, int* __restrict__ status) {
  constexpr int W = T / 64;
  // rows of wide tables are not prefetched: two 64-float rows per lane do not fit 16 waves per CU
  constexpr bool PREFETCH = DP <= 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char kg_lds[];
  __shared__ double s_red[W];
  __shared__ unsigned s_mx[W];
  const long long* rec = tab + (long long)blockIdx.x * KG_REC;
  const long long base = rec[0];
  const int n = (int)rec[1], k = (int)rec[2];
  const long long coff = rec[3];
  const int grp = (int)rec[4];
  const long long run = rec[5];
  const double thr = __longlong_as_double(rec[6]);
  const int rep = (int)rec[7];  // a power of two
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int KD = k * DP, sstride = KD | 1, cstride = k | 1;
  float* cen = reinterpret_cast<float*>(kg_lds);                                   // [k][DP]
  float* cnew = cen + KD;                                                          // [k][DP]
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(cnew + KD);     // [rep][sstride]
  int* cnt = reinterpret_cast<int*>(acc + (long long)rep * sstride);               // [rep][cstride]
  float* shv = reinterpret_cast<float*>(cnt + rep * cstride);                      // [k]
  const float* Xg = X + base * DP;

  // ---- the group's max |x|: scale of the fixed-point sums, and the non-finite check
  unsigned mb = 0u;
  for (int i = tid; i < n; i += T) {
    float x[DP];
    kg_load_row<DP>(Xg, i, x);
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const unsigned b = __float_as_uint(x[d]) & 0x7fffffffu;
      mb = b > mb ? b : mb;
    }
  }
  mb = av::wave_max(mb);
  if (lane == 0) s_mx[w] = mb;
  for (int i = tid; i < KD; i += T) cen[i] = C[coff * DP + i];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < W; ++q) mb = s_mx[q] > mb ? s_mx[q] : mb;
  if (mb >= 0x7f800000u) {  // inf or NaN somewhere in the group (uniform: every thread leaves)
    if (tid == 0) status[grp] = 1;
    return;
  }
  int e = 0;  // max < 2^e, as frexp
  if (mb != 0u) e = (mb >> 23) ? (int)(mb >> 23) - 126 : (32 - __clz((int)mb)) - 149;
  const double scale = __longlong_as_double((long long)(1023 + 40 - e) << 52);  // 2^(40 - e)
  unsigned long long* my_acc = acc + (long long)(tid & (rep - 1)) * sstride;
  int* my_cnt = cnt + (tid & (rep - 1)) * cstride;

  // one assignment pass over the group: counts (and sums) into the replicas, returns the SSE
  auto pass = [&](const float* cc, bool sums) -> double {
    for (int i = tid; i < rep * sstride; i += T) acc[i] = 0ull;
    for (int i = tid; i < rep * cstride; i += T) cnt[i] = 0;
    __syncthreads();
    double s = 0.0;
    float xn[PREFETCH ? DP : 1];
    if constexpr (PREFETCH) {
      if (tid < n) kg_load_row<DP>(Xg, tid, xn);
    }
    for (int i = tid; i < n; i += T) {
      float x[DP];
      if constexpr (PREFETCH) {
#pragma unroll
        for (int d = 0; d < DP; ++d) x[d] = xn[d];
        if (i + T < n) kg_load_row<DP>(Xg, i + T, xn);
      } else {
        kg_load_row<DP>(Xg, i, x);
      }
      float best = kg_dist<DP>(x, cc);
      int bj = 0;
      for (int j = 1; j < k; ++j) {
        const float dj = kg_dist<DP>(x, cc + j * DP);
        if (dj < best) { best = dj; bj = j; }
      }
      s += (double)best;
      atomicAdd(&my_cnt[bj], 1);
      if (sums) {
#pragma unroll
        for (int d = 0; d < DP; ++d)
          if (d < D)
            atomicAdd(&my_acc[bj * DP + d], (unsigned long long)__double2ll_rn((double)x[d] * scale));
      }
    }
    s = av::wave_sum(s);
    if (lane == 0) s_red[w] = s;
    __syncthreads();
    double tot = s_red[0];
#pragma unroll
    for (int q = 1; q < W; ++q) tot += s_red[q];
    return tot;
  };

  int it = 0, done = 0;
  while (it < max_iter && !done) {
    const double sse = pass(cen, true);
    if (tid == 0) hist[run * max_iter + it] = sse;
    for (int i = tid; i < KD; i += T) {
      const int c = i / DP;
      long long S = 0;
      int m = 0;
      for (int r = 0; r < rep; ++r) {
        S += (long long)acc[(long long)r * sstride + i];
        m += cnt[r * cstride + c];
      }
      cnew[i] = m > 0 ? (float)((double)S / ((double)m * scale)) : cen[i];
    }
    __syncthreads();
    if (tid < k) {
#pragma clang fp contract(off)
      float sh = 0.f;
      for (int d = 0; d < DP; ++d) {
        const float t = cnew[tid * DP + d] - cen[tid * DP + d];
        sh = sh + t * t;
      }
      shv[tid] = sh;
    }
    __syncthreads();
    float agg = shv[0];
    if (mode == 0) {
      for (int c = 1; c < k; ++c) agg = fmaxf(agg, shv[c]);
    } else {
      for (int c = 1; c < k; ++c) agg = agg + shv[c];
    }
    done = (double)agg <= thr;
    float* t = cen;
    cen = cnew;
    cnew = t;
    ++it;
  }
  const double sse = pass(cen, false);
  for (int c = tid; c < k; c += T) {
    int m = 0;
    for (int r = 0; r < rep; ++r) m += cnt[r * cstride + c];
    counts[coff + c] = m;
  }
  for (int i = tid; i < KD; i += T) C[coff * DP + i] = cen[i];
  if (tid == 0) {
    sse_out[run] = sse;
    iters[run] = it;
    conv[run] = done;
  }
}

template <int DP>
const void* kg_fn(int threads) {
  switch (threads) {
    case 64: return (const void*)kmeans_groups_kernel<DP, 64>;
    case 256: return (const void*)kmeans_groups_kernel<DP, 256>;
    case 1024: return (const void*)kmeans_groups_kernel<DP, 1024>;
    default: return nullptr;
  }
}

}  // namespace

namespace avk {

// Workgroup size of a run: a function of ITS group's rows only (the SSE order depends on it).
int kmeans_groups_threads(long long n) { return n <= 512 ? 64 : (n <= 8192 ? 256 : 1024); }

// Accumulator replicas of a run: the largest power of two <= 32 whose tables fit 32 KiB.
int kmeans_groups_rep(int k, int DP) {
  const size_t per = 8 * (size_t)((k * DP) | 1) + 4 * (size_t)(k | 1);
  int rep = 32;
  while (rep > 1 && rep * per > 32 * 1024) rep >>= 1;
  return rep;
}

size_t kmeans_groups_lds(int k, int DP, int rep) {
  return 8 * (size_t)k * DP + (size_t)rep * (8 * (size_t)((k * DP) | 1) + 4 * (size_t)(k | 1)) + 4 * (size_t)k;
}

void kmeans_groups(const float* X, const long long* tab, int nruns, int DP, int D, int threads, size_t lds,
                   int max_iter, int mode, float* C, int* counts, double* sse, int* iters, int* conv, double* hist,
                   int* status, hipStream_t stream) {
  if (nruns < 1) return;
  const void* fn = nullptr;
  switch (DP) {
    case 2: fn = kg_fn<2>(threads); break;
    case 4: fn = kg_fn<4>(threads); break;
    case 8: fn = kg_fn<8>(threads); break;
    case 16: fn = kg_fn<16>(threads); break;
    case 32: fn = kg_fn<32>(threads); break;
    case 64: fn = kg_fn<64>(threads); break;
    default: break;
  }
  if (!fn) throw std::runtime_error("kmeans_groups: D must be padded to 2/4/8/16/32/64 and threads 64/256/1024");
  if (D < 1 || D > DP) throw std::runtime_error("kmeans_groups: 1 <= D <= padded D");
  if (lds > 160 * 1024) throw std::runtime_error("kmeans_groups: LDS budget exceeded");
  if (lds > 64 * 1024) AV_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  void* args[] = {(void*)&X, (void*)&tab, (void*)&D, (void*)&max_iter, (void*)&mode, (void*)&C, (void*)&counts,
                  (void*)&sse, (void*)&iters, (void*)&conv, (void*)&hist, (void*)&status};
  AV_HIP_CHECK(hipLaunchKernel(fn, dim3(nruns), dim3(threads), args, lds, stream));
}

}  // namespace avk
