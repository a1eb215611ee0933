// Isolation forest on CDNA4 (gfx950): one launch grows every tree, one launch scores every row.
//
// The arithmetic is the definition in models/iforest.py (iforest_build_twin, iforest_path_twin),
// operation for operation; every draw is philox_draw(seed ^ key, tree_base + t, index), so a forest
// depends on no grid or launch split.  All a tree stores is a count, a minimum or a maximum: the
// order in which a workgroup visits rows is free.  fp contract is off: thr = lo + u * (hi - lo) rounds
// the product and the sum separately, and the path sum adds one tree after the other.
//
// iforest_build_kernel: one workgroup (4 waves) per tree.  The sampled row indices (Floyd's algorithm:
// the draws in parallel, the collisions resolved by wave 0), a node-ordered permutation of the sample
// slots (two copies, one read and one written per level) and the segment of every heap node live in
// LDS, 16 KiB in all.  The sample tile [psi][D | 1] sits in dynamic LDS when it fits 48 KiB
// (TILE = true); otherwise rows are read through the permutation from global memory (TILE = false),
// where the psi * D floats of one tree stay in cache.  Level by level, a wave takes a node: lanes
// are (row group, feature), min / max meet by xor shuffles, the Philox decision is wave-uniform, and
// the segment is partitioned by ballots, left rows from the front and right rows from the back.
//
// iforest_score_kernel: one row per lane.  The block's rows sit in an LDS tile with an odd stride
// (the feature index is a runtime value: a register array would go to scratch); trees come through
// LDS in chunks of IF_CHUNK_BYTES, ascending, 8 bytes per node (feature or -1, then threshold or
// leaf_c); four trees are walked at once for latency, and added in tree order.  A walk takes exactly
// L steps, so a node index stays below M whatever the table holds, and a feature outside [-1, D)
// is staged as a leaf (the binding refuses such a table before the launch).
#include <climits>
#include <stdexcept>
#include <string>

#include "avenir_common.h"
#include "avenir_kernels.h"

#pragma clang fp contract(off)

namespace {

using av::lane_id;
using av::wave_id;

constexpr int IFB_T = 256;                 // build: threads per workgroup
constexpr int IFB_PSI = 1024;              // build: rows per tree at most
constexpr int IFB_M = 2048;                // nodes per tree at most, + 1
constexpr int IFB_TILE_BYTES = 48 * 1024;  // build: dynamic LDS for the sample tile
constexpr int IF_CHUNK_BYTES = 24 * 1024;  // score: LDS for a chunk of trees
constexpr unsigned long long IF_SAMPLE_KEY = 0x9E6C63D0876A9A47ull;
constexpr unsigned long long IF_NODE_KEY = 0xB5AD4ECEDA1CE2A9ull;

template <bool TILE>
__device__ __forceinline__ float if_value(const float* __restrict__ X, const float* tile, const int* idx, int D,
                                          int stride, int slot, int f) {
  return TILE ? tile[slot * stride + f] : X[(long long)idx[slot] * D + f];
}

template <bool TILE>
__global__ __launch_bounds__(IFB_T) void iforest_build_kernel(const float* __restrict__ X, long long n, int D, int dp,
                                                              int psi, int L, unsigned long long key_s,
                                                              unsigned long long key_n, unsigned long long tree_base,
                                                              int* __restrict__ feat, float* __restrict__ thr,
                                                              int* __restrict__ size) {
  __shared__ int idx[IFB_PSI];
  __shared__ unsigned short perm[2][IFB_PSI];
  __shared__ unsigned short hstart[IFB_M], hcnt[IFB_M];
  extern __shared__ float tile[];
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  const int M = (2 << L) - 1, stride = D | 1;
  const unsigned long long g = tree_base + blockIdx.x;
  int* tf = feat + (long long)blockIdx.x * M;
  float* tt = thr + (long long)blockIdx.x * M;
  int* ts = size + (long long)blockIdx.x * M;
  const int j0 = (int)(n - psi);

  for (int s = tid; s < psi; s += IFB_T) {
    const av::u4 d = av::philox_draw(key_s, g, (unsigned long long)s);
    idx[s] = (int)__umulhi(d.x, (unsigned)(j0 + s) + 1u);
    perm[0][s] = (unsigned short)s;
  }
  for (int i = tid; i < M; i += IFB_T) hcnt[i] = 0;
  __syncthreads();
  if (wave == 0) {
    // Floyd: slot s keeps its draw unless an earlier slot holds it.  Every lane stores the same
    // value, so each lane's later loads follow its own store.
    for (int s = 1; s < psi; ++s) {
      const int r = idx[s];
      bool hit = false;
      for (int k = lane; k < s; k += 64) hit |= idx[k] == r;
      if (__ballot(hit)) idx[s] = j0 + s;
    }
    hstart[0] = 0;
    hcnt[0] = (unsigned short)psi;
  }
  __syncthreads();
  if (TILE) {
    for (int i = tid; i < psi * D; i += IFB_T) {
      const int s = i / D, c = i - s * D;
      tile[s * stride + c] = X[(long long)idx[s] * D + c];
    }
    __syncthreads();
  }

  const int groups = 64 / dp, f = lane & (dp - 1), grp = lane / dp;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int lev = 0; lev < L; ++lev) {
    const int base = (1 << lev) - 1, width = 1 << lev;
    const unsigned short* src = perm[lev & 1];
    unsigned short* dst = perm[(lev & 1) ^ 1];
    for (int i = base + wave; i < base + width; i += IFB_T / 64) {
      const int c = hcnt[i], s0 = hstart[i];
      int fsel = -1;
      float th = 0.0f;
      if (c > 1) {
        float mn = __builtin_inff(), mx = -__builtin_inff();
        if (f < D)
          for (int r = grp; r < c; r += groups) {
            const float v = if_value<TILE>(X, tile, idx, D, stride, src[s0 + r], f);
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
          }
        for (int o = dp; o < 64; o <<= 1) {
          const float a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
          mn = a < mn ? a : mn;
          mx = b > mx ? b : mx;
        }
        const bool varies = lane < D && mx > mn;
        const unsigned long long mask = __ballot(varies);
        const unsigned nv = (unsigned)__popcll(mask);
        if (nv) {
          const av::u4 d = av::philox_draw(key_n, g, (unsigned long long)i);
          const int k = (int)__umulhi(d.x, nv);
          fsel = __ffsll((unsigned long long)__ballot(varies && __popcll(mask & below) == k)) - 1;
          const float lo = __shfl(mn, fsel, 64), hi = __shfl(mx, fsel, 64);
          const float u = (float)(d.y >> 8) * (1.0f / 16777216.0f);
          th = lo + u * (hi - lo);
          if (!(th < hi)) th = lo;
          int nl = 0, nr = 0;
          for (int r0 = 0; r0 < c; r0 += 64) {
            const int r = r0 + lane;
            const bool act = r < c;
            const int slot = act ? src[s0 + r] : src[s0];
            const bool go = act && if_value<TILE>(X, tile, idx, D, stride, slot, fsel) > th;
            const unsigned long long bl = __ballot(act && !go), br = __ballot(go);
            if (act)
              dst[go ? s0 + c - 1 - (nr + __popcll(br & below)) : s0 + nl + __popcll(bl & below)] =
                  (unsigned short)slot;
            nl += __popcll(bl);
            nr += __popcll(br);
          }
          if (lane == 0) {
            hstart[2 * i + 1] = (unsigned short)s0;
            hcnt[2 * i + 1] = (unsigned short)nl;
            hstart[2 * i + 2] = (unsigned short)(s0 + nl);
            hcnt[2 * i + 2] = (unsigned short)(c - nl);
          }
        }
      }
      if (lane == 0) {
        tf[i] = fsel;
        tt[i] = th;
        ts[i] = c;
      }
    }
    __syncthreads();
  }
  for (int i = (1 << L) - 1 + tid; i < M; i += IFB_T) {
    tf[i] = -1;
    tt[i] = 0.0f;
    ts[i] = hcnt[i];
  }
}

// K trees at once: K independent chains of LDS reads.  The terms join acc in tree order.
template <int K>
__device__ __forceinline__ void if_walk(const int2* tr, int M, int L, const float* xr, float& acc) {
  int node[K], depth[K];
#pragma unroll
  for (int k = 0; k < K; ++k) node[k] = depth[k] = 0;
  for (int s = 0; s < L; ++s) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int2 nd = tr[k * M + node[k]];
      const bool inner = nd.x >= 0;
      const float xv = xr[inner ? nd.x : 0];
      node[k] = inner ? 2 * node[k] + 1 + (xv > __int_as_float(nd.y) ? 1 : 0) : node[k];
      depth[k] += inner ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) acc = acc + ((float)depth[k] + __int_as_float(tr[k * M + node[k]].y));
}

__global__ __launch_bounds__(256) void iforest_score_kernel(const float* __restrict__ X, long long n, int D,
                                                            const int2* __restrict__ nodes, int T, int M, int L,
                                                            int tile_ints, int chunk_trees, float* __restrict__ out) {
  extern __shared__ int lds[];
  float* xs = reinterpret_cast<float*>(lds);               // [rows][D | 1]
  int2* tr = reinterpret_cast<int2*>(lds + tile_ints);     // [chunk_trees][M]
  const int tid = threadIdx.x, rows = blockDim.x, stride = D | 1;
  const long long r0 = (long long)blockIdx.x * rows;
  const int nr = (int)min((long long)rows, n - r0);
  const float* src = X + r0 * D;
  for (int i = tid; i < nr * D; i += rows) {
    const int r = i / D;
    xs[r * stride + (i - r * D)] = src[i];
  }
  const bool active = tid < nr;
  const float* xr = xs + (active ? tid : 0) * stride;
  float acc = 0.0f;
  for (int t0 = 0; t0 < T; t0 += chunk_trees) {
    const int nt = min(chunk_trees, T - t0);
    __syncthreads();
    const int2* g = nodes + (long long)t0 * M;
    for (int i = tid; i < nt * M; i += rows) {
      int2 v = g[i];
      if (v.x < -1 || v.x >= D) v.x = -1;
      tr[i] = v;
    }
    __syncthreads();
    if (active) {
      int t = 0;
      for (; t + 4 <= nt; t += 4) if_walk<4>(tr + t * M, M, L, xr, acc);
      for (; t < nt; ++t) if_walk<1>(tr + t * M, M, L, xr, acc);
    }
  }
  if (active) out[r0 + tid] = acc / (float)T;
}

int if_depth(int psi) {
  int L = 1;
  while ((1 << L) < psi) ++L;
  return L;
}

}  // namespace

namespace avk {

void iforest_build(const float* X, long long n, int D, int psi, int T, unsigned long long seed,
                   unsigned long long tree_base, int* feat, float* thr, int* size, hipStream_t stream) {
  if (n < 1 || n >= (1LL << 31)) throw std::runtime_error("iforest_build: 1 <= n < 2^31");
  if (D < 1 || D > 64) throw std::runtime_error("iforest_build: 1 <= D <= 64");
  if (psi < 1 || psi > IFB_PSI || psi > n) throw std::runtime_error("iforest_build: 1 <= psi <= min(1024, n)");
  if (T < 1) throw std::runtime_error("iforest_build: at least one tree");
  const int L = if_depth(psi);
  int dp = 1;
  while (dp < D) dp <<= 1;
  const size_t tile = (size_t)psi * (D | 1) * sizeof(float);
  const unsigned long long ks = seed ^ IF_SAMPLE_KEY, kn = seed ^ IF_NODE_KEY;
  if (tile <= (size_t)IFB_TILE_BYTES)
    iforest_build_kernel<true><<<(unsigned)T, IFB_T, tile, stream>>>(X, n, D, dp, psi, L, ks, kn, tree_base, feat, thr,
                                                                    size);
  else
    iforest_build_kernel<false><<<(unsigned)T, IFB_T, 0, stream>>>(X, n, D, dp, psi, L, ks, kn, tree_base, feat, thr,
                                                                  size);
  AV_HIP_CHECK(hipGetLastError());
}

void iforest_score(const float* X, long long n, int D, const int* nodes, int T, int L, float* out,
                   hipStream_t stream) {
  if (D < 1 || D > 64) throw std::runtime_error("iforest_score: 1 <= D <= 64");
  if (L < 1 || L > 10) throw std::runtime_error("iforest_score: 1 <= depth <= 10 (psi <= 1024)");
  if (T < 1) throw std::runtime_error("iforest_score: at least one tree");
  if (n < 0) throw std::runtime_error("iforest_score: n >= 0");
  if (n == 0) return;
  const int M = (2 << L) - 1;
  const int rows = D <= 32 ? 256 : 128;
  const long long grid = (n + rows - 1) / rows;
  if (grid > INT_MAX) throw std::runtime_error("iforest_score: too many rows");
  const int tile_ints = (rows * (D | 1) + 1) & ~1;        // the trees start 8-byte aligned
  const int chunk_trees = std::min(T, std::max(1, IF_CHUNK_BYTES / (M * 8)));
  const size_t lds = (size_t)tile_ints * 4 + (size_t)chunk_trees * M * 8;
  iforest_score_kernel<<<(unsigned)grid, rows, lds, stream>>>(X, n, D, reinterpret_cast<const int2*>(nodes), T, M, L,
                                                              tile_ints, chunk_trees, out);
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace avk
