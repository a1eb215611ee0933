// DBSCAN on CDNA4 (gfx950): exact neighbour counts, a lock-free union-find over the core graph and
// the border sweep.  No kernel stores a distance block or an adjacency list: memory is O(n * D).
//
// The arithmetic is the definition in models/dbscan.py (dbscan_twin), operation for operation:
//
//   * t = x[i, d] - x[j, d] in fp32; euclidean adds t * t, manhattan |t|; every subtraction,
//     product and add is rounded on its own (fp contract off);
//   * the even columns are summed in one chain in ascending d, the odd columns in another, and
//     s = even + odd (the two halves of a packed fp32 register, as pairs_within_kernel keeps them);
//     zero padding columns add exact zeros, so every D class gives the same bits;
//   * j is a neighbour of i iff s <= thr.  thr is found on the host: for the euclidean metric the
//     largest fp32 v with sqrtf(v) <= eps (so the kernel needs no square root), for manhattan
//     float(eps).  s is symmetric in (i, j): (a - b)^2 and |a - b| round as (b - a)^2 and |b - a|.
//
// Every output is an integer that depends on the predicate alone (a count, a minimum, the smallest
// index of a connected component), so the result depends on no grid, split or execution order.
//
// Tile shape of pairs_within_kernel (distance.hip): a workgroup holds AR "A" rows in LDS (256 for
// rows of <= 16 floats, else 64), read by broadcast, 4 floats per read; each of its 256 lanes holds
// one "B" row in registers.  A workgroup walks the A tiles of one range of a_range rows (grid.y);
// the partial results of the ranges meet by integer atomics.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>

#include "avenir_common.h"
#include "avenir_kernels.h"

#pragma clang fp contract(off)

#include "avenir_pairtile.h"

namespace {

// ---- counts -------------------------------------------------------------------------------------
template <int DMAX, int MET>
__global__ __launch_bounds__(DB_T) void dbscan_count_kernel(const float* __restrict__ X, long long n, int D, float thr,
                                                            long long a_range, int* __restrict__ counts) {
  constexpr int AR = db_tile_rows<DMAX>();
  __shared__ float4 As[AR][DMAX / 4];
  const long long j = (long long)blockIdx.x * DB_T + threadIdx.x;
  const bool active = j < n;
  f2 b[DMAX / 2];
  db_load_row<DMAX>(b, X, j, active, D);
  const long long a_begin = (long long)blockIdx.y * a_range, a_end = min(n, a_begin + a_range);
  int cnt = 0;
  for (long long a0 = a_begin; a0 < a_end; a0 += AR) {
    __syncthreads();
    db_load_tile<DMAX, AR>(As, X, a0, a_end, D);
    __syncthreads();
    const int na = (int)min((long long)AR, a_end - a0);
#pragma unroll 4
    for (int r = 0; r < na; ++r) cnt += db_pair<DMAX, MET>(As[r], b) <= thr ? 1 : 0;
  }
  if (active && cnt) atomicAdd(&counts[j], cnt);
}

// ---- union-find ---------------------------------------------------------------------------------
// parent[x] <= x always.  find walks to the node that is its own parent; unite hooks the larger of
// two roots under the smaller with an atomic min and, when the node turned out not to be a root any
// more, carries on with the parent the min displaced (or kept).  Take the graph of the parent edges
// plus one edge per unite still under way: no step of find or unite splits one of its components,
// and a stale read only yields an earlier ancestor, which is in the same component.  So once every
// unite has returned, each component is one tree whose root is its smallest index.  Every loop
// moves to strictly smaller indices and no lane waits for another, so each terminates.
// G: parent in global memory (agent-scope atomics: the L2s of the XCDs are not coherent for plain
// loads); otherwise in LDS (workgroup scope).
template <bool G>
__device__ __forceinline__ int uf_load(int* p) {
  if constexpr (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool G>
__device__ __forceinline__ int uf_min(int* p, int v) {
  if constexpr (G) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool G>
__device__ __forceinline__ int uf_find(int* parent, int x) {
  for (;;) {
    const int p = uf_load<G>(parent + x);
    if (p == x) return x;
    x = p;   // p < x
  }
}

template <bool G>
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find<G>(parent, a);
    b = uf_find<G>(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // a > b
    const int old = uf_min<G>(parent + a, b);
    if (old == a) return;   // a was a root and now hangs under b
    a = old;                // old < a: unite what a pointed to with b
  }
}

// Tiles of Xc x Xc on or above the diagonal.  Adjacent pairs are united in an LDS union-find over
// the tile's AR A rows (nodes 0 .. AR-1) and 256 B rows (nodes AR ..); after a barrier every node
// whose tile root is another node sends ONE union to the global array, so the global traffic is
// bounded by the nodes of a tile, not by its adjacent pairs.
template <int DMAX, int MET>
__global__ __launch_bounds__(DB_T) void dbscan_union_kernel(const float* __restrict__ Xc, long long nc, int D,
                                                            float thr, long long a_range, int* parent) {
  constexpr int AR = db_tile_rows<DMAX>();
  __shared__ float4 As[AR][DMAX / 4];
  __shared__ int lp[AR + DB_T];
  const long long b0 = (long long)blockIdx.x * DB_T, j = b0 + threadIdx.x;
  const bool active = j < nc;
  const long long j_last = min(nc, b0 + DB_T) - 1;
  f2 b[DMAX / 2];
  db_load_row<DMAX>(b, Xc, j, active, D);
  const long long a_begin = (long long)blockIdx.y * a_range, a_end = min(nc, a_begin + a_range);
  const int me = AR + threadIdx.x;
  for (long long a0 = a_begin; a0 < a_end; a0 += AR) {
    // every pair of this and of each later tile has j <= i: the mirrored tile covers it (uniform)
    if (j_last <= a0) break;
    __syncthreads();
    db_load_tile<DMAX, AR>(As, Xc, a0, a_end, D);
    for (int k = threadIdx.x; k < AR + DB_T; k += DB_T) lp[k] = k;
    __syncthreads();
    const int na = (int)min((long long)AR, a_end - a0);
    if (active) {
      for (int r = 0; r < na; ++r)
        if (db_pair<DMAX, MET>(As[r], b) <= thr && uf_find<false>(lp, r) != uf_find<false>(lp, me))
          uf_unite<false>(lp, r, me);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < AR + DB_T; k += DB_T) {
      const int root = uf_find<false>(lp, k);   // only rows that exist were ever united
      if (root != k)
        uf_unite<true>(parent, (int)(k < AR ? a0 + k : b0 + (k - AR)), (int)(root < AR ? a0 + root : b0 + (root - AR)));
    }
  }
}

// after the kernel boundary: plain loads see every union
__global__ __launch_bounds__(DB_T) void dbscan_flatten_kernel(const int* __restrict__ parent, long long nc,
                                                              int* __restrict__ root) {
  const long long c = (long long)blockIdx.x * DB_T + threadIdx.x;
  if (c >= nc) return;
  int x = (int)c;
  for (int p = parent[x]; p != x; p = parent[x]) x = p;
  root[c] = x;
}

// ---- border points ------------------------------------------------------------------------------
// lanes hold the non-core candidates, tiles the core rows with their roots beside them
template <int DMAX, int MET>
__global__ __launch_bounds__(DB_T) void dbscan_border_kernel(const float* __restrict__ Xb, long long nb,
                                                             const float* __restrict__ Xc, long long nc,
                                                             const int* __restrict__ root, int D, float thr,
                                                             long long a_range, int* __restrict__ min_root) {
  constexpr int AR = db_tile_rows<DMAX>();
  __shared__ float4 As[AR][DMAX / 4];
  __shared__ int s_root[AR];
  const long long j = (long long)blockIdx.x * DB_T + threadIdx.x;
  const bool active = j < nb;
  f2 b[DMAX / 2];
  db_load_row<DMAX>(b, Xb, j, active, D);
  const long long a_begin = (long long)blockIdx.y * a_range, a_end = min(nc, a_begin + a_range);
  int m = INT_MAX;
  for (long long a0 = a_begin; a0 < a_end; a0 += AR) {
    __syncthreads();
    db_load_tile<DMAX, AR>(As, Xc, a0, a_end, D);
    for (int r = threadIdx.x; r < AR; r += DB_T) s_root[r] = a0 + r < a_end ? root[a0 + r] : INT_MAX;
    __syncthreads();
    const int na = (int)min((long long)AR, a_end - a0);
#pragma unroll 4
    for (int r = 0; r < na; ++r)
      if (db_pair<DMAX, MET>(As[r], b) <= thr) m = min(m, s_root[r]);
  }
  if (active && m != INT_MAX) atomicMin(&min_root[j], m);
}

void db_check(const char* what, long long nA, long long nB, int D, int metric, float thr, long long a_range) {
  const std::string w(what);
  if (nA < 0 || nB < 0 || nA >= (1LL << 31) || nB >= (1LL << 31)) throw std::runtime_error(w + ": rows must be < 2^31");
  if (D < 1 || D > 64) throw std::runtime_error(w + ": 1 <= D <= 64");
  if (metric != 0 && metric != 1) throw std::runtime_error(w + ": metric 0 (euclidean) or 1 (manhattan)");
  if (!(thr >= 0.f) || !std::isfinite(thr)) throw std::runtime_error(w + ": the threshold must be finite and >= 0");
  if (a_range < 0) throw std::runtime_error(w + ": a_range must be >= 0");
}

}  // namespace

namespace avk {

// counts[j] += |{i : s(i, j) <= thr}| (the point itself included); counts must be zero on entry
void dbscan_count(const float* X, long long n, int D, int metric, float thr, long long a_range, int* counts,
                  hipStream_t stream) {
  db_check("dbscan_count", n, n, D, metric, thr, a_range);
  if (n == 0) return;
  const int AR = db_rows(D);
  const long long rg = db_range(n, n, AR, a_range, 2048);
  const dim3 grid((unsigned)((n + DB_T - 1) / DB_T), (unsigned)((n + rg - 1) / rg));
#define AV_DB_COUNT(DM, ME) dbscan_count_kernel<DM, ME><<<grid, DB_T, 0, stream>>>(X, n, D, thr, rg, counts)
  AV_DB_DISPATCH(AV_DB_COUNT);
#undef AV_DB_COUNT
  AV_HIP_CHECK(hipGetLastError());
}

// parent [nc] must hold the identity on entry; root[c] = smallest index of c's component
void dbscan_union(const float* Xc, long long nc, int D, int metric, float thr, long long a_range, int* parent,
                  int* root, hipStream_t stream) {
  db_check("dbscan_union", nc, nc, D, metric, thr, a_range);
  if (nc == 0) return;
  const int AR = db_rows(D);
  const long long rg = db_range(nc, nc, AR, a_range, 8192);
  const dim3 grid((unsigned)((nc + DB_T - 1) / DB_T), (unsigned)((nc + rg - 1) / rg));
#define AV_DB_UNION(DM, ME) dbscan_union_kernel<DM, ME><<<grid, DB_T, 0, stream>>>(Xc, nc, D, thr, rg, parent)
  AV_DB_DISPATCH(AV_DB_UNION);
#undef AV_DB_UNION
  AV_HIP_CHECK(hipGetLastError());
  dbscan_flatten_kernel<<<(unsigned)((nc + DB_T - 1) / DB_T), DB_T, 0, stream>>>(parent, nc, root);
  AV_HIP_CHECK(hipGetLastError());
}

// min_root[j] = min(min_root[j], smallest root among the core neighbours of candidate j); min_root
// must hold INT_MAX on entry
void dbscan_border(const float* Xb, long long nb, const float* Xc, long long nc, const int* root, int D, int metric,
                   float thr, long long a_range, int* min_root, hipStream_t stream) {
  db_check("dbscan_border", nc, nb, D, metric, thr, a_range);
  if (nb == 0 || nc == 0) return;
  const int AR = db_rows(D);
  const long long rg = db_range(nc, nb, AR, a_range, 2048);
  const dim3 grid((unsigned)((nb + DB_T - 1) / DB_T), (unsigned)((nc + rg - 1) / rg));
#define AV_DB_BORDER(DM, ME) \
  dbscan_border_kernel<DM, ME><<<grid, DB_T, 0, stream>>>(Xb, nb, Xc, nc, root, D, thr, rg, min_root)
  AV_DB_DISPATCH(AV_DB_BORDER);
#undef AV_DB_BORDER
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace avk
