// Agglomerative clustering on CDNA4 (gfx950) by rounds of reciprocal nearest pairs over a dense fp32
// matrix: the fill, the row minima, the pair detection and the two Lance-Williams update phases.
//
// The arithmetic is the definition in models/agglo.py (agglo_twin), operation for operation:
//
//   * M[i][j] is the pair sum s(i, j) of avenir_pairtile.h (models/dbscan.py), or its correctly
//     rounded square root; the diagonal and the padding columns n .. ld - 1 hold +inf, and so does
//     the column of every slot that has died, so the row sweep reads no mask;
//   * nn[k] minimises the 64-bit key (fp32 bits << 32) | column over row k: entries are >= +0, so
//     bit order is value order and ties go to the smallest column;
//   * i < j merge in a round iff nn[i] = j and nn[j] = i; slot i survives;
//   * new distances are Lance-Williams in fp32 with every operation rounded on its own (fp contract
//     off, IEEE division); the pairs of a round count as applied in ascending order of the survivor.
//
// M stays symmetric bit for bit, so the new row of a survivor i is a function of its old row and
// of the row of its dead partner j alone (phase 1), and the new entries of a row r that does not
// merge are a function of row r alone (phase 2): what pair q = (k, l) makes of d(r, k), d(r, l) is
// the same LW_q whichever of the two rows computes it.  No kernel reads what another workgroup of
// the same launch writes; the rows of dead slots are never written again and never read after the
// round they died in.  The output is a set of merge records whose order is free (the host sorts
// them), so the atomic appends make no result depend on the execution order.
#include <cmath>
#include <stdexcept>
#include <string>

#include "avenir_common.h"
#include "avenir_kernels.h"
#include "avenir_pairtile.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int AG_T = 256;          // threads per workgroup of every kernel here
constexpr int AG_WAVE_ROW = 512;   // rows of up to this many floats take one wave, longer ones a workgroup

__device__ __forceinline__ float ag_inf() { return __int_as_float(0x7f800000); }

// ---- matrix fill --------------------------------------------------------------------------------
// lanes hold the columns j, tiles the rows i; top takes the largest off-diagonal bit pattern
template <int DMAX, int MET, bool SQRT>
__global__ __launch_bounds__(DB_T) void agglo_fill_kernel(const float* __restrict__ X, long long n, int D, long long ld,
                                                          long long a_range, float* __restrict__ M,
                                                          unsigned* __restrict__ top) {
  constexpr int AR = db_tile_rows<DMAX>();
  __shared__ float4 As[AR][DMAX / 4];
  const long long j = (long long)blockIdx.x * DB_T + threadIdx.x;
  const bool active = j < n;
  f2 b[DMAX / 2];
  db_load_row<DMAX>(b, X, j, active, D);
  const long long a_begin = (long long)blockIdx.y * a_range, a_end = min(n, a_begin + a_range);
  unsigned mx = 0;
  for (long long a0 = a_begin; a0 < a_end; a0 += AR) {
    __syncthreads();
    db_load_tile<DMAX, AR>(As, X, a0, a_end, D);
    __syncthreads();
    const int na = (int)min((long long)AR, a_end - a0);
#pragma unroll 4
    for (int r = 0; r < na; ++r) {
      const long long i = a0 + r;
      float v = db_pair<DMAX, MET>(As[r], b);
      if constexpr (SQRT) v = sqrtf(v);   // the correctly rounded expansion (no fast-math flag in this build)
      if (!active || i == j) v = ag_inf();
      else mx = max(mx, (unsigned)__float_as_int(v));
      if (j < ld) M[i * ld + j] = v;
    }
  }
  mx = av::wave_max(mx);
  if (av::lane_id() == 0 && mx) atomicMax(top, mx);
}

// ---- row minima ---------------------------------------------------------------------------------
__device__ __forceinline__ u64 ag_key_min(u64 a, u64 b) { return a < b ? a : b; }

template <int CTRL>
__device__ __forceinline__ u64 ag_dpp(u64 v) {
  const unsigned lo = (unsigned)av::dpp_i<CTRL>((int)(unsigned)v), hi = (unsigned)av::dpp_i<CTRL>((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 ag_lane(u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// the steps of av::wave_reduce_f on a 64-bit key; the result is wave-uniform
__device__ __forceinline__ u64 ag_wave_min(u64 v) {
  v = ag_key_min(v, ag_dpp<0xB1>(v));    // quad_perm [1,0,3,2]
  v = ag_key_min(v, ag_dpp<0x4E>(v));    // quad_perm [2,3,0,1]
  v = ag_key_min(v, ag_dpp<0x124>(v));   // row_ror:4
  v = ag_key_min(v, ag_dpp<0x128>(v));   // row_ror:8
  return ag_key_min(ag_key_min(ag_lane(v, 0), ag_lane(v, 16)), ag_key_min(ag_lane(v, 32), ag_lane(v, 48)));
}

// WPR waves per row: 1 (four rows per workgroup) or 4 (one row per workgroup)
template <int WPR>
__global__ __launch_bounds__(AG_T) void agglo_rowmin_kernel(const float* __restrict__ M, long long ld,
                                                            const int* __restrict__ act, int n_act,
                                                            u64* __restrict__ key) {
  __shared__ u64 part[4];
  const int wave = av::wave_id(), lane = av::lane_id();
  const long long slot = WPR == 1 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
  if (slot >= n_act) return;   // a whole wave (WPR 1); never taken for WPR 4
  const int r = act[slot];
  const float4* __restrict__ row = reinterpret_cast<const float4*>(M + (long long)r * ld);
  const int nq = (int)(ld >> 2);
  unsigned bb = 0xffffffffu, bc = 0xffffffffu;   // above every entry: the first one read wins
#pragma unroll 4
  for (int q = WPR == 1 ? lane : (int)threadIdx.x; q < nq; q += 64 * WPR) {
    const float4 v = row[q];
    const unsigned c = 4u * (unsigned)q;
    const unsigned e0 = __float_as_int(v.x), e1 = __float_as_int(v.y), e2 = __float_as_int(v.z), e3 = __float_as_int(v.w);
    if (e0 < bb) { bb = e0; bc = c; }            // ascending columns: strict, the first minimum stays
    if (e1 < bb) { bb = e1; bc = c + 1; }
    if (e2 < bb) { bb = e2; bc = c + 2; }
    if (e3 < bb) { bb = e3; bc = c + 3; }
  }
  const u64 k = ag_wave_min(((u64)bb << 32) | bc);
  if constexpr (WPR == 1) {
    if (lane == 0) key[r] = k;
  } else {
    if (lane == 0) part[wave] = k;
    __syncthreads();
    if (threadIdx.x == 0) key[r] = ag_key_min(ag_key_min(part[0], part[1]), ag_key_min(part[2], part[3]));
  }
}

// ---- pair detection -----------------------------------------------------------------------------
// cnt[0] counts the pairs, cnt[1] the slots that stay active (both zero on entry); mate[k] is the
// partner of every active slot k, or -1.  The records of this round go to h, rnd, si, sj from
// ``done`` on, in any order.
__global__ __launch_bounds__(AG_T) void agglo_detect_kernel(const u64* __restrict__ key, int n,
                                                            const int* __restrict__ act, int n_act,
                                                            int* __restrict__ act_next, int* __restrict__ pairs,
                                                            int* __restrict__ mate, int* __restrict__ cnt,
                                                            float* __restrict__ h, int* __restrict__ rnd,
                                                            int* __restrict__ si, int* __restrict__ sj, int done,
                                                            int round) {
  const long long t = (long long)blockIdx.x * AG_T + threadIdx.x;
  if (t >= n_act) return;
  const int k = act[t];
  const u64 kk = key[k];
  const unsigned j = (unsigned)kk;
  const bool rec = j < (unsigned)n && j != (unsigned)k && (unsigned)key[j] == (unsigned)k;
  mate[k] = rec ? (int)j : -1;
  if (rec && (unsigned)k > j) return;   // this slot dies
  act_next[atomicAdd(&cnt[1], 1)] = k;
  if (rec) {
    const int p = atomicAdd(&cnt[0], 1);
    pairs[p] = k;
    h[done + p] = __int_as_float((int)(unsigned)(kk >> 32));
    rnd[done + p] = round;
    si[done + p] = k;
    sj[done + p] = (int)j;
  }
}

// ---- Lance-Williams -----------------------------------------------------------------------------
// a = d(i, k), b = d(j, k), c = d(i, j); 0 single, 1 complete, 2 average, 3 ward (on squares)
template <int LINK>
__device__ __forceinline__ float ag_lw(float a, float b, float c, float ni, float nj, float nk) {
  if constexpr (LINK == 0) {
    return fminf(a, b);
  } else if constexpr (LINK == 1) {
    return fmaxf(a, b);
  } else if constexpr (LINK == 2) {
    const float ta = ni * a, tb = nj * b;
    return fmaxf((ta + tb) / (ni + nj), c);
  } else {
    const float ta = (ni + nk) * a, tb = (nj + nk) * b, tc = nk * c;
    return fmaxf(((ta + tb) - tc) / ((ni + nj) + nk), c);
  }
}

__device__ __forceinline__ float ag_height(u64 key) { return __int_as_float((int)(unsigned)(key >> 32)); }

// Phase 1: the survivor i of pair blockIdx.x rewrites its own row from its old row and row j.
// Against a pair q = (k, l) the two updates nest in the order of the survivors; thread k writes
// (i, k), nobody writes (i, l) here (phase 2 does), and thread l does nothing.
template <int LINK>
__global__ __launch_bounds__(AG_T) void agglo_merge_rows_kernel(float* __restrict__ M, long long ld, int n,
                                                                const int* __restrict__ pairs,
                                                                const int* __restrict__ mate,
                                                                const int* __restrict__ size,
                                                                const u64* __restrict__ key) {
  const int c = blockIdx.y * AG_T + threadIdx.x;
  if (c >= n) return;
  const int i = pairs[blockIdx.x], j = mate[i];
  const int nc = size[c], mc = mate[c];
  if (nc == 0 || c == i || c == j) return;      // dead before this round, or the pair itself
  if (mc >= 0 && c > mc) return;                // dies in this round
  float* __restrict__ Ri = M + (long long)i * ld;
  const float* __restrict__ Rj = M + (long long)j * ld;
  const float ni = (float)size[i], nj = (float)size[j], cp = ag_height(key[i]);
  float out;
  if (mc < 0) {
    out = ag_lw<LINK>(Ri[c], Rj[c], cp, ni, nj, (float)nc);
  } else {
    const int l = mc;                           // c = k survives pair q = (k, l)
    const float nk = (float)nc, nl = (float)size[l], cq = ag_height(key[c]);
    const float aik = Ri[c], ajk = Rj[c], ail = Ri[l], ajl = Rj[l];
    if (i < c) {                                // p first, then q
      const float rk = ag_lw<LINK>(aik, ajk, cp, ni, nj, nk), rl = ag_lw<LINK>(ail, ajl, cp, ni, nj, nl);
      out = ag_lw<LINK>(rk, rl, cq, nk, nl, ni + nj);
    } else {                                    // q first, then p
      const float ri = ag_lw<LINK>(aik, ail, cq, nk, nl, ni), rj = ag_lw<LINK>(ajk, ajl, cq, nk, nl, nj);
      out = ag_lw<LINK>(ri, rj, cp, ni, nj, nk + nl);
    }
  }
  Ri[c] = out;
}

// Phase 2: the columns.  Row r = act_next[blockIdx.x], thread t takes pair t = (k, l): a row that
// does not merge computes d(r, k) from its own two entries, every row gets +inf in column l.
template <int LINK>
__global__ __launch_bounds__(AG_T) void agglo_columns_kernel(float* __restrict__ M, long long ld,
                                                             const int* __restrict__ act_next,
                                                             const int* __restrict__ pairs, int n_pairs,
                                                             const int* __restrict__ mate,
                                                             const int* __restrict__ size,
                                                             const u64* __restrict__ key) {
  const int t = blockIdx.y * AG_T + threadIdx.x;
  if (t >= n_pairs) return;
  const int r = act_next[blockIdx.x];
  const int k = pairs[t], l = mate[k];
  float* __restrict__ Rr = M + (long long)r * ld;
  if (mate[r] < 0)
    Rr[k] = ag_lw<LINK>(Rr[k], Rr[l], ag_height(key[k]), (float)size[k], (float)size[l], (float)size[r]);
  Rr[l] = ag_inf();
}

// after both phases: the survivor takes the size of the pair
__global__ __launch_bounds__(AG_T) void agglo_sizes_kernel(const int* __restrict__ pairs, int n_pairs,
                                                           const int* __restrict__ mate, int* __restrict__ size) {
  const int t = blockIdx.x * AG_T + threadIdx.x;
  if (t >= n_pairs) return;
  const int i = pairs[t], j = mate[i];
  size[i] += size[j];
  size[j] = 0;
}

template <int LINK>
void ag_update(float* M, long long n, long long ld, const int* act_next, int n_next, const int* pairs, int n_pairs,
               const int* mate, int* size, const u64* key, hipStream_t stream) {
  const dim3 g1((unsigned)n_pairs, (unsigned)((n + AG_T - 1) / AG_T));
  agglo_merge_rows_kernel<LINK><<<g1, AG_T, 0, stream>>>(M, ld, (int)n, pairs, mate, size, key);
  const dim3 g2((unsigned)n_next, (unsigned)((n_pairs + AG_T - 1) / AG_T));
  agglo_columns_kernel<LINK><<<g2, AG_T, 0, stream>>>(M, ld, act_next, pairs, n_pairs, mate, size, key);
  agglo_sizes_kernel<<<(unsigned)((n_pairs + AG_T - 1) / AG_T), AG_T, 0, stream>>>(pairs, n_pairs, mate, size);
}

}  // namespace

namespace avk {

// M [n][ld] = s(i, j) or its square root, +inf on the diagonal and in columns n .. ld - 1; top[0]
// (zero on entry) = the largest off-diagonal bit pattern
void agglo_matrix(const float* X, long long n, int D, int metric, bool take_sqrt, float* M, long long ld,
                  unsigned* top, hipStream_t stream) {
  if (n < 1 || n >= (1LL << 24)) throw std::runtime_error("agglo_matrix: 1 <= n < 2^24");
  if (D < 1 || D > 64) throw std::runtime_error("agglo_matrix: 1 <= D <= 64");
  if (metric != 0 && metric != 1) throw std::runtime_error("agglo_matrix: metric 0 (euclidean) or 1 (manhattan)");
  if (ld < n || ld % 4) throw std::runtime_error("agglo_matrix: ld must be a multiple of 4 and >= n");
  const int AR = db_rows(D);
  const long long rg = db_range(n, ld, AR, 0, 2048);
  const dim3 grid((unsigned)((ld + DB_T - 1) / DB_T), (unsigned)((n + rg - 1) / rg));
#define AV_AG_FILL(DM, ME)                                                                              \
  do {                                                                                                  \
    if (take_sqrt) agglo_fill_kernel<DM, ME, true><<<grid, DB_T, 0, stream>>>(X, n, D, ld, rg, M, top); \
    else agglo_fill_kernel<DM, ME, false><<<grid, DB_T, 0, stream>>>(X, n, D, ld, rg, M, top);          \
  } while (0)
  AV_DB_DISPATCH(AV_AG_FILL);
#undef AV_AG_FILL
  AV_HIP_CHECK(hipGetLastError());
}

// The rounds.  On entry size [n] holds ones, act [2][n] the identity in its first half, cnt [2 * n]
// zeros; key [n], mate [n], pairs [n] are scratch.  h, rnd, si, sj [n - 1] take the merge records.
// One counter is read back per round; at most n - 1 rounds.  Returns the number of rounds.
int agglo_merge(float* M, long long n, long long ld, int linkage, unsigned long long* key, int* mate, int* size,
                int* act, int* pairs, int* cnt, float* h, int* rnd, int* si, int* sj, hipStream_t stream) {
  if (n < 1 || n >= (1LL << 24)) throw std::runtime_error("agglo_merge: 1 <= n < 2^24");
  if (ld < n || ld % 4) throw std::runtime_error("agglo_merge: ld must be a multiple of 4 and >= n");
  if (linkage < 0 || linkage > 3) throw std::runtime_error("agglo_merge: linkage 0 .. 3");
  int n_act = (int)n, done = 0, round = 0, cur = 0;
  while (n_act > 1) {
    if (round >= n - 1) throw std::runtime_error("agglo_merge: not finished after n - 1 rounds");
    const int* a = act + (long long)cur * n;
    int* a_next = act + (long long)(1 - cur) * n;
    if (ld <= AG_WAVE_ROW)
      agglo_rowmin_kernel<1><<<(unsigned)((n_act + 3) / 4), AG_T, 0, stream>>>(M, ld, a, n_act, key);
    else
      agglo_rowmin_kernel<4><<<(unsigned)n_act, AG_T, 0, stream>>>(M, ld, a, n_act, key);
    agglo_detect_kernel<<<(unsigned)((n_act + AG_T - 1) / AG_T), AG_T, 0, stream>>>(
        key, (int)n, a, n_act, a_next, pairs, mate, cnt + 2 * round, h, rnd, si, sj, done, round);
    AV_HIP_CHECK(hipGetLastError());
    int n_pairs = 0;
    AV_HIP_CHECK(hipMemcpyAsync(&n_pairs, cnt + 2 * round, sizeof(int), hipMemcpyDeviceToHost, stream));
    AV_HIP_CHECK(hipStreamSynchronize(stream));
    if (n_pairs < 1 || 2 * n_pairs > n_act)
      throw std::runtime_error("agglo_merge: round " + std::to_string(round) + " found " + std::to_string(n_pairs) +
                               " reciprocal pairs among " + std::to_string(n_act) + " clusters");
    const int n_next = n_act - n_pairs;
    if (n_next > 1) {
      switch (linkage) {
        case 0: ag_update<0>(M, n, ld, a_next, n_next, pairs, n_pairs, mate, size, key, stream); break;
        case 1: ag_update<1>(M, n, ld, a_next, n_next, pairs, n_pairs, mate, size, key, stream); break;
        case 2: ag_update<2>(M, n, ld, a_next, n_next, pairs, n_pairs, mate, size, key, stream); break;
        default: ag_update<3>(M, n, ld, a_next, n_next, pairs, n_pairs, mate, size, key, stream); break;
      }
      AV_HIP_CHECK(hipGetLastError());
    }
    done += n_pairs;
    n_act = n_next;
    cur = 1 - cur;
    ++round;
  }
  return round;
}

}  // namespace avk
