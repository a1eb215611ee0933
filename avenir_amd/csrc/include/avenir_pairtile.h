// The pair tile shared by the kernels that sweep all pairs of rows (dbscan.hip, agglo.hip): the tile
// shape of pairs_within_kernel (distance.hip) and the fp32 pair sum s(i, j) that models/dbscan.py
// defines (_pair_sums), operation for operation.  A workgroup holds AR "A" rows in LDS (256 for rows
// of <= 16 floats, else 64), read by broadcast, 4 floats per read; each of its 256 lanes holds one
// "B" row in registers.  Nothing after this header contracts a product and an add into an FMA.
#pragma once
#include <algorithm>

#include "avenir_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DB_T = 256;   // lanes (= B rows) per workgroup

typedef float f2 __attribute__((ext_vector_type(2)));

template <int DMAX>
constexpr int db_tile_rows() { return DMAX <= 16 ? 256 : 64; }

// the lane's row, columns D..DMAX-1 zero
template <int DMAX>
__device__ __forceinline__ void db_load_row(f2 (&b)[DMAX / 2], const float* __restrict__ X, long long j, bool active,
                                            int D) {
#pragma unroll
  for (int c = 0; c < DMAX / 2; ++c)
    b[c] = f2{active && 2 * c < D ? X[j * D + 2 * c] : 0.f, active && 2 * c + 1 < D ? X[j * D + 2 * c + 1] : 0.f};
}

// rows a0 .. a0 + AR - 1 of A into LDS; rows past nA and columns past D are zero
template <int DMAX, int AR>
__device__ __forceinline__ void db_load_tile(float4 (&As)[AR][DMAX / 4], const float* __restrict__ A, long long a0,
                                             long long nA, int D) {
  float* Af = reinterpret_cast<float*>(As);
  for (int e = threadIdx.x; e < AR * DMAX; e += DB_T) {
    const int r = e / DMAX, c = e - r * DMAX;
    Af[e] = (a0 + r < nA && c < D) ? A[(a0 + r) * D + c] : 0.f;
  }
}

// s(i, j): the contract's sum, even columns in .x, odd columns in .y
template <int DMAX, int MET>
__device__ __forceinline__ float db_pair(const float4* __restrict__ row, const f2 (&b)[DMAX / 2]) {
  f2 acc = f2{0.f, 0.f};
#pragma unroll
  for (int c4 = 0; c4 < DMAX / 4; ++c4) {
    const float4 a = row[c4];
    const f2 d0 = f2{a.x, a.y} - b[2 * c4], d1 = f2{a.z, a.w} - b[2 * c4 + 1];
    if constexpr (MET == 0) {
      acc = acc + d0 * d0;
      acc = acc + d1 * d1;
    } else {
      acc = acc + __builtin_elementwise_abs(d0);
      acc = acc + __builtin_elementwise_abs(d1);
    }
  }
  return acc.x + acc.y;
}

// ---- launch geometry ----------------------------------------------------------------------------
// A rows per grid.y range: the caller's value rounded up to whole tiles, else enough ranges for
// ``target`` workgroups; never more than 65535 ranges
long long db_range(long long nA, long long nB, int AR, long long a_range, long long target) {
  const long long gx = (nB + DB_T - 1) / DB_T, tiles = (nA + AR - 1) / AR;
  long long r;
  if (a_range > 0) {
    r = (a_range + AR - 1) / AR * AR;
  } else {
    const long long gy = std::max(1LL, std::min(tiles, target / std::max(1LL, gx)));
    r = (tiles + gy - 1) / gy * AR;
  }
  const long long r_min = (tiles + 65534) / 65535 * AR;
  return std::min(std::max(r, r_min), std::max(tiles, 1LL) * AR);
}

int db_rows(int D) { return D <= 16 ? db_tile_rows<16>() : db_tile_rows<64>(); }

// F(DMAX-class, metric) for the padded D class of D and the metric
#define AV_DB_DISPATCH(F)                                    \
  do {                                                       \
    if (metric == 0) {                                       \
      if (D <= 4) { F(4, 0); }                               \
      else if (D <= 8) { F(8, 0); }                          \
      else if (D <= 16) { F(16, 0); }                        \
      else if (D <= 32) { F(32, 0); }                        \
      else { F(64, 0); }                                     \
    } else {                                                 \
      if (D <= 4) { F(4, 1); }                               \
      else if (D <= 8) { F(8, 1); }                          \
      else if (D <= 16) { F(16, 1); }                        \
      else if (D <= 32) { F(32, 1); }                        \
      else { F(64, 1); }                                     \
    }                                                        \
  } while (0)

}  // namespace
