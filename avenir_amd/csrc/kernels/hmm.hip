// K14b: Baum-Welch E-step for discrete HMMs on CDNA4 (gfx950), one launch per chunk of sequences.
//
// hmm_estep_kernel runs the scaled forward pass, the scaled backward pass and the S x S pair
// posteriors of every step of every sequence, and sums the expected counts exactly:
//
//   * lane layout as viterbi_small_kernel: 64 / SP sequences share a wavefront (SP = power of two
//     >= S, at least 4), lane group g owns a sequence and lane j of the group state j; at
//     33 <= S <= 64 one sequence per wavefront.  Values of other states come by shuffles inside the
//     group (v_readlane at SP = 64).
//   * arithmetic is the definition in models/hmm_em.py (hmm_estep_reference), operation for
//     operation: probability space, fp32, every operation rounded on its own (fp contract off), sums
//     in ascending index order from 0, rescaling by powers of two only (frexp / ldexp), one IEEE
//     division per sequence, and every posterior converted on its own to 2^-32 fixed point (round
//     to nearest even) and added as a 64-bit integer.  Integer sums are order-free, so the result
//     does not depend on the grid, the chunking or the order of the atomics, and equals the twin
//     bit for bit.  The kernel runs in hipcc's default float mode (fp32 subnormals kept), as numpy.
//   * the transition matrix sits in LDS once, rows padded to an odd length: the forward pass walks a
//     column (lanes along a row: consecutive banks), the backward pass a row per lane (odd stride:
//     distinct banks), so one copy serves both walks without conflicts; up to 16 states each lane
//     copies its column and its row into registers once and the loops read no LDS for A.  B is in LDS when it and
//     the [S, O] emission sums fit (template flag LDSB), and read from global memory otherwise.
//   * the forward vectors of every step, and the running exponent, are kept in an HBM workspace
//     [rows, T, S] + [rows, T], written and read by the lane that owns the state.
//   * pair posteriors are summed in registers (lane j holds column j of the [S, S] table), emission
//     posteriors in LDS (ds_add_u64) or, without LDSB, straight into global memory; a block flushes
//     its tables once with 64-bit global atomics.
#include "avenir_common.h"
#include "avenir_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int HT = 256;             // 4 waves per block
constexpr int HMM_MAX_BLOCKS = 2048;
constexpr size_t HMM_LDSB_CAP = 64 * 1024;   // B and the emission sums join A in LDS below this

typedef unsigned long long u64;

struct HmmArgs {
  const short* obs;   // [n, T]; a negative or out-of-range value ends the sequence
  long long n;
  int T, S, O;
  const float* A;     // [S, S]
  const float* B;     // [S, O]
  const float* pi;    // [S]
  u64* trans;         // [S, S]  2^-32 fixed point
  u64* emit;          // [S, O]
  u64* init;          // [S]
  u64* stats;         // sequences, steps, empty, impossible
  float* Z;           // [n]
  int* E;             // [n]
  float* ws_alpha;    // [n, T, S]
  int* ws_exp;        // [n, T]
};

template <int SP>
__device__ __forceinline__ float grp_get(float v, int base, int i) {  // value of the group's lane i (i uniform)
  if constexpr (SP == 64) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
  else return __shfl(v, base + i, 64);
}

template <int SP>
__device__ __forceinline__ float grp_max(float m) {
#pragma unroll
  for (int o = SP / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

__device__ __forceinline__ int bin_exp(float m) {  // frexp exponent; 0 for 0
  int e = 0;
  if (m > 0.f) (void)frexpf(m, &e);
  return e;
}

// v * 2^d rounded to the nearest even integer (v >= 0, the result is far below 2^63)
__device__ __forceinline__ u64 quant(float v, int d) { return (u64)rintf(ldexpf(v, d)); }

template <int SP, bool LDSB>
__global__ __launch_bounds__(HT) void hmm_estep_kernel(const HmmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int G = 64 / SP;
  const int S = a.S, T = a.T, O = a.O, ld = S | 1;
  u64* sT = reinterpret_cast<u64*>(smem);   // [S, S]
  u64* sI = sT + S * S;                     // [S]
  u64* sStat = sI + S;                      // [4]
  u64* sE = sStat + 4;                      // [S, O] when LDSB
  float* sA = reinterpret_cast<float*>(sE + (LDSB ? S * O : 0));  // [S, ld]
  float* sB = sA + S * ld;                  // [S, O] when LDSB
  const int nq = S * S + S + 4 + (LDSB ? S * O : 0);
  for (int i = threadIdx.x; i < nq; i += HT) sT[i] = 0;
  for (int i = threadIdx.x; i < S * S; i += HT) sA[(i / S) * ld + i % S] = a.A[i];
  if (LDSB)
    for (int i = threadIdx.x; i < S * O; i += HT) sB[i] = a.B[i];
  __syncthreads();

  const int lane = threadIdx.x & 63, grp = lane / SP, j = lane % SP, base = grp * SP;
  const bool jS = j < S;
  const int jc = jS ? j : 0;
  const float pij = jS ? a.pi[j] : 0.f;
  u64 tacc[SP];
#pragma unroll
  for (int i = 0; i < SP; ++i) tacc[i] = 0;
  // up to 16 states a lane keeps its column (forward, pairs) and its row (backward) of A in
  // registers; the LDS copy serves the larger models
  constexpr bool AREG = SP <= 16;
  float acol[AREG ? SP : 1], arow[AREG ? SP : 1];
  if constexpr (AREG) {
#pragma unroll
    for (int i = 0; i < SP; ++i) {
      acol[i] = i < S ? sA[i * ld + jc] : 0.f;
      arow[i] = i < S ? sA[jc * ld + i] : 0.f;
    }
  }
  u64 iacc = 0;
  unsigned n_seq = 0, n_empty = 0, n_imp = 0;
  u64 n_steps = 0;

  const long long nwaves = (long long)gridDim.x * (HT / 64);
  const long long ntasks = (a.n + G - 1) / G;
  for (long long task = (long long)blockIdx.x * (HT / 64) + (threadIdx.x >> 6); task < ntasks; task += nwaves) {
    const long long seq = task * G + grp;
    const bool live = seq < a.n;
    const short* ob = a.obs + (live ? seq * T : 0);
    float* wa = a.ws_alpha + (live ? seq * T * S : 0);
    int* we = a.ws_exp + (live ? seq * T : 0);

    // ---- forward: alpha_t(j) = (sum_i alpha_{t-1}(i) A[i][j]) B[j][o_t], rescaled by 2^-e ----
    float alpha = 0.f;
    int L = 0, cexp = 0;
    bool act = live, ok = live;
    for (int t = 0; t < T; ++t) {
      const int ot = act ? ob[t] : -1;
      if (ot < 0 || ot >= O) act = false;
      if (!__any(act)) break;
      float acc = pij;
      if (t > 0) {
        acc = 0.f;
#pragma unroll
        for (int i = 0; i < SP; ++i) {
          if (i < S) {  // wave-uniform
            const float p = grp_get<SP>(alpha, base, i);
            float av;
            if constexpr (AREG) av = acol[i];
            else av = sA[i * ld + jc];
            acc = acc + p * av;
          }
        }
      }
      const float bv = (act && jS) ? (LDSB ? sB[j * O + ot] : a.B[(long long)j * O + ot]) : 0.f;
      const float na = acc * bv;
      const float m = grp_max<SP>(na);
      const int e = bin_exp(m);
      if (act) {
        if (m > 0.f) {
          alpha = ldexpf(na, -e);
          cexp += e;
          if (jS) wa[t * S + j] = alpha;
          if (j == 0) we[t] = cexp;
          ++L;
        } else {  // every state has probability 0: the sequence is impossible under the model
          ok = false;
          act = false;
        }
      }
    }
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < SP; ++i) {
      if (i < S) z = z + grp_get<SP>(alpha, base, i);
    }
    const bool good = ok && L > 0;
    const float rinv = good ? 1.0f / z : 0.f;
    const int Etot = cexp;
    if (live && j == 0) {
      a.Z[seq] = good ? z : 0.f;
      a.E[seq] = good ? Etot : 0;
      if (good) { ++n_seq; n_steps += (u64)L; }
      else if (ok) ++n_empty;
      else ++n_imp;
    }
    __threadfence_block();  // the exponents below were written by the group's lane 0

    // ---- backward: beta_t(i) = sum_j A[i][j] w(j), w(j) = B[j][o_{t+1}] beta_{t+1}(j) ----
    float beta = 0.f;
    int bexp = 0;
    for (int t = T - 1; t >= 0; --t) {
      const bool v = good && t < L;
      if (!__any(v)) continue;
      const float at = (v && jS) ? wa[t * S + j] : 0.f;
      const int ct = v ? we[t] : 0;
      const int ot = v ? ob[t] : 0;
      const bool step = v && t < L - 1;
      if (v && !step) { beta = jS ? 1.f : 0.f; bexp = 0; }
      const int o1 = step ? ob[t + 1] : 0;
      const float w = (step && jS) ? (LDSB ? sB[j * O + o1] : a.B[(long long)j * O + o1]) * beta : 0.f;
      // xi_{t+1}(i, j) = alpha_t(i) A[i][j] w(j) / Z: lane j adds column j
      const int dx = ct + bexp - Etot + 32;
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        if (i < S) {
          const float ai = grp_get<SP>(at, base, i);
          float av;
          if constexpr (AREG) av = acol[i];
          else av = sA[i * ld + jc];
          const float x = ((ai * av) * w) * rinv;
          tacc[i] += quant(x, dx);
        }
      }
      float nb = 0.f;
#pragma unroll
      for (int jj = 0; jj < SP; ++jj) {
        if (jj < S) {
          const float wj = grp_get<SP>(w, base, jj);
          float av;
          if constexpr (AREG) av = arow[jj];
          else av = sA[jc * ld + jj];
          nb = nb + av * wj;
        }
      }
      if (!jS) nb = 0.f;
      const float m = grp_max<SP>(nb);
      const int e = bin_exp(m);
      if (step) {
        beta = ldexpf(nb, -e);
        bexp += e;
      }
      // gamma_t(j) = alpha_t(j) beta_t(j) / Z
      const u64 q = quant((at * beta) * rinv, ct + bexp - Etot + 32);
      if (v && jS && q) {
        if (LDSB) atomicAdd(&sE[j * O + ot], q);
        else atomicAdd(&a.emit[(long long)j * O + ot], q);
        if (t == 0) iacc += q;
      }
    }
  }

  // ---- flush: registers -> block tables (LDS) -> global, 64-bit integer atomics ----
  if (jS) {
#pragma unroll
    for (int i = 0; i < SP; ++i) {
      if (i < S && tacc[i]) atomicAdd(&sT[i * S + j], tacc[i]);
    }
    if (iacc) atomicAdd(&sI[j], iacc);
  }
  if (j == 0) {
    if (n_seq) atomicAdd(&sStat[0], (u64)n_seq);
    if (n_steps) atomicAdd(&sStat[1], n_steps);
    if (n_empty) atomicAdd(&sStat[2], (u64)n_empty);
    if (n_imp) atomicAdd(&sStat[3], (u64)n_imp);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < S * S; i += HT)
    if (sT[i]) atomicAdd(&a.trans[i], sT[i]);
  for (int i = threadIdx.x; i < S; i += HT)
    if (sI[i]) atomicAdd(&a.init[i], sI[i]);
  for (int i = threadIdx.x; i < 4; i += HT)
    if (sStat[i]) atomicAdd(&a.stats[i], sStat[i]);
  if (LDSB)
    for (int i = threadIdx.x; i < S * O; i += HT)
      if (sE[i]) atomicAdd(&a.emit[i], sE[i]);
}

size_t hmm_lds_bytes(int S, int O, bool ldsb) {
  const size_t so = ldsb ? (size_t)S * O : 0;
  return 8 * ((size_t)S * S + S + 4 + so) + 4 * ((size_t)S * (S | 1) + so);
}

template <int SP>
void launch_hmm(const HmmArgs& a, hipStream_t stream) {
  constexpr int G = 64 / SP;
  const bool ldsb = hmm_lds_bytes(a.S, a.O, true) <= HMM_LDSB_CAP;
  const size_t lds = hmm_lds_bytes(a.S, a.O, ldsb);
  if (lds > HMM_LDSB_CAP) throw std::runtime_error("hmm_estep: tables do not fit in LDS");
  const long long per_block = (long long)(HT / 64) * G;
  const long long need = (a.n + per_block - 1) / per_block;
  const unsigned grid = (unsigned)(need < HMM_MAX_BLOCKS ? need : HMM_MAX_BLOCKS);
  if (ldsb) hmm_estep_kernel<SP, true><<<grid, HT, lds, stream>>>(a);
  else hmm_estep_kernel<SP, false><<<grid, HT, lds, stream>>>(a);
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace

namespace avk {

void hmm_estep(const short* obs, long long n, int T, int S, int O, const float* A, const float* B,
               const float* pi, unsigned long long* trans, unsigned long long* emit, unsigned long long* init,
               float* Z, int* E, unsigned long long* stats, float* workspace, hipStream_t stream) {
  if (n <= 0 || T <= 0) return;
  if (S < 1 || S > 64) throw std::runtime_error("hmm_estep: 1 <= S <= 64");
  const HmmArgs a{obs, n, T, S, O, A, B, pi, trans, emit, init, stats, Z, E, workspace,
                  reinterpret_cast<int*>(workspace + n * (long long)T * S)};
  if (S <= 4) launch_hmm<4>(a, stream);
  else if (S <= 8) launch_hmm<8>(a, stream);
  else if (S <= 16) launch_hmm<16>(a, stream);
  else if (S <= 32) launch_hmm<32>(a, stream);
  else launch_hmm<64>(a, stream);
}

}  // namespace avk
