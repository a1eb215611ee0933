// K22: many simulated-annealing chains in one persistent launch (CDNA4, gfx950).
//
// Reference: one SA chain per Spark partition, mutating string-encoded solutions through the
// BasicSearchDomain SPI (S/optimize/SimulatedAnnealing.scala:111-187,
// J/optimize/BasicSearchDomain.java:272-394, cost J/examples/TaskScheduleSearch.java:169-305).
// Here an assignment-type domain (solution s[L] with s[i] in [0, V); total cost = mean_i C[i][s[i]];
// a solution is invalid when two positions with a conflict share a value) is compiled into a
// [L][V] cost table and an [L][L] conflict table, and every lane runs one chain for `iters`
// Metropolis steps: O(1) cost delta per move, O(L) validity check, Philox randomness, geometric or
// linear cooling — the whole optimisation is one kernel launch for thousands of chains.
#include <stdexcept>

#include "avenir_common.h"
#include "avenir_kernels.h"

namespace {

// true when position i conflicts with no other position holding the same value
__device__ __forceinline__ bool position_ok(const short* s, int L, int i, const uint8_t* __restrict__ conflict) {
  const short v = s[i * 64];
  const uint8_t* row = conflict + (long long)i * L;
  for (int j = 0; j < L; ++j)
    if (j != i && s[j * 64] == v && row[j]) return false;
  return true;
}

// One chain per lane, 64-lane workgroups (one wave): the chain's current solution lives in LDS as
// column `lane` of an [L][64] short tile (lane-private, conflict-free), the best solution is written
// to global memory only on improvement.  Move = reassign one position to a different value; with
// `swap` set, the position that already held the new value takes the old one (the reference's
// replaceSolutionComponent, J/examples/TaskScheduleSearch.java:140-166).
__global__ __launch_bounds__(64) void sa_assign_kernel(
    const float* __restrict__ cost, int L, int V, const uint8_t* __restrict__ conflict, int swap,
    short* __restrict__ sol, float* __restrict__ cur_cost, short* __restrict__ best_sol,
    float* __restrict__ best_cost, int P, int iters, float t0, float cool, int interval, int geometric,
    int max_retry, unsigned long long seed, unsigned long long offset, int it_begin, float temp_start,
    unsigned long long* __restrict__ stats, long long chain_base) {
  extern __shared__ short lds_sol[];
  const int lane = threadIdx.x;
  const int p = blockIdx.x * 64 + lane;
  const bool live = p < P;
  // Philox stream of GLOBAL chain chain_base + p: a chain draws the same moves whichever rank
  // (and launch) runs it, so chains can be re-dealt over a different world size on resume
  const unsigned long long gp = (unsigned long long)(chain_base + p);
  short* s = lds_sol + lane;  // element j at s[j * 64]
  if (live)
    for (int j = 0; j < L; ++j) s[j * 64] = sol[(long long)p * L + j];
  if (!live) return;
  short* bs = best_sol + (long long)p * L;
  float c = cur_cost[p];
  float bc = best_cost[p];
  // resumable: a run split into segments [it_begin, it_begin + iters) draws the same Philox counters
  // and follows the same cooling schedule as one uninterrupted launch
  float temp = temp_start;
  unsigned long long acc_better = 0, acc_worse = 0, rejected = 0;
  const float invL = 1.f / (float)L;
  for (int it = it_begin; it < it_begin + iters; ++it) {
    int pos = -1, nv = 0, old = 0, j2 = -1;
    for (int tr = 0; tr <= max_retry; ++tr) {
      const av::u4 r = av::philox_draw(seed, offset + (unsigned long long)it * (max_retry + 1) + tr, gp);
      const int cp = min((int)(av::u32_to_unit(r.x) * (float)L), L - 1);
      int cv = min((int)(av::u32_to_unit(r.y) * (float)(V - 1)), V - 2);
      const int ov = s[cp * 64];
      if (cv >= ov) ++cv;  // a different value
      int sw = -1;
      if (swap)
        for (int j = 0; j < L; ++j)
          if (j != cp && s[j * 64] == cv) { sw = j; break; }
      s[cp * 64] = (short)cv;
      if (sw >= 0) s[sw * 64] = (short)ov;
      const bool ok = !conflict || (position_ok(s, L, cp, conflict) && (sw < 0 || position_ok(s, L, sw, conflict)));
      if (ok) { pos = cp; nv = cv; old = ov; j2 = sw; break; }
      s[cp * 64] = (short)ov;
      if (sw >= 0) s[sw * 64] = (short)cv;
    }
    if (pos >= 0) {
      float delta = cost[(long long)pos * V + nv] - cost[(long long)pos * V + old];
      if (j2 >= 0) delta += cost[(long long)j2 * V + old] - cost[(long long)j2 * V + nv];
      delta *= invL;
      const av::u4 r2 = av::philox_draw(seed ^ 0x9e3779b97f4a7c15ull, offset + it, gp);
      const bool accept = delta <= 0.f || av::u32_to_unit(r2.x) < __expf(-delta / fmaxf(temp, 1e-12f));
      if (accept) {
        c += delta;
        if (delta <= 0.f) ++acc_better; else ++acc_worse;
        if (c < bc) {
          bc = c;
          for (int j = 0; j < L; ++j) bs[j] = s[j * 64];
        }
      } else {
        s[pos * 64] = (short)old;
        if (j2 >= 0) s[j2 * 64] = (short)nv;
        ++rejected;
      }
    }
    // cooling every `interval` moves: geometric, or linear T0 - it * rate (the Python optimiser's
    // form, P/mlextra/optsolo.py:84-88; the Scala linear branch subtracts T0 each time, a bug)
    if (interval > 0 && (it + 1) % interval == 0)
      temp = geometric ? temp * cool : fmaxf(t0 - (float)(it + 1) * cool, 1e-12f);
  }
  for (int j = 0; j < L; ++j) sol[(long long)p * L + j] = s[j * 64];
  cur_cost[p] = c;
  best_cost[p] = bc;
  if (stats) {
    if (p == 0) stats[3] = (unsigned long long)__float_as_uint(temp);  // segment hand-off temperature
    atomicAdd(&stats[0], acc_better);
    atomicAdd(&stats[1], acc_worse);
    atomicAdd(&stats[2], rejected);
  }
}

// ---- island genetic algorithm: one workgroup (one wave) per island, G generations per launch ----
// Reference: Spark GA — an independent GA per partition (S/optimize/GeneticAlgorithm.scala:70-163) —
// and the Python GeneticAlgorithmOptimizer (P/mlextra/optpopu.py:98-187: pool, mating list,
// replacement, purge).  An island's pool [P][L], its costs and the children of a generation live in
// LDS; per generation, one lane per member / pair / child:
//   1. rank the pool by (cost, index) (lane j counts the members ahead of member j) -> ord[];
//      hist[g] = the best cost at the generation's start;
//   2. pair k < r draws Philox(seed, 256 (gen_base + g) + k, island): parents ord[a], ord[b] (a != b) from the
//      m best, crossover point x in [1, L), children a[:x] b[x:] and b[:x] a[x:]; with `mutate`,
//      Philox(seed ^ M, 16 ctr + try, island) moves one position of each child to a different
//      value (a swap move with `swap`), retried until the child is valid (<= 10 tries);
//   3. lane c < 2r prices child c: fp32 sum of C[l][s_l] in position order times 1/L, or
//      `invalid` when two conflicting positions share a value;
//   4. the best r children by (cost, index) replace the worst r members (purge_first) or join the
//      pool, whose best P by (cost, index; members before children) survive — written to the other
//      pool buffer in rank order.
// The island's stream is keyed by its GLOBAL index (island_base + blockIdx.x), so any world size
// yields the same islands; optimize/ga.py::ga_assign_reference is the bit-exact host twin.
constexpr int GA_MAX_TRY = 10;

__device__ __forceinline__ bool ga_valid(const short* s, int L, const uint8_t* __restrict__ conflict) {
  if (conflict)
    for (int i = 0; i < L; ++i)
      for (int j = i + 1; j < L; ++j)
        if (s[i] == s[j] && conflict[(long long)i * L + j]) return false;
  return true;
}

__device__ __forceinline__ float ga_price(const short* s, int L, int V, const float* __restrict__ cost,
                                          const uint8_t* __restrict__ conflict, float invL, float invalid) {
  float acc = 0.f;
  for (int l = 0; l < L; ++l) acc += cost[(long long)l * V + s[l]];
  return ga_valid(s, L, conflict) ? acc * invL : invalid;
}

// lane j < n counts the elements ahead of element j by (cost, index) and writes ord[rank] = j
__device__ __forceinline__ void ga_rank(const float* c, int n, int lane, int* ord) {
  if (lane < n) {
    const float cl = c[lane];
    int rk = 0;
    for (int j = 0; j < n; ++j) rk += (c[j] < cl) || (c[j] == cl && j < lane);
    ord[rk] = lane;
  }
}

// Step 4 of a generation (both island kernels; every lane of the workgroup calls it): the source
// of every next-pool slot -> nsrc, then the next pool pb / pc2 gathered from pa / kid.
__device__ __forceinline__ void ga_replace(const short* pa, short* pb, const short* kid, const float* pc, float* pc2,
                                           const float* kc, const int* ord, const int* kord, int* nsrc, int P, int L,
                                           int r, int purge_first, int lane) {
  if (purge_first) {
    if (lane < P) nsrc[lane] = lane < P - r ? ord[lane] : P + kord[lane - (P - r)];
  } else if (lane < P + r) {
    // candidate lane: member ord-independent index (lane < P) or child kord[lane - P]; its rank
    // among all candidates by (cost, candidate index)
    const int src = lane < P ? lane : P + kord[lane - P];
    const float c = lane < P ? pc[lane] : kc[src - P];
    int rk = 0;
    for (int j = 0; j < P + r; ++j) {
      const int sj = j < P ? j : P + kord[j - P];
      const float cj = j < P ? pc[j] : kc[sj - P];
      rk += (cj < c) || (cj == c && j < lane);
    }
    if (rk < P) nsrc[rk] = src;
  }
  __syncthreads();
  for (int e = lane; e < P * L; e += 64) {
    const int slot = e / L, l = e - slot * L;
    const int src = nsrc[slot];
    pb[e] = src < P ? pa[(size_t)src * L + l] : kid[(size_t)(src - P) * L + l];
  }
  if (lane < P) {
    const int src = nsrc[lane];
    pc2[lane] = src < P ? pc[src] : kc[src - P];
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void ga_assign_kernel(
    const float* __restrict__ cost, int L, int V, const uint8_t* __restrict__ conflict, float invalid,
    short* __restrict__ pop, float* __restrict__ pop_cost, float* __restrict__ hist, int P, int G, int m, int r,
    int purge_first, int mutate, int swap, unsigned long long seed, long long island_base, int gen_base) {
  extern __shared__ unsigned char ga_lds[];
  short* pa = reinterpret_cast<short*>(ga_lds);   // [P][L] current pool
  short* pb = pa + (size_t)P * L;                 // [P][L] next pool
  short* kid = pb + (size_t)P * L;                // [2r][L] children
  float* pc = reinterpret_cast<float*>(kid + (size_t)2 * r * L);  // [P] pool costs
  float* pc2 = pc + P;                            // [P] next pool costs
  float* kc = pc2 + P;                            // [2r] child costs
  int* ord = reinterpret_cast<int*>(kc + 2 * r);  // [P] pool order
  int* kord = ord + P;                            // [2r] child order
  int* nsrc = kord + 2 * r;                       // [P] source of next pool slot (>= P: child)
  const int lane = threadIdx.x;
  const long long isl = blockIdx.x;
  const unsigned long long gi = (unsigned long long)(island_base + isl);
  const float invL = 1.f / (float)L;
  short* gpop = pop + isl * P * L;
  for (int e = lane; e < P * L; e += 64) pa[e] = gpop[e];
  if (lane < P) pc[lane] = pop_cost[isl * P + lane];
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    // 1. rank
    ga_rank(pc, P, lane, ord);
    __syncthreads();
    if (lane == 0) hist[isl * G + g] = pc[ord[0]];
    // 2. children
    if (lane < r) {
      const unsigned long long ctr = 256ull * (unsigned long long)(gen_base + g) + lane;
      const av::u4 R = av::philox_draw(seed, ctr, gi);
      const int a = min((int)(av::u32_to_unit(R.x) * (float)m), m - 1);
      int b = 0;
      if (m > 1) {
        b = min((int)(av::u32_to_unit(R.y) * (float)(m - 1)), m - 2);
        b += b >= a;
      }
      const int x = L > 1 ? 1 + min((int)(av::u32_to_unit(R.z) * (float)(L - 1)), L - 2) : 0;
      const short* A = pa + (size_t)ord[a] * L;
      const short* B = pa + (size_t)ord[b] * L;
      short* c1 = kid + (size_t)(2 * lane) * L;
      short* c2 = c1 + L;
      for (int l = 0; l < L; ++l) {
        c1[l] = l < x ? A[l] : B[l];
        c2[l] = l < x ? B[l] : A[l];
      }
      if (mutate) {
        // one position to a different value (with `swap`, the first other position holding that
        // value takes the old one: the domain's swap move), redrawn up to GA_MAX_TRY times until
        // the child is valid; the last attempt stays otherwise (BasicSearchDomain.mutateSolution)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          short* c = h == 0 ? c1 : c2;
          for (int t = 0; t < GA_MAX_TRY; ++t) {
            const av::u4 Q = av::philox_draw(seed ^ 0xD1B54A32D192ED03ull, ctr * 16ull + t, gi);
            const unsigned qp = h == 0 ? Q.x : Q.z, qv = h == 0 ? Q.y : Q.w;
            const int pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
            const int old = c[pos];
            int v = min((int)(av::u32_to_unit(qv) * (float)(V - 1)), V - 2);
            v += v >= old;
            int holder = -1;
            if (swap)
              for (int j = 0; j < L; ++j)
                if (j != pos && c[j] == v) { holder = j; break; }
            if (holder >= 0) c[holder] = (short)old;
            c[pos] = (short)v;
            if (t == GA_MAX_TRY - 1 || ga_valid(c, L, conflict)) break;
            c[pos] = (short)old;
            if (holder >= 0) c[holder] = (short)v;
          }
        }
      }
    }
    __syncthreads();
    // 3. price the children
    if (lane < 2 * r) kc[lane] = ga_price(kid + (size_t)lane * L, L, V, cost, conflict, invL, invalid);
    __syncthreads();
    ga_rank(kc, 2 * r, lane, kord);
    __syncthreads();
    // 4. replacement
    ga_replace(pa, pb, kid, pc, pc2, kc, ord, kord, nsrc, P, L, r, purge_first, lane);
    short* t = pa; pa = pb; pb = t;
    float* tc = pc; pc = pc2; pc2 = tc;
  }
  for (int e = lane; e < P * L; e += 64) gpop[e] = pa[e];
  if (lane < P) pop_cost[isl * P + lane] = pc[lane];
}

// ---- island GA over a meeting-schedule domain (P/app/mesched.py, optimize/domains.py) ----------
// The frame of ga_assign_kernel (one wave per island, pools / children / costs in LDS for all G
// generations, Philox by global island index) with the domain's own validity and cost:
//   * a solution is (day, hour, minute) index triples of M meetings, L = 3 M; meeting i starts at
//     (days[d] - 1) 86400 + hours[h] 3600 + minutes[mi] 60 s and lasts dur[i] s;
//   * invalid: two meetings with a common participant overlap, a meeting of a blocked person
//     overlaps the blocked interval, or an ordered pair (a, b) has end[a] > start[b] — integers only;
//   * cost: per person q, over the days with a meeting, free = sum(36000 - booked) and
//     nslots = sum(cnt + 1).  With ndays = the number of distinct days of q's meetings these are
//     36000 ndays - (total duration of q's meetings) and (meetings of q) + ndays, so no per-day
//     counters are kept: one OR of day bits per person.  pc = 8 - (free / nslots) / 3600,
//     cost = sum(pc w) / sum(w) in fp32 with q ascending, multiply and add rounded separately;
//   * lane c < 2r builds, mutates and prices child c of pair c >> 1 — both lanes of a pair draw the
//     same Philox word, the crossover cut falls between meetings, mutation moves one index to a
//     different value of its table (tables of one value are left alone).
// Each child lane keeps the start second and the day bit of every meeting of its child in two
// lane-private LDS rows (odd stride: conflict-free), so no private array is indexed dynamically.
// optimize/ga_meeting.py::ga_meeting_reference is the bit-exact host twin.
constexpr int MT_MAX_M = 32, MT_MAX_Q = 256, MT_MAX_CARD = 32, MT_MAX_LIST = 16;
constexpr int MT_DOM_INTS = 3 * MT_MAX_CARD + 2 * MT_MAX_M + 2 * MT_MAX_Q + 5 * MT_MAX_LIST;  // staged domain

__host__ __device__ constexpr size_t mt_a16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

struct MtLds {  // the staged domain
  const int *days, *hours, *minutes, *dur, *blocked, *ordered;
  const unsigned *share, *member;
  const float* role_w;
  int M, Q, nb, no;
};

// start second and day bit of meeting i of solution c
__device__ __forceinline__ void mt_place(const MtLds& D, const short* c, int i, int* st, unsigned* db) {
  const int d = c[3 * i];
  st[i] = (D.days[d] - 1) * 86400 + D.hours[c[3 * i + 1]] * 3600 + D.minutes[c[3 * i + 2]] * 60;
  db[i] = 1u << d;
}

__device__ __forceinline__ bool mt_valid(const MtLds& D, const int* st) {
  bool ok = true;
  for (int i = 1; i < D.M; ++i) {
    unsigned mk = D.share[i] & ((1u << i) - 1u);  // share is symmetric: pairs j < i
    const int si = st[i], ei = si + D.dur[i];
    while (mk) {
      const int j = __ffs(mk) - 1;
      mk &= mk - 1;
      const int sj = st[j];
      ok &= !(si < sj + D.dur[j] && sj < ei);
    }
  }
  for (int b = 0; b < D.nb; ++b) {
    unsigned mk = (unsigned)D.blocked[3 * b];
    const int bs = D.blocked[3 * b + 1], be = D.blocked[3 * b + 2];
    while (mk) {
      const int i = __ffs(mk) - 1;
      mk &= mk - 1;
      const int si = st[i];
      ok &= !(si < be && bs < si + D.dur[i]);
    }
  }
  for (int o = 0; o < D.no; ++o) {
    const int a = D.ordered[2 * o], b = D.ordered[2 * o + 1];
    ok &= st[a] + D.dur[a] <= st[b];
  }
  return ok;
}

__device__ __forceinline__ float mt_cost(const MtLds& D, const unsigned* db) {
#pragma clang fp contract(off)  // the twin rounds pc * w and the add separately
  float num = 0.f, den = 0.f;
  for (int q = 0; q < D.Q; ++q) {
    unsigned mk = D.member[q];
    if (!mk) continue;
    const int nmeet = __popc(mk);
    unsigned dm = 0;
    int booked = 0;
    while (mk) {
      const int i = __ffs(mk) - 1;
      mk &= mk - 1;
      dm |= db[i];
      booked += D.dur[i];
    }
    const int nday = __popc(dm);
    const int free_q = 36000 * nday - booked, nslots = nmeet + nday;
    const float pc = 8.f - ((float)free_q / (float)nslots) / 3600.f;
    const float w = D.role_w[q];
    const float pw = pc * w;
    num = num + pw;
    den = den + w;
  }
  return num / fmaxf(den, 1e-12f);
}

__global__ __launch_bounds__(64) void ga_meeting_kernel(
    avk::GaMeetingDomain dom, float invalid, short* __restrict__ pop, float* __restrict__ pop_cost,
    float* __restrict__ hist, int P, int G, int m, int r, int purge_first, int mutate, unsigned long long seed,
    long long island_base, unsigned long long gen_base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_lds[];
  const int M = dom.M, L = 3 * M, Ms = M | 1;  // Ms: odd stride of the lane-private rows
  unsigned char* cur = gm_lds;
  short* pa = reinterpret_cast<short*>(cur);  cur += mt_a16((size_t)P * L * sizeof(short));      // [P][L] pool
  short* pb = reinterpret_cast<short*>(cur);  cur += mt_a16((size_t)P * L * sizeof(short));      // [P][L] next pool
  short* kid = reinterpret_cast<short*>(cur); cur += mt_a16((size_t)2 * r * L * sizeof(short));  // [2r][L] children
  float* pc = reinterpret_cast<float*>(cur);  cur += mt_a16((size_t)P * sizeof(float));
  float* pc2 = reinterpret_cast<float*>(cur); cur += mt_a16((size_t)P * sizeof(float));
  float* kc = reinterpret_cast<float*>(cur);  cur += mt_a16((size_t)2 * r * sizeof(float));
  int* ord = reinterpret_cast<int*>(cur);     cur += mt_a16((size_t)P * sizeof(int));
  int* kord = reinterpret_cast<int*>(cur);    cur += mt_a16((size_t)2 * r * sizeof(int));
  int* nsrc = reinterpret_cast<int*>(cur);    cur += mt_a16((size_t)P * sizeof(int));
  int* st_all = reinterpret_cast<int*>(cur);  cur += mt_a16((size_t)2 * r * Ms * sizeof(int));   // [2r][Ms] starts
  unsigned* db_all = reinterpret_cast<unsigned*>(cur); cur += mt_a16((size_t)2 * r * Ms * sizeof(int));  // day bits
  int* di = reinterpret_cast<int*>(cur);      // the domain, MT_DOM_INTS dwords
  int* l_days = di;
  int* l_hours = l_days + MT_MAX_CARD;
  int* l_minutes = l_hours + MT_MAX_CARD;
  int* l_dur = l_minutes + MT_MAX_CARD;
  unsigned* l_share = reinterpret_cast<unsigned*>(l_dur + MT_MAX_M);
  unsigned* l_member = l_share + MT_MAX_M;
  float* l_role = reinterpret_cast<float*>(l_member + MT_MAX_Q);
  int* l_blocked = reinterpret_cast<int*>(l_role + MT_MAX_Q);
  int* l_ordered = l_blocked + 3 * MT_MAX_LIST;

  const int lane = threadIdx.x;
  const long long isl = blockIdx.x;
  const unsigned long long gi = (unsigned long long)(island_base + isl);
  if (lane < dom.nd) l_days[lane] = dom.days[lane];
  if (lane < dom.nh) l_hours[lane] = dom.hours[lane];
  if (lane < dom.nm) l_minutes[lane] = dom.minutes[lane];
  if (lane < M) {
    l_dur[lane] = dom.dur[lane];
    l_share[lane] = dom.share[lane];
  }
  for (int q = lane; q < dom.Q; q += 64) {
    l_member[q] = dom.member[q];
    l_role[q] = dom.role_w[q];
  }
  if (lane < 3 * dom.nb) l_blocked[lane] = dom.blocked[lane];
  if (lane < 2 * dom.no) l_ordered[lane] = dom.ordered[lane];
  const MtLds D{l_days, l_hours, l_minutes, l_dur, l_blocked, l_ordered, l_share, l_member, l_role,
                M, dom.Q, dom.nb, dom.no};
  short* gpop = pop + isl * P * L;
  for (int e = lane; e < P * L; e += 64) pa[e] = gpop[e];
  if (lane < P) pc[lane] = pop_cost[isl * P + lane];
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    // 1. rank
    ga_rank(pc, P, lane, ord);
    __syncthreads();
    if (lane == 0) hist[isl * G + g] = pc[ord[0]];
    // 2 + 3. lane c: child c of pair c >> 1, built, mutated and priced
    if (lane < 2 * r) {
      const int h = lane & 1;
      const unsigned long long ctr = 256ull * (gen_base + (unsigned long long)g) + (unsigned long long)(lane >> 1);
      const av::u4 R = av::philox_draw(seed, ctr, gi);
      const int a = min((int)(av::u32_to_unit(R.x) * (float)m), m - 1);
      int b = 0;
      if (m > 1) {
        b = min((int)(av::u32_to_unit(R.y) * (float)(m - 1)), m - 2);
        b += b >= a;
      }
      const int cut = M > 1 ? 3 * (1 + min((int)(av::u32_to_unit(R.z) * (float)(M - 1)), M - 2)) : 0;
      const short* A = pa + (size_t)ord[h ? b : a] * L;  // head of this child
      const short* B = pa + (size_t)ord[h ? a : b] * L;  // tail
      short* c = kid + (size_t)lane * L;
      int* st = st_all + lane * Ms;
      unsigned* db = db_all + lane * Ms;
      for (int l = 0; l < L; ++l) c[l] = l < cut ? A[l] : B[l];
      for (int i = 0; i < M; ++i) mt_place(D, c, i, st, db);
      bool ok;
      if (mutate) {
        // one index to a different value of its table, redrawn up to GA_MAX_TRY times until the
        // child is valid; the last attempt stays otherwise
        for (int t = 0;; ++t) {
          const av::u4 Q = av::philox_draw(seed ^ 0xD1B54A32D192ED03ull, ctr * 16ull + (unsigned long long)t, gi);
          const unsigned qp = h == 0 ? Q.x : Q.z, qv = h == 0 ? Q.y : Q.w;
          const int pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
          const int mi = pos / 3, comp = pos - 3 * mi;
          const int card = comp == 0 ? dom.nd : comp == 1 ? dom.nh : dom.nm;
          const int old = c[pos];
          if (card > 1) {
            int v = min((int)(av::u32_to_unit(qv) * (float)(card - 1)), card - 2);
            v += v >= old;
            c[pos] = (short)v;
            mt_place(D, c, mi, st, db);
          }
          ok = mt_valid(D, st);
          if (ok || t == GA_MAX_TRY - 1) break;
          if (card > 1) {
            c[pos] = (short)old;
            mt_place(D, c, mi, st, db);
          }
        }
      } else {
        ok = mt_valid(D, st);
      }
      kc[lane] = ok ? mt_cost(D, db) : invalid;
    }
    __syncthreads();
    ga_rank(kc, 2 * r, lane, kord);
    __syncthreads();
    // 4. replacement
    ga_replace(pa, pb, kid, pc, pc2, kc, ord, kord, nsrc, P, L, r, purge_first, lane);
    short* t = pa; pa = pb; pb = t;
    float* tc = pc; pc = pc2; pc2 = tc;
  }
  for (int e = lane; e < P * L; e += 64) gpop[e] = pa[e];
  if (lane < P) pop_cost[isl * P + lane] = pc[lane];
}

}  // namespace

namespace avk {

size_t ga_assign_lds(int P, int L, int r) {
  return (size_t)(2 * P + 2 * r) * L * sizeof(short) + (size_t)(2 * P + 2 * r) * sizeof(float) +
         (size_t)(2 * P + 2 * r) * sizeof(int);
}

void ga_assign(const float* cost, int L, int V, const uint8_t* conflict, float invalid, short* pop, float* pop_cost,
               float* hist, int islands, int P, int G, int m, int r, int purge_first, int mutate, int swap,
               unsigned long long seed, long long island_base, int gen_base, hipStream_t stream) {
  if (islands <= 0 || G <= 0) return;
  if (P < 2 || P > 64 || r < 1 || 2 * r > 64 || r > P || m < 1 || m > P || L < 1 || V < 2)
    throw std::invalid_argument("ga_assign: 2 <= P <= 64, 1 <= r <= min(P, 32), 1 <= m <= P, L >= 1, V >= 2");
  if (!purge_first && P + r > 64) throw std::invalid_argument("ga_assign: P + r <= 64 when children join the pool");
  const size_t lds = ga_assign_lds(P, L, r);
  if (lds > 64 * 1024) throw std::invalid_argument("ga_assign: pool, children and costs exceed 64 KiB of LDS");
  ga_assign_kernel<<<islands, 64, lds, stream>>>(cost, L, V, conflict, invalid, pop, pop_cost, hist, P, G, m, r,
                                                 purge_first, mutate, swap, seed, island_base, gen_base);
  AV_HIP_CHECK(hipGetLastError());
}

size_t ga_meeting_lds(int P, int L, int r) {
  const size_t Ms = (size_t)(L / 3) | 1;
  return 2 * mt_a16((size_t)P * L * sizeof(short)) + mt_a16((size_t)2 * r * L * sizeof(short)) +
         4 * mt_a16((size_t)P * 4) + 2 * mt_a16((size_t)2 * r * 4) +  // pc, pc2, ord, nsrc; kc, kord
         2 * mt_a16((size_t)2 * r * Ms * sizeof(int)) + mt_a16((size_t)MT_DOM_INTS * sizeof(int));
}

void ga_meeting(const GaMeetingDomain& dom, float invalid, short* pop, float* pop_cost, float* hist, int islands,
                int P, int G, int m, int r, int purge_first, int mutate, unsigned long long seed,
                long long island_base, unsigned long long gen_base, hipStream_t stream) {
  if (dom.M < 1 || dom.M > MT_MAX_M || dom.Q < 1 || dom.Q > MT_MAX_Q)
    throw std::invalid_argument("ga_meeting: 1 <= M <= 32, 1 <= Q <= 256");
  if (dom.nd < 1 || dom.nd > MT_MAX_CARD || dom.nh < 1 || dom.nh > MT_MAX_CARD || dom.nm < 1 || dom.nm > MT_MAX_CARD)
    throw std::invalid_argument("ga_meeting: value tables of 1..32 entries");
  if (dom.nb < 0 || dom.nb > MT_MAX_LIST || dom.no < 0 || dom.no > MT_MAX_LIST)
    throw std::invalid_argument("ga_meeting: at most 16 blocked entries and 16 ordered pairs");
  if (P < 2 || P > 64 || r < 1 || 2 * r > 64 || r > P || m < 1 || m > P)
    throw std::invalid_argument("ga_meeting: 2 <= P <= 64, 1 <= r <= min(P, 32), 1 <= m <= P");
  if (!purge_first && P + r > 64) throw std::invalid_argument("ga_meeting: P + r <= 64 when children join the pool");
  const size_t lds = ga_meeting_lds(P, 3 * dom.M, r);
  if (lds > 64 * 1024) throw std::invalid_argument("ga_meeting: pool, children and costs exceed 64 KiB of LDS");
  if (islands <= 0 || G <= 0) return;
  ga_meeting_kernel<<<islands, 64, lds, stream>>>(dom, invalid, pop, pop_cost, hist, P, G, m, r, purge_first, mutate,
                                                  seed, island_base, gen_base);
  AV_HIP_CHECK(hipGetLastError());
}

void sa_assign(const float* cost, int L, int V, const uint8_t* conflict, int swap, short* sol, float* cur_cost,
               short* best_sol, float* best_cost, int P, int iters, float t0, float cool, int interval,
               int geometric, int max_retry, unsigned long long seed, unsigned long long offset,
               int it_begin, float temp_start, unsigned long long* stats, long long chain_base, hipStream_t stream) {
  if (P <= 0 || iters <= 0) return;
  const size_t lds = (size_t)L * 64 * sizeof(short);
  sa_assign_kernel<<<(P + 63) / 64, 64, lds, stream>>>(cost, L, V, conflict, swap, sol, cur_cost, best_sol,
                                                       best_cost, P, iters, t0, cool, interval, geometric, max_retry,
                                                       seed, offset, it_begin, temp_start, stats, chain_base);
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace avk
