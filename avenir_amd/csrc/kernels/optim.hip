// K22: stochastic search in persistent launches (CDNA4, gfx950) — island genetic algorithms and
// simulated-annealing chains over three domains each: assignments (a [L][V] cost table and an
// [L][L] conflict table), meeting schedules and feature subsets scored by naive Bayes; tabu
// search over assignments (tabu_assign_kernel, one chain per wave); and the evolutionary optimiser's
// steady-state islands over the same three domains (eo_*_kernel on the frame eo_island, at the end).
//
// Reference: one SA chain or one GA per Spark partition, mutating string-encoded solutions through
// the BasicSearchDomain SPI (S/optimize/SimulatedAnnealing.scala:111-187,
// S/optimize/GeneticAlgorithm.scala:70-163, J/optimize/BasicSearchDomain.java:272-394, cost
// J/examples/TaskScheduleSearch.java:169-305).  Here a whole optimisation is one launch: an island
// is a workgroup (ga_assign_kernel, ga_meeting_kernel, ga_subset_kernel on one frame, ga_island),
// and an SA chain is a lane (sa_assign_kernel, sa_meeting_kernel) or 1 to 16 waves
// (sa_subset_kernel), thousands of chains per launch, all launched from one run record (SaRun).
#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "avenir_common.h"
#include "avenir_kernels.h"

namespace {

// ---- island genetic algorithm: one workgroup per island, G generations per launch ---------------
// Reference: Spark GA — an independent GA per partition (S/optimize/GeneticAlgorithm.scala:70-163) —
// and the Python GeneticAlgorithmOptimizer (P/mlextra/optpopu.py:98-187: pool, mating list,
// replacement, purge).  An island's pool of P solutions, its costs and the 2r children of a
// generation live in LDS for all G generations; per generation, one lane per member / child:
//   1. rank the pool by (cost, index) (lane j counts the members ahead of member j) -> ord[];
//      hist[g] = the best cost at the generation's start;
//   2. lane c < 2r breeds child c of pair k = c >> 1.  Both lanes of a pair draw
//      Philox(seed, 256 (gen_base + g) + k, island): parents ord[a], ord[b] (a != b) from the m best
//      and a crossover cut; child 2k is a's head with b's tail, child 2k + 1 b's head with a's tail.
//      With `mutate`, attempt t of the pair draws Philox(seed ^ MUT, 16 ctr + t, island): words
//      (x, y) give position and value for child 2k, (z, w) for child 2k + 1, so the two children
//      are mutated independently; an attempt that leaves the child invalid is taken back and
//      redrawn, the last of GA_MAX_TRY attempts stays (BasicSearchDomain.mutateSolution);
//   3. the child is priced (`invalid` for an invalid one) -> kc[c], and the children are ranked;
//   4. the best r children by (cost, index) replace the worst r members (purge_first) or join the
//      pool, whose best P by (cost, index; members before children) survive — written to the other
//      pool buffer in rank order.
// The island's stream is keyed by its GLOBAL index (island_base + blockIdx.x), so any world size
// yields the same islands.  What a solution is, when it is valid and what it costs is the domain's:
// each kernel below supplies steps 2 and 3 as its `breed` callable.  optimize/ga.py::
// ga_islands_reference is the frame's bit-exact host twin.
constexpr int GA_MAX_TRY = 10;
constexpr unsigned long long GA_MUT_KEY = 0xD1B54A32D192ED03ull;

struct GaArgs {
  int P, G, m, r, purge_first, mutate;
  unsigned long long seed;
  long long island_base;
  unsigned long long gen_base;
};

__host__ __device__ constexpr size_t ga_a16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// An island's working set in LDS.  A solution is L elements of T (L shorts, or one 32-bit mask).
template <class T>
struct GaPool {
  T *pa, *pb, *kid;      // [P][L] current pool, [P][L] next pool, [2r][L] children
  float *pc, *pc2, *kc;  // [P] pool costs, [P] next pool costs, [2r] child costs
  int *ord, *kord;       // [P] pool order, [2r] child order
  int* nsrc;             // [P] source of next pool slot (>= P: child)

  // every array 16-aligned from a 16-aligned base; returns the first byte past the view
  __device__ __forceinline__ unsigned char* carve(unsigned char* cur, int P, int L, int r) {
    pa = reinterpret_cast<T*>(cur);       cur += ga_a16((size_t)P * L * sizeof(T));
    pb = reinterpret_cast<T*>(cur);       cur += ga_a16((size_t)P * L * sizeof(T));
    kid = reinterpret_cast<T*>(cur);      cur += ga_a16((size_t)2 * r * L * sizeof(T));
    pc = reinterpret_cast<float*>(cur);   cur += ga_a16((size_t)P * sizeof(float));
    pc2 = reinterpret_cast<float*>(cur);  cur += ga_a16((size_t)P * sizeof(float));
    kc = reinterpret_cast<float*>(cur);   cur += ga_a16((size_t)2 * r * sizeof(float));
    ord = reinterpret_cast<int*>(cur);    cur += ga_a16((size_t)P * sizeof(int));
    kord = reinterpret_cast<int*>(cur);   cur += ga_a16((size_t)2 * r * sizeof(int));
    nsrc = reinterpret_cast<int*>(cur);   cur += ga_a16((size_t)P * sizeof(int));
    return cur;
  }
  __host__ __device__ static constexpr size_t bytes(int P, int L, int r) {
    return 2 * ga_a16((size_t)P * L * sizeof(T)) + ga_a16((size_t)2 * r * L * sizeof(T)) +
           4 * ga_a16((size_t)P * 4) + 2 * ga_a16((size_t)2 * r * 4);  // pc, pc2, ord, nsrc; kc, kord
  }
};

// lane j < n counts the elements ahead of element j by (cost, index) and writes ord[rank] = j
__device__ __forceinline__ void ga_rank(const float* c, int n, int lane, int* ord) {
  if (lane < n) {
    const float cl = c[lane];
    int rk = 0;
    for (int j = 0; j < n; ++j) rk += (c[j] < cl) || (c[j] == cl && j < lane);
    ord[rk] = lane;
  }
}

// Step 4 of a generation (every thread of the workgroup calls it, `nt` of them): the source of
// every next-pool slot -> nsrc, then the next pool pb / pc2 gathered from pa / kid.
template <class T>
__device__ __forceinline__ void ga_replace(const T* pa, T* pb, const T* kid, const float* pc, float* pc2,
                                           const float* kc, const int* ord, const int* kord, int* nsrc, int P, int L,
                                           int r, int purge_first, int lane, int nt) {
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
  for (int e = lane; e < P * L; e += nt) {
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

// Step 2's parent draw of the pair with counter ctr: a, b (ranks among the m best, a != b unless
// m = 1) and the unit cut x in [1, ncut) (0 at ncut = 1), which the domain scales to its positions.
struct GaPair {
  int a, b, x;
};

__device__ __forceinline__ GaPair ga_draw_pair(unsigned long long seed, unsigned long long ctr, unsigned long long gi,
                                               int m, int ncut) {
  const av::u4 R = av::philox_draw(seed, ctr, gi);
  GaPair p;
  p.a = min((int)(av::u32_to_unit(R.x) * (float)m), m - 1);
  p.b = 0;
  if (m > 1) {
    p.b = min((int)(av::u32_to_unit(R.y) * (float)(m - 1)), m - 2);
    p.b += p.b >= p.a;
  }
  p.x = ncut > 1 ? 1 + min((int)(av::u32_to_unit(R.z) * (float)(ncut - 1)), ncut - 2) : 0;
  return p;
}

// Step 2's mutation of child h (0 / 1) of the pair with counter ctr.  The domain supplies
// apply(position word, value word): one attempt; valid(): is the child valid now; undo(): take the
// attempt back.  Returns the child's validity (without `mutate`: of the child as crossed).
template <class Apply, class Valid, class Undo>
__device__ __forceinline__ bool ga_mutate(const GaArgs& A, unsigned long long ctr, unsigned long long gi, int h,
                                          Apply apply, Valid valid, Undo undo) {
  if (!A.mutate) return valid();
  for (int t = 0;; ++t) {
    const av::u4 Q = av::philox_draw(A.seed ^ GA_MUT_KEY, ctr * 16ull + (unsigned long long)t, gi);
    apply(h ? Q.z : Q.x, h ? Q.w : Q.y);
    const bool ok = valid();
    if (ok || t == GA_MAX_TRY - 1) return ok;
    undo();
  }
}

// pop [islands][P][L] int16 <-> the island's pool: L shorts per member, or the 0 / 1 row as one mask
__device__ __forceinline__ void ga_load(short* pa, const short* gpop, int P, int L, int tid, int nt) {
  for (int e = tid; e < P * L; e += nt) pa[e] = gpop[e];
}
__device__ __forceinline__ void ga_load(unsigned* pa, const short* gpop, int P, int L, int tid, int nt) {
  if (tid < P) {
    unsigned mk = 0;
    for (int f = 0; f < L; ++f) mk |= (unsigned)(gpop[tid * L + f] != 0) << f;
    pa[tid] = mk;
  }
}
__device__ __forceinline__ void ga_store(short* gpop, const short* pa, int P, int L, int tid, int nt) {
  for (int e = tid; e < P * L; e += nt) gpop[e] = pa[e];
}
__device__ __forceinline__ void ga_store(short* gpop, const unsigned* pa, int P, int L, int tid, int nt) {
  for (int e = tid; e < P * L; e += nt) {
    const int p = e / L;
    gpop[e] = (short)((pa[p] >> (e - p * L)) & 1u);
  }
}

// The island of this workgroup (every thread calls it, `nt` of them; P, 2r and P + r <= 64 <= nt):
// pool in, G generations, pool out.  breed(ctr0) is steps 2 and 3 of a generation whose pair k has
// the counter ctr0 + k: called by every thread, it leaves the children in V.kid and their costs in
// V.kc and may hold barriers of its own; the frame's barrier follows it.  The barrier after the
// load also covers whatever the kernel staged in LDS before the call.
template <class T, class Breed>
__device__ __forceinline__ void ga_island(GaPool<T>& V, const GaArgs& A, int L, short* __restrict__ pop,
                                          float* __restrict__ pop_cost, float* __restrict__ hist, int tid, int nt,
                                          Breed breed) {
  const long long isl = blockIdx.x;
  const int P = A.P, E = sizeof(T) == sizeof(short) ? L : 1;  // elements of T per solution
  short* gpop = pop + isl * P * L;
  float* ghist = hist + isl * A.G;
  ga_load(V.pa, gpop, P, L, tid, nt);
  if (tid < P) V.pc[tid] = pop_cost[isl * P + tid];
  __syncthreads();
  for (int g = 0; g < A.G; ++g) {
    // 1. rank
    ga_rank(V.pc, P, tid, V.ord);
    __syncthreads();
    if (tid == 0) ghist[g] = V.pc[V.ord[0]];
    // 2 + 3. children and their costs
    breed(256ull * (A.gen_base + (unsigned long long)g));
    __syncthreads();
    ga_rank(V.kc, 2 * A.r, tid, V.kord);
    __syncthreads();
    // 4. replacement
    ga_replace(V.pa, V.pb, V.kid, V.pc, V.pc2, V.kc, V.ord, V.kord, V.nsrc, P, E, A.r, A.purge_first, tid, nt);
    T* t = V.pa; V.pa = V.pb; V.pb = t;
    float* tc = V.pc; V.pc = V.pc2; V.pc2 = tc;
  }
  ga_store(gpop, V.pa, P, L, tid, nt);
  if (tid < P) pop_cost[isl * P + tid] = V.pc[tid];
}

// ---- island GA over an assignment domain (one wave per island) ---------------------------------
// The frame above with:
//   * a solution is L values in [0, V); the crossover cut x lies in [1, L);
//   * mutation moves one position to a different value (with `swap`, the first other position
//     holding that value takes the old one: the domain's swap move);
//   * invalid: two conflicting positions share a value;
//   * cost: fp32 sum of C[l][s_l] in position order times 1/L.
// optimize/ga.py::ga_assign_reference is the bit-exact host twin.
// S is the element stride of s: 1 for rows, IW for the lane-private columns of the evolutionary kernels.
template <int S = 1>
__device__ __forceinline__ bool ga_valid(const short* s, int L, const uint8_t* __restrict__ conflict) {
  if (conflict)
    for (int i = 0; i < L; ++i)
      for (int j = i + 1; j < L; ++j)
        if (s[i * S] == s[j * S] && conflict[(long long)i * L + j]) return false;
  return true;
}

template <int S = 1>
__device__ __forceinline__ float ga_price(const short* s, int L, int V, const float* __restrict__ cost,
                                          const uint8_t* __restrict__ conflict, float invL, float invalid) {
  float acc = 0.f;
  for (int l = 0; l < L; ++l) acc += cost[(long long)l * V + s[l * S]];
  return ga_valid<S>(s, L, conflict) ? acc * invL : invalid;
}

__global__ __launch_bounds__(64) void ga_assign_kernel(
    const float* __restrict__ cost, int L, int V, const uint8_t* __restrict__ conflict, float invalid, int swap,
    short* __restrict__ pop, float* __restrict__ pop_cost, float* __restrict__ hist, GaArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ga_lds[];
  GaPool<short> W;
  W.carve(ga_lds, A.P, L, A.r);
  const int lane = threadIdx.x;
  const unsigned long long gi = (unsigned long long)(A.island_base + (long long)blockIdx.x);
  const float invL = 1.f / (float)L;
  ga_island(W, A, L, pop, pop_cost, hist, lane, 64, [&](unsigned long long ctr0) {
    short* c = W.kid + (size_t)lane * L;
    if (lane < 2 * A.r) {
      const int h = lane & 1;
      const unsigned long long ctr = ctr0 + (unsigned long long)(lane >> 1);
      const GaPair pr = ga_draw_pair(A.seed, ctr, gi, A.m, L);
      const short* Hd = W.pa + (size_t)W.ord[h ? pr.b : pr.a] * L;  // head of this child
      const short* Tl = W.pa + (size_t)W.ord[h ? pr.a : pr.b] * L;  // tail
      for (int l = 0; l < L; ++l) c[l] = l < pr.x ? Hd[l] : Tl[l];
      int pos = 0, old = 0, v = 0, holder = -1;
      ga_mutate(
          A, ctr, gi, h,
          [&](unsigned qp, unsigned qv) {
            pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
            old = c[pos];
            v = min((int)(av::u32_to_unit(qv) * (float)(V - 1)), V - 2);
            v += v >= old;
            holder = -1;
            if (swap)
              for (int j = 0; j < L; ++j)
                if (j != pos && c[j] == v) { holder = j; break; }
            if (holder >= 0) c[holder] = (short)old;
            c[pos] = (short)v;
          },
          [&] { return ga_valid(c, L, conflict); },
          [&] {
            c[pos] = (short)old;
            if (holder >= 0) c[holder] = (short)v;
          });
    }
    __syncthreads();
    if (lane < 2 * A.r) W.kc[lane] = ga_price(c, L, V, cost, conflict, invL, invalid);
  });
}

// ---- island GA over a meeting-schedule domain (P/app/mesched.py, optimize/domains.py) ----------
// The island frame above (one wave per island) with the domain's own validity and cost:
//   * a solution is (day, hour, minute) index triples of M meetings, L = 3 M; meeting i starts at
//     (days[d] - 1) 86400 + hours[h] 3600 + minutes[mi] 60 s and lasts dur[i] s;
//   * invalid: two meetings with a common participant overlap, a meeting of a blocked person
//     overlaps the blocked interval, or an ordered pair (a, b) has end[a] > start[b] — integers only;
//   * cost: per person q, over the days with a meeting, free = sum(36000 - booked) and
//     nslots = sum(cnt + 1).  With ndays = the number of distinct days of q's meetings these are
//     36000 ndays - (total duration of q's meetings) and (meetings of q) + ndays, so no per-day
//     counters are kept: one OR of day bits per person.  pc = 8 - (free / nslots) / 3600,
//     cost = sum(pc w) / sum(w) in fp32 with q ascending, multiply and add rounded separately;
//   * the crossover cut falls between meetings (3 x), mutation moves one index to a different value
//     of its table (tables of one value are left alone).
// Each child lane keeps the start second and the day bit of every meeting of its child in two
// lane-private LDS rows (odd stride: conflict-free), so no private array is indexed dynamically.
// optimize/ga_meeting.py::ga_meeting_reference is the bit-exact host twin.
constexpr int MT_MAX_M = 32, MT_MAX_Q = 256, MT_MAX_CARD = 32, MT_MAX_LIST = 16;
constexpr int MT_DOM_INTS = 3 * MT_MAX_CARD + 2 * MT_MAX_M + 2 * MT_MAX_Q + 5 * MT_MAX_LIST;  // staged domain

struct MtLds {  // the staged domain
  const int *days, *hours, *minutes, *dur, *blocked, *ordered;
  const unsigned *share, *member;
  const float* role_w;
  int M, Q, nb, no;
};

// start second and day bit of meeting i of solution c.  S is the element stride of c, st and db:
// 1 for rows, 64 for the lane-private [j][64] columns of the annealing kernel.
template <int S = 1>
__device__ __forceinline__ void mt_place(const MtLds& D, const short* c, int i, int* st, unsigned* db) {
  const int d = c[3 * i * S];
  st[i * S] = (D.days[d] - 1) * 86400 + D.hours[c[(3 * i + 1) * S]] * 3600 + D.minutes[c[(3 * i + 2) * S]] * 60;
  db[i * S] = 1u << d;
}

template <int S = 1>
__device__ __forceinline__ bool mt_valid(const MtLds& D, const int* st) {
  bool ok = true;
  for (int i = 1; i < D.M; ++i) {
    unsigned mk = D.share[i] & ((1u << i) - 1u);  // share is symmetric: pairs j < i
    const int si = st[i * S], ei = si + D.dur[i];
    while (mk) {
      const int j = __ffs(mk) - 1;
      mk &= mk - 1;
      const int sj = st[j * S];
      ok &= !(si < sj + D.dur[j] && sj < ei);
    }
  }
  for (int b = 0; b < D.nb; ++b) {
    unsigned mk = (unsigned)D.blocked[3 * b];
    const int bs = D.blocked[3 * b + 1], be = D.blocked[3 * b + 2];
    while (mk) {
      const int i = __ffs(mk) - 1;
      mk &= mk - 1;
      const int si = st[i * S];
      ok &= !(si < be && bs < si + D.dur[i]);
    }
  }
  for (int o = 0; o < D.no; ++o) {
    const int a = D.ordered[2 * o], b = D.ordered[2 * o + 1];
    ok &= st[a * S] + D.dur[a] <= st[b * S];
  }
  return ok;
}

template <int S = 1>
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
      dm |= db[i * S];
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

// The domain -> MT_DOM_INTS dwords of LDS at di, by the 64 lanes of a wave (every table and list has
// at most 64 entries but member / role_w); the caller's barrier follows.
__device__ __forceinline__ MtLds mt_stage(const avk::GaMeetingDomain& dom, int* di, int lane) {
  int* l_days = di;
  int* l_hours = l_days + MT_MAX_CARD;
  int* l_minutes = l_hours + MT_MAX_CARD;
  int* l_dur = l_minutes + MT_MAX_CARD;
  unsigned* l_share = reinterpret_cast<unsigned*>(l_dur + MT_MAX_M);
  unsigned* l_member = l_share + MT_MAX_M;
  float* l_role = reinterpret_cast<float*>(l_member + MT_MAX_Q);
  int* l_blocked = reinterpret_cast<int*>(l_role + MT_MAX_Q);
  int* l_ordered = l_blocked + 3 * MT_MAX_LIST;
  if (lane < dom.nd) l_days[lane] = dom.days[lane];
  if (lane < dom.nh) l_hours[lane] = dom.hours[lane];
  if (lane < dom.nm) l_minutes[lane] = dom.minutes[lane];
  if (lane < dom.M) {
    l_dur[lane] = dom.dur[lane];
    l_share[lane] = dom.share[lane];
  }
  for (int q = lane; q < dom.Q; q += 64) {
    l_member[q] = dom.member[q];
    l_role[q] = dom.role_w[q];
  }
  if (lane < 3 * dom.nb) l_blocked[lane] = dom.blocked[lane];
  if (lane < 2 * dom.no) l_ordered[lane] = dom.ordered[lane];
  return MtLds{l_days, l_hours, l_minutes, l_dur, l_blocked, l_ordered, l_share, l_member, l_role,
               dom.M, dom.Q, dom.nb, dom.no};
}

__global__ __launch_bounds__(64) void ga_meeting_kernel(
    avk::GaMeetingDomain dom, float invalid, short* __restrict__ pop, float* __restrict__ pop_cost,
    float* __restrict__ hist, GaArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_lds[];
  const int M = dom.M, L = 3 * M, Ms = M | 1;  // Ms: odd stride of the lane-private rows
  GaPool<short> W;
  unsigned char* cur = W.carve(gm_lds, A.P, L, A.r);
  int* st_all = reinterpret_cast<int*>(cur);  cur += ga_a16((size_t)2 * A.r * Ms * sizeof(int));   // [2r][Ms] starts
  unsigned* db_all = reinterpret_cast<unsigned*>(cur); cur += ga_a16((size_t)2 * A.r * Ms * sizeof(int));  // day bits
  const int lane = threadIdx.x;
  const unsigned long long gi = (unsigned long long)(A.island_base + (long long)blockIdx.x);
  const MtLds D = mt_stage(dom, reinterpret_cast<int*>(cur), lane);  // the frame's first barrier covers it
  ga_island(W, A, L, pop, pop_cost, hist, lane, 64, [&](unsigned long long ctr0) {
    if (lane < 2 * A.r) {
      const int h = lane & 1;
      const unsigned long long ctr = ctr0 + (unsigned long long)(lane >> 1);
      const GaPair pr = ga_draw_pair(A.seed, ctr, gi, A.m, M);
      const int cut = 3 * pr.x;
      const short* Hd = W.pa + (size_t)W.ord[h ? pr.b : pr.a] * L;  // head of this child
      const short* Tl = W.pa + (size_t)W.ord[h ? pr.a : pr.b] * L;  // tail
      short* c = W.kid + (size_t)lane * L;
      int* st = st_all + lane * Ms;
      unsigned* db = db_all + lane * Ms;
      for (int l = 0; l < L; ++l) c[l] = l < cut ? Hd[l] : Tl[l];
      for (int i = 0; i < M; ++i) mt_place(D, c, i, st, db);
      int pos = 0, mi = 0, card = 0, old = 0;
      const bool ok = ga_mutate(
          A, ctr, gi, h,
          [&](unsigned qp, unsigned qv) {
            pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
            mi = pos / 3;
            const int comp = pos - 3 * mi;
            card = comp == 0 ? dom.nd : comp == 1 ? dom.nh : dom.nm;
            old = c[pos];
            if (card > 1) {
              int v = min((int)(av::u32_to_unit(qv) * (float)(card - 1)), card - 2);
              v += v >= old;
              c[pos] = (short)v;
              mt_place(D, c, mi, st, db);
            }
          },
          [&] { return mt_valid(D, st); },
          [&] {
            if (card > 1) {
              c[pos] = (short)old;
              mt_place(D, c, mi, st, db);
            }
          });
      W.kc[lane] = ok ? mt_cost(D, db) : invalid;
    }
  });
}

// ---- feature subsets scored by naive Bayes (P/app/fesel.py, optimize/domains.py) ---------------
// LL [N][F][C] holds per-row, per-feature, per-class log-likelihoods; a subset is a 32-bit mask
// (bit f = feature f included).  The score of row n and class c is log_prior[c] plus LL[n][f][c]
// over the set bits, f ascending, one fp32 add each; the prediction is the lowest c with the
// largest score and a subset's error count is the number of rows whose prediction differs from
// the label.  Counts are integers, so they depend on no grid, tile or workgroup size.
//
// Both kernels stage a tile of TR rows in LDS (row stride F C | 1: lanes on consecutive rows hit
// distinct banks) and give every thread one row of the tile.  With TR >= 64 a wave shares its
// masks: each is read by broadcast into a scalar register, the scalar unit walks its set bits and
// one ballot count per mask goes to the LDS counters.  Tiles of 16 or 32 rows (F C > 191) put
// several masks on a wave: every thread then takes groups of FS_K masks, reads each LL value once
// per group and applies it to FS_K running scores under the masks' bits.
// optimize/ga_subset.py holds the bit-exact host twins.
constexpr int FS_TILE_BYTES = 48 * 1024, FS_MASK_CHUNK = 1024, FS_K = 4, FS_MAX_C = 16;

inline int fs_tile_rows(int FC, int nt) {
  int tr = nt;
  while (tr > 16 && (size_t)tr * (FC | 1) * sizeof(float) > (size_t)FS_TILE_BYTES) tr >>= 1;
  return tr;
}

// rows [n0, n0 + nr) of LL -> tile; magic = ceil(2^32 / FC) turns e / FC into one multiply
// (exact while e FC < 2^32; e < 2^14 and FC <= 512 here)
__device__ __forceinline__ void fs_stage(float* tile, const float* __restrict__ LL, long long n0, int nr, int FC,
                                         int stride, unsigned magic, int tid, int nt) {
  const float* src = LL + n0 * FC;
  const int tot = nr * FC;
  for (int e = tid; e < tot; e += nt) {
    const int row = (int)__umulhi((unsigned)e, magic);
    tile[row * stride + (e - row * FC)] = src[e];
  }
}

// The scoring core: is the row with log-likelihoods ll [F][C] mis-predicted under each of K subsets?
template <int K>
__device__ __forceinline__ void fs_row_miss(const float* ll, const float* prior, int F, int C, const unsigned (&mk)[K],
                                            int label, bool (&miss)[K]) {
  float best[K];
  int bc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    best[k] = 0.f;
    bc[k] = 0;
  }
  for (int c = 0; c < C; ++c) {
    float s[K];
    const float p = prior[c];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = p;
    const float* q = ll + c;
    for (int f = 0; f < F; ++f) {
      const float v = q[f * C];
#pragma unroll
      for (int k = 0; k < K; ++k) s[k] = ((mk[k] >> f) & 1u) ? s[k] + v : s[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (c == 0 || s[k] > best[k]) {
        best[k] = s[k];
        bc[k] = c;
      }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) miss[k] = bc[k] != label;
}

// The same scores for ONE subset that the whole wave shares (mk in a scalar register): the scalar
// unit walks the set bits, f ascending, and the vector unit spends one add per included feature
// and class; two classes advance together for independent add chains.
__device__ __forceinline__ bool fs_row_miss_uniform(const float* ll, const float* prior, int C, unsigned mk, int label) {
  float best = 0.f;
  int bc = 0;
  for (int c = 0; c < C; c += 2) {
    const bool two = c + 1 < C;
    float s0 = prior[c], s1 = two ? prior[c + 1] : 0.f;
    const float* q = ll + c;
    for (unsigned m = mk; m; m &= m - 1u) {
      const int o = (__ffs(m) - 1) * C;
      s0 = s0 + q[o];
      if (two) s1 = s1 + q[o + 1];
    }
    if (c == 0 || s0 > best) {
      best = s0;
      bc = c;
    }
    if (two && s1 > best) {
      best = s1;
      bc = c + 1;
    }
  }
  return bc != label;
}

// Every thread of the workgroup: the nr staged rows against the masks masks[d], d = idx[j] (or j
// without idx), j < nm; the misses of mask d are added to cnt[d].  labels points at the tile's row 0.
__device__ __forceinline__ void fs_score_tile(const float* tile, int stride, int TR, int nr, const float* prior, int F,
                                              int C, const int* __restrict__ labels, const unsigned* masks,
                                              const int* idx, int nm, int* cnt, int tid, int nt) {
  const int sh = __ffs(TR) - 1;  // TR and nt are powers of two, TR <= nt
  const int row = tid & (TR - 1), slot = tid >> sh, nslot = nt >> sh;
  const bool live = row < nr;
  const int label = live ? labels[row] : 0;
  const float* ll = tile + row * stride;
  if (TR >= 64) {  // a wave shares slot, hence its masks: one ballot count per mask
    for (int j = __builtin_amdgcn_readfirstlane(slot); j < nm; j += nslot) {
      const int dst = idx ? idx[j] : j;
      const unsigned mk = (unsigned)__builtin_amdgcn_readfirstlane((int)masks[dst]);
      const bool hit = fs_row_miss_uniform(ll, prior, C, mk, label) && live;
      const int n = __popcll(__ballot(hit));
      if ((tid & 63) == 0 && n) atomicAdd(&cnt[dst], n);
    }
    return;
  }
  for (int j0 = slot * FS_K; j0 < nm; j0 += nslot * FS_K) {
    unsigned mk[FS_K];
    int dst[FS_K];
#pragma unroll
    for (int k = 0; k < FS_K; ++k) {
      const int j = j0 + k;
      dst[k] = j < nm ? (idx ? idx[j] : j) : -1;
      mk[k] = dst[k] >= 0 ? masks[dst[k]] : 0u;
    }
    bool miss[FS_K];
    fs_row_miss<FS_K>(ll, prior, F, C, mk, label, miss);
#pragma unroll
    for (int k = 0; k < FS_K; ++k) {
      if (live && miss[k] && dst[k] >= 0) atomicAdd(&cnt[dst[k]], 1);
    }
  }
}

// out[b] += the error count of masks[b] over this block's row tiles (tiles blockIdx.x, + gridDim.x,
// ...); the launcher clears out.  Masks go through LDS in chunks of mchunk <= FS_MASK_CHUNK, the
// chunks dealt over blockIdx.y so that few row tiles still fill the chip.
__global__ __launch_bounds__(256) void subset_errors_kernel(
    const float* __restrict__ LL, const float* __restrict__ log_prior, const int* __restrict__ labels, int N, int F,
    int C, const unsigned* __restrict__ masks, int B, int* __restrict__ out, int TR, int mchunk) {
  extern __shared__ __attribute__((aligned(16))) float fs_tile[];
  __shared__ unsigned s_mask[FS_MASK_CHUNK];
  __shared__ int s_cnt[FS_MASK_CHUNK];
  __shared__ float s_prior[FS_MAX_C];
  const int tid = threadIdx.x, FC = F * C, stride = FC | 1;
  const unsigned magic = 0xFFFFFFFFu / (unsigned)FC + 1u;
  const unsigned fmask = F == 32 ? ~0u : (1u << F) - 1u;
  const int ntiles = (N + TR - 1) / TR;
  if (tid < C) s_prior[tid] = log_prior[tid];
  for (int b0 = blockIdx.y * mchunk; b0 < B; b0 += gridDim.y * mchunk) {
    const int nb = min(mchunk, B - b0);
    for (int j = tid; j < nb; j += 256) {
      s_mask[j] = masks[b0 + j] & fmask;
      s_cnt[j] = 0;
    }
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
      const long long n0 = (long long)t * TR;
      const int nr = min(TR, N - (int)n0);
      fs_stage(fs_tile, LL, n0, nr, FC, stride, magic, tid, 256);
      __syncthreads();
      fs_score_tile(fs_tile, stride, TR, nr, s_prior, F, C, labels + n0, s_mask, nullptr, nb, s_cnt, tid, 256);
      __syncthreads();
    }
    for (int j = tid; j < nb; j += 256) {
      const int c = s_cnt[j];
      if (c) atomicAdd(&out[b0 + j], c);
    }
  }
}

// ---- island GA over feature subsets ------------------------------------------------------------
// The island frame above with a solution held as one 32-bit mask; wave 0 breeds (lane c < 2r, child
// c), then every wave of the workgroup scores:
//   * valid: min_size <= popcount <= max_size; mutation flips one bit (the value word of the
//     shared counter layout is unused);
//   * the crossover cut lies in [1, F) (none at F = 1);
//   * cost: every wave of the workgroup scores the valid children over the N rows, tile by
//     tile, into integer LDS counters; cost = (float)errors / (float)N, `invalid` for an invalid child.
// pop stays int16 [islands][P][F] of 0 / 1 at the interface; it is packed on entry and unpacked
// on exit.  The workgroup has blockDim.x = 256 or 1,024 threads; no result depends on it.
// optimize/ga_subset.py::ga_subset_reference is the bit-exact host twin.
__global__ __launch_bounds__(1024) void ga_subset_kernel(
    const float* __restrict__ LL, const float* __restrict__ log_prior, const int* __restrict__ labels, int N, int F,
    int C, int min_size, int max_size, float invalid, short* __restrict__ pop, float* __restrict__ pop_cost,
    float* __restrict__ hist, GaArgs A, int TR) {
  extern __shared__ __attribute__((aligned(16))) float fs_tile[];
  __shared__ unsigned s_pool[2][64], s_kid[64];
  __shared__ float s_pc[2][64], s_kc[64], s_prior[FS_MAX_C];
  __shared__ int s_ord[64], s_kord[64], s_nsrc[64], s_cnt[64], s_vk[64], s_nv;
  GaPool<unsigned> W{s_pool[0], s_pool[1], s_kid, s_pc[0], s_pc[1], s_kc, s_ord, s_kord, s_nsrc};
  const int tid = threadIdx.x, nt = blockDim.x, FC = F * C, stride = FC | 1;
  const unsigned magic = 0xFFFFFFFFu / (unsigned)FC + 1u;
  const int ntiles = (N + TR - 1) / TR;
  const unsigned long long gi = (unsigned long long)(A.island_base + (long long)blockIdx.x);
  if (tid < C) s_prior[tid] = log_prior[tid];
  bool staged = false;
  ga_island(W, A, F, pop, pop_cost, hist, tid, nt, [&](unsigned long long ctr0) {
    // wave 0: lane c builds and mutates child c of pair c >> 1; the valid children are listed in s_vk
    bool ok = false;
    if (tid < 64) {
      if (tid < 2 * A.r) {
        const int h = tid & 1;
        const unsigned long long ctr = ctr0 + (unsigned long long)(tid >> 1);
        const GaPair pr = ga_draw_pair(A.seed, ctr, gi, A.m, F);
        const unsigned low = (1u << pr.x) - 1u;  // cut <= 31
        const unsigned Hd = W.pa[W.ord[h ? pr.b : pr.a]], Tl = W.pa[W.ord[h ? pr.a : pr.b]];  // head, tail
        unsigned c = (Hd & low) | (Tl & ~low);
        int pos = 0;
        ok = ga_mutate(
            A, ctr, gi, h,
            [&](unsigned qp, unsigned) {
              pos = min((int)(av::u32_to_unit(qp) * (float)F), F - 1);
              c ^= 1u << pos;
            },
            [&] {
              const int sz = __popc(c);
              return sz >= min_size && sz <= max_size;
            },
            [&] { c ^= 1u << pos; });
        s_kid[tid] = c;
        s_kc[tid] = invalid;
        s_cnt[tid] = 0;
      }
      const unsigned long long vb = __ballot(ok);
      if (ok) s_vk[__popcll(vb & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) s_nv = __popcll(vb);
    }
    __syncthreads();
    // all waves: the valid children over the N rows
    const int nv = s_nv;
    if (nv)
      for (int t = 0; t < ntiles; ++t) {
        const long long n0 = (long long)t * TR;
        const int nr = min(TR, N - (int)n0);
        if (ntiles > 1 || !staged) {  // a single tile stays staged for the whole launch
          fs_stage(fs_tile, LL, n0, nr, FC, stride, magic, tid, nt);
          staged = true;
          __syncthreads();
        }
        fs_score_tile(fs_tile, stride, TR, nr, s_prior, F, C, labels + n0, s_kid, s_vk, nv, s_cnt, tid, nt);
        __syncthreads();
      }
    if (ok) s_kc[tid] = (float)s_cnt[tid] / (float)N;
  });
}

// ---- simulated-annealing chains over assignment, meeting-schedule and feature-subset domains ----
// Reference: the Spark simulatedAnnealing job and SimulatedAnnealingOptimizer
// (P/mlextra/optsolo.py:34-88, which `fesel sa` drives).  Chain g = chain_base + p is GLOBAL; move
// `it` of [it_begin, it_begin + iters):
//   1. attempts tr = 0..max_retry draw Philox(seed, offset + it (max_retry + 1) + tr, g): word x
//      picks the position, word y the value; the first attempt that gives a valid candidate is the
//      move, and without one nothing happens (no counter changes);
//   2. the candidate is priced from scratch, so cur_cost is always the price of sol;
//   3. cc <= c is accepted (`better`, also from c = inf); otherwise
//      u(Philox(seed ^ 0x9E3779B97F4A7C15, offset + it, g).x) < sa_exp(-((cc - c) / max(temp, 1e-12)))
//      is accepted (`worse_accepted`); the rest is `rejected`;
//   4. on acceptance sol = cand, c = cc, and c < best_cost replaces the best;
//   5. cooling after every move, when interval > 0 and (it + 1) % interval == 0: temp * cool, or
//      max(t0 - (float)(it + 1) cool, 1e-12), product and difference rounded separately.
// Every fp32 operation is rounded on its own (no contraction) and sa_exp is built from such
// operations alone, so optimize/sa.py::sa_chains_reference equals the kernels bit for bit, the
// Metropolis decision included.  What a solution is, when it is valid and what it costs is the
// domain's: the meeting and subset kernels supply propose / price / settle / improved to sa_chain.
struct SaArgs {
  int P;
  long long iters, it_begin;
  float t0, cool;
  long long interval;
  int geometric, max_retry;
  unsigned long long seed, offset;
  float temp_start;
  long long chain_base;
};

// exp(x) for x <= 0 (clamped to -87, where the result is still a normal number): k = rint(x log2 e),
// two-constant Cody-Waite reduction, degree-6 Taylor polynomial by Horner, exact scaling by 2^k.
// Within 1e-6 relative of exp; optimize/sa.py::sa_exp is the same operations in the same order.
__device__ __forceinline__ float sa_exp(float x) {
#pragma clang fp contract(off)
  x = fmaxf(x, -87.f);
  const float k = rintf(x * 1.4426950408889634f);
  float r = x - k * 0.693359375f;  // 355 / 512: the product is exact
  r = r - k * -2.12194440e-4f;
  float p = 1.f / 720.f;
  p = p * r + 1.f / 120.f;
  p = p * r + 1.f / 24.f;
  p = p * r + 1.f / 6.f;
  p = p * r + 0.5f;
  p = p * r + 1.f;
  p = p * r + 1.f;
  return ldexpf(p, (int)k);
}

// step 3: 0 rejected, 1 better, 2 worse but accepted
__device__ __forceinline__ int sa_accept(const SaArgs& A, long long it, unsigned long long gp, float cc, float c,
                                         float temp) {
#pragma clang fp contract(off)
  if (cc <= c) return 1;
  const av::u4 r = av::philox_draw(A.seed ^ 0x9e3779b97f4a7c15ull, A.offset + (unsigned long long)it, gp);
  const float q = (cc - c) / fmaxf(temp, 1e-12f);
  return av::u32_to_unit(r.x) < sa_exp(-q) ? 2 : 0;
}

// step 5
__device__ __forceinline__ float sa_cool(const SaArgs& A, long long it, float temp) {
#pragma clang fp contract(off)
  if (A.interval > 0 && (it + 1) % A.interval == 0) {
    if (A.geometric) return temp * A.cool;
    const float d = (float)(it + 1) * A.cool;
    return fmaxf(A.t0 - d, 1e-12f);
  }
  return temp;
}

struct SaChain {  // what a chain carries besides its solution
  float c, bc, temp;
  unsigned long long better, worse, rejected;
};

// The moves of one chain.  propose(x, y) -> bool: one attempt; it leaves a valid candidate pending
// and takes an invalid one back.  price(moved) -> float: the pending candidate's cost; every thread
// calls it every move (it may hold barriers), its value counts only where moved.  settle(accepted):
// the candidate becomes the solution, or is taken back.  improved(): the solution is the new best.
// A chain that is not `live` proposes nothing and only keeps price's barriers.
template <class Propose, class Price, class Settle, class Improved>
__device__ __forceinline__ void sa_chain(const SaArgs& A, unsigned long long gp, bool live, SaChain& S,
                                         Propose propose, Price price, Settle settle, Improved improved) {
  const unsigned long long R = (unsigned long long)A.max_retry + 1ull;
  for (long long it = A.it_begin; it < A.it_begin + A.iters; ++it) {
    bool moved = false;
    if (live)
      for (int tr = 0; tr <= A.max_retry && !moved; ++tr) {
        const av::u4 q = av::philox_draw(A.seed, A.offset + (unsigned long long)it * R + (unsigned long long)tr, gp);
        moved = propose(q.x, q.y);
      }
    const float cc = price(moved);
    if (moved) {
      const int a = sa_accept(A, it, gp, cc, S.c, S.temp);
      settle(a != 0);
      if (a) {
        S.c = cc;
        if (a == 1) ++S.better; else ++S.worse;
        if (S.c < S.bc) {
          S.bc = S.c;
          improved();
        }
      } else {
        ++S.rejected;
      }
    }
    S.temp = sa_cool(A, it, S.temp);
  }
}

// stats[0..2] += the chain's counters; local chain 0 leaves the hand-off temperature's bits in stats[3]
__device__ __forceinline__ void sa_report(unsigned long long* __restrict__ stats, long long p, const SaChain& S) {
  if (!stats) return;
  if (p == 0) stats[3] = (unsigned long long)__float_as_uint(S.temp);
  if (S.better) atomicAdd(&stats[0], S.better);
  if (S.worse) atomicAdd(&stats[1], S.worse);
  if (S.rejected) atomicAdd(&stats[2], S.rejected);
}

// true when position i conflicts with no other position holding the same value
__device__ __forceinline__ bool position_ok(const short* s, int L, int i, const uint8_t* __restrict__ conflict) {
  const short v = s[i * 64];
  const uint8_t* row = conflict + (long long)i * L;
  for (int j = 0; j < L; ++j)
    if (j != i && s[j * 64] == v && row[j]) return false;
  return true;
}

// Assignments (s[i] in [0, V); cost = mean_i C[i][s[i]]; invalid when two positions with a conflict
// share a value).  The kernel keeps its own arguments, 32-bit move counter and stats hand-off: its
// loop is latency-bound with the scalar registers at their cap and ran 1.7 to 7 % slower on SaArgs /
// SaChain.  It prices by the O(1) cost delta, accepts through __expf and cools by an expression the
// compiler may contract: optimize/sa.py::sa_assign_reference follows it closely, not bit for bit.
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

// Meeting schedules: one chain per lane, 64-lane workgroups.  The chain's index triples, start
// seconds and day bits are columns `lane` of [3 M][64] short, [M][64] int and [M][64] unsigned LDS
// tiles (lane-private, one bank per lane), the domain is staged behind them.  A move is the island
// kernel's mutation: one index to a different value of its table (a table of one value leaves the
// solution as it is); it touches one meeting, so mt_place runs for that meeting alone, and taking a
// move back places the old value again.  The best solution goes to global memory on improvement.
__global__ __launch_bounds__(64) void sa_meeting_kernel(
    avk::GaMeetingDomain dom, short* __restrict__ sol, float* __restrict__ cur_cost, short* __restrict__ best_sol,
    float* __restrict__ best_cost, unsigned long long* __restrict__ stats, SaArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
  const int M = dom.M, L = 3 * M;
  const int lane = threadIdx.x;
  short* s = reinterpret_cast<short*>(sm_lds) + lane;                                     // element j at s[j * 64]
  int* st = reinterpret_cast<int*>(sm_lds + (size_t)L * 64 * sizeof(short)) + lane;       // start of meeting i at st[i * 64]
  unsigned* db = reinterpret_cast<unsigned*>(st - lane + (size_t)M * 64) + lane;          // its day bit
  const MtLds D = mt_stage(dom, reinterpret_cast<int*>(db - lane + (size_t)M * 64), lane);
  const long long p = (long long)blockIdx.x * 64 + lane;
  const bool live = p < A.P;
  if (live)
    for (int j = 0; j < L; ++j) s[j * 64] = sol[p * L + j];
  __syncthreads();
  if (!live) return;
  for (int i = 0; i < M; ++i) mt_place<64>(D, s, i, st, db);
  const unsigned long long gp = (unsigned long long)(A.chain_base + p);
  short* bs = best_sol + p * L;
  SaChain S{cur_cost[p], best_cost[p], A.temp_start, 0, 0, 0};
  int pos = 0, mi = 0, card = 0, old = 0;
  auto put = [&](int v) {
    if (card > 1) {
      s[pos * 64] = (short)v;
      mt_place<64>(D, s, mi, st, db);
    }
  };
  sa_chain(
      A, gp, true, S,
      [&](unsigned qp, unsigned qv) {
        pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
        mi = pos / 3;
        const int comp = pos - 3 * mi;
        card = comp == 0 ? dom.nd : comp == 1 ? dom.nh : dom.nm;
        old = s[pos * 64];
        int v = min((int)(av::u32_to_unit(qv) * (float)(card - 1)), card - 2);
        v += v >= old;
        put(v);
        const bool ok = mt_valid<64>(D, st);
        if (!ok) put(old);
        return ok;
      },
      [&](bool moved) { return moved ? mt_cost<64>(D, db) : 0.f; },
      [&](bool accepted) {
        if (!accepted) put(old);
      },
      [&] {
        for (int j = 0; j < L; ++j) bs[j] = s[j * 64];
      });
  for (int j = 0; j < L; ++j) sol[p * L + j] = s[j * 64];
  cur_cost[p] = S.c;
  best_cost[p] = S.bc;
  sa_report(stats, p, S);
}

// Feature subsets: a workgroup of 256 or 1,024 threads whose waves are split into chains of w waves
// each (w = 1, 2, 4, 8 or 16).  All chains of the workgroup share the staged row tile (odd stride,
// the labels behind it; a single tile stays resident for the whole launch).  Every lane of a chain
// draws the same Philox words, so the chain's masks, costs and counters are wave-uniform and each
// of its waves carries them; the candidate mask is handed to the scoring as a scalar.  A chain's
// waves walk the tile's 64-row groups (wave `sub` takes groups sub, sub + w, ...), count misses by
// ballot into a register, and the w partial counts meet in an integer LDS counter.  The counters
// are three deep: move k adds to counter k % 3 and clears counter (k + 1) % 3, whose last readers
// passed a barrier before, so one barrier per tile and move is enough.  Error counts are
// integers: no result depends on w, the thread count or the tile size.
constexpr int SA_FS_MAX_CHAINS = 16;  // chains per workgroup: 1,024 threads of one-wave chains

__global__ __launch_bounds__(1024) void sa_subset_kernel(
    const float* __restrict__ LL, const float* __restrict__ log_prior, const int* __restrict__ labels, int N, int F,
    int C, int min_size, int max_size, short* __restrict__ sol, float* __restrict__ cur_cost,
    short* __restrict__ best_sol, float* __restrict__ best_cost, unsigned long long* __restrict__ stats, SaArgs A,
    int TR, int w) {
  extern __shared__ __attribute__((aligned(16))) float fs_tile[];
  __shared__ float s_prior[FS_MAX_C];
  __shared__ int s_cnt[3][SA_FS_MAX_CHAINS];
  const int tid = threadIdx.x, nt = blockDim.x, FC = F * C, stride = FC | 1;
  const unsigned magic = 0xFFFFFFFFu / (unsigned)FC + 1u;
  const int ntiles = (N + TR - 1) / TR;
  int* s_lab = reinterpret_cast<int*>(fs_tile + (size_t)TR * stride);  // [TR] labels of the staged rows
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wsh = __ffs(w) - 1, ci = wave >> wsh, sub = wave & (w - 1), cpw = (nt >> 6) >> wsh;
  const long long p = (long long)blockIdx.x * cpw + ci;
  const bool live = p < A.P;
  const unsigned long long gp = (unsigned long long)(A.chain_base + p);
  if (tid < C) s_prior[tid] = log_prior[tid];
  if (tid < 3 * SA_FS_MAX_CHAINS) (&s_cnt[0][0])[tid] = 0;
  unsigned mk = 0, bmk = 0, cand = 0;
  SaChain S{0.f, 0.f, A.temp_start, 0, 0, 0};
  if (live) {
    const bool in = lane < F;
    mk = (unsigned)__ballot(in && sol[p * F + (in ? lane : 0)] != 0);
    bmk = (unsigned)__ballot(in && best_sol[p * F + (in ? lane : 0)] != 0);
    S.c = cur_cost[p];
    S.bc = best_cost[p];
  }
  __syncthreads();
  bool staged = false;
  int k = 0;  // move of this launch
  sa_chain(
      A, gp, live, S,
      [&](unsigned qp, unsigned) {
        const int pos = min((int)(av::u32_to_unit(qp) * (float)F), F - 1);
        cand = (unsigned)__builtin_amdgcn_readfirstlane((int)(mk ^ (1u << pos)));
        const int sz = __popc(cand);
        return sz >= min_size && sz <= max_size;
      },
      [&](bool moved) {
        int* cnt = s_cnt[k % 3];
        if (tid < SA_FS_MAX_CHAINS) s_cnt[(k + 1) % 3][tid] = 0;
        ++k;
        int n = 0;
        for (int t = 0; t < ntiles; ++t) {
          const long long n0 = (long long)t * TR;
          const int nr = min(TR, N - (int)n0);
          if (ntiles > 1 || !staged) {
            fs_stage(fs_tile, LL, n0, nr, FC, stride, magic, tid, nt);
            for (int e = tid; e < nr; e += nt) s_lab[e] = labels[n0 + e];
            staged = true;
            __syncthreads();
          }
          if (moved) {
            const int ng = (nr + 63) >> 6;
            for (int g = sub; g < ng; g += w) {
              const int row = g * 64 + lane;
              const int rr = min(row, nr - 1);  // lanes past the tile score its last row, uncounted
              const bool miss = fs_row_miss_uniform(fs_tile + rr * stride, s_prior, C, cand, s_lab[rr]);
              n += __popcll(__ballot(miss && row < nr));
            }
            if (t == ntiles - 1 && lane == 0 && n) atomicAdd(&cnt[ci], n);
          }
          __syncthreads();  // the counts are in; the tile may be staged again
        }
        return (float)__builtin_amdgcn_readfirstlane(cnt[ci]) / (float)N;
      },
      [&](bool accepted) {
        if (accepted) mk = cand;
      },
      [&] { bmk = mk; });
  if (live && sub == 0) {
    if (lane < F) {
      sol[p * F + lane] = (short)((mk >> lane) & 1u);
      best_sol[p * F + lane] = (short)((bmk >> lane) & 1u);
    }
    if (lane == 0) {
      cur_cost[p] = S.c;
      best_cost[p] = S.bc;
      sa_report(stats, p, S);
    }
  }
}

// ---- tabu search over assignments: one chain per wave, all iterations in one launch -------------
// Reference: the tenure purge of TabuSearchDomain (J/optimize/TabuSearchDomain.java:54-66) over the
// full single-reassignment neighbourhood.  A chain's state is its solution, the solution's cost, the
// best solution and cost, and tabu[l][v] = the first iteration at which moving position l to value
// v is free again.  Iteration `it`:
//   1. every cell (l, v) is priced nc = cost + ((C[l][v] - C[l][sol[l]]) / (float)L), each operation
//      rounded on its own (an IEEE division, not a product with 1 / L);
//   2. a cell is bad when v == sol[l] or a position j != l with conflict[l][j] holds v;
//   3. it is admissible when not bad and (tabu[l][v] <= it or nc < the best cost at the
//      iteration's start: aspiration);
//   4. the move is the admissible cell of smallest nc < +inf, ties to the smallest l V + v;
//   5. a move sets tabu[l][sol[l]] = it + tenure, sol[l] = v, cost = nc (moves, and aspirated when
//      the cell was tabu); without one the chain stalls;
//   6. a cost below the best replaces the best;  7. hist[p][it - it_begin] = the best cost.
// Nothing is drawn, so optimize/tabu.py::tabu_assign_reference equals the kernel bit for bit.
// A wave keeps in LDS, per chain: the tabu table, cnt[l][v] = the number of j != l with
// conflict[l][j] and sol[j] == v (validity of a cell is one read; a move updates one column of it,
// lane j the row of position j), the solution and cur[l] = C[l][sol[l]].  The 4, 2 or 1 waves of a
// workgroup share an LDS copy of C and of the transposed conflict table (STAGED; avk::
// tabu_assign_plan); where those do not fit, one wave per workgroup reads both from global memory.
// Lanes walk the L V cells in steps of 64 carrying (l, v), each keeps its best cell as one 64-bit
// key — the order-preserving image of nc's bits above the flat index — and the wave minimum of the
// keys (DPP + v_readlane) is the move.  The chain loop holds no workgroup barrier: LDS runs one
// wave's instructions in order, so a wave's reads see its earlier writes.
constexpr unsigned long long TB_NONE = ~0ull;

// monotone float -> unsigned, both zeros to one key
__device__ __forceinline__ unsigned tb_key(float f) {
  const unsigned u = __float_as_uint(f == 0.f ? 0.f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int CTRL>
__device__ __forceinline__ unsigned long long tb_min_step(unsigned long long v) {
  const unsigned lo = (unsigned)av::dpp_i<CTRL>((int)(unsigned)v);
  const unsigned hi = (unsigned)av::dpp_i<CTRL>((int)(unsigned)(v >> 32));
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o < v ? o : v;
}
__device__ __forceinline__ unsigned long long tb_readlane(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
// wave minimum of 64-bit keys, wave-uniform (all 64 lanes active)
__device__ __forceinline__ unsigned long long tb_wave_min(unsigned long long v) {
  v = tb_min_step<0xB1>(v);
  v = tb_min_step<0x4E>(v);
  v = tb_min_step<0x124>(v);
  v = tb_min_step<0x128>(v);
  const unsigned long long a = tb_readlane(v, 0), b = tb_readlane(v, 16), c = tb_readlane(v, 32), d = tb_readlane(v, 48);
  const unsigned long long ab = a < b ? a : b, cd = c < d ? c : d;
  return ab < cd ? ab : cd;
}

__host__ __device__ constexpr size_t tb_chain_bytes(size_t L, size_t V) {
  return ga_a16(4 * L * V) + ga_a16(4 * L) + ga_a16(2 * L * V) + ga_a16(2 * L);  // tabu, cur, cnt, sol
}
__host__ __device__ constexpr size_t tb_shared_bytes(size_t L, size_t V) { return ga_a16(4 * L * V) + ga_a16(L * L); }

template <bool STAGED>
__global__ __launch_bounds__(256) void tabu_assign_kernel(
    const float* __restrict__ cost, int L, int V, const uint8_t* __restrict__ conflict, short* __restrict__ sol,
    float* __restrict__ cur_cost, short* __restrict__ best_sol, float* __restrict__ best_cost, int* __restrict__ tabu,
    float* __restrict__ hist, int P, int iters, int it_begin, int tenure, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char tb_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int LV = L * V;
  const long long p = (long long)blockIdx.x * W + wave;
  unsigned char* at = tb_lds;
  const float* C = cost;
  const uint8_t* cf = conflict;  // conflict[j][l] at cf[j * cj + l * cl]
  int cj = L, cl = 1;
  if (STAGED) {
    float* Cs = reinterpret_cast<float*>(at);
    uint8_t* Ts = at + ga_a16((size_t)4 * LV);
    at += tb_shared_bytes(L, V);
    // the waves that own a chain stage the tables; the others only keep the barrier
    const int live = min((long long)W, (long long)P - (long long)blockIdx.x * W) * 64;
    if ((int)threadIdx.x < live) {
      for (int i = threadIdx.x; i < LV; i += live) Cs[i] = cost[i];
      if (conflict)
        for (int i = threadIdx.x; i < L * L; i += live) {
          const int l = i / L, j = i - l * L;
          Ts[i] = conflict[(long long)j * L + l];  // Ts[l][j] = conflict[j][l]
        }
    }
    __syncthreads();
    C = Cs;
    cf = Ts;  // read only with a conflict table
    cj = 1;
    cl = L;
  }
  if (p >= P) return;
  at += (size_t)wave * tb_chain_bytes(L, V);
  int* tb = reinterpret_cast<int*>(at);                                      at += ga_a16((size_t)4 * LV);
  float* cur = reinterpret_cast<float*>(at);                                 at += ga_a16((size_t)4 * L);
  unsigned short* cnt = reinterpret_cast<unsigned short*>(at);               at += ga_a16((size_t)2 * LV);
  short* s = reinterpret_cast<short*>(at);
  short* gs = sol + p * L;
  short* bs = best_sol + p * L;
  int* gt = tabu + p * LV;
  float* gh = hist + p * iters;
  for (int j = lane; j < L; j += 64) {
    const short x = gs[j];
    s[j] = x;
    cur[j] = C[j * V + x];
  }
  for (int i = lane; i < LV; i += 64) {
    tb[i] = gt[i];
    cnt[i] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  if (conflict)  // lane l owns row l of cnt
    for (int l = lane; l < L; l += 64)
      for (int j = 0; j < L; ++j)
        if (j != l && cf[(long long)l * cj + (long long)j * cl]) ++cnt[l * V + s[j]];
  __builtin_amdgcn_wave_barrier();
  float c = cur_cost[p], bc = best_cost[p];
  const float Lf = (float)L;
  const int l0 = lane / V, v0 = lane - l0 * V, dl = 64 / V, dv = 64 - dl * V;
  unsigned long long moves = 0, stalls = 0, aspirated = 0;
  for (int k = 0; k < iters; ++k) {
    const int it = it_begin + k;
    unsigned long long key = TB_NONE;
    int bl = 0, bv = 0;
    float bn = 0.f;
    for (int i = lane, l = l0, v = v0; i < LV; i += 64) {
      const float d = C[i] - cur[l];
      const float q = d / Lf;
      const float nc = c + q;
      const bool bad = v == s[l] || cnt[i] != 0;
      if (!bad && (tb[i] <= it || nc < bc) && nc < INFINITY) {
        const unsigned long long kk = ((unsigned long long)tb_key(nc) << 32) | (unsigned)i;
        if (kk < key) { key = kk; bl = l; bv = v; bn = nc; }
      }
      l += dl;
      v += dv;
      if (v >= V) { v -= V; ++l; }
    }
    key = tb_wave_min(key);
    if (key != TB_NONE) {
      const int i = (int)(unsigned)key;  // lane i & 63 holds the cell
      const int l = __builtin_amdgcn_readlane(bl, i & 63), v = __builtin_amdgcn_readlane(bv, i & 63);
      const int old = s[l];
      aspirated += tb[i] > it ? 1 : 0;
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        tb[l * V + old] = it + tenure;
        s[l] = (short)v;
        cur[l] = C[i];
      }
      if (conflict)  // positions in conflict with l see `old` leave and v arrive
        for (int j = lane; j < L; j += 64)
          if (j != l && cf[(long long)j * cj + (long long)l * cl]) {
            --cnt[j * V + old];
            ++cnt[j * V + v];
          }
      c = av::lane_f(bn, i & 63);
      ++moves;
      __builtin_amdgcn_wave_barrier();
    } else {
      ++stalls;
    }
    if (c < bc) {
      bc = c;
      for (int j = lane; j < L; j += 64) bs[j] = s[j];
    }
    if (lane == 0) gh[k] = bc;
  }
  for (int j = lane; j < L; j += 64) gs[j] = s[j];
  for (int i = lane; i < LV; i += 64) gt[i] = tb[i];
  if (lane == 0) {
    cur_cost[p] = c;
    best_cost[p] = bc;
    if (moves) atomicAdd(&stats[0], moves);
    if (stalls) atomicAdd(&stats[1], stalls);
    if (aspirated) atomicAdd(&stats[2], aspirated);
  }
}

// ---- evolutionary optimiser: steady-state islands, one island per lane ---------------------------
// Reference: EvolutionaryOptimizer (P/mlextra/optpopu.py:32-92): tournament selection, a mutated
// clone, purge by cost and age.  An island's state is its pool pop int16 [P][L], the members' costs
// fp32 [P] and insertion stamps born int32 [P] (distinct; a fresh pool has born[j] = j), the best
// solution seen and its cost.  Island g = island_base + i is GLOBAL; iteration `it` of
// [it_begin, it_begin + iters), every fp32 operation rounded on its own:
//   1. tournament: k = select distinct slots.  Draw j = 0..k-1 takes
//      t = min((int)(u_j (float)(P - j)), P - j - 1) and picks the t-th slot, slots ascending, that
//      no earlier draw picked; u_j is word j & 3 of Philox(seed ^ EO_SEL_KEY, 16 it + (j >> 2), g).
//      The picked set is a 64-bit mask in registers.  The winner is the picked slot of smallest
//      cost, ties to the earlier draw;
//   2. clone and mutate: attempt t = 0..EO_MAX_TRY-1 draws Philox(seed ^ GA_MUT_KEY, 16 it + t, g),
//      word x the position, word y the value, and applies the domain's mutation (that of its island
//      GA kernel) to the clone of the winner; an attempt that leaves the whole clone invalid is
//      taken back, the first valid attempt is the child.  Without one the iteration inserts
//      nothing and counts in `stalls`;
//   3. the child is priced from scratch by the domain's price function;
//   4. purge: a_j = the number of members with an older stamp than member j,
//      age_j = ((float)(P - a_j) age_scale) / (float)P, fin_j = cost_j when finite, else 1e30,
//      aggr_j = w fin_j + (1 - w) age_j; the victim has the largest aggr, ties to the oldest.  The
//      child takes the victim's slot with stamp P + it (`inserted`);
//   5. a child cost strictly below best_cost replaces the best (`improved`);
//      hist[i][it - it_begin] = the island's best cost after the iteration.
// 2 <= P <= 64, 1 <= select <= P, it_begin + iters + P < 2^31.  A run cut into segments through
// the state equals one run.  optimize/eo.py::eo_islands_reference is the frame's bit-exact host twin.
//
// Assignments and meetings (eo_assign_kernel, eo_meeting_kernel; subsets: eo_subset_kernel below):
// one island per lane, one wave per workgroup carrying IW islands: the pool, the clone, the costs
// and the age ranks a_j are columns `lane` of [.][IW] LDS tiles (lane-private; no private array is
// indexed at run time).  IW is the largest of 64, 32, ..., 1 whose columns fit 64 KiB
// (avk::eo_assign_plan / eo_meeting_plan): big pools leave lanes idle.  The ranks are kept
// incrementally (an insert lowers the ranks above the victim's by one, the child gets P - 1), so an
// iteration scans the pool once for the tournament and once for the purge; stamps are only read
// at the start and written to global memory at an insert, as is the best solution at an improvement.
constexpr int EO_MAX_TRY = 5;  // the reference's maxTry
constexpr unsigned long long EO_SEL_KEY = 0xA0761D6478BD642Full;

struct EoArgs {
  int I, P, iters, select, it_begin;
  float w, age_scale;
  unsigned long long seed;
  long long island_base;
};

struct EoIsland {  // what an island carries besides its pool
  float bc;
  unsigned long long inserted, stalls, improved;
};

// position of the t-th (from 0) set bit of m, which has more than t set bits
__device__ __forceinline__ int eo_nth_set(unsigned long long m, int t) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w; w >>= 1) {
    const int c = __popcll(m & ((1ull << w) - 1ull));
    if (t >= c) {
      t -= c;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

// Step 4's score of a member of cost c and age rank a, each operation rounded on its own
__device__ __forceinline__ float eo_aggr(const EoArgs& A, float c, int a) {
#pragma clang fp contract(off)
  const float fin = isfinite(c) ? c : 1e30f;
  const float num = (float)(A.P - a) * A.age_scale;
  const float age = num / (float)A.P;
  const float x = A.w * fin, y = (1.f - A.w) * age;
  return x + y;
}

// a_j of member j from the island's stamps
__device__ __forceinline__ int eo_rank(const int* __restrict__ gborn, int P, int j) {
  const int bj = gborn[j];
  int a = 0;
  for (int i = 0; i < P; ++i) a += gborn[i] < bj;
  return a;
}

// A pool whose costs pc[j * IW] and age ranks rk[j * IW] are lane-private LDS columns (the island of
// a lane): the purge is two scans of the P members.
template <int IW>
struct EoColumns {
  float* pc;
  short* rk;
  int* gborn;  // the island's row of born
  __device__ __forceinline__ void init(const EoArgs& A) {
    for (int j = 0; j < A.P; ++j) rk[j * IW] = (short)eo_rank(gborn, A.P, j);
  }
  __device__ __forceinline__ float cost(int slot) const { return pc[slot * IW]; }
  // the child of cost cc replaces the victim; returns the victim's slot
  __device__ __forceinline__ int purge(const EoArgs& A, float cc, int it) {
    const int P = A.P;
    int vic = 0, vr = 0;
    float va = 0.f;
    for (int j = 0; j < P; ++j) {
      const int a = rk[j * IW];
      const float aggr = eo_aggr(A, pc[j * IW], a);
      if (j == 0 || aggr > va || (aggr == va && a < vr)) {
        va = aggr;
        vr = a;
        vic = j;
      }
    }
    for (int j = 0; j < P; ++j) {
      const int a = rk[j * IW];
      if (a > vr) rk[j * IW] = (short)(a - 1);
    }
    rk[vic * IW] = (short)(P - 1);
    pc[vic * IW] = cc;
    gborn[vic] = P + it;
    return vic;
  }
};

// The iterations of one island.  `pool` holds the members' costs and age ranks (EoColumns, EoLanes):
// cost(slot), and purge(A, cc, it) -> the victim's slot.  clone(j): member j -> the clone;
// mutate(x, y): one attempt on the clone; valid(): is the clone valid now; undo(): take the attempt
// back; price(ok) -> the clone's cost: every thread calls it every iteration (it may hold
// barriers), its value counts only where ok; insert(j): the clone -> slot j; improved(): the clone
// is the new best.  An island that is not `live` only keeps price's barriers; `lead` marks the one
// thread of an island that writes its row ghist of hist.
template <class Pool, class Clone, class Mutate, class Valid, class Undo, class Price, class Insert, class Improved>
__device__ __forceinline__ void eo_island(const EoArgs& A, unsigned long long g, bool live, bool lead, EoIsland& S,
                                          Pool& pool, float* __restrict__ ghist, Clone clone, Mutate mutate,
                                          Valid valid, Undo undo, Price price, Insert insert, Improved improved) {
  const int P = A.P;
  const unsigned long long all = P == 64 ? ~0ull : (1ull << P) - 1ull;
  for (int k = 0; k < A.iters; ++k) {
    const int it = A.it_begin + k;
    bool ok = false;
    if (live) {
      // 1. tournament
      unsigned long long free = all;
      av::u4 R{0, 0, 0, 0};
      int win = 0;
      float wc = 0.f;
      for (int j = 0; j < A.select; ++j) {
        const int q = j & 3;
        if (q == 0)
          R = av::philox_draw(A.seed ^ EO_SEL_KEY, 16ull * (unsigned long long)it + (unsigned long long)(j >> 2), g);
        const unsigned word = q == 0 ? R.x : q == 1 ? R.y : q == 2 ? R.z : R.w;
        const int n = P - j;
        const int t = min((int)(av::u32_to_unit(word) * (float)n), n - 1);
        const int slot = eo_nth_set(free, t);
        free &= ~(1ull << slot);
        const float c = pool.cost(slot);
        if (j == 0 || c < wc) {
          wc = c;
          win = slot;
        }
      }
      // 2. clone and mutate
      clone(win);
      for (int t = 0; t < EO_MAX_TRY && !ok; ++t) {
        const av::u4 Q = av::philox_draw(A.seed ^ GA_MUT_KEY, 16ull * (unsigned long long)it + (unsigned long long)t, g);
        mutate(Q.x, Q.y);
        ok = valid();
        if (!ok) undo();
      }
    }
    // 3. price
    const float cc = price(ok);
    if (ok) {
      // 4. purge
      insert(pool.purge(A, cc, it));
      ++S.inserted;
      // 5. best
      if (cc < S.bc) {
        S.bc = cc;
        improved();
        ++S.improved;
      }
    } else if (live) {
      ++S.stalls;
    }
    if (lead) ghist[k] = S.bc;
  }
}

__device__ __forceinline__ void eo_report(unsigned long long* __restrict__ stats, const EoIsland& S) {
  if (S.inserted) atomicAdd(&stats[0], S.inserted);
  if (S.stalls) atomicAdd(&stats[1], S.stalls);
  if (S.improved) atomicAdd(&stats[2], S.improved);
}

// bytes of the lane-private columns of one island: costs, (meetings: start seconds and day bits,)
// age ranks, pool and clone — the 4-byte arrays first, so every array is aligned at any IW
__host__ __device__ constexpr size_t eo_island_bytes(size_t P, size_t L, size_t M) {
  return 4 * P + 8 * M + 2 * P + 2 * P * L + 2 * L;
}

// Assignments: the mutation of ga_assign_kernel (one position to a different value; with `swap` the
// first other position holding that value takes the old one), ga_valid and ga_price on the clone's
// column.  A child is valid when it is priced, so ga_price runs without the conflict table.
template <int IW>
__global__ __launch_bounds__(64) void eo_assign_kernel(
    const float* __restrict__ cost, int L, int V, const uint8_t* __restrict__ conflict, int swap,
    short* __restrict__ pop, float* __restrict__ pop_cost, int* __restrict__ born, short* __restrict__ best,
    float* __restrict__ best_cost, float* __restrict__ hist, unsigned long long* __restrict__ stats, EoArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eo_lds[];
  const int lane = threadIdx.x, P = A.P;
  const long long i = (long long)blockIdx.x * IW + lane;
  if (lane >= IW || i >= A.I) return;
  float* pc = reinterpret_cast<float*>(eo_lds) + lane;                    // cost of member j at pc[j * IW]
  short* rk = reinterpret_cast<short*>(eo_lds + (size_t)4 * P * IW) + lane;
  short* pl = rk + (size_t)P * IW;                                        // element l of member j at pl[(j L + l) IW]
  short* c = pl + (size_t)P * L * IW;                                     // the clone
  short* gpop = pop + i * P * L;
  short* gbest = best + i * L;
  for (int e = 0; e < P * L; ++e) pl[e * IW] = gpop[e];
  for (int j = 0; j < P; ++j) pc[j * IW] = pop_cost[i * P + j];
  EoIsland S{best_cost[i], 0, 0, 0};
  const float invL = 1.f / (float)L;
  int pos = 0, old = 0, v = 0, holder = -1;
  EoColumns<IW> pool{pc, rk, born + i * P};
  pool.init(A);
  eo_island(
      A, (unsigned long long)(A.island_base + i), true, true, S, pool, hist + i * A.iters,
      [&](int j) {
        for (int l = 0; l < L; ++l) c[l * IW] = pl[(j * L + l) * IW];
      },
      [&](unsigned qp, unsigned qv) {
        pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
        old = c[pos * IW];
        v = min((int)(av::u32_to_unit(qv) * (float)(V - 1)), V - 2);
        v += v >= old;
        holder = -1;
        if (swap)
          for (int j = 0; j < L; ++j)
            if (j != pos && c[j * IW] == v) { holder = j; break; }
        if (holder >= 0) c[holder * IW] = (short)old;
        c[pos * IW] = (short)v;
      },
      [&] { return ga_valid<IW>(c, L, conflict); },
      [&] {
        c[pos * IW] = (short)old;
        if (holder >= 0) c[holder * IW] = (short)v;
      },
      [&](bool ok) { return ok ? ga_price<IW>(c, L, V, cost, nullptr, invL, 0.f) : 0.f; },
      [&](int j) {
        for (int l = 0; l < L; ++l) pl[(j * L + l) * IW] = c[l * IW];
      },
      [&] {
        for (int l = 0; l < L; ++l) gbest[l] = c[l * IW];
      });
  for (int e = 0; e < P * L; ++e) gpop[e] = pl[e * IW];
  for (int j = 0; j < P; ++j) pop_cost[i * P + j] = pc[j * IW];
  best_cost[i] = S.bc;
  eo_report(stats, S);
}

// Meeting schedules: the mutation of ga_meeting_kernel (one index to a different value of its table,
// a one-value table leaves the clone alone), mt_valid and mt_cost on the clone's start seconds and
// day bits, two more lane-private columns; the domain is staged in front of the columns.
template <int IW>
__global__ __launch_bounds__(64) void eo_meeting_kernel(
    avk::GaMeetingDomain dom, short* __restrict__ pop, float* __restrict__ pop_cost, int* __restrict__ born,
    short* __restrict__ best, float* __restrict__ best_cost, float* __restrict__ hist,
    unsigned long long* __restrict__ stats, EoArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char eo_lds[];
  const int lane = threadIdx.x, P = A.P, M = dom.M, L = 3 * M;
  const MtLds D = mt_stage(dom, reinterpret_cast<int*>(eo_lds), lane);
  __syncthreads();
  const long long i = (long long)blockIdx.x * IW + lane;
  if (lane >= IW || i >= A.I) return;
  unsigned char* at = eo_lds + (size_t)MT_DOM_INTS * sizeof(int);
  float* pc = reinterpret_cast<float*>(at) + lane;                        at += (size_t)4 * P * IW;
  int* st = reinterpret_cast<int*>(at) + lane;                            at += (size_t)4 * M * IW;
  unsigned* db = reinterpret_cast<unsigned*>(at) + lane;                  at += (size_t)4 * M * IW;
  short* rk = reinterpret_cast<short*>(at) + lane;
  short* pl = rk + (size_t)P * IW;
  short* c = pl + (size_t)P * L * IW;
  short* gpop = pop + i * P * L;
  short* gbest = best + i * L;
  for (int e = 0; e < P * L; ++e) pl[e * IW] = gpop[e];
  for (int j = 0; j < P; ++j) pc[j * IW] = pop_cost[i * P + j];
  EoIsland S{best_cost[i], 0, 0, 0};
  int pos = 0, mi = 0, card = 0, old = 0;
  auto put = [&](int v) {
    if (card > 1) {
      c[pos * IW] = (short)v;
      mt_place<IW>(D, c, mi, st, db);
    }
  };
  EoColumns<IW> pool{pc, rk, born + i * P};
  pool.init(A);
  eo_island(
      A, (unsigned long long)(A.island_base + i), true, true, S, pool, hist + i * A.iters,
      [&](int j) {
        for (int l = 0; l < L; ++l) c[l * IW] = pl[(j * L + l) * IW];
        for (int m = 0; m < M; ++m) mt_place<IW>(D, c, m, st, db);
      },
      [&](unsigned qp, unsigned qv) {
        pos = min((int)(av::u32_to_unit(qp) * (float)L), L - 1);
        mi = pos / 3;
        const int comp = pos - 3 * mi;
        card = comp == 0 ? dom.nd : comp == 1 ? dom.nh : dom.nm;
        old = c[pos * IW];
        int v = min((int)(av::u32_to_unit(qv) * (float)(card - 1)), card - 2);
        v += v >= old;
        put(v);
      },
      [&] { return mt_valid<IW>(D, st); },
      [&] { put(old); },
      [&](bool ok) { return ok ? mt_cost<IW>(D, db) : 0.f; },
      [&](int j) {
        for (int l = 0; l < L; ++l) pl[(j * L + l) * IW] = c[l * IW];
      },
      [&] {
        for (int l = 0; l < L; ++l) gbest[l] = c[l * IW];
      });
  for (int e = 0; e < P * L; ++e) gpop[e] = pl[e * IW];
  for (int j = 0; j < P; ++j) pop_cost[i * P + j] = pc[j * IW];
  best_cost[i] = S.bc;
  eo_report(stats, S);
}

// A pool held by a wave, one member per lane (lane j < P: mask, cost and age rank in registers).
// Every lane of the wave follows the same island, so slots and costs are wave-uniform: a member's
// cost is one v_readlane, and the victim is the wave minimum of an order-preserving 64-bit key —
// the complement of aggr's key above the rank and the lane, so the largest aggr wins, ties to the
// oldest.  All 64 lanes must be active in purge.
struct EoLanes {
  unsigned mk;
  float c;
  int a, lane;
  int* gborn;  // the island's row of born; written by the island's leading wave
  bool writer;
  __device__ __forceinline__ float cost(int slot) const {
    return av::lane_f(c, __builtin_amdgcn_readfirstlane(slot));
  }
  __device__ __forceinline__ int purge(const EoArgs& A, float cc, int it) {
    unsigned long long key = TB_NONE;
    if (lane < A.P)
      key = ((unsigned long long)(~tb_key(eo_aggr(A, c, a))) << 32) | ((unsigned)a << 8) | (unsigned)lane;
    key = tb_wave_min(key);
    const int vic = (int)(key & 0xffu), vr = (int)((key >> 8) & 0xffffffu);
    if (a > vr) --a;
    if (lane == vic) {
      a = A.P - 1;
      c = cc;
      if (writer) gborn[vic] = A.P + it;
    }
    return vic;
  }
};

// Feature subsets: the structure of sa_subset_kernel — workgroups of 256 or 1,024 threads whose waves
// are split into islands of w = 1..16 waves over one shared staged row tile, the clone's mask in a
// scalar register, ballot counts meeting in the three-deep integer LDS counter (one barrier per tile
// and iteration).  The pool is an EoLanes in every wave of the island: all of them draw the same
// Philox words and see the same counts, so the copies stay equal without LDS or a further barrier.
// A mutation flips one bit (the value word is unused); valid: min_size <= popcount <= max_size;
// cost = (float)errors / (float)N.  pop, best stay int16 0 / 1 rows at the interface.
__global__ __launch_bounds__(1024) void eo_subset_kernel(
    const float* __restrict__ LL, const float* __restrict__ log_prior, const int* __restrict__ labels, int N, int F,
    int C, int min_size, int max_size, short* __restrict__ pop, float* __restrict__ pop_cost, int* __restrict__ born,
    short* __restrict__ best, float* __restrict__ best_cost, float* __restrict__ hist,
    unsigned long long* __restrict__ stats, EoArgs A, int TR, int w) {
  extern __shared__ __attribute__((aligned(16))) float fs_tile[];
  __shared__ float s_prior[FS_MAX_C];
  __shared__ int s_cnt[3][SA_FS_MAX_CHAINS];
  const int tid = threadIdx.x, nt = blockDim.x, FC = F * C, stride = FC | 1, P = A.P;
  const unsigned magic = 0xFFFFFFFFu / (unsigned)FC + 1u;
  const int ntiles = (N + TR - 1) / TR;
  int* s_lab = reinterpret_cast<int*>(fs_tile + (size_t)TR * stride);  // [TR] labels of the staged rows
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wsh = __ffs(w) - 1, ci = wave >> wsh, sub = wave & (w - 1), cpw = (nt >> 6) >> wsh;
  const long long p = (long long)blockIdx.x * cpw + ci;
  const bool live = p < A.I;
  if (tid < C) s_prior[tid] = log_prior[tid];
  if (tid < 3 * SA_FS_MAX_CHAINS) (&s_cnt[0][0])[tid] = 0;
  EoLanes pool{0u, 0.f, 0, lane, nullptr, false};
  EoIsland S{0.f, 0, 0, 0};
  unsigned bmk = 0, cand = 0;
  if (live) {
    pool.gborn = born + p * P;
    pool.writer = sub == 0;
    if (lane < P) {
      const short* row = pop + (p * P + lane) * F;
      for (int f = 0; f < F; ++f) pool.mk |= (unsigned)(row[f] != 0) << f;
      pool.c = pop_cost[p * P + lane];
      pool.a = eo_rank(pool.gborn, P, lane);
    }
    const bool in = lane < F;
    bmk = (unsigned)__ballot(in && best[p * F + (in ? lane : 0)] != 0);
    S.bc = best_cost[p];
  }
  __syncthreads();
  bool staged = false;
  int k = 0;  // iteration of this launch
  int pos = 0;
  eo_island(
      A, (unsigned long long)(A.island_base + p), live, live && sub == 0 && lane == 0, S, pool,
      hist + (live ? p : 0) * A.iters,
      [&](int j) { cand = (unsigned)__builtin_amdgcn_readlane((int)pool.mk, __builtin_amdgcn_readfirstlane(j)); },
      [&](unsigned qp, unsigned) {
        pos = min((int)(av::u32_to_unit(qp) * (float)F), F - 1);
        cand = (unsigned)__builtin_amdgcn_readfirstlane((int)(cand ^ (1u << pos)));
      },
      [&] {
        const int sz = __popc(cand);
        return sz >= min_size && sz <= max_size;
      },
      [&] { cand = (unsigned)__builtin_amdgcn_readfirstlane((int)(cand ^ (1u << pos))); },
      [&](bool ok) {  // the scoring of sa_subset_kernel's price
        int* cnt = s_cnt[k % 3];
        if (tid < SA_FS_MAX_CHAINS) s_cnt[(k + 1) % 3][tid] = 0;
        ++k;
        int n = 0;
        for (int t = 0; t < ntiles; ++t) {
          const long long n0 = (long long)t * TR;
          const int nr = min(TR, N - (int)n0);
          if (ntiles > 1 || !staged) {
            fs_stage(fs_tile, LL, n0, nr, FC, stride, magic, tid, nt);
            for (int e = tid; e < nr; e += nt) s_lab[e] = labels[n0 + e];
            staged = true;
            __syncthreads();
          }
          if (ok) {
            const int ng = (nr + 63) >> 6;
            for (int gq = sub; gq < ng; gq += w) {
              const int row = gq * 64 + lane;
              const int rr = min(row, nr - 1);  // lanes past the tile score its last row, uncounted
              const bool miss = fs_row_miss_uniform(fs_tile + rr * stride, s_prior, C, cand, s_lab[rr]);
              n += __popcll(__ballot(miss && row < nr));
            }
            if (t == ntiles - 1 && lane == 0 && n) atomicAdd(&cnt[ci], n);
          }
          __syncthreads();  // the counts are in; the tile may be staged again
        }
        return (float)__builtin_amdgcn_readfirstlane(cnt[ci]) / (float)N;
      },
      [&](int j) {
        if (lane == j) pool.mk = cand;
      },
      [&] { bmk = cand; });
  if (live && sub == 0) {
    if (lane < P) {
      short* row = pop + (p * P + lane) * F;
      for (int f = 0; f < F; ++f) row[f] = (short)((pool.mk >> f) & 1u);
      pop_cost[p * P + lane] = pool.c;
    }
    if (lane < F) best[p * F + lane] = (short)((bmk >> lane) & 1u);
    if (lane == 0) {
      best_cost[p] = S.bc;
      eo_report(stats, S);
    }
  }
}

}  // namespace

namespace avk {

// one lane per member, per child and, when the children join the pool, per candidate
void ga_check_pool(const char* who, long long P, long long m, long long r, bool purge_first) {
  if (P < 2 || P > 64 || r < 1 || 2 * r > 64 || r > P || m < 1 || m > P)
    throw std::invalid_argument(std::string(who) + ": 2 <= P <= 64, 1 <= r <= min(P, 32), 1 <= m <= P");
  if (!purge_first && P + r > 64)
    throw std::invalid_argument(std::string(who) + ": P + r <= 64 when children join the pool");
}

size_t ga_assign_lds(int P, int L, int r) { return GaPool<short>::bytes(P, L, r); }

void ga_assign(const float* cost, int L, int V, const uint8_t* conflict, float invalid, short* pop, float* pop_cost,
               float* hist, int islands, int P, int G, int m, int r, int purge_first, int mutate, int swap,
               unsigned long long seed, long long island_base, unsigned long long gen_base, hipStream_t stream) {
  if (islands <= 0 || G <= 0) return;
  if (L < 1 || V < 2) throw std::invalid_argument("ga_assign: L >= 1, V >= 2");
  ga_check_pool("ga_assign", P, m, r, purge_first);
  const size_t lds = ga_assign_lds(P, L, r);
  if (lds > 64 * 1024) throw std::invalid_argument("ga_assign: pool, children and costs exceed 64 KiB of LDS");
  ga_assign_kernel<<<islands, 64, lds, stream>>>(cost, L, V, conflict, invalid, swap, pop, pop_cost, hist,
                                                 GaArgs{P, G, m, r, purge_first, mutate, seed, island_base, gen_base});
  AV_HIP_CHECK(hipGetLastError());
}

size_t ga_meeting_lds(int P, int L, int r) {
  const size_t Ms = (size_t)(L / 3) | 1;
  return GaPool<short>::bytes(P, L, r) + 2 * ga_a16((size_t)2 * r * Ms * sizeof(int)) +
         ga_a16((size_t)MT_DOM_INTS * sizeof(int));
}

// the limits of the meeting-schedule kernels (what mt_stage keeps in LDS)
static void mt_check(const char* who, const GaMeetingDomain& dom) {
  if (dom.M < 1 || dom.M > MT_MAX_M || dom.Q < 1 || dom.Q > MT_MAX_Q)
    throw std::invalid_argument(std::string(who) + ": 1 <= M <= 32, 1 <= Q <= 256");
  if (dom.nd < 1 || dom.nd > MT_MAX_CARD || dom.nh < 1 || dom.nh > MT_MAX_CARD || dom.nm < 1 || dom.nm > MT_MAX_CARD)
    throw std::invalid_argument(std::string(who) + ": value tables of 1..32 entries");
  if (dom.nb < 0 || dom.nb > MT_MAX_LIST || dom.no < 0 || dom.no > MT_MAX_LIST)
    throw std::invalid_argument(std::string(who) + ": at most 16 blocked entries and 16 ordered pairs");
}

void ga_meeting(const GaMeetingDomain& dom, float invalid, short* pop, float* pop_cost, float* hist, int islands,
                int P, int G, int m, int r, int purge_first, int mutate, unsigned long long seed,
                long long island_base, unsigned long long gen_base, hipStream_t stream) {
  mt_check("ga_meeting", dom);
  ga_check_pool("ga_meeting", P, m, r, purge_first);
  const size_t lds = ga_meeting_lds(P, 3 * dom.M, r);
  if (lds > 64 * 1024) throw std::invalid_argument("ga_meeting: pool, children and costs exceed 64 KiB of LDS");
  if (islands <= 0 || G <= 0) return;
  ga_meeting_kernel<<<islands, 64, lds, stream>>>(dom, invalid, pop, pop_cost, hist,
                                                  GaArgs{P, G, m, r, purge_first, mutate, seed, island_base, gen_base});
  AV_HIP_CHECK(hipGetLastError());
}

static void fs_check(int N, int F, int C, const char* who) {
  if (F < 1 || F > 32 || C < 2 || C > FS_MAX_C || N < 1 || N >= (1 << 24))
    throw std::invalid_argument(std::string(who) + ": 1 <= F <= 32, 2 <= C <= 16, 1 <= N < 2^24");
}

int ga_subset_threads(int N) { return N > 2048 ? 1024 : 256; }

size_t ga_subset_lds(int N, int F, int C) {
  const int FC = F * C;
  return (size_t)fs_tile_rows(FC, ga_subset_threads(N)) * (FC | 1) * sizeof(float);
}

void subset_errors(const float* LL, const float* log_prior, const int* labels, int N, int F, int C,
                   const unsigned* masks, int B, int* out, hipStream_t stream) {
  fs_check(N, F, C, "subset_errors");
  if (B <= 0) return;
  AV_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)B * sizeof(int), stream));
  const int FC = F * C, TR = fs_tile_rows(FC, 256);
  const int ntiles = (N + TR - 1) / TR;
  const size_t lds = (size_t)TR * (FC | 1) * sizeof(float);
  // about 1,024 workgroups: row tiles first, then chunks of at least 16 masks
  const int gx = std::min(ntiles, 1024);
  const int mchunk = std::min(FS_MASK_CHUNK, std::max(16, (B + 1024 / gx - 1) / (1024 / gx)));
  const int gy = std::min((B + mchunk - 1) / mchunk, 1024);
  subset_errors_kernel<<<dim3(gx, gy), 256, lds, stream>>>(LL, log_prior, labels, N, F, C, masks, B, out, TR, mchunk);
  AV_HIP_CHECK(hipGetLastError());
}

void ga_subset(const float* LL, const float* log_prior, const int* labels, int N, int F, int C, int min_size,
               int max_size, float invalid, short* pop, float* pop_cost, float* hist, int islands, int P, int G, int m,
               int r, int purge_first, int mutate, unsigned long long seed, long long island_base,
               unsigned long long gen_base, hipStream_t stream) {
  fs_check(N, F, C, "ga_subset");
  ga_check_pool("ga_subset", P, m, r, purge_first);
  if (islands <= 0 || G <= 0) return;
  const int FC = F * C, nt = ga_subset_threads(N), TR = fs_tile_rows(FC, nt);
  const size_t lds = (size_t)TR * (FC | 1) * sizeof(float);
  ga_subset_kernel<<<islands, nt, lds, stream>>>(LL, log_prior, labels, N, F, C, min_size, max_size, invalid, pop,
                                                 pop_cost, hist,
                                                 GaArgs{P, G, m, r, purge_first, mutate, seed, island_base, gen_base}, TR);
  AV_HIP_CHECK(hipGetLastError());
}

static SaArgs sa_args(const char* who, const SaRun& r, int P) {
  if (r.iters < 0 || r.it_begin < 0 || r.max_retry < 0 || r.max_retry >= (1 << 20) ||
      r.it_begin + r.iters >= (1LL << 40))
    throw std::invalid_argument(std::string(who) + ": 0 <= max_retry < 2^20, 0 <= it_begin, iters, it_begin + iters < 2^40");
  return SaArgs{P, r.iters, r.it_begin, r.t0, r.cool, r.interval, r.geometric, r.max_retry, r.seed, r.offset,
                r.temp_start, r.chain_base};
}

void sa_assign(const float* cost, int L, int V, const uint8_t* conflict, int swap, short* sol, float* cur_cost,
               short* best_sol, float* best_cost, int P, const SaRun& run, unsigned long long* stats,
               hipStream_t stream) {
  if (L < 1 || L > 512 || V < 2 || V > 32767)
    throw std::invalid_argument("sa_assign: 1 <= L <= 512 (the [L][64] solution tile is 64 KiB of LDS), 2 <= V <= 32767");
  const SaArgs A = sa_args("sa_assign", run, P);
  if (A.it_begin + A.iters >= (1LL << 31) || A.interval != (int)A.interval)
    throw std::invalid_argument("sa_assign: it_begin + iters and interval must fit 31 bits (the kernel's move counter)");
  if (P <= 0 || run.iters <= 0) return;
  const size_t lds = (size_t)L * 64 * sizeof(short);
  sa_assign_kernel<<<(P + 63) / 64, 64, lds, stream>>>(
      cost, L, V, conflict, swap, sol, cur_cost, best_sol, best_cost, P, (int)A.iters, A.t0, A.cool, (int)A.interval,
      A.geometric, A.max_retry, A.seed, A.offset, (int)A.it_begin, A.temp_start, stats, A.chain_base);
  AV_HIP_CHECK(hipGetLastError());
}

size_t sa_meeting_lds(int M) {
  return (size_t)3 * M * 64 * sizeof(short) + (size_t)2 * M * 64 * sizeof(int) + (size_t)MT_DOM_INTS * sizeof(int);
}

void sa_meeting(const GaMeetingDomain& dom, short* sol, float* cur_cost, short* best_sol, float* best_cost, int P,
                const SaRun& run, unsigned long long* stats, hipStream_t stream) {
  mt_check("sa_meeting", dom);
  const SaArgs A = sa_args("sa_meeting", run, P);
  const size_t lds = sa_meeting_lds(dom.M);
  if (lds > 64 * 1024) throw std::invalid_argument("sa_meeting: the chains' tiles exceed 64 KiB of LDS");
  if (P <= 0 || run.iters <= 0) return;
  sa_meeting_kernel<<<(P + 63) / 64, 64, lds, stream>>>(dom, sol, cur_cost, best_sol, best_cost, stats, A);
  AV_HIP_CHECK(hipGetLastError());
}

// Workgroup size, waves per chain and tile rows of sa_subset.  Auto (waves_per_chain = 0): every
// chain starts with all waves of its workgroup and w halves until at most 512 workgroups remain,
// so few chains get many waves each and many chains share their tiles.
SaSubsetPlan sa_subset_plan(int N, int F, int C, int P, int waves_per_chain) {
  int nt = ga_subset_threads(N), w = waves_per_chain;
  if (w == 0) {
    w = nt / 64;
    while (w > 1 && (long long)P * w / (nt / 64) > 512) w >>= 1;
  } else {
    if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16)
      throw std::invalid_argument("sa_subset: waves_per_chain must be 0 (auto), 1, 2, 4, 8 or 16");
    if (w > nt / 64) nt = 1024;
  }
  const int FC = F * C, TR = fs_tile_rows(FC, nt), cpw = nt / 64 / w;
  return SaSubsetPlan{nt, w, TR, (P + cpw - 1) / cpw, (size_t)TR * (FC | 1) * sizeof(float) + (size_t)TR * sizeof(int)};
}

void sa_subset(const float* LL, const float* log_prior, const int* labels, int N, int F, int C, int min_size,
               int max_size, short* sol, float* cur_cost, short* best_sol, float* best_cost, int P, const SaRun& run,
               unsigned long long* stats, int waves_per_chain, hipStream_t stream) {
  fs_check(N, F, C, "sa_subset");
  const SaArgs A = sa_args("sa_subset", run, P);
  const SaSubsetPlan pl = sa_subset_plan(N, F, C, std::max(P, 1), waves_per_chain);
  if (pl.lds > 56 * 1024) throw std::invalid_argument("sa_subset: the row tile exceeds its LDS");
  if (P <= 0 || run.iters <= 0) return;
  sa_subset_kernel<<<pl.grid, pl.threads, pl.lds, stream>>>(LL, log_prior, labels, N, F, C, min_size, max_size, sol,
                                                           cur_cost, best_sol, best_cost, stats, A, pl.rows, pl.waves);
  AV_HIP_CHECK(hipGetLastError());
}

// 4, 2 or 1 chains (waves) per workgroup beside one shared copy of the cost and conflict tables;
// one chain per workgroup without the copy where even that does not fit
TabuPlan tabu_assign_plan(int L, int V) {
  const size_t per = tb_chain_bytes(L, V), shared = tb_shared_bytes(L, V);
  for (int w = 4; w >= 1; w >>= 1)
    if (w * per + shared <= TABU_LDS_LIMIT) return TabuPlan{w, 1, w * per + shared};
  return TabuPlan{1, 0, per};
}

size_t tabu_assign_lds(int L, int V) { return tabu_assign_plan(L, V).lds; }

void tabu_assign(const float* cost, int L, int V, const uint8_t* conflict, short* sol, float* cur_cost,
                 short* best_sol, float* best_cost, int* tabu, float* hist, int P, long long iters, long long it_begin,
                 long long tenure, unsigned long long* stats, hipStream_t stream) {
  if (L < 1 || V < 1 || V > 32767) throw std::invalid_argument("tabu_assign: L >= 1, 1 <= V <= 32767");
  if (iters < 0 || it_begin < 0 || tenure < 0 || it_begin + iters + tenure >= (1LL << 31))
    throw std::invalid_argument("tabu_assign: 0 <= iters, it_begin, tenure and it_begin + iters + tenure < 2^31");
  const TabuPlan pl = tabu_assign_plan(L, V);
  if (pl.lds > TABU_LDS_LIMIT) throw std::invalid_argument("tabu_assign: a chain's tables exceed 64 KiB of LDS");
  if (P <= 0 || iters == 0) return;
  const int grid = (P + pl.waves - 1) / pl.waves;
  if (pl.staged)
    tabu_assign_kernel<true><<<grid, 64 * pl.waves, pl.lds, stream>>>(cost, L, V, conflict, sol, cur_cost, best_sol,
                                                                     best_cost, tabu, hist, P, (int)iters,
                                                                     (int)it_begin, (int)tenure, stats);
  else
    tabu_assign_kernel<false><<<grid, 64 * pl.waves, pl.lds, stream>>>(cost, L, V, conflict, sol, cur_cost, best_sol,
                                                                      best_cost, tabu, hist, P, (int)iters,
                                                                      (int)it_begin, (int)tenure, stats);
  AV_HIP_CHECK(hipGetLastError());
}

// IW = the largest of 64, 32, ..., 1 islands per wave whose columns fit beside `shared` bytes;
// IW = 0 (no kernel) when one island does not fit
static EoPlan eo_plan(size_t per, size_t shared) {
  for (int iw = 64; iw >= 1; iw >>= 1)
    if (shared + iw * per <= EO_LDS_LIMIT) return EoPlan{iw, shared + iw * per};
  return EoPlan{0, shared + per};
}

EoPlan eo_assign_plan(int P, int L) { return eo_plan(eo_island_bytes(P, L, 0), 0); }

EoPlan eo_meeting_plan(int P, int M) {
  return eo_plan(eo_island_bytes(P, 3 * (size_t)M, M), (size_t)MT_DOM_INTS * sizeof(int));
}

static EoArgs eo_args(const char* who, const EoRun& r, int I, int P) {
  if (P < 2 || P > 64 || r.select < 1 || r.select > P)
    throw std::invalid_argument(std::string(who) + ": 2 <= P <= 64, 1 <= select <= P");
  if (r.iters < 0 || r.it_begin < 0 || r.iters >= (1LL << 31) || r.it_begin >= (1LL << 31) ||
      r.it_begin + r.iters + P >= (1LL << 31))
    throw std::invalid_argument(std::string(who) + ": 0 <= iters, it_begin and it_begin + iters + P < 2^31");
  if (!(r.w >= 0.f && r.w <= 1.f) || !(r.age_scale >= 0.f && r.age_scale < INFINITY))
    throw std::invalid_argument(std::string(who) + ": 0 <= w <= 1, 0 <= age_scale < inf");
  return EoArgs{I, P, (int)r.iters, r.select, (int)r.it_begin, r.w, r.age_scale, r.seed, r.island_base};
}

// f(std::integral_constant<int, IW>) for the plan's IW
template <class F>
static void eo_with_iw(int iw, F f) {
  switch (iw) {
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
}

void eo_assign(const float* cost, int L, int V, const uint8_t* conflict, int swap, short* pop, float* pop_cost,
               int* born, short* best, float* best_cost, float* hist, unsigned long long* stats, int I, int P,
               const EoRun& run, hipStream_t stream) {
  if (L < 1 || V < 2 || V > 32767) throw std::invalid_argument("eo_assign: L >= 1, 2 <= V <= 32767");
  const EoArgs A = eo_args("eo_assign", run, I, P);
  const EoPlan pl = eo_assign_plan(P, L);
  if (!pl.islands) throw std::invalid_argument("eo_assign: an island's pool exceeds 64 KiB of LDS");
  if (I <= 0 || run.iters == 0) return;
  eo_with_iw(pl.islands, [&](auto iw) {
    constexpr int IW = decltype(iw)::value;
    eo_assign_kernel<IW><<<(I + IW - 1) / IW, 64, pl.lds, stream>>>(cost, L, V, conflict, swap, pop, pop_cost, born,
                                                                    best, best_cost, hist, stats, A);
  });
  AV_HIP_CHECK(hipGetLastError());
}

void eo_meeting(const GaMeetingDomain& dom, short* pop, float* pop_cost, int* born, short* best, float* best_cost,
                float* hist, unsigned long long* stats, int I, int P, const EoRun& run, hipStream_t stream) {
  mt_check("eo_meeting", dom);
  const EoArgs A = eo_args("eo_meeting", run, I, P);
  const EoPlan pl = eo_meeting_plan(P, dom.M);
  if (!pl.islands) throw std::invalid_argument("eo_meeting: an island's pool exceeds 64 KiB of LDS");
  if (I <= 0 || run.iters == 0) return;
  eo_with_iw(pl.islands, [&](auto iw) {
    constexpr int IW = decltype(iw)::value;
    eo_meeting_kernel<IW><<<(I + IW - 1) / IW, 64, pl.lds, stream>>>(dom, pop, pop_cost, born, best, best_cost, hist,
                                                                     stats, A);
  });
  AV_HIP_CHECK(hipGetLastError());
}

// the workgroup plan is sa_subset's: islands of `waves_per_island` waves (0: the launcher's choice)
void eo_subset(const float* LL, const float* log_prior, const int* labels, int N, int F, int C, int min_size,
               int max_size, short* pop, float* pop_cost, int* born, short* best, float* best_cost, float* hist,
               unsigned long long* stats, int I, int P, const EoRun& run, int waves_per_island, hipStream_t stream) {
  fs_check(N, F, C, "eo_subset");
  const EoArgs A = eo_args("eo_subset", run, I, P);
  const SaSubsetPlan pl = sa_subset_plan(N, F, C, std::max(I, 1), waves_per_island);
  if (pl.lds > 56 * 1024) throw std::invalid_argument("eo_subset: the row tile exceeds its LDS");
  if (I <= 0 || run.iters == 0) return;
  eo_subset_kernel<<<pl.grid, pl.threads, pl.lds, stream>>>(LL, log_prior, labels, N, F, C, min_size, max_size, pop,
                                                           pop_cost, born, best, best_cost, hist, stats, A, pl.rows,
                                                           pl.waves);
  AV_HIP_CHECK(hipGetLastError());
}

}  // namespace avk
