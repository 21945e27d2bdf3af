// sst_final.hip -- the final program by exact enumeration (gfx950): the optimal
// sequence of a spectrum, the question Predictor.predict asks its last solver
// call (prediction.py:158-166: LinearProgramInstance(...).evaluate,
// linear_program.py:164-225 the program, :238-313 its reading).  The definition
// is in include/sst.h (sst_final_program_device).
//
// For a fixed y (one row per position) the program decomposes: every fragment
// independently takes the admissible interval whose sum is nearest to its
// mass.  So the optimum is a minimum over y of a sum of per-fragment minima,
// and k_final_program enumerates y: one spectrum per workgroup, persistent grid
// with static striding over the spectra, lanes over the mixed-radix indices of y.
//
// Prologue per spectrum (LDS): one scan of the fragments for the conditions
// that make the spectrum SKIPPED; per position |A_i| and its first row; thread 0
// then walks the positions once: the prefix sums Pbase(i) with every free
// position (|A_i| > 1) at its first row, k(i) = the free positions before i, the
// free positions' radices and, per digit, the row, its mass above the first
// row's (mod 2^32: the true prefix sums are below 2^32) and whether it is
// modified; combos = prod |A_i|, saturating.  At most 22 free positions and 512
// table entries are recorded: beyond either combos > 2^22 >= max_combos (radices
// are in [2, 127], and x <= 18.2 log2(x) there, so radices of product <= 2^22 sum
// to <= 400).  Then the row-free test, one row per thread, as keep mode's.
//
// A lane decodes its index (least significant digit = last free position) into
// D[k][lane], k = 0 .. free positions: the digits' masses summed over the first
// k free positions, so that P(i) = Pbase(i) + D[k(i)][lane] is the prefix sum of
// its y (Pbase and k are shared, D is [k][lane]: a lane's column stays in one
// bank whatever k it reads).  It counts the modified rows and skips y above
// mod_cap.  The fragment records (qfix, class, ends) are held in LDS in chunks of
// kFinalF; a lane keeps its partial objective across the chunks of one pass (a
// spectrum of one chunk loads it once).  Terminal fragments walk their range of
// ends, START_END takes the total, an internal fragment is a two-pointer sweep
// over the non-decreasing prefix sums (O(L), the empty interval included: i == j).
// Every lane keeps (best, the smallest objective above it, count, first index,
// feasible count) and stops summing a y once its partial objective is above
// both (costs only add, so that y changes none of them, nor the workgroup's);
// the workgroup reduces the lanes' records by a tree in LDS.  Nothing in the
// result depends on the order of the reduction: identical calls give identical
// arrays.
//
// Epilogue: every lane decodes the winner (the same D in every column), threads
// over positions write seq, threads over fragments walk the admissible intervals
// in (l, r) order for iv and sum.  Every global store is a plain vector store of
// an output element; no global atomics, no scratch buffer.
//
// The robust variant (k_final_robust, sst_final_robust_device: the same body, kRobust): frag_use 2 marks a fragment
// the solver may still drop.  The enumeration above runs over the required fragments alone and gives y*; where the
// spectrum holds optional fragments the prefix sums P* of y* go to LDS and the enumeration runs once more over all
// used fragments, an optional one's cost capped at its cost under y* (c*_j, computed from P* by the thread that loads
// its record, on every load: nothing is kept per optional fragment).  cap(y) - cap(y*) is the smallest of obj_T(y) -
// obj_T(y*) over all subsets T of the optional fragments, so y* is the unique optimum of every obj_T iff it is of cap
// (include/sst.h).  The capped costs are non-negative terms as the plain ones: bookkeeping, early stop and order are
// the first pass's.  The extra LDS (caps, P*, two words) is an extension struct k_final_program does not instantiate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sst_internal.h"

namespace sst {

namespace {

constexpr int kFinalWG = 256;
constexpr int kFinalF = 512;        // fragment records per chunk
constexpr int kFinalMaxLen = 253;   // as the alignment certificate
constexpr int kFinalMaxFree = 22;   // free positions of a spectrum of at most 2^22 assignments
constexpr int kFinalTable = 512;    // digits of all free positions together
constexpr uint32_t kFinalMaxUsed = 16384;
constexpr uint64_t kNone64 = ~0ull;
static_assert(SST_FINAL_MAX_COMBOS == 1ull << kFinalMaxFree, "every free position has at least two rows");

struct FinalLds {
  uint32_t D[kFinalMaxFree + 1][kFinalWG];  // per lane: its digits' masses over the first k free positions
  unsigned long long r_best[kFinalWG];      // the reduction
  unsigned long long r_next[kFinalWG];
  uint32_t r_count[kFinalWG];
  uint32_t r_first[kFinalWG];
  uint32_t r_feas[kFinalWG];
  int64_t f_q[kFinalF];         // a chunk's records: qfix
  uint32_t f_meta[kFinalF];     // class | unused << 2 | first end << 8 | last end << 16
  uint32_t pbase[256];          // P(i) with every free position at its first row, i in [0, L]
  uint32_t w[SST_MAX_ROWS + 8];
  uint32_t t_delta[kFinalTable];  // per digit of a free position: its row's mass above the first row's (mod 2^32)
  uint8_t t_row[kFinalTable];
  uint8_t t_mod[kFinalTable];
  uint16_t f_off[kFinalMaxFree + 2];  // a free position's first digit in the table
  uint8_t f_radix[kFinalMaxFree + 2];
  uint8_t kof[256];             // free positions before position i, i in [0, L]
  uint8_t p_cnt[256];           // |A_i|, and its first row
  uint8_t p_first[256];
  uint8_t w_digit[kFinalMaxFree + 2];  // the winner's digits
  unsigned long long mod[2];    // the table's modified rows
  unsigned long long combos;
  uint32_t flags;               // 1: an empty A_i; 2: a SKIPPED condition among the used fragments; 4: a row is not free
  uint32_t n_used;
  uint32_t n_free;
  int32_t fixed_mod;            // modified rows among the positions of one row
};
static_assert(sizeof(FinalLds) <= 64 * 1024, "static LDS");

// The robust variant's extension: k_final_program does not instantiate it.
struct FinalRobustLds : FinalLds {
  unsigned long long f_cap[kFinalF];  // a chunk's records: c*_j of an optional record, kNone64 of a required one
  uint32_t pstar[256];                // P*(i): the prefix sums of y*, i in [0, L]
  unsigned long long cstar;           // the sum of c*_j over the optional fragments
  uint32_t n_optional;
};
static_assert(sizeof(FinalRobustLds) <= 54613, "three workgroups per CU (160 KiB of LDS)");

template <bool kRobust>
using FinalLdsOf = std::conditional_t<kRobust, FinalRobustLds, FinalLds>;

struct FinalKArgs {
  sst_final_args a;
  const int* w;
  int n_rows;
};

struct FinalRobustKArgs {
  sst_final_robust_args r;
  const int* w;
  int n_rows;
};

// which fragments a pass of the enumeration sums: every used one (k_final_program), the required ones (the robust
// variant's first pass), every used one with the optional ones' costs capped (its second pass)
enum { kPassAll = 0, kPassRequired = 1, kPassCapped = 2 };

// A_i of position p: P_i & alpha where P_i != 0, else alpha; row 0 excluded (a0 / a1 hold rows 1 .. n_rows - 1 only)
__device__ __forceinline__ void final_set(const uint64_t* skel, uint64_t a0, uint64_t a1, int p, uint64_t& m0,
                                          uint64_t& m1) {
  const uint64_t p0 = skel[2 * p], p1 = skel[2 * p + 1];
  if (p0 | p1) {
    m0 = p0 & a0;
    m1 = p1 & a1;
  } else {
    m0 = a0;
    m1 = a1;
  }
}

// qfix of a fragment; false where the model does not hold (u not finite or |u| >= 2^32)
__device__ __forceinline__ bool final_qfix(double su, double prec, int64_t& q) {
  const double u = su / prec;
  if (!(__builtin_fabs(u) < 0x1p32)) return false;  // (NaN and the infinities fail the comparison)
  q = (int64_t)__builtin_rint(u * 65536.0);
  return true;
}

// class and range of ends of a fragment, as a record's meta word; false: a terminal fragment with an end outside [0, L - 1]
__device__ __forceinline__ bool final_meta(uint8_t code, int mn, int mx, int L, uint32_t& meta) {
  const uint32_t cls = (code >> 2) & 3u;
  meta = cls;
  if (cls == 1 || cls == 2) {
    if (mn < 0 || mn >= L || mx < 0 || mx >= L) return false;
    const int lo = mn < mx ? mn : mx, hi = cls == 1 ? mx : mn;
    meta |= (uint32_t)lo << 8 | (uint32_t)hi << 16;
  }
  return true;
}

__device__ __forceinline__ uint32_t final_prefix(const FinalLds& s, int i, int tid) {
  return s.pbase[i] + s.D[s.kof[i]][tid];
}

// the prefix sums a cost is taken over: the lane's y, or y* (P* in LDS)
struct FinalLanePrefix {
  const FinalLds& s;
  int tid;
  __device__ __forceinline__ uint32_t operator()(int i) const { return final_prefix(s, i, tid); }
};
struct FinalStarPrefix {
  const uint32_t* p;
  __device__ __forceinline__ uint32_t operator()(int i) const { return p[i]; }
};

__device__ __forceinline__ uint64_t final_dist(int64_t q, uint32_t sum) {
  const int64_t d = q - (int64_t)((uint64_t)sum << 16);
  return (uint64_t)(d < 0 ? -d : d);
}

// c_j(y) of the y whose prefix sums are P
template <class Prefix>
__device__ __forceinline__ uint64_t final_cost(const Prefix& P, int64_t q, uint32_t meta, int L) {
  const uint32_t cls = meta & 3u;
  const int lo = (int)((meta >> 8) & 0xffu), hi = (int)((meta >> 16) & 0xffu);
  if (cls == 3) return final_dist(q, P(L));
  uint64_t best = kNone64;
  if (cls == 1) {
    for (int r = lo; r <= hi; ++r) {
      const uint64_t c = final_dist(q, P(r + 1));
      best = c < best ? c : best;
    }
    return best;
  }
  if (cls == 2) {
    const uint32_t total = P(L);
    for (int l = lo; l <= hi; ++l) {
      const uint64_t c = final_dist(q, total - P(l));
      best = c < best ? c : best;
    }
    return best;
  }
  if (q <= 0) return (uint64_t)(-q);  // every sum is >= 0: the empty interval
  // i <= j over P(0 .. L): the sum P(j) - P(i) grows with j and falls with i; the pointer that can still improve moves
  int i = 0, j = 0;
  uint32_t pi = P(0), pj = pi;
  for (;;) {
    const int64_t d = q - (int64_t)((uint64_t)(pj - pi) << 16);
    const uint64_t c = (uint64_t)(d < 0 ? -d : d);
    best = c < best ? c : best;
    if (d > 0) {
      if (j == L) break;
      pj = P(++j);
    } else {
      if (d == 0) break;
      pi = P(++i);  // (d < 0 only where i < j, as q > 0)
    }
  }
  return best;
}

// The lane's column of D from the index of a y; returns its modified rows among the free positions.  w_digit: the
// digits are also written there (the winner, by one thread).
__device__ __forceinline__ int final_decode(FinalLds& s, uint32_t idx, int n_free, int tid, bool digits) {
  int mods = 0;
  uint32_t rem = idx;
  for (int f = n_free - 1; f >= 0; --f) {
    const uint32_t radix = s.f_radix[f], d = rem % radix;
    rem /= radix;
    const int e = (int)s.f_off[f] + (int)d;
    s.D[f + 1][tid] = s.t_delta[e];
    mods += s.t_mod[e];
    if (digits) s.w_digit[f] = (uint8_t)d;
  }
  uint32_t acc = 0;
  s.D[0][tid] = 0;
  for (int f = 0; f < n_free; ++f) {
    acc += s.D[f + 1][tid];
    s.D[f + 1][tid] = acc;
  }
  return mods;
}

// A spectrum that is not SOLVED: its per-spectrum outputs and the defaults of its positions and fragments.
__device__ __forceinline__ void final_write_unsolved(const sst_final_args& a, int64_t g, uint8_t status, uint64_t combos,
                                                     int64_t pos0, int64_t n_pos, int64_t f0, int64_t nf_all, int tid) {
  if (tid == 0) {
    a.status[g] = status;
    a.combos[g] = combos;
    a.n_feas[g] = 0;
    a.best[g] = 0;
    a.n_opt[g] = 0;
    a.gap[g] = kNone64;
  }
  for (int64_t p = tid; p < n_pos; p += kFinalWG) a.seq[pos0 + p] = 0;
  for (int64_t j = tid; j < nf_all; j += kFinalWG) {
    a.iv[f0 + j] = 0xFFFE;
    a.sum[f0 + j] = 0;
  }
}

// The robust outputs of spectrum g (one thread).
__device__ __forceinline__ void final_write_robust(const sst_final_robust_args& r, int64_t g, uint32_t n_optional,
                                                   uint64_t cstar, uint64_t rbest, uint32_t rn_opt, uint64_t rgap) {
  r.n_optional[g] = n_optional;
  r.cstar[g] = cstar;
  r.rbest[g] = rbest;
  r.rn_opt[g] = rn_opt;
  r.rgap[g] = rgap;
}

// A spectrum that is not SOLVED, the robust outputs included: 0, and rgap UINT64_MAX.
template <bool kRobust>
__device__ __forceinline__ void final_unsolved(const sst_final_args& a, const sst_final_robust_args* rb, int tid,
                                               int64_t g, uint8_t status, uint64_t combos, int64_t pos0, int64_t n_pos,
                                               int64_t f0, int64_t nf_all) {
  final_write_unsolved(a, g, status, combos, pos0, n_pos, f0, nf_all, tid);
  if constexpr (kRobust)
    if (tid == 0) final_write_robust(*rb, g, 0, 0, 0, 0, kNone64);
}

// Does the fragment at `at` enter this pass?
template <int kPass>
__device__ __forceinline__ bool final_in_pass(const uint8_t* use, int64_t at) {
  if constexpr (kPass == kPassRequired) return !use || (use[at] && use[at] != 2);
  return !use || use[at];
}

// One enumeration of the spectrum's y: every lane's (best, the smallest objective above it, count, first index,
// feasible count) over the indices it takes.  kPassCapped: cst receives the c*_j of the optional records this
// thread loaded (each record once: while base == 0).
template <int kPass, class Lds>
__device__ __forceinline__ void final_enumerate(Lds& s, const sst_final_args& a, int64_t f0, int64_t nf_all, int L,
                                                uint64_t combos, int n_free, int fixed_mod, int mod_cap, int tid,
                                                uint64_t& best, uint64_t& next, uint32_t& count, uint32_t& first_at,
                                                uint32_t& feas, uint64_t& cst) {
  const int n_chunks = (int)((nf_all + kFinalF - 1) / kFinalF);
  for (uint32_t base = 0; base < (uint32_t)combos; base += kFinalWG) {
    const uint32_t idx = base + (uint32_t)tid;
    bool ok = idx < (uint32_t)combos;
    if (ok) ok = fixed_mod + final_decode(s, idx, n_free, tid, false) <= mod_cap;
    uint64_t obj = 0;
    bool live = ok;  // the objective is still summed
    for (int c = n_chunks - 1; c >= 0; --c) {  // (the last fragments first: see below)
      const int nf = (int)(nf_all - (int64_t)c * kFinalF < kFinalF ? nf_all - (int64_t)c * kFinalF : kFinalF);
      if (n_chunks > 1 || base == 0) {
        __syncthreads();  // the previous chunk's records are no longer read
        for (int j = tid; j < nf; j += kFinalWG) {
          const int64_t at = f0 + (int64_t)c * kFinalF + j;
          int64_t q = 0;
          uint32_t meta = 4u;
          if (final_in_pass<kPass>(a.frag_use, at)) {  // (a used fragment is within the model: checked above)
            final_qfix(a.frag_su[at], a.prec, q);
            final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
          }
          s.f_q[j] = q;
          s.f_meta[j] = meta;
          if constexpr (kPass == kPassCapped) {
            uint64_t cap = kNone64;
            if (a.frag_use && a.frag_use[at] == 2) {  // c*_j again on every load: nothing is kept per fragment
              cap = final_cost(FinalStarPrefix{s.pstar}, q, meta, L);
              if (base == 0) cst += cap;
            }
            s.f_cap[j] = cap;
          }
        }
        __syncthreads();
      }
      // from the last record down: the hand-off's order is ascending su, and the heavy fragments tell the y apart
      if (live)
        for (int j = nf - 1; j >= 0 && live; --j) {
          const uint32_t meta = s.f_meta[j];
          if (meta & 4u) continue;
          if constexpr (kPass == kPassCapped) {
            const uint64_t cost = final_cost(FinalLanePrefix{s, tid}, s.f_q[j], meta, L), cap = s.f_cap[j];
            obj += cost < cap ? cost : cap;
          } else {
            obj += final_cost(FinalLanePrefix{s, tid}, s.f_q[j], meta, L);
          }
          live = obj <= next;  // costs only add: above the lane's two smallest objectives y changes no output
        }
    }
    if (ok) ++feas;
    if (live) {
      if (obj < best) {
        next = best;
        best = obj;
        count = 1;
        first_at = idx;
      } else if (obj == best) {
        ++count;
      } else if (obj < next) {
        next = obj;
      }
    }
  }
}

// The workgroup's record from the lanes': r_best[0], r_next[0], r_count[0], r_first[0], r_feas[0].
__device__ __forceinline__ void final_reduce(FinalLds& s, int tid, uint64_t best, uint64_t next, uint32_t count,
                                             uint32_t first_at, uint32_t feas) {
  s.r_best[tid] = best;
  s.r_next[tid] = next;
  s.r_count[tid] = count;
  s.r_first[tid] = first_at;
  s.r_feas[tid] = feas;
  __syncthreads();
  for (int stride = kFinalWG / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      const uint64_t b1 = s.r_best[tid], b2 = s.r_best[tid + stride];
      const uint64_t n1 = s.r_next[tid], n2 = s.r_next[tid + stride];
      const uint32_t i1 = s.r_first[tid], i2 = s.r_first[tid + stride];
      s.r_feas[tid] += s.r_feas[tid + stride];
      if (b1 == b2) {
        s.r_next[tid] = n1 < n2 ? n1 : n2;
        s.r_count[tid] += s.r_count[tid + stride];
        s.r_first[tid] = i1 < i2 ? i1 : i2;
      } else if (b1 < b2) {
        s.r_next[tid] = n1 < b2 ? n1 : b2;
      } else {
        s.r_best[tid] = b2;
        s.r_next[tid] = n2 < b1 ? n2 : b1;
        s.r_count[tid] = s.r_count[tid + stride];
        s.r_first[tid] = i2;
      }
    }
    __syncthreads();
  }
}

// The kernel body.  kRobust (k_final_robust, sst_final_robust_device): frag_use 2 marks an optional fragment; the
// first enumeration runs over the required fragments alone, and where the spectrum holds optional ones a second one
// runs over all of them with every optional cost capped at its cost under y* (include/sst.h).  rb: the five robust
// outputs (kRobust only).
template <bool kRobust, class KArgs>
__device__ __forceinline__ void final_body(FinalLdsOf<kRobust>& s, const KArgs& k, const sst_final_args& a,
                                           const sst_final_robust_args* rb) {
  const int tid = (int)threadIdx.x;
  const int n_rows = k.n_rows;

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kFinalWG) s.w[r] = r < n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;
  if (n_rows < 64) {
    rows0 &= (1ull << n_rows) - 1;
    rows1 = 0;
  } else if (n_rows < 128) {
    rows1 = (1ull << (n_rows - 64)) - 1;
  }
  if (tid < 2) s.mod[tid] = 0;
  __syncthreads();
  for (int r = 1 + tid; r < n_rows && r < 128; r += kFinalWG)
    if (a.row_mod[r]) atomicOr(&s.mod[r >> 6], 1ull << (r & 63));
  __syncthreads();
  const uint64_t mod0 = s.mod[0], mod1 = s.mod[1];

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    if (nf_all <= 0) {  // a default spectrum, or one without fragments: nothing is computed
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_NONE, 0, pos0, n_pos, f0, 0);
      continue;
    }
    const int L = a.seq_len[g];
    if (!(L >= 0 && L <= kFinalMaxLen && n_pos == (int64_t)L)) {
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_SKIPPED, 0, pos0, n_pos, f0, nf_all);
      continue;
    }
    const uint64_t* skel = a.skeleton + 2 * pos0;
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    const int mod_cap = a.mod_cap[g];
    __syncthreads();  // the previous spectrum's LDS is no longer read
    if (tid == 0) {
      s.flags = 0;
      s.n_used = 0;
      if constexpr (kRobust) s.n_optional = 0;
    }
    __syncthreads();

    // the used fragments: their number, and the conditions the model does not hold under
    {
      uint32_t used = 0, optional = 0;
      bool bad = false;
      for (int64_t j = tid; j < nf_all; j += kFinalWG) {
        const int64_t at = f0 + j;
        if (a.frag_use && !a.frag_use[at]) continue;
        ++used;
        if constexpr (kRobust) optional += a.frag_use && a.frag_use[at] == 2;
        int64_t q;
        uint32_t meta;
        bad = bad || !final_qfix(a.frag_su[at], a.prec, q) ||
              !final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
      }
      if (used) atomicAdd(&s.n_used, used);
      if constexpr (kRobust)
        if (optional) atomicAdd(&s.n_optional, optional);
      if (bad) atomicOr(&s.flags, 2u);
    }
    for (int p = tid; p < L; p += kFinalWG) {
      uint64_t m0, m1;
      final_set(skel, a0, a1, p, m0, m1);
      const int cnt = __builtin_popcountll(m0) + __builtin_popcountll(m1);
      s.p_cnt[p] = (uint8_t)cnt;
      s.p_first[p] = (uint8_t)(m0 ? __builtin_ctzll(m0) : m1 ? 64 + __builtin_ctzll(m1) : 0);
      if (cnt == 0) atomicOr(&s.flags, 1u);
    }
    __syncthreads();
    if ((s.flags & 2u) || s.n_used > kFinalMaxUsed) {
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_SKIPPED, 0, pos0, n_pos, f0, nf_all);
      continue;
    }
    if (s.flags & 1u) {  // (combos = prod |A_i| = 0)
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_INFEASIBLE, 0, pos0, n_pos, f0, nf_all);
      continue;
    }

    if (tid == 0) {  // one walk over the positions
      uint64_t combos = 1;
      uint32_t pre = 0;
      int n_free = 0, t_n = 0, fixed_mod = 0;
      bool over = false;  // more free positions or digits than are recorded: combos > 2^22
      for (int p = 0; p < L; ++p) {
        const int cnt = s.p_cnt[p], first = s.p_first[p];
        s.pbase[p] = pre;
        s.kof[p] = (uint8_t)n_free;
        pre += s.w[first];
        combos = combos > kNone64 / (uint64_t)cnt ? kNone64 : combos * (uint64_t)cnt;
        if (cnt == 1) {
          fixed_mod += (int)(((first < 64 ? mod0 : mod1) >> (first & 63)) & 1u);
        } else if (!over) {
          if (n_free == kFinalMaxFree || t_n + cnt > kFinalTable) {
            over = true;
            continue;
          }
          uint64_t m0, m1;
          final_set(skel, a0, a1, p, m0, m1);
          s.f_off[n_free] = (uint16_t)t_n;
          s.f_radix[n_free] = (uint8_t)cnt;
          for (int h = 0; h < 2; ++h)
            for (uint64_t m = h ? m1 : m0; m; m &= m - 1) {
              const int bit = __builtin_ctzll(m), row = 64 * h + bit;
              s.t_delta[t_n] = s.w[row] - s.w[first];
              s.t_row[t_n] = (uint8_t)row;
              s.t_mod[t_n] = (uint8_t)(((h ? mod1 : mod0) >> bit) & 1u);
              ++t_n;
            }
          ++n_free;
        }
      }
      s.pbase[L] = pre;
      s.kof[L] = (uint8_t)n_free;
      s.combos = combos;
      s.n_free = (uint32_t)n_free;
      s.fixed_mod = fixed_mod;
    }
    // the row-free test: one row of alpha per thread, n_r counted over the positions' sets
    for (int r = 1 + tid; r < n_rows; r += kFinalWG) {
      const uint64_t bit = 1ull << (r & 63);
      if (!((r < 64 ? a0 : a1) & bit)) continue;
      int n_r = 0;
      for (int p = 0; p < L; ++p) {
        uint64_t m0, m1;
        final_set(skel, a0, a1, p, m0, m1);
        n_r += ((r < 64 ? m0 : m1) & bit) != 0;
      }
      const int cap = a.row_cap[(int64_t)L * n_rows + r];
      const bool modified = ((r < 64 ? mod0 : mod1) & bit) != 0;
      if (!(cap >= n_r || (modified && cap >= mod_cap))) atomicOr(&s.flags, 4u);
    }
    __syncthreads();
    const uint64_t combos = s.combos;
    if (s.flags & 4u) {
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_NOT_FREE, combos, pos0, n_pos, f0, nf_all);
      continue;
    }
    if (combos > a.max_combos) {
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_TOO_LARGE, combos, pos0, n_pos, f0, nf_all);
      continue;
    }

    // the enumeration: combos <= 2^22, every free position is recorded
    const int n_free = (int)s.n_free, fixed_mod = s.fixed_mod;
    uint64_t best = kNone64, next = kNone64, cst = 0;
    uint32_t count = 0, first_at = 0, feas = 0;
    final_enumerate<kRobust ? kPassRequired : kPassAll>(s, a, f0, nf_all, L, combos, n_free, fixed_mod, mod_cap, tid, best,
                                                        next, count, first_at, feas, cst);
    final_reduce(s, tid, best, next, count, first_at, feas);
    const uint32_t n_feas = s.r_feas[0];
    if (n_feas == 0) {
      final_unsolved<kRobust>(a, rb, tid, g, SST_FINAL_INFEASIBLE, combos, pos0, n_pos, f0, nf_all);
      continue;
    }
    const uint32_t winner = s.r_first[0];
    if (tid == 0) {
      a.status[g] = SST_FINAL_SOLVED;
      a.combos[g] = combos;
      a.n_feas[g] = n_feas;
      a.best[g] = s.r_best[0];
      a.n_opt[g] = s.r_count[0];
      a.gap[g] = s.r_next[0] == kNone64 ? kNone64 : s.r_next[0] - s.r_best[0];
    }
    if constexpr (kRobust) {
      const uint32_t n_optional = s.n_optional;
      if (n_optional == 0) {  // cap == obj: the second enumeration would repeat the first
        if (tid == 0)
          final_write_robust(*rb, g, 0, 0, s.r_best[0], s.r_count[0],
                             s.r_next[0] == kNone64 ? kNone64 : s.r_next[0] - s.r_best[0]);
      } else {
        // P*: every lane's column holds the winner's D
        final_decode(s, winner, n_free, tid, false);
        for (int i = tid; i <= L; i += kFinalWG) s.pstar[i] = final_prefix(s, i, tid);
        if (tid == 0) s.cstar = 0;
        __syncthreads();
        best = next = kNone64;
        count = first_at = feas = 0;
        final_enumerate<kPassCapped>(s, a, f0, nf_all, L, combos, n_free, fixed_mod, mod_cap, tid, best, next, count,
                                     first_at, feas, cst);
        if (cst) atomicAdd(&s.cstar, (unsigned long long)cst);
        final_reduce(s, tid, best, next, count, first_at, feas);
        if (tid == 0)
          final_write_robust(*rb, g, n_optional, s.cstar, s.r_best[0], s.r_count[0],
                             s.r_next[0] == kNone64 ? kNone64 : s.r_next[0] - s.r_best[0]);
      }
    }
    // the winner again: every lane's column holds its D
    final_decode(s, winner, n_free, tid, tid == 0);
    __syncthreads();
    for (int p = tid; p < L; p += kFinalWG) {
      const int f = s.kof[p];
      a.seq[pos0 + p] = s.p_cnt[p] == 1 ? s.p_first[p] : s.t_row[(int)s.f_off[f] + (int)s.w_digit[f]];
    }
    for (int64_t j = tid; j < nf_all; j += kFinalWG) {
      const int64_t at = f0 + j;
      uint16_t iv = 0xFFFE;
      uint32_t sum = 0;
      if (!a.frag_use || a.frag_use[at]) {
        int64_t q = 0;
        uint32_t meta = 0;
        final_qfix(a.frag_su[at], a.prec, q);
        final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
        const uint32_t cls = meta & 3u;
        const int lo = (int)((meta >> 8) & 0xffu), hi = (int)((meta >> 16) & 0xffu);
        uint64_t c_best = kNone64;
        // the admissible intervals in (l, r) order, the empty one last; a later one wins only where it is nearer
        if (cls == 3) {
          iv = L ? (uint16_t)(L - 1) : (uint16_t)0xFFFF;
          sum = final_prefix(s, L, tid);
        } else if (cls == 1) {
          for (int r = lo; r <= hi; ++r) {
            const uint32_t x = final_prefix(s, r + 1, tid);
            const uint64_t c = final_dist(q, x);
            if (c < c_best) {
              c_best = c;
              iv = (uint16_t)r;
              sum = x;
            }
          }
        } else if (cls == 2) {
          const uint32_t total = final_prefix(s, L, tid);
          for (int l = lo; l <= hi; ++l) {
            const uint32_t x = total - final_prefix(s, l, tid);
            const uint64_t c = final_dist(q, x);
            if (c < c_best) {
              c_best = c;
              iv = (uint16_t)(l << 8 | (L - 1));
              sum = x;
            }
          }
        } else {
          for (int l = 0; l < L; ++l) {
            const uint32_t pl = final_prefix(s, l, tid);
            for (int r = l; r < L; ++r) {
              const uint32_t x = final_prefix(s, r + 1, tid) - pl;
              const uint64_t c = final_dist(q, x);
              if (c < c_best) {
                c_best = c;
                iv = (uint16_t)(l << 8 | r);
                sum = x;
              }
              if ((int64_t)((uint64_t)x << 16) >= q) break;  // the sums of [l, r + 1 ..] are no nearer
            }
          }
          if (final_dist(q, 0) < c_best) {
            iv = 0xFFFF;
            sum = 0;
          }
        }
      }
      a.iv[at] = iv;
      a.sum[at] = sum;
    }
  }
}

__global__ __launch_bounds__(kFinalWG) void k_final_program(FinalKArgs k) {
  __shared__ FinalLds s;
  final_body<false>(s, k, k.a, nullptr);
}

__global__ __launch_bounds__(kFinalWG) void k_final_robust(FinalRobustKArgs k) {
  __shared__ FinalRobustLds s;
  final_body<true>(s, k, k.r.base, &k.r);
}

// ---- the bounded search (k_final_search, sst_final_search_device; the definition is in include/sst.h) --------------
//
// k_final_robust has run with the caller's max_combos: the spectra it left TOO_LARGE passed every earlier test, and
// they are the ones searched.  k_final_search_list (one workgroup) lists them in spectrum order and writes the three
// search outputs' defaults (mode 1 where SOLVED).  k_final_search: one spectrum of the list per workgroup, persistent
// grid with static striding.  Prologue as k_final_program's, with per free position its smallest and largest mass and
// its modified rows; thread 0 counts n_feas over the number of modified rows (saturating u64).
//
// A sweep walks the free positions.  The frontier of a level lives in the workgroup's slice of the workspace: per node
// kSearchWords words of rows (one byte per free position, word-major so that lanes read neighbouring words) and one
// word of modified rows, ping-ponged between two buffers; the leaves' objectives go to a third array.  Lanes run over
// (node, child) pairs in node-major order, 256 pairs a round.  A lane builds A[k][lane], the masses of its node's rows
// summed over the first k free positions; per level the workgroup shares bmin / bmax (the one-row positions' prefix
// sums plus the open free positions' smallest / largest masses) and kk = min(free positions before i, depth), so that
// Pmin(i) = bmin[i] + A[kk[i]][lane] and Pmax likewise.  The fragment records sit in LDS in chunks of kSearchF; a lane
// stops summing once its bound is above T (terms only add).  An internal fragment is a two-pointer walk: for a fixed l
// the minimum of d lies at the first r with 65536 Smax >= qfix or just before it, and that r does not decrease with l.
// The survivors of a round are placed by a prefix sum over the workgroup, in pair order: every level is in index order,
// the first leaf at the minimum is the one of smallest index, and the count is known before anything is written, so an
// overflow writes nothing.  Outputs are written once both passes are through; until then the spectrum keeps
// k_final_robust's TOO_LARGE defaults.  Plain vector stores, no global atomics.
constexpr int kSearchMaxFree = SST_FINAL_SEARCH_MAX_FREE;
constexpr int kSearchF = 256;                          // fragment records per chunk
constexpr int kSearchWords = kSearchMaxFree / 4;       // row words of a node record
constexpr int kSearchRec = kSearchWords + 1;           // and its modified rows
constexpr uint64_t kSearchTMax = (1ull << 63) - 1;

struct SearchRed {  // the reduction over the leaves
  unsigned long long r_best[kFinalWG];
  unsigned long long r_next[kFinalWG];
  uint32_t r_count[kFinalWG];
  uint32_t r_first[kFinalWG];
};

struct SearchLds {
  union {
    uint32_t A[kSearchMaxFree + 1][kFinalWG];  // per lane: its node's masses over the first k free positions
    SearchRed red;                             // the reduction over the leaves (no bound is evaluated then)
    unsigned long long ways[kSearchMaxFree + 2];  // n_feas: assignments by modified rows (thread 0, before the sweeps)
  };
  int64_t f_q[kSearchF];               // a chunk's records: qfix
  unsigned long long f_cap[kSearchF];  // c*_j of an optional record (pass 2), kNone64 of a required one
  uint32_t f_meta[kSearchF];           // class | not in this pass << 2 | first end << 8 | last end << 16
  uint32_t bmin[256], bmax[256];       // the level's shared part of Pmin(i), Pmax(i), i in [0, L]
  uint32_t pone[256];                  // the masses of the one-row positions before i
  uint32_t pstar[256];                 // P*(i): the prefix sums of y*
  uint32_t w[SST_MAX_ROWS + 8];
  uint32_t scan[kFinalWG];
  uint32_t f_min[kSearchMaxFree], f_max[kSearchMaxFree];        // a free position's smallest and largest mass
  uint32_t m_min[kSearchMaxFree + 1], m_max[kSearchMaxFree + 1];  // their sums over the first k free positions
  uint32_t lv_mass[128];               // the level's rows in ascending order: mass, row, modified
  uint8_t lv_row[128];
  uint8_t lv_mod[128];
  uint8_t kof[256];                    // free positions before position i, i in [0, L]
  uint8_t kk[256];                     // min(kof[i], the level's depth)
  uint8_t p_cnt[256];
  uint8_t p_first[256];
  uint8_t rowof[256];                  // y*
  uint8_t f_pos[kSearchMaxFree];
  uint8_t f_radix[kSearchMaxFree];
  uint8_t f_nmod[kSearchMaxFree];      // its modified rows
  uint8_t all_mod_from[kSearchMaxFree + 1];  // free positions k .. n - 1 all of whose rows are modified
  unsigned long long mod[2];
  unsigned long long n_feas;
  unsigned long long cstar;
  uint32_t n_optional;
  uint32_t n_free;                     // kSearchMaxFree + 1: more than that
  int32_t fixed_mod;
};
static_assert(sizeof(SearchLds) <= 64 * 1024, "static LDS");

struct FinalSearchKArgs {
  sst_final_search_args x;
  const int* w;
  int n_rows;
  uint32_t* list;     // [1 + n_spec]: the number of searched spectra, then their indices
  uint32_t* ws;       // a workgroup's slice: two frontiers of kSearchRec words by max_width, then max_width u64
  uint64_t ws_words;  // words per slice
};

__device__ __forceinline__ uint64_t search_sat_mul(uint64_t a, uint64_t b) {
  return b && a > kNone64 / b ? kNone64 : a * b;
}
__device__ __forceinline__ uint64_t search_sat_add(uint64_t a, uint64_t b) { return a > kNone64 - b ? kNone64 : a + b; }

// d(l, r) of an interval whose smallest and largest sums are smin, smax
__device__ __forceinline__ uint64_t search_d(int64_t q, uint32_t smin, uint32_t smax) {
  const int64_t x = (int64_t)((uint64_t)smin << 16) - q, y = q - (int64_t)((uint64_t)smax << 16);
  const int64_t m = x > y ? x : y;
  return m > 0 ? (uint64_t)m : 0;
}

__device__ __forceinline__ uint32_t search_pmin(const SearchLds& s, int i, int tid) { return s.bmin[i] + s.A[s.kk[i]][tid]; }
__device__ __forceinline__ uint32_t search_pmax(const SearchLds& s, int i, int tid) { return s.bmax[i] + s.A[s.kk[i]][tid]; }

// lb_j of the lane's node
__device__ __forceinline__ uint64_t search_lb(const SearchLds& s, int tid, int64_t q, uint32_t meta, int L) {
  const uint32_t cls = meta & 3u;
  const int lo = (int)((meta >> 8) & 0xffu), hi = (int)((meta >> 16) & 0xffu);
  if (cls == 3) return search_d(q, search_pmin(s, L, tid), search_pmax(s, L, tid));
  uint64_t best = kNone64;
  if (cls == 1) {
    for (int r = lo; r <= hi && best; ++r) {
      const uint64_t c = search_d(q, search_pmin(s, r + 1, tid), search_pmax(s, r + 1, tid));
      best = c < best ? c : best;
    }
    return best;
  }
  if (cls == 2) {
    const uint32_t tmin = search_pmin(s, L, tid), tmax = search_pmax(s, L, tid);
    for (int l = lo; l <= hi && best; ++l) {
      const uint64_t c = search_d(q, tmin - search_pmin(s, l, tid), tmax - search_pmax(s, l, tid));
      best = c < best ? c : best;
    }
    return best;
  }
  if (q <= 0) return (uint64_t)(-q);  // every sum is >= 0: the empty interval
  best = (uint64_t)q;                 // the empty interval
  // e: the first prefix index above l with 65536 (Pmax(e) - Pmax(l)) >= q (L + 1: none); it does not decrease with l.
  // Before it d = q - 65536 Smax falls with r, from it on d = max(0, 65536 Smin - q) rises: the minimum is at e or e - 1.
  int e = 1;
  for (int l = 0; l < L && best; ++l) {
    const uint32_t xl = search_pmax(s, l, tid);
    if (e <= l) e = l + 1;
    while (e <= L && (int64_t)((uint64_t)(search_pmax(s, e, tid) - xl) << 16) < q) ++e;
    if (e <= L) {
      const uint64_t c = search_d(q, search_pmin(s, e, tid) - search_pmin(s, l, tid), search_pmax(s, e, tid) - xl);
      best = c < best ? c : best;
    }
    if (e - 1 > l) {
      const uint64_t c = search_d(q, search_pmin(s, e - 1, tid) - search_pmin(s, l, tid), search_pmax(s, e - 1, tid) - xl);
      best = c < best ? c : best;
    }
  }
  return best;
}

// iv and sum of a used fragment under the y whose prefix sums are P: the smallest (l, r) among the minimisers of c_j
// (the walk of final_body's epilogue, over P* and not over a lane's column)
template <class Prefix>
__device__ __forceinline__ void search_interval(const Prefix& P, int64_t q, uint32_t meta, int L, uint16_t& iv,
                                               uint32_t& sum) {
  const uint32_t cls = meta & 3u;
  const int lo = (int)((meta >> 8) & 0xffu), hi = (int)((meta >> 16) & 0xffu);
  uint64_t c_best = kNone64;
  // the admissible intervals in (l, r) order, the empty one last; a later one wins only where it is nearer
  if (cls == 3) {
    iv = L ? (uint16_t)(L - 1) : (uint16_t)0xFFFF;
    sum = P(L);
  } else if (cls == 1) {
    for (int r = lo; r <= hi; ++r) {
      const uint32_t x = P(r + 1);
      const uint64_t c = final_dist(q, x);
      if (c < c_best) {
        c_best = c;
        iv = (uint16_t)r;
        sum = x;
      }
    }
  } else if (cls == 2) {
    const uint32_t total = P(L);
    for (int l = lo; l <= hi; ++l) {
      const uint32_t x = total - P(l);
      const uint64_t c = final_dist(q, x);
      if (c < c_best) {
        c_best = c;
        iv = (uint16_t)(l << 8 | (L - 1));
        sum = x;
      }
    }
  } else {
    for (int l = 0; l < L; ++l) {
      const uint32_t pl = P(l);
      for (int r = l; r < L; ++r) {
        const uint32_t x = P(r + 1) - pl;
        const uint64_t c = final_dist(q, x);
        if (c < c_best) {
          c_best = c;
          iv = (uint16_t)(l << 8 | r);
          sum = x;
        }
        if ((int64_t)((uint64_t)x << 16) >= q) break;  // the sums of [l, r + 1 ..] are no nearer
      }
    }
    if (final_dist(q, 0) < c_best) {
      iv = 0xFFFF;
      sum = 0;
    }
  }
}

// One sweep.  Returns false on overflow.  leaves: |S_n|; their records lie in frontier `side`, their objectives behind
// the two frontiers.  nodes gains the sweep's count.  kPass: kPassRequired, or kPassCapped (P* in s.pstar).
template <int kPass>
__device__ __forceinline__ bool search_sweep(SearchLds& s, const sst_final_args& a, const uint64_t* skel, uint64_t a0,
                                             uint64_t a1, uint64_t mod0, uint64_t mod1, int64_t f0, int64_t nf_all, int L,
                                             int n_free, int mod_cap, uint64_t T, uint32_t* ws, uint32_t max_width,
                                             int tid, uint32_t& leaves, int& side, uint64_t& nodes) {
  const int n_chunks = (int)((nf_all + kSearchF - 1) / kSearchF);
  const uint64_t W = max_width;
  uint64_t* lbv = (uint64_t*)(ws + 2ull * kSearchRec * W);
  const int fixed_mod = s.fixed_mod;
  const bool root_leaf = n_free == 0;  // the root is the one leaf: one round evaluates it, whatever T
  bool loaded = false;
  uint32_t m = 1;  // |S_d|
  side = 0;
  for (int d = 0; d < (root_leaf ? 1 : n_free); ++d) {
    const int depth = root_leaf ? 0 : d + 1;  // of the nodes this level evaluates
    const uint32_t radix = root_leaf ? 1u : s.f_radix[d];
    const uint32_t* cur = ws + (uint64_t)side * kSearchRec * W;
    uint32_t* nxt = ws + (uint64_t)(side ^ 1) * kSearchRec * W;
    __syncthreads();  // the previous level's tables are no longer read, and its records are written
    if (!root_leaf && tid < (int)radix) {  // the tid-th row of this position's set
      uint64_t m0, m1;
      final_set(skel, a0, a1, s.f_pos[d], m0, m1);
      const int n0 = __builtin_popcountll(m0);
      uint64_t mm = tid < n0 ? m0 : m1;
      for (int i = tid < n0 ? tid : tid - n0; i > 0; --i) mm &= mm - 1;
      const int bit = __builtin_ctzll(mm), row = (tid < n0 ? 0 : 64) + bit;
      s.lv_row[tid] = (uint8_t)row;
      s.lv_mass[tid] = s.w[row];
      s.lv_mod[tid] = (uint8_t)(((tid < n0 ? mod0 : mod1) >> bit) & 1u);
    }
    for (int i = tid; i <= L; i += kFinalWG) {
      const int kf = s.kof[i];
      s.kk[i] = (uint8_t)(kf < depth ? kf : depth);
      s.bmin[i] = s.pone[i] + (kf > depth ? s.m_min[kf] - s.m_min[depth] : 0u);
      s.bmax[i] = s.pone[i] + (kf > depth ? s.m_max[kf] - s.m_max[depth] : 0u);
    }
    __syncthreads();
    const uint32_t pairs = m * radix;  // (at most 2^16 * 127)
    const bool last = depth == n_free;
    uint32_t out = 0;
    for (uint32_t base = 0; base < pairs; base += kFinalWG) {
      const uint32_t pair = base + (uint32_t)tid;
      bool live = pair < pairs;  // the bound is still summed
      const uint32_t node = live ? pair / radix : 0u, c = live ? pair % radix : 0u;
      uint32_t mods = 0;
      if (live) {
        uint32_t acc = 0;
        s.A[0][tid] = 0;
        for (int t = 0; t < d; t += 4) {
          const uint32_t word = cur[(uint64_t)(t >> 2) * W + node];
          for (int b = 0; b < 4 && t + b < d; ++b) {
            acc += s.w[(word >> (8 * b)) & 0xffu];
            s.A[t + b + 1][tid] = acc;
          }
        }
        if (d > 0) mods = cur[(uint64_t)kSearchWords * W + node];
        if (!root_leaf) {
          s.A[d + 1][tid] = acc + s.lv_mass[c];
          mods += s.lv_mod[c];
          live = fixed_mod + (int)mods + (int)s.all_mod_from[depth] <= mod_cap;
        }
      }
      uint64_t lb = 0;
      for (int ch = n_chunks - 1; ch >= 0; --ch) {
        const int nf = (int)(nf_all - (int64_t)ch * kSearchF < kSearchF ? nf_all - (int64_t)ch * kSearchF : kSearchF);
        if (n_chunks > 1 || !loaded) {
          __syncthreads();  // the previous chunk's records are no longer read
          for (int j = tid; j < nf; j += kFinalWG) {
            const int64_t at = f0 + (int64_t)ch * kSearchF + j;
            int64_t q = 0;
            uint32_t meta = 4u;
            if (final_in_pass<kPass>(a.frag_use, at)) {
              final_qfix(a.frag_su[at], a.prec, q);
              final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
            }
            s.f_q[j] = q;
            s.f_meta[j] = meta;
            if constexpr (kPass == kPassCapped) {
              uint64_t cap = kNone64;
              if (a.frag_use && a.frag_use[at] == 2) cap = final_cost(FinalStarPrefix{s.pstar}, q, meta, L);
              s.f_cap[j] = cap;
            }
          }
          __syncthreads();
        }
        for (int j = nf - 1; j >= 0 && live; --j) {
          const uint32_t meta = s.f_meta[j];
          if (meta & 4u) continue;
          uint64_t cost = search_lb(s, tid, s.f_q[j], meta, L);
          if constexpr (kPass == kPassCapped) cost = cost < s.f_cap[j] ? cost : s.f_cap[j];
          lb += cost;
          live = root_leaf || lb <= T;  // terms only add
        }
      }
      loaded = true;
      // the survivors' places in pair order: an inclusive prefix sum over the workgroup
      const uint32_t keep = live ? 1u : 0u;
      s.scan[tid] = keep;
      __syncthreads();
      for (int off = 1; off < kFinalWG; off <<= 1) {
        const uint32_t v = tid >= off ? s.scan[tid - off] : 0u;
        __syncthreads();
        s.scan[tid] += v;
        __syncthreads();
      }
      const uint32_t total = s.scan[kFinalWG - 1];
      if ((uint64_t)out + total > W) return false;  // (the same in every lane) overflow: nothing of this round is written
      if (keep) {
        const uint64_t at = out + s.scan[tid] - 1u;
        if (!root_leaf) {
          for (int wi = 0; wi <= d >> 2; ++wi) {
            uint32_t word = wi * 4 < d ? cur[(uint64_t)wi * W + node] : 0u;
            if (wi == d >> 2) {
              const int sh = 8 * (d & 3);
              word = (word & ~(0xffu << sh)) | (uint32_t)s.lv_row[c] << sh;
            }
            nxt[(uint64_t)wi * W + at] = word;
          }
          nxt[(uint64_t)kSearchWords * W + at] = mods;
        }
        if (last) lbv[at] = lb;
      }
      out += total;
      __syncthreads();  // scan[] is rewritten by the next round
    }
    if (!root_leaf) {
      nodes += out;
      side ^= 1;
    }
    m = out;
    if (m == 0) break;
  }
  leaves = m;
  return true;
}

// The workgroup's record from the lanes' (final_reduce's tree without the feasible count): r_best[0], r_next[0],
// r_count[0], r_first[0].
__device__ __forceinline__ void search_reduce(SearchRed& s, int tid, uint64_t best, uint64_t next, uint32_t count,
                                              uint32_t first_at) {
  s.r_best[tid] = best;
  s.r_next[tid] = next;
  s.r_count[tid] = count;
  s.r_first[tid] = first_at;
  __syncthreads();
  for (int stride = kFinalWG / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      const uint64_t b1 = s.r_best[tid], b2 = s.r_best[tid + stride];
      const uint64_t n1 = s.r_next[tid], n2 = s.r_next[tid + stride];
      const uint32_t i1 = s.r_first[tid], i2 = s.r_first[tid + stride];
      if (b1 == b2) {
        s.r_next[tid] = n1 < n2 ? n1 : n2;
        s.r_count[tid] += s.r_count[tid + stride];
        s.r_first[tid] = i1 < i2 ? i1 : i2;
      } else if (b1 < b2) {
        s.r_next[tid] = n1 < b2 ? n1 : b2;
      } else {
        s.r_best[tid] = b2;
        s.r_next[tid] = n2 < b1 ? n2 : b1;
        s.r_count[tid] = s.r_count[tid + stride];
        s.r_first[tid] = i2;
      }
    }
    __syncthreads();
  }
}

// (min, the smallest value above it, how many leaves attain it, the first of them) over a sweep's leaves, in s.red
__device__ __forceinline__ void search_summary(SearchLds& s, const uint64_t* lbv, uint32_t leaves, int tid) {
  uint64_t best = kNone64, next = kNone64;
  uint32_t count = 0, first_at = 0;
  for (uint32_t i = (uint32_t)tid; i < leaves; i += kFinalWG) {
    const uint64_t v = lbv[i];
    if (v < best) {
      next = best;
      best = v;
      count = 1;
      first_at = i;
    } else if (v == best) {
      ++count;
    } else if (v < next) {
      next = v;
    }
  }
  __syncthreads();  // the sweep's records are written, A is no longer read
  search_reduce(s.red, tid, best, next, count, first_at);
}

__global__ __launch_bounds__(kFinalWG) void k_final_search_list(FinalSearchKArgs k) {
  __shared__ uint32_t cnt[kFinalWG];
  const sst_final_args& a = k.x.robust.base;
  const int tid = (int)threadIdx.x;
  const int64_t per = (a.n_spec + kFinalWG - 1) / kFinalWG;
  const int64_t lo = tid * per < a.n_spec ? tid * per : a.n_spec, hi = lo + per < a.n_spec ? lo + per : a.n_spec;
  uint32_t c = 0;
  for (int64_t g = lo; g < hi; ++g) {
    const uint8_t st = a.status[g];
    k.x.mode[g] = st == SST_FINAL_SOLVED ? 1 : 0;
    k.x.rounds[g] = 0;
    k.x.nodes[g] = 0;
    c += st == SST_FINAL_TOO_LARGE;
  }
  cnt[tid] = c;
  __syncthreads();
  for (int off = 1; off < kFinalWG; off <<= 1) {
    const uint32_t v = tid >= off ? cnt[tid - off] : 0u;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  uint32_t at = cnt[tid] - c;
  for (int64_t g = lo; g < hi; ++g)
    if (a.status[g] == SST_FINAL_TOO_LARGE) k.list[1 + at++] = (uint32_t)g;
  if (tid == kFinalWG - 1) k.list[0] = cnt[tid];
}

__global__ __launch_bounds__(kFinalWG) void k_final_search(FinalSearchKArgs k) {
  __shared__ SearchLds s;
  const sst_final_search_args& x = k.x;
  const sst_final_args& a = x.robust.base;
  const int tid = (int)threadIdx.x;
  const int n_rows = k.n_rows;
  const uint64_t W = x.max_width, H = x.horizon;
  uint32_t* ws = k.ws + (uint64_t)blockIdx.x * k.ws_words;
  const uint64_t* lbv = (const uint64_t*)(ws + 2ull * kSearchRec * W);

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kFinalWG) s.w[r] = r < n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;
  if (n_rows < 64) {
    rows0 &= (1ull << n_rows) - 1;
    rows1 = 0;
  } else if (n_rows < 128) {
    rows1 = (1ull << (n_rows - 64)) - 1;
  }
  if (tid < 2) s.mod[tid] = 0;
  __syncthreads();
  for (int r = 1 + tid; r < n_rows && r < 128; r += kFinalWG)
    if (a.row_mod[r]) atomicOr(&s.mod[r >> 6], 1ull << (r & 63));
  __syncthreads();
  const uint64_t mod0 = s.mod[0], mod1 = s.mod[1];

  const uint32_t n_list = k.list[0];
  for (uint32_t li = blockIdx.x; li < n_list; li += gridDim.x) {
    // a listed spectrum has fragments, is modelled, has no empty A_i and is row-free: k_final_robust's tests
    const int64_t g = k.list[1 + li];
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    const int64_t pos0 = a.pos_off[g];
    const int L = a.seq_len[g];
    const uint64_t* skel = a.skeleton + 2 * pos0;
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    const int mod_cap = a.mod_cap[g];
    __syncthreads();  // the previous spectrum's LDS is no longer read
    if (tid == 0) {
      s.n_optional = 0;
      s.cstar = 0;
    }
    __syncthreads();
    {
      uint32_t optional = 0;
      for (int64_t j = tid; j < nf_all; j += kFinalWG) optional += a.frag_use && a.frag_use[f0 + j] == 2;
      if (optional) atomicAdd(&s.n_optional, optional);
    }
    for (int p = tid; p < L; p += kFinalWG) {
      uint64_t m0, m1;
      final_set(skel, a0, a1, p, m0, m1);
      s.p_cnt[p] = (uint8_t)(__builtin_popcountll(m0) + __builtin_popcountll(m1));
      s.p_first[p] = (uint8_t)(m0 ? __builtin_ctzll(m0) : m1 ? 64 + __builtin_ctzll(m1) : 0);
    }
    __syncthreads();
    if (tid == 0) {  // one walk over the positions
      uint32_t pre = 0;
      int n_free = 0, fixed_mod = 0;
      for (int p = 0; p < L; ++p) {
        const int cnt = s.p_cnt[p], first = s.p_first[p];
        s.pone[p] = pre;
        s.kof[p] = (uint8_t)n_free;
        if (cnt == 1) {
          pre += s.w[first];
          fixed_mod += (int)(((first < 64 ? mod0 : mod1) >> (first & 63)) & 1u);
        } else {
          if (n_free < kSearchMaxFree) {
            s.f_pos[n_free] = (uint8_t)p;
            s.f_radix[n_free] = (uint8_t)cnt;
          }
          ++n_free;
        }
      }
      s.pone[L] = pre;
      s.kof[L] = (uint8_t)n_free;
      s.n_free = (uint32_t)n_free;
      s.fixed_mod = fixed_mod;
    }
    __syncthreads();
    const int n_free = (int)s.n_free;
    if (n_free > kSearchMaxFree) continue;  // TOO_LARGE, as k_final_robust left it
    if (tid < n_free) {  // a free position's smallest and largest mass, and its modified rows
      uint64_t m0, m1;
      final_set(skel, a0, a1, s.f_pos[tid], m0, m1);
      uint32_t lo = ~0u, hi = 0u;
      for (int h = 0; h < 2; ++h)
        for (uint64_t mm = h ? m1 : m0; mm; mm &= mm - 1) {
          const uint32_t x = s.w[64 * h + __builtin_ctzll(mm)];
          lo = x < lo ? x : lo;
          hi = x > hi ? x : hi;
        }
      s.f_min[tid] = lo;
      s.f_max[tid] = hi;
      s.f_nmod[tid] = (uint8_t)(__builtin_popcountll(m0 & mod0) + __builtin_popcountll(m1 & mod1));
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t lo = 0, hi = 0;
      for (int f = 0; f < n_free; ++f) {
        s.m_min[f] = lo;
        s.m_max[f] = hi;
        lo += s.f_min[f];
        hi += s.f_max[f];
      }
      s.m_min[n_free] = lo;
      s.m_max[n_free] = hi;
      int all_mod = 0;
      s.all_mod_from[n_free] = 0;
      for (int f = n_free - 1; f >= 0; --f) {
        all_mod += s.f_nmod[f] == s.f_radix[f];
        s.all_mod_from[f] = (uint8_t)all_mod;
      }
      // n_feas: ways[k] = the assignments of the free positions so far with k modified rows, k within the cap
      const int room = mod_cap - s.fixed_mod < n_free ? mod_cap - s.fixed_mod : n_free;
      uint64_t n_feas = 0;
      if (room >= 0) {
        for (int i = 0; i <= room; ++i) s.ways[i] = i == 0;
        for (int f = 0; f < n_free; ++f) {
          const uint64_t with = s.f_nmod[f], without = (uint64_t)s.f_radix[f] - with;
          for (int i = room; i >= 0; --i)
            s.ways[i] = search_sat_add(search_sat_mul(s.ways[i], without), i ? search_sat_mul(s.ways[i - 1], with) : 0);
        }
        for (int i = 0; i <= room; ++i) n_feas = search_sat_add(n_feas, s.ways[i]);
      }
      s.n_feas = n_feas;
    }
    __syncthreads();
    const uint64_t n_feas = s.n_feas;
    if (n_feas == 0) {
      if (tid == 0) a.status[g] = SST_FINAL_INFEASIBLE;
      continue;
    }

    // pass 1: the required fragments
    uint32_t rounds = 0, leaves = 0;
    uint64_t nodes = 0;
    int side = 0;
    bool over = false;
    uint64_t T = H > 65536 ? H : 65536;
    for (;;) {
      ++rounds;
      over = !search_sweep<kPassRequired>(s, a, skel, a0, a1, mod0, mod1, f0, nf_all, L, n_free, mod_cap, T, ws,
                                          x.max_width, tid, leaves, side, nodes);
      if (over || leaves) break;
      if (T == kSearchTMax) {  // (n_feas > 0 and objectives stay below 2^63: not reached)
        over = true;
        break;
      }
      T = T > kSearchTMax / 4 ? kSearchTMax : 4 * T;
    }
    if (over) continue;  // TOO_LARGE
    search_summary(s, lbv, leaves, tid);
    if (s.red.r_best[0] + H > T) {
      const uint64_t again = s.red.r_best[0] + H;
      ++rounds;
      if (!search_sweep<kPassRequired>(s, a, skel, a0, a1, mod0, mod1, f0, nf_all, L, n_free, mod_cap, again, ws,
                                       x.max_width, tid, leaves, side, nodes))
        continue;
      search_summary(s, lbv, leaves, tid);
    }
    const uint64_t best = s.red.r_best[0];
    const uint32_t n_opt = s.red.r_count[0];
    const uint64_t gap = s.red.r_next[0] != kNone64 && s.red.r_next[0] - best <= H ? s.red.r_next[0] - best : H + 1;
    {  // y*: the first leaf at the minimum (the leaves are in index order)
      const uint32_t* rec = ws + (uint64_t)side * kSearchRec * W + s.red.r_first[0];
      for (int p = tid; p < L; p += kFinalWG) {
        const int f = s.kof[p];
        s.rowof[p] = s.p_cnt[p] == 1 ? s.p_first[p] : (uint8_t)(rec[(uint64_t)(f >> 2) * W] >> (8 * (f & 3)));
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t pre = 0;
      for (int p = 0; p < L; ++p) {
        s.pstar[p] = pre;
        pre += s.w[s.rowof[p]];
      }
      s.pstar[L] = pre;
    }
    __syncthreads();
    const uint32_t n_optional = s.n_optional;
    uint64_t cstar = 0, rbest = best, rgap = gap;
    uint32_t rn_opt = n_opt;
    if (n_optional) {  // pass 2: every used fragment, the optional ones' bounds capped at their cost under y*
      uint64_t cst = 0;
      for (int64_t j = tid; j < nf_all; j += kFinalWG) {
        const int64_t at = f0 + j;
        if (!(a.frag_use && a.frag_use[at] == 2)) continue;
        int64_t q = 0;
        uint32_t meta = 0;
        final_qfix(a.frag_su[at], a.prec, q);
        final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
        cst += final_cost(FinalStarPrefix{s.pstar}, q, meta, L);
      }
      if (cst) atomicAdd(&s.cstar, (unsigned long long)cst);
      __syncthreads();
      cstar = s.cstar;
      ++rounds;
      if (!search_sweep<kPassCapped>(s, a, skel, a0, a1, mod0, mod1, f0, nf_all, L, n_free, mod_cap, best + cstar + H,
                                     ws, x.max_width, tid, leaves, side, nodes))
        continue;
      search_summary(s, lbv, leaves, tid);
      rbest = s.red.r_best[0];
      rn_opt = s.red.r_count[0];
      rgap = s.red.r_next[0] != kNone64 && s.red.r_next[0] - rbest <= H ? s.red.r_next[0] - rbest : H + 1;
    }
    if (tid == 0) {
      a.status[g] = SST_FINAL_SOLVED;
      a.n_feas[g] = n_feas;
      a.best[g] = best;
      a.n_opt[g] = n_opt;
      a.gap[g] = gap;
      final_write_robust(x.robust, g, n_optional, cstar, rbest, rn_opt, rgap);
      x.mode[g] = 2;
      x.rounds[g] = rounds;
      x.nodes[g] = nodes;
    }
    for (int p = tid; p < L; p += kFinalWG) a.seq[pos0 + p] = s.rowof[p];
    for (int64_t j = tid; j < nf_all; j += kFinalWG) {
      const int64_t at = f0 + j;
      if (a.frag_use && !a.frag_use[at]) continue;  // (an unused fragment keeps 0xFFFE and 0)
      int64_t q = 0;
      uint32_t meta = 0;
      uint16_t iv = 0xFFFE;
      uint32_t sum = 0;
      final_qfix(a.frag_su[at], a.prec, q);
      final_meta(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
      search_interval(FinalStarPrefix{s.pstar}, q, meta, L, iv, sum);
      a.iv[at] = iv;
      a.sum[at] = sum;
    }
  }
}

}  // namespace

hipError_t launch_final(const sst_final_args& a, const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  const FinalKArgs k{a, w, n_rows};
  const unsigned grid = (unsigned)(a.n_spec < (int64_t)n_wg ? a.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_final_program, dim3(grid), dim3(kFinalWG), 0, st, k);
  return hipGetLastError();
}

hipError_t launch_final_robust(const sst_final_robust_args& r, const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (r.base.n_spec <= 0) return hipSuccess;
  const FinalRobustKArgs k{r, w, n_rows};
  const unsigned grid = (unsigned)(r.base.n_spec < (int64_t)n_wg ? r.base.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_final_robust, dim3(grid), dim3(kFinalWG), 0, st, k);
  return hipGetLastError();
}

uint64_t final_search_ws_words(uint32_t max_width) { return (2ull * kSearchRec + 2) * max_width; }

hipError_t launch_final_search(const sst_final_search_args& x, const int* w, int n_rows, uint32_t* list, uint32_t* ws,
                               int n_wg, hipStream_t st) {
  if (x.robust.base.n_spec <= 0) return hipSuccess;
  const FinalSearchKArgs k{x, w, n_rows, list, ws, final_search_ws_words(x.max_width)};
  hipLaunchKernelGGL(k_final_search_list, dim3(1), dim3(kFinalWG), 0, st, k);
  hipLaunchKernelGGL(k_final_search, dim3((unsigned)n_wg), dim3(kFinalWG), 0, st, k);
  return hipGetLastError();
}

}  // namespace sst
