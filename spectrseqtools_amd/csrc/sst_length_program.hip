// sst_length_program.hip -- the length program by exact enumeration (gfx950): the
// optimal objective value of the program determine_lp_score builds for one
// candidate sequence length (skeleton_building.py:254-289), the only thing
// select_sequence_length_with_lp reads of it (:236-250).  The definition is in
// include/sst.h (sst_length_program_device).
//
// The program holds terminal fragments only, and for a fixed y (one row per
// position) every fragment independently takes the admissible interval whose sum
// is nearest to its mass: the optimum is a minimum over y of a sum of
// per-fragment minima, as the final program's (sst_final.hip), and only the
// minimum is wanted -- no argmin, no count, no gap.
//
// k_length_program: one (spectrum, candidate) pair per workgroup of 256 lanes,
// persistent grid with static striding over the candidate list, lanes over the
// mixed-radix indices of y.  Every piece of per-candidate LDS state is set inside
// the work loop.
//
// Prologue per candidate: the spectrum of the candidate (a search of cand_off);
// one scan of the fragments for a shape that raises, one that is not modelled,
// a mass outside the fixed-point limits; the combined skeleton at length c and
// the position sets A_i (two u64 per position, in LDS), |A_i| and the first row;
// thread 0 then walks the positions once as k_final_program's does (Pbase, k(i),
// the free positions' radices and digit tables, combos); the row-free test at
// length c, one row per thread.
//
// Body: a lane decodes its index into D[k][lane] (the digits' masses summed over
// the first k free positions, P(i) = Pbase(i) + D[k(i)][lane]), counts the
// modified rows and skips y above mod_cap.  The fragment records (qfix, shape,
// range of ends -- computed from the raw ends at c on every load) sit in LDS in
// chunks of kLenF.  A lane stops summing a y once its partial objective reaches
// the smallest objective the workgroup has completed so far (one u64 in LDS,
// lowered by an LDS atomic minimum): costs only add, so such a y cannot lower
// the minimum, and a minimum does not depend on the order it is taken in.  n_feas
// counts every feasible y all the same.  The workgroup ends with a tree reduction
// over the lanes' best and feasible counts.  Every global store is a plain vector
// store of an output element; no global atomics, no scratch buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sst_internal.h"

namespace sst {

namespace {

constexpr int kLenWG = 256;
constexpr int kLenF = 512;        // fragment records per chunk
constexpr int kLenMaxLen = 253;   // as the alignment certificate
constexpr int kLenMaxFree = 22;   // free positions of a candidate of at most 2^22 assignments
constexpr int kLenTable = 512;    // digits of all free positions together
constexpr uint32_t kLenMaxFrag = 16384;
constexpr uint64_t kLenNone64 = ~0ull;
static_assert(SST_FINAL_MAX_COMBOS == 1ull << kLenMaxFree, "every free position has at least two rows");

// a fragment's shape at length c: the admissible intervals _set_x and the contiguity constraints leave
enum { kShapeEmpty = 0, kShapePrefix = 1, kShapeSuffix = 2, kShapeWhole = 3 };
enum { kRuleOk = 0, kRuleRaises = 1, kRuleNotModelled = 2 };

struct LengthLds {
  uint32_t D[kLenMaxFree + 1][kLenWG];  // per lane: its digits' masses over the first k free positions
  unsigned long long r_best[kLenWG];    // the reduction
  uint32_t r_feas[kLenWG];
  int64_t f_q[kLenF];         // a chunk's records: qfix
  uint32_t f_meta[kLenF];     // shape | first end << 8 | last end << 16
  unsigned long long m0[256];  // A_i, rows 1 .. 63 and 64 .. 127
  unsigned long long m1[256];
  uint32_t pbase[256];        // P(i) with every free position at its first row, i in [0, c]
  uint32_t w[SST_MAX_ROWS + 8];
  uint32_t t_delta[kLenTable];  // per digit of a free position: its row's mass above the first row's (mod 2^32)
  uint8_t t_mod[kLenTable];
  uint16_t f_off[kLenMaxFree + 2];  // a free position's first digit in the table
  uint8_t f_radix[kLenMaxFree + 2];
  uint8_t kof[256];           // free positions before position i, i in [0, c]
  uint8_t p_cnt[256];         // |A_i|, and its first row
  uint8_t p_first[256];
  unsigned long long mod[2];  // the table's modified rows
  unsigned long long combos;
  unsigned long long wg_best;  // the smallest objective a lane of the workgroup has completed
  uint32_t flags;             // 1: a fragment raises; 2: one is not modelled; 4: an empty A_i; 8: a row is not free
  uint32_t n_free;
  int32_t fixed_mod;          // modified rows among the positions of one row
};
static_assert(sizeof(LengthLds) <= 54613, "three workgroups per CU (160 KiB of LDS)");

struct LengthKArgs {
  sst_length_program_args a;
  const int* w;
  int n_rows;
};

// qfix of a fragment; false where the model does not hold (u not finite or |u| >= 2^32)
__device__ __forceinline__ bool length_qfix(double su, double prec, int64_t& q) {
  const double u = su / prec;
  if (!(__builtin_fabs(u) < 0x1p32)) return false;  // (NaN and the infinities fail the comparison)
  q = (int64_t)__builtin_rint(u * 65536.0);
  return true;
}

// The shape of a terminal fragment at a sequence of n = max(c, 0) positions, from the walk's raw ends
// (skeleton_building.py:267-276 the ends, linear_program.py:74-102 the fixings; include/sst.h).  meta is set where the
// rule is kRuleOk; its ends are within [0, n - 1].
__device__ __forceinline__ int length_shape(uint8_t code, int32_t min_end, int32_t max_end, int64_t n, uint32_t& meta) {
  const uint32_t cls = (code >> 2) & 3u;
  meta = kShapeWhole;
  if (cls == 3) return kRuleOk;
  if (cls == 1) {  // START: x = 1 on range(mn + 1), then x = 0 on range(mx + 1, n)
    const int64_t mn = (int64_t)min_end - 1, mx = (int64_t)max_end - 1;
    if (mn >= n || mx + 1 < -n) return kRuleRaises;
    if (mx + 1 <= 0) {  // the zeros wrap over every position
      meta = kShapeEmpty;
      return kRuleOk;
    }
    if (mn < 0) return kRuleNotModelled;  // no x is fixed to 1
    const int64_t lo = mn < mx ? mn : mx, hi = mx < n - 1 ? mx : n - 1;
    meta = kShapePrefix | (uint32_t)lo << 8 | (uint32_t)hi << 16;
    return kRuleOk;
  }
  if (cls == 2) {  // END: x = 0 on range(mx), then x = 1 on range(mn, n)
    const int64_t mn = n - (int64_t)min_end, mx = n - (int64_t)max_end;
    if (mx > n || mn < -n) return kRuleRaises;
    if (mn < 0) return kRuleOk;  // the ones wrap over every position: WHOLE
    if (mn >= n) {               // no x is fixed to 1
      if (mx != n) return kRuleNotModelled;
      meta = kShapeEmpty;        // every x is fixed to 0
      return kRuleOk;
    }
    const int64_t m = mx < mn ? mx : mn, lo = m > 0 ? m : 0;
    meta = kShapeSuffix | (uint32_t)lo << 8 | (uint32_t)mn << 16;
    return kRuleOk;
  }
  return kRuleNotModelled;  // a fragment of neither side is no terminal fragment
}

__device__ __forceinline__ uint32_t length_prefix(const LengthLds& s, int i, int tid) {
  return s.pbase[i] + s.D[s.kof[i]][tid];
}

__device__ __forceinline__ uint64_t length_dist(int64_t q, uint32_t sum) {
  const int64_t d = q - (int64_t)((uint64_t)sum << 16);
  return (uint64_t)(d < 0 ? -d : d);
}

// c_j(y) of the lane's y
__device__ __forceinline__ uint64_t length_cost(const LengthLds& s, int tid, int64_t q, uint32_t meta, int L) {
  const uint32_t shape = meta & 3u;
  const int lo = (int)((meta >> 8) & 0xffu), hi = (int)((meta >> 16) & 0xffu);
  if (shape == kShapeWhole) return length_dist(q, length_prefix(s, L, tid));
  if (shape == kShapeEmpty) return (uint64_t)(q < 0 ? -q : q);
  uint64_t best = kLenNone64;
  if (shape == kShapePrefix) {
    for (int r = lo; r <= hi; ++r) {
      const uint64_t c = length_dist(q, length_prefix(s, r + 1, tid));
      best = c < best ? c : best;
    }
    return best;
  }
  const uint32_t total = length_prefix(s, L, tid);
  for (int l = lo; l <= hi; ++l) {
    const uint64_t c = length_dist(q, total - length_prefix(s, l, tid));
    best = c < best ? c : best;
  }
  return best;
}

// The lane's column of D from the index of a y; returns its modified rows among the free positions.
__device__ __forceinline__ int length_decode(LengthLds& s, uint32_t idx, int n_free, int tid) {
  int mods = 0;
  uint32_t rem = idx;
  for (int f = n_free - 1; f >= 0; --f) {
    const uint32_t radix = s.f_radix[f], d = rem % radix;
    rem /= radix;
    const int e = (int)s.f_off[f] + (int)d;
    s.D[f + 1][tid] = s.t_delta[e];
    mods += s.t_mod[e];
  }
  uint32_t acc = 0;
  s.D[0][tid] = 0;
  for (int f = 0; f < n_free; ++f) {
    acc += s.D[f + 1][tid];
    s.D[f + 1][tid] = acc;
  }
  return mods;
}

// The four outputs of candidate k (one thread).
__device__ __forceinline__ void length_write(const sst_length_program_args& a, int64_t k, int tid, uint8_t status,
                                             uint64_t combos, uint64_t n_feas, uint64_t best) {
  if (tid == 0) {
    a.status[k] = status;
    a.combos[k] = combos;
    a.n_feas[k] = n_feas;
    a.best[k] = best;
  }
}

}  // namespace

__global__ __launch_bounds__(kLenWG) void k_length_program(LengthKArgs k) {
  __shared__ LengthLds s;
  const sst_length_program_args& a = k.a;
  const int tid = (int)threadIdx.x;
  const int n_rows = k.n_rows;

  // the table: the same for every candidate
  for (int r = tid; r < SST_MAX_ROWS + 8; r += kLenWG) s.w[r] = r < n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;
  if (n_rows < 64) {
    rows0 &= (1ull << n_rows) - 1;
    rows1 = 0;
  } else if (n_rows < 128) {
    rows1 = (1ull << (n_rows - 64)) - 1;
  }
  if (tid < 2) s.mod[tid] = 0;
  __syncthreads();
  for (int r = 1 + tid; r < n_rows && r < 128; r += kLenWG)
    if (a.row_mod[r]) atomicOr(&s.mod[r >> 6], 1ull << (r & 63));
  __syncthreads();
  const uint64_t mod0 = s.mod[0], mod1 = s.mod[1];

  for (int64_t kc = blockIdx.x; kc < a.n_cand; kc += gridDim.x) {
    __syncthreads();  // the previous candidate's LDS is no longer read
    if (tid == 0) {
      s.flags = 0;
      s.wg_best = kLenNone64;
    }
    __syncthreads();
    if (!a.valid[kc]) {  // never chosen, never updates best_val: nothing is computed
      length_write(a, kc, tid, SST_LEN_INVALID, 0, 0, 0);
      continue;
    }
    // the candidate's spectrum: the largest g with cand_off[g] <= kc
    int64_t g = 0;
    for (int64_t hi = a.n_spec - 1; g < hi;) {
      const int64_t mid = g + (hi - g + 1) / 2;
      if (a.cand_off[mid] <= kc) g = mid;
      else hi = mid - 1;
    }
    const int64_t c64 = a.cand_len[kc];
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    const int M = a.max_len[g];

    // the fragments at this length: one that raises, one outside the model
    {
      uint32_t bits = 0;
      const int64_t n = c64 > 0 ? c64 : 0;
      for (int64_t j = tid; j < nf_all; j += kLenWG) {
        const int64_t at = f0 + j;
        int64_t q;
        uint32_t meta;
        const int rule = length_shape(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], n, meta);
        bits |= rule == kRuleRaises ? 1u : rule == kRuleNotModelled ? 2u : 0u;
        if (!length_qfix(a.frag_su[at], a.prec, q)) bits |= 2u;
      }
      if (bits) atomicOr(&s.flags, bits);
    }
    __syncthreads();
    if (s.flags & 1u) {  // the constructor raises: the value is +inf
      length_write(a, kc, tid, SST_LEN_RAISES, 0, 0, 0);
      continue;
    }
    if (c64 < 1 || c64 > kLenMaxLen || c64 > (int64_t)M || nf_all <= 0 || nf_all > (int64_t)kLenMaxFrag ||
        (s.flags & 2u)) {
      length_write(a, kc, tid, SST_LEN_NOT_MODELLED, 0, 0, 0);
      continue;
    }
    const int L = (int)c64;  // 1 <= L <= min(M, 253)
    const uint64_t* st = a.skeleton + 2 * a.skel_off[g];  // S_0 .. S_{M-1}, then the reversed END skeleton E_0 .. E_{M-1}
    const uint64_t* en = st + 2 * (int64_t)M;
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    const int mod_cap = a.mod_cap[kc];

    // the combined skeleton at L and its position sets
    for (int p = tid; p < L; p += kLenWG) {
      const int e = M - L + p;
      const uint64_t s0 = st[2 * p], s1 = st[2 * p + 1], e0 = en[2 * e], e1 = en[2 * e + 1];
      uint64_t c0 = s0 & e0, c1 = s1 & e1;  // the intersection, else the union
      if (!(c0 | c1)) {
        c0 = s0 | e0;
        c1 = s1 | e1;
      }
      const uint64_t m0 = (c0 | c1) ? c0 & a0 : a0, m1 = (c0 | c1) ? c1 & a1 : a1;
      const int cnt = __builtin_popcountll(m0) + __builtin_popcountll(m1);
      s.m0[p] = m0;
      s.m1[p] = m1;
      s.p_cnt[p] = (uint8_t)cnt;
      s.p_first[p] = (uint8_t)(m0 ? __builtin_ctzll(m0) : m1 ? 64 + __builtin_ctzll(m1) : 0);
      if (cnt == 0) atomicOr(&s.flags, 4u);
    }
    __syncthreads();
    if (s.flags & 4u) {  // (combos = prod |A_i| = 0)
      length_write(a, kc, tid, SST_LEN_INFEASIBLE, 0, 0, 0);
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
        combos = combos > kLenNone64 / (uint64_t)cnt ? kLenNone64 : combos * (uint64_t)cnt;
        if (cnt == 1) {
          fixed_mod += (int)(((first < 64 ? mod0 : mod1) >> (first & 63)) & 1u);
        } else if (!over) {
          if (n_free == kLenMaxFree || t_n + cnt > kLenTable) {
            over = true;
            continue;
          }
          s.f_off[n_free] = (uint16_t)t_n;
          s.f_radix[n_free] = (uint8_t)cnt;
          for (int h = 0; h < 2; ++h)
            for (uint64_t m = h ? s.m1[p] : s.m0[p]; m; m &= m - 1) {
              const int bit = __builtin_ctzll(m), row = 64 * h + bit;
              s.t_delta[t_n] = s.w[row] - s.w[first];
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
    // the row-free test at length L: one row of alpha per thread, n_r counted over the positions' sets
    for (int r = 1 + tid; r < n_rows; r += kLenWG) {
      const uint64_t bit = 1ull << (r & 63);
      if (!((r < 64 ? a0 : a1) & bit)) continue;
      int n_r = 0;
      for (int p = 0; p < L; ++p) n_r += ((r < 64 ? s.m0[p] : s.m1[p]) & bit) != 0;
      const int cap = a.row_cap[(int64_t)L * n_rows + r];
      const bool modified = ((r < 64 ? mod0 : mod1) & bit) != 0;
      if (!(cap >= n_r || (modified && cap >= mod_cap))) atomicOr(&s.flags, 8u);
    }
    __syncthreads();
    const uint64_t combos = s.combos;
    if (s.flags & 8u) {
      length_write(a, kc, tid, SST_LEN_NOT_FREE, combos, 0, 0);
      continue;
    }
    if (combos > a.max_combos) {
      length_write(a, kc, tid, SST_LEN_TOO_LARGE, combos, 0, 0);
      continue;
    }

    // the enumeration: combos <= 2^22, every free position is recorded
    const int n_free = (int)s.n_free, fixed_mod = s.fixed_mod;
    const int n_chunks = (int)((nf_all + kLenF - 1) / kLenF);
    uint64_t best = kLenNone64;
    uint32_t feas = 0;
    for (uint32_t base = 0; base < (uint32_t)combos; base += kLenWG) {
      const uint32_t idx = base + (uint32_t)tid;
      bool ok = idx < (uint32_t)combos;
      if (ok) ok = fixed_mod + length_decode(s, idx, n_free, tid) <= mod_cap;
      // the smallest completed objective so far; any value read here was achieved, so stopping at it is safe
      const uint64_t bound = *(volatile unsigned long long*)&s.wg_best;
      uint64_t obj = 0;
      bool live = ok;  // the objective is still summed
      for (int ch = n_chunks - 1; ch >= 0; --ch) {  // the last fragments first: the heavy ones tell the y apart
        const int nf = (int)(nf_all - (int64_t)ch * kLenF < kLenF ? nf_all - (int64_t)ch * kLenF : kLenF);
        if (n_chunks > 1 || base == 0) {
          __syncthreads();  // the previous chunk's records are no longer read
          for (int j = tid; j < nf; j += kLenWG) {
            const int64_t at = f0 + (int64_t)ch * kLenF + j;
            int64_t q = 0;
            uint32_t meta = kShapeWhole;
            length_qfix(a.frag_su[at], a.prec, q);  // (within the model: checked above)
            length_shape(a.frag_code[at], a.frag_min_end[at], a.frag_max_end[at], L, meta);
            s.f_q[j] = q;
            s.f_meta[j] = meta;
          }
          __syncthreads();
        }
        if (live)
          for (int j = nf - 1; j >= 0 && live; --j) {
            obj += length_cost(s, tid, s.f_q[j], s.f_meta[j], L);
            live = obj < bound;  // costs only add: at the bound or above, y cannot lower the minimum
          }
      }
      if (ok) ++feas;
      if (live) {  // obj < bound <= best
        best = obj;
        atomicMin(&s.wg_best, (unsigned long long)obj);
      }
    }
    s.r_best[tid] = best;
    s.r_feas[tid] = feas;
    __syncthreads();
    for (int stride = kLenWG / 2; stride > 0; stride >>= 1) {
      if (tid < stride) {
        const unsigned long long b1 = s.r_best[tid], b2 = s.r_best[tid + stride];
        s.r_best[tid] = b1 < b2 ? b1 : b2;
        s.r_feas[tid] += s.r_feas[tid + stride];
      }
      __syncthreads();
    }
    const uint32_t n_feas = s.r_feas[0];
    if (n_feas == 0)
      length_write(a, kc, tid, SST_LEN_INFEASIBLE, combos, 0, 0);
    else
      length_write(a, kc, tid, SST_LEN_SOLVED, combos, n_feas, s.r_best[0]);
  }
}

hipError_t launch_length_program(const sst_length_program_args& a, const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0 || a.n_cand <= 0) return hipSuccess;
  const LengthKArgs k{a, w, n_rows};
  const unsigned grid = (unsigned)(a.n_cand < (int64_t)n_wg ? a.n_cand : (int64_t)n_wg);
  hipLaunchKernelGGL(k_length_program, dim3(grid), dim3(kLenWG), 0, st, k);
  return hipGetLastError();
}

}  // namespace sst
