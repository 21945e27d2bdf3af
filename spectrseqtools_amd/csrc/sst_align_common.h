// sst_align_common.h -- what the alignment certificate's kernels share
// (sst_align.hip, sst_align_caps.hip): the LDS records of a chunk of fragments,
// the searches, the position sets and the match of an interval's list against
// the chunk.  Every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sst_internal.h"
#include "sst_quant.h"

namespace sst {

namespace {

constexpr int kAlignWaves = 4;
constexpr int kAlignWG = 64 * kAlignWaves;
constexpr int kAlignK = (int)SST_ALIGN_CAPACITY;  // entries of a closed interval's list
constexpr int kAlignF = 384;                      // fragment records per chunk
constexpr int kAlignMaxLen = 253;                 // sums fit u32, (l, r) fits 2 x 8 bits next to 0xFF
constexpr int kAlignWaveWords = 4 * kAlignK;      // list A, list B (K each), merge temp (2 K)
constexpr int64_t kAlignClamp = (int64_t)1 << 61;

struct AlignLds {  // carved from the dynamic LDS behind the waves' lists
  int64_t f_t[kAlignF];      // target
  int64_t f_w[kAlignF];      // W
  uint32_t f_meta[kAlignF];  // class | skipped << 2 | min_end << 8 | max_end << 16
  uint32_t f_nfit[kAlignF];
  uint32_t f_first[kAlignF];
  uint32_t f_open[kAlignF];
  uint32_t p_min[256];       // per position: smallest / largest mass of A_i
  uint32_t p_max[256];
  uint32_t w[SST_MAX_ROWS + 8];
  unsigned long long w_max;  // largest W of the chunk
  uint32_t flags;            // 1: an empty A_i; 2: targets not ascending; 16 << class: class present
};

constexpr size_t kAlignLdsBytes = (size_t)kAlignWaves * kAlignWaveWords * 4 + sizeof(AlignLds);
static_assert(2 * kAlignLdsBytes <= kCuLdsBytes, "two workgroups per CU");

__device__ __forceinline__ void wave_sync() {  // LDS written by some lanes of this wave, read by others
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int64_t clamp_f(double x) {  // exact for |x| < 2^61; NaN -> -2^61
  if (!(x > -0x1p61)) return -kAlignClamp;
  if (x > 0x1p61) return kAlignClamp;
  return (int64_t)x;
}

// entries of a[0, n) below v (a ascending)
__device__ __forceinline__ int lower_u32(const uint32_t* a, int n, uint32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// entries of a[0, n) not above v
__device__ __forceinline__ int upper_u32(const uint32_t* a, int n, uint32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int lower_i64(const int64_t* a, int n, int64_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// A_i of position i: P_i & alpha where P_i != 0, else alpha; row 0 excluded
__device__ __forceinline__ void position_set(const uint64_t* skel, int64_t at, uint64_t a0, uint64_t a1, uint64_t& m0,
                                             uint64_t& m1) {
  const uint64_t p0 = skel[2 * at], p1 = skel[2 * at + 1];
  if (p0 | p1) {
    m0 = p0 & a0;
    m1 = p1 & a1;
  } else {
    m0 = a0;
    m1 = a1;
  }
}

struct Interval {
  int l, r;        // (0xFF, 0xFF): the empty interval
  int64_t lo, hi;  // LO, HI
  bool open;
  const uint32_t* list;
  int n;
};

// Every fragment of the chunk the interval is admissible for: fit / open.
// mode 0: a forward sweep (internal, START, START_END), 1: the backward sweep
// (END), 2: the empty interval (internal; START_END where L == 0).
__device__ __forceinline__ void match_fragments(AlignLds& s, int nf, const Interval& iv, int mode, int L, int lane) {
  const bool cut = !(s.flags & 2u);
  const int64_t wm = (int64_t)s.w_max;
  const int j0 = cut ? lower_i64(s.f_t, nf, iv.lo - wm) : 0;
  const int j1 = cut ? lower_i64(s.f_t, nf, iv.hi + wm + 1) : nf;
  for (int j = j0 + lane; j < j1; j += 64) {
    const uint32_t meta = s.f_meta[j];
    if (meta & 4u) continue;
    const int cls = (int)(meta & 3u), mn = (int)((meta >> 8) & 0xffu), mx = (int)((meta >> 16) & 0xffu);
    bool ok;
    if (mode == 0)
      ok = cls == 0 || (cls == 1 && iv.l == 0 && iv.r >= (mn < mx ? mn : mx) && iv.r <= mx) ||
           (cls == 3 && iv.l == 0 && iv.r == L - 1);
    else if (mode == 1)
      ok = cls == 2 && iv.l >= (mn < mx ? mn : mx) && iv.l <= mn;
    else
      ok = cls == 0 || (cls == 3 && L == 0);
    if (!ok || s.f_w[j] < 0) continue;  // W < 0: an empty window
    const int64_t flo = s.f_t[j] - s.f_w[j], fhi = s.f_t[j] + s.f_w[j];
    if (fhi < iv.lo || flo > iv.hi) continue;
    if (iv.open) {
      atomicOr(&s.f_open[j], 1u);
      continue;
    }
    const uint32_t a = flo > iv.lo ? (uint32_t)(flo - iv.lo) : 0u;  // <= HI - LO < 2^32
    const int at = lower_u32(iv.list, iv.n, a);
    if (at < iv.n && (int64_t)iv.list[at] <= fhi - iv.lo) {
      atomicAdd(&s.f_nfit[j], 1u);
      atomicMin(&s.f_first[j], (uint32_t)(iv.l << 8 | iv.r));
    }
  }
}

struct AlignKArgs {
  sst_align_args a;
  const int* w;  // the table's integer row masses
  int n_rows;
  double rprec;
};

constexpr int kSplitWaves = 3;
constexpr int kSplitWG = 64 * kSplitWaves;
constexpr int kSplitWaveWords = 5 * kAlignK;  // three lists of K (A, and B's two), merge temp (2 K)

struct SplitLds {  // behind the waves' lists
  AlignLds s;                 // the chunk's records: base-OPEN fragments only, in their original order
  int64_t f_at[kAlignF];      // a record's fragment, from the spectrum's first
  uint32_t wave_n[kSplitWaves];
};

constexpr size_t kSplitLdsBytes = (size_t)kSplitWaves * kSplitWaveWords * 4 + sizeof(SplitLds);
static_assert(2 * kSplitLdsBytes <= kCuLdsBytes, "two workgroups per CU");
static_assert(kAlignF >= kSplitWG, "a chunk takes at least one block of the status scan");
static_assert(SST_MAX_ROWS <= kAlignK, "one position is closed, so the first list is never empty");

// (k_align_windows keeps the next two steps in its own body, so that the code
// it compiles to stays what it was; the other three kernels call these.)
// Position p's smallest / largest mass of A_i into p_min / p_max; flags bit 0 if A_i is empty.
__device__ __forceinline__ void position_range(AlignLds& s, const uint64_t* skel, int64_t pos0, int p, uint64_t a0,
                                               uint64_t a1) {
  uint64_t m0, m1;
  position_set(skel, pos0 + p, a0, a1, m0, m1);
  const int cnt = __builtin_popcountll(m0) + __builtin_popcountll(m1);
  uint32_t lo = 0xffffffffu, hi = 0;
  for (uint64_t m = m0; m; m &= m - 1) {
    const uint32_t x = s.w[__builtin_ctzll(m)];
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
  }
  for (uint64_t m = m1; m; m &= m - 1) {
    const uint32_t x = s.w[64 + __builtin_ctzll(m)];
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
  }
  s.p_min[p] = lo;
  s.p_max[p] = hi;
  if (cnt == 0) atomicOr(&s.flags, 1u);
}

// Record j of the chunk from fragment `at`: target, W, class / ends, cleared results; the chunk's flags and w_max.
__device__ __forceinline__ void load_record(AlignLds& s, int j, int64_t at, const sst_align_args& a, double rprec, int L) {
  const int64_t t = clamp_f(rint_quot(a.frag_su[at], a.prec, rprec));
  int64_t w = clamp_f(ceil_quot(a.tol * a.frag_obs[at], a.prec, rprec));
  if (w < 0) w = -1;  // a negative W: nothing fits (|s - target| <= W has no solution)
  const uint32_t cls = (a.frag_code[at] >> 2) & 3u;
  const int mn = a.frag_min_end[at], mx = a.frag_max_end[at];
  const bool skipped = (cls == 1 || cls == 2) && (mn < 0 || mn >= L || mx < 0 || mx >= L);
  s.f_t[j] = t;
  s.f_w[j] = w;
  s.f_meta[j] = cls | (skipped ? 4u : 0u) | (skipped ? 0u : ((uint32_t)mn & 0xffu) << 8 | ((uint32_t)mx & 0xffu) << 16);
  s.f_nfit[j] = 0;
  s.f_first[j] = 0xffffffffu;
  s.f_open[j] = 0;
  if (!skipped) atomicOr(&s.flags, 16u << cls);
  if (w > 0) atomicMax(&s.w_max, (unsigned long long)w);
}

}  // namespace

}  // namespace sst
