// sst_align.hip -- the alignment certificate (gfx950): which surviving
// fragments of a spectrum no window of its skeleton can explain, the question
// filter_with_lp (prediction.py:229-259) asks one LinearProgramInstance per
// fragment (linear_program.py).  The definition is in include/sst.h
// (sst_align_windows_device and the five entry points behind it).
//
// Two kernel bodies, each compiled with and without the program's universal
// modification cap (template parameter kCaps; Variant<> holds what differs),
// and under the cap also in keep mode (kKeep, below):
//
//   align_windows  k_align_windows, k_align_windows_caps: one spectrum per
//                  workgroup, persistent grid over spectra.
//   align_split    k_align_split, k_align_split_caps: the two-list split of the
//                  open intervals over the former's outputs.
//
// The capped certificate is the general one.  Every list entry is a sum's u32
// offset and, beside it, one u8: the sum's smallest excess (modified rows
// chosen beyond the interval's forced positions).  Without the cap there are no
// excess bytes, every cost is 0 and nothing ever leaves a list; the code that
// touches them is compiled out (if constexpr), nothing is decided at run time.
//
// Per position the workgroup first derives A_i's smallest and largest row mass
// (LDS); an empty A_i ends the spectrum (INFEASIBLE).  Under the cap the pass
// also derives, per position, "forced" (every row of A_i is modified) and "the
// smallest mass pays" (not forced, and no unmodified row has the position's
// smallest mass), and counts the forced positions F; F > mod_cap is INFEASIBLE,
// else E = mod_cap - F (<= 253).
// The fragments are taken in chunks of kAlignF records held in LDS (target,
// W, class / ends, and the three result words n_fit, first, open), so a
// spectrum of any fragment count runs, one sweep set per chunk.
//
// Waves take sweeps round robin: "forward from l" for every left end l
// (interior left ends only when the chunk has internal fragments), one
// "backward from L - 1" for the END class (its intervals all end at L - 1), and
// the empty interval.  A sweep keeps S_E(l, r) as a sorted list of distinct u32
// offsets from LO(l, r) in the wave's LDS slice; LO and HI are 64-bit scalars
// (the uncapped sums of minima and maxima: a conservative cut only).
// Extending by a position adds its minimum to LO; a position of one mass
// changes nothing else (it costs nothing: forced, or an unmodified row has it).
// A position of several masses unions one shifted copy of the list per further
// row, one at a time: offset + d, excess + c with c = row_mod - forced.  The
// copy of the smallest mass stays the list itself unless that mass pays: then
// the union starts empty and the unshifted copy is merged like any other, with
// c = 1.  A union is a stable rank merge into the wave's 2 K temp (each lane
// places its elements by binary search in the other list, the excess bytes
// travel along), then a ballot / mbcnt compaction that drops equal neighbours,
// keeping the smaller excess of the two, and drops what is above E, so what is
// stored and counted is S_E only.  (A copy with c > E is empty and is skipped.)
// The first union above K entries makes the sweep open for good (|S_E| never
// shrinks when an interval grows): from there only LO and HI move.
//
// Per interval the wave cuts the chunk's fragments (ascending targets) by
// binary search to those whose target lies in [LO - Wmax, HI + Wmax], then
// each lane tests one fragment: class admissibility, window against [LO, HI],
// and a binary search of the list for the first offset >= target - W - LO.
// Results combine with LDS atomics (add, min, or).  A sweep ends early once
// LO - Wmax passes the largest target (row masses are >= 0, so LO never
// falls).  A chunk whose targets are not ascending is not cut and its sweeps
// do not end early: still exact, only slower.
//
// The split: the workgroup scans the spectrum's status bytes and compacts the
// base-OPEN fragments, in their order, into the same LDS records (a chunk is
// closed once fewer than a scan block's worth of records are free); a spectrum
// without one costs that scan only.  The sweeps are the former's, over open
// intervals only: phase A builds the list up to the last closed interval
// [l, m*] and matches nothing; phase B starts a fresh list at m* + 1 (its
// excess against its own forced positions).  While it is closed, [l, r] is
// split-closed: the wave takes the cut's fragments one at a time, lanes over
// the entries a of A within [lo' - max(B), hi'], each searching B for the first
// entry >= lo' - a, and a ballot says whether any pair fits.  Under the cap a
// pair fits only if its two excesses together stay within E, so the lane walks
// B's entries inside its window until one is within E - e_a.  (Lanes over
// fragments would leave most of the wave idle, a spectrum has few OPEN
// fragments, and would walk A serially.)  Once B passes K every further
// interval of the sweep is undecided and only marks windows that meet [LO, HI].
//
// LDS per workgroup, two workgroups per CU in every variant (Variant<> asserts
// it, and that one more wave would cost the second workgroup under the cap):
//   k_align_windows       4 waves x 16 KiB of lists (A, B, 2 K of merge temp)
//                         + 12 KiB of records + 2.5 KiB of tables = 78.5 KiB
//   k_align_split         3 waves x 20 KiB (A, B's two lists, merge temp) + the
//                         same + 3 KiB of record -> fragment indices = 77.5 KiB
//   k_align_windows_caps  the bytes raise a wave's lists to 20 KiB: 3 waves,
//                         60 + 15.2 = 75.2 KiB (4 waves: 80 + 15, one workgroup)
//   k_align_split_caps    25 KiB a wave: 2 waves, 50 + 18.2 = 68.2 KiB
//   k_align_windows_keep, k_align_split_keep: the caps kernels' + 1.5 KiB
// Every global store is a plain vector store of an output element; the only
// atomics are LDS atomics.
//
// Keep mode (a third compile-time axis, kKeep, which requires kCaps: k_align_
// windows_keep, k_align_split_keep; nothing of it is decided at run time in the
// four kernels above).  Once per spectrum, one row per thread counts n_r, the
// positions whose set holds the row, and tests it against row_cap[L * n_rows +
// r]: the spectrum is row-free iff every row of alpha is free (the split reads
// the base kernel's spec_free instead).  A record carries W - W_in in two spare
// bits of f_meta and one more word, f_keep: where the search for W hits in a
// row-free spectrum, the first entry >= target - W_in - LO is at most two
// entries further (distinct integers, W - W_in <= 2), and if it is <= target +
// W_in - LO the interval joins f_keep by an LDS min.  The split's walk over B
// goes on until an entry within budget also lies in the inner window.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sst_internal.h"
#include "sst_quant.h"

namespace sst {

namespace {

constexpr int kAlignK = (int)SST_ALIGN_CAPACITY;  // entries of a closed interval's list
constexpr int kAlignF = 384;                      // fragment records per chunk
constexpr int kAlignMaxLen = 253;                 // sums fit u32, (l, r) fits 2 x 8 bits next to 0xFF
constexpr int64_t kAlignClamp = (int64_t)1 << 61;
static_assert(SST_MAX_ROWS <= kAlignK, "one position is closed, so the first list is never empty");
static_assert(kAlignMaxLen + 1 <= 255, "an excess and one more fit a byte");

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

struct SplitLds {  // the split's records
  AlignLds s;             // the chunk's records: base-OPEN fragments only, in their original order
  int64_t f_at[kAlignF];  // a record's fragment, from the spectrum's first
  uint32_t wave_n[3];     // (the widest split workgroup's waves)
};

struct CapsLds {  // behind AlignLds / SplitLds, under the cap only
  unsigned long long mod[2];  // the table's modified rows as two masks
  uint32_t n_forced;          // F
  uint8_t p_flag[256];        // per position: 1 forced, 2 the smallest mass pays
};

struct KeepLds {  // behind CapsLds, in keep mode only
  uint32_t f_keep[kAlignF];  // per record: l << 8 | r of the smallest interval with an inner fit
  uint32_t row_bad;          // some row of alpha is not free
  uint32_t pad;
};

// What differs between the six kernels, at compile time: the waves of a
// workgroup, the bytes of a wave's slice of lists and the LDS structs behind them.
template <bool kSplit_, bool kCaps_, bool kKeep_ = false>
struct Variant {
  static constexpr bool kSplit = kSplit_, kCaps = kCaps_, kKeep = kKeep_;
  static_assert(kCaps || !kKeep, "keep mode decides on the capped lists");
  static constexpr int kWaves = kSplit ? (kCaps ? 2 : 3) : (kCaps ? 3 : 4);
  static constexpr int kWG = 64 * kWaves;
  static constexpr int kLists = kSplit ? 5 : 4;  // K entries each: A, B (the split: B's two), 2 K of merge temp
  static constexpr int kWaveBytes = kLists * kAlignK * (kCaps ? 5 : 4);  // u32 offsets, then one u8 per entry
  using Records = std::conditional_t<kSplit, SplitLds, AlignLds>;
  static constexpr size_t kRecordsAt = (size_t)kWaves * kWaveBytes;
  static constexpr size_t kCapsAt = kRecordsAt + sizeof(Records);
  static constexpr size_t kKeepAt = kCapsAt + sizeof(CapsLds);
  static constexpr size_t kLdsBytes = kCapsAt + (kCaps ? sizeof(CapsLds) : 0) + (kKeep ? sizeof(KeepLds) : 0);
  static_assert(2 * kLdsBytes <= kCuLdsBytes, "two workgroups per CU");
  static_assert(!kCaps || (size_t)(kWaves + 1) * kWaveBytes + sizeof(Records) > kCuLdsBytes / 2,
                "one more wave would cost the second workgroup");
  static_assert(kWaveBytes % 8 == 0 && sizeof(Records) % 8 == 0 && sizeof(CapsLds) % 8 == 0,
                "the records behind the lists stay aligned");
  static_assert(!kSplit || (kAlignF >= kWG && kWaves <= 3),
                "a chunk takes at least one block of the status scan; SplitLds serves every split workgroup");
};

template <bool kCaps>
struct List {
  uint32_t* v;  // offsets from LO, ascending and distinct
};
template <>
struct List<true> {
  uint32_t* v;
  uint8_t* e;  // the smallest excess that reaches each
};

// List i of a wave's slice: the u32 offsets first, the excess bytes behind all of them.
template <class V>
__device__ __forceinline__ List<V::kCaps> list_at(uint8_t* mine, int i) {
  List<V::kCaps> l;
  l.v = reinterpret_cast<uint32_t*>(mine) + i * kAlignK;
  if constexpr (V::kCaps) l.e = mine + (4 * V::kLists + i) * kAlignK;
  return l;
}

struct AlignKArgs {
  sst_align_args a;
  const int* w;  // the table's integer row masses
  int n_rows;
  double rprec;
};

struct AlignCapsKArgs {
  AlignKArgs k;
  sst_align_caps c;
};

struct AlignKeepKArgs {
  AlignCapsKArgs kc;
  sst_align_keep kp;
};

template <bool kCaps>
struct CapState {};
template <>
struct CapState<true> {
  const uint8_t* p_flag;  // CapsLds::p_flag
  uint64_t mod0, mod1;    // the table's modified rows
  uint32_t E;             // the spectrum's budget beyond its forced positions
  uint32_t* f_keep;       // KeepLds::f_keep            (these two: set and read in keep mode only)
  bool row_free;          // every row of alpha is free: S_E is the program's set of sums
};

template <bool kCaps>
struct Spectrum : CapState<kCaps> {  // what the sweeps need of the spectrum (wave-uniform)
  const uint64_t* skel;              // its first position
  uint64_t a0, a1;                   // alpha, rows 1 .. n_rows - 1
  int L;
};

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

// A_i of position p: P_i & alpha where P_i != 0, else alpha; row 0 excluded
template <bool kCaps>
__device__ __forceinline__ void position_set(const Spectrum<kCaps>& sp, int p, uint64_t& m0, uint64_t& m1) {
  const uint64_t p0 = sp.skel[2 * p], p1 = sp.skel[2 * p + 1];
  if (p0 | p1) {
    m0 = p0 & sp.a0;
    m1 = p1 & sp.a1;
  } else {
    m0 = sp.a0;
    m1 = sp.a1;
  }
}

// Once per workgroup: the table's row masses into LDS, the masks of rows
// 1 .. n_rows - 1 and, under the cap, of the modified rows among them (one row
// per thread; row 0 is in no A_i).  Ends on a barrier under the cap.
template <class V>
__device__ __forceinline__ void load_table(AlignLds& s, CapsLds* cl, const AlignKArgs& k, const sst_align_caps& c,
                                           int tid, uint64_t& rows0, uint64_t& rows1, Spectrum<V::kCaps>& sp) {
  for (int r = tid; r < SST_MAX_ROWS + 8; r += V::kWG) s.w[r] = r < k.n_rows ? (uint32_t)k.w[r] : 0u;
  rows0 = ~1ull;
  rows1 = ~0ull;
  if (k.n_rows < 64) {
    rows0 &= (1ull << k.n_rows) - 1;
    rows1 = 0;
  } else if (k.n_rows < 128) {
    rows1 = (1ull << (k.n_rows - 64)) - 1;
  }
  if constexpr (V::kCaps) {
    if (tid < 2) cl->mod[tid] = 0;
    __syncthreads();
    for (int r = 1 + tid; r < k.n_rows && r < 128; r += V::kWG)
      if (c.row_mod[r]) atomicOr(&cl->mod[r >> 6], 1ull << (r & 63));
    __syncthreads();
    sp.mod0 = cl->mod[0];
    sp.mod1 = cl->mod[1];
    sp.p_flag = cl->p_flag;
  }
}

// Position p's smallest / largest mass of A_i into p_min / p_max; flags bit 0
// if A_i is empty.  Under the cap also the position's two flags and its share of F.
template <bool kCaps>
__device__ __forceinline__ void position_range(AlignLds& s, CapsLds* cl, const Spectrum<kCaps>& sp, int p) {
  uint64_t m0, m1;
  position_set(sp, p, m0, m1);
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
  if constexpr (kCaps) {
    const uint64_t u0 = m0 & ~sp.mod0, u1 = m1 & ~sp.mod1;  // the unmodified rows of A_i
    const bool forced = !(u0 | u1);
    bool pays = !forced;
    for (uint64_t m = u0; m; m &= m - 1) pays = pays && s.w[__builtin_ctzll(m)] != lo;
    for (uint64_t m = u1; m; m &= m - 1) pays = pays && s.w[64 + __builtin_ctzll(m)] != lo;
    cl->p_flag[p] = (uint8_t)((forced ? 1u : 0u) | (pays ? 2u : 0u));
    if (forced) atomicAdd(&cl->n_forced, 1u);
  }
}

// E of a spectrum with `forced` <= cap forced positions
__device__ __forceinline__ uint32_t budget(int cap, int forced) {
  return (uint32_t)(cap - forced < kAlignMaxLen ? cap - forced : kAlignMaxLen);
}

// floor(num / den) on the IEEE f64 quotient, as ceil_quot (sst_quant.h) takes the ceiling
__device__ __forceinline__ double floor_quot(double num, double den, double rden) {
  if (num == 0.0) return 0.0;
  const double q = num * rden;
  if (!(__builtin_fabs(q) < 0x1p40) || __builtin_fabs(q - __builtin_rint(q)) <= __builtin_fabs(q) * 0x1p-50)
    return __builtin_floor(num / den);
  return __builtin_floor(q);
}

// W - W_in of a fragment as f_meta's bits 4 - 5: 0 (both clamped), 1 (q an integer), 2; 3: W_in = -1, nothing fits
// inside.  W_in = floor(q) - 1 for a finite q = tol * obs / prec >= 1, clamped like W.
__device__ __forceinline__ uint32_t inner_code(double num, double prec, double rprec, int64_t w) {
  const double f = floor_quot(num, prec, rprec);
  if (!(f >= 1.0) || !(f <= 0x1.fffffffffffffp1023)) return 3u;
  const int64_t w_in = f > 0x1p61 ? kAlignClamp : clamp_f(f) - 1;
  return (uint32_t)(w - w_in);
}

// Record j of the chunk from fragment `at`: target, W, class / ends, cleared results; the chunk's flags and w_max.
template <bool kKeep>
__device__ __forceinline__ void load_record(AlignLds& s, uint32_t* f_keep, int j, int64_t at, const sst_align_args& a,
                                            double rprec, int L) {
  const int64_t t = clamp_f(rint_quot(a.frag_su[at], a.prec, rprec));
  int64_t w = clamp_f(ceil_quot(a.tol * a.frag_obs[at], a.prec, rprec));
  if (w < 0) w = -1;  // a negative W: nothing fits (|s - target| <= W has no solution)
  const uint32_t cls = (a.frag_code[at] >> 2) & 3u;
  const int mn = a.frag_min_end[at], mx = a.frag_max_end[at];
  const bool skipped = (cls == 1 || cls == 2) && (mn < 0 || mn >= L || mx < 0 || mx >= L);
  s.f_t[j] = t;
  s.f_w[j] = w;
  uint32_t meta = cls | (skipped ? 4u : 0u) | (skipped ? 0u : ((uint32_t)mn & 0xffu) << 8 | ((uint32_t)mx & 0xffu) << 16);
  if constexpr (kKeep) {
    meta |= inner_code(a.tol * a.frag_obs[at], a.prec, rprec, w) << 4;
    f_keep[j] = 0xffffffffu;
  }
  s.f_meta[j] = meta;
  s.f_nfit[j] = 0;
  s.f_first[j] = 0xffffffffu;
  s.f_open[j] = 0;
  if (!skipped) atomicOr(&s.flags, 16u << cls);
  if (w > 0) atomicMax(&s.w_max, (unsigned long long)w);
}

// A chunk begins: behind a barrier (the previous chunk's records are written out) its flags and w_max are cleared.
__device__ __forceinline__ void begin_chunk(AlignLds& s, int tid) {
  __syncthreads();
  if (tid == 0) {
    s.flags = 0;
    s.w_max = 0;
  }
}

// The chunk's records are loaded (a barrier behind them): flags bit 1 unless the
// targets ascend; returns the classes among its fragments (bit c: class c).
template <class V>
__device__ __forceinline__ uint32_t classes_present(AlignLds& s, int nf, int tid) {
  for (int j = tid; j + 1 < nf; j += V::kWG)
    if (s.f_t[j] > s.f_t[j + 1]) atomicOr(&s.flags, 2u);
  __syncthreads();
  return s.flags >> 4;
}

// One status for every fragment of a spectrum that is not modelled (SKIPPED) or has no alignment at all (INFEASIBLE).
template <class V>
__device__ __forceinline__ void write_spectrum(const sst_align_args& a, const sst_align_keep& kp, int64_t f0,
                                               int64_t nf_all, bool infeasible, int tid) {
  for (int64_t j = tid; j < nf_all; j += V::kWG) {
    a.status[f0 + j] = infeasible ? SST_ALIGN_INFEASIBLE : SST_ALIGN_SKIPPED;
    a.alignable[f0 + j] = infeasible ? 0 : 1;
    a.n_fit[f0 + j] = 0;
    a.first[f0 + j] = 0xFFFE;
    if constexpr (V::kKeep) {
      kp.keep[f0 + j] = 0;
      kp.keep_first[f0 + j] = 0xFFFE;
    }
  }
}

// The chunk's results to its fragments: record j is fragment first + j, in the
// split first + f_at[j] (a record SKIPPED there is not base-OPEN by the base
// kernel's outputs: it is left as it is).
template <class V>
__device__ __forceinline__ void write_chunk(const AlignLds& s, const uint32_t* f_keep, const int64_t* f_at,
                                            const sst_align_args& a, const sst_align_keep& kp, int64_t first, int nf,
                                            int tid) {
  for (int j = tid; j < nf; j += V::kWG) {
    const bool skipped = (s.f_meta[j] & 4u) != 0;
    if (V::kSplit && skipped) continue;
    const int64_t at = first + (V::kSplit ? f_at[j] : (int64_t)j);
    const uint32_t n = s.f_nfit[j];
    const uint8_t st = skipped      ? SST_ALIGN_SKIPPED
                       : n          ? SST_ALIGN_FIT
                       : s.f_open[j] ? SST_ALIGN_OPEN
                                     : SST_ALIGN_NONE;
    a.status[at] = st;
    a.alignable[at] = st != SST_ALIGN_NONE;
    a.n_fit[at] = n;
    a.first[at] = n ? (uint16_t)s.f_first[j] : (uint16_t)0xFFFE;
    if constexpr (V::kKeep) {  // (a skipped record matches nothing: its word stays cleared)
      const uint32_t kf = f_keep[j];
      kp.keep[at] = kf != 0xffffffffu;
      kp.keep_first[at] = kf != 0xffffffffu ? (uint16_t)kf : (uint16_t)0xFFFE;
    }
  }
}

struct Interval {
  int l, r;        // (0xFF, 0xFF): the empty interval
  int64_t lo, hi;  // LO, HI
  bool open;
  const uint32_t* list;
  int n;
};

// Fragment j of the chunk against interval iv: false unless iv is admissible
// for its class and its window meets [LO, HI]; else the window as offsets from
// LO (hi >= 0, lo <= HI - LO < 2^32).  mode 0: a forward sweep (internal,
// START, START_END), 1: the backward sweep (END), 2: the empty interval
// (internal; START_END where L == 0).
__device__ __forceinline__ bool window_of(const AlignLds& s, int j, const Interval& iv, int mode, int L, int64_t& lo,
                                          int64_t& hi) {
  const uint32_t meta = s.f_meta[j];
  if (meta & 4u) return false;
  const int cls = (int)(meta & 3u), mn = (int)((meta >> 8) & 0xffu), mx = (int)((meta >> 16) & 0xffu);
  bool ok;
  if (mode == 0)
    ok = cls == 0 || (cls == 1 && iv.l == 0 && iv.r >= (mn < mx ? mn : mx) && iv.r <= mx) ||
         (cls == 3 && iv.l == 0 && iv.r == L - 1);
  else if (mode == 1)
    ok = cls == 2 && iv.l >= (mn < mx ? mn : mx) && iv.l <= mn;
  else
    ok = cls == 0 || (cls == 3 && L == 0);
  if (!ok || s.f_w[j] < 0) return false;  // W < 0: an empty window
  const int64_t flo = s.f_t[j] - s.f_w[j], fhi = s.f_t[j] + s.f_w[j];
  if (fhi < iv.lo || flo > iv.hi) return false;
  lo = flo - iv.lo;
  hi = fhi - iv.lo;
  return true;
}

// The chunk's records [j0, j1) whose window can meet [LO, HI] (all of them where the targets do not ascend).
__device__ __forceinline__ void cut_chunk(const AlignLds& s, int nf, const Interval& iv, int& j0, int& j1) {
  const bool cut = !(s.flags & 2u);
  const int64_t wm = (int64_t)s.w_max;
  j0 = cut ? lower_i64(s.f_t, nf, iv.lo - wm) : 0;
  j1 = cut ? lower_i64(s.f_t, nf, iv.hi + wm + 1) : nf;
}

// Every fragment of the chunk the interval is admissible for: fit / open.  In
// keep mode, f_keep of a row-free spectrum (else nullptr): also "fits inside".
// The inner window lies d = W - W_in <= 2 inside the outer one at both ends and
// the list's entries are distinct integers, so the first entry >= lo + d is at
// most d entries behind the first >= lo: the second lower-bound search is a
// walk of at most two steps from where the first one ended.
template <bool kKeep>
__device__ __forceinline__ void match_fragments(AlignLds& s, uint32_t* f_keep, int nf, const Interval& iv, int mode,
                                                int L, int lane) {
  int j0, j1;
  cut_chunk(s, nf, iv, j0, j1);
  for (int j = j0 + lane; j < j1; j += 64) {
    int64_t lo, hi;
    if (!window_of(s, j, iv, mode, L, lo, hi)) continue;
    if (iv.open) {
      atomicOr(&s.f_open[j], 1u);
      continue;
    }
    const uint32_t a = lo > 0 ? (uint32_t)lo : 0u;
    const int at = lower_u32(iv.list, iv.n, a);
    if (at < iv.n && (int64_t)iv.list[at] <= hi) {
      atomicAdd(&s.f_nfit[j], 1u);
      atomicMin(&s.f_first[j], (uint32_t)(iv.l << 8 | iv.r));
      if constexpr (kKeep) {
        const int64_t d = (int64_t)((s.f_meta[j] >> 4) & 3u);
        if (f_keep && d != 3) {
          int in = at;
          while (in < iv.n && (int64_t)iv.list[in] < lo + d) ++in;
          if (in < iv.n && (int64_t)iv.list[in] <= hi - d) atomicMin(&f_keep[j], (uint32_t)(iv.l << 8 | iv.r));
        }
      }
    }
  }
}

// The fragments of the chunk the split-closed interval iv (LO, HI of both
// halves together) is admissible for, one at a time by the whole wave: lanes
// over the entries a of A that can take part, each searching B for the first
// entry >= lo' - a (under the cap: from there for one within E - e_a); any
// lane's hit is a fit.  A, B: offsets from LO_A, LO_B.
// In keep mode (under the cap), where the spectrum is row-free: the walk over
// B's entries inside the window goes on until one within budget also lies
// inside the inner window [lo + d, hi - d], and the fragment's entries of A
// are taken until a pair fits inside or they are exhausted.
template <bool kCaps, bool kKeep>
__device__ __forceinline__ void match_split(AlignLds& s, int nf, const Interval& iv, const Spectrum<kCaps>& sp,
                                            List<kCaps> A, int nA, List<kCaps> B, int nB, int mode, int lane) {
  int j0, j1;
  cut_chunk(s, nf, iv, j0, j1);
  const int64_t b_max = (int64_t)B.v[nB - 1];
  for (int j = j0; j < j1; ++j) {  // (wave-uniform)
    int64_t lo, hi;                // a + b in [lo, hi]
    if (!window_of(s, j, iv, mode, sp.L, lo, hi)) continue;
    const int i0 = lo - b_max > 0 ? lower_u32(A.v, nA, (uint32_t)(lo - b_max)) : 0;
    const int i1 = hi >= (int64_t)A.v[nA - 1] ? nA : upper_u32(A.v, nA, (uint32_t)hi);
    bool fit = false;
    [[maybe_unused]] bool inside = false, want = false;  // want: an inner fit is still looked for
    [[maybe_unused]] int64_t d = 0;
    if constexpr (kKeep) {
      d = (int64_t)((s.f_meta[j] >> 4) & 3u);
      want = sp.row_free && d != 3;
    }
    for (int c0 = i0; c0 < i1 && !(fit && !want); c0 += 64) {
      bool hit = false;
      [[maybe_unused]] bool hit_in = false;
      const int i = c0 + lane;
      if (i < i1) {
        const int64_t x = (int64_t)A.v[i], need = lo - x;  // need <= b_max by i0
        if constexpr (kCaps) {
          const uint32_t left = sp.E - A.e[i];  // (every listed excess is <= E)
          for (int at = need > 0 ? lower_u32(B.v, nB, (uint32_t)need) : 0; at < nB && (int64_t)B.v[at] <= hi - x; ++at)
            if (B.e[at] <= left) {
              hit = true;
              if constexpr (kKeep) {
                if (!want) break;
                const int64_t b = (int64_t)B.v[at];
                if (b >= need + d && b <= hi - x - d) {
                  hit_in = true;
                  break;
                }
              } else {
                break;
              }
            }
        } else {
          const int at = need > 0 ? lower_u32(B.v, nB, (uint32_t)need) : 0;
          hit = at < nB && (int64_t)B.v[at] <= hi - x;
        }
      }
      fit = fit || __ballot(hit) != 0;
      if constexpr (kKeep) {
        if (want && __ballot(hit_in) != 0) {
          inside = true;
          want = false;
        }
      }
    }
    if (fit && lane == 0) {
      atomicAdd(&s.f_nfit[j], 1u);
      atomicMin(&s.f_first[j], (uint32_t)(iv.l << 8 | iv.r));
    }
    if constexpr (kKeep)
      if (inside && lane == 0) atomicMin(&sp.f_keep[j], (uint32_t)(iv.l << 8 | iv.r));
  }
}

// dst = the distinct values of u[0, nu) and o[0, no) + d, ascending (u, o
// ascending and distinct; dst may be u; tmp holds nu + no entries).  Under the
// cap the copy o + d costs c more, equal values keep the smaller excess and
// values whose excess is above E are dropped.  Returns their number; only the
// first kAlignK are stored.
template <bool kCaps>
__device__ __forceinline__ int union_shifted(List<kCaps> u, int nu, List<kCaps> o, int no, uint32_t d, uint32_t c,
                                             uint32_t E, List<kCaps> tmp, List<kCaps> dst, int lane) {
  for (int i = lane; i < nu; i += 64) {
    const uint32_t x = u.v[i];
    const int at = i + (x >= d ? lower_u32(o.v, no, x - d) : 0);  // before an equal shifted entry
    tmp.v[at] = x;
    if constexpr (kCaps) tmp.e[at] = u.e[i];
  }
  for (int j = lane; j < no; j += 64) {
    const uint32_t y = o.v[j] + d;
    const int at = j + upper_u32(u.v, nu, y);
    tmp.v[at] = y;
    if constexpr (kCaps) tmp.e[at] = (uint8_t)(o.e[j] + c);  // <= 253 + 1
  }
  wave_sync();
  const int nt = nu + no;
  int base = 0;
  for (int c0 = 0; c0 < nt; c0 += 64) {
    const int k = c0 + lane;
    bool keep = false;
    uint32_t v = 0, e = 0;
    if (k < nt) {
      v = tmp.v[k];
      keep = k == 0 || tmp.v[k - 1] != v;
      if constexpr (kCaps) {
        e = tmp.e[k];
        if (k + 1 < nt && tmp.v[k + 1] == v) {
          const uint32_t e2 = tmp.e[k + 1];
          e = e2 < e ? e2 : e;
        }
        keep = keep && e <= E;
      }
    }
    const uint64_t m = __ballot(keep);
    const int at = base + (int)lanes_below(m);
    if (keep && at < kAlignK) {
      dst.v[at] = v;
      if constexpr (kCaps) dst.e[at] = (uint8_t)e;
    }
    base += __builtin_popcountll(m);
  }
  wave_sync();
  return base;
}

// cur (n entries, a closed list) extended by position p (several masses); the
// new count, above kAlignK if a union passes it (cur is then intact, the
// partial union is in `other`).  Swaps cur / other when the list moves.
template <bool kCaps>
__device__ __forceinline__ int extend_list(const AlignLds& s, const Spectrum<kCaps>& sp, List<kCaps>& cur,
                                           List<kCaps>& other, List<kCaps> tmp, int n, int p, uint32_t pmin, int lane) {
  uint64_t m0, m1;
  position_set(sp, p, m0, m1);
  bool forced = false, pays = false;
  uint32_t E = 0;
  if constexpr (kCaps) {
    forced = sp.p_flag[p] & 1u;
    pays = sp.p_flag[p] & 2u;
    E = sp.E;
  }
  List<kCaps> u = cur;  // the union so far: the copy of the smallest mass, where it is free
  int nu = n;
  if (pays) {
    u = other;
    nu = 0;
  }
  for (int h = 0; h < 2; ++h) {
    for (uint64_t m = h ? m1 : m0; m; m &= m - 1) {
      const int bit = __builtin_ctzll(m);
      const uint32_t d = s.w[64 * h + bit] - pmin;
      uint32_t c = 0;
      if constexpr (kCaps) c = forced ? 0u : (uint32_t)(((h ? sp.mod1 : sp.mod0) >> bit) & 1u);
      if ((d == 0 && !pays) || c > E) continue;  // (c > E: every entry of the copy is over budget)
      nu = union_shifted(u, nu, cur, n, d, c, E, tmp, other, lane);
      u = other;
      if (nu > kAlignK) return nu;
    }
  }
  if (u.v == other.v) {
    const List<kCaps> x = cur;
    cur = other;
    other = x;
  }
  return nu;
}

// The list {0} (the empty sum, excess 0), visible to the wave.
template <bool kCaps>
__device__ __forceinline__ void list_of_zero(List<kCaps> l, int lane) {
  if (lane == 0) {
    l.v[0] = 0;
    if constexpr (kCaps) l.e[0] = 0;
  }
  wave_sync();
}

// f_keep where the spectrum is row-free, else (and outside keep mode) nullptr: nothing is kept
template <class V>
__device__ __forceinline__ uint32_t* keep_words(const Spectrum<V::kCaps>& sp) {
  if constexpr (V::kKeep) return sp.row_free ? sp.f_keep : nullptr;
  return nullptr;
}

// One sweep of a wave: positions `from`, from + dir, ... to the skeleton's end.
template <class V>
__device__ __forceinline__ void sweep(AlignLds& s, const Spectrum<V::kCaps>& sp, uint8_t* mine, int nf, int from,
                                      int dir, int lane) {
  List<V::kCaps> cur = list_at<V>(mine, 0), other = list_at<V>(mine, 1);  // cur: S_E(l, r) - LO
  const List<V::kCaps> tmp = list_at<V>(mine, 2);
  list_of_zero(cur, lane);
  Interval iv{from, from, 0, 0, false, cur.v, 1};
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  for (int p = from; p >= 0 && p < sp.L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;  // LO never falls: no later interval of this sweep meets a window
    if (!iv.open && pmax != pmin) {
      const int n = extend_list(s, sp, cur, other, tmp, iv.n, p, pmin, lane);
      if (n > kAlignK) iv.open = true; else iv.n = n;
      iv.list = cur.v;
    }
    match_fragments<V::kKeep>(s, keep_words<V>(sp), nf, iv, dir > 0 ? 0 : 1, sp.L, lane);
  }
}

// One sweep of a wave over the open intervals only.  Phase A: the list of
// sweep() up to the last closed interval [from, m*] (nothing is matched: a
// base-OPEN fragment has no closed fit).  Phase B: a fresh list from m* + dir;
// while it is closed the interval is split-closed (match_split), afterwards
// undecided: only LO and HI move and a window that meets them is marked open.
template <class V>
__device__ __forceinline__ void sweep_split(AlignLds& s, const Spectrum<V::kCaps>& sp, uint8_t* mine, int nf, int from,
                                            int dir, int lane) {
  List<V::kCaps> la = list_at<V>(mine, 0), lb = list_at<V>(mine, 1), spare = list_at<V>(mine, 2);
  const List<V::kCaps> tmp = list_at<V>(mine, 3);
  const int L = sp.L;
  list_of_zero(la, lane);
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  int64_t lo = 0, hi = 0;
  int nA = 1, p = from;
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    if (prune && lo + pmin - wm > t_last) return;  // LO never falls
    if (pmax != pmin) {
      const int n = extend_list(s, sp, la, spare, tmp, nA, p, pmin, lane);
      if (n > kAlignK) break;  // [from, p] is open: A = S_E(from, p - dir)
      nA = n;
    }
    lo += pmin;
    hi += pmax;
  }
  if (p < 0 || p >= L || p == from) return;  // no open interval in this sweep
  list_of_zero(lb, lane);
  int nB = 1;
  Interval iv{from, from, lo, hi, false, lb.v, 1};
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;
    if (!iv.open && pmax != pmin) {
      const int n = extend_list(s, sp, lb, spare, tmp, nB, p, pmin, lane);
      if (n > kAlignK) iv.open = true; else nB = n;
    }
    if (iv.open)
      match_fragments<false>(s, nullptr, nf, iv, dir > 0 ? 0 : 1, L, lane);  // (an open interval keeps nothing)
    else
      match_split<V::kCaps, V::kKeep>(s, nf, iv, sp, la, nA, lb, nB, dir > 0 ? 0 : 1, lane);
  }
}

// The next base-OPEN fragments of a spectrum's status bytes from `next` on, in
// order, as records 0 .. of the chunk (f_at), until fewer than a block's worth
// of records are free; returns their number.
template <class V>
__device__ __forceinline__ int scan_open(SplitLds& sl, const uint8_t* status, int64_t nf_all, int64_t& next, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  int nf = 0;
  while (next < nf_all && kAlignF - nf >= V::kWG) {
    const int64_t j = next + tid;
    const bool open = j < nf_all && status[j] == SST_ALIGN_OPEN;
    const uint64_t m = __ballot(open);
    __syncthreads();  // wave_n of the previous block is read
    if (lane == 0) sl.wave_n[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    int before = nf, total = 0;
    for (int w = 0; w < V::kWaves; ++w) {
      const int n = (int)sl.wave_n[w];
      if (w < wave) before += n;
      total += n;
    }
    if (open) sl.f_at[before + (int)lanes_below(m)] = j;
    nf += total;
    next += V::kWG;
  }
  return nf;
}

template <class V>
struct Workgroup {  // the workgroup's dynamic LDS and a thread's place in it
  typename V::Records& rec;
  CapsLds* cl;  // (dereferenced under the cap only)
  KeepLds* kl;  // (in keep mode only)
  int tid, lane, wave;
  uint8_t* mine;  // the wave's lists
  __device__ __forceinline__ explicit Workgroup(uint8_t* lds)
      : rec(*reinterpret_cast<typename V::Records*>(lds + V::kRecordsAt)),
        cl(reinterpret_cast<CapsLds*>(lds + V::kCapsAt)),
        kl(reinterpret_cast<KeepLds*>(lds + V::kKeepAt)),
        tid((int)threadIdx.x), lane(tid & 63), wave(tid >> 6), mine(lds + wave * V::kWaveBytes) {}
};

// Keep mode, a modelled and feasible spectrum: is every row of alpha (row 0
// excluded) free?  One row per thread, n_r counted over the positions' sets;
// free iff row_cap >= n_r, or the row is modified and row_cap >= mod_cap (all
// modified rows together appear at most mod_cap times).  row_bad is cleared
// behind a barrier before; ends on a barrier.
template <class V>
__device__ __forceinline__ bool rows_free(KeepLds* kl, const Spectrum<true>& sp, const int32_t* row_cap, int n_rows,
                                          int mod_cap, int tid) {
  for (int r = 1 + tid; r < n_rows; r += V::kWG) {
    const uint64_t bit = 1ull << (r & 63);
    if (!((r < 64 ? sp.a0 : sp.a1) & bit)) continue;
    int n_r = 0;
    for (int p = 0; p < sp.L; ++p) {
      uint64_t m0, m1;
      position_set(sp, p, m0, m1);
      n_r += ((r < 64 ? m0 : m1) & bit) != 0;
    }
    const int cap = row_cap[(int64_t)sp.L * n_rows + r];
    const bool modified = ((r < 64 ? sp.mod0 : sp.mod1) & bit) != 0;
    if (!(cap >= n_r || (modified && cap >= mod_cap))) atomicOr(&kl->row_bad, 1u);
  }
  __syncthreads();
  return kl->row_bad == 0;
}

// k_align_windows, k_align_windows_caps, k_align_windows_keep (c is read under the cap only, kp in keep mode only)
template <bool kCaps, bool kKeep = false>
__device__ __forceinline__ void align_windows(const AlignKArgs& k, const sst_align_caps& c, const sst_align_keep& kp) {
  using V = Variant<false, kCaps, kKeep>;
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const Workgroup<V> wg(reinterpret_cast<uint8_t*>(align_lds));
  const sst_align_args& a = k.a;
  AlignLds& s = wg.rec;
  const int tid = wg.tid, lane = wg.lane;
  Spectrum<kCaps> sp;
  uint64_t rows0, rows1;
  load_table<V>(s, wg.cl, k, c, tid, rows0, rows1, sp);
  uint32_t* f_keep = nullptr;
  if constexpr (kKeep) sp.f_keep = f_keep = wg.kl->f_keep;

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) {
      if constexpr (kKeep)
        if (tid == 0) kp.spec_free[g] = 0;  // (nothing is computed for a spectrum without fragments)
      continue;
    }
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    sp.skel = a.skeleton + 2 * pos0;
    sp.a0 = a.alpha[2 * g] & rows0;
    sp.a1 = a.alpha[2 * g + 1] & rows1;
    sp.L = L;
    __syncthreads();  // the previous spectrum's LDS is no longer read
    if (tid == 0) {
      s.flags = 0;
      if constexpr (kCaps) wg.cl->n_forced = 0;
      if constexpr (kKeep) wg.kl->row_bad = 0;
    }
    __syncthreads();
    const bool modelled = L >= 0 && L <= kAlignMaxLen && n_pos == (int64_t)L;
    if (modelled)
      for (int p = tid; p < L; p += V::kWG) position_range(s, wg.cl, sp, p);
    __syncthreads();
    // an empty A_i, or F > mod_cap: among modelled spectra only (an unmodelled one is SKIPPED whatever its mod_cap)
    bool infeasible = modelled && (s.flags & 1u) != 0;
    if constexpr (kCaps) {
      const int cap = c.mod_cap[g], n_forced = (int)wg.cl->n_forced;
      infeasible = infeasible || (modelled && n_forced > cap);
      sp.E = budget(cap, n_forced);
    }
    if (!modelled || infeasible) {
      write_spectrum<V>(a, kp, f0, nf_all, infeasible, tid);
      if constexpr (kKeep)
        if (tid == 0) kp.spec_free[g] = 0;
      continue;
    }
    if constexpr (kKeep) {
      sp.row_free = rows_free<V>(wg.kl, sp, kp.row_cap, k.n_rows, c.mod_cap[g], tid);
      if (tid == 0) kp.spec_free[g] = sp.row_free;
    }

    for (int64_t c0 = 0; c0 < nf_all; c0 += kAlignF) {
      const int nf = (int)(nf_all - c0 < kAlignF ? nf_all - c0 : kAlignF);
      begin_chunk(s, tid);
      __syncthreads();
      for (int j = tid; j < nf; j += V::kWG) load_record<kKeep>(s, f_keep, j, f0 + c0 + j, a, k.rprec, L);
      __syncthreads();
      const uint32_t present = classes_present<V>(s, nf, tid);
      // sweeps: t < L forward from t; t == L backward from L - 1; t == L + 1 the empty interval
      for (int t = wg.wave; t < L + 2; t += V::kWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u)) sweep<V>(s, sp, wg.mine, nf, t, 1, lane);
        } else if (t == L) {
          if (present & 0x4u) sweep<V>(s, sp, wg.mine, nf, L - 1, -1, lane);
        } else if (present & (L == 0 ? 0x9u : 0x1u)) {
          const List<kCaps> zero = list_at<V>(wg.mine, 0);
          list_of_zero(zero, lane);
          const Interval iv{0xFF, 0xFF, 0, 0, false, zero.v, 1};
          match_fragments<kKeep>(s, keep_words<V>(sp), nf, iv, 2, L, lane);
        }
      }
      __syncthreads();
      write_chunk<V>(s, f_keep, nullptr, a, kp, f0 + c0, nf, tid);
    }
  }
}

// k_align_split, k_align_split_caps, k_align_split_keep: over the outputs of k_align_windows(_caps, _keep) (c is
// read under the cap only, kp in keep mode only: spec_free is the base kernel's, the row test is not run again)
template <bool kCaps, bool kKeep = false>
__device__ __forceinline__ void align_split(const AlignKArgs& k, const sst_align_caps& c, const sst_align_keep& kp) {
  using V = Variant<true, kCaps, kKeep>;
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const Workgroup<V> wg(reinterpret_cast<uint8_t*>(align_lds));
  const sst_align_args& a = k.a;
  SplitLds& sl = wg.rec;
  AlignLds& s = sl.s;
  const int tid = wg.tid, lane = wg.lane;
  Spectrum<kCaps> sp;
  uint64_t rows0, rows1;
  load_table<V>(s, wg.cl, k, c, tid, rows0, rows1, sp);
  uint32_t* f_keep = nullptr;
  if constexpr (kKeep) sp.f_keep = f_keep = wg.kl->f_keep;

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) continue;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    // (a base-OPEN fragment implies a modelled spectrum; anything else in the status bytes is not followed)
    if (!(L >= 1 && L <= kAlignMaxLen && n_pos == (int64_t)L)) continue;
    sp.skel = a.skeleton + 2 * pos0;
    sp.a0 = a.alpha[2 * g] & rows0;
    sp.a1 = a.alpha[2 * g + 1] & rows1;
    sp.L = L;
    int cap = 0;
    if constexpr (kCaps) cap = c.mod_cap[g];
    if constexpr (kKeep) sp.row_free = kp.spec_free[g] != 0;
    bool have_pos = false;

    for (int64_t next = 0; next < nf_all;) {
      begin_chunk(s, tid);
      if constexpr (kCaps)
        if (tid == 0 && !have_pos) wg.cl->n_forced = 0;
      const int nf = scan_open<V>(sl, a.status + f0, nf_all, next, tid);
      if (nf == 0) break;  // (only when the fragments are exhausted)
      __syncthreads();
      const bool first_chunk = !have_pos;
      if (first_chunk) {  // the spectrum has a base-OPEN fragment: its positions' masses (flags and F)
        have_pos = true;
        for (int p = tid; p < L; p += V::kWG) position_range(s, wg.cl, sp, p);
      }
      for (int j = tid; j < nf; j += V::kWG) load_record<kKeep>(s, f_keep, j, f0 + sl.f_at[j], a, k.rprec, L);
      __syncthreads();
      // an empty A_i or F > mod_cap (never with a base-OPEN fragment): the spectrum is left as it is
      if (s.flags & 1u) break;
      if constexpr (kCaps) {
        const int n_forced = (int)wg.cl->n_forced;
        if (n_forced > cap) break;
        if (first_chunk) sp.E = budget(cap, n_forced);
      }
      const uint32_t present = classes_present<V>(s, nf, tid);
      // sweeps: t < L forward from t; t == L backward from L - 1 (the empty interval is closed)
      for (int t = wg.wave; t < L + 1; t += V::kWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u)) sweep_split<V>(s, sp, wg.mine, nf, t, 1, lane);
        } else if (present & 0x4u) {
          sweep_split<V>(s, sp, wg.mine, nf, L - 1, -1, lane);
        }
      }
      __syncthreads();
      write_chunk<V>(s, f_keep, sl.f_at, a, kp, f0, nf, tid);
    }
  }
}

using Windows = Variant<false, false>;
using Split = Variant<true, false>;
using WindowsCaps = Variant<false, true>;
using SplitCaps = Variant<true, true>;

using WindowsKeep = Variant<false, true, true>;
using SplitKeep = Variant<true, true, true>;

__global__ __launch_bounds__(Windows::kWG) void k_align_windows(AlignKArgs k) {
  align_windows<false>(k, sst_align_caps{}, sst_align_keep{});
}
__global__ __launch_bounds__(Split::kWG) void k_align_split(AlignKArgs k) {
  align_split<false>(k, sst_align_caps{}, sst_align_keep{});
}
__global__ __launch_bounds__(WindowsCaps::kWG) void k_align_windows_caps(AlignCapsKArgs kc) {
  align_windows<true>(kc.k, kc.c, sst_align_keep{});
}
__global__ __launch_bounds__(SplitCaps::kWG) void k_align_split_caps(AlignCapsKArgs kc) {
  align_split<true>(kc.k, kc.c, sst_align_keep{});
}
__global__ __launch_bounds__(WindowsKeep::kWG) void k_align_windows_keep(AlignKeepKArgs kk) {
  align_windows<true, true>(kk.kc.k, kk.kc.c, kk.kp);
}
__global__ __launch_bounds__(SplitKeep::kWG) void k_align_split_keep(AlignKeepKArgs kk) {
  align_split<true, true>(kk.kc.k, kk.kc.c, kk.kp);
}

template <class V, class KArgs>
hipError_t launch(void (*kernel)(KArgs), const KArgs& k, int64_t n_spec, int n_wg, hipStream_t st) {
  // (per device: a process may hold one context per GPU)
  if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)V::kLdsBytes))
    return e;
  const unsigned grid = (unsigned)(n_spec < (int64_t)n_wg ? n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(V::kWG), V::kLdsBytes, st, k);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_align(bool split, const sst_align_args& a, const sst_align_caps* caps, const sst_align_keep* keep,
                        const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  const AlignKArgs k{a, w, n_rows, 1.0 / a.prec};
  if (!caps)
    return split ? launch<Split>(k_align_split, k, a.n_spec, n_wg, st)
                 : launch<Windows>(k_align_windows, k, a.n_spec, n_wg, st);
  const AlignCapsKArgs kc{k, *caps};
  if (keep) {
    const AlignKeepKArgs kk{kc, *keep};
    return split ? launch<SplitKeep>(k_align_split_keep, kk, a.n_spec, n_wg, st)
                 : launch<WindowsKeep>(k_align_windows_keep, kk, a.n_spec, n_wg, st);
  }
  return split ? launch<SplitCaps>(k_align_split_caps, kc, a.n_spec, n_wg, st)
               : launch<WindowsCaps>(k_align_windows_caps, kc, a.n_spec, n_wg, st);
}

}  // namespace sst
