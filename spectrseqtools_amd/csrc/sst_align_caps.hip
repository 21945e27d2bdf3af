// sst_align_caps.hip -- the alignment certificate under the program's universal
// modification cap (gfx950): k_align_windows_caps, k_align_split_caps
// (include/sst.h: sst_align_windows_caps_device, sst_align_split_caps_device).
// A translation unit of its own, so that sst_align.hip's two kernels compile to
// the code they had before; what both share is in sst_align_common.h.
#include "sst_align_common.h"

namespace sst {

namespace {

// ---------------------------------------------------------------------------
// k_align_windows_caps and k_align_split_caps are sst_align.hip's two kernels
// with one u8 beside every u32 list entry: the sum's smallest excess (modified
// rows chosen beyond the interval's forced positions).
//
// Per spectrum the position pass also derives, per position, "forced" (every
// row of A_i is modified) and "the smallest mass pays" (not forced, and no
// unmodified row has the position's smallest mass), and counts the forced
// positions F; F > mod_cap is INFEASIBLE, else E = mod_cap - F (<= 253).
//
// Extending a list by a position unions one shifted copy per row: offset + d,
// excess + c with c = row_mod - forced.  The copy of the smallest mass stays
// the list itself (only LO moves) unless that mass pays: then the union starts
// empty and the unshifted copy is merged like any other, with c = 1.  The rank
// merge carries the excess bytes; the ballot compaction keeps the smaller
// excess of two equal neighbours and drops what is above E, so what is stored
// and counted is S_E only.  (A copy with c > E is empty and is skipped.)
// A position of one mass costs nothing: forced, or an unmodified row has it.
//
// LDS: the bytes raise a wave's lists to 20 KiB (base) and 25 KiB (split).  At
// the 4 and 3 waves of the uncapped kernels that is 80 + 15 and 75 + 18 KiB: past
// 80 KiB, one workgroup per CU.  3 and 2 waves keep two: 60 + 15.2 = 75.2 KiB
// and 50 + 18.2 = 68.2 KiB.
// ---------------------------------------------------------------------------
constexpr int kCapsWaves = 3;
constexpr int kCapsWG = 64 * kCapsWaves;
constexpr int kCapsWaveBytes = kAlignWaveWords * 5;  // u32 lists + one u8 per entry: 20 KiB
constexpr int kCapsSplitWaves = 2;
constexpr int kCapsSplitWG = 64 * kCapsSplitWaves;
constexpr int kCapsSplitWaveBytes = kSplitWaveWords * 5;  // 25 KiB

struct CapsLds {  // behind AlignLds / SplitLds
  unsigned long long mod[2];  // the table's modified rows as two masks
  uint32_t n_forced;          // F
  uint8_t p_flag[256];        // per position: 1 forced, 2 the smallest mass pays
};

constexpr size_t kCapsLdsBytes = (size_t)kCapsWaves * kCapsWaveBytes + sizeof(AlignLds) + sizeof(CapsLds);
constexpr size_t kCapsSplitLdsBytes = (size_t)kCapsSplitWaves * kCapsSplitWaveBytes + sizeof(SplitLds) + sizeof(CapsLds);
static_assert(2 * kCapsLdsBytes <= kCuLdsBytes, "two workgroups per CU");
static_assert(2 * kCapsSplitLdsBytes <= kCuLdsBytes, "two workgroups per CU");
static_assert((size_t)(kCapsWaves + 1) * kCapsWaveBytes + sizeof(AlignLds) > kCuLdsBytes / 2 &&
                  (size_t)(kCapsSplitWaves + 1) * kCapsSplitWaveBytes + sizeof(SplitLds) > kCuLdsBytes / 2,
              "one more wave would cost the second workgroup");
static_assert(kCapsWaveBytes % 8 == 0 && kCapsSplitWaveBytes % 8 == 0 && sizeof(AlignLds) % 8 == 0 &&
                  sizeof(SplitLds) % 8 == 0, "the records behind the lists stay aligned");
static_assert(kAlignF >= kCapsSplitWG && kCapsSplitWaves <= kSplitWaves, "SplitLds serves the narrower workgroup");
static_assert(kAlignMaxLen + 1 <= 255, "an excess and one more fit a byte");

struct CapList {
  uint32_t* v;  // offsets from LO, ascending and distinct
  uint8_t* e;   // the smallest excess that reaches each
};

struct AlignCapsKArgs {
  AlignKArgs k;
  sst_align_caps c;
};

// The modified rows of the table as two masks: built once per workgroup in LDS,
// one row per thread (row 0 is in no A_i).  Ends on a barrier.
__device__ __forceinline__ void mod_masks(CapsLds& cl, const uint8_t* row_mod, int n_rows, int tid, int n_threads,
                                          uint64_t& mod0, uint64_t& mod1) {
  if (tid < 2) cl.mod[tid] = 0;
  __syncthreads();
  for (int r = 1 + tid; r < n_rows && r < 128; r += n_threads)
    if (row_mod[r]) atomicOr(&cl.mod[r >> 6], 1ull << (r & 63));
  __syncthreads();
  mod0 = cl.mod[0];
  mod1 = cl.mod[1];
}

// position_range, and the position's two flags and its share of F.
__device__ __forceinline__ void position_caps(AlignLds& s, CapsLds& cl, const uint64_t* skel, int64_t pos0, int p,
                                              uint64_t a0, uint64_t a1, uint64_t mod0, uint64_t mod1) {
  position_range(s, skel, pos0, p, a0, a1);
  uint64_t m0, m1;
  position_set(skel, pos0 + p, a0, a1, m0, m1);
  const uint64_t u0 = m0 & ~mod0, u1 = m1 & ~mod1;  // the unmodified rows of A_i
  const bool forced = !(u0 | u1);
  const uint32_t lo = s.p_min[p];
  bool pays = !forced;
  for (uint64_t m = u0; m; m &= m - 1) pays = pays && s.w[__builtin_ctzll(m)] != lo;
  for (uint64_t m = u1; m; m &= m - 1) pays = pays && s.w[64 + __builtin_ctzll(m)] != lo;
  cl.p_flag[p] = (uint8_t)((forced ? 1u : 0u) | (pays ? 2u : 0u));
  if (forced) atomicAdd(&cl.n_forced, 1u);
}

// union_shifted with the excess: the copy o + d costs c more.  Equal values
// keep the smaller excess; values whose excess is above E are dropped.
__device__ __forceinline__ int union_caps(CapList u, int nu, CapList o, int no, uint32_t d, uint32_t c, uint32_t E,
                                          CapList tmp, CapList dst, int lane) {
  for (int i = lane; i < nu; i += 64) {
    const uint32_t x = u.v[i];
    const int at = i + (x >= d ? lower_u32(o.v, no, x - d) : 0);  // before an equal shifted entry
    tmp.v[at] = x;
    tmp.e[at] = u.e[i];
  }
  for (int j = lane; j < no; j += 64) {
    const uint32_t y = o.v[j] + d;
    const int at = j + upper_u32(u.v, nu, y);
    tmp.v[at] = y;
    tmp.e[at] = (uint8_t)(o.e[j] + c);  // <= 253 + 1
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
      e = tmp.e[k];
      if (k + 1 < nt && tmp.v[k + 1] == v) {
        const uint32_t e2 = tmp.e[k + 1];
        e = e2 < e ? e2 : e;
      }
      keep = (k == 0 || tmp.v[k - 1] != v) && e <= E;
    }
    const uint64_t m = __ballot(keep);
    const int at = base + (int)lanes_below(m);
    if (keep && at < kAlignK) {
      dst.v[at] = v;
      dst.e[at] = (uint8_t)e;
    }
    base += __builtin_popcountll(m);
  }
  wave_sync();
  return base;
}

// cur (n entries, closed) extended by the position at `at` under the cap; the
// new count, above kAlignK if a union passes it (cur is then intact).  Swaps
// cur / other when the list moves.
__device__ __forceinline__ int extend_caps(AlignLds& s, CapList& cur, CapList& other, CapList tmp, int n,
                                           const uint64_t* skel, int64_t at, uint64_t a0, uint64_t a1, uint64_t mod0,
                                           uint64_t mod1, uint32_t pmin, uint32_t flag, uint32_t E, int lane) {
  uint64_t m0, m1;
  position_set(skel, at, a0, a1, m0, m1);
  const bool forced = flag & 1u, pays = flag & 2u;
  CapList u = cur;  // the union so far: the copy of the smallest mass, where it is free
  int nu = n;
  if (pays) {
    u = other;
    nu = 0;
  }
  for (int h = 0; h < 2; ++h) {
    const uint64_t mod = h ? mod1 : mod0;
    for (uint64_t m = h ? m1 : m0; m; m &= m - 1) {
      const int bit = __builtin_ctzll(m);
      const uint32_t d = s.w[64 * h + bit] - pmin;
      const uint32_t c = forced ? 0u : (uint32_t)((mod >> bit) & 1u);
      if ((d == 0 && !pays) || c > E) continue;  // (c > E: every entry of the copy is over budget)
      nu = union_caps(u, nu, cur, n, d, c, E, tmp, other, lane);
      u = other;
      if (nu > kAlignK) return nu;
    }
  }
  if (u.v == other.v) {
    const CapList x = cur;
    cur = other;
    other = x;
  }
  return nu;
}

// sweep() under the cap.
__device__ __forceinline__ void sweep_caps(AlignLds& s, const CapsLds& cl, uint8_t* mine, const sst_align_args& a,
                                           int64_t pos0, uint64_t a0, uint64_t a1, uint64_t mod0, uint64_t mod1,
                                           uint32_t E, int L, int nf, int from, int dir, int lane) {
  uint32_t* words = reinterpret_cast<uint32_t*>(mine);
  uint8_t* bytes = mine + 4 * kAlignWaveWords;
  CapList cur{words, bytes}, other{words + kAlignK, bytes + kAlignK};
  const CapList tmp{words + 2 * kAlignK, bytes + 2 * kAlignK};
  if (lane == 0) {
    cur.v[0] = 0;
    cur.e[0] = 0;
  }
  wave_sync();
  Interval iv{from, from, 0, 0, false, cur.v, 1};
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  for (int p = from; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;  // LO never falls
    if (!iv.open && pmax != pmin) {
      const int n = extend_caps(s, cur, other, tmp, iv.n, a.skeleton, pos0 + p, a0, a1, mod0, mod1, pmin, cl.p_flag[p],
                                E, lane);
      if (n > kAlignK) iv.open = true; else iv.n = n;
      iv.list = cur.v;
    }
    match_fragments(s, nf, iv, dir > 0 ? 0 : 1, L, lane);
  }
}

__global__ __launch_bounds__(kCapsWG) void k_align_windows_caps(AlignCapsKArgs kc) {
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const AlignKArgs& k = kc.k;
  const sst_align_args& a = k.a;
  uint8_t* lds = reinterpret_cast<uint8_t*>(align_lds);
  AlignLds& s = *reinterpret_cast<AlignLds*>(lds + kCapsWaves * kCapsWaveBytes);
  CapsLds& cl = *reinterpret_cast<CapsLds*>(lds + kCapsWaves * kCapsWaveBytes + sizeof(AlignLds));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t* mine = lds + wave * kCapsWaveBytes;

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kCapsWG) s.w[r] = r < k.n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;  // rows 1 .. n_rows - 1
  if (k.n_rows < 64) {
    rows0 &= (1ull << k.n_rows) - 1;
    rows1 = 0;
  } else if (k.n_rows < 128) {
    rows1 = (1ull << (k.n_rows - 64)) - 1;
  }
  uint64_t mod0, mod1;
  mod_masks(cl, kc.c.row_mod, k.n_rows, tid, kCapsWG, mod0, mod1);

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) continue;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    const int cap = kc.c.mod_cap[g];
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    __syncthreads();  // the previous spectrum's LDS is no longer read
    if (tid == 0) {
      s.flags = 0;
      cl.n_forced = 0;
    }
    __syncthreads();
    const bool modelled = L >= 0 && L <= kAlignMaxLen && n_pos == (int64_t)L;
    if (modelled)
      for (int p = tid; p < L; p += kCapsWG) position_caps(s, cl, a.skeleton, pos0, p, a0, a1, mod0, mod1);
    __syncthreads();
    const int n_forced = (int)cl.n_forced;
    // an empty A_i, or F > mod_cap: among modelled spectra only (an unmodelled one is SKIPPED whatever its mod_cap)
    const bool infeasible = modelled && ((s.flags & 1u) != 0 || n_forced > cap);
    if (!modelled || infeasible) {  // one status for every fragment of the spectrum
      for (int64_t j = tid; j < nf_all; j += kCapsWG) {
        a.status[f0 + j] = infeasible ? SST_ALIGN_INFEASIBLE : SST_ALIGN_SKIPPED;
        a.alignable[f0 + j] = infeasible ? 0 : 1;
        a.n_fit[f0 + j] = 0;
        a.first[f0 + j] = 0xFFFE;
      }
      continue;
    }
    const uint32_t E = (uint32_t)(cap - n_forced < kAlignMaxLen ? cap - n_forced : kAlignMaxLen);

    for (int64_t c0 = 0; c0 < nf_all; c0 += kAlignF) {
      const int nf = (int)(nf_all - c0 < kAlignF ? nf_all - c0 : kAlignF);
      __syncthreads();  // the previous chunk's records are written out
      if (tid == 0) {
        s.flags = 0;
        s.w_max = 0;
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kCapsWG) load_record(s, j, f0 + c0 + j, a, k.rprec, L);
      __syncthreads();
      for (int j = tid; j + 1 < nf; j += kCapsWG)
        if (s.f_t[j] > s.f_t[j + 1]) atomicOr(&s.flags, 2u);
      __syncthreads();
      const uint32_t present = s.flags >> 4;  // bit c: class c among the chunk's fragments
      // sweeps: t < L forward from t; t == L backward from L - 1; t == L + 1 the empty interval
      for (int t = wave; t < L + 2; t += kCapsWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u))
            sweep_caps(s, cl, mine, a, pos0, a0, a1, mod0, mod1, E, L, nf, t, 1, lane);
        } else if (t == L) {
          if (present & 0x4u) sweep_caps(s, cl, mine, a, pos0, a0, a1, mod0, mod1, E, L, nf, L - 1, -1, lane);
        } else if (present & (L == 0 ? 0x9u : 0x1u)) {
          uint32_t* zero = reinterpret_cast<uint32_t*>(mine);
          if (lane == 0) zero[0] = 0;
          wave_sync();
          const Interval iv{0xFF, 0xFF, 0, 0, false, zero, 1};  // sum 0, excess 0
          match_fragments(s, nf, iv, 2, L, lane);
        }
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kCapsWG) {
        const int64_t at = f0 + c0 + j;
        const uint32_t n = s.f_nfit[j];
        const uint8_t st = (s.f_meta[j] & 4u) ? SST_ALIGN_SKIPPED
                           : n            ? SST_ALIGN_FIT
                           : s.f_open[j]  ? SST_ALIGN_OPEN
                                          : SST_ALIGN_NONE;
        a.status[at] = st;
        a.alignable[at] = st != SST_ALIGN_NONE;
        a.n_fit[at] = n;
        a.first[at] = n ? (uint16_t)s.f_first[j] : (uint16_t)0xFFFE;
      }
    }
  }
}

// match_split under the cap: a pair fits only if its two excesses together
// stay within E, so a lane walks B's entries inside its window, from the first
// one >= lo' - a, until one is within E - e_a.
__device__ __forceinline__ void match_split_caps(AlignLds& s, int nf, const Interval& iv, CapList A, int nA, CapList B,
                                                 int nB, uint32_t E, int mode, int L, int lane) {
  const bool cut = !(s.flags & 2u);
  const int64_t wm = (int64_t)s.w_max;
  const int j0 = cut ? lower_i64(s.f_t, nf, iv.lo - wm) : 0;
  const int j1 = cut ? lower_i64(s.f_t, nf, iv.hi + wm + 1) : nf;
  const int64_t b_max = (int64_t)B.v[nB - 1];
  for (int j = j0; j < j1; ++j) {  // (wave-uniform)
    const uint32_t meta = s.f_meta[j];
    if (meta & 4u) continue;
    const int cls = (int)(meta & 3u), mn = (int)((meta >> 8) & 0xffu), mx = (int)((meta >> 16) & 0xffu);
    bool ok;
    if (mode == 0)
      ok = cls == 0 || (cls == 1 && iv.l == 0 && iv.r >= (mn < mx ? mn : mx) && iv.r <= mx) ||
           (cls == 3 && iv.l == 0 && iv.r == L - 1);
    else
      ok = cls == 2 && iv.l >= (mn < mx ? mn : mx) && iv.l <= mn;
    if (!ok || s.f_w[j] < 0) continue;
    const int64_t flo = s.f_t[j] - s.f_w[j], fhi = s.f_t[j] + s.f_w[j];
    if (fhi < iv.lo || flo > iv.hi) continue;
    const int64_t lo = flo - iv.lo, hi = fhi - iv.lo;  // a + b in [lo, hi]; hi >= 0, lo <= HI - LO < 2^32
    const int i0 = lo - b_max > 0 ? lower_u32(A.v, nA, (uint32_t)(lo - b_max)) : 0;
    const int i1 = hi >= (int64_t)A.v[nA - 1] ? nA : upper_u32(A.v, nA, (uint32_t)hi);
    bool fit = false;
    for (int c0 = i0; c0 < i1 && !fit; c0 += 64) {
      bool hit = false;
      const int i = c0 + lane;
      if (i < i1) {
        const int64_t x = (int64_t)A.v[i], need = lo - x;  // need <= b_max by i0
        const uint32_t left = E - A.e[i];                  // (every listed excess is <= E)
        for (int at = need > 0 ? lower_u32(B.v, nB, (uint32_t)need) : 0; at < nB && (int64_t)B.v[at] <= hi - x; ++at)
          if (B.e[at] <= left) {
            hit = true;
            break;
          }
      }
      fit = __ballot(hit) != 0;
    }
    if (fit && lane == 0) {
      atomicAdd(&s.f_nfit[j], 1u);
      atomicMin(&s.f_first[j], (uint32_t)(iv.l << 8 | iv.r));
    }
  }
}

// sweep_split() under the cap: A = S_E(from, m*), m* the last interval whose
// capped list is closed; B = S_E(m* + dir, p), its excess against its own
// forced positions.
__device__ __forceinline__ void sweep_split_caps(AlignLds& s, const CapsLds& cl, uint8_t* mine, const sst_align_args& a,
                                                 int64_t pos0, uint64_t a0, uint64_t a1, uint64_t mod0, uint64_t mod1,
                                                 uint32_t E, int L, int nf, int from, int dir, int lane) {
  uint32_t* words = reinterpret_cast<uint32_t*>(mine);
  uint8_t* bytes = mine + 4 * kSplitWaveWords;
  CapList la{words, bytes}, lb{words + kAlignK, bytes + kAlignK}, spare{words + 2 * kAlignK, bytes + 2 * kAlignK};
  const CapList tmp{words + 3 * kAlignK, bytes + 3 * kAlignK};
  if (lane == 0) {
    la.v[0] = 0;
    la.e[0] = 0;
  }
  wave_sync();
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  int64_t lo = 0, hi = 0;
  int nA = 1, p = from;
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    if (prune && lo + pmin - wm > t_last) return;  // LO never falls
    if (pmax != pmin) {
      const int n = extend_caps(s, la, spare, tmp, nA, a.skeleton, pos0 + p, a0, a1, mod0, mod1, pmin, cl.p_flag[p], E,
                                lane);
      if (n > kAlignK) break;  // [from, p] is open: A = S_E(from, p - dir)
      nA = n;
    }
    lo += pmin;
    hi += pmax;
  }
  if (p < 0 || p >= L || p == from) return;  // no open interval in this sweep
  if (lane == 0) {
    lb.v[0] = 0;
    lb.e[0] = 0;
  }
  wave_sync();
  int nB = 1;
  Interval iv{from, from, lo, hi, false, lb.v, 1};
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;
    if (!iv.open && pmax != pmin) {
      const int n = extend_caps(s, lb, spare, tmp, nB, a.skeleton, pos0 + p, a0, a1, mod0, mod1, pmin, cl.p_flag[p], E,
                                lane);
      if (n > kAlignK) iv.open = true; else nB = n;
    }
    if (iv.open)
      match_fragments(s, nf, iv, dir > 0 ? 0 : 1, L, lane);
    else
      match_split_caps(s, nf, iv, la, nA, lb, nB, E, dir > 0 ? 0 : 1, L, lane);
  }
}

__global__ __launch_bounds__(kCapsSplitWG) void k_align_split_caps(AlignCapsKArgs kc) {
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const AlignKArgs& k = kc.k;
  const sst_align_args& a = k.a;
  uint8_t* lds = reinterpret_cast<uint8_t*>(align_lds);
  SplitLds& sl = *reinterpret_cast<SplitLds*>(lds + kCapsSplitWaves * kCapsSplitWaveBytes);
  CapsLds& cl = *reinterpret_cast<CapsLds*>(lds + kCapsSplitWaves * kCapsSplitWaveBytes + sizeof(SplitLds));
  AlignLds& s = sl.s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint8_t* mine = lds + wave * kCapsSplitWaveBytes;

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kCapsSplitWG) s.w[r] = r < k.n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;  // rows 1 .. n_rows - 1
  if (k.n_rows < 64) {
    rows0 &= (1ull << k.n_rows) - 1;
    rows1 = 0;
  } else if (k.n_rows < 128) {
    rows1 = (1ull << (k.n_rows - 64)) - 1;
  }
  uint64_t mod0, mod1;
  mod_masks(cl, kc.c.row_mod, k.n_rows, tid, kCapsSplitWG, mod0, mod1);

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) continue;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    // (a base-OPEN fragment implies a modelled spectrum; anything else in the status bytes is not followed)
    if (!(L >= 1 && L <= kAlignMaxLen && n_pos == (int64_t)L)) continue;
    const int cap = kc.c.mod_cap[g];
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    bool have_pos = false;
    uint32_t E = 0;

    for (int64_t next = 0; next < nf_all;) {
      __syncthreads();  // the previous chunk's records are written out
      if (tid == 0) {
        s.flags = 0;
        s.w_max = 0;
        if (!have_pos) cl.n_forced = 0;
      }
      int nf = 0;
      // the next base-OPEN fragments, in order, until fewer than a block's worth of records are free
      while (next < nf_all && kAlignF - nf >= kCapsSplitWG) {
        const int64_t j = next + tid;
        const bool open = j < nf_all && a.status[f0 + j] == SST_ALIGN_OPEN;
        const uint64_t m = __ballot(open);
        __syncthreads();  // wave_n of the previous block is read
        if (lane == 0) sl.wave_n[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        int before = nf, total = 0;
        for (int w = 0; w < kCapsSplitWaves; ++w) {
          const int n = (int)sl.wave_n[w];
          if (w < wave) before += n;
          total += n;
        }
        if (open) sl.f_at[before + (int)lanes_below(m)] = j;
        nf += total;
        next += kCapsSplitWG;
      }
      if (nf == 0) break;  // (only when the fragments are exhausted)
      __syncthreads();
      const bool first_chunk = !have_pos;
      if (first_chunk) {  // the spectrum has a base-OPEN fragment: its positions' masses, flags and F
        have_pos = true;
        for (int p = tid; p < L; p += kCapsSplitWG) position_caps(s, cl, a.skeleton, pos0, p, a0, a1, mod0, mod1);
      }
      for (int j = tid; j < nf; j += kCapsSplitWG) load_record(s, j, f0 + sl.f_at[j], a, k.rprec, L);
      __syncthreads();
      // an empty A_i or F > mod_cap (never with a base-OPEN fragment): the spectrum is left as it is
      if ((s.flags & 1u) || (int)cl.n_forced > cap) break;
      if (first_chunk) E = (uint32_t)(cap - (int)cl.n_forced < kAlignMaxLen ? cap - (int)cl.n_forced : kAlignMaxLen);
      for (int j = tid; j + 1 < nf; j += kCapsSplitWG)
        if (s.f_t[j] > s.f_t[j + 1]) atomicOr(&s.flags, 2u);
      __syncthreads();
      const uint32_t present = s.flags >> 4;
      // sweeps: t < L forward from t; t == L backward from L - 1 (the empty interval is closed)
      for (int t = wave; t < L + 1; t += kCapsSplitWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u))
            sweep_split_caps(s, cl, mine, a, pos0, a0, a1, mod0, mod1, E, L, nf, t, 1, lane);
        } else if (present & 0x4u) {
          sweep_split_caps(s, cl, mine, a, pos0, a0, a1, mod0, mod1, E, L, nf, L - 1, -1, lane);
        }
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kCapsSplitWG) {
        if (s.f_meta[j] & 4u) continue;
        const int64_t at = f0 + sl.f_at[j];
        const uint32_t n = s.f_nfit[j];
        const uint8_t st = n ? SST_ALIGN_FIT : s.f_open[j] ? SST_ALIGN_OPEN : SST_ALIGN_NONE;
        a.status[at] = st;
        a.alignable[at] = st != SST_ALIGN_NONE;
        a.n_fit[at] = n;
        a.first[at] = n ? (uint16_t)s.f_first[j] : (uint16_t)0xFFFE;
      }
    }
  }
}

}  // namespace

hipError_t launch_align_windows_caps(const sst_align_args& a, const sst_align_caps& caps, const int* w, int n_rows,
                                     int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute((const void*)k_align_windows_caps, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kCapsLdsBytes))
    return e;
  AlignCapsKArgs k{{a, w, n_rows, 1.0 / a.prec}, caps};
  const unsigned grid = (unsigned)(a.n_spec < (int64_t)n_wg ? a.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_align_windows_caps, dim3(grid), dim3(kCapsWG), kCapsLdsBytes, st, k);
  return hipGetLastError();
}

hipError_t launch_align_split_caps(const sst_align_args& a, const sst_align_caps& caps, const int* w, int n_rows,
                                   int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute((const void*)k_align_split_caps, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kCapsSplitLdsBytes))
    return e;
  AlignCapsKArgs k{{a, w, n_rows, 1.0 / a.prec}, caps};
  const unsigned grid = (unsigned)(a.n_spec < (int64_t)n_wg ? a.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_align_split_caps, dim3(grid), dim3(kCapsSplitWG), kCapsSplitLdsBytes, st, k);
  return hipGetLastError();
}

}  // namespace sst
