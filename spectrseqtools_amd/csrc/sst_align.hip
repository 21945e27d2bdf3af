// sst_align.hip -- the alignment certificate (gfx950): which surviving
// fragments of a spectrum no window of its skeleton can explain, the question
// filter_with_lp (prediction.py:229-259) asks one LinearProgramInstance per
// fragment (linear_program.py).  The definition is in include/sst.h
// (sst_align_windows_device).
//
//   k_align_windows  one spectrum per workgroup, persistent grid over spectra.
//
// Per position the workgroup first derives A_i's smallest and largest row
// mass (LDS); an empty A_i ends the spectrum (INFEASIBLE).
// The fragments are taken in chunks of kAlignF records held in LDS (target,
// W, class / ends, and the three result words n_fit, first, open), so a
// spectrum of any fragment count runs, one sweep set per chunk.
//
// Waves take sweeps round robin: "forward from l" for every left end l
// (interior left ends only when the chunk has internal fragments), one
// "backward from L - 1" for the END class (its intervals all end at L - 1), and
// the empty interval.  A sweep keeps S(l, r) as a sorted list of distinct u32
// offsets from LO(l, r) in the wave's LDS slice; LO and HI are 64-bit scalars.
// Extending by a position adds its minimum to LO; a position of one mass
// changes nothing else.  A position of several masses unions one shifted copy
// of the list per further mass, one at a time: a stable rank merge into the
// wave's 2 K temp (each lane places its elements by binary search in the other
// list), then a ballot / mbcnt compaction that drops equal neighbours.  The
// first union above K entries makes the sweep open for good (|S| never
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
// LDS per workgroup: 4 waves x 16 KiB of lists + 12 KiB of fragment records
// + 2.5 KiB of position / mass tables = 78.5 KiB, two workgroups per CU.
// Every global store is a plain vector store of an output element; the only
// atomics are LDS atomics.
//
//   k_align_split    the two-list split of the open intervals over the former's
//                    outputs (sst_align_split_device): one spectrum per
//                    workgroup, persistent grid.
//
// The workgroup scans the spectrum's status bytes and compacts the base-OPEN
// fragments, in their order, into the same LDS records (a chunk is closed once
// fewer than a scan block's worth of records are free); a spectrum without one
// costs that scan only.  The sweeps are the former's, over open intervals only:
// phase A builds the list up to the last closed interval [l, m*] and matches
// nothing; phase B starts a fresh list at m* + 1.  While it is closed, [l, r]
// is split-closed: the wave takes the cut's fragments one at a time, lanes
// over the entries a of A within [lo' - max(B), hi'], each searching B for the
// first entry >= lo' - a, and a ballot says whether any pair fits.  (Lanes
// over fragments would leave most of the wave idle, a spectrum has few OPEN
// fragments, and would walk A serially.)  Once B passes K every further
// interval of the sweep is undecided and only marks windows that meet [LO, HI].
// LDS per workgroup: 3 waves x 20 KiB (A, B's two lists, merge temp) + 12 KiB
// of records + 3 KiB of record -> fragment indices + 2.5 KiB of tables = 77.5
// KiB, two workgroups per CU.
#include "sst_align_common.h"

namespace sst {

namespace {

// dst = the distinct values of u[0, nu) and o[0, no) + d, ascending (u, o
// ascending and distinct; dst may be u; tmp holds nu + no words).  Returns
// their number; only the first kAlignK are stored.
__device__ __forceinline__ int union_shifted(const uint32_t* u, int nu, const uint32_t* o, int no, uint32_t d,
                                             uint32_t* tmp, uint32_t* dst, int lane) {
  for (int i = lane; i < nu; i += 64) {
    const uint32_t x = u[i];
    tmp[i + (x >= d ? lower_u32(o, no, x - d) : 0)] = x;  // before an equal shifted entry
  }
  for (int j = lane; j < no; j += 64) {
    const uint32_t y = o[j] + d;
    tmp[j + upper_u32(u, nu, y)] = y;
  }
  wave_sync();
  const int nt = nu + no;
  int base = 0;
  for (int c0 = 0; c0 < nt; c0 += 64) {
    const int k = c0 + lane;
    const bool keep = k < nt && (k == 0 || tmp[k - 1] != tmp[k]);
    const uint64_t m = __ballot(keep);
    const int at = base + (int)lanes_below(m);
    if (keep && at < kAlignK) dst[at] = tmp[k];
    base += __builtin_popcountll(m);
  }
  wave_sync();
  return base;
}

// One sweep of a wave: positions `from`, from + dir, ... to the skeleton's end.
__device__ __forceinline__ void sweep(AlignLds& s, uint32_t* mine, const sst_align_args& a, int64_t pos0, uint64_t a0,
                                      uint64_t a1, int L, int nf, int from, int dir, int lane) {
  uint32_t* cur = mine;                  // S(l, r) - LO
  uint32_t* other = mine + kAlignK;
  uint32_t* tmp = mine + 2 * kAlignK;
  if (lane == 0) cur[0] = 0;
  wave_sync();
  Interval iv{from, from, 0, 0, false, cur, 1};
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  for (int p = from; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;  // LO never falls: no later interval of this sweep meets a window
    if (!iv.open && pmax != pmin) {
      uint64_t m0, m1;
      position_set(a.skeleton, pos0 + p, a0, a1, m0, m1);
      const uint32_t* u = cur;  // the union so far: the copy of the position's smallest mass
      int nu = iv.n;
      for (int h = 0; h < 2 && !iv.open; ++h) {
        for (uint64_t m = h ? m1 : m0; m && !iv.open; m &= m - 1) {
          const uint32_t d = s.w[64 * h + __builtin_ctzll(m)] - pmin;
          if (d == 0) continue;
          nu = union_shifted(u, nu, cur, iv.n, d, tmp, other, lane);
          u = other;
          if (nu > kAlignK) iv.open = true;
        }
      }
      if (!iv.open && u == other) {
        uint32_t* x = cur;
        cur = other;
        other = x;
        iv.n = nu;
      }
      iv.list = cur;
    }
    match_fragments(s, nf, iv, dir > 0 ? 0 : 1, L, lane);
  }
}

__global__ __launch_bounds__(kAlignWG) void k_align_windows(AlignKArgs k) {
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const sst_align_args& a = k.a;
  AlignLds& s = *reinterpret_cast<AlignLds*>(align_lds + kAlignWaves * kAlignWaveWords);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* mine = align_lds + wave * kAlignWaveWords;

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kAlignWG) s.w[r] = r < k.n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;  // rows 1 .. n_rows - 1
  if (k.n_rows < 64) {
    rows0 &= (1ull << k.n_rows) - 1;
    rows1 = 0;
  } else if (k.n_rows < 128) {
    rows1 = (1ull << (k.n_rows - 64)) - 1;
  }

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) continue;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    __syncthreads();  // the previous spectrum's LDS is no longer read
    if (tid == 0) s.flags = 0;
    __syncthreads();
    const bool modelled = L >= 0 && L <= kAlignMaxLen && n_pos == (int64_t)L;
    if (modelled) {
      for (int p = tid; p < L; p += kAlignWG) {
        uint64_t m0, m1;
        position_set(a.skeleton, pos0 + p, a0, a1, m0, m1);
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
    }
    __syncthreads();
    const bool infeasible = (s.flags & 1u) != 0;
    if (!modelled || infeasible) {  // one status for every fragment of the spectrum
      for (int64_t j = tid; j < nf_all; j += kAlignWG) {
        a.status[f0 + j] = infeasible ? SST_ALIGN_INFEASIBLE : SST_ALIGN_SKIPPED;
        a.alignable[f0 + j] = infeasible ? 0 : 1;
        a.n_fit[f0 + j] = 0;
        a.first[f0 + j] = 0xFFFE;
      }
      continue;
    }

    for (int64_t c0 = 0; c0 < nf_all; c0 += kAlignF) {
      const int nf = (int)(nf_all - c0 < kAlignF ? nf_all - c0 : kAlignF);
      __syncthreads();  // the previous chunk's records are written out
      if (tid == 0) {
        s.flags = 0;
        s.w_max = 0;
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kAlignWG) {
        const int64_t at = f0 + c0 + j;
        const int64_t t = clamp_f(rint_quot(a.frag_su[at], a.prec, k.rprec));
        int64_t w = clamp_f(ceil_quot(a.tol * a.frag_obs[at], a.prec, k.rprec));
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
      __syncthreads();
      for (int j = tid; j + 1 < nf; j += kAlignWG)
        if (s.f_t[j] > s.f_t[j + 1]) atomicOr(&s.flags, 2u);
      __syncthreads();
      const uint32_t present = s.flags >> 4;  // bit c: class c among the chunk's fragments
      // sweeps: t < L forward from t; t == L backward from L - 1; t == L + 1 the empty interval
      for (int t = wave; t < L + 2; t += kAlignWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u)) sweep(s, mine, a, pos0, a0, a1, L, nf, t, 1, lane);
        } else if (t == L) {
          if (present & 0x4u) sweep(s, mine, a, pos0, a0, a1, L, nf, L - 1, -1, lane);
        } else if (present & (L == 0 ? 0x9u : 0x1u)) {
          if (lane == 0) mine[0] = 0;
          wave_sync();
          const Interval iv{0xFF, 0xFF, 0, 0, false, mine, 1};
          match_fragments(s, nf, iv, 2, L, lane);
        }
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kAlignWG) {
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

// ---------------------------------------------------------------------------
// k_align_split: the two-list split of the open intervals
// (sst_align_split_device).  Input: the four outputs of k_align_windows.
// ---------------------------------------------------------------------------
// The fragments of the chunk the split-closed interval iv (LO, HI of both
// halves together) is admissible for, one at a time by the whole wave: lanes
// over the entries a of A that can take part, each searching B for the first
// entry >= lo' - a; any lane's hit is a fit.  A, B: offsets from LO_A, LO_B.
__device__ __forceinline__ void match_split(AlignLds& s, int nf, const Interval& iv, const uint32_t* A, int nA,
                                            const uint32_t* B, int nB, int mode, int L, int lane) {
  const bool cut = !(s.flags & 2u);
  const int64_t wm = (int64_t)s.w_max;
  const int j0 = cut ? lower_i64(s.f_t, nf, iv.lo - wm) : 0;
  const int j1 = cut ? lower_i64(s.f_t, nf, iv.hi + wm + 1) : nf;
  const int64_t b_max = (int64_t)B[nB - 1];
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
    const int i0 = lo - b_max > 0 ? lower_u32(A, nA, (uint32_t)(lo - b_max)) : 0;
    const int i1 = hi >= (int64_t)A[nA - 1] ? nA : upper_u32(A, nA, (uint32_t)hi);
    bool fit = false;
    for (int c0 = i0; c0 < i1 && !fit; c0 += 64) {
      bool hit = false;
      const int i = c0 + lane;
      if (i < i1) {
        const int64_t a = (int64_t)A[i], need = lo - a;  // need <= b_max by i0
        const int at = need > 0 ? lower_u32(B, nB, (uint32_t)need) : 0;
        hit = at < nB && (int64_t)B[at] <= hi - a;
      }
      fit = __ballot(hit) != 0;
    }
    if (fit && lane == 0) {
      atomicAdd(&s.f_nfit[j], 1u);
      atomicMin(&s.f_first[j], (uint32_t)(iv.l << 8 | iv.r));
    }
  }
}

// dst (n entries so far, a closed list) extended by position p as sweep()
// does; the new count, above kAlignK if the union passes it (dst is then
// intact, the partial union is in `other`).  Swaps dst / other when it moves.
__device__ __forceinline__ int extend_list(AlignLds& s, uint32_t*& cur, uint32_t*& other, uint32_t* tmp, int n,
                                           const sst_align_args& a, int64_t at, uint64_t a0, uint64_t a1,
                                           uint32_t pmin, int lane) {
  uint64_t m0, m1;
  position_set(a.skeleton, at, a0, a1, m0, m1);
  const uint32_t* u = cur;
  int nu = n;
  for (int h = 0; h < 2; ++h) {
    for (uint64_t m = h ? m1 : m0; m; m &= m - 1) {
      const uint32_t d = s.w[64 * h + __builtin_ctzll(m)] - pmin;
      if (d == 0) continue;
      nu = union_shifted(u, nu, cur, n, d, tmp, other, lane);
      u = other;
      if (nu > kAlignK) return nu;
    }
  }
  if (u == other) {
    uint32_t* x = cur;
    cur = other;
    other = x;
  }
  return nu;
}

// One sweep of a wave over the open intervals only.  Phase A: the list of
// sweep() up to the last closed interval [from, m*] (nothing is matched: a
// base-OPEN fragment has no closed fit).  Phase B: a fresh list from m* + dir;
// while it is closed the interval is split-closed (match_split), afterwards
// undecided: only LO and HI move and a window that meets them is marked open.
__device__ __forceinline__ void sweep_split(AlignLds& s, uint32_t* mine, const sst_align_args& a, int64_t pos0,
                                            uint64_t a0, uint64_t a1, int L, int nf, int from, int dir, int lane) {
  uint32_t* la = mine;
  uint32_t* lb = mine + kAlignK;
  uint32_t* spare = mine + 2 * kAlignK;
  uint32_t* tmp = mine + 3 * kAlignK;
  if (lane == 0) la[0] = 0;
  wave_sync();
  const bool prune = !(s.flags & 2u);
  const int64_t t_last = s.f_t[nf - 1], wm = (int64_t)s.w_max;
  int64_t lo = 0, hi = 0;
  int nA = 1, p = from;
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    if (prune && lo + pmin - wm > t_last) return;  // LO never falls
    if (pmax != pmin) {
      const int n = extend_list(s, la, spare, tmp, nA, a, pos0 + p, a0, a1, pmin, lane);
      if (n > kAlignK) break;  // [from, p] is open: A = S(from, p - dir)
      nA = n;
    }
    lo += pmin;
    hi += pmax;
  }
  if (p < 0 || p >= L || p == from) return;  // no open interval in this sweep
  if (lane == 0) lb[0] = 0;
  wave_sync();
  int nB = 1;
  Interval iv{from, from, lo, hi, false, lb, 1};
  for (; p >= 0 && p < L; p += dir) {
    const uint32_t pmin = s.p_min[p], pmax = s.p_max[p];
    iv.lo += pmin;
    iv.hi += pmax;
    if (dir > 0) iv.r = p; else iv.l = p;
    if (prune && iv.lo - wm > t_last) break;
    if (!iv.open && pmax != pmin) {
      const int n = extend_list(s, lb, spare, tmp, nB, a, pos0 + p, a0, a1, pmin, lane);
      if (n > kAlignK) iv.open = true; else nB = n;
    }
    if (iv.open)
      match_fragments(s, nf, iv, dir > 0 ? 0 : 1, L, lane);
    else
      match_split(s, nf, iv, la, nA, lb, nB, dir > 0 ? 0 : 1, L, lane);
  }
}

__global__ __launch_bounds__(kSplitWG) void k_align_split(AlignKArgs k) {
  extern __shared__ __attribute__((aligned(16))) uint32_t align_lds[];
  const sst_align_args& a = k.a;
  SplitLds& sl = *reinterpret_cast<SplitLds*>(align_lds + kSplitWaves * kSplitWaveWords);
  AlignLds& s = sl.s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* mine = align_lds + wave * kSplitWaveWords;

  for (int r = tid; r < SST_MAX_ROWS + 8; r += kSplitWG) s.w[r] = r < k.n_rows ? (uint32_t)k.w[r] : 0u;
  uint64_t rows0 = ~1ull, rows1 = ~0ull;  // rows 1 .. n_rows - 1
  if (k.n_rows < 64) {
    rows0 &= (1ull << k.n_rows) - 1;
    rows1 = 0;
  } else if (k.n_rows < 128) {
    rows1 = (1ull << (k.n_rows - 64)) - 1;
  }

  for (int64_t g = blockIdx.x; g < a.n_spec; g += gridDim.x) {
    const int64_t f0 = a.frag_off[g], nf_all = a.frag_off[g + 1] - f0;
    if (nf_all <= 0) continue;
    const int64_t pos0 = a.pos_off[g], n_pos = a.pos_off[g + 1] - pos0;
    const int L = a.seq_len[g];
    // (a base-OPEN fragment implies a modelled spectrum; anything else in the status bytes is not followed)
    if (!(L >= 1 && L <= kAlignMaxLen && n_pos == (int64_t)L)) continue;
    const uint64_t a0 = a.alpha[2 * g] & rows0, a1 = a.alpha[2 * g + 1] & rows1;
    bool have_pos = false;

    for (int64_t next = 0; next < nf_all;) {
      __syncthreads();  // the previous chunk's records are written out
      if (tid == 0) {
        s.flags = 0;
        s.w_max = 0;
      }
      int nf = 0;
      // the next base-OPEN fragments, in order, until fewer than a block's worth of records are free
      while (next < nf_all && kAlignF - nf >= kSplitWG) {
        const int64_t j = next + tid;
        const bool open = j < nf_all && a.status[f0 + j] == SST_ALIGN_OPEN;
        const uint64_t m = __ballot(open);
        __syncthreads();  // wave_n of the previous block is read
        if (lane == 0) sl.wave_n[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        int before = nf, total = 0;
        for (int w = 0; w < kSplitWaves; ++w) {
          const int n = (int)sl.wave_n[w];
          if (w < wave) before += n;
          total += n;
        }
        if (open) sl.f_at[before + (int)lanes_below(m)] = j;
        nf += total;
        next += kSplitWG;
      }
      if (nf == 0) break;  // (only when the fragments are exhausted)
      __syncthreads();
      if (!have_pos) {  // the spectrum has a base-OPEN fragment: its positions' smallest / largest masses
        have_pos = true;
        for (int p = tid; p < L; p += kSplitWG) position_range(s, a.skeleton, pos0, p, a0, a1);
      }
      for (int j = tid; j < nf; j += kSplitWG) load_record(s, j, f0 + sl.f_at[j], a, k.rprec, L);
      __syncthreads();
      if (s.flags & 1u) break;  // an empty A_i (never with a base-OPEN fragment): the spectrum is left as it is
      for (int j = tid; j + 1 < nf; j += kSplitWG)
        if (s.f_t[j] > s.f_t[j + 1]) atomicOr(&s.flags, 2u);
      __syncthreads();
      const uint32_t present = s.flags >> 4;
      // sweeps: t < L forward from t; t == L backward from L - 1 (the empty interval is closed)
      for (int t = wave; t < L + 1; t += kSplitWaves) {
        if (t < L) {
          if (present & (t == 0 ? 0xBu : 0x1u)) sweep_split(s, mine, a, pos0, a0, a1, L, nf, t, 1, lane);
        } else if (present & 0x4u) {
          sweep_split(s, mine, a, pos0, a0, a1, L, nf, L - 1, -1, lane);
        }
      }
      __syncthreads();
      for (int j = tid; j < nf; j += kSplitWG) {
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

hipError_t launch_align_split(const sst_align_args& a, const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute((const void*)k_align_split, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kSplitLdsBytes))
    return e;
  AlignKArgs k{a, w, n_rows, 1.0 / a.prec};
  const unsigned grid = (unsigned)(a.n_spec < (int64_t)n_wg ? a.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_align_split, dim3(grid), dim3(kSplitWG), kSplitLdsBytes, st, k);
  return hipGetLastError();
}

hipError_t launch_align_windows(const sst_align_args& a, const int* w, int n_rows, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute((const void*)k_align_windows, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kAlignLdsBytes))
    return e;  // (per device: a process may hold one context per GPU)
  AlignKArgs k{a, w, n_rows, 1.0 / a.prec};
  const unsigned grid = (unsigned)(a.n_spec < (int64_t)n_wg ? a.n_spec : (int64_t)n_wg);
  hipLaunchKernelGGL(k_align_windows, dim3(grid), dim3(kAlignWG), kAlignLdsBytes, st, k);
  return hipGetLastError();
}

}  // namespace sst
