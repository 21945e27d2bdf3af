// sst_handoff.hip -- the device pipeline's dense per-spectrum hand-off
// (gfx950): what Predictor.predict holds when it reaches its MILP stages
// (prediction.py:88-103 after build_skeleton, skeleton_building.py:67-109),
// compacted per spectrum so that one download per array delivers it.
//
//   k_handoff_count  n_frag[g] = the flagged rows among spectrum g's cnt[g]
//                    rows (slots 4 * peak_off[g] + i), n_pos[g] = seq_len[g];
//                    both 0 where active[g] == 0.  The caller scans both
//                    (launch_scan_u32) into frag_off / pos_off.
//   k_handoff_emit   the flagged rows of spectrum g in ascending row order (a
//                    stable compaction) as structure-of-arrays records at
//                    frag_off[g], and the first seq_len[g] position masks of
//                    its combined skeleton at pos_off[g].
//
// One wave (64 lanes) per spectrum, grid-stride over spectra; the wave walks
// its rows in tiles of 64: ballot of the flag, each lane's rank among the
// tile's survivors by mbcnt, a wave-uniform running base, plain vector stores.
// No LDS, no atomics; every offset 64-bit.  A spectrum of 65 532 rows is 1 024
// tiles of one wave -- such spectra are rare.  Both kernels move few bytes per
// row (1 flag byte read; 33 bytes written per survivor) and are bound by the
// launch and the rows' flag reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sst_internal.h"

namespace sst {

namespace {

constexpr int kHandoffWG = 256;  // 4 waves: 4 spectra per workgroup pass

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kHandoffWG) void k_handoff_count(sst_handoff_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kHandoffWG / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (kHandoffWG / 64);
  for (int64_t g = wave; g < a.n_spec; g += n_waves) {
    uint32_t n = 0, L = 0;
    if (a.active[g]) {
      const int64_t off = 4 * a.peak_off[g];
      const int64_t rows = (int64_t)a.cnt[g];
      for (int64_t i0 = 0; i0 < rows; i0 += 64) {  // (wave-uniform trip count: every lane reaches the ballot)
        const int64_t i = i0 + lane;
        const bool on = i < rows && a.flags[off + i] != 0;
        n += (uint32_t)__builtin_popcountll(__ballot(on));
      }
      const int32_t sl = a.seq_len[g];
      L = sl > 0 ? (uint32_t)sl : 0u;
    }
    if (lane == 0) {
      a.n_frag[g] = n;
      a.n_pos[g] = L;
    }
  }
}

__global__ __launch_bounds__(kHandoffWG) void k_handoff_emit(sst_handoff_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kHandoffWG / 64) + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (kHandoffWG / 64);
  for (int64_t g = wave; g < a.n_spec; g += n_waves) {
    if (!a.active[g]) continue;
    const int64_t off = 4 * a.peak_off[g];
    const int64_t rows = (int64_t)a.cnt[g];
    uint64_t base = a.frag_off[g];  // wave-uniform: the spectrum's next free record
    for (int64_t i0 = 0; i0 < rows; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool on = i < rows && a.flags[off + i] != 0;
      const uint64_t m = __ballot(on);
      if (on) {
        const uint64_t at = base + lanes_below(m);
        a.index[at] = (int32_t)i;
        a.code[at] = (uint8_t)(a.r_meta[off + i] & 0x1fu);
        a.su[at] = a.r_su[off + i];
        a.obs[at] = a.r_ob[off + i];
        a.out_min_end[at] = a.min_end[off + i];
        a.out_max_end[at] = a.max_end[off + i];
      }
      base += (uint64_t)__builtin_popcountll(m);
    }
    // the combined skeleton's used positions (seq_len of the max_len reserved), two u64 words each
    const int32_t sl = a.seq_len[g];
    const int64_t words = sl > 0 ? 2 * (int64_t)sl : 0;
    const uint64_t* src = a.comb + 2 * a.comb_off[g];
    uint64_t* dst = a.skeleton + 2 * a.pos_off[g];
    for (int64_t k = lane; k < words; k += 64) dst[k] = src[k];
  }
}

unsigned handoff_grid(int64_t n_spec, int n_wg) {
  const int64_t need = (n_spec + kHandoffWG / 64 - 1) / (kHandoffWG / 64);
  return (unsigned)(need < (int64_t)n_wg ? need : (int64_t)n_wg);
}

}  // namespace

hipError_t launch_handoff_count(const sst_handoff_args& a, int n_wg, hipStream_t st) {
  if (a.n_spec > 0) hipLaunchKernelGGL(k_handoff_count, dim3(handoff_grid(a.n_spec, n_wg)), dim3(kHandoffWG), 0, st, a);
  if (hipError_t e = hipGetLastError()) return e;
  if (hipError_t e = launch_scan_u32(a.n_frag, a.frag_off, a.n_spec, st)) return e;
  return launch_scan_u32(a.n_pos, a.pos_off, a.n_spec, st);
}

hipError_t launch_handoff_emit(const sst_handoff_args& a, int n_wg, hipStream_t st) {
  if (a.n_spec <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_handoff_emit, dim3(handoff_grid(a.n_spec, n_wg)), dim3(kHandoffWG), 0, st, a);
  return hipGetLastError();
}

}  // namespace sst
