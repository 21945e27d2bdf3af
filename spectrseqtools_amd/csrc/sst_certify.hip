// sst_certify.hip -- certify an uploaded packed table (gfx950): one streaming,
// read-only pass that proves the words are the table set_up_bit_table
// (mass_table.py:207-248) produces for the table's masses, so that the table
// can be given the state of one built here (sst_table_certify).
//
// The criterion is local: every word against words of the same table.  With
// pair(r, m) the 2-bit cell of mass m in row r (bits 2 * (C - 1 - m % C) of
// word (r, m / C); bit0 low, bit1 the "left" bit):
//   row 0        pair(0, 0) = 3, every other cell 0
//   row r >= 1   bit0(r, m) = [pair(r - 1, m) != 0]
//                bit1(r, m) = [m >= w_r and pair(r, m - w_r) != 0]
//   columns below the last: the word equals that expected word;
//   last column: one k in [0, C], the same for every row, with
//                word == expected & ((full << 2k) & full)
//                (the family of mass_table.py:246; max_mass is not known here).
// Only for rows with w_r >= C (the host checks): then the cell a left move
// reads lies in an earlier column than the cell itself: never in the same
// word and never in the last column, so the mask cannot leak into any cell.
//
//   k_table_certify<C>       one thread per word, grid (ceil(n_cols / 256)
//                            rounded up to a multiple of 8, n_rows).
//                            Word-parallel: the cells' "non-zero" flags are
//                            (x | x >> 1) & alt_sec; the expected bit1 field
//                            comes from the words of row r at columns
//                            c - step and c - step - 1 (step = w_r / C)
//                            shifted by w_r % C cells.  Lane i's second word is
//                            lane i - 1's first: one shuffle instead of a load
//                            (lane 0 loads its own).  Each XCD walks one
//                            contiguous eighth of every row, so the re-reads
//                            hit its L2 (0.277 -> 0.235 ms on the full table).
//   k_table_certify_last<C>  the last column alone, one thread per row: the
//                            first row at which the running intersection of
//                            the rows' admissible k becomes empty.  Launched
//                            only when the main kernel left no k.
//
// Output, 16 bytes: out[0] = min over violating words of row << 32 | column
// (one atomicMin per wave after a ballot), out[1] = the set of k every
// last-column word admits (atomicAnd, bit k).  No scratch buffer: a 582 MB
// table is checked with nothing allocated beside it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sst_internal.h"

namespace sst {

namespace {

constexpr int kCertifyWG = 256;

template <int C>
__device__ __forceinline__ uint64_t cword(const void* __restrict__ p, int64_t o) {
  if (C == 32) return ((const uint64_t*)p)[o];
  if (C == 16) return ((const uint32_t*)p)[o];
  if (C == 8) return ((const uint16_t*)p)[o];
  return ((const uint8_t*)p)[o];
}
template <int C>
__device__ __forceinline__ uint64_t cfull() {
  return C == 32 ? ~0ull : ((1ull << (2 * C)) - 1ull);
}
// per-cell "pair != 0" flags, at each cell's bit0
template <int C>
__device__ __forceinline__ uint64_t cells_set(uint64_t x) {
  return (x | (x >> 1)) & (0x5555555555555555ull & cfull<C>());
}
// the word set_up_bit_table leaves at (r >= 1, c) before the last-column mask:
// prev = word (r - 1, c), a = word (r, c - step), b = word (r, c - step - 1)
// (0 where the column is negative), shift = w_r % C
template <int C>
__device__ __forceinline__ uint64_t expected_word(uint64_t prev, uint64_t a, uint64_t b, int shift) {
  uint64_t left = cells_set<C>(a) >> (2 * shift);
  if (shift) left |= (cells_set<C>(b) << (2 * (C - shift))) & cfull<C>();
  return cells_set<C>(prev) | (left << 1);
}
// bit k: word == expected & ((full << 2k) & full), k in [0, C]
template <int C>
__device__ __forceinline__ uint64_t admissible_k(uint64_t word, uint64_t expected) {
  uint64_t set = 0;
  for (int k = 0; k <= C; ++k) {
    const uint64_t mask = k == C ? 0ull : (cfull<C>() << (2 * k)) & cfull<C>();
    if (word == (expected & mask)) set |= 1ull << k;
  }
  return set;
}

template <int C>
__global__ __launch_bounds__(kCertifyWG) void k_table_certify(const void* __restrict__ packed,
                                                              const int* __restrict__ w, int64_t n_cols,
                                                              unsigned long long* __restrict__ out) {
  const int r = blockIdx.y;
  // gridDim.x is a multiple of 8 and workgroups are dealt round-robin over the
  // 8 XCDs in launch order (observed, used for speed only): x % 8 names the
  // XCD in every row, and each XCD takes one contiguous eighth of the row in
  // ascending order, so the re-reads (the word above, the left move's words)
  // find the lines in that XCD's L2
  const unsigned per_xcd = gridDim.x / 8;
  const int64_t blk = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  const int64_t c = blk * kCertifyWG + threadIdx.x;
  const bool in = c < n_cols;
  const int64_t row = (int64_t)r * n_cols;
  uint64_t word = 0, expected = 0;
  if (r == 0) {  // (wave-uniform: the row is the block's)
    if (in) {
      word = cword<C>(packed, c);
      expected = c == 0 ? 3ull << (2 * C - 2) : 0ull;
    }
  } else {
    const int wr = w[r];
    const int shift = wr % C;
    const int64_t ca = c - wr / C;  // <= c: only the row start needs a bound
    uint64_t a = 0, prev = 0;
    if (in) {
      word = cword<C>(packed, row + c);
      prev = cword<C>(packed, row - n_cols + c);
      if (ca >= 0) a = cword<C>(packed, row + ca);
    }
    uint64_t b = 0;
    if (shift) {
      b = __shfl_up((unsigned long long)a, 1);  // lane i - 1 holds column c - 1: its `a` is word (r, ca - 1)
      if ((threadIdx.x & 63) == 0) b = in && ca >= 1 ? cword<C>(packed, row + ca - 1) : 0ull;
    }
    expected = expected_word<C>(prev, a, b, shift);
  }
  const bool last = c == n_cols - 1;
  const uint64_t bad = __ballot(in && !last && word != expected);
  if (bad && (threadIdx.x & 63) == 0) {
    const int64_t first = c + (__ffsll((unsigned long long)bad) - 1);  // lanes hold ascending columns
    atomicMin(out, (unsigned long long)r << 32 | (unsigned long long)first);
  }
  if (last) atomicAnd(out + 1, (unsigned long long)admissible_k<C>(word, expected));
}

template <int C>
__global__ __launch_bounds__(128) void k_table_certify_last(const void* __restrict__ packed,
                                                            const int* __restrict__ w, int n_rows, int64_t n_cols,
                                                            unsigned long long* __restrict__ out) {
  __shared__ uint64_t sets[128];
  const int r = threadIdx.x;
  const int64_t c = n_cols - 1;
  if (r < n_rows) {
    const int64_t row = (int64_t)r * n_cols;
    const uint64_t word = cword<C>(packed, row + c);
    uint64_t expected;
    if (r == 0) {
      expected = c == 0 ? 3ull << (2 * C - 2) : 0ull;
    } else {
      const int wr = w[r];
      const int64_t ca = c - wr / C;
      const uint64_t a = ca >= 0 ? cword<C>(packed, row + ca) : 0ull;
      const uint64_t b = ca >= 1 ? cword<C>(packed, row + ca - 1) : 0ull;
      expected = expected_word<C>(cword<C>(packed, row - n_cols + c), a, b, wr % C);
    }
    sets[r] = admissible_k<C>(word, expected);
  }
  __syncthreads();
  if (r == 0) {
    uint64_t run = ~0ull;
    for (int k = 0; k < n_rows; ++k) {
      run &= sets[k];
      if (!run) {
        atomicMin(out, (unsigned long long)k << 32 | (unsigned long long)c);
        break;
      }
    }
  }
}

}  // namespace

// out[2] on the device: {~0, ~0} before the first launch.  n_rows <= 120,
// n_cols < 2^31 / C (sst_table_upload checked both).
hipError_t launch_table_certify(int C, const void* packed, const int* w, int n_rows, int64_t n_cols,
                                unsigned long long* out, hipStream_t st) {
  const int64_t blocks = (n_cols + kCertifyWG - 1) / kCertifyWG;
  const dim3 grid((unsigned)((blocks + 7) / 8 * 8), (unsigned)n_rows);  // (whole blocks past n_cols idle)
  switch (C) {
    case 4: hipLaunchKernelGGL(k_table_certify<4>, grid, dim3(kCertifyWG), 0, st, packed, w, n_cols, out); break;
    case 8: hipLaunchKernelGGL(k_table_certify<8>, grid, dim3(kCertifyWG), 0, st, packed, w, n_cols, out); break;
    case 16: hipLaunchKernelGGL(k_table_certify<16>, grid, dim3(kCertifyWG), 0, st, packed, w, n_cols, out); break;
    default: hipLaunchKernelGGL(k_table_certify<32>, grid, dim3(kCertifyWG), 0, st, packed, w, n_cols, out);
  }
  return hipGetLastError();
}
hipError_t launch_table_certify_last(int C, const void* packed, const int* w, int n_rows, int64_t n_cols,
                                     unsigned long long* out, hipStream_t st) {
  if (n_rows > 128) return hipErrorInvalidValue;
  switch (C) {
    case 4: hipLaunchKernelGGL(k_table_certify_last<4>, dim3(1), dim3(128), 0, st, packed, w, n_rows, n_cols, out); break;
    case 8: hipLaunchKernelGGL(k_table_certify_last<8>, dim3(1), dim3(128), 0, st, packed, w, n_rows, n_cols, out); break;
    case 16: hipLaunchKernelGGL(k_table_certify_last<16>, dim3(1), dim3(128), 0, st, packed, w, n_rows, n_cols, out); break;
    default: hipLaunchKernelGGL(k_table_certify_last<32>, dim3(1), dim3(128), 0, st, packed, w, n_rows, n_cols, out);
  }
  return hipGetLastError();
}

}  // namespace sst
