// What the two sliding-window loops share (window_test.hip: ScanNet; kitti_window_test.hip: SemanticKITTI): the chunking of
// a scene into waves of 64 consecutive points and the per-window scan of the chunk histogram; and what the two SemanticKITTI
// loops share (kitti_window_test.hip, kitti_block_test.hip): a point's windows as one range per axis and the wave's rectangle.
#pragma once
#include "common.hpp"

namespace pasnl {

// pass 2: per window an exclusive scan over the chunks, in place; counts[w] = the window's size
static __global__ __launch_bounds__(256) void window_scan_kernel(long nchunks, int* __restrict__ hist, int* __restrict__ counts) {
  __shared__ int wsum[4];
  int* row = hist + (size_t)blockIdx.x * nchunks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (long base = 0; base < nchunks; base += 256) {
    const long k = base + threadIdx.x;
    const int v = k < nchunks ? row[k] : 0;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      all += wsum[w];
    }
    if (k < nchunks) row[k] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

struct KWinMember {
  int xlo, xhi, ylo, yhi;  // an empty range on either axis, or z outside: xhi < xlo
};

// the rectangle of windows that holds every membership of the wave's 64 points (empty: xhi < xlo): uniform over the wave
__device__ __forceinline__ KWinMember wave_rect(KWinMember m) {
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(m.xlo, o, 64), b = __shfl_xor(m.xhi, o, 64), c = __shfl_xor(m.ylo, o, 64), d = __shfl_xor(m.yhi, o, 64);
    m.xlo = a < m.xlo ? a : m.xlo;
    m.xhi = b > m.xhi ? b : m.xhi;
    m.ylo = c < m.ylo ? c : m.ylo;
    m.yhi = d > m.yhi ? d : m.yhi;
  }
  m.xlo = __builtin_amdgcn_readfirstlane(m.xlo);  // every lane holds the same four values: the loops over them are scalar
  m.xhi = __builtin_amdgcn_readfirstlane(m.xhi);
  m.ylo = __builtin_amdgcn_readfirstlane(m.ylo);
  m.yhi = __builtin_amdgcn_readfirstlane(m.yhi);
  return m;
}

}  // namespace pasnl

static inline unsigned wt_blocks(long n, int t) { return (unsigned)((n + t - 1) / t); }
static inline long wt_chunks(long n) { return (n + 63) / 64; }
