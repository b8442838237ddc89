// Device pieces the two test loops share (scan_test.hip: SemanticKITTI; scene_test.hip and the fused pick of crop.hip:
// ScanNet): numpy's argmin and min on float64, the LDS sort of a crop's (d2, position) pairs, a NaN-propagating max, the
// winner mark and the float32 softmax of a crop's votes.
#pragma once
#include "common.hpp"

namespace pasnl {

constexpr int ST_THREADS = 1024;
constexpr int ST_WAVES = ST_THREADS / 64;

// numpy argmin order on float64: a NaN first (the first NaN), then the smaller value, then the lower index (-0 == +0)
__device__ __forceinline__ bool st_before(double va, long ia, double vb, long ib) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return na;
  if (na) return ia < ib;
  return va < vb || (va == vb && ia < ib);
}

// (value, index) argmin over [0, n) of v[] by one workgroup of ST_THREADS; every thread returns the winner's index (-1 if n == 0)
__device__ inline long st_argmin(const double* __restrict__ v, long n, double* shv, long* shi) {
  double bv = 0.0;
  long bi = -1;
  for (long i = threadIdx.x; i < n; i += ST_THREADS) {
    const double x = v[i];
    if (bi < 0 || st_before(x, i, bv, bi)) { bv = x; bi = i; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const long oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (bi < 0 || st_before(ov, oi, bv, bi))) { bv = ov; bi = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { shv[wave] = bv; shi[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < ST_WAVES; ++w)
      if (shi[w] >= 0 && (shi[0] < 0 || st_before(shv[w], shi[w], shv[0], shi[0]))) { shv[0] = shv[w]; shi[0] = shi[w]; }
  }
  __syncthreads();
  const long r = shi[0];
  __syncthreads();
  return r;
}

// np.min of v[0..n) by one workgroup of ST_THREADS (NaN propagates); the value is thread 0's.  sh: ST_WAVES doubles.
__device__ __forceinline__ double st_min(const double* __restrict__ p, long n, double* sh) {
  double m = __builtin_inf();
  bool nan = false;
  for (long i = threadIdx.x; i < n; i += ST_THREADS) {
    const double x = p[i];
    nan |= x != x;
    m = x < m ? x : m;
  }
  if (nan) m = __builtin_nan("");
  for (int o = 32; o > 0; o >>= 1) {
    const double q = __shfl_xor(m, o, 64);
    m = (m != m || q != q) ? __builtin_nan("") : (q < m ? q : m);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < ST_WAVES; ++w) m = (m != m || sh[w] != sh[w]) ? __builtin_nan("") : (sh[w] < m ? sh[w] : m);
  return m;
}

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : (a > b ? a : b); }

// np.mean(axis=0) of an (N,3) array is, per column, ONE sum in row order: a dependent chain of N adds.  This continues the
// chain `acc` of column `col` down rows [0, cnt) of a 3-wide row-major tile (the loads go eight at a time ahead of the adds;
// the adds stay in order).  A chain starts at -0: -0 + x == x for every x, so it starts at the first row as numpy's does.
template <typename T>
__device__ __forceinline__ T st_chain3(T acc, const T* tile, int cnt, int col) {
  int k = 0;
  for (; k + 8 <= cnt; k += 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = tile[(k + u) * 3 + col];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = acc + v[u];
  }
  for (; k < cnt; ++k) acc = acc + tile[k * 3 + col];
  return acc;
}

// ---- votes of a crop: of the rows that select the same point the last one wins; win[] holds -1 between crops
static __global__ __launch_bounds__(256) void vote_mark_kernel(int num_point, const int* __restrict__ select, int* __restrict__ win) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < num_point) atomicMax(&win[select[j]], j);
}

// tf.nn.softmax of one row in float32: max, exp(x - max), their sum in index order, the division.  The two pieces serve a
// row that is read in passes (grid_eval.hip: from LDS, no private array): the same function on the same argument gives the
// same bits, so a term recomputed from (m, s) is the term vote_softmax stores.
__device__ __forceinline__ float vote_softmax_term(float x, float m) { return expf(x - m); }
__device__ __forceinline__ void vote_softmax_max_sum(const float* v, int nc, float& m, float& s) {
  m = v[0];
  for (int q = 1; q < nc; ++q) m = v[q] > m ? v[q] : m;
  s = 0.0f;
  for (int q = 0; q < nc; ++q) s += vote_softmax_term(v[q], m);
}
__device__ __forceinline__ void vote_softmax(const float* __restrict__ v, int nc, float* p) {
  float m = v[0];
  for (int q = 1; q < nc; ++q) m = v[q] > m ? v[q] : m;
  float s = 0.0f;
  for (int q = 0; q < nc; ++q) { p[q] = vote_softmax_term(v[q], m); s += p[q]; }
  for (int q = 0; q < nc; ++q) p[q] = p[q] / s;
}

// ---- order / permute: bitonic sort of (d2 bits, position) in LDS.  The flipped-merge form sorts any count m without padding:
// a partner at or past m would be +inf and never moves, so those compare-exchanges are skipped.
constexpr int OP_CAP = 14336;  // 14336 * 10 B = 140 KiB of LDS (gfx950: 160 KiB per workgroup)

__device__ __forceinline__ void op_cx(unsigned long long* key, unsigned short* pos, int i, int j) {
  const unsigned long long ki = key[i], kj = key[j];
  const unsigned short pi = pos[i], pj = pos[j];
  if (ki > kj || (ki == kj && pi > pj)) { key[i] = kj; key[j] = ki; pos[i] = pj; pos[j] = pi; }
}

// sorts key[0..m) ascending by (key, pos) with pos[] carried along; one workgroup of ST_THREADS, ends on a barrier
__device__ __forceinline__ void op_sort(unsigned long long* key, unsigned short* pos, int m) {
  const int tid = threadIdx.x;
  int p2 = 1;
  while (p2 < m) p2 <<= 1;
  for (int size = 2; size <= p2; size <<= 1) {
    const int half = size >> 1;
    for (int t = tid; t < p2 / 2; t += ST_THREADS) {
      const int g = t / half, r = t % half;
      const int i = g * size + r, j = g * size + size - 1 - r;
      if (j < m) op_cx(key, pos, i, j);
    }
    __syncthreads();
    for (int stride = half >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < p2 / 2; t += ST_THREADS) {
        const int i = (t / stride) * 2 * stride + t % stride, j = i + stride;
        if (j < m) op_cx(key, pos, i, j);
      }
      __syncthreads();
    }
  }
}

}  // namespace pasnl
