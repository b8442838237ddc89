// The ScanNet sliding-window whole-scene test loop around the forward, on the device: reference ScanNet/scannet_dataset.py
// (D) :183-300 `ScannetDatasetWholeSceneSlidingWindow.__getitem__` -- move a fifth of the scene's points by noise, cut the
// scene into overlapping 1.5 m windows, merge the small ones, deal every block out in rows of block_points -- and
// ScanNet/test_scannet.py (T) :96-103, 143-163 -- argmax over classes 1..C-1, one integer vote per weighted row entry, the
// argmax of the pool.  The third sibling of scan_test.hip and scene_test.hip.  Everything that has to equal numpy is done in
// numpy's dtypes and order (the library builds with -ffp-contract=off); the exactness contract is stated in include/pasnl.h
// per entry point and restated on the host in tests/window_flow_ref.py.
//
// What stays on the host: the numpy RNG stream (choices, shifts, the blocks' shuffles) and the merge of small blocks, which
// works on per-window counts and centres only.  One vote of one scene is
//   pasnl_window_noise (2 launches) -> pasnl_window_bounds (1) -> [six floats down] -> pasnl_window_count (clear + 2) ->
//   [W counts down; merge; permutations up] -> pasnl_window_fill (1) -> per batch: pasnl_window_gather, forward,
//   pasnl_window_vote with no synchronisation in between.
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"
#include "window_scan.hpp"

namespace pasnl {

// ---- the noise step (D:192-212)
constexpr int WT_TILE = 4096;                          // points per staged tile: 48 KiB of LDS
constexpr int WT_PER = WT_TILE * 3 / ST_THREADS;       // floats a thread stages per tile

// np.mean(raw_xyz, axis=0) of a float32 (N,3) view is, per column, one float32 sum in index order divided by float32(N): a
// dependent chain of N adds.  The workgroup stages tiles into LDS (the next tile's loads are in flight while the chain
// runs) and lanes 0..2 of the first wave carry the x, y and z chains.  Then all threads take max / min of raw - centroid
// over the three columns together.  -> stats[0..3) = centroid, stats[3] = max_length.
__global__ __launch_bounds__(ST_THREADS) void window_centroid_kernel(long n, const float* __restrict__ xyz, float* __restrict__ stats) {
  __shared__ float tile[WT_TILE * 3];
  __shared__ float shmax[ST_WAVES], shmin[ST_WAVES], cen[3];
  const int tid = threadIdx.x;
  const long total = n * 3;
  float reg[WT_PER];
#pragma unroll
  for (int q = 0; q < WT_PER; ++q) {
    const long k = (long)q * ST_THREADS + tid;
    reg[q] = k < total ? xyz[k] : 0.0f;
  }
  float acc = -0.0f;  // -0 + x == x for every x: the chain starts at the first row as numpy's does
  for (long base = 0; base < total; base += WT_TILE * 3) {
#pragma unroll
    for (int q = 0; q < WT_PER; ++q) tile[q * ST_THREADS + tid] = reg[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < WT_PER; ++q) {
      const long k = base + WT_TILE * 3 + (long)q * ST_THREADS + tid;
      reg[q] = k < total ? xyz[k] : 0.0f;
    }
    if (tid < 3) {
      const long left = n - base / 3;
      const int cnt = left < WT_TILE ? (int)left : WT_TILE;
      acc = st_chain3(acc, tile, cnt, tid);
    }
    __syncthreads();
  }
  if (tid < 3) cen[tid] = acc / (float)n;
  __syncthreads();
  float mx = -__builtin_inff(), mn = __builtin_inff();
  int a = tid % 3;  // ST_THREADS % 3 == 1: the column advances by one per trip
  for (long k = tid; k < total; k += ST_THREADS) {
    const float v = xyz[k] - cen[a];
    mx = v > mx ? v : mx;
    mn = v < mn ? v : mn;
    a = a == 2 ? 0 : a + 1;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float p = __shfl_xor(mx, o, 64), q = __shfl_xor(mn, o, 64);
    mx = p > mx ? p : mx;
    mn = q < mn ? q : mn;
  }
  if ((tid & 63) == 0) { shmax[tid >> 6] = mx; shmin[tid >> 6] = mn; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < ST_WAVES; ++w) {
      mx = shmax[w] > mx ? shmax[w] : mx;
      mn = shmin[w] < mn ? shmin[w] : mn;
    }
    const float hi = fabsf(mx), lo = fabsf(mn);
    stats[0] = cen[0]; stats[1] = cen[1]; stats[2] = cen[2];
    stats[3] = lo > hi ? lo : hi;  // max(abs(max_l), abs(min_l))
  }
}
static_assert(ST_THREADS % 3 == 1, "the column walk of window_centroid_kernel");

// point_set_ini[choices, 0:3] = (normalized[choices] + shift) * max_length + centroid, and semantic_seg_ini[choices] = 0 as a
// stamp: one thread per draw, only the last occurrence of a point stores (it reads nothing but its own row, so in place).
__global__ __launch_bounds__(256) void window_move_kernel(int m, const int* __restrict__ choices, const double* __restrict__ shift,
                                                          const unsigned char* __restrict__ last, const float* __restrict__ stats,
                                                          long n, float* __restrict__ xyz, int* __restrict__ stamp, int serial) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m || !last[j]) return;
  const long i = choices[j];
  if (i < 0 || i >= n) return;
  const float ml = stats[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float nrm = (xyz[i * 3 + a] - stats[a]) / ml;  // float32 - float32, float32 / float32
    double v = (double)nrm + shift[(size_t)j * 3 + a];   // float64 from here
    v = v * (double)ml;
    v = v + (double)stats[a];
    xyz[i * 3 + a] = (float)v;
  }
  stamp[i] = serial;
}

// ---- np.min / np.max over axis 0 (D:214-215): one workgroup -> out[0..3) = coordmin, out[3..6) = coordmax
__global__ __launch_bounds__(ST_THREADS) void window_bounds_kernel(long n, const float* __restrict__ xyz, float* __restrict__ out) {
  __shared__ float sh[ST_WAVES][6];
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (long p = threadIdx.x; p < n; p += ST_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = xyz[p * 3 + a];
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float p = __shfl_xor(lo[a], o, 64), q = __shfl_xor(hi[a], o, 64);
      lo[a] = p < lo[a] ? p : lo[a];
      hi[a] = q > hi[a] ? q : hi[a];
    }
  }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) { sh[threadIdx.x >> 6][a] = lo[a]; sh[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = sh[0][a];
    for (int w = 1; w < ST_WAVES; ++w) v = a < 3 ? (sh[w][a] < v ? sh[w][a] : v) : (sh[w][a] > v ? sh[w][a] : v);
    out[a] = v;
  }
}

// ---- windows (D:223-242): curmin = float64(coordmin) + i * delta, curmax = curmin + 1.5, membership inside 0.2 and the mask
// inside 0.001 -- window_scan.hpp's three passes over this grid
static inline ColumnGrid window_grid(int nx, int ny, double delta) { return {nx, ny, delta, 1.5, false, 0.2, 0.001}; }

// ---- rows (D:271-300): one thread per row entry
__global__ __launch_bounds__(256) void window_gather_kernel(long entries, long real_entries, const int* __restrict__ rowpos, long cap,
                                                            const int* __restrict__ cat_idx, const unsigned char* __restrict__ cat_mask,
                                                            long n, const float* __restrict__ xyz, const float* __restrict__ rgb, int nfeat,
                                                            const int* __restrict__ labels, const int* __restrict__ stamp, int serial,
                                                            float* __restrict__ out_data, int* __restrict__ out_label,
                                                            int* __restrict__ out_weight, int* __restrict__ out_idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int width = 3 + nfeat;
  float* row = out_data + (size_t)e * width;
  long pos = e < real_entries ? (long)rowpos[e] : -1;
  long i = pos >= 0 && pos < cap ? (long)cat_idx[pos] : -1;
  if (i < 0 || i >= n) {  // a row past the scene's last one: zeros (an index outside the lists is never drawn)
    for (int f = 0; f < width; ++f) row[f] = 0.0f;
    out_label[e] = 0; out_weight[e] = 0; out_idx[e] = 0;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) row[a] = xyz[i * 3 + a];
  for (int f = 0; f < nfeat; ++f) row[3 + f] = rgb[i * nfeat + f];
  out_label[e] = stamp[i] == serial ? 0 : labels[i];
  out_weight[e] = cat_mask[pos];
  out_idx[e] = (int)i;
}

// ---- votes (T:159-161, 96-103): integer counters, exact and order-free
__global__ __launch_bounds__(256) void window_vote_kernel(long entries, int c, const float* __restrict__ logits, const int* __restrict__ idx,
                                                          const int* __restrict__ weight, long n, int* __restrict__ pool) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries || weight[e] == 0) return;
  const float* row = logits + (size_t)e * c;
  int a = 1;
  float best = row[1];
  bool nan = best != best;
  for (int q = 2; q < c && !nan; ++q) {  // np.argmax(pred_val[:, :, 1:], 2) + 1: the first maximum, the first NaN
    const float v = row[q];
    if (v > best || v != v) { best = v; a = q; nan = v != v; }
  }
  const long i = idx[e];
  if (i < 0 || i >= n) return;
  atomicAdd(&pool[(size_t)i * c + a], 1);
}

// np.argmax(vote_label_pool, 1): the first maximum; a row without a vote gives 0
__global__ __launch_bounds__(256) void window_pool_labels_kernel(long n, int c, const int* __restrict__ pool, int* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* row = pool + (size_t)i * c;
  int a = 0, best = row[0];
  for (int q = 1; q < c; ++q)
    if (row[q] > best) { best = row[q]; a = q; }
  out[i] = a;
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_window_noise(long n, float* xyz, int m, const int* choices, const double* shift, const unsigned char* last,
                                  int serial, int* stamp, float* stats, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && m >= 0 && n <= (1L << 30), PASNL_EINVAL);
  PASNL_REQUIRE(xyz && stamp && stats && (m == 0 || (choices && shift && last)), PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  hipLaunchKernelGGL(window_centroid_kernel, dim3(1), dim3(ST_THREADS), 0, s, n, xyz, stats);
  if (m > 0)
    hipLaunchKernelGGL(window_move_kernel, dim3(wt_blocks(m, 256)), dim3(256), 0, s, m, choices, shift, last, stats, n, xyz, stamp, serial);
  return pasnl_launch_status();
}

extern "C" int pasnl_window_bounds(long n, const float* xyz, float* out_bounds, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30), PASNL_EINVAL);
  PASNL_REQUIRE(xyz && out_bounds, PASNL_ENULL);
  hipLaunchKernelGGL(window_bounds_kernel, dim3(1), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), n, xyz, out_bounds);
  return pasnl_launch_status();
}

extern "C" size_t pasnl_window_hist_bytes(long n, int nx, int ny) { return wt_hist_bytes(n, nx, ny); }

extern "C" int pasnl_window_count(long n, const float* xyz, const float* bounds, int nx, int ny, double delta, int* hist, int* out_counts,
                                  pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && delta > 0.0, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  return wt_count(n, xyz, bounds, window_grid(nx, ny, delta), hist, out_counts, pasnl_hip_stream(stream));
}

extern "C" int pasnl_window_fill(long n, const float* xyz, const float* bounds, int nx, int ny, double delta, const int* hist,
                                 const int* woff, long cap, int* out_idx, unsigned char* out_mask, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && delta > 0.0 && cap > 0, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx && out_mask, PASNL_ENULL);
  return wt_fill(n, xyz, bounds, window_grid(nx, ny, delta), -1, 0.0, hist, woff, cap, out_idx, out_mask, pasnl_hip_stream(stream));
}

extern "C" int pasnl_window_gather(int rows, int real_rows, int block_points, const int* rowpos, long cap, const int* cat_idx,
                                   const unsigned char* cat_mask, long n, const float* xyz, const float* rgb, int nfeat, const int* labels,
                                   const int* stamp, int serial, float* out_data, int* out_label, int* out_weight, int* out_idx,
                                   pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && real_rows >= 0 && real_rows <= rows && block_points > 0 && nfeat >= 0 && n > 0 && cap > 0, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(cat_idx && cat_mask && xyz && labels && stamp && out_data && out_label && out_weight && out_idx &&
                    (real_rows == 0 || rowpos) && (nfeat == 0 || rgb), PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(window_gather_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries,
                     (long)real_rows * block_points, rowpos, cap, cat_idx, cat_mask, n, xyz, rgb, nfeat, labels, stamp, serial, out_data,
                     out_label, out_weight, out_idx);
  return pasnl_launch_status();
}

extern "C" int pasnl_window_vote(int rows, int block_points, int c, const float* logits, const int* idx, const int* weight, long n,
                                 int* pool, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && c >= 2 && n > 0, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && idx && weight && pool, PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(window_vote_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, c, logits, idx,
                     weight, n, pool);
  return pasnl_launch_status();
}

extern "C" int pasnl_window_pool_labels(long n, int c, const int* pool, int* out_labels, pasnl_stream_t stream) {
  PASNL_REQUIRE(n >= 0 && c >= 1, PASNL_EINVAL);
  if (n == 0) return PASNL_OK;
  PASNL_REQUIRE(pool && out_labels, PASNL_ENULL);
  hipLaunchKernelGGL(window_pool_labels_kernel, dim3(wt_blocks(n, 256)), dim3(256), 0, pasnl_hip_stream(stream), n, c, pool, out_labels);
  return pasnl_launch_status();
}
