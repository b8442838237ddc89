// The SemanticKITTI sliding-window whole-scan test loop around the forward, on the device: reference
// SemanticKITTI/semantic_kitti_dataset.py (D) :278-355 `SemanticKittiDatasetSlidingWindow.__getitem__` -- cut the scan into
// overlapping block_size windows at `stride`, merge the small ones (empty ones included), deal every block out in rows of
// block_points -- and SemanticKITTI/test_semantic_kitti.py (T) :99-105, 149-175 -- the optional rotation about z, argmax over
// classes 1..C-1, one integer vote per row entry, the argmax of the pool.  The sibling of window_test.hip for lidar scans:
// thousands of windows per scan, nearly all of them empty for any one wave, no noise step and no margin mask.  The vote and
// the pool's argmax are window_test.hip's pasnl_window_vote (with a weight buffer of ones) and pasnl_window_pool_labels.
//
// What stays on the host: the numpy RNG stream (the blocks' shuffles, the rotation angles) and the merge, which works on
// per-window counts and centres only.  One vote of one scan is
//   pasnl_window_bounds (1 launch) -> [six floats down] -> pasnl_kwindow_count (clear + 2) -> [W counts down; merge;
//   permutations up] -> pasnl_kwindow_fill (1) -> per batch: pasnl_kwindow_gather, forward, pasnl_window_vote with no
//   synchronisation in between.
#include <limits.h>
#include <math.h>
#include "common.hpp"
#include "window_scan.hpp"

namespace pasnl {

constexpr int KW_WAVES = 4;  // chunks (of 64 consecutive points, one wave each) per workgroup

// The windows of one axis that hold coordinate p: lo..hi, none when hi < lo.  The comparisons are the reference's own: the
// float32 coordinate, widened, against the float64 bounds curmin - 0.2 and curmax + 0.2 with curmin = origin + i * stride and
// curmax = curmin + block -- every window of the axis is tested, no index is derived from a division.  Both bounds are
// monotone in i (sums and products of rounded monotone terms), so the members are one contiguous range.
__device__ __forceinline__ void axis_range(double p, double origin, int count, double stride, double block, int& lo, int& hi) {
  lo = count;
  hi = -1;
  for (int i = 0; i < count; ++i) {
    const double curmin = origin + (double)i * stride;
    const double curmax = curmin + block;
    if (p >= curmin - 0.2 && p <= curmax + 0.2) {
      lo = i < lo ? i : lo;
      hi = i;
    }
  }
}

__device__ __forceinline__ KWinMember kwin_member(const float* __restrict__ p, const float* __restrict__ b, int nx, int ny, double block,
                                                  double stride) {
  KWinMember m;
  axis_range((double)p[0], (double)b[0], nx, stride, block, m.xlo, m.xhi);
  axis_range((double)p[1], (double)b[1], ny, stride, block, m.ylo, m.yhi);
  const double pz = (double)p[2];
  const double zmin = (double)b[2] + 0.0;
  const double zmax = zmin + (double)(b[5] - b[2]);  // float64(float32(coordmax_z - coordmin_z))
  const bool z = pz >= zmin - 0.2 && pz <= zmax + 0.2;
  if (!z || m.yhi < m.ylo || m.xhi < m.xlo) m = {nx, -1, ny, -1};
  return m;
}

// pass 1: hist[w][chunk] = members of window w among the chunk's 64 points (a ballot: no atomics at all).  hist is cleared
// beforehand: a wave stores only for the windows that hold one of its points.
__global__ __launch_bounds__(64 * KW_WAVES) void kwindow_count_kernel(long n, const float* __restrict__ xyz, const float* __restrict__ bounds,
                                                                      int nx, int ny, double block, double stride, long nchunks,
                                                                      int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * KW_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // whole waves leave
  const long p = c * 64 + lane;
  KWinMember m = {nx, -1, ny, -1};
  if (p < n) m = kwin_member(xyz + p * 3, bounds, nx, ny, block, stride);
  const KWinMember r = wave_rect(m);
  for (int i = r.xlo; i <= r.xhi; ++i) {
    const bool fx = i >= m.xlo && i <= m.xhi;
    for (int j = r.ylo; j <= r.yhi; ++j) {
      const unsigned long long ballot = __ballot(fx && j >= m.ylo && j <= m.yhi);
      if (ballot != 0ull && lane == 0) hist[((size_t)i * ny + j) * nchunks + c] = __popcll(ballot);
    }
  }
}

// pass 3 (pass 2 is window_scan_kernel): a member's place is woff[w] + (members in earlier chunks) + (members among the lower
// lanes): ascending scan index
__global__ __launch_bounds__(64 * KW_WAVES) void kwindow_fill_kernel(long n, const float* __restrict__ xyz, const float* __restrict__ bounds,
                                                                     int nx, int ny, double block, double stride, long nchunks,
                                                                     const int* __restrict__ hist, const int* __restrict__ woff, long cap,
                                                                     int* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * KW_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const long p = c * 64 + lane;
  KWinMember m = {nx, -1, ny, -1};
  if (p < n) m = kwin_member(xyz + p * 3, bounds, nx, ny, block, stride);
  const KWinMember r = wave_rect(m);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = r.xlo; i <= r.xhi; ++i) {
    const bool fx = i >= m.xlo && i <= m.xhi;
    for (int j = r.ylo; j <= r.yhi; ++j) {
      const bool in = fx && j >= m.ylo && j <= m.yhi;
      const unsigned long long ballot = __ballot(in);
      if (in) {
        const size_t w = (size_t)i * ny + j;
        const int off = woff[w];
        const long pos = (long)off + hist[w * nchunks + c] + __popcll(ballot & below);
        if (off >= 0 && pos < cap) out_idx[pos] = (int)p;  // (the host sizes the lists from the counts: always taken)
      }
    }
  }
}

// ---- rows (D:334-351) and the rotation about z (T:160-161, provider.py:71-89): one thread per row entry
__global__ __launch_bounds__(256) void kwindow_gather_kernel(long entries, long real_entries, int block_points, const int* __restrict__ rowpos,
                                                             long cap, const int* __restrict__ cat_idx, long n, const float* __restrict__ xyz,
                                                             const float* __restrict__ remission, int nfeat,
                                                             const double* __restrict__ angles, float* __restrict__ out_data,
                                                             int* __restrict__ out_idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int width = 3 + nfeat;
  float* row = out_data + (size_t)e * width;
  const long pos = e < real_entries ? (long)rowpos[e] : -1;
  const long i = pos >= 0 && pos < cap ? (long)cat_idx[pos] : -1;
  if (i < 0 || i >= n) {  // a row past the scan's last one: zeros (an index outside the lists is never drawn)
    for (int f = 0; f < width; ++f) row[f] = 0.0f;
    out_idx[e] = 0;
    return;
  }
  float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1];
  if (angles) {  // [x y z] @ [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] in float64, stored as float32
    const double a = angles[e / block_points];
    const double cosval = cos(a), sinval = sin(a);
    const double xd = (double)x, yd = (double)y;
    x = (float)(xd * cosval + yd * -sinval);
    y = (float)(xd * sinval + yd * cosval);
  }
  row[0] = x;
  row[1] = y;
  row[2] = xyz[i * 3 + 2];
  if (nfeat) row[3] = remission[i];
  out_idx[e] = (int)i;
}

}  // namespace pasnl

using namespace pasnl;

// what the windows' positions must fit: w = i * ny + j and the launch of one workgroup per window
static inline bool kw_grid_ok(int nx, int ny) { return (long)nx * (long)ny <= (long)INT_MAX; }

extern "C" size_t pasnl_kwindow_hist_bytes(long n, int nx, int ny) {
  if (n <= 0 || nx <= 0 || ny <= 0 || !kw_grid_ok(nx, ny)) return 0;
  return (size_t)nx * (size_t)ny * (size_t)wt_chunks(n) * sizeof(int);
}

extern "C" int pasnl_kwindow_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, int* hist,
                                   int* out_counts, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && stride > 0.0, PASNL_EINVAL);
  PASNL_REQUIRE(kw_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = wt_chunks(n);
  if (hipMemsetAsync(hist, 0, pasnl_kwindow_hist_bytes(n, nx, ny), s) != hipSuccess) return PASNL_ELAUNCH;
  hipLaunchKernelGGL(kwindow_count_kernel, dim3(wt_blocks(nchunks, KW_WAVES)), dim3(64 * KW_WAVES), 0, s, n, xyz, bounds, nx, ny, block,
                     stride, nchunks, hist);
  hipLaunchKernelGGL(window_scan_kernel, dim3((unsigned)(nx * ny)), dim3(256), 0, s, nchunks, hist, out_counts);
  return pasnl_launch_status();
}

extern "C" int pasnl_kwindow_fill(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, const int* hist,
                                  const int* woff, long cap, int* out_idx, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && stride > 0.0 && cap > 0, PASNL_EINVAL);
  PASNL_REQUIRE(kw_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx, PASNL_ENULL);
  const long nchunks = wt_chunks(n);
  hipLaunchKernelGGL(kwindow_fill_kernel, dim3(wt_blocks(nchunks, KW_WAVES)), dim3(64 * KW_WAVES), 0, pasnl_hip_stream(stream), n, xyz,
                     bounds, nx, ny, block, stride, nchunks, hist, woff, cap, out_idx);
  return pasnl_launch_status();
}

extern "C" int pasnl_kwindow_gather(int rows, int real_rows, int block_points, const int* rowpos, long cap, const int* cat_idx, long n,
                                    const float* xyz, const float* remission, int nfeat, const double* angles, float* out_data,
                                    int* out_idx, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && real_rows >= 0 && real_rows <= rows && block_points > 0 && (nfeat == 0 || nfeat == 1) && n > 0 && cap > 0,
                PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(cat_idx && xyz && out_data && out_idx && (real_rows == 0 || rowpos) && (nfeat == 0 || remission), PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(kwindow_gather_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries,
                     (long)real_rows * block_points, block_points, rowpos, cap, cat_idx, n, xyz, remission, nfeat, angles, out_data, out_idx);
  return pasnl_launch_status();
}
