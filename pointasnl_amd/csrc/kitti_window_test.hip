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
#include <math.h>
#include "common.hpp"
#include "window_scan.hpp"

namespace pasnl {

// windows (D:296-301): curmin = float64(coordmin) + i * stride, curmax = curmin + block, membership inside 0.2, no mask --
// window_scan.hpp's three passes over this grid
static inline ColumnGrid kwindow_grid(int nx, int ny, double block, double stride) { return {nx, ny, stride, block, false, 0.2, 0.0}; }

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

extern "C" size_t pasnl_kwindow_hist_bytes(long n, int nx, int ny) { return wt_hist_bytes(n, nx, ny); }

extern "C" int pasnl_kwindow_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, int* hist,
                                   int* out_counts, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && stride > 0.0, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  return wt_count(n, xyz, bounds, kwindow_grid(nx, ny, block, stride), hist, out_counts, pasnl_hip_stream(stream));
}

extern "C" int pasnl_kwindow_fill(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, const int* hist,
                                  const int* woff, long cap, int* out_idx, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && stride > 0.0 && cap > 0, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx, PASNL_ENULL);
  return wt_fill(n, xyz, bounds, kwindow_grid(nx, ny, block, stride), -1, 0.0, hist, woff, cap, out_idx, nullptr, pasnl_hip_stream(stream));
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
