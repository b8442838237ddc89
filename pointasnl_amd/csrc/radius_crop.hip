// The radius form of the grid crops (`in_radius > 0`): reference ScanNet/scannet_dataset_grid.py (D) :491-492
// `input_trees[split][cloud_ind].query_radius(pick_point, r=config.in_radius)[0]` and
// SemanticKITTI/semantic_kitti_dataset_grid.py (K) :268-269 `search_tree.query_radius(center_point, r=in_radius)[0]`, and the
// lines that turn the member list into a crop (D:500-501, 519-539 with data_rep D:692-703; K:274-283).
//
// sklearn's query_radius returns exactly the points with ((dx*dx)+(dy*dy))+(dz*dz) <= r*r in float64 (dx = float64(x) - c),
// listed in the positional order of the tree's idx_array (a depth-first traversal, left before right).  The crop shuffles
// POSITIONS of that list, so the order decides which points a crop holds: `order` is that idx_array, flat beside the flat
// points, and the member list comes out in its order.  The method is window_scan.hpp's: the positions go in chunks of 64,
// one wave each;
//   count  hist[crop][chunk] = members among the chunk's 64 positions, by ballot
//   scan   per crop an exclusive scan over its chunks, in place; out_count[crop] = the total
//   fill   a member's place is (members in earlier chunks) + (members among the lower lanes)
// No atomics: the list is deterministic.  Three launches, no host synchronisation; the caller reads out_count back to draw
// the shuffle (its length is the count), then the gather applies it.
#include <math.h>
#include <type_traits>
#include "common.hpp"
#include "window_scan.hpp"

namespace pasnl {

// position p of crop's scan -> (in-scan index, member?).  A NaN coordinate fails the comparison: not a member.  An order
// entry outside the scan (the callers check their permutations) is no member either, so nothing is read out of bounds.
template <class D>
__device__ __forceinline__ bool rc_member(const D& d, const float* __restrict__ points, const int* __restrict__ order, long p,
                                          double r2, int& index) {
  index = -1;
  if (p >= (long)d.n) return false;
  const int i = order ? order[(size_t)d.offset + p] : (int)p;
  if (i < 0 || i >= d.n) return false;
  index = i;
  const float* q = points + ((size_t)d.offset + (size_t)i) * 3;
  const double dx = (double)q[0] - (double)d.cx, dy = (double)q[1] - (double)d.cy, dz = (double)q[2] - (double)d.cz;
  const double d2 = (dx * dx + dy * dy) + dz * dz;  // sklearn's rdist on its float64 copy (-ffp-contract=off)
  return d2 <= r2;
}

// count: grid = (blocks of COL_WAVES chunks of the largest scan, b)
template <class D>
__global__ __launch_bounds__(64 * COL_WAVES) void radius_count_kernel(long nchunks_max, const float* __restrict__ points,
                                                                      const D* __restrict__ desc, double r2,
                                                                      const int* __restrict__ order, int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long chunk = (long)blockIdx.x * COL_WAVES + (threadIdx.x >> 6);
  const D d = desc[blockIdx.y];
  if (chunk >= nchunks_max || chunk * 64 >= (long)d.n) return;  // whole waves leave: past this crop's own scan
  int index;
  const unsigned long long ballot = __ballot(rc_member(d, points, order, chunk * 64 + lane, r2, index));
  if (lane == 0) hist[(size_t)blockIdx.y * nchunks_max + chunk] = __popcll(ballot);
}

// scan: grid = b
template <class D>
__global__ __launch_bounds__(256) void radius_scan_kernel(long nchunks_max, const D* __restrict__ desc, int* __restrict__ hist,
                                                          int* __restrict__ out_count) {
  __shared__ int wsum[4];
  const long n = (long)desc[blockIdx.x].n;
  long nchunks = n > 0 ? (n + 63) / 64 : 0;  // the chunks the count kernel wrote
  nchunks = nchunks < nchunks_max ? nchunks : nchunks_max;
  const int total = chunk_scan_exclusive(hist + (size_t)blockIdx.x * nchunks_max, nchunks, wsum);
  if (threadIdx.x == 0) out_count[blockIdx.x] = total;
}

// fill: the count kernel's grid
template <class D>
__global__ __launch_bounds__(64 * COL_WAVES) void radius_fill_kernel(long nchunks_max, const float* __restrict__ points,
                                                                     const D* __restrict__ desc, double r2,
                                                                     const int* __restrict__ order, const int* __restrict__ hist,
                                                                     int* __restrict__ out_members, long member_stride) {
  const int lane = threadIdx.x & 63;
  const long chunk = (long)blockIdx.x * COL_WAVES + (threadIdx.x >> 6);
  const D d = desc[blockIdx.y];
  if (chunk >= nchunks_max || chunk * 64 >= (long)d.n) return;
  int index;
  const bool in = rc_member(d, points, order, chunk * 64 + lane, r2, index);
  const unsigned long long ballot = __ballot(in);
  if (in) {
    const long pos = (long)hist[(size_t)blockIdx.y * nchunks_max + chunk] + __popcll(ballot & ((1ull << lane) - 1ull));
    if (pos < member_stride) out_members[(size_t)blockIdx.y * member_stride + pos] = index;  // (member_stride >= n: always)
  }
}

// gather: grid = (blocks of 256 rows, b).  SCENE: rows relative to the float64 centre, colours, abs_coords
// (pasnl_scene_order_gather's contract); otherwise the scan's points as they are (pasnl_crop_order_permute's).
template <class D>
__global__ __launch_bounds__(256) void radius_gather_kernel(const D* __restrict__ desc, const float* __restrict__ points,
                                                            const float* __restrict__ colors, int nfeat,
                                                            const int* __restrict__ members, long member_stride,
                                                            const int* __restrict__ count, const int* __restrict__ perm,
                                                            int num_point, int abs_coords, int* __restrict__ out_select,
                                                            float* __restrict__ out_rows) {
  constexpr bool SCENE = std::is_same<D, pasnl_scene_crop_t>::value;
  const int c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= num_point) return;
  const D d = desc[c];
  long m = (long)count[c];
  m = m < member_stride ? m : member_stride;
  const int q = perm[(size_t)c * num_point + j];
  if (q < 0 || (long)q >= m) return;  // the row and its select entry stay as they were
  const int sel = members[(size_t)c * member_stride + q];
  if (sel < 0 || sel >= d.n) return;
  out_select[(size_t)c * num_point + j] = sel;
  const float* sp = points + ((size_t)d.offset + (size_t)sel) * 3;
  if constexpr (SCENE) {
    const int width = 3 + nfeat + (abs_coords ? 3 : 0);
    float* row = out_rows + ((size_t)c * num_point + j) * width;
    const double ctr[3] = {(double)d.cx, (double)d.cy, (double)d.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = (float)((double)sp[a] - ctr[a]);                   // (points[input_inds] - pick_point).astype(float32)
      row[a] = x;
      if (abs_coords) row[3 + nfeat + a] = (float)((double)x + ctr[a]);  // float32(input_points + pick_point), D:539
    }
    const float* sc = colors + ((size_t)d.offset + (size_t)sel) * nfeat;
    for (int f = 0; f < nfeat; ++f) row[3 + f] = sc[f];
  } else {
    float* row = out_rows + ((size_t)c * num_point + j) * 3;
    row[0] = sp[0]; row[1] = sp[1]; row[2] = sp[2];
  }
}

static inline long rc_chunks(long n) { return (n + 63) / 64; }

template <class D>
static int rc_members(int b, long nmax, const float* points, const D* desc, double radius, const int* order, int* out_members,
                      long member_stride, int* out_count, void* workspace, size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(b > 0 && b <= 65535 && nmax > 0 && nmax < (1l << 31) && member_stride >= nmax, PASNL_EINVAL);
  PASNL_REQUIRE(radius > 0.0, PASNL_EINVAL);  // (false for a NaN radius too)
  PASNL_REQUIRE(points && desc && out_members && out_count && workspace, PASNL_ENULL);
  PASNL_REQUIRE(workspace_bytes >= pasnl_scan_radius_workspace_bytes(b, nmax), PASNL_EWORKSPACE);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = rc_chunks(nmax);
  const double r2 = radius * radius;  // sklearn: the reduced radius r*r in double, inclusive
  int* hist = static_cast<int*>(workspace);
  const dim3 grid((unsigned)((nchunks + COL_WAVES - 1) / COL_WAVES), (unsigned)b);
  hipLaunchKernelGGL(radius_count_kernel<D>, grid, dim3(64 * COL_WAVES), 0, s, nchunks, points, desc, r2, order, hist);
  hipLaunchKernelGGL(radius_scan_kernel<D>, dim3(b), dim3(256), 0, s, nchunks, desc, hist, out_count);
  hipLaunchKernelGGL(radius_fill_kernel<D>, grid, dim3(64 * COL_WAVES), 0, s, nchunks, points, desc, r2, order, hist, out_members,
                     member_stride);
  return pasnl_launch_status();
}

template <class D>
static int rc_gather(int b, const D* desc, const float* points, const float* colors, int nfeat, const int* members,
                     long member_stride, const int* count, const int* perm, int num_point, int abs_coords, int* out_select,
                     float* out_rows, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && b <= 65535 && num_point > 0 && member_stride > 0 && nfeat >= 0, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(desc && points && members && count && perm && out_select && out_rows && (nfeat == 0 || colors), PASNL_ENULL);
  hipLaunchKernelGGL(radius_gather_kernel<D>, dim3((unsigned)((num_point + 255) / 256), (unsigned)b), dim3(256), 0,
                     pasnl_hip_stream(stream), desc, points, nfeat > 0 ? colors : nullptr, nfeat, members, member_stride, count, perm,
                     num_point, abs_coords, out_select, out_rows);
  return pasnl_launch_status();
}

}  // namespace pasnl

using namespace pasnl;

extern "C" size_t pasnl_scan_radius_workspace_bytes(int b, long nmax) {
  if (b <= 0 || nmax <= 0) return 0;
  return (size_t)b * (size_t)rc_chunks(nmax) * sizeof(int);
}

extern "C" int pasnl_scan_radius_members(int b, long nmax, const float* points, const pasnl_scan_crop_t* desc, double radius,
                                         const int* order, int* out_members, long member_stride, int* out_count, void* workspace,
                                         size_t workspace_bytes, pasnl_stream_t stream) {
  return rc_members(b, nmax, points, desc, radius, order, out_members, member_stride, out_count, workspace, workspace_bytes, stream);
}

extern "C" int pasnl_scene_radius_members(int b, long nmax, const float* points, const pasnl_scene_crop_t* desc, double radius,
                                          const int* order, int* out_members, long member_stride, int* out_count, void* workspace,
                                          size_t workspace_bytes, pasnl_stream_t stream) {
  return rc_members(b, nmax, points, desc, radius, order, out_members, member_stride, out_count, workspace, workspace_bytes, stream);
}

extern "C" int pasnl_scan_radius_gather(int b, const pasnl_scan_crop_t* desc, const float* points, const int* members,
                                        long member_stride, const int* count, const int* perm, int num_point, int* out_select,
                                        float* out_points, pasnl_stream_t stream) {
  return rc_gather(b, desc, points, nullptr, 0, members, member_stride, count, perm, num_point, 0, out_select, out_points, stream);
}

extern "C" int pasnl_scene_radius_gather(int b, const pasnl_scene_crop_t* desc, const float* points, const float* colors, int nfeat,
                                         const int* members, long member_stride, const int* count, const int* perm, int num_point,
                                         int abs_coords, int* out_select, float* out_input, pasnl_stream_t stream) {
  return rc_gather(b, desc, points, colors, nfeat, members, member_stride, count, perm, num_point, abs_coords, out_select, out_input,
                   stream);
}
