// SemanticKITTI's two training-time validation loops around the forward, on the device: reference
// SemanticKITTI/semantic_kitti_dataset.py (D) :68-109 `SemanticKittiDataset.__getitem__` (a block_size column round a drawn
// point, up to ten tries until 70 % of it is labelled, resampled to sample_points rows) and :164-211
// `SemanticKittiDataset_whole.__getitem__` (every non-empty column of a non-overlapping block_size grid, resampled likewise),
// SemanticKITTI/train_semantic_kitti.py (T) :267-328 `eval_one_epoch` and :331-418 `eval_whole_scene_one_epoch`, and
// utils/provider.py (P) :71-89 `rotate_point_cloud_z`.  The sibling of block_test.hip for lidar scans: the column's side and
// the mask's padding are parameters, there is no voxel key and no normalize_data, the weight is a float32 table looked up the
// reference's way, and the remission column is the reference's.  The count, scan and fill kernels and the crop box are
// window_scan.hpp's, the bounds pasnl_window_bounds and the score pasnl_block_score.  Everything that has to equal numpy is
// done in numpy's dtypes (the library builds with -ffp-contract=off); the contract is stated in include/pasnl.h per entry
// point and restated on the host in tests/kitti_block_flow_ref.py.
//
// What stays on the host: the numpy RNG stream (the centre of every try, the resampling choices, the rotation angles), the
// acceptance test of a try (one Python-float comparison on two integers) and the carry-over of rows between scans.
//   chopped: per try pasnl_kblock_crop_stats -> [two integers down]; then [choices up] -> pasnl_kblock_fill -> pasnl_kblock_gather
//   whole:   pasnl_kblock_grid_count -> [nx*ny counts down; choices up] -> pasnl_kblock_fill -> pasnl_kblock_gather
//   per batch, with no synchronisation: (chopped: pasnl_kblock_rotate ->) forward -> pasnl_block_score
#include <math.h>
#include "common.hpp"
#include "window_scan.hpp"

namespace pasnl {

constexpr int KB_CLASS_MAX = 256;  // classes of the weight table (pasnl_block_score's limit: the rows are scored by it)
constexpr double KB_OUTER = 0.2;   // the margin of membership (D:87, D:187)

// ---- the chopped column (D:82-86) is window_scan.hpp's CropBox round the centre with half = block_size / 2; the whole-scan
// grid (D:184-187) is its ColumnGrid with curmin = float64(coordmin) + i * block, curmax = float64(coordmin) + (i + 1) * block;
// the mask (D:95, D:193) is either's test with `padding`
static inline ColumnGrid kblock_grid(int nx, int ny, double block, double padding) { return {nx, ny, block, block, true, KB_OUTER, padding}; }

// One try, one wave per chunk: hist[c] = members, hist[nchunks + c] = members with label > 0 (two ballots, no atomics)
__global__ __launch_bounds__(64 * COL_WAVES) void kblock_crop_stats_kernel(long n, const float* __restrict__ xyz, const int* __restrict__ labels,
                                                                          const float* __restrict__ bounds, long centre, double half,
                                                                          long nchunks, int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * COL_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // whole waves leave
  const CropBox box = crop_box(xyz + centre * 3, bounds, half);
  const long p = c * 64 + lane;
  bool in = false, lab = false;
  if (p < n) {
    const double q[3] = {(double)xyz[p * 3], (double)xyz[p * 3 + 1], (double)xyz[p * 3 + 2]};
    in = crop_inside(box, q, KB_OUTER);
    lab = in && labels[p] > 0;
  }
  const unsigned long long bin = __ballot(in), blab = __ballot(lab);
  if (lane == 0) {
    hist[c] = __popcll(bin);
    hist[nchunks + c] = __popcll(blab);
  }
}

// ---- rows (D:100-107, D:195-203): one thread per row entry
__global__ __launch_bounds__(256) void kblock_gather_kernel(long entries, int block_points, const int* __restrict__ rowpos,
                                                            const int* __restrict__ rowbase, long cap, const int* __restrict__ cat_idx,
                                                            const unsigned char* __restrict__ cat_mask, long n, const float* __restrict__ xyz,
                                                            const float* __restrict__ remission, int nfeat, const int* __restrict__ labels, int c,
                                                            const float* __restrict__ lut, int quirks, float* __restrict__ out_data,
                                                            int* __restrict__ out_label, float* __restrict__ out_smpw) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int width = 3 + nfeat;
  float* row = out_data + (size_t)e * width;
  const long pos = rowpos[e];
  const long draw = pos - (long)rowbase[e / block_points];  // the raw rng.choice value
  const long i = pos >= 0 && pos < cap ? (long)cat_idx[pos] : -1;
  const int seg = i >= 0 && i < n ? labels[i] : -1;
  // quirks: label_weights = lut[label] is per POINT and is indexed by the label VALUE (D:77, D:104): the weight of the label
  // of scan point number seg; and the remission is that of scan point number `draw` (D:107).  (a position outside the lists
  // is never drawn, a label outside the table never stored, and the host refuses n <= max(label): then nothing is read)
  const long wsrc = quirks ? (long)seg : i;
  const long rsrc = quirks ? draw : i;
  const int wl = seg >= 0 && seg < c && wsrc >= 0 && wsrc < n ? labels[wsrc] : -1;
  if (wl < 0 || wl >= c || (nfeat && (rsrc < 0 || rsrc >= n))) {
    for (int f = 0; f < width; ++f) row[f] = 0.0f;
    out_label[e] = 0;
    out_smpw[e] = 0.0f;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) row[a] = xyz[i * 3 + a];
  if (nfeat) row[3] = remission[rsrc];
  out_label[e] = seg;
  out_smpw[e] = lut[wl] * (cat_mask[pos] ? 1.0f : 0.0f);  // sample_weight *= mask: float32 *= bool
}

// ---- P:71-89 as T:290 applies it: the float32 row widened, [x y z] @ [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] in float64,
// stored as float32; one thread per row entry (it reads its own entry before it writes it: src == batch is allowed)
__global__ __launch_bounds__(256) void kblock_rotate_kernel(long entries, int block_points, int width, const float* src,
                                                            const double* __restrict__ rot, float* batch) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const float* r = src + (size_t)e * width;
  float* o = batch + (size_t)e * width;
  const long k = e / block_points;
  const double cosval = rot[k * 2], sinval = rot[k * 2 + 1];
  const double x = (double)r[0], y = (double)r[1];
  const float ox = (float)(x * cosval + y * -sinval), oy = (float)(x * sinval + y * cosval);
  for (int f = width - 1; f >= 2; --f) o[f] = r[f];
  o[0] = ox;
  o[1] = oy;
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_kblock_crop_stats(long n, const float* xyz, const int* labels, const float* bounds, long centre, double half, int* hist,
                                       int* out_stats, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && centre >= 0 && centre < n && half >= 0.0 && half < INFINITY, PASNL_EINVAL);
  PASNL_REQUIRE(xyz && labels && bounds && hist && out_stats, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = wt_chunks(n);
  hipLaunchKernelGGL(kblock_crop_stats_kernel, dim3(wt_blocks(nchunks, COL_WAVES)), dim3(64 * COL_WAVES), 0, s, n, xyz, labels, bounds, centre,
                     half, nchunks, hist);
  hipLaunchKernelGGL(window_scan_kernel, dim3(2), dim3(256), 0, s, nchunks, hist, out_stats);
  return pasnl_launch_status();
}

extern "C" int pasnl_kblock_grid_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, int* hist, int* out_counts,
                                       pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && block < INFINITY, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  return wt_count(n, xyz, bounds, kblock_grid(nx, ny, block, 0.0), hist, out_counts, pasnl_hip_stream(stream));
}

extern "C" int pasnl_kblock_fill(long n, const float* xyz, const float* bounds, long centre, double half, int nx, int ny, double block,
                                 double padding, const int* hist, const int* woff, long cap, int* out_idx, unsigned char* out_mask,
                                 pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && cap > 0 && centre < n && padding == padding, PASNL_EINVAL);
  PASNL_REQUIRE(centre >= 0 ? (nx == 1 && ny == 1 && half >= 0.0 && half < INFINITY) : (block > 0.0 && block < INFINITY), PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx && out_mask, PASNL_ENULL);
  return wt_fill(n, xyz, bounds, kblock_grid(nx, ny, block, padding), centre, half, hist, woff, cap, out_idx, out_mask,
                 pasnl_hip_stream(stream));
}

extern "C" int pasnl_kblock_gather(int rows, int block_points, const int* rowpos, const int* rowbase, long cap, const int* cat_idx,
                                   const unsigned char* cat_mask, long n, const float* xyz, const float* remission, int nfeat,
                                   const int* labels, int c, const float* lut, int quirks, float* out_data, int* out_label, float* out_smpw,
                                   pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && (nfeat == 0 || nfeat == 1) && n > 0 && cap > 0 && c >= 1, PASNL_EINVAL);
  PASNL_REQUIRE(c <= KB_CLASS_MAX, PASNL_EUNSUPPORTED);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(rowpos && rowbase && cat_idx && cat_mask && xyz && labels && lut && out_data && out_label && out_smpw && (nfeat == 0 || remission),
                PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(kblock_gather_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, block_points, rowpos,
                     rowbase, cap, cat_idx, cat_mask, n, xyz, remission, nfeat, labels, c, lut, quirks, out_data, out_label, out_smpw);
  return pasnl_launch_status();
}

extern "C" int pasnl_kblock_rotate(int rows, int block_points, int width, const float* src, const double* rot, float* batch,
                                   pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && width >= 3, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(src && rot && batch, PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(kblock_rotate_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, block_points, width,
                     src, rot, batch);
  return pasnl_launch_status();
}
