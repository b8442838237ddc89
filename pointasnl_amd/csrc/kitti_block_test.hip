// SemanticKITTI's two training-time validation loops around the forward, on the device: reference
// SemanticKITTI/semantic_kitti_dataset.py (D) :68-109 `SemanticKittiDataset.__getitem__` (a block_size column round a drawn
// point, up to ten tries until 70 % of it is labelled, resampled to sample_points rows) and :164-211
// `SemanticKittiDataset_whole.__getitem__` (every non-empty column of a non-overlapping block_size grid, resampled likewise),
// SemanticKITTI/train_semantic_kitti.py (T) :267-328 `eval_one_epoch` and :331-418 `eval_whole_scene_one_epoch`, and
// utils/provider.py (P) :71-89 `rotate_point_cloud_z`.  The sibling of block_test.hip for lidar scans: the column's side and
// the mask's padding are parameters, there is no voxel key and no normalize_data, the grid has no limit per axis (a wave
// visits only the columns round its own points, as in kitti_window_test.hip), the weight is a float32 table looked up the
// reference's way, and the remission column is the reference's.  The scan kernel and the chunking are window_scan.hpp's, the
// bounds pasnl_window_bounds and the score pasnl_block_score.  Everything that has to equal numpy is done in numpy's dtypes
// (the library builds with -ffp-contract=off); the contract is stated in include/pasnl.h per entry point and restated on the
// host in tests/kitti_block_flow_ref.py.
//
// What stays on the host: the numpy RNG stream (the centre of every try, the resampling choices, the rotation angles), the
// acceptance test of a try (one Python-float comparison on two integers) and the carry-over of rows between scans.
//   chopped: per try pasnl_kblock_crop_stats -> [two integers down]; then [choices up] -> pasnl_kblock_fill -> pasnl_kblock_gather
//   whole:   pasnl_kblock_grid_count -> [nx*ny counts down; choices up] -> pasnl_kblock_fill -> pasnl_kblock_gather
//   per batch, with no synchronisation: (chopped: pasnl_kblock_rotate ->) forward -> pasnl_block_score
#include <limits.h>
#include <math.h>
#include "common.hpp"
#include "window_scan.hpp"

namespace pasnl {

constexpr int KB_WAVES = 4;        // chunks (of 64 consecutive points, one wave each) per workgroup
constexpr int KB_CLASS_MAX = 256;  // classes of the weight table (pasnl_block_score's limit: the rows are scored by it)
constexpr double KB_OUTER = 0.2;   // the margin of membership (D:87, D:187)

// ---- the chopped column (D:82-86): float64 bounds round the float32 centre, z from the float32 extent of the scan
struct KBox {
  double lo[3], hi[3];
};

__device__ __forceinline__ KBox kcrop_box(const float* __restrict__ centre, const float* __restrict__ b, double half) {
  KBox box;
  box.lo[0] = (double)centre[0] - half;  // curcenter - [block_size / 2, block_size / 2, 14]: float32 array - list -> float64
  box.hi[0] = (double)centre[0] + half;
  box.lo[1] = (double)centre[1] - half;
  box.hi[1] = (double)centre[1] + half;
  box.lo[2] = (double)b[2];  // curmin[2] = coordmin[2]; curmax[2] = coordmax[2]
  box.hi[2] = (double)b[5];
  return box;
}

__device__ __forceinline__ bool kbox_inside(const KBox& box, const double* p, double margin) {
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in = in && p[a] >= box.lo[a] - margin && p[a] <= box.hi[a] + margin;
  return in;
}

// One try, one wave per chunk: hist[c] = members, hist[nchunks + c] = members with label > 0 (two ballots, no atomics)
__global__ __launch_bounds__(64 * KB_WAVES) void kblock_crop_stats_kernel(long n, const float* __restrict__ xyz, const int* __restrict__ labels,
                                                                          const float* __restrict__ bounds, long centre, double half,
                                                                          long nchunks, int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * KB_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // whole waves leave
  const KBox box = kcrop_box(xyz + centre * 3, bounds, half);
  const long p = c * 64 + lane;
  bool in = false, lab = false;
  if (p < n) {
    const double q[3] = {(double)xyz[p * 3], (double)xyz[p * 3 + 1], (double)xyz[p * 3 + 2]};
    in = kbox_inside(box, q, KB_OUTER);
    lab = in && labels[p] > 0;
  }
  const unsigned long long bin = __ballot(in), blab = __ballot(lab);
  if (lane == 0) {
    hist[c] = __popcll(bin);
    hist[nchunks + c] = __popcll(blab);
  }
}

// ---- the whole-scan grid (D:184-187): curmin = float64(coordmin) + i * block, curmax = float64(coordmin) + (i + 1) * block
// -- NOT curmin + block.  The columns of one axis that hold coordinate p: lo..hi, none when hi < lo; every column of the axis
// is tested with the reference's own comparison, no index is derived from a division.  Both bounds are monotone in i, so the
// members are one contiguous range (window_scan.hpp's KWinMember; wave_rect is the wave's rectangle of them).
__device__ __forceinline__ void kgrid_axis_range(double p, double origin, int count, double block, int& lo, int& hi) {
  lo = count;
  hi = -1;
  for (int i = 0; i < count; ++i) {
    const double curmin = origin + (double)i * block;
    const double curmax = origin + (double)(i + 1) * block;
    if (p >= curmin - KB_OUTER && p <= curmax + KB_OUTER) {
      lo = i < lo ? i : lo;
      hi = i;
    }
  }
}

__device__ __forceinline__ double kgrid_zmax(const float* __restrict__ b) {
  return (double)b[2] + (double)(b[5] - b[2]);  // coordmin + [.., .., coordmax[2] - coordmin[2]]: a float32 difference
}

__device__ __forceinline__ KWinMember kgrid_member(const float* __restrict__ p, const float* __restrict__ b, int nx, int ny, double block) {
  KWinMember m;
  kgrid_axis_range((double)p[0], (double)b[0], nx, block, m.xlo, m.xhi);
  kgrid_axis_range((double)p[1], (double)b[1], ny, block, m.ylo, m.yhi);
  const double pz = (double)p[2];
  const double zmin = (double)b[2] + 0.0;
  const bool z = pz >= zmin - KB_OUTER && pz <= kgrid_zmax(b) + KB_OUTER;
  if (!z || m.yhi < m.ylo || m.xhi < m.xlo) m = {nx, -1, ny, -1};
  return m;
}

// the mask of D:193 for column (i, j): the same test with `padding`
__device__ __forceinline__ bool kgrid_mask(const float* __restrict__ p, const float* __restrict__ b, int i, int j, double block, double padding) {
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  const double xmin = (double)b[0] + (double)i * block, xmax = (double)b[0] + (double)(i + 1) * block;
  const double ymin = (double)b[1] + (double)j * block, ymax = (double)b[1] + (double)(j + 1) * block;
  const double zmin = (double)b[2] + 0.0, zmax = kgrid_zmax(b);
  return px >= xmin - padding && px <= xmax + padding && py >= ymin - padding && py <= ymax + padding && pz >= zmin - padding &&
         pz <= zmax + padding;
}

// whole scan, pass 1: hist[w][chunk] = members of column w among the chunk's 64 points (a ballot: no atomics at all).  hist
// is cleared beforehand: a wave stores only for the columns that hold one of its points.
__global__ __launch_bounds__(64 * KB_WAVES) void kblock_grid_count_kernel(long n, const float* __restrict__ xyz, const float* __restrict__ bounds,
                                                                          int nx, int ny, double block, long nchunks, int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * KB_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const long p = c * 64 + lane;
  KWinMember m = {nx, -1, ny, -1};
  if (p < n) m = kgrid_member(xyz + p * 3, bounds, nx, ny, block);
  const KWinMember r = wave_rect(m);
  for (int i = r.xlo; i <= r.xhi; ++i) {
    const bool fx = i >= m.xlo && i <= m.xhi;
    for (int j = r.ylo; j <= r.yhi; ++j) {
      const unsigned long long ballot = __ballot(fx && j >= m.ylo && j <= m.yhi);
      if (ballot != 0ull && lane == 0) hist[((size_t)i * ny + j) * nchunks + c] = __popcll(ballot);
    }
  }
}

// both loops, the last pass: a member's place is woff[w] + (members in earlier chunks) + (members among the lower lanes):
// ascending scan index.  centre >= 0: the chopped column round that point (nx = ny = 1); centre < 0: the grid.
__global__ __launch_bounds__(64 * KB_WAVES) void kblock_fill_kernel(long n, const float* __restrict__ xyz, const float* __restrict__ bounds,
                                                                    long centre, double half, int nx, int ny, double block, double padding,
                                                                    long nchunks, const int* __restrict__ hist, const int* __restrict__ woff,
                                                                    long cap, int* __restrict__ out_idx, unsigned char* __restrict__ out_mask) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * KB_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const long p = c * 64 + lane;
  const bool crop = centre >= 0;
  KWinMember m = {nx, -1, ny, -1};
  bool crop_mask = false;
  if (p < n) {
    if (crop) {
      const KBox box = kcrop_box(xyz + centre * 3, bounds, half);
      const double q[3] = {(double)xyz[p * 3], (double)xyz[p * 3 + 1], (double)xyz[p * 3 + 2]};
      if (kbox_inside(box, q, KB_OUTER)) m = {0, 0, 0, 0};
      crop_mask = kbox_inside(box, q, padding);
    } else {
      m = kgrid_member(xyz + p * 3, bounds, nx, ny, block);
    }
  }
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
        if (off >= 0 && pos < cap) {  // (the host sizes the lists from the counts: always taken for a listed column)
          out_idx[pos] = (int)p;
          out_mask[pos] = (crop ? crop_mask : kgrid_mask(xyz + p * 3, bounds, i, j, block, padding)) ? 1 : 0;
        }
      }
    }
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

// what the columns' positions must fit: w = i * ny + j and the launch of one workgroup per column
static inline bool kb_grid_ok(int nx, int ny) { return (long)nx * (long)ny <= (long)INT_MAX; }

extern "C" int pasnl_kblock_crop_stats(long n, const float* xyz, const int* labels, const float* bounds, long centre, double half, int* hist,
                                       int* out_stats, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && centre >= 0 && centre < n && half >= 0.0 && half < INFINITY, PASNL_EINVAL);
  PASNL_REQUIRE(xyz && labels && bounds && hist && out_stats, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = wt_chunks(n);
  hipLaunchKernelGGL(kblock_crop_stats_kernel, dim3(wt_blocks(nchunks, KB_WAVES)), dim3(64 * KB_WAVES), 0, s, n, xyz, labels, bounds, centre,
                     half, nchunks, hist);
  hipLaunchKernelGGL(window_scan_kernel, dim3(2), dim3(256), 0, s, nchunks, hist, out_stats);
  return pasnl_launch_status();
}

extern "C" int pasnl_kblock_grid_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, int* hist, int* out_counts,
                                       pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && block > 0.0 && block < INFINITY, PASNL_EINVAL);
  PASNL_REQUIRE(kb_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = wt_chunks(n);
  if (hipMemsetAsync(hist, 0, (size_t)nx * (size_t)ny * (size_t)nchunks * sizeof(int), s) != hipSuccess) return PASNL_ELAUNCH;
  hipLaunchKernelGGL(kblock_grid_count_kernel, dim3(wt_blocks(nchunks, KB_WAVES)), dim3(64 * KB_WAVES), 0, s, n, xyz, bounds, nx, ny, block,
                     nchunks, hist);
  hipLaunchKernelGGL(window_scan_kernel, dim3((unsigned)(nx * ny)), dim3(256), 0, s, nchunks, hist, out_counts);
  return pasnl_launch_status();
}

extern "C" int pasnl_kblock_fill(long n, const float* xyz, const float* bounds, long centre, double half, int nx, int ny, double block,
                                 double padding, const int* hist, const int* woff, long cap, int* out_idx, unsigned char* out_mask,
                                 pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && cap > 0 && centre < n && padding == padding, PASNL_EINVAL);
  PASNL_REQUIRE(centre >= 0 ? (nx == 1 && ny == 1 && half >= 0.0 && half < INFINITY) : (block > 0.0 && block < INFINITY), PASNL_EINVAL);
  PASNL_REQUIRE(kb_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx && out_mask, PASNL_ENULL);
  const long nchunks = wt_chunks(n);
  hipLaunchKernelGGL(kblock_fill_kernel, dim3(wt_blocks(nchunks, KB_WAVES)), dim3(64 * KB_WAVES), 0, pasnl_hip_stream(stream), n, xyz, bounds,
                     centre, half, nx, ny, block, padding, nchunks, hist, woff, cap, out_idx, out_mask);
  return pasnl_launch_status();
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
