// What the four block and window test loops share (window_test.hip, block_test.hip: ScanNet; kitti_window_test.hip,
// kitti_block_test.hip: SemanticKITTI).  Each cuts a cloud into a grid of overlapping x/y columns and lists every column's
// members in ascending index order: the cloud goes in chunks of 64 consecutive points, one wave each;
//   pass 1 (column_count_kernel)  hist[w][chunk] = members of column w in the chunk, by ballot (no atomics at all)
//   pass 2 (window_scan_kernel)   per column an exclusive scan over the chunks, in place; counts[w] = the column's size
//   pass 3 (column_fill_kernel)   a member's place is woff[w] + (members in earlier chunks) + (members among the lower lanes)
// The loops differ in the ColumnGrid their C wrappers fill in, and in nothing else.
//
// A point's columns along one axis are a range lo..hi, and a wave visits only the rectangle round its own points.  The
// range is exact, not a bound: curmin_i = fl(origin + fl(i * stride)) is monotone non-decreasing in i, and so is either form
// of curmax_i, fl(curmin_i + side) or fl(origin + fl((i + 1) * side)), because rounding is monotone and so a sum or product of
// rounded non-decreasing terms is non-decreasing; subtracting or adding the margin keeps that.  So p >= curmin_i - m holds
// on a prefix of i and p <= curmax_i + m on a suffix: the members of an axis are contiguous, and the hull axis_range returns
// is the member set itself.  The mask is evaluated per (i, j) directly and needs no such argument.
#pragma once
#include <limits.h>
#include "common.hpp"

namespace pasnl {

constexpr int COL_WAVES = 4;  // chunks (of 64 consecutive points, one wave each) per workgroup

struct ColumnGrid {
  int nx, ny;
  double stride, side;  // curmin_i = float64(coordmin) + i * stride
  bool tiled;           // curmax_i = float64(coordmin) + (i + 1) * side (the two grids: NOT curmin_i + side, which rounds
                        // differently) or curmin_i + side (the two sliding windows)
  double outer, inner;  // the margin of membership, and of the mask (unused where no mask is written)
};

// The reference's own comparison for column i of one axis: the float32 coordinate, widened, against the float64 bounds
__device__ __forceinline__ bool axis_holds(const ColumnGrid& g, double p, double origin, int i, double margin) {
  const double curmin = origin + (double)i * g.stride;
  const double curmax = g.tiled ? origin + (double)(i + 1) * g.side : curmin + g.side;
  return p >= curmin - margin && p <= curmax + margin;
}

// z: curmin = coordmin_z + 0, curmax = curmin + float64(float32(coordmax_z - coordmin_z))
__device__ __forceinline__ bool z_holds(double pz, const float* __restrict__ b, double margin) {
  const double zmin = (double)b[2] + 0.0;
  const double zmax = zmin + (double)(b[5] - b[2]);
  return pz >= zmin - margin && pz <= zmax + margin;
}

// The columns of one axis that hold coordinate p: lo..hi, none when hi < lo.  Every column of the axis is tested, no index
// is derived from a division.
__device__ __forceinline__ void axis_range(const ColumnGrid& g, double p, double origin, int count, int& lo, int& hi) {
  lo = count;
  hi = -1;
  for (int i = 0; i < count; ++i) {
    if (axis_holds(g, p, origin, i, g.outer)) {
      lo = i < lo ? i : lo;
      hi = i;
    }
  }
}

struct KWinMember {
  int xlo, xhi, ylo, yhi;  // an empty range on either axis, or z outside: xhi < xlo
};

__device__ __forceinline__ KWinMember column_member(const ColumnGrid& g, const float* __restrict__ p, const float* __restrict__ b) {
  KWinMember m;
  axis_range(g, (double)p[0], (double)b[0], g.nx, m.xlo, m.xhi);
  axis_range(g, (double)p[1], (double)b[1], g.ny, m.ylo, m.yhi);
  if (!z_holds((double)p[2], b, g.outer) || m.yhi < m.ylo || m.xhi < m.xlo) m = {g.nx, -1, g.ny, -1};
  return m;
}

// the mask for column (i, j): the same test with the inner margin
__device__ __forceinline__ bool column_mask(const ColumnGrid& g, const float* __restrict__ p, const float* __restrict__ b, int i, int j) {
  return axis_holds(g, (double)p[0], (double)b[0], i, g.inner) && axis_holds(g, (double)p[1], (double)b[1], j, g.inner) &&
         z_holds((double)p[2], b, g.inner);
}

// the rectangle of columns that holds every membership of the wave's 64 points (empty: xhi < xlo): uniform over the wave
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

// ---- the chopped column of the two block loops: float64 bounds round the float32 centre, z from the float32 extent
struct CropBox {
  double lo[3], hi[3];
};

__device__ __forceinline__ CropBox crop_box(const float* __restrict__ centre, const float* __restrict__ b, double half) {
  CropBox box;
  box.lo[0] = (double)centre[0] - half;  // curcenter - [half, half, ..]: float32 array - list -> float64
  box.hi[0] = (double)centre[0] + half;
  box.lo[1] = (double)centre[1] - half;
  box.hi[1] = (double)centre[1] + half;
  box.lo[2] = (double)b[2];  // curmin[2] = coordmin[2]; curmax[2] = coordmax[2]
  box.hi[2] = (double)b[5];
  return box;
}

__device__ __forceinline__ bool crop_inside(const CropBox& box, const double* p, double margin) {
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in = in && p[a] >= box.lo[a] - margin && p[a] <= box.hi[a] + margin;
  return in;
}

// What a wave lists: the chopped column round point `centre` as the single column 0 (centre >= 0: member inside the outer
// margin of the box, mask inside the inner one), or the grid's columns (centre < 0)
__device__ __forceinline__ KWinMember listed_member(const ColumnGrid& g, long centre, double half, const float* __restrict__ xyz, long p,
                                                    const float* __restrict__ b, bool& crop_mask) {
  if (centre < 0) return column_member(g, xyz + p * 3, b);
  const CropBox box = crop_box(xyz + centre * 3, b, half);
  const double q[3] = {(double)xyz[p * 3], (double)xyz[p * 3 + 1], (double)xyz[p * 3 + 2]};
  crop_mask = crop_inside(box, q, g.inner);
  if (crop_inside(box, q, g.outer)) return {0, 0, 0, 0};
  return {g.nx, -1, g.ny, -1};
}

// pass 1.  hist is cleared beforehand: a wave stores only for the columns that hold one of its points.
static __global__ __launch_bounds__(64 * COL_WAVES) void column_count_kernel(long n, const float* __restrict__ xyz,
                                                                             const float* __restrict__ bounds, ColumnGrid g, long nchunks,
                                                                             int* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * COL_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // whole waves leave
  const long p = c * 64 + lane;
  KWinMember m = {g.nx, -1, g.ny, -1};
  if (p < n) m = column_member(g, xyz + p * 3, bounds);
  const KWinMember r = wave_rect(m);
  for (int i = r.xlo; i <= r.xhi; ++i) {
    const bool fx = i >= m.xlo && i <= m.xhi;
    for (int j = r.ylo; j <= r.yhi; ++j) {
      const unsigned long long ballot = __ballot(fx && j >= m.ylo && j <= m.yhi);
      if (ballot != 0ull && lane == 0) hist[((size_t)i * g.ny + j) * nchunks + c] = __popcll(ballot);
    }
  }
}

// pass 2 for one row of per-chunk counts, by one workgroup of 256: an exclusive scan in place -> the row's total (every
// thread's).  wsum: 4 ints of LDS.
__device__ __forceinline__ int chunk_scan_exclusive(int* __restrict__ row, long nchunks, int* wsum) {
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
  return carry;
}

static __global__ __launch_bounds__(256) void window_scan_kernel(long nchunks, int* __restrict__ hist, int* __restrict__ counts) {
  __shared__ int wsum[4];
  const int total = chunk_scan_exclusive(hist + (size_t)blockIdx.x * nchunks, nchunks, wsum);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// pass 3: ascending index within every column.  out_mask may be null: then no mask is written.
static __global__ __launch_bounds__(64 * COL_WAVES) void column_fill_kernel(long n, const float* __restrict__ xyz,
                                                                            const float* __restrict__ bounds, ColumnGrid g, long centre,
                                                                            double half, long nchunks, const int* __restrict__ hist,
                                                                            const int* __restrict__ woff, long cap, int* __restrict__ out_idx,
                                                                            unsigned char* __restrict__ out_mask) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * COL_WAVES + (threadIdx.x >> 6);
  if (c >= nchunks) return;
  const long p = c * 64 + lane;
  KWinMember m = {g.nx, -1, g.ny, -1};
  bool crop_mask = false;
  if (p < n) m = listed_member(g, centre, half, xyz, p, bounds, crop_mask);
  const KWinMember r = wave_rect(m);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = r.xlo; i <= r.xhi; ++i) {
    const bool fx = i >= m.xlo && i <= m.xhi;
    for (int j = r.ylo; j <= r.yhi; ++j) {
      const bool in = fx && j >= m.ylo && j <= m.yhi;
      const unsigned long long ballot = __ballot(in);
      if (in) {
        const size_t w = (size_t)i * g.ny + j;
        const int off = woff[w];
        const long pos = (long)off + hist[w * nchunks + c] + __popcll(ballot & below);
        if (off >= 0 && pos < cap) {  // (the host sizes the lists from the counts: always taken for a listed column)
          out_idx[pos] = (int)p;
          if (out_mask) out_mask[pos] = (centre >= 0 ? crop_mask : column_mask(g, xyz + p * 3, bounds, i, j)) ? 1 : 0;
        }
      }
    }
  }
}

}  // namespace pasnl

static inline unsigned wt_blocks(long n, int t) { return (unsigned)((n + t - 1) / t); }
static inline long wt_chunks(long n) { return (n + 63) / 64; }

// what the columns' positions must fit: w = i * ny + j and the launch of one workgroup per column
static inline bool wt_grid_ok(int nx, int ny) { return (long)nx * (long)ny <= (long)INT_MAX; }

static inline size_t wt_hist_bytes(long n, int nx, int ny) {
  if (n <= 0 || nx <= 0 || ny <= 0 || !wt_grid_ok(nx, ny)) return 0;
  return (size_t)nx * (size_t)ny * (size_t)wt_chunks(n) * sizeof(int);
}

// passes 1 and 2 for a checked grid -> the scanned hist and the columns' counts
static inline int wt_count(long n, const float* xyz, const float* bounds, const pasnl::ColumnGrid& g, int* hist, int* out_counts,
                           hipStream_t s) {
  const long nchunks = wt_chunks(n);
  if (hipMemsetAsync(hist, 0, wt_hist_bytes(n, g.nx, g.ny), s) != hipSuccess) return PASNL_ELAUNCH;
  hipLaunchKernelGGL(pasnl::column_count_kernel, dim3(wt_blocks(nchunks, pasnl::COL_WAVES)), dim3(64 * pasnl::COL_WAVES), 0, s, n, xyz,
                     bounds, g, nchunks, hist);
  hipLaunchKernelGGL(pasnl::window_scan_kernel, dim3((unsigned)(g.nx * g.ny)), dim3(256), 0, s, nchunks, hist, out_counts);
  return pasnl_launch_status();
}

// pass 3 for a checked grid
static inline int wt_fill(long n, const float* xyz, const float* bounds, const pasnl::ColumnGrid& g, long centre, double half,
                          const int* hist, const int* woff, long cap, int* out_idx, unsigned char* out_mask, hipStream_t s) {
  const long nchunks = wt_chunks(n);
  hipLaunchKernelGGL(pasnl::column_fill_kernel, dim3(wt_blocks(nchunks, pasnl::COL_WAVES)), dim3(64 * pasnl::COL_WAVES), 0, s, n, xyz,
                     bounds, g, centre, half, nchunks, hist, woff, cap, out_idx, out_mask);
  return pasnl_launch_status();
}
