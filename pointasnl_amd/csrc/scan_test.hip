// The SemanticKITTI test loop around the forward, on the device: reference SemanticKITTI/semantic_kitti_dataset_grid.py
// (D) :192-245 `get_batch_gen('test')` -- pick the least-visited point, crop around it, raise the possibility of what the
// crop covered -- and test_semantic_kitti_grid.py (T) :147-180 -- smooth the votes into a float16 table, reproject onto
// the raw scan, write labels.  Everything that has to equal numpy is done in numpy's dtypes and order (the library builds
// with -ffp-contract=off); the exactness contract is stated in include/pasnl.h per entry point and restated on the host in
// tests/scan_flow_ref.py.
//
// One crop is a chain on ONE stream:  pick -> pasnl_knn_crop_indirect (crop.hip) -> order/permute -> update (3 launches).
// The crop descriptor (pasnl_scan_crop_t) carries the pick from kernel to kernel, so the host never reads anything back
// inside an epoch and the chain is capturable.  The RNG draws of crop_pc (buffer, shuffle) depend only on lengths the host
// knows and are drawn there, in the reference's order.
//
// Last-write-wins (numpy fancy-index assignment with repeated indices): `win` holds, per point of the scan, the largest
// crop row j that names it (vector atomic max); the row whose j is stored writes and resets the entry to -1.  A row that
// does not win reads either the winner's j or -1, never its own, so no ordering between rows is needed and the scratch is
// all -1 again at the end of the launch.
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"

namespace pasnl {

static_assert(sizeof(pasnl_scan_crop_t) == 40, "the descriptor layout is part of the ABI (scan_tester.DESC_BYTES)");

__global__ __launch_bounds__(ST_THREADS) void scan_pick_kernel(int s, const long long* __restrict__ offsets,
                                                               const double* __restrict__ possibility,
                                                               const double* __restrict__ min_possibility,
                                                               const float* __restrict__ points, const int* __restrict__ k,
                                                               pasnl_scan_crop_t* __restrict__ desc, int* __restrict__ out_cloud) {
  __shared__ double shv[ST_WAVES];
  __shared__ long shi[ST_WAVES];
  const long cloud = st_argmin(min_possibility, s, shv, shi);
  const long long off = offsets[cloud];
  const long n = (long)(offsets[cloud + 1] - off);
  const long pick = st_argmin(possibility + off, n, shv, shi);
  if (threadIdx.x == 0) {
    pasnl_scan_crop_t d;
    d.offset = off; d.cloud = (int)cloud; d.pick = (int)pick; d.n = (int)n; d.k = *k; d.pad = 0;
    const float* c = points + (size_t)(off + (pick < 0 ? 0 : pick)) * 3;
    d.cx = c[0]; d.cy = c[1]; d.cz = c[2];
    *desc = d;
    if (out_cloud) *out_cloud = (int)cloud;
  }
}

// ---- order / permute (the LDS sort is test_loop.hpp's op_sort)
__global__ __launch_bounds__(ST_THREADS) void crop_order_permute_kernel(const pasnl_scan_crop_t* __restrict__ desc,
                                                                        const float* __restrict__ points, const int* __restrict__ idx,
                                                                        const double* __restrict__ d2, int kcap,
                                                                        const int* __restrict__ perm, int num_point,
                                                                        int* __restrict__ out_select, float* __restrict__ out_points) {
  __shared__ unsigned long long key[OP_CAP];
  __shared__ unsigned short pos[OP_CAP];
  const int c = blockIdx.x, tid = threadIdx.x;
  const pasnl_scan_crop_t d = desc[c];
  int m = d.k < kcap ? d.k : kcap;
  m = m < d.n ? m : d.n;  // the count pasnl_knn_crop_indirect selected
  const int* ic = idx + (size_t)c * kcap;
  const double* dc = d2 + (size_t)c * kcap;
  for (int i = tid; i < m; i += ST_THREADS) {
    key[i] = (unsigned long long)__double_as_longlong(dc[i]);
    pos[i] = (unsigned short)i;
  }
  __syncthreads();
  op_sort(key, pos, m);
  const int* pc = perm + (size_t)c * num_point;
  int* os = out_select + (size_t)c * num_point;
  float* op = out_points + (size_t)c * num_point * 3;
  const float* sp = points + (size_t)d.offset * 3;
  for (int j = tid; j < num_point; j += ST_THREADS) {
    int q = pc[j];
    q = q < 0 ? 0 : (q >= m ? m - 1 : q);  // (the host draws a permutation of [0, k): never taken)
    const int sel = m > 0 ? ic[pos[q]] : 0;
    os[j] = sel;
    op[(size_t)j * 3] = sp[(size_t)sel * 3];
    op[(size_t)j * 3 + 1] = sp[(size_t)sel * 3 + 1];
    op[(size_t)j * 3 + 2] = sp[(size_t)sel * 3 + 2];
  }
}

// ---- possibility update
__device__ __forceinline__ float up_dist(const float* __restrict__ p, const pasnl_scan_crop_t& d) {
  // (selected_pc - pc[pick_idx]) in float64 (sklearn's copy), .astype(float32), squared and summed over the axis in float32
  const float dx = (float)((double)p[0] - (double)d.cx), dy = (float)((double)p[1] - (double)d.cy),
              dz = (float)((double)p[2] - (double)d.cz);
  return (dx * dx + dy * dy) + dz * dz;
}

// one workgroup: max(dists) -> scratch[0]; win[idx] = max row naming idx
__global__ __launch_bounds__(ST_THREADS) void up_mark_kernel(int num_point, const pasnl_scan_crop_t* __restrict__ desc,
                                                             const float* __restrict__ points, const int* __restrict__ select,
                                                             int* __restrict__ win, float* __restrict__ scratch) {
  __shared__ float sh[ST_WAVES];
  const pasnl_scan_crop_t d = *desc;
  const float* sp = points + (size_t)d.offset * 3;
  float m = -__builtin_inff();
  for (int j = threadIdx.x; j < num_point; j += ST_THREADS) {
    const int i = select[j];
    m = nan_max(m, up_dist(sp + (size_t)i * 3, d));
    atomicMax(&win[i], j);
  }
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < ST_WAVES; ++w) m = nan_max(m, sh[w]);
    scratch[0] = m;
  }
}

__global__ __launch_bounds__(256) void up_apply_kernel(int num_point, const pasnl_scan_crop_t* __restrict__ desc,
                                                       const float* __restrict__ points, const int* __restrict__ select,
                                                       double* __restrict__ possibility, int* __restrict__ win,
                                                       const float* __restrict__ scratch) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= num_point) return;
  const pasnl_scan_crop_t d = *desc;
  const int i = select[j];
  if (__hip_atomic_load(&win[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) return;
  const float dist = up_dist(points + (size_t)(d.offset + i) * 3, d);
  float delta = 1.0f - dist / scratch[0];
  delta = delta * delta;
  double* p = possibility + d.offset + i;
  *p = *p + (double)delta;
  __hip_atomic_store(&win[i], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one workgroup: min_possibility[cloud] = min(possibility of the scan), NaN propagating (np.min)
__global__ __launch_bounds__(ST_THREADS) void up_min_kernel(const pasnl_scan_crop_t* __restrict__ desc,
                                                            const double* __restrict__ possibility, double* __restrict__ min_possibility) {
  __shared__ double sh[ST_WAVES];
  const pasnl_scan_crop_t d = *desc;
  const double m = st_min(possibility + d.offset, d.n, sh);
  if (threadIdx.x == 0) min_possibility[d.cloud] = m;
}

__global__ __launch_bounds__(256) void scratch_init_kernel(long n, int* __restrict__ win) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) win[i] = -1;
}

// ---- votes: crop `c` of the batch (the mark is test_loop.hpp's vote_mark_kernel)
constexpr int VOTE_MAXC = 64;

__global__ __launch_bounds__(256) void vote_apply_kernel(int num_point, int nc, const float* __restrict__ values, int is_logits,
                                                         const int* __restrict__ select, const int* __restrict__ cloud,
                                                         const long long* __restrict__ offsets, unsigned short smooth_old,
                                                         float smooth_new, _Float16* __restrict__ test_probs, int* __restrict__ win) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= num_point) return;
  const int i = select[j];
  if (__hip_atomic_load(&win[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) return;
  const float* v = values + (size_t)j * nc;
  float p[VOTE_MAXC];
  if (is_logits) {
    vote_softmax(v, nc, p);
  } else {
    for (int q = 0; q < nc; ++q) p[q] = v[q];
  }
  const _Float16 h = __builtin_bit_cast(_Float16, smooth_old);
  _Float16* row = test_probs + ((size_t)offsets[*cloud] + (size_t)i) * (size_t)nc;  // 64-bit: the table may exceed 2^31 entries
  for (int q = 0; q < nc; ++q) {
    const _Float16 prod = (_Float16)((float)h * (float)row[q]);  // numpy float16 multiply: exact f32 product, one rounding
    row[q] = (_Float16)((float)prod + smooth_new * p[q]);        // float16 + float32 -> float32, stored with RNE
  }
  __hip_atomic_store(&win[i], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- reprojection: counting-sorted uniform grid + exact ring search
struct RpWs {
  int* count;   // [cells]
  int* start;   // [cells + 1]
  int* ids;     // [n_sub]
  int* bsum;    // [blocks of RP_SCAN]
};
constexpr int RP_SCAN = 4096;  // cells per block of the prefix sum (1024 threads x 4)
static inline size_t rp_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t rp_layout(long n_sub, long cells, char* base, RpWs* w) {
  const long nb = (cells + RP_SCAN - 1) / RP_SCAN;
  size_t off = 0;
  w->count = reinterpret_cast<int*>(base + off); off += rp_align((size_t)cells * 4);
  w->start = reinterpret_cast<int*>(base + off); off += rp_align((size_t)(cells + 1) * 4);
  w->ids = reinterpret_cast<int*>(base + off); off += rp_align((size_t)(n_sub > 0 ? n_sub : 1) * 4);
  w->bsum = reinterpret_cast<int*>(base + off); off += rp_align((size_t)(nb + 1) * 4);
  return off;
}

struct RpGrid {
  double ox, oy, oz, h;
  int nx, ny, nz;
};
__device__ __forceinline__ int rp_axis(double v, double o, double h, int nd) {
  const double t = floor((v - o) / h);
  return t < 0.0 ? 0 : (t >= (double)nd ? nd - 1 : (int)t);  // (NaN -> nd - 1)
}
__device__ __forceinline__ long rp_cell(const float* p, const RpGrid& g, int& ix, int& iy, int& iz) {
  ix = rp_axis((double)p[0], g.ox, g.h, g.nx);
  iy = rp_axis((double)p[1], g.oy, g.h, g.ny);
  iz = rp_axis((double)p[2], g.oz, g.h, g.nz);
  return ((long)iz * g.ny + iy) * g.nx + ix;
}

__global__ __launch_bounds__(256) void rp_zero_kernel(long cells, int* __restrict__ count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < cells) count[i] = 0;
}
__global__ __launch_bounds__(256) void rp_count_kernel(long n_sub, const float* __restrict__ sub, RpGrid g, int* __restrict__ count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_sub) return;
  int ix, iy, iz;
  atomicAdd(&count[rp_cell(sub + i * 3, g, ix, iy, iz)], 1);
}
// exclusive prefix sum of count -> start, block-local (block sums into bsum), then the block offsets are added
__global__ __launch_bounds__(ST_THREADS) void rp_scan_kernel(long cells, const int* __restrict__ in, int* __restrict__ out,
                                                             int* __restrict__ bsum) {
  __shared__ int sh[ST_WAVES];
  const long base = (long)blockIdx.x * RP_SCAN + (long)threadIdx.x * 4;
  int v[4], s = 0;
  for (int e = 0; e < 4; ++e) { v[e] = base + e < cells ? in[base + e] : 0; s += v[e]; }
  const int incl = wave_inclusive_sum_i32(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int pre = incl - s;
  for (int w = 0; w < wave; ++w) pre += sh[w];
  for (int e = 0; e < 4; ++e) {
    if (base + e < cells) out[base + e] = pre;
    pre += v[e];
  }
  if (threadIdx.x == ST_THREADS - 1) bsum[blockIdx.x] = pre;
}
// one workgroup: exclusive prefix of the block sums (sequential per chunk: nb <= cells / 4096 is small), total -> start[cells]
__global__ __launch_bounds__(64) void rp_scan_blocks_kernel(long nb, int* __restrict__ bsum, int* __restrict__ start, long cells) {
  if (threadIdx.x != 0) return;
  int acc = 0;
  for (long b = 0; b < nb; ++b) { const int t = bsum[b]; bsum[b] = acc; acc += t; }
  start[cells] = acc;
}
__global__ __launch_bounds__(256) void rp_add_kernel(long cells, int* __restrict__ start, const int* __restrict__ bsum,
                                                     int* __restrict__ cursor) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const int v = start[i] + bsum[i / RP_SCAN];
  start[i] = v;
  cursor[i] = v;
}
__global__ __launch_bounds__(256) void rp_fill_kernel(long n_sub, const float* __restrict__ sub, RpGrid g, int* __restrict__ cursor,
                                                      int* __restrict__ ids) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_sub) return;
  int ix, iy, iz;
  ids[atomicAdd(&cursor[rp_cell(sub + i * 3, g, ix, iy, iz)], 1)] = (int)i;  // (order within a cell is free: ties go by index)
}

__global__ __launch_bounds__(256) void rp_query_kernel(long n_raw, const float* __restrict__ raw, const float* __restrict__ sub,
                                                       RpGrid g, const int* __restrict__ start, const int* __restrict__ ids,
                                                       int* __restrict__ out) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n_raw) return;
  const float* rp = raw + q * 3;
  const double qx = (double)rp[0], qy = (double)rp[1], qz = (double)rp[2];
  int cx, cy, cz;
  rp_cell(rp, g, cx, cy, cz);
  unsigned long long best = ~0ull;  // f64 key bits (non-negative: they order like the number), then the index
  int bi = -1;
  const int rmax = max(g.nx, max(g.ny, g.nz));
  const double margin = 1e-6 * g.h;
  for (int r = 0; r <= rmax; ++r) {
    const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r, z0 = cz - r, z1 = cz + r;
    for (int z = max(z0, 0); z <= min(z1, g.nz - 1); ++z)
      for (int y = max(y0, 0); y <= min(y1, g.ny - 1); ++y) {
        const bool yzface = z == z0 || z == z1 || y == y0 || y == y1;
        for (int x = max(x0, 0); x <= min(x1, g.nx - 1); x += (yzface || x == x1) ? 1 : (x1 - x)) {  // ring r only
          const long cell = ((long)z * g.ny + y) * g.nx + x;
          for (int e = start[cell]; e < start[cell + 1]; ++e) {
            const int i = ids[e];
            const float* sp = sub + (size_t)i * 3;
            const double dx = (double)sp[0] - qx, dy = (double)sp[1] - qy, dz = (double)sp[2] - qz;
            const unsigned long long key = (unsigned long long)__double_as_longlong((dx * dx + dy * dy) + dz * dz);
            if (key < best || (key == best && i < bi)) { best = key; bi = i; }
          }
        }
      }
    // every cell outside rings 0..r lies beyond one face of the box of cells [c-r, c+r]; a face at the grid's edge has none
    double gap = __builtin_inf();
    if (x0 > 0) gap = fmin(gap, qx - (g.ox + (double)x0 * g.h));
    if (x1 < g.nx - 1) gap = fmin(gap, (g.ox + (double)(x1 + 1) * g.h) - qx);
    if (y0 > 0) gap = fmin(gap, qy - (g.oy + (double)y0 * g.h));
    if (y1 < g.ny - 1) gap = fmin(gap, (g.oy + (double)(y1 + 1) * g.h) - qy);
    if (z0 > 0) gap = fmin(gap, qz - (g.oz + (double)z0 * g.h));
    if (z1 < g.nz - 1) gap = fmin(gap, (g.oz + (double)(z1 + 1) * g.h) - qz);
    if (gap == __builtin_inf()) break;  // every cell has been examined
    gap -= margin;
    if (bi >= 0 && gap > 0.0 && gap * gap > __longlong_as_double((long long)best) * (1.0 + 1e-9)) break;
  }
  out[q] = bi;
}

__global__ __launch_bounds__(256) void labels_kernel(long n_raw, const int* __restrict__ proj, const _Float16* __restrict__ probs,
                                                     int nc, const int* __restrict__ lut, unsigned* __restrict__ out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_raw) return;
  const long r = proj ? (long)proj[j] : j;
  const _Float16* row = probs + (size_t)r * nc;
  int a = 0;
  float best = (float)row[0];
  for (int q = 1; q < nc && best == best; ++q) {  // np.argmax: the first maximum; the first NaN ends the search
    const float v = (float)row[q];
    if (v > best || v != v) { best = v; a = q; }
  }
  const unsigned pred = (unsigned)a;
  out[j] = ((pred >> 16) << 16) + (unsigned)lut[pred & 0xFFFFu];
}

}  // namespace pasnl

using namespace pasnl;

static inline unsigned st_blocks(long n, int t) { return (unsigned)((n + t - 1) / t); }

extern "C" int pasnl_scan_pick(int s, const long long* offsets, const double* possibility, const double* min_possibility,
                               const float* points, const int* k, pasnl_scan_crop_t* desc, int* out_cloud, pasnl_stream_t stream) {
  PASNL_REQUIRE(s > 0, PASNL_EINVAL);
  PASNL_REQUIRE(offsets && possibility && min_possibility && points && k && desc, PASNL_ENULL);
  hipLaunchKernelGGL(scan_pick_kernel, dim3(1), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), s, offsets, possibility,
                     min_possibility, points, k, desc, out_cloud);
  return pasnl_launch_status();
}

extern "C" int pasnl_crop_order_permute(int b, const pasnl_scan_crop_t* desc, const float* points, const int* idx, const double* d2,
                                        int kcap, const int* perm, int num_point, int* out_select, float* out_points,
                                        pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && kcap > 0 && num_point > 0, PASNL_EINVAL);
  PASNL_REQUIRE(kcap <= OP_CAP, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(desc && points && idx && d2 && perm && out_select && out_points, PASNL_ENULL);
  hipLaunchKernelGGL(crop_order_permute_kernel, dim3(b), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), desc, points, idx, d2, kcap,
                     perm, num_point, out_select, out_points);
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_possibility_update(int num_point, const pasnl_scan_crop_t* desc, const float* points, const int* select,
                                             double* possibility, double* min_possibility, int* win, float* scratch,
                                             pasnl_stream_t stream) {
  PASNL_REQUIRE(num_point > 0, PASNL_EINVAL);
  PASNL_REQUIRE(desc && points && select && possibility && min_possibility && win && scratch, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  hipLaunchKernelGGL(up_mark_kernel, dim3(1), dim3(ST_THREADS), 0, s, num_point, desc, points, select, win, scratch);
  hipLaunchKernelGGL(up_apply_kernel, dim3(st_blocks(num_point, 256)), dim3(256), 0, s, num_point, desc, points, select, possibility,
                     win, (const float*)scratch);
  hipLaunchKernelGGL(up_min_kernel, dim3(1), dim3(ST_THREADS), 0, s, desc, (const double*)possibility, min_possibility);
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_scratch_init(long n, int* win, pasnl_stream_t stream) {
  PASNL_REQUIRE(n >= 0, PASNL_EINVAL);
  if (n == 0) return PASNL_OK;
  PASNL_REQUIRE(win, PASNL_ENULL);
  hipLaunchKernelGGL(scratch_init_kernel, dim3(st_blocks(n, 256)), dim3(256), 0, pasnl_hip_stream(stream), n, win);
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_vote(int b, int num_point, int c, const float* values, int is_logits, const int* select, const int* cloud,
                               const long long* offsets, unsigned short smooth_old, float smooth_new, void* test_probs, int* win,
                               pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && num_point > 0 && c > 0, PASNL_EINVAL);
  PASNL_REQUIRE(c <= VOTE_MAXC, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(values && select && cloud && offsets && test_probs && win, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const unsigned g = st_blocks(num_point, 256);
  for (int i = 0; i < b; ++i) {  // crop after crop: a later crop of the batch smooths what the earlier one wrote
    const int* sel = select + (size_t)i * num_point;
    hipLaunchKernelGGL(vote_mark_kernel, dim3(g), dim3(256), 0, s, num_point, sel, win);
    hipLaunchKernelGGL(vote_apply_kernel, dim3(g), dim3(256), 0, s, num_point, c, values + (size_t)i * num_point * c, is_logits, sel,
                       cloud + i, offsets, smooth_old, smooth_new, static_cast<_Float16*>(test_probs), win);
  }
  return pasnl_launch_status();
}

extern "C" size_t pasnl_scan_reproject_workspace_bytes(long n_sub, long cells) {
  if (n_sub < 0 || cells <= 0) return 0;
  RpWs w;
  return rp_layout(n_sub, cells, nullptr, &w);
}

extern "C" int pasnl_scan_reproject(long n_sub, const float* sub, long n_raw, const float* raw, double ox, double oy, double oz,
                                    double h, int nx, int ny, int nz, int* out_proj, void* workspace, size_t workspace_bytes,
                                    pasnl_stream_t stream) {
  PASNL_REQUIRE(n_sub > 0 && n_sub < (1l << 31) && n_raw >= 0 && h > 0.0 && nx > 0 && ny > 0 && nz > 0, PASNL_EINVAL);
  const long cells = (long)nx * ny * nz;
  PASNL_REQUIRE(cells < (1l << 30), PASNL_EINVAL);
  if (n_raw == 0) return PASNL_OK;
  PASNL_REQUIRE(sub && raw && out_proj && workspace, PASNL_ENULL);
  RpWs w;
  PASNL_REQUIRE(workspace_bytes >= rp_layout(n_sub, cells, static_cast<char*>(workspace), &w), PASNL_EWORKSPACE);
  hipStream_t s = pasnl_hip_stream(stream);
  RpGrid g{ox, oy, oz, h, nx, ny, nz};
  const long nb = (cells + RP_SCAN - 1) / RP_SCAN;
  hipLaunchKernelGGL(rp_zero_kernel, dim3(st_blocks(cells, 256)), dim3(256), 0, s, cells, w.count);
  hipLaunchKernelGGL(rp_count_kernel, dim3(st_blocks(n_sub, 256)), dim3(256), 0, s, n_sub, sub, g, w.count);
  hipLaunchKernelGGL(rp_scan_kernel, dim3((unsigned)nb), dim3(ST_THREADS), 0, s, cells, (const int*)w.count, w.start, w.bsum);
  hipLaunchKernelGGL(rp_scan_blocks_kernel, dim3(1), dim3(64), 0, s, nb, w.bsum, w.start, cells);
  hipLaunchKernelGGL(rp_add_kernel, dim3(st_blocks(cells, 256)), dim3(256), 0, s, cells, w.start, (const int*)w.bsum, w.count);
  hipLaunchKernelGGL(rp_fill_kernel, dim3(st_blocks(n_sub, 256)), dim3(256), 0, s, n_sub, sub, g, w.count, w.ids);
  hipLaunchKernelGGL(rp_query_kernel, dim3(st_blocks(n_raw, 256)), dim3(256), 0, s, n_raw, raw, sub, g, (const int*)w.start,
                     (const int*)w.ids, out_proj);
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_labels(long n_raw, const int* proj, const void* probs, int c, const int* lut, int nlut, unsigned* out,
                                 pasnl_stream_t stream) {
  PASNL_REQUIRE(n_raw >= 0 && c > 0 && nlut >= c, PASNL_EINVAL);
  if (n_raw == 0) return PASNL_OK;
  PASNL_REQUIRE(probs && lut && out, PASNL_ENULL);
  hipLaunchKernelGGL(labels_kernel, dim3(st_blocks(n_raw, 256)), dim3(256), 0, pasnl_hip_stream(stream), n_raw, proj,
                     static_cast<const _Float16*>(probs), c, lut, out);
  return pasnl_launch_status();
}
