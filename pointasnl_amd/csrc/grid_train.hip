// The grid training input loops round the forward, on the device: reference ScanNet/scannet_dataset_grid.py (D) :435-645
// and SemanticKITTI/semantic_kitti_dataset_grid.py (K) :193-354, the `'training'` split of get_batch_gen and
// `tf_augment_input`.  The pick, the crop, the order and the potential update are the test loops' kernels (crop.hip,
// scan_test.hip, scene_test.hip); this file adds what only training needs:
//
//   pasnl_scan_pick_given    the descriptors of b crops whose scan and pick the host drew (K:216-221)
//   pasnl_scan_train_labels  the label / sample-weight gather of b crops (D:525-531, K:222, 237-239)
//   pasnl_scan_augment       tf_augment_input and the colour drop of b crops, one launch, one thread per point
//
// The augmentation's random numbers are Philox4x32-10 words in plain integer arithmetic, addressed by (seed, item, point):
// nothing is stored between launches, a captured chain replays with the item number the host staged, and
// tests/philox_ref.py restates every draw on the host.  The library builds with -ffp-contract=off: every float32 operation
// below is rounded on its own, as include/pasnl.h states.
//
// The augmentation is bound by memory and launch latency: b * num_point * width * 8 bytes moved against about a hundred
// integer operations per point; rows are read and written by consecutive threads, nothing else is tuned.
#include <math.h>
#include "common.hpp"

namespace pasnl {

constexpr int GT_THREADS = 256;
constexpr int GT_PICK_CHUNK = 64;  // host cloud indices per launch of pick_given_kernel (they travel as a kernel argument)

struct GtClouds {
  int v[GT_PICK_CHUNK];
};

__global__ __launch_bounds__(GT_PICK_CHUNK) void pick_given_kernel(int b, GtClouds clouds, const long long* __restrict__ offsets,
                                                                   const float* __restrict__ points, const int* __restrict__ pick,
                                                                   const int* __restrict__ k, pasnl_scan_crop_t* __restrict__ desc) {
  const int c = threadIdx.x;
  if (c >= b) return;
  const int cloud = clouds.v[c];
  const long long off = offsets[cloud];
  const long n = (long)(offsets[cloud + 1] - off);
  const int p = pick[c];
  const bool inside = p >= 0 && (long)p < n;
  pasnl_scan_crop_t d;
  d.offset = off; d.cloud = cloud; d.pick = p; d.n = inside ? (int)n : 0; d.k = k[c]; d.pad = 0;
  d.cx = d.cy = d.cz = 0.0f;
  if (inside) {
    const float* q = points + (size_t)(off + p) * 3;
    d.cx = q[0]; d.cy = q[1]; d.cz = q[2];
  }
  desc[c] = d;
}

__global__ __launch_bounds__(GT_THREADS) void train_labels_kernel(int num_point, const int* __restrict__ select,
                                                                  const int* __restrict__ cloud, const long long* __restrict__ offsets,
                                                                  const int* __restrict__ labels, const float* __restrict__ weights,
                                                                  int nw, int* __restrict__ out_labels, float* __restrict__ out_weights) {
  const int j = blockIdx.x * GT_THREADS + threadIdx.x, c = blockIdx.y;
  if (j >= num_point) return;
  const size_t e = (size_t)c * num_point + j;
  const int l = labels[(size_t)offsets[cloud[c]] + (size_t)select[e]];
  out_labels[e] = l;
  out_weights[e] = (weights && l >= 0 && l < nw) ? weights[l] : 0.0f;
}

// (Philox4x32-10 and its float32 uniform live in common.hpp: the dropout of bn_train.hip draws from the same generator)
__device__ __forceinline__ float gt_uniform(unsigned w) { return philox_uniform(w); }

// Box-Muller: radius from u1 = ((wa >> 8) + 1) * 2^-24 in (0,1], angle 2 pi u2 with u2 = (wb >> 8) * 2^-24 (the sine and the
// cosine take 2 u2 in half turns: no rounded angle) -> (r cos, r sin)
__device__ __forceinline__ void gt_box_muller(unsigned wa, unsigned wb, float& g0, float& g1) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * gt_uniform(wb), &sn, &cs);
  g0 = r * cs;
  g1 = r * sn;
}

struct GtConfig {
  int vertical, anisotropic, sym[3];
  float scale_min, scale_max, noise, color;
};

// (src and dst may be the same buffer: a thread reads its row before it writes it, and no other thread touches that row)
__global__ __launch_bounds__(GT_THREADS) void augment_kernel(int num_point, int width, const float* src, float* dst, GtConfig cfg,
                                                             unsigned long long seed, const unsigned long long* __restrict__ item0,
                                                             float* __restrict__ out_params, float* __restrict__ out_noise) {
  __shared__ float par[8];  // theta, cos, sin, s0, s1, s2, keep, 0
  const int c = blockIdx.y;
  const unsigned long long item = item0[0] + (unsigned long long)c;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), i0 = (unsigned)item, i1 = (unsigned)(item >> 32);
  if (threadIdx.x == 0) {
    const Philox4 a = philox4x32_10(0u, i0, i1, 0u, k0, k1), s = philox4x32_10(1u, i0, i1, 0u, k0, k1);
    float theta = 0.0f, cs = 1.0f, sn = 0.0f;
    if (cfg.vertical) {
      theta = gt_uniform(a.w[0]) * 6.2831853071795864769f;
      cs = (float)cos((double)theta);
      sn = (float)sin((double)theta);
    }
    par[0] = theta; par[1] = cs; par[2] = sn;
    const float span = cfg.scale_max - cfg.scale_min;
    for (int i = 0; i < 3; ++i) {
      const float sc = cfg.scale_min + gt_uniform(a.w[cfg.anisotropic ? 1 + i : 1]) * span;
      par[3 + i] = (cfg.sym[i] && !(gt_uniform(s.w[i]) > 0.5f)) ? -sc : sc;
    }
    par[6] = gt_uniform(s.w[3]) < cfg.color ? 1.0f : 0.0f;
    par[7] = 0.0f;
    if (out_params && blockIdx.x == 0)
      for (int i = 0; i < 8; ++i) out_params[(size_t)c * 8 + i] = par[i];
  }
  __syncthreads();
  const int j = blockIdx.x * GT_THREADS + threadIdx.x;
  if (j >= num_point) return;
  const size_t row = (size_t)c * num_point + j;
  const float* in = src + row * width;
  float* out = dst + row * width;
  const Philox4 g = philox4x32_10((unsigned)j, i0, i1, 1u, k0, k1);
  float nx, ny, nz, unused;
  gt_box_muller(g.w[0], g.w[1], nx, ny);
  gt_box_muller(g.w[2], g.w[3], nz, unused);
  const float x = in[0], y = in[1], z = in[2];
  float rx = x, ry = y;
  if (cfg.vertical) {
    rx = (x * par[1]) + (y * par[2]);
    ry = (y * par[1]) - (x * par[2]);
  }
  const float keep = par[6];
  float rest[3];
  const int ncol = width >= 6 ? 3 : 0;
  for (int q = 0; q < ncol; ++q) rest[q] = in[3 + q] * keep;
  out[0] = rx * par[3] + cfg.noise * nx;
  out[1] = ry * par[4] + cfg.noise * ny;
  out[2] = z * par[5] + cfg.noise * nz;
  for (int q = 0; q < ncol; ++q) out[3 + q] = rest[q];
  if (src != dst)
    for (int q = 3 + ncol; q < width; ++q) out[q] = in[q];
  if (out_noise) {
    out_noise[row * 3] = nx;
    out_noise[row * 3 + 1] = ny;
    out_noise[row * 3 + 2] = nz;
  }
}

}  // namespace pasnl

using namespace pasnl;

static inline unsigned gt_blocks(int n) { return (unsigned)((n + GT_THREADS - 1) / GT_THREADS); }

extern "C" int pasnl_scan_pick_given(int b, int s, const long long* offsets, const float* points, const int* cloud, const int* pick,
                                     const int* k, pasnl_scan_crop_t* desc, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && s > 0, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(offsets && points && cloud && pick && k && desc, PASNL_ENULL);
  for (int c = 0; c < b; ++c) PASNL_REQUIRE(cloud[c] >= 0 && cloud[c] < s, PASNL_EINVAL);
  for (int c0 = 0; c0 < b; c0 += GT_PICK_CHUNK) {
    const int m = b - c0 < GT_PICK_CHUNK ? b - c0 : GT_PICK_CHUNK;
    GtClouds cl;
    for (int c = 0; c < GT_PICK_CHUNK; ++c) cl.v[c] = c < m ? cloud[c0 + c] : 0;
    hipLaunchKernelGGL(pick_given_kernel, dim3(1), dim3(GT_PICK_CHUNK), 0, pasnl_hip_stream(stream), m, cl, offsets, points,
                       pick + c0, k + c0, desc + c0);
  }
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_train_labels(int b, int num_point, const int* select, const int* cloud, const long long* offsets,
                                       const int* labels, const float* weights, int nw, int* out_labels, float* out_weights,
                                       pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && b <= 65535 && num_point > 0 && nw >= 0, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(select && cloud && offsets && labels && out_labels && out_weights, PASNL_ENULL);
  hipLaunchKernelGGL(train_labels_kernel, dim3(gt_blocks(num_point), b), dim3(GT_THREADS), 0, pasnl_hip_stream(stream), num_point,
                     select, cloud, offsets, labels, weights, nw, out_labels, out_weights);
  return pasnl_launch_status();
}

extern "C" int pasnl_scan_augment(int b, int num_point, int width, const float* src, float* dst, int rotation, float scale_min,
                                  float scale_max, int anisotropic, int sym_x, int sym_y, int sym_z, float noise, float color,
                                  unsigned long long seed, const unsigned long long* item0, float* out_params, float* out_noise,
                                  pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && b <= 65535 && num_point > 0 && width >= 3 && (rotation == 0 || rotation == 1), PASNL_EINVAL);
  PASNL_REQUIRE(scale_min <= scale_max && noise >= 0.0f && color == color, PASNL_EINVAL);  // (NaN fails each comparison)
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(src && dst && item0, PASNL_ENULL);
  GtConfig cfg;
  cfg.vertical = rotation; cfg.anisotropic = anisotropic != 0;
  cfg.sym[0] = sym_x != 0; cfg.sym[1] = sym_y != 0; cfg.sym[2] = sym_z != 0;
  cfg.scale_min = scale_min; cfg.scale_max = scale_max; cfg.noise = noise; cfg.color = color;
  hipLaunchKernelGGL(augment_kernel, dim3(gt_blocks(num_point), b), dim3(GT_THREADS), 0, pasnl_hip_stream(stream), num_point, width,
                     src, dst, cfg, seed, item0, out_params, out_noise);
  return pasnl_launch_status();
}
