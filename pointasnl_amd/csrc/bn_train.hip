// Training-mode batch norm and dropout for gfx950 (reference utils/tf_util.py:512-531 batch_norm_template with
// is_training=True, :594-615 dropout): pasnl_cls_bn_train, pasnl_cls_bn_train_grad, pasnl_cls_dropout.  include/pasnl.h has the
// contracts, DESIGN.md 4.6 the structure and the bounds.
//
// The matrix is (rows, c) row-major, the channel last, and every reduction runs over rows.  A workgroup of 256 threads is a
// (ly, lx) rectangle, lx * ly = 256: lx lanes along the channel axis, each owning VW consecutive channels (VW = 4 with 16-byte
// accesses where c % 4 == 0 and every matrix pointer is 16-byte aligned, else VW = 1), ly rows at a time.  lx is the smallest
// power of two with lx * VW >= c, at most 64: a wave reads 64 / lx whole rows' worth of contiguous bytes.  grid.x tiles the
// channel axis in lx * VW columns, grid.y cuts the rows into slabs -- the slab count comes from the row count (one slab per
// BNT_SLAB_ROWS rows, up to BNT_MAX_BLOCKS workgroups), so a (10^6, 4) matrix fills the device as a (10^6, 128) one does.
//
// Column sums are taken in float64 (sum x and sum x^2, or sum g and sum g xhat): a thread adds its rows in ascending order, the
// ly threads of a column are folded by a fixed tree in LDS, each workgroup writes ONE partial per column into the workspace and
// a second launch adds the slabs' partials -- lane l the slabs l, l + 64, ..., then a fixed butterfly.  No atomics, nothing
// depends on the order workgroups run in: the same bytes in give the same bits out.  var = E[x^2] - mean^2 is formed in
// float64, where a column with |mean| / std = 2^10 still keeps 2^-33 of its variance.
//
//   rows > BNT_SMALL_ROWS:  partial sums | finalize (statistics, moving update)  | apply          3 launches
//                           partial sums | finalize (grad_gamma, grad_beta)      | grad_x         3 launches (2 without grad_x)
//   rows <= BNT_SMALL_ROWS: one launch, one workgroup per BNT_SMALL_LX * VW channels does all three steps (the FC heads).
//
// Traffic: forward x twice and y once; backward x, y, grad_y twice and grad_x once (y only with the ReLU mask).
#include <math.h>
#include "common.hpp"

namespace pasnl {

constexpr int BNT_THREADS = 256;
constexpr int BNT_MAX_LX = 64;        // lanes along the channel axis: a channel tile is BNT_MAX_LX * VW columns at most
constexpr int BNT_SLAB_ROWS = 256;    // rows per partial-sum workgroup at least
constexpr int BNT_MAX_BLOCKS = 2048;  // partial-sum workgroups at most (8 per CU)
constexpr int BNT_SMALL_ROWS = 128;   // up to here a call is ONE launch
constexpr int BNT_SMALL_LX = 8;       // ... whose workgroups are (32, 8): 8 * VW channels each
constexpr int BNT_APPLY_ROWS = 4;     // rows per thread of the elementwise passes

// slabs of the partial sums, as include/pasnl.h states it (a bound for both vector widths: the scalar path has more channel
// tiles and takes fewer slabs)
static inline long bnt_slabs(long rows, int c) {
  const long by_rows = (rows + BNT_SLAB_ROWS - 1) / BNT_SLAB_ROWS;
  const long by_grid = BNT_MAX_BLOCKS / ((c + BNT_MAX_LX * 4 - 1) / (BNT_MAX_LX * 4));
  return by_rows < 1 ? 1 : (by_rows < (by_grid < 1 ? 1 : by_grid) ? by_rows : (by_grid < 1 ? 1 : by_grid));
}

struct BntPlan {
  int lx_log2, ctiles;
  long slabs, slab_rows;
};

static inline BntPlan bnt_plan(long rows, int c, int vw, bool small) {
  BntPlan p;
  const int max_lx = small ? BNT_SMALL_LX : BNT_MAX_LX;
  p.lx_log2 = 0;
  while ((1 << p.lx_log2) < max_lx && (long)(1 << p.lx_log2) * vw < c) ++p.lx_log2;
  const int tile = (1 << p.lx_log2) * vw;
  p.ctiles = (c + tile - 1) / tile;
  long slabs = bnt_slabs(rows, c);
  const long by_grid = BNT_MAX_BLOCKS / p.ctiles;
  if (slabs > by_grid) slabs = by_grid < 1 ? 1 : by_grid;
  const int ly = BNT_THREADS >> p.lx_log2;
  p.slab_rows = ((rows + slabs - 1) / slabs + ly - 1) / ly * ly;  // whole (ly)-row steps
  p.slabs = (rows + p.slab_rows - 1) / p.slab_rows;               // <= slabs: no empty slab
  return p;
}

template <int VW>
__device__ __forceinline__ void bnt_load(const float* p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VW>
__device__ __forceinline__ void bnt_store(float* p, const float (&v)[VW]) {
  if constexpr (VW == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// the two column sums of rows r0 + ty, r0 + ty + ly, ... < r1, then folded over ty by a fixed tree: valid in the threads ty == 0.
// GRAD: (sum g, sum g xhat) with g = grad_y [y > 0]; else (sum x, sum x^2).
template <int VW, bool GRAD>
__device__ __forceinline__ void bnt_column_sums(long r0, long r1, int c, int ch, int lx_log2, const float* __restrict__ x,
                                                const float* __restrict__ y, const float* __restrict__ gy,
                                                const float (&mean)[VW], const float (&rstd)[VW], int act, double (&s)[VW],
                                                double (&q)[VW], double (*red)[BNT_THREADS][VW]) {
  const int lx = 1 << lx_log2, ly = BNT_THREADS >> lx_log2;
  const int tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
#pragma unroll
  for (int k = 0; k < VW; ++k) s[k] = q[k] = 0.0;
  if (ch < c) {
#pragma unroll 4
    for (long r = r0 + ty; r < r1; r += ly) {
      const size_t e = (size_t)r * c + ch;
      float xv[VW];
      bnt_load<VW>(x + e, xv);
      if constexpr (GRAD) {
        float gv[VW];
        bnt_load<VW>(gy + e, gv);
        if (act) {
          float yv[VW];
          bnt_load<VW>(y + e, yv);
#pragma unroll
          for (int k = 0; k < VW; ++k) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < VW; ++k) {
          const float xh = (xv[k] - mean[k]) * rstd[k];
          s[k] += (double)gv[k];
          q[k] += (double)gv[k] * (double)xh;
        }
      } else {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
          const double d = (double)xv[k];
          s[k] += d;
          q[k] += d * d;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    red[0][threadIdx.x][k] = s[k];
    red[1][threadIdx.x][k] = q[k];
  }
  for (int h = ly >> 1; h >= 1; h >>= 1) {
    __syncthreads();
    if (ty < h) {
      const int o = ((ty + h) << lx_log2) + tx;
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        red[0][threadIdx.x][k] += red[0][o][k];
        red[1][threadIdx.x][k] += red[1][o][k];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    s[k] = red[0][tx][k];
    q[k] = red[1][tx][k];
  }
}

// statistics of one column from its two sums; the moving update of TF's assign_moving_average(zero_debias=False)
__device__ __forceinline__ void bnt_statistics(double s, double q, long rows, float eps, float decay, int unbiased, int ch,
                                               float* moving_mean, float* moving_var, float* save_mean, float* save_rstd,
                                               float& mean_f, float& rstd_f) {
  const double mean = s / (double)rows;
  double var = q / (double)rows - mean * mean;
  var = var > 0.0 ? var : 0.0;
  mean_f = (float)mean;
  rstd_f = (float)(1.0 / sqrt(var + (double)eps));
  save_mean[ch] = mean_f;
  save_rstd[ch] = rstd_f;
  if (moving_mean) {
    const float keep = 1.0f - decay;
    const float batch_var = (float)(unbiased ? var * ((double)rows / (double)(rows > 1 ? rows - 1 : 1)) : var);
    const float mm = moving_mean[ch], mv = moving_var[ch];
    moving_mean[ch] = mm - (mm - mean_f) * keep;
    moving_var[ch] = mv - (mv - batch_var) * keep;
  }
}

template <int VW>
__device__ __forceinline__ void bnt_apply_rows(long r0, long r1, long step, int c, int ch, const float* __restrict__ x,
                                               const float (&mean)[VW], const float (&rstd)[VW], const float (&ga)[VW],
                                               const float (&be)[VW], int act, float* __restrict__ y) {
  for (long r = r0; r < r1; r += step) {
    const size_t e = (size_t)r * c + ch;
    float v[VW];
    bnt_load<VW>(x + e, v);
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const float z = ((v[k] - mean[k]) * rstd[k]) * ga[k] + be[k];
      v[k] = act ? (z > 0.0f ? z : 0.0f) : z;
    }
    bnt_store<VW>(y + e, v);
  }
}

// grad_x = gamma rstd (g - grad_beta / rows - xhat grad_gamma / rows)
template <int VW>
__device__ __forceinline__ void bnt_grad_rows(long r0, long r1, long step, int c, int ch, const float* __restrict__ x,
                                              const float* __restrict__ y, const float* __restrict__ gy, const float (&mean)[VW],
                                              const float (&rstd)[VW], const float (&scale)[VW], const float (&mb)[VW],
                                              const float (&mg)[VW], int act, float* __restrict__ gx) {
  for (long r = r0; r < r1; r += step) {
    const size_t e = (size_t)r * c + ch;
    float xv[VW], gv[VW];
    bnt_load<VW>(x + e, xv);
    bnt_load<VW>(gy + e, gv);
    if (act) {
      float yv[VW];
      bnt_load<VW>(y + e, yv);
#pragma unroll
      for (int k = 0; k < VW; ++k) gv[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const float xh = (xv[k] - mean[k]) * rstd[k];
      gv[k] = scale[k] * ((gv[k] - mb[k]) - xh * mg[k]);
    }
    bnt_store<VW>(gx + e, gv);
  }
}

// ---- rows > BNT_SMALL_ROWS: partial sums -> workspace [2][slabs][c] float64
template <int VW, bool GRAD>
__global__ __launch_bounds__(BNT_THREADS) void bnt_partial_kernel(long rows, int c, int lx_log2, long slab_rows,
                                                                  const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ gy, const float* __restrict__ save_mean,
                                                                  const float* __restrict__ save_rstd, int act,
                                                                  double* __restrict__ part) {
  __shared__ double red[2][BNT_THREADS][VW];
  const int lx = 1 << lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
  const int ch = (blockIdx.x * lx + tx) * VW;
  const long r0 = (long)blockIdx.y * slab_rows, r1 = r0 + slab_rows < rows ? r0 + slab_rows : rows;
  float mean[VW], rstd[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    mean[k] = (GRAD && ch < c) ? save_mean[ch + k] : 0.0f;
    rstd[k] = (GRAD && ch < c) ? save_rstd[ch + k] : 0.0f;
  }
  double s[VW], q[VW];
  bnt_column_sums<VW, GRAD>(r0, r1, c, ch, lx_log2, x, y, gy, mean, rstd, act, s, q, red);
  if (ty == 0 && ch < c) {
    const size_t slabs = gridDim.y;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      part[(size_t)blockIdx.y * c + ch + k] = s[k];
      part[(slabs + blockIdx.y) * c + ch + k] = q[k];
    }
  }
}

// one wave per column: lane l adds the slabs l, l + 64, ... in ascending order, then a butterfly (every lane ends with the
// same sum).  GRAD: (grad_beta, grad_gamma) = the sums; else the statistics and the moving update.
template <bool GRAD>
__global__ __launch_bounds__(BNT_THREADS) void bnt_finalize_kernel(long rows, int c, int slabs, const double* __restrict__ part,
                                                                   float eps, float decay, int unbiased, float* moving_mean,
                                                                   float* moving_var, float* __restrict__ out0,
                                                                   float* __restrict__ out1) {
  const int ch = blockIdx.x * (BNT_THREADS / PASNL_WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (ch >= c) return;
  double s = 0.0, q = 0.0;
  for (int sl = lane; sl < slabs; sl += PASNL_WAVE) {
    s += part[(size_t)sl * c + ch];
    q += part[((size_t)slabs + sl) * c + ch];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    q += __shfl_xor(q, off);
  }
  if (lane != 0) return;
  if constexpr (GRAD) {
    out0[ch] = (float)q;  // grad_gamma
    out1[ch] = (float)s;  // grad_beta
  } else {
    float m, r;
    bnt_statistics(s, q, rows, eps, decay, unbiased, ch, moving_mean, moving_var, out0, out1, m, r);
  }
}

template <int VW>
__global__ __launch_bounds__(BNT_THREADS) void bnt_apply_kernel(long rows, int c, int lx_log2, const float* __restrict__ x,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ save_mean,
                                                                const float* __restrict__ save_rstd, int act,
                                                                float* __restrict__ y) {
  const int lx = 1 << lx_log2, ly = BNT_THREADS >> lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
  const int ch = (blockIdx.x * lx + tx) * VW;
  if (ch >= c) return;
  float mean[VW], rstd[VW], ga[VW], be[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    mean[k] = save_mean[ch + k]; rstd[k] = save_rstd[ch + k]; ga[k] = gamma[ch + k]; be[k] = beta[ch + k];
  }
  bnt_apply_rows<VW>((long)blockIdx.y * ly + ty, rows, (long)gridDim.y * ly, c, ch, x, mean, rstd, ga, be, act, y);
}

template <int VW>
__global__ __launch_bounds__(BNT_THREADS) void bnt_grad_x_kernel(long rows, int c, int lx_log2, const float* __restrict__ x,
                                                                 const float* __restrict__ y, const float* __restrict__ gy,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ save_mean,
                                                                 const float* __restrict__ save_rstd,
                                                                 const float* __restrict__ grad_gamma,
                                                                 const float* __restrict__ grad_beta, int act,
                                                                 float* __restrict__ gx) {
  const int lx = 1 << lx_log2, ly = BNT_THREADS >> lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
  const int ch = (blockIdx.x * lx + tx) * VW;
  if (ch >= c) return;
  float mean[VW], rstd[VW], scale[VW], mb[VW], mg[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    mean[k] = save_mean[ch + k]; rstd[k] = save_rstd[ch + k]; scale[k] = gamma[ch + k] * rstd[k];
    mb[k] = grad_beta[ch + k] / (float)rows; mg[k] = grad_gamma[ch + k] / (float)rows;
  }
  bnt_grad_rows<VW>((long)blockIdx.y * ly + ty, rows, (long)gridDim.y * ly, c, ch, x, y, gy, mean, rstd, scale, mb, mg, act, gx);
}

// ---- rows <= BNT_SMALL_ROWS: everything in one launch, one workgroup per channel tile
template <int VW>
__global__ __launch_bounds__(BNT_THREADS) void bnt_small_kernel(long rows, int c, int lx_log2, const float* __restrict__ x,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, float decay, int act, int unbiased, float* moving_mean,
                                                                float* moving_var, float* __restrict__ y,
                                                                float* __restrict__ save_mean, float* __restrict__ save_rstd) {
  __shared__ double red[2][BNT_THREADS][VW];
  __shared__ float stat[2][BNT_MAX_LX][VW];
  const int lx = 1 << lx_log2, ly = BNT_THREADS >> lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
  const int ch = (blockIdx.x * lx + tx) * VW;
  float mean[VW], rstd[VW], ga[VW], be[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) mean[k] = rstd[k] = 0.0f;
  double s[VW], q[VW];
  bnt_column_sums<VW, false>(0, rows, c, ch, lx_log2, x, nullptr, nullptr, mean, rstd, 0, s, q, red);
  if (ty == 0 && ch < c) {
#pragma unroll
    for (int k = 0; k < VW; ++k)
      bnt_statistics(s[k], q[k], rows, eps, decay, unbiased, ch + k, moving_mean, moving_var, save_mean, save_rstd, stat[0][tx][k],
                     stat[1][tx][k]);
  }
  __syncthreads();
  if (ch >= c) return;
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    mean[k] = stat[0][tx][k]; rstd[k] = stat[1][tx][k]; ga[k] = gamma[ch + k]; be[k] = beta[ch + k];
  }
  bnt_apply_rows<VW>(ty, rows, ly, c, ch, x, mean, rstd, ga, be, act, y);
}

template <int VW>
__global__ __launch_bounds__(BNT_THREADS) void bnt_small_grad_kernel(long rows, int c, int lx_log2, const float* __restrict__ x,
                                                                     const float* __restrict__ y, const float* __restrict__ gy,
                                                                     const float* __restrict__ gamma,
                                                                     const float* __restrict__ save_mean,
                                                                     const float* __restrict__ save_rstd, int act,
                                                                     float* __restrict__ gx, float* __restrict__ grad_gamma,
                                                                     float* __restrict__ grad_beta) {
  __shared__ double red[2][BNT_THREADS][VW];
  __shared__ float sums[2][BNT_MAX_LX][VW];
  const int lx = 1 << lx_log2, ly = BNT_THREADS >> lx_log2, tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> lx_log2;
  const int ch = (blockIdx.x * lx + tx) * VW;
  float mean[VW], rstd[VW], scale[VW], mb[VW], mg[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    mean[k] = ch < c ? save_mean[ch + k] : 0.0f;
    rstd[k] = ch < c ? save_rstd[ch + k] : 0.0f;
  }
  double s[VW], q[VW];
  bnt_column_sums<VW, true>(0, rows, c, ch, lx_log2, x, y, gy, mean, rstd, act, s, q, red);
  if (ty == 0 && ch < c) {
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      grad_beta[ch + k] = sums[0][tx][k] = (float)s[k];
      grad_gamma[ch + k] = sums[1][tx][k] = (float)q[k];
    }
  }
  __syncthreads();
  if (ch >= c || gx == nullptr) return;
#pragma unroll
  for (int k = 0; k < VW; ++k) {
    scale[k] = gamma[ch + k] * rstd[k];
    mb[k] = sums[0][tx][k] / (float)rows;
    mg[k] = sums[1][tx][k] / (float)rows;
  }
  bnt_grad_rows<VW>(ty, rows, ly, c, ch, x, y, gy, mean, rstd, scale, mb, mg, act, gx);
}

// workgroups along the rows of an elementwise pass: BNT_APPLY_ROWS rows per thread, the grid's y limit respected
static inline unsigned bnt_apply_grid_y(long rows, int lx_log2) {
  const long per = (long)(BNT_THREADS >> lx_log2) * BNT_APPLY_ROWS;
  const long gy = (rows + per - 1) / per;
  return (unsigned)(gy < 1 ? 1 : (gy > 65535 ? 65535 : gy));
}

static inline bool bnt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool bnt_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <int VW>
static int bnt_forward(long rows, int c, const float* x, const float* gamma, const float* beta, float eps, float decay, int act,
                       int unbiased, float* moving_mean, float* moving_var, float* y, float* save_mean, float* save_rstd,
                       double* part, hipStream_t st) {
  if (rows <= BNT_SMALL_ROWS) {
    const BntPlan p = bnt_plan(rows, c, VW, true);
    hipLaunchKernelGGL(bnt_small_kernel<VW>, dim3(p.ctiles), dim3(BNT_THREADS), 0, st, rows, c, p.lx_log2, x, gamma, beta, eps, decay,
                       act, unbiased, moving_mean, moving_var, y, save_mean, save_rstd);
    return pasnl_launch_status();
  }
  const BntPlan p = bnt_plan(rows, c, VW, false);
  hipLaunchKernelGGL((bnt_partial_kernel<VW, false>), dim3(p.ctiles, (unsigned)p.slabs), dim3(BNT_THREADS), 0, st, rows, c, p.lx_log2,
                     p.slab_rows, x, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0,
                     part);
  hipLaunchKernelGGL(bnt_finalize_kernel<false>, dim3((c + 3) / 4), dim3(BNT_THREADS), 0, st, rows, c, (int)p.slabs, part, eps, decay,
                     unbiased, moving_mean, moving_var, save_mean, save_rstd);
  hipLaunchKernelGGL(bnt_apply_kernel<VW>, dim3(p.ctiles, bnt_apply_grid_y(rows, p.lx_log2)), dim3(BNT_THREADS), 0, st, rows, c,
                     p.lx_log2, x, gamma, beta, save_mean, save_rstd, act, y);
  return pasnl_launch_status();
}

template <int VW>
static int bnt_backward(long rows, int c, const float* x, const float* y, const float* gamma, const float* save_mean,
                        const float* save_rstd, int act, const float* grad_y, float* grad_x, float* grad_gamma, float* grad_beta,
                        double* part, hipStream_t st) {
  if (rows <= BNT_SMALL_ROWS) {
    const BntPlan p = bnt_plan(rows, c, VW, true);
    hipLaunchKernelGGL(bnt_small_grad_kernel<VW>, dim3(p.ctiles), dim3(BNT_THREADS), 0, st, rows, c, p.lx_log2, x, y, grad_y, gamma,
                       save_mean, save_rstd, act, grad_x, grad_gamma, grad_beta);
    return pasnl_launch_status();
  }
  const BntPlan p = bnt_plan(rows, c, VW, false);
  hipLaunchKernelGGL((bnt_partial_kernel<VW, true>), dim3(p.ctiles, (unsigned)p.slabs), dim3(BNT_THREADS), 0, st, rows, c, p.lx_log2,
                     p.slab_rows, x, y, grad_y, save_mean, save_rstd, act, part);
  hipLaunchKernelGGL(bnt_finalize_kernel<true>, dim3((c + 3) / 4), dim3(BNT_THREADS), 0, st, rows, c, (int)p.slabs, part, 0.0f, 0.0f, 0,
                     (float*)nullptr, (float*)nullptr, grad_gamma, grad_beta);
  if (grad_x)
    hipLaunchKernelGGL(bnt_grad_x_kernel<VW>, dim3(p.ctiles, bnt_apply_grid_y(rows, p.lx_log2)), dim3(BNT_THREADS), 0, st, rows, c,
                       p.lx_log2, x, y, grad_y, gamma, save_mean, save_rstd, grad_gamma, grad_beta, act, grad_x);
  return pasnl_launch_status();
}

// four consecutive elements per thread = the four words of one Philox block
__global__ __launch_bounds__(BNT_THREADS) void dropout_kernel(long n, float keep_prob, unsigned k0, unsigned k1, unsigned stream_id,
                                                              unsigned call, int vec, const float* x, float* y) {
  const long blk = (long)blockIdx.x * BNT_THREADS + threadIdx.x, i0 = blk * 4;
  if (i0 >= n) return;
  const Philox4 w = philox4x32_10((unsigned)blk, (unsigned)((unsigned long long)blk >> 32), call, stream_id, k0, k1);
  float v[4];
  if (vec && i0 + 4 <= n) {
    bnt_load<4>(x + i0, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = philox_uniform(w.w[k]) < keep_prob ? v[k] / keep_prob : 0.0f;
    bnt_store<4>(y + i0, v);
    return;
  }
  for (int k = 0; k < 4 && i0 + k < n; ++k) y[i0 + k] = philox_uniform(w.w[k]) < keep_prob ? x[i0 + k] / keep_prob : 0.0f;
}

}  // namespace pasnl

using namespace pasnl;

static size_t bnt_workspace_bytes(long rows, int c) {
  if (rows <= 0 || c <= 0) return 0;
  return (size_t)2 * sizeof(double) * (size_t)c * (size_t)bnt_slabs(rows, c);
}

extern "C" size_t pasnl_cls_bn_train_workspace_bytes(long rows, int c) { return bnt_workspace_bytes(rows, c); }
extern "C" size_t pasnl_cls_bn_train_grad_workspace_bytes(long rows, int c) { return bnt_workspace_bytes(rows, c); }

extern "C" int pasnl_cls_bn_train(long rows, int c, const float* x, const float* gamma, const float* beta, float eps, float decay,
                                  int act, int unbiased, float* moving_mean, float* moving_var, float* y, float* save_mean,
                                  float* save_rstd, void* workspace, size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && c > 0 && (act == 0 || act == 1) && eps > 0.0f && decay >= 0.0f && decay <= 1.0f, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(x && gamma && beta && y && save_mean && save_rstd && (moving_mean == nullptr) == (moving_var == nullptr), PASNL_ENULL);
  PASNL_REQUIRE(bnt_aligned4(x) && bnt_aligned4(y) && (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0) &&
                    (size_t)rows <= (size_t)1 << 40,
                PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(workspace && workspace_bytes >= bnt_workspace_bytes(rows, c), PASNL_EWORKSPACE);
  double* part = static_cast<double*>(workspace);
  const hipStream_t st = pasnl_hip_stream(stream);
  if (c % 4 == 0 && bnt_aligned16(x) && bnt_aligned16(y))
    return bnt_forward<4>(rows, c, x, gamma, beta, eps, decay, act, unbiased != 0, moving_mean, moving_var, y, save_mean, save_rstd,
                          part, st);
  return bnt_forward<1>(rows, c, x, gamma, beta, eps, decay, act, unbiased != 0, moving_mean, moving_var, y, save_mean, save_rstd, part,
                        st);
}

extern "C" int pasnl_cls_bn_train_grad(long rows, int c, const float* x, const float* y, const float* gamma, const float* save_mean,
                                       const float* save_rstd, int act, const float* grad_y, float* grad_x, float* grad_gamma,
                                       float* grad_beta, void* workspace, size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && c > 0 && (act == 0 || act == 1), PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(x && (y || act == 0) && gamma && save_mean && save_rstd && grad_y && grad_gamma && grad_beta, PASNL_ENULL);
  PASNL_REQUIRE(bnt_aligned4(x) && bnt_aligned4(y) && bnt_aligned4(grad_y) && bnt_aligned4(grad_x) &&
                    (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0) && (size_t)rows <= (size_t)1 << 40,
                PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(workspace && workspace_bytes >= bnt_workspace_bytes(rows, c), PASNL_EWORKSPACE);
  double* part = static_cast<double*>(workspace);
  const hipStream_t st = pasnl_hip_stream(stream);
  if (c % 4 == 0 && bnt_aligned16(x) && bnt_aligned16(y) && bnt_aligned16(grad_y) && bnt_aligned16(grad_x))
    return bnt_backward<4>(rows, c, x, y, gamma, save_mean, save_rstd, act, grad_y, grad_x, grad_gamma, grad_beta, part, st);
  return bnt_backward<1>(rows, c, x, y, gamma, save_mean, save_rstd, act, grad_y, grad_x, grad_gamma, grad_beta, part, st);
}

extern "C" int pasnl_cls_dropout(long n, float keep_prob, unsigned long long seed, unsigned stream_id, unsigned call, const float* x,
                                 float* y, pasnl_stream_t stream) {
  PASNL_REQUIRE(n >= 0 && keep_prob > 0.0f && keep_prob <= 1.0f, PASNL_EINVAL);
  if (n == 0) return PASNL_OK;
  PASNL_REQUIRE(x && y, PASNL_ENULL);
  PASNL_REQUIRE(bnt_aligned4(x) && bnt_aligned4(y) && (size_t)n <= (size_t)1 << 40, PASNL_EUNSUPPORTED);
  const long blocks = ((n + 3) / 4 + BNT_THREADS - 1) / BNT_THREADS;
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)blocks), dim3(BNT_THREADS), 0, pasnl_hip_stream(stream), n, keep_prob,
                     (unsigned)seed, (unsigned)(seed >> 32), stream_id, call, (int)(bnt_aligned16(x) && bnt_aligned16(y)), x, y);
  return pasnl_launch_status();
}
