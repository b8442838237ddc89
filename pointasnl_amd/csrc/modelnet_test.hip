// The ModelNet40 classification evaluation loop around the forward, on the device: reference modelnet_dataset.py (D) :9-37
// `pc_normalize` and `farthest_point_sample`, :79-136 `_get_item` / `next_batch`, test.py (T) :105-174 `eval_one_epoch` and
// utils/provider.py (P) :8-24 `normalize_data`.  The fifth sibling of scan_test.hip, scene_test.hip, window_test.hip and
// kitti_window_test.hip.  Everything that has to equal numpy is done in numpy's dtypes and order (the library builds with
// -ffp-contract=off); the exactness contract is stated in include/pasnl.h per entry point and restated on the host in
// tests/modelnet_flow_ref.py.
//
// What stays on the host: the numpy RNG stream (one start index per sampled shape, the noise uniforms, the discarded
// shuffle of every vote).  One batch is
//   [first visit, uniform: pasnl_modelnet_fps -> pasnl_modelnet_normalize] -> pasnl_modelnet_batch -> [pasnl_modelnet_noise]
//   -> per vote: forward, pasnl_cls_vote -> pasnl_cls_tally
// with no synchronisation in between; the counters come down once, at the end of the epoch.  The training loop (train.py
// :208-264) puts pasnl_modelnet_augment -- next_batch fused with the augmentation chain of utils/provider.py -- in the place of
// pasnl_modelnet_batch and takes one vote.
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"
#include "window_scan.hpp"

namespace pasnl {

// ---- D:16-37: numpy's farthest point sampling, one workgroup per raw shape
constexpr int MF_CAP = 12288;                 // raw rows of one shape: 12288 * 12 B = 144 KiB of LDS (gfx950: 160 KiB per workgroup)
constexpr int MF_PER = MF_CAP / ST_THREADS;   // running distances a thread keeps in registers

// The shape's xyz sits in LDS (a stride of three floats between lanes: no bank conflict); a thread keeps the running distances
// of its points in registers.  A round's pick is the maximum of (distance bits, ~index) as one 64-bit key: distances are sums of
// squares (>= +0, their bits order as the values do), so the largest key is the largest distance and, among equals, the
// lowest index -- np.argmax.  Wave maximum by DPP, then 16 keys through LDS (two buffers: one barrier per round).
__global__ __launch_bounds__(ST_THREADS) void modelnet_fps_kernel(int npoint, int ld, long n_shapes, const int* __restrict__ ids,
                                                                  const long* __restrict__ row0, const int* __restrict__ nraw,
                                                                  const int* __restrict__ start, long total_rows, int n_hi,
                                                                  const float* __restrict__ raw, int* __restrict__ out_idx,
                                                                  float* __restrict__ out_rows, int out_ld) {
  extern __shared__ float pts[];  // (n, 3)
  __shared__ unsigned long long shkey[2][ST_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long id = ids ? (long)ids[blockIdx.x] : (long)blockIdx.x;
  if (id < 0 || id >= n_shapes) return;  // (uniform over the workgroup, as every return below)
  const int n = nraw[id];
  const long r0 = row0[id];
  int far = start[blockIdx.x];
  if (n < npoint || n > n_hi || n > MF_CAP || r0 < 0 || r0 + n > total_rows || far < 0 || far >= n) return;
  const float* __restrict__ src = raw + (size_t)r0 * ld;
  for (int i = tid; i < n; i += ST_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) pts[i * 3 + a] = src[(size_t)i * ld + a];
  }
  float dist[MF_PER];
#pragma unroll
  for (int q = 0; q < MF_PER; ++q) dist[q] = 1e10f;  // np.ones((N,)) * 1e10: exact in float32
  __syncthreads();
  const size_t out0 = (size_t)id * npoint;
  for (int r = 0; r < npoint; ++r) {
    if (tid == 0 && out_idx) out_idx[out0 + r] = far;
    if (out_rows && tid < out_ld) out_rows[(out0 + r) * out_ld + tid] = src[(size_t)far * ld + tid];
    const float cx = pts[far * 3], cy = pts[far * 3 + 1], cz = pts[far * 3 + 2];
    unsigned long long best = 0ull;  // below every real key: their low words are >= ~MF_CAP
#pragma unroll
    for (int q = 0; q < MF_PER; ++q) {
      const int i = q * ST_THREADS + tid;
      if (i < n) {
        const float dx = pts[i * 3] - cx, dy = pts[i * 3 + 1] - cy, dz = pts[i * 3 + 2] - cz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < dist[q]) dist[q] = d;
        const unsigned long long key = ((unsigned long long)__float_as_uint(dist[q]) << 32) | (0xFFFFFFFFu - (unsigned)i);
        best = key > best ? key : best;
      }
    }
    best = wave_max_u64(best);
    if (lane == 0) shkey[r & 1][wave] = best;
    __syncthreads();
    unsigned long long m = shkey[r & 1][0];
#pragma unroll
    for (int w = 1; w < ST_WAVES; ++w) m = shkey[r & 1][w] > m ? shkey[r & 1][w] : m;
    far = (int)(0xFFFFFFFFu - (unsigned)m);
  }
}

// ---- D:9-14: pc_normalize in place on columns 0..2 of one prepared shape per workgroup
constexpr int MN_TILE = 4096;  // rows per staged tile: 48 KiB of LDS

__global__ __launch_bounds__(ST_THREADS) void modelnet_normalize_kernel(int npoint, int ld, long n_shapes, const int* __restrict__ ids,
                                                                        float* __restrict__ data) {
  __shared__ float tile[MN_TILE * 3];
  __shared__ float cen[3], shm[ST_WAVES];
  const int tid = threadIdx.x;
  const long id = ids ? (long)ids[blockIdx.x] : (long)blockIdx.x;
  if (id < 0 || id >= n_shapes) return;
  float* __restrict__ p = data + (size_t)id * npoint * ld;
  float acc = -0.0f;
  for (int base = 0; base < npoint; base += MN_TILE) {
    const int cnt = npoint - base < MN_TILE ? npoint - base : MN_TILE;
    for (int k = tid; k < cnt * 3; k += ST_THREADS) tile[k] = p[(size_t)(base + k / 3) * ld + k % 3];
    __syncthreads();
    if (tid < 3) acc = st_chain3(acc, tile, cnt, tid);
    __syncthreads();
  }
  if (tid < 3) cen[tid] = acc / (float)npoint;
  __syncthreads();
  float m = -__builtin_inff();
  for (int i = tid; i < npoint; i += ST_THREADS) {
    const float x = p[(size_t)i * ld] - cen[0], y = p[(size_t)i * ld + 1] - cen[1], z = p[(size_t)i * ld + 2] - cen[2];
    m = nan_max(m, sqrtf((x * x + y * y) + z * z));
  }
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) shm[tid >> 6] = m;
  __syncthreads();
  m = shm[0];
#pragma unroll
  for (int w = 1; w < ST_WAVES; ++w) m = nan_max(m, shm[w]);
  for (int i = tid; i < npoint; i += ST_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[(size_t)i * ld + a] = (p[(size_t)i * ld + a] - cen[a]) / m;
  }
}

// ---- D:124-136, T:135-136: bsize prepared shapes into the first rows of the persistent batch; one thread per float
__global__ __launch_bounds__(256) void modelnet_batch_kernel(long entries, int bsize, long per_shape, const int* __restrict__ order,
                                                             long n_shapes, const float* __restrict__ prepared,
                                                             const int* __restrict__ shape_labels, float* __restrict__ batch,
                                                             int* __restrict__ labels) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const long id = order[e / per_shape];
  if (id < 0 || id >= n_shapes) return;
  batch[e] = prepared[(size_t)id * per_shape + e % per_shape];
  if (e < bsize) {
    const long lid = order[e];
    if (lid >= 0 && lid < n_shapes) labels[e] = shape_labels[lid];
  }
}

// ---- train.py:224-241 with P:39-253: next_batch and the whole augmentation chain, one thread per output point.  The draws
// are the host's; every product and sum is numpy's float64 one, rounded to float32 where the reference's arrays are float32.
__device__ __forceinline__ void ma_dot(const double x[3], const double* __restrict__ m, double out[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (x[0] * m[c] + x[1] * m[3 + c]) + x[2] * m[6 + c];
}

template <int CH>
__global__ __launch_bounds__(256) void modelnet_augment_kernel(long entries, int bsize, int npoint, const int* __restrict__ order,
                                                               long n_shapes, const float* __restrict__ prepared,
                                                               const int* __restrict__ shape_labels, const double* __restrict__ mats,
                                                               const double* __restrict__ scale, const double* __restrict__ shift,
                                                               const int* __restrict__ perm, const double* __restrict__ ratio,
                                                               const double* __restrict__ u, float* __restrict__ batch,
                                                               int* __restrict__ labels) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int i = (int)(e / npoint), j = (int)(e % npoint);
  const long id = order[i];
  if (id < 0 || id >= n_shapes) return;
  if (j == 0) labels[i] = shape_labels[id];
  const int p = perm[u[e] <= ratio[i] ? 0 : j];  // P:250-252 behind P:47-49: a dropped point is the shuffled cloud's first
  if (p < 0 || p >= npoint) return;
  const float* __restrict__ src = prepared + ((size_t)id * npoint + p) * CH;
  float x[CH];
  if (CH == 6) {  // rows of 24 bytes: three 8-byte reads
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float2 v = reinterpret_cast<const float2*>(src)[q];
      x[2 * q] = v.x, x[2 * q + 1] = v.y;
    }
  } else {  // rows of 12 bytes are 8-byte aligned at every other row only
#pragma unroll
    for (int q = 0; q < CH; ++q) x[q] = src[q];
  }
  const double s = scale[i];
  if (mats) {
    const double* __restrict__ a = mats + (size_t)i * 18;
#pragma unroll
    for (int h = 0; h < CH; h += 3) {
      double v[3] = {(double)x[h], (double)x[h + 1], (double)x[h + 2]}, w[3];
      ma_dot(v, a, w);
      if (CH == 3) {  // P:59: rotate_point_cloud allocates float32
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = (double)(float)w[c];
      }
      ma_dot(w, a + 9, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) x[h + c] = (float)v[c];  // P:118,188: float32
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // float32 *= float64, float32 += float64: each rounds
      const float t = (float)((double)x[c] * s);
      x[c] = (float)((double)t + shift[i * 3 + c]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = (float)(((double)x[c] * s) + shift[i * 3 + c]);  // float64 until the feed
  }
  float* __restrict__ dst = batch + (size_t)e * CH;
  if (CH == 6) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float2*>(dst)[q] = make_float2(x[2 * q], x[2 * q + 1]);
  } else {
#pragma unroll
    for (int q = 0; q < CH; ++q) dst[q] = x[q];
  }
}

// ---- T:129-132 with P:8-24: one (K,3) float64 block per workgroup -> float32 rows 0..K-1, columns 0..2, of its batch row
__global__ __launch_bounds__(256) void modelnet_noise_kernel(int k, const double* __restrict__ uniforms, int npoint, int ch,
                                                             float* __restrict__ batch) {
  __shared__ double cen[3], shm[4];
  const int tid = threadIdx.x;
  const double* __restrict__ p = uniforms + (size_t)blockIdx.x * k * 3;
  float* __restrict__ out = batch + (size_t)blockIdx.x * npoint * ch;
  if (tid < 3) cen[tid] = st_chain3(-0.0, p, k, tid) / (double)k;
  __syncthreads();
  double m = -__builtin_inf();
  for (int i = tid; i < k; i += 256) {
    const double x = p[i * 3] - cen[0], y = p[i * 3 + 1] - cen[1], z = p[i * 3 + 2] - cen[2];
    m = nan_max(m, sqrt((x * x + y * y) + z * z));
  }
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) shm[tid >> 6] = m;
  __syncthreads();
  m = nan_max(nan_max(shm[0], shm[1]), nan_max(shm[2], shm[3]));
  for (int i = tid; i < k; i += 256) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[(size_t)i * ch + a] = (float)((p[i * 3 + a] - cen[a]) / m);  // the feed into a float32 placeholder
  }
}

// ---- T:147-149 for one vote: float64 += float32 sums, and the batch's mean cross-entropy into loss[1] (loss_vote)
__global__ __launch_bounds__(256) void cls_vote_kernel(int b, int c, const float* __restrict__ logits, const int* __restrict__ labels,
                                                       double* __restrict__ sums, double* __restrict__ loss) {
  __shared__ double shs[4];
  const int tid = threadIdx.x;
  for (int e = tid; e < b * c; e += 256) sums[e] += (double)logits[e];
  double part = 0.0;
  for (int r = tid; r < b; r += 256) {
    const float* row = logits + (size_t)r * c;
    float mx = row[0];
    for (int q = 1; q < c; ++q) mx = row[q] > mx ? row[q] : mx;
    float s = 0.0f;
    for (int q = 0; q < c; ++q) s += expf(row[q] - mx);
    const int l = labels[r];
    if (l >= 0 && l < c) part += (double)((logf(s) + mx) - row[l]);
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if ((tid & 63) == 0) shs[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) loss[1] += (((shs[0] + shs[1]) + shs[2]) + shs[3]) / (double)b;
}

// ---- T:150-162: argmax of the sums, the counters, and the sums cleared for the next batch
__global__ __launch_bounds__(256) void cls_tally_kernel(int b, int bsize, int c, int num_votes, const int* __restrict__ labels,
                                                        double* __restrict__ sums, long long* __restrict__ totals,
                                                        long long* __restrict__ seen_class, long long* __restrict__ correct_class,
                                                        int* __restrict__ preds, double* __restrict__ loss) {
  const int tid = threadIdx.x;
  for (int i = tid; i < bsize; i += 256) {
    const double* row = sums + (size_t)i * c;
    int a = 0;
    double best = row[0];
    bool nan = best != best;
    for (int q = 1; q < c && !nan; ++q) {  // np.argmax: the first maximum, the first NaN
      const double v = row[q];
      if (v > best || v != v) { best = v; a = q; nan = v != v; }
    }
    preds[i] = a;
    const int l = labels[i];
    if (l >= 0 && l < c) {
      atomicAdd((unsigned long long*)&seen_class[l], 1ull);
      if (a == l) {
        atomicAdd((unsigned long long*)&correct_class[l], 1ull);
        atomicAdd((unsigned long long*)&totals[0], 1ull);
      }
    }
  }
  __syncthreads();  // every row is read before any is cleared
  for (int e = tid; e < b * c; e += 256) sums[e] = 0.0;
  if (tid == 0) {
    totals[1] += bsize;
    totals[2] += b;
    loss[0] += loss[1] / (double)num_votes;  // loss_vote /= num_votes; loss_sum += loss_vote
    loss[1] = 0.0;
  }
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_modelnet_fps_cap(void) { return MF_CAP; }

extern "C" int pasnl_modelnet_fps(int s, int npoint, int ld, long n_shapes, const int* ids, const long* row0, const int* nraw,
                                  const int* start, int n_min, int n_max, long total_rows, const float* raw, int* out_idx,
                                  float* out_rows, int out_ld, pasnl_stream_t stream) {
  PASNL_REQUIRE(s >= 0 && npoint > 0 && ld >= 3 && n_shapes >= 0 && n_min > 0 && n_max >= n_min && total_rows >= 0, PASNL_EINVAL);
  PASNL_REQUIRE(npoint <= n_min && (ids || s <= n_shapes) && (!out_rows || (out_ld >= 3 && out_ld <= ld)), PASNL_EINVAL);
  PASNL_REQUIRE(n_max <= MF_CAP, PASNL_EUNSUPPORTED);
  if (s == 0) return PASNL_OK;
  PASNL_REQUIRE(row0 && nraw && start && raw && (out_idx || out_rows), PASNL_ENULL);
  const int rc = launch(modelnet_fps_kernel, dim3(s), dim3(ST_THREADS), (size_t)n_max * 3 * sizeof(float), pasnl_hip_stream(stream),
                        npoint, ld, n_shapes, ids, row0, nraw, start, total_rows, n_max, raw, out_idx, out_rows, out_ld);
  return rc != PASNL_OK ? rc : pasnl_launch_status();
}

extern "C" int pasnl_modelnet_normalize(int s, int npoint, int ld, long n_shapes, const int* ids, float* data, pasnl_stream_t stream) {
  PASNL_REQUIRE(s >= 0 && npoint > 0 && ld >= 3 && n_shapes >= 0 && (ids || s <= n_shapes), PASNL_EINVAL);
  if (s == 0) return PASNL_OK;
  PASNL_REQUIRE(data, PASNL_ENULL);
  hipLaunchKernelGGL(modelnet_normalize_kernel, dim3(s), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), npoint, ld, n_shapes, ids, data);
  return pasnl_launch_status();
}

extern "C" int pasnl_modelnet_batch(int b, int bsize, int npoint, int ch, const int* order, long n_order, long start, long n_shapes,
                                    const float* prepared, const int* shape_labels, float* batch, int* labels, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && bsize >= 0 && bsize <= b && npoint > 0 && (ch == 3 || ch == 6) && n_shapes >= 0 && start >= 0 &&
                    n_order >= 0 && start + bsize <= n_order, PASNL_EINVAL);
  if (b == 0 || bsize == 0) return PASNL_OK;
  PASNL_REQUIRE(order && prepared && shape_labels && batch && labels, PASNL_ENULL);
  const long per_shape = (long)npoint * ch, entries = (long)bsize * per_shape;
  hipLaunchKernelGGL(modelnet_batch_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, bsize, per_shape,
                     order + start, n_shapes, prepared, shape_labels, batch, labels);
  return pasnl_launch_status();
}

extern "C" int pasnl_modelnet_augment(int b, int bsize, int npoint, int ch, const int* order, long n_order, long start, long n_shapes,
                                      const float* prepared, const int* shape_labels, const double* mats, const double* scale,
                                      const double* shift, const int* perm, const double* ratio, const double* u, float* batch,
                                      int* labels, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && bsize >= 0 && bsize <= b && npoint >= 1 && (ch == 3 || ch == 6) && n_shapes >= 0 && start >= 0 &&
                    n_order >= 0 && start + bsize <= n_order, PASNL_EINVAL);
  if (bsize == 0) return PASNL_OK;
  PASNL_REQUIRE(order && prepared && shape_labels && scale && shift && perm && ratio && u && batch && labels, PASNL_ENULL);
  const long entries = (long)bsize * npoint;
  if (ch == 6)
    hipLaunchKernelGGL(modelnet_augment_kernel<6>, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, bsize,
                       npoint, order + start, n_shapes, prepared, shape_labels, mats, scale, shift, perm, ratio, u, batch, labels);
  else
    hipLaunchKernelGGL(modelnet_augment_kernel<3>, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, bsize,
                       npoint, order + start, n_shapes, prepared, shape_labels, mats, scale, shift, perm, ratio, u, batch, labels);
  return pasnl_launch_status();
}

extern "C" int pasnl_modelnet_noise(int bsize, int k, const double* uniforms, int npoint, int ch, float* batch, pasnl_stream_t stream) {
  PASNL_REQUIRE(bsize >= 0 && npoint > 0 && (ch == 3 || ch == 6) && k >= 1 && k <= npoint, PASNL_EINVAL);
  if (bsize == 0) return PASNL_OK;
  PASNL_REQUIRE(uniforms && batch, PASNL_ENULL);
  hipLaunchKernelGGL(modelnet_noise_kernel, dim3(bsize), dim3(256), 0, pasnl_hip_stream(stream), k, uniforms, npoint, ch, batch);
  return pasnl_launch_status();
}

extern "C" int pasnl_cls_vote(int b, int c, const float* logits, const int* labels, double* sums, double* loss, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && c >= 1 && (long)b * c <= (1L << 30), PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && labels && sums && loss, PASNL_ENULL);
  hipLaunchKernelGGL(cls_vote_kernel, dim3(1), dim3(256), 0, pasnl_hip_stream(stream), b, c, logits, labels, sums, loss);
  return pasnl_launch_status();
}

extern "C" int pasnl_cls_tally(int b, int bsize, int c, int num_votes, const int* labels, double* sums, long long* totals,
                               long long* seen_class, long long* correct_class, int* preds, double* loss, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && bsize >= 0 && bsize <= b && c >= 1 && num_votes >= 1 && (long)b * c <= (1L << 30), PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(labels && sums && totals && seen_class && correct_class && preds && loss, PASNL_ENULL);
  hipLaunchKernelGGL(cls_tally_kernel, dim3(1), dim3(256), 0, pasnl_hip_stream(stream), b, bsize, c, num_votes, labels, sums, totals,
                     seen_class, correct_class, preds, loss);
  return pasnl_launch_status();
}
