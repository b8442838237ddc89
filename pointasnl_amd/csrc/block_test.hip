// ScanNet's two training-time validation loops around the forward, on the device: reference ScanNet/scannet_dataset.py (D)
// :31-64 `ScannetDataset.__getitem__` (a 1.5 m column round a drawn centre, rejected unless 70 % of it is labelled and 2 % of a
// 31x31x62 voxel grid is occupied, resampled to block_points rows) and :92-129 `ScannetDatasetWholeScene.__getitem__` (every
// non-empty column of a non-overlapping 1.5 m grid, resampled likewise), ScanNet/train_scannet.py (T) :279-329
// `eval_one_epoch` and :333-420 `eval_whole_scene_one_epoch` (argmax over ALL classes, counters under smpw > 0, the weighted
// cross-entropy) and utils/provider.py (P) :8-24 `normalize_data`, :71-89 `rotate_point_cloud_z`.  The sixth sibling of
// scan_test.hip, scene_test.hip, window_test.hip, kitti_window_test.hip and modelnet_test.hip.  Everything that has to equal
// numpy is done in numpy's dtypes and order (the library builds with -ffp-contract=off); the exactness contract is stated in
// include/pasnl.h per entry point and restated on the host in tests/block_flow_ref.py.
//
// What stays on the host: the numpy RNG stream (the centre of every try, the resampling choices, the rotation angles), the
// acceptance test of a try (two Python-float comparisons on three integers) and the carry-over of rows between scenes.
//   chopped: per try pasnl_block_crop_stats -> [four integers down]; then [choices up] -> pasnl_block_fill -> pasnl_block_gather
//   whole:   pasnl_block_grid_count -> [nx*ny counts down; choices up] -> pasnl_block_fill -> pasnl_block_gather
//   per batch, with no synchronisation: pasnl_block_normalize -> forward -> pasnl_block_score
// The training input loop (T:233-276 `train_one_epoch`, and SemanticKITTI/train_semantic_kitti.py:223-264) draws the same
// chopped items in a shuffled order; per batch: pasnl_block_train_batch (rotate, round, normalize: the other order; the
// SemanticKITTI loop only rotates, pasnl_kblock_rotate) -> step -> pasnl_block_train_score (tallies over every entry).
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"
#include "window_scan.hpp"

namespace pasnl {

constexpr int BT_KEYS = 1 << 19;       // voxel keys the bitmap distinguishes: 64 KiB of LDS per workgroup
constexpr int BT_MAX_GROUPS = 1024;    // workgroups of the statistics pass (each clears and merges one LDS bitmap)
constexpr int BT_CLASS_MAX = 256;      // classes whose counters a workgroup keeps in LDS
constexpr int BT_SCORE_GROUPS = 256;   // workgroups of the score pass == partial loss sums the last pass adds in order

// ---- the chopped column (D:41-46, 52) is window_scan.hpp's CropBox round the centre with half = 0.75, its mask margin 0.01;
// the whole-scene grid (D:107-109, 115) is its ColumnGrid with curmin = float64(coordmin) + i * 1.5,
// curmax = float64(coordmin) + (i + 1) * 1.5 (i * 1.5 and (i + 1) * 1.5 are exact), its mask margin 0.001
constexpr double BT_HALF = 0.75;
static inline ColumnGrid block_grid(long centre, int nx, int ny) { return {nx, ny, 1.5, 1.5, true, 0.2, centre >= 0 ? 0.01 : 0.001}; }

// Pass 1 of a try, one wave per chunk: hist[c] = members (0.2 margin), hist[nchunks + c] = members with label > 0 (two
// ballots, no atomics), and the voxel key of every member inside the 0.01 margin set in the workgroup's LDS bitmap, which is
// OR-merged into bitmap[1 + word] at the end; bitmap[0] flags a key outside [key_lo, key_lo + 32 * words) or a NaN key.
__global__ __launch_bounds__(64 * COL_WAVES) void block_crop_stats_kernel(long n, const float* __restrict__ xyz, const int* __restrict__ labels,
                                                                         const float* __restrict__ bounds, long centre, double key_lo,
                                                                         int words, long nchunks, int* __restrict__ hist,
                                                                         unsigned* __restrict__ bitmap) {
  extern __shared__ unsigned bits[];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int k = tid; k < words; k += 64 * COL_WAVES) bits[k] = 0u;
  __syncthreads();
  const CropBox box = crop_box(xyz + centre * 3, bounds, BT_HALF);
  const double span = (double)words * 32.0;
  for (long c = (long)blockIdx.x * COL_WAVES + (tid >> 6); c < nchunks; c += (long)gridDim.x * COL_WAVES) {  // (wave-uniform)
    const long p = c * 64 + lane;
    bool in20 = false, in1 = false, lab = false;
    double q[3] = {0.0, 0.0, 0.0};
    if (p < n) {
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = (double)xyz[p * 3 + a];
      in20 = crop_inside(box, q, 0.2);
      in1 = in20 && crop_inside(box, q, 0.01);
      lab = in20 && labels[p] > 0;
    }
    const unsigned long long b20 = __ballot(in20), bl = __ballot(lab);
    if (lane == 0) {
      hist[c] = __popcll(b20);
      hist[nchunks + c] = __popcll(bl);
    }
    if (in1) {  // np.ceil((p - curmin) / (curmax - curmin) * [31.0, 31.0, 62.0]); vx * 31.0 * 62.0 + vy * 62.0 + vz
      const double vx = ceil(((q[0] - box.lo[0]) / (box.hi[0] - box.lo[0])) * 31.0);
      const double vy = ceil(((q[1] - box.lo[1]) / (box.hi[1] - box.lo[1])) * 31.0);
      const double vz = ceil(((q[2] - box.lo[2]) / (box.hi[2] - box.lo[2])) * 62.0);
      const double rel = (((vx * 31.0) * 62.0 + vy * 62.0) + vz) - key_lo;  // integers far below 2^53: exact
      if (rel >= 0.0 && rel < span) {
        const unsigned r = (unsigned)rel;
        atomicOr(&bits[r >> 5], 1u << (r & 31u));
      } else {
        atomicOr(&bitmap[0], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < words; k += 64 * COL_WAVES) {
    const unsigned v = bits[k];
    if (v) atomicOr(&bitmap[1 + k], v);
  }
}

// Pass 3 of a try (pass 2 is window_scan_kernel over the two histograms): len(np.unique(keys)) = the bitmap's popcount
__global__ __launch_bounds__(256) void block_unique_kernel(int words, const unsigned* __restrict__ bitmap, int* __restrict__ stats) {
  __shared__ int sh[4];
  int cnt = 0;
  for (int k = threadIdx.x; k < words; k += 256) cnt += __popc(bitmap[1 + k]);
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[2] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    stats[3] = (int)bitmap[0];
  }
}

// ---- rows (D:58-63, D:116-122): one thread per row entry
__global__ __launch_bounds__(256) void block_gather_kernel(long entries, const int* __restrict__ rowpos, long cap, const int* __restrict__ cat_idx,
                                                           const unsigned char* __restrict__ cat_mask, long n, const float* __restrict__ xyz,
                                                           const float* __restrict__ rgb, int nfeat, const int* __restrict__ labels, int c,
                                                           const double* __restrict__ labelweights, float* __restrict__ out_data,
                                                           int* __restrict__ out_label, float* __restrict__ out_smpw) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int width = 3 + nfeat;
  float* row = out_data + (size_t)e * width;
  const long pos = rowpos[e];
  const long i = pos >= 0 && pos < cap ? (long)cat_idx[pos] : -1;
  const int l = i >= 0 && i < n ? labels[i] : -1;
  if (l < 0 || l >= c) {  // (a position outside the lists is never drawn, a label outside the table never stored)
    for (int f = 0; f < width; ++f) row[f] = 0.0f;
    out_label[e] = 0;
    out_smpw[e] = 0.0f;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) row[a] = xyz[i * 3 + a];
  for (int f = 0; f < nfeat; ++f) row[3 + f] = rgb[i * nfeat + f];
  out_label[e] = l;
  out_smpw[e] = (float)(labelweights[l] * (cat_mask[pos] ? 1.0 : 0.0));  // float64 weight *= mask, stored to a float32 batch
}

// ---- P:8-24 (+ P:71-89): one block of the batch per workgroup, in float64 as both loops hold the batch
constexpr int BN_TILE = 2048;  // rows per staged tile: 48 KiB of LDS

// P:19-21 of one block p (npoint,width) f32 by its workgroup: cen[] = per column the float64 chain / float64(npoint); -> m =
// max sqrt((x*x + y*y) + z*z) of the centred rows, in every thread.  It only reads p (its stores go to LDS).
__device__ __forceinline__ double block_centre_radius(int npoint, int width, const float* p, double* tile, double* cen, double* shm) {
  const int tid = threadIdx.x;
  double acc = -0.0;
  for (int base = 0; base < npoint; base += BN_TILE) {
    const int cnt = npoint - base < BN_TILE ? npoint - base : BN_TILE;
    for (int k = tid; k < cnt * 3; k += ST_THREADS) tile[k] = (double)p[(size_t)(base + k / 3) * width + k % 3];
    __syncthreads();
    if (tid < 3) acc = st_chain3(acc, tile, cnt, tid);
    __syncthreads();
  }
  if (tid < 3) cen[tid] = acc / (double)npoint;
  __syncthreads();
  double m = -__builtin_inf();
  for (int i = tid; i < npoint; i += ST_THREADS) {
    const double x = (double)p[(size_t)i * width] - cen[0], y = (double)p[(size_t)i * width + 1] - cen[1],
                 z = (double)p[(size_t)i * width + 2] - cen[2];
    m = nan_max(m, sqrt((x * x + y * y) + z * z));
  }
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) shm[tid >> 6] = m;
  __syncthreads();
  m = shm[0];
#pragma unroll
  for (int w = 1; w < ST_WAVES; ++w) m = nan_max(m, shm[w]);
  return m;
}

__global__ __launch_bounds__(ST_THREADS) void block_normalize_kernel(int npoint, int width, const float* __restrict__ src,
                                                                     const double* __restrict__ rot, float* __restrict__ batch) {
  __shared__ double tile[BN_TILE * 3];
  __shared__ double cen[3], shm[ST_WAVES];
  const int tid = threadIdx.x;
  const float* __restrict__ p = src + (size_t)blockIdx.x * npoint * width;
  float* __restrict__ out = batch + (size_t)blockIdx.x * npoint * width;
  const double m = block_centre_radius(npoint, width, p, tile, cen, shm);
  const bool turn = rot != nullptr;
  const double cosval = turn ? rot[blockIdx.x * 2] : 1.0, sinval = turn ? rot[blockIdx.x * 2 + 1] : 0.0;
  for (int i = tid; i < npoint; i += ST_THREADS) {
    const float* r = p + (size_t)i * width;
    float* o = out + (size_t)i * width;
    const double x = ((double)r[0] - cen[0]) / m, y = ((double)r[1] - cen[1]) / m, z = ((double)r[2] - cen[2]) / m;
    if (turn) {  // [x y z] @ [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] in float64, stored as float32
      o[0] = (float)(x * cosval + y * -sinval);
      o[1] = (float)(x * sinval + y * cosval);
    } else {
      o[0] = (float)x;  // the feed into a float32 placeholder
      o[1] = (float)y;
    }
    o[2] = (float)z;
    for (int f = 3; f < width; ++f) o[f] = r[f];
  }
}

// ---- T:253-254, the training order: rotate_point_cloud_z (P:71-89) on the float64 batch, its result ROUNDED TO FLOAT32
// (rotated_data is float32), then normalize_data (P:8-24) on that float32 block widened again.  One block per workgroup, one
// launch.  The rounded block is held in the output: a thread reads its own rows of src before it writes them (src == batch is
// allowed), and behind the barrier the workgroup reads back what it wrote.  z is carried: x*0 + y*0 + z*1 is z for finite
// input up to the sign of a zero, which the centroid subtraction removes unless the centroid is exactly zero.
__global__ __launch_bounds__(ST_THREADS) void block_train_batch_kernel(int npoint, int width, const float* src, const double* __restrict__ rot,
                                                                       float* batch) {
  __shared__ double tile[BN_TILE * 3];
  __shared__ double cen[3], shm[ST_WAVES];
  const int tid = threadIdx.x;
  const float* p = src + (size_t)blockIdx.x * npoint * width;
  float* out = batch + (size_t)blockIdx.x * npoint * width;
  const double cosval = rot[blockIdx.x * 2], sinval = rot[blockIdx.x * 2 + 1];
  for (int i = tid; i < npoint; i += ST_THREADS) {
    const float* r = p + (size_t)i * width;
    float* o = out + (size_t)i * width;
    const double x = (double)r[0], y = (double)r[1];
    const float ox = (float)(x * cosval + y * -sinval), oy = (float)(x * sinval + y * cosval);
    for (int f = width - 1; f >= 2; --f) o[f] = r[f];
    o[0] = ox;
    o[1] = oy;
  }
  __syncthreads();
  const double m = block_centre_radius(npoint, width, out, tile, cen, shm);  // (its last barrier is behind every read of out)
  for (int i = tid; i < npoint; i += ST_THREADS) {
    float* o = out + (size_t)i * width;
    const double x = ((double)o[0] - cen[0]) / m, y = ((double)o[1] - cen[1]) / m, z = ((double)o[2] - cen[2]) / m;
    o[0] = (float)x;
    o[1] = (float)y;
    o[2] = (float)z;
  }
}

// ---- what the validation score and the training score share: the prediction, one entry's cross-entropy, the partial sums
// np.argmax(pred_val, 2) of one row of c logits: the first maximum, the first NaN
__device__ __forceinline__ int score_argmax(const float* row, int c) {
  int a = 0;
  float best = row[0];
  bool nan = best != best;
  for (int q = 1; q < c && !nan; ++q) {
    const float v = row[q];
    if (v > best || v != v) { best = v; a = q; nan = v != v; }
  }
  return a;
}

// the cross-entropy of one row against label l: a float32 log-sum-exp
__device__ __forceinline__ float score_cross_entropy(const float* row, int c, int l) {
  float mx = row[0];
  for (int q = 1; q < c; ++q) mx = row[q] > mx ? row[q] : mx;
  float s = 0.0f;
  for (int q = 0; q < c; ++q) s += expf(row[q] - mx);
  return (logf(s) + mx) - row[l];
}

// A workgroup of 256: its threads' sums of w * ce and counts of w != 0 reduced over the lanes by shuffles into shs / shn [wave];
// its barrier is also behind every thread's LDS counting
__device__ __forceinline__ void score_reduce(double sum, int nz, double* shs, int* shn) {
  const int tid = threadIdx.x;
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    nz += __shfl_xor(nz, o, 64);
  }
  if ((tid & 63) == 0) { shs[tid >> 6] = sum; shn[tid >> 6] = nz; }
  __syncthreads();
}

// ... and the four waves in order into part_sum / part_cnt [blockIdx.x]
__device__ __forceinline__ void score_store(const double* shs, const int* shn, double* __restrict__ part_sum, long long* __restrict__ part_cnt) {
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ((shs[0] + shs[1]) + shs[2]) + shs[3];
    part_cnt[blockIdx.x] = ((shn[0] + shn[1]) + shn[2]) + shn[3];
  }
}

// ---- T:311-321, T:391-402: the counters (integers: exact and order-free) and the batch's weighted cross-entropy
// counters (2 + 4c) i64: total_correct, total_seen, then seen[c], correct[c], iou_deno[c], label histogram[c]
__global__ __launch_bounds__(256) void block_score_kernel(long entries, int c, const float* __restrict__ logits, const int* __restrict__ labels,
                                                          const float* __restrict__ smpw, long long* __restrict__ counters,
                                                          double* __restrict__ part_sum, long long* __restrict__ part_cnt) {
  __shared__ int cnt[2 + 4 * BT_CLASS_MAX];
  __shared__ double shs[4];
  __shared__ int shn[4];
  const int tid = threadIdx.x, ncnt = 2 + 4 * c;
  for (int k = tid; k < ncnt; k += 256) cnt[k] = 0;
  __syncthreads();
  double sum = 0.0;
  int nz = 0;
  for (long e = (long)blockIdx.x * 256 + tid; e < entries; e += (long)gridDim.x * 256) {
    const float* row = logits + (size_t)e * c;
    const int a = score_argmax(row, c);
    const int l = labels[e];
    const float w = smpw[e];
    if (l < 0 || l >= c) continue;
    atomicAdd(&cnt[2 + 3 * c + l], 1);  // np.histogram(batch_label, range(c + 1)): every entry
    if (w > 0.0f) {
      atomicAdd(&cnt[2 + l], 1);
      atomicAdd(&cnt[2 + 2 * c + l], 1);                // (pred == l) | (label == l), l = the label
      if (a == l) {
        atomicAdd(&cnt[2 + c + l], 1);
        if (l > 0) atomicAdd(&cnt[0], 1);
      } else {
        atomicAdd(&cnt[2 + 2 * c + a], 1);              // ..., l = the prediction
      }
      if (l > 0) atomicAdd(&cnt[1], 1);
    }
    if (w != 0.0f) {  // tf.losses.sparse_softmax_cross_entropy(weights=smpw): sum(w * ce) / count(w != 0)
      sum += (double)w * (double)score_cross_entropy(row, c, l);
      nz += 1;
    }
  }
  score_reduce(sum, nz, shs, shn);
  for (int k = tid; k < ncnt; k += 256)
    if (cnt[k]) atomicAdd((unsigned long long*)&counters[k], (unsigned long long)cnt[k]);
  score_store(shs, shn, part_sum, part_cnt);
}

// ---- T:264-272: the training tallies -- every entry counts, with no smpw > 0 and no label > 0 -- and the same loss
// counters (3) i64: total_correct, total_seen, total_iou_deno; sum_l ((pred == l) | (label == l)) is 1 for an entry whose
// prediction and label agree and 2 for one where they do not
__global__ __launch_bounds__(256) void block_train_score_kernel(long entries, int c, const float* __restrict__ logits,
                                                                const int* __restrict__ labels, const float* __restrict__ smpw,
                                                                long long* __restrict__ counters, double* __restrict__ part_sum,
                                                                long long* __restrict__ part_cnt) {
  __shared__ int cnt[2];
  __shared__ double shs[4];
  __shared__ int shn[4];
  const int tid = threadIdx.x;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  double sum = 0.0;
  int nz = 0, correct = 0, seen = 0;
  for (long e = (long)blockIdx.x * 256 + tid; e < entries; e += (long)gridDim.x * 256) {
    const float* row = logits + (size_t)e * c;
    const int a = score_argmax(row, c);
    const int l = labels[e];
    const float w = smpw[e];
    if (l < 0 || l >= c) continue;
    seen += 1;
    correct += a == l;
    if (w != 0.0f) {
      sum += (double)w * (double)score_cross_entropy(row, c, l);
      nz += 1;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    correct += __shfl_xor(correct, o, 64);
    seen += __shfl_xor(seen, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicAdd(&cnt[0], correct);
    atomicAdd(&cnt[1], seen);
  }
  score_reduce(sum, nz, shs, shn);
  score_store(shs, shn, part_sum, part_cnt);
  if (tid == 0 && cnt[1]) {
    atomicAdd((unsigned long long*)&counters[0], (unsigned long long)cnt[0]);
    atomicAdd((unsigned long long*)&counters[1], (unsigned long long)cnt[1]);
    atomicAdd((unsigned long long*)&counters[2], (unsigned long long)(2 * cnt[1] - cnt[0]));
  }
}

// the partial sums in workgroup order: loss[1] = the batch's classify loss, loss[0] += it
__global__ __launch_bounds__(64) void block_loss_kernel(int groups, const double* __restrict__ part_sum, const long long* __restrict__ part_cnt,
                                                        double* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  long long nz = 0;
  for (int g = 0; g < groups; ++g) { sum += part_sum[g]; nz += part_cnt[g]; }
  const double v = nz > 0 ? sum / (double)nz : 0.0;
  loss[1] = v;
  loss[0] += v;
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_block_key_capacity(void) { return BT_KEYS; }

extern "C" int pasnl_block_crop_stats(long n, const float* xyz, const int* labels, const float* bounds, long centre, long long key_lo,
                                      long span, int* hist, unsigned int* bitmap, int* out_stats, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && centre >= 0 && centre < n && span > 0, PASNL_EINVAL);
  PASNL_REQUIRE(span <= BT_KEYS, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && labels && bounds && hist && bitmap && out_stats, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long nchunks = wt_chunks(n);
  const int words = (int)((span + 31) / 32);
  const unsigned groups = wt_blocks(nchunks, COL_WAVES) < (unsigned)BT_MAX_GROUPS ? wt_blocks(nchunks, COL_WAVES) : (unsigned)BT_MAX_GROUPS;
  if (hipMemsetAsync(bitmap, 0, (size_t)(1 + words) * sizeof(unsigned), s) != hipSuccess) return PASNL_ELAUNCH;
  const int rc = launch(block_crop_stats_kernel, dim3(groups), dim3(64 * COL_WAVES), (size_t)words * sizeof(unsigned), s, n, xyz, labels, bounds,
                        centre, (double)key_lo, words, nchunks, hist, bitmap);
  if (rc != PASNL_OK) return rc;
  hipLaunchKernelGGL(window_scan_kernel, dim3(2), dim3(256), 0, s, nchunks, hist, out_stats);
  hipLaunchKernelGGL(block_unique_kernel, dim3(1), dim3(256), 0, s, words, bitmap, out_stats);
  return pasnl_launch_status();
}

extern "C" int pasnl_block_grid_count(long n, const float* xyz, const float* bounds, int nx, int ny, int* hist, int* out_counts,
                                      pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0, PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && out_counts, PASNL_ENULL);
  return wt_count(n, xyz, bounds, block_grid(-1, nx, ny), hist, out_counts, pasnl_hip_stream(stream));
}

extern "C" int pasnl_block_fill(long n, const float* xyz, const float* bounds, long centre, int nx, int ny, const int* hist, const int* woff,
                                long cap, int* out_idx, unsigned char* out_mask, pasnl_stream_t stream) {
  PASNL_REQUIRE(n > 0 && n <= (1L << 30) && nx > 0 && ny > 0 && cap > 0 && centre < n && (centre < 0 || (nx == 1 && ny == 1)),
                PASNL_EINVAL);
  PASNL_REQUIRE(wt_grid_ok(nx, ny), PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(xyz && bounds && hist && woff && out_idx && out_mask, PASNL_ENULL);
  return wt_fill(n, xyz, bounds, block_grid(centre, nx, ny), centre, BT_HALF, hist, woff, cap, out_idx, out_mask, pasnl_hip_stream(stream));
}

extern "C" int pasnl_block_gather(int rows, int block_points, const int* rowpos, long cap, const int* cat_idx, const unsigned char* cat_mask,
                                  long n, const float* xyz, const float* rgb, int nfeat, const int* labels, int c, const double* labelweights,
                                  float* out_data, int* out_label, float* out_smpw, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && nfeat >= 0 && n > 0 && cap > 0 && c >= 1, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(rowpos && cat_idx && cat_mask && xyz && labels && labelweights && out_data && out_label && out_smpw && (nfeat == 0 || rgb),
                PASNL_ENULL);
  const long entries = (long)rows * block_points;
  hipLaunchKernelGGL(block_gather_kernel, dim3(wt_blocks(entries, 256)), dim3(256), 0, pasnl_hip_stream(stream), entries, rowpos, cap, cat_idx,
                     cat_mask, n, xyz, rgb, nfeat, labels, c, labelweights, out_data, out_label, out_smpw);
  return pasnl_launch_status();
}

extern "C" int pasnl_block_normalize(int rows, int block_points, int width, const float* src, const double* rot, float* batch,
                                     pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && width >= 3, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(src && batch, PASNL_ENULL);
  hipLaunchKernelGGL(block_normalize_kernel, dim3(rows), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), block_points, width, src, rot, batch);
  return pasnl_launch_status();
}

extern "C" int pasnl_block_train_batch(int rows, int block_points, int width, const float* src, const double* rot, float* batch,
                                       pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && width >= 3, PASNL_EINVAL);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(src && rot && batch, PASNL_ENULL);
  hipLaunchKernelGGL(block_train_batch_kernel, dim3(rows), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), block_points, width, src, rot, batch);
  return pasnl_launch_status();
}

extern "C" size_t pasnl_block_score_workspace_bytes(void) { return (size_t)BT_SCORE_GROUPS * (sizeof(double) + sizeof(long long)); }

// the validation score and the training score: one counting kernel over the entries, then the partial sums in order
template <typename Kernel>
static int score_launch(Kernel kernel, int rows, int block_points, int c, const float* logits, const int* labels, const float* smpw,
                        long long* counters, double* loss, void* workspace, pasnl_stream_t stream) {
  PASNL_REQUIRE(rows >= 0 && block_points > 0 && c >= 1, PASNL_EINVAL);
  PASNL_REQUIRE(c <= BT_CLASS_MAX, PASNL_EUNSUPPORTED);
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && labels && smpw && counters && loss && workspace, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const long entries = (long)rows * block_points;
  const int groups = wt_blocks(entries, 256) < (unsigned)BT_SCORE_GROUPS ? (int)wt_blocks(entries, 256) : BT_SCORE_GROUPS;
  double* part_sum = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_sum + BT_SCORE_GROUPS);
  hipLaunchKernelGGL(kernel, dim3(groups), dim3(256), 0, s, entries, c, logits, labels, smpw, counters, part_sum, part_cnt);
  hipLaunchKernelGGL(block_loss_kernel, dim3(1), dim3(64), 0, s, groups, part_sum, part_cnt, loss);
  return pasnl_launch_status();
}

extern "C" int pasnl_block_score(int rows, int block_points, int c, const float* logits, const int* labels, const float* smpw,
                                 long long* counters, double* loss, void* workspace, pasnl_stream_t stream) {
  return score_launch(block_score_kernel, rows, block_points, c, logits, labels, smpw, counters, loss, workspace, stream);
}

extern "C" int pasnl_block_train_score(int rows, int block_points, int c, const float* logits, const int* labels, const float* smpw,
                                       long long* counters, double* loss, void* workspace, pasnl_stream_t stream) {
  return score_launch(block_train_score_kernel, rows, block_points, c, logits, labels, smpw, counters, loss, workspace, stream);
}
