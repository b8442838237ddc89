// The per-epoch evaluation of the two grid pipelines on the device: `eval_one_epoch` of ScanNet/train_scannet_grid.py (S)
// :304-434 -- the chopped evaluation, the persistent float64 table `validation_probs` smoothed with val_smooth, the voting
// evaluation through validation_proj -- and of SemanticKITTI/train_semantic_kitti_grid.py (K) :265-330.  The generators are
// scene_test.hip's and grid_train.hip's; what is here is what the evaluation does with the model's output:
//
//   pasnl_scan_eval_confusion        softmax, argmax with the ignored columns inserted and the per-crop confusions of a whole
//                                    batch, summed (S:359-368, K:301-310): one launch
//   pasnl_scene_eval_vote            the smoothing of S:346-351 into the float64 table: two launches per crop
//   pasnl_scene_eval_vote_confusion  S:396-410 for one scene: argmax per sub-sampled point, then the confusion of the
//                                    reprojected predictions: two launches
//
// A thread owns a row of up to 65 values.  Read straight from global memory every lane would walk its own 84-byte stride,
// and a private `p[64]` under run-time indices lives in scratch; so a workgroup stages a tile of GE_ROWS rows into LDS with
// coalesced loads and each thread takes max, sum and argmax from its LDS row in passes (expf is recomputed: the same
// function on the same argument, the same bits).  The LDS row stride is padded to an odd number of words (dwords for
// float rows: ds_read_b32 banks are (a/4) % 32; 8-byte words for double rows: ds_read_b64 banks are (a/4) % 64 over a
// 32-lane half), so the row-per-lane reads of a pass hit distinct banks.  Confusion counters sit in LDS and are flushed once
// per workgroup with 64-bit integer atomics (exact and order-free); there is no floating-point atomic.  The library builds
// with -ffp-contract=off: the smoothing's two products and its sum are three roundings, as numpy's are.
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"
#include "window_scan.hpp"

namespace pasnl {

constexpr int GE_ROWS = 256;    // rows of a tile = threads of a workgroup
constexpr int GE_MAXL = 64;     // label values (the ignored mask is one 64-bit word)
constexpr int GE_BLOCKS = 512;  // workgroups of the counting kernels (each flushes nl * nl counters once)

// rows [0, cnt) of a row-major (cnt, w) array -> LDS at row stride ws; consecutive threads load consecutive elements
template <typename T>
__device__ __forceinline__ void ge_stage(const T* __restrict__ g, int cnt, int w, int ws, T* tile) {
  const int total = cnt * w, dr = GE_ROWS / w, dc = GE_ROWS % w;
  int row = (int)threadIdx.x / w, col = (int)threadIdx.x % w;
  for (int e = threadIdx.x; e < total; e += GE_ROWS) {
    tile[row * ws + col] = g[e];
    row += dr;
    col += dc;
    if (col >= w) { col -= w; ++row; }
  }
}

// np.argmax over the row with a zero inserted at every l whose bit of `ig` is set: the first maximum, the first NaN
// (scene_labels_kernel's rule).  value(q): column q of the table row; nc + popcount(ig) == nl is the caller's.
template <typename T, typename F>
__device__ __forceinline__ int ge_argmax(unsigned long long ig, int nl, F value) {
  int a = 0, q = 0;
  T best = (T)0;
  bool nan = false;
  for (int l = 0; l < nl; ++l) {
    const bool g = (ig >> l) & 1ull;
    const T v = g ? (T)0 : value(q);
    q += g ? 0 : 1;
    if (!nan && (l == 0 || v > best || v != v)) { best = v; a = l; nan = v != v; }
  }
  return a;
}

// ---- the per-crop confusions of a batch: rows = b * num_point
__global__ __launch_bounds__(GE_ROWS) void eval_confusion_kernel(long rows, int nc, const float* __restrict__ values, int is_logits,
                                                                 const int* __restrict__ truth, unsigned long long ig, int nl,
                                                                 unsigned long long* __restrict__ out) {
  extern __shared__ unsigned ge_cm[];  // nl * nl counters, then the tile
  float* tile = reinterpret_cast<float*>(ge_cm + nl * nl);
  const int w = is_logits ? nc + 1 : nc, ws = w | 1, skip = is_logits ? 1 : 0;
  for (int i = threadIdx.x; i < nl * nl; i += GE_ROWS) ge_cm[i] = 0u;
  __syncthreads();
  const long ntiles = (rows + GE_ROWS - 1) / GE_ROWS;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long r0 = t * GE_ROWS;
    const int cnt = rows - r0 < GE_ROWS ? (int)(rows - r0) : GE_ROWS;
    ge_stage(values + (size_t)r0 * w, cnt, w, ws, tile);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const float* v = tile + threadIdx.x * ws + skip;  // tf.nn.softmax(pred[:, :, 1:]): column 0 dropped
      int a;
      if (is_logits) {
        float m, s;
        vote_softmax_max_sum(v, nc, m, s);
        a = ge_argmax<float>(ig, nl, [&](int q) { return vote_softmax_term(v[q], m) / s; });
      } else {
        a = ge_argmax<float>(ig, nl, [&](int q) { return v[q]; });
      }
      const int tr = truth[r0 + threadIdx.x];
      if (tr >= 0 && tr < nl) atomicAdd(&ge_cm[tr * nl + a], 1u);
    }
    __syncthreads();  // the next tile overwrites this one
  }
  for (int i = threadIdx.x; i < nl * nl; i += GE_ROWS) {
    const unsigned v = ge_cm[i];
    if (v != 0u) atomicAdd(&out[i], (unsigned long long)v);
  }
}

// ---- the smoothing of one crop into the float64 table (the mark is test_loop.hpp's vote_mark_kernel)
__global__ __launch_bounds__(GE_ROWS) void eval_vote_apply_kernel(int num_point, int nc, const float* __restrict__ values, int is_logits,
                                                                  const int* __restrict__ select, const int* __restrict__ cloud,
                                                                  const long long* __restrict__ offsets, double smooth_old,
                                                                  float smooth_new, double* __restrict__ val_probs,
                                                                  int* __restrict__ win) {
  extern __shared__ float ge_tile[];
  const int w = is_logits ? nc + 1 : nc, ws = w | 1, skip = is_logits ? 1 : 0;
  const int r0 = blockIdx.x * GE_ROWS;
  const int cnt = num_point - r0 < GE_ROWS ? num_point - r0 : GE_ROWS;
  ge_stage(values + (size_t)r0 * w, cnt, w, ws, ge_tile);
  __syncthreads();
  if ((int)threadIdx.x >= cnt) return;
  const int j = r0 + threadIdx.x;
  const int i = select[j];
  if (__hip_atomic_load(&win[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) return;
  const float* v = ge_tile + threadIdx.x * ws + skip;
  float m = 0.0f, s = 1.0f;
  if (is_logits) vote_softmax_max_sum(v, nc, m, s);
  double* row = val_probs + ((size_t)offsets[*cloud] + (size_t)i) * (size_t)nc;  // 64-bit: the table may exceed 2^31 entries
  for (int q = 0; q < nc; ++q) {
    const float p = is_logits ? vote_softmax_term(v[q], m) / s : v[q];
    const float b = smooth_new * p;        // (1 - val_smooth) * probs: a float32 product (numpy >= 2: the Python float is weak)
    const double a = smooth_old * row[q];  // val_smooth * validation_probs[c_i][inds]: a float64 product
    row[q] = a + (double)b;
  }
  __hip_atomic_store(&win[i], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the voting evaluation of one scene: argmax per sub-sampled point ...
__global__ __launch_bounds__(GE_ROWS) void eval_sub_preds_kernel(long n, const double* __restrict__ probs, int nc, unsigned long long ig,
                                                                 int nl, int* __restrict__ sub_preds) {
  extern __shared__ double ge_dtile[];
  const int ws = nc | 1;
  const long r0 = (long)blockIdx.x * GE_ROWS;
  const int cnt = n - r0 < GE_ROWS ? (int)(n - r0) : GE_ROWS;
  ge_stage(probs + (size_t)r0 * nc, cnt, nc, ws, ge_dtile);
  __syncthreads();
  if ((int)threadIdx.x >= cnt) return;
  const double* v = ge_dtile + threadIdx.x * ws;
  sub_preds[r0 + threadIdx.x] = ge_argmax<double>(ig, nl, [&](int q) { return v[q]; });
}

// ... and the confusion of the predictions reprojected onto the m evaluation points
__global__ __launch_bounds__(GE_ROWS) void eval_vote_confusion_kernel(long m, const int* __restrict__ proj, const int* __restrict__ labels,
                                                                      const int* __restrict__ label_values, int nl, long n,
                                                                      const int* __restrict__ sub_preds,
                                                                      unsigned long long* __restrict__ out) {
  extern __shared__ unsigned ge_vcm[];  // nl * nl counters, then nl label values
  int* lv = reinterpret_cast<int*>(ge_vcm + nl * nl);
  for (int i = threadIdx.x; i < nl * nl; i += GE_ROWS) ge_vcm[i] = 0u;
  if ((int)threadIdx.x < nl) lv[threadIdx.x] = label_values[threadIdx.x];
  __syncthreads();
  for (long j = (long)blockIdx.x * GE_ROWS + threadIdx.x; j < m; j += (long)gridDim.x * GE_ROWS) {  // < 2^32 points per workgroup
    const long r = proj ? (long)proj[j] : j;
    if (r < 0 || r >= n) continue;
    const int t = labels[j], p = sub_preds[r];
    int ti = -1;
    for (int l = 0; l < nl; ++l) ti = lv[l] == t ? l : ti;
    if (ti >= 0 && p >= 0 && p < nl) atomicAdd(&ge_vcm[ti * nl + p], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nl * nl; i += GE_ROWS) {
    const unsigned v = ge_vcm[i];
    if (v != 0u) atomicAdd(&out[i], (unsigned long long)v);
  }
}

// the ignored flags as one word; false if nc + their number != nl
static bool ge_ignored_mask(const int* ignored, int nl, int nc, unsigned long long* mask) {
  unsigned long long g = 0ull;
  int cnt = 0;
  for (int l = 0; l < nl; ++l)
    if (ignored[l] != 0) { g |= 1ull << l; ++cnt; }
  *mask = g;
  return nc + cnt == nl;
}

}  // namespace pasnl

using namespace pasnl;

static inline unsigned ge_count_blocks(long n) {
  const unsigned blocks = wt_blocks(n, GE_ROWS);
  return blocks < (unsigned)GE_BLOCKS ? blocks : (unsigned)GE_BLOCKS;
}

extern "C" int pasnl_scan_eval_confusion(int b, int num_point, int nc, const float* values, int is_logits, const int* truth,
                                         const int* ignored, int nl, long long* out, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && b <= 65535 && num_point > 0 && nc > 0 && nl > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nl <= GE_MAXL, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(values && truth && ignored && out, PASNL_ENULL);
  unsigned long long ig;  // ignored: nl ints in HOST memory, read here
  PASNL_REQUIRE(ge_ignored_mask(ignored, nl, nc, &ig), PASNL_EINVAL);
  const long rows = (long)b * num_point;
  const int ws = (is_logits ? nc + 1 : nc) | 1;
  const int rc = launch(eval_confusion_kernel, dim3(ge_count_blocks(rows)), dim3(GE_ROWS), (size_t)(nl * nl + GE_ROWS * ws) * 4,
                        pasnl_hip_stream(stream), rows, nc, values, is_logits, truth, ig, nl, reinterpret_cast<unsigned long long*>(out));
  return rc != PASNL_OK ? rc : pasnl_launch_status();
}

extern "C" int pasnl_scene_eval_vote(int b, int num_point, int nc, const float* values, int is_logits, const int* select,
                                     const int* cloud, const long long* offsets, double smooth_old, float smooth_new,
                                     double* val_probs, int* win, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && num_point > 0 && nc > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nc <= GE_MAXL, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(values && select && cloud && offsets && val_probs && win, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const unsigned g = wt_blocks(num_point, GE_ROWS);
  const size_t width = (size_t)(is_logits ? nc + 1 : nc);
  const size_t lds = (size_t)GE_ROWS * (width | 1) * 4;
  for (int i = 0; i < b; ++i) {  // crop after crop: a later crop of the batch smooths what the earlier one wrote
    const int* sel = select + (size_t)i * num_point;
    hipLaunchKernelGGL(vote_mark_kernel, dim3(g), dim3(256), 0, s, num_point, sel, win);
    const int rc = launch(eval_vote_apply_kernel, dim3(g), dim3(GE_ROWS), lds, s, num_point, nc, values + (size_t)i * num_point * width,
                          is_logits, sel, cloud + i, offsets, smooth_old, smooth_new, val_probs, win);
    if (rc != PASNL_OK) return rc;
  }
  return pasnl_launch_status();
}

extern "C" int pasnl_scene_eval_vote_confusion(long n, const double* probs, int nc, long m, const int* proj, const int* labels,
                                               const int* label_values, const int* ignored, int nl, int* sub_preds, long long* out,
                                               pasnl_stream_t stream) {
  PASNL_REQUIRE(n >= 0 && m >= 0 && nc > 0 && nl > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nl <= GE_MAXL, PASNL_EUNSUPPORTED);
  if (n == 0) return PASNL_OK;  // no sub-sampled point: every proj[j] is outside [0, 0)
  PASNL_REQUIRE(probs && ignored && sub_preds && (m == 0 || (labels && label_values && out)), PASNL_ENULL);
  unsigned long long ig;  // ignored: nl ints in HOST memory, read here
  PASNL_REQUIRE(ge_ignored_mask(ignored, nl, nc, &ig), PASNL_EINVAL);
  hipStream_t s = pasnl_hip_stream(stream);
  const int rc = launch(eval_sub_preds_kernel, dim3(wt_blocks(n, GE_ROWS)), dim3(GE_ROWS), (size_t)GE_ROWS * (nc | 1) * 8, s, n, probs, nc,
                        ig, nl, sub_preds);
  if (rc != PASNL_OK) return rc;
  if (m > 0) {
    hipLaunchKernelGGL(eval_vote_confusion_kernel, dim3(ge_count_blocks(m)), dim3(GE_ROWS), (size_t)(nl * nl + nl) * 4, s, m, proj, labels,
                       label_values, nl, n, sub_preds, reinterpret_cast<unsigned long long*>(out));
  }
  return pasnl_launch_status();
}
