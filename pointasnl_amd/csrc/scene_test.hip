// The ScanNet grid test and validation loops around the forward, on the device: reference ScanNet/scannet_dataset_grid.py
// (D) :435-549 `get_batch_gen('test' | 'validation')` -- pick the least-visited point, move it by Gaussian noise, crop
// around that float64 position, raise the potentials of what the crop covered -- and ScanNet/test_scannet_grid.py (T)
// :95-229 / :231-448 -- smooth the votes into a float32 table of C - 1 classes, reproject onto the mesh vertices, score
// with confusion matrices.  The sibling of scan_test.hip (SemanticKITTI); what the two share is test_loop.hpp.  Everything
// that has to equal numpy is done in numpy's dtypes and order (the library builds with -ffp-contract=off); the exactness
// contract is stated in include/pasnl.h per entry point and restated on the host in tests/scene_flow_ref.py.
//
// One crop is a chain of TEN launches on one stream: pasnl_scene_pick_crop (crop.hip: the pick fused into the radix
// selection's init, then its five passes, count and write) -> pasnl_scene_order_gather -> pasnl_scene_potential_update.
// The descriptor (pasnl_scene_crop_t, a float64 centre) carries the pick from kernel to kernel; the RNG draws (noise,
// buffer, shuffle) depend only on lengths the host knows and are drawn there, in the reference's order.
//
// Last-write-wins (numpy fancy-index assignment with repeated indices) uses the `win` scratch as scan_test.hip does.
#include <math.h>
#include "common.hpp"
#include "test_loop.hpp"
#include "window_scan.hpp"

namespace pasnl {

static_assert(sizeof(pasnl_scene_crop_t) == 48, "the descriptor layout is part of the ABI (scene_tester.DESC_BYTES)");

// ---- order / permute / gather: one workgroup per crop
__global__ __launch_bounds__(ST_THREADS) void scene_order_gather_kernel(const pasnl_scene_crop_t* __restrict__ desc,
                                                                        const float* __restrict__ points,
                                                                        const float* __restrict__ colors, const int* __restrict__ idx,
                                                                        const double* __restrict__ d2, int kcap,
                                                                        const int* __restrict__ perm, int num_point, int nfeat,
                                                                        int abs_coords, int* __restrict__ out_select,
                                                                        float* __restrict__ out_input) {
  __shared__ unsigned long long key[OP_CAP];
  __shared__ unsigned short pos[OP_CAP];
  const int c = blockIdx.x, tid = threadIdx.x;
  const pasnl_scene_crop_t d = desc[c];
  int m = d.k < kcap ? d.k : kcap;
  m = m < d.n ? m : d.n;  // the count the selection wrote
  const int* ic = idx + (size_t)c * kcap;
  const double* dc = d2 + (size_t)c * kcap;
  for (int i = tid; i < m; i += ST_THREADS) {
    key[i] = (unsigned long long)__double_as_longlong(dc[i]);
    pos[i] = (unsigned short)i;
  }
  __syncthreads();
  op_sort(key, pos, m);
  const int width = 3 + nfeat + (abs_coords ? 3 : 0);
  const int* pc = perm + (size_t)c * num_point;
  int* os = out_select + (size_t)c * num_point;
  float* oi = out_input + (size_t)c * num_point * width;
  const float* sp = points + (size_t)d.offset * 3;
  const float* sc = colors ? colors + (size_t)d.offset * nfeat : nullptr;
  const double ctr[3] = {d.cx, d.cy, d.cz};
  for (int j = tid; j < num_point; j += ST_THREADS) {
    int q = pc[j];
    q = q < 0 ? 0 : (q >= m ? m - 1 : q);  // (the host draws a permutation of [0, k): never taken)
    const int sel = m > 0 ? ic[pos[q]] : 0;
    os[j] = sel;
    float* row = oi + (size_t)j * width;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float x = (float)((double)sp[(size_t)sel * 3 + a] - ctr[a]);  // (points[input_inds] - pick_point).astype(float32)
      row[a] = x;
      if (abs_coords) row[3 + nfeat + a] = (float)((double)x + ctr[a]);   // float32(input_points + pick_point), D:539
    }
    for (int f = 0; f < nfeat; ++f) row[3 + f] = sc[(size_t)sel * nfeat + f];
  }
}

// ---- potential update: one workgroup does max(dists), the update and the scene's new minimum
__device__ __forceinline__ float sc_dist(const float* __restrict__ p, const pasnl_scene_crop_t& d) {
  const float dx = (float)((double)p[0] - d.cx), dy = (float)((double)p[1] - d.cy), dz = (float)((double)p[2] - d.cz);
  return (dx * dx + dy * dy) + dz * dz;  // np.sum(np.square(.astype(float32)), axis=1)
}

__global__ __launch_bounds__(ST_THREADS) void scene_update_kernel(int num_point, const pasnl_scene_crop_t* __restrict__ desc,
                                                                  const float* __restrict__ points, const int* __restrict__ select,
                                                                  double* __restrict__ potentials, double* __restrict__ min_potentials,
                                                                  int* __restrict__ win) {
  __shared__ float shf[ST_WAVES];
  __shared__ double shd[ST_WAVES];
  const pasnl_scene_crop_t d = *desc;
  const float* sp = points + (size_t)d.offset * 3;
  float m = -__builtin_inff();
  for (int j = threadIdx.x; j < num_point; j += ST_THREADS) {
    const int i = select[j];
    m = nan_max(m, sc_dist(sp + (size_t)i * 3, d));
    atomicMax(&win[i], j);
  }
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = m;
  __syncthreads();  // (also orders the atomics on win in front of the loads below)
  m = shf[0];
  for (int w = 1; w < ST_WAVES; ++w) m = nan_max(m, shf[w]);
  double* pot = potentials + d.offset;
  for (int j = threadIdx.x; j < num_point; j += ST_THREADS) {
    const int i = select[j];
    if (__hip_atomic_load(&win[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) continue;
    float delta = 1.0f - sc_dist(sp + (size_t)i * 3, d) / m;
    delta = delta * delta;
    pot[i] = pot[i] + (double)delta;
    __hip_atomic_store(&win[i], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();  // the workgroup's own stores are visible to it: the minimum reads the updated potentials
  const double mn = st_min(pot, d.n, shd);
  if (threadIdx.x == 0) min_potentials[d.cloud] = mn;
}

// ---- votes: crop `c` of the batch, float32 table of nc = C - 1 classes (the mark is test_loop.hpp's vote_mark_kernel)
constexpr int SV_MAXC = 64;

__global__ __launch_bounds__(256) void scene_vote_apply_kernel(int num_point, int nc, const float* __restrict__ values, int is_logits,
                                                               const int* __restrict__ select, const int* __restrict__ cloud,
                                                               const long long* __restrict__ offsets, float smooth_old,
                                                               float smooth_new, float* __restrict__ test_probs, int* __restrict__ win) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= num_point) return;
  const int i = select[j];
  if (__hip_atomic_load(&win[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) return;
  float p[SV_MAXC];
  if (is_logits) {  // tf.nn.softmax(pred[:, :, 1:]): rows of nc + 1 logits, column 0 dropped
    vote_softmax(values + (size_t)j * (nc + 1) + 1, nc, p);
  } else {
    const float* v = values + (size_t)j * nc;
    for (int q = 0; q < nc; ++q) p[q] = v[q];
  }
  float* row = test_probs + ((size_t)offsets[*cloud] + (size_t)i) * (size_t)nc;  // 64-bit: the table may exceed 2^31 entries
  for (int q = 0; q < nc; ++q) {
    const float a = smooth_old * row[q], b = smooth_new * p[q];  // two float32 products, one float32 sum (not contracted)
    row[q] = a + b;
  }
  __hip_atomic_store(&win[i], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- reprojection outputs
constexpr int SL_MAXL = 64;

__global__ __launch_bounds__(256) void scene_labels_kernel(long m, const int* __restrict__ proj, const float* __restrict__ probs, int nc,
                                                           const double* __restrict__ potentials, const int* __restrict__ label_values,
                                                           const int* __restrict__ ignored, int nl, int* __restrict__ out_preds,
                                                           double* __restrict__ out_pots, float* __restrict__ out_probs) {
  __shared__ int lv[SL_MAXL], ig[SL_MAXL];
  if (threadIdx.x < nl) { lv[threadIdx.x] = label_values[threadIdx.x]; ig[threadIdx.x] = ignored[threadIdx.x]; }
  __syncthreads();
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const long r = proj ? (long)proj[j] : j;
  const float* row = probs + (size_t)r * nc;
  int a = 0, q = 0;
  float best = 0.0f;
  bool nan = false;
  for (int l = 0; l < nl; ++l) {  // np.argmax over the row with a zero at every ignored label: the first maximum, the first NaN
    const float v = ig[l] ? 0.0f : row[q];
    if (!ig[l]) {
      if (out_probs) out_probs[(size_t)j * nc + q] = v;
      ++q;
    }
    if (!nan && (l == 0 || v > best || v != v)) { best = v; a = l; nan = v != v; }
  }
  out_preds[j] = lv[a];
  if (out_pots) out_pots[j] = potentials[r];
}

// ---- confusion matrix: per-workgroup counters in LDS, one flush
constexpr int CM_MAXL = 64;
constexpr int CM_BLOCKS = 512;

__global__ __launch_bounds__(256) void confusion_kernel(long n, const int* __restrict__ targets, const int* __restrict__ preds,
                                                        const int* __restrict__ label_values, int nl,
                                                        unsigned long long* __restrict__ out) {
  extern __shared__ unsigned cm[];  // nl * nl counters, then nl label values
  int* lv = reinterpret_cast<int*>(cm + nl * nl);
  for (int i = threadIdx.x; i < nl * nl; i += 256) cm[i] = 0u;
  if (threadIdx.x < nl) lv[threadIdx.x] = label_values[threadIdx.x];
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {  // < 2^32 points per workgroup
    const int t = targets[i], p = preds[i];
    int ti = -1, pi = -1;
    for (int l = 0; l < nl; ++l) {
      ti = lv[l] == t ? l : ti;
      pi = lv[l] == p ? l : pi;
    }
    if (ti >= 0 && pi >= 0) atomicAdd(&cm[ti * nl + pi], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nl * nl; i += 256) {
    const unsigned v = cm[i];
    if (v != 0u) atomicAdd(&out[i], (unsigned long long)v);
  }
}

}  // namespace pasnl

using namespace pasnl;


extern "C" int pasnl_scene_order_gather(int b, const pasnl_scene_crop_t* desc, const float* points, const float* colors, int nfeat,
                                        const int* idx, const double* d2, int kcap, const int* perm, int num_point, int abs_coords,
                                        int* out_select, float* out_input, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && kcap > 0 && num_point > 0 && nfeat >= 0, PASNL_EINVAL);
  PASNL_REQUIRE(kcap <= OP_CAP, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(desc && points && idx && d2 && perm && out_select && out_input && (nfeat == 0 || colors), PASNL_ENULL);
  hipLaunchKernelGGL(scene_order_gather_kernel, dim3(b), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), desc, points,
                     nfeat > 0 ? colors : nullptr, idx, d2, kcap, perm, num_point, nfeat, abs_coords, out_select, out_input);
  return pasnl_launch_status();
}

extern "C" int pasnl_scene_potential_update(int num_point, const pasnl_scene_crop_t* desc, const float* points, const int* select,
                                            double* potentials, double* min_potentials, int* win, pasnl_stream_t stream) {
  PASNL_REQUIRE(num_point > 0, PASNL_EINVAL);
  PASNL_REQUIRE(desc && points && select && potentials && min_potentials && win, PASNL_ENULL);
  hipLaunchKernelGGL(scene_update_kernel, dim3(1), dim3(ST_THREADS), 0, pasnl_hip_stream(stream), num_point, desc, points, select,
                     potentials, min_potentials, win);
  return pasnl_launch_status();
}

extern "C" int pasnl_scene_vote(int b, int num_point, int nc, const float* values, int is_logits, const int* select, const int* cloud,
                                const long long* offsets, float smooth_old, float smooth_new, float* test_probs, int* win,
                                pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && num_point > 0 && nc > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nc <= SV_MAXC, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(values && select && cloud && offsets && test_probs && win, PASNL_ENULL);
  hipStream_t s = pasnl_hip_stream(stream);
  const unsigned g = wt_blocks(num_point, 256);
  const size_t width = (size_t)(is_logits ? nc + 1 : nc);
  for (int i = 0; i < b; ++i) {  // crop after crop: a later crop of the batch smooths what the earlier one wrote
    const int* sel = select + (size_t)i * num_point;
    hipLaunchKernelGGL(vote_mark_kernel, dim3(g), dim3(256), 0, s, num_point, sel, win);
    hipLaunchKernelGGL(scene_vote_apply_kernel, dim3(g), dim3(256), 0, s, num_point, nc, values + (size_t)i * num_point * width,
                       is_logits, sel, cloud + i, offsets, smooth_old, smooth_new, test_probs, win);
  }
  return pasnl_launch_status();
}

extern "C" int pasnl_scene_labels(long m, const int* proj, const float* probs, int nc, const double* potentials,
                                  const int* label_values, const int* ignored, int nl, int* out_preds, double* out_pots,
                                  float* out_probs, pasnl_stream_t stream) {
  PASNL_REQUIRE(m >= 0 && nc > 0 && nl > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nl <= SL_MAXL, PASNL_EUNSUPPORTED);
  if (m == 0) return PASNL_OK;
  PASNL_REQUIRE(probs && label_values && ignored && out_preds && (potentials || !out_pots), PASNL_ENULL);
  hipLaunchKernelGGL(scene_labels_kernel, dim3(wt_blocks(m, 256)), dim3(256), 0, pasnl_hip_stream(stream), m, proj, probs, nc,
                     potentials, label_values, ignored, nl, out_preds, out_pots, out_probs);
  return pasnl_launch_status();
}

extern "C" int pasnl_confusion_matrix(long n, const int* targets, const int* preds, const int* label_values, int nl, long long* out,
                                      pasnl_stream_t stream) {
  PASNL_REQUIRE(n >= 0 && nl > 0, PASNL_EINVAL);
  PASNL_REQUIRE(nl <= CM_MAXL, PASNL_EUNSUPPORTED);
  if (n == 0) return PASNL_OK;
  PASNL_REQUIRE(targets && preds && label_values && out, PASNL_ENULL);
  const unsigned blocks = wt_blocks(n, 256 * 16);
  hipLaunchKernelGGL(confusion_kernel, dim3(blocks < (unsigned)CM_BLOCKS ? blocks : (unsigned)CM_BLOCKS), dim3(256),
                     (size_t)(nl * nl + nl) * 4, pasnl_hip_stream(stream), n, targets, preds, label_values, nl,
                     reinterpret_cast<unsigned long long*>(out));
  return pasnl_launch_status();
}
