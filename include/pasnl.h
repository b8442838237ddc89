/*
 * pasnl.h -- C ABI of libpasnl_hip.so: the MI355X (gfx950) set-abstraction hot path of PointASNL.
 *
 * This is the drop-in boundary.  Every entry point replaces one C++ "Launcher" (or CPU loop) that the
 * reference's TensorFlow OpKernels call with raw pointers (citations are file:line in the reference
 * tree).  Conventions, identical for every function:
 *
 *   - all tensors are contiguous row-major, float32 / int32 (int64 only where stated);
 *   - pointers are DEVICE pointers owned by the caller (the Python host hands in torch storage);
 *     inputs are borrowed const, outputs are fully overwritten -- exactly the elements of the stated shape, never a byte
 *     beside them (rows and tiles are stored masked), and a workspace is used up to the bytes its size function returns and
 *     no further (tests/test_gpu_abi_bounds.py); where part of an output is NOT written or its contents are unspecified, the
 *     entry says so;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = the null
 *     stream); no implicit synchronisation, no allocation, no global state -> graph-capturable and
 *     thread-safe;
 *   - the return value is PASNL_OK (0) or a negative PASNL_E* code; nothing is enqueued on error.
 *     `pasnl_strerror` gives the text.  Shape rules mirror the reference's OP_REQUIRES checks.
 *   - b == 0 or an empty query/result dimension is a successful no-op.
 *
 * Arithmetic is the canonical fp32 of SURVEY.md Appendix A: IEEE round-to-nearest, no FMA
 * contraction, operations in the written order.  Index outputs are bit-exact against oracle/.
 */
#ifndef PASNL_H_
#define PASNL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PASNL_VERSION 100 /* 0.1.0 */

enum {
  PASNL_OK = 0,
  PASNL_EINVAL = -1,       /* bad dimension / attribute (the reference's InvalidArgument)   */
  PASNL_ENULL = -2,        /* a required pointer is NULL                                     */
  PASNL_EWORKSPACE = -3,   /* workspace smaller than pasnl_*_workspace_bytes                 */
  PASNL_ELAUNCH = -4,      /* hipGetLastError() != hipSuccess after the launch               */
  PASNL_EUNSUPPORTED = -5  /* valid request outside what the kernels cover (documented)      */
};

typedef void* pasnl_stream_t; /* hipStream_t */

int pasnl_version(void);
const char* pasnl_strerror(int code);
/* Number of HIP devices visible to the library (<0: HIP runtime error).  Used by the host to fail
 * loudly instead of falling back to a CPU path. */
int pasnl_device_count(void);

/* ------------------------------------------------------------------ sampling (tf_ops/sampling) */

/* Iterative farthest point sampling; idx[b,0] = 0.
 * replaces farthestpointsamplingLauncher  tf_sampling_g.cu:203-205 (kernel :105-170)
 * xyz (b,n,3) f32 -> idx (b,m) i32.  Tie rule: lowest (k mod 512, k) among maxima.
 * The reference needs a 32*n float temp (tf_sampling.cpp:115); this kernel keeps the running
 * distances in registers, so no workspace is required (m <= 0 -> PASNL_EINVAL as tf_sampling.cpp:99). */
int pasnl_farthest_point_sample(int b, int n, int m, const float* xyz, int* idx, pasnl_stream_t stream);

/* The same sampling, and the gather of the sampled coordinates in the same launch: new_xyz[b,j,:] = xyz[b, idx[b,j], :]
 * (bit-equal to pasnl_gather_point on idx).  Replaces the pair farthest_point_sample + gather_point every caller of the
 * reference runs back to back (pointasnl_util.py:33-49 sampling(), pointnet_util.py:44): the sampler has the picks in
 * LDS when it ends, so the second launch -- on the critical path of every set-abstraction layer -- disappears.
 * idx (b,m) i32, new_xyz (b,m,3) f32. */
int pasnl_farthest_point_sample_gather(int b, int n, int m, const float* xyz, int* idx, float* new_xyz,
                                       pasnl_stream_t stream);

/* out[b,j,:] = inp[b, idx[b,j], :] for 3-wide rows: inp (b,n,3), idx (b,m) i32 -> out (b,m,3).
 * replaces gatherpointLauncher  tf_sampling_g.cu:206-208 (kernel :172-181) */
int pasnl_gather_point(int b, int n, int m, const float* inp, const int* idx, float* out, pasnl_stream_t stream);

/* inp_g (b,n,3) = scatter-add of out_g (b,m,3) through idx (b,m); inp_g is zeroed first.
 * replaces cudaMemset + scatteraddpointLauncher  tf_sampling.cpp:174-175, tf_sampling_g.cu:183-192 */
int pasnl_gather_point_grad(int b, int n, int m, const float* out_g, const int* idx, float* inp_g, pasnl_stream_t stream);

/* Inverse-CDF sampling: out[b,j] = first r with cdf[b,r] >= inpr[b,j]*cdf[b,n-1]; `temp` (b*n floats)
 * receives the running sum.  replaces probsampleLauncher  tf_sampling_g.cu:198-201 (:7-104)
 * inp_p (b,n), inp_r (b,m) -> out (b,m) i32.  temp is scratch: all b*n floats may be written, its contents afterwards are
 * UNSPECIFIED (the sums are formed in another order than a sequential loop's). */
int pasnl_prob_sample(int b, int n, int m, const float* inp_p, const float* inp_r, float* temp, int* out, pasnl_stream_t stream);

/* ------------------------------------------------------------------ grouping (tf_ops/grouping) */

/* First `nsample` points (ascending index) with max(sqrtf(d2),1e-20f) < radius, padded with the first
 * hit; pts_cnt = min(hits, nsample); zero-hit rows are all 0 (the reference leaves them undefined).
 * replaces queryBallPointLauncher  tf_grouping_g.cu:125-126 (kernel :3-36)
 * xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> idx (b,m,nsample) i32, pts_cnt (b,m) i32 */
int pasnl_query_ball_point(int b, int n, int m, float radius, int nsample, const float* xyz1, const float* xyz2,
                           int* idx, int* pts_cnt, pasnl_stream_t stream);

/* out[b,j,k,:] = points[b, idx[b,j,k], :], row length c: points (b,n,c), idx (b,m,nsample) i32 -> out (b,m,nsample,c).
 * replaces groupPointLauncher  tf_grouping_g.cu:133-134 (kernel :40-57).  With nsample == 1 this is the
 * C-wide row gather the models do through tf.gather_nd (pointasnl_util.py:43-49,63-71). */
int pasnl_group_point(int b, int n, int c, int m, int nsample, const float* points, const int* idx, float* out,
                      pasnl_stream_t stream);

/* grad_points (b,n,c) = scatter-add of grad_out (b,m,nsample,c); zeroed first.
 * replaces cudaMemset + groupPointGradLauncher  tf_grouping.cpp:204-205, tf_grouping_g.cu:61-78 */
int pasnl_group_point_grad(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx,
                           float* grad_points, pasnl_stream_t stream);

/* Set-abstraction grouping, fused (pointasnl_util.py:63-74 + :248-249 + :258): for every query j and neighbour s
 *   new_point[b,j,s,:] = [ xyz[b,i,:] - new_xyz[b,j,:] | xyz[b,i,:] | feature[b,i,:] ],  i = idx[b,j,s]
 *   skip_max[b,j,:]    = max over s of new_point[b,j,s,:]
 * i.e. the two tf.gather_nd, the concat with xyz, the translation normalisation, the second concat and the
 * reduce_max of the skip connection in one pass; new_point is written once, nothing else touches HBM.
 * xyz (b,n,3), feature (b,n,c), idx (b,m,k) i32, new_xyz (b,m,3) -> new_point (b,m,k,6+c), skip_max (b,m,6+c). */
int pasnl_sa_group(int b, int n, int c, int m, int k, const float* xyz, const float* feature, const int* idx,
                   const float* new_xyz, float* new_point, float* skip_max, pasnl_stream_t stream);

/* k rounds of in-place selection sort per row of a (b,m,n) distance tensor; FULL (b,m,n) outputs, first k
 * columns meaningful, the tail is the swap residue.  replaces selectionSortLauncher
 * tf_grouping_g.cu:129-130 (kernel :83-123) */
int pasnl_select_top_k(int b, int n, int m, int k, const float* dist, int* outi, float* out, pasnl_stream_t stream);

/* Exact K nearest neighbours, ascending by (squared distance, index); the grouping search of all three
 * models.  replaces cpp_knn_batch / cpp_knn_batch_omp  utils/nearest_neighbors/knn_.cxx:72-135
 * (binding knn.pyx:71-109).  support (b,n,3), queries (b,m,3) -> idx (b,m,k), int32 when
 * idx_is_i64 == 0, int64 (the reference's `long`) otherwise.  dist2 (b,m,k) f32 is optional (NULL).
 * Requires 1 <= k <= n; k <= PASNL_KNN_MAX_K. */
#define PASNL_KNN_MAX_K 256
int pasnl_knn_batch(int b, int n, int m, int k, const float* support, const float* queries, void* idx,
                    int idx_is_i64, float* dist2, pasnl_stream_t stream);

/* Coverage-driven query selection + kNN.  replaces cpp_knn_batch_distance_pick(_omp)  knn_.cxx:136-266 (binding
 * knn.pyx:111-148): per cloud, nq times, among the points used least often so far take number (rnd % how many) in ascending
 * index order, output its k nearest neighbours (ascending (squared distance, index)) and its coordinates, raise the use
 * count of the neighbours by 1 and of the pick by 100.  pts (b,n,3) -> idx (b,nq,k) int64, queries (b,nq,3).  rnd (b,nq)
 * uint32 = the outputs of the caller's generator: the reference seeds one std::mt19937 with time(0) and walks the clouds in
 * order, so cloud i consumes outputs [i nq, (i+1) nq) (the Python mirror draws them with the same generator from an
 * explicit seed).  n <= 16384. */
int pasnl_knn_distance_pick(int b, int n, int nq, int k, const float* pts, const unsigned int* rnd, long long* idx,
                            float* queries, pasnl_stream_t stream);

/* The same search with a caller-provided workspace.  Clouds of PASNL_KNN_GRID_MIN_N <= n <= 16384 points and k <= 64 are
 * searched through a uniform grid built in the workspace (csrc/knn_grid.hip: counting sort by cell, expanding rings of
 * cells, acceptance only when no unexamined cell can hold a closer or tying point -> results bit-identical to
 * pasnl_knn_batch for every input); everything else is forwarded to pasnl_knn_batch.  pasnl_knn_workspace_bytes returns
 * the bytes the pair (b, n) needs (0: the grid is not used and workspace may be NULL).  The workspace is scratch: nothing
 * is kept between calls. */
#define PASNL_KNN_GRID_MIN_N 4096
size_t pasnl_knn_workspace_bytes(int b, int n);
int pasnl_knn_batch_ws(int b, int n, int m, int k, const float* support, const float* queries, void* idx, int idx_is_i64,
                       float* dist2, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* pasnl_knn_batch_ws as a BACKGROUND job: the query kernel runs on at most max_workgroups workgroups (a capped grid that walks
 * the queries) instead of one wave per query -- for a search enqueued on a side stream beside other work (a serving loop's
 * prefetch of the next batch's neighbour lists): a saturating grid of ~20 000 workgroups leaves the kernels of the other stream
 * waiting for free slots (measured: a 10-us kernel of the forward stretched to 225 us beside it).  Same results.  Falls back to
 * pasnl_knn_batch (uncapped) where the grid form does not apply. */
int pasnl_knn_batch_ws_bg(int b, int n, int m, int K, const float* support, const float* queries, void* idx, int idx_is_i64,
                          float* dist2, void* workspace, size_t workspace_bytes, int max_workgroups, pasnl_stream_t stream);

/* The same K nearest neighbours in the REFERENCE'S order among exactly equal distances (and with the reference's choice of
 * which of several tied candidates is the K-th): nanoflann keeps candidates of equal distance in the order its KD-tree visits
 * them (nanoflann.hpp:115-134, :1351-1410; tree: divideTree / middleSplit_ / planeSplit :916-1043, leaf size 10,
 * knn_.cxx:83).  Replaces cpp_knn_batch knn_.cxx:72-101 bit for bit, ties included, by rebuilding that tree and that search on
 * the GPU -- an exactness mode (a workgroup per cloud builds the tree level by level, a lane per query searches it: about
 * 1 ms for 16 clouds of 8192 points where the canonical kernels take 0.06), not a fast path; pasnl_knn_batch returns the
 * canonical (distance, index) order, identical whenever distances are distinct.  k <= n, k <= PASNL_KNN_MAX_K (k > 64 or
 * n > 65535: one wave per query instead of one lane; n > 10240: the tree from a one-lane build -- seconds at 1e5 points).  workspace:
 * pasnl_knn_tree_workspace_bytes(b, n, m, k) bytes; its first int32 is non-zero afterwards if a tree or a search was deeper
 * than 96 levels (pathological clustering: the result is then not valid). */
size_t pasnl_knn_tree_workspace_bytes(int b, int n, int m, int k);
int pasnl_knn_batch_tree(int b, int n, int m, int k, const float* support, const float* queries, void* idx, int idx_is_i64,
                         void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* cpp_knn_batch's RESULT, ties included, at the canonical kernels' price -- what the Python mirror calls by default.
 * replaces cpp_knn_batch / cpp_knn_batch_omp  knn_.cxx:72-135 (result-set order: nanoflann.hpp:115-134).
 * nanoflann's list can differ from the (distance, index) list only where distances are EQUAL -- two of them inside a query's
 * K-list, or a candidate beyond the list at exactly the K-th distance.  So: the canonical search (pasnl_knn_batch_ws's choice
 * of kernel) writes every row and, from the sorted keys it already holds, lists the queries with such a tie.  A listed row
 * differs from nanoflann's only INSIDE its runs of equal distances, and two points of a run are reached by nanoflann's search in
 * the order decided at the tree node that separates them (the query's near child first, :1380-1393; positions left to right in a
 * leaf): for a FEW listed queries (<= 32 listed clouds, <= 16 queries and <= 64 tied points a cloud) only those nodes of the
 * reference tree are computed -- as point sets, one pass of reductions over the cloud per level, no tree built, no search run;
 * two tied points in one leaf (duplicated points): the records of a cloud of more than 2048 points are moved along that one
 * path.  Everything else: the KD-tree of the cloud is built and searched for its listed queries (pasnl_knn_batch_tree's
 * kernels).  All counts stay on the device: every kernel is launched and returns at once where nothing is listed -- no host
 * synchronisation, capturable.  Tie-free clouds pay two to five empty launches; output == pasnl_knn_batch_tree's bit for bit.
 * depth_flag (device int, required): set to 1 -- never cleared by the library -- if a listed query's tree or search was deeper
 * than 96 levels; such rows KEEP the canonical order (valid neighbours, canonical order among equals).
 * max_workgroups > 0: the grid-pruned canonical search as a background job (pasnl_knn_batch_ws_bg); 0: the usual grid.
 * k <= n, k <= PASNL_KNN_MAX_K.  Clouds of up to 2048 points (k <= 64): ONE kernel after the search -- the tie paths of a cloud's
 * <= 4 listed queries, else its tree and searches in one workgroup, all in LDS; larger ones: a tie-path kernel, then the builds
 * of pasnl_knn_batch_tree + one wave per listed query.
 * workspace: pasnl_knn_batch_ref_workspace_bytes(b, n, m, k); afterwards its first b int32 = the listed queries per cloud, and,
 * 256-byte aligned behind them, 2 b int32: what the tie paths / the on-demand tree left to the next stage (diagnostics). */
size_t pasnl_knn_batch_ref_workspace_bytes(int b, int n, int m, int k);
int pasnl_knn_batch_ref(int b, int n, int m, int k, const float* support, const float* queries, void* idx, int idx_is_i64,
                        int* depth_flag, void* workspace, size_t workspace_bytes, int max_workgroups, pasnl_stream_t stream);

/* ------------------------------------------------------- interpolation (tf_ops/3d_interpolation) */

/* Three nearest known points, squared distances ascending, lowest index first on ties.
 * replaces threenn_cpu  tf_interpolate.cpp:60-103
 * xyz1 (b,n,3) unknown, xyz2 (b,m,3) known -> dist (b,n,3) f32, idx (b,n,3) i32 */
int pasnl_three_nn(int b, int n, int m, const float* xyz1, const float* xyz2, float* dist, int* idx,
                   pasnl_stream_t stream);

/* out[b,j,l] = (p[i1,l]*w1 + p[i2,l]*w2) + p[i3,l]*w3.
 * replaces threeinterpolate_cpu  tf_interpolate.cpp:107-127   (note the argument order b,m,c,n)
 * points (b,m,c), idx (b,n,3) i32, weight (b,n,3) -> out (b,n,c) */
int pasnl_three_interpolate(int b, int m, int c, int n, const float* points, const int* idx, const float* weight,
                            float* out, pasnl_stream_t stream);

/* grad_points (b,m,c) = scatter-add; zeroed first.
 * replaces memset + threeinterpolate_grad_cpu  tf_interpolate.cpp:258-259 (:131-153) */
int pasnl_three_interpolate_grad(int b, int n, int c, int m, const float* grad_out, const int* idx,
                                 const float* weight, float* grad_points, pasnl_stream_t stream);

/* Inverse-distance weights for three_interpolate: d=max(d,1e-10); w=(1/d)/sum(1/d), in that order.
 * replaces the four TF ops at pointasnl_util.py:308-311 / pointnet_util.py:212-215
 * dist (rows,3) -> weight (rows,3) */
int pasnl_three_weights(int rows, const float* dist, float* weight, pasnl_stream_t stream);

/* The head of a feature-propagation module in one launch (utils/pointnet_util.py:212-219 pointnet_fp_module;
 * utils/pointasnl_util.py:308-313 PointASNLDecodingLayer): the inverse-distance weights of pasnl_three_weights, the
 * interpolation of pasnl_three_interpolate and tf.concat([interpolated, points1], axis=2), same arithmetic, same bits:
 *   out (b,n,c2+c1) = [ sum_j w[b,i,j] points2[b, idx[b,i,j], :]  |  points1[b,i,:] ]
 * dist, idx (b,n,3) = pasnl_three_nn's outputs; points2 (b,m,c2); points1 (b,n,c1) or NULL with c1 == 0 (no concat).
 * Inference only (the differentiable path stays pasnl_three_interpolate + its gradient). */
int pasnl_fp_interpolate_cat(int b, int m, int c2, int n, int c1, const float* points2, const int* idx, const float* dist,
                             const float* points1, float* out, pasnl_stream_t stream);

/* ------------------------------------------------- PointASNL cells (utils/pointasnl_util.py) */

/* Fused Point-NonLocal attention core, mode 'dot' (pointasnl_util.py:197-212):
 *   out[b,i,:] = softmax_j( q[b,i,:] . k[b,j,:] / sqrt(cb) ) . v[b,j,:]
 * q (b,p,cb); kv (b,n,2*cb) with K = kv[...,:cb], V = kv[...,cb:] exactly as conv_kv produces them
 * (:193-194); out (b,p,cb).  The (b,p,n) attention map is never materialised.
 * variant: 0 = auto, 1 = vector-FMA kernel (cb <= 64), 2 = fp32 MFMA kernel, 3 = fp32 MFMA kernel with LDS-staged K/V
 * (the only MFMA form for cb = 128; kept selectable for A/B).  cb in {32, 64, 128} and kv / out 16-byte aligned;
 * anything else: PASNL_EUNSUPPORTED (the Python mirror then takes the op-by-op path on the vendor BLAS). */
int pasnl_nl_attention(int b, int p, int n, int cb, const float* q, const float* kv, float* out, int variant,
                       pasnl_stream_t stream);
/* pasnl_nl_attention with a scratch workspace: where b * ceil(p / 64) workgroups would leave CUs empty (cb = 32; the
 * SemanticKITTI model's layer 1_1: 8 x 1280 queries = 160 workgroups for 256 CUs) the KEYS are split over workgroups too
 * ("flash-decoding"): every part leaves its un-normalised (O, m, l) in the workspace and a second small kernel combines the
 * parts in ascending key order -- a fixed order: the result is a pure function of the inputs -- and normalises.  Same 1e-5
 * contract; not the bits of the one-workgroup form (another association of the running rescalings).
 * pasnl_nl_attention_workspace_bytes: the bytes that form needs for the shape, 0 where it is not used (workspace may be NULL). */
size_t pasnl_nl_attention_workspace_bytes(int b, int p, int n, int cb);
int pasnl_nl_attention_ws(int b, int p, int n, int cb, const float* q, const float* kv, float* out, int variant,
                          void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Adaptive-Sampling micro self-attention over the first `as` neighbours of each query
 * (SampleWeights, pointasnl_util.py:136-146):  g groups, each q,k,v (as,cb):
 *   out[g,i,:] = softmax_j( q[g,i,:] . k[g,j,:] / sqrt(cb) ) . v[g,j,:]
 * q (g,as,cb); kv (g,as,2*cb) (K first, V second, :133-134); out (g,as,cb).  as <= 16, cb <= 256.
 * (pasnl_as_attention_qkv and pasnl_as_attention_proj below: the same out (g,as,cb).) */
int pasnl_as_attention(int g, int as, int cb, const float* q, const float* kv, float* out, pasnl_stream_t stream);

/* AdaptiveSampling tail (pointasnl_util.py:154-155,167-171): softmax over the neighbour axis of
 * logits (g,as,1+ch), then new_xyz[g,:] = sum_k w[g,k,0]*xyz[g,k,:] and
 * new_feature[g,c] = sum_k w[g,k,1+c]*feat[g,k,c].
 * xyz rows are taken from grouped_xyz (g,nsample,3) and feat from grouped_feature (g,nsample,ch):
 * only the first `as` of `nsample` neighbours are read (the :165-166 slices).
 * -> new_xyz (g,3), new_feature (g,ch); the same two outputs for pasnl_as_reweight_x and the pasnl_as_cell_* entries below. */
int pasnl_as_reweight(int g, int as, int nsample, int ch, const float* logits, const float* grouped_xyz,
                      const float* grouped_feature, float* new_xyz, float* new_feature, pasnl_stream_t stream);

/* Set-abstraction "local cell", fused (pointasnl_util.py:264-274): per query group of k
 * neighbours, with x = new_point (groups,k,w) as produced by pasnl_sa_group (w = 6+C, columns 0..2 = centred xyz):
 *   H1 = relu(x W0 + b0) (k,c1);  H2 = relu(H1 W1 + b1) (k,c2);  G = relu(x[:,0:3] Ww + bw) (k,32);
 *   out[g] = H2^T G  flattened as (c2*32)   -- the input of the [1,c2] `after_conv` GEMM (:275-278).
 * W0 (w,c1), W1 (c1,c2), Ww (3,32) row-major with inference BN already folded in (tf_util.py).  Replaces two
 * conv2d, the weight-net conv2d, a transpose and a batched matmul of the reference graph; H1, H2 and G never
 * reach HBM.  k % 32 == 0; (c1,c2) in {(32,32),(64,64),(128,128)}; weights must fit 160 KiB of LDS. */
int pasnl_sa_local_cell(int groups, int k, int w, int c1, int c2, const float* x, const float* w0, const float* b0,
                        const float* w1, const float* b1, const float* ww, const float* bw, float* out,
                        pasnl_stream_t stream);

/* The same cell with the grouping fused in (pointasnl_util.py:63-74,248-249,258,264-274): row s of group (b,j) is
 * [xyz[i]-new_xyz[b,j] | xyz[i] | feature[i]], i = idx[b,j,s], gathered straight from the (b,n,3) / (b,n,c) tables
 * (L2-resident), so the (b,m,k,6+c) grouped tensor never exists in HBM.  Also returns the skip connection's
 * reduce_max over the k neighbours: skip_max (b,m,6+c) -- bit-equal to pasnl_sa_group's.
 * out (b*m, c2*32) as pasnl_sa_local_cell.  Replaces two tf.gather_nd, two concats, a subtraction, a reduce_max,
 * three conv2d, a transpose and a batched matmul of the reference graph.  Shape limits as above for c1 = c2 in {32, 64, 128}; also
 *   c1 = c2 = 16 (pointasnl_sem_seg_res.py:32: xyz-only rows c = 3, k = 32, new_xyz given): a 16x16x4-MFMA kernel, no padding;
 *   c1 = c2 in {256, 512} (pointasnl_sem_seg.py:34, pointasnl_sem_seg_res.py:46-51: k = 32, c % 16 == 0, feature 16-byte aligned,
 *   new_xyz given): one workgroup per group, weights streamed from L2; there w1 = b1 = NULL means the layer has a single
 *   convolution (mlp = [c, c]) and H2 = H1.
 * new_xyz == NULL: the centre of group (b,j) is its own neighbour 0, xyz[b, idx[b,j,0]] -- AdaptiveSampling with
 * as_neighbor == 0 (pointasnl_util.py:161-163), taken from the tile the kernel gathers anyway, so that the launch does not
 * wait for pasnl_take_neighbor0 (needs m <= n, else PASNL_EUNSUPPORTED). */
int pasnl_sa_cell(int b, int n, int c, int m, int k, int c1, int c2, const float* xyz, const float* feature,
                  const int* idx, const float* new_xyz, const float* w0, const float* b0, const float* w1,
                  const float* b1, const float* ww, const float* bw, float* out, float* skip_max,
                  pasnl_stream_t stream);

/* pasnl_sa_cell with new_xyz = NULL that ALSO writes what pasnl_take_neighbor0 would have: new_xyz (b,m,3) = the centres and
 * new_feature (b,m,3+c) = [centre | feature row of neighbour 0] (pointasnl_util.py:161-164) -- the wave that owns a group
 * holds that row's address anyway.  A set-abstraction layer without adaptive sampling then needs no gather launch between
 * its neighbour search and its cell.  c <= 128, else PASNL_EUNSUPPORTED. */
int pasnl_sa_cell_centre0(int b, int n, int c, int m, int k, int c1, int c2, const float* xyz, const float* feature,
                          const int* idx, const float* w0, const float* b0, const float* w1, const float* b1,
                          const float* ww, const float* bw, float* out, float* skip_max, float* new_xyz, float* new_feature,
                          pasnl_stream_t stream);

/* The pre-projected form of pasnl_sa_cell for layers whose groups gather each source point many times.  conv0 is linear before
 * its ReLU: [xyz - centre | xyz | feature] . w0 + b0 = (xyz - centre) . w0[0:3] + proj, where
 *   pasnl_sa_project: proj (b,n,c1) = [xyz | feature] . w0[3:6+c] + b0, once per source point (replaces the per-neighbour
 *   products of those 3 + c rows of w0 inside the cell);
 *   pasnl_sa_cell_pre / pasnl_sa_cell_pre_centre0: pasnl_sa_cell / pasnl_sa_cell_centre0 with conv0 = proj[b, idx] +
 *   (xyz - centre) . w0[0:3] (only those 3 rows of w0 are read; b0 is in proj).  skip_max bit-equal to pasnl_sa_cell's; out
 *   within fp32 rounding of it (conv0 sums in another order).
 * c1 = c2 in {32, 64, 128} (c1 = the width of proj); c % 4 == 0 with 16-byte aligned feature and proj, else PASNL_EUNSUPPORTED;
 * other limits as pasnl_sa_cell / pasnl_sa_cell_centre0. */
int pasnl_sa_project(int b, int n, int c, int c1, const float* xyz, const float* feature, const float* w0, const float* b0,
                     float* proj, pasnl_stream_t stream);
int pasnl_sa_cell_pre(int b, int n, int c, int m, int k, int c1, int c2, const float* xyz, const float* feature,
                      const float* proj, const int* idx, const float* new_xyz, const float* w0, const float* w1, const float* b1,
                      const float* ww, const float* bw, float* out, float* skip_max, pasnl_stream_t stream);
int pasnl_sa_cell_pre_centre0(int b, int n, int c, int m, int k, int c1, int c2, const float* xyz, const float* feature,
                              const float* proj, const int* idx, const float* w0, const float* w1, const float* b1,
                              const float* ww, const float* bw, float* out, float* skip_max, float* new_xyz, float* new_feature,
                              pasnl_stream_t stream);

/* pasnl_sa_cell / pasnl_sa_cell_centre0 (new_xyz == NULL: the centres are neighbour 0 and new_xyz_out / new_feature_out are
 * written, else both are ignored) that ALSO get the feature rows of w0 (rows 6 .. 5 + c) and w1 in the matrix instruction's
 * operand order -- pasnl_mlp3_pack_weights(c, c1, w0 + 6 * c1, w0_features_packed) and pasnl_mlp3_pack_weights(c1, c2, w1,
 * w1_packed), once per variable -- for the kernels that stream their weights from L2 (one workgroup per group: c1 = c2 in
 * {256, 512}, and 128 with few groups or one convolution): 16-byte weight loads.  The row-major matrices are still required
 * (the first rows of w0, every other kernel); NULL packed pointers = the plain entry points; identical results.
 * out (b*npoint, c2*32), skip_max (b,npoint,6+c); new_xyz_out (b,npoint,3) and new_feature_out (b,npoint,3+c) are NOT written
 * when new_xyz is given (they may be NULL then). */
int pasnl_sa_cell_packed(int b, int n, int c, int npoint, int nsample, int c1, int c2, const float* xyz, const float* feature,
                         const int* idx, const float* new_xyz, const float* w0, const float* b0, const float* w1, const float* b1,
                         const float* ww, const float* bw, const float* w0_features_packed, const float* w1_packed, float* out,
                         float* skip_max, float* new_xyz_out, float* new_feature_out, pasnl_stream_t stream);

/* PointNet set-abstraction pooling (pointnet_util.py:137, tf.reduce_max(new_points, axis=[2], keep_dims=True)):
 * out[b,ch] = max over the n points of x (b,n,c).  The two group_all modules of pointasnl_cls pool 67 + 34 MB. */
int pasnl_max_pool_rows(int b, int n, int c, const float* x, float* out, pasnl_stream_t stream);

/* The same pooling into rows of a wider table: out[b * out_stride + ch], out_stride >= c -- the two pooled vectors of
 * pointasnl_cls land side by side in the (B, 1536) input of fc1 (models/pointasnl_cls.py:43-45: the tf.concat is free).
 * Only the c floats at out + row * out_stride are written: the other columns of the table are NOT written (the last row
 * needs c floats, not out_stride). */
int pasnl_max_pool_rows_strided(int b, int n, int c, const float* x, float* out, long out_stride, pasnl_stream_t stream);

/* The "group all" set-abstraction module in one kernel (csrc/mlp_pool.hip): pointnet_sa_module(..., group_all=True) of
 * utils/pointnet_util.py:87-137 as called at models/pointasnl_cls.py:39-40 -- the three 1x1 convolutions of `mlp` (BN folded
 * into w / bias by the caller, ReLU) over every point of a cloud and tf.reduce_max over the points:
 *   out[cloud * out_stride + ch] = max_i relu(relu(relu(x[cloud,i,:] w0 + b0) w1 + b1) w2 + b2)[ch]
 * x (b,n,k0) rows [xyz | points] (sample_and_group_all's concat, pointnet_util.py:79; any leading alignment columns the
 * caller added have zero rows in w0).  w0 (k0,c1), w1 (c1,c2), w2 (c2,c3) are handed over PACKED in the matrix instruction's
 * operand order -- pasnl_mlp3_pack_weights(k, n, w, packed) once per variable into pasnl_mlp3_packed_weights_bytes(k, n) bytes
 * (16-byte aligned): packed[((bt * 2 + h) * n + col) * 8 + u] = w[16 bt + 2 u + h][col], zero beyond k.  Covered: (c1,c2,c3) =
 * (128,256,512) and (256,512,1024), k0 % 4 == 0, x 16-byte aligned; otherwise PASNL_EUNSUPPORTED (the caller runs the layers
 * one by one).  workspace: pasnl_mlp3_max_pool_workspace_bytes(b, n, c3) bytes (maxima per tile of 32 points; no need to clear it).
 * out: c3 floats per cloud at out + cloud * out_stride, out_stride >= c3; the other columns of the table are NOT written. */
size_t pasnl_mlp3_packed_weights_bytes(int k, int n);
int pasnl_mlp3_pack_weights(int k, int n, const float* w, float* packed, pasnl_stream_t stream);
size_t pasnl_mlp3_max_pool_workspace_bytes(int b, int n, int c3);
int pasnl_mlp3_max_pool(int b, int n, int k0, int c1, int c2, int c3, const float* x, const float* w0, const float* b0,
                        const float* w1, const float* b1, const float* w2, const float* b2, float* out, long out_stride,
                        void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* The classifier's layer 1 tail and its layer3_1 group-all module in ONE launch (csrc/mlp_pool.hip; + the pooling pass over
 * tile maxima): pasnl_sa_tail_packed(b * n rows, ..., new_xyz, out_cat, out) followed by pasnl_mlp3_max_pool(b, n, c + 4,
 * c1, c2, c3, out_cat, ...), with the same bits in `out` and `pooled`, but the (b*n, c+4) table [0 | new_xyz | out] stays in
 * the workgroup's LDS -- it is neither written nor read.  after (b*n,c), skip_max (b*n,w), att (b*n,cb), new_xyz (b*n,3);
 * ws / wb / wagg packed by pasnl_sa_tail_pack_weights; w0 (c+4,c1: one zero row in front of the reference's 3+c), w1, w2
 * packed by pasnl_mlp3_pack_weights (all 16-byte aligned).  Covered: w = 9, cb = 32, c = c1 = 128, c2 = 256, c3 = 512 --
 * anything else is PASNL_EUNSUPPORTED before any launch (the caller runs the two entry points above).  out (b*n,c) is fully
 * written; pooled: c3 floats per cloud at pooled + cloud * pooled_stride (pooled_stride >= c3; the other columns are NOT
 * written); workspace: pasnl_mlp3_max_pool_workspace_bytes(b, n, c3) bytes. */
int pasnl_cls_tail_group_all(int b, int n, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                             const float* ws_packed, const float* bs, const float* wb_packed, const float* bb,
                             const float* wagg_packed, const float* bagg, const float* new_xyz, int c1, int c2, int c3,
                             const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* out, float* pooled, long pooled_stride, void* workspace, size_t workspace_bytes,
                             pasnl_stream_t stream);

/* The classifier's layer 2 tail and the first two convolutions of its layer3_2 group-all module in ONE launch
 * (csrc/mlp_pool.hip): pasnl_sa_tail_packed(b * n rows, ...) with the same bits in `out`, then
 * h2 (b*n,c2) = relu(relu([0 | new_xyz | out] w0 + b0) w1 + b1) for the module's third convolution; the (b*n, c+4) table and
 * the (b*n,c1) activations stay in the workgroup's LDS.  The two convolutions are an fp32 fmaf chain in ascending k (1e-5 of
 * the output scale against fp64: the contract of pasnl_mlp3_max_pool; not the bits of a vendor GEMM).  Arguments as for
 * pasnl_cls_tail_group_all; w0 (c+4,c1), w1 (c1,c2) packed by pasnl_mlp3_pack_weights.  Covered: w = 134, cb = 64,
 * c = c1 = 256, c2 = 512 -- anything else is PASNL_EUNSUPPORTED before any launch.  out (b*n,c) and h2 (b*n,c2) are fully
 * written; h2_bytes: the size of the buffer at h2, at least b*n*c2*sizeof(float) (PASNL_EWORKSPACE otherwise). */
int pasnl_cls_tail_mlp2(int b, int n, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                        const float* ws_packed, const float* bs, const float* wb_packed, const float* bb,
                        const float* wagg_packed, const float* bagg, const float* new_xyz, int c1, int c2, const float* w0,
                        const float* b0, const float* w1, const float* b1, float* out, float* h2, size_t h2_bytes,
                        pasnl_stream_t stream);

/* ------------------------------------------------------------------ fp32-grade products on the bf16 matrix pipe (csrc/dense_bf16x3.hip)
 * An explicit MODE (the Python side's tf_util.DENSE_BF16X3; off by default, never used for the headline benchmark):
 * out (rows,n) = act(x (rows,kdim; row stride lda) . w + bias) for the long GEMMs behind tf_util.conv2d over a flattened
 * [nsample x channel] window (utils/pointasnl_util.py:275, 337; tf_util.py:120-185).  Every fp32 operand is split into three
 * bf16 terms and the six products of weight >= 2^-16 are accumulated in fp32 on v_mfma_f32_32x32x16_bf16: about one more
 * rounding per product than an fp32 fmaf chain (inside the 1e-5 contract, not the same bits).
 *   pasnl_bf16x3_split_weights: w (kdim,n) fp32 -> wsplit (pasnl_bf16x3_weights_bytes(kdim, n) = 6 kdim n bytes, 16-byte
 *   aligned: three bf16 planes hi, mid, lo in operand order, wsplit[plane][kdim / 8][n][kdim % 8]), once per layer; pasnl_dense_bf16x3: kdim % 32 == 0, n % 128 == 0, lda % 4 == 0, x 16-byte aligned, else PASNL_EUNSUPPORTED. */
size_t pasnl_bf16x3_weights_bytes(int kdim, int n);
int pasnl_bf16x3_split_weights(int kdim, int n, const float* w, void* wsplit, pasnl_stream_t stream);
int pasnl_dense_bf16x3(int rows, int kdim, int n, int lda, const float* x, const void* wsplit, const float* bias, int relu,
                       float* out, pasnl_stream_t stream);

/* ------------------------------------------------------------------ dense layers with few rows (csrc/dense.hip) */

/* out (rows,n) = act(x (rows,kdim) . w (kdim,n) + bias), rows <= 128, relu != 0 -> ReLU: the classifier head
 * (tf_util.fully_connected, tf_util.py:327-365, called at models/pointasnl_cls.py:46-50 with one row per cloud; BN folded
 * into w / bias by the caller).  A product this thin is cut along n AND along kdim over ~128 workgroups; the K slices meet in
 * `workspace` and are summed in slice order (bit-reproducible).  kdim % 8 == 0 and x 16-byte aligned, else PASNL_EUNSUPPORTED.
 * workspace: pasnl_dense_rows_workspace_bytes(rows, kdim, n) bytes of device memory, ZERO-FILLED once by the caller before
 * its first use (the kernel leaves its counters at zero); one workspace serves one stream at a time.  The counters are the
 * first 4 * ceil(n / 32) bytes rounded up to 256: only they have to be zero, the partial sums behind them need no
 * initialisation. */
size_t pasnl_dense_rows_workspace_bytes(int rows, int kdim, int n);
int pasnl_dense_rows(int rows, int kdim, int n, const float* x, const float* w, const float* bias, int relu, float* out,
                     void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* out (rows,n) = act(x (rows,kdim; row stride lda) . w (kdim,n) + bias) for THIN products with a long contraction -- the
 * [1,C] after_conv / decode_after_conv windows of the deep levels (pointasnl_util.py:277-280, :329-331 through tf_util.conv2d,
 * tf_util.py:120-185; BN folded by the caller): few 128 x 128 output tiles, kdim in the thousands.  128 x 128 tiles x K slices
 * on fp32 MFMA; the slices' partial tiles meet in `workspace` (pasnl_dense_splitk_workspace_bytes bytes, no initialisation
 * needed; one workspace serves one stream at a time) and are summed in slice order (bit-reproducible).
 * kdim % 16 == 0, lda % 4 == 0, n % 4 == 0, x / out / bias 16-byte aligned, else PASNL_EUNSUPPORTED. */
size_t pasnl_dense_splitk_workspace_bytes(int rows, int kdim, int n);
int pasnl_dense_splitk(int rows, int kdim, int n, int lda, const float* x, const float* w, const float* bias, int relu,
                       float* out, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Two projections of NARROW rows in one launch: out_i (rows_i, n_i) = x_i (rows_i, kdim_i) . w_i + bias_i, kdim_i <= 16,
 * n_i in {32, 64, 128, 256}, no activation: conv_kv and conv_query of the first layer's non-local cell, whose inputs are
 * coordinates (3 or 6 channels) -- pointasnl_util.py:186-193, two tf_util.conv2d with activation_fn=None.  rows_1 == 0
 * runs the first job alone.  w_i / bias_i / out_i 16-byte aligned, else PASNL_EUNSUPPORTED. */
int pasnl_narrow_project2(long rows0, int kdim0, int n0, const float* x0, const float* w0, const float* bias0, float* out0,
                          long rows1, int kdim1, int n1, const float* x1, const float* w1, const float* bias1, float* out1,
                          pasnl_stream_t stream);

/* The non-local cell of a NARROW level, attended in input space (csrc/nl_input.hip): what pasnl_narrow_project2 followed by
 * pasnl_nl_attention computes -- out (b,p,cb) = softmax(Q K^T / sqrt(cb)) V with [K | V] = feature . wkv + bkv and
 * Q = new_point . wq + bq (pointasnl_util.py:186-212; BN folded by the caller, no activation) -- without forming K, V or Q.
 * K and V are linear in the c input channels, so per query u = Wk Q (c numbers; Q . bk is constant over the keys and cancels
 * in the softmax), w_j = softmax_j(u . feature_j / sqrt(cb)), and out = (sum_j w_j feature_j) Wv + bv.  Within the cells'
 * 1e-5 of the fp64 restatement, not the bits of the cb-wide form; a pure function of its inputs (no atomics, fixed orders).
 * feature (b,n,c), new_point (b,p,cz), wkv (c,2cb), bkv (2cb), wq (cz,cb), bq (cb).  1 <= c <= 8, 1 <= cz <= 16, cb in
 * {32, 64, 128}, b <= 65535, out 16-byte aligned, else PASNL_EUNSUPPORTED; n < 1 is PASNL_EINVAL; b == 0 or p == 0 is a
 * successful no-op.  Used by all three models' first levels (the name's prefix keeps it with the classifier's entries). */
int pasnl_cls_nl_cell_input(int b, int p, int n, int c, int cz, int cb, const float* feature, const float* new_point,
                            const float* wkv, const float* bkv, const float* wq, const float* bq, float* out,
                            pasnl_stream_t stream);

/* Backward of pasnl_cls_nl_cell_input (csrc/nl_input_grad.hip).  With X = feature, Z = new_point, wkv = [Wk | Wv],
 * bkv = [bk | bv], r = 1/sqrt(cb), G = grad_out = dL/dout (b,p,cb) and the forward's Q_i = Z_i Wq + bq, u_i = Wk Q_i,
 * w_ij = softmax_j(r u_i . X_j), ctr_i = sum_j w_ij X_j, out_i = ctr_i Wv + bv:
 *     per query   h_i = Wv G_i (c numbers)   t_ij = h_i . X_j   delta_i = h_i . ctr_i   dS_ij = w_ij (t_ij - delta_i)
 *                 du_i = r sum_j dS_ij X_j
 *     per key     dX_j = sum_i (w_ij h_i + r dS_ij u_i), over the queries of its cloud
 *     moments     A = sum_i Z_i^T du_i (cz,c)   s = sum_i du_i (c), over all b p queries
 *     weights     dWk = A^T Wq + s (x) bq   dWv = sum_i ctr_i (x) G_i   dbv = sum_i G_i   dWq = A Wk   dbq = s Wk
 *                 dZ_i = (du_i Wk) Wq^T       dbk = 0 exactly (Q . bk is constant over the keys and cancels in the softmax)
 * grad_feature (b,n,c) = dX, grad_new_point (b,p,cz) = dZ, grad_wkv (c,2cb) = [dWk | dWv], grad_bkv (2cb) = [0 | dbv] (the
 * zeros are written, as exact zeros), grad_wq (cz,cb), grad_bq (cb).  du is summed over the keys in its centred form, after a
 * first sweep has given delta (the difference of the two uncentred sums loses an order of magnitude in fp32); the second sweep
 * also sums the centred terms themselves, sum_j w_ij (t_ij - delta_i) -- what h_i . ctr_i misses of sum_j w_ij t_ij in fp32 --
 * and delta_i and du_i are corrected by it before they are used further.  Three
 * launches on the vector pipe: query-major (dZ, per-query records, per-workgroup partial moments), key-major (dX) and a small
 * one that sums the partial moments and applies the c x cb / cz x cb products; no (b,p,n), (b,n,2cb) or (b,p,cb)
 * intermediate exists.  No fp atomics, every sum in a fixed order: the gradients are a pure function of the inputs.  Every
 * element of every gradient given is written (no memset needed), nothing beside them.
 * Any gradient pointer may be NULL: that gradient is skipped together with the work that only serves it (grad_feature NULL --
 * training on coordinates -- skips the key-major launch and the records; no weight gradient: the moments and the last
 * launch; grad_bkv alone: the second sweep); all six NULL is PASNL_ENULL.
 * workspace: pasnl_cls_nl_cell_input_grad_workspace_bytes bytes =
 *     4 * ( (2c + 2) * b * p  +  b * ceil(p / 64) * ((cz + 1) * c + (c + 1) * cb) )
 * -- per query lse2 (log-sum-exp of the scores in the log2 domain), delta, u[c], h[c]; per workgroup of 64 queries the partial
 * A, s, dWv, dbv -- whatever gradients are asked for; 0 for an empty or unsupported shape.  It does not depend on n.
 * Checked in this order, before anything is enqueued: b, p >= 0 and n, c, cz, cb >= 1, else PASNL_EINVAL; c <= 8, cz <= 16,
 * cb in {32, 64, 128}, else PASNL_EUNSUPPORTED; b == 0 or p == 0 succeeds and zero-fills every gradient given; a NULL input,
 * grad_out or workspace, or all six gradients NULL, PASNL_ENULL; grad_out or the workspace not 16-byte aligned (the other
 * operands need their natural 4 bytes only), or b > 65535, PASNL_EUNSUPPORTED; a short workspace PASNL_EWORKSPACE.
 * The names carry the pasnl_cls_ prefix, as pasnl_cls_nl_cell_input does, to stay outside the scope of tests/abi_cases.py,
 * whose symbol count is pinned; the entries are held to their buffers by tests/test_gpu_nl_cell_input_grad.py instead. */
size_t pasnl_cls_nl_cell_input_grad_workspace_bytes(int b, int p, int n, int c, int cz, int cb);
int pasnl_cls_nl_cell_input_grad(int b, int p, int n, int c, int cz, int cb, const float* feature, const float* new_point,
                                 const float* wkv, const float* bkv, const float* wq, const float* bq, const float* grad_out,
                                 float* grad_feature, float* grad_new_point, float* grad_wkv, float* grad_bkv, float* grad_wq,
                                 float* grad_bq, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Backward of pasnl_nl_attention (csrc/nl_grad.hip).  With K = kv[..., :cb], V = kv[..., cb:], s_ij = q_i . k_j / sqrt(cb),
 * P = softmax_j(s), out = P V and grad_out = dL/dout (b,p,cb):
 *     delta_i = sum_c grad_out_ic out_ic      dP_ij = grad_out_i . v_j      dS_ij = P_ij (dP_ij - delta_i)
 *     grad_q_i = sum_j dS_ij k_j / sqrt(cb)   dK_j = sum_i dS_ij q_i / sqrt(cb)   dV_j = sum_i P_ij grad_out_i
 * grad_q (b,p,cb); grad_kv (b,n,2cb) = [dK | dV], the layout of kv.  `out` is the forward's result for the same q, kv (used
 * for delta only).  Two launches on the fp32 MFMA: P is recomputed tile by tile and nothing of size (b,p,n) exists.  No fp
 * atomics, every sum in a fixed order: the gradients are a pure function of the inputs.  Every element of grad_q and grad_kv
 * is written (no memset needed), nothing beside them.
 * grad_q or grad_kv may be NULL: that gradient is skipped together with the work that only serves it; both NULL is
 * PASNL_ENULL.  workspace: pasnl_cls_nl_attention_grad_workspace_bytes bytes = the rows' statistics only, lse2[b,p] (log-sum-
 * exp of the scores in the log2 domain) and delta[b,p]: 8 b p bytes (0 for an empty shape or an unsupported cb).
 * Checked in this order, before anything is enqueued: b, p >= 0 and n > 0, else PASNL_EINVAL; cb in {32, 64, 128}, else
 * PASNL_EUNSUPPORTED; b == 0 or p == 0 is a successful no-op (p == 0 with grad_kv given: grad_kv is zero-filled); NULL q, kv,
 * out, grad_out or workspace PASNL_ENULL; an operand or the workspace not 16-byte aligned, or b > 65535, PASNL_EUNSUPPORTED;
 * a short workspace PASNL_EWORKSPACE.
 * The names carry the pasnl_cls_ prefix, as pasnl_cls_nl_cell_input does, to stay outside the scope of tests/abi_cases.py,
 * whose symbol count is pinned; the entries are held to their buffers by tests/test_gpu_nl_grad.py instead. */
size_t pasnl_cls_nl_attention_grad_workspace_bytes(int b, int p, int n, int cb);
int pasnl_cls_nl_attention_grad(int b, int p, int n, int cb, const float* q, const float* kv, const float* out,
                                const float* grad_out, float* grad_q, float* grad_kv, void* workspace, size_t workspace_bytes,
                                pasnl_stream_t stream);

/* Deterministic backward of gather_point / group_point / three_interpolate: the gradient row of a source point is
 * the sum of its contributions in ascending order of the forward output element -- the order of the reference's
 * sequential CPU loop (tf_interpolate.cpp:131-153) -- so results are bit-reproducible (the reference's GPU kernels,
 * tf_sampling_g.cu:183-192 and tf_grouping_g.cu:61-78, scatter with atomicAdd and are not).  No fp atomics; every
 * destination row is written (no memset needed).  Out-of-range indices are ignored.
 * workspace: device memory of pasnl_grad_workspace_bytes(b, targets_per_cloud, contributions_per_cloud) bytes, where
 * (targets, contributions) = (n, m) for gather_point, (n, m*nsample) for group_point, (m, 3*n) for three_interpolate.
 * Argument meaning as the atomic versions above.  targets_per_cloud <= 38400 (LDS histogram). */
size_t pasnl_grad_workspace_bytes(int b, int targets, long contributions);
int pasnl_gather_point_grad_det(int b, int n, int m, const float* out_g, const int* idx, float* inp_g, void* workspace,
                                size_t workspace_bytes, pasnl_stream_t stream);
int pasnl_group_point_grad_det(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx,
                               float* grad_points, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);
int pasnl_three_interpolate_grad_det(int b, int n, int c, int m, const float* grad_out, const int* idx, const float* weight,
                                     float* grad_points, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Backward of the AdaptiveSampling cell's three parts that are not GEMMs (csrc/as_grad.hip): the micro attention, the
 * re-weighting tail and the gather.  No fp atomics, every sum in a fixed order: the gradients are a pure function of the inputs.
 * Every element of a gradient that is given is written (no memset needed), nothing beside it.
 * The names carry the pasnl_cls_ prefix, as pasnl_cls_nl_attention_grad does, to stay outside the scope of tests/abi_cases.py,
 * whose symbol count is pinned; the entries are held to their buffers by tests/test_gpu_as_grad.py instead.
 *
 * pasnl_cls_as_attention_grad: backward of pasnl_as_attention.  Per group, with K = kv[..., :cb], V = kv[..., cb:],
 * P = softmax_j(q_i . k_j / sqrt(cb)) over the `as` keys and g = grad_out (g,as,cb):
 *     dV = P^T g      dP = g V^T      delta_i = sum_j P_ij dP_ij      dS = P o (dP - delta)
 *     grad_q = dS K / sqrt(cb)        dK = dS^T Q / sqrt(cb)          grad_kv (g,as,2cb) = [dK | dV]
 * P is recomputed from q and kv: nothing of the forward is needed and there is no workspace.  One wave per group on the fp32
 * MFMA; as <= 16, any cb <= 256.  With as == 1 (P == 1) grad_q and the dK half are exact zeros.
 * grad_q or grad_kv may be NULL: that gradient's products are skipped; both NULL is PASNL_ENULL.
 * pasnl_cls_as_attention_qkv_grad: the same for pasnl_as_attention_qkv, kvq (g,as,3cb) = [K | V | Q] ->
 * grad_kvq (g,as,3cb) = [dK | dV | dQ], the whole row.
 * Checked in this order, before anything is enqueued: g >= 0, as > 0, cb > 0, else PASNL_EINVAL; as <= 16 and cb <= 256, else
 * PASNL_EUNSUPPORTED; g == 0 is a successful no-op; NULL q, kv (kvq), grad_out or no gradient to write, PASNL_ENULL. */
int pasnl_cls_as_attention_grad(int g, int as, int cb, const float* q, const float* kv, const float* grad_out, float* grad_q,
                                float* grad_kv, pasnl_stream_t stream);
int pasnl_cls_as_attention_qkv_grad(int g, int as, int cb, const float* kvq, const float* grad_out, float* grad_kvq,
                                    pasnl_stream_t stream);

/* pasnl_cls_as_reweight_grad: backward of pasnl_as_reweight.  With w[s,o] = softmax_s(logits[s,o]), X = grouped_xyz,
 * F = grouped_feature, gxyz = grad_new_xyz (g,3), gfeat = grad_new_feature (g,ch), and
 * t_s = sum_d gxyz[d] X[s,d] for o = 0, t_s = gfeat[o-1] F[s,o-1] for o >= 1:
 *     grad_logits[s,o] = w[s,o] (t_s - sum_r w[r,o] t_r)      dX[s,d] = w[s,0] gxyz[d]      dF[s,j] = w[s,1+j] gfeat[j]
 * Sums over the neighbours run in ascending s.  grad_logits (g,as,1+ch); grad_grouped_xyz (g,nsample,3) = dX and
 * grad_grouped_feature (g,nsample,ch) = dF, their rows as..nsample-1 written as zeros.  With as == 1 grad_logits is exact zeros.
 * pasnl_cls_as_reweight_x_grad: backward of pasnl_as_reweight_x, x (g,as,3+ch).  grad_x (g,as,3+ch): columns 0-2 are zeros,
 * column 3+j holds dF[s,j], and for j < 3 dX[s,j] is added to it (those columns of x are the coordinates AND the first three
 * features).
 * Any of the three (two) gradients may be NULL and is then skipped; all NULL is PASNL_ENULL.  grouped_xyz, grouped_feature
 * (x) are read for grad_logits only.
 * Checked in the order of the forward entries: g >= 0, as > 0, nsample >= as, ch > 0 (x form: ch > 3), else PASNL_EINVAL;
 * as <= 16, else PASNL_EUNSUPPORTED; g == 0 is a successful no-op; NULL logits, grad_new_xyz, grad_new_feature, no gradient
 * to write, or grad_logits without the grouped tensors (x), PASNL_ENULL. */
int pasnl_cls_as_reweight_grad(int g, int as, int nsample, int ch, const float* logits, const float* grouped_xyz,
                               const float* grouped_feature, const float* grad_new_xyz, const float* grad_new_feature,
                               float* grad_logits, float* grad_grouped_xyz, float* grad_grouped_feature, pasnl_stream_t stream);
int pasnl_cls_as_reweight_x_grad(int g, int as, int ch, const float* logits, const float* x, const float* grad_new_xyz,
                                 const float* grad_new_feature, float* grad_logits, float* grad_x, pasnl_stream_t stream);

/* pasnl_cls_as_gather_grad: backward of pasnl_as_gather, whose rows are [xyz[i_s] - xyz[i_0] | xyz[i_s] | feature[i_s]].
 * grad_x (b,m,as,6+c) is folded to one row per gathered point,
 *     r[j,s] = [gx[j,s,0:3] + gx[j,s,3:6] - (s == 0 ? sum_t gx[j,t,0:3] : 0) | gx[j,s,6:]]      (sum over t ascending)
 * and r is scattered to grad_xyz (b,n,3) and grad_feature (b,n,c) by the machinery of pasnl_group_point_grad_det: each source
 * point's row is the sum of its contributions in ascending order of the forward output element (j,s); every destination row
 * is written, a point no group drew gets exact zeros.  idx (b,m,k): only its first `as` columns are read.
 * grad_xyz or grad_feature may be NULL: that scatter is skipped; both NULL is PASNL_ENULL.
 * workspace: pasnl_cls_as_gather_grad_workspace_bytes bytes =
 *     pasnl_grad_workspace_bytes(b, n, m*as) + 4 b m as (1 + 3 + c)      (the lists; idx's first columns, r)
 * (0 for b <= 0, n <= 0, c <= 0, m < 0 or as <= 0).
 * Checked in this order, before anything is enqueued: b, m >= 0 and n, c, k, as > 0 and as <= k, else PASNL_EINVAL;
 * n <= 38400 (the lists' LDS histogram) and m*as < 2^31, else PASNL_EUNSUPPORTED; b == 0 is a successful no-op; no gradient
 * to write, or NULL grad_x / idx with b m as > 0, PASNL_ENULL; a NULL or short workspace PASNL_EWORKSPACE; a workspace that
 * is not 4-byte aligned PASNL_EUNSUPPORTED. */
size_t pasnl_cls_as_gather_grad_workspace_bytes(int b, int n, int c, int m, int as);
int pasnl_cls_as_gather_grad(int b, int n, int c, int m, int k, int as, const float* grad_x, const int* idx, float* grad_xyz,
                             float* grad_feature, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Backward of a set-abstraction layer's grouping and local cell (csrc/sa_grad.hip).  No fp atomics, every sum in a fixed order
 * that depends on the arguments alone (never on the device): the gradients are a pure function of the inputs.  Every element of
 * a gradient that is given is written (no memset needed), nothing beside it.  (pasnl_cls_ prefix: see above.)
 *
 * pasnl_cls_sa_local_cell_grad: backward of pasnl_sa_local_cell.  Per group, X = x[g] (k,w), dM = grad_out[g] (c2,32), and the
 * forward's H1 = relu(X W0 + b0), H2 = relu(H1 W1 + b1), G = relu(X[:,0:3] Ww + bw) recomputed (nothing of the forward is saved):
 *     dH2 = G dM^T     dG = H2 dM     dZ2 = dH2 o [H2 > 0]     dZg = dG o [G > 0]     dH1 = dZ2 W1^T     dZ1 = dH1 o [H1 > 0]
 *     grad_x = dZ1 W0^T,  grad_x[:,0:3] += dZg Ww^T
 *     grad_w1 = sum H1^T dZ2     grad_b1 = sum dZ2     grad_w0 = sum X^T dZ1     grad_b0 = sum dZ1
 *     grad_ww = sum X[:,0:3]^T dZg     grad_bw = sum dZg                        (sums over all groups and rows)
 * Shapes as the forward's: grad_x (groups,k,w), grad_w0 (w,c1), grad_b0 (c1), grad_w1 (c1,c2), grad_b1 (c2), grad_ww (3,32),
 * grad_bw (32).  One wave per group on the fp32 32x32x2 MFMA, weights in LDS.  The weight gradients are accumulated in
 * registers by min(groups, 1024) waves, wave s taking groups s, s + slots, ...; each flushes one partial slot and a second
 * launch sums the slots in ascending order.
 * Supported: k % 32 == 0, (c1,c2) = (32,32) or (64,64), 3 <= w <= 96.  Every kernel keeps its accumulators in registers (no
 * scratch); where the weight-gradient accumulators and grad_x's tiles do not fit the register file together -- (32,32) with
 * w > 64, (64,64) with w > 32 -- the call is two or three launches of the first kernel, each producing a part ({dW1, db1, dWw,
 * dbw}, {dW0, db0}, grad_x) from its own recomputed forward: the same bits as one launch.  Wider cells (128 and up), c1 != c2
 * and wider rows are PASNL_EUNSUPPORTED (the Python mirror then differentiates the op-by-op chain).
 * Any gradient pointer may be NULL.  grad_x == NULL skips the product dZ1 W0^T; with no weight gradient at all there are no
 * partials, no row-p transposes, no second launch and the workspace is not touched (it may be NULL); in a one-launch form the
 * six weight gradients are accumulated together and a NULL one among them is only not written, in the three-launch form a part
 * none of whose gradients is asked for is not run.  All seven NULL is PASNL_ENULL.
 * workspace: pasnl_cls_sa_local_cell_grad_workspace_bytes(groups, w, c1, c2) bytes =
 *     4 min(groups, 1024) (w c1 + c1 + c1 c2 + c2 + 96 + 32)        (0 for groups <= 0, w < 3, c1 <= 0 or c2 <= 0)
 * Checked in this order, before anything is enqueued: groups >= 0, k > 0, w >= 3, c1, c2 > 0, else PASNL_EINVAL; the supported
 * set above, else PASNL_EUNSUPPORTED; groups == 0 zero-fills the weight gradients given and is done; NULL x, a weight, a bias,
 * grad_out, or no gradient to write, PASNL_ENULL; with a weight gradient asked for, a workspace that is not 4-byte aligned
 * PASNL_EUNSUPPORTED, then a NULL or short one PASNL_EWORKSPACE. */
size_t pasnl_cls_sa_local_cell_grad_workspace_bytes(int groups, int w, int c1, int c2);
int pasnl_cls_sa_local_cell_grad(int groups, int k, int w, int c1, int c2, const float* x, const float* w0, const float* b0,
                                 const float* w1, const float* b1, const float* ww, const float* bw, const float* grad_out,
                                 float* grad_x, float* grad_w0, float* grad_b0, float* grad_w1, float* grad_b1, float* grad_ww,
                                 float* grad_bw, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* pasnl_cls_sa_group_grad: backward of pasnl_sa_group, new_point[j,s] = [xyz[i] - new_xyz[j] | xyz[i] | feature[i]],
 * i = idx[b,j,s], skip[j] = max_s new_point[j,s].  grad_new_point (b,m,k,6+c) and grad_skip (b,m,6+c); either may be NULL and
 * then counts as zeros.  The maximum follows TensorFlow's reduce_max rule: every element equal to its column's maximum gets
 * grad_skip / count, the comparison made on the forward's own float32 values (recomputed with the forward's expression).  With
 * e[j,s] = grad_new_point[j,s] + share[j,s]:
 *     r[j,s] = [e[0:3] + e[3:6] | e[6:]]          grad_new_xyz[j] = -sum_s e[j,s,0:3]      (s ascending)
 * and r is scattered to grad_xyz (b,n,3) and grad_feature (b,n,c) by the machinery of pasnl_group_point_grad_det: each source
 * point's row is the sum of its contributions in ascending order of (j,s); an index drawn twice in a group shares and then
 * re-sums at its point; every destination row is written, a point no group drew gets exact zeros.  grad_new_xyz (b,m,3).
 * Each of the three gradients may be NULL and is then skipped; all NULL is PASNL_ENULL.
 * workspace: pasnl_cls_sa_group_grad_workspace_bytes(b, n, c, m, k) bytes =
 *     pasnl_grad_workspace_bytes(b, n, m*k) + 4 b m k (3 + c)                  (the lists; r)
 * (0 for b <= 0, n <= 0, c <= 0, m < 0 or k <= 0); not touched, and may be NULL, when only grad_new_xyz is asked for.
 * Checked in this order, before anything is enqueued: b, m >= 0 and n, c, k > 0, else PASNL_EINVAL; n <= 38400 (the lists' LDS
 * histogram), m*k < 2^31 and b*m < 2^31, else PASNL_EUNSUPPORTED; b == 0 is a successful no-op; no gradient to write, or NULL
 * xyz / feature / idx / new_xyz with b m k > 0, PASNL_ENULL; with a scatter asked for, a workspace that is not 4-byte aligned
 * PASNL_EUNSUPPORTED, then a NULL or short one PASNL_EWORKSPACE. */
size_t pasnl_cls_sa_group_grad_workspace_bytes(int b, int n, int c, int m, int k);
int pasnl_cls_sa_group_grad(int b, int n, int c, int m, int k, const float* xyz, const float* feature, const int* idx,
                            const float* new_xyz, const float* grad_new_point, const float* grad_skip, float* grad_xyz,
                            float* grad_feature, float* grad_new_xyz, void* workspace, size_t workspace_bytes,
                            pasnl_stream_t stream);

/* Training-mode batch norm (csrc/bn_train.hip; reference utils/tf_util.py:512-531, batch_norm_template with is_training=True:
 * tf.contrib.layers.batch_norm(decay=bn_decay, updates_collections=None, epsilon 1e-3)).  x is a (rows, c) float32 matrix, row-
 * major, the channel last -- a GEMM's output; every statistic is over rows.  (pasnl_cls_ prefix: see above.)
 *
 * pasnl_cls_bn_train: per column j, in float64 from float64 sums of x and x^2,
 *     mean_j = sum_r x[r,j] / rows     var_j = max(sum_r x[r,j]^2 / rows - mean_j^2, 0)  (biased)     rstd_j = 1 / sqrt(var_j + eps)
 * rounded to float32 into save_mean (c) and save_rstd (c), and in float32, each operation rounded on its own,
 *     y[r,j] = act(((x[r,j] - mean_j) * rstd_j) * gamma_j + beta_j)                 act: 0 none, 1 ReLU
 * moving_mean / moving_var (c): both NULL = no update; else updated in place as assign_moving_average(zero_debias=False) does,
 *     m <- m - (m - batch) * (1 - decay)       batch = mean_j, and for the variance var_j * rows / max(rows - 1, 1) when
 * unbiased != 0 (TF's fused kernel, with its rows == 1 guard), else var_j.  y must not overlap x.
 *
 * pasnl_cls_bn_train_grad: with g = grad_y [y > 0] when act == 1, else grad_y (y is then not read and may be NULL), and
 * xhat = (x - save_mean) * save_rstd in float32:
 *     grad_beta_j = sum_r g[r,j]      grad_gamma_j = sum_r g[r,j] xhat[r,j]             (float64 sums, rounded to float32)
 *     grad_x[r,j] = (gamma_j * rstd_j) * ((g[r,j] - grad_beta_j / rows) - xhat[r,j] * (grad_gamma_j / rows))
 * grad_x == NULL skips that pass; grad_gamma and grad_beta are always written.  grad_x must not overlap an input.
 *
 * Deterministic: no atomics; a thread adds its rows in ascending order, a workgroup folds its threads by a fixed tree and writes
 * one float64 partial per column and slab into the workspace, a second launch adds the slabs in a fixed order: the results are
 * a pure function of the arguments.  16-byte accesses where c % 4 == 0 and x, y, grad_y, grad_x are 16-byte aligned, else 4-byte
 * ones.  rows <= 128 is ONE launch.
 * workspace (both entries): pasnl_cls_bn_train[_grad]_workspace_bytes(rows, c) =
 *     16 c min(ceil(rows / 256), max(1, 2048 / ceil(c / 256)))        (0 for rows <= 0 or c <= 0; integer division)
 * bytes, 8-byte aligned; its contents before the call do not matter.
 * Checked in this order, before anything is enqueued: rows >= 0, c > 0, act in {0, 1}, and for the forward eps > 0 and
 * 0 <= decay <= 1, else PASNL_EINVAL; rows == 0 is a successful no-op; a NULL matrix, vector or output (the forward: x, gamma,
 * beta, y, save_mean, save_rstd, or exactly one of the moving pair; the backward: x, y with act == 1, gamma, save_mean,
 * save_rstd, grad_y, grad_gamma, grad_beta) PASNL_ENULL; a matrix pointer that is not 4-byte aligned, a workspace that is not
 * 8-byte aligned, or rows > 2^40, PASNL_EUNSUPPORTED; a NULL or short workspace PASNL_EWORKSPACE. */
size_t pasnl_cls_bn_train_workspace_bytes(long rows, int c);
int pasnl_cls_bn_train(long rows, int c, const float* x, const float* gamma, const float* beta, float eps, float decay, int act,
                       int unbiased, float* moving_mean, float* moving_var, float* y, float* save_mean, float* save_rstd,
                       void* workspace, size_t workspace_bytes, pasnl_stream_t stream);
size_t pasnl_cls_bn_train_grad_workspace_bytes(long rows, int c);
int pasnl_cls_bn_train_grad(long rows, int c, const float* x, const float* y, const float* gamma, const float* save_mean,
                            const float* save_rstd, int act, const float* grad_y, float* grad_x, float* grad_gamma,
                            float* grad_beta, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* pasnl_cls_dropout (csrc/bn_train.hip; reference utils/tf_util.py:594-615, tf.nn.dropout(inputs, keep_prob) in training):
 *     y[i] = x[i] / keep_prob  where element i is kept, else 0            (float32 division; y may be x)
 * Element i is kept iff (w >> 8) * 2^-24 < keep_prob (float32, exact), w = word (i & 3) of the Philox4x32-10 block at
 *     key (seed lo, seed hi),  counter ((i >> 2) lo, (i >> 2) hi, call, stream_id)
 * -- the generator of pasnl_scan_augment.  No mask is stored: the backward is the same call on the incoming gradient with the
 * same (seed, stream_id, call).  TensorFlow's own generator is not reproduced.
 * Checked in this order, before anything is enqueued: n >= 0 and 0 < keep_prob <= 1, else PASNL_EINVAL; n == 0 is a successful
 * no-op; NULL x or y PASNL_ENULL; a pointer that is not 4-byte aligned, or n > 2^40, PASNL_EUNSUPPORTED. */
int pasnl_cls_dropout(long n, float keep_prob, unsigned long long seed, unsigned stream_id, unsigned call, const float* x, float* y,
                      pasnl_stream_t stream);

/* Tail of a set-abstraction layer, fused (pointasnl_util.py:258-261 skip connection, :213-216 back-projection of the
 * non-local cell, :282-290 the two adds and the aggregation layer):
 *   out = relu( ( after + relu(skip_max ws + bs) + relu(att wb + bb) ) wagg + bagg )
 * after (rows,c) = the after_conv output; skip_max (rows,w) = pasnl_sa_cell's skip maxima; att (rows,cb) = pasnl_nl_attention's
 * output (cb == 0 and att/wb/bb NULL for a layer without non-local cell); ws (w,c), wb (cb,c), wagg (c,c) and the biases are
 * the BN-folded `skip`, `conv_back_project`, `aggregation` layers; out (rows,c).  c % 32 == 0 and c <= 512, else
 * PASNL_EUNSUPPORTED (the Python mirror then runs the three GEMMs and two adds). */
int pasnl_sa_tail(int rows, int w, int cb, int c, const float* after, const float* skip_max, const float* att, const float* ws,
                  const float* bs, const float* wb, const float* bb, const float* wagg, const float* bagg, float* out,
                  pasnl_stream_t stream);

/* pasnl_sa_tail with the residual connection of the `_res` model in its epilogue (models/pointasnl_sem_seg_res.py:37,42,47,52:
 * l1_2_points += l1_1_points ...):  out = pasnl_sa_tail(...) + residual, residual (rows,c). */
int pasnl_sa_tail_res(int rows, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                      const float* ws, const float* bs, const float* wb, const float* bb, const float* wagg,
                      const float* bagg, const float* residual, float* out, pasnl_stream_t stream);

/* pasnl_sa_tail / _res / _cat with the three weight matrices PACKED in the matrix instruction's operand order (the kernel then
 * reads them in 16-byte pieces: 3-5 us per launch): pasnl_sa_tail_pack_weights(k, c, w, packed) once per variable into
 * pasnl_sa_tail_packed_weights_bytes(k, c) bytes (16-byte aligned): packed[((chunk * 2 + h) * c + col) * 16 + t] =
 * w[32 chunk + 2 t + h][col], zero beyond k.  residual (rows,c) or NULL; out_cat + new_xyz or NULL (see pasnl_sa_tail_cat).
 * out (rows,c); out_cat (rows,c+4) when given. */
size_t pasnl_sa_tail_packed_weights_bytes(int k, int c);
int pasnl_sa_tail_pack_weights(int k, int c, const float* w, float* packed, pasnl_stream_t stream);
int pasnl_sa_tail_packed(int rows, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                         const float* ws_packed, const float* bs, const float* wb_packed, const float* bb, const float* wagg_packed,
                         const float* bagg, const float* residual, const float* new_xyz, float* out_cat, float* out,
                         pasnl_stream_t stream);

/* pasnl_sa_tail that writes its rows a second time as out_cat (rows, c + 4) = [0 | new_xyz (rows,3) | out]: the
 * tf.concat([xyz, points]) the next group_all module starts with (pointnet_util.py:77-80, sample_and_group_all), one
 * zero column in front so that the rows stay 16-byte aligned (the consumer's weights get a zero row in front). */
int pasnl_sa_tail_cat(int rows, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                      const float* ws, const float* bs, const float* wb, const float* bb, const float* wagg,
                      const float* bagg, float* out, const float* new_xyz, float* out_cat, pasnl_stream_t stream);

/* Decoder local cell (PointASNLDecodingLayer, pointasnl_util.py:323-331): per point p of the dense level with its k
 * nearest neighbours i_s = idx[b,p,s] (self-kNN on xyz):
 *   F = [xyz[i_s] | feature[i_s]] (k,3+c);  G = relu((xyz[i_s]-xyz[p]) Ww + bw) (k,32);  out[b,p] = F^T G  (3+c,32)
 * = the input of the [1,3+c] `decode_after_conv` GEMM.  feature = the three_interpolate output (b,n,c); Ww (3,32), bw
 * (32) = decode_weight_net/wconv0 with inference BN folded.  Replaces two tf.gather_nd, a concat, a subtraction, a
 * conv2d, a transpose and a batched matmul; no grouped tensor in HBM.  k in {16, 32}. */
int pasnl_decode_cell(int b, int n, int c, int k, const float* xyz, const float* feature, const int* idx, const float* ww,
                      const float* bw, float* out, pasnl_stream_t stream);

/* The same cell with its (3+c)*32 output values per point in a TILED order, for a consumer that contracts all of them (the
 * `decode_after_conv` GEMM with its weight rows permuted to match): 4 full-width 1-KiB stores per 32-channel tile instead
 * of 16 256-byte ones and, for c % 128 == 0, one 16-byte feature load per neighbour and 128 features instead of four 4-byte
 * ones -- the plain kernel is bound by the vector-memory instructions it issues, not by bytes.  Position q of a point holds
 *     q < 96:                                        channel q / 32 (a coordinate), j = q % 32          (reference order)
 *     q = 96 + T*1024 + (2g+h)*128 + 4m + i:         channel 3 + 32 V (T / V) + V m + T % V,   j = 8g + 4h + i
 * with V = pasnl_decode_cell_tiled_v4(c, feature) ? 4 : 1, g < 4, h < 2, m < 32, i < 4.  k == 16 and c % 32 == 0, else
 * PASNL_EUNSUPPORTED. */
int pasnl_decode_cell_tiled(int b, int n, int c, int k, const float* xyz, const float* feature, const int* idx,
                            const float* ww, const float* bw, float* out, pasnl_stream_t stream);
int pasnl_decode_cell_tiled_v4(int c, const float* feature);

/* AdaptiveSampling with as_neighbor == 0 (pointasnl_util.py:161-164): new_xyz (b,m,3) = xyz[idx[b,j,0]] and
 * new_feature (b,m,3+c) = [xyz | feature][idx[b,j,0]], idx (b,m,k) the neighbour indices of the layer. */
int pasnl_take_neighbor0(int b, int n, int c, int m, int k, const float* xyz, const float* feature, const int* idx,
                         float* new_xyz, float* new_feature, pasnl_stream_t stream);

/* AdaptiveSampling without the grouped tensors (pointasnl_util.py:121-171):
 *   pasnl_as_gather: x (b,m,as,6+c) = [xyz[i_s]-xyz[i_0] | xyz[i_s] | feature[i_s]], i_s = idx[b,j,s], s < as -- the
 *     input of conv_kv_ds / conv_query_ds (concat(normalized_xyz, shift_group_points)); idx (b,m,k) with k >= as.
 *   pasnl_as_attention_qkv: as pasnl_as_attention on ONE tensor kvq (g,as,3*cb) = [K | V | Q] per row (the output of
 *     a single GEMM with the conv_kv_ds and conv_query_ds weights side by side).
 *   pasnl_as_reweight_x: as pasnl_as_reweight, reading coordinates and (xyz | feature) rows (ch = 3+c channels) from x. */
int pasnl_as_gather(int b, int n, int c, int m, int k, int as, const float* xyz, const float* feature, const int* idx, float* out,
                    pasnl_stream_t stream);
int pasnl_as_attention_qkv(int g, int as, int cb, const float* kvq, float* out, pasnl_stream_t stream);
/*   pasnl_as_attention_proj: the same attention with the projections fused in, for narrow inputs (w <= 15, cb = 32 or 64):
 *   x (g,as,w) = the rows pasnl_as_gather produces, wkvq (w,3*cb) / bkvq (3*cb) = the BN-folded [conv_kv_ds | conv_query_ds]
 *   weights (pointasnl_util.py:126-135); K, V, Q = x.wkvq + bkvq never reach memory. */
int pasnl_as_attention_proj(int g, int as, int cb, int w, const float* x, const float* wkvq, const float* bkvq, float* out,
                            pasnl_stream_t stream);
/*   pasnl_as_cell_narrow: the whole AdaptiveSampling cell of a narrow layer after the gather (pointasnl_util.py:112-173): the
 *   projections and the attention as above, then mlp2 (cb -> 32 -> 1+ch; wa (cb,32), ba (32), wb (32,1+ch), bb (1+ch), BN
 *   folded), the softmax over the neighbours and the re-weighted sums.  x (g,as,w) with w = 3 + ch <= 15 ->
 *   new_xyz (g,3), new_feature (g,ch). */
int pasnl_as_cell_narrow(int g, int as, int cb, int w, int ch, const float* x, const float* wkvq, const float* bkvq,
                         const float* wa, const float* ba, const float* wb, const float* bb, float* new_xyz, float* new_feature,
                         pasnl_stream_t stream);
/*   pasnl_as_cell_wide: the same cell for wide layers, after their projection GEMM: kvq (g,as,3*cb) = [K | V | Q] rows
 *   (any cb <= 144: the reference's widths are (3 + c) / 2 = 33, 65, ...), x (g,as,w) the gathered rows (for the re-weighted sums) -> new_xyz (g,3), new_feature (g,ch). */
int pasnl_as_cell_wide(int g, int as, int cb, int w, int ch, const float* kvq, const float* x, const float* wa, const float* ba,
                       const float* wb, const float* bb, float* new_xyz, float* new_feature, pasnl_stream_t stream);

/* pasnl_as_cell_wide on projection rows that are WIDER than 3 cb: kvq (g*as, ld), ld >= 3 cb, columns [K | V | Q | unused].
 * The reference's bottleneck widths are (3 + c) / 2 = 33, 65, ...: a GEMM with N = 195 runs at 38 TF where N = 224 runs at
 * 82 (measured, 98304 x 134 inputs), so the Python mirror pads the projection's weights with zero columns. */
int pasnl_as_cell_wide_ld(int g, int as, int cb, int w, int ch, const float* kvq, int ld, const float* x, const float* wa,
                          const float* ba, const float* wb, const float* bb, float* new_xyz, float* new_feature,
                          pasnl_stream_t stream);
int pasnl_as_reweight_x(int g, int as, int ch, const float* logits, const float* x, float* new_xyz, float* new_feature,
                        pasnl_stream_t stream);

/* Voxel-grid subsampling (utils/cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:4-106), the input
 * stage of the ScanNet / SemanticKITTI "grid" pipelines: points (n,3) [+ features (n,fdim)] [+ classes (n,ldim)] ->
 * one row per occupied voxel of edge sample_dl: barycentre, feature mean, majority label.  Voxel keys, fp32 sums in
 * input order and the barycentre / mean arithmetic follow the reference bit for bit; rows come out in ASCENDING VOXEL
 * KEY (the reference emits unordered_map iteration order) and a label tie goes to the smallest label (the reference:
 * first maximum in hash order).  Outputs are sized for n rows: out_points (n,3), out_features (n,fdim), out_classes (n,ldim)
 * i32; out_count (device int) receives the number of voxels, and the rows past it are NOT written.
 * workspace: pasnl_grid_subsample_workspace_bytes(n) bytes of device memory.  No host synchronisation. */
size_t pasnl_grid_subsample_workspace_bytes(long n);
int pasnl_grid_subsample(long n, int fdim, int ldim, const float* points, const float* features, const int* classes,
                         float sample_dl, float* out_points, float* out_features, int* out_classes, int* out_count,
                         void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* The search inside `crop_pc` (SemanticKITTI/semantic_kitti_dataset_grid.py:265-272): around ONE centre per crop, the k nearest
 * points of a scan -- sklearn `KDTree.query(center, k=num_point+buffer)` (:271) -- or every point within a radius --
 * `query_radius(center, r=in_radius)` (:269).  b crops; crop c searches the n points at points + c*scan_stride*3
 * (scan_stride = 0: every crop searches the same scan) around centres[c,:].  Ranking key: the squared distance
 * ((dx*dx)+(dy*dy))+(dz*dz) evaluated in DOUBLE on the float32 coordinates (what sklearn computes on its float64 copy of
 * the data), so the selected set is sklearn's; a tie at the k-th distance goes to the lowest indices (sklearn: tree visit
 * order).  radius > 0: the radius form, d2 <= radius*radius inclusive (k ignored); otherwise k[c] (device ints; NULL: kcap
 * for every crop) nearest, clamped to [0, min(n, kcap)].
 * -> out_idx (b,kcap) i32: the selected indices in ASCENDING INDEX order (crop_pc shuffles them at once, :274; sort by
 * out_d2 for KDTree.query's order), entries behind the count are not written; out_d2 (b,kcap) f64 their squared
 * distances (NULL: not wanted), entries behind the count not written either (a point with a NaN coordinate has d2 = NaN
 * and ranks behind +inf, lowest index first; its out_d2 is that NaN with the sign bit clear); out_count (b) i32: the number selected (radius form: the TRUE number within the radius,
 * which may exceed kcap -- only the first kcap by index are stored).
 * An exact radix selection on the 63 key bits (no tree), 8 launches, no host synchronisation.
 * workspace: pasnl_knn_crop_workspace_bytes(b, n) bytes (8 n per crop for the keys + histograms). */
size_t pasnl_knn_crop_workspace_bytes(int b, long n);
int pasnl_knn_crop(int b, long n, long scan_stride, const float* points, const float* centres, const int* k, int kcap,
                   double radius, int* out_idx, double* out_d2, int* out_count, void* workspace, size_t workspace_bytes,
                   pasnl_stream_t stream);

/* ---- The SemanticKITTI test loop on the device (SemanticKITTI/semantic_kitti_dataset_grid.py:192-245 `get_batch_gen('test')`
 * and test_semantic_kitti_grid.py:128-180 `ModelTester.test`).  S scans live in ONE flat buffer: points (N,3) f32, scan i
 * at rows [offsets[i], offsets[i+1]) (offsets (S+1) i64), its possibility at the same rows of a flat (N,) f64 buffer and
 * its votes at the same rows of a flat (N,C) float16 buffer (row addresses are 64-bit).  One crop is picked, cropped,
 * ordered and accounted by a chain of launches on one stream with no fork and no host synchronisation; the crop travels
 * between them as a device descriptor: */
typedef struct pasnl_scan_crop {
  long long offset;   /* first row of the scan in the flat buffers                  */
  int cloud;          /* cloud_ind (D:224)                                           */
  int pick;           /* pick_idx inside the scan (D:225)                            */
  int n;              /* the scan's point count                                      */
  int k;              /* num_point + buffer of this crop (D:270)                     */
  float cx, cy, cz;   /* the centre: points[offset + pick] (D:266)                   */
  int pad;
} pasnl_scan_crop_t;

/* Pick (D:224-225): cloud = argmin(min_possibility[0..S)), then pick = argmin(possibility of that scan) -- the FIRST index
 * among equal minima at both levels, numpy's NaN rule (the first NaN wins, -0 == +0).  k: ONE device int, this crop's
 * num_point + buffer (drawn on the host).  -> desc (one descriptor), out_cloud (one int, NULL: not wanted).  One
 * workgroup, a 64-bit (value, index) reduction. */
int pasnl_scan_pick(int s, const long long* offsets, const double* possibility, const double* min_possibility,
                    const float* points, const int* k, pasnl_scan_crop_t* desc, int* out_cloud, pasnl_stream_t stream);

/* pasnl_knn_crop's k form for b crops whose scan, centre and k are the descriptors desc[0..b) on the device (the same
 * kernels behind a template flag; results bit-identical to pasnl_knn_crop on the same scan, centre and k).  nmax: the
 * largest scan's count (the grid is sized for it; blocks past a crop's own count exit); kcap >= every desc[c].k.
 * workspace: pasnl_knn_crop_workspace_bytes(b, nmax) bytes. */
int pasnl_knn_crop_indirect(int b, long nmax, const float* points, const pasnl_scan_crop_t* desc, int kcap, int* out_idx,
                            double* out_d2, int* out_count, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* The rest of crop_pc (D:271-277) for b crops: rank the desc[c].k selected entries (idx ascending, d2 f64: the output of
 * pasnl_knn_crop_indirect, rows of kcap) by (d2, index) -- sklearn's nearest-first order, ties by the lowest index --
 * then out_select[c][j] = nearest_first[perm[c][j]] for j < num_point (perm (b,num_point) i32: the first num_point
 * entries of the host's rng.shuffle(arange(k)), D:287-291), and out_points[c][j] = points[offset + out_select[c][j]]
 * (the batch's (b,num_point,3) model input).  One workgroup per crop sorts in LDS: kcap <= 14336, else
 * PASNL_EUNSUPPORTED. */
int pasnl_crop_order_permute(int b, const pasnl_scan_crop_t* desc, const float* points, const int* idx, const double* d2, int kcap,
                             const int* perm, int num_point, int* out_select, float* out_points, pasnl_stream_t stream);

/* The possibility update of one crop (D:231-234), in the reference's dtypes: dists = ((dx*dx)+dy*dy)+dz*dz in f32 with
 * dx = (float)((double)x - (double)cx); delta = (1 - dists / max(dists))^2 in f32 (max propagates NaN);
 * possibility[idx] = possibility[idx] + (double)delta with the LAST occurrence of a repeated index winning (numpy
 * fancy-index +=); then min_possibility[cloud] = min(possibility of the scan) (NaN propagates).  select: (num_point) i32
 * indices into the scan.  win: nmax device ints, all -1 before the call and after it (pasnl_scan_scratch_init).
 * scratch: 4 device bytes.  Three launches. */
int pasnl_scan_possibility_update(int num_point, const pasnl_scan_crop_t* desc, const float* points, const int* select,
                                  double* possibility, double* min_possibility, int* win, float* scratch, pasnl_stream_t stream);

/* win := -1 for n ints (the scratch of the update and the vote). */
int pasnl_scan_scratch_init(long n, int* win, pasnl_stream_t stream);

/* The votes of b crops (T:147-154), crop after crop in batch order: probs = softmax(values[c][j]) in f32 (is_logits;
 * otherwise values are the probabilities), then for every class
 * new = fp16( (float)fp16(smooth_old * old) + smooth_new * probs ): smooth_old the float16 bits of fp16(test_smooth),
 * smooth_new = float32(1 - test_smooth); a repeated index within a crop: the last occurrence wins.  values (b,num_point,C)
 * f32; select (b,num_point) i32; cloud (b) i32 device; offsets (S+1) i64; test_probs: the flat (N,C) float16 buffer.
 * win: as in pasnl_scan_possibility_update.  Two launches per crop. */
int pasnl_scan_vote(int b, int num_point, int c, const float* values, int is_logits, const int* select, const int* cloud,
                    const long long* offsets, unsigned short smooth_old, float smooth_new, void* test_probs, int* win,
                    pasnl_stream_t stream);

/* proj_inds (D:168-169, 182-183: sklearn KDTree(sub).query(raw)): for each of n_raw raw points the nearest of n_sub
 * sub-sampled points by the f64 key ((dx*dx)+(dy*dy))+(dz*dz) of the f32 coordinates, ties to the LOWEST index (sklearn:
 * tree order).  A uniform grid of nx*ny*nz cells of edge h from (ox,oy,oz) (chosen by the caller; every sub point must lie
 * inside it) is counting-sorted, then every raw point searches rings of cells outwards until no unexamined cell can hold a
 * closer or tying point (a conservative margin of 1e-6 h).  workspace: pasnl_scan_reproject_workspace_bytes(n_sub, cells). */
size_t pasnl_scan_reproject_workspace_bytes(long n_sub, long cells);
int pasnl_scan_reproject(long n_sub, const float* sub, long n_raw, const float* raw, double ox, double oy, double oz, double h,
                         int nx, int ny, int nz, int* out_proj, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* Labels (T:165-180): pred = argmax over the float16 row probs[proj[j]] (C classes, the FIRST maximum; a NaN wins as in
 * numpy), out[j] = ((pred >> 16) << 16) + lut[pred & 0xFFFF] as uint32.  proj (n_raw) i32 in [0, n_sub) (NULL: the
 * identity); lut (nlut) i32 with nlut >= c. */
int pasnl_scan_labels(long n_raw, const int* proj, const void* probs, int c, const int* lut, int nlut, unsigned* out,
                      pasnl_stream_t stream);

/* ---- The ScanNet grid test and validation loops on the device (ScanNet/scannet_dataset_grid.py (D) :435-549
 * `get_batch_gen('test' | 'validation')`, ScanNet/test_scannet_grid.py (T) :95-229 `test_cloud_segmentation` and :231-448
 * `test_cloud_segmentation_on_val`).  S scenes live in ONE flat buffer as the scans above do: points (N,3) f32, colours
 * (N,F) f32, potentials (N,) f64 and votes (N,C-1) FLOAT32 at the rows [offsets[i], offsets[i+1]).  The crop centre is a
 * float64 position that is no point of the scene, so the descriptor is its own: */
typedef struct pasnl_scene_crop {
  long long offset;   /* first row of the scene in the flat buffers                  */
  int cloud;          /* cloud_ind (D:483)                                            */
  int pick;           /* point_ind inside the scene (D:484)                           */
  int n;              /* the scene's point count                                      */
  int k;              /* num_point + buffer of this crop (D:494-498)                  */
  double cx, cy, cz;  /* pick_point = float64(points[pick]) + noise (D:485-489)       */
} pasnl_scene_crop_t;

/* Pick (D:483-489): the two-level argmin of pasnl_scan_pick (first index among equals, numpy's NaN rule), then
 * centre = (double)points[offset + pick] + noise[0..3).  k: ONE device int; noise: THREE device doubles, the host's
 * rng.normal(scale=0.35, size=(1,3)).  -> desc (one descriptor), out_cloud (one int, NULL: not wanted).  One workgroup. */
int pasnl_scene_pick(int s, const long long* offsets, const double* potentials, const double* min_potentials,
                     const float* points, const int* k, const double* noise, pasnl_scene_crop_t* desc, int* out_cloud,
                     pasnl_stream_t stream);

/* pasnl_knn_crop_indirect around the float64 centres of desc[0..b) (`input_trees[...].query(pick_point, k)`, D:498): the
 * same kernels behind a template parameter, the key ((dx*dx)+(dy*dy))+(dz*dz) with dx = (double)x - cx.  With centres
 * that are float32 values the results are bit-identical to pasnl_knn_crop_indirect.  Ties at the k-th distance go to the
 * lowest index.  workspace: pasnl_knn_crop_workspace_bytes(b, nmax) bytes. */
int pasnl_knn_crop_scene(int b, long nmax, const float* points, const pasnl_scene_crop_t* desc, int kcap, int* out_idx,
                         double* out_d2, int* out_count, void* workspace, size_t workspace_bytes, pasnl_stream_t stream);

/* pasnl_scene_pick and pasnl_knn_crop_scene for ONE crop with the pick fused into the selection's init kernel: eight
 * launches instead of nine, the same results.  workspace: pasnl_knn_crop_workspace_bytes(1, nmax) bytes. */
int pasnl_scene_pick_crop(int s, const long long* offsets, const double* potentials, const double* min_potentials,
                          const float* points, const int* k, const double* noise, pasnl_scene_crop_t* desc, int* out_cloud,
                          long nmax, int kcap, int* out_idx, double* out_d2, int* out_count, void* workspace,
                          size_t workspace_bytes, pasnl_stream_t stream);

/* The rest of the crop (D:500-501, 519-539) for b crops: rank the selected entries by (d2, index) and apply perm as
 * pasnl_crop_order_permute does -> out_select (b,num_point) i32; then the model input out_input (b,num_point,W) f32 with
 * W = 3 + nfeat (+ 3 if abs_coords): xyz = (float)((double)p - c); the scene's colour row (colors (N,nfeat) f32, nfeat = 0:
 * none, colors may be NULL); abs_coords: (float)((double)xyz + c), the reference's three extra feature columns (D:539).
 * One workgroup per crop sorts in LDS: kcap <= 14336, else PASNL_EUNSUPPORTED. */
int pasnl_scene_order_gather(int b, const pasnl_scene_crop_t* desc, const float* points, const float* colors, int nfeat,
                             const int* idx, const double* d2, int kcap, const int* perm, int num_point, int abs_coords,
                             int* out_select, float* out_input, pasnl_stream_t stream);

/* The potential update of one crop (D:512-516) in the reference's dtypes, as pasnl_scan_possibility_update with the
 * distances taken against the float64 centre: dists in f32 from (float)((double)x - cx); delta = (1 - dists/max(dists))^2;
 * potentials[idx] += (double)delta (last occurrence of a repeated index); min_potentials[cloud] = np.min of the scene.
 * win: as in pasnl_scan_possibility_update.  ONE launch (one workgroup: maximum, update and minimum behind barriers). */
int pasnl_scene_potential_update(int num_point, const pasnl_scene_crop_t* desc, const float* points, const int* select,
                                 double* potentials, double* min_potentials, int* win, pasnl_stream_t stream);

/* The votes of b crops (T:141-149 / 283-291), crop after crop in batch order, into the FLOAT32 table of nc = C - 1 classes:
 * new = f32(smooth_old * old) + f32(smooth_new * probs) -- numpy's `python_float * float32_array`: smooth_old =
 * float32(test_smooth), smooth_new = float32(1 - test_smooth), two float32 products and one float32 sum.  is_logits: values
 * (b,num_point,nc+1) f32 and probs = softmax(values[..., 1:]) in f32 (T:95); otherwise values (b,num_point,nc) are the
 * probabilities.  A repeated index within a crop: the last occurrence wins.  nc <= 64.  Two launches per crop. */
int pasnl_scene_vote(int b, int num_point, int nc, const float* values, int is_logits, const int* select, const int* cloud,
                     const long long* offsets, float smooth_old, float smooth_new, float* test_probs, int* win,
                     pasnl_stream_t stream);

/* What the reference writes per cloud at a checkpoint (T:183-218 / 316-328, 409-433), for m output points: the row
 * r = proj[j] (NULL: j) of the scene's table probs (n,nc) f32; out_preds[j] = label_values[argmax(row with a zero inserted
 * at every l with ignored[l] != 0)] (nl label values, the FIRST maximum, numpy's NaN rule; the caller checks nc + the number
 * of ignored labels == nl); out_pots[j] = potentials[r] (NULL: not wanted; potentials: the SCENE's rows); out_probs (m,nc) =
 * row (NULL: not wanted).  nl <= 64. */
int pasnl_scene_labels(long m, const int* proj, const float* probs, int nc, const double* potentials, const int* label_values,
                       const int* ignored, int nl, int* out_preds, double* out_pots, float* out_probs, pasnl_stream_t stream);

/* sklearn.metrics.confusion_matrix(targets, preds, labels=label_values) (T:336, 395), ADDED to out (nl,nl) i64:
 * out[i][j] += #{targets == label_values[i] and preds == label_values[j]}; a point whose target or prediction is not a
 * listed value is dropped.  label_values distinct, nl <= 64.  Counters are private to a workgroup in LDS and flushed once
 * with 64-bit atomics (integers: exact and order-free). */
int pasnl_confusion_matrix(long n, const int* targets, const int* preds, const int* label_values, int nl, long long* out,
                           pasnl_stream_t stream);

/* ---- The grid training input loops on the device (csrc/grid_train.hip): the `'training'` split of get_batch_gen in
 * ScanNet/scannet_dataset_grid.py (D) :435-549 and SemanticKITTI/semantic_kitti_dataset_grid.py (K) :193-292, and
 * `tf_augment_input` with the colour drop (D:551-645, K:294-354).  The pick, crop, order and potential update are the test
 * loops' entries above; the tallies of train_scannet_grid.py:264-302 and train_semantic_kitti_grid.py:224-263 are
 * pasnl_block_train_score.  None of the three entries synchronises with the host. */

/* The descriptors of b crops whose scan and pick the host drew (K:216-221: `cloud_ind = i`,
 * `pick_idx = np.random.choice(len(pc), 1)`): desc[c] = {offset = offsets[cloud[c]], cloud[c], pick[c], n, k[c], centre =
 * points[offset + pick[c]]} over s scans.  cloud: b ints in HOST memory (the generator's scan order is the host's; they
 * travel as kernel arguments, so a captured launch holds the ones it was captured with), one outside [0, s) -> PASNL_EINVAL;
 * pick, k: b DEVICE ints each (staged draws).  A pick outside its scan writes n = 0, an empty crop (the caller checks its
 * picks before it stages them). */
int pasnl_scan_pick_given(int b, int s, const long long* offsets, const float* points, const int* cloud, const int* pick,
                          const int* k, pasnl_scan_crop_t* desc, pasnl_stream_t stream);

/* The labels and sample weights of b crops (D:525-531, K:222, 237-239): out_labels[c][j] = labels[offsets[cloud[c]] +
 * select[c][j]] with labels the flat (N,) i32 class indices beside the flat points, cloud (b) i32 on the device, select
 * (b,num_point) i32 indices into each crop's scan; out_weights[c][j] = weights[out_labels[c][j]], weights (nw) f32.  A label
 * outside [0, nw) is written as it is with weight 0 (the callers check the range once, where the reference would raise
 * IndexError).  weights == NULL: all-zero weights (the validation split, D:528-529).  b <= 65535.  One launch. */
int pasnl_scan_train_labels(int b, int num_point, const int* select, const int* cloud, const long long* offsets, const int* labels,
                            const float* weights, int nw, int* out_labels, float* out_weights, pasnl_stream_t stream);

/* tf_augment_input and the colour drop (D:586-645 with D:564-568, K:304-354) of b crops of (num_point, width) f32 rows, src ->
 * dst (src == dst allowed), one launch, one thread per point.  rotation: 1 'vertical', 0 'none' (else PASNL_EINVAL); scale_min <=
 * scale_max; anisotropic; sym_x, sym_y, sym_z; noise >= 0 (the stddev); color (the keep probability): columns 3..5 are
 * multiplied by keep when width >= 6, every further column is copied; width >= 3, b <= 65535.
 * Random numbers are Philox4x32-10 words: key (seed lo, seed hi), counter (j, item lo, item hi, stream), item = item0[0] + c
 * (item0: ONE device unsigned long long, the running number of the batch's first crop; seed: a host value); a uniform is u =
 * (w >> 8) * 2^-24 in [0,1).  Stream 0, per crop: j = 0 -> u_theta, u_sx, u_sy, u_sz; j = 1 -> u_symx, u_symy, u_symz, u_colour.
 * theta = u_theta * f32(2 pi); cos, sin = f32 of the double cosine and sine of (double)theta; s_i = scale_min + u_si *
 * (scale_max - scale_min), each operation rounded to f32 (u_sx for all axes unless anisotropic), negated where the axis'
 * symmetry is on and not (u_sym > 0.5) -- tf.round(u) * 2 - 1; keep = u_colour < color.  Stream 1, per point j: Box-Muller
 * normals in f32, (x, y) from words (0, 1) and z from words (2, 3) (its second value dropped): r = sqrt(-2 log(((wa >> 8) + 1)
 * * 2^-24)), (r cos, r sin)(2 pi (wb >> 8) 2^-24).  Then, in f32 with no contraction: x' = (x*c) + (y*s), y' = (y*c) - (x*s),
 * z' = z ('none': x' = x, y' = y); out_i = x'_i * s_i + f32(noise * normal_i).  TF's own generator and the summation order of
 * its matmul are not reproduced.  out_params (b,8) f32: theta, cos, sin, s0, s1, s2, keep, 0 ('none': 0, 1, 0); out_noise
 * (b,num_point,3) f32: the unit normals; either may be NULL. */
int pasnl_scan_augment(int b, int num_point, int width, const float* src, float* dst, int rotation, float scale_min, float scale_max,
                       int anisotropic, int sym_x, int sym_y, int sym_z, float noise, float color, unsigned long long seed,
                       const unsigned long long* item0, float* out_params, float* out_noise, pasnl_stream_t stream);

/* ---- The per-epoch evaluation of the grid pipelines on the device (csrc/grid_eval.hip): `eval_one_epoch` of
 * ScanNet/train_scannet_grid.py (S) :304-434 and SemanticKITTI/train_semantic_kitti_grid.py (K) :265-330.  The generators
 * are the entries above; the float32 IoU arithmetic on the (nl,nl) matrix stays on the host (one read-back per epoch).  None
 * of the three entries synchronises with the host.  `ignored`: nl ints in HOST memory (non-zero: the label is ignored),
 * read by the call; they travel as a kernel argument.  nl <= 64, else PASNL_EUNSUPPORTED; nc + the number of ignored labels
 * != nl -> PASNL_EINVAL. */

/* The per-crop confusions of a whole batch, summed (S:359-368, K:301-310), ADDED to out (nl,nl) i64, rows the truth.
 * is_logits: values (b,num_point,nc+1) f32 and probs = softmax(values[..., 1:]) in f32 (S:310, K:268), in the operation order
 * of pasnl_scene_vote's softmax; otherwise values (b,num_point,nc) f32 are the probabilities.  The prediction is np.argmax of
 * the float32 PROBABILITIES with a zero inserted at every ignored l (the first maximum, numpy's NaN rule: logits that round
 * to equal probabilities give the first index); truth (b,num_point) i32 class indices, one outside [0, nl) is dropped.
 * out[truth][prediction] += 1.  b <= 65535; b == 0 is a no-op.  ONE launch: rows staged through LDS in tiles of 256 at an odd
 * row stride, counters in LDS, one flush per workgroup with 64-bit integer atomics. */
int pasnl_scan_eval_confusion(int b, int num_point, int nc, const float* values, int is_logits, const int* truth, const int* ignored,
                              int nl, long long* out, pasnl_stream_t stream);

/* S:346-351 for b crops, crop after crop in batch order, into the FLOAT64 table val_probs ((N,nc) rows, scene c at row
 * offsets[c]): new = smooth_old * old + (double)(smooth_new * probs) -- numpy >= 2's `val_smooth * float64_array +
 * (1 - val_smooth) * float32_array`: a float64 product with smooth_old = val_smooth, a FLOAT32 product with smooth_new =
 * float32(1 - val_smooth), widened and added in float64; nothing is contracted.  values, is_logits, select, cloud, win: as in
 * pasnl_scene_vote (a repeated index within a crop: the last occurrence wins).  nc <= 64.  Two launches per crop. */
int pasnl_scene_eval_vote(int b, int num_point, int nc, const float* values, int is_logits, const int* select, const int* cloud,
                          const long long* offsets, double smooth_old, float smooth_new, double* val_probs, int* win,
                          pasnl_stream_t stream);

/* The voting evaluation of one scene (S:396-410): sub_preds[r] = np.argmax of row r of the scene's float64 table probs (n,nc)
 * with a zero inserted at every ignored l (an index into label_values; once per sub-sampled point, into the caller's (n,)
 * i32 buffer); then for the m evaluation points out[index of labels[j] in label_values][sub_preds[proj[j]]] += 1 into (nl,nl)
 * i64.  proj == NULL: j.  A label that is not a listed value is dropped (sklearn); proj[j] outside [0, n) is ignored.  m == 0:
 * sub_preds only; n == 0: a no-op.  Two launches. */
int pasnl_scene_eval_vote_confusion(long n, const double* probs, int nc, long m, const int* proj, const int* labels,
                                    const int* label_values, const int* ignored, int nl, int* sub_preds, long long* out,
                                    pasnl_stream_t stream);

/* ---- The radius form of the grid crops, `in_radius > 0` (csrc/radius_crop.hip): ScanNet/scannet_dataset_grid.py (D) :491-492
 * and SemanticKITTI/semantic_kitti_dataset_grid.py (K) :268-269, `query_radius(centre, r=in_radius)[0]` on the scan's sklearn
 * KDTree, and the lines that make a crop of the member list (D:500-501, 519-539, 692-703; K:274-283).  The crop shuffles
 * POSITIONS of that list and its length is the count, so the count goes to the host (one read-back per crop) between the two
 * entries. */

/* The per-chunk counts of the two members entries below: one int per chunk of 64 positions of the largest scan, per crop. */
size_t pasnl_scan_radius_workspace_bytes(int b, long nmax);

/* The member lists of b crops (K:268-269): crop c reads its scan and float32 centre from desc[c]; a point is a member when
 * ((dx*dx)+(dy*dy))+(dz*dz) <= radius*radius in DOUBLE with dx = (double)x - (double)cx -- the rule of pasnl_knn_crop's radius
 * form, sklearn's on its float64 copy; a NaN coordinate is no member.  order: a flat (N,) i32 array beside the flat points,
 * order[offset + p] the in-scan index of tree position p (np.asarray(tree.idx_array) of the reference's tree; NULL: the
 * identity); an entry outside [0, n) is skipped.  -> out_members[c*member_stride + j], j < out_count[c]: the members in
 * POSITION order (sklearn's order of query_radius), entries behind the count not written; out_count (b) i32 exact.
 * member_stride >= nmax (nothing is truncated), nmax: the largest scan's count (blocks past a crop's own count exit);
 * radius > 0 and not NaN, else PASNL_EINVAL.  Ballots and an exclusive scan over chunks of 64 positions, no atomics: three
 * launches, deterministic.  workspace: pasnl_scan_radius_workspace_bytes(b, nmax) bytes. */
int pasnl_scan_radius_members(int b, long nmax, const float* points, const pasnl_scan_crop_t* desc, double radius, const int* order,
                              int* out_members, long member_stride, int* out_count, void* workspace, size_t workspace_bytes,
                              pasnl_stream_t stream);

/* pasnl_scan_radius_members around the float64 centres of desc[0..b) (D:491-492: `query_radius(pick_point, r=in_radius)`): the
 * same kernels behind a template parameter, dx = (double)x - cx. */
int pasnl_scene_radius_members(int b, long nmax, const float* points, const pasnl_scene_crop_t* desc, double radius,
                               const int* order, int* out_members, long member_stride, int* out_count, void* workspace,
                               size_t workspace_bytes, pasnl_stream_t stream);

/* The rest of crop_pc (K:274-283) for b crops: out_select[c][j] = members[c*member_stride + perm[c][j]] for j < num_point and
 * out_points[c][j] = points[offset + out_select[c][j]], as pasnl_crop_order_permute writes them.  perm (b,num_point) i32: the
 * host's composition of `shuffle_idx`, `[:num_point]` and the duplicated rows (K:277-281).  count (b) i32 is read on the
 * device (the output of the members entry): a perm entry outside [0, count[c]) leaves its row and its select entry
 * unwritten, and nothing behind the count is read.  One launch. */
int pasnl_scan_radius_gather(int b, const pasnl_scan_crop_t* desc, const float* points, const int* members, long member_stride,
                             const int* count, const int* perm, int num_point, int* out_select, float* out_points,
                             pasnl_stream_t stream);

/* The rest of the ScanNet crop (D:500-501, 519-539 with data_rep, D:692-703): the select rule of pasnl_scan_radius_gather, and
 * the model input rows out_input (b,num_point,W) f32 under pasnl_scene_order_gather's contract -- xyz relative to the float64
 * centre, the colour row (nfeat = 0: none, colors may be NULL), abs_coords. */
int pasnl_scene_radius_gather(int b, const pasnl_scene_crop_t* desc, const float* points, const float* colors, int nfeat,
                              const int* members, long member_stride, const int* count, const int* perm, int num_point,
                              int abs_coords, int* out_select, float* out_input, pasnl_stream_t stream);

/* ---- The ScanNet sliding-window whole-scene test loop on the device (ScanNet/scannet_dataset.py (D) :183-300
 * `ScannetDatasetWholeSceneSlidingWindow.__getitem__`, ScanNet/test_scannet.py (T) :96-103 `add_vote` and :107-196
 * `eval_one_epoch`).  One scene at a time: xyz (n,3) f32 is the scene's OWN buffer, moved in place vote after vote as the
 * reference moves scene_points_list[index]; colours (n,nfeat) f32 never move.  The numpy RNG stream and the merge of small
 * blocks (D:244-269, over counts and centres only) stay on the host.  n <= 2^30; coordinates are finite. */

/* The noise step (D:192-212).  centroid = np.mean(xyz, axis=0) as numpy computes it for a float32 (n,3) view: per column ONE
 * float32 sum in index order (a dependent chain: tiles staged in LDS, the x, y and z chains in three lanes), divided by
 * float32(n); max_length = max(|max|, |min|) of the float32 xyz - centroid over all three columns.  Then for every draw j
 * with last[j] != 0: i = choices[j], xyz[i] = float32((float64(float32((xyz[i] - centroid) / max_length)) + shift[j]) *
 * float64(max_length) + float64(centroid)) and stamp[i] = serial (semantic_seg_ini[choices] = 0 for this call: a label reads
 * as 0 while its stamp equals the call's serial).  choices (m) i32 in [0,n): the host's rng.choice(n, m); shift (m,3) f64:
 * (rng.randn(m,3) - 0.5) / 0.5 * 0.002; last (m) u8: 1 where no later draw names the same point (numpy's fancy assignment
 * keeps that one; every value is read before any store).  -> stats[0..3) centroid, stats[3] max_length (device floats).
 * Two launches. */
int pasnl_window_noise(long n, float* xyz, int m, const int* choices, const double* shift, const unsigned char* last, int serial,
                       int* stamp, float* stats, pasnl_stream_t stream);

/* coordmin / coordmax (D:214-215): out_bounds[0..3) = np.min(xyz, axis=0), out_bounds[3..6) = np.max(xyz, axis=0).  One
 * workgroup. */
int pasnl_window_bounds(long n, const float* xyz, float* out_bounds, pasnl_stream_t stream);

/* Window membership (D:223-233), counted.  Window w = i * ny + j (i < nx, j < ny, the reference's loop order) has
 * curmin = float64(coordmin) + [i * delta, j * delta, 0] and curmax = curmin + [1.5, 1.5, float32(coordmax_z - coordmin_z)];
 * a point is a member when its float32 coordinates are >= curmin - 0.2 and <= curmax + 0.2 on all three axes, compared in
 * float64 exactly so (every window of an axis is tested: no index comes out of a division).  bounds: the six device floats
 * of pasnl_window_bounds.  hist: pasnl_window_hist_bytes(n, nx, ny) device bytes -- per window and chunk of 64 consecutive
 * points the member count (cleared, then a wave ballot: a wave stores only for the windows round its own points), then
 * scanned in place per window to the count in earlier chunks; it is the input of pasnl_window_fill.  -> out_counts (nx*ny)
 * i32, empty windows included.  No limit per axis: nx * ny <= INT_MAX, else PASNL_EUNSUPPORTED (pasnl_window_hist_bytes: 0).
 * A clear and two launches. */
size_t pasnl_window_hist_bytes(long n, int nx, int ny);
int pasnl_window_count(long n, const float* xyz, const float* bounds, int nx, int ny, double delta, int* hist, int* out_counts,
                       pasnl_stream_t stream);

/* The member lists (D:229-241), each written straight to its place in the concatenation the host's merge decided
 * (D:263-268): window w's members, in ascending scene index, go to out_idx[woff[w] ...] (woff (nx*ny) i32, -1: skip the
 * window), and out_mask[...] is the 0.001-margin test of D:234 (the sample weight of every split but 'train').  A member's
 * rank is its chunk's scanned count plus the members among the lower lanes of its wave: deterministic, no arrival order.
 * cap: the length of out_idx / out_mask (nothing is written at or past it). */
int pasnl_window_fill(long n, const float* xyz, const float* bounds, int nx, int ny, double delta, const int* hist, const int* woff,
                      long cap, int* out_idx, unsigned char* out_mask, pasnl_stream_t stream);

/* Rows (D:271-300): rowpos (real_rows,block_points) i32 holds, per row entry, the position in the concatenated lists that
 * the host's shuffles chose (D:281-289); entry e gets i = cat_idx[rowpos[e]] and out_data[e] = xyz[i] | rgb[i] (3 + nfeat
 * f32), out_label[e] = labels[i], or 0 where stamp[i] == serial (D:211), out_weight[e] = cat_mask[rowpos[e]] (i32 0/1),
 * out_idx[e] = i.  Rows real_rows..rows-1 are written as zeros: the reference leaves stale data in the unused rows of a
 * scene's last batch (T:147-150) and never votes them. */
int pasnl_window_gather(int rows, int real_rows, int block_points, const int* rowpos, long cap, const int* cat_idx,
                        const unsigned char* cat_mask, long n, const float* xyz, const float* rgb, int nfeat, const int* labels,
                        const int* stamp, int serial, float* out_data, int* out_label, int* out_weight, int* out_idx,
                        pasnl_stream_t stream);

/* The vote (T:159-161 with add_vote, T:96-103): for every entry with weight != 0, pred = argmax(logits[e][1:]) + 1 (the
 * FIRST maximum, numpy's NaN rule) and pool[idx[e]][pred] += 1.  logits (rows,block_points,c) f32; pool (n,c) i32: integer
 * counters, exact and order-free (no float atomics).  c >= 2. */
int pasnl_window_vote(int rows, int block_points, int c, const float* logits, const int* idx, const int* weight, long n, int* pool,
                      pasnl_stream_t stream);

/* pred_label = np.argmax(vote_label_pool, 1) (T:163): the FIRST maximum of every row of pool (n,c) i32; a row without a
 * vote gives 0.  The counts of T:164-170 follow from pasnl_confusion_matrix over (labels, pred_label). */
int pasnl_window_pool_labels(long n, int c, const int* pool, int* out_labels, pasnl_stream_t stream);

/* ---- The SemanticKITTI sliding-window whole-scan test loop on the device (SemanticKITTI/semantic_kitti_dataset.py (D)
 * :278-355 `SemanticKittiDatasetSlidingWindow.__getitem__`, SemanticKITTI/test_semantic_kitti.py (T) :99-105 `add_vote` and
 * :108-231 `eval_one_epoch`).  One scan at a time: xyz (n,3) f32 never moves (there is no noise step), remission (n) f32 is
 * optional.  coordmin / coordmax (D:289-290) come from pasnl_window_bounds, the vote (T:166, T:99-105) is pasnl_window_vote
 * with a weight buffer of ones and final_preds (T:174-175) is pasnl_window_pool_labels: both are general in c.  The numpy RNG
 * stream and the merge of small blocks (D:311-327, over counts and centres only, empty windows included) stay on the host.
 * n <= 2^30; coordinates are finite. */

/* Window membership (D:296-302), counted.  Window w = i * ny + j (i < nx, j < ny, the reference's loop order) has
 * curmin = float64(coordmin) + [i * stride, j * stride, 0] and curmax = curmin + [block, block, float64(float32(coordmax_z -
 * coordmin_z))]; a point is a member when its float32 coordinates, widened to float64, are >= curmin - 0.2 and <= curmax +
 * 0.2 on all three axes (every window of an axis is tested with exactly these comparisons: no index comes out of a
 * division; along an axis the members are one contiguous range lo..hi because both bounds are monotone in i).  bounds: the
 * six device floats of pasnl_window_bounds.  hist: pasnl_kwindow_hist_bytes(n, nx, ny) device bytes -- cleared, then per
 * window and chunk of 64 consecutive points the member count (a wave ballot; a wave stores only for the windows inside the
 * rectangle of its points' ranges that hold one of them), then scanned in place per window to the count in earlier chunks; it
 * is the input of pasnl_kwindow_fill.  -> out_counts (nx*ny) i32, 0 for an empty window.  No limit per axis: nx * ny <=
 * INT_MAX, else PASNL_EUNSUPPORTED (pasnl_kwindow_hist_bytes: 0).  A clear and two launches. */
size_t pasnl_kwindow_hist_bytes(long n, int nx, int ny);
int pasnl_kwindow_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, int* hist,
                        int* out_counts, pasnl_stream_t stream);

/* The member lists (D:300-307, curchoice_idx), each written straight to its place in the concatenation the host's merge
 * decided (D:325-326): window w's members, in ascending scan index, go to out_idx[woff[w] ...] (woff (nx*ny) i32, -1: skip
 * the window).  A member's rank is its chunk's scanned count plus the members among the lower lanes of its wave:
 * deterministic, no arrival order.  cap: the length of out_idx (nothing is written at or past it). */
int pasnl_kwindow_fill(long n, const float* xyz, const float* bounds, int nx, int ny, double block, double stride, const int* hist,
                       const int* woff, long cap, int* out_idx, pasnl_stream_t stream);

/* Rows (D:334-351) as a batch is fed (T:149-161): rowpos (real_rows,block_points) i32 holds, per row entry, the position in
 * the concatenated lists that the host's shuffles chose (D:337-345); entry e gets i = cat_idx[rowpos[e]], out_data[e] =
 * xyz[i] followed by remission[i] when nfeat == 1 (3 + nfeat f32; nfeat is 0 or 1) and out_idx[e] = i.  Rows
 * real_rows..rows-1 are written as zeros: the reference leaves stale data in the unused rows of a scan's last batch (T:157)
 * and never votes them.  angles (rows) f64 or NULL: rotate_point_cloud_z (utils/provider.py:71-89) per row, xyz @ [[cos, sin,
 * 0], [-sin, cos, 0], [0, 0, 1]] computed in float64 from the cos and sin of the host's angle and rounded to float32 (within
 * one float32 ulp of numpy's product, whose dgemm fixes no summation order). */
int pasnl_kwindow_gather(int rows, int real_rows, int block_points, const int* rowpos, long cap, const int* cat_idx, long n,
                         const float* xyz, const float* remission, int nfeat, const double* angles, float* out_data, int* out_idx,
                         pasnl_stream_t stream);

/* ---- The ModelNet40 classification evaluation loop on the device (modelnet_dataset.py (D) :9-37 `pc_normalize` and
 * `farthest_point_sample`, :79-136 `_get_item` / `next_batch`; test.py (T) :105-174 `eval_one_epoch`; utils/provider.py (P)
 * :8-24 `normalize_data`).  All raw shapes live in one flat (total_rows, ld) f32 buffer, shape `id` at rows row0[id] ..
 * row0[id] + nraw[id]; the prepared set is (n_shapes, npoint, ch) f32 beside it.  The numpy RNG stream stays on the host.
 * Coordinates are finite. */

/* farthest_point_sample (D:16-37) for s raw shapes at once, one workgroup each: NOT the TF sampler of
 * pasnl_farthest_point_sample (start 0, another tie rule).  Call-shape j is shape ids[j] (ids NULL: j) and starts at
 * start[j], the host's randint(0, N).  float32 as numpy runs it on the float32 rows: dx = x - cx, d = (dx*dx + dy*dy) + dz*dz
 * without contraction, the running distance starts at 1e10 and is replaced only by a strictly smaller d, the next pick is
 * np.argmax (the FIRST index among equal maxima).  Columns 0..2 of the ld-wide rows are read.  -> out_idx (n_shapes,npoint)
 * i32 and / or out_rows (n_shapes,npoint,out_ld) f32, the picked rows' first out_ld columns (point[centroids]); both are
 * indexed by the shape's id; either may be NULL.  n_min / n_max: the smallest and largest nraw among the shapes of the call,
 * as the host knows them (a shape outside them, or outside its buffer, is skipped): npoint > n_min -> PASNL_EINVAL (the
 * reference fails at the batch assignment); n_max > pasnl_modelnet_fps_cap() = 12288 rows, what fits the workgroup's LDS ->
 * PASNL_EUNSUPPORTED (T:50 asserts NUM_POINT <= 10000, the raw shapes' size). */
int pasnl_modelnet_fps_cap(void);
int pasnl_modelnet_fps(int s, int npoint, int ld, long n_shapes, const int* ids, const long* row0, const int* nraw, const int* start,
                       int n_min, int n_max, long total_rows, const float* raw, int* out_idx, float* out_rows, int out_ld,
                       pasnl_stream_t stream);

/* pc_normalize (D:9-14) in place on columns 0..2 of s shapes (ids[j], or j) of data (n_shapes,npoint,ld) f32, numpy's bits:
 * centroid = per column ONE float32 sum down the rows divided by float32(npoint) (np.mean(axis=0), the chain of
 * pasnl_window_noise), pc - centroid, m = max(sqrt((x*x + y*y) + z*z)) in float32, pc / m.  One workgroup per shape. */
int pasnl_modelnet_normalize(int s, int npoint, int ld, long n_shapes, const int* ids, float* data, pasnl_stream_t stream);

/* next_batch into the persistent batch (D:124-136, T:135-136): row i < bsize of batch (b,npoint,ch) f32 becomes prepared shape
 * order[start + i] and labels[i] (b) i32 its class shape_labels[...]; rows bsize..b-1 of both are NOT touched -- in the last
 * batch of an epoch they still hold the batch before it, as in the reference.  order (n_order) i32: the dataset's idxs.  ch is
 * 3 or 6. */
int pasnl_modelnet_batch(int b, int bsize, int npoint, int ch, const int* order, long n_order, long start, long n_shapes,
                         const float* prepared, const int* shape_labels, float* batch, int* labels, pasnl_stream_t stream);

/* The training loop's input side (train.py:224-241 with utils/provider.py (P) :39-253): next_batch fused with the whole
 * augmentation chain, one launch.  For i < bsize and j < npoint, row (i, j) of batch (b,npoint,ch) f32 is computed from ONE row
 * of prepared shape order[start + i], and labels[i] is that shape's class; rows bsize..b-1 of both are NOT touched (the short
 * last batch keeps the augmented batch before it, train.py:214,240).  Only RNG draws come from the host: mats (bsize,2,9) f64,
 * row-major, per cloud the rotation about y (P:61-66, 99-104) then R = Rz.Ry.Rx of the perturbation (P:120-130, 190-200), or
 * NULL when rotation is off; scale (bsize) f64 (P:241); shift (bsize,3) f64 (P:227); perm (npoint) i32, the batch's one
 * shuffled arange (P:47-49); ratio (bsize) f64 (P:249) and u (bsize,npoint) f64 (P:250).  The source row is perm[0] when
 * u[i][j] <= ratio[i] (a tie drops) and perm[j] otherwise: the shuffle precedes the dropout, so P:252's first point is row
 * perm[0] of the unshuffled cloud after every other step.  float64 arithmetic in train.py:226-237's order, every product
 * (x0*M[0][c] + x1*M[1][c]) + x2*M[2][c]: ch = 6, rotation: float32((x @ A) @ R) for xyz and normal alike (P:107 stays float64,
 * P:118 is float32); ch = 3, rotation: float32(float32(x @ A) @ R) (P:59 is float32); then on columns 0..2
 * float32(float64(x) * scale) and float32(float64(that) + shift[c]) -- numpy >= 2's in-place float32 ops with float64
 * operands.  Rotation off: float32((x * scale) + shift[c]) on columns 0..2, one rounding at the feed; normals are copied.
 * A perm entry outside [0, npoint) or an order entry outside [0, n_shapes) leaves its rows unwritten.  bsize > b, start +
 * bsize > n_order, npoint < 1 or ch not 3 or 6 -> PASNL_EINVAL. */
int pasnl_modelnet_augment(int b, int bsize, int npoint, int ch, const int* order, long n_order, long start, long n_shapes,
                           const float* prepared, const int* shape_labels, const double* mats, const double* scale,
                           const double* shift, const int* perm, const double* ratio, const double* u, float* batch, int* labels,
                           pasnl_stream_t stream);

/* The noisy points (T:129-132 with normalize_data, P:8-24): uniforms (bsize,k,3) f64 as the host drew them; each (k,3) block
 * is normalised in float64 -- per column one sum down the rows / float64(k), subtracted, divided by
 * max(sqrt((x*x + y*y) + z*z)) -- rounded to float32 (the feed into a float32 placeholder) and written to rows 0..k-1,
 * columns 0..2 of batch rows 0..bsize-1.  Other columns and rows are not touched.  k = 1 gives 0/0 = NaN, as numpy does.
 * 1 <= k <= npoint. */
int pasnl_modelnet_noise(int bsize, int k, const double* uniforms, int npoint, int ch, float* batch, pasnl_stream_t stream);

/* One vote (T:147-149): sums (b,c) f64 += float64(logits (b,c) f32) over ALL b rows (numpy's float64 += float32), and
 * loss[1] += the batch's mean sparse-softmax cross-entropy over all b rows, stale ones included (a log-sum-exp shifted by the
 * row maximum in float32, the mean in float64: compared under a tolerance, never by bits).  loss: two f64, {loss_sum,
 * loss_vote}. */
int pasnl_cls_vote(int b, int c, const float* logits, const int* labels, double* sums, double* loss, pasnl_stream_t stream);

/* The end of a batch (T:150-162): preds[i] = np.argmax(sums[i]) (the FIRST maximum) for rows i < bsize; totals[0]
 * (total_correct) += matches, totals[1] (total_seen) += bsize, totals[2] (total_object) += b; seen_class / correct_class (c)
 * count the rows' labels; loss[0] += loss[1] / num_votes and loss[1] = 0; sums are cleared.  All counters i64. */
int pasnl_cls_tally(int b, int bsize, int c, int num_votes, const int* labels, double* sums, long long* totals, long long* seen_class,
                    long long* correct_class, int* preds, double* loss, pasnl_stream_t stream);

/* ---- ScanNet's training-time validation loops on the device (ScanNet/scannet_dataset.py (D) :31-64
 * `ScannetDataset.__getitem__` and :92-129 `ScannetDatasetWholeScene.__getitem__`; ScanNet/train_scannet.py (T) :279-329
 * `eval_one_epoch` and :333-420 `eval_whole_scene_one_epoch`; utils/provider.py (P) :8-24 `normalize_data` and :71-89
 * `rotate_point_cloud_z`).  One scene at a time: xyz (n,3) f32 never moves, labels (n) i32 in [0,c); coordmin / coordmax
 * (D:37-38, D:98-99) are the six device floats of pasnl_window_bounds.  The numpy RNG stream, the acceptance test of a try
 * (D:55, two Python-float comparisons on three integers) and the carry-over of rows between scenes (T:357-382, over row
 * counts only) stay on the host.  n <= 2^30; coordinates are finite. */

/* The keys the voxel bitmap distinguishes (2^19): bitmap buffers hold 1 + capacity / 32 device words. */
int pasnl_block_key_capacity(void);

/* One try of the chopped-scene crop (D:41-55), counted in one pass over the scene.  The centre is read on the device:
 * curcenter = xyz[centre], curmin = float64(curcenter) - [0.75, 0.75, .], curmax = float64(curcenter) + [0.75, 0.75, .],
 * curmin[2] = float64(coordmin_z), curmax[2] = float64(coordmax_z).  A point is a member when its float32 coordinates,
 * widened, are >= curmin - 0.2 and <= curmax + 0.2 on all three axes, compared in float64 exactly so (D:46); the mask of D:52
 * is the same test with 0.01.  For the masked members the voxel key is the reference's float64 expression, operation for
 * operation: v = ceil((p - curmin) / (curmax - curmin) * [31, 31, 62]), key = vx * 31.0 * 62.0 + vy * 62.0 + vz -- a key,
 * not a cell triple: distinct triples that share a key count once, as under np.unique.  Keys are counted with a bitmap over
 * [key_lo, key_lo + span) that the host sizes from the extents (a workgroup sets bits in LDS, OR-merges them into `bitmap`,
 * and a last pass takes the popcount); span > pasnl_block_key_capacity() -> PASNL_EUNSUPPORTED.  hist:
 * pasnl_window_hist_bytes(n, 2, 1) device bytes -- per chunk of 64 consecutive points the member count and the count of
 * members with label > 0 (wave ballots), each scanned in place to the count in earlier chunks; the first row is the input
 * of pasnl_block_fill.  -> out_stats (4) i32: m = len(cur_semantic_seg), np.sum(cur_semantic_seg > 0), len(np.unique(keys)),
 * and a flag that is non-zero when a key fell outside the span or was NaN (the count is then not to be used).  A clear and
 * three launches. */
int pasnl_block_crop_stats(long n, const float* xyz, const int* labels, const float* bounds, long centre, long long key_lo, long span,
                           int* hist, unsigned int* bitmap, int* out_stats, pasnl_stream_t stream);

/* The whole-scene columns (D:105-113), counted.  Column w = i * ny + j (i < nx, j < ny, the reference's loop order) has
 * curmin = float64(coordmin) + [i * 1.5, j * 1.5, 0] and curmax = float64(coordmin) + [(i + 1) * 1.5, (j + 1) * 1.5,
 * float32(coordmax_z - coordmin_z)] -- the upper bound is NOT curmin + 1.5 as in pasnl_window_count, and rounds
 * differently; membership is the 0.2-margin test of pasnl_block_crop_stats.  hist: pasnl_window_hist_bytes(n, nx, ny) device
 * bytes, as in pasnl_window_count.  -> out_counts (nx*ny) i32, empty columns included.  No limit per axis: nx * ny <=
 * INT_MAX, else PASNL_EUNSUPPORTED.  A clear and two launches. */
int pasnl_block_grid_count(long n, const float* xyz, const float* bounds, int nx, int ny, int* hist, int* out_counts,
                           pasnl_stream_t stream);

/* The member lists (D:47-52, D:110-115): column w's members, in ascending scene index, go to out_idx[woff[w] ...] (woff
 * (nx*ny) i32, -1: skip the column) and out_mask[...] is the inner-margin test -- 0.01 for the chopped column (centre >= 0,
 * nx = ny = 1, hist from pasnl_block_crop_stats of the same centre), 0.001 for the grid (centre < 0, hist from
 * pasnl_block_grid_count).  A member's rank is its chunk's scanned count plus the members among the lower lanes of its
 * wave: deterministic, no arrival order.  cap: the length of out_idx / out_mask (nothing is written at or past it). */
int pasnl_block_fill(long n, const float* xyz, const float* bounds, long centre, int nx, int ny, const int* hist, const int* woff, long cap,
                     int* out_idx, unsigned char* out_mask, pasnl_stream_t stream);

/* Rows (D:58-63, D:116-122): rowpos (rows,block_points) i32 holds, per row entry, woff[w] + the host's rng.choice(count_w,
 * block_points) draw; entry e gets i = cat_idx[rowpos[e]], out_data[e] = xyz[i] | rgb[i] (3 + nfeat f32), out_label[e] =
 * labels[i] and out_smpw[e] = float32(labelweights[labels[i]] * cat_mask[rowpos[e]]) (labelweights (c) f64; the float64
 * product as the reference forms it, rounded as the float32 batch rounds it). */
int pasnl_block_gather(int rows, int block_points, const int* rowpos, long cap, const int* cat_idx, const unsigned char* cat_mask, long n,
                       const float* xyz, const float* rgb, int nfeat, const int* labels, int c, const double* labelweights,
                       float* out_data, int* out_label, float* out_smpw, pasnl_stream_t stream);

/* normalize_data (P:8-24), then optionally rotate_point_cloud_z (P:71-89), for rows blocks of src (rows,block_points,width)
 * f32 into batch (rows,block_points,width) f32, one workgroup per block, in float64 as both loops hold the batch: centroid =
 * per column ONE float64 sum down the rows (the chain of pasnl_window_noise) / float64(block_points), pc - centroid, m =
 * max(sqrt((x*x + y*y) + z*z)), pc / m.  rot NULL: rounded to float32, the feed into the placeholder (T:384).  rot (rows,2)
 * f64 = the host's cos and sin of each row's angle: [x y z] @ [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]] on the float64
 * block, rounded to float32 (T:301-302; within one float32 ulp of numpy's product, whose dgemm fixes no summation order).
 * Columns 3.. are copied. */
int pasnl_block_normalize(int rows, int block_points, int width, const float* src, const double* rot, float* batch,
                          pasnl_stream_t stream);

/* The score of one batch (T:311-321, T:391-402): pred = np.argmax(logits, 2) over ALL c classes (the FIRST maximum, numpy's
 * NaN rule); counters (2 + 4c) i64 += total_correct, total_seen, then per class seen, correct, iou_deno under smpw > 0 and
 * the label histogram of every entry (T:316): integers, exact and order-free.  loss[1] = the batch's classify loss as
 * tf.losses.sparse_softmax_cross_entropy(labels, logits, weights=smpw) gives it -- sum(w * ce) / count(w != 0), 0 when
 * that count is 0 (a float32 log-sum-exp per entry, float64 partial sums per workgroup added in workgroup order: no float
 * atomics; compared under a tolerance, never by bits) -- and loss[0] += loss[1].  workspace:
 * pasnl_block_score_workspace_bytes() device bytes.  c <= 256, else PASNL_EUNSUPPORTED.  Two launches. */
size_t pasnl_block_score_workspace_bytes(void);
int pasnl_block_score(int rows, int block_points, int c, const float* logits, const int* labels, const float* smpw, long long* counters,
                      double* loss, void* workspace, pasnl_stream_t stream);

/* The transform of the training input loop (T:253-254 of `train_one_epoch`, T:233-276), the other order: rotate_point_cloud_z
 * (P:71-89) first, then normalize_data (P:8-24), for rows blocks of src (rows,block_points,width) f32 into batch, one
 * workgroup per block, one launch.  The float32 row is widened to float64; x' = x * cos + y * (-sin), y' = x * sin + y * cos
 * with rot (rows,2) f64 = the host's cos and sin of each row's angle (required: NULL is PASNL_ENULL), the explicit sums of
 * pasnl_block_normalize (within one float32 ulp of numpy's product, whose dgemm fixes no summation order); z is carried --
 * x*0 + y*0 + z*1 is z for finite input up to the sign of a zero, and the centroid subtraction below removes that sign unless
 * the centroid is exactly zero.  The three coordinates are ROUNDED TO FLOAT32, as `rotated_data` is float32; on that float32
 * block normalize_data runs as in pasnl_block_normalize: the centroid's float64 chains / float64(block_points), pc - centroid,
 * m = max(sqrt((x*x + y*y) + z*z)), pc / m, rounded to float32.  The two orders do not give the same bits.  A block whose
 * rows are all one point has m == 0 and gets the reference's NaN (0 / 0).  Columns 3.. are copied.  The rounded block is held
 * in batch between the two stages, and every row of src is read before that row of batch is written: src == batch is
 * allowed; any other overlap is not. */
int pasnl_block_train_batch(int rows, int block_points, int width, const float* src, const double* rot, float* batch,
                            pasnl_stream_t stream);

/* The tallies of one training batch (T:264-272): pred = np.argmax(logits, 2) as in pasnl_block_score (the FIRST maximum,
 * numpy's NaN rule); counters (3) i64 += total_correct = np.sum(pred == label), total_seen = rows * block_points and
 * total_iou_deno = sum over l of np.sum((pred == l) | (label == l)) -- 1 for an entry whose prediction and label agree, 2
 * for one where they differ -- over EVERY entry, with no smpw > 0 and no label > 0: integers, exact and order-free.  Labels
 * are in [0, c) by the callers' checks; an entry outside that range is skipped (it counts nowhere, total_seen included), as
 * in pasnl_block_score.  loss[1] = the batch's classify loss and loss[0] += loss[1], defined and computed as there (the same
 * code: sum(w * ce) / count(w != 0), 0 when that count is 0; a tolerance, never bits).  workspace:
 * pasnl_block_score_workspace_bytes() device bytes.  c <= 256, else PASNL_EUNSUPPORTED.  Two launches. */
int pasnl_block_train_score(int rows, int block_points, int c, const float* logits, const int* labels, const float* smpw,
                            long long* counters, double* loss, void* workspace, pasnl_stream_t stream);

/* ---- SemanticKITTI's training-time validation loops on the device (SemanticKITTI/semantic_kitti_dataset.py (D) :68-109
 * `SemanticKittiDataset.__getitem__` and :164-211 `SemanticKittiDataset_whole.__getitem__`; SemanticKITTI/train_semantic_kitti.py
 * (T) :267-328 `eval_one_epoch` and :331-418 `eval_whole_scene_one_epoch`; utils/provider.py (P) :71-89
 * `rotate_point_cloud_z`).  One scan at a time: xyz (n,3) f32 never moves, labels (n) i32 in [0,c), remission (n) f32 is
 * optional; coordmin / coordmax (D:78-79, D:174-175) are the six device floats of pasnl_window_bounds, and a batch is scored
 * by pasnl_block_score.  Every comparison is the reference's own: the float32 coordinate widened to float64 against a float64
 * bound; no index is derived from a division.  The numpy RNG stream, the acceptance test of a try (D:97) and the carry-over of
 * rows between scans (T:354-379, over row counts only) stay on the host.  n <= 2^30; coordinates are finite. */

/* One try of the chopped-scan crop (D:82-97), counted in one pass over the scan.  The centre is read on the device:
 * curcenter = xyz[centre], curmin = float64(curcenter) - [half, half, .], curmax = float64(curcenter) + [half, half, .] with
 * half = the host's block_size / 2, curmin[2] = float64(coordmin_z), curmax[2] = float64(coordmax_z).  A point is a member
 * when it is >= curmin - 0.2 and <= curmax + 0.2 on all three axes (D:87).  hist: pasnl_window_hist_bytes(n, 2, 1) device
 * bytes -- per chunk of 64 consecutive points the member count and the count of members with label > 0 (wave ballots), each
 * scanned in place to the count in earlier chunks; the first row is the input of pasnl_kblock_fill.  -> out_stats (2) i32:
 * len(cur_semantic_seg) and np.sum(cur_semantic_seg > 0).  Two launches. */
int pasnl_kblock_crop_stats(long n, const float* xyz, const int* labels, const float* bounds, long centre, double half, int* hist,
                            int* out_stats, pasnl_stream_t stream);

/* The whole-scan columns (D:182-192), counted.  Column w = i * ny + j (i < nx, j < ny, the reference's loop order) has curmin
 * = float64(coordmin) + [i * block, j * block, 0] and curmax = float64(coordmin) + [(i + 1) * block, (j + 1) * block,
 * float64(float32(coordmax_z - coordmin_z))] -- the upper bound is NOT curmin + block; membership is the 0.2-margin test of
 * pasnl_kblock_crop_stats.  hist: pasnl_kwindow_hist_bytes(n, nx, ny) device bytes, laid out as there -- cleared, then per
 * column and chunk the member count (a wave stores only for the columns inside the rectangle of its points' ranges; both
 * bounds are monotone in i, so an axis's columns for a point are one range), then scanned in place per column.  ->
 * out_counts (nx*ny) i32, empty columns included.  No limit per axis: nx * ny <= INT_MAX, else PASNL_EUNSUPPORTED.  Cost:
 * every point tests every column of both axes, nx + ny float64 comparisons per point here and again in pasnl_kblock_fill --
 * nothing at the 10 to 100 columns per axis of a lidar scan, linear in them beyond.  A clear and two launches. */
int pasnl_kblock_grid_count(long n, const float* xyz, const float* bounds, int nx, int ny, double block, int* hist, int* out_counts,
                            pasnl_stream_t stream);

/* The member lists (D:87-95, D:186-193): column w's members, in ascending scan index, go to out_idx[woff[w] ...] (woff
 * (nx*ny) i32, -1: skip the column) and out_mask[...] is the same test with `padding` in place of 0.2 (D:95, D:193).  centre
 * >= 0: the chopped column round that point (nx = ny = 1, hist from pasnl_kblock_crop_stats of the same centre and half);
 * centre < 0: the grid (hist from pasnl_kblock_grid_count of the same nx, ny and block).  A member's rank is its chunk's
 * scanned count plus the members among the lower lanes of its wave: deterministic, no atomics and no arrival order.  cap: the
 * length of out_idx / out_mask (nothing is written at or past it). */
int pasnl_kblock_fill(long n, const float* xyz, const float* bounds, long centre, double half, int nx, int ny, double block, double padding,
                      const int* hist, const int* woff, long cap, int* out_idx, unsigned char* out_mask, pasnl_stream_t stream);

/* Rows (D:100-107, D:195-203): rowpos (rows,block_points) i32 holds, per row entry, woff[w] + the host's rng.choice(count_w,
 * block_points) draw and rowbase (rows) i32 the row's woff[w], so the draw itself is rowpos[e] - rowbase[row].  Entry e gets
 * i = cat_idx[rowpos[e]], seg = labels[i], out_data[e] = xyz[i] followed by one remission when nfeat == 1 (nfeat is 0 or 1),
 * out_label[e] = seg.  lut (c) f32, c <= 256 else PASNL_EUNSUPPORTED.  quirks != 0 reproduces the reference: out_smpw[e] =
 * float32(lut[labels[seg]]) * float32(mask) -- label_weights = lut[label] is a per-point array that D:104 indexes by label
 * value, so the caller guarantees n > max(label) -- and the remission is remission[rowpos[e] - rowbase[row]], that of scan
 * point number `draw` (D:107 indexes the scan's remissions by the raw draw).  quirks == 0 is the evident intent: out_smpw[e]
 * = lut[seg] * mask and remission[i]. */
int pasnl_kblock_gather(int rows, int block_points, const int* rowpos, const int* rowbase, long cap, const int* cat_idx,
                        const unsigned char* cat_mask, long n, const float* xyz, const float* remission, int nfeat, const int* labels,
                        int c, const float* lut, int quirks, float* out_data, int* out_label, float* out_smpw, pasnl_stream_t stream);

/* rotate_point_cloud_z (P:71-89) as T:290 applies it to the float64 batch, for rows blocks of src (rows,block_points,width)
 * f32 into batch: [x y] -> [x * cos - y * sin, x * sin + y * cos] in float64 from the float32 row, rounded to float32 (within
 * one float32 ulp of numpy's product, whose dgemm fixes no summation order); columns 2.. are copied.  rot (rows,2) f64 = the
 * host's cos and sin of each row's angle.  src == batch is allowed.  There is no normalize_data in these loops. */
int pasnl_kblock_rotate(int rows, int block_points, int width, const float* src, const double* rot, float* batch, pasnl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PASNL_H_ */
