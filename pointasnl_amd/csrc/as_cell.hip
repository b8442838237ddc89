// The AdaptiveSampling cell's forward for gfx950 (reference utils/pointasnl_util.py:112-173, SampleWeights and
// AdaptiveSampling; restated in oracle/cells.py): the gather of a group's first `as` neighbours, the micro attention over them
// (on projected rows, or with the projections fused in), the re-weighting tail, and the whole cell after the gather in one
// kernel (narrow and wide layers).  The fused backward is as_grad.hip; what the two share is as_core.hpp.  DESIGN.md 4.4.
//
// fp32 in, fp32 out, tolerance 1e-5 against the fp32 oracle; the products run on v_mfma_f32_16x16x4_f32 (exact fp32 fmaf chains).
#include <math.h>
#include "as_core.hpp"

namespace pasnl {

// =============================================================================================
// Adaptive-Sampling micro attention: one wave per group, as <= 16 neighbours padded to a 16x16 tile,
// v_mfma_f32_16x16x4_f32, operands straight from global memory (a group is a few KB, L2/L1 resident).
//   S^T[key][query]:  D[row = 4*(l>>4)+r][col = l&15],   A = K[key = l&15][4t + (l>>4)],
//                                                        B = Q[query = l&15][4t + (l>>4)]
//   softmax over keys = 4 in-lane values + exchanges with lanes l^16, l^32
//   O^T[ch][query] += V^T . P^T with step t contracting key 4*(l>>4)+t
// =============================================================================================
__global__ __launch_bounds__(256) void as_attention_kernel(long groups, int as, int cb, float qscale, int qs, int kvs,
                                                          const float* __restrict__ q, const float* __restrict__ kv,
                                                          float* __restrict__ out) {
  // qs / kvs = row strides of q and kv in floats (cb and 2cb for separate tensors; 3cb for one [K|V|Q] tensor)
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;
  const int col = lane & 15, grp = lane >> 4;
  const float* qg = q + (size_t)g * as * qs;
  const float* kg = kv + (size_t)g * as * kvs;
  const bool rowok = col < as;  // this lane's key row (as A operand) / query (as B operand) exists
  f32x4 S = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < cb; c0 += 4) {
    int c = c0 + grp;
    bool okc = rowok && c < cb;
    float a = okc ? kg[(size_t)col * kvs + c] : 0.f;
    float b = okc ? qg[(size_t)col * qs + c] * qscale : 0.f;
    S = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, S, 0, 0, 0);
  }
  const float inv = as_softmax_keys(S, as, grp);
  const float* vg = kg + cb;  // V = second half of each kv row
  for (int c0 = 0; c0 < cb; c0 += 16) {
    f32x4 O = {0.f, 0.f, 0.f, 0.f};
    int ch = c0 + col;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int key = 4 * grp + t;
      float a = (key < as && ch < cb) ? vg[(size_t)key * kvs + ch] : 0.f;
      O = __builtin_amdgcn_mfma_f32_16x16x4f32(a, S[t], O, 0, 0, 0);
    }
    // O^T[ch = c0 + 4*grp + r][query = col]
    if (rowok) {
      float* op = out + ((size_t)g * as + col) * cb + c0 + 4 * grp;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (c0 + 4 * grp + r < cb) op[r] = O[r] * inv;
    }
  }
}

// =============================================================================================
// AdaptiveSampling tail: softmax over the neighbour axis, then the weighted sums.
// One thread per (group, column) of the (1+ch)-wide logits; column 0 re-weights xyz.
// =============================================================================================
__global__ __launch_bounds__(256) void as_reweight_kernel(long groups, int as, int nsample, int ch, int xs, int fs,
                                                         const float* __restrict__ logits,
                                                         const float* __restrict__ gxyz, const float* __restrict__ gfeat,
                                                         float* __restrict__ new_xyz, float* __restrict__ new_feature) {
  // xs / fs = row strides of the grouped coordinates / features in floats (3 and ch for separate tensors)
  const int w = 1 + ch;
  const long total = groups * w;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    long g = e / w;
    int c = (int)(e - g * w);
    float v[AS_MAX];
#pragma unroll
    for (int k = 0; k < AS_MAX; ++k) v[k] = k < as ? logits[((size_t)g * as + k) * w + c] : -INFINITY;
    const float sum = as_softmax_column(as, v);
    if (c == 0) {
      float ax = 0.f, ay = 0.f, az = 0.f;
      const float* xp = gxyz + (size_t)g * nsample * xs;
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k)
        if (k < as) {
          float wk = v[k] / sum;
          ax += xp[k * xs] * wk; ay += xp[k * xs + 1] * wk; az += xp[k * xs + 2] * wk;
        }
      new_xyz[g * 3] = ax; new_xyz[g * 3 + 1] = ay; new_xyz[g * 3 + 2] = az;
    } else {
      float a = 0.f;
      const float* fp = gfeat + (size_t)g * nsample * fs + (c - 1);
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k)
        if (k < as) a += fp[(size_t)k * fs] * (v[k] / sum);
      new_feature[(size_t)g * ch + (c - 1)] = a;
    }
  }
}

// =============================================================================================
// AdaptiveSampling input (pointasnl_util.py:121-124,165-166): for every group the first `as` neighbours as rows
//     [xyz[i_s] - xyz[i_0] | xyz[i_s] | feature[i_s]]   (as x (6+C)),   i_s = idx[b,j,s]
// = concat(normalized_xyz, shift_group_points) of the reference, gathered straight from the tables (one launch
// instead of two gathers, a slice, a subtraction and two concats).  Columns 3.. are also the (xyz | feature) rows
// the re-weighting tail needs, so nothing else of the grouped tensors is ever materialised.
// =============================================================================================
// thread per element: narrow rows (the xyz-only layers, 6 + c = 9 columns)
__global__ __launch_bounds__(256) void as_gather_elem_kernel(int n, int c, int m, int k, int as, long total,
                                                            const float* __restrict__ xyz, const float* __restrict__ feature,
                                                            const int* __restrict__ idx, float* __restrict__ out) {
  const int w = 6 + c;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / w;  // (b, j, s)
    const int col = (int)(e - row * w);
    const long gj = row / as;  // (b, j)
    const int sidx = (int)(row - gj * as);
    const long bi = gj / m;
    const int i = idx[gj * k + sidx];
    float v;
    if (col < 3) {
      const int i0 = idx[gj * k];
      v = xyz[((size_t)bi * n + i) * 3 + col] - xyz[((size_t)bi * n + i0) * 3 + col];
    } else if (col < 6) {
      v = xyz[((size_t)bi * n + i) * 3 + (col - 3)];
    } else {
      v = feature[((size_t)bi * n + i) * c + (col - 6)];
    }
    out[e] = v;
  }
}

// One wave per output row (b, j, s): the row's (cloud, neighbour index, first-neighbour index) are wave-uniform, the
// lanes run over its 6 + c columns (the thread-per-element version spent ~150 instructions per float on three 64-bit
// divisions: 44 us for 52 MB at cls layer2).
__global__ __launch_bounds__(256) void as_gather_kernel(int n, int c, int m, int k, int as, long rows,
                                                       const float* __restrict__ xyz, const float* __restrict__ feature,
                                                       const int* __restrict__ idx, float* __restrict__ out) {
  const int w = 6 + c;
  const int lane = threadIdx.x & 63;
  const long nwaves = (long)gridDim.x * 4;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
    const long gj = row / as;  // (b, j)
    const int sidx = (int)(row - gj * as);
    const long bi = gj / m;
    const int i = idx[gj * k + sidx], i0 = idx[gj * k];
    const float* ps = xyz + ((size_t)bi * n + i) * 3;
    const float* p0 = xyz + ((size_t)bi * n + i0) * 3;
    const float* fs = feature + ((size_t)bi * n + i) * c;
    float* o = out + (size_t)row * w;
    if (lane < 6) o[lane] = lane < 3 ? ps[lane] - p0[lane] : ps[lane - 3];
    for (int col = lane; col < c; col += 64) o[6 + col] = fs[col];
  }
}
// ---------------------------------------------------------------------------------------------
// AdaptiveSampling micro attention with the K / V / Q projections computed on the fly (narrow inputs: w <= 15, the
// xyz-only first layers, w = 9).  The projection output would be (groups*as, 3cb) floats -- 151 MB at cls layer1,
// written by a GEMM that is pure HBM traffic at K = 9 and read once by the attention.  Here AsProj (as_core.hpp) forms V and
// the score tile of a group from its rows in registers, and
//     O^T = V[t] (A) x P[t] (B)
//   one wave per group, persistent over groups
// ---------------------------------------------------------------------------------------------
constexpr int AS_PROJ_MAXW = 15;
template <int KS, int CBLK>  // k-steps of 4 inputs (w + 1 <= 4 KS), 16-channel blocks (cb = 16 CBLK)
__global__ __launch_bounds__(256) void as_attention_proj_kernel(long groups, int as, int w, float qscale,
                                                               const float* __restrict__ x, const float* __restrict__ wkvq,
                                                               const float* __restrict__ bkvq, float* __restrict__ out) {
  constexpr int CB = 16 * CBLK;
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, grp = lane >> 4;
  AsProj<KS, CBLK> proj;
  proj.load_weights(wkvq, bkvq, w, qscale, col, grp);
  const long nwaves = (long)gridDim.x * 4;
  for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g < groups; g += nwaves) {
    float xv[KS];
    const float* xp = x + ((size_t)g * as + min(col, as - 1)) * w;
    proj.load_x(xp, as, w, col, grp, xv);
    f32x4 V[CBLK], S;
    proj.project(xv, V, S);
    const float inv = as_softmax_keys(S, as, grp);
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
      f32x4 O = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) O = __builtin_amdgcn_mfma_f32_16x16x4f32(V[cb][t], S[t], O, 0, 0, 0);
      if (col < as)  // O^T[ch = cb*16 + 4*grp + r][query = col]
        *reinterpret_cast<float4*>(out + ((size_t)g * as + col) * CB + cb * 16 + 4 * grp) =
            make_float4(O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The whole AdaptiveSampling cell of a narrow layer (w = 6 + c <= 15 inputs, 1 + ch <= 16 weights per neighbour) in ONE
// kernel after the gather (pointasnl_util.py:112-173): projections + micro attention as in as_attention_proj_kernel, then
//     hid^T    = relu(Wa'^T . att^T + ba)   (cb -> 32; the attention output O^T is already the B operand, the bias
//                                            is the accumulator's initial value)
//     logit^T  = Wb'^T . hid^T + bb         (32 -> 1 + ch)   -> lane (neighbour s = col, grp) holds outputs o = 4*grp + r
//     softmax over the neighbours = over the 16 lanes of a DPP row; weighted sums of the gathered rows the same way.
// Nothing but the gathered rows is read and only new_xyz (g,3) / new_feature (g,ch) are written: the (groups*as, cb),
// (.., 32) and (.., 1+ch) intermediates of the op-by-op chain (50 + 50 + 11 MB at cls layer1) never exist.
// ---------------------------------------------------------------------------------------------
template <int KS, int CBLK>
__global__ __launch_bounds__(256) void as_cell_narrow_kernel(long groups, int as, int w, int ch, float qscale,
                                                            const float* __restrict__ x, const float* __restrict__ wkvq,
                                                            const float* __restrict__ bkvq, const float* __restrict__ wa,
                                                            const float* __restrict__ ba, const float* __restrict__ wb,
                                                            const float* __restrict__ bb, float* __restrict__ new_xyz,
                                                            float* __restrict__ new_feature) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, grp = lane >> 4;
  const int nout = 1 + ch;
  AsProj<KS, CBLK> proj;
  proj.load_weights(wkvq, bkvq, w, qscale, col, grp);
  // mlp2_0: A[m = h][k-slot grp] of step (cb, r) = Wa[cb*16 + 4*grp + r][hb*16 + col]; its bias as accumulator start
  float wa_r[CBLK][4][2];
  f32x4 ba_r[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ba_r[hb][r] = ba[hb * 16 + 4 * grp + r];
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) wa_r[cb][r][hb] = wa[(size_t)(cb * 16 + 4 * grp + r) * 32 + hb * 16 + col];
  }
  // mlp2_1: A[m = o][k-slot grp] of step (hb, r) = Wb[hb*16 + 4*grp + r][o = col]
  float wb_r[2][4];
  f32x4 bb_r;
#pragma unroll
  for (int r = 0; r < 4; ++r) bb_r[r] = 4 * grp + r < nout ? bb[4 * grp + r] : 0.f;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 4; ++r) wb_r[hb][r] = col < nout ? wb[(size_t)(hb * 16 + 4 * grp + r) * nout + col] : 0.f;

  const long nwaves = (long)gridDim.x * 4;
  for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g < groups; g += nwaves) {
    float xv[KS];
    const float* xp = x + ((size_t)g * as + min(col, as - 1)) * w;
    proj.load_x(xp, as, w, col, grp, xv);
    // the columns this lane re-weights: output o = 4*grp + r multiplies x column 3 + (o - 1) (o >= 1), output 0 the xyz
    float xo[4], xc[3];
#pragma unroll
    for (int r = 0; r < 4; ++r) xo[r] = xp[min(max(2 + 4 * grp + r, 3), w - 1)];
#pragma unroll
    for (int d = 0; d < 3; ++d) xc[d] = xp[3 + d];

    f32x4 V[CBLK], S;
    proj.project(xv, V, S);
    const float inv = as_softmax_keys(S, as, grp);
    // att^T blocks (O^T / l) feed mlp2_0 directly
    f32x4 H[2] = {ba_r[0], ba_r[1]};
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
      f32x4 O = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) O = __builtin_amdgcn_mfma_f32_16x16x4f32(V[cb][t], S[t], O, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = O[r] * inv;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) H[hb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa_r[cb][r][hb], a, H[hb], 0, 0, 0);
      }
    }
    f32x4 L = bb_r;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 4; ++r) L = __builtin_amdgcn_mfma_f32_16x16x4f32(wb_r[hb][r], fmaxf(H[hb][r], 0.f), L, 0, 0, 0);
    // L[r] = logit of neighbour `col` for output o = 4*grp + r; softmax over the neighbours = over the row's lanes
    float wgt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = col < as ? L[r] : -INFINITY;
      const float mx = row16_max(v);
      const float e = col < as ? fast_exp2((v - mx) * LOG2E) : 0.f;
      wgt[r] = e / row16_sum(e);
    }
    // weighted sums over the neighbours; lane col == 0 of every row writes its outputs
    float sx[3], sf[4];
#pragma unroll
    for (int d = 0; d < 3; ++d) sx[d] = row16_sum(col < as ? wgt[0] * xc[d] : 0.f);  // (only grp 0 holds output 0)
#pragma unroll
    for (int r = 0; r < 4; ++r) sf[r] = row16_sum(col < as ? wgt[r] * xo[r] : 0.f);
    if (col == 0) {
      if (grp == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) new_xyz[g * 3 + d] = sx[d];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 4 * grp + r;
        if (o >= 1 && o < nout) new_feature[(size_t)g * ch + (o - 1)] = sf[r];
      }
    }
  }
}
// ---------------------------------------------------------------------------------------------
// The AdaptiveSampling cell of a WIDE layer after its projection GEMM (w = 6 + c > 15: K = w is a GEMM worth running):
// kvq (g, as, 3cb) = [K | V | Q] rows -> attention -> mlp2 -> softmax over the neighbours -> re-weighted sums, as in
// as_cell_narrow_kernel, with the projected operands read from memory in the layouts that kernel computes them in
// (K^T / Q^T: 4 consecutive channels of the lane's row; V: coalesced row reads).  Wa, Wb (32 x (1+ch)) and the second bias
// sit in LDS.  Differences from the narrow cell, all about what a wave waits for:
//   * every load is unconditional and masked by a product (a select in front of a load makes the compiler predicate the
//     load: branch + load + full wait per matrix step -- DESIGN.md 6 "loads behind a select");
//   * the logits are formed TRANSPOSED (a lane owns an output and four neighbours): the softmax over the neighbours is
//     in-lane work plus two exchanges between the 16-lane rows per reduction, one division per output, and the 16 outputs of
//     a block leave as one 64-byte store;
//   * the features a block re-weights are requested one block ahead; 3 waves per SIMD (__launch_bounds__(256, 3)).
// ---------------------------------------------------------------------------------------------
template <int CBLK>  // 16 (CBLK - 1) < cb <= 16 CBLK (the reference's bottleneck widths are (3 + c) / 2: 33, 65, ...): only
                     // the LAST block of 16 channels needs clamped addresses and masks, the others load at constant offsets
__global__ __launch_bounds__(256, 3) void as_cell_wide_kernel(long groups, int as, int cb, int w, int ch, float qscale,
                                                          const float* __restrict__ kvq, int ld, const float* __restrict__ x,
                                                          const float* __restrict__ wa, const float* __restrict__ ba,
                                                          const float* __restrict__ wb, const float* __restrict__ bb,
                                                          float* __restrict__ new_xyz, float* __restrict__ new_feature) {
  const int cb3 = ld;  // row stride of kvq: 3 cb, or more when the projection GEMM was given a rounder width
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Wbs = reinterpret_cast<float*>(smem);  // [32][nout]
  const int nout = 1 + ch;
  float* Bbs = Wbs + 32 * nout;                 // [nout] (+ 16 zeros: the last block of outputs reads past nout)
  float* Was = Bbs + nout + 16;                 // [16 CBLK][WAS_LD]: Wa, rows past cb zero (the padded channels contribute
  constexpr int WAS_LD = 36;                    //  nothing); stride 36: the four 16-lane rows of a read hit all 32 banks
  for (int i = threadIdx.x; i < 32 * nout; i += 256) Wbs[i] = wb[i];
  for (int i = threadIdx.x; i < nout + 16; i += 256) Bbs[i] = i < nout ? bb[i] : 0.f;
  for (int i = threadIdx.x; i < 16 * CBLK * 32; i += 256) Was[(i >> 5) * WAS_LD + (i & 31)] = (i >> 5) < cb ? wa[i] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, grp = lane >> 4;
  f32x4 ba_r[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 4; ++r) ba_r[hb][r] = ba[hb * 16 + 4 * grp + r];
  const int noblk = (nout + 15) >> 4;
  const long nwaves = (long)gridDim.x * 4;
  for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g < groups; g += nwaves) {
    const float* kq = kvq + ((size_t)g * as + min(col, as - 1)) * cb3;  // this lane's [K | V | Q] row
    const float* vb = kvq + (size_t)g * as * cb3 + cb;                  // V rows of the group
    f32x4 S = {0.f, 0.f, 0.f, 0.f};
    const float mrow = col < as ? 1.f : 0.f;
#pragma unroll
    for (int cbk = 0; cbk < CBLK; ++cbk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = cbk * 16 + 4 * grp + r;
        // unconditional loads (the last block's on clamped addresses), masked by a PRODUCT: behind `ok ? value : 0` the
        // compiler makes the load itself conditional -- a branch, the load and a full wait in front of every matrix step
        const bool last = cbk == CBLK - 1;
        const int cc = last ? min(c, cb - 1) : c;
        const float kk = kq[cc], qq = kq[2 * cb + cc];
        const float m = last ? (col < as && c < cb ? 1.f : 0.f) : mrow;
        S = __builtin_amdgcn_mfma_f32_16x16x4f32(kk * m, qq * (qscale * m), S, 0, 0, 0);
      }
    const float inv = as_softmax_keys(S, as, grp);
    // The re-weighting at the end works on TRANSPOSED logits: lane (col, grp) owns output ob*16 + col and the neighbours
    // 4 grp + r.  What it multiplies: column 2 + o of its four neighbours' rows (coalesced over col), and for output 0 their
    // coordinates.  The first block's values are requested here, a matrix chain ahead of their use (and after the K / Q
    // registers have been released) -- not one by one in front of each use.
    const float* xg = x + (size_t)g * as * w;
    int xrow[4];
    float x3[4][3], xo[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      xrow[r] = min(4 * grp + r, as - 1) * w;
#pragma unroll
      for (int d = 0; d < 3; ++d) x3[r][d] = xg[xrow[r] + min(3 + d, w - 1)];
      xo[r] = xg[xrow[r] + min(2 + col, w - 1)];
    }
    f32x4 H[2] = {ba_r[0], ba_r[1]};
    int vrow[4];
    float vmask[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      vrow[t] = min(4 * grp + t, as - 1) * cb3;
      vmask[t] = 4 * grp + t < as ? 1.f : 0.f;
    }
#pragma unroll
    for (int cbk = 0; cbk < CBLK; ++cbk) {
      f32x4 O = {0.f, 0.f, 0.f, 0.f};
      const int vc = cbk * 16 + col;  // V[key][vc]: lanes over channels
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int key = 4 * grp + t;
        const bool last = cbk == CBLK - 1;
        const float v = vb[vrow[t] + (last ? min(vc, cb - 1) : vc)];
        O = __builtin_amdgcn_mfma_f32_16x16x4f32(v * (last ? (key < as && vc < cb ? 1.f : 0.f) : vmask[t]), S[t], O, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = O[r] * inv;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
          H[hb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Was[(cbk * 16 + 4 * grp + r) * WAS_LD + hb * 16 + col], a, H[hb], 0, 0, 0);
      }
    }
    float hr[2][4];
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 4; ++r) hr[hb][r] = fmaxf(H[hb][r], 0.f);
    // (a use the compiler cannot move: without it the coordinate loads are sunk into the one branch that reads them)
#pragma unroll
    for (int r = 0; r < 4; ++r) asm volatile("" ::"v"(x3[r][0]), "v"(x3[r][1]), "v"(x3[r][2]));
    for (int ob = 0; ob < noblk; ++ob) {
      float xn[4];  // the next block's column, in flight under this block's matrix steps and softmax
#pragma unroll
      for (int r = 0; r < 4; ++r) xn[r] = xg[xrow[r] + min(2 + (ob + 1) * 16 + col, w - 1)];
      // logits, transposed: L[r] = logit of output ob*16 + col for neighbour 4 grp + r (the operands of the reference-order
      // product, swapped).  The softmax over the neighbours is then three in-lane steps and two exchanges between the four
      // 16-lane rows per reduction, ONE division per output -- not a 16-lane DPP reduction per (output, reduction)
      f32x4 L;
      const float b0 = Bbs[ob * 16 + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) L[r] = b0;
      const int oc = min(ob * 16 + col, nout - 1);
      const float mo = ob * 16 + col < nout ? 1.f : 0.f;
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          L = __builtin_amdgcn_mfma_f32_16x16x4f32(hr[hb][r], Wbs[(hb * 16 + 4 * grp + r) * nout + oc] * mo, L, 0, 0, 0);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        L[r] = 4 * grp + r < as ? L[r] : -INFINITY;
        mx = fmaxf(mx, L[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));  // finite: neighbour 0 is always valid
      float den = 0.f, num = 0.f, n3[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = fast_exp2((L[r] - mx) * LOG2E);  // 0 for the padding neighbours; their (clamped) rows are finite
        den += e;
        num += e * xo[r];
        if (ob == 0) {
#pragma unroll
          for (int d = 0; d < 3; ++d) n3[d] += e * x3[r][d];
        }
      }
      den += __shfl_xor(den, 16);
      num += __shfl_xor(num, 16);
      den += __shfl_xor(den, 32);
      num += __shfl_xor(num, 32);
      const int o = ob * 16 + col;
      if (ob == 0) {  // (uniform) output 0 re-weights the coordinates
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          n3[d] += __shfl_xor(n3[d], 16);
          n3[d] += __shfl_xor(n3[d], 32);
        }
        if (lane == 0) {
#pragma unroll
          for (int d = 0; d < 3; ++d) new_xyz[g * 3 + d] = n3[d] / den;
        }
      }
      if (grp == 0 && o >= 1 && o < nout) new_feature[(size_t)g * ch + (o - 1)] = num / den;  // 16 consecutive floats
#pragma unroll
      for (int r = 0; r < 4; ++r) xo[r] = xn[r];
    }
  }
}

// one wave per group, four to a workgroup, at most `cap` workgroups (the kernels that stride over the groups)
static dim3 as_persistent_grid(int g, long cap) {
  const long wgs = ((long)g + 3) / 4;
  return dim3((unsigned)(wgs < cap ? wgs : cap));
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_as_cell_wide_ld(int g, int as, int cb, int w, int ch, const float* kvq, int ld, const float* x,
                                     const float* wa, const float* ba, const float* wb, const float* bb, float* new_xyz,
                                     float* new_feature, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0 && w > 0 && ch > 0 && ld >= 3 * cb, PASNL_EINVAL);
  PASNL_REQUIRE(as <= 16 && cb <= 144 && w == 3 + ch, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(kvq && x && wa && ba && wb && bb && new_xyz && new_feature, PASNL_ENULL);
  const size_t lds = ((size_t)33 * (1 + ch) + 16 + (size_t)((cb + 15) / 16 > 9 ? 9 : (cb + 15) / 16) * 16 * 36) * sizeof(float);
  PASNL_REQUIRE(lds <= 64 * 1024, PASNL_EUNSUPPORTED);
  // persistent workgroups: a wave's weights (registers) and the workgroup's Wb (LDS) are loaded once
  const dim3 grid = as_persistent_grid(g, 768), block(256);
  hipStream_t st = pasnl_hip_stream(stream);
  static const decltype(&as_cell_wide_kernel<1>) kernels[] = {as_cell_wide_kernel<1>, as_cell_wide_kernel<2>, as_cell_wide_kernel<3>,
                                                               as_cell_wide_kernel<4>, as_cell_wide_kernel<5>, as_cell_wide_kernel<6>,
                                                               as_cell_wide_kernel<7>, as_cell_wide_kernel<8>, as_cell_wide_kernel<9>};
  const int cblk = (cb + 15) / 16;  // exact: the kernel treats every block of 16 channels but the last as full
  if (launch(kernels[(cblk < 9 ? cblk : 9) - 1], grid, block, lds, st, (long)g, as, cb, w, ch, as_qscale(cb), kvq, ld, x, wa, ba, wb,
             bb, new_xyz, new_feature) != PASNL_OK)
    return PASNL_ELAUNCH;
  return pasnl_launch_status();
}

extern "C" int pasnl_as_cell_wide(int g, int as, int cb, int w, int ch, const float* kvq, const float* x, const float* wa,
                                  const float* ba, const float* wb, const float* bb, float* new_xyz, float* new_feature,
                                  pasnl_stream_t stream) {
  return pasnl_as_cell_wide_ld(g, as, cb, w, ch, kvq, 3 * cb, x, wa, ba, wb, bb, new_xyz, new_feature, stream);
}

extern "C" int pasnl_as_cell_narrow(int g, int as, int cb, int w, int ch, const float* x, const float* wkvq, const float* bkvq,
                                    const float* wa, const float* ba, const float* wb, const float* bb, float* new_xyz,
                                    float* new_feature, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0 && w > 0 && ch > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= 16 && w <= pasnl::AS_PROJ_MAXW && (cb == 32 || cb == 64) && 1 + ch <= 16 && w == 3 + ch,
                PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(x && wkvq && bkvq && wa && ba && wb && bb && new_xyz && new_feature, PASNL_ENULL);
  return with_as_proj(w, cb, [&](auto ks, auto cblk) {
    hipLaunchKernelGGL((as_cell_narrow_kernel<ks(), cblk()>), as_persistent_grid(g, 2048), dim3(256), 0, pasnl_hip_stream(stream),
                       (long)g, as, w, ch, as_qscale(cb), x, wkvq, bkvq, wa, ba, wb, bb, new_xyz, new_feature);
    return pasnl_launch_status();
  });
}

extern "C" int pasnl_as_attention_proj(int g, int as, int cb, int w, const float* x, const float* wkvq, const float* bkvq,
                                       float* out, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0 && w > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= 16 && w <= pasnl::AS_PROJ_MAXW && (cb == 32 || cb == 64), PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(x && wkvq && bkvq && out, PASNL_ENULL);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, PASNL_EINVAL);
  return with_as_proj(w, cb, [&](auto ks, auto cblk) {  // persistent: a lane's weights are loaded once
    hipLaunchKernelGGL((as_attention_proj_kernel<ks(), cblk()>), as_persistent_grid(g, 2048), dim3(256), 0, pasnl_hip_stream(stream),
                       (long)g, as, w, as_qscale(cb), x, wkvq, bkvq, out);
    return pasnl_launch_status();
  });
}

extern "C" int pasnl_as_attention(int g, int as, int cb, const float* q, const float* kv, float* out,
                                  pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= 16 && cb <= 256, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(q && kv && out, PASNL_ENULL);
  hipLaunchKernelGGL(as_attention_kernel, dim3((unsigned)(((long)g + 3) / 4)), dim3(256), 0, pasnl_hip_stream(stream), (long)g,
                     as, cb, as_qscale(cb), cb, 2 * cb, q, kv, out);
  return pasnl_launch_status();
}

extern "C" int pasnl_as_attention_qkv(int g, int as, int cb, const float* kvq, float* out, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= 16 && cb <= 256, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(kvq && out, PASNL_ENULL);
  hipLaunchKernelGGL(as_attention_kernel, dim3((unsigned)(((long)g + 3) / 4)), dim3(256), 0, pasnl_hip_stream(stream), (long)g,
                     as, cb, as_qscale(cb), 3 * cb, 3 * cb, kvq + 2 * cb, kvq, out);
  return pasnl_launch_status();
}

extern "C" int pasnl_as_gather(int b, int n, int c, int m, int k, int as, const float* xyz, const float* feature, const int* idx,
                               float* out, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && c > 0 && m >= 0 && k > 0 && as > 0 && as <= k, PASNL_EINVAL);
  long rows = (long)b * m * as;
  if (rows == 0) return PASNL_OK;
  PASNL_REQUIRE(xyz && feature && idx && out, PASNL_ENULL);
  if (c < 26) {  // fewer than 32 columns: a wave per row would idle most of its lanes (74 vs 18 us at cls layer1)
    hipLaunchKernelGGL(as_gather_elem_kernel, dim3(as_grid(rows * (6 + c))), dim3(256), 0, pasnl_hip_stream(stream), n, c, m, k, as,
                       rows * (6 + c), xyz, feature, idx, out);
    return pasnl_launch_status();
  }
  // (a wave per row)
  hipLaunchKernelGGL(as_gather_kernel, dim3(as_grid(rows * 64)), dim3(256), 0, pasnl_hip_stream(stream), n, c, m, k, as, rows, xyz,
                     feature, idx, out);
  return pasnl_launch_status();
}

extern "C" int pasnl_as_reweight(int g, int as, int nsample, int ch, const float* logits, const float* grouped_xyz,
                                 const float* grouped_feature, float* new_xyz, float* new_feature, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && nsample >= as && ch > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && grouped_xyz && grouped_feature && new_xyz && new_feature, PASNL_ENULL);
  hipLaunchKernelGGL(as_reweight_kernel, dim3(as_grid((long)g * (1 + ch))), dim3(256), 0, pasnl_hip_stream(stream), (long)g, as,
                     nsample, ch, 3, ch, logits, grouped_xyz, grouped_feature, new_xyz, new_feature);
  return pasnl_launch_status();
}

extern "C" int pasnl_as_reweight_x(int g, int as, int ch, const float* logits, const float* x, float* new_xyz,
                                   float* new_feature, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && ch > 3, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && x && new_xyz && new_feature, PASNL_ENULL);
  // x rows = [xyz - xyz0 | xyz | feature] (3 + ch floats): coordinates and the (xyz | feature) rows both start at column 3
  const int w = 3 + ch;
  hipLaunchKernelGGL(as_reweight_kernel, dim3(as_grid((long)g * (1 + ch))), dim3(256), 0, pasnl_hip_stream(stream), (long)g, as, as,
                     ch, w, w, logits, x + 3, x + 3, new_xyz, new_feature);
  return pasnl_launch_status();
}
