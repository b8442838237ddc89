// What the forward (as_cell.hip) and the fused backward (as_grad.hip) of the AdaptiveSampling cell share: one definition each, so
// that the P and the re-weighting weights the backward recomputes are the forward's by construction.
//
// A group is as <= AS_MAX neighbours padded to one 16 x 16 tile of v_mfma_f32_16x16x4_f32, one wave per group: lane l holds
// column col = l & 15 and rows 4 grp + r (grp = l >> 4, r = 0..3) of a D tile.  Scores live in the log2 domain (as_qscale is
// folded into Q).  The build is -ffp-contract=off; nothing here reorders a sum.
#pragma once
#include <math.h>
#include "common.hpp"

namespace pasnl {

constexpr int AS_MAX = 16;  // neighbours per group (the 16 x 16 tile)

// Softmax over the KEYS of a key-major score tile S^T[key = 4 grp + r][query = col]: keys past `as` are masked, the maximum and
// the sum are 4 in-lane values and exchanges with lanes l ^ 16, l ^ 32.  Leaves the unnormalised exp2 values in S (0 for a
// masked key) and returns 1 / their sum (finite: key 0 exists).
__device__ __forceinline__ float as_softmax_keys(f32x4& S, int as, int grp) {
  float tmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    S[r] = (4 * grp + r) < as ? S[r] : -INFINITY;
    tmax = fmaxf(tmax, S[r]);
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    S[r] = fast_exp2(S[r] - tmax);
    psum += S[r];
  }
  psum += __shfl_xor(psum, 16);
  psum += __shfl_xor(psum, 32);
  return 1.0f / psum;
}

// The K / V / Q projections of a narrow layer computed on the fly (w <= 15 inputs): X' = [x | 1 | 0..] (the constant column
// carries the biases), W' = the BN-folded weights with the bias as row w, qscale folded into Wq'.  Everything is a chain of
// 16x16x4 MFMAs whose D layouts are already the next product's operand layouts (lane = (col, grp)):
//     K^T = Wk'^T . X'^T  and  Q^T = Wq'^T . X'^T   -> lane (row = col, grp) holds channels 4*grp + r of a 16-block
//     V   = X' . Wv'                                -> lane (channel = col, grp) holds keys 4*grp + r
//     S   = sum over (block, r) of K^T[r] (A) x Q^T[r] (B): the pairing of channels inside a step is free as long
//           as K and Q agree on it               -> lane (query = col, grp) holds keys 4*grp + r
// A lane's weights (<= 48 values) live in registers for the whole kernel.
template <int KS, int CBLK>  // k-steps of 4 inputs (w + 1 <= 4 KS), 16-channel blocks (cb = 16 CBLK)
struct AsProj {
  static constexpr int CB = 16 * CBLK;
  float wk[KS][CBLK], wv[KS][CBLK], wq[KS][CBLK];  // W'[k][c] for this lane's k = 4s + grp, c = cb*16 + col

  // columns of wkvq (w, 3 CB) and bkvq (3 CB): [K | V | Q]
  __device__ __forceinline__ void load_weights(const float* __restrict__ wkvq, const float* __restrict__ bkvq, int w, float qscale,
                                               int col, int grp) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + grp;
#pragma unroll
      for (int cb = 0; cb < CBLK; ++cb) {
        const int c = cb * 16 + col;
        const float* wrow = wkvq + (size_t)min(k, w - 1) * 3 * CB;
        wk[s][cb] = k < w ? wrow[c] : (k == w ? bkvq[c] : 0.f);
        wv[s][cb] = k < w ? wrow[CB + c] : (k == w ? bkvq[CB + c] : 0.f);
        wq[s][cb] = (k < w ? wrow[2 * CB + c] : (k == w ? bkvq[2 * CB + c] : 0.f)) * qscale;
      }
    }
  }

  // X'[row = col][k = 4s + grp] from xp = the lane's row of x (clamped to the group's last); rows past `as` are zero rows (their
  // keys are masked, their queries not stored)
  static __device__ __forceinline__ void load_x(const float* __restrict__ xp, int as, int w, int col, int grp, float (&xv)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + grp;
      const float v = xp[min(k, w - 1)];
      xv[s] = col < as ? (k < w ? v : (k == w ? 1.f : 0.f)) : 0.f;
    }
  }

  // V and the key-major score tile S^T of the group whose X' is xv
  __device__ __forceinline__ void project(const float (&xv)[KS], f32x4 (&V)[CBLK], f32x4& S) const {
    f32x4 Kt[CBLK], Qt[CBLK];
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
      Kt[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; Qt[cb] = Kt[cb]; V[cb] = Kt[cb];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        Kt[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[s][cb], xv[s], Kt[cb], 0, 0, 0);
        Qt[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[s][cb], xv[s], Qt[cb], 0, 0, 0);
        V[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s], wv[s][cb], V[cb], 0, 0, 0);
      }
    }
    S = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) S = __builtin_amdgcn_mfma_f32_16x16x4f32(Kt[cb][r], Qt[cb][r], S, 0, 0, 0);
  }
};

// Softmax over the neighbours of one column of the re-weighting tail's logits: v[k] = the logit of neighbour k, -inf past `as`,
// on entry; on return v[k] = expf(logit - max), 0 past `as`.  Returns their sum in ascending k (the callers divide: v[k] / sum).
__device__ __forceinline__ float as_softmax_column(int as, float (&v)[AS_MAX]) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < AS_MAX; ++k) mx = fmaxf(mx, v[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < AS_MAX; ++k) {
    v[k] = k < as ? expf(v[k] - mx) : 0.f;
    sum += v[k];
  }
  return sum;
}

// ---- host side
// the attention kernels' score scale: 1 / sqrt(cb) in the log2 domain
static inline float as_qscale(int cb) { return LOG2E / sqrtf((float)cb); }

// workgroups of 256 threads for a grid-stride loop over `total` elements
static inline unsigned as_grid(long total) {
  const long grid = (total + 255) / 256;
  return (unsigned)(grid > 16384 ? 16384 : grid);
}

// f(KS, CBLK) as integral constants for the AsProj instance of a narrow layer: w inputs and the bias in KS = 2..4 k-steps,
// cb = 32 or 64 (the entry points refuse anything else).  Only those six kernels are instantiated.
template <class F>
int with_as_proj(int w, int cb, F&& f) {
  auto with_ks = [&](auto cblk) {
    const int ks = (w + 1 + 3) / 4;
    if (ks <= 2) return f(std::integral_constant<int, 2>{}, cblk);
    if (ks == 3) return f(std::integral_constant<int, 3>{}, cblk);
    return f(std::integral_constant<int, 4>{}, cblk);
  };
  if (cb == 32) return with_ks(std::integral_constant<int, 2>{});
  return with_ks(std::integral_constant<int, 4>{});
}

}  // namespace pasnl
