// The product of a set-abstraction layer's tail (cells.hip: sa_tail_kernel), shared with the kernels that run a tail in front
// of other work (mlp_pool.hip: tail_group_all_kernel): one definition, so that both give the same bits.
#pragma once
#include "common.hpp"

namespace pasnl {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row index held in register r of lane-half h of a 32x32 MFMA C/D tile
__device__ __forceinline__ int kappa(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// ---- the MFMA attention kernels' softmax helpers (cells.hip forward, nl_grad.hip backward; fast_exp2: common.hpp)
// A value combined across the two halves of the wave (lane l with lane l ^ 32): v_permlane32_swap_b32 with both operands the
// same register leaves {value of lane l & 31, value of lane (l & 31) + 32} in every lane -- one vector instruction where
// __shfl_xor(v, 32) is a ds_bpermute_b32 (an LDS round trip).  lo + hi in both halves: the same bits as own + other.
__device__ __forceinline__ float half_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// A-operand stream of one 32-channel output block: weight rows k (lanes 0-31) / k+1 (lanes 32-63), 16 k-steps per chunk,
// the next chunk requested while the current one feeds the MFMAs.
constexpr int TAIL_KS = 16;  // k-steps (pairs of input channels) per operand chunk
// PACKED: the matrix in operand order (pasnl_sa_tail_pack_weights): P[chunk][h][column][t] = W[32 chunk + 2 t + h][column], zero
// beyond kdim -- a lane's 16 words of a chunk are 64 contiguous bytes = four 16-byte loads instead of sixteen 4-byte ones (the
// weight loads were 5 of a launch's 31 us: EXPERIMENTS "Round 5")
template <bool PACKED>
struct TailW {
  const float* __restrict__ base;  // W + cbase + l32  (PACKED: the matrix itself)
  int C, kdim, h;
  int col;                         // PACKED: cbase + l32
  __device__ __forceinline__ void load(int k0, float (&a)[TAIL_KS]) const {
    if constexpr (PACKED) {
      const int chunk = min(k0 >> 5, ((kdim + 31) >> 5) - 1);  // (the request behind the last chunk re-reads it)
      const float4* p = reinterpret_cast<const float4*>(base + ((size_t)(chunk * 2 + h) * C + col) * TAIL_KS);
#pragma unroll
      for (int q = 0; q < TAIL_KS / 4; ++q) {
        const float4 v = p[q];
        a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
      }
      return;
    }
#pragma unroll
    for (int t = 0; t < TAIL_KS; ++t) {
      // rows past kdim are CLAMPED, not skipped: the X tile is zero there, so any finite weight contributes nothing, and
      // unconditional loads need no branch each and let the waits count (a skipped load costs an exec test per load and
      // the waits in front of the products all became vmcnt(0))
      const int kk = min(k0 + 2 * t + h, kdim - 1);
      a[t] = base[(size_t)kk * C];
    }
  }
};

// acc += W[:, block]^T . X^T for X rows held in LDS as xs[k * 33 + row] (k-major, zero-padded to a multiple of 2 TAIL_KS
// channels).  Chunks of TAIL_KS unconditional MFMAs (zero X beyond kdim), the next chunk's weights in flight.
template <bool PACKED>
__device__ __forceinline__ f32x16 tail_product(const TailW<PACKED>& W, const float* __restrict__ xs, int l32, f32x16 acc) {
  // `a` feeds the products while `b` (the next chunk) is in flight, covered by TAIL_KS products (~1000 cycles: an L2 round
  // trip).  One loop body without an early exit -- an exit between a load and its use lets the compiler sink the load behind
  // the exit, right in front of its use -- and the rotation as register copies after the products: by then `b` has arrived.
  float a[TAIL_KS], b[TAIL_KS];
  W.load(0, a);
  for (int k0 = 0; k0 < W.kdim; k0 += 2 * TAIL_KS) {
    W.load(k0 + 2 * TAIL_KS, b);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < TAIL_KS / 4; ++g)
      if (k0 + 8 * g < W.kdim) {  // uniform: a narrow product (9 skip columns) does not pay for a whole chunk
#pragma unroll
        for (int t = 4 * g; t < 4 * g + 4; ++t)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], xs[(k0 + 2 * t + W.h) * 33 + l32], acc, 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < TAIL_KS; ++t) a[t] = b[t];
  }
  return acc;
}

}  // namespace pasnl
