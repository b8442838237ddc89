// Backward of a set-abstraction layer's grouping and local cell (grouping.hip: sa_group_kernel, cells.hip:
// sa_local_cell_kernel) for gfx950: pasnl_cls_sa_local_cell_grad and pasnl_cls_sa_group_grad.  DESIGN.md 4.5 has the formulas,
// the tile orientations and the resource figures.
//
// Local cell.  Per group, X (k x w), dM = grad_out[g] (c2 x 32); H1, H2, G are recomputed, nothing of the forward is saved:
//     dH2 = G dM^T     dG = H2 dM     dZ2 = dH2 o [H2 > 0]     dZg = dG o [G > 0]     dH1 = dZ2 W1^T     dZ1 = dH1 o [H1 > 0]
//     dX = dZ1 W0^T,  dX[:, 0:3] += dZg Ww^T
//     dW1 = sum H1^T dZ2   db1 = sum dZ2   dW0 = sum X^T dZ1   db0 = sum dZ1   dWw = sum X[:, 0:3]^T dZg   dbw = sum dZg
// One wave per group on v_mfma_f32_32x32x2_f32, 32 neighbours (p) at a time, weights in LDS, as the forward.  A D tile holds,
// in lane (ql, h), column ql and the 16 rows kappa(r, h): as an A operand it is D^T . B, as a B operand A . D -- either way the
// product contracts the tile's ROW index.  So every tile is formed in the orientation its consumer contracts:
//     H1^T[c1][p]  A = W0 (LDS)           B = X row (regs)       as the forward
//     H2  [p][c2]  A = H1^T               B = W1 (LDS)           as the forward; H2^T = its transpose
//     G^T [j][p]   A = Ww (LDS)           B = X row              the forward's product with A and B exchanged
//     dG^T[j][p]   A = dM[c2][j] (global) B = H2^T
//     dH2^T[c2][p] A = dM[c2][j] (global) B = G^T
//     dH1^T[c1][p] A = W1^T (LDS copy)    B = dZ2^T
//     dX  [p][c]   A = dZ1^T              B = W0^T (LDS copy);   columns 0-2: A = dZg^T, B = Ww^T
//     dW1 [c1][c2] A = H1 [p][c1]         B = dZ2[p][c2]         dW0[c][c1]: A = X[p][c] (global), B = dZ1[p][c1]
//     dWw [c][j]   A = X[p][c] (global)   B = dZg[p][j]
// The row-p forms the weight gradients contract (H1, dZ2, dZ1, dZg) and H2^T are transposes of a tile through a 32 x 33 LDS
// patch of the wave's own: 32 LDS accesses per lane where a second MFMA chain would be 32 to 64 instructions of 64 cycles.
// The weight-gradient accumulators stay in registers over a wave's whole persistent loop and are flushed once, to the wave's
// slot of the partials; sa_local_cell_fold_kernel sums the slots in ascending order.  The slot count depends on `groups`
// alone (min(groups, SAG_SLOTS)), never on the device: the gradients are a pure function of the inputs.  No fp atomics.
//
// Grouping.  new_point[j,s] = [xyz[i] - new_xyz[j] | xyz[i] | feature[i]], skip[j] = max_s new_point[j,s].  With
// e[j,s] = grad_new_point[j,s] + share[j,s], share = grad_skip[j] / count on every element equal to its column's maximum
// (TensorFlow's reduce_max rule; the maximum recomputed with the forward's float32 expression):
//     r[j,s] = [e[0:3] + e[3:6] | e[6:]]        grad_new_xyz[j] = -sum_s e[j,s,0:3]   (s ascending)
// and r is scattered by the ordered segmented sums of grouping.hip (pasnl_group_point_grad_det), as pasnl_cls_as_gather_grad
// does: one scatter per output, no fp atomics.
#include "common.hpp"
#include "sa_tail.hpp"

namespace pasnl {

constexpr int SAG_SLOTS = 1024;   // cap of the partial slots (one per wave): 256 workgroups of 4 waves
constexpr int SAG_MAX_W32 = 96;   // widest x row at c1 = c2 = 32: three 32-channel chunks of dW0 accumulators
constexpr int SAG_MAX_W64 = 96;   //               at c1 = c2 = 64 (beyond one chunk: three launches, see local_cell_grad_launch)
constexpr int SAG_TP = 33;        // row pitch of a wave's transpose patch

// floats of one partial slot: [dW0 (w,c1) | db0 (c1) | dW1 (c1,c2) | db1 (c2) | dWw (3,32) | dbw (32)]
static inline size_t sag_partial_floats(int w, int c1, int c2) {
  return (size_t)w * c1 + c1 + (size_t)c1 * c2 + c2 + 3 * 32 + 32;
}
static inline long sag_slots(long groups) { return groups < SAG_SLOTS ? groups : SAG_SLOTS; }

// D tile -> its transpose, through the wave's own LDS patch T (32 x SAG_TP floats)
__device__ __forceinline__ f32x16 tile_transpose(const f32x16& d, float* T, int ql, int h) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the reads of the patch's previous use)
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) T[ql * SAG_TP + kappa(r, h)] = d[r];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f32x16 e;
#pragma unroll
  for (int r = 0; r < 16; ++r) e[r] = T[kappa(r, h) * SAG_TP + ql];
  return e;
}

__device__ __forceinline__ float tile_sum(const f32x16& d) {
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += d[r];
  return s;
}

// C = c1 = c2; NCH = 32-channel chunks of an x row.  What a launch produces: G1 = the partials of dW1, db1, dWw, dbw; G0 = those of
// dW0, db0; DX = grad_x.  Each part adds accumulators or tiles of its own to the recomputed forward and the dZ chain the three
// share, so the parts that fit the register file together run as one launch and the others as launches of their own
// (local_cell_grad_launch): the bits do not depend on the split.
template <int C, int NCH, bool G1, bool G0, bool DX>
__global__ __launch_bounds__(256) void sa_local_cell_grad_kernel(long groups, long slots, int k, int w, const float* __restrict__ x,
                                                                const float* __restrict__ w0, const float* __restrict__ b0,
                                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                                const float* __restrict__ ww, const float* __restrict__ bw,
                                                                const float* __restrict__ gout, float* __restrict__ grad_x,
                                                                float* __restrict__ partials) {
  constexpr int NB = C / 32;
  constexpr int wp = NCH * 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* W0s = reinterpret_cast<float*>(smem);  // [wp][C]   rows >= w are zeros
  float* W0Ts = W0s + wp * C;                   // [C][wp]
  float* W1s = W0Ts + C * wp;                   // [C][C]
  float* W1Ts = W1s + C * C;                    // [C][C]
  float* Wws = W1Ts + C * C;                    // [4][32]   row 3 = 0
  float* B0s = Wws + 4 * 32;                    // [C]
  float* Bws = B0s + C;                         // [32]
  float* Ts = Bws + 32;                         // [4 waves][32][SAG_TP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, ql = lane & 31;

  for (int i = tid; i < wp * C; i += 256) {
    const float v = (i / C) < w ? w0[i] : 0.f;
    W0s[i] = v;
    W0Ts[(i % C) * wp + i / C] = v;
  }
  for (int i = tid; i < C * C; i += 256) {
    const float v = w1[i];
    W1s[i] = v;
    W1Ts[(i % C) * C + i / C] = v;
  }
  for (int i = tid; i < 4 * 32; i += 256) Wws[i] = i < 3 * 32 ? ww[i] : 0.f;
  for (int i = tid; i < C; i += 256) B0s[i] = b0[i];
  for (int i = tid; i < 32; i += 256) Bws[i] = bw[i];
  __syncthreads();

  const long slot = (long)blockIdx.x * 4 + wave;
  if (slot >= slots) return;  // (the whole wave; no barrier follows)
  float* T = Ts + wave * 32 * SAG_TP;

  float b1r[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) b1r[cb] = b1[cb * 32 + ql];

  // weight-gradient accumulators of the wave's whole loop
  f32x16 dW1[G1 ? NB : 1][G1 ? NB : 1], dW0[G0 ? NCH : 1][G0 ? NB : 1], dWw;
  float db1[NB], db0[NB], dbw = 0.f;
#pragma unroll
  for (int a = 0; a < (G1 ? NB : 1); ++a)
#pragma unroll
    for (int c = 0; c < (G1 ? NB : 1); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) dW1[a][c][r] = 0.f;
#pragma unroll
  for (int a = 0; a < (G0 ? NCH : 1); ++a)
#pragma unroll
    for (int c = 0; c < (G0 ? NB : 1); ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) dW0[a][c][r] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) dWw[r] = 0.f;
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) db1[cb] = db0[cb] = 0.f;

  for (long g = slot; g < groups; g += slots) {
    const float* gm = gout + (size_t)g * C * 32;  // dM[c2][j]
    for (int tile = 0; tile < k; tile += 32) {
      const float* xtile = x + ((size_t)g * k + tile) * w;
      const float* xrow = xtile + (size_t)ql * w;  // this lane's neighbour row

      // ---- forward, recomputed: H1^T[c1][p] and G^T[j][p]
      f32x16 H1T[NB], GT;
#pragma unroll
      for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) H1T[ob][r] = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) GT[r] = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        float xr[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int c = ch * 32 + 2 * t + h;
          xr[t] = c < w ? xrow[c] : 0.f;
        }
        if (ch == 0) {
          GT = __builtin_amdgcn_mfma_f32_32x32x2f32(Wws[h * 32 + ql], xr[0], GT, 0, 0, 0);
          GT = __builtin_amdgcn_mfma_f32_32x32x2f32(Wws[(2 + h) * 32 + ql], xr[1], GT, 0, 0, 0);
        }
        const int live = min(16, (w - ch * 32 + 1) >> 1);  // MFMA steps with a non-zero k pair (uniform)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          if (t < live) {
            const float* wrow = W0s + (ch * 32 + 2 * t + h) * C + ql;
#pragma unroll
            for (int ob = 0; ob < NB; ++ob)
              H1T[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[ob * 32], xr[t], H1T[ob], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) H1T[ob][r] = fmaxf(H1T[ob][r] + B0s[ob * 32 + kappa(r, h)], 0.f);
#pragma unroll
      for (int r = 0; r < 16; ++r) GT[r] = fmaxf(GT[r] + Bws[kappa(r, h)], 0.f);

      __builtin_amdgcn_sched_barrier(0);
      // ---- H2[p][c2] by the forward's chain, kept as H2^T[c2][p]
      f32x16 H2T[NB];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        f32x16 H2;
#pragma unroll
        for (int r = 0; r < 16; ++r) H2[r] = 0.f;
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
          const float* w1p = W1s + (blk * 32 + 4 * h) * C + cb * 32 + ql;
#pragma unroll
          for (int t = 0; t < 16; ++t)
            H2 = __builtin_amdgcn_mfma_f32_32x32x2f32(H1T[blk][t], w1p[kappa(t, 0) * C], H2, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) H2[r] = fmaxf(H2[r] + b1r[cb], 0.f);
        H2T[cb] = tile_transpose(H2, T, ql, h);
        __builtin_amdgcn_sched_barrier(0);
      }

      __builtin_amdgcn_sched_barrier(0);
      // ---- dG^T[j][p] = dM^T . H2^T, masked by G^T
      f32x16 dZgT;
#pragma unroll
      for (int r = 0; r < 16; ++r) dZgT[r] = 0.f;
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t)
          dZgT = __builtin_amdgcn_mfma_f32_32x32x2f32(gm[(cb * 32 + kappa(t, h)) * 32 + ql], H2T[cb][t], dZgT, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) dZgT[r] = GT[r] > 0.f ? dZgT[r] : 0.f;

      __builtin_amdgcn_sched_barrier(0);
      // ---- dH2^T[c2][p] = dM . G^T, masked by H2^T: dZ2^T takes H2^T's registers
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.f;
        const float* gr = gm + (cb * 32 + ql) * 32 + 4 * h;
#pragma unroll
        for (int t = 0; t < 16; ++t) d = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[kappa(t, 0)], GT[t], d, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) H2T[cb][r] = H2T[cb][r] > 0.f ? d[r] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
      }

      __builtin_amdgcn_sched_barrier(0);
      if constexpr (G1) {
        // ---- dW1 += H1^T . dZ2, db1 += column sums of dZ2: both operands as row-p tiles
        f32x16 dZ2[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          dZ2[cb] = tile_transpose(H2T[cb], T, ql, h);
          db1[cb] += tile_sum(dZ2[cb]);
        }
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) {
          const f32x16 H1 = tile_transpose(H1T[ob], T, ql, h);
#pragma unroll
          for (int cb = 0; cb < NB; ++cb)
#pragma unroll
            for (int t = 0; t < 16; ++t)
              dW1[ob][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(H1[t], dZ2[cb][t], dW1[ob][cb], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }

      __builtin_amdgcn_sched_barrier(0);
      // ---- dH1^T[c1][p] = W1 . dZ2^T, masked by H1^T: dZ1^T takes H1^T's registers
#pragma unroll
      for (int ob = 0; ob < NB; ++ob) {
        f32x16 d;
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          const float* wt = W1Ts + (cb * 32 + 4 * h) * C + ob * 32 + ql;
#pragma unroll
          for (int t = 0; t < 16; ++t) d = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[kappa(t, 0) * C], H2T[cb][t], d, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) H1T[ob][r] = H1T[ob][r] > 0.f ? d[r] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
      }

      __builtin_amdgcn_sched_barrier(0);
      // X as a row-p A operand of the sums over the neighbours: X[p = kappa(t, h)][c = ch*32 + ql], rows read from global memory
      f32x16 dZg;
      if constexpr (G1) {
        // ---- dWw += X[:, 0:3]^T . dZg, dbw (with G0: on chunk 0's operands of the loop below)
        dZg = tile_transpose(dZgT, T, ql, h);
        dbw += tile_sum(dZg);
      }
      if constexpr (G1 && !G0) {
        const float* xc = xtile + (size_t)(4 * h) * w + min(ql, w - 1);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const float v = xc[(size_t)kappa(t, 0) * w];
          dWw = __builtin_amdgcn_mfma_f32_32x32x2f32(ql < w ? v : 0.f, dZg[t], dWw, 0, 0, 0);
        }
      }
      if constexpr (G0) {
        // ---- dW0 += X^T . dZ1, db0
        f32x16 dZ1[NB];
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) {
          dZ1[ob] = tile_transpose(H1T[ob], T, ql, h);
          db0[ob] += tile_sum(dZ1[ob]);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c = ch * 32 + ql;
          const float* xc = xtile + (size_t)(4 * h) * w + min(c, w - 1);
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float v = xc[(size_t)kappa(t, 0) * w];
            const float xa = c < w ? v : 0.f;
            if constexpr (G1)
              if (ch == 0) dWw = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, dZg[t], dWw, 0, 0, 0);
#pragma unroll
            for (int ob = 0; ob < NB; ++ob)
              dW0[ch][ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, dZ1[ob][t], dW0[ch][ob], 0, 0, 0);
          }
        }
      }

      __builtin_amdgcn_sched_barrier(0);
      if constexpr (DX) {
        // ---- dX[p][c] = dZ1 . W0^T (+ dZg . Ww^T in columns 0-2): rows p = kappa(r, h), 32 consecutive columns per store
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (ch * 32 < w) {
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
              const float* wt = W0Ts + (ob * 32 + 4 * h) * wp + ch * 32 + ql;
#pragma unroll
              for (int t = 0; t < 16; ++t) d = __builtin_amdgcn_mfma_f32_32x32x2f32(H1T[ob][t], wt[kappa(t, 0) * wp], d, 0, 0, 0);
            }
            if (ch == 0) {
              const float* wr = Wws + min(ql, 3) * 32 + 4 * h;  // Ww[c = ql][j]; row 3 is zeros
#pragma unroll
              for (int t = 0; t < 16; ++t) d = __builtin_amdgcn_mfma_f32_32x32x2f32(dZgT[t], wr[kappa(t, 0)], d, 0, 0, 0);
            }
            const int c = ch * 32 + ql;
            if (c < w) {
              float* o = grad_x + ((size_t)g * k + tile + 4 * h) * w + c;
#pragma unroll
              for (int r = 0; r < 16; ++r) o[(size_t)kappa(r, 0) * w] = d[r];
            }
          }
        }
      }
    }
  }

  float* P = partials + (size_t)slot * ((size_t)w * C + C + C * C + C + 3 * 32 + 32);
  if constexpr (G0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = ch * 32 + kappa(r, h);
          if (c < w) P[(size_t)c * C + ob * 32 + ql] = dW0[ch][ob][r];
        }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
      const float v = half_sum(db0[ob]);
      if (h == 0) P[(size_t)w * C + ob * 32 + ql] = v;
    }
  }
  if constexpr (G1) {
    P += (size_t)w * C + C;
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
      for (int cb = 0; cb < NB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) P[(ob * 32 + kappa(r, h)) * C + cb * 32 + ql] = dW1[ob][cb][r];
    P += C * C;
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      const float v = half_sum(db1[cb]);
      if (h == 0) P[cb * 32 + ql] = v;
    }
    P += C;
    if (h == 0) {  // rows c = kappa(r, 0) = r for r < 3
#pragma unroll
      for (int r = 0; r < 3; ++r) P[r * 32 + ql] = dWw[r];
    }
    P += 3 * 32;
    const float v = half_sum(dbw);
    if (h == 0) P[ql] = v;
  }
}

// element e of a slot -> its gradient: the slots summed in ascending order
__global__ __launch_bounds__(256) void sa_local_cell_fold_kernel(long slots, int w, int c1, int c2, const float* __restrict__ partials,
                                                                float* __restrict__ gw0, float* __restrict__ gb0,
                                                                float* __restrict__ gw1, float* __restrict__ gb1,
                                                                float* __restrict__ gww, float* __restrict__ gbw) {
  const long n0 = (long)w * c1, n1 = n0 + c1, n2 = n1 + (long)c1 * c2, n3 = n2 + c2, n4 = n3 + 96, total = n4 + 32;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float* dst = e < n0 ? (gw0 ? gw0 + e : nullptr)
             : e < n1 ? (gb0 ? gb0 + (e - n0) : nullptr)
             : e < n2 ? (gw1 ? gw1 + (e - n1) : nullptr)
             : e < n3 ? (gb1 ? gb1 + (e - n2) : nullptr)
             : e < n4 ? (gww ? gww + (e - n3) : nullptr)
                      : (gbw ? gbw + (e - n4) : nullptr);
  if (dst == nullptr) return;
  float s = 0.f;
  for (long i = 0; i < slots; ++i) s += partials[(size_t)i * total + e];
  *dst = s;
}

__global__ __launch_bounds__(256) void sag_zero_kernel(long n, float* __restrict__ p) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = 0.f;
}

static size_t sag_lds_bytes(int c, int nch) {
  const int wp = nch * 32;
  return ((size_t)2 * wp * c + (size_t)2 * c * c + 4 * 32 + c + 32 + 4 * 32 * SAG_TP) * sizeof(float);
}

template <int C, int NCH>
static int local_cell_grad_launch(long groups, int k, int w, const float* x, const float* w0, const float* b0, const float* w1,
                                  const float* b1, const float* ww, const float* bw, const float* gout, float* grad_x,
                                  float* partials, bool want1, bool want0, hipStream_t st) {
  const long slots = sag_slots(groups);
  const dim3 grid((unsigned)((slots + 3) / 4)), block(256);
  const size_t lds = sag_lds_bytes(C, NCH);
  auto run = [&](auto kernel, float* gx, float* part) {
    return launch(kernel, grid, block, lds, st, groups, slots, k, w, x, w0, b0, w1, b1, ww, bw, gout, gx, part);
  };
  float* const none = nullptr;
  // one launch where the three parts fit the register file together; else the parts that do, one after the other (each repeats
  // the recomputed forward)
  constexpr int PARTS = (C == 32 && NCH <= 2) || (C == 64 && NCH == 1) ? 1 : (C == 32 ? 2 : 3);
  if constexpr (PARTS == 1) {
    if (partials != nullptr && grad_x != nullptr) return run(sa_local_cell_grad_kernel<C, NCH, true, true, true>, grad_x, partials);
  }
  if (partials != nullptr) {
    int rc;
    if constexpr (PARTS <= 2) {
      rc = run(sa_local_cell_grad_kernel<C, NCH, true, true, false>, none, partials);
    } else {
      // (a part none of whose gradients is asked for is not run: the fold does not read its region of the slots)
      rc = want1 ? run(sa_local_cell_grad_kernel<C, NCH, true, false, false>, none, partials) : PASNL_OK;
      if (rc == PASNL_OK && want0) rc = run(sa_local_cell_grad_kernel<C, NCH, false, true, false>, none, partials);
    }
    if (rc != PASNL_OK || grad_x == nullptr) return rc;
  }
  return run(sa_local_cell_grad_kernel<C, NCH, false, false, true>, grad_x, none);
}

// one thread per (group, folded column q of 3 + c): q < 3 folds columns q and 3 + q of the group's rows, q >= 3 is column 3 + q
__global__ __launch_bounds__(256) void sa_group_fold_kernel(int n, int c, int m, int k, long total, const float* __restrict__ xyz,
                                                           const float* __restrict__ feature, const int* __restrict__ idx,
                                                           const float* __restrict__ new_xyz, const float* __restrict__ gnp,
                                                           const float* __restrict__ gskip, float* __restrict__ r_xyz,
                                                           float* __restrict__ r_feat, float* __restrict__ grad_new_xyz) {
  const int wq = 3 + c, W = 6 + c;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long g = e / wq;
    const int q = (int)(e - g * wq);
    const long bi = g / m;
    const int* gi = idx + g * k;
    const float* gp = gnp ? gnp + (size_t)g * k * W : nullptr;
    if (q >= 3) {
      if (r_feat == nullptr) continue;
      const float* cf = feature + (size_t)bi * n * c + (q - 3);
      float mx = -INFINITY, share = 0.f;
      if (gskip != nullptr) {
        int cnt = 0;
        for (int s = 0; s < k; ++s) {
          const float v = cf[(size_t)gi[s] * c];
          if (v > mx) { mx = v; cnt = 1; }
          else if (v == mx) ++cnt;
        }
        share = gskip[g * W + 3 + q] / (float)cnt;
      }
      for (int s = 0; s < k; ++s) {
        float ev = gp ? gp[(size_t)s * W + 3 + q] : 0.f;
        if (gskip != nullptr && cf[(size_t)gi[s] * c] == mx) ev += share;
        r_feat[((size_t)g * k + s) * c + (q - 3)] = ev;
      }
      continue;
    }
    if (r_xyz == nullptr && grad_new_xyz == nullptr) continue;
    const float* cx = xyz + (size_t)bi * n * 3 + q;
    const float centre = new_xyz[g * 3 + q];
    float mx0 = -INFINITY, mx3 = -INFINITY, share0 = 0.f, share3 = 0.f;
    if (gskip != nullptr) {
      int cnt0 = 0, cnt3 = 0;
      for (int s = 0; s < k; ++s) {
        const float v3 = cx[(size_t)gi[s] * 3];
        const float v0 = v3 - centre;  // the forward's expression
        if (v0 > mx0) { mx0 = v0; cnt0 = 1; }
        else if (v0 == mx0) ++cnt0;
        if (v3 > mx3) { mx3 = v3; cnt3 = 1; }
        else if (v3 == mx3) ++cnt3;
      }
      share0 = gskip[g * W + q] / (float)cnt0;
      share3 = gskip[g * W + 3 + q] / (float)cnt3;
    }
    float acc = 0.f;
    for (int s = 0; s < k; ++s) {
      float e0 = gp ? gp[(size_t)s * W + q] : 0.f;
      float e3 = gp ? gp[(size_t)s * W + 3 + q] : 0.f;
      if (gskip != nullptr) {
        const float v3 = cx[(size_t)gi[s] * 3];
        const float v0 = v3 - centre;
        if (v0 == mx0) e0 += share0;
        if (v3 == mx3) e3 += share3;
      }
      acc += e0;
      if (r_xyz != nullptr) r_xyz[((size_t)g * k + s) * 3 + q] = e0 + e3;
    }
    if (grad_new_xyz != nullptr) grad_new_xyz[g * 3 + q] = -acc;
  }
}

static unsigned sag_grid(long total) {
  const long grid = (total + 255) / 256;
  return (unsigned)(grid > 16384 ? 16384 : grid);
}

}  // namespace pasnl

using namespace pasnl;

extern "C" size_t pasnl_cls_sa_local_cell_grad_workspace_bytes(int groups, int w, int c1, int c2) {
  if (groups <= 0 || w < 3 || c1 <= 0 || c2 <= 0) return 0;
  return (size_t)sag_slots(groups) * sag_partial_floats(w, c1, c2) * sizeof(float);
}

extern "C" int pasnl_cls_sa_local_cell_grad(int groups, int k, int w, int c1, int c2, const float* x, const float* w0, const float* b0,
                                            const float* w1, const float* b1, const float* ww, const float* bw,
                                            const float* grad_out, float* grad_x, float* grad_w0, float* grad_b0, float* grad_w1,
                                            float* grad_b1, float* grad_ww, float* grad_bw, void* workspace, size_t workspace_bytes,
                                            pasnl_stream_t stream) {
  PASNL_REQUIRE(groups >= 0 && k > 0 && w >= 3 && c1 > 0 && c2 > 0, PASNL_EINVAL);
  PASNL_REQUIRE(k % 32 == 0 && c1 == c2 && (c1 == 32 || c1 == 64) && w <= (c1 == 32 ? SAG_MAX_W32 : SAG_MAX_W64),
                PASNL_EUNSUPPORTED);
  const bool wgrad = grad_w0 || grad_b0 || grad_w1 || grad_b1 || grad_ww || grad_bw;
  hipStream_t st = pasnl_hip_stream(stream);
  if (groups == 0) {  // the sums over no group
    struct { float* p; long n; } z[6] = {{grad_w0, (long)w * c1}, {grad_b0, c1}, {grad_w1, (long)c1 * c2},
                                         {grad_b1, c2},           {grad_ww, 96}, {grad_bw, 32}};
    if (!wgrad) return PASNL_OK;
    for (auto& t : z)
      if (t.p != nullptr) hipLaunchKernelGGL(sag_zero_kernel, dim3(sag_grid(t.n)), dim3(256), 0, st, t.n, t.p);
    return pasnl_launch_status();
  }
  PASNL_REQUIRE(x && w0 && b0 && w1 && b1 && ww && bw && grad_out && (grad_x || wgrad), PASNL_ENULL);
  PASNL_REQUIRE(!wgrad || workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(!wgrad || (workspace && workspace_bytes >= pasnl_cls_sa_local_cell_grad_workspace_bytes(groups, w, c1, c2)),
                PASNL_EWORKSPACE);
  float* partials = wgrad ? static_cast<float*>(workspace) : nullptr;
  const int nch = (w + 31) / 32;
  int rc;
#define SAG_CASE(C_, N_)                                                                                                     \
  if (c1 == C_ && nch == N_)                                                                                                  \
    rc = local_cell_grad_launch<C_, N_>(groups, k, w, x, w0, b0, w1, b1, ww, bw, grad_out, grad_x, partials,               \
                                        grad_w1 || grad_b1 || grad_ww || grad_bw, grad_w0 || grad_b0, st);                  \
  else
  SAG_CASE(32, 1) SAG_CASE(32, 2) SAG_CASE(32, 3) SAG_CASE(64, 1) SAG_CASE(64, 2) SAG_CASE(64, 3) rc = PASNL_EUNSUPPORTED;
#undef SAG_CASE
  if (rc != PASNL_OK) return rc;
  if (wgrad) {
    const long total = (long)sag_partial_floats(w, c1, c2);
    hipLaunchKernelGGL(sa_local_cell_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, sag_slots(groups), w, c1, c2,
                       partials, grad_w0, grad_b0, grad_w1, grad_b1, grad_ww, grad_bw);
  }
  return pasnl_launch_status();
}

// [lists of the ordered scatter | r_xyz (rows,3) | r_feat (rows,c)], rows = b m k
extern "C" size_t pasnl_cls_sa_group_grad_workspace_bytes(int b, int n, int c, int m, int k) {
  if (b <= 0 || n <= 0 || c <= 0 || m < 0 || k <= 0) return 0;
  const size_t rows = (size_t)b * m * k;
  return pasnl_grad_workspace_bytes(b, n, (long)m * k) + rows * (size_t)(3 + c) * sizeof(float);
}

extern "C" int pasnl_cls_sa_group_grad(int b, int n, int c, int m, int k, const float* xyz, const float* feature, const int* idx,
                                       const float* new_xyz, const float* grad_new_point, const float* grad_skip, float* grad_xyz,
                                       float* grad_feature, float* grad_new_xyz, void* workspace, size_t workspace_bytes,
                                       pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && c > 0 && m >= 0 && k > 0, PASNL_EINVAL);
  PASNL_REQUIRE(n <= 38400 && (long)m * k < (1L << 31) && (long)b * m < (1L << 31), PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  const long groups = (long)b * m, rows = groups * k;
  PASNL_REQUIRE((grad_xyz || grad_feature || grad_new_xyz) && (rows == 0 || (xyz && feature && idx && new_xyz)), PASNL_ENULL);
  const bool scatter = grad_xyz || grad_feature;
  PASNL_REQUIRE(!scatter || workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(!scatter || (workspace && workspace_bytes >= pasnl_cls_sa_group_grad_workspace_bytes(b, n, c, m, k)),
                PASNL_EWORKSPACE);
  const size_t lists_bytes = pasnl_grad_workspace_bytes(b, n, (long)m * k);
  float* r_xyz = scatter ? reinterpret_cast<float*>(static_cast<char*>(workspace) + lists_bytes) : nullptr;
  float* r_feat = scatter ? r_xyz + (size_t)rows * 3 : nullptr;
  if (rows > 0) {
    hipLaunchKernelGGL(sa_group_fold_kernel, dim3(sag_grid(groups * (3 + c))), dim3(256), 0, pasnl_hip_stream(stream), n, c, m, k,
                       groups * (3 + c), xyz, feature, idx, new_xyz, grad_new_point, grad_skip, grad_xyz ? r_xyz : nullptr,
                       grad_feature ? r_feat : nullptr, grad_new_xyz);
    PASNL_REQUIRE(pasnl_launch_status() == PASNL_OK, PASNL_ELAUNCH);
  }
  // the two scatters share the lists' region: they run one after the other on the stream
  if (grad_xyz != nullptr) {
    const int rc = pasnl_group_point_grad_det(b, n, 3, m, k, r_xyz, idx, grad_xyz, workspace, lists_bytes, stream);
    if (rc != PASNL_OK) return rc;
  }
  if (grad_feature != nullptr) {
    const int rc = pasnl_group_point_grad_det(b, n, c, m, k, r_feat, idx, grad_feature, workspace, lists_bytes, stream);
    if (rc != PASNL_OK) return rc;
  }
  return PASNL_OK;
}
