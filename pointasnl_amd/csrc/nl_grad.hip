// Backward of the non-local attention core (cells.hip: nl_attention_*_kernel) for gfx950: pasnl_cls_nl_attention_grad.
//   s_ij = q_i . k_j / sqrt(cb), P = softmax_j(s), O = P V, g = dL/dO:
//     delta_i = sum_c g_ic O_ic          dP_ij = g_i . v_j           dS_ij = P_ij (dP_ij - delta_i)
//     dQ_i = sum_j dS_ij k_j / sqrt(cb)  dK_j = sum_i dS_ij q_i / sqrt(cb)   dV_j = sum_i P_ij g_i
// Nothing of size (B,P,N) exists: P is recomputed tile by tile from Q, K and the rows' log-sum-exp, as the forward computes it.
// Two launches on the fp32 MFMA (v_mfma_f32_32x32x2_f32), both in the forward's "swapped" form -- a product leaves its result
// in the layout the next one takes as its B operand, so nothing is transposed:
//   * nl_grad_query_kernel: a workgroup owns 32 queries, its SPLIT waves walk every SPLIT-th block of 32 keys.  Sweep 1 forms
//     S^T = K_blk . Q^T and the running (max, sum) of each query; the waves' statistics meet in LDS and every wave folds them in
//     ascending wave order (the same bits in each), lse2 = m + log2(l) and delta go to the workspace.  Sweep 2 (dQ wanted):
//     S^T - lse2 comes out of a chain whose accumulator STARTS at -lse2, dP^T = V_blk . g^T out of a second one,
//     dS^T = exp2(S^T - lse2) (dP^T - delta) in registers, dQ^T += K_blk^T . dS^T (the forward's O^T += V^T . P^T with K in
//     V's place; no rescaling, the statistics are final).  Partials merged through LDS by wave 0 in ascending wave order.
//   * nl_grad_key_kernel: a workgroup owns 32 keys, its waves walk query blocks of 32.  S = Q_blk . K^T puts in lane (key, h)
//     the 16 queries kappa(r, h); their lse2 (the initial accumulator) and delta come from the workspace; dP = g_blk . V^T;
//     dV^T += g_blk^T . P and dK^T += Q_blk^T . dS with g / Q rows as coalesced 128-byte A operands.
// Every sum has a fixed order and there is no atomic: the gradients are a pure function of the inputs.
// Rows past a ragged end are zero-filled operands, and the probability of a masked key or query is SELECTED to 0 (never
// multiplied): nothing stale can reach an accumulator.  Scores stay in the log2 domain (log2e / sqrt(cb) folded into Q, as
// in the forward); the gradient scale is 1 / sqrt(cb).
// Registers (DESIGN.md "Non-local attention: backward"): cb <= 64 keeps every operand in registers; at cb = 128 the key-major
// kernel's K and V tiles (B operands shared by all waves of the workgroup) live in LDS.
#include <math.h>
#include <type_traits>
#include "common.hpp"
#include "sa_tail.hpp"

namespace pasnl {

constexpr int NLG_B = 32;  // queries / keys per block

// HC contiguous floats of a row as 16-byte loads; a row that does not exist gives zeros
template <int HC>
__device__ __forceinline__ void nlg_load_row(const float* __restrict__ src, bool valid, float scale, float (&dst)[HC]) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
  for (int g = 0; g < HC / 4; ++g) {
    const float4 v = s4[g];
    dst[4 * g] = valid ? v.x * scale : 0.f;
    dst[4 * g + 1] = valid ? v.y * scale : 0.f;
    dst[4 * g + 2] = valid ? v.z * scale : 0.f;
    dst[4 * g + 3] = valid ? v.w * scale : 0.f;
  }
}

template <int CB, int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void nl_grad_query_kernel(int p, int n, float qscale, float gscale,
                                                                  const float* __restrict__ q, const float* __restrict__ kv,
                                                                  const float* __restrict__ out, const float* __restrict__ gout,
                                                                  float* __restrict__ grad_q, float* __restrict__ lse2,
                                                                  float* __restrict__ delta) {
  constexpr int HC = CB / 2;  // MFMA steps of a score chain = channels per half-wave (step t: channels t and HC + t)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* stats = reinterpret_cast<float*>(smem);  // [SPLIT][2][64]
  float* park = stats + SPLIT * 2 * 64;           // [SPLIT - 1][HC][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;
  const int bi = blockIdx.y, q0 = blockIdx.x * NLG_B;
  const bool qvalid = q0 + ql < p;
  const size_t qrow = (size_t)bi * p + min(q0 + ql, p - 1);
  const float* kvb = kv + (size_t)bi * n * 2 * CB;

  // Q and g as B operands: B[k = h][j = ql] = X[query][h * HC + t]
  float qreg[HC], greg[HC];
  nlg_load_row<HC>(q + qrow * CB + HC * h, qvalid, qscale, qreg);
  nlg_load_row<HC>(gout + qrow * CB + HC * h, qvalid, 1.f, greg);
  // delta = g . O as the diagonal of the MFMA product O_tile . g^T: the SAME chain (channel pairing, order) as dP = V . g^T
  // below, so that where a query's softmax is one-hot (O = that key's V row, bit for bit) dP - delta cancels exactly
  float dl;
  {
    float oreg[HC];
    nlg_load_row<HC>(out + qrow * CB + HC * h, qvalid, 1.f, oreg);
    f32x16 D;
#pragma unroll
    for (int r = 0; r < 16; ++r) D[r] = 0.f;
#pragma unroll
    for (int t = 0; t < HC; ++t) D = __builtin_amdgcn_mfma_f32_32x32x2f32(oreg[t], greg[t], D, 0, 0, 0);
    float mine = 0.f;  // D[i = kappa(r, h)][j = ql]: the diagonal element of column ql sits in half (ql >> 2) & 1
#pragma unroll
    for (int r = 0; r < 16; ++r) mine = kappa(r, h) == ql ? D[r] : mine;
    const auto both = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine), __float_as_uint(mine), false, false);
    dl = __uint_as_float(((ql >> 2) & 1) ? both[1] : both[0]);
  }

  // ---- sweep 1: the statistics of this wave's key blocks
  float mrun = -INFINITY, lrun = 0.f;
  for (int base = wave * NLG_B; base < n; base += SPLIT * NLG_B) {
    const int cnt = min(NLG_B, n - base);
    float kreg[HC];
    nlg_load_row<HC>(kvb + (size_t)(base + min(ql, cnt - 1)) * 2 * CB + HC * h, ql < cnt, 1.f, kreg);
    f32x16 S;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = 0.f;
#pragma unroll
    for (int t = 0; t < HC; ++t) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[t], qreg[t], S, 0, 0, 0);
    if (cnt < NLG_B) {
#pragma unroll
      for (int r = 0; r < 16; ++r) S[r] = kappa(r, h) < cnt ? S[r] : -INFINITY;
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, S[r]);
    tmax = half_max(tmax);
    const float mnew = fmaxf(mrun, tmax);  // finite: every block has >= 1 valid key
    const float alpha = fast_exp2(mrun - mnew);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) psum += fast_exp2(S[r] - mnew);
    psum = half_sum(psum);
    lrun = lrun * alpha + psum;
    mrun = mnew;
  }
  if constexpr (SPLIT > 1) {
    // every wave folds all SPLIT partial statistics in ascending wave order: the same bits in each, no broadcast
    stats[(wave * 2) * 64 + lane] = mrun;
    stats[(wave * 2 + 1) * 64 + lane] = lrun;
    __syncthreads();
    mrun = stats[lane];  // wave 0 has a block (n > 0): finite
    lrun = stats[64 + lane];
    for (int w = 1; w < SPLIT; ++w) {
      const float mw = stats[(w * 2) * 64 + lane], lw = stats[(w * 2 + 1) * 64 + lane];
      const float mnew = fmaxf(mrun, mw);
      const float a0 = fast_exp2(mrun - mnew);
      const float a1 = mw == -INFINITY ? 0.f : fast_exp2(mw - mnew);  // a wave that saw no key block: m = -inf, l = 0
      lrun = lrun * a0 + lw * a1;
      mrun = mnew;
    }
  }
  const float lse = mrun + __log2f(lrun);  // l >= 1: the maximum's own term
  if (wave == 0 && h == 0 && qvalid) {
    lse2[qrow] = lse;
    delta[qrow] = dl;
  }
  if (grad_q == nullptr) return;  // (uniform)

  // ---- sweep 2: dQ^T += K_blk^T . dS^T
  f32x16 dQ[CB / 32];
#pragma unroll
  for (int c = 0; c < CB / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dQ[c][r] = 0.f;
  for (int base = wave * NLG_B; base < n; base += SPLIT * NLG_B) {
    const int cnt = min(NLG_B, n - base);
    const float* krow = kvb + (size_t)(base + min(ql, cnt - 1)) * 2 * CB + HC * h;
    float kreg[HC], vreg[HC];
    nlg_load_row<HC>(krow, ql < cnt, 1.f, kreg);
    nlg_load_row<HC>(krow + CB, ql < cnt, 1.f, vreg);
    f32x16 S, dP;  // -lse2 is the score chain's initial accumulator; delta is subtracted after its chain (see above)
#pragma unroll
    for (int r = 0; r < 16; ++r) { S[r] = -lse; dP[r] = 0.f; }
#pragma unroll
    for (int t = 0; t < HC; ++t) S = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[t], qreg[t], S, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < HC; ++t) dP = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[t], greg[t], dP, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ds = fast_exp2(S[r]) * (dP[r] - dl);
      S[r] = (qvalid && kappa(r, h) < cnt) ? ds : 0.f;
    }
#pragma unroll
    for (int c = 0; c < CB / 32; ++c) {
      float ka[16];  // A[i = channel c * 32 + ql][k = key kappa(t, h)]: coalesced 128-byte row reads
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float v = kvb[(size_t)(base + min(kappa(t, h), cnt - 1)) * 2 * CB + c * 32 + ql];
        ka[t] = kappa(t, h) < cnt ? v : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) dQ[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[t], S[t], dQ[c], 0, 0, 0);
    }
  }
  if constexpr (SPLIT > 1) {
    if (wave > 0) {
      float* pw = park + (size_t)(wave - 1) * HC * 64;
#pragma unroll
      for (int c = 0; c < CB / 32; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) pw[(c * 16 + r) * 64 + lane] = dQ[c][r];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < SPLIT; ++w) {  // (a wave that saw no key block parked zeros)
      const float* pw = park + (size_t)(w - 1) * HC * 64;
#pragma unroll
      for (int c = 0; c < CB / 32; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[c][r] += pw[(c * 16 + r) * 64 + lane];
    }
  }
  if (qvalid) {  // dQ^T[channel = c * 32 + kappa(r, h)][query = ql]
    float* op = grad_q + qrow * CB;
#pragma unroll
    for (int c = 0; c < CB / 32; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(op + c * 32 + 8 * g + 4 * h) = make_float4(
            dQ[c][4 * g] * gscale, dQ[c][4 * g + 1] * gscale, dQ[c][4 * g + 2] * gscale, dQ[c][4 * g + 3] * gscale);
  }
}

template <int CB, int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void nl_grad_key_kernel(int p, int n, float qscale, float gscale,
                                                                const float* __restrict__ q, const float* __restrict__ kv,
                                                                const float* __restrict__ gout, const float* __restrict__ lse2,
                                                                const float* __restrict__ delta, float* __restrict__ grad_kv) {
  constexpr int HC = CB / 2;
  constexpr bool KV_LDS = CB == 128;  // the workgroup's K and V tiles in LDS instead of 2 * HC registers per lane
  constexpr int KS = CB + 1;          // padded row stride: lane ql reads bank ql + const
  constexpr int TILE_FLOATS = KV_LDS ? 2 * NLG_B * KS : 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ks = reinterpret_cast<float*>(smem);  // [32][KS]
  float* Vs = Ks + NLG_B * KS;                 // [32][KS]
  float* park = reinterpret_cast<float*>(smem) + TILE_FLOATS;  // [SPLIT - 1][HC][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;
  const int bi = blockIdx.y, k0 = blockIdx.x * NLG_B;
  const bool kvalid = k0 + ql < n;
  const size_t krow = (size_t)bi * n + min(k0 + ql, n - 1);
  const float* qb = q + (size_t)bi * p * CB;
  const float* gb = gout + (size_t)bi * p * CB;
  const float* lb = lse2 + (size_t)bi * p;
  const float* db = delta + (size_t)bi * p;

  // K and V as B operands: B[k = h][j = ql] = X[key][h * HC + t]
  float kreg[KV_LDS ? 1 : HC], vreg[KV_LDS ? 1 : HC];
  if constexpr (KV_LDS) {
    const int cnt = min(NLG_B, n - k0);
    for (int f = tid; f < NLG_B * (2 * CB / 4); f += SPLIT * 64) {
      const int row = f / (2 * CB / 4), c4 = (f - row * (2 * CB / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < cnt) v = *reinterpret_cast<const float4*>(kv + ((size_t)bi * n + k0 + row) * 2 * CB + c4);
      float* d = c4 < CB ? Ks + row * KS + c4 : Vs + row * KS + (c4 - CB);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
  } else {
    nlg_load_row<HC>(kv + krow * 2 * CB + HC * h, kvalid, 1.f, kreg);
    nlg_load_row<HC>(kv + krow * 2 * CB + CB + HC * h, kvalid, 1.f, vreg);
  }
  const float* ksrow = Ks + ql * KS + HC * h;
  const float* vsrow = Vs + ql * KS + HC * h;

  f32x16 dK[CB / 32], dV[CB / 32];
#pragma unroll
  for (int c = 0; c < CB / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dK[c][r] = 0.f; dV[c][r] = 0.f; }

  for (int base = wave * NLG_B; base < p; base += SPLIT * NLG_B) {
    const int cnt = min(NLG_B, p - base);
    f32x16 S, dP;  // lane (key ql, h): queries kappa(r, h); -lse2 is the score chain's initial accumulator
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = -lb[base + min(kappa(r, h), cnt - 1)];
      dP[r] = 0.f;
    }
    {
      float qa[HC];  // A[i = query ql][k = h] = Q[query][h * HC + t] * log2e / sqrt(cb)
      nlg_load_row<HC>(qb + (size_t)(base + min(ql, cnt - 1)) * CB + HC * h, ql < cnt, qscale, qa);
#pragma unroll
      for (int t = 0; t < HC; ++t)
        S = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[t], KV_LDS ? ksrow[t] : kreg[KV_LDS ? 0 : t], S, 0, 0, 0);
    }
    {
      float ga[HC];
      nlg_load_row<HC>(gb + (size_t)(base + min(ql, cnt - 1)) * CB + HC * h, ql < cnt, 1.f, ga);
#pragma unroll
      for (int t = 0; t < HC; ++t)
        dP = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[t], KV_LDS ? vsrow[t] : vreg[KV_LDS ? 0 : t], dP, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool valid = kvalid && kappa(r, h) < cnt;
      const float pr = fast_exp2(S[r]);
      S[r] = valid ? pr : 0.f;
      dP[r] = valid ? pr * (dP[r] - db[base + min(kappa(r, h), cnt - 1)]) : 0.f;
    }
    // dV^T += g_blk^T . P and dK^T += Q_blk^T . dS: A[i = channel c * 32 + ql][k = query kappa(t, h)], coalesced row reads
#pragma unroll
    for (int c = 0; c < CB / 32; ++c) {
      float a[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float v = gb[(size_t)(base + min(kappa(t, h), cnt - 1)) * CB + c * 32 + ql];
        a[t] = kappa(t, h) < cnt ? v : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) dV[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], S[t], dV[c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const float v = qb[(size_t)(base + min(kappa(t, h), cnt - 1)) * CB + c * 32 + ql];
        a[t] = kappa(t, h) < cnt ? v : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 16; ++t) dK[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], dP[t], dK[c], 0, 0, 0);
    }
  }

  if constexpr (SPLIT > 1) {
    // two rounds through one park region (dK, then dV), each folded by wave 0 in ascending wave order
    float* pw = park + (size_t)(wave > 0 ? wave - 1 : 0) * HC * 64;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      if (round == 1) __syncthreads();  // wave 0 has read round 0's parks
      if (wave > 0) {
#pragma unroll
        for (int c = 0; c < CB / 32; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) pw[(c * 16 + r) * 64 + lane] = round == 0 ? dK[c][r] : dV[c][r];
      }
      __syncthreads();
      if (wave == 0) {
        for (int w = 1; w < SPLIT; ++w) {  // (a wave that saw no query block parked zeros)
          const float* src = park + (size_t)(w - 1) * HC * 64;
#pragma unroll
          for (int c = 0; c < CB / 32; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              if (round == 0) dK[c][r] += src[(c * 16 + r) * 64 + lane];
              else dV[c][r] += src[(c * 16 + r) * 64 + lane];
            }
        }
      }
    }
    if (wave > 0) return;
  }
  if (kvalid) {  // [dK | dV]^T[channel = c * 32 + kappa(r, h)][key = ql]
    float* op = grad_kv + krow * 2 * CB;
#pragma unroll
    for (int c = 0; c < CB / 32; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(op + c * 32 + 8 * g + 4 * h) = make_float4(
            dK[c][4 * g] * gscale, dK[c][4 * g + 1] * gscale, dK[c][4 * g + 2] * gscale, dK[c][4 * g + 3] * gscale);
        *reinterpret_cast<float4*>(op + CB + c * 32 + 8 * g + 4 * h) =
            make_float4(dV[c][4 * g], dV[c][4 * g + 1], dV[c][4 * g + 2], dV[c][4 * g + 3]);
      }
  }
}

// waves per workgroup, as the forward chooses them: enough to fill the chip (~4 per SIMD), at least 4 blocks per wave
static int nlg_split(long tiles, long blocks, int cap) {
  int want = 1;
  while (want < cap && tiles * want < 4096 && want * 2 * 4 <= blocks) want *= 2;
  return want;
}
// cb = 128: four waves (one per SIMD) have the whole register file; the key-major kernel keeps two accumulator sets, so
// cb = 64 stays at four waves there too
template <int CB> constexpr int NLG_QUERY_CAP = CB == 128 ? 4 : 8;
template <int CB> constexpr int NLG_KEY_CAP = CB == 32 ? 8 : 4;

template <int CB, int SPLIT>
static int nlg_query_launch(int b, int p, int n, float qscale, float gscale, const float* q, const float* kv, const float* out,
                            const float* gout, float* grad_q, float* lse2, float* delta, hipStream_t st) {
  const size_t lds = SPLIT > 1 ? ((size_t)SPLIT * 2 * 64 + (size_t)(SPLIT - 1) * (CB / 2) * 64) * sizeof(float) : 0;  // stats + parks
  return launch(nl_grad_query_kernel<CB, SPLIT>, dim3((p + NLG_B - 1) / NLG_B, b), dim3(SPLIT * 64), lds, st, p, n, qscale, gscale, q,
                kv, out, gout, grad_q, lse2, delta);
}
template <int CB, int SPLIT>
static int nlg_key_launch(int b, int p, int n, float qscale, float gscale, const float* q, const float* kv, const float* gout,
                          const float* lse2, const float* delta, float* grad_kv, hipStream_t st) {
  const size_t lds = ((CB == 128 ? (size_t)2 * NLG_B * (CB + 1) : 0) + (size_t)(SPLIT - 1) * (CB / 2) * 64) * sizeof(float);
  return launch(nl_grad_key_kernel<CB, SPLIT>, dim3((n + NLG_B - 1) / NLG_B, b), dim3(SPLIT * 64), lds, st, p, n, qscale, gscale, q,
                kv, gout, lse2, delta, grad_kv);
}

template <int CB>
static int nlg_dispatch(int b, int p, int n, const float* q, const float* kv, const float* out, const float* gout, float* grad_q,
                        float* grad_kv, float* lse2, float* delta, hipStream_t st) {
  const float qscale = LOG2E / sqrtf((float)CB), gscale = 1.0f / sqrtf((float)CB);
  const long qtiles = (long)b * ((p + NLG_B - 1) / NLG_B), qblocks = (p + NLG_B - 1) / NLG_B;
  const long ktiles = (long)b * ((n + NLG_B - 1) / NLG_B), kblocks = (n + NLG_B - 1) / NLG_B;
  auto query = [&](auto split) {
    return nlg_query_launch<CB, decltype(split)::value>(b, p, n, qscale, gscale, q, kv, out, gout, grad_q, lse2, delta, st);
  };
  auto key = [&](auto split) {
    return nlg_key_launch<CB, decltype(split)::value>(b, p, n, qscale, gscale, q, kv, gout, lse2, delta, grad_kv, st);
  };
  const int sq = nlg_split(qtiles, kblocks, NLG_QUERY_CAP<CB>);
  int rc = with_split<1, NLG_QUERY_CAP<CB>>(sq, query);
  if (rc != PASNL_OK) return rc;
  if (grad_kv != nullptr) {
    const int sk = nlg_split(ktiles, qblocks, NLG_KEY_CAP<CB>);
    rc = with_split<1, NLG_KEY_CAP<CB>>(sk, key);
    if (rc != PASNL_OK) return rc;
  }
  return pasnl_launch_status();
}

}  // namespace pasnl

using namespace pasnl;

extern "C" size_t pasnl_cls_nl_attention_grad_workspace_bytes(int b, int p, int n, int cb) {
  if (b <= 0 || p <= 0 || n <= 0 || !(cb == 32 || cb == 64 || cb == 128)) return 0;
  return (size_t)2 * sizeof(float) * (size_t)b * (size_t)p;  // lse2[b,p], delta[b,p]
}

extern "C" int pasnl_cls_nl_attention_grad(int b, int p, int n, int cb, const float* q, const float* kv, const float* out,
                                           const float* grad_out, float* grad_q, float* grad_kv, void* workspace,
                                           size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && p >= 0 && n > 0 && cb > 0, PASNL_EINVAL);
  PASNL_REQUIRE(cb == 32 || cb == 64 || cb == 128, PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  if (p == 0) {  // no query: the keys and values receive no gradient
    if (grad_kv == nullptr) return PASNL_OK;
    PASNL_REQUIRE(hipMemsetAsync(grad_kv, 0, (size_t)b * n * 2 * cb * sizeof(float), pasnl_hip_stream(stream)) == hipSuccess,
                  PASNL_ELAUNCH);
    return PASNL_OK;
  }
  PASNL_REQUIRE(q && kv && out && grad_out && (grad_q || grad_kv) && workspace, PASNL_ENULL);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out) |
                  reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_q) |
                  reinterpret_cast<uintptr_t>(grad_kv) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(workspace_bytes >= pasnl_cls_nl_attention_grad_workspace_bytes(b, p, n, cb), PASNL_EWORKSPACE);
  hipStream_t st = pasnl_hip_stream(stream);
  float* lse2 = static_cast<float*>(workspace);
  float* delta = lse2 + (size_t)b * p;
  if (cb == 32) return nlg_dispatch<32>(b, p, n, q, kv, out, grad_out, grad_q, grad_kv, lse2, delta, st);
  if (cb == 64) return nlg_dispatch<64>(b, p, n, q, kv, out, grad_out, grad_q, grad_kv, lse2, delta, st);
  return nlg_dispatch<128>(b, p, n, q, kv, out, grad_out, grad_q, grad_kv, lse2, delta, st);
}
