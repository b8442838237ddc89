// Backward of the AdaptiveSampling cell's three parts that are not GEMMs (as_cell.hip: as_attention_kernel, as_reweight_kernel,
// as_gather_*_kernel) for gfx950: pasnl_cls_as_attention_grad / _qkv_grad, pasnl_cls_as_reweight_grad / _x_grad and
// pasnl_cls_as_gather_grad.  DESIGN.md 4.4 has the formulas and the resource figures.
//
// Micro attention.  Per group of as <= 16 neighbours, s_ij = q_i . k_j / sqrt(cb), P = softmax_j(s), g = dL/dO:
//     dV = P^T g      dP = g V^T      delta_i = sum_j P_ij dP_ij      dS = P o (dP - delta)
//     dQ = dS K / sqrt(cb)            dK = dS^T Q / sqrt(cb)
// One wave per group on v_mfma_f32_16x16x4_f32, `as` padded to the 16 x 16 tile, in the forward's two tile forms.  A product
// whose B operand is a D tile contracts the tile's ROW index, so the tile is formed once per orientation (a score chain is
// cb / 4 MFMAs -- cheaper than a transpose through LDS):
//   * key-major   S^T[key = 4 grp + r][query = col] = K . Q^T,  dP^T = V . g^T:   dQ^T[ch][query] += K^T . dS^T
//   * query-major S  [query = 4 grp + r][key = col] = Q . K^T,  dP   = g . V^T:   dV^T[ch][key] += g^T . P,  dK^T[ch][key] += Q^T . dS
// P is recomputed from Q and K: nothing of the forward is saved, there is no workspace.  No sum crosses a group: no atomics.
// delta is the sum of P_ij dP_ij over the SAME tile dS is formed from, not g . O rounded on its own: with as == 1 (P == 1) it
// is dP itself, bit for bit, so dS, grad_q and dK are exact zeros (DESIGN.md 4.2 on the residue a separate delta leaves).
// Rows and channels past the ragged ends are zero-filled operands and the probability / dS of a masked key or query is SELECTED
// to 0, never multiplied: nothing stale reaches an accumulator.
//
// Re-weighting tail.  w[s,o] = softmax_s(logits[s,o]); t_s = gxyz . X[s] (o = 0), gfeat[o-1] F[s,o-1] (o >= 1):
//     dlogits[s,o] = w[s,o] (t_s - sum_r w[r,o] t_r)      dX[s,d] = w[s,0] gxyz[d]      dF[s,j] = w[s,1+j] gfeat[j]
// One thread per (group, column), as the forward; sums over the neighbours in ascending s.
//
// Gather.  The forward rows are [xyz[i_s] - xyz[i_0] | xyz[i_s] | feature[i_s]]: grad_x is folded to one row per gathered
// point, r[j,s] = [gx[0:3] + gx[3:6] - (s == 0 ? sum_t gx[j,t,0:3] : 0) | gx[6:]], and r is scattered by the ordered segmented
// sums of grouping.hip (pasnl_group_point_grad_det): no second scatter, no fp atomics.
#include <math.h>
#include "as_core.hpp"

namespace pasnl {

// qs / kvs = row strides of q and kv in floats, gqs / gkvs those of grad_q and grad_kv (cb and 2cb for separate tensors; 3cb
// for one [K | V | Q] tensor and its gradient); gout rows are cb floats
__global__ __launch_bounds__(256) void as_attention_grad_kernel(long groups, int as, int cb, float qscale, float gscale, int qs,
                                                               int kvs, int gqs, int gkvs, const float* __restrict__ q,
                                                               const float* __restrict__ kv, const float* __restrict__ gout,
                                                               float* __restrict__ grad_q, float* __restrict__ grad_kv) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;  // (the whole wave)
  const int col = lane & 15, grp = lane >> 4;
  const float* qg = q + (size_t)g * as * qs;
  const float* kg = kv + (size_t)g * as * kvs;
  const float* vg = kg + cb;  // V = second half of each kv row
  const float* gg = gout + (size_t)g * as * cb;
  const bool rowok = col < as;  // this lane's row as an A / B operand of a score chain, and its column of the D tile

  if (grad_q != nullptr) {
    // ---- key-major: S^T[key = 4 grp + r][query = col], dP^T likewise; dQ^T[ch][query] += K^T . dS^T
    f32x4 S = {0.f, 0.f, 0.f, 0.f}, dP = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cb; c0 += 4) {
      const int c = c0 + grp;
      const bool okc = rowok && c < cb;
      const float kk = okc ? kg[(size_t)col * kvs + c] : 0.f;
      const float qq = okc ? qg[(size_t)col * qs + c] * qscale : 0.f;
      const float vv = okc ? vg[(size_t)col * kvs + c] : 0.f;
      const float go = okc ? gg[(size_t)col * cb + c] : 0.f;
      S = __builtin_amdgcn_mfma_f32_16x16x4f32(kk, qq, S, 0, 0, 0);
      dP = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, go, dP, 0, 0, 0);
    }
    const float inv = as_softmax_keys(S, as, grp);
    float delta = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      S[r] = (4 * grp + r) < as ? S[r] * inv : 0.f;
      delta += S[r] * dP[r];
    }
    delta += __shfl_xor(delta, 16);
    delta += __shfl_xor(delta, 32);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ds = S[r] * (dP[r] - delta);
      S[r] = (rowok && (4 * grp + r) < as) ? ds : 0.f;
    }
    for (int c0 = 0; c0 < cb; c0 += 16) {
      f32x4 O = {0.f, 0.f, 0.f, 0.f};
      const int ch = c0 + col;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int key = 4 * grp + t;
        const float a = (key < as && ch < cb) ? kg[(size_t)key * kvs + ch] : 0.f;
        O = __builtin_amdgcn_mfma_f32_16x16x4f32(a, S[t], O, 0, 0, 0);
      }
      if (rowok) {  // dQ^T[ch = c0 + 4 grp + r][query = col]
        float* op = grad_q + ((size_t)g * as + col) * gqs + c0 + 4 * grp;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c0 + 4 * grp + r < cb) op[r] = O[r] * gscale;
      }
    }
  }

  if (grad_kv != nullptr) {
    // ---- query-major: S[query = 4 grp + r][key = col], dP likewise; dV^T[ch][key] += g^T . P, dK^T[ch][key] += Q^T . dS
    f32x4 S = {0.f, 0.f, 0.f, 0.f}, dP = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < cb; c0 += 4) {
      const int c = c0 + grp;
      const bool okc = rowok && c < cb;
      const float qq = okc ? qg[(size_t)col * qs + c] * qscale : 0.f;
      const float kk = okc ? kg[(size_t)col * kvs + c] : 0.f;
      const float go = okc ? gg[(size_t)col * cb + c] : 0.f;
      const float vv = okc ? vg[(size_t)col * kvs + c] : 0.f;
      S = __builtin_amdgcn_mfma_f32_16x16x4f32(qq, kk, S, 0, 0, 0);
      dP = __builtin_amdgcn_mfma_f32_16x16x4f32(go, vv, dP, 0, 0, 0);
    }
    f32x4 P, dS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = rowok ? S[r] : -INFINITY;
      const float m = row16_max(s);  // finite: key 0 exists
      const float e = fast_exp2(s - m);  // 0 for a masked key
      const float esum = row16_sum(e);   // (every lane takes part in the exchanges: nothing of them inside a branch)
      const float pr = e * (1.0f / esum);
      const float dl = row16_sum(pr * dP[r]);
      const bool valid = rowok && (4 * grp + r) < as;
      P[r] = valid ? pr : 0.f;
      dS[r] = valid ? pr * (dP[r] - dl) : 0.f;
    }
    for (int c0 = 0; c0 < cb; c0 += 16) {
      f32x4 dV = {0.f, 0.f, 0.f, 0.f}, dK = {0.f, 0.f, 0.f, 0.f};
      const int ch = c0 + col;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int qi = 4 * grp + t;
        const bool ok = qi < as && ch < cb;
        const float ga = ok ? gg[(size_t)qi * cb + ch] : 0.f;
        const float qa = ok ? qg[(size_t)qi * qs + ch] : 0.f;
        dV = __builtin_amdgcn_mfma_f32_16x16x4f32(ga, P[t], dV, 0, 0, 0);
        dK = __builtin_amdgcn_mfma_f32_16x16x4f32(qa, dS[t], dK, 0, 0, 0);
      }
      if (rowok) {  // [dK | dV]^T[ch = c0 + 4 grp + r][key = col]
        float* op = grad_kv + ((size_t)g * as + col) * gkvs + c0 + 4 * grp;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c0 + 4 * grp + r < cb) {
            op[r] = dK[r] * gscale;
            op[cb + r] = dV[r];
          }
      }
    }
  }
}

// One thread per (group, column o) of the (1+ch)-wide logits, as as_reweight_kernel.  xs / fs = row strides of the coordinates
// and features the forward read, gxs / gfs those of their gradients.
// XFORM: coordinates and features are both columns 3.. of x (g,as,3+ch) and grad_f points at column 3 of grad_x: column 3+j
// receives dF[s,j], plus dX[s,j] for j < 3; columns 0-2 are zeros.  Otherwise rows as..nsample-1 of both gradients are zeros.
template <bool XFORM>
__global__ __launch_bounds__(256) void as_reweight_grad_kernel(long groups, int as, int nsample, int ch, int xs, int fs, int gxs,
                                                              int gfs, const float* __restrict__ logits,
                                                              const float* __restrict__ gxyz, const float* __restrict__ gfeat,
                                                              const float* __restrict__ gnx, const float* __restrict__ gnf,
                                                              float* __restrict__ grad_logits, float* __restrict__ grad_x,
                                                              float* __restrict__ grad_f) {
  const int w = 1 + ch;
  const long total = groups * w;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long g = e / w;
    const int o = (int)(e - g * w);
    const float* lg = logits + (size_t)g * as * w;
    // softmax over the neighbours of column `column`: the forward's, normalised as it normalises
    auto softmax_column = [&](int column, float (&v)[AS_MAX]) {
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k) v[k] = k < as ? lg[(size_t)k * w + column] : -INFINITY;
      const float sum = as_softmax_column(as, v);
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k) v[k] = v[k] / sum;
    };
    float v[AS_MAX];
    softmax_column(o, v);
    const float gx0 = gnx[g * 3], gx1 = gnx[g * 3 + 1], gx2 = gnx[g * 3 + 2];
    const float gf = o > 0 ? gnf[(size_t)g * ch + (o - 1)] : 0.f;
    if (grad_logits != nullptr) {
      float t[AS_MAX];
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k) {
        t[k] = 0.f;
        if (k < as) {
          if (o == 0) {
            const float* xp = gxyz + ((size_t)g * nsample + k) * xs;
            t[k] = (gx0 * xp[0] + gx1 * xp[1]) + gx2 * xp[2];
          } else {
            t[k] = gf * gfeat[((size_t)g * nsample + k) * fs + (o - 1)];
          }
          dot += v[k] * t[k];
        }
      }
#pragma unroll
      for (int k = 0; k < AS_MAX; ++k)
        if (k < as) grad_logits[((size_t)g * as + k) * w + o] = v[k] * (t[k] - dot);
    }
    if constexpr (XFORM) {
      if (grad_f == nullptr) continue;
      if (o == 0) {
        for (int k = 0; k < as; ++k) {
          float* p = grad_x + ((size_t)g * as + k) * gxs;
          p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        }
      } else if (o <= 3) {  // the columns that serve as coordinates too: dF + dX
        float v0[AS_MAX];
        softmax_column(0, v0);
        const float gxd = o == 1 ? gx0 : o == 2 ? gx1 : gx2;
#pragma unroll
        for (int k = 0; k < AS_MAX; ++k)
          if (k < as) grad_f[((size_t)g * as + k) * gfs + (o - 1)] = v[k] * gf + v0[k] * gxd;
      } else {
#pragma unroll
        for (int k = 0; k < AS_MAX; ++k)
          if (k < as) grad_f[((size_t)g * as + k) * gfs + (o - 1)] = v[k] * gf;
      }
    } else {
      if (o == 0) {
        if (grad_x != nullptr) {
#pragma unroll
          for (int k = 0; k < AS_MAX; ++k)
            if (k < as) {
              float* p = grad_x + ((size_t)g * nsample + k) * gxs;
              p[0] = v[k] * gx0; p[1] = v[k] * gx1; p[2] = v[k] * gx2;
            }
          for (int k = as; k < nsample; ++k) {
            float* p = grad_x + ((size_t)g * nsample + k) * gxs;
            p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
          }
        }
      } else if (grad_f != nullptr) {
#pragma unroll
        for (int k = 0; k < AS_MAX; ++k)
          if (k < as) grad_f[((size_t)g * nsample + k) * gfs + (o - 1)] = v[k] * gf;
        for (int k = as; k < nsample; ++k) grad_f[((size_t)g * nsample + k) * gfs + (o - 1)] = 0.f;
      }
    }
  }
}

// grad_x (rows, 6+c), rows = (b, j, s): r_xyz (rows,3), r_feat (rows,c) and the first `as` columns of idx as (rows)
__global__ __launch_bounds__(256) void as_gather_fold_kernel(int c, int k, int as, long total, const float* __restrict__ gx,
                                                            const int* __restrict__ idx, float* __restrict__ r_xyz,
                                                            float* __restrict__ r_feat, int* __restrict__ idx_as) {
  const int w = 3 + c, wx = 6 + c;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / w;
    const int col = (int)(e - row * w);
    const float* src = gx + (size_t)row * wx;
    if (col >= 3) {
      if (r_feat != nullptr) r_feat[(size_t)row * c + (col - 3)] = src[3 + col];
      continue;
    }
    const long gj = row / as;
    const int s = (int)(row - gj * as);
    if (col == 0) idx_as[row] = idx[gj * k + s];
    if (r_xyz == nullptr) continue;
    float v = src[col] + src[3 + col];
    if (s == 0) {  // neighbour 0 is subtracted from every row of its group
      float sum = 0.f;
      for (int t = 0; t < as; ++t) sum += src[(size_t)t * wx + col];
      v -= sum;
    }
    r_xyz[(size_t)row * 3 + col] = v;
  }
}

static int as_attention_grad_launch(int g, int as, int cb, int qs, int kvs, int gqs, int gkvs, const float* q, const float* kv,
                                    const float* gout, float* grad_q, float* grad_kv, hipStream_t st) {
  hipLaunchKernelGGL(as_attention_grad_kernel, dim3((unsigned)(((long)g + 3) / 4)), dim3(256), 0, st, (long)g, as, cb, as_qscale(cb),
                     1.0f / sqrtf((float)cb), qs, kvs, gqs, gkvs, q, kv, gout, grad_q, grad_kv);
  return pasnl_launch_status();
}

}  // namespace pasnl

using namespace pasnl;

extern "C" int pasnl_cls_as_attention_grad(int g, int as, int cb, const float* q, const float* kv, const float* grad_out,
                                           float* grad_q, float* grad_kv, pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX && cb <= 256, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(q && kv && grad_out && (grad_q || grad_kv), PASNL_ENULL);
  return as_attention_grad_launch(g, as, cb, cb, 2 * cb, cb, 2 * cb, q, kv, grad_out, grad_q, grad_kv, pasnl_hip_stream(stream));
}

extern "C" int pasnl_cls_as_attention_qkv_grad(int g, int as, int cb, const float* kvq, const float* grad_out, float* grad_kvq,
                                               pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && cb > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX && cb <= 256, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(kvq && grad_out && grad_kvq, PASNL_ENULL);
  return as_attention_grad_launch(g, as, cb, 3 * cb, 3 * cb, 3 * cb, 3 * cb, kvq + 2 * cb, kvq, grad_out, grad_kvq + 2 * cb, grad_kvq,
                                  pasnl_hip_stream(stream));
}

extern "C" int pasnl_cls_as_reweight_grad(int g, int as, int nsample, int ch, const float* logits, const float* grouped_xyz,
                                          const float* grouped_feature, const float* grad_new_xyz, const float* grad_new_feature,
                                          float* grad_logits, float* grad_grouped_xyz, float* grad_grouped_feature,
                                          pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && nsample >= as && ch > 0, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && grad_new_xyz && grad_new_feature && (grad_logits || grad_grouped_xyz || grad_grouped_feature),
                PASNL_ENULL);
  PASNL_REQUIRE(grad_logits == nullptr || (grouped_xyz && grouped_feature), PASNL_ENULL);
  hipLaunchKernelGGL(as_reweight_grad_kernel<false>, dim3(as_grid((long)g * (1 + ch))), dim3(256), 0, pasnl_hip_stream(stream),
                     (long)g, as, nsample, ch, 3, ch, 3, ch, logits, grouped_xyz, grouped_feature, grad_new_xyz, grad_new_feature,
                     grad_logits, grad_grouped_xyz, grad_grouped_feature);
  return pasnl_launch_status();
}

extern "C" int pasnl_cls_as_reweight_x_grad(int g, int as, int ch, const float* logits, const float* x, const float* grad_new_xyz,
                                            const float* grad_new_feature, float* grad_logits, float* grad_x,
                                            pasnl_stream_t stream) {
  PASNL_REQUIRE(g >= 0 && as > 0 && ch > 3, PASNL_EINVAL);
  PASNL_REQUIRE(as <= AS_MAX, PASNL_EUNSUPPORTED);
  if (g == 0) return PASNL_OK;
  PASNL_REQUIRE(logits && grad_new_xyz && grad_new_feature && (grad_logits || grad_x), PASNL_ENULL);
  PASNL_REQUIRE(grad_logits == nullptr || x, PASNL_ENULL);
  // x rows = [xyz - xyz0 | xyz | feature] (3 + ch floats): coordinates and the (xyz | feature) rows both start at column 3
  const int w = 3 + ch;
  hipLaunchKernelGGL(as_reweight_grad_kernel<true>, dim3(as_grid((long)g * (1 + ch))), dim3(256), 0, pasnl_hip_stream(stream),
                     (long)g, as, as, ch, w, w, w, w, logits, x ? x + 3 : nullptr, x ? x + 3 : nullptr, grad_new_xyz, grad_new_feature,
                     grad_logits, grad_x, grad_x ? grad_x + 3 : nullptr);
  return pasnl_launch_status();
}

// [lists of the ordered scatter | idx_as (rows) | r_xyz (rows,3) | r_feat (rows,c)], rows = b m as
extern "C" size_t pasnl_cls_as_gather_grad_workspace_bytes(int b, int n, int c, int m, int as) {
  if (b <= 0 || n <= 0 || c <= 0 || m < 0 || as <= 0) return 0;
  const size_t rows = (size_t)b * m * as;
  return pasnl_grad_workspace_bytes(b, n, (long)m * as) + rows * (size_t)(1 + 3 + c) * sizeof(float);
}

extern "C" int pasnl_cls_as_gather_grad(int b, int n, int c, int m, int k, int as, const float* grad_x, const int* idx,
                                        float* grad_xyz, float* grad_feature, void* workspace, size_t workspace_bytes,
                                        pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && c > 0 && m >= 0 && k > 0 && as > 0 && as <= k, PASNL_EINVAL);
  PASNL_REQUIRE(n <= 38400 && (long)m * as < (1L << 31), PASNL_EUNSUPPORTED);
  if (b == 0) return PASNL_OK;
  const long rows = (long)b * m * as;
  PASNL_REQUIRE((grad_xyz || grad_feature) && (rows == 0 || (grad_x && idx)), PASNL_ENULL);
  PASNL_REQUIRE(workspace && workspace_bytes >= pasnl_cls_as_gather_grad_workspace_bytes(b, n, c, m, as), PASNL_EWORKSPACE);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, PASNL_EUNSUPPORTED);
  const size_t lists_bytes = pasnl_grad_workspace_bytes(b, n, (long)m * as);
  int* idx_as = reinterpret_cast<int*>(static_cast<char*>(workspace) + lists_bytes);
  float* r_xyz = reinterpret_cast<float*>(idx_as + rows);
  float* r_feat = r_xyz + (size_t)rows * 3;
  if (rows > 0) {
    hipLaunchKernelGGL(as_gather_fold_kernel, dim3(as_grid(rows * (3 + c))), dim3(256), 0, pasnl_hip_stream(stream), c, k, as,
                       rows * (3 + c), grad_x, idx, grad_xyz ? r_xyz : nullptr, grad_feature ? r_feat : nullptr, idx_as);
    PASNL_REQUIRE(pasnl_launch_status() == PASNL_OK, PASNL_ELAUNCH);
  }
  // the two scatters share the lists' region: they run one after the other on the stream
  if (grad_xyz != nullptr) {
    const int rc = pasnl_group_point_grad_det(b, n, 3, m, as, r_xyz, idx_as, grad_xyz, workspace, lists_bytes, stream);
    if (rc != PASNL_OK) return rc;
  }
  if (grad_feature != nullptr) {
    const int rc = pasnl_group_point_grad_det(b, n, c, m, as, r_feat, idx_as, grad_feature, workspace, lists_bytes, stream);
    if (rc != PASNL_OK) return rc;
  }
  return PASNL_OK;
}
