// Point-NonLocal cell on NARROW features, attended in input space (pasnl_cls_nl_cell_input; include/pasnl.h has the contract).
//
// conv_kv and conv_query have no activation, so K = X Wk + bk and V = X Wv + bv are linear images of the C-channel input rows
// and the cb-wide contractions of softmax(Q K^T / sqrt(cb)) V have rank C:
//   u   = Wk Q                      a C-vector per query (Q . bk is the same for every key and cancels in the softmax)
//   w_j = softmax_j(u . X_j / sqrt(cb))
//   ctr = sum_j w_j X_j             a softmax-weighted centroid of the input rows
//   out = ctr Wv + bv               (sum_j w_j = 1)
// Per (query, key) pair that is C FMAs for the score, the online softmax and C FMAs for the centroid: no matrix instruction,
// no (B,N,2cb) / (B,P,cb) intermediates.
//
// One lane owns one query: u, the running maximum m, the running sum l and the C-vector accumulator stay in registers.  A
// workgroup is 64 queries x SPLIT waves; wave w walks the w-th contiguous range of the cloud's keys.  Key rows are the same
// for every lane: a wave copies its range into its own LDS region CHUNK rows at a time (the next chunk's global loads are in
// flight while the current one is consumed; no workgroup barrier in the loop) and reads the rows back as broadcasts, so a key
// costs the vector pipe nothing but the arithmetic.  Scores of a block of KB keys are formed first, then one block maximum,
// one rescale of (l, acc) and one exp2 per pair (scores live in the log2 domain: log2e / sqrt(cb) is folded into u).  The
// waves' partial (m, l, acc) meet in LDS and are folded in ascending wave order; a wave that saw no key carries m = -inf,
// l = 0.  Every sum has a fixed order: the result is a pure function of the inputs.
// The projection, the staged stream, the block step, the key ranges, the wave fold and the split rule are nl_input_core.hpp's,
// which the backward (nl_input_grad.hip) uses too.
#include <math.h>
#include "nl_input_core.hpp"

namespace pasnl {

constexpr int NLI_KB = 16;      // keys per softmax block
constexpr int NLI_CHUNK = 256;  // keys a wave stages at a time

// CT: channels the kernel carries (CT == 3: c == 3 exactly; otherwise any c <= CT, the channels beyond c are zeros)
template <int CT, int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void nl_input_kernel(int p, int n, int c, int cz, int cb, float scale,
                                                              const float* __restrict__ feature,
                                                              const float* __restrict__ new_point,
                                                              const float* __restrict__ wkv, const float* __restrict__ bkv,
                                                              const float* __restrict__ wq, const float* __restrict__ bq,
                                                              float* __restrict__ out) {
  constexpr int RW = CT <= 4 ? 4 : 8;          // floats of a staged row
  constexpr int WAVE_ROWS = NLI_CHUNK * RW;    // floats of a wave's staging region
  constexpr int PARK = (CT + 2) * 64;          // floats a wave parks: CT vectors, m, l
  extern __shared__ __align__(16) float nli_smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* rows = nli_smem + wave * WAVE_ROWS;
  float* park = nli_smem + SPLIT * WAVE_ROWS;  // [SPLIT][CT + 2][64]
  const int bi = blockIdx.y, q0 = blockIdx.x * 64;
  const int qi = min(q0 + lane, p - 1);
  const float* zrow = new_point + ((size_t)bi * p + qi) * cz;
  const float* f = feature + (size_t)bi * n * c;

  float u[CT];
  nli_project<CT, SPLIT, PARK, false>(c, cz, cb, scale, zrow, nullptr, wkv, wq, bq, park, wave, lane, u, nullptr);

  // ---- this wave's keys, then the waves' partial results folded by wave 0 and the centroid back through Wv
  int k0, k1;
  nli_key_range<NLI_KB>(wave, n, SPLIT, k0, k1);
  float m = -INFINITY, l = 0.f, acc[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) acc[ch] = 0.f;
  nli_stream<RW, NLI_CHUNK>(
      k0, k1, rows, lane, [&](int key, float (&v)[RW]) { nli_load_key<CT, RW>(f, key, k1, c, v); },
      [&](const float* rp, int cnt) { nli_blocks<NLI_KB, CT, RW>(rp, cnt, u, m, l, acc); });
  nli_fold<CT, SPLIT, PARK, false>(park, wave, lane, m, l, acc);
  if (wave == 0) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) park[ch * 64 + lane] = acc[ch] * inv;
  }
  __syncthreads();
  float ctr[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) ctr[ch] = park[ch * 64 + lane];
  if (q0 + lane < p) {
    float* op = out + ((size_t)bi * p + q0 + lane) * cb;
    for (int kg = wave * 4; kg < cb; kg += SPLIT * 4) {
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = bkv[cb + kg + j];
#pragma unroll
      for (int ch = 0; ch < CT; ++ch)
        if (CT == 3 || ch < c) {
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = fmaf(ctr[ch], wkv[ch * 2 * cb + cb + kg + j], o[j]);
        }
      *reinterpret_cast<float4*>(op + kg) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int CT, int SPLIT>
static int nl_input_launch(int b, int p, int n, int c, int cz, int cb, float scale, const float* feature, const float* new_point,
                    const float* wkv, const float* bkv, const float* wq, const float* bq, float* out, hipStream_t st) {
  const size_t lds = (size_t)SPLIT * (NLI_CHUNK * (CT <= 4 ? 4 : 8) + (CT + 2) * 64) * sizeof(float);
  if (launch(nl_input_kernel<CT, SPLIT>, dim3((p + 63) / 64, b), dim3(SPLIT * 64), lds, st, p, n, c, cz, cb, scale, feature,
             new_point, wkv, bkv, wq, bq, out) != PASNL_OK)
    return PASNL_ELAUNCH;
  return pasnl_launch_status();
}

template <int CT>
static int nl_input_dispatch(int b, int p, int n, int c, int cz, int cb, float scale, const float* feature, const float* new_point,
                      const float* wkv, const float* bkv, const float* wq, const float* bq, float* out, hipStream_t st) {
  return nli_with_split<CT>(nli_split(b, p, n), [&](auto s) {
    return nl_input_launch<CT, decltype(s)::value>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
  });
}

}  // namespace pasnl

extern "C" int pasnl_cls_nl_cell_input(int b, int p, int n, int c, int cz, int cb, const float* feature, const float* new_point,
                                       const float* wkv, const float* bkv, const float* wq, const float* bq, float* out,
                                       pasnl_stream_t stream) {
  using namespace pasnl;
  PASNL_REQUIRE(b >= 0 && p >= 0 && n >= 1 && c >= 1 && cz >= 1 && cb >= 1, PASNL_EINVAL);
  PASNL_REQUIRE(c <= 8 && cz <= 16 && (cb == 32 || cb == 64 || cb == 128), PASNL_EUNSUPPORTED);
  if (b == 0 || p == 0) return PASNL_OK;
  PASNL_REQUIRE(feature && new_point && wkv && bkv && wq && bq && out, PASNL_ENULL);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, PASNL_EUNSUPPORTED);
  hipStream_t st = pasnl_hip_stream(stream);
  // scores are kept in the log2 domain: exp(x / sqrt(cb) - m) == exp2(x * log2e / sqrt(cb) - m')
  const float scale = LOG2E / sqrtf((float)cb);
  if (c == 3) return nl_input_dispatch<3>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
  return nl_input_dispatch<8>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
}
