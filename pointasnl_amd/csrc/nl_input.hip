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
#include <math.h>
#include "common.hpp"

namespace pasnl {

constexpr float NLI_LOG2E = 1.4426950408889634f;
constexpr int NLI_KB = 16;      // keys per softmax block
constexpr int NLI_CHUNK = 256;  // keys a wave stages at a time
constexpr int NLI_MIN_KEYS = 64;  // a wave's range is at least this long before the keys are split further

__device__ __forceinline__ float nli_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// one block of KB staged rows (valid of them are keys if MASK) folded into (m, l, acc)
template <int CT, int RW, bool MASK>
__device__ __forceinline__ void nli_block(const float* rowp, int valid, const float (&u)[CT], float& m, float& l, float (&acc)[CT]) {
  float x[NLI_KB][RW], s[NLI_KB];
#pragma unroll
  for (int j = 0; j < NLI_KB; ++j)
#pragma unroll
    for (int g = 0; g < RW / 4; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(rowp + j * RW + 4 * g);
      x[j][4 * g] = v.x; x[j][4 * g + 1] = v.y; x[j][4 * g + 2] = v.z; x[j][4 * g + 3] = v.w;
    }
#pragma unroll
  for (int j = 0; j < NLI_KB; ++j) {
    float t = u[0] * x[j][0];
#pragma unroll
    for (int ch = 1; ch < CT; ++ch) t = fmaf(u[ch], x[j][ch], t);
    s[j] = (MASK && j >= valid) ? -INFINITY : t;
  }
  float bm = s[0];
#pragma unroll
  for (int j = 1; j < NLI_KB; ++j) bm = fmaxf(bm, s[j]);
  const float mnew = fmaxf(m, bm);  // finite: key 0 of a block is always valid
  const float alpha = nli_exp2(m - mnew);  // m = -inf (nothing seen yet): 0
  l *= alpha;
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) acc[ch] *= alpha;
#pragma unroll
  for (int j = 0; j < NLI_KB; ++j) {
    const float pj = nli_exp2(s[j] - mnew);  // masked rows: 0 (their staged values are zeros)
    l += pj;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) acc[ch] = fmaf(pj, x[j][ch], acc[ch]);
  }
  m = mnew;
}

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
  constexpr int RPL = NLI_CHUNK / 64;          // rows of a chunk a lane copies
  extern __shared__ __align__(16) float nli_smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* rows = nli_smem + wave * WAVE_ROWS;
  float* park = nli_smem + SPLIT * WAVE_ROWS;  // [SPLIT][CT + 2][64]
  const int bi = blockIdx.y, q0 = blockIdx.x * 64;
  const int qi = min(q0 + lane, p - 1);
  const float* zrow = new_point + ((size_t)bi * p + qi) * cz;
  const float* f = feature + (size_t)bi * n * c;

  // ---- u = Wk (Z Wq + bq): the bottleneck's columns in groups of four, dealt to the waves; the partial sums meet in LDS
  float u[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) u[ch] = 0.f;
  for (int kg = wave * 4; kg < cb; kg += SPLIT * 4) {
    float qv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) qv[j] = bq[kg + j];
    for (int i = 0; i < cz; ++i) {
      const float zi = zrow[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) qv[j] = fmaf(zi, wq[i * cb + kg + j], qv[j]);
    }
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
      if (CT == 3 || ch < c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) u[ch] = fmaf(qv[j], wkv[ch * 2 * cb + kg + j], u[ch]);
      }
  }
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) park[wave * PARK + ch * 64 + lane] = u[ch];
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) {
    float t = park[ch * 64 + lane];
    for (int w = 1; w < SPLIT; ++w) t += park[w * PARK + ch * 64 + lane];
    u[ch] = t * scale;
  }
  __syncthreads();  // (park is written again at the merge)

  // ---- this wave's keys [k0, k1): whole blocks where the cloud has them
  const int per = ((n + SPLIT - 1) / SPLIT + NLI_KB - 1) / NLI_KB * NLI_KB;
  const int k0 = (int)min((long)wave * per, (long)n), k1 = (int)min((long)k0 + per, (long)n);
  float m = -INFINITY, l = 0.f, acc[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) acc[ch] = 0.f;

  float pre[RPL][CT];  // the next chunk on its way in
  auto fetch = [&](int kc) {
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      const int key = kc + r * 64 + lane;
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) pre[r][ch] = (key < k1 && (CT == 3 || ch < c)) ? f[(size_t)key * c + ch] : 0.f;
    }
  };
  if (k0 < k1) fetch(k0);
  for (int kc = k0; kc < k1; kc += NLI_CHUNK) {
#pragma unroll
    for (int r = 0; r < RPL; ++r)
#pragma unroll
      for (int g = 0; g < RW / 4; ++g) {
        float4 v;
        v.x = pre[r][4 * g];
        v.y = 4 * g + 1 < CT ? pre[r][4 * g + 1 < CT ? 4 * g + 1 : 0] : 0.f;
        v.z = 4 * g + 2 < CT ? pre[r][4 * g + 2 < CT ? 4 * g + 2 : 0] : 0.f;
        v.w = 4 * g + 3 < CT ? pre[r][4 * g + 3 < CT ? 4 * g + 3 : 0] : 0.f;
        *reinterpret_cast<float4*>(rows + (r * 64 + lane) * RW + 4 * g) = v;
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (kc + NLI_CHUNK < k1) fetch(kc + NLI_CHUNK);
    const int cnt = min(NLI_CHUNK, k1 - kc);
    int j0 = 0;
    for (; j0 + NLI_KB <= cnt; j0 += NLI_KB) nli_block<CT, RW, false>(rows + j0 * RW, NLI_KB, u, m, l, acc);
    if (j0 < cnt) nli_block<CT, RW, true>(rows + j0 * RW, cnt - j0, u, m, l, acc);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // every lane has read the chunk before the next one lands on it
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // ---- fold the waves' partial results in ascending wave order (wave 0), then the centroid goes back through Wv
  if (wave > 0) {
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) park[wave * PARK + ch * 64 + lane] = acc[ch];
    park[wave * PARK + CT * 64 + lane] = m;
    park[wave * PARK + (CT + 1) * 64 + lane] = l;
  }
  __syncthreads();
  if (wave == 0) {
    for (int w = 1; w < SPLIT; ++w) {
      const float* pw = park + w * PARK;
      const float mw = pw[CT * 64 + lane], lw = pw[(CT + 1) * 64 + lane];
      const float mnew = fmaxf(m, mw);  // a wave that saw no key has m = -inf, l = 0, acc = 0
      const float a0 = m == -INFINITY ? 0.f : nli_exp2(m - mnew);
      const float a1 = mw == -INFINITY ? 0.f : nli_exp2(mw - mnew);
      l = l * a0 + lw * a1;
      m = mnew;
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) acc[ch] = acc[ch] * a0 + pw[ch * 64 + lane] * a1;
    }
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

// Waves per workgroup: the smallest of 4, 8, 16 that puts two waves on every SIMD (2048), as long as a wave keeps
// NLI_MIN_KEYS keys of its own.  cls layer 1 (64 x 512 queries, 1024 keys): 4 -> 2048 waves of 256 keys; ScanNet layer 1
// (16 x 1024, 8192 keys): 8 -> 2048 waves; KITTI (8 x 1280, 10240 keys): 16 -> 2560 waves in 160 workgroups.
static int nl_input_split(int b, int p, int n) {
  const long tiles = (long)b * ((p + 63) / 64);
  int split = 4;
  while (split < 16 && tiles * split < 2048 && n / (split * 2) >= NLI_MIN_KEYS) split *= 2;
  return split;
}

template <int CT>
static int nl_input_dispatch(int b, int p, int n, int c, int cz, int cb, float scale, const float* feature, const float* new_point,
                      const float* wkv, const float* bkv, const float* wq, const float* bq, float* out, hipStream_t st) {
  const int split = nl_input_split(b, p, n);
  if constexpr (CT <= 4) {  // (16 waves are 128 registers a lane: a block of the wide form's rows alone would fill them)
    if (split == 16) return nl_input_launch<CT, 16>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
  }
  switch (split) {
    case 16:
    case 8: return nl_input_launch<CT, 8>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
    default: return nl_input_launch<CT, 4>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
  }
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
  const float scale = NLI_LOG2E / sqrtf((float)cb);
  if (c == 3) return nl_input_dispatch<3>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
  return nl_input_dispatch<8>(b, p, n, c, cz, cb, scale, feature, new_point, wkv, bkv, wq, bq, out, st);
}
