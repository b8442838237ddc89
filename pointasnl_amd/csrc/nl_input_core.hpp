// What the forward (nl_input.hip) and the backward (nl_input_grad.hip) of the input-space Point-NonLocal cell share: one
// definition each, so that the backward's recomputed u, scores and softmax statistics are the forward's by construction.
//
// One lane owns one query (key-major launch: one key); a workgroup is 64 lanes x SPLIT waves and wave w walks the w-th
// contiguous range of the items the lanes attend over.  An item's row is the same for every lane: a wave copies its range
// into its own LDS region CHUNK rows at a time (nli_stream) and reads the rows back as broadcasts.  Scores of a block of KB
// keys are formed first, then one block maximum, one rescale of (l, acc) and one exp2 per pair (nli_block; scores live in
// the log2 domain: log2e / sqrt(cb) is folded into u by nli_project).  The waves' partial (m, l, acc) meet in LDS and are
// folded in ascending wave order (nli_fold).  The build is -ffp-contract=off: every fmaf against a * b + c here is a
// decision about bits.
#pragma once
#include <math.h>
#include "common.hpp"

namespace pasnl {

constexpr int NLI_MIN_ITEMS = 64;  // a wave's range is at least this long before it is split further

__device__ __forceinline__ void nli_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave walks the items [i0, i1) CHUNK at a time through its own LDS region: load(item, row) fetches one item's RW floats
// (zeros past the range), the next chunk's loads are in flight while use(rows, count) consumes the current one.  No
// workgroup barrier inside.  (The loop is the forward's own: with the last chunk left by a break its wide form needs two
// registers more.)
template <int RW, int CHUNK, class Load, class Use>
__device__ __forceinline__ void nli_stream(int i0, int i1, float* rows, int lane, Load&& load, Use&& use) {
  constexpr int RPL = CHUNK / 64;  // rows of a chunk a lane copies
  float pre[RPL][RW];
  auto fetch = [&](int ic) {
#pragma unroll
    for (int r = 0; r < RPL; ++r) load(ic + r * 64 + lane, pre[r]);
  };
  if (i0 < i1) fetch(i0);
  for (int ic = i0; ic < i1; ic += CHUNK) {
#pragma unroll
    for (int r = 0; r < RPL; ++r)
#pragma unroll
      for (int g = 0; g < RW / 4; ++g)
        *reinterpret_cast<float4*>(rows + (r * 64 + lane) * RW + 4 * g) =
            make_float4(pre[r][4 * g], pre[r][4 * g + 1], pre[r][4 * g + 2], pre[r][4 * g + 3]);
    nli_wave_sync();
    if (ic + CHUNK < i1) fetch(ic + CHUNK);
    use(rows, min(CHUNK, i1 - ic));
    nli_wave_sync();  // every lane has read the chunk before the next one lands on it
  }
}

template <int RW>
__device__ __forceinline__ void nli_read_row(const float* rowp, float (&x)[RW]) {
#pragma unroll
  for (int g = 0; g < RW / 4; ++g) {
    const float4 v = *reinterpret_cast<const float4*>(rowp + 4 * g);
    x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
  }
}

// Key `key` of the cloud at f as a staged row: its c channels (CT == 3: c == 3 exactly), zeros beyond them and past k1
template <int CT, int RW>
__device__ __forceinline__ void nli_load_key(const float* f, int key, int k1, int c, float (&v)[RW]) {
#pragma unroll
  for (int ch = 0; ch < RW; ++ch) v[ch] = (ch < CT && key < k1 && (CT == 3 || ch < c)) ? f[(size_t)key * c + ch] : 0.f;
}

// one block of KB staged rows (valid of them are keys if MASK) folded into (m, l, acc)
template <int KB, int CT, int RW, bool MASK>
__device__ __forceinline__ void nli_block(const float* rowp, int valid, const float (&u)[CT], float& m, float& l, float (&acc)[CT]) {
  float x[KB][RW], s[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) nli_read_row<RW>(rowp + j * RW, x[j]);
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    float t = u[0] * x[j][0];
#pragma unroll
    for (int ch = 1; ch < CT; ++ch) t = fmaf(u[ch], x[j][ch], t);
    s[j] = (MASK && j >= valid) ? -INFINITY : t;
  }
  float bm = s[0];
#pragma unroll
  for (int j = 1; j < KB; ++j) bm = fmaxf(bm, s[j]);
  const float mnew = fmaxf(m, bm);  // finite: key 0 of a block is always valid
  const float alpha = fast_exp2(m - mnew);  // m = -inf (nothing seen yet): 0
  l *= alpha;
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) acc[ch] *= alpha;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const float pj = fast_exp2(s[j] - mnew);  // masked rows: 0 (their staged values are zeros)
    l += pj;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) acc[ch] = fmaf(pj, x[j][ch], acc[ch]);
  }
  m = mnew;
}

// The cnt staged rows of a chunk: whole blocks, then a masked one.  (m, l, acc) reach this through the by-reference captures
// of nli_stream's `use`; the blocks run on copies, which keeps the forward's wide form at the 218 registers it had with the
// loop written out in the kernel (220 on the references).
template <int KB, int CT, int RW>
__device__ __forceinline__ void nli_blocks(const float* rp, int cnt, const float (&u)[CT], float& m, float& l, float (&acc)[CT]) {
  float m_ = m, l_ = l, a_[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) a_[ch] = acc[ch];
  int j0 = 0;
  for (; j0 + KB <= cnt; j0 += KB) nli_block<KB, CT, RW, false>(rp + j0 * RW, KB, u, m_, l_, a_);
  if (j0 < cnt) nli_block<KB, CT, RW, true>(rp + j0 * RW, cnt - j0, u, m_, l_, a_);
  m = m_, l = l_;
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) acc[ch] = a_[ch];
}

// u = Wk (Z Wq + bq) * scale in every wave's registers and, WITH_H, h = Wv G beside it (h: CT floats; else unused).  The
// bottleneck's columns go in groups of four to the waves; the partial sums meet in the first CT (WITH_H: 2 CT) planes of each
// wave's PARK floats of `park` and are added in ascending wave order.  Two workgroup barriers: park is free again on return.
template <int CT, int SPLIT, int PARK, bool WITH_H>
__device__ __forceinline__ void nli_project(int c, int cz, int cb, float scale, const float* zrow, const float* grow,
                                            const float* wkv, const float* wq, const float* bq, float* park, int wave, int lane,
                                            float (&u)[CT], float* h) {
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) {
    u[ch] = 0.f;
    if constexpr (WITH_H) h[ch] = 0.f;
  }
  for (int kg = wave * 4; kg < cb; kg += SPLIT * 4) {
    float qv[4], gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) qv[j] = bq[kg + j];
    for (int i = 0; i < cz; ++i) {
      const float zi = zrow[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) qv[j] = fmaf(zi, wq[i * cb + kg + j], qv[j]);
    }
    if constexpr (WITH_H) {
      const float4 g4 = *reinterpret_cast<const float4*>(grow + kg);
      gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
    }
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
      if (CT == 3 || ch < c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u[ch] = fmaf(qv[j], wkv[ch * 2 * cb + kg + j], u[ch]);
          if constexpr (WITH_H) h[ch] = fmaf(gv[j], wkv[ch * 2 * cb + cb + kg + j], h[ch]);
        }
      }
  }
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) {
    park[wave * PARK + ch * 64 + lane] = u[ch];
    if constexpr (WITH_H) park[wave * PARK + (CT + ch) * 64 + lane] = h[ch];
  }
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) {
    float t = park[ch * 64 + lane], th = WITH_H ? park[(CT + ch) * 64 + lane] : 0.f;
    for (int w = 1; w < SPLIT; ++w) {
      t += park[w * PARK + ch * 64 + lane];
      if constexpr (WITH_H) th += park[w * PARK + (CT + ch) * 64 + lane];
    }
    u[ch] = t * scale;
    if constexpr (WITH_H) h[ch] = th;
  }
  __syncthreads();
}

// wave `wave` of `split`'s keys [k0, k1) of n: whole blocks of KB where the cloud has them
template <int KB>
__device__ __forceinline__ void nli_key_range(int wave, int n, int split, int& k0, int& k1) {
  const int per = ((n + split - 1) / split + KB - 1) / KB * KB;
  k0 = (int)min((long)wave * per, (long)n);
  k1 = (int)min((long)k0 + per, (long)n);
}

// The waves' partial (m, l, acc) folded into wave 0's in ascending wave order, through the first CT + 2 planes of each
// wave's PARK floats of `park` (one workgroup barrier).  A wave that saw no key carries m = -inf, l = 0, acc = 0.
// FUSED: the merges as fmaf(x, a0, y * a1) (the backward's: see its comment on delta); otherwise x * a0 + y * a1.
template <int CT, int SPLIT, int PARK, bool FUSED>
__device__ __forceinline__ void nli_fold(float* park, int wave, int lane, float& m, float& l, float (&acc)[CT]) {
  if (wave > 0) {
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) park[wave * PARK + ch * 64 + lane] = acc[ch];
    park[wave * PARK + CT * 64 + lane] = m;
    park[wave * PARK + (CT + 1) * 64 + lane] = l;
  }
  __syncthreads();
  if (wave == 0) {
    auto merge = [](float x, float a0, float y, float a1) { return FUSED ? fmaf(x, a0, y * a1) : x * a0 + y * a1; };
    for (int w = 1; w < SPLIT; ++w) {
      const float* pw = park + w * PARK;
      const float mw = pw[CT * 64 + lane], lw = pw[(CT + 1) * 64 + lane];
      const float mnew = fmaxf(m, mw);
      const float a0 = m == -INFINITY ? 0.f : fast_exp2(m - mnew);
      const float a1 = mw == -INFINITY ? 0.f : fast_exp2(mw - mnew);
      l = merge(l, a0, lw, a1);
      m = mnew;
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) acc[ch] = merge(acc[ch], a0, pw[ch * 64 + lane], a1);
    }
  }
}

// Waves per workgroup of a launch with one lane per `lanes` (queries, or keys in the key-major launch) that attends over
// `items`: the smallest of 4, 8, 16 that puts two waves on every SIMD (2048), as long as a wave keeps NLI_MIN_ITEMS items of
// its own.  cls layer 1 (64 x 512 queries, 1024 keys): 4 -> 2048 waves of 256 keys; ScanNet layer 1 (16 x 1024, 8192 keys):
// 8 -> 2048 waves; KITTI (8 x 1280, 10240 keys): 16 -> 2560 waves in 160 workgroups.
static int nli_split(int b, int lanes, int items) {
  const long tiles = (long)b * ((lanes + 63) / 64);
  int split = 4;
  while (split < 16 && tiles * split < 2048 && items / (split * 2) >= NLI_MIN_ITEMS) split *= 2;
  return split;
}

// f(std::integral_constant<int, SPLIT>) for nli_split's choice.  16 waves are 128 registers a lane: a block of the wide form's
// rows alone would fill them, so CT == 8 stops at 8 waves.
template <int CT, class F>
static int nli_with_split(int split, F&& f) {
  return with_split<4, (CT <= 4 ? 16 : 8)>(split, f);
}

}  // namespace pasnl
