// Backward of the input-space Point-NonLocal cell (nl_input.hip): pasnl_cls_nl_cell_input_grad; include/pasnl.h has the contract.
//
// The forward is  Q = Z Wq + bq,  u = Wk Q,  w_j = softmax_j(r u . X_j),  ctr = sum_j w_j X_j,  out = ctr Wv + bv  (r = 1/sqrt(cb)).
// With G = dL/dout its backward keeps the forward's rank: per query  h = Wv G  (c numbers),  t_j = h . X_j,  delta = h . ctr,
// dS_j = w_j (t_j - delta),  du = r sum_j dS_j X_j;  per key  dX_j = sum_i (w_ij h_i + r dS_ij u_i);  and the weight gradients are
// products of the tiny moments  A = sum_i Z_i^T du_i (cz,c),  s = sum_i du_i (c),  dWv = sum_i ctr_i (x) G_i,  dbv = sum_i G_i:
//   dWk = A^T Wq + s (x) bq    dWq = A Wk    dbq = s Wk    dZ_i = du_i (Wk Wq^T)    dbk = 0.
// No matrix instruction, nothing cb-wide per key, no (b,p,cb) dQ.
//
// Three launches, no atomics, every sum in a fixed order:
//   query-major  nl_input_grad_query_kernel: the forward's structure (one lane per query, 64 queries x SPLIT waves, wave w walks
//                the w-th range of the cloud's keys through its own LDS region, rows read back as broadcasts), built from the
//                forward's own pieces (nl_input_core.hpp: projection, staged stream, block step, wave fold).  It recomputes u,
//                sweeps the keys ONCE for (m, l, ctr) -- hence lse and delta -- and a SECOND time for
//                du = r sum_j w_j (t_j - delta) X_j: the centred terms are summed as they are, never as the difference of two
//                large sums, and their own sum corrects delta and du for what h . ctr lost.  It writes dZ, the per-query
//                records (lse in the log2 domain, delta, u, h: 2c + 2 floats) and the workgroup's partial moments (its
//                queries in ascending order).
//   key-major    nl_input_grad_key_kernel: one lane per key, the records of its cloud's queries broadcast from LDS, queries
//                split over the waves, partial rows folded in ascending wave order -> dX.  Skipped when grad_feature is NULL.
//   finish       nl_input_grad_finish_kernel: the workgroups' partial moments summed in a fixed order (16 interleaved
//                ascending runs, then the runs in ascending order) and the c x cb / cz x cb products applied.
#include <math.h>
#include "nl_input_core.hpp"

namespace pasnl {

constexpr float NLIG_LN2 = 0.6931471805599453f;
constexpr int NLIG_KB = 8;          // keys per block: one maximum and one rescale in the first sweep, rows read ahead in both
                                    // (the forward's 16 and this kernel's h, delta and lse2 do not fit 16 waves' 128 registers)
// keys a wave stages at a time (query-major); 16 waves have 128 registers a lane and shorter ranges: half the rows in flight
constexpr int nlig_key_chunk(int split) { return split == 16 ? 128 : 256; }
constexpr int NLIG_RUNS = 16;       // interleaved runs of the finish kernel's sums (its waves)
// what a call needs: the second sweep (du, and the delta of the records); the moments A, s; the moments dWv, dbv
enum { NLIG_DU = 1, NLIG_A = 2, NLIG_V = 4 };

// ---------------------------------------------------------------------------------------------------------------------------
// query-major.  CT: channels carried (CT == 3: c == 3 exactly; otherwise any c <= CT, the channels beyond c are zeros).
// rec: planes of b * p floats -- lse2, delta, u[c] (log2 domain, as the scores are taken), h[c].
// part: per workgroup  A (cz,c) | s (c) | dWv (c,cb) | dbv (cb).
// ---------------------------------------------------------------------------------------------------------------------------
template <int CT, int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void nl_input_grad_query_kernel(
    int p, int n, int c, int cz, int cb, float scale, float rs, int flags, const float* __restrict__ feature,
    const float* __restrict__ new_point, const float* __restrict__ wkv, const float* __restrict__ wq,
    const float* __restrict__ bq, const float* __restrict__ gout, float* __restrict__ rec, float* __restrict__ grad_z,
    float* __restrict__ part) {
  constexpr int RW = CT <= 4 ? 4 : 8;             // floats of a staged key row
  constexpr int CHUNK = nlig_key_chunk(SPLIT);
  constexpr int WAVE_ROWS = CHUNK * RW;           // floats of a wave's staging region
  constexpr int PARK = 2 * CT * 64;               // floats a wave parks: (u, h), then (acc, m, l), then (du, e)
  extern __shared__ __align__(16) float nlig_smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* rows = nlig_smem + wave * WAVE_ROWS;
  float* park = nlig_smem + SPLIT * WAVE_ROWS;  // [SPLIT][2 CT][64]
  float* fin = park + SPLIT * PARK;             // [2 CT + 2][64]: du, ctr, lse2, delta of the tile's queries
  float* mz = fin + (2 * CT + 2) * 64;          // [c][cz]: Wk Wq^T
  const int bi = blockIdx.y, q0 = blockIdx.x * 64;
  const int qi = min(q0 + lane, p - 1);
  const size_t qrow = (size_t)bi * p + qi;
  const float* zrow = new_point + qrow * cz;
  const float* grow = gout + qrow * cb;
  const float* f = feature + (size_t)bi * n * c;

  if (grad_z != nullptr && (int)threadIdx.x < c * cz) {  // dZ_i = du_i (Wk Wq^T): the (c,cz) matrix once per workgroup
    const int ch = threadIdx.x / cz, a = threadIdx.x - ch * cz;
    float t = 0.f;
    for (int k = 0; k < cb; ++k) t = fmaf(wkv[ch * 2 * cb + k], wq[a * cb + k], t);
    mz[threadIdx.x] = t;
  }

  // ---- the forward's u (scaled) and h = Wv G beside it, then this wave's keys
  float u[CT], h[CT];
  nli_project<CT, SPLIT, PARK, true>(c, cz, cb, scale, zrow, grow, wkv, wq, bq, park, wave, lane, u, h);
  int k0, k1;
  nli_key_range<NLIG_KB>(wave, n, SPLIT, k0, k1);
  auto load_key = [&](int key, float (&v)[RW]) { nli_load_key<CT, RW>(f, key, k1, c, v); };

  // ---- first sweep, the forward's online pass: (m, l, sum_j p_j X_j) -> ctr, lse2, delta
  {
    float m = -INFINITY, l = 0.f, acc[CT];
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) acc[ch] = 0.f;
    nli_stream<RW, CHUNK>(k0, k1, rows, lane, load_key,
                          [&](const float* rp, int cnt) { nli_blocks<NLIG_KB, CT, RW>(rp, cnt, u, m, l, acc); });
    nli_fold<CT, SPLIT, PARK, true>(park, wave, lane, m, l, acc);
    if (wave == 0) {
      // (delta = h . ctr is taken from large t_j where one key dominates: ctr keeps every rounding it can -- fused merges, a
      // true division)
      float dl = 0.f;
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) {
        const float ctr = acc[ch] / l;
        fin[(CT + ch) * 64 + lane] = ctr;
        dl = fmaf(h[ch], ctr, dl);
      }
      fin[2 * CT * 64 + lane] = m + log2f(l);
      fin[(2 * CT + 1) * 64 + lane] = dl;
    }
    __syncthreads();
  }
  const float lse2 = fin[2 * CT * 64 + lane], delta = fin[(2 * CT + 1) * 64 + lane];

  // ---- second sweep: du = r sum_j w_j (t_j - delta) X_j with w_j = exp2(s_j - lse2), the centred terms summed directly.
  // Their plain sum e = sum_j w_j (t_j - delta) is what delta = h . ctr misses of sum_j w_j t_j -- a few ulp of delta, which is
  // large where one far key dominates, and which every dS_ij of the key-major launch would carry.  e is a sum of small terms
  // and costs one add a pair: delta + e goes into the record, and du takes the same step, du -= r e ctr.
  if (flags & NLIG_DU) {
    float du[CT], es = 0.f;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) du[ch] = 0.f;
    auto pair = [&](const float* rowp) {
      float x[RW];
      nli_read_row<RW>(rowp, x);
      float s = u[0] * x[0], t = h[0] * x[0];
#pragma unroll
      for (int ch = 1; ch < CT; ++ch) {
        s = fmaf(u[ch], x[ch], s);
        t = fmaf(h[ch], x[ch], t);
      }
      const float ds = fast_exp2(s - lse2) * (t - delta);
      es += ds;
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) du[ch] = fmaf(ds, x[ch], du[ch]);
    };
    nli_stream<RW, CHUNK>(k0, k1, rows, lane, load_key, [&](const float* rp, int cnt) {
      int j0 = 0;
      for (; j0 + NLIG_KB <= cnt; j0 += NLIG_KB) {
#pragma unroll
        for (int j = 0; j < NLIG_KB; ++j) pair(rp + (j0 + j) * RW);
      }
      for (; j0 < cnt; ++j0) pair(rp + j0 * RW);
    });
    if (wave > 0) {
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) park[wave * PARK + ch * 64 + lane] = du[ch];
      park[wave * PARK + CT * 64 + lane] = es;
    }
    __syncthreads();
    if (wave == 0) {  // (a wave that saw no key parked zeros)
      for (int w = 1; w < SPLIT; ++w) es += park[w * PARK + CT * 64 + lane];
#pragma unroll
      for (int ch = 0; ch < CT; ++ch) {
        float t = du[ch];
        for (int w = 1; w < SPLIT; ++w) t += park[w * PARK + ch * 64 + lane];
        fin[ch * 64 + lane] = fmaf(-es, fin[(CT + ch) * 64 + lane], t) * rs;
      }
      fin[(2 * CT + 1) * 64 + lane] = delta + es;
    }
    __syncthreads();
  }

  const bool qvalid = q0 + lane < p;
  if (grad_z != nullptr && qvalid) {  // the cz columns dealt to the waves
    for (int a = wave; a < cz; a += SPLIT) {
      float t = fin[lane] * mz[a];
      for (int ch = 1; ch < c; ++ch) t = fmaf(fin[ch * 64 + lane], mz[ch * cz + a], t);
      grad_z[qrow * cz + a] = t;
    }
  }
  if (rec != nullptr && wave == 1 && qvalid) {
    const size_t bp = (size_t)gridDim.y * p;
    float* rp = rec + qrow;
    rp[0] = lse2;
    rp[bp] = fin[(2 * CT + 1) * 64 + lane];
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
      if (CT == 3 || ch < c) {
        rp[(size_t)(2 + ch) * bp] = u[ch];
        rp[(size_t)(2 + c + ch) * bp] = h[ch];
      }
  }
  if (part != nullptr && (flags & (NLIG_A | NLIG_V))) {  // the tile's queries in ascending order, one element per thread
    const int nq = min(64, p - q0);
    const int ea = cz * c, e_all = ea + c + c * cb + cb;
    float* pt = part + ((size_t)bi * gridDim.x + blockIdx.x) * e_all;
    const float* z0 = new_point + ((size_t)bi * p + q0) * cz;
    const float* g0 = gout + ((size_t)bi * p + q0) * cb;
    for (int e = threadIdx.x; e < e_all; e += SPLIT * 64) {
      float t = 0.f;
      if (e < ea + c) {
        if (!(flags & NLIG_A)) continue;
        if (e < ea) {
          const int a = e / c, ch = e - a * c;
          for (int i = 0; i < nq; ++i) t = fmaf(z0[i * cz + a], fin[ch * 64 + i], t);
        } else {
          for (int i = 0; i < nq; ++i) t += fin[(e - ea) * 64 + i];
        }
      } else {
        if (!(flags & NLIG_V)) continue;
        const int e2 = e - ea - c;
        if (e2 < c * cb) {
          const int ch = e2 / cb, k = e2 - ch * cb;
          for (int i = 0; i < nq; ++i) t = fmaf(fin[(CT + ch) * 64 + i], g0[i * cb + k], t);
        } else {
          for (int i = 0; i < nq; ++i) t += g0[i * cb + e2 - c * cb];
        }
      }
      pt[e] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// key-major: dX_j = sum_i (w_ij h_i + r dS_ij u_i) over the queries of the key's cloud
// ---------------------------------------------------------------------------------------------------------------------------
template <int CT, int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void nl_input_grad_key_kernel(int p, int n, int c, const float* __restrict__ feature,
                                                                       const float* __restrict__ rec,
                                                                       float* __restrict__ grad_x) {
  constexpr int RW = (2 * CT + 2 + 3) / 4 * 4;  // a staged record: u[CT], h[CT], lse2, delta
  constexpr int CHUNK = CT <= 4 ? 128 : 64;     // records a wave stages at a time
  constexpr int WAVE_ROWS = CHUNK * RW;
  extern __shared__ __align__(16) float nlig_smem[];
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* rows = nlig_smem + wave * WAVE_ROWS;
  float* park = nlig_smem + SPLIT * WAVE_ROWS;  // [SPLIT][CT][64]
  const int bi = blockIdx.y, j0 = blockIdx.x * 64;
  const int key = min(j0 + lane, n - 1);
  const size_t bp = (size_t)gridDim.y * p;
  const float* rq = rec + (size_t)bi * p;

  float x[CT], acc[CT];
#pragma unroll
  for (int ch = 0; ch < CT; ++ch) {
    x[ch] = (CT == 3 || ch < c) ? feature[((size_t)bi * n + key) * c + ch] : 0.f;
    acc[ch] = 0.f;
  }
  const int per = (p + SPLIT - 1) / SPLIT;
  const int i0 = (int)min((long)wave * per, (long)p), i1 = (int)min((long)i0 + per, (long)p);
  nli_stream<RW, CHUNK>(
      i0, i1, rows, lane,
      [&](int i, float (&v)[RW]) {
        const bool in = i < i1;
#pragma unroll
        for (int ch = 0; ch < CT; ++ch) {
          const bool on = in && (CT == 3 || ch < c);
          v[ch] = on ? rq[(size_t)(2 + ch) * bp + i] : 0.f;
          v[CT + ch] = on ? rq[(size_t)(2 + c + ch) * bp + i] : 0.f;
        }
        v[2 * CT] = in ? rq[i] : 0.f;
        v[2 * CT + 1] = in ? rq[bp + i] : 0.f;
#pragma unroll
        for (int k = 2 * CT + 2; k < RW; ++k) v[k] = 0.f;
      },
      [&](const float* rp, int cnt) {
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
          float r[RW];
          nli_read_row<RW>(rp + i * RW, r);
          float s = r[0] * x[0], t = r[CT] * x[0];
#pragma unroll
          for (int ch = 1; ch < CT; ++ch) {
            s = fmaf(r[ch], x[ch], s);
            t = fmaf(r[CT + ch], x[ch], t);
          }
          const float w = fast_exp2(s - r[2 * CT]);
          const float dsl = w * (t - r[2 * CT + 1]) * NLIG_LN2;  // r dS u = dS ln2 (u in the log2 domain)
#pragma unroll
          for (int ch = 0; ch < CT; ++ch) acc[ch] = fmaf(dsl, r[ch], fmaf(w, r[CT + ch], acc[ch]));
        }
      });
  if (wave > 0) {
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) park[(wave * CT + ch) * 64 + lane] = acc[ch];
  }
  __syncthreads();
  if (wave == 0 && j0 + lane < n) {
    float* op = grad_x + ((size_t)bi * n + key) * c;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
      if (CT == 3 || ch < c) {
        float t = acc[ch];
        for (int w = 1; w < SPLIT; ++w) t += park[(w * CT + ch) * 64 + lane];  // (a wave that saw no query parked zeros)
        op[ch] = t;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// finish: the partial moments summed over the workgroups that wrote them, then the products.  Workgroups [0, vtiles) own 64
// elements of [dWv | dbv] each; the last one owns A and s and everything made of them, and the zeros of dbk.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NLIG_RUNS * 64) void nl_input_grad_finish_kernel(
    long nparts, int c, int cz, int cb, int vtiles, int flags, const float* __restrict__ part, const float* __restrict__ wkv,
    const float* __restrict__ wq, const float* __restrict__ bq, float* __restrict__ grad_wkv, float* __restrict__ grad_bkv,
    float* __restrict__ grad_wq, float* __restrict__ grad_bq) {
  __shared__ float red[NLIG_RUNS][64];
  __shared__ float mom[(16 + 1) * 8];  // A (cz,c), then s (c)
  const int tx = threadIdx.x & 63, run = threadIdx.x >> 6;
  const int ea = cz * c, e_all = ea + c + (c + 1) * cb;
  // element e over all partials: run r takes partials r, r + RUNS, ... in ascending order, then the runs in ascending order
  auto fold = [&](int e, bool valid) {
    float t = 0.f;
    if (valid)
      for (long i = run; i < nparts; i += NLIG_RUNS) t += part[(size_t)i * e_all + e];
    red[run][tx] = t;
    __syncthreads();
    float r = red[0][tx];
    for (int g = 1; g < NLIG_RUNS; ++g) r += red[g][tx];
    __syncthreads();
    return r;
  };
  if ((int)blockIdx.x < vtiles) {
    const int e2 = blockIdx.x * 64 + tx;
    const bool valid = e2 < (c + 1) * cb;
    const float r = fold(ea + c + e2, valid);
    if (run == 0 && valid) {
      if (e2 < c * cb) {
        const int ch = e2 / cb, k = e2 - ch * cb;
        if (grad_wkv != nullptr) grad_wkv[ch * 2 * cb + cb + k] = r;
      } else if (grad_bkv != nullptr) {
        grad_bkv[cb + e2 - c * cb] = r;
      }
    }
    return;
  }
  if (grad_bkv != nullptr)  // Q . bk is constant over the keys and cancels in the softmax
    for (int k = threadIdx.x; k < cb; k += NLIG_RUNS * 64) grad_bkv[k] = 0.f;
  if (!(flags & NLIG_A)) return;
  for (int e0 = 0; e0 < ea + c; e0 += 64) {
    const bool valid = e0 + tx < ea + c;
    const float r = fold(e0 + tx, valid);
    if (run == 0 && valid) mom[e0 + tx] = r;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < (c + cz + 1) * cb; o += NLIG_RUNS * 64) {
    const int row = o / cb, k = o - row * cb;
    if (row < c) {  // dWk = A^T Wq + s (x) bq
      if (grad_wkv == nullptr) continue;
      float t = mom[ea + row] * bq[k];
      for (int a = 0; a < cz; ++a) t = fmaf(mom[a * c + row], wq[a * cb + k], t);
      grad_wkv[row * 2 * cb + k] = t;
    } else if (row < c + cz) {  // dWq = A Wk
      if (grad_wq == nullptr) continue;
      const int a = row - c;
      float t = 0.f;
      for (int ch = 0; ch < c; ++ch) t = fmaf(mom[a * c + ch], wkv[ch * 2 * cb + k], t);
      grad_wq[a * cb + k] = t;
    } else {  // dbq = s Wk
      if (grad_bq == nullptr) continue;
      float t = 0.f;
      for (int ch = 0; ch < c; ++ch) t = fmaf(mom[ea + ch], wkv[ch * 2 * cb + k], t);
      grad_bq[k] = t;
    }
  }
}

struct NligArgs {
  int b, p, n, c, cz, cb, flags;
  const float *feature, *new_point, *wkv, *wq, *bq, *gout;
  float *grad_x, *grad_z, *rec, *part;
};

template <int CT, int SPLIT>
static int nlig_query_launch(const NligArgs& a, hipStream_t st) {
  const size_t lds = ((size_t)SPLIT * (nlig_key_chunk(SPLIT) * (CT <= 4 ? 4 : 8) + 2 * CT * 64) + (2 * CT + 2) * 64 + 8 * 16) * sizeof(float);
  // scores in the log2 domain, with the forward's own factor: exp(x / sqrt(cb) - m) == exp2(x * log2e / sqrt(cb) - m')
  const float scale = LOG2E / sqrtf((float)a.cb), rs = 1.0f / sqrtf((float)a.cb);
  return launch(nl_input_grad_query_kernel<CT, SPLIT>, dim3((a.p + 63) / 64, a.b), dim3(SPLIT * 64), lds, st, a.p, a.n, a.c, a.cz,
                a.cb, scale, rs, a.flags, a.feature, a.new_point, a.wkv, a.wq, a.bq, a.gout,
                a.grad_x != nullptr ? a.rec : nullptr, a.grad_z, a.part);
}
template <int CT, int SPLIT>
static int nlig_key_launch(const NligArgs& a, hipStream_t st) {
  const size_t lds = (size_t)SPLIT * ((CT <= 4 ? 128 : 64) * ((2 * CT + 2 + 3) / 4 * 4) + CT * 64) * sizeof(float);
  return launch(nl_input_grad_key_kernel<CT, SPLIT>, dim3((a.n + 63) / 64, a.b), dim3(SPLIT * 64), lds, st, a.p, a.n, a.c, a.feature,
                a.rec, a.grad_x);
}

// keys split over the waves of the query-major launch, queries over those of the key-major one
template <int CT>
static int nlig_dispatch(const NligArgs& a, hipStream_t st) {
  int rc = nli_with_split<CT>(nli_split(a.b, a.p, a.n), [&](auto s) { return nlig_query_launch<CT, decltype(s)::value>(a, st); });
  if (rc != PASNL_OK || a.grad_x == nullptr) return rc;
  return nli_with_split<CT>(nli_split(a.b, a.n, a.p), [&](auto s) { return nlig_key_launch<CT, decltype(s)::value>(a, st); });
}

static size_t nlig_record_floats(int b, int p, int c) { return (size_t)(2 * c + 2) * (size_t)b * (size_t)p; }
static size_t nlig_moment_floats(int c, int cz, int cb) { return (size_t)(cz + 1) * c + (size_t)(c + 1) * cb; }

}  // namespace pasnl

using namespace pasnl;

extern "C" size_t pasnl_cls_nl_cell_input_grad_workspace_bytes(int b, int p, int n, int c, int cz, int cb) {
  if (b <= 0 || p <= 0 || n <= 0 || c < 1 || c > 8 || cz < 1 || cz > 16 || !(cb == 32 || cb == 64 || cb == 128)) return 0;
  const size_t tiles = (size_t)b * (size_t)((p + 63) / 64);
  return sizeof(float) * (nlig_record_floats(b, p, c) + tiles * nlig_moment_floats(c, cz, cb));
}

extern "C" int pasnl_cls_nl_cell_input_grad(int b, int p, int n, int c, int cz, int cb, const float* feature,
                                            const float* new_point, const float* wkv, const float* bkv, const float* wq,
                                            const float* bq, const float* grad_out, float* grad_feature, float* grad_new_point,
                                            float* grad_wkv, float* grad_bkv, float* grad_wq, float* grad_bq, void* workspace,
                                            size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && p >= 0 && n >= 1 && c >= 1 && cz >= 1 && cb >= 1, PASNL_EINVAL);
  PASNL_REQUIRE(c <= 8 && cz <= 16 && (cb == 32 || cb == 64 || cb == 128), PASNL_EUNSUPPORTED);
  hipStream_t st = pasnl_hip_stream(stream);
  if (b == 0 || p == 0) {  // no query: nothing receives a gradient
    const struct { float* ptr; size_t count; } outs[] = {
        {grad_feature, (size_t)b * n * c}, {grad_new_point, 0},     {grad_wkv, (size_t)c * 2 * cb},
        {grad_bkv, (size_t)2 * cb},        {grad_wq, (size_t)cz * cb}, {grad_bq, (size_t)cb}};
    for (const auto& o : outs)
      if (o.ptr != nullptr && o.count > 0)
        PASNL_REQUIRE(hipMemsetAsync(o.ptr, 0, o.count * sizeof(float), st) == hipSuccess, PASNL_ELAUNCH);
    return PASNL_OK;
  }
  PASNL_REQUIRE(feature && new_point && wkv && bkv && wq && bq && grad_out && workspace, PASNL_ENULL);
  PASNL_REQUIRE(grad_feature || grad_new_point || grad_wkv || grad_bkv || grad_wq || grad_bq, PASNL_ENULL);
  PASNL_REQUIRE(((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(workspace_bytes >= pasnl_cls_nl_cell_input_grad_workspace_bytes(b, p, n, c, cz, cb), PASNL_EWORKSPACE);

  NligArgs a{};
  a.b = b, a.p = p, a.n = n, a.c = c, a.cz = cz, a.cb = cb;
  a.feature = feature, a.new_point = new_point, a.wkv = wkv, a.wq = wq, a.bq = bq, a.gout = grad_out;
  a.grad_x = grad_feature, a.grad_z = grad_new_point;
  a.rec = static_cast<float*>(workspace);
  a.part = a.rec + nlig_record_floats(b, p, c);
  const bool need_a = grad_wkv || grad_wq || grad_bq, need_v = grad_wkv || grad_bkv;
  a.flags = (need_a || grad_new_point || grad_feature ? NLIG_DU : 0) | (need_a ? NLIG_A : 0) | (need_v ? NLIG_V : 0);
  const int rc = c == 3 ? nlig_dispatch<3>(a, st) : nlig_dispatch<8>(a, st);
  if (rc != PASNL_OK) return rc;
  if (need_a || need_v) {
    const int vtiles = need_v ? ((c + 1) * cb + 63) / 64 : 0;
    const long nparts = (long)b * ((p + 63) / 64);
    hipLaunchKernelGGL(nl_input_grad_finish_kernel, dim3(vtiles + 1), dim3(NLIG_RUNS * 64), 0, st, nparts, c, cz, cb, vtiles,
                       a.flags, a.part, wkv, wq, bq, grad_wkv, grad_bkv, grad_wq, grad_bq);
  }
  return pasnl_launch_status();
}
