// The "group all" PointNet set-abstraction module of the classifier in ONE kernel (+ a pooling pass over tile maxima):
// reference utils/pointnet_util.py:87-137 as called at models/pointasnl_cls.py:39-40 (layer3_1: 512 points x [128, 256, 512],
// layer3_2: 128 points x [256, 512, 1024]) -- sample_and_group_all (every point of the cloud is one group), three 1x1
// convolutions (BN folded, ReLU) and tf.reduce_max over the group.  Round 4 ran it as three vendor GEMMs + a pooling kernel
// per module: eight launches at 58-123 TF whose 256 tiles (one per CU) stretch by whatever shares a CU with them (the next
// batch's sampler: 78 -> 141 us for the widest product).
//
// One workgroup of 8 waves owns a tile of 32 RB points of one cloud (RB = 2 row blocks where 64 rows of activations fit the
// LDS -- every weight then feeds two products --, else 1) and carries it through all three convolutions:
//   X (rows x k0) -> LDS buffer A;  H1 = relu(X W0 + b0) -> LDS buffer B;  H2 = relu(H1 W1 + b1) -> buffer A;
//   H3 = relu(H2 W2 + b2) never leaves the registers: its column maxima over the tile's rows go to partial[cloud][tile][:].
// v_mfma_f32_32x32x2_f32 with A = the activations (row ql of the tile, LDS, odd row pitch: conflict-free), B = the weights
// (straight from global memory / L2, PACKED in operand order: 32 bytes per lane and batch of eight steps, see mp_mm),
// D[m = row kappa(r, h)][n = channel]: the bias is one value per lane, the store of a block is column-contiguous, and the
// pooled maximum is a maximum over a lane's 16 accumulators and one exchange between the wave's halves.  A wave owns the
// 32-channel blocks wave, wave + 8, ...: one LDS operand feeds up to four products.  Operands of the NEXT eight steps are
// requested while eight steps multiply (two register sets).  The grid has 4 (n = 128, 32-row tiles) or 8 (n = 512, 64-row tiles) tiles
// per cloud: more workgroups than CUs, handed out by the dispatcher as CUs become free -- a CU that shares its time with the sampler simply
// takes fewer tiles.  fp32 MFMA: an exact fmaf chain (another summation order than the vendor GEMM's: parity 1e-5 of scale).
//
// tail_group_all_kernel (pasnl_cls_tail_group_all) is layer3_1's form of the same kernel with the classifier's layer 1 tail in
// front of it: the tile's X rows are not read from a table but computed in place from the tail's inputs (mlp3_tile is the part
// the two kernels share; the tail's products are sa_tail.hpp's, shared with cells.hip).  tail_mlp2_kernel (pasnl_cls_tail_mlp2)
// is layer 2's: its tail and the first two convolutions of layer3_2, whose third stays a vendor GEMM (see there).
#include "common.hpp"
#include "sa_tail.hpp"

namespace pasnl {

typedef float mp_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mp_kappa(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

// Weights in OPERAND order (pasnl_mlp3_pack_weights): for a batch of 8 matrix steps = 16 contraction indices 16 bt .. + 15, lane
// (column n, half h) needs W[16 bt + 2 u + h][n], u = 0 .. 7 -- packed as P[bt][h][n][u]: 32 contiguous bytes per lane and
// batch = two 16-byte loads (round 5 first read them as eight 4-byte loads of the row-major matrix: a quarter of the bytes
// per instruction; with the loads ablated the kernel ran 25 / 50 us faster), a half-wave's 32 columns 1 KiB contiguous.  The
// contraction length is padded to a multiple of 16 with zero weights (the activations there only have to be finite).
//
// acc[i] += X[32 rows][16 NBT] . W[16 NBT][block i]  for the wave's NB blocks.  xrow = in + ql * pitch + h;  the lane's packed
// weights of block i start at Wp + loff[i] (floats; h and the column folded in), a batch further every 16 WOUT floats.
template <int WOUT, int NB, int RB>
__device__ __forceinline__ void mp_mm(const float* xrow, int rbstride, int NBT, const float* __restrict__ Wp, const int (&loff)[NB],
                                      mp_f32x16 (&acc)[RB][NB]) {
  constexpr int BT = 8;
  float xb[2][RB][BT];
  float4 wa[2][NB][2];
  auto load = [&](int set, int bt) {
    const float* wrow = Wp + (size_t)bt * (16 * WOUT);  // (uniform: a scalar base, the lane's offset in a register)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      wa[set][i][0] = *reinterpret_cast<const float4*>(wrow + loff[i]);
      wa[set][i][1] = *reinterpret_cast<const float4*>(wrow + loff[i] + 4);
    }
#pragma unroll
    for (int u = 0; u < BT; ++u)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
        xb[set][rb][u] = xrow[rb * rbstride + 2 * (bt * BT + u)];
  };
  load(0, 0);
  for (int bt = 0; bt < NBT; bt += 2) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int b0 = bt + half;
      if (b0 < NBT) {
        load(half ^ 1, min(b0 + 1, NBT - 1));  // the next batch (a dummy re-read behind the last one)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < BT; ++u) {
          float wv[NB];
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const float4 q = wa[half][i][u >> 2];
            wv[i] = (u & 3) == 0 ? q.x : ((u & 3) == 1 ? q.y : ((u & 3) == 2 ? q.z : q.w));
          }
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int i = 0; i < NB; ++i)
              acc[rb][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[half][rb][u], wv[i], acc[rb][i], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// one convolution of the tile: out[row][channel] = relu(in . W + bias), blocks of 32 channels dealt to the waves round robin
template <int WOUT, int RB>
__device__ __forceinline__ void mp_layer(const float* in, int pin, int K, const float* __restrict__ W, const float* __restrict__ bias,
                                         float* out, int pout, int wave, int ql, int h, int rows = 32 * RB) {
  constexpr int NW = 8, BLOCKS = WOUT / 32, NB = BLOCKS >= NW ? BLOCKS / NW : 1;
  if constexpr (BLOCKS * RB == NW && RB > 1) {
    // fewer blocks than waves (layer 0 of the narrower module): the tile's row blocks go to different waves instead of
    // idling half of them -- wave w owns block w mod BLOCKS of row block w / BLOCKS
    const int rb = wave / BLOCKS;
    mp_layer<WOUT, 1>(in + rb * 32 * pin, pin, K, W, bias, out + rb * 32 * pout, pout, wave % BLOCKS, ql, h);
    return;
  }
  if (wave >= BLOCKS) return;  // (fewer blocks than waves)
  int loff[NB];
  mp_f32x16 acc[RB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    loff[i] = (h * WOUT + (wave + NW * i) * 32 + ql) * 8;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][i][r] = 0.f;
  }
  mp_mm<WOUT, NB, RB>(in + ql * pin + h, 32 * pin, (K + 15) >> 4, W, loff, acc);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int ch = (wave + NW * i) * 32 + ql;
    const float bb = bias[ch];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (rb * 32 + mp_kappa(r, h) < rows)  // (rows: the default keeps every row -- the tile is LDS; a tile stored to memory ends with its cloud)
          out[(rb * 32 + mp_kappa(r, h)) * pout + ch] = fmaxf(acc[rb][i][r] + bb, 0.f);
  }
}

// the three convolutions of a tile staged in A ([32 RB][pa]: X, then H2; Bf [32 RB][C1 + 1]: H1), behind the barrier that
// published X: the column maxima of relu(H2 W2 + b2) over the tile's rows go to po[0 .. C3)
template <int C1, int C2, int C3, int RB>
__device__ __forceinline__ void mlp3_tile(float* A, int pa, float* Bf, int k0, const float* __restrict__ w0, const float* __restrict__ b0,
                                          const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                          const float* __restrict__ b2, float* __restrict__ po, int wave, int ql, int h) {
  constexpr int NW = 8, PB = C1 + 1;
  mp_layer<C1, RB>(A, pa, k0, w0, b0, Bf, PB, wave, ql, h);
  __syncthreads();
  mp_layer<C2, RB>(Bf, PB, C1, w1, b1, A, pa, wave, ql, h);
  __syncthreads();
  // ---- the last convolution, pooled: column maxima over the tile's rows (max and relu(. + bias) commute)
  constexpr int NB = C3 / 32 / NW;
  int loff[NB];
  mp_f32x16 acc[RB][NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    loff[i] = (h * C3 + (wave + NW * i) * 32 + ql) * 8;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][i][r] = 0.f;
  }
  mp_mm<C3, NB, RB>(A + ql * pa + h, 32 * pa, C2 >> 4, w2, loff, acc);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    float mx = acc[0][i][0];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[rb][i][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));  // the other half of the wave holds the other 16 rows
    const int ch = (wave + NW * i) * 32 + ql;
    if (h == 0) po[ch] = fmaxf(mx + b2[ch], 0.f);
  }
}

template <int C1, int C2, int C3, int RB>
__global__ __launch_bounds__(512) void mlp3_pool_kernel(int n, int k0, const float* __restrict__ x, const float* __restrict__ w0,
                                                        const float* __restrict__ b0, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, float* __restrict__ partial) {
  constexpr int NW = 8;
  static_assert(C1 % 32 == 0 && C2 % 256 == 0 && C3 % 256 == 0, "blocks of 32 channels; the two wide layers fill all eight waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int pa = max((k0 + 15) & ~15, C2) | 1;  // odd row pitch (k0 and C2 are even)
  constexpr int TR = 32 * RB;                 // rows per tile
  float* A = reinterpret_cast<float*>(smem);  // [TR][pa]: X, then H2
  float* Bf = A + TR * pa;                    // [TR][C1 + 1]: H1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, ql = lane & 31;
  const int tile = blockIdx.x, cloud = blockIdx.y;
  // ---- the tile's rows (a row beyond the cloud repeats its last point: no maximum changes)
  {
    const int q4 = k0 >> 2;
    const float4* xc = reinterpret_cast<const float4*>(x + (size_t)cloud * n * k0);
    for (int r = wave; r < TR; r += NW) {
      const int row = min(tile * TR + r, n - 1);
      for (int q = lane; q < q4; q += 64) {
        const float4 v = xc[(size_t)row * q4 + q];
        float* d = A + r * pa + 4 * q;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
      // the contraction of layer 0 runs to the next multiple of 16 (zero weights there): finite operands
      if (lane < ((k0 + 15) & ~15) - k0) A[r * pa + k0 + lane] = 0.f;
    }
  }
  __syncthreads();
  mlp3_tile<C1, C2, C3, RB>(A, pa, Bf, k0, w0, b0, w1, b1, w2, b2, partial + ((size_t)cloud * gridDim.x + tile) * C3, wave, ql, h);
}

// ---- The classifier's layer 1 tail (cells.hip: sa_tail_kernel, w = 9 skip columns, cb = 32, C = 128) in front of layer3_1
// (mlp 128, 256, 512), one launch: what the tail writes is exactly what the group-all module reads, 64 rows at a time, so the
// [0 | xyz | out] table never goes through memory (17 MB written and read back per forward of 64 clouds) and the tail's own
// launch -- a single wave of workgroups whose time is one workgroup's chain of round trips -- disappears.
// Per 64-row tile of one cloud, eight waves: the rows of after / skip / att are staged TRANSPOSED, two 32-row blocks side by
// side in the tail's own layout (xs[k * 33 + row]); wave w runs tail stage 1 and then stage 2 for channel block w & 3 of row
// block w >> 2 through tail_product itself (sa_tail.hpp: bias as the initial accumulator, k in ascending pairs -- the bits of
// the separate launch); stage 2's D tile goes straight to columns 4.. of the tile's X rows, whose columns 0..3 = [0 | xyz]
// were staged with the rest; `out` rows are stored from X (coalesced, rows past the cloud masked) and the three convolutions
// follow as in mlp3_pool_kernel.  A row past the cloud repeats the cloud's last point in EVERY staged table, so its X row
// repeats the last row and no maximum changes.  LDS: X [64][257] and behind it the tail's tiles, which H1 [64][129] reuses.
constexpr int TG_C = 128, TG_W = 9, TG_CB = 32, TG_K0 = TG_C + 4, TG_C2 = 256, TG_C3 = 512, TG_TR = 64;
constexpr int TG_PA = (((TG_K0 + 15) & ~15) > TG_C2 ? ((TG_K0 + 15) & ~15) : TG_C2) | 1;
constexpr int TG_TAIL_FLOATS = 2 * (TG_C + 32 + 32) * 33;  // V^T, S^T, N^T of two row blocks (S and N padded to 32 channels)
constexpr int TG_H1_FLOATS = TG_TR * (TG_C + 1);
constexpr size_t TG_LDS_BYTES = ((size_t)TG_TR * TG_PA + (TG_TAIL_FLOATS > TG_H1_FLOATS ? TG_TAIL_FLOATS : TG_H1_FLOATS)) * sizeof(float);
static_assert(TG_LDS_BYTES <= LDS_MAX_BYTES, "X rows + the tail's tiles fit one workgroup's LDS");
static_assert(TG_W <= 2 * TAIL_KS && TG_CB == 2 * TAIL_KS && TG_C % 64 == 0 && TG_C / 32 * 2 == 8, "one (channel block, row block) per wave");

__global__ __launch_bounds__(512) void tail_group_all_kernel(int n, const float* __restrict__ after, const float* __restrict__ S,
                                                             const float* __restrict__ N, const float* __restrict__ Ws,
                                                             const float* __restrict__ bs, const float* __restrict__ Wb,
                                                             const float* __restrict__ bb, const float* __restrict__ Wagg,
                                                             const float* __restrict__ bagg, const float* __restrict__ xyz3,
                                                             const float* __restrict__ w0, const float* __restrict__ b0,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             float* __restrict__ out, float* __restrict__ partial) {
  constexpr int C = TG_C, pa = TG_PA, RPW = TG_TR / 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* A = reinterpret_cast<float*>(smem);  // [64][pa]: X = [0 | xyz | O | zeros to 144], then H2
  float* Bf = A + TG_TR * pa;                 // the tail's tiles, then H1 [64][C + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const int tile = blockIdx.x, cloud = blockIdx.y;
  const long cloud0 = (long)cloud * n;
  const int rb = wave >> 2;                    // the row block this wave stages 8 rows of -- and computes a channel block of
  float* vt = Bf + rb * (C * 33);              // [C][33]   V^T of the row block
  float* st = Bf + 2 * C * 33 + rb * (32 * 33);        // [32][33]  S^T, zero beyond w
  float* nt_ = Bf + 2 * (C + 32) * 33 + rb * (32 * 33);  // [32][33]  N^T
  // ---- the tile's rows, every request before the first write (one round trip); lanes 0-31 take S, lanes 32-63 take N
  {
    float v[3][RPW], cx[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const long row = cloud0 + min(tile * TG_TR + wave * RPW + i, n - 1);
      v[0][i] = after[row * C + lane];
      v[1][i] = after[row * C + 64 + lane];
      v[2][i] = h ? N[row * TG_CB + l32] : S[row * TG_W + min(l32, TG_W - 1)];
      cx[i] = xyz3[row * 3 + max(min(lane, 3) - 1, 0)];
    }
    __builtin_amdgcn_sched_barrier(0);
    const int rr0 = (wave & 3) * RPW;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      vt[lane * 33 + rr0 + i] = v[0][i];
      vt[(64 + lane) * 33 + rr0 + i] = v[1][i];
      (h ? nt_ : st)[l32 * 33 + rr0 + i] = (h || l32 < TG_W) ? v[2][i] : 0.f;
      float* xr = A + (wave * RPW + i) * pa;
      if (lane < 4) xr[lane] = lane ? cx[i] : 0.f;
      else if (lane < 4 + ((TG_K0 + 15) & ~15) - TG_K0) xr[TG_K0 + lane - 4] = 0.f;  // layer 0 contracts to a multiple of 16
    }
  }
  __syncthreads();
  const int cbase = (wave & 3) * 32;
  // ---- tail stage 1: V^T += relu(Ws^T S^T + bs) + relu(Wb^T N^T + bb)
  {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = bs[cbase + kappa(i, h)];
    acc = tail_product(TailW<true>{Ws, C, TG_W, h, cbase + l32}, st, l32, acc);
    f32x16 v;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = fmaxf(acc[i], 0.f);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = bb[cbase + kappa(i, h)];
    acc = tail_product(TailW<true>{Wb, C, TG_CB, h, cbase + l32}, nt_, l32, acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] += fmaxf(acc[i], 0.f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* cell = vt + (cbase + kappa(i, h)) * 33 + l32;
      *cell = *cell + v[i];
    }
  }
  __syncthreads();
  // ---- tail stage 2: O^T = relu(Wagg^T V^T + bagg), the lane's 16 channels of row l32 straight into the tile's X row
  {
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = bagg[cbase + kappa(i, h)];
    o = tail_product(TailW<true>{Wagg, C, C, h, cbase + l32}, vt, l32, o);
    float* xr = A + (rb * 32 + l32) * pa + 4 + cbase;
#pragma unroll
    for (int i = 0; i < 16; ++i) xr[kappa(i, h)] = fmaxf(o[i], 0.f);
  }
  __syncthreads();  // X is complete, and every wave has read V^T: H1 may overwrite the tail's tiles
  // ---- the layer's output rows (128-byte pieces; the stores drain behind layer 0's products)
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int r = wave * RPW + i, row = tile * TG_TR + r;
    if (row < n) {
      float* o = out + (cloud0 + row) * C;
      o[lane] = A[r * pa + 4 + lane];
      o[64 + lane] = A[r * pa + 4 + 64 + lane];
    }
  }
  mlp3_tile<TG_C, TG_C2, TG_C3, 2>(A, pa, Bf, TG_K0, w0, b0, w1, b1, w2, b2, partial + ((size_t)cloud * gridDim.x + tile) * TG_C3, wave, l32, h);
}

// ---- The classifier's layer 2 tail (sa_tail_kernel<8>, w = 134 skip columns, cb = 64, C = 256) and the first two convolutions
// of layer3_2 (260 -> 256 -> 512) in one launch (pasnl_cls_tail_mlp2).  As three launches -- the tail and two vendor GEMMs of
// 1.1 and 2.1 GFLOP -- each is a single wave of 256 workgroups whose time is one workgroup's chain of round trips, and `out`,
// the [0 | xyz | out] table and H1 go out to memory and come back in between.  Here a workgroup of eight waves owns a tile of 32
// rows of one cloud: the tail as in sa_tail_kernel<8> (wave = channel block, the products are tail_product's: the bits of the
// separate launch), stage 2's D tile straight into the tile's X rows [0 | xyz | O | zeros to 272] in LDS, `out` stored from
// there, then conv0 (X -> H1, LDS) and conv1 (H1 -> H2, stored with ReLU for the third convolution, which stays the vendor's
// GEMM -- at 8192 rows its 8.6 GFLOP ran faster there than in mlp3_pool_kernel -- followed by the pooling pass).
// LDS: X [32][273], behind it the tail's tiles V^T [256][33], S^T [160][33], N^T [64][33], which H1 [32][257] reuses.
constexpr int T2_C = 256, T2_W = 134, T2_CB = 64, T2_K0 = T2_C + 4, T2_C1 = 256, T2_C2 = 512, T2_TR = 32;
constexpr int T2_K0P = (T2_K0 + 15) & ~15;
constexpr int T2_PA = T2_K0P | 1;
constexpr int T2_WP = (T2_W + 2 * TAIL_KS - 1) & ~(2 * TAIL_KS - 1);
constexpr int T2_TAIL_FLOATS = (T2_C + T2_WP + T2_CB) * 33;
constexpr int T2_H1_FLOATS = T2_TR * (T2_C1 + 1);
constexpr size_t T2_LDS_BYTES = ((size_t)T2_TR * T2_PA + (T2_TAIL_FLOATS > T2_H1_FLOATS ? T2_TAIL_FLOATS : T2_H1_FLOATS)) * sizeof(float);
static_assert(T2_LDS_BYTES <= LDS_MAX_BYTES, "X rows + the tail's tiles fit one workgroup's LDS");
static_assert(T2_C == 8 * 32 && T2_C1 == 8 * 32 && T2_C2 % 256 == 0 && T2_C % 64 == 0 && T2_CB == 64 && T2_WP <= 192 && T2_K0P - T2_K0 <= 60,
              "one channel block per wave; the staging's segment counts");

__global__ __launch_bounds__(512) void tail_mlp2_kernel(int n, const float* __restrict__ after, const float* __restrict__ S,
                                                        const float* __restrict__ N, const float* __restrict__ Ws,
                                                        const float* __restrict__ bs, const float* __restrict__ Wb,
                                                        const float* __restrict__ bb, const float* __restrict__ Wagg,
                                                        const float* __restrict__ bagg, const float* __restrict__ xyz3,
                                                        const float* __restrict__ w0, const float* __restrict__ b0,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        float* __restrict__ out, float* __restrict__ h2) {
  constexpr int C = T2_C, pa = T2_PA, RPW = T2_TR / 8, SA = C / 64, SS = (T2_WP + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* A = reinterpret_cast<float*>(smem);  // [32][pa]: X = [0 | xyz | O | zeros to 272]
  float* Bf = A + T2_TR * pa;                 // the tail's tiles, then H1 [32][C1 + 1]
  float* vt = Bf;                             // [C][33]   V^T
  float* st = vt + C * 33;                    // [WP][33]  S^T, zero beyond w
  float* nt_ = st + T2_WP * 33;               // [CB][33]  N^T
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l32 = lane & 31;
  const int tile = blockIdx.x, cloud = blockIdx.y;
  const long cloud0 = (long)cloud * n;
  // ---- the tile's rows, every request before the first write (one round trip); a row past the cloud repeats its last point
  {
    float va[SA][RPW], vs[SS][RPW], vn[RPW], cx[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const long row = cloud0 + min(tile * T2_TR + wave * RPW + i, n - 1);
#pragma unroll
      for (int s = 0; s < SA; ++s) va[s][i] = after[row * C + s * 64 + lane];
#pragma unroll
      for (int s = 0; s < SS; ++s) vs[s][i] = S[row * T2_W + min(s * 64 + lane, T2_W - 1)];
      vn[i] = N[row * T2_CB + lane];
      cx[i] = xyz3[row * 3 + max(min(lane, 3) - 1, 0)];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
#pragma unroll
      for (int s = 0; s < SA; ++s) vt[(s * 64 + lane) * 33 + r] = va[s][i];
#pragma unroll
      for (int s = 0; s < SS; ++s) {
        const int c = s * 64 + lane;
        if (c < T2_WP) st[c * 33 + r] = c < T2_W ? vs[s][i] : 0.f;
      }
      nt_[lane * 33 + r] = vn[i];
      float* xr = A + r * pa;
      if (lane < 4) xr[lane] = lane ? cx[i] : 0.f;
      else if (lane < 4 + T2_K0P - T2_K0) xr[T2_K0 + lane - 4] = 0.f;  // conv0 contracts to a multiple of 16
    }
  }
  __syncthreads();
  const int cbase = wave * 32;
  // ---- tail stage 1: V^T += relu(Ws^T S^T + bs) + relu(Wb^T N^T + bb)
  {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = bs[cbase + kappa(i, h)];
    acc = tail_product(TailW<true>{Ws, C, T2_W, h, cbase + l32}, st, l32, acc);
    f32x16 v;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = fmaxf(acc[i], 0.f);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = bb[cbase + kappa(i, h)];
    acc = tail_product(TailW<true>{Wb, C, T2_CB, h, cbase + l32}, nt_, l32, acc);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] += fmaxf(acc[i], 0.f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* cell = vt + (cbase + kappa(i, h)) * 33 + l32;
      *cell = *cell + v[i];
    }
  }
  __syncthreads();
  // ---- tail stage 2: O^T = relu(Wagg^T V^T + bagg), the lane's 16 channels of row l32 straight into the tile's X row
  {
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = bagg[cbase + kappa(i, h)];
    o = tail_product(TailW<true>{Wagg, C, C, h, cbase + l32}, vt, l32, o);
    float* xr = A + l32 * pa + 4 + cbase;
#pragma unroll
    for (int i = 0; i < 16; ++i) xr[kappa(i, h)] = fmaxf(o[i], 0.f);
  }
  __syncthreads();  // X is complete, and every wave has read V^T: H1 may overwrite the tail's tiles
  // ---- the layer's output rows (256-byte pieces; the stores drain behind conv0's products)
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int r = wave * RPW + i, row = tile * T2_TR + r;
    if (row < n) {
      float* o = out + (cloud0 + row) * C;
#pragma unroll
      for (int s = 0; s < SA; ++s) o[s * 64 + lane] = A[r * pa + 4 + s * 64 + lane];
    }
  }
  mp_layer<T2_C1, 1>(A, pa, T2_K0, w0, b0, Bf, T2_C1 + 1, wave, l32, h);
  __syncthreads();
  mp_layer<T2_C2, 1>(Bf, T2_C1 + 1, T2_C1, w1, b1, h2 + (cloud0 + (long)tile * T2_TR) * T2_C2, T2_C2, wave, l32, h, n - tile * T2_TR);
}

// W (K, N) row-major -> P[bt][h][n][u] = W[16 bt + 2 u + h][n] (zero beyond K): one thread per 16-byte piece
__global__ __launch_bounds__(256) void mlp3_pack_kernel(int K, int N, const float* __restrict__ W, float* __restrict__ P) {
  const long total = (long)((K + 15) >> 4) * 2 * N * 2;  // 16-byte pieces
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int half = (int)(e & 1);
    const long lane = e >> 1;  // (bt * 2 + h) * N + n
    const int n = (int)(lane % N);
    const long bh = lane / N;
    const int h = (int)(bh & 1), bt = (int)(bh >> 1);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * bt + 2 * (4 * half + j) + h;
      v[j] = k < K ? W[(size_t)k * N + n] : 0.f;
    }
    reinterpret_cast<float4*>(P)[e] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

template <int C1, int C2, int C3, int RB>
static int mlp3_launch(int b, int n, int k0, const float* x, const float* w0, const float* b0, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* partial, hipStream_t st) {
  const int k0p = (k0 + 15) & ~15;
  const int pa = (k0p > C2 ? k0p : C2) | 1;
  const size_t lds = ((size_t)32 * RB * pa + (size_t)32 * RB * (C1 + 1)) * sizeof(float);
  if (lds > LDS_MAX_BYTES) return PASNL_EUNSUPPORTED;
  if (launch(mlp3_pool_kernel<C1, C2, C3, RB>, dim3((n + 32 * RB - 1) / (32 * RB), b), dim3(512), lds, st, n, k0, x, w0, b0, w1, b1,
             w2, b2, partial) != PASNL_OK)
    return PASNL_ELAUNCH;
  return pasnl_launch_status();
}

}  // namespace pasnl

using namespace pasnl;

extern "C" size_t pasnl_mlp3_max_pool_workspace_bytes(int b, int n, int c3) {
  if (b <= 0 || n <= 0 || c3 <= 0) return 0;
  return (size_t)b * ((n + 31) / 32) * c3 * sizeof(float);
}

extern "C" size_t pasnl_mlp3_packed_weights_bytes(int k, int n) {
  if (k <= 0 || n <= 0) return 0;
  return (size_t)((k + 15) & ~15) * n * sizeof(float);
}

extern "C" int pasnl_mlp3_pack_weights(int k, int n, const float* w, float* packed, pasnl_stream_t stream) {
  PASNL_REQUIRE(k > 0 && n > 0, PASNL_EINVAL);
  PASNL_REQUIRE(w && packed, PASNL_ENULL);
  PASNL_REQUIRE(reinterpret_cast<uintptr_t>(packed) % 16 == 0, PASNL_EUNSUPPORTED);
  const long pieces = (long)((k + 15) >> 4) * 4 * n;
  const long g = (pieces + 255) / 256;
  hipLaunchKernelGGL(mlp3_pack_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, pasnl_hip_stream(stream), k, n, w, packed);
  return pasnl_launch_status();
}

extern "C" int pasnl_mlp3_max_pool(int b, int n, int k0, int c1, int c2, int c3, const float* x, const float* w0, const float* b0,
                                   const float* w1, const float* b1, const float* w2, const float* b2, float* out, long out_stride,
                                   void* workspace, size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && k0 > 0 && c1 > 0 && c2 > 0 && c3 > 0 && out_stride >= c3, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(x && w0 && b0 && w1 && b1 && w2 && b2 && out && workspace, PASNL_ENULL);
  PASNL_REQUIRE(workspace_bytes >= pasnl_mlp3_max_pool_workspace_bytes(b, n, c3), PASNL_EWORKSPACE);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  // rows read in 16-byte pieces; an even contraction length per MFMA step pair
  PASNL_REQUIRE(k0 % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2)) % 16 == 0,
                PASNL_EUNSUPPORTED);  // (packed weights: read in 16-byte pieces)
  hipStream_t st = pasnl_hip_stream(stream);
  float* partial = static_cast<float*>(workspace);
  int rc;
  int tr;  // rows per tile: two row blocks where the activations of 64 rows fit the LDS (every weight then feeds two products)
  if (c1 == 128 && c2 == 256 && c3 == 512) { tr = 64; rc = mlp3_launch<128, 256, 512, 2>(b, n, k0, x, w0, b0, w1, b1, w2, b2, partial, st); }
  else if (c1 == 256 && c2 == 512 && c3 == 1024) { tr = 32; rc = mlp3_launch<256, 512, 1024, 1>(b, n, k0, x, w0, b0, w1, b1, w2, b2, partial, st); }
  else return PASNL_EUNSUPPORTED;
  if (rc != PASNL_OK) return rc;
  // maxima over the tiles of a cloud -> out[cloud * out_stride + channel]
  return pasnl_max_pool_rows_strided(b, (n + tr - 1) / tr, c3, partial, out, out_stride, stream);
}

extern "C" int pasnl_cls_tail_group_all(int b, int n, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                                        const float* ws_packed, const float* bs, const float* wb_packed, const float* bb,
                                        const float* wagg_packed, const float* bagg, const float* new_xyz, int c1, int c2, int c3,
                                        const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                        const float* b2, float* out, float* pooled, long pooled_stride, void* workspace,
                                        size_t workspace_bytes, pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && w > 0 && cb > 0 && c > 0 && c1 > 0 && c2 > 0 && c3 > 0 && pooled_stride >= c3, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(after && skip_max && att && ws_packed && bs && wb_packed && bb && wagg_packed && bagg && new_xyz, PASNL_ENULL);
  PASNL_REQUIRE(w0 && b0 && w1 && b1 && w2 && b2 && out && pooled && workspace, PASNL_ENULL);
  PASNL_REQUIRE(workspace_bytes >= pasnl_mlp3_max_pool_workspace_bytes(b, n, c3), PASNL_EWORKSPACE);
  PASNL_REQUIRE(w == TG_W && cb == TG_CB && c == TG_C && c1 == TG_C && c2 == TG_C2 && c3 == TG_C3, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(ws_packed) | reinterpret_cast<uintptr_t>(wb_packed) | reinterpret_cast<uintptr_t>(wagg_packed) |
                 reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2)) % 16 == 0,
                PASNL_EUNSUPPORTED);  // (packed weights: read in 16-byte pieces)
  const int tiles = (n + TG_TR - 1) / TG_TR;
  if (launch(tail_group_all_kernel, dim3(tiles, b), dim3(512), TG_LDS_BYTES, pasnl_hip_stream(stream), n, after, skip_max, att, ws_packed,
             bs, wb_packed, bb, wagg_packed, bagg, new_xyz, w0, b0, w1, b1, w2, b2, out, static_cast<float*>(workspace)) != PASNL_OK)
    return PASNL_ELAUNCH;
  if (pasnl_launch_status() != PASNL_OK) return PASNL_ELAUNCH;
  return pasnl_max_pool_rows_strided(b, tiles, c3, static_cast<const float*>(workspace), pooled, pooled_stride, stream);
}

extern "C" int pasnl_cls_tail_mlp2(int b, int n, int w, int cb, int c, const float* after, const float* skip_max, const float* att,
                                   const float* ws_packed, const float* bs, const float* wb_packed, const float* bb,
                                   const float* wagg_packed, const float* bagg, const float* new_xyz, int c1, int c2, const float* w0,
                                   const float* b0, const float* w1, const float* b1, float* out, float* h2, size_t h2_bytes,
                                   pasnl_stream_t stream) {
  PASNL_REQUIRE(b >= 0 && n > 0 && w > 0 && cb > 0 && c > 0 && c1 > 0 && c2 > 0, PASNL_EINVAL);
  if (b == 0) return PASNL_OK;
  PASNL_REQUIRE(after && skip_max && att && ws_packed && bs && wb_packed && bb && wagg_packed && bagg && new_xyz, PASNL_ENULL);
  PASNL_REQUIRE(w0 && b0 && w1 && b1 && out && h2, PASNL_ENULL);
  PASNL_REQUIRE(w == T2_W && cb == T2_CB && c == T2_C && c1 == T2_C1 && c2 == T2_C2, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE(h2_bytes >= (size_t)b * n * c2 * sizeof(float), PASNL_EWORKSPACE);
  PASNL_REQUIRE(b <= 65535, PASNL_EUNSUPPORTED);
  PASNL_REQUIRE((reinterpret_cast<uintptr_t>(ws_packed) | reinterpret_cast<uintptr_t>(wb_packed) | reinterpret_cast<uintptr_t>(wagg_packed) |
                 reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w1)) % 16 == 0,
                PASNL_EUNSUPPORTED);  // (packed weights: read in 16-byte pieces)
  if (launch(tail_mlp2_kernel, dim3((n + T2_TR - 1) / T2_TR, b), dim3(512), T2_LDS_BYTES, pasnl_hip_stream(stream), n, after, skip_max, att,
             ws_packed, bs, wb_packed, bb, wagg_packed, bagg, new_xyz, w0, b0, w1, b1, out, h2) != PASNL_OK)
    return PASNL_ELAUNCH;
  return pasnl_launch_status();
}
