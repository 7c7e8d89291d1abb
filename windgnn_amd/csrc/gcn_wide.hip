// GraphConvLayer wider than 64 features: max(F_in, F_out) > 64 over a dense adjacency of S <= 64 stations, exact fp32.
//
// Reference: GraphConvLayer(input_dim, output_dim), src/step5_gcn_layer_model.py:6-23 -- forward relu((A X) W + b).  gcn_any.hip
// keeps A, W and the tile in LDS and an [F_in, F_out] accumulator in registers; neither fits past 64.  Here W is streamed in
// [GW_KC][GW_NB] blocks and the weight gradient is a split-K GEMM over all ntiles * S rows.  Every product runs on
// v_mfma_f32_16x16x4_f32 (common.h: mfma16, bitwise an fmaf chain along k); no operand is rounded.
//
//   forward   gcn_wide_fwd_kernel, grid (min(ntiles, 1024), ceil(F_out / 128)): per tile and K chunk of 32 columns of X,
//             P = A X[:, chunk] goes from LDS to LDS and is multiplied into the [64][128] block of out held in registers;
//             bias + ReLU on the way out.  P never reaches HBM.  Reads X once per column block, writes out once.
//             F_out <= 32 (the model's hid -> 13 layer): gcn_wide_fwd_thin_kernel, out = relu(A (X W) + b) -- U = X W over
//             the K chunks in registers, ONE aggregation of 32 columns per tile.
//   backward  V = A^T (dout * [out > 0]) -- gcn_wide_bwd_agg_kernel, grid (min(ntiles, 1024), ceil(F_out / 64)), mask on the way
//             in, per-workgroup column sums of dZ for db.  Then, since A^T (dZ W^T) = (A^T dZ) W^T and (A X)^T dZ = X^T (A^T dZ),
//               dW = X^T V   gemm.hip's exact-fp32 GEMM, split-K partials [splitk][F_in][F_out] summed in a fixed order,
//               dX = V W^T   the same GEMM (skipped when dX == NULL),
//             so ONE aggregation serves both gradients and no P is recomputed.  No floating-point atomics anywhere.
// Rows >= S and columns past a tensor's extent exist as zeros in LDS only.
#include "common.h"

namespace {

constexpr int GW_THREADS = 256;
constexpr int GW_ROWS = 64;                 // the tile's rows, padded: 4 MFMA row tiles
constexpr int GW_KC = 32;                   // columns of X per K chunk
constexpr int GW_NB = 128;                  // columns of out per workgroup (forward)
constexpr int GW_CB = 64;                   // columns of dout per workgroup (backward aggregation)
constexpr int GW_MAXGRID = 1024;            // workgroups along the tiles
// LDS pitches (floats).  An MFMA A-operand read has 16 rows x 4 k per wave: pitch = 4 mod 64 spreads it over 64 banks; a
// B-operand read has 4 k rows x 16 columns: pitch = 16 mod 64 does.
constexpr int GW_LDA = GW_ROWS + 4, GW_LDX = GW_KC + 16, GW_LDP = GW_KC + 4, GW_LDW = GW_NB + 16, GW_LDZ = GW_CB + 16;

// sA[m][k] = A[m][k] (or A[k][m]) for m, k < S, zeros up to 64 x 64
template <bool TRANSPOSE>
__device__ __forceinline__ void gw_load_adj(int S, const float* __restrict__ A, float* sA) {
  for (int i = threadIdx.x; i < GW_ROWS * GW_ROWS; i += GW_THREADS) {
    const int m = i / GW_ROWS, k = i % GW_ROWS;
    float v = 0.f;
    if (m < S && k < S) v = TRANSPOSE ? A[k * S + m] : A[m * S + k];
    sA[m * GW_LDA + k] = v;
  }
}

// One 16 x 16 tile of sA[16 i ..][0 .. ks) times sB[0 .. ks)[16 j ..], ks a multiple of 4
__device__ __forceinline__ f32x4 gw_agg_tile(const float* sA, const float* sB, int ldb, int i, int j, int ks, int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* a = sA + (16 * i + (lane & 15)) * GW_LDA + (lane >> 4);
  const float* b = sB + (lane >> 4) * ldb + 16 * j + (lane & 15);
  for (int k = 0; k < ks; k += 4) acc = mfma16(a[k], b[k * ldb], acc);
  return acc;
}

// The staging of one (tile, K chunk) step of the forward, fetched into registers a step ahead so that the loads fly under the
// previous step's products: GW_XQ values of the tile's X[:, chunk], GW_WQ of W[chunk, block].  Out of extent = 0, never read.
constexpr int GW_XQ = GW_ROWS * GW_KC / GW_THREADS, GW_WQ = GW_KC * GW_NB / GW_THREADS;
__device__ __forceinline__ void gw_fwd_fetch(float (&xr)[GW_XQ], float (&wr)[GW_WQ], int S, int Fi, int Fo, int n0, int t, int k0,
                                             const float* __restrict__ X, const float* __restrict__ W) {
  const int klen = min(GW_KC, Fi - k0);
  const float* x = X + (size_t)t * S * Fi + k0;
  const float* w = W + (size_t)k0 * Fo + n0;
#pragma unroll
  for (int q = 0; q < GW_XQ; ++q) {
    const int i = threadIdx.x + q * GW_THREADS, j = i / GW_KC, c = i % GW_KC;
    xr[q] = (j < S && c < klen) ? x[(size_t)j * Fi + c] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < GW_WQ; ++q) {
    const int i = threadIdx.x + q * GW_THREADS, kk = i / GW_NB, c = i % GW_NB;
    wr[q] = (kk < klen && n0 + c < Fo) ? w[(size_t)kk * Fo + c] : 0.f;
  }
}

__global__ void __launch_bounds__(GW_THREADS) gcn_wide_fwd_kernel(int S, int Fi, int Fo, int ntiles, const float* __restrict__ A,
                                                                 const float* __restrict__ X, const float* __restrict__ W,
                                                                 const float* __restrict__ b, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sA[GW_ROWS * GW_LDA];
  __shared__ __attribute__((aligned(16))) float sX[GW_ROWS * GW_LDX];
  __shared__ __attribute__((aligned(16))) float sP[GW_ROWS * GW_LDP];
  __shared__ __attribute__((aligned(16))) float sW[GW_KC * GW_LDW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrt = (S + 15) >> 4, S4 = (S + 3) & ~3;
  const int n0 = blockIdx.y * GW_NB;
  // The block of out in registers: wave w owns columns [32 w, 32 w + 32) of every row tile -- or, when the block has at most 32
  // live columns (the last block at F_out = 129, say), row tile w alone, so that all four waves multiply
  const bool narrow = Fo - n0 <= 32;
  const int cw = narrow ? 0 : 32 * wave;
  gw_load_adj<false>(S, A, sA);
  float bv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + cw + 16 * j + (lane & 15);
    bv[j] = col < Fo ? b[col] : 0.f;
  }
  const int nch = (Fi + GW_KC - 1) / GW_KC;                       // K chunks per tile
  float xr[GW_XQ], wr[GW_WQ];
  gw_fwd_fetch(xr, wr, S, Fi, Fo, n0, blockIdx.x, 0, X, W);
  f32x4 acc[4][2];
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {          // tiles of this workgroup
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nch; ++ch) {                            // K chunks
      const int k0 = ch * GW_KC;
      const int klen = min(GW_KC, Fi - k0), k4 = (klen + 3) & ~3, ncj = (klen + 15) >> 4;
      __syncthreads();                                            // A loaded / the previous step's sX, sP, sW no longer read
#pragma unroll
      for (int q = 0; q < GW_XQ; ++q) {
        const int i = threadIdx.x + q * GW_THREADS, j = i / GW_KC, c = i % GW_KC;
        if (j < S4) sX[j * GW_LDX + c] = xr[q];
      }
#pragma unroll
      for (int q = 0; q < GW_WQ; ++q) {
        const int i = threadIdx.x + q * GW_THREADS, kk = i / GW_NB, c = i % GW_NB;
        if (kk < k4) sW[kk * GW_LDW + c] = wr[q];
      }
      if (ch + 1 < nch) gw_fwd_fetch(xr, wr, S, Fi, Fo, n0, t, k0 + GW_KC, X, W);           // the next step's operands
      else if (t + (int)gridDim.x < ntiles) gw_fwd_fetch(xr, wr, S, Fi, Fo, n0, t + gridDim.x, 0, X, W);
      __syncthreads();
      // P[:, chunk] = A X[:, chunk]   (src/step5_gcn_layer_model.py:15): the (row tile, column tile) pairs dealt round the waves
      for (int pr = wave; pr < nrt * ncj; pr += GW_THREADS / 64) {
        const int i = pr / ncj, j = pr % ncj;
        const f32x4 p = gw_agg_tile(sA, sX, GW_LDX, i, j, S4, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[(16 * i + 4 * (lane >> 4) + r) * GW_LDP + 16 * j + (lane & 15)] = p[r];
      }
      __syncthreads();
      // out block += P[:, chunk] W[chunk, block]   (:18)
      for (int kk = 0; kk < k4; kk += 4) {
        float wv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) wv[j] = sW[(kk + (lane >> 4)) * GW_LDW + cw + 16 * j + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rt = narrow ? wave : i;
          if (narrow ? (i == 0 && wave < nrt) : (i < nrt)) {
            const float pv = sP[(16 * rt + (lane & 15)) * GW_LDP + kk + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(pv, wv[j], acc[i][j]);
          }
        }
      }
    }
    float* o = out + (size_t)t * S * Fo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rt = narrow ? wave : i;
      if (narrow && i > 0) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + cw + 16 * j + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + 4 * (lane >> 4) + r;
          if (row < S && col < Fo) {                               // relu(. + b)   (:18, :21)
            const float z = acc[i][j][r] + bv[j];
            o[(size_t)row * Fo + col] = z > 0.f ? z : 0.f;
          }
        }
      }
    }
  }
}

// The forward for F_out <= GW_TB, the model's hid -> 13 layer: out = relu(A (X W) + b), the other association.  U = X W is
// accumulated over the K chunks in registers (wave w owns row tile w), so the aggregation runs once per tile on GW_TB columns
// instead of once per chunk on all of X's -- S S F_out instead of S S F multiply-adds -- and a chunk costs two barriers.
constexpr int GW_TB = 32;                                         // columns of the thin forward's one block
constexpr int GW_LDXT = GW_KC + 4, GW_LDWT = GW_TB + 16, GW_LDU = GW_TB + 16;   // X as an A operand; W and U as B operands
constexpr int GW_WQT = GW_KC * GW_TB / GW_THREADS;
__device__ __forceinline__ void gw_thin_fetch(float (&xr)[GW_XQ], float (&wr)[GW_WQT], int S, int Fi, int Fo, int t, int k0,
                                              const float* __restrict__ X, const float* __restrict__ W) {
  const int klen = min(GW_KC, Fi - k0);
  const float* x = X + (size_t)t * S * Fi + k0;
  const float* w = W + (size_t)k0 * Fo;
#pragma unroll
  for (int q = 0; q < GW_XQ; ++q) {
    const int i = threadIdx.x + q * GW_THREADS, j = i / GW_KC, c = i % GW_KC;
    xr[q] = (j < S && c < klen) ? x[(size_t)j * Fi + c] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < GW_WQT; ++q) {
    const int i = threadIdx.x + q * GW_THREADS, kk = i / GW_TB, c = i % GW_TB;
    wr[q] = (kk < klen && c < Fo) ? w[(size_t)kk * Fo + c] : 0.f;
  }
}

__global__ void __launch_bounds__(GW_THREADS) gcn_wide_fwd_thin_kernel(int S, int Fi, int Fo, int ntiles,
                                                                      const float* __restrict__ A, const float* __restrict__ X,
                                                                      const float* __restrict__ W, const float* __restrict__ b,
                                                                      float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sA[GW_ROWS * GW_LDA];
  __shared__ __attribute__((aligned(16))) float sX[GW_ROWS * GW_LDXT];
  __shared__ __attribute__((aligned(16))) float sW[GW_KC * GW_LDWT];
  __shared__ __attribute__((aligned(16))) float sU[GW_ROWS * GW_LDU];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrt = (S + 15) >> 4, S4 = (S + 3) & ~3, ncj = (Fo + 15) >> 4;
  gw_load_adj<false>(S, A, sA);
  const int nch = (Fi + GW_KC - 1) / GW_KC;                       // K chunks per tile
  float xr[GW_XQ], wr[GW_WQT];
  gw_thin_fetch(xr, wr, S, Fi, Fo, blockIdx.x, 0, X, W);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {          // tiles of this workgroup
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int ch = 0; ch < nch; ++ch) {                            // K chunks
      const int k0 = ch * GW_KC;
      const int k4 = (min(GW_KC, Fi - k0) + 3) & ~3;
      __syncthreads();                                            // A loaded / the previous step's sX, sW, sU no longer read
#pragma unroll
      for (int q = 0; q < GW_XQ; ++q) {                           // all 64 rows: rows >= S are zeros, so U's are
        const int i = threadIdx.x + q * GW_THREADS;
        sX[(i / GW_KC) * GW_LDXT + i % GW_KC] = xr[q];
      }
#pragma unroll
      for (int q = 0; q < GW_WQT; ++q) {
        const int i = threadIdx.x + q * GW_THREADS;
        sW[(i / GW_TB) * GW_LDWT + i % GW_TB] = wr[q];
      }
      if (ch + 1 < nch) gw_thin_fetch(xr, wr, S, Fi, Fo, t, k0 + GW_KC, X, W);              // the next step's operands
      else if (t + (int)gridDim.x < ntiles) gw_thin_fetch(xr, wr, S, Fi, Fo, t + gridDim.x, 0, X, W);
      __syncthreads();
      if (wave < nrt)                                             // U[row tile w] += X[row tile w, chunk] W[chunk, :]
        for (int kk = 0; kk < k4; kk += 4) {
          const float xv = sX[(16 * wave + (lane & 15)) * GW_LDXT + kk + (lane >> 4)];
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j] = mfma16(xv, sW[(kk + (lane >> 4)) * GW_LDWT + 16 * j + (lane & 15)], acc[j]);
        }
    }
    if (wave < nrt) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sU[(16 * wave + 4 * (lane >> 4) + r) * GW_LDU + 16 * j + (lane & 15)] = acc[j][r];
    }
    __syncthreads();
    float* o = out + (size_t)t * S * Fo;
    for (int pr = wave; pr < nrt * ncj; pr += GW_THREADS / 64) {  // out = relu(A U + b): the (row, column) tile pairs
      const int i = pr / ncj, j = pr % ncj;
      const f32x4 z = gw_agg_tile(sA, sU, GW_LDU, i, j, S4, lane);
      const int col = 16 * j + (lane & 15);
      const float bv = col < Fo ? b[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * i + 4 * (lane >> 4) + r;
        if (row < S && col < Fo) {
          const float v = z[r] + bv;
          o[(size_t)row * Fo + col] = v > 0.f ? v : 0.f;
        }
      }
    }
  }
}

// One tile's share of dZ = dout * [out > 0] per thread, fetched a tile ahead
constexpr int GW_ZQ = GW_ROWS * GW_CB / GW_THREADS;
__device__ __forceinline__ void gw_bwd_fetch(float (&zr)[GW_ZQ], int S, int Fo, int c0, int clen, int t,
                                             const float* __restrict__ out, const float* __restrict__ dout) {
  const size_t base = (size_t)t * S * Fo + c0;
  float o[GW_ZQ];
#pragma unroll
  for (int q = 0; q < GW_ZQ; ++q) {
    const int i = threadIdx.x + q * GW_THREADS, s = i / GW_CB, c = i % GW_CB;
    const bool in = s < S && c < clen;
    o[q] = in ? out[base + (size_t)s * Fo + c] : 0.f;
    zr[q] = in ? dout[base + (size_t)s * Fo + c] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < GW_ZQ; ++q) zr[q] = o[q] > 0.f ? zr[q] : 0.f;
}

// V[n] = A^T dZ[n], dZ = dout * [out > 0]; dbpart[blockIdx.x][f] = the workgroup's sum of dZ[.][f] over its tiles
__global__ void __launch_bounds__(GW_THREADS) gcn_wide_bwd_agg_kernel(int S, int Fo, int ntiles, const float* __restrict__ A,
                                                                     const float* __restrict__ out,
                                                                     const float* __restrict__ dout, float* __restrict__ V,
                                                                     float* __restrict__ dbpart) {
  __shared__ __attribute__((aligned(16))) float sA[GW_ROWS * GW_LDA];
  __shared__ __attribute__((aligned(16))) float sZ[GW_ROWS * GW_LDZ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrt = (S + 15) >> 4, S4 = (S + 3) & ~3;
  const int c0 = blockIdx.y * GW_CB;
  const int clen = min(GW_CB, Fo - c0), ncj = (clen + 15) >> 4;
  gw_load_adj<true>(S, A, sA);
  float accb = 0.f;                                               // thread c < clen owns db[c0 + c]
  float zr[GW_ZQ];
  gw_bwd_fetch(zr, S, Fo, c0, clen, blockIdx.x, out, dout);
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {          // tiles of this workgroup
    const size_t base = (size_t)t * S * Fo + c0;
    __syncthreads();                                              // A^T loaded / the previous tile's sZ no longer read
#pragma unroll
    for (int q = 0; q < GW_ZQ; ++q) {
      const int i = threadIdx.x + q * GW_THREADS, s = i / GW_CB, c = i % GW_CB;
      if (s < S4) sZ[s * GW_LDZ + c] = zr[q];
    }
    if (t + (int)gridDim.x < ntiles) gw_bwd_fetch(zr, S, Fo, c0, clen, t + gridDim.x, out, dout);   // the next tile's
    __syncthreads();
    if ((int)threadIdx.x < clen)
      for (int s = 0; s < S; ++s) accb += sZ[s * GW_LDZ + threadIdx.x];
    for (int pr = wave; pr < nrt * ncj; pr += GW_THREADS / 64) {  // the (row tile, column tile) pairs dealt round the waves
      const int i = pr / ncj, j = pr % ncj;
      const f32x4 v = gw_agg_tile(sA, sZ, GW_LDZ, i, j, S4, lane);
      const int col = 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * i + 4 * (lane >> 4) + r;
        if (row < S && col < clen) V[base + (size_t)row * Fo + col] = v[r];
      }
    }
  }
  if ((int)threadIdx.x < clen) dbpart[(size_t)blockIdx.x * Fo + c0 + threadIdx.x] = accb;
}

// dst[i] = sum_r partial[r][i] in a fixed order: the split-K partials of dW, the per-workgroup partials of db.  16 outputs a
// workgroup; thread (q, c) adds rows q, q + 16, ... of output c in ascending order, then thread (0, c) the 16 sums in ascending q
constexpr int GW_SUM_COLS = 16, GW_SUM_ROWS = 16;
__global__ void __launch_bounds__(GW_SUM_COLS * GW_SUM_ROWS) gcn_wide_sum_kernel(const float* __restrict__ partial, int rows, int n,
                                                                                float* __restrict__ dst) {
  __shared__ float red[GW_SUM_ROWS][GW_SUM_COLS + 1];
  const int c = threadIdx.x % GW_SUM_COLS, q = threadIdx.x / GW_SUM_COLS;
  const size_t i = (size_t)blockIdx.x * GW_SUM_COLS + c;
  float s = 0.f;
  if (i < (size_t)n)
    for (int r = q; r < rows; r += GW_SUM_ROWS) s += partial[(size_t)r * n + i];
  red[q][c] = s;
  __syncthreads();
  if (q == 0 && i < (size_t)n) {
    float tot = red[0][c];
#pragma unroll
    for (int r = 1; r < GW_SUM_ROWS; ++r) tot += red[r][c];
    dst[i] = tot;
  }
}

int gw_grid(int ntiles) { return ntiles < GW_MAXGRID ? ntiles : GW_MAXGRID; }

// Split-K factor of dW = X^T V over rows = ntiles * S: about 1024 workgroups in all, chunks of at least 64 rows
int gw_splitk(int ntiles, int S, int Fi, int Fo) {
  const int64_t rows = (int64_t)ntiles * S;
  const int tiles = gemm_f32_tiles(Fi, Fo);
  int64_t sk = (1024 + tiles - 1) / tiles;
  if (sk > rows / 64) sk = rows / 64;
  return sk < 1 ? 1 : (int)sk;
}

// workspace regions, each a multiple of 64 floats (256 bytes): V [rows][Fo] | dbpart [grid][Fo] | dW partials [splitk][Fi][Fo]
struct GwPlan { size_t v, dbpart, dwpart, total; };
GwPlan gw_plan(int ntiles, int S, int Fi, int Fo) {
  GwPlan p;
  p.v = 0;
  p.dbpart = p.v + align_up((size_t)ntiles * S * Fo, 64);
  p.dwpart = p.dbpart + align_up((size_t)gw_grid(ntiles) * Fo, 64);
  p.total = p.dwpart + align_up((size_t)gw_splitk(ntiles, S, Fi, Fo) * Fi * Fo, 64);
  return p;
}

}  // namespace

bool gcn_wide_supported(int S, int Fi, int Fo) { return S >= 1 && S <= GW_ROWS && Fi >= 1 && Fo >= 1 && (Fi > 64 || Fo > 64); }
// what the kernels index with 32-bit integers or hand to gemm.hip as int extents
bool gcn_wide_countable(int ntiles, int S, int Fi, int Fo) {
  const int64_t lim = 1ll << 31;
  return (int64_t)ntiles * S * (Fi > Fo ? Fi : Fo) < lim && (int64_t)Fi * Fo < lim;
}
size_t gcn_wide_bwd_ws_floats(int ntiles, int S, int Fi, int Fo) { return gw_plan(ntiles, S, Fi, Fo).total; }

int launch_gcn_wide_fwd(int ntiles, int S, int Fi, int Fo, const float* A, const float* X, const float* W, const float* b,
                        float* out, hipStream_t st) {
  if (Fo <= GW_TB) {
    PROF_LAUNCH("gcn_wide_fwd_thin_kernel", (double)ntiles * (2.0 * S * S * Fo + 2.0 * S * Fi * Fo), 4.0 * ntiles * S * ((double)Fi + Fo),
                st, hipLaunchKernelGGL(gcn_wide_fwd_thin_kernel, dim3(gw_grid(ntiles)), dim3(GW_THREADS), 0, st, S, Fi, Fo, ntiles, A,
                                       X, W, b, out));
    WGNN_CHECK_LAUNCH();
    return WGNN_OK;
  }
  const int nb = cdiv_i(Fo, GW_NB);
  PROF_LAUNCH("gcn_wide_fwd_kernel", (double)ntiles * nb * 2.0 * S * S * Fi + (double)ntiles * 2.0 * S * Fi * Fo,
              4.0 * ntiles * S * ((double)Fi * nb + Fo), st,
              hipLaunchKernelGGL(gcn_wide_fwd_kernel, dim3(gw_grid(ntiles), nb), dim3(GW_THREADS), 0, st, S, Fi, Fo, ntiles, A, X,
                                 W, b, out));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

int launch_gcn_wide_bwd(int ntiles, int S, int Fi, int Fo, const float* A, const float* X, const float* W, const float* out,
                        const float* dout, float* dW, float* db, float* dX, float* ws, hipStream_t st) {
  const GwPlan pl = gw_plan(ntiles, S, Fi, Fo);
  const int rows = ntiles * S, grid = gw_grid(ntiles), sk = gw_splitk(ntiles, S, Fi, Fo);
  float* V = ws + pl.v;
  float* dbpart = ws + pl.dbpart;
  float* dwpart = ws + pl.dwpart;
  PROF_LAUNCH("gcn_wide_bwd_agg_kernel", (double)ntiles * 2.0 * S * S * Fo, 12.0 * rows * (double)Fo, st,
              hipLaunchKernelGGL(gcn_wide_bwd_agg_kernel, dim3(grid, cdiv_i(Fo, GW_CB)), dim3(GW_THREADS), 0, st, S, Fo, ntiles, A,
                                 out, dout, V, dbpart));
  WGNN_CHECK_LAUNCH();
  PROF_LAUNCH("gcn_wide_sum_kernel", 0.0, 4.0 * (grid + 1) * (double)Fo, st,
              hipLaunchKernelGGL(gcn_wide_sum_kernel, dim3(cdiv_i(Fo, GW_SUM_COLS)), dim3(GW_SUM_COLS * GW_SUM_ROWS), 0, st, dbpart, grid, Fo,
                                 db));
  WGNN_CHECK_LAUNCH();
  GemmArgs g{};                                                   // dW[f][o] = sum_row X[row][f] V[row][o]
  g.A = X; g.lda = Fi; g.a_kcontig = 0;
  g.B = V; g.ldb = Fo; g.b_kcontig = 0;
  g.C = nullptr; g.ldc = Fo;
  g.M = Fi; g.N = Fo; g.K = rows;
  g.splitk = sk; g.partial = dwpart;
  int rc = launch_gemm_f32(g, st);
  if (rc != WGNN_OK) return rc;
  const int n = Fi * Fo;
  PROF_LAUNCH("gcn_wide_sum_kernel", 0.0, 4.0 * (sk + 1) * (double)n, st,
              hipLaunchKernelGGL(gcn_wide_sum_kernel, dim3((unsigned)(((size_t)n + GW_SUM_COLS - 1) / GW_SUM_COLS)),
                                 dim3(GW_SUM_COLS * GW_SUM_ROWS), 0, st, dwpart, sk, n, dW));
  WGNN_CHECK_LAUNCH();
  if (dX) {                                                       // dX[row][f] = sum_o V[row][o] W[f][o]
    GemmArgs d{};
    d.A = V; d.lda = Fo; d.a_kcontig = 1;
    d.B = W; d.ldb = Fo; d.b_kcontig = 1;
    d.C = dX; d.ldc = Fi;
    d.M = rows; d.N = Fi; d.K = Fo;
    d.splitk = 1; d.partial = nullptr;
    rc = launch_gemm_f32(d, st);
    if (rc != WGNN_OK) return rc;
  }
  return WGNN_OK;
}
