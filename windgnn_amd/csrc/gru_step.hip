// One hour of carried-state inference as ONE launch (wgnn_fwd_state with T = 1): both graph convolutions of the hour's
// [S,13] tile, the GRU input projection, W_hh h0 and the GRU cell.
//
// Reference: GCN_GRU.forward (src/step6_gcn_gru_combined_model.py:13-27) for ONE timestep, with nn.GRU called with the
// caller's hx (:23) -- the forecaster's hourly update: h_t = GRU(relu(A relu(A x_t W1 + b1) W2 + b2), h_{t-1}).
//
// Why VALU and not MFMA: at T = 1 and B <= WGNN_STEP_MAX_B the step multiplies 0.67 MB of GRU weights (S = 34, H = 102) by
// a handful of vectors -- a matrix-VECTOR product, bound by the weight bytes and the latency of one pass over them, not by
// math.  An MFMA tile would be 1/16 .. 1/4 full and would need the fp16 planes of the weights the split modes stage; plain
// fp32 FMA on the weights as the caller passed them is exact fp32 in every math mode and needs no image.
//
// Shape: workgroup (x, y) owns hidden units j = 4 x + wave (gate rows j, H + j, 2H + j of W_ih and W_hh: one unit per wave)
// and windows b = 4 y .. 4 y + 3.  Every workgroup recomputes the tiny GCN of its windows in LDS (A and the tiles staged
// there), so that no workgroup needs another's result: no inter-workgroup communication, no atomics.  A wave streams its
// three W_ih rows once into registers (16-byte loads; rows of S*13 floats start at any 4-byte offset, so each row is split
// into a scalar head up to the next 16-byte boundary, 16-byte body chunks and a scalar tail), issued before the GCN so their
// latency hides under it; the dot products are reduced inside the wave (xor butterfly).
#include "common.h"

namespace {

constexpr int STEP_THREADS = 256;              // 4 waves = 4 hidden units
constexpr int STEP_WB = 4;                     // windows per workgroup
constexpr int STEP_SMAX = 64;                  // dense adjacency bound (LDS)
constexpr int STEP_IW = STEP_SMAX * 13;        // LDS row of one window's [S][13] tile
constexpr int STEP_HMAX = 128;
constexpr int STEP_MC = (STEP_IW / 4 + 63) / 64;   // 16-byte body chunks of a W_ih row per lane (I <= 832: 4)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(STEP_THREADS) gru_step_kernel(int B, int S, int H, const float* __restrict__ A,
                                                                const float* __restrict__ X, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ W2,
                                                                const float* __restrict__ b2, const float* __restrict__ Wih,
                                                                const float* __restrict__ bih, const float* __restrict__ Whh,
                                                                const float* __restrict__ bhh, const float* __restrict__ h0,
                                                                float* __restrict__ Y, float* __restrict__ hn) {
  __shared__ __attribute__((aligned(16))) float As[STEP_SMAX * STEP_SMAX];
  __shared__ __attribute__((aligned(16))) float Xg[STEP_WB * STEP_IW];    // the hour's tiles, later g (layer 2's output)
  __shared__ __attribute__((aligned(16))) float Pb[STEP_WB * STEP_IW];    // A @ In of the current layer
  __shared__ __attribute__((aligned(16))) float H1[STEP_WB * STEP_IW];    // layer 1's output
  __shared__ __attribute__((aligned(16))) float Hs[STEP_WB * STEP_HMAX];  // h0 of the windows (zeros without h0)
  __shared__ float Ws[2][13 * 13 + 13];                                   // W1 | b1, W2 | b2

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.y * STEP_WB;
  const int nw = B - b0 < STEP_WB ? B - b0 : STEP_WB;
  const int I = S * 13;
  const int j = blockIdx.x * (STEP_THREADS / 64) + wave;
  const bool unit = j < H;                                               // wave-uniform

  // ---- stage the GCN operands (A, the tiles, the conv weights) and h0
  for (int e = tid; e < S * S; e += STEP_THREADS) As[e] = A[e];
  for (int e = tid; e < nw * I; e += STEP_THREADS) Xg[(e / I) * STEP_IW + e % I] = X[(size_t)b0 * I + e];
  for (int e = tid; e < 2 * (13 * 13 + 13); e += STEP_THREADS) {
    const int l = e / (13 * 13 + 13), k = e % (13 * 13 + 13);
    Ws[l][k] = k < 169 ? (l ? W2 : W1)[k] : (l ? b2 : b1)[k - 169];
  }
  for (int e = tid; e < STEP_WB * STEP_HMAX; e += STEP_THREADS) {
    const int w = e / STEP_HMAX, k = e % STEP_HMAX;
    Hs[e] = (h0 && w < nw && k < H) ? h0[(size_t)(b0 + w) * H + k] : 0.f;
  }

  // ---- this wave's gate rows, in flight under the GCN
  f32x4 wv[3][STEP_MC];
  float wx[3], wh[3][2], bi[3], bh[3];
  int hd[3], nbq[3], ex[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int row = q * H + (unit ? j : 0);
    const float* rp = Wih + (size_t)row * I;
    int h = (int)((4 - (((uintptr_t)rp >> 2) & 3)) & 3);
    h = h < I ? h : I;
    const int nb = (I - h) >> 2, tail = I - h - 4 * nb;
    hd[q] = h;
    nbq[q] = nb;
#pragma unroll
    for (int m = 0; m < STEP_MC; ++m) {
      const int c = lane + 64 * m;
      wv[q][m] = (unit && c < nb) ? *(const f32x4*)(rp + h + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    ex[q] = lane < h ? lane : ((lane >= 4 && lane < 4 + tail) ? h + 4 * nb + lane - 4 : -1);
    wx[q] = (unit && ex[q] >= 0) ? rp[ex[q]] : 0.f;
    const float* hp = Whh + (size_t)row * H;
    wh[q][0] = (unit && lane < H) ? hp[lane] : 0.f;
    wh[q][1] = (unit && lane + 64 < H) ? hp[lane + 64] : 0.f;
    bi[q] = bih[row];
    bh[q] = bhh[row];
  }
  __syncthreads();

  // ---- the two graph convolutions, relu((A @ In) @ W + b) (src/step5_gcn_layer_model.py:15,18,21), fp32 FMA chains
  const int n_out = nw * I;
  auto a_times = [&](const float* In) {        // Pb = A @ In
    for (int o = tid; o < n_out; o += STEP_THREADS) {
      const int w = o / I, r = o % I, s = r / 13, f = r % 13;
      const float* ar = As + s * S;
      const float* in = In + w * STEP_IW + f;
      float acc = 0.f;
      for (int u = 0; u < S; ++u) acc = fmaf(ar[u], in[u * 13], acc);
      Pb[w * STEP_IW + r] = acc;
    }
  };
  auto times_w = [&](int l, float* Out) {      // Out = relu(Pb @ W_l + b_l)
    for (int o = tid; o < n_out; o += STEP_THREADS) {
      const int w = o / I, r = o % I, s = r / 13, f = r % 13;
      const float* pr = Pb + w * STEP_IW + s * 13;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 13; ++k) acc = fmaf(pr[k], Ws[l][k * 13 + f], acc);
      Out[w * STEP_IW + r] = fmaxf(acc + Ws[l][169 + f], 0.f);
    }
  };
  a_times(Xg);
  __syncthreads();
  times_w(0, H1);
  __syncthreads();
  a_times(H1);
  __syncthreads();
  times_w(1, Xg);                              // g overwrites the tiles
  __syncthreads();
  if (!unit) return;                           // (no barrier below)

  // ---- gi = W_ih g + b_ih, gh = W_hh h0 + b_hh for the wave's unit and each window; then the cell
  for (int w = 0; w < nw; ++w) {
    const float* g = Xg + w * STEP_IW;
    float gi[3], gh[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float* gq = g + hd[q];
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int m = 0; m < STEP_MC; ++m) {     // chunk lane + 64 m: elements hd + 4 c .. + 3 of the row (< I)
        const int c = 4 * (lane + 64 * m);
        if (lane + 64 * m < nbq[q]) {
          a0 = fmaf(wv[q][m][0], gq[c], a0);
          a1 = fmaf(wv[q][m][1], gq[c + 1], a1);
          a0 = fmaf(wv[q][m][2], gq[c + 2], a0);
          a1 = fmaf(wv[q][m][3], gq[c + 3], a1);
        }
      }
      if (ex[q] >= 0) a0 = fmaf(wx[q], g[ex[q]], a0);
      const float* hv = Hs + w * STEP_HMAX;
      float c0 = fmaf(wh[q][0], hv[lane], 0.f);
      c0 = fmaf(wh[q][1], hv[lane + 64], c0);
      gi[q] = wave_sum(a0 + a1) + bi[q];
      gh[q] = wave_sum(c0) + bh[q];
    }
    if (lane == 0) {
      const int b = b0 + w;
      const float r = sigmoid_fast(gi[0] + gh[0]);             // (the recurrences' forms, common.h)
      const float z = sigmoid_fast(gi[1] + gh[1]);
      const float n = tanh_fast(fmaf(r, gh[2], gi[2]));
      const float hnew = (1.f - z) * n + z * Hs[w * STEP_HMAX + j];
      if (Y) Y[(size_t)b * H + j] = hnew;
      if (hn) hn[(size_t)b * H + j] = hnew;
    }
  }
}

}  // namespace

bool gru_step_supported(int B, int S, int H) {
  return B >= 1 && B <= WGNN_STEP_MAX_B && S >= 1 && S <= STEP_SMAX && H >= 1 && H <= STEP_HMAX;
}

int launch_gru_step(int B, int S, int H, const float* A, const float* X, const float* W1, const float* b1, const float* W2,
                    const float* b2, const float* Wih, const float* bih, const float* Whh, const float* bhh, const float* h0,
                    float* Y, float* hn, hipStream_t st) {
  if (!gru_step_supported(B, S, H)) return WGNN_ERR_UNSUPPORTED;
  if (((uintptr_t)Wih & 3) != 0) return WGNN_ERR_UNSUPPORTED;     // float-aligned rows (torch tensors always are)
  const int I = S * 13;
  const dim3 grid(cdiv_i(H, STEP_THREADS / 64), cdiv_i(B, STEP_WB));
  // algorithmic: the two convolutions and both GRU products per window; bytes: weights, A, X, h0 once, Y and h_n out
  const double fl = (double)B * (2.0 * 2.0 * ((double)S * S * 13 + (double)S * 13 * 13) + 2.0 * 3 * H * ((double)I + H));
  const double by = 4.0 * (3.0 * H * (I + H) + 6.0 * H + (double)S * S + 2 * (13 * 13 + 13)) +
                    4.0 * B * ((double)I + (h0 ? H : 0) + (Y ? H : 0) + (hn ? H : 0));
  PROF_LAUNCH("gru_step_kernel", fl, by, st,
              hipLaunchKernelGGL(gru_step_kernel, grid, dim3(STEP_THREADS), 0, st, B, S, H, A, X, W1, b1, W2, b2, Wih, bih,
                                 Whh, bhh, h0, Y, hn));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}
