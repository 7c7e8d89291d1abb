// GRU recurrence over the window, forward and backward (BPTT), exact-fp32 MFMA, W_hh resident in REGISTERS.
//
// Reference: nn.GRU(gru_input, gru_hidden_dim, batch_first=True) called with h0 = 0 at
// src/step6_gcn_gru_combined_model.py:11,23 (torch gate order r,z,n):
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r*gh_n), h = (1-z) n + z h_prev
// with gi = W_ih g + b_ih (precomputed for every timestep by the input-projection GEMM) and
// gh = W_hh h_prev + b_hh computed here; and its BPTT (src/main.py:79).
//
// One workgroup owns 16 windows (one MFMA M tile) for all T steps, 8 waves; wave w owns hidden units [16w, 16w + 16) of
// all three gates, so the gate math is lane-local in the C layout of v_mfma_f32_16x16x4_f32 (bitwise an fp32 fmaf chain).
// Each wave keeps its slice of W_hh (forward: [k = h index][n = gate unit]; backward: W_hh^T, [k = gate row][n = hidden
// unit]) as MFMA B operands in VGPRs for the whole launch -- 3 x 26 / 78 registers at H = 102 -- so LDS carries only the
// 16 x H state (h_t, or dgh_t) between waves, double-buffered by step parity (one barrier per step).  The MFMA's k slots
// are free to permute as long as A and B agree: lane (m, kq) takes k = kq KS + ks in step ks, i.e. a lane's A operands
// of all steps are KS CONTIGUOUS floats of its state row and come in as a few wide LDS reads instead of one per MFMA.
// (Round 2's kernels kept W_hh in LDS: two 4-byte LDS reads per MFMA and two barriers per step, 125 / 176 us.)
//
// What else the kernels do, so that no launch-sized pass is left around them in the exact-fp32 step:
//   forward  -- with labels (wgnn_fwd_loss): per-workgroup sums of (h - label)^2 into the stash (the loss needs no pass over
//               Y and the labels); the B operand of the dW_hh GEMM, [Hprev | 1 | 0..] with 16-byte aligned rows, written
//               directly (was hprev_pad_kernel); last_only (wgnn_fwd_last): only h_{T-1} * mul + add leaves the chip;
//   backward -- with labels: dY = 2 (Y - labels) grad_scale / n formed from the h_prev it loads anyway (no dY tensor, no
//               mse_kernel), the loss finalised by workgroup 0; of dGH only the n third is stored (dGHn): its r and z thirds
//               equal dGI's and the dW_hh GEMM takes them from there (two-source A operand, gemm32.hip).
#include <type_traits>

#include "common.h"
#include "../../include/windgnn_series_masked.h"

namespace {

constexpr int MB = 16;        // windows per workgroup (one MFMA M tile)
constexpr int NTHREADS = 512; // 8 waves -> up to 128 hidden units
typedef float f32x2 __attribute__((ext_vector_type(2)));

// N contiguous floats (N even) from LDS into registers with the widest reads the alignment allows
template <int N>
__device__ __forceinline__ void lds_row(const float* p, float (&a)[N]) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const f32x4 v = *(const f32x4*)(p + 4 * i);
      a[4 * i] = v[0]; a[4 * i + 1] = v[1]; a[4 * i + 2] = v[2]; a[4 * i + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const f32x2 v = *(const f32x2*)(p + 2 * i);
      a[2 * i] = v[0]; a[2 * i + 1] = v[1];
    }
  }
}

// GI rows between the first rows of two consecutive windows: T (window-major GI), or the stride of a SeriesRows; 0 for a
// SeriesStarts (the workgroup's base is the series' base, and a window's first row comes from the table: series_start)
template <typename A, typename... R>
__device__ __forceinline__ A first_of(A a, R...) { return a; }   // the row mapping of a pack (a MaskedLabels tag may follow it)
template <typename... S>
__device__ __forceinline__ int gi_window_rows(int T, S... s) {
  if constexpr ((std::is_same<S, SeriesRows>::value || ...)) return first_of(s...).stride;
  else if constexpr ((std::is_same<S, SeriesStarts>::value || ...)) return 0;
  else return T;
}
// SeriesStarts: the first series row of window w (w < B), clamped so that rows [start, start + T) lie inside the series
template <typename... S>
__device__ __forceinline__ int series_start(int w, S... s) {
  const SeriesStarts ss = first_of(s...);
  return min(max(ss.starts[w], 0), ss.last);
}
__device__ __forceinline__ LossFn lossfn_of(SeriesRows, LossFn f) { return f; }     // the loss spec of a pack that has one
__device__ __forceinline__ LossFn lossfn_of(SeriesStarts, LossFn f) { return f; }
// the first spare word behind the tag (common.h: WGNN_STATS_TAG_LOSSFN); the second holds delta's bits for Huber and 0 otherwise
__device__ __forceinline__ unsigned lossfn_word(LossFn f) { return (unsigned)f.kind | (unsigned)f.masked << 8; }
__device__ __forceinline__ unsigned lossfn_delta(LossFn f) { return f.kind == 2 ? __float_as_uint(f.delta) : 0u; }
// The three kinds without a branch in the recurrences' steps.  With d = h - label and a = |d|, the forward adds
//   fmaf(a > thr ? lin : q d,  a > thr ? a - off : d,  sum):   MSE  thr = inf:  fmaf(d, d, sum), the other instances' chain
//                                                              L1   thr = -1:   sum + a        Huber  thr = delta:  both arms
// and BPTT takes rho'(d) = a > gthr ? copysign(lin, d) : d (MSE: d, the 2 is in the factor; L1: gthr = 0, so sign(0) = 0;
// Huber: the clamp).  A NaN fails both comparisons and stays a NaN.
struct LossArms { float thr, q, lin, off, gthr; };
__device__ __forceinline__ LossArms loss_arms(LossFn f) {
  if (f.kind == 1) return LossArms{-1.f, 1.f, 1.f, 0.f, 0.f};
  if (f.kind == 2) return LossArms{f.delta, 0.5f, f.delta, 0.5f * f.delta, f.delta};
  return LossArms{__builtin_inff(), 1.f, 1.f, 0.f, __builtin_inff()};
}
// did wgnn_series_fwd_lossfn write this buffer, with this spec?
__device__ __forceinline__ bool lossfn_paired(const float* stat_part, int nb, LossFn f) {
  const unsigned* w = (const unsigned*)(stat_part + 2 * (size_t)nb + 1);
  return stat_part[2 * (size_t)nb] == WGNN_STATS_TAG_LOSSFN && w[0] == lossfn_word(f) && w[1] == lossfn_delta(f) &&
         w[2] == (unsigned)f.t_from;
}

// unsigned long long c = the sum of a forward's n per-workgroup label counts, formed by every thread of a BPTT workgroup
// (integers: any order; uses the kernel's `lane` and `wave`).  read (workgroup-uniform) = false: nothing is loaded, c = 0.
// A macro, not a function: both users expand the text the masked instances were compiled from, so their code stays as it was.
#define BLOCK_COUNT_SUM(c, counts, n, read)                                       \
  __shared__ unsigned long long cred[NTHREADS / 64];                              \
  const unsigned* cnts = (counts);                                                \
  unsigned long long c = 0;                                                       \
  if (read)                                                                       \
    for (int i = threadIdx.x; i < (n); i += NTHREADS) c += cnts[i];               \
  _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);   \
  if (lane == 0) cred[wave] = c;                                                  \
  __syncthreads();                                                                \
  c = 0;                                                                          \
  _Pragma("unroll") for (int w = 0; w < NTHREADS / 64; ++w) c += cred[w]

// gate stash: grux.hip's layout, [workgroup][t][wave][r | z | n | gh_n][lane] x float4 (the 4 window rows a lane owns):
// one 16-byte access per lane and component, 1 KB per wave-instruction
__host__ __device__ inline size_t gate_floats(int B, int T, int H) {
  return (size_t)((B + MB - 1) / MB) * T * ((H + 15) / 16) * 4 * 64 * 4;
}

// Sr (empty, or one SeriesRows: wgnn_series_fwd): GI is one series and window w reads row w * stride + t of it, and so are the
// labels (wgnn_series_fwd_loss: Lab = Ls [ls_rows][H], the same row); everything the kernel writes stays window-major.
// Or one SeriesStarts (wgnn_series_fwd_at): the row is clamp(starts[w], 0, last) + t.
// A MaskedLabels behind either (wgnn_series_fwd_loss_masked): a NaN label is no label -- it adds nothing to the sum and the
// maximum, and the workgroup leaves the integer count of its labels behind the statistics (common.h: masked_counts).
// Or a LossFn behind either (wgnn_series_fwd_lossfn): the sum is of rho(h - label) for the spec's kind over the steps
// t >= t_from (and, with masked, the labels that are not NaN); the counts, a third tag and the spec go behind the statistics.
template <int KS, bool ST = false, typename... Sr>   // k steps of 4 over the hidden index, 4 KS >= H, KS even; ST: the wgnn_fwd_state instance
__global__ void __launch_bounds__(NTHREADS) gru_fwd_kernel(int B, int T, int H, const float* __restrict__ GI, int ldgi,
                                                           const float* __restrict__ Whh,
                                                           const float* __restrict__ bhh, float* __restrict__ Y,
                                                           float* __restrict__ gates, const float* __restrict__ Lab,
                                                           float* __restrict__ stat_part, float* __restrict__ hprev,
                                                           int hq, int last_only, float y_mul, float y_add,
                                                           const float* __restrict__ h0, float* __restrict__ hn,
                                                           Sr... series) {
  constexpr bool SR = sizeof...(Sr) > 0;
  constexpr bool SS = (std::is_same<Sr, SeriesStarts>::value || ...);
  constexpr bool MK = (std::is_same<Sr, MaskedLabels>::value || ...);
  constexpr bool LF = (std::is_same<Sr, LossFn>::value || ...);
  // h0 (nullable, wgnn_fwd_state): [B][H] initial state instead of zeros; hn (nullable): h_{T-1} [B][H], unrounded
  if (!ST) { h0 = nullptr; hn = nullptr; }       // (the plain forward's instance compiles exactly as before)
  constexpr int KP = 4 * KS, HS = KP + 4;          // row stride: 16-byte aligned rows
  __shared__ __attribute__((aligned(16))) float hbuf[2 * MB * HS];
  for (int i = threadIdx.x; i < 2 * MB * HS; i += NTHREADS) {
    const int m = i / HS, k = i % HS;              // buffer 0 (m < MB) holds h_{-1}
    hbuf[i] = (h0 && m < MB && k < H && blockIdx.x * MB + m < B) ? h0[(size_t)(blockIdx.x * MB + m) * H + k] : 0.f;
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int j = 16 * wave + lm;
  const bool active = 16 * wave < H;               // wave-uniform
  const bool jv = j < H;
  const int jc = jv ? j : H - 1;
  const int b0 = blockIdx.x * MB;
  // tag behind the MSE partial pairs: set by wgnn_fwd_loss, cleared by a plain forward on the same stash
  if constexpr (LF) {   // a third tag, and the spec in the three spare words: the backward must come with the same one
    if (stat_part && blockIdx.x == 0 && threadIdx.x == 0) {
      const LossFn fn = lossfn_of(series...);
      stat_part[2 * gridDim.x] = Lab ? WGNN_STATS_TAG_LOSSFN : 0.f;
      unsigned* w = (unsigned*)(stat_part + 2 * gridDim.x + 1);
      w[0] = lossfn_word(fn);
      w[1] = lossfn_delta(fn);
      w[2] = (unsigned)fn.t_from;
    }
  } else
  if (stat_part && blockIdx.x == 0 && threadIdx.x == 0)
    stat_part[2 * gridDim.x] = Lab ? (MK ? WGNN_STATS_TAG_MASKED : WGNN_STATS_TAG) : 0.f;
  if (hprev) {
    // [Hprev | 1 | 0..] rows: the constant tail of every row (b, t) and the whole row (b, 0) (h_{-1} = 0); the body of
    // row (b, t + 1) is written with h_t below
    const int tail = hq - H;
    for (int q = threadIdx.x; q < MB * T * tail; q += NTHREADS) {
      const int m = q / (T * tail), rem = q % (T * tail), t = rem / tail, c = H + rem % tail;
      if (b0 + m < B) hprev[((size_t)(b0 + m) * T + t) * hq + c] = c == H ? 1.f : 0.f;
    }
    for (int q = threadIdx.x; q < MB * H; q += NTHREADS) {
      const int m = q / H, c = q % H;
      if (b0 + m < B) hprev[((size_t)(b0 + m) * T) * hq + c] = 0.f;
    }
  }

  float WB[3][KS];                                 // B operand of step ks: W_hh[gate H + j][k = lk KS + ks]
#pragma unroll
  for (int gate = 0; gate < 3; ++gate)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = lk * KS + ks;
      WB[gate][ks] = (jv && k < H) ? Whh[(size_t)(gate * H + j) * H + k] : 0.f;
    }
  const float bh_r = bhh[jc], bh_z = bhh[H + jc], bh_n = bhh[2 * H + jc];

  const float* GIw = GI + (size_t)b0 * gi_window_rows(T, series...) * ldgi;
  float* Yw = Y + (size_t)b0 * T * H;
  const float* Labw = Lab ? Lab + (size_t)b0 * gi_window_rows(T, series...) * H : nullptr;   // series: Ls [ls_rows][H], hour-major
  float* Hpw = hprev ? hprev + (size_t)b0 * T * hq : nullptr;
  const int NW = (H + 15) / 16;
  // three components per record, r | z | gh_n: the BPTT kernel recomputes n = tanh(gi_n + r gh_n) from GI's n third, which
  // stays in the stash (round 4, as in grux.hip: the recurrences are bound by their bytes)
  f32x4* gatesw = gates ? (f32x4*)gates + ((size_t)blockIdx.x * T * NW + wave) * 3 * 64 + lane : nullptr;
  int rowt[4];            // (local window row) * T, clamped to the last valid window
  int rowg[4];            // series: (local window row) * stride, the window's first GI row
  bool rowok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * lk + r;
    rowok[r] = jv && b0 + m < B;
    rowt[r] = (b0 + m < B ? m : B - 1 - b0) * T;
    if constexpr (SS) rowg[r] = series_start(b0 + m < B ? b0 + m : B - 1, series...);
    else if constexpr (SR) rowg[r] = (b0 + m < B ? m : B - 1 - b0) * gi_window_rows(T, series...);
  }
  float gi[3][4], gin[3][4], lab[4] = {0.f, 0.f, 0.f, 0.f}, labn[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_gi = [&](int t, float (&dst)[3][4], float (&ldst)[4]) {
    const int tc = t < T ? t : T - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = ((SR ? rowg[r] : rowt[r]) + tc) * ldgi + jc;
      dst[0][r] = GIw[o];
      dst[1][r] = GIw[o + H];
      dst[2][r] = GIw[o + 2 * H];
      if (Lab) ldst[r] = Labw[((SR ? rowg[r] : rowt[r]) + tc) * H + jc];   // the label row is the GI row
    }
  };
  load_gi(0, gi, lab);
  float hold[4] = {0.f, 0.f, 0.f, 0.f};
  if (h0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) hold[r] = rowok[r] ? h0[(size_t)(b0 + 4 * lk + r) * H + j] : 0.f;
  }
  float ssum = 0.f, smax = 0.f;
  unsigned cnt = 0;       // MK, LF: labels seen by this thread (at most 4 T)
  LossFn fn{};            // LF: the spec and its arms, scalars
  LossArms arms{};
  if constexpr (LF) {
    fn = lossfn_of(series...);
    arms = loss_arms(fn);
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const float* hcur = hbuf + (t & 1) * MB * HS;          // h_{t-1}
    float* hnext = hbuf + ((t + 1) & 1) * MB * HS;         // h_t goes here
    load_gi(t + 1, gin, labn);                             // prefetch under this step's MFMAs
    float hnew[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      f32x4 ar, az, an;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ar[r] = gi[0][r] + bh_r;
        az[r] = gi[1][r] + bh_z;
        an[r] = bh_n;
      }
      float a[KS];
      lds_row<KS>(hcur + lm * HS + lk * KS, a);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        ar = mfma16(a[ks], WB[0][ks], ar);
        az = mfma16(a[ks], WB[1][ks], az);
        an = mfma16(a[ks], WB[2][ks], an);
      }
      f32x4 rg4, zg4, ng4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // hardware exp2 / rcp forms (|error| < 3e-7, as in grux.hip and gru_small.hip)
        const float rg = sigmoid_fast(ar[r]);
        const float zg = sigmoid_fast(az[r]);
        const float ng = tanh_fast(__builtin_fmaf(rg, an[r], gi[2][r]));   // the BPTT kernel recomputes exactly this
        rg4[r] = rg; zg4[r] = zg; ng4[r] = ng;
        hnew[r] = (1.f - zg) * ng + zg * hold[r];
        if (rowok[r]) {
          if (!last_only) Yw[(rowt[r] + t) * H + j] = hnew[r];
          else if (t == T - 1) Y[(size_t)(b0 + 4 * lk + r) * H + j] = hnew[r] * y_mul + y_add;
          if (hn && t == T - 1) hn[(size_t)(b0 + 4 * lk + r) * H + j] = hnew[r];
          if (Hpw && t + 1 < T) Hpw[(rowt[r] + t + 1) * hq + j] = hnew[r];
          if constexpr (LF) {
            // rho as ONE fmaf(a, b, ssum) for every kind, operands picked by selects (LossArms above the loop): no branch
            // inside the step.  A warm-up step (t < t_from) and a missing label are selected away together, as below.
            const bool has = t >= fn.t_from && (!fn.masked || lab[r] == lab[r]);
            const float dl = has ? hnew[r] - lab[r] : 0.f;
            const float ad = fabsf(dl);
            const bool lin = ad > arms.thr;                  // (a NaN takes the quadratic arm and stays one)
            ssum = fmaf(lin ? arms.lin : arms.q * dl, lin ? ad - arms.off : dl, ssum);
            smax = fmaxf(smax, ad);
            cnt += has ? 1u : 0u;
          } else if constexpr (MK) {
            const bool has = lab[r] == lab[r];               // a NaN is no label; the select keeps NaN * 0 out of the sum
            const float dl = has ? hnew[r] - lab[r] : 0.f;
            ssum = fmaf(dl, dl, ssum);
            smax = fmaxf(smax, fabsf(dl));
            cnt += has ? 1u : 0u;
          } else if (Lab) {
            const float dl = hnew[r] - lab[r];
            ssum = fmaf(dl, dl, ssum);
            smax = fmaxf(smax, fabsf(dl));
          }
        }
        hold[r] = hnew[r];
      }
      if (gates) {
        f32x4* rec = gatesw + (size_t)t * NW * 3 * 64;
        rec[0] = rg4;
        rec[64] = zg4;
        rec[128] = an;
      }
      if (jv) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hnext[(4 * lk + r) * HS + j] = hnew[r];
      }
    }
    __syncthreads();                               // h_t complete; everyone is done reading h_{t-1}
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) gi[q][r] = gin[q][r];
#pragma unroll
    for (int r = 0; r < 4; ++r) lab[r] = labn[r];
  }
  if (Lab) {   // block partials in a fixed order: lanes (xor tree), then the 8 waves
    __shared__ float red[2][NTHREADS / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ssum += __shfl_xor(ssum, o, 64);
      smax = fmaxf(smax, __shfl_xor(smax, o, 64));
    }
    if (lane == 0) {
      red[0][wave] = ssum;
      red[1][wave] = smax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = 0.f, m = 0.f;
#pragma unroll
      for (int w = 0; w < NTHREADS / 64; ++w) {
        s += red[0][w];
        m = fmaxf(m, red[1][w]);
      }
      stat_part[blockIdx.x] = s;
      stat_part[gridDim.x + blockIdx.x] = m;
    }
    if constexpr (MK || LF) {   // the exact count: integer adds, any order
      __shared__ unsigned redc[NTHREADS / 64];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) redc[wave] = cnt;
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < NTHREADS / 64; ++w) c += redc[w];
        masked_counts(stat_part, gridDim.x)[blockIdx.x] = c;
      }
    }
  }
}

// BPTT.  Per step (t descending), with dh = dY_t + dh_next:
//   dn = dh (1-z), dz = dh (hprev - n), dnt = dn (1-n^2), dr = dnt gh_n,
//   dar = dr r (1-r), daz = dz z (1-z);  dgi = [dar, daz, dnt], dgh = [dar, daz, dnt r]
//   dh_next = dh z + dgh W_hh
// Outputs for the GEMMs that follow: dGI rows [B*T][ldd] (3H layout, zero K padding) and dGHn = dnt r rows [B*T][hn].
// St (empty, or one BwdState: wgnn_bwd_state_part): h_{-1} = h0, the carry starts at dh_n, and the step at t = 0 also forms
// dh_{-1} = dh z + dgh W_hh into dh0.  Or one SeriesRows (wgnn_series_bwd / wgnn_series_bwd_mse): GIn, and Lab if given, are
// one series each, as in the forward; or one SeriesStarts (the _at entry points), likewise.  A MaskedLabels behind either
// (wgnn_series_bwd_mse_masked): dY = 2 grad_scale (Y - label) / m where the label is not NaN and +0 elsewhere, m = the sum of the
// forward's per-workgroup counts, which EVERY workgroup adds up itself before its loop (integers: no order to fix, no launch
// between forward and backward); coef_lab carries grad_scale, inv_n is unused; m = 0: loss NaN, dY = 0, WGNN_STATUS_NO_LABELS.
// Or a LossFn behind either (wgnn_series_bwd_lossfn): dY = coef_lab rho'(Y - label) on the steps t >= t_from (and, with
// masked, where the label is not NaN), +0 elsewhere; every step still runs.  Without masked inv_n and coef_lab come from the
// host (m = B (T - t_from) H), with it from the counts as above.  stat_part must be this spec's forward's: else loss NaN, dY = 0.
template <int KS3, typename... St>   // k steps of 4 over the gate-row index, 4 KS3 >= 3H, KS3 even
__global__ void __launch_bounds__(NTHREADS) gru_bwd_kernel(int B, int T, int H, const float* __restrict__ Whh,
                                                           const float* __restrict__ Y, const float* __restrict__ dY,
                                                           const float* __restrict__ Lab,
                                                           const float* __restrict__ gates,
                                                           const float* __restrict__ GIn, int ldgi,
                                                           float* __restrict__ dGI,
                                                           int ldd, float* __restrict__ dGN, int hn,
                                                           float* __restrict__ dGH /*nullable: full rows [B*T][ldd]*/,
                                                           const float* __restrict__ stat_part, int nstat, float inv_n,
                                                           float coef_lab, float* __restrict__ loss_out,
                                                           unsigned* status, St... state) {
  constexpr bool SS = (std::is_same<St, SeriesStarts>::value || ...);
  constexpr bool SR = (std::is_same<St, SeriesRows>::value || ...) || SS;
  constexpr bool ST = sizeof...(St) > 0 && !SR;
  constexpr bool MK = (std::is_same<St, MaskedLabels>::value || ...);
  constexpr bool LF = (std::is_same<St, LossFn>::value || ...);
  const BwdState sb = bwd_state(state...);
  constexpr int KP = 4 * KS3, DS = KP + 4;
  __shared__ __attribute__((aligned(16))) float dbuf[2 * MB * DS];   // dgh rows [dar | daz | dnr | 0..], by step parity
  for (int i = threadIdx.x; i < 2 * MB * DS; i += NTHREADS) dbuf[i] = 0.f;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int j = 16 * wave + lm;
  const bool active = 16 * wave < H;
  const bool jv = j < H;
  const int jc = jv ? j : H - 1;
  const int b0 = blockIdx.x * MB;
  const int G3 = 3 * H;
  if constexpr (MK) {
    BLOCK_COUNT_SUM(c, masked_counts(stat_part, nstat), nstat, true);
    const bool counted = stat_part[2 * nstat] == WGNN_STATS_TAG_MASKED;   // else: not this forward's buffer, no count to trust
    if (!counted) c = 0;
    // the two factors as launch_gru_bwd forms them on the host from n_loss (IEEE division)
    inv_n = c ? 1.0f / (float)c : __builtin_nanf("");       // m = 0: loss[0] = NaN whatever the partial sums hold
    coef_lab = c ? 2.0f * coef_lab / (float)c : 0.f;
    if (counted && c == 0 && blockIdx.x == 0 && threadIdx.x == 0 && status) atomicOr(status, WGNN_STATUS_NO_LABELS);
  }
  bool paired = false;    // LF: this spec's forward wrote stat_part
  LossFn fn{};            // LF: the spec and its arms, scalars
  LossArms arms{};
  if constexpr (LF) {
    fn = lossfn_of(state...);
    arms = loss_arms(fn);
    paired = lossfn_paired(stat_part, nstat, fn);
    if (fn.masked) {      // (uniform) m from the forward's counts, as above; coef_lab carries grad_scale
      // (a buffer this forward did not write may be wgnn_series_fwd_loss's shorter one: its counts are not even read)
      BLOCK_COUNT_SUM(c, masked_counts(stat_part, nstat), nstat, paired);
      inv_n = c ? 1.0f / (float)c : __builtin_nanf("");
      coef_lab = c ? (fn.kind == 0 ? 2.0f * coef_lab / (float)c : coef_lab / (float)c) : 0.f;
      if (paired && c == 0 && blockIdx.x == 0 && threadIdx.x == 0 && status) atomicOr(status, WGNN_STATUS_NO_LABELS);
    } else if (!paired) {
      coef_lab = 0.f;     // another forward's statistics: dY = 0, and the loss below is NaN
    }
  }
  if (stat_part && blockIdx.x == 0) {   // loss = (sum of the forward's per-workgroup partial sums) / n, fixed order
    __shared__ float sred[NTHREADS / 64];
    float a = 0.f;
    for (int i = threadIdx.x; i < nstat; i += NTHREADS) a += stat_part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) sred[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      a = 0.f;
#pragma unroll
      for (int w = 0; w < NTHREADS / 64; ++w) a += sred[w];
      const bool tagged = LF ? paired : stat_part[2 * nstat] == (MK ? WGNN_STATS_TAG_MASKED : WGNN_STATS_TAG);
      loss_out[0] = tagged ? a * inv_n : __builtin_nanf("");     // no statistics of these labels in the stash: loud
      if (!tagged && status) atomicOr(status, WGNN_STATUS_NO_LOSS_STATS);
    }
  }
  {  // zero the K-padding columns [3H, ldd) of this workgroup's dGI rows and [H, hn) of its dGHn rows
    const int nrows = min(MB, B - b0) * T;
    const int npad = ldd - G3, npn = hn - H;
    for (int i = threadIdx.x; i < nrows * npad; i += NTHREADS)
      dGI[((size_t)b0 * T + i / npad) * ldd + G3 + i % npad] = 0.f;
    if (dGN)
      for (int i = threadIdx.x; i < nrows * npn; i += NTHREADS)
        dGN[((size_t)b0 * T + i / npn) * hn + H + i % npn] = 0.f;
    if (dGH)
      for (int i = threadIdx.x; i < nrows * npad; i += NTHREADS)
        dGH[((size_t)b0 * T + i / npad) * ldd + G3 + i % npad] = 0.f;
  }

  float WT[KS3];                                   // B operand of step ks: W_hh[k = lk KS3 + ks][j]
#pragma unroll
  for (int ks = 0; ks < KS3; ++ks) {
    const int k = lk * KS3 + ks;
    WT[ks] = (jv && k < G3) ? Whh[(size_t)k * H + j] : 0.f;
  }
  const int NW = (H + 15) / 16;
  const f32x4* gatesw = (const f32x4*)gates + ((size_t)blockIdx.x * T * NW + (active ? wave : 0)) * 3 * 64 + lane;
  const float* GIw = GIn + (size_t)b0 * gi_window_rows(T, state...) * ldgi + 2 * H;   // n third of this workgroup's GI rows (stash)
  const float* Yw = Y + (size_t)b0 * T * H;
  const float* dYw = dY ? dY + (size_t)b0 * T * H : nullptr;
  const float* Labw = Lab ? Lab + (size_t)b0 * gi_window_rows(T, state...) * H : nullptr;   // series: Ls, hour-major
  float* dGIw = dGI + (size_t)b0 * T * ldd;
  float* dGNw = dGN ? dGN + (size_t)b0 * T * hn : nullptr;
  float* dGHw = dGH ? dGH + (size_t)b0 * T * ldd : nullptr;
  int rowt[4];
  int rowg[4];            // series: (local window row) * stride
  bool rowok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * lk + r;
    rowok[r] = jv && b0 + m < B;
    rowt[r] = (b0 + m < B ? m : B - 1 - b0) * T;
    if constexpr (SS) rowg[r] = series_start(b0 + m < B ? b0 + m : B - 1, state...);
    else if constexpr (SR) rowg[r] = (b0 + m < B ? m : B - 1 - b0) * gi_window_rows(T, state...);
  }
  // h0 in registers before the loop: a load under `tc == 0` inside load_step would make the compiler wait for all of
  // the step's prefetches at the join
  float h0r[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ST) {
#pragma unroll
    for (int r = 0; r < 4; ++r) h0r[r] = sb.h0[(size_t)(b0 + rowt[r] / T) * H + jc];
  }
  struct StepIn { float dy[4], r[4], z[4], n[4], ghn[4], hp[4]; };
  auto load_step = [&](int t, StepIn& s) {
    const int tc = t > 0 ? t : 0;
    const f32x4* rec = gatesw + (size_t)tc * NW * 3 * 64;
    const f32x4 r4 = rec[0], z4 = rec[64], g4 = rec[128];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int bt = rowt[r] + tc;
      s.dy[r] = Lab ? Labw[(SR ? rowg[r] + tc : bt) * H + jc] : dYw[bt * H + jc];   // the label (series: at the GI row), or dY itself
      s.r[r] = r4[r];
      s.z[r] = z4[r];
      s.n[r] = GIw[(SR ? rowg[r] + tc : bt) * ldgi + jc];          // gi_n: n itself is formed in the step
      s.ghn[r] = g4[r];
      const float hp = Yw[(bt - (tc > 0 ? 1 : 0)) * H + jc];
      s.hp[r] = tc > 0 ? hp : 0.f;
      if constexpr (ST) {   // (a discarded branch: the plain instance's lambda does not even capture sb)
        if (tc == 0) s.hp[r] = h0r[r];
      }
    }
  };
  StepIn cur, nxt;
  load_step(T - 1, cur);
  float ycur[4] = {0.f, 0.f, 0.f, 0.f};              // Y[b, t]: the h_prev of step t + 1
  if (Lab) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ycur[r] = Yw[(rowt[r] + T - 1) * H + jc];
  }
  f32x4 dhn = {0.f, 0.f, 0.f, 0.f};
  if (ST && sb.dhn) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dhn[r] = rowok[r] ? sb.dhn[(size_t)(b0 + 4 * lk + r) * H + j] : 0.f;
  }
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    float* ds = dbuf + (t & 1) * MB * DS;
    load_step(t - 1, nxt);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * lk + r;
        float dyv;
        if constexpr (LF) {
          const bool on = paired && t >= fn.t_from && (!fn.masked || cur.dy[r] == cur.dy[r]);
          const float rr = ycur[r] - cur.dy[r];
          const float g = fabsf(rr) > arms.gthr ? copysignf(arms.lin, rr) : rr;   // rho' without a branch (LossArms)
          dyv = on ? g * coef_lab : 0.f;                       // outside M: exactly +0, whatever the label holds
        } else if constexpr (MK) dyv = cur.dy[r] == cur.dy[r] ? (ycur[r] - cur.dy[r]) * coef_lab : 0.f;   // no label: exactly +0
        else dyv = Lab ? (ycur[r] - cur.dy[r]) * coef_lab : cur.dy[r];
        const float dh = rowok[r] ? dyv + dhn[r] : 0.f;
        const float rg = cur.r[r], zg = cur.z[r];
        const float ng = tanh_fast(__builtin_fmaf(rg, cur.ghn[r], cur.n[r]));   // the forward's n, bit for bit
        const float dn = dh * (1.f - zg);
        const float dz = dh * (cur.hp[r] - ng);
        const float dnt = dn * (1.f - ng * ng);
        const float dr = dnt * cur.ghn[r];
        const float dar = dr * rg * (1.f - rg);
        const float daz = dz * zg * (1.f - zg);
        const float dnr = dnt * rg;
        acc[r] = dh * zg;
        if (jv) {
          ds[m * DS + j] = dar;
          ds[m * DS + H + j] = daz;
          ds[m * DS + 2 * H + j] = dnr;
          if (rowok[r]) {
            float* gi = dGIw + (size_t)(rowt[r] + t) * ldd;
            gi[j] = dar;
            gi[H + j] = daz;
            gi[2 * H + j] = dnt;
            if (dGNw) dGNw[(size_t)(rowt[r] + t) * hn + j] = dnr;
            if (dGHw) {                          // small B*T: the general GEMM wants dGH whole
              float* gh = dGHw + (size_t)(rowt[r] + t) * ldd;
              gh[j] = dar;
              gh[H + j] = daz;
              gh[2 * H + j] = dnr;
            }
          }
        }
      }
    }
    __syncthreads();
    if (active && (ST || t > 0)) {
      // dgh W_hh over the 3H gate rows: four independent accumulator chains (one KS3-long dependent chain of 16x16x4
      // MFMAs is pure latency)
      f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
      const float* row = ds + lm * DS + lk * KS3;
      constexpr int CH = KS3 % 4 == 0 ? 4 : (KS3 % 6 == 0 ? 6 : 2);      // k steps per LDS read batch (divides KS3)
      static_assert(KS3 % CH == 0, "batching of the state-row reads");
#pragma unroll
      for (int c0 = 0; c0 < KS3; c0 += CH) {
        float a[CH];
        lds_row<CH>(row + c0, a);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
          const int ks = c0 + u;
          if ((ks & 3) == 0) acc = mfma16(a[u], WT[ks], acc);
          else if ((ks & 3) == 1) a1 = mfma16(a[u], WT[ks], a1);
          else if ((ks & 3) == 2) a2 = mfma16(a[u], WT[ks], a2);
          else a3 = mfma16(a[u], WT[ks], a3);
        }
      }
      acc = (acc + a1) + (a2 + a3);
      if (ST && t == 0 && sb.dh0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (rowok[r]) sb.dh0[(size_t)(b0 + 4 * lk + r) * H + j] = acc[r];
      }
    }
    dhn = acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) ycur[r] = cur.hp[r];   // Y[b, t-1]
    cur = nxt;
  }
}

// smallest supported step count >= need (instantiations: even, dense around the 34-station shapes)
int pick_ks(int need, const int* list, int n) {
  for (int i = 0; i < n; ++i)
    if (list[i] >= need) return list[i];
  return -1;
}
const int FWD_KS[] = {4, 8, 12, 16, 20, 24, 26, 28, 32};
const int BWD_KS3[] = {12, 24, 36, 48, 60, 72, 78, 84, 96};

}  // namespace

bool gru_shape_supported(int H) { return H >= 1 && H <= 16 * (NTHREADS / 64); }
size_t gru_gates_floats(int B, int T, int H) { return gate_floats(B, T, H); }
int gru_blocks(int B) { return cdiv_i(B, MB); }
int gru_hn(int H) { return 4 * cdiv_i(H, 4); }          // row width of the dGHn rows (16-byte aligned rows)
int gru_msplit(int H) { return 4 * cdiv_i(2 * H, 4); }   // first GEMM row of the dGHn block in the dW_hh product

// The one place each kernel's argument list is written.  Pack is the kernel's trailing pack: nothing, a row mapping
// (SeriesRows / SeriesStarts), a MaskedLabels or LossFn behind one, or (backward) a BwdState.
template <int K, bool ST, typename... Pack>
static void gru_fwd_go(const GruFwdArgs& a, hipStream_t st, Pack... pack) {
  hipLaunchKernelGGL((gru_fwd_kernel<K, ST, Pack...>), dim3(cdiv_i(a.B, MB)), dim3(NTHREADS), 0, st, a.B, a.T, a.H, a.GI, a.ldgi,
                     a.Whh, a.bhh, a.Y, a.gates, a.labels, a.stat_part, a.hprev, a.hq, a.last_only, a.y_mul, a.y_add,
                     ST ? a.h0 : nullptr, ST ? a.hn : nullptr, pack...);
}
template <int K, typename... Pack>
static void gru_bwd_go(const GruBwdArgs& a, float inv_n, float coef, hipStream_t st, Pack... pack) {
  hipLaunchKernelGGL((gru_bwd_kernel<K, Pack...>), dim3(cdiv_i(a.B, MB)), dim3(NTHREADS), 0, st, a.B, a.T, a.H, a.Whh, a.Y, a.dY,
                     a.labels, a.gates, a.GI, a.ldgi, a.dGI, a.ldd, a.dGHn, gru_hn(a.H), a.dGH, a.stat_part, gru_blocks(a.B), inv_n,
                     coef, a.loss, a.status, pack...);
}

int launch_gru_fwd(const GruFwdArgs& a, hipStream_t st) {
  const int B = a.B, T = a.T, H = a.H;
  const SeriesMap& m = a.map;
  if (!gru_shape_supported(H)) return WGNN_ERR_UNSUPPORTED;
  if (a.masked && (!(m.stride || m.starts) || !a.labels || !a.stat_part || a.last_only)) return WGNN_ERR_UNSUPPORTED;
  if (a.lossfn && (!(m.stride || m.starts) || !a.labels || !a.stat_part || a.masked)) return WGNN_ERR_UNSUPPORTED;
  if (a.lossfn && !lossfn_valid(*a.lossfn, T)) return WGNN_ERR_SHAPE;
  // last_only with labels: a spec alone (include/windgnn_series_val.h: the statistics of a forward that keeps nothing else)
  if (a.last_only && (a.gates || a.hprev || (a.labels && !a.lossfn))) return WGNN_ERR_UNSUPPORTED;
  if (m.stride < 0 || (m.stride && (a.h0 || a.hn))) return WGNN_ERR_UNSUPPORTED;
  if (m.starts && (m.stride || a.h0 || a.hn || m.starts_last < 0)) return WGNN_ERR_UNSUPPORTED;
  if ((m.stride || m.starts) && a.labels && m.ls_rows * H >= (1ll << 31)) return WGNN_ERR_SHAPE;   // 32-bit offsets into Ls
  if (m.starts && a.labels && m.ls_rows < (int64_t)m.starts_last + T) return WGNN_ERR_SHAPE;   // every clamped window has its label rows
  if (a.hprev && (a.hq < H + 1 || a.hq % 4 != 0)) return WGNN_ERR_SHAPE;
  const int ks = pick_ks(cdiv_i(H, 4), FWD_KS, (int)(sizeof(FWD_KS) / sizeof(int)));
  const double bt = (double)B * T;
  const double fl = bt * 2.0 * 3 * H * H;
  const double by = bt * 4.0 * (3 * H + (a.last_only ? 0 : H) + (a.labels ? H : 0) + (a.hprev ? a.hq : 0)) +
                    (a.gates ? 3.0 * gate_floats(B, T, H) : 0.0);     // three of the buffer's four components are used
  // FGO: a series instance under its own name, the pack spelled out; FMAP: either row mapping ahead of what else the pack holds
#define FGO(K, NAME, ...) PROF_LAUNCH("gru_fwd_kernel<" #K NAME ">", fl, by, st, (gru_fwd_go<K, false>(a, st, __VA_ARGS__)))
#define FMAP(K, NAME, TAIL)                                                                                       \
  do {                                                                                                            \
    if (m.starts) FGO(K, ",starts" NAME, SeriesStarts{m.starts, m.starts_last}, TAIL);                            \
    else FGO(K, NAME, SeriesRows{m.stride}, TAIL);                                                                \
  } while (0)
#define FCASE(K)                                                                                                  \
  case K:                                                                                                         \
    if (a.lossfn) FMAP(K, ",lossfn", *a.lossfn);                                                                  \
    else if (a.masked) FMAP(K, ",masked", MaskedLabels{});                                                        \
    else if (m.starts) FGO(K, ",starts", SeriesStarts{m.starts, m.starts_last});                                  \
    else PROF_LAUNCH("gru_fwd_kernel<" #K ">", fl, by, st,                                                        \
                     if (m.stride) gru_fwd_go<K, false>(a, st, SeriesRows{m.stride});                             \
                     else if (a.h0 || a.hn) gru_fwd_go<K, true>(a, st);                                           \
                     else gru_fwd_go<K, false>(a, st));                                                           \
    break
  switch (ks) {
    FCASE(4); FCASE(8); FCASE(12); FCASE(16); FCASE(20); FCASE(24); FCASE(26); FCASE(28); FCASE(32);
    default: return WGNN_ERR_UNSUPPORTED;
  }
#undef FCASE
#undef FMAP
#undef FGO
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

// labels: dY = (Y - labels) * 2 grad_scale / n_loss is formed in the kernel; with stat_part (the forward's partial sums + tag)
// workgroup 0 also writes loss[0] = mean((Y - labels)^2).
int launch_gru_bwd(const GruBwdArgs& a, hipStream_t st) {
  const int B = a.B, T = a.T, H = a.H;
  const SeriesMap& m = a.map;
  const LossFn* lossfn = a.lossfn;
  if (!gru_shape_supported(H)) return WGNN_ERR_UNSUPPORTED;
  if (a.masked && (!(m.stride || m.starts) || !a.labels || !a.stat_part || a.state)) return WGNN_ERR_UNSUPPORTED;
  if (lossfn && (!(m.stride || m.starts) || !a.labels || !a.stat_part || a.state || a.masked)) return WGNN_ERR_UNSUPPORTED;
  if (lossfn && !lossfn_valid(*lossfn, T)) return WGNN_ERR_SHAPE;
  if (a.state && (!a.state->h0 || a.labels)) return WGNN_ERR_UNSUPPORTED;
  if (m.stride < 0 || (m.stride && a.state)) return WGNN_ERR_UNSUPPORTED;
  if (m.starts && (m.stride || a.state || m.starts_last < 0)) return WGNN_ERR_UNSUPPORTED;
  if ((m.stride || m.starts) && a.labels && m.ls_rows * H >= (1ll << 31)) return WGNN_ERR_SHAPE;   // 32-bit offsets into Ls
  if (m.starts && a.labels && m.ls_rows < (int64_t)m.starts_last + T) return WGNN_ERR_SHAPE;
  if ((a.dY == nullptr) == (a.labels == nullptr) || a.ldd < 3 * H || (a.dGHn == nullptr) == (a.dGH == nullptr)) return WGNN_ERR_SHAPE;
  if (a.stat_part && (!a.labels || !a.loss)) return WGNN_ERR_NULL;
  if (!a.GI || a.ldgi < 3 * H) return WGNN_ERR_NULL;
  const int ks3 = pick_ks(cdiv_i(3 * H, 4), BWD_KS3, (int)(sizeof(BWD_KS3) / sizeof(int)));
  const float inv_n = 1.0f / (float)a.n_loss, coef = 2.0f * a.grad_scale / (float)a.n_loss;
  const double bt = (double)B * T;
  const double fl = bt * 2.0 * 3 * H * H, by = bt * 4.0 * (H + H + 3 * H + (a.dGH ? 3 * H : H)) + 3.0 * gate_floats(B, T, H) +
                                          bt * 4.0 * H;   // + GI's n third
  // a loss spec without missing labels: m = B (T - t_from) H, and no factor 2 but for the mean square; with them, as masked
  const int64_t fn_m = lossfn ? (int64_t)B * (T - lossfn->t_from) * H : 1;
  const float fn_inv = lossfn && !lossfn->masked ? 1.0f / (float)fn_m : 0.f;
  const float fn_coef = !lossfn || lossfn->masked ? a.grad_scale
                        : (lossfn->kind == 0 ? 2.0f * a.grad_scale / (float)fn_m : a.grad_scale / (float)fn_m);
  // BGO: a series instance under its own name with the two loss factors it takes; BMAP: either row mapping ahead of the tail.
  // masked: the kernel forms both factors from the forward's count; coef_lab carries grad_scale there
#define BGO(K, NAME, INV, COEF, ...) \
  PROF_LAUNCH("gru_bwd_kernel<" #K NAME ">", fl, by, st, (gru_bwd_go<K>(a, INV, COEF, st, __VA_ARGS__)))
#define BMAP(K, NAME, INV, COEF, TAIL)                                                                            \
  do {                                                                                                            \
    if (m.starts) BGO(K, ",starts" NAME, INV, COEF, SeriesStarts{m.starts, m.starts_last}, TAIL);                 \
    else BGO(K, NAME, INV, COEF, SeriesRows{m.stride}, TAIL);                                                     \
  } while (0)
#define BCASE(K)                                                                                                  \
  case K:                                                                                                         \
    if (lossfn) BMAP(K, ",lossfn", fn_inv, fn_coef, *lossfn);                                                     \
    else if (a.masked) BMAP(K, ",masked", 0.f, a.grad_scale, MaskedLabels{});                                     \
    else if (m.starts) BGO(K, ",starts", inv_n, coef, SeriesStarts{m.starts, m.starts_last});                     \
    else PROF_LAUNCH("gru_bwd_kernel<" #K ">", fl, by, st,                                                        \
                     if (m.stride) gru_bwd_go<K>(a, inv_n, coef, st, SeriesRows{m.stride});                       \
                     else if (a.state) gru_bwd_go<K>(a, inv_n, coef, st, *a.state);                               \
                     else gru_bwd_go<K>(a, inv_n, coef, st));                                                     \
    break
  switch (ks3) {
    BCASE(12); BCASE(24); BCASE(36); BCASE(48); BCASE(60); BCASE(72); BCASE(78); BCASE(84); BCASE(96);
    default: return WGNN_ERR_UNSUPPORTED;
  }
#undef BCASE
#undef BMAP
#undef BGO
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}
