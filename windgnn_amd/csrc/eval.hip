// On-device evaluation statistics (include/windgnn_eval.h): the reference's test loop, src/main.py:100-157, as five fp64 sums
// per column kept in a caller-owned accumulator, and the four published figures formed from them in one small launch.
//
// Decomposition.  A workgroup is EV_COLS columns x EV_ROWS window lanes: lane x of a wave reads column c0 + x (coalesced along
// c in pred, in row T-1 of the labels and in abs_err), window lane y takes windows b0 + y, b0 + y + EV_ROWS, ...  The four
// window lanes meet in LDS and are added in lane order by the y = 0 threads, which own their column:
//   * one slice (few windows, or enough column tiles to fill the chip): the owner adds straight into the header -- 1 launch;
//   * several slices (few columns, many windows): grid.y slices of the windows, each owner stores its four sums to the private
//     partials behind the header ([slice][4][H] doubles); eval_fold_kernel, one thread per column, adds them in slice order and
//     then into the header -- 2 launches.
// Either way every header element is read and written by exactly one thread per launch, in a fixed order: no atomics.
// All arithmetic is fp64 VALU; contraction is off so that truth, e and a round exactly as numpy's separate operations do.
#include "common.h"

#include "../../include/windgnn_eval.h"
#include "../../include/windgnn_series_masked.h"

#pragma clang fp contract(off)

namespace {

constexpr int EV_COLS = 64, EV_ROWS = 4;   // one wave per window lane
constexpr int EV_MAX_SLICES = 256;         // window slices per column tile, at most
constexpr int EV_TARGET_WGS = 1024;        // slices * column tiles aimed at (4 per CU)
constexpr int EV_MIN_WINDOWS = 32;         // windows per slice below which slicing stops paying (8 per thread)

inline int64_t ev_tiles(int H) { return ((int64_t)H + EV_COLS - 1) / EV_COLS; }
// the most slices any B gets at this H: sizes the private partials, so wgnn_eval_bytes depends on H alone
inline int ev_max_slices(int H) {
  const int64_t s = EV_TARGET_WGS / ev_tiles(H);
  return (int)(s < 1 ? 1 : s > EV_MAX_SLICES ? EV_MAX_SLICES : s);
}
inline size_t ev_header_bytes(int H) { return align_up(sizeof(double) * 5 * (size_t)H, 256); }

// partial == nullptr: add into the header; else store the slice's four sums at partial[(slice * 4 + k) * H + c]
__global__ void __launch_bounds__(EV_COLS* EV_ROWS) eval_accum_kernel(const float* __restrict__ pred, const float* __restrict__ labels,
                                                                      int B, int T, int H, int per_slice, double wmin, double wrange,
                                                                      double* __restrict__ header, double* __restrict__ partial,
                                                                      float* __restrict__ abs_err) {
  __shared__ double red[EV_ROWS - 1][4][EV_COLS];
  const int x = threadIdx.x, y = threadIdx.y;
  const int64_t c = (int64_t)blockIdx.x * EV_COLS + x;
  const int64_t b0 = (int64_t)blockIdx.y * per_slice;
  const int64_t b1 = b0 + per_slice < B ? b0 + per_slice : B;
  double se2 = 0.0, sabs = 0.0, sa = 0.0, sa2 = 0.0;
  if (c < H) {
    const size_t lrow = (size_t)T * H;
    const float* lp = labels + (size_t)(T - 1) * H + c;
    const float* pp = pred + c;
#pragma unroll 4
    for (int64_t b = b0 + y; b < b1; b += EV_ROWS) {
      const double truth = (double)lp[(size_t)b * lrow] * wrange + wmin;
      const double e = truth - (double)pp[(size_t)b * H];
      const double ae = fabs(e);
      const double a = 1.0 - ae / truth;
      se2 += e * e;
      sabs += ae;
      sa += a;
      sa2 += a * a;
      if (abs_err) abs_err[(size_t)b * H + c] = (float)ae;
    }
  }
  if (y > 0) {
    red[y - 1][0][x] = se2;
    red[y - 1][1][x] = sabs;
    red[y - 1][2][x] = sa;
    red[y - 1][3][x] = sa2;
  }
  __syncthreads();
  if (y != 0 || c >= H) return;
#pragma unroll
  for (int r = 0; r < EV_ROWS - 1; ++r) {
    se2 += red[r][0][x];
    sabs += red[r][1][x];
    sa += red[r][2][x];
    sa2 += red[r][3][x];
  }
  if (partial) {
    double* q = partial + (size_t)blockIdx.y * 4 * H + c;
    q[0] = se2;
    q[(size_t)H] = sabs;
    q[2 * (size_t)H] = sa;
    q[3 * (size_t)H] = sa2;
  } else {
    header[c] += (double)B;
    header[(size_t)H + c] += se2;
    header[2 * (size_t)H + c] += sabs;
    header[3 * (size_t)H + c] += sa;
    header[4 * (size_t)H + c] += sa2;
  }
}

__global__ void __launch_bounds__(256) eval_fold_kernel(const double* __restrict__ partial, int slices, int B, int H,
                                                        double* __restrict__ header) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int z = 0; z < slices; ++z) {
    const double* q = partial + (size_t)z * 4 * H + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += q[(size_t)k * H];
  }
  header[c] += (double)B;
#pragma unroll
  for (int k = 0; k < 4; ++k) header[(size_t)(k + 1) * H + c] += s[k];
}

// eval_accum_kernel with the truth of window b at a row of ONE label series Ls [ls_rows][H] (include/windgnn_series_masked.h):
// row (starts ? clamp(starts[b], 0, last) : b * stride) + T - 1.  SKIP = false: the arithmetic, the order and the partial layout
// of eval_accum_kernel, so the header comes out bit for bit.  SKIP: a NaN truth adds nothing, not even to the column's count,
// which becomes a fifth sum (an exact integer in fp64) -- partial[(slice * 5 + k) * H + c], k = 4 the count -- and abs_err
// receives NaN there.
template <bool SKIP>
__global__ void __launch_bounds__(EV_COLS* EV_ROWS) eval_accum_series_kernel(const float* __restrict__ pred, const float* __restrict__ Ls,
                                                                             const int* __restrict__ starts, int stride, int last,
                                                                             int B, int T, int H, int per_slice, double wmin,
                                                                             double wrange, double* __restrict__ header,
                                                                             double* __restrict__ partial, float* __restrict__ abs_err) {
  constexpr int NP = SKIP ? 5 : 4;
  __shared__ double red[EV_ROWS - 1][NP][EV_COLS];
  const int x = threadIdx.x, y = threadIdx.y;
  const int64_t c = (int64_t)blockIdx.x * EV_COLS + x;
  const int64_t b0 = (int64_t)blockIdx.y * per_slice;
  const int64_t b1 = b0 + per_slice < B ? b0 + per_slice : B;
  double se2 = 0.0, sabs = 0.0, sa = 0.0, sa2 = 0.0, cnt = 0.0;
  if (c < H) {
    const float* lp = Ls + (size_t)(T - 1) * H + c;
    const float* pp = pred + c;
#pragma unroll 4
    for (int64_t b = b0 + y; b < b1; b += EV_ROWS) {
      const int64_t row = starts ? (int64_t)min(max(starts[b], 0), last) : b * stride;
      const float tf = lp[(size_t)row * H];
      if (SKIP && tf != tf) {
        if (abs_err) abs_err[(size_t)b * H + c] = tf;
        continue;
      }
      const double truth = (double)tf * wrange + wmin;
      const double e = truth - (double)pp[(size_t)b * H];
      const double ae = fabs(e);
      const double a = 1.0 - ae / truth;
      se2 += e * e;
      sabs += ae;
      sa += a;
      sa2 += a * a;
      if (SKIP) cnt += 1.0;
      if (abs_err) abs_err[(size_t)b * H + c] = (float)ae;
    }
  }
  if (y > 0) {
    red[y - 1][0][x] = se2;
    red[y - 1][1][x] = sabs;
    red[y - 1][2][x] = sa;
    red[y - 1][3][x] = sa2;
    if (SKIP) red[y - 1][NP - 1][x] = cnt;
  }
  __syncthreads();
  if (y != 0 || c >= H) return;
#pragma unroll
  for (int r = 0; r < EV_ROWS - 1; ++r) {
    se2 += red[r][0][x];
    sabs += red[r][1][x];
    sa += red[r][2][x];
    sa2 += red[r][3][x];
    if (SKIP) cnt += red[r][NP - 1][x];
  }
  if (partial) {
    double* q = partial + (size_t)blockIdx.y * NP * H + c;
    q[0] = se2;
    q[(size_t)H] = sabs;
    q[2 * (size_t)H] = sa;
    q[3 * (size_t)H] = sa2;
    if (SKIP) q[4 * (size_t)H] = cnt;
  } else {
    header[c] += SKIP ? cnt : (double)B;
    header[(size_t)H + c] += se2;
    header[2 * (size_t)H + c] += sabs;
    header[3 * (size_t)H + c] += sa;
    header[4 * (size_t)H + c] += sa2;
  }
}

// eval_fold_kernel for the five partials of a skip_missing call: the count comes from the slices, not from B
__global__ void __launch_bounds__(256) eval_fold_count_kernel(const double* __restrict__ partial, int slices, int H,
                                                              double* __restrict__ header) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int z = 0; z < slices; ++z) {
    const double* q = partial + (size_t)z * 5 * H + c;
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] += q[(size_t)k * H];
  }
  header[c] += s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) header[(size_t)(k + 1) * H + c] += s[k];
}

__global__ void __launch_bounds__(256) eval_stats_kernel(const double* __restrict__ header, int H, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  const double n = header[c];
  const double mse = header[(size_t)H + c] / n, mae = header[2 * (size_t)H + c] / n;
  const double mean = header[3 * (size_t)H + c] / n;
  const double var = header[4 * (size_t)H + c] / n - mean * mean;
  float* o = out + 4 * (size_t)c;
  o[0] = (float)sqrt(mse);
  o[1] = (float)mae;
  o[2] = (float)mean;
  o[3] = (float)sqrt(var < 0.0 ? 0.0 : var);   // (not fmax: a NaN variance stays NaN, as np.std's does)
}

}  // namespace

extern "C" {

int wgnn_eval_version(void) { return WGNN_EVAL_VERSION; }

size_t wgnn_eval_bytes(int32_t H) {
  if (H < 1) return 0;
  return ev_header_bytes(H) + align_up(sizeof(double) * 4 * (size_t)H * (size_t)ev_max_slices(H), 256);
}

int wgnn_eval_accum(const float* pred, const float* labels, int32_t B, int32_t T, int32_t H, float wind_min, float wind_max,
                    void* acc, float* abs_err, void* stream) {
  if (!pred || !labels || !acc) return WGNN_ERR_NULL;
  if (B < 1 || T < 1 || H < 1) return WGNN_ERR_SHAPE;
  const int64_t tiles = ev_tiles(H);
  int slices = (int)(((int64_t)B + EV_MIN_WINDOWS - 1) / EV_MIN_WINDOWS);
  if (slices > ev_max_slices(H)) slices = ev_max_slices(H);
  const int per_slice = (int)(((int64_t)B + slices - 1) / slices);
  slices = (int)(((int64_t)B + per_slice - 1) / per_slice);   // no empty slice
  double* header = (double*)acc;
  double* partial = slices > 1 ? (double*)((char*)acc + ev_header_bytes(H)) : nullptr;
  const double wmin = (double)wind_min, wrange = (double)wind_max - (double)wind_min;
  hipStream_t st = (hipStream_t)stream;
  const double bytes = (double)B * H * (abs_err ? 12.0 : 8.0);
  PROF_LAUNCH("eval_accum_kernel", 0.0, bytes, st,
              hipLaunchKernelGGL(eval_accum_kernel, dim3((unsigned)tiles, (unsigned)slices), dim3(EV_COLS, EV_ROWS), 0, st, pred,
                                 labels, B, T, H, per_slice, wmin, wrange, header, partial, abs_err));
  WGNN_CHECK_LAUNCH();
  if (partial) {
    PROF_LAUNCH("eval_fold_kernel", 0.0, 32.0 * H * slices, st,
                hipLaunchKernelGGL(eval_fold_kernel, dim3((unsigned)(((int64_t)H + 255) / 256)), dim3(256), 0, st, partial, slices, B,
                                   H, header));
    WGNN_CHECK_LAUNCH();
  }
  return WGNN_OK;
}

int wgnn_eval_accum_series(const float* pred, const float* Ls, int64_t ls_rows, const int32_t* starts, int32_t stride, int32_t B,
                           int32_t T, int32_t H, float wind_min, float wind_max, int32_t skip_missing, void* acc, float* abs_err,
                           void* stream) {
  if (!pred || !Ls || !acc) return WGNN_ERR_NULL;
  if (B < 1 || T < 1 || H < 1 || stride < 0 || (stride > 0 && starts)) return WGNN_ERR_SHAPE;
  if (stride == 0 && !starts) return WGNN_ERR_NULL;
  if (ls_rows < T || ls_rows * H >= (1ll << 31) || (!starts && (int64_t)(B - 1) * stride + T > ls_rows)) return WGNN_ERR_SHAPE;
  const int64_t tiles = ev_tiles(H);
  // skip_missing = 0: wgnn_eval_accum's slicing; else five partials per slice in the same private area
  const int cap = skip_missing ? (4 * ev_max_slices(H)) / 5 : ev_max_slices(H);
  int slices = (int)(((int64_t)B + EV_MIN_WINDOWS - 1) / EV_MIN_WINDOWS);
  if (slices > cap) slices = cap;
  if (slices < 1) slices = 1;
  const int per_slice = (int)(((int64_t)B + slices - 1) / slices);
  slices = (int)(((int64_t)B + per_slice - 1) / per_slice);   // no empty slice
  double* header = (double*)acc;
  double* partial = slices > 1 ? (double*)((char*)acc + ev_header_bytes(H)) : nullptr;
  const double wmin = (double)wind_min, wrange = (double)wind_max - (double)wind_min;
  const int last = (int)(ls_rows - T);
  hipStream_t st = (hipStream_t)stream;
  const double bytes = (double)B * H * (abs_err ? 12.0 : 8.0);
  if (skip_missing) {
    PROF_LAUNCH("eval_accum_series_kernel<skip>", 0.0, bytes, st,
                hipLaunchKernelGGL(eval_accum_series_kernel<true>, dim3((unsigned)tiles, (unsigned)slices), dim3(EV_COLS, EV_ROWS), 0,
                                   st, pred, Ls, starts, stride, last, B, T, H, per_slice, wmin, wrange, header, partial, abs_err));
  } else {
    PROF_LAUNCH("eval_accum_series_kernel", 0.0, bytes, st,
                hipLaunchKernelGGL(eval_accum_series_kernel<false>, dim3((unsigned)tiles, (unsigned)slices), dim3(EV_COLS, EV_ROWS), 0,
                                   st, pred, Ls, starts, stride, last, B, T, H, per_slice, wmin, wrange, header, partial, abs_err));
  }
  WGNN_CHECK_LAUNCH();
  if (partial) {
    const dim3 grid((unsigned)(((int64_t)H + 255) / 256));
    if (skip_missing) {
      PROF_LAUNCH("eval_fold_count_kernel", 0.0, 40.0 * H * slices, st,
                  hipLaunchKernelGGL(eval_fold_count_kernel, grid, dim3(256), 0, st, partial, slices, H, header));
    } else {
      PROF_LAUNCH("eval_fold_kernel", 0.0, 32.0 * H * slices, st,
                  hipLaunchKernelGGL(eval_fold_kernel, grid, dim3(256), 0, st, partial, slices, B, H, header));
    }
    WGNN_CHECK_LAUNCH();
  }
  return WGNN_OK;
}

int wgnn_eval_stats(const void* acc, int32_t H, float* out, void* stream) {
  if (!acc || !out) return WGNN_ERR_NULL;
  if (H < 1) return WGNN_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("eval_stats_kernel", 0.0, 56.0 * H, st,
              hipLaunchKernelGGL(eval_stats_kernel, dim3((unsigned)(((int64_t)H + 255) / 256)), dim3(256), 0, st,
                                 (const double*)acc, H, out));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}
}
