// Series mode (include/windgnn_series.h, include/windgnn_series_train.h, include/windgnn_series_at.h): the entry points, their
// validation, the fold kernels of the backward, the check of a table of window starts, and the kernels of the forward-only
// validation pass (include/windgnn_series_val.h): its finish and the three single-thread launches on its record.
// The launches themselves are api.hip's (series_fwd / series_bwd): they run the materialised path's own front end, weight-gradient
// products and GCN backward on two of its layouts, with gru.hip's recurrences reading GI at series rows.
#include "common.h"
#include "../../include/windgnn_series.h"
#include "../../include/windgnn_series_train.h"
#include "../../include/windgnn_series_at.h"
#include "../../include/windgnn_series_masked.h"
#include "../../include/windgnn_series_lossfn.h"
#include "../../include/windgnn_series_val.h"

#include <cmath>
#include <stddef.h>

namespace {

// dGIs[tau][c] = sum over w in [w_lo, w_hi] of dGI[w * T + tau - w * stride][c]: one thread per destination float4, the terms
// added in ascending w (store-then-sum per destination: no atomics, so the result does not depend on scheduling).  Every
// destination has at most ceil(T / stride) terms.  Columns >= G3 (the K padding the GEMMs read) and rows no window covers
// are written as zeros.
__global__ void __launch_bounds__(256) series_fold_kernel(const float* __restrict__ dGI, int n, int T, int stride, int rows,
                                                          int G3, int ld, float* __restrict__ dGIs) {
  const int ld4 = ld >> 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * ld4) return;
  const int tau = (int)(i / ld4), c = 4 * (int)(i % ld4);
  int w_hi = tau / stride;
  if (w_hi > n - 1) w_hi = n - 1;
  const int w_lo = tau >= T ? (tau - T) / stride + 1 : 0;      // smallest w with w * stride + T > tau
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int w = w_lo; w <= w_hi; ++w) {
    const f32x4 v = *(const f32x4*)(dGI + ((size_t)w * T + (size_t)(tau - w * stride)) * ld + c);
    acc += v;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (c + q >= G3) acc[q] = 0.f;
  *(f32x4*)(dGIs + (size_t)tau * ld + c) = acc;
}

// The fold for windows at a table of starts (include/windgnn_series_at.h).  starts is non-decreasing, so the windows that cover
// hour tau -- tau - T < starts[w] <= tau -- are the index range [lower_bound(tau - T + 1), upper_bound(tau)): two binary searches,
// then the terms in ascending w as above.  Duplicated starts make the range longer than T.  The searches stay inside [0, n) for
// any table; a term whose row tau - starts[w] is not in [0, T) (possible only in a table that series_starts_check_kernel has
// flagged) is skipped, so no table can take a read outside dGI.
__global__ void __launch_bounds__(256) series_fold_at_kernel(const float* __restrict__ dGI, const int* __restrict__ starts,
                                                             int n, int T, int rows, int G3, int ld,
                                                             float* __restrict__ dGIs) {
  const int ld4 = ld >> 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)rows * ld4) return;
  const int tau = (int)(i / ld4), c = 4 * (int)(i % ld4);
  int lo = 0, hi = n;                    // first w with starts[w] > tau - T
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] > tau - T) hi = mid;
    else lo = mid + 1;
  }
  const int w_lo = lo;
  hi = n;                                // first w >= w_lo with starts[w] > tau
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] > tau) hi = mid;
    else lo = mid + 1;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int w = w_lo; w < lo; ++w) {
    const int t = tau - starts[w];
    if ((unsigned)t < (unsigned)T) {
      const f32x4 v = *(const f32x4*)(dGI + ((size_t)w * T + (size_t)t) * ld + c);
      acc += v;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (c + q >= G3) acc[q] = 0.f;
  *(f32x4*)(dGIs + (size_t)tau * ld + c) = acc;
}

// One thread per window: a start outside [0, last] or below its predecessor is reported in the status word; nothing else is
// written.  (The kernels that read the table clamp; this is what tells the caller that they had to.)
__global__ void __launch_bounds__(256) series_starts_check_kernel(const int* __restrict__ starts, int n, int last,
                                                                  unsigned* status) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= n) return;
  const int s = starts[w];
  report_status(status, s < 0 || s > last || (w > 0 && s < starts[w - 1]), WGNN_STATUS_WINDOW_START);
}

// ---- validation (include/windgnn_series_val.h) ----
constexpr size_t VAL_BYTES = 256;
constexpr int VAL_THREADS = 512;         // the BPTT workgroup: the loss below is summed in its order

struct ValRecord {                       // the public words of include/windgnn_series_val.h
  double sum;
  unsigned long long count;
  double mean;
  float max_abs, loss;
  int64_t calls, passes, stale;
};
static_assert(sizeof(ValRecord) <= VAL_BYTES && offsetof(ValRecord, loss) == 28 && offsetof(ValRecord, stale) == 48, "public layout");

__device__ __forceinline__ void val_open(ValRecord* rec) {
  rec->sum = 0.0;
  rec->count = 0ull;
  rec->mean = __builtin_nan("");
  rec->max_abs = 0.f;
  rec->loss = __builtin_nanf("");
  rec->calls = 0;
}

__global__ void __launch_bounds__(64) val_init_kernel(unsigned long long* __restrict__ rec) {
  const int i = threadIdx.x;
  if (i < (int)(VAL_BYTES / 8)) rec[i] = 0ull;      // every byte, then the words that are not zero (the same thread order)
  __syncthreads();
  if (i == 0) val_open((ValRecord*)rec);
}

__global__ void __launch_bounds__(64) val_begin_kernel(ValRecord* __restrict__ rec) {
  if (threadIdx.x == 0) val_open(rec);
}

__global__ void __launch_bounds__(64) val_close_kernel(ValRecord* __restrict__ rec, const int32_t* __restrict__ improved) {
  if (threadIdx.x != 0) return;
  rec->passes += 1;
  if (improved) rec->stale = improved[0] ? 0 : rec->stale + 1;
}

// The loss of a forward-only pass from the statistics gru_fwd_kernel<.., LossFn> left in stat_part
// [nstat sums | nstat maxima | tag | 3 spec words | nstat counts]: ONE workgroup.  loss_out[0] restates the loss block of
// gru_bwd_kernel -- per-thread strided sum, xor tree over the lanes, the 8 waves ascending, times 1.0f / (float)m -- so that it
// comes out with the bits the training pair writes.  m is the sum of the counts for both values of fn.masked (the forward
// always writes them; with masked = 0 it is n (T - t_from) H, what the host forms for BPTT).  Statistics that are not this
// spec's forward's: NaN and WGNN_STATUS_NO_LOSS_STATS; m = 0: NaN and WGNN_STATUS_NO_LABELS.  For the record one thread adds
// the partial sums in ascending order in fp64 and the maxima, takes the counts' sum, and rewrites the public words.
__global__ void __launch_bounds__(VAL_THREADS) series_val_finish_kernel(const float* __restrict__ stat_part, int nstat, LossFn fn,
                                                                        float* __restrict__ loss_out, ValRecord* __restrict__ rec,
                                                                        unsigned* status) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned* w = (const unsigned*)(stat_part + 2 * (size_t)nstat + 1);
  const bool paired = stat_part[2 * (size_t)nstat] == WGNN_STATS_TAG_LOSSFN && w[0] == ((unsigned)fn.kind | (unsigned)fn.masked << 8) &&
                      w[1] == (fn.kind == 2 ? __float_as_uint(fn.delta) : 0u) && w[2] == (unsigned)fn.t_from;
  __shared__ unsigned long long cred[VAL_THREADS / 64];
  __shared__ float sred[VAL_THREADS / 64];
  const unsigned* cnts = masked_counts(stat_part, nstat);
  unsigned long long c = 0;
  float a = 0.f;
  if (paired)     // (another forward's buffer may be the shorter one: its counts are not even read)
    for (int i = threadIdx.x; i < nstat; i += VAL_THREADS) c += cnts[i];
  for (int i = threadIdx.x; i < nstat; i += VAL_THREADS) a += stat_part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o, 64);
    a += __shfl_xor(a, o, 64);
  }
  if (lane == 0) {
    cred[wave] = c;
    sred[wave] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    c = 0;
    a = 0.f;
#pragma unroll
    for (int v = 0; v < VAL_THREADS / 64; ++v) {
      c += cred[v];
      a += sred[v];
    }
    const float inv_n = c ? 1.0f / (float)c : __builtin_nanf("");
    if (loss_out) loss_out[0] = paired ? a * inv_n : __builtin_nanf("");
    if (status && !paired) atomicOr(status, WGNN_STATUS_NO_LOSS_STATS);
    if (status && paired && c == 0) atomicOr(status, WGNN_STATUS_NO_LABELS);
  }
  if (!rec) return;      // (uniform)
  // The record: onto the running sum term by term, so that calls cut at workgroup boundaries add the same terms in the same
  // order as one call.  The workgroup stages VAL_THREADS sums and maxima at a time in LDS; thread 0 alone adds them, ascending.
  __shared__ float ssum[VAL_THREADS], smax[VAL_THREADS];
  double sum = paired ? rec->sum : __builtin_nan("");
  float mx = rec->max_abs;
  for (int base = 0; base < nstat; base += VAL_THREADS) {
    const int i = base + (int)threadIdx.x;
    if (i < nstat) {
      ssum[threadIdx.x] = stat_part[i];
      smax[threadIdx.x] = stat_part[nstat + i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(VAL_THREADS, nstat - base);
      for (int k = 0; k < m; ++k) {
        sum += (double)ssum[k];
        mx = fmaxf(mx, smax[k]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const unsigned long long count = rec->count + c;
  const double mean = count ? sum / (double)count : __builtin_nan("");
  rec->sum = sum;
  rec->count = count;
  rec->mean = mean;
  rec->max_abs = mx;
  rec->loss = (float)mean;
  rec->calls += 1;
}

struct Plan {
  wgnn_dims front, rec;
  SeriesPlan sp;
};

// Everything about sd that needs no pointer: the order is shape, scope, then the element-count limits of both layouts
// at: the dims of include/windgnn_series_at.h -- stride = 0 means "a table", whose values size nothing
int plan(const wgnn_series_dims* sd, Plan* pl, bool at = false) {
  if (!sd) return WGNN_ERR_NULL;
  if (at) {   // (the fit below then reads T <= rows)
    if (sd->rows < 1 || sd->T < 1 || sd->stride != 0 || sd->n < 1 || sd->S < 1 || sd->H < 1 || sd->F != 13) return WGNN_ERR_SHAPE;
  } else {
    if (sd->rows < 1 || sd->T < 1 || sd->stride < 1 || sd->n < 1 || sd->S < 1 || sd->H < 1 || sd->F != 13) return WGNN_ERR_SHAPE;
  }
  if ((int64_t)(sd->n - 1) * sd->stride + sd->T > (int64_t)sd->rows) return WGNN_ERR_SHAPE;
  if (sd->math != WGNN_MATH_F32 || sd->io != WGNN_IO_F32 || sd->adj_format != WGNN_ADJ_DENSE || sd->S > 64 ||
      !gru_shape_supported(sd->H))
    return WGNN_ERR_UNSUPPORTED;
  pl->front = wgnn_dims{1, sd->rows, sd->S, sd->F, sd->H, sd->math, sd->adj_format, 0, sd->io};
  pl->rec = wgnn_dims{sd->n, sd->T, sd->S, sd->F, sd->H, sd->math, sd->adj_format, 0, sd->io};
  return series_plan(&pl->front, &pl->rec, &pl->sp);
}

bool all8(const float* const* v) {
  for (int t = 0; t < 8; ++t)
    if (!v[t]) return false;
  return true;
}
bool complete(const wgnn_params* p) {
  const float* v[8] = {p->conv1_weight, p->conv1_bias, p->conv2_weight, p->conv2_bias, p->w_ih, p->w_hh, p->b_ih, p->b_hh};
  return all8(v);
}
bool complete(const wgnn_grads* g) {
  const float* v[8] = {g->conv1_weight, g->conv1_bias, g->conv2_weight, g->conv2_bias, g->w_ih, g->w_hh, g->b_ih, g->b_hh};
  return all8(v);
}

int launch_starts_check(const wgnn_series_dims* sd, const int* starts, void* workspace, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("series_starts_check_kernel", 0.0, 4.0 * sd->n, st,
              hipLaunchKernelGGL(series_starts_check_kernel, dim3((unsigned)cdiv_i(sd->n, 256)), dim3(256), 0, st, starts, sd->n,
                                 sd->rows - sd->T, (unsigned*)workspace));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

// what the request of every entry point shares
SeriesCall request(const wgnn_series_dims* sd, const Plan& pl, const float* A, const float* Xs, const wgnn_params* p,
                   const int* starts, void* workspace, void* stream) {
  SeriesCall c = {};
  c.front = &pl.front; c.rec = &pl.rec; c.map.stride = sd->stride; c.map.starts = starts;
  c.A = A; c.Xs = Xs; c.p = p; c.workspace = workspace; c.sp = pl.sp; c.stream = stream;
  return c;
}

// at: the table entry points (starts is then required, and checked on the device ahead of everything else)
int forward(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float* Y, float* last,
            float wind_min, float wind_max, void* stash, void* workspace, size_t workspace_bytes, void* stream,
            bool at = false, const int* starts = nullptr) {
  Plan pl;
  int rc = plan(sd, &pl, at);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || (!Y && !last) || !workspace || !complete(p) || (at && !starts)) return WGNN_ERR_NULL;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  if (at && (rc = launch_starts_check(sd, starts, workspace, stream)) != WGNN_OK) return rc;
  SeriesCall c = request(sd, pl, A, Xs, p, starts, workspace, stream);
  c.Y = Y; c.last = last; c.wind_min = wind_min; c.wind_max = wind_max; c.stash = stash;
  return series_fwd(c);
}

int backward(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y, const float* dY,
             const void* stash, const wgnn_grads* grads, void* workspace, size_t workspace_bytes, void* stream, bool at = false,
             const int* starts = nullptr) {
  Plan pl;
  int rc = plan(sd, &pl, at);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || !Y || !dY || !stash || !grads || !workspace || !complete(p) || !complete(grads) || (at && !starts))
    return WGNN_ERR_NULL;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  if (at && (rc = launch_starts_check(sd, starts, workspace, stream)) != WGNN_OK) return rc;
  SeriesCall c = request(sd, pl, A, Xs, p, starts, workspace, stream);
  c.Y = (float*)Y; c.dY = dY; c.stash = (void*)stash; c.grads = grads;
  return series_bwd(c);
}

// the label rows a call needs: up to the last row a window covers -- any row of the series, for a table
bool labels_fit(const wgnn_series_dims* sd, bool at, int64_t ls_rows) {
  const int64_t need = at ? (int64_t)sd->rows : (int64_t)(sd->n - 1) * sd->stride + sd->T;
  return ls_rows >= need && ls_rows * sd->H < (1ll << 31);
}

// include/windgnn_series_lossfn.h: the caller's spec as the kernels' argument, or why not
int loss_spec(const wgnn_series_dims* sd, const wgnn_lossfn* fn, LossFn* out) {
  if (!fn) return WGNN_ERR_NULL;
  *out = LossFn{fn->kind, fn->kind == WGNN_LOSS_HUBER ? fn->delta : 0.f, fn->t_from, fn->masked};
  return lossfn_valid(*out, sd->T) ? WGNN_OK : WGNN_ERR_SHAPE;
}

int forward_loss(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Ls,
                 int64_t ls_rows, float* Y, void* stash, void* loss_buf, void* workspace, size_t workspace_bytes, void* stream,
                 bool at = false, const int* starts = nullptr, bool masked = false, bool lossfn = false,
                 const wgnn_lossfn* fn = nullptr) {
  if (sd && !Y) return WGNN_ERR_NULL;      // before the dims, as in wgnn_series_fwd
  Plan pl;
  int rc = plan(sd, &pl, at);
  if (rc != WGNN_OK) return rc;
  if ((masked || lossfn) && !at && starts) return WGNN_ERR_SHAPE;      // a table with a stride (windgnn_series_masked.h)
  if (!A || !Xs || !p || !Ls || !loss_buf || !workspace || !complete(p) || (at && !starts)) return WGNN_ERR_NULL;
  if (!labels_fit(sd, at, ls_rows)) return WGNN_ERR_SHAPE;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  LossFn spec{};
  if (lossfn && (rc = loss_spec(sd, fn, &spec)) != WGNN_OK) return rc;      // last of the host checks, ahead of any launch
  if (at && (rc = launch_starts_check(sd, starts, workspace, stream)) != WGNN_OK) return rc;
  SeriesCall c = request(sd, pl, A, Xs, p, starts, workspace, stream);
  c.Y = Y; c.stash = stash; c.Ls = Ls; c.map.ls_rows = ls_rows; c.loss_buf = (float*)loss_buf;
  c.masked = masked; c.lossfn = lossfn ? &spec : nullptr;
  return series_fwd(c);
}

int backward_mse(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                 const float* Ls, int64_t ls_rows, float grad_scale, const void* stash, const void* loss_buf, float* loss,
                 const wgnn_grads* grads, void* workspace, size_t workspace_bytes, void* stream, bool at = false,
                 const int* starts = nullptr, bool masked = false, bool lossfn = false, const wgnn_lossfn* fn = nullptr) {
  Plan pl;
  int rc = plan(sd, &pl, at);
  if (rc != WGNN_OK) return rc;
  if ((masked || lossfn) && !at && starts) return WGNN_ERR_SHAPE;
  if (!A || !Xs || !p || !Y || !Ls || !stash || !loss_buf || !loss || !grads || !workspace || !complete(p) || !complete(grads) ||
      (at && !starts))
    return WGNN_ERR_NULL;
  if (!labels_fit(sd, at, ls_rows) || !std::isfinite(grad_scale) || !(grad_scale > 0.f)) return WGNN_ERR_SHAPE;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  LossFn spec{};
  if (lossfn && (rc = loss_spec(sd, fn, &spec)) != WGNN_OK) return rc;
  if (at && (rc = launch_starts_check(sd, starts, workspace, stream)) != WGNN_OK) return rc;
  SeriesCall c = request(sd, pl, A, Xs, p, starts, workspace, stream);
  c.Y = (float*)Y; c.stash = (void*)stash; c.grads = grads; c.Ls = Ls; c.map.ls_rows = ls_rows; c.loss_buf = (float*)loss_buf;
  c.grad_scale = grad_scale; c.loss = loss; c.masked = masked; c.lossfn = lossfn ? &spec : nullptr;
  return series_bwd(c);
}

// include/windgnn_series_val.h: floats of the workspace -- [front end, forward alone | loss_buf | last rows]
struct ValLayout { size_t loss_buf, last, total; };
ValLayout val_layout(const wgnn_series_dims* sd, const Plan& pl) {
  ValLayout v;
  v.loss_buf = pl.sp.ws_front_fwd;
  v.last = v.loss_buf + align_up(series_masked_loss_floats(sd->n), 64);
  v.total = v.last + align_up((size_t)sd->n * sd->H, 64);
  return v;
}

int validate(const wgnn_series_dims* sd, const float* A, const float* Xs, const int* starts, const wgnn_params* p,
             const float* Ls, int64_t ls_rows, const wgnn_lossfn* fn, float wind_min, float wind_max, float* last, float* loss,
             void* val, void* workspace, size_t workspace_bytes, void* stream) {
  if (sd && !loss && !val) return WGNN_ERR_NULL;      // nothing to report: before the dims, as Y in wgnn_series_fwd_lossfn
  const bool at = sd && sd->stride == 0;
  Plan pl;
  int rc = plan(sd, &pl, at);
  if (rc != WGNN_OK) return rc;
  if (!at && starts) return WGNN_ERR_SHAPE;           // a table with a stride
  if (!A || !Xs || !p || !Ls || !workspace || !complete(p) || (at && !starts)) return WGNN_ERR_NULL;
  if (val && (uintptr_t)val % VAL_BYTES != 0) return WGNN_ERR_SHAPE;
  if (!labels_fit(sd, at, ls_rows)) return WGNN_ERR_SHAPE;
  const ValLayout vl = val_layout(sd, pl);
  if (workspace_bytes < sizeof(float) * vl.total) return WGNN_ERR_WORKSPACE;
  LossFn spec{};
  if ((rc = loss_spec(sd, fn, &spec)) != WGNN_OK) return rc;      // last of the host checks, ahead of any launch
  if (at && (rc = launch_starts_check(sd, starts, workspace, stream)) != WGNN_OK) return rc;
  float* ws = (float*)workspace;
  float* loss_buf = ws + vl.loss_buf;
  SeriesCall c = request(sd, pl, A, Xs, p, starts, workspace, stream);   // last and Ls, no stash: a forward alone
  c.last = last ? last : ws + vl.last; c.wind_min = wind_min; c.wind_max = wind_max;
  c.Ls = Ls; c.map.ls_rows = ls_rows; c.loss_buf = loss_buf; c.lossfn = &spec;
  rc = series_fwd(c);
  if (rc != WGNN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = gru_blocks(sd->n);
  PROF_LAUNCH("series_val_finish_kernel", 3.0 * nb, 12.0 * nb, st,
              hipLaunchKernelGGL(series_val_finish_kernel, dim3(1), dim3(VAL_THREADS), 0, st, loss_buf, nb, spec, loss,
                                 (ValRecord*)val, (unsigned*)workspace));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

}  // namespace

int launch_series_fold(const float* dGI, int n, int T, int stride, int rows, int G3, int ld, float* dGIs, hipStream_t st) {
  if (ld % 4 != 0 || G3 > ld || stride < 1) return WGNN_ERR_SHAPE;
  const size_t items = (size_t)rows * (ld / 4);
  const int terms = cdiv_i(T, stride);
  PROF_LAUNCH("series_fold_kernel", (double)items * 4 * terms, 4.0 * items * 4 * (terms + 1), st,
              hipLaunchKernelGGL(series_fold_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, dGI, n, T, stride,
                                 rows, G3, ld, dGIs));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

int launch_series_fold_at(const float* dGI, const int* starts, int n, int T, int rows, int G3, int ld, float* dGIs,
                          hipStream_t st) {
  if (ld % 4 != 0 || G3 > ld || !starts) return WGNN_ERR_SHAPE;
  const size_t items = (size_t)rows * (ld / 4);
  const double terms = (double)n * T / rows;      // mean coverage of an hour
  PROF_LAUNCH("series_fold_at_kernel", (double)items * 4 * terms, 4.0 * items * 4 * (terms + 1), st,
              hipLaunchKernelGGL(series_fold_at_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, dGI, starts, n, T,
                                 rows, G3, ld, dGIs));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

extern "C" {

int wgnn_series_version(void) { return WGNN_SERIES_VERSION; }

size_t wgnn_series_workspace_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl) == WGNN_OK ? sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec) : 0;
}

size_t wgnn_series_stash_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl) == WGNN_OK ? sizeof(float) * (pl.sp.st_front + pl.sp.st_rec) : 0;
}

int wgnn_series_fwd(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float* Y, void* stash,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (sd && !Y) return WGNN_ERR_NULL;
  return forward(sd, A, Xs, p, Y, nullptr, 0.f, 1.f, stash, workspace, workspace_bytes, stream);
}

int wgnn_series_fwd_last(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float wind_min,
                         float wind_max, float* last, void* workspace, size_t workspace_bytes, void* stream) {
  if (sd && !last) return WGNN_ERR_NULL;
  return forward(sd, A, Xs, p, nullptr, last, wind_min, wind_max, nullptr, workspace, workspace_bytes, stream);
}

int wgnn_series_bwd(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                    const float* dY, const void* stash, const wgnn_grads* grads, void* workspace, size_t workspace_bytes,
                    void* stream) {
  return backward(sd, A, Xs, p, Y, dY, stash, grads, workspace, workspace_bytes, stream);
}

// ---- include/windgnn_series_train.h ----
int wgnn_series_train_version(void) { return WGNN_SERIES_TRAIN_VERSION; }

size_t wgnn_series_loss_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl) == WGNN_OK ? sizeof(float) * series_loss_floats(sd->n) : 0;
}

int wgnn_series_fwd_loss(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Ls,
                         int64_t ls_rows, float* Y, void* stash, void* loss_buf, void* workspace, size_t workspace_bytes,
                         void* stream) {
  return forward_loss(sd, A, Xs, p, Ls, ls_rows, Y, stash, loss_buf, workspace, workspace_bytes, stream);
}

int wgnn_series_bwd_mse(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                        const float* Ls, int64_t ls_rows, float grad_scale, const void* stash, const void* loss_buf, float* loss,
                        const wgnn_grads* grads, void* workspace, size_t workspace_bytes, void* stream) {
  return backward_mse(sd, A, Xs, p, Y, Ls, ls_rows, grad_scale, stash, loss_buf, loss, grads, workspace, workspace_bytes, stream);
}

size_t wgnn_series_status_offset(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl) == WGNN_OK ? sizeof(float) * pl.sp.ws_front : 0;
}

// ---- include/windgnn_series_at.h ----
int wgnn_series_at_version(void) { return WGNN_SERIES_AT_VERSION; }

size_t wgnn_series_at_workspace_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, true) == WGNN_OK ? sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec) : 0;
}

size_t wgnn_series_at_stash_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, true) == WGNN_OK ? sizeof(float) * (pl.sp.st_front + pl.sp.st_rec) : 0;
}

size_t wgnn_series_at_loss_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, true) == WGNN_OK ? sizeof(float) * series_loss_floats(sd->n) : 0;
}

size_t wgnn_series_at_status_offset(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, true) == WGNN_OK ? sizeof(float) * pl.sp.ws_front : 0;
}

int wgnn_series_fwd_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                       float* Y, void* stash, void* workspace, size_t workspace_bytes, void* stream) {
  if (sd && !Y) return WGNN_ERR_NULL;
  return forward(sd, A, Xs, p, Y, nullptr, 0.f, 1.f, stash, workspace, workspace_bytes, stream, true, starts);
}

int wgnn_series_fwd_last_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                            const wgnn_params* p, float wind_min, float wind_max, float* last, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (sd && !last) return WGNN_ERR_NULL;
  return forward(sd, A, Xs, p, nullptr, last, wind_min, wind_max, nullptr, workspace, workspace_bytes, stream, true, starts);
}

int wgnn_series_bwd_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                       const float* Y, const float* dY, const void* stash, const wgnn_grads* grads, void* workspace,
                       size_t workspace_bytes, void* stream) {
  return backward(sd, A, Xs, p, Y, dY, stash, grads, workspace, workspace_bytes, stream, true, starts);
}

int wgnn_series_fwd_loss_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                            const wgnn_params* p, const float* Ls, int64_t ls_rows, float* Y, void* stash, void* loss_buf,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return forward_loss(sd, A, Xs, p, Ls, ls_rows, Y, stash, loss_buf, workspace, workspace_bytes, stream, true, starts);
}

int wgnn_series_bwd_mse_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                           const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return backward_mse(sd, A, Xs, p, Y, Ls, ls_rows, grad_scale, stash, loss_buf, loss, grads, workspace, workspace_bytes, stream,
                      true, starts);
}

// ---- include/windgnn_series_masked.h (wgnn_eval_accum_series: eval.hip) ----
int wgnn_series_masked_version(void) { return WGNN_SERIES_MASKED_VERSION; }

size_t wgnn_series_masked_loss_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, sd && sd->stride == 0) == WGNN_OK ? sizeof(float) * series_masked_loss_floats(sd->n) : 0;
}

int wgnn_series_fwd_loss_masked(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                                const wgnn_params* p, const float* Ls, int64_t ls_rows, float* Y, void* stash, void* loss_buf,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return forward_loss(sd, A, Xs, p, Ls, ls_rows, Y, stash, loss_buf, workspace, workspace_bytes, stream, sd && sd->stride == 0,
                      starts, true);
}

int wgnn_series_bwd_mse_masked(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                               const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                               const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return backward_mse(sd, A, Xs, p, Y, Ls, ls_rows, grad_scale, stash, loss_buf, loss, grads, workspace, workspace_bytes, stream,
                      sd && sd->stride == 0, starts, true);
}

// ---- include/windgnn_series_lossfn.h ----
int wgnn_series_lossfn_version(void) { return WGNN_SERIES_LOSSFN_VERSION; }

size_t wgnn_series_lossfn_bytes(const wgnn_series_dims* sd) { return wgnn_series_masked_loss_bytes(sd); }

int wgnn_series_fwd_lossfn(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Ls, int64_t ls_rows, const wgnn_lossfn* fn, float* Y, void* stash,
                           void* loss_buf, void* workspace, size_t workspace_bytes, void* stream) {
  return forward_loss(sd, A, Xs, p, Ls, ls_rows, Y, stash, loss_buf, workspace, workspace_bytes, stream, sd && sd->stride == 0,
                      starts, false, true, fn);
}

int wgnn_series_bwd_lossfn(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                           const wgnn_lossfn* fn, const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads,
                           void* workspace, size_t workspace_bytes, void* stream) {
  return backward_mse(sd, A, Xs, p, Y, Ls, ls_rows, grad_scale, stash, loss_buf, loss, grads, workspace, workspace_bytes, stream,
                      sd && sd->stride == 0, starts, false, true, fn);
}

// ---- include/windgnn_series_val.h ----
int wgnn_series_val_version(void) { return WGNN_SERIES_VAL_VERSION; }

size_t wgnn_val_bytes(void) { return VAL_BYTES; }

int wgnn_val_init(void* val, void* stream) {
  if (!val) return WGNN_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("val_init_kernel", 0.0, (double)VAL_BYTES, st,
              hipLaunchKernelGGL(val_init_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)val));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

int wgnn_val_begin(void* val, void* stream) {
  if (!val) return WGNN_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("val_begin_kernel", 0.0, 40.0, st,
              hipLaunchKernelGGL(val_begin_kernel, dim3(1), dim3(64), 0, st, (ValRecord*)val));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

size_t wgnn_series_val_workspace_bytes(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl, sd && sd->stride == 0) == WGNN_OK ? sizeof(float) * val_layout(sd, pl).total : 0;
}

int wgnn_series_val(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                    const float* Ls, int64_t ls_rows, const wgnn_lossfn* fn, float wind_min, float wind_max, float* last,
                    float* loss, void* val, void* workspace, size_t workspace_bytes, void* stream) {
  return validate(sd, A, Xs, starts, p, Ls, ls_rows, fn, wind_min, wind_max, last, loss, val, workspace, workspace_bytes, stream);
}

int wgnn_val_close(void* val, const void* best, void* stream) {
  if (!val) return WGNN_ERR_NULL;
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("val_close_kernel", 0.0, 24.0, st,
              hipLaunchKernelGGL(val_close_kernel, dim3(1), dim3(64), 0, st, (ValRecord*)val,
                                 best ? (const int32_t*)((const char*)best + 32) : nullptr));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

}  // extern "C"
