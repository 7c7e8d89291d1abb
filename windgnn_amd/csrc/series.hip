// Series mode (include/windgnn_series.h, include/windgnn_series_train.h): the entry points, their validation, and the fold
// kernel of the backward.
// The launches themselves are api.hip's (series_fwd / series_bwd): they run the materialised path's own front end, weight-gradient
// products and GCN backward on two of its layouts, with gru.hip's recurrences reading GI at series rows.
#include "common.h"
#include "../../include/windgnn_series.h"
#include "../../include/windgnn_series_train.h"

#include <cmath>

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

struct Plan {
  wgnn_dims front, rec;
  SeriesPlan sp;
};

// Everything about sd that needs no pointer: the order is shape, scope, then the element-count limits of both layouts
int plan(const wgnn_series_dims* sd, Plan* pl) {
  if (!sd) return WGNN_ERR_NULL;
  if (sd->rows < 1 || sd->T < 1 || sd->stride < 1 || sd->n < 1 || sd->S < 1 || sd->H < 1 || sd->F != 13) return WGNN_ERR_SHAPE;
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

int forward(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float* Y, float* last,
            float wind_min, float wind_max, void* stash, void* workspace, size_t workspace_bytes, void* stream) {
  Plan pl;
  const int rc = plan(sd, &pl);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || (!Y && !last) || !workspace || !complete(p)) return WGNN_ERR_NULL;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  return series_fwd(&pl.front, &pl.rec, sd->stride, A, Xs, p, Y, last, wind_min, wind_max, stash, workspace, pl.sp, stream);
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
  Plan pl;
  const int rc = plan(sd, &pl);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || !Y || !dY || !stash || !grads || !workspace || !complete(p) || !complete(grads)) return WGNN_ERR_NULL;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  return series_bwd(&pl.front, &pl.rec, sd->stride, A, Xs, p, Y, dY, stash, grads, workspace, pl.sp, stream);
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
  if (sd && !Y) return WGNN_ERR_NULL;      // before the dims, as in wgnn_series_fwd
  Plan pl;
  const int rc = plan(sd, &pl);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || !Ls || !loss_buf || !workspace || !complete(p)) return WGNN_ERR_NULL;
  if (ls_rows < (int64_t)(sd->n - 1) * sd->stride + sd->T || ls_rows * sd->H >= (1ll << 31)) return WGNN_ERR_SHAPE;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  return series_fwd_loss(&pl.front, &pl.rec, sd->stride, A, Xs, p, Ls, ls_rows, Y, stash, (float*)loss_buf, workspace, pl.sp,
                         stream);
}

int wgnn_series_bwd_mse(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                        const float* Ls, int64_t ls_rows, float grad_scale, const void* stash, const void* loss_buf, float* loss,
                        const wgnn_grads* grads, void* workspace, size_t workspace_bytes, void* stream) {
  Plan pl;
  const int rc = plan(sd, &pl);
  if (rc != WGNN_OK) return rc;
  if (!A || !Xs || !p || !Y || !Ls || !stash || !loss_buf || !loss || !grads || !workspace || !complete(p) || !complete(grads))
    return WGNN_ERR_NULL;
  if (ls_rows < (int64_t)(sd->n - 1) * sd->stride + sd->T || ls_rows * sd->H >= (1ll << 31) || !std::isfinite(grad_scale) ||
      !(grad_scale > 0.f))
    return WGNN_ERR_SHAPE;
  if (workspace_bytes < sizeof(float) * (pl.sp.ws_front + pl.sp.ws_rec)) return WGNN_ERR_WORKSPACE;
  return series_bwd_mse(&pl.front, &pl.rec, sd->stride, A, Xs, p, Y, Ls, ls_rows, grad_scale, stash, (const float*)loss_buf,
                        loss, grads, workspace, pl.sp, stream);
}

size_t wgnn_series_status_offset(const wgnn_series_dims* sd) {
  Plan pl;
  return plan(sd, &pl) == WGNN_OK ? sizeof(float) * pl.sp.ws_front : 0;
}

}  // extern "C"
