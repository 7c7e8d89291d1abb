// Stand-alone host-sanitizer driver for include/windgnn_series_masked.h (built and run by tools/asan_series_masked.py, CPU only):
// every validation path of the three entry points on fake device pointers.  Each call must be refused on the host, before any
// HIP call -- on a machine without a GPU a call that got past its checks would fail to launch instead of returning the code
// expected here.  Exit status 0 = every refusal as expected (and no sanitizer report, which aborts with its own status).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../include/windgnn_series_masked.h"

namespace {

int failures = 0;
void expect(int got, int want, const char* what, int line) {
  if (got != want) {
    std::printf("line %d: %s returned %d, expected %d\n", line, what, got, want);
    ++failures;
  }
}
#define EXPECT(call, want) expect((call), (want), #call, __LINE__)

template <typename T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

struct Args {
  wgnn_series_dims sd;
  const wgnn_series_dims* sdp;
  const float *A, *Xs, *Ls, *Y_in;
  const int32_t* starts;
  wgnn_params p;
  const wgnn_params* pp;
  wgnn_grads g;
  const wgnn_grads* gp;
  float *Y, *loss;
  void *stash, *loss_buf, *ws;
  int64_t ls_rows;
  size_t ws_bytes;
  float grad_scale;
};

Args make(int stride) {
  Args a{};
  a.sd = wgnn_series_dims{14, 5, stride, 4, 7, 13, 21, WGNN_MATH_F32, WGNN_ADJ_DENSE, 0, WGNN_IO_F32};
  a.sdp = &a.sd;
  a.A = fake<const float>(8192); a.Xs = fake<const float>(1u << 20); a.Ls = fake<const float>(1u << 22);
  a.starts = stride == 0 ? fake<const int32_t>(1u << 21) : nullptr;
  const float* w = fake<const float>(4096);
  a.p = wgnn_params{};
  a.p.conv1_weight = a.p.conv1_bias = a.p.conv2_weight = a.p.conv2_bias = a.p.w_ih = a.p.w_hh = a.p.b_ih = a.p.b_hh = w;
  a.pp = &a.p;
  float* gw = fake<float>(4096);
  a.g = wgnn_grads{};
  a.g.conv1_weight = a.g.conv1_bias = a.g.conv2_weight = a.g.conv2_bias = a.g.w_ih = a.g.w_hh = a.g.b_ih = a.g.b_hh = gw;
  a.gp = &a.g;
  a.Y = fake<float>(1u << 24); a.loss = fake<float>(1u << 26);
  a.stash = fake<void>(1u << 28); a.loss_buf = fake<void>(1u << 30); a.ws = fake<void>(1ull << 40);
  a.ls_rows = 14; a.ws_bytes = (size_t)1 << 40; a.grad_scale = 1.f;
  return a;
}

int fwd(const Args& a) {
  return wgnn_series_fwd_loss_masked(a.sdp, a.A, a.Xs, a.starts, a.pp, a.Ls, a.ls_rows, a.Y, a.stash, a.loss_buf, a.ws, a.ws_bytes,
                                     nullptr);
}
int bwd(const Args& a) {
  return wgnn_series_bwd_mse_masked(a.sdp, a.A, a.Xs, a.starts, a.pp, a.Y, a.Ls, a.ls_rows, a.grad_scale, a.stash, a.loss_buf, a.loss,
                                    a.gp, a.ws, a.ws_bytes, nullptr);
}
void both(const Args& a, int want, const char* what, int line) {
  expect(fwd(a), want, what, line);
  expect(bwd(a), want, what, line);
}
#define BOTH(a, want) both((a), (want), #a " (fwd, bwd)", __LINE__)

void series_pair(int stride) {
  // NULL pointers
  { Args a = make(stride); a.sdp = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.A = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.Xs = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.pp = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.p.w_hh = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.Ls = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.Y = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.loss_buf = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.ws = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(stride); a.loss = nullptr; EXPECT(bwd(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.stash = nullptr; EXPECT(bwd(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.gp = nullptr; EXPECT(bwd(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.g.b_ih = nullptr; EXPECT(bwd(a), WGNN_ERR_NULL); }
  // bad dims: shape before scope
  { Args a = make(stride); a.sd.T = 15; a.ls_rows = 1 << 20; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.T = 0; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.n = 0; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.rows = 0; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.F = 12; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.S = 0; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.H = 0; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.math = 1; a.sd.F = 12; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.math = 1; BOTH(a, WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.adj_format = 1; a.sd.nnz = 20; BOTH(a, WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.H = 129; BOTH(a, WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.S = 65; BOTH(a, WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.io = 1; BOTH(a, WGNN_ERR_UNSUPPORTED); }
  // a short label series, and one past the 32-bit offsets
  { Args a = make(stride); a.ls_rows = stride == 0 ? 13 : 3 * stride + 5 - 1; BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.ls_rows = ((int64_t)1 << 31) / 21 + 1; BOTH(a, WGNN_ERR_SHAPE); }
  // grad_scale
  const float bad_scale[] = {0.f, -1.f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  for (float s : bad_scale) {
    Args a = make(stride);
    a.grad_scale = s;
    EXPECT(bwd(a), WGNN_ERR_SHAPE);
  }
  // a workspace one byte short
  {
    Args a = make(stride);
    const size_t need = stride == 0 ? wgnn_series_at_workspace_bytes(&a.sd) : wgnn_series_workspace_bytes(&a.sd);
    if (need == 0) { std::printf("stride %d: workspace query refused valid dims\n", stride); ++failures; }
    a.ws_bytes = need - 1;
    BOTH(a, WGNN_ERR_WORKSPACE);
    const size_t plain = stride == 0 ? wgnn_series_at_loss_bytes(&a.sd) : wgnn_series_loss_bytes(&a.sd);
    if (wgnn_series_masked_loss_bytes(&a.sd) != plain + 4) { std::printf("stride %d: masked loss bytes\n", stride); ++failures; }
  }
}

int eval(const float* pred, const float* Ls, int64_t ls_rows, const int32_t* starts, int stride, int B, int T, int H, void* acc) {
  return wgnn_eval_accum_series(pred, Ls, ls_rows, starts, stride, B, T, H, 0.f, 1.f, 1, acc, nullptr, nullptr);
}

}  // namespace

int main() {
  if (wgnn_series_masked_version() != WGNN_SERIES_MASKED_VERSION) { std::printf("version\n"); return 1; }
  series_pair(0);
  series_pair(1);
  series_pair(3);
  // the two forms do not mix
  { Args a = make(1); a.starts = fake<const int32_t>(1u << 21); BOTH(a, WGNN_ERR_SHAPE); }
  { Args a = make(0); a.starts = nullptr; BOTH(a, WGNN_ERR_NULL); }
  { Args a = make(-1); BOTH(a, WGNN_ERR_SHAPE); }
  if (wgnn_series_masked_loss_bytes(nullptr) != 0) { std::printf("loss bytes of NULL dims\n"); ++failures; }

  const float *pred = fake<const float>(1u << 20), *Ls = fake<const float>(1u << 22);
  const int32_t* table = fake<const int32_t>(1u << 21);
  void* acc = fake<void>(1u << 24);
  EXPECT(eval(nullptr, Ls, 40, nullptr, 1, 8, 5, 21, acc), WGNN_ERR_NULL);
  EXPECT(eval(pred, nullptr, 40, nullptr, 1, 8, 5, 21, acc), WGNN_ERR_NULL);
  EXPECT(eval(pred, Ls, 40, nullptr, 1, 8, 5, 21, nullptr), WGNN_ERR_NULL);
  EXPECT(eval(pred, Ls, 40, nullptr, 0, 8, 5, 21, acc), WGNN_ERR_NULL);          // a table's call without the table
  EXPECT(eval(pred, Ls, 40, table, 1, 8, 5, 21, acc), WGNN_ERR_SHAPE);           // a stride with a table
  EXPECT(eval(pred, Ls, 40, nullptr, -1, 8, 5, 21, acc), WGNN_ERR_SHAPE);
  EXPECT(eval(pred, Ls, 40, nullptr, 1, 0, 5, 21, acc), WGNN_ERR_SHAPE);
  EXPECT(eval(pred, Ls, 40, nullptr, 1, 8, 0, 21, acc), WGNN_ERR_SHAPE);
  EXPECT(eval(pred, Ls, 40, nullptr, 1, 8, 5, 0, acc), WGNN_ERR_SHAPE);
  EXPECT(eval(pred, Ls, 11, nullptr, 1, 8, 5, 21, acc), WGNN_ERR_SHAPE);         // (B - 1) * stride + T = 12 rows needed
  EXPECT(eval(pred, Ls, 18, nullptr, 2, 8, 5, 21, acc), WGNN_ERR_SHAPE);
  EXPECT(eval(pred, Ls, 4, table, 0, 8, 5, 21, acc), WGNN_ERR_SHAPE);            // ls_rows < T
  EXPECT(eval(pred, Ls, ((int64_t)1 << 31) / 21 + 1, nullptr, 1, 8, 5, 21, acc), WGNN_ERR_SHAPE);

  if (failures) {
    std::printf("asan_series_masked: %d unexpected results\n", failures);
    return 1;
  }
  std::printf("asan_series_masked: every refusal of the masked entry points came back from the host, no report\n");
  return 0;
}
