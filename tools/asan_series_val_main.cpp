// Stand-alone host-sanitizer driver for include/windgnn_series_val.h (built and run by tools/asan_series_val.py, CPU only): every
// validation path of wgnn_series_val and of the record's three calls on fake device pointers.  Each call must be refused on the
// host, before any HIP call -- on a machine without a GPU a call that got past its checks would fail to launch instead of
// returning the code expected here.  Exit status 0 = every refusal as expected (and no sanitizer report, which aborts with its
// own status).
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../include/windgnn_series_val.h"

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
  const float *A, *Xs, *Ls;
  const int32_t* starts;
  wgnn_params p;
  const wgnn_params* pp;
  wgnn_lossfn fn;
  const wgnn_lossfn* fnp;
  float *last, *loss;
  void *val, *ws;
  int64_t ls_rows;
  size_t ws_bytes;
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
  a.fn = wgnn_lossfn{WGNN_LOSS_L1, 0.f, 0, 0};
  a.fnp = &a.fn;
  a.last = fake<float>(1u << 24); a.loss = fake<float>(1u << 26);
  a.val = fake<void>(1ull << 33); a.ws = fake<void>(1ull << 40);
  a.ls_rows = 14; a.ws_bytes = (size_t)1 << 40;
  return a;
}

int run(const Args& a) {
  return wgnn_series_val(a.sdp, a.A, a.Xs, a.starts, a.pp, a.Ls, a.ls_rows, a.fnp, 0.f, 1.f, a.last, a.loss, a.val, a.ws, a.ws_bytes,
                         nullptr);
}

void entry_point(int stride) {
  // NULL pointers; loss and val both NULL: nothing to report
  { Args a = make(stride); a.sdp = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.A = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.Xs = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.pp = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.p.w_hh = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.Ls = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.ws = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.fnp = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(stride); a.loss = nullptr; a.val = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  // bad dims: shape before scope
  { Args a = make(stride); a.sd.T = 15; a.ls_rows = 1 << 20; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.T = 0; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.n = 0; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.rows = 0; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.F = 12; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.S = 0; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.H = 0; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.sd.math = 1; EXPECT(run(a), WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.adj_format = 1; a.sd.nnz = 20; EXPECT(run(a), WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.H = 129; EXPECT(run(a), WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.S = 65; EXPECT(run(a), WGNN_ERR_UNSUPPORTED); }
  { Args a = make(stride); a.sd.io = 1; EXPECT(run(a), WGNN_ERR_UNSUPPORTED); }
  // a record off its 256-byte alignment, a short label series, and one past the 32-bit offsets
  { Args a = make(stride); a.val = fake<void>((1ull << 33) + 128); EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.ls_rows = stride == 0 ? 13 : 3 * stride + 5 - 1; EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(stride); a.ls_rows = ((int64_t)1 << 31) / 21 + 1; EXPECT(run(a), WGNN_ERR_SHAPE); }
  // a workspace one byte short: with either output alone, with a NULL `last`, and ahead of a bad spec
  {
    Args a = make(stride);
    const size_t need = wgnn_series_val_workspace_bytes(&a.sd);
    const size_t train = stride == 0 ? wgnn_series_at_workspace_bytes(&a.sd) : wgnn_series_workspace_bytes(&a.sd);
    if (need == 0 || need >= train) { std::printf("stride %d: workspace bytes %zu (training %zu)\n", stride, need, train); ++failures; }
    a.ws_bytes = need - 1;
    EXPECT(run(a), WGNN_ERR_WORKSPACE);
    { Args b = a; b.loss = nullptr; EXPECT(run(b), WGNN_ERR_WORKSPACE); }
    { Args b = a; b.val = nullptr; b.last = nullptr; EXPECT(run(b), WGNN_ERR_WORKSPACE); }
    { Args b = a; b.fn.kind = 3; EXPECT(run(b), WGNN_ERR_WORKSPACE); }
  }
  // the spec, each bad field on its own (T = 5)
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const wgnn_lossfn bad[] = {{-1, 0.f, 0, 0}, {3, 0.f, 0, 0}, {0, 0.f, 0, 2}, {1, 0.f, 0, -1}, {1, 0.f, -1, 0}, {1, 0.f, 5, 0},
                             {2, 0.f, 0, 0}, {2, -0.25f, 0, 1}, {2, inf, 0, 0}, {2, nan, 2, 0}};
  for (const wgnn_lossfn& f : bad) {
    Args a = make(stride);
    a.fn = f;
    EXPECT(run(a), WGNN_ERR_SHAPE);
  }
}

}  // namespace

int main() {
  if (wgnn_series_val_version() != WGNN_SERIES_VAL_VERSION) { std::printf("version\n"); return 1; }
  if (wgnn_val_bytes() == 0 || wgnn_val_bytes() % 256 != 0) { std::printf("record bytes\n"); return 1; }
  entry_point(0);
  entry_point(1);
  entry_point(3);
  // the two forms do not mix
  { Args a = make(1); a.starts = fake<const int32_t>(1u << 21); EXPECT(run(a), WGNN_ERR_SHAPE); }
  { Args a = make(0); a.starts = nullptr; EXPECT(run(a), WGNN_ERR_NULL); }
  { Args a = make(-1); EXPECT(run(a), WGNN_ERR_SHAPE); }
  if (wgnn_series_val_workspace_bytes(nullptr) != 0) { std::printf("workspace bytes of NULL dims\n"); ++failures; }
  // the record's own calls
  EXPECT(wgnn_val_init(nullptr, nullptr), WGNN_ERR_NULL);
  EXPECT(wgnn_val_begin(nullptr, nullptr), WGNN_ERR_NULL);
  EXPECT(wgnn_val_close(nullptr, fake<const void>(1ull << 34), nullptr), WGNN_ERR_NULL);

  if (failures) {
    std::printf("asan_series_val: %d unexpected results\n", failures);
    return 1;
  }
  std::printf("asan_series_val: every refusal of the validation entry points came back from the host, no report\n");
  return 0;
}
