// Keeping the best parameters on the device (include/windgnn_best.h): the reference's rule, src/main.py:83-86, as a 256-byte
// record and a copy of the 8 parameter tensors into a caller-owned snapshot.
//
// The decision hazard.  Every workgroup of the copy must act on the same decision, and the decision reads best_loss, which a
// winning call rewrites: a workgroup that started late would compare the loss with the value its own call published and
// skip its share of the copy.  The form here splits the call: best_decide_kernel, ONE thread, compares and rewrites the record
// (best_loss, best_step, the counters and the flag `improved`); best_copy_kernel follows it on the stream and reads nothing
// but that flag, which no launch writes while it runs.  (The one-launch alternative -- two private copies of the decision
// state alternated by call parity -- needs the parity on the host, i.e. state outside the caller's record, which the record
// being plain copyable memory rules out)
//
// The copy.  One launch for all 8 tensors: the 8 (source, destination, length) triples travel by value, and the workgroups
// are dealt to the tensors in proportion to their length, at most BEST_MAX_WGS in all (8 per CU), each walking its tensor in a
// grid-stride loop of 16-byte loads and stores with 64-bit element indices (w_ih of BASELINE configs[4] alone is 2.6 GB).
// The tensors are views of a flat fp32 buffer at offsets such as 169, 182, 351: 4-byte aligned, lengths not multiples of 4.
// Per tensor the head up to the first 16-byte boundary of the SOURCE and the tail behind the last whole vector are moved as
// single floats by the tensor's first workgroup; no access is widened across a tensor's end.  If source and destination sit
// at different offsets inside 16 bytes no vector form serves both, and the tensor moves as single floats.
#include "common.h"

#include <stddef.h>

#include "../../include/windgnn_best.h"

namespace {

constexpr int BEST_THREADS = 256;
constexpr int BEST_MAX_WGS = 2048;       // 256 CUs x 8 workgroups
constexpr size_t BEST_BYTES = 256;

struct BestRecord {                      // the public words of include/windgnn_best.h
  double best_loss;
  int64_t best_step, calls, improvements;
  int32_t improved;
};
static_assert(sizeof(BestRecord) <= BEST_BYTES && offsetof(BestRecord, improved) == 32, "public layout");

struct BestCopyArgs {
  const float* src[8];
  float* dst[8];
  int64_t n[8];
  int wg0[9];                            // tensor t owns workgroups [wg0[t], wg0[t + 1])
};

__global__ void __launch_bounds__(64) best_init_kernel(unsigned long long* __restrict__ rec, double threshold) {
  const int i = threadIdx.x;
  if (i >= (int)(BEST_BYTES / 8)) return;
  unsigned long long w = 0ull;
  if (i == 0) w = (unsigned long long)__double_as_longlong(threshold);
  if (i == 1) w = ~0ull;                 // best_step = -1
  rec[i] = w;
}

__global__ void __launch_bounds__(64) best_decide_kernel(const float* __restrict__ loss, int64_t step, BestRecord* __restrict__ rec) {
  if (threadIdx.x != 0) return;
  const double l = (double)loss[0];
  const bool win = l < rec->best_loss;   // (false for a NaN loss)
  rec->calls += 1;
  if (win) {
    rec->best_loss = l;
    rec->best_step = step;
    rec->improvements += 1;
  }
  rec->improved = win ? 1 : 0;
}

__global__ void __launch_bounds__(BEST_THREADS) best_copy_kernel(BestCopyArgs a, const int32_t* __restrict__ improved) {
  if (improved[0] == 0) return;
  const int b = blockIdx.x;
  // the tensor this workgroup serves: selects over the by-value table (a dynamic index would put it into scratch)
  const float* src = a.src[0];
  float* dst = a.dst[0];
  int64_t n = a.n[0];
  int first = a.wg0[0], end = a.wg0[1];
#pragma unroll
  for (int t = 1; t < 8; ++t) {
    if (b >= a.wg0[t]) {
      src = a.src[t]; dst = a.dst[t]; n = a.n[t];
      first = a.wg0[t]; end = a.wg0[t + 1];
    }
  }
  const int64_t tid = (int64_t)(b - first) * BEST_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)(end - first) * BEST_THREADS;
  const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
  if (((sa ^ da) & 15) != 0) {           // no common 16-byte phase: single floats
    for (int64_t i = tid; i < n; i += stride) dst[i] = src[i];
    return;
  }
  int64_t head = (int64_t)(((16 - (sa & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t nv = (n - head) >> 2;    // whole 16-byte vectors behind the head
  const int64_t tail0 = head + 4 * nv;
  const f32x4* __restrict__ s4 = (const f32x4*)(src + head);
  f32x4* __restrict__ d4 = (f32x4*)(dst + head);
  int64_t i = tid;
  for (; i + 3 * stride < nv; i += 4 * stride) {   // four loads in flight per thread
    const f32x4 v0 = s4[i], v1 = s4[i + stride], v2 = s4[i + 2 * stride], v3 = s4[i + 3 * stride];
    d4[i] = v0; d4[i + stride] = v1; d4[i + 2 * stride] = v2; d4[i + 3 * stride] = v3;
  }
  for (; i < nv; i += stride) d4[i] = s4[i];
  if (b == first) {                      // head (< 4 floats) and tail (< 4 floats)
    const int k = threadIdx.x;
    if (k < head) dst[k] = src[k];
    if (k >= 64 && tail0 + (k - 64) < n && k - 64 < 4) dst[tail0 + (k - 64)] = src[tail0 + (k - 64)];
  }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

inline void slots(const wgnn_params& p, const float** out) {
  out[0] = p.conv1_weight; out[1] = p.conv1_bias; out[2] = p.conv2_weight; out[3] = p.conv2_bias;
  out[4] = p.w_ih; out[5] = p.w_hh; out[6] = p.b_ih; out[7] = p.b_hh;
}

}  // namespace

extern "C" {

int wgnn_best_version(void) { return WGNN_BEST_VERSION; }

size_t wgnn_best_bytes(void) { return BEST_BYTES; }

int wgnn_best_init(void* best, double threshold, void* stream) {
  if (!best) return WGNN_ERR_NULL;
  if (threshold != threshold) return WGNN_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("best_init_kernel", 0.0, (double)BEST_BYTES, st,
              hipLaunchKernelGGL(best_init_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)best, threshold));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

int wgnn_keep_best(const wgnn_dims* d, const float* loss, const wgnn_params* p, const wgnn_params* best_p, int64_t step,
                   void* best, void* stream) {
  if (!d || !loss || !p || !best_p || !best) return WGNN_ERR_NULL;
  const float *src[8], *dst[8];
  slots(*p, src);
  slots(*best_p, dst);
  for (int t = 0; t < 8; ++t)
    if (!src[t] || !dst[t]) return WGNN_ERR_NULL;
  if (wgnn_workspace_bytes(d) == 0 || step < 0) return WGNN_ERR_SHAPE;
  const int64_t F = d->F, G3 = 3 * (int64_t)d->H, I = (int64_t)d->S * F;
  const int64_t n[8] = {F * F, F, F * F, F, G3 * I, G3 * (int64_t)d->H, G3, G3};
  for (int t = 0; t < 8; ++t)
    for (int u = 0; u < 8; ++u)
      if (overlap(dst[t], sizeof(float) * (size_t)n[t], src[u], sizeof(float) * (size_t)n[u])) return WGNN_ERR_SHAPE;
  BestCopyArgs a;
  int64_t want[8], total = 0;
  for (int t = 0; t < 8; ++t) {
    a.src[t] = src[t]; a.dst[t] = (float*)dst[t]; a.n[t] = n[t];
    want[t] = (n[t] / 4 + BEST_THREADS - 1) / BEST_THREADS;   // one vector per thread ...
    if (want[t] < 1) want[t] = 1;
    total += want[t];
  }
  a.wg0[0] = 0;
  for (int t = 0; t < 8; ++t) {           // ... scaled down to the chip: the grid-stride loop takes the rest
    // (8 workgroups of the budget are held back for the floor of one per tensor, so the sum stays within BEST_MAX_WGS)
    int64_t w = total > BEST_MAX_WGS ? want[t] * (BEST_MAX_WGS - 8) / total : want[t];
    if (w < 1) w = 1;
    a.wg0[t + 1] = a.wg0[t] + (int)w;
  }
  double elems = 0.0;
  for (int t = 0; t < 8; ++t) elems += (double)n[t];
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH("best_decide_kernel", 0.0, 48.0, st,
              hipLaunchKernelGGL(best_decide_kernel, dim3(1), dim3(64), 0, st, loss, step, (BestRecord*)best));
  WGNN_CHECK_LAUNCH();
  PROF_LAUNCH("best_copy_kernel", 0.0, 8.0 * elems, st,
              hipLaunchKernelGGL(best_copy_kernel, dim3((unsigned)a.wg0[8]), dim3(BEST_THREADS), 0, st, a,
                                 (const int32_t*)((const char*)best + offsetof(BestRecord, improved))));
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}
}
