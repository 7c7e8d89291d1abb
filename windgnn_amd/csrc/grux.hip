// GRU recurrence, split-fp16 ("f16x3") MFMA, weights resident in REGISTERS.
//
// Reference: nn.GRU (1 layer, batch_first, h0 = 0, gates r,z,n) at
// src/step6_gcn_gru_combined_model.py:11,23 and its BPTT (src/main.py:79).
//
// One workgroup = 16 windows for all T steps, 8 waves; wave w owns hidden units [16w, 16w+16) for
// all three gates, so the gate math is lane-local in the 16x16 C layout.  Each wave keeps its slice
// of W_hh (forward: B operand [k = h index][n = gate unit]; backward: W_hh^T slice
// [k = gate row][n = hidden unit]) as fp16 hi/lo MFMA fragments in VGPRs for the whole launch
// (96 / 80 registers at H = 102); LDS only carries the 16 x H state (h, or dgh in the backward)
// between waves, stored as fp16 hi/lo rows padded to a conflict-free stride.
// Backward values (dY ~ 1e-9) are multiplied by the power of two scales[0] on load and written
// SCALED to dGI/dGH; the weight-gradient GEMMs un-scale in their epilogues.
#include "common.h"
#include <type_traits>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int MB = 16;
constexpr int NTHREADS = 512;
// 16-byte components of a gate-stash record: r | z | n | gh_n, plus h_t itself when Y on the wire is 16-bit (the BPTT
// kernel then takes h_{t-1} from the stash: the rounded Y is not the forward's hidden state)
__host__ __device__ constexpr int grec(int io) { return io ? 5 : 4; }

struct Frag { h8 hi, lo; };

__device__ __forceinline__ f32x4 mfma_x(h8 a, h8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// X3: split-fp16 three-pass product; !X3: plain fp16 operands, one pass ("f16" math mode)
template <bool X3>
__device__ __forceinline__ f32x4 mfma3(const Frag& a, const Frag& b, f32x4 c) {
  if (X3) {
    c = mfma_x(a.lo, b.hi, c);
    c = mfma_x(a.hi, b.lo, c);
  }
  c = mfma_x(a.hi, b.hi, c);
  return c;
}
// hi = fp16(x) (v_cvt_pk_f16_f32, 2 values per instruction), lo = fp16(x - hi) with the difference
// formed by v_fma_mix_f32 reading hi straight out of the packed register: 2 VALU per value instead
// of the 3 hipcc emits for the C expression (these kernels are VALU-issue-bound on exactly this).
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
  float t0, t1;
  asm("v_cvt_pk_f16_f32 %0, %4, %5\n\t"
      "v_fma_mix_f32 %2, %0, -1.0, %4 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mix_f32 %3, %0, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_cvt_pk_f16_f32 %1, %2, %3\n\t"
      "s_nop 1"   // VALU write -> MFMA operand read needs 2 wait states; hipcc pads nothing inside/after asm
      : "=&v"(hi), "=&v"(lo), "=&v"(t0), "=&v"(t1)
      : "v"(x0), "v"(x1));
}
__device__ __forceinline__ Frag split_vals(const float (&x)[8]) {   // weights: once per launch, both halves
  typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
  u32x4v hi, lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned h, l;
    split2(x[2 * j], x[2 * j + 1], h, l);
    hi[j] = h;
    lo[j] = l;
  }
  Frag f;
  f.hi = __builtin_bit_cast(h8, hi);
  f.lo = __builtin_bit_cast(h8, lo);
  return f;
}
// io-typed element access (wgnn_io): 0 = fp32, 1 = fp16, 2 = bf16 (round to nearest even on store)
__device__ __forceinline__ float io_load(const void* p, int idx, int io) {
  if (io == 0) return ((const float*)p)[idx];
  const unsigned short u = ((const unsigned short*)p)[idx];
  if (io == 1) return (float)__builtin_bit_cast(_Float16, u);
  return __builtin_bit_cast(float, (unsigned)u << 16);
}
__device__ __forceinline__ void io_store(void* p, int idx, float v, int io) {
  if (io == 0) { ((float*)p)[idx] = v; return; }
  if (io == 1) { ((_Float16*)p)[idx] = (_Float16)v; return; }
  ((__bf16*)p)[idx] = (__bf16)v;      // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
}
template <bool X3>
__device__ __forceinline__ void put_split(_Float16* hi, _Float16* lo, int idx, float v) {
  const _Float16 h = (_Float16)v;
  hi[idx] = h;
  if (X3) lo[idx] = (_Float16)(v - (float)h);
}
// One gate's slice of W_hh as the forward's B operand, [k = h index][n = gate unit j], k = 32 ks + 8 g + jj: zero from column H
// on, so the ones column of the state tile meets zeros (b_hh enters through the accumulators).  The BPTT kernel that
// recomputes gh_n builds its n-gate fragments here too: the same values in the same registers of the fragment.
template <int KS>
__device__ __forceinline__ bool whh_gate_frags(const float* __restrict__ Whh, int H, int gate, int j, bool jv, int g,
                                               Frag (&W)[KS]) {
  bool bad = false;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float x[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int k = 32 * ks + 8 * g + jj;
      x[jj] = (jv && k < H) ? Whh[(size_t)(gate * H + j) * H + k] : 0.f;
      bad |= out_of_fp16_range(x[jj]);
    }
    W[ks] = split_vals(x);
  }
  return bad;
}
// acc[q] += [h | 1 | 0..] W[q] for NG gates over the state tile (hi plane, lo plane; rows of HS = 32 KS + 8 halfs): K steps in
// ascending order, per K step the three passes of mfma3, one accumulator per gate.  The forward runs it on all three gates,
// the BPTT kernel that recomputes gh_n on the n gate alone: per accumulator the same instructions in the same order.
template <int KS, bool X3, int NG>
__device__ __forceinline__ void hh_product(const _Float16* hhi, const _Float16* hlo, int c, int g, const Frag (*W)[KS],
                                           f32x4 (&acc)[NG]) {
  constexpr int HS = 32 * KS + 8;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    Frag a;
    a.hi = *(const h8*)(hhi + c * HS + 32 * ks + 8 * g);
    if (X3) a.lo = *(const h8*)(hlo + c * HS + 32 * ks + 8 * g);
    else a.lo = a.hi;
#pragma unroll
    for (int q = 0; q < NG; ++q) acc[q] = mfma3<X3>(a, W[q][ks], acc[q]);
  }
}

// ------------------------------------------------------------------------------------------------
// IO: Y and the labels are 16-bit on the wire (fp16 / bf16 by `io`) and move through LDS as whole rows; the fp32
// instance keeps the direct per-lane accesses (the row path was 30 % slower there: measured 116 vs 84 us).
// GI: the input projection [B*T][ldgi] in the 3H layout -- fp32 for the split (X3) instances, ONE fp16 plane for the one-pass
// fp16 instances (WGNN_MATH_F16: pgemm_nt's OUT16 epilogue; half the bytes of the largest intermediate of that mode)
// RC (the split modes' stateless fp32-I/O step, api.hip ghn_recompute): the record is r | z -- gh_n is not stored, the BPTT
// kernel recomputes it from the h_{t-1} it loads anyway
template <int KS, bool X3, bool IO, bool ST = false, bool RC = false>   // K steps of 32 over the hidden index (+ the ones column): KS = ceil((H+1)/32)
__global__ void __launch_bounds__(NTHREADS) grux_fwd_kernel(int B, int T, int H, const void* __restrict__ GI, int ldgi,
                                                            const float* __restrict__ Whh,
                                                            const float* __restrict__ bhh, void* __restrict__ Y,
                                                            float* __restrict__ gates, _Float16* __restrict__ yp_hi,
                                                            _Float16* __restrict__ yp_lo, unsigned* status,
                                                            const void* __restrict__ Lab,
                                                            float* __restrict__ stat_part, int io, int last_only,
                                                            float y_mul, float y_add, const float* __restrict__ h0,
                                                            float* __restrict__ hn) {
  // h0 (nullable, wgnn_fwd_state): [B][H] fp32 initial state instead of zeros, split into the planes like every h_t (a value
  // beyond fp16's range is reported as WGNN_STATUS_ACT_RANGE); hn (nullable): h_{T-1} [B][H] as fp32, never rounded to `io`.
  // ST: the wgnn_fwd_state instance; the plain forward's (ST = false) ignores h0 / hn and compiles exactly as before
  static_assert(!RC || (X3 && !IO && !ST), "gh_n is recomputed in the stateless fp32-I/O split step only");
  if (!ST) { h0 = nullptr; hn = nullptr; }
  // last_only (wgnn_fwd_last, inference): Y is [B][H] fp32 and receives only h_{T-1} * y_mul + y_add -- the evaluation
  // read-out of src/main.py:103,116 without writing (and re-reading) the other T-1 rows
  constexpr int HP = 32 * KS;                      // plane row width (halfs): h, then 1.0 at column H, then 0
  constexpr int HS = 32 * KS + 8;                  // row stride in halfs: 16-B aligned, conflict-free reads
  // h state is double-buffered: step t reads buffer t&1 and writes h_t into the other one, so a single
  // barrier per step suffices (the recurrence is latency-bound: every barrier is on the critical path)
  __shared__ __attribute__((aligned(16))) _Float16 hbuf[2 * 2 * MB * HS];
  bool h0bad = false;
  for (int i = threadIdx.x; i < 2 * 2 * MB * HS; i += NTHREADS) {
    const int m = (i % (MB * HS)) / HS, k = i % HS, b = blockIdx.x * MB + m;
    float v = 0.f;                                 // buffer 0 (i < 2 MB HS) holds h_{-1}: hi plane, then lo plane
    if (h0 && i < 2 * MB * HS && k < H && b < B) {
      const float x = h0[(size_t)b * H + k];
      h0bad |= out_of_fp16_range(x);
      v = i < MB * HS ? x : (X3 ? x - (float)(_Float16)x : 0.f);
    }
    hbuf[i] = (_Float16)v;
  }
  report_status(status, h0bad, WGNN_STATUS_ACT_RANGE);
  __syncthreads();
  if (threadIdx.x < 2 * MB)   // ones column of both buffers' hi planes (W_hh fragments are 0 there)
    hbuf[(threadIdx.x / MB) * 2 * MB * HS + (threadIdx.x % MB) * HS + H] = (_Float16)1.f;

  // tag behind the MSE partial pairs: set by wgnn_fwd_loss, cleared by a plain wgnn_fwd on the same stash, checked by the
  // BPTT kernel when the caller claims (part bit 8) that the statistics of THESE labels are in the stash
  if (stat_part && blockIdx.x == 0 && threadIdx.x == 0) stat_part[2 * gridDim.x] = Lab ? WGNN_STATS_TAG : 0.f;
  if (yp_hi && blockIdx.x == 0 && threadIdx.x < HP) {   // row B*T: what [Hprev | 1] looks like at t = 0
    yp_hi[(size_t)B * T * HP + threadIdx.x] = (_Float16)(threadIdx.x == H ? 1.f : 0.f);
    yp_lo[(size_t)B * T * HP + threadIdx.x] = (_Float16)0.f;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int j = 16 * wave + c;
  const bool active = 16 * wave < H;               // wave-uniform
  const bool jv = j < H;
  const int jc = jv ? j : H - 1;
  const int b0 = blockIdx.x * MB;

  bool wbad = false;
  Frag WB[3][KS];                                  // B operand: W_hh[(gate*H + j)][k], k = 32ks + 8g + jj
#pragma unroll
  for (int gate = 0; gate < 3; ++gate) wbad |= whh_gate_frags<KS>(Whh, H, gate, j, jv, g, WB[gate]);
  if (blockIdx.x == 0) report_status(status, wbad, WGNN_STATUS_WEIGHT_RANGE);
  const float bh_r = bhh[jc], bh_z = bhh[H + jc], bh_n = bhh[2 * H + jc];

  // Addressing: one workgroup-uniform 64-bit base per array (the workgroup's first window) plus 32-bit lane
  // offsets.  Row indices are clamped so every load is unconditional.
  typedef typename std::conditional<X3, float, _Float16>::type gi_t;
  const gi_t* GIw = (const gi_t*)GI + (size_t)b0 * T * ldgi;
  constexpr int esz = IO ? 2 : 4;                  // bytes per element of Y and the labels (wgnn_io)
  void* Yw = (char*)Y + (size_t)b0 * T * H * esz;
  // gate stash in this kernel's own register layout, [workgroup][t][wave][r | z | n | gh_n][lane] x float4 (the 4 window
  // rows a lane owns): one 16-byte store per lane and component (a full 1 KB per wave-instruction) instead of sixteen
  // 4-byte stores in 64-byte segments; the BPTT kernel (same thread <-> (rows, unit) map) reads it back the same way.
  // All four stay fp32: packing r and z as unorm16 (12 bytes per record: forward -4 us, BPTT -11 us) was tried and is
  // WRONG for trained weights -- saturated gates need r (1 - r) to fp32's own precision (8 % gradient error on the
  // wind_gnn_7.pth fixture).
  const int NW = (H + 15) / 16;
  // One-pass fp16 mode (X3 = false; tolerance class 5e-2): the record is fp16 -- [r | z] and [n | gh_n] as two 8-half
  // (16-byte) components -- half the stash bytes of the two recurrences, which are bound by exactly those bytes at the bench
  // size.  (Evaluated on the fp64 oracle in round 3: gradient errors 0.9-2.8e-4 of max, independent of B: outside the 1e-4
  // bar of the split modes, far inside this mode's.)  The h_t component of 16-bit I/O stays fp32.
  // Split modes (round 4): THREE fp32 components, r | z | gh_n -- n is not stored: the BPTT kernel recomputes it as
  // tanh(gi_n + r gh_n) from the n third of GI, which the forward keeps in the stash (the projection GEMM writes GI there
  // instead of into the workspace: no extra traffic); 44 MB less stash per step at B = 4096 for 42 MB of GI read back.
  // RC: TWO, r | z, packed at the start of the same region -- gh_n depends on nothing but h_{t-1}, which the BPTT kernel loads
  // from Y anyway and multiplies by the n rows of W_hh itself (another 44 MB less written here and 44 MB less read there).
  constexpr int GREC = X3 ? (IO ? 4 : (RC ? 2 : 3)) : (IO ? 3 : 2);       // 16-byte components per lane and (t, wave)
  f32x4* gatesw = gates ? (f32x4*)gates + ((size_t)blockIdx.x * T * NW + wave) * GREC * 64 + lane : nullptr;
  int rowt[4];            // (local window row) * T, clamped to the last valid window
  bool rowok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;
    rowok[r] = jv && b0 + m < B;
    rowt[r] = (b0 + m < B ? m : B - 1 - b0) * T;
  }
  // ---- Y out and labels in go through LDS as whole rows: a row (b, t) of Y or of the labels is H contiguous elements,
  // moved as "units" of 2 elements (8 bytes fp32, 4 bytes fp16 / bf16) by consecutive threads, instead of each owner
  // lane storing / loading single elements in 64-byte (32-byte at 16 bits) segments.  ytile / ltile are double-buffered
  // by step parity like hbuf.  Unit q = threadIdx.x + 512 i of the workgroup's 16 rows: fixed for the whole launch.
  constexpr int HY = HP + 2;                       // fp32 row stride of the tiles (even: 8-byte aligned pairs)
  __shared__ __attribute__((aligned(16))) float ytile[IO ? 2 * MB * HY : 4];
  __shared__ __attribute__((aligned(16))) float ltile[IO ? 2 * MB * HY : 4];
  const int UPR = (H + 1) / 2;                     // units per row
  constexpr int NU = (MB * (HP / 2) + NTHREADS - 1) / NTHREADS;
  int u_lds[NU], u_glb[NU], u_n[NU];               // tile offset (m * HY + e), row-relative global element offset, elements (0, 1, 2)
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int q = threadIdx.x + NTHREADS * i;
    const int m = q / UPR, e = 2 * (q % UPR);
    const bool ok = q < MB * UPR && b0 + m < B;
    u_lds[i] = ok ? m * HY + e : 0;
    u_glb[i] = ok ? m * T * H + e : 0;
    u_n[i] = ok ? (e + 1 < H ? 2 : 1) : 0;
  }
  // wgnn_fwd_loss: the MSE statistics (sum of squares, max |Y - L|) are taken here, from the h this kernel
  // holds in registers, so no later pass re-reads Y and the labels for them
  const void* Labw = Lab ? (const char*)Lab + (size_t)b0 * T * H * esz : nullptr;
  f32x2 lraw[NU];                                  // the next step's label units, in flight (raw bits when 16-bit)
  auto load_lab = [&](int t) {
    if (!IO || !Lab) return;
    const int tc = t < T ? t : T - 1;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int o = u_glb[i] + tc * H;
      if (io == 0) {
        if (u_n[i] == 2) lraw[i] = *(const f32x2*)((const float*)Labw + o);
        else if (u_n[i] == 1) lraw[i][0] = ((const float*)Labw)[o];
      } else {
        if (u_n[i] == 2) lraw[i][0] = __builtin_bit_cast(float, *(const unsigned*)((const unsigned short*)Labw + o));
        else if (u_n[i] == 1) lraw[i][0] = __builtin_bit_cast(float, (unsigned)((const unsigned short*)Labw)[o]);
      }
    }
  };
  auto stage_lab = [&](int t) {                    // labels of step t -> ltile[t & 1] as fp32
    if (!IO || !Lab) return;
    float* lt = ltile + (t & 1) * MB * HY;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if (u_n[i] == 0) continue;
      f32x2 v = lraw[i];
      if (io == 1) {
        v = __builtin_convertvector(__builtin_bit_cast(h2v, __builtin_bit_cast(unsigned, lraw[i][0])), f32x2);
      } else if (io == 2) {
        const unsigned u = __builtin_bit_cast(unsigned, lraw[i][0]);
        v[0] = __builtin_bit_cast(float, u << 16);
        v[1] = __builtin_bit_cast(float, u & 0xffff0000u);
      }
      lt[u_lds[i]] = v[0];
      if (u_n[i] == 2) lt[u_lds[i] + 1] = v[1];
    }
  };
  float ssum = 0.f, smax = 0.f;
  float lab[4] = {0.f, 0.f, 0.f, 0.f}, labn[4] = {0.f, 0.f, 0.f, 0.f};   // fp32 I/O: the owner lanes load their labels
  float gi[3][4], gin[3][4];
  auto load_gi = [&](int t, float (&dst)[3][4], float (&ldst)[4]) {
    const int tc = t < T ? t : T - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = (rowt[r] + tc) * ldgi + jc;
      dst[0][r] = (float)GIw[o];
      dst[1][r] = (float)GIw[o + H];
      dst[2][r] = (float)GIw[o + 2 * H];
      if (!IO && Lab) ldst[r] = ((const float*)Labw)[(rowt[r] + tc) * H + jc];
    }
  };
  load_lab(0);
  stage_lab(0);
  load_gi(0, gi, lab);
  float hold[4] = {0.f, 0.f, 0.f, 0.f};
  if (h0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) hold[r] = rowok[r] ? h0[(size_t)(b0 + 4 * g + r) * H + j] : 0.f;
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const _Float16* hhi = hbuf + (t & 1) * 2 * MB * HS;          // h_{t-1}
    const _Float16* hlo = hhi + MB * HS;
    _Float16* nhi = hbuf + ((t + 1) & 1) * 2 * MB * HS;          // h_t goes here
    _Float16* nlo = nhi + MB * HS;
    load_gi(t + 1, gin, labn);                     // prefetch under this step's MFMAs
    load_lab(t + 1);
    float* yt = ytile + (t & 1) * MB * HY;
    const float* lt = ltile + (t & 1) * MB * HY;
    float hnew[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      f32x4 acc[3];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[0][r] = gi[0][r] + bh_r;
        acc[1][r] = gi[1][r] + bh_z;
        acc[2][r] = bh_n;
      }
      hh_product<KS, X3, 3>(hhi, hlo, c, g, WB, acc);
      const f32x4 ar = acc[0], az = acc[1], an = acc[2];
      f32x4 rg4, zg4, ng4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {                      // the four rows' gate chains in ONE basic block (they interleave);
        const float rg = sigmoid_fast(ar[r]);            // everything conditional comes in the loop below
        const float zg = sigmoid_fast(az[r]);
        const float ng = tanh_fast(__builtin_fmaf(rg, an[r], gi[2][r]));   // the BPTT kernel recomputes exactly this
        rg4[r] = rg; zg4[r] = zg; ng4[r] = ng;
        hnew[r] = (1.f - zg) * ng + zg * hold[r];
        hold[r] = hnew[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (IO) {
          if (jv) yt[(4 * g + r) * HY + j] = hnew[r];   // -> Y through the row copy-out below
        } else if (rowok[r]) {
          if (!last_only) ((float*)Yw)[(rowt[r] + t) * H + j] = hnew[r];
          else if (t == T - 1) ((float*)Y)[(size_t)(b0 + 4 * g + r) * H + j] = hnew[r] * y_mul + y_add;
        }
        if (hn && rowok[r] && t == T - 1) hn[(size_t)(b0 + 4 * g + r) * H + j] = hnew[r];
        if (rowok[r] && Lab) {                          // the statistics use the unrounded h
          const float dl = hnew[r] - (IO ? lt[(4 * g + r) * HY + j] : lab[r]);
          ssum = fmaf(dl, dl, ssum);
          smax = fmaxf(smax, fabsf(dl));
        }
      }
      if (gates) {
        f32x4* rec = gatesw + (size_t)t * NW * GREC * 64;
        if (X3) {
          rec[0] = rg4;
          rec[64] = zg4;
          if (!RC) rec[128] = an;
        } else {
          h8 rz, ng;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            rz[r] = (_Float16)rg4[r];
            rz[4 + r] = (_Float16)zg4[r];
            ng[r] = (_Float16)ng4[r];
            ng[4 + r] = (_Float16)an[r];
          }
          rec[0] = __builtin_bit_cast(f32x4, rz);
          rec[64] = __builtin_bit_cast(f32x4, ng);
        }
        if (IO) {
          const f32x4 h4 = {hnew[0], hnew[1], hnew[2], hnew[3]};
          rec[(GREC - 1) * 64] = h4;
        }
      }
    }
    if (active) {                                    // lanes past H aim at the row's pad halfs (never read as K, never copied out)
#pragma unroll
      for (int r = 0; r < 4; ++r) put_split<X3>(nhi, nlo, (4 * g + r) * HS + (jv ? j : HP + (c & 7)), hnew[r]);
    }
    stage_lab(t + 1);                              // other parity than the labels read above
    __syncthreads();                               // h_t complete; everyone is done reading h_{t-1}
#pragma unroll
    for (int i = 0; i < (IO ? NU : 0); ++i) {      // row (b, t) of Y, 2 elements per thread, rounded once to the I/O type
      if (ST && !Y) break;                         // (wgnn_fwd_state with Y = NULL: h_n only)
      if (u_n[i] == 0) continue;
      const float v0 = yt[u_lds[i]], v1 = yt[u_lds[i] + 1];
      const int o = u_glb[i] + t * H;
      if (io == 0) {
        if (u_n[i] == 2) { const f32x2 v = {v0, v1}; *(f32x2*)((float*)Yw + o) = v; }
        else ((float*)Yw)[o] = v0;
      } else {
        unsigned pk;
        if (io == 1) {
          const f32x2 v = {v0, v1};
          pk = __builtin_bit_cast(unsigned, __builtin_convertvector(v, h2v));
        } else {
          typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
          const f32x2 v = {v0, v1};
          pk = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf2));
        }
        if (u_n[i] == 2) *(unsigned*)((unsigned short*)Yw + o) = pk;
        else ((unsigned short*)Yw)[o] = (unsigned short)pk;
      }
    }
    if (yp_hi) {   // h_t as fp16 planes (the B operand of the dW_hh GEMM): 16-byte chunks straight from LDS
      for (int q = threadIdx.x; q < (X3 ? 2 : 1) * MB * (HP / 8); q += NTHREADS) {
        const int plane = q / (MB * (HP / 8)), rem = q % (MB * (HP / 8));
        const int m = rem / (HP / 8), ch = rem % (HP / 8);
        const int b = b0 + m;
        if (b < B) {
          const h8 v = *(const h8*)((plane ? nlo : nhi) + m * HS + 8 * ch);
          // non-temporal: the planes are next read by the dW_hh GEMM, four kernels later; kept out of the Infinity Cache they
          // leave it to the gate stash and Y, which the BPTT kernel reads back right after this one
          __builtin_nontemporal_store(v, (h8*)((plane ? yp_lo : yp_hi) + (size_t)b0 * T * HP + (m * T + t) * HP + 8 * ch));
        }
      }
    }
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
      float a = 0.f, m = 0.f;
#pragma unroll
      for (int w = 0; w < NTHREADS / 64; ++w) {
        a += red[0][w];
        m = fmaxf(m, red[1][w]);
      }
      stat_part[blockIdx.x] = a;
      stat_part[gridDim.x + blockIdx.x] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// BPTT; per step (t descending), dh = s*dY_t + dh_next (everything in units scaled by s = scales[0]):
//   dn = dh (1-z), dz = dh (hprev - n), dnt = dn (1-n^2), dr = dnt gh_n,
//   dar = dr r (1-r), daz = dz z (1-z);  dgi = [dar, daz, dnt], dgh = [dar, daz, dnt r]
//   dh_next = dh z + dgh W_hh
// Outputs for the weight-gradient GEMMs: dGI planes [B*T][ldd] in the 3H layout, and of dGH ONLY its n third,
// dGHn = dnt*r, planes [B*T][HN] (dGH's r and z thirds equal dGI's: the dW_hh GEMM takes them from the dGI planes).
// In LDS the dgh row is laid out [dar | daz | pad to MS = 8*ceil(2H/8) | dnr] so that the dnr block is 16-byte aligned
// for the copy-out; the W_hh^T fragments' k index follows the same layout.
// St (empty, or one BwdState: wgnn_bwd_state_part): h_{-1} = h0, the carry starts at s dh_n, and the step at t = 0 also
// forms dh_{-1} = dh z + dgh W_hh, written (times scales[1]) to dh0.
// KSF > 0 (the forward's RC instances wrote r | z records; KSF is the forward's KS = ceil((H + 1) / 32)): gh_n of step t - 1 is
// recomputed during step t, as b_hn + [h_{t-2} | 1 | 0..] W_hn by the forward's own hh_product on the forward's own
// fragments, from a state tile split exactly as the forward's -- Y[b, t-2] IS the fp32 h the forward split, so the product is
// the forward's bit for bit.  h_{t-2} is prefetched two steps ahead, its tile is written before the step's first barrier and
// read behind it, beside the dgh W_hh product: nothing of it sits on the chain from dh_next to the next step.
template <int KSB, bool X3, bool IO, int KSF, typename... St>   // K steps of 32 over the padded dgh row: KSB = ceil((MS + H) / 32); IO: as grux_fwd_kernel
__global__ void __launch_bounds__(NTHREADS) grux_bwd_kernel(int B, int T, int H, const float* __restrict__ Whh,
                                                            const void* __restrict__ Y, const float* __restrict__ dY,
                                                            const void* __restrict__ Lab, int io,
                                                            const float* __restrict__ gates,
                                                            const float* __restrict__ GIn, int ldgi,
                                                            const float* __restrict__ scales,
                                                            _Float16* __restrict__ dGI_hi, _Float16* __restrict__ dGI_lo,
                                                            int ldd, _Float16* __restrict__ dGN_hi,
                                                            _Float16* __restrict__ dGN_lo,
                                                            const float* __restrict__ stat_part, int nstat, float inv_n,
                                                            float coef_in, float* __restrict__ loss_out,
                                                            float* __restrict__ scales_out, unsigned* status,
                                                            int write_lo, const float* __restrict__ bhh, St... state) {
  constexpr bool ST = sizeof...(St) > 0;
  constexpr bool RC = KSF > 0;
  static_assert(!RC || (X3 && !IO && !ST), "gh_n is recomputed in the stateless fp32-I/O split step only");
  const BwdState sb = bwd_state(state...);
  // write_lo == 0 (X3, large B*T): dGI / dGHn leave the chip as ONE fp16 plane (the lo halves stay in LDS, where the
  // recurrence's own product dgh W_hh uses them): the three GEMMs that consume them run two passes
  constexpr int DS = 32 * KSB + 24;   // row stride in halfs: odd in 16-byte units (conflict-free b128 rows); 8 zero pad halfs, then 8 dump halfs
  // stat_part != null (wgnn_bwd_mse_part(.. | 8) after wgnn_fwd_loss): the loss, the power-of-two range scale and the dY
  // coefficient are finalised HERE from the forward recurrence's nstat partial pairs (sum | max), by every workgroup for
  // itself (2 nstat floats out of L2; the max is order-independent, so all workgroups agree on the scale), instead of in a
  // launch of their own; workgroup 0 publishes loss and scales for the kernels that follow.
  float s_fin = 1.f, c_fin = coef_in;
  if (stat_part) {
    __shared__ float sred[2][NTHREADS / 64];
    float a = 0.f, m = 0.f;
    for (int i = threadIdx.x; i < nstat; i += NTHREADS) {
      a += stat_part[i];
      m = fmaxf(m, stat_part[nstat + i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      m = fmaxf(m, __shfl_xor(m, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      sred[0][threadIdx.x >> 6] = a;
      sred[1][threadIdx.x >> 6] = m;
    }
    __syncthreads();
    a = 0.f;
    m = 0.f;
#pragma unroll
    for (int w = 0; w < NTHREADS / 64; ++w) {
      a += sred[0][w];
      m = fmaxf(m, sred[1][w]);
    }
    const bool tagged = stat_part[2 * nstat] == WGNN_STATS_TAG;
    m *= fabsf(coef_in);
    if (m > 0.f && m < 3.0e38f) {
      int e;
      frexpf(m, &e);
      s_fin = ldexpf(1.f, 1 - e);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      loss_out[0] = tagged ? a * inv_n : __builtin_nanf("");     // no statistics of these labels in the stash: loud, not stale
      scales_out[0] = s_fin;
      scales_out[1] = 1.f / s_fin;
      scales_out[2] = coef_in;
      if (!tagged && status) atomicOr(status, WGNN_STATUS_NO_LOSS_STATS);
    }
  }
  // per step parity: dgh hi | dgh lo (padded layout, also the MFMA A operand) | dgi hi | dgi lo (3H layout); columns
  // never written (K padding, the tail of the dnr block) stay zero.  Double-buffered by step parity (kept with
  // the second barrier below: dropping that barrier was slower)
  __shared__ __attribute__((aligned(16))) _Float16 dbuf2[2 * 4 * MB * DS];
  for (int i = threadIdx.x; i < 2 * 4 * MB * DS; i += NTHREADS) dbuf2[i] = (_Float16)0.f;
  // RC: the forward's state tile [h | 1 | 0..], hi plane then lo plane, rows of HSF halfs; the tile of step s is htile2[s & 1]
  constexpr int HPF = 32 * KSF, HSF = 32 * KSF + 8;
  __shared__ __attribute__((aligned(16))) _Float16 htile2[RC ? 2 * 2 * MB * HSF : 8];
  if (RC) {
    for (int i = threadIdx.x; i < 2 * 2 * MB * HSF; i += NTHREADS)   // zeros, and the ones column of both hi planes
      htile2[i] = (_Float16)((i % (2 * MB * HSF) < MB * HSF && i % HSF == H) ? 1.f : 0.f);
    __syncthreads();                                                 // (the owner lanes write h_{T-2} below)
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int j = 16 * wave + c;
  const bool active = 16 * wave < H;
  const bool jv = j < H;
  const int jc = jv ? j : H - 1;
  const int b0 = blockIdx.x * MB;
  const int MS = 8 * ((2 * H + 7) / 8), HN = 8 * ((H + 7) / 8);
  const float s_in = stat_part ? s_fin : (scales ? scales[0] : 1.f);
  // fused MSE (wgnn_bwd_mse_part): dY is not materialised, dY[b,t] = (Y[b,t] - L[b,t]) * scales[2] is formed here;
  // Y[b,t] is the h_prev this kernel loaded for step t+1, so only L is read in dY's place.
  const float coef = stat_part ? c_fin : (Lab ? scales[2] : 1.f);

  Frag WT[KSB];                                    // B operand: W_hh[row(k)][j], k = 32ks + 8g + jj in the padded layout
#pragma unroll
  for (int ks = 0; ks < KSB; ++ks) {
    float x[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int k = 32 * ks + 8 * g + jj;
      const int row = k < 2 * H ? k : ((k >= MS && k - MS < H) ? 2 * H + (k - MS) : -1);
      x[jj] = (jv && row >= 0) ? Whh[(size_t)row * H + j] : 0.f;
    }
    WT[ks] = split_vals(x);
  }
  Frag WN[1][RC ? KSF : 1];                        // RC: the forward's n-gate B operand (32 registers at H = 102) and b_hn
  float bh_n = 0.f;
  if constexpr (RC) {
    whh_gate_frags<KSF>(Whh, H, 2, j, jv, g, WN[0]);
    bh_n = bhh[2 * H + jc];
  }
  constexpr int GREC = X3 ? (IO ? 4 : (RC ? 2 : 3)) : (IO ? 3 : 2);       // as grux_fwd_kernel: r | z (| gh_n) (+ h), or fp16 records
  const int NW = (H + 15) / 16;                              // gate stash: grux_fwd_kernel's register layout
  const f32x4* gatesw = (const f32x4*)gates + ((size_t)blockIdx.x * T * NW + (active ? wave : 0)) * GREC * 64 + lane;
  // 16-bit I/O: Y on the wire is rounded, so h_{t-1} (and the Y of the fused dY) is the 5th component of the stash
  // records; explicit dY is always fp32; labels are io-typed and come in through LDS as whole rows (see grux_fwd_kernel)
  constexpr int esz = IO ? 2 : 4;
  const float* GIw = X3 ? GIn + (size_t)b0 * T * ldgi + 2 * H : nullptr;   // n third of this workgroup's GI rows (stash)
  const void* Labw = Lab ? (const char*)Lab + (size_t)b0 * T * H * esz : nullptr;
  const float* dYw = dY ? dY + (size_t)b0 * T * H : nullptr;
  const float* Yw = (const float*)Y + (size_t)b0 * T * H;
  int rowt[4];
  bool rowok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;
    rowok[r] = jv && b0 + m < B;
    rowt[r] = (b0 + m < B ? m : B - 1 - b0) * T;
  }
  // ---- copy-out plan, fixed for the whole launch: per step the workgroup moves, as 16-byte chunks,
  // 2 planes x 16 rows x ldd/8 chunks of the dgi tile and 2 planes x 16 rows x HN/8 chunks of the dnr block.
  // Chunk q = threadIdx.x + 512 i: its LDS offset, destination and row stride never change (only t does).
  constexpr int NCH = (2 * MB * (4 * KSB) + 2 * MB * (4 * KSB) / 2 + NTHREADS - 1) / NTHREADS;   // upper bound
  int c_lds[NCH], c_step[NCH];
  _Float16* c_dst[NCH];
  {
    const int cpr = ldd / 8, cpn = HN / 8;
    const int n_i = 2 * MB * cpr, n_n = 2 * MB * cpn;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int q = threadIdx.x + NTHREADS * i;
      c_dst[i] = nullptr;
      c_lds[i] = 0;
      c_step[i] = 0;
      if (q < n_i) {
        const int plane = q / (MB * cpr), rem = q % (MB * cpr), m = rem / cpr, ch = rem % cpr;
        if (b0 + m < B && ((X3 && write_lo) || plane == 0)) {
          c_lds[i] = (2 + plane) * MB * DS + m * DS + 8 * ch;
          c_dst[i] = (plane ? dGI_lo : dGI_hi) + ((size_t)(b0 + m) * T) * ldd + 8 * ch;
          c_step[i] = ldd;
        }
      } else if (q - n_i < n_n) {
        q -= n_i;
        const int plane = q / (MB * cpn), rem = q % (MB * cpn), m = rem / cpn, ch = rem % cpn;
        if (b0 + m < B && ((X3 && write_lo) || plane == 0)) {
          c_lds[i] = plane * MB * DS + m * DS + MS + 8 * ch;
          c_dst[i] = (plane ? dGN_lo : dGN_hi) + ((size_t)(b0 + m) * T) * HN + 8 * ch;
          c_step[i] = HN;
        }
      }
    }
  }
  constexpr int HY = 32 * ((KSB * 32 / 3 + 31) / 32) + 34;     // >= H + 2 (H <= (32 KSB) / 3 + a few), even
  __shared__ __attribute__((aligned(16))) float ltile[IO ? 2 * MB * HY : 4];
  const int UPR = (H + 1) / 2;
  constexpr int NU = IO ? (MB * (HY / 2) + NTHREADS - 1) / NTHREADS : 1;
  int u_lds[NU], u_glb[NU], u_n[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int q = threadIdx.x + NTHREADS * i;
    const int m = q / UPR, e = 2 * (q % UPR);
    const bool ok = IO && Lab && q < MB * UPR && b0 + m < B;
    u_lds[i] = ok ? m * HY + e : 0;
    u_glb[i] = ok ? m * T * H + e : 0;
    u_n[i] = ok ? (e + 1 < H ? 2 : 1) : 0;
  }
  f32x2 lraw[NU];
  auto load_lab = [&](int t) {
    const int tc = t > 0 ? t : 0;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int o = u_glb[i] + tc * H;
      if (io == 0) {
        if (u_n[i] == 2) lraw[i] = *(const f32x2*)((const float*)Labw + o);
        else if (u_n[i] == 1) lraw[i][0] = ((const float*)Labw)[o];
      } else {
        if (u_n[i] == 2) lraw[i][0] = __builtin_bit_cast(float, *(const unsigned*)((const unsigned short*)Labw + o));
        else if (u_n[i] == 1) lraw[i][0] = __builtin_bit_cast(float, (unsigned)((const unsigned short*)Labw)[o]);
      }
    }
  };
  auto stage_lab = [&](int t) {                    // labels of step t -> ltile[t & 1] as fp32
    float* lt = ltile + (t & 1) * MB * HY;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if (u_n[i] == 0) continue;
      f32x2 v = lraw[i];
      if (io == 1) {
        v = __builtin_convertvector(__builtin_bit_cast(h2v, __builtin_bit_cast(unsigned, lraw[i][0])), f32x2);
      } else if (io == 2) {
        const unsigned u = __builtin_bit_cast(unsigned, lraw[i][0]);
        v[0] = __builtin_bit_cast(float, u << 16);
        v[1] = __builtin_bit_cast(float, u & 0xffff0000u);
      }
      lt[u_lds[i]] = v[0];
      if (u_n[i] == 2) lt[u_lds[i] + 1] = v[1];
    }
  };
  // the state's boundary values in registers before the loop: a load under `tc == 0` inside load_step would make the
  // compiler wait for all of the step's prefetches at the join
  float h0r[4] = {0.f, 0.f, 0.f, 0.f};
  float s_out = 1.f;
  if constexpr (ST) {
#pragma unroll
    for (int r = 0; r < 4; ++r) h0r[r] = sb.h0[(size_t)(b0 + rowt[r] / T) * H + jc];
    s_out = scales ? scales[1] : 1.f;
  }
  struct StepIn { float dy[4], r[4], z[4], n[4], ghn[4], hp[4]; };
  auto load_step = [&](int t, StepIn& s) {
    const int tc = t > 0 ? t : 0;
    const f32x4* rec = gatesw + (size_t)tc * NW * GREC * 64;
    f32x4 r4, z4, n4, g4 = {0.f, 0.f, 0.f, 0.f};
    if (X3) {
      r4 = rec[0]; z4 = rec[64];
      if (!RC) g4 = rec[128];                            // (RC: gh_n comes out of the step before, see the loop)
#pragma unroll
      for (int r = 0; r < 4; ++r) n4[r] = GIw[(rowt[r] + tc) * ldgi + jc];      // gi_n: n itself is formed in the step
    } else {
      const h8 rz = __builtin_bit_cast(h8, rec[0]), ng = __builtin_bit_cast(h8, rec[64]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        r4[r] = (float)rz[r];
        z4[r] = (float)rz[4 + r];
        n4[r] = (float)ng[r];
        g4[r] = (float)ng[4 + r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int bt = rowt[r] + tc;
      // 16-bit labels are read from ltile at the top of their step; fp32 labels / dY by the owner lane
      s.dy[r] = Lab ? (IO ? 0.f : ((const float*)Labw)[bt * H + jc]) : dYw[bt * H + jc];
      s.r[r] = r4[r];
      s.z[r] = z4[r];
      s.n[r] = n4[r];
      s.ghn[r] = g4[r];
      const float hp = (IO || RC) ? 0.f : Yw[(bt - (tc > 0 ? 1 : 0)) * H + jc];   // (RC: load_hprev, a step earlier)
      s.hp[r] = tc > 0 ? hp : 0.f;
      if constexpr (ST) {   // (a discarded branch: the plain instance's lambda does not even capture sb)
        if (tc == 0) s.hp[r] = h0r[r];
      }
    }
    if (IO && tc > 0) {                                  // h_{t-1} = 5th component of step t-1's record
      const f32x4 h4 = (gatesw + (size_t)(tc - 1) * NW * GREC * 64)[(GREC - 1) * 64];
#pragma unroll
      for (int r = 0; r < 4; ++r) s.hp[r] = h4[r];
    }
  };
  // RC: h_{s-1}, the hp of step s, on its own -- the loop asks for it two steps ahead, so that its tile can be written
  // before the first barrier of the step that recomputes gh_n of step s, from a load issued a whole step earlier
  auto load_hprev = [&](int s, float (&hp)[4]) {
    const int sc = s > 0 ? s : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = Yw[(rowt[r] + sc - (sc > 0 ? 1 : 0)) * H + jc];
      hp[r] = sc > 0 ? v : 0.f;
    }
  };
  // the owner lanes' part of the tile of step s: the forward's put_split, columns past H into the row's pad halfs
  auto put_hprev = [&](int s, const float (&hp)[4]) {
    _Float16* thi = htile2 + (s & 1) * 2 * MB * HSF;
#pragma unroll
    for (int r = 0; r < 4; ++r) put_split<true>(thi, thi + MB * HSF, (4 * g + r) * HSF + (jv ? j : HPF + (c & 7)), hp[r]);
  };
  auto ghn_of = [&](int s, float (&ghn)[4]) {            // gh_n of step s from its tile: the forward's product, n gate alone
    const _Float16* thi = htile2 + (s & 1) * 2 * MB * HSF;
    f32x4 a[1] = {{bh_n, bh_n, bh_n, bh_n}};
    hh_product<RC ? KSF : 1, true, 1>(thi, thi + MB * HSF, c, g, WN, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) ghn[r] = a[0][r];
  };
  StepIn cur, nxt;
  load_step(T - 1, cur);
  float hq[4] = {0.f, 0.f, 0.f, 0.f};                    // RC: the hp of the step after next
  if (RC) {
    load_hprev(T - 1, cur.hp);
    load_hprev(T - 2, hq);
    if (active) put_hprev(T - 1, cur.hp);                // read behind the barrier in front of the loop
  }
  float ycur[4] = {0.f, 0.f, 0.f, 0.f};
  if (Lab) {
    if (IO) {
      const f32x4 h4 = (gatesw + (size_t)(T - 1) * NW * GREC * 64)[(GREC - 1) * 64];
#pragma unroll
      for (int r = 0; r < 4; ++r) ycur[r] = h4[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) ycur[r] = Yw[(rowt[r] + T - 1) * H + jc];
    }
    if (IO) {
      load_lab(T - 1);
      stage_lab(T - 1);
    }
  }
  f32x4 dhn = {0.f, 0.f, 0.f, 0.f};
  if (ST && sb.dhn) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dhn[r] = rowok[r] ? sb.dhn[(size_t)(b0 + 4 * g + r) * H + j] * s_in : 0.f;
  }
  // columns of this lane's unit in the dgh row (r | z | pad | n r) and the dgi row (r | z | n); lanes past H: the dump halfs
  const int o_pad = 32 * KSB + 8 + (c & 7);
  const int o_r = jv ? j : o_pad, o_z = jv ? H + j : o_pad, o_n = jv ? MS + j : o_pad, o_t = jv ? 2 * H + j : o_pad;
  __syncthreads();
  if (RC && active) ghn_of(T - 1, cur.ghn);

  for (int t = T - 1; t >= 0; --t) {
    _Float16* dbuf = dbuf2 + (t & 1) * 4 * MB * DS;
    _Float16* dhi = dbuf;
    _Float16* dlo = dbuf + MB * DS;
    _Float16* ihi = dbuf + 2 * MB * DS;
    _Float16* ilo = dbuf + 3 * MB * DS;
    load_step(t - 1, nxt);
    if (RC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) nxt.hp[r] = hq[r];     // loaded during step t + 1
      load_hprev(t - 2, hq);
    }
    if (IO && Lab) load_lab(t - 1);
    const float* lt = ltile + (t & 1) * MB * HY;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * g + r;
        const float dyv = Lab ? (ycur[r] - (IO ? lt[m * HY + jc] : cur.dy[r])) * coef : cur.dy[r];
        const float dh = rowok[r] ? dyv * s_in + dhn[r] : 0.f;
        const float rg = cur.r[r], zg = cur.z[r];
        const float ng = X3 ? tanh_fast(__builtin_fmaf(rg, cur.ghn[r], cur.n[r])) : cur.n[r];   // the forward's n, bit for bit
        const float dn = dh * (1.f - zg);
        const float dz = dh * (cur.hp[r] - ng);
        const float dnt = dn * (1.f - ng * ng);
        const float dr = dnt * cur.ghn[r];
        const float dar = dr * rg * (1.f - rg);
        const float daz = dz * zg * (1.f - zg);
        const float dnr = dnt * rg;
        acc[r] = dh * zg;
        // No branch on jv and no read-back: lanes past H aim at the row's 8 dump halfs (never read as K, never copied out),
        // so the four rows' chains sit in one basic block, and dar / daz go to both tiles from registers (the former
        // `ihi[..] = dhi[..]` copies were 16 serialized LDS round trips per step): 101.2 -> 97.5 us (r4, same box)
        const _Float16 arh = (_Float16)dar, azh = (_Float16)daz, nrh = (_Float16)dnr, nth = (_Float16)dnt;
        dhi[m * DS + o_r] = arh;
        dhi[m * DS + o_z] = azh;
        dhi[m * DS + o_n] = nrh;
        ihi[m * DS + o_r] = arh;
        ihi[m * DS + o_z] = azh;
        ihi[m * DS + o_t] = nth;
        if (X3) {
          const _Float16 arl = (_Float16)(dar - (float)arh), azl = (_Float16)(daz - (float)azh);
          dlo[m * DS + o_r] = arl;
          dlo[m * DS + o_z] = azl;
          dlo[m * DS + o_n] = (_Float16)(dnr - (float)nrh);
          ilo[m * DS + o_r] = arl;
          ilo[m * DS + o_z] = azl;
          ilo[m * DS + o_t] = (_Float16)(dnt - (float)nth);
        }
      }
      if (RC && t > 0) put_hprev(t - 1, nxt.hp);         // the other parity than the tile this step's gh_n came from
    }
    if (IO && Lab) stage_lab(t - 1);   // other parity than the labels read above; visible after the barrier
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i) {   // planes out: rows (b, t) of dGI and of dGHn
      if (c_dst[i]) {
        const h8 v = *(const h8*)(dbuf + c_lds[i]);
        *(h8*)(c_dst[i] + (size_t)t * c_step[i]) = v;
      }
    }
    if (active && (ST || t > 0)) {
#pragma unroll
      for (int ks = 0; ks < KSB; ++ks) {
        Frag a;
        a.hi = *(const h8*)(dhi + c * DS + 32 * ks + 8 * g);
        if (X3) a.lo = *(const h8*)(dlo + c * DS + 32 * ks + 8 * g);
        else a.lo = a.hi;
        acc = mfma3<X3>(a, WT[ks], acc);
      }
      if (ST && t == 0 && sb.dh0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (rowok[r]) sb.dh0[(size_t)(b0 + 4 * g + r) * H + j] = acc[r] * s_out;
      }
      if (RC && t > 0) ghn_of(t - 1, nxt.ghn);           // behind the same barrier as dgh: complete for every wave
    }
    dhn = acc;
    __syncthreads();   // measured: without it the waves drift apart and the step gets 8 % slower (LDS contention)
#pragma unroll
    for (int r = 0; r < 4; ++r) ycur[r] = cur.hp[r];   // Y[b, t-1]
    cur = nxt;
  }
}

}  // namespace

bool grux_shape_supported(int H) { return H >= 1 && H <= 127; }

int grux_hp(int H) { return 32 * cdiv_i(H + 1, 32); }
size_t grux_gates_floats(int B, int T, int H, int io) {
  return (size_t)cdiv_i(B, MB) * T * cdiv_i(H, 16) * grec(io) * 64 * 4;
}
int grux_blocks(int B) { return cdiv_i(B, MB); }
// bytes the recurrences really move for the stash: fp16 records in the one-pass mode (grux_gates_floats() sizes the buffer
// for the split modes' fp32 records whatever the mode)
static double gates_bytes(int B, int T, int H, int io, bool x3, bool rc = false /*r | z records: gh_n is recomputed*/) {
  return (double)cdiv_i(B, MB) * T * cdiv_i(H, 16) * (x3 ? (io ? 4 : (rc ? 2 : 3)) : (io ? 3 : 2)) * 64 * 16.0;
}
// The forward K steps (KS of grux_fwd_kernel) among the hidden widths of one BPTT instance KSB: the lowest and the highest
// (they differ where a bracket of KSB straddles H + 1 = 32 n); 0: no H <= 127 selects that KSB
constexpr int ghn_ksb(int H) { return (8 * ((2 * H + 7) / 8) + H + 31) / 32; }
constexpr int ghn_ksf(int K, bool hi) {
  int v = 0;
  for (int H = 1; H <= 127; ++H)
    if (ghn_ksb(H) == K && (v == 0 || hi)) v = (H + 32) / 32;
  return v;
}

// The one place each kernel's argument list is written (yh / yl: the two Y planes, formed by the launcher)
template <int K, bool X3, bool IO, bool ST, bool RC = false>
static void grux_fwd_go(const GruxFwdArgs& a, _Float16* yh, _Float16* yl, hipStream_t st) {
  hipLaunchKernelGGL((grux_fwd_kernel<K, X3, IO, ST, RC>), dim3(cdiv_i(a.B, MB)), dim3(NTHREADS), 0, st, a.B, a.T, a.H, a.GI, a.ldgi,
                     a.Whh, a.bhh, a.Y, a.gates, yh, yl, a.status, a.labels, a.stat_part, a.io, a.last_only, a.y_mul, a.y_add,
                     ST ? a.h0 : nullptr, ST ? a.hn : nullptr);
}

int launch_grux_fwd(const GruxFwdArgs& a, hipStream_t st) {
  const int B = a.B, T = a.T, H = a.H, io = a.io;
  const bool x3 = a.x3;
  const bool rc = a.ghn_rc && a.gates;             // r | z records (api.hip ghn_recompute): the stateless fp32-I/O split step only
  if (rc && (!x3 || io || a.h0 || a.hn)) return WGNN_ERR_UNSUPPORTED;
  if (a.last_only && (io != 0 || a.gates || a.y_planes || a.labels)) return WGNN_ERR_UNSUPPORTED;
  if (!a.Y && (!io || !a.hn || a.last_only)) return WGNN_ERR_NULL;   // Y = NULL: 16-bit I/O with h_n only (fp32: last_only into h_n)
  _Float16* yh = (_Float16*)a.y_planes;
  _Float16* yl = yh ? yh + (a.plane_rows ? a.plane_rows : (size_t)B * T + 1) * grux_hp(H) : nullptr;
  const double bt = (double)B * T;
  const double fl = bt * 2.0 * 3 * H * H,
               by = bt * ((x3 ? 4.0 : 2.0) * 3 * H + (io ? 2.0 : 4.0) * ((a.last_only ? 0 : H) + (a.labels ? H : 0))) +
                    (a.gates ? gates_bytes(B, T, H, io, x3, rc) : 0.0);
#define FLAUNCH(K, X3V, IOV, NAME)                                                                                 \
  PROF_LAUNCH(NAME, fl, by, st,                                                                                    \
              if (a.h0 || a.hn) grux_fwd_go<K, X3V, IOV, true>(a, yh, yl, st);                                     \
              else grux_fwd_go<K, X3V, IOV, false>(a, yh, yl, st))
#define FCASE(K)                                                                                                   \
  if (rc) PROF_LAUNCH("grux_fwd_kernel<" #K ">", fl, by, st, (grux_fwd_go<K, true, false, false, true>(a, yh, yl, st))); \
  else if (x3 && !io) FLAUNCH(K, true, false, "grux_fwd_kernel<" #K ">");                                          \
  else if (x3) FLAUNCH(K, true, true, "grux_fwd_kernel<" #K ">");                                                  \
  else if (!io) FLAUNCH(K, false, false, "grux_fwd_kernel<" #K ",f16>");                                           \
  else FLAUNCH(K, false, true, "grux_fwd_kernel<" #K ",f16>")
  switch (cdiv_i(H + 1, 32)) {
    case 1: FCASE(1); break;
    case 2: FCASE(2); break;
    case 3: FCASE(3); break;
    case 4: FCASE(4); break;
    default: return WGNN_ERR_UNSUPPORTED;
  }
#undef FCASE
#undef FLAUNCH
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}

int grux_hn(int H) { return 8 * cdiv_i(H, 8); }
int grux_msplit(int H) { return 8 * cdiv_i(2 * H, 8); }

// what launch_grux_bwd forms for the kernel: the hi / lo planes of dGI and dGHn, and the loss factors
struct GruxBwdFormed {
  _Float16 *ih, *il, *nh, *nl;
  int nstat;
  float inv_n, coef_in;
};
template <int K, bool X3, bool IO, int KSF, typename... Pack>   // Pack: nothing, or the BwdState
static void grux_bwd_go(const GruxBwdArgs& a, const GruxBwdFormed& f, hipStream_t st, Pack... pack) {
  hipLaunchKernelGGL((grux_bwd_kernel<K, X3, IO, KSF, Pack...>), dim3(cdiv_i(a.B, MB)), dim3(NTHREADS), 0, st, a.B, a.T, a.H, a.Whh,
                     a.Y, a.dY, a.labels, a.io, a.gates, a.GI, a.ldgi, a.scales, f.ih, f.il, a.ldd, f.nh, f.nl, a.stat_part, f.nstat,
                     f.inv_n, f.coef_in, a.loss, a.scales_out, a.status, a.write_lo, a.bhh, pack...);
}

int launch_grux_bwd(const GruxBwdArgs& a, hipStream_t st) {
  const int B = a.B, T = a.T, H = a.H, io = a.io;
  const bool x3 = a.x3, ghn_rc = a.ghn_rc;
  if (a.state && (!a.state->h0 || a.labels || a.stat_part)) return WGNN_ERR_UNSUPPORTED;   // (the state backward takes dY)
  if (ghn_rc && (!x3 || io || a.state || !a.bhh)) return WGNN_ERR_UNSUPPORTED;         // (r | z records: api.hip ghn_recompute)
  const int ksf = cdiv_i(H + 1, 32);               // the forward's K steps: the recomputed gh_n runs the forward's product
  // stat_part != null: loss and scales are finalised inside the kernel (once a separate one-block launch)
  GruxBwdFormed f;
  f.nstat = grux_blocks(B);
  f.inv_n = a.stat_part ? 1.0f / (float)a.n_loss : 0.f;
  f.coef_in = a.stat_part ? 2.0f * a.grad_scale / (float)a.n_loss : 0.f;
  f.ih = (_Float16*)a.dGI_planes;
  f.il = f.ih + (size_t)B * T * a.ldd;
  f.nh = (_Float16*)a.dGHn_planes;
  f.nl = f.nh + (size_t)B * T * grux_hn(H);
  const int ksb = cdiv_i(grux_msplit(H) + H, 32);
  if (a.ldd % 8 != 0 || a.ldd < 3 * H || a.ldd > 32 * ksb) return WGNN_ERR_SHAPE;
  if (x3 && (!a.GI || a.ldgi < 3 * H)) return WGNN_ERR_NULL;
  const double bt = (double)B * T;
  const double fl = bt * 2.0 * 3 * H * H,
               by = bt * ((io ? 2.0 + 4.0 : 4.0 + 4.0) * H + (x3 && a.write_lo ? 4.0 : 2.0) * (3 * H + H)) +
                    gates_bytes(B, T, H, io, x3, ghn_rc) + (x3 ? bt * 4.0 * H : 0.0);   // Y + labels in, planes out, stash (+ GI's n third) in
#define BLAUNCH(K, X3V, IOV, NAME)                                                                                \
  PROF_LAUNCH(NAME, fl, by, st,                                                                                   \
              if (a.state) grux_bwd_go<K, X3V, IOV, 0>(a, f, st, *a.state);                                       \
              else grux_bwd_go<K, X3V, IOV, 0>(a, f, st))
#define BLAUNCH_RC(K, KSFV) PROF_LAUNCH("grux_bwd_kernel<" #K ">", fl, by, st, (grux_bwd_go<K, true, false, KSFV>(a, f, st)))
#define BCASE(K)                                                                                                  \
  if (ghn_rc && ksf == ghn_ksf(K, false)) BLAUNCH_RC(K, ghn_ksf(K, false));                                       \
  else if (ghn_rc && ksf == ghn_ksf(K, true)) BLAUNCH_RC(K, ghn_ksf(K, true));                                    \
  else if (ghn_rc) return WGNN_ERR_UNSUPPORTED;                                                                   \
  else if (x3 && !io) BLAUNCH(K, true, false, "grux_bwd_kernel<" #K ">");                                         \
  else if (x3) BLAUNCH(K, true, true, "grux_bwd_kernel<" #K ">");                                                 \
  else if (!io) BLAUNCH(K, false, false, "grux_bwd_kernel<" #K ",f16>");                                          \
  else BLAUNCH(K, false, true, "grux_bwd_kernel<" #K ",f16>")
  switch (ksb) {
    case 1: BCASE(1); break;
    case 2: BCASE(2); break;
    case 3: BCASE(3); break;
    case 4: BCASE(4); break;
    case 5: BCASE(5); break;
    case 6: BCASE(6); break;
    case 7: BCASE(7); break;
    case 8: BCASE(8); break;
    case 9: BCASE(9); break;
    case 10: BCASE(10); break;
    case 11: BCASE(11); break;
    case 12: BCASE(12); break;
    default: return WGNN_ERR_UNSUPPORTED;
  }
#undef BCASE
#undef BLAUNCH_RC
#undef BLAUNCH
  WGNN_CHECK_LAUNCH();
  return WGNN_OK;
}
