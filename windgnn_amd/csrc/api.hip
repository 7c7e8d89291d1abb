// extern "C" entry points of libwindgnn_hip.so (declared in include/windgnn.h).
// Orchestrates the kernels of gcn.hip / gemm.hip / gru.hip / train_ops.hip on the caller's stream,
// inside caller-owned workspace and stash buffers.  No allocation, no host synchronisation.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "common.h"
#include "../../include/windgnn_optim.h"
#include "../../include/windgnn_sched.h"

namespace {

inline size_t rup(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Layout {
  size_t BT, I, Ip, G3, Gp, H, Hp;
  size_t Id;                       // row pitch of dg: I rounded up to 16 floats, so that the NT GEMMs' 64-byte store segments are aligned
  int np_g3, np_i;                 // padded plane rows of the two split-weight images (f16x3)
  // forward workspace (float offsets)
  size_t ws_GI, ws_g, ws_planes_f, ws_Ylast, ws_xtail_f, ws_xtail_b, fwd_floats;
  // stash
  size_t st_g, st_gates, st_yp, stash_floats;
  // backward workspace
  size_t ws_dGI, ws_dGH, ws_dg, ws_part_ih, ws_part_hh, ws_gcnpart, ws_planes_b, ws_scales, ws_dY, bwd_floats;
  // caller-kept images of W_ih (wgnn_params.prepared): float offsets inside that buffer, 0 floats = this mode has none
  size_t prep_f, prep_b, prep_floats;
  int prep_kind;                                 // 0 none, 1 fp16 planes, 2 padded fp32
  int sk_ih, sk_hh;
  bool tn_merge;                                 // both products are pgemm_tn_kernel tiles: one launch can run them (pgemm_tn2_kernel)
  // which kernels run: the fp16-plane family needs the dense LDS-resident GCN and the register-resident GRU;
  // shapes beyond the fast kernels (CSR adjacency, wide hidden state) use general.hip in exact fp32
  bool x3, gen_gcn, gen_gru, g32, g32tn;
  int hq;
  int np_h;                                      // padded rows of split(W_hh^T) (general f16x3 GRU)
  bool dg16;                                     // ... and dg itself ONE fp16 plane (dense GCN only)
  bool gi16;                                     // one-pass fp16 mode: the input projection GI is ONE fp16 plane
  bool dgi1;                                     // f16x3 at large B*T: dGI / dGHn are ONE fp16 plane, their three GEMMs run two passes
  bool gen2p;                                    // f16x3g on the wide-GRU path: the three GEMMs skip the lo plane of dGI / dGH
  bool small, rec32;                             // exact fp32: one-window-per-workgroup recurrences / the register-resident MFMA ones
  size_t st_hprev;                               // exact fp32, large B*T: [Hprev | 1 | 0..] rows written by the forward recurrence
  bool dghn;                                     // only the n third of dGH is stored (dGHn): fast f16x3 recurrence; rec32 at large B*T
  int hn, msplit, m_hh;                          // its row width, its first GEMM row, GEMM rows of the dW_hh product
  size_t st_h1;                                  // general GCN: layer-1 activations
  size_t st_stats;                               // wgnn_fwd_loss: MSE partial pairs (sum | max) of the forward recurrence
  size_t st_GI;                                  // split modes, register-resident recurrence: GI lives in the stash (BPTT recomputes n from its n third)
  bool gi_stash, ghn_rc;                         // ghn_rc: ... and those records are r | z, BPTT recomputes gh_n as well (ghn_recompute)
  size_t ws_gh, ws_h1, ws_yp, ws_hhp_f, ws_kp_f, ws_hc, ws_du, ws_dhz, ws_dhw, ws_hhp_b, ws_kp_b, ws_dc;   // general GRU / GCN scratch
  size_t ws_ntk_f, ws_ntk_b;                     // exact fp32, few rows: split-K partial sums of the GI / dg products
  size_t ws_aimg_f, ws_aimg_b;                   // large-shape NT plane GEMMs (configs[4]): the A operand (g / dGI) rewritten as an image
  // the state stash (wgnn_state_stash_bytes): the stash plus a copy of h0, and the dW_hh product's B operand holds h0 at every
  // window start -- fp16-plane modes: B more plane rows [h0[b] | 1 | 0..] behind the B*T rows of h_t (plane_rows = B*T + B);
  // exact fp32: the [Hprev | 1 | 0..] rows on every path, with row (b, 0) = h0[b]
  bool state;
  size_t plane_rows;                             // rows per Y plane: B*T + 1, or B*T + B in the state stash
  size_t st_h0;                                  // [B][H] fp32: h0 (zeros when the caller passed none)
};

// (min_rows = 64 measured against 128 / 192 / 256 at B*T = 6144 in round 3: fewer, longer K chunks cost the split-K GEMMs more
// -- 54 -> 78 -> 103 -> 129 us for the two -- than the smaller partial sums save the finish kernel, 16.7 -> 12.2 -> 10.9 us)
int pick_splitk(size_t BT, int tiles, int target_wgs, int min_rows) {
  int by_rows = (int)(BT / (size_t)min_rows);
  int by_grid = target_wgs / (tiles > 0 ? tiles : 1);
  int sk = by_rows < by_grid ? by_rows : by_grid;
  if (sk >= 8) sk -= sk % 8;       // multiples of 8 keep the tiles of one K chunk on one XCD
  return sk < 1 ? 1 : sk;
}

// the split-fp16 modes whose products take three passes (hi x hi + hi x lo + lo x hi); f16 takes one, f32 none
bool three_pass(const wgnn_dims* d) { return d->math == WGNN_MATH_F16X3 || d->math == WGNN_MATH_F16X3G; }

Layout make_layout(const wgnn_dims* d, bool state = false, int series = SER_NONE /*SER_FRONT / SER_REC: common.h*/) {
  Layout L;
  L.state = state;
  L.x3 = d->math != WGNN_MATH_F32;                                      // the fp16-plane kernel family
  L.gen_gcn = d->adj_format == WGNN_ADJ_CSR;
  L.gen_gru = L.x3 ? !grux_shape_supported(d->H) : !gru_shape_supported(d->H);
  const bool x3 = L.x3;
  L.BT = (size_t)d->B * d->T;
  L.I = (size_t)d->S * d->F;
  L.Ip = rup(L.I + 1, 32);                  // room for the ones column at index I
  L.Id = rup(L.I, 16);                      // (dg's 1768-byte rows made the dg GEMM write 23 % more than its output: 215 vs 174 MB)
  L.H = d->H;
  L.Hp = x3 ? (size_t)grux_hp(d->H) : 0;
  L.G3 = 3 * (size_t)d->H;
  L.Gp = rup(L.G3, 32);
  L.np_g3 = pgemm_nt_np((int)L.G3);
  L.np_i = pgemm_nt_np((int)L.I);
  auto al = [](size_t x) { return align_up(x, 64); };
  // exact fp32 at large B*T: the big-tile GEMMs of gemm32.hip on zero-padded copies of W_ih / W_ih^T
  L.g32 = !x3 && !L.gen_gcn && !L.gen_gru && gemm32_nt_supported(L.BT, (int)L.Ip, (int)L.Gp);
  L.g32tn = L.g32 && gemm32_tn_supported(L.BT);          // the split-K dW products (same threshold today)
  L.small = !x3 && !L.gen_gru && !series && gru_small_supported(d->B, d->H);
  L.rec32 = !x3 && !L.gen_gru && !L.small;
  // the images of W_ih the GEMMs stage: sized from S and H alone (the exact-fp32 ones are USED from B*T >= 4096 only),
  // so that a caller-kept copy (wgnn_params.prepared) serves every batch size
  const bool g32_shape = !x3 && !L.gen_gcn && !L.gen_gru && gemm32_nt_supported(1u << 30, (int)L.Ip, (int)L.Gp);
  const size_t planes_f = ser_front(series, x3 ? (size_t)L.np_g3 * L.Ip : (g32_shape ? (size_t)gemm32_nt_rows((int)L.G3) * L.Ip : 0));   // 2 planes of halfs = that many floats
  const size_t planes_b = ser_front(series, x3 ? (size_t)L.np_i * L.Gp : (g32_shape ? (size_t)gemm32_nt_rows((int)L.I) * L.Gp : 0));
  L.prep_kind = x3 ? 1 : (g32_shape ? 2 : 0);
  L.prep_f = 0;
  L.prep_b = al(planes_f);
  L.prep_floats = L.prep_kind ? al(planes_f) + al(planes_b) : 0;
  constexpr size_t HDR = WGNN_STATUS_BYTES / sizeof(float);   // status block at the start of the workspace
  size_t o = HDR;
  L.ws_GI = o; o += al(ser_front(series, L.BT * L.Gp));   // rows padded to 128-B multiples
  L.ws_g = o; o += al(ser_front(series, L.BT * L.Ip));    // fp32 g (f32 mode) or its two fp16 planes (f16x3): same bytes
  L.ws_planes_f = o; o += al(planes_f);
  L.np_h = pgemm_nt_np((int)L.H);
  L.ws_gh = o; o += al(L.gen_gru ? (size_t)d->B * L.Gp : 0);
  L.ws_h1 = o; o += al(L.gen_gcn ? L.BT * L.I : 0);
  L.ws_yp = o; o += al(L.gen_gru && x3 ? (L.BT + 1) * L.Hp : 0);            // h planes when there is no stash
  L.ws_hhp_f = o; o += al(L.gen_gru && x3 ? (size_t)L.np_g3 * L.Hp : 0);    // split(W_hh | b_hh)
  L.ws_kp_f = o; o += al(L.gen_gru && x3 ? pgemm_nt_kpart_floats(d->B, (int)L.Gp, (int)L.Hp) : 0);
  L.ws_hc = o; o += al(L.gen_gru && x3 ? (size_t)d->B * L.Hp : 0);          // compact planes of h_{t-1}
  L.ws_xtail_f = o; o += al(ser_front(series, (L.I & 1) && !L.gen_gcn ? L.I + 1 : 0));        // private copy of X's last tile (odd S*13: see xtail_copy)
  // wgnn_fwd_last where the recurrence writes all of Y: wgnn_fwd_last has no stash, so g lives in ws_g and is dead once GI
  // is formed -- Y aliases it whenever it fits (H <= Ip: always when H = 3S), and only otherwise gets a region of its own
  if ((x3 && !L.gen_gru) || L.rec32 || L.H <= L.Ip) { L.ws_Ylast = L.ws_g; }
  else { L.ws_Ylast = o; o += al(L.BT * L.H); }
  // the A operand of the large-shape projection GEMM as an image (pgemm_big.hip): g's two planes, when the shape is one of its
  L.ws_aimg_f = o; o += al(x3 ? pgemm_nt256_aimg_bytes((int)L.BT, (int)L.G3, (int)L.Ip, 2) / 4 : 0);
  {
    const int sk = (!x3 && !L.g32 && L.BT < 65536) ? gemm_f32_nt_splitk((int)L.BT, (int)L.G3, (int)L.I) : 1;
    L.ws_ntk_f = o; o += al(ser_front(series, sk > 1 ? (size_t)sk * L.BT * L.G3 : 0));
  }
  L.fwd_floats = o;
  o = 0;
  L.st_g = o; o += al(ser_front(series, L.BT * L.Ip));
  {  // r, z, n, gh_n of every step: [B*T][4H] fp32, or the register-resident recurrences' own record layout
    const size_t plain = L.BT * 4 * L.H, grec = (x3 && !L.gen_gru) ? grux_gates_floats(d->B, d->T, d->H, d->io)
                                                                   : (L.rec32 ? gru_gates_floats(d->B, d->T, d->H) : 0);
    L.st_gates = o; o += al(series == SER_FRONT ? 0 : series == SER_REC ? grec : (plain > grec ? plain : grec));
  }
  L.plane_rows = L.BT + (state ? (size_t)d->B : 1);
  L.st_yp = o; o += al(L.plane_rows * L.Hp);   // two planes of B*T + 1 rows (state stash: B*T + B)
  L.st_h1 = o; o += al(L.gen_gcn ? L.BT * L.I : 0);
  {  // partial pairs (sum | max) + the tag word: one pair per workgroup of the forward recurrence (B / 16, or B for gru_small)
    const size_t nb = L.small ? (size_t)gru_small_blocks(d->B) : (size_t)grux_blocks(d->B);
    L.st_stats = o; o += al(series ? 0 : 2 * nb + 4);   // (series mode keeps them in the caller's loss_buf: windgnn_series_train.h)
  }
  // split fp16 modes with the register-resident recurrence: the gate records hold r | z | gh_n only (r | z under ghn_rc, in the
  // same region) and the BPTT kernel forms n = tanh(gi_n + r gh_n) from GI, so GI goes into the stash, not the workspace
  L.gi_stash = (x3 && !L.gen_gru && three_pass(d)) || L.rec32; L.ghn_rc = !series && !L.gen_gru && ghn_recompute(d, state);
  L.st_GI = o; o += al(ser_front(series, L.gi_stash ? L.BT * L.Gp : 0));
  L.hq = (int)rup(L.H + 1, 16);
  const bool hprev_rows = L.g32tn || (state && !x3);                // (the state stash: every exact-fp32 path)
  L.st_hprev = o; o += al(ser_rec(series, hprev_rows ? L.BT * (size_t)L.hq : 0));   // [Hprev|1] with 16-byte aligned rows (exact fp32, large B*T)
  L.st_h0 = o; o += al(state ? (size_t)d->B * L.H : 0);
  L.stash_floats = o;
  L.dghn = (x3 && !L.gen_gru) || (L.rec32 && L.g32tn);
  // WGNN_MATH_F16X3G, from B*T = 4096 rows: dGI / dGHn travel as ONE fp16 plane (relative rounding 2^-12, independent per
  // element); it averages out in everything they feed -- the weight gradients sum B*T rows, the conv gradients B*T*S -- and
  // the lo plane is not written, staged or multiplied (error model and measured errors)
  L.dgi1 = d->math == WGNN_MATH_F16X3G && !L.gen_gru && L.BT >= 4096;
  // ... and on the wide-GRU path (BASELINE configs[4]: H = 12288, B*T = 3072 per GPU; its BPTT cell kernel still writes both
  // planes) the same three GEMMs simply leave dGI's / dGH's lo plane unread from B*T = 3072 rows: dW_ih one pass, dW_hh and dg
  // two -- 128 of that configuration's 175 ms per step are these products
  L.gen2p = d->math == WGNN_MATH_F16X3G && L.gen_gru && L.BT >= 3072;
  // (the GCN backward rounds dg to fp16 planes anyway: measured conv gradients 5.0e-6 vs 1.7e-6 in f16x3g; the one-pass
  // fp16 mode, whose own tolerance is 5e-2, takes it at every size)
  L.dg16 = (L.dgi1 || (d->math == WGNN_MATH_F16 && !L.gen_gru)) && !L.gen_gcn;
  // the one-pass fp16 mode (tolerance class 5e-2) also takes the forward's largest intermediate, GI [B*T][3H], as one fp16
  // plane: the projection GEMM writes and the recurrence reads half the bytes (rows keep the pitch Gp, in halfs)
  L.gi16 = d->math == WGNN_MATH_F16 && !L.gen_gru;   // (grux_fwd_kernel<.., X3 = false> reads fp16 rows)
  L.hn = x3 ? grux_hn(d->H) : gru_hn(d->H);
  L.msplit = x3 ? grux_msplit(d->H) : gru_msplit(d->H);
  // GEMM rows of the dW_hh product: [dGI_r | dGI_z | pad to msplit | dGHn]
  L.m_hh = L.dghn ? (x3 ? L.msplit + L.hn : L.msplit + (int)L.H) : (int)L.G3;
  if (x3) {
    // one workgroup per CU (256: MI355X) and product.  Register-resident recurrence: both products are pgemm_tn_kernel tiles
    // and share one launch (bwd_weights, WGNN_OPT_TN_MERGED) in which a workgroup runs one work item of each.  The splits are
    // a function of the dims alone -- not of the launch form, not of the device: the K chunks are the units finish sums in
    // a fixed order, so a moved chunk boundary regroups fp32 sums and a training run no longer repeats bit for bit
    // (profiles/tn_merged_ab.txt section B).
    L.sk_ih = pick_splitk(L.BT, pgemm_tn_tiles((int)L.G3, (int)L.I + 1), 256, 64);
    L.sk_hh = pick_splitk(L.BT, pgemm_tn_tiles(L.m_hh, (int)L.H + 1), 256, 64);
    L.tn_merge = L.dghn;
  } else {
    L.tn_merge = false;
    // K chunks of at least 128 rows (B*T = 6144 at BASELINE configs[1]: with 256-row chunks the dW_hh product had 72 workgroups)
    L.sk_ih = L.g32tn ? pick_splitk(L.BT, gemm32_tn_tiles((int)L.G3, (int)L.I + 1), 256, 64)   // one workgroup per CU
                    : pick_splitk(L.BT, gemm_f32_tiles((int)L.G3, (int)L.I + 1), 1024, 128);
    L.sk_hh = L.g32tn ? pick_splitk(L.BT, gemm32_tn_tiles(L.m_hh, (int)L.H + 1), 256, 64)
                    : pick_splitk(L.BT, gemm_f32_tiles((int)L.G3, (int)L.H + 1), 1024, 128);
  }
  size_t part_ih = (size_t)L.sk_ih * L.G3 * (L.g32tn ? (size_t)gemm32_tn_pitch((int)L.I + 1) : L.I + 1);
  size_t part_hh = (size_t)L.sk_hh * (size_t)L.m_hh * (L.g32tn ? (size_t)gemm32_tn_pitch((int)L.H + 1) : L.H + 1);
  if (x3) {
    part_ih = pgemm_tn_partial_floats((int)L.G3, (int)L.I + 1, L.sk_ih);
    part_hh = pgemm_tn_partial_floats(L.m_hh, (int)L.H + 1, L.sk_hh);
  }
  o = HDR;
  L.ws_dGI = o; o += al(L.BT * L.Gp);   // fp32, or hi+lo fp16 planes (same bytes)
  L.ws_dGH = o; o += al(ser_rec(series, L.dghn ? L.BT * (size_t)L.hn : L.BT * L.Gp));   // dGHn planes, or full dGH (general GRU / f32)
  L.ws_dg = o; o += al(ser_front(series, L.BT * L.Id));
  L.ws_part_ih = o; o += al(ser_front(series, part_ih));     // separate regions: with WGNN_BWD_DEFER both stay live until wgnn_finish
  L.ws_part_hh = o; o += al(ser_rec(series, part_hh));
  {
    size_t a = gcn32_bwd_partial_floats((int)L.BT), b = gcnx2_bwd_partial_floats((int)L.BT);
    if (L.gen_gcn) a = gcn_csr_bwd_partial_floats();
    L.ws_gcnpart = o; o += al(ser_front(series, a > b ? a : b));
  }
  L.ws_du = o; o += al(L.gen_gcn ? L.BT * L.I : 0);
  L.ws_dhz = o; o += al(L.gen_gru ? (size_t)d->B * L.H : 0);
  L.ws_dhw = o; o += al(L.gen_gru ? (size_t)d->B * L.H : 0);
  L.ws_hhp_b = o; o += al(L.gen_gru && x3 ? (size_t)L.np_h * L.Gp : 0);     // split(W_hh^T)
  L.ws_kp_b = o; o += al(L.gen_gru && x3 ? pgemm_nt_kpart_floats(d->B, (int)L.H, (int)L.Gp) : 0);
  L.ws_dc = o; o += al(L.gen_gru && x3 ? (size_t)d->B * L.Gp : 0);          // compact planes of dgh_t
  L.ws_planes_b = o; o += al(planes_b);
  L.ws_scales = o; o += al(4096);          // 3 scales, then up to 2 x 1024 block partials from offset 64
  L.ws_dY = o; o += al(series ? 0 : L.BT * L.H);          // wgnn_bwd_mse_part outside the fused kernel: dY lives here
  L.ws_xtail_b = o; o += al(ser_front(series, (L.I & 1) && !L.gen_gcn ? L.I + 1 : 0));
  L.ws_aimg_b = o; o += al(x3 ? pgemm_nt256_aimg_bytes((int)L.BT, (int)L.I, (int)L.Gp, 2) / 4 : 0);   // dGI's planes as an image (dg GEMM)
  {
    const int sk = (!x3 && !L.g32 && L.BT < 65536) ? gemm_f32_nt_splitk((int)L.BT, (int)L.I, (int)L.G3) : 1;
    L.ws_ntk_b = o; o += al(ser_front(series, sk > 1 ? (size_t)sk * L.BT * L.I : 0));
  }
  L.bwd_floats = o;
  return L;
}

// The eight slots of wgnn_params / wgnn_grads in state_dict order: conv1.w, conv1.b, conv2.w, conv2.b, w_ih, w_hh, b_ih, b_hh
template <class P>
void slots(const P& s, float* out[8]) {
  const float* v[8] = {s.conv1_weight, s.conv1_bias, s.conv2_weight, s.conv2_bias, s.w_ih, s.w_hh, s.b_ih, s.b_hh};
  for (int t = 0; t < 8; ++t) out[t] = const_cast<float*>(v[t]);
}

// every slot is set; conv = false: the four GRU slots only (wgnn_gru_fwd / wgnn_gru_bwd)
template <class P>
bool complete(const P& s, bool conv = true) {
  float* v[8];
  slots(s, v);
  for (int t = conv ? 0 : 4; t < 8; ++t)
    if (!v[t]) return false;
  return true;
}

// two buffers share a byte (a NULL one shares none)
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  return a && b && (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}

// torch.optim.Adam's bias corrections and hyper-parameters, into FinishArgs or RowsAdamArgs
template <class Args>
void set_adam(Args& a, const wgnn_adam* adam) {
  const double bc1 = 1.0 - pow((double)adam->beta1, (double)adam->step);
  const double bc2 = 1.0 - pow((double)adam->beta2, (double)adam->step);
  a.lr_over_bc1 = (float)(adam->lr / bc1);
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  a.b1 = adam->beta1; a.b2 = adam->beta2; a.eps = adam->eps;
}

// the caller-kept fp16-plane images of [W_ih | b_ih] and W_ih^T (prep_kind 1), into FinishArgs or RowsAdamArgs
template <class Args>
void set_planes(Args& a, const Layout& L, void* prepared) {
  a.pf_hi = (_Float16*)((float*)prepared + L.prep_f); a.pf_lo = a.pf_hi + (size_t)L.np_g3 * L.Ip;
  a.pb_hi = (_Float16*)((float*)prepared + L.prep_b); a.pb_lo = a.pb_hi + (size_t)L.np_i * L.Gp;
  a.np_g3 = L.np_g3; a.np_i = L.np_i;
}

// The reduction half of a finish launch: which & 4 -> the split-K partials of the two GRU weight-gradient products,
// which & 2 -> the per-workgroup partial rows of the GCN backward; gradients go to `g`.
void fill_reduce(const Layout& L, const wgnn_dims* d, const wgnn_grads* g, float* ws, int which, FinishArgs& a) {
  a.scales = ws + L.ws_scales;
  a.status = (unsigned*)ws;
  slots(*g, a.g);
  const int F = d->F;
  const int64_t n[8] = {(int64_t)F * F, F, (int64_t)F * F, F, (int64_t)L.G3 * (int64_t)L.I, (int64_t)L.G3 * (int64_t)L.H,
                        (int64_t)L.G3, (int64_t)L.G3};
  for (int t = 0; t < 8; ++t) a.n[t] = (int)n[t];
  a.I = (int)L.I;
  if (which & 4) {
    FinSeg& ih = a.ih;
    ih.partial = ws + L.ws_part_ih;
    ih.splitk = L.sk_ih;
    ih.kind = L.x3 ? 2 : 1;
    ih.Mout = ih.Mgemm = (int)L.G3; ih.Nout = (int)L.I + 1; ih.ncols = (int)L.I;
    ih.scaled = L.x3;
    FinSeg& hh = a.hh;
    hh = ih;
    hh.partial = ws + L.ws_part_hh;
    hh.splitk = L.sk_hh;
    hh.Nout = (int)L.H + 1; hh.ncols = (int)L.H;
    hh.Mgemm = L.m_hh;
    ih.pitch = L.g32tn ? gemm32_tn_pitch(ih.Nout) : ih.Nout;
    hh.pitch = L.g32tn ? gemm32_tn_pitch(hh.Nout) : hh.Nout;
    if (L.dghn) { hh.msplit = L.msplit; hh.rows1 = 2 * d->H; }     // GEMM rows [dGI_r | dGI_z | pad | dGHn]
    if (L.x3) {
      pgemm_tn_geom((int)L.G3, ih.Nout, &ih.T, &ih.nNb, &ih.ntiles);
      pgemm_tn_geom(L.m_hh, hh.Nout, &hh.T, &hh.nNb, &hh.ntiles);
    }
  }
  if (which & 2) {
    a.conv_partial = ws + L.ws_gcnpart;
    a.conv_rows = L.gen_gcn ? gcn_csr_bwd_rows()
                            : (L.x3 ? gcnx_bwd_grid((int)L.BT, d->S, three_pass(d)) : gcn32_bwd_grid((int)L.BT, d->S));
  }
}

// The optimiser half of a finish launch: parameters (updated in place), moments, hyper-parameters and the images to refresh
void fill_adam(const Layout& L, const wgnn_params* p, const wgnn_adam* adam, FinishArgs& a) {
  slots(*p, a.p);
  slots(adam->exp_avg, a.m);
  slots(adam->exp_avg_sq, a.v);
  a.adam = 1;
  set_adam(a, adam);
  if (p->prepared && L.prep_kind) {
    a.prep_kind = L.prep_kind;
    if (L.prep_kind == 1) {
      set_planes(a, L, p->prepared);
    } else {
      a.wp = (float*)p->prepared + L.prep_f;
      a.wt = (float*)p->prepared + L.prep_b;
    }
    a.Ip = (int)L.Ip; a.Gp = (int)L.Gp;
  }
}

// wgnn_finish_norm(which): the reduction of `which`, and through elem_mask a read of the other tensors as they stand in g
void fill_norm(const Layout& L, const wgnn_dims* d, const wgnn_grads* g, float* ws, int which, FinishArgs& a) {
  fill_reduce(L, d, g, ws, which, a);
  a.elem_mask = ((which & 4) ? 0u : 0xF0u) | ((which & 2) ? 0u : 0x0Fu);
}

// floats of `clip`: its header and one partial sum per block of the widest of the four wgnn_finish_norm launches; 0 if one
// of them exceeds a launch's grid.  Geometry only: the pointers of the FinishArgs built here are never followed.
size_t clip_floats(const Layout& L, const wgnn_dims* d) {
  const wgnn_grads none = {};
  float* const nowhere = reinterpret_cast<float*>((uintptr_t)WGNN_STATUS_BYTES);
  int64_t most = 0;
  for (int which = 0; which <= 6; which += 2) {
    FinishArgs a = {};
    fill_norm(L, d, &none, nowhere, which, a);
    int64_t grid;
    if (finish_grid(a, &grid) != WGNN_OK) return 0;
    most = grid > most ? grid : most;
  }
  return rup((size_t)CLIP_HDR + (size_t)most, 64);
}

// Process-wide options (wgnn_set_option / wgnn_get_option).  Keys 0 (WGNN_OPT_FUSED_FWD) and 6 (WGNN_OPT_TN_MERGED) choose
// between schedules with bit-identical results; key 4 (WGNN_OPT_BIG_GEMM) changes the summation order of the large NT plane
// products.  Keys 1, 2, 3 and 5 are retired: their other sides never measured better and went with their code paths.
//
// WGNN_OPT_FUSED_FWD: which forwards run the fused GCN + projection kernel (gcngi.hip).
//   1 (default)  forwards WITHOUT a stash (inference: wgnn_fwd(stash = NULL), wgnn_fwd_last) -- where it measured faster
//                (B = 4096: f16x3 238 -> 215 us, f16 + bf16 I/O 149 -> 139 us; no g plane reaches HBM);
//   2            every forward it supports, training too (there the stash copy of g makes it slower: 742 -> 770 us per step
//                in f16x3, 514.5 -> 514.4 in f16: DESIGN.md, fused front end);
//   0            never.  The results are bit-identical either way (tests/test_gpu_parity.py).
// The initial value comes from the environment variable WGNN_FUSED_FWD, read ONCE (a getenv per call let the
// path change mid-process and raced with putenv from other threads); afterwards only wgnn_set_option changes it.
std::atomic<int> g_opt[WGNN_OPT_COUNT];
std::once_flag g_opt_once;

int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  if (!e || !e[0]) return dflt;
  char* end = nullptr;
  const long v = strtol(e, &end, 10);
  return (end == e || v < lo || v > hi) ? dflt : (int)v;
}

void init_options() {
  std::call_once(g_opt_once, [] {
    for (int k = 0; k < WGNN_OPT_COUNT; ++k) g_opt[k].store(0, std::memory_order_relaxed);
    g_opt[WGNN_OPT_FUSED_FWD].store(env_int("WGNN_FUSED_FWD", 1, 0, 2), std::memory_order_relaxed);
    g_opt[WGNN_OPT_BIG_GEMM].store(1, std::memory_order_relaxed);
    g_opt[WGNN_OPT_TN_MERGED].store(1, std::memory_order_relaxed);
  });
}

int opt(int key) {
  init_options();
  return g_opt[key].load(std::memory_order_relaxed);
}

// option keys wgnn_set_option / wgnn_get_option accept (1, 2, 3 and 5 are retired and never reused)
bool known_option(int key) { return key == WGNN_OPT_FUSED_FWD || key == WGNN_OPT_BIG_GEMM || key == WGNN_OPT_TN_MERGED; }

int check_dims(const wgnn_dims* d) {
  if (!d) return WGNN_ERR_NULL;
  if (d->B < 1 || d->T < 1 || d->S < 1 || d->H < 1) return WGNN_ERR_SHAPE;
  if (d->F != 13) return WGNN_ERR_SHAPE;            // the reference hard-codes 13 (step6:16)
  if ((int64_t)d->B * d->T > (1 << 30)) return WGNN_ERR_SHAPE;
  if (d->math != WGNN_MATH_F32 && d->math != WGNN_MATH_F16X3 && d->math != WGNN_MATH_F16 && d->math != WGNN_MATH_F16X3G)
    return WGNN_ERR_DTYPE;
  if (d->io != WGNN_IO_F32 && d->io != WGNN_IO_F16 && d->io != WGNN_IO_BF16) return WGNN_ERR_DTYPE;
  // 16-bit X / Y / labels: only the fp16-plane kernel family with the dense LDS-resident GCN and the register-resident GRU
  if (d->io != WGNN_IO_F32 &&
      (d->math == WGNN_MATH_F32 || d->adj_format != WGNN_ADJ_DENSE || d->S > 64 || !grux_shape_supported(d->H)))
    return WGNN_ERR_UNSUPPORTED;
  if (d->adj_format == WGNN_ADJ_CSR) {
    if (d->nnz < 1 || (int64_t)d->nnz > (int64_t)d->S * d->S) return WGNN_ERR_SHAPE;
  } else if (d->adj_format == WGNN_ADJ_DENSE) {
    if (d->S > 64) return WGNN_ERR_UNSUPPORTED;     // dense adjacency is the LDS-resident path; larger graphs: CSR
  } else {
    return WGNN_ERR_UNSUPPORTED;
  }
  // 32-bit element counts inside the kernels: one weight matrix / one activation matrix must stay below 2^31
  if ((int64_t)3 * d->H * d->S * d->F >= (1ll << 31) || (int64_t)3 * d->H * d->H >= (1ll << 31)) return WGNN_ERR_SHAPE;
  if ((int64_t)d->B * d->T * d->S * d->F >= (1ll << 31) || (int64_t)d->B * d->T * 4 * d->H >= (1ll << 31))
    return WGNN_ERR_SHAPE;
  return WGNN_OK;
}

// ---- the forward ----------------------------------------------------------------------------------------------------------
// One forward request; every forward entry point fills one and calls fwd().
//   wgnn_fwd, wgnn_fwd_loss  Y, and with a stash what the backward needs (with labels also the MSE partials of Y - labels)
//   wgnn_gru_fwd             the same from g_in [B*T][S*F] instead of A and X: the recurrent half alone, conv slots unused
//   wgnn_fwd_last            last [B][H] = Y[:, T-1, :] * (wind_max - wind_min) + wind_min, no stash; Y is only written where
//                            the recurrence cannot skip it (into the workspace)
//   wgnn_fwd_state           state: no stash; the recurrence starts from h0 (NULL = zeros: exactly wgnn_fwd's kernels) and
//                            leaves the unrounded h_{T-1} in hn (nullable); Y may be NULL (then only hn is written)
//   wgnn_fwd_state_stash     sst: the training forward from h0 (nullable) into the state stash (make_layout(d, true)), which
//                            also receives h0 itself and the window-start rows of the dW_hh product's B operand; hn nullable
struct FwdCall {
  const float* A = nullptr;
  const void* X = nullptr;
  const float* g_in = nullptr;
  const wgnn_params* p = nullptr;
  const void* labels = nullptr;
  const float* h0 = nullptr;
  void* Y = nullptr;
  float* hn = nullptr;
  float* last = nullptr;
  float wind_min = 0.f, wind_max = 1.f;
  void* stash = nullptr;
  bool state = false, sst = false;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  FwdCall(void* ws, size_t ws_bytes, void* st) : workspace(ws), workspace_bytes(ws_bytes), stream(st) {}
};

// A validated forward: its layout and the buffers it resolves to
struct Fwd {
  const wgnn_dims* d;
  const FwdCall& c;
  const Layout& L;
  hipStream_t st = (hipStream_t)c.stream;
  float* ws = (float*)c.workspace;
  unsigned* status = (unsigned*)c.workspace;       // word 0 of the status block (include/windgnn.h)
  float* sf = (float*)c.stash;
  float* GI = (sf && L.gi_stash) ? sf + L.st_GI : ws + L.ws_GI;
  float* g = sf ? sf + L.st_g : ws + L.ws_g;
  float* gates = sf ? sf + L.st_gates : nullptr;
  bool full = three_pass(d);                       // three-pass split products (false: one fp16 pass, or exact fp32)
  // the staged image of [W_ih | b_ih]: the caller's (wgnn_prepare_weights / wgnn_finish keep it current) or rebuilt here
  bool kept = c.p->prepared != nullptr && L.prep_kind != 0;
  float* img_f = kept ? (float*)c.p->prepared + L.prep_f : ws + L.ws_planes_f;
  // the register-resident recurrences write last / h_n themselves; the others write every row of Y -- into the workspace
  // when the caller has no Y (wgnn_fwd_last, wgnn_fwd_state without Y) -- and last / h_n are read out of it
  bool reg = (L.x3 && !L.gen_gru) || L.rec32;
  void* Y = (!reg && (c.last || (c.state && !c.Y))) ? ws + L.ws_Ylast : c.Y;
};

// Front end: A and X (or g_in) -> GI = [g | 1] [W_ih | b_ih]^T, with g kept in the stash if there is one
int fwd_front(const Fwd& f) {
  const wgnn_dims* d = f.d;
  const FwdCall& c = f.c;
  const Layout& L = f.L;
  const wgnn_params* p = c.p;
  const int fmode = opt(WGNN_OPT_FUSED_FWD);
  int rc;
  if (c.g_in) {   // wgnn_gru_fwd: the caller's g (exact fp32, dense: checked in fwd), given its ones column
    rc = launch_pack_g(c.g_in, L.BT, (int)L.I, f.g, (int)L.Ip, f.st);
  } else if (L.x3 && !L.gen_gcn && !L.gen_gru && (fmode == 2 || (fmode == 1 && !f.sf)) && gcngi_supported(d->S, d->H, f.full)) {
    // Fused (gcngi.hip): GCN layers + input projection in one persistent kernel, g through LDS.  The results are bit-identical
    // to the separate launches below (same products, same summation order); WGNN_OPT_FUSED_FWD selects (above).
    const int planes = f.sf ? ((f.full && !L.dgi1) ? 2 : 1) : 0;   // what the backward reads of g: hi (mask, one-pass dW_ih), + lo (strict)
    return launch_gcngi_fwd((int)L.BT, d->S, c.A, c.X, d->io, p->conv1_weight, p->conv1_bias, p->conv2_weight, p->conv2_bias,
                            f.sf ? (void*)f.g : nullptr, (int)L.Ip, planes, f.img_f, L.np_g3, f.GI, (int)L.Gp, (int)L.G3, f.full,
                            f.status, f.ws + L.ws_xtail_f, f.st);
  } else if (L.gen_gcn) {   // CSR adjacency: exact fp32 SpMM layers; layer 2 writes g as fp32 rows, or as the split modes' planes
    rc = launch_gcn2_csr_fwd((int)L.BT, d->S, d->nnz, c.A, (const float*)c.X, p->conv1_weight, p->conv1_bias, p->conv2_weight,
                             p->conv2_bias, f.sf ? f.sf + L.st_h1 : f.ws + L.ws_h1, L.x3 ? nullptr : f.g, L.x3 ? f.g : nullptr,
                             L.Ip, f.full, L.x3 ? f.status : nullptr, f.st);
  } else if (L.x3) {
    rc = launch_gcnx2_fwd((int)L.BT, d->S, c.A, c.X, d->io, p->conv1_weight, p->conv1_bias, p->conv2_weight, p->conv2_bias, f.g,
                          (int)L.Ip, f.full, f.status, f.ws + L.ws_xtail_f, f.st);
  } else {
    rc = launch_gcn32_fwd((int)L.BT, d->S, c.A, (const float*)c.X, p->conv1_weight, p->conv1_bias, p->conv2_weight,
                          p->conv2_bias, f.g, (int)L.Ip, f.ws + L.ws_xtail_f, f.st);
  }
  if (rc != WGNN_OK) return rc;
  if (L.x3) {      // against the stage-major planes of [W_ih | b_ih]
    const _Float16* ghi = (const _Float16*)f.g;
    const size_t aimg_f = pgemm_nt256_aimg_bytes((int)L.BT, (int)L.G3, (int)L.Ip, 2);
    return launch_pgemm_nt(ghi, ghi + L.BT * L.Ip, (int)L.Ip, (int)L.BT, (int)L.Ip, f.img_f, L.np_g3, f.GI, (int)L.Gp,
                           (int)L.G3, nullptr, f.full, nullptr, f.st, L.gi16, aimg_f ? f.ws + L.ws_aimg_f : nullptr);
  }
  if (L.g32) {     // against a zero-padded copy of [W_ih | b_ih]
    if (!f.kept) {
      rc = launch_pad_weight(p->w_ih, (int)L.G3, (int)L.I, 0, p->b_ih, f.img_f, gemm32_nt_rows((int)L.G3), (int)L.Ip, f.st);
      if (rc != WGNN_OK) return rc;
    }
    return launch_gemm32_nt(f.g, (int)L.Ip, (int)L.BT, (int)L.Ip, f.img_f, f.GI, (int)L.Gp, (int)L.G3, f.st);
  }
  GemmArgs ga = {};
  ga.A = f.g; ga.lda = (int)L.Ip; ga.a_kcontig = 1;
  ga.B = p->w_ih; ga.ldb = (int)L.I; ga.b_kcontig = 1;
  ga.C = f.GI; ga.ldc = (int)L.Gp; ga.M = (int)L.BT; ga.N = (int)L.G3; ga.K = (int)L.I;
  ga.bias = p->b_ih; ga.splitk = 1;
  // few rows (the reference's own call shape: 168): split-K + a fixed-order sum, so that more than 15 workgroups work
  return launch_gemm_f32_nt(ga, gemm_f32_nt_splitk(ga.M, ga.N, ga.K) > 1 && L.BT < 65536 ? f.ws + L.ws_ntk_f : nullptr, f.st);
}

// Recurrence: GI -> Y, last or h_n (and, with a stash, the gate records, the Y planes / [Hprev | 1] rows and the loss statistics)
int fwd_recurrence(const Fwd& f) {
  const wgnn_dims* d = f.d;
  const FwdCall& c = f.c;
  const Layout& L = f.L;
  const wgnn_params* p = c.p;
  const float y_mul = c.wind_max - c.wind_min, y_add = c.wind_min;   // every read-out forms its multiplier this way, in fp32
  const bool hn_only = c.state && !f.Y;   // a register-resident recurrence without Y: last_only into hn (fp32 I/O) / no Y rows
  float* Y = (float*)f.Y;
  // labels (wgnn_fwd_loss): the training recurrences also leave the MSE partial sums / maxima of (Y - labels) in the stash
  // (a stash without labels gets its tag word cleared: bit 8 of a later backward cannot trust stale statistics)
  const void* labels = f.sf ? c.labels : nullptr;
  float* stats = f.sf ? f.sf + L.st_stats : nullptr;
  float* hprev = (f.sf && (L.g32tn || c.sst)) ? f.sf + L.st_hprev : nullptr;   // [Hprev | 1 | 0..] rows for the dW_hh GEMM
  int rc;
  if (L.x3 && !L.gen_gru) {   // split fp16, W_hh in registers
    GruxFwdArgs a = {};
    a.B = d->B; a.T = d->T; a.H = d->H; a.GI = f.GI; a.ldgi = (int)L.Gp; a.Whh = p->w_hh; a.bhh = p->b_hh;
    a.x3 = f.full; a.status = f.status;
    if (c.last) {
      a.Y = c.last; a.last_only = 1; a.y_mul = y_mul; a.y_add = y_add;
      return launch_grux_fwd(a, f.st);
    }
    a.io = d->io; a.h0 = c.h0;
    if (c.state) {
      const int lo = hn_only && d->io == WGNN_IO_F32;
      a.Y = lo ? (void*)c.hn : f.Y; a.last_only = lo; a.hn = lo ? nullptr : c.hn;
      return launch_grux_fwd(a, f.st);
    }
    a.Y = f.Y; a.hn = c.hn; a.gates = f.gates; a.labels = labels; a.stat_part = stats;
    a.y_planes = f.sf && !hh_from_y(d, L.tn_merge, c.sst) ? f.sf + L.st_yp : nullptr;   // (no Y planes for a dW_hh from Y)
    a.plane_rows = c.sst ? L.plane_rows : 0; a.ghn_rc = L.ghn_rc;
    rc = launch_grux_fwd(a, f.st);
  } else if (L.rec32 || L.small) {   // exact fp32, W_hh in registers
    GruFwdArgs a = {};
    a.B = d->B; a.T = d->T; a.H = d->H; a.GI = f.GI; a.ldgi = (int)L.Gp; a.Whh = p->w_hh; a.bhh = p->b_hh;
    if (L.rec32 && c.last) {
      a.Y = c.last; a.last_only = 1; a.y_mul = y_mul; a.y_add = y_add;
      return launch_gru_fwd(a, f.st);
    }
    a.h0 = c.h0;
    if (L.rec32 && c.state) {
      a.Y = hn_only ? c.hn : Y; a.last_only = hn_only ? 1 : 0; a.hn = hn_only ? nullptr : c.hn;
      return launch_gru_fwd(a, f.st);
    }
    a.Y = Y; a.hn = c.hn; a.gates = f.gates; a.labels = (const float*)labels; a.stat_part = stats; a.hprev = hprev; a.hq = L.hq;
    // few windows (L.small): one per workgroup instead of sixteen
    rc = L.rec32 ? launch_gru_fwd(a, f.st) : launch_gru_small_fwd(a, f.st);
  } else if (L.x3) {          // any hidden width: one plane GEMM per step against split(W_hh | b_hh)
    rc = launch_split_weight2(p->w_hh, (int)L.G3, (int)L.H, 0, p->b_hh, (int)L.H, f.ws + L.ws_hhp_f, L.np_g3, (int)L.Hp,
                              f.status, f.st);
    if (rc == WGNN_OK)
      rc = launch_gru_gen_fwd_x3(d->B, d->T, d->H, f.GI, (int)L.Gp, f.ws + L.ws_hhp_f, L.np_g3, p->b_hh, Y, f.gates,
                                 f.sf ? f.sf + L.st_yp : f.ws + L.ws_yp, f.ws + L.ws_gh, f.ws + L.ws_kp_f, f.ws + L.ws_hc,
                                 f.full, f.st, c.h0, c.sst ? L.plane_rows : 0);
  } else {
    rc = launch_gru_gen_fwd(d->B, d->T, d->H, f.GI, (int)L.Gp, p->w_hh, p->b_hh, Y, f.gates, f.ws + L.ws_gh, f.st, c.h0);
  }
  if (rc != WGNN_OK) return rc;
  const size_t h4 = (size_t)d->H * 4;
  if (L.gen_gru && c.hn &&    // the general recurrences have no h_n output: h_n = Y[:, T-1, :]
      hipMemcpy2DAsync(c.hn, h4, Y + (size_t)(d->T - 1) * d->H, d->T * h4, h4, d->B, hipMemcpyDeviceToDevice, f.st) != hipSuccess)
    return WGNN_ERR_HIP;
  if (c.sst) {   // the dW_hh product's B operand at every window start: h0 (the recurrences wrote zeros / [0 | 1] there)
    const float* h0c = f.sf + L.st_h0;
    if (L.x3) {  // B plane rows [h0[b] | 1 | 0..] behind the B*T rows of h_t (pgemm_tn's per-window extra rows)
      _Float16* yh = (_Float16*)(f.sf + L.st_yp);
      return launch_h0_planes(d->B, d->H, (int)L.Hp, h0c, yh + L.BT * L.Hp, yh + (L.plane_rows + L.BT) * L.Hp, f.st);
    }
    float* hp = f.sf + L.st_hprev;
    const size_t hq4 = (size_t)L.hq * 4;
    if (L.gen_gru && L.BT > 1 &&       // the general recurrence writes no [Hprev | 1] rows: row k = Y row k - 1 (the ones
        hipMemcpy2DAsync(hp + L.hq, hq4, Y, h4, h4, L.BT - 1, hipMemcpyDeviceToDevice, f.st) != hipSuccess)
      return WGNN_ERR_HIP;             // column is gemm_f32's virtual one)
    return hipMemcpy2DAsync(hp, (size_t)d->T * hq4, h0c, h4, h4, d->B, hipMemcpyDeviceToDevice, f.st) == hipSuccess ? WGNN_OK
                                                                                                              : WGNN_ERR_HIP;
  }
  if (c.last)    // the recurrences that cannot skip Y: read the last row out of the workspace
    return wgnn_predict_last(Y, d->B, d->T, d->H, c.wind_min, c.wind_max, c.last, c.stream);
  return WGNN_OK;
}

int fwd(const wgnn_dims* d, const FwdCall& c) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if ((!c.g_in && (!c.A || !c.X)) || !c.p || (!c.Y && !c.last && !(c.state && c.hn)) || (c.sst && !c.stash) || !c.workspace)
    return WGNN_ERR_NULL;
  if (!complete(*c.p, !c.g_in)) return WGNN_ERR_NULL;
  if (c.g_in && (d->math != WGNN_MATH_F32 || d->io != WGNN_IO_F32 || d->adj_format != WGNN_ADJ_DENSE)) return WGNN_ERR_UNSUPPORTED;
  // h0 is read by every workgroup while others already write h_n / Y: the buffers must not overlap
  const size_t hb = (size_t)d->B * d->H * sizeof(float), yb = (size_t)d->B * d->T * d->H * (d->io == WGNN_IO_F32 ? 4 : 2);
  if (overlap(c.h0, hb, c.hn, hb) || overlap(c.h0, hb, c.Y, yb) || overlap(c.Y, yb, c.hn, hb)) return WGNN_ERR_UNSUPPORTED;
  const Layout L = make_layout(d, c.sst);
  if (c.workspace_bytes < sizeof(float) * L.fwd_floats) return WGNN_ERR_WORKSPACE;
  const wgnn_params* p = c.p;
  hipStream_t st = (hipStream_t)c.stream;
  // wgnn_fwd_state, one hour, small batch, the reference's dense graph: the whole step as one launch (csrc/gru_step.hip)
  if (c.state && d->T == 1 && d->adj_format == WGNN_ADJ_DENSE && d->io == WGNN_IO_F32 && gru_step_supported(d->B, d->S, d->H))
    return launch_gru_step(d->B, d->S, d->H, c.A, (const float*)c.X, p->conv1_weight, p->conv1_bias, p->conv2_weight,
                           p->conv2_bias, p->w_ih, p->b_ih, p->w_hh, p->b_hh, c.h0, (float*)c.Y, c.hn, st);
  const Fwd f{d, c, L};
  if (c.sst &&   // the state stash keeps h0 (or zeros) for the backward
      (c.h0 ? hipMemcpyAsync(f.sf + L.st_h0, c.h0, hb, hipMemcpyDeviceToDevice, st)
            : hipMemsetAsync(f.sf + L.st_h0, 0, hb, st)) != hipSuccess)
    return WGNN_ERR_HIP;
  if (L.x3 && !f.kept) {   // W_ih as stage-major fp16 planes [np_g3][Ip] with b_ih folded into column I (g's ones column)
    rc = launch_split_weight2(p->w_ih, (int)L.G3, (int)L.I, 0, p->b_ih, (int)L.I, f.img_f, L.np_g3, (int)L.Ip, f.status, st);
    if (rc != WGNN_OK) return rc;
  }
  rc = fwd_front(f);
  if (rc != WGNN_OK) return rc;
  return fwd_recurrence(f);
}

// ---- the backward ---------------------------------------------------------------------------------------------------------
// One backward request; every backward entry point fills one and calls bwd().  part: the bit mask of wgnn_bwd_part.
//   wgnn_bwd_part        dY
//   wgnn_bwd_mse_part    labels, grad_scale, loss: dY = 2 (Y - labels) grad_scale / n is never written where the recurrence
//                        kernel forms it itself; loss[0] = mean((Y - labels)^2); part bit 8: the forward was wgnn_fwd_loss
//   wgnn_bwd_state_part  sst: a state stash; the BPTT kernels start from dh_n (nullable) and h0 (the stash's copy) and leave
//                        dh_{-1} in dh0 (nullable); the dW_hh products read h0 at every window start
//   wgnn_gru_bwd         dg_out: the recurrent half alone -- the four GRU gradients and dg [B*T][S*F]; A, X and the conv slots
//                        of p and of g unused
//   wgnn_bwd_rows        part 4 alone over a row range (bwd_weights): Y, stash, g only
struct BwdCall {
  const float* A = nullptr;
  const void* X = nullptr;
  const wgnn_params* p = nullptr;
  const void* Y = nullptr;
  const float* dY = nullptr;
  const void* labels = nullptr;
  float grad_scale = 1.f;
  float* loss = nullptr;
  const void* stash = nullptr;
  const wgnn_grads* g = nullptr;
  int part = 0;
  float* dg_out = nullptr;
  bool sst = false;
  const float* dhn = nullptr;
  float* dh0 = nullptr;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  BwdCall(void* ws, size_t ws_bytes, void* st) : workspace(ws), workspace_bytes(ws_bytes), stream(st) {}
};

// A validated backward: its layout and the buffers it resolves to
struct Bwd {
  const wgnn_dims* d;
  const BwdCall& c;
  const Layout& L;
  hipStream_t st = (hipStream_t)c.stream;
  float* ws = (float*)c.workspace;
  unsigned* status = (unsigned*)c.workspace;
  const float* sf = (const float*)c.stash;
  const float* Y = (const float*)c.Y;          // io-typed (d->io): only the kernels that take `io` see 16-bit data
  const float* gact = sf + L.st_g;
  float* dGI = ws + L.ws_dGI;
  float* dGH = ws + L.ws_dGH;
  float* dg = ws + L.ws_dg;
  float* scales = ws + L.ws_scales;   // [0] = 2^k, [1] = 2^-k (split-fp16 range scaling), [2] = dY coefficient; partials from 64
  bool full = three_pass(d);
  bool defer = c.part & WGNN_BWD_DEFER;          // partial sums stay in the workspace for wgnn_finish
  bool stats_ready = (c.part & 8) && c.labels;   // wgnn_fwd_loss left the MSE partials in the stash
  // the recurrence kernel forms dY from the labels itself: the fast f16x3 recurrence always (its statistics pass is
  // cheap), the exact-fp32 register-resident one when the forward left the loss statistics in the stash
  bool fused_loss = c.labels && ((L.x3 && !L.gen_gru) || ((L.rec32 || L.small) && stats_ready));
};

// Part 1: the BPTT recurrence, dY (or the loss and dY from the labels) -> the dGI / dGH buffers of the workspace
int bwd_rec(const Bwd& b) {
  const wgnn_dims* d = b.d;
  const BwdCall& c = b.c;
  const Layout& L = b.L;
  const wgnn_params* p = c.p;
  const float* labels = (const float*)c.labels;
  const float* gates = b.sf + L.st_gates;
  const float* stats = b.fused_loss && b.stats_ready ? b.sf + L.st_stats : nullptr;
  const BwdState sbs = {c.sst ? b.sf + L.st_h0 : nullptr, c.dhn, c.dh0};
  const BwdState* sb = c.sst ? &sbs : nullptr;
  const float* dY = c.dY;
  int rc;
  if (labels && !b.fused_loss) {   // other kernels: materialise dY in the workspace
    rc = launch_mse(b.Y, labels, (int64_t)L.BT * L.H, c.grad_scale, b.ws + L.ws_dY, c.loss, b.scales + 64, b.st);
    if (rc != WGNN_OK) return rc;
    dY = b.ws + L.ws_dY;
  }
  if (L.x3) {
    // Everything downstream of dY is linear in it: run it in units scaled by scales[0] = 2^k (so that
    // fp16 never sees ~1e-9 values) and multiply only the final gradients by scales[1] = 2^-k.
    if (b.fused_loss && b.stats_ready)   // the forward recurrence already reduced (Y - labels): the BPTT kernel finalises
      rc = WGNN_OK;
    else if (b.fused_loss)   // loss, the range scale and the dY coefficient in one pass over Y and the labels
      rc = launch_mse_stats(b.Y, labels, (int64_t)L.BT * L.H, c.grad_scale, c.loss, b.scales, b.scales + 64, b.st);
    else
      rc = launch_amax_scale(dY, (int64_t)L.BT * L.H, b.scales, b.scales + 64, b.st,   // 448 partials after the scales (896
                             c.dhn, c.dhn ? (int64_t)d->B * d->H : 0);               // with dh_n: the carry is scaled too)
    if (rc != WGNN_OK) return rc;
    if (L.gen_gru) {
      rc = launch_split_weight2(p->w_hh, (int)L.G3, (int)L.H, 1, nullptr, 0, b.ws + L.ws_hhp_b, L.np_h, (int)L.Gp, b.status,
                                b.st);
      if (rc != WGNN_OK) return rc;
      return launch_gru_gen_bwd_x3(d->B, d->T, d->H, b.ws + L.ws_hhp_b, L.np_h, b.Y, dY, gates, b.scales, b.dGI, b.dGH,
                                   (int)L.Gp, b.ws + L.ws_dhz, b.ws + L.ws_dhw, b.ws + L.ws_kp_b, b.ws + L.ws_dc, b.full, b.st, sb);
    }
    GruxBwdArgs a = {};
    a.B = d->B; a.T = d->T; a.H = d->H; a.Whh = p->w_hh; a.Y = c.Y; a.io = d->io; a.gates = gates;
    a.dY = b.fused_loss ? nullptr : dY; a.labels = b.fused_loss ? c.labels : nullptr;
    a.GI = L.gi_stash ? b.sf + L.st_GI : nullptr; a.ldgi = (int)L.Gp;
    a.scales = b.scales; a.dGI_planes = b.dGI; a.dGHn_planes = b.dGH; a.ldd = (int)L.Gp; a.x3 = b.full;
    a.stat_part = stats; a.n_loss = (int64_t)L.BT * L.H; a.grad_scale = c.grad_scale; a.loss = c.loss; a.scales_out = b.scales;
    a.status = b.status; a.write_lo = L.dgi1 ? 0 : 1; a.state = sb; a.bhh = p->b_hh; a.ghn_rc = L.ghn_rc;
    return launch_grux_bwd(a, b.st);
  }
  if (L.gen_gru)
    return launch_gru_gen_bwd(d->B, d->T, d->H, p->w_hh, b.Y, dY, gates, b.dGI, b.dGH, (int)L.Gp, b.ws + L.ws_dhz,
                              b.ws + L.ws_dhw, b.st, sb);
  GruBwdArgs a = {};
  a.B = d->B; a.T = d->T; a.H = d->H; a.Whh = p->w_hh; a.Y = b.Y; a.gates = gates;
  a.dY = b.fused_loss ? nullptr : dY; a.labels = b.fused_loss ? labels : nullptr;
  a.dGI = b.dGI; a.ldd = (int)L.Gp;
  a.stat_part = stats; a.n_loss = (int64_t)L.BT * L.H; a.grad_scale = c.grad_scale; a.loss = c.loss; a.status = b.status;
  a.state = sb;
  if (L.small) {
    a.dGH = b.dGH;
    return launch_gru_small_bwd(a, b.st);
  }
  // register-resident recurrence: dGHn alone when the dW_hh GEMM has the two-source A operand; fused loss
  a.GI = b.sf + L.st_GI; a.ldgi = (int)L.Gp;
  a.dGHn = L.dghn ? b.dGH : nullptr; a.dGH = L.dghn ? nullptr : b.dGH;
  return launch_gru_bwd(a, b.st);
}

// Part 4: dW_hh | db_hh = dGH^T [Hprev | 1] and dW_ih | db_ih = dGI^T [g | 1] (prods: WGNN_ROWS_HH | WGNN_ROWS_IH, in that
// order) over gate rows [r0, r0 + rows): the whole products are [0, 3H).  A range (wgnn_bwd_rows: one product, the wide-GRU
// path only -- no two-source A operand, no gemm32) is an offset on the A operand and a smaller Mout with the whole product's
// split-K count; its reduction writes those rows of g alone.  Reads only Y, the stash and the workspace.
int bwd_weights(const Bwd& b, int prods, int r0, int rows) {
  const wgnn_dims* d = b.d;
  const Layout& L = b.L;
  float* part_ih = b.ws + L.ws_part_ih;
  float* part_hh = b.ws + L.ws_part_hh;
  const bool sst = b.c.sst;
  int rc = WGNN_OK;
  if (L.x3) {
    const _Float16* dGIh = (const _Float16*)b.dGI + r0;
    const _Float16* dGHh = (const _Float16*)b.dGH + r0;
    const _Float16* gh = (const _Float16*)b.gact;
    const _Float16 *yph = (const _Float16*)(b.sf + L.st_yp), *ypl = yph + L.plane_rows * L.Hp;
    const size_t PG = L.BT * L.Gp;
    // Hprev row (b,t) = Y-plane row (b,t-1); row B*T stands in at t = 0, or in the state stash row B*T + b, window b's own
    // [h0 | 1].  Register-resident recurrence: dGH = [dGI_r | dGI_z | dGHn], the A operand takes GEMM rows < msplit from the
    // dGI planes and rows >= msplit from the dGHn planes; the reduce kernel maps the GEMM rows back to W_hh's rows.
    TnProd hh = {};
    hh.lda = (int)L.Gp; hh.Bhi = yph; hh.Blo = ypl; hh.ldb = (int)L.Hp; hh.shift_T = d->T; hh.splitk = L.sk_hh;
    hh.partial = part_hh; hh.Nout = (int)L.H + 1; hh.x3 = b.full; hh.per_window = sst;
    if (L.dghn) {
      hh.Ahi = dGIh; hh.Alo = L.dgi1 ? nullptr : dGIh + PG; hh.Mout = L.m_hh;
      hh.A2hi = dGHh; hh.A2lo = L.dgi1 ? nullptr : dGHh + L.BT * (size_t)L.hn; hh.lda2 = L.hn; hh.msplit = L.msplit;
      hh.b_stream = true;
    } else {
      hh.Ahi = dGHh; hh.Alo = L.gen2p ? nullptr : dGHh + PG; hh.Mout = rows;
    }
    // (single-plane dGI: ONE pass, hi(dGI) x hi(g) -- the rounding of g, too, is independent per element and averages
    // out over the B*T rows this product sums: measured 8.8e-6 of max at B*T = 6144 against 5.9e-6 with g's lo plane.
    // The same was measured for dW_hh (7e-5: h rows are correlated) and dg (2.8e-4 on the conv gradients: the rounding
    // of W_ih is the same for every row and does not average) and NOT adopted: they keep hi x (hi + lo).)
    const bool one_pass_ih = L.dgi1 || L.gen2p;
    TnProd ih = {};
    ih.Ahi = dGIh; ih.Alo = one_pass_ih ? dGIh : dGIh + PG; ih.lda = (int)L.Gp;
    ih.Bhi = gh; ih.Blo = gh + L.BT * L.Ip; ih.ldb = (int)L.Ip; ih.splitk = L.sk_ih;
    ih.partial = part_ih; ih.Mout = rows; ih.Nout = (int)L.I + 1; ih.x3 = b.full && !one_pass_ih; ih.b_stream = true;
    auto one = [&](const TnProd& p) {
      return launch_pgemm_tn(p.Ahi, p.Alo, p.lda, p.Bhi, p.Blo, p.ldb, p.shift_T, (int)L.BT, p.splitk, p.partial, p.Mout, p.Nout,
                             p.x3, p.A2hi, p.A2lo, p.lda2, p.msplit, b.st, p.b_stream, p.per_window);
    };
    // WGNN_OPT_TN_MERGED: both products as one launch whose work items are exactly the workgroups of the two launches
    // (same tiles, same K chunks, same partial regions: bit-identical)
    if (prods == (WGNN_ROWS_IH | WGNN_ROWS_HH) && L.tn_merge && opt(WGNN_OPT_TN_MERGED) && pgemm_tn2_covers(ih, hh)) {
      rc = launch_pgemm_tn2(ih, tn_b_from_y(hh, hh_from_y(d, L.tn_merge, sst) ? b.Y : nullptr, (int)L.H), (int)L.BT, b.st);
    } else {
      if (prods & WGNN_ROWS_HH) {
        rc = one(hh);
        if (rc != WGNN_OK) return rc;
      }
      if (prods & WGNN_ROWS_IH) rc = one(ih);
    }
  } else {
    const float* hp = b.sf + L.st_hprev;   // [Hprev | 1 | 0..] rows written by the forward recurrence (large B*T, state stash)
    if (prods & WGNN_ROWS_HH) {            // Hprev row (b,t) = Y row (b,t-1), zero at t = 0
      if (L.g32tn && L.dghn)   // dGH = [dGI_r | dGI_z | dGHn]: GEMM rows < msplit from dGI, the rest from dGHn
        rc = launch_gemm32_tn(b.dGI, (int)L.Gp, hp, L.hq, (int)L.BT, L.sk_hh, part_hh, L.m_hh, (int)L.H + 1, b.dGH, L.hn,
                              L.msplit, b.st);
      else if (L.g32tn)
        rc = launch_gemm32_tn(b.dGH, (int)L.Gp, hp, L.hq, (int)L.BT, L.sk_hh, part_hh, rows, (int)L.H + 1, nullptr, 0, 0, b.st);
      else {
        GemmArgs a = {};
        a.A = b.dGH + r0; a.lda = (int)L.Gp; a.a_kcontig = 0;
        a.B = b.Y; a.ldb = (int)L.H; a.b_kcontig = 0; a.ones_col = 1; a.shift_T = d->T;
        if (sst) { a.B = hp; a.ldb = L.hq; a.shift_T = 0; }   // the state stash's rows, h0 at window starts
        a.M = rows; a.N = (int)L.H + 1; a.K = (int)L.BT;
        a.splitk = L.sk_hh; a.partial = part_hh;
        rc = launch_gemm_f32(a, b.st);
      }
      if (rc != WGNN_OK) return rc;
    }
    if (prods & WGNN_ROWS_IH) {
      if (L.g32tn) {     // g carries its ones column (gcn32_fwd)
        rc = launch_gemm32_tn(b.dGI, (int)L.Gp, b.gact, (int)L.Ip, (int)L.BT, L.sk_ih, part_ih, rows, (int)L.I + 1, nullptr, 0,
                              0, b.st);
      } else {
        GemmArgs a = {};
        a.A = b.dGI + r0; a.lda = (int)L.Gp; a.a_kcontig = 0;
        a.B = b.gact; a.ldb = (int)L.Ip; a.b_kcontig = 0; a.ones_col = 1;
        a.M = rows; a.N = (int)L.I + 1; a.K = (int)L.BT;
        a.splitk = L.sk_ih; a.partial = part_ih;
        rc = launch_gemm_f32(a, b.st);
      }
    }
  }
  if (rc != WGNN_OK || b.defer) return rc;
  // the reduce-only form of the finish launch; a range's: its product's segment alone, output pointers at row r0
  FinishArgs a = {};
  fill_reduce(L, d, b.c.g, b.ws, 4, a);
  if (prods != (WGNN_ROWS_IH | WGNN_ROWS_HH)) {
    const bool ih = prods == WGNN_ROWS_IH;
    FinSeg& s = ih ? a.ih : a.hh;
    (ih ? a.hh : a.ih) = FinSeg{};
    if (rows != (int)L.G3) {   // (a whole product alone -- the series backward's -- keeps fill_reduce's segment, two-source rows included)
      s.Mout = s.Mgemm = rows;
      if (L.x3) pgemm_tn_geom(rows, s.Nout, &s.T, &s.nNb, &s.ntiles);
    }
    a.g[ih ? 4 : 5] += (size_t)r0 * s.ncols;                         // w_ih / w_hh
    a.g[ih ? 6 : 7] += r0;                                           // b_ih / b_hh
  }
  return launch_finish(a, b.st);
}

// Part 2: dg = dGI W_ih (split modes: in scaled units), then the GCN backward -> the four conv gradients; wgnn_gru_bwd hands
// dg to the caller instead
int bwd_dg(const Bwd& b) {
  const wgnn_dims* d = b.d;
  const BwdCall& c = b.c;
  const Layout& L = b.L;
  const wgnn_params* p = c.p;
  const bool kept = p->prepared != nullptr && L.prep_kind != 0;
  float* img_b = kept ? (float*)p->prepared + L.prep_b : b.ws + L.ws_planes_b;     // staged image of W_ih^T
  int rc;
  if (L.x3) {      // against split(W_ih^T) [np_i][Gp]
    if (!kept) {
      rc = launch_split_weight2(p->w_ih, (int)L.G3, (int)L.I, 1, nullptr, 0, img_b, L.np_i, (int)L.Gp, b.status, b.st);
      if (rc != WGNN_OK) return rc;
    }
    const _Float16* dGIh = (const _Float16*)b.dGI;
    const size_t aimg_b = pgemm_nt256_aimg_bytes((int)L.BT, (int)L.I, (int)L.Gp, 2);
    rc = launch_pgemm_nt(dGIh, (L.dgi1 || L.gen2p) ? nullptr : dGIh + L.BT * L.Gp, (int)L.Gp, (int)L.BT, (int)L.Gp, img_b,
                         L.np_i, b.dg, (int)L.Id, (int)L.I, nullptr, b.full, nullptr, b.st, L.dg16,
                         aimg_b ? b.ws + L.ws_aimg_b : nullptr);
  } else if (L.g32) {   // against a zero-padded copy of W_ih^T [I -> padded][Gp]
    if (!kept) {
      rc = launch_pad_weight(p->w_ih, (int)L.G3, (int)L.I, 1, nullptr, img_b, gemm32_nt_rows((int)L.I), (int)L.Gp, b.st);
      if (rc != WGNN_OK) return rc;
    }
    rc = launch_gemm32_nt(b.dGI, (int)L.Gp, (int)L.BT, (int)L.Gp, img_b, b.dg, (int)L.Id, (int)L.I, b.st);
  } else {
    GemmArgs a = {};
    a.A = b.dGI; a.lda = (int)L.Gp; a.a_kcontig = 1;
    a.B = p->w_ih; a.ldb = (int)L.I; a.b_kcontig = 0;
    a.C = b.dg; a.ldc = (int)L.Id; a.M = (int)L.BT; a.N = (int)L.I; a.K = (int)L.G3; a.splitk = 1;
    rc = launch_gemm_f32_nt(a, gemm_f32_nt_splitk(a.M, a.N, a.K) > 1 && L.BT < 65536 ? b.ws + L.ws_ntk_b : nullptr, b.st);
  }
  if (rc != WGNN_OK) return rc;
  if (c.dg_out) return launch_unpack_dg(b.dg, L.BT, (int)L.I, (int)L.Id, c.dg_out, b.st);
  if (L.gen_gcn)   // split modes: g as its hi plane, dg in scaled units
    rc = launch_gcn2_csr_bwd((int)L.BT, d->S, d->nnz, c.A, (const float*)c.X, p->conv2_weight, b.sf + L.st_h1,
                             L.x3 ? nullptr : b.gact, L.x3 ? b.gact : nullptr, L.Ip, b.dg, L.Id, L.x3 ? b.scales : nullptr,
                             b.ws + L.ws_du, b.ws + L.ws_gcnpart, nullptr, nullptr, nullptr, nullptr, b.st);
  else if (L.x3)
    rc = launch_gcnx2_bwd((int)L.BT, d->S, c.A, c.X, d->io, p->conv1_weight, p->conv1_bias, p->conv2_weight, b.gact, (int)L.Ip,
                          b.dg, (int)L.Id, L.dg16, b.scales, /*scale_in=*/0, b.ws + L.ws_gcnpart, b.full, b.ws + L.ws_xtail_b,
                          b.st);
  else
    rc = launch_gcn32_bwd((int)L.BT, d->S, c.A, (const float*)c.X, p->conv1_weight, p->conv1_bias, p->conv2_weight, b.gact,
                          (int)L.Ip, b.dg, (int)L.Id, nullptr, nullptr, nullptr, nullptr, b.ws + L.ws_gcnpart,
                          b.ws + L.ws_xtail_b, b.st);
  if (rc != WGNN_OK || b.defer) return rc;
  FinishArgs a = {};   // the reduce-only form of the finish launch
  fill_reduce(L, d, c.g, b.ws, 2, a);
  return launch_finish(a, b.st);
}

int bwd(const wgnn_dims* d, const BwdCall& c) {
  const int which = c.part;
  if (which < 1 || which > 31 || (which & 7) == 0) return WGNN_ERR_SHAPE;
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if ((!c.dg_out && (!c.A || !c.X)) || !c.p || !c.Y || (!c.dY && !c.labels) || !c.stash || !c.g || !c.workspace)
    return WGNN_ERR_NULL;
  if (c.labels && (which & 1) && !c.loss) return WGNN_ERR_NULL;
  if (!complete(*c.g, !c.dg_out)) return WGNN_ERR_NULL;
  if (c.dg_out && (d->math != WGNN_MATH_F32 || d->io != WGNN_IO_F32 || d->adj_format != WGNN_ADJ_DENSE || which != 7))
    return WGNN_ERR_UNSUPPORTED;
  const Layout L = make_layout(d, c.sst);
  if (c.workspace_bytes < sizeof(float) * L.bwd_floats) return WGNN_ERR_WORKSPACE;
  const Bwd b{d, c, L};
  // 16-bit labels / Y: the statistics must come from wgnn_fwd_loss (the stand-alone pass reads fp32 only)
  if (d->io != WGNN_IO_F32 && c.labels && (which & 1) && !(b.fused_loss && b.stats_ready)) return WGNN_ERR_UNSUPPORTED;
  if (which & 1) {
    rc = bwd_rec(b);
    if (rc != WGNN_OK) return rc;
  }
  if (which & 4) {   // the four GRU gradients are final after it: a data-parallel caller can start reducing them
    rc = bwd_weights(b, WGNN_ROWS_IH | WGNN_ROWS_HH, 0, (int)L.G3);
    if (rc != WGNN_OK) return rc;
  }
  return (which & 2) ? bwd_dg(b) : WGNN_OK;
}

// Row ranges of the weight-gradient products (wgnn_bwd_rows / wgnn_finish_rows): the wide-GRU path only, where each product
// is ONE TN GEMM with a plain A operand -- the register-resident recurrences remap dW_hh's GEMM rows (msplit), and the one-pass
// fp16 mode is not offered.  The alignment is the GEMM's M tile: a range is an offset on the A operand plus a smaller Mout,
// and with whole tiles and the whole product's split-K count every element sums the same terms in the same order.
int rows_align(const wgnn_dims* d, const Layout& L) {
  if (!L.gen_gru || d->math == WGNN_MATH_F16) return 0;
  return L.x3 ? TN_BM : 128;
}

int check_rows(const wgnn_dims* d, const Layout& L, int which, int row0, int rows) {
  if ((which & ~(WGNN_ROWS_IH | WGNN_ROWS_HH | WGNN_ROWS_STATE)) != 0 ||
      ((which & 3) != WGNN_ROWS_IH && (which & 3) != WGNN_ROWS_HH))
    return WGNN_ERR_SHAPE;
  if (which & WGNN_ROWS_STATE) return WGNN_ERR_UNSUPPORTED;          // per-window dW_hh rows (the state stash)
  const int al = rows_align(d, L);
  if (al == 0) return WGNN_ERR_UNSUPPORTED;
  const int64_t end = (int64_t)row0 + rows;
  if (row0 < 0 || rows < 1 || end > (int64_t)L.G3 || row0 % al != 0 || (end % al != 0 && end != (int64_t)L.G3))
    return WGNN_ERR_SHAPE;
  return WGNN_OK;
}

}  // namespace

int opt_big_gemm() { return opt(WGNN_OPT_BIG_GEMM); }

// Whether the dW_hh product of this step takes h from the caller's fp32 Y (TnProd::By) instead of the stash's fp16 Y planes,
// which the forward recurrence then does not write: their region of the stash stays untouched, the layout and
// wgnn_stash_bytes are as they were.  Both sides of a step ask here, so WGNN_OPT_TN_MERGED must not change between a forward
// and its backward.  In scope: the merged weight-gradient launch (tn_merge: the register-resident recurrence of the fp16-plane
// family) in the split-fp16 modes with fp32 I/O -- 16-bit Y is rounded on the wire, not the value the planes split -- and
// the stateless step: the carried-state entries (sst) keep their per-window [h0 | 1] plane rows.  Series mode and
// wgnn_bwd_rows run one product per launch and do not ask; every layout with tn_merge passes pgemm_tn2_covers (two-source A,
// H <= 127: one N block of at most four tiles), so a step that asked takes the merged launch.  WGNN_OPT_TN_MERGED = 0 (two
// launches) is the plane form, bit for bit the same; the environment variable WGNN_TN_YFP32 = 0, read once, keeps the planes
// under the merged launch too (the alternated runs of profiles/tn_yfp32_ab.txt).
bool hh_from_y(const wgnn_dims* d, bool tn_merge, bool sst) {
  static const int from_env = env_int("WGNN_TN_YFP32", 1, 0, 1);
  return tn_merge && three_pass(d) && d->io == WGNN_IO_F32 && !sst && from_env && opt(WGNN_OPT_TN_MERGED);
}

// Whether the gate records of this step are r | z: the forward recurrence stores no gh_n and the BPTT kernel recomputes it as
// b_hn + W_hn h_{t-1} from the h_{t-1} it loads anyway (grux.hip, the RC instances) -- 4 B x 16 ceil(H / 16) columns x B*T less
// written and less read back.  make_layout asks once per call (Layout::ghn_rc), and the forward launch and bwd_rec take it from
// their layout, so every forward and every backward entry point on the same dims agree on the record.  In scope, as hh_from_y:
// the register-resident recurrence (H <= 127) of the split-fp16 modes with fp32 I/O -- only there is Y[b, t-1] the very fp32 h
// the forward split into its MFMA operand, which makes the recomputed gh_n the forward's bit for bit -- and the stateless
// step; 16-bit I/O, the carried-state entries, series mode, the one-pass fp16 records, gru.hip, gru_small.hip and the wide-GRU
// path keep their records.  The record region and everything behind it stay where they are: the freed third is left alone.
// The environment variable WGNN_GHN_RECOMPUTE = 0 keeps the three-component record; it is read at every call (not cached), so one
// process can run both forms -- a forward and its backward must see the same value.
bool ghn_recompute(const wgnn_dims* d, bool sst) {
  return three_pass(d) && grux_shape_supported(d->H) && d->io == WGNN_IO_F32 && !sst && env_int("WGNN_GHN_RECOMPUTE", 1, 0, 1);
}

// ---- series mode (series.hip validates and sizes; the launches live here, next to the layouts and the parts they reuse) ----
// Workspace: [front | rec], each a workspace of its layout with a status block of its own; stash: [front | rec] likewise.
int series_plan(const wgnn_dims* df, const wgnn_dims* dr, SeriesPlan* sp) {
  int rc = check_dims(df);
  if (rc == WGNN_OK) rc = check_dims(dr);
  if (rc != WGNN_OK) return rc;
  const Layout Lf = make_layout(df, false, SER_FRONT), Lr = make_layout(dr, false, SER_REC);
  if ((int64_t)Lf.BT * (int64_t)Lf.Gp >= (1ll << 31)) return WGNN_ERR_SHAPE;   // 32-bit row offsets into GI_s (gru.hip)
  sp->ws_front = Lf.fwd_floats > Lf.bwd_floats ? Lf.fwd_floats : Lf.bwd_floats;
  sp->ws_rec = Lr.fwd_floats > Lr.bwd_floats ? Lr.fwd_floats : Lr.bwd_floats;
  sp->ws_front_fwd = Lf.fwd_floats;
  sp->st_front = Lf.stash_floats;
  sp->st_rec = Lr.stash_floats;
  sp->st_g = Lf.BT * Lf.Ip; sp->st_GI = Lf.BT * Lf.Gp;
  sp->st_gates = gru_gates_floats(dr->B, dr->T, dr->H);
  sp->st_hprev = Lr.g32tn ? Lr.BT * (size_t)Lr.hq : 0;
  return WGNN_OK;
}

// Ls / loss_buf (wgnn_series_fwd_loss, both or neither): the recurrence also reads the label series and leaves the MSE partial
// pairs and the tag in loss_buf; Y and the stash are the same either way.  map.starts (with stride = 0; include/windgnn_series_at.h):
// window w begins at row starts[w], clamped into [0, rows - T], instead of w * stride -- the recurrence is the only reader.
// last with Ls (include/windgnn_series_val.h): a forward alone, nothing is kept
int series_fwd(const SeriesCall& c) {
  const wgnn_dims *df = c.front, *dr = c.rec;
  const wgnn_params* p = c.p;
  const Layout Lf = make_layout(df, false, SER_FRONT);
  FwdCall cf(c.workspace, sizeof(float) * (c.last && c.Ls ? c.sp.ws_front_fwd : c.sp.ws_front), c.stream);
  cf.A = c.A; cf.X = c.Xs; cf.p = p; cf.stash = c.stash;
  const Fwd f{df, cf, Lf};
  int rc = fwd_front(f);                 // g_s and GI_s, once per hour (into the stash if there is one, else the workspace)
  if (rc != WGNN_OK) return rc;
  GruFwdArgs a = {};
  a.B = dr->B; a.T = dr->T; a.H = dr->H; a.GI = f.GI; a.ldgi = (int)Lf.Gp; a.Whh = p->w_hh; a.bhh = p->b_hh;
  a.map = c.map;
  a.map.starts_last = df->T - dr->T;     // the largest legal start: rows - T
  a.labels = c.Ls; a.stat_part = c.loss_buf; a.masked = c.masked; a.lossfn = c.lossfn;
  if (c.last) {
    a.Y = c.last; a.last_only = 1; a.y_mul = c.wind_max - c.wind_min; a.y_add = c.wind_min;
    return launch_gru_fwd(a, f.st);
  }
  const Layout Lr = make_layout(dr, false, SER_REC);
  float* sr = c.stash ? (float*)c.stash + c.sp.st_front : nullptr;
  a.Y = c.Y; a.gates = sr ? sr + Lr.st_gates : nullptr;
  a.hprev = sr && Lr.g32tn ? sr + Lr.st_hprev : nullptr; a.hq = Lr.hq;
  return launch_gru_fwd(a, f.st);
}

// dY, or Ls with the forward's loss_buf (wgnn_series_bwd_mse): BPTT forms dY = (Y - label) 2 grad_scale / (n T H) itself and its
// workgroup 0 finalises loss[0]; a missing tag sets WGNN_STATUS_NO_LOSS_STATS in the rec half's status block
int series_bwd(const SeriesCall& c) {
  const wgnn_dims *df = c.front, *dr = c.rec;
  const Layout Lf = make_layout(df, false, SER_FRONT), Lr = make_layout(dr, false, SER_REC);
  const float* sff = (const float*)c.stash;
  BwdCall cr((float*)c.workspace + c.sp.ws_front, sizeof(float) * c.sp.ws_rec, c.stream);
  cr.p = c.p; cr.Y = c.Y; cr.dY = c.dY; cr.stash = sff + c.sp.st_front; cr.g = c.grads; cr.part = 7;
  const Bwd br{dr, cr, Lr};
  BwdCall cf(c.workspace, sizeof(float) * c.sp.ws_front, c.stream);
  cf.A = c.A; cf.X = c.Xs; cf.p = c.p; cf.Y = c.Y; cf.dY = c.dY; cf.stash = c.stash; cf.g = c.grads; cf.part = 7;
  const Bwd bf{df, cf, Lf};
  // 1. BPTT per window: n is recomputed from GI_s rows w * stride + t; dGI / dGHn (or dGH) come out window-major
  GruBwdArgs a = {};
  a.B = dr->B; a.T = dr->T; a.H = dr->H; a.Whh = c.p->w_hh; a.Y = c.Y; a.dY = c.dY; a.labels = c.Ls;
  a.gates = br.sf + Lr.st_gates; a.GI = sff + Lf.st_GI; a.ldgi = (int)Lf.Gp; a.dGI = br.dGI; a.ldd = (int)Lr.Gp;
  a.dGHn = Lr.dghn ? br.dGH : nullptr; a.dGH = Lr.dghn ? nullptr : br.dGH;
  a.stat_part = c.loss_buf; a.n_loss = (int64_t)Lr.BT * Lr.H; a.grad_scale = c.grad_scale; a.loss = c.loss;
  a.status = c.Ls ? br.status : nullptr;
  a.map = c.map;
  a.map.starts_last = df->T - dr->T;
  a.masked = c.masked; a.lossfn = c.lossfn;
  int rc = launch_gru_bwd(a, br.st);
  if (rc != WGNN_OK) return rc;
  // 2. dW_hh | db_hh over the n * T window-major rows
  rc = bwd_weights(br, WGNN_ROWS_HH, 0, (int)Lr.G3);
  if (rc != WGNN_OK) return rc;
  // 3. dGI_s[tau] = sum over the windows that cover tau
  rc = c.map.starts ? launch_series_fold_at(br.dGI, c.map.starts, dr->B, dr->T, df->T, (int)Lf.G3, (int)Lf.Gp, bf.dGI, bf.st)
                    : launch_series_fold(br.dGI, dr->B, dr->T, c.map.stride, df->T, (int)Lf.G3, (int)Lf.Gp, bf.dGI, bf.st);
  if (rc != WGNN_OK) return rc;
  // 4. + 5. dW_ih | db_ih, dg and the GCN backward over the `rows` hours, each with its reduction
  rc = bwd_weights(bf, WGNN_ROWS_IH, 0, (int)Lf.G3);
  if (rc != WGNN_OK) return rc;
  return bwd_dg(bf);
}

size_t series_loss_floats(int n) { return 2 * (size_t)gru_blocks(n) + 4; }   // pairs, tag, 3 spare words (as Layout::st_stats)
size_t series_masked_loss_floats(int n) { return series_loss_floats(n) + (size_t)gru_blocks(n); }   // + the label counts

extern "C" {

int wgnn_version(void) { return WGNN_VERSION; }

int wgnn_get_option(int key) { return known_option(key) ? opt(key) : WGNN_ERR_SHAPE; }

int wgnn_set_option(int key, int value) {
  if (!known_option(key)) return WGNN_ERR_SHAPE;
  if (key == WGNN_OPT_FUSED_FWD && (value < 0 || value > 2)) return WGNN_ERR_SHAPE;
  if ((key == WGNN_OPT_BIG_GEMM || key == WGNN_OPT_TN_MERGED) && (value < 0 || value > 1)) return WGNN_ERR_SHAPE;
  init_options();
  return g_opt[key].exchange(value, std::memory_order_relaxed);
}

const char* wgnn_strerror(int status) {
  switch (status) {
    case WGNN_OK: return "ok";
    case WGNN_ERR_NULL: return "required pointer is NULL";
    case WGNN_ERR_SHAPE: return "invalid shape (need B,T,S,H >= 1 and F == 13)";
    case WGNN_ERR_DTYPE: return "unsupported dtype / math mode";
    case WGNN_ERR_WORKSPACE: return "workspace or stash too small";
    case WGNN_ERR_UNSUPPORTED:
      return "configuration not supported by this build (a dense adjacency needs S <= 64: pass larger graphs as CSR)";
    case WGNN_ERR_HIP: return "HIP runtime error (kernel launch failed)";
    case WGNN_ERR_RANGE:
      return "a value left fp16's range in an fp16-plane math mode (status block bits: 1 activation, 2 weight, 4 "
             "non-finite gradient): normalise the inputs or use WGNN_MATH_F32; or (bit 8) the backward was told the "
             "forward's loss statistics are in the stash but the last forward on it was not wgnn_fwd_loss";
    default: return "unknown status";
  }
}

size_t wgnn_workspace_bytes(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  Layout L = make_layout(d);
  return sizeof(float) * (L.fwd_floats > L.bwd_floats ? L.fwd_floats : L.bwd_floats);
}

size_t wgnn_stash_bytes(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  return sizeof(float) * make_layout(d).stash_floats;
}

size_t wgnn_state_stash_bytes(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  return sizeof(float) * make_layout(d, true).stash_floats;
}

size_t wgnn_prepared_bytes(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  return sizeof(float) * make_layout(d).prep_floats;
}

int wgnn_fwd(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, void* Y, void* stash,
             void* workspace, size_t workspace_bytes, void* stream) {
  FwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.Y = Y; c.stash = stash;
  return fwd(d, c);
}

int wgnn_fwd_loss(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const void* labels,
                  void* Y, void* stash, void* workspace, size_t workspace_bytes, void* stream) {
  if (!labels || !stash) return WGNN_ERR_NULL;
  FwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.labels = labels; c.Y = Y; c.stash = stash;
  return fwd(d, c);
}

int wgnn_fwd_last(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, float wind_min,
                  float wind_max, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!out) return WGNN_ERR_NULL;
  if (d && d->io != WGNN_IO_F32) return WGNN_ERR_UNSUPPORTED;
  FwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.last = out; c.wind_min = wind_min; c.wind_max = wind_max;
  return fwd(d, c);
}

int wgnn_fwd_state(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const float* h0, void* Y,
                   float* h_n, void* workspace, size_t workspace_bytes, void* stream) {
  FwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.h0 = h0; c.Y = Y; c.hn = h_n; c.state = true;
  return fwd(d, c);
}

int wgnn_fwd_state_stash(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const float* h0, void* Y,
                         float* h_n, void* stash, void* workspace, size_t workspace_bytes, void* stream) {
  FwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.h0 = h0; c.Y = Y; c.hn = h_n; c.stash = stash; c.sst = true;
  return fwd(d, c);
}

int wgnn_gru_fwd(const wgnn_dims* d, const float* g, const wgnn_params* p, void* Y, void* stash, void* workspace,
                 size_t workspace_bytes, void* stream) {
  if (!g) return WGNN_ERR_NULL;
  FwdCall c(workspace, workspace_bytes, stream);
  c.g_in = g; c.p = p; c.Y = Y; c.stash = stash;
  return fwd(d, c);
}

int wgnn_prepare_weights(const wgnn_dims* d, const wgnn_params* p, void* workspace, size_t workspace_bytes,
                         void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!p || !p->w_ih || !p->b_ih || !p->prepared || !workspace) return WGNN_ERR_NULL;
  if (workspace_bytes < WGNN_STATUS_BYTES) return WGNN_ERR_WORKSPACE;
  const Layout L = make_layout(d);
  if (L.prep_kind == 0) return WGNN_ERR_UNSUPPORTED;            // wgnn_prepared_bytes() said 0
  hipStream_t st = (hipStream_t)stream;
  float* img_f = (float*)p->prepared + L.prep_f;
  float* img_b = (float*)p->prepared + L.prep_b;
  if (L.prep_kind == 1) {
    rc = launch_split_weight2(p->w_ih, (int)L.G3, (int)L.I, 0, p->b_ih, (int)L.I, img_f, L.np_g3, (int)L.Ip,
                              (unsigned*)workspace, st);
    if (rc != WGNN_OK) return rc;
    return launch_split_weight2(p->w_ih, (int)L.G3, (int)L.I, 1, nullptr, 0, img_b, L.np_i, (int)L.Gp, (unsigned*)workspace, st);
  }
  rc = launch_pad_weight(p->w_ih, (int)L.G3, (int)L.I, 0, p->b_ih, img_f, gemm32_nt_rows((int)L.G3), (int)L.Ip, st);
  if (rc != WGNN_OK) return rc;
  return launch_pad_weight(p->w_ih, (int)L.G3, (int)L.I, 1, nullptr, img_b, gemm32_nt_rows((int)L.I), (int)L.Gp, st);
}

int wgnn_bwd(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const void* Y,
             const float* dY, const void* stash, const wgnn_grads* g, void* workspace, size_t workspace_bytes,
             void* stream) {
  return wgnn_bwd_part(d, A, X, p, Y, dY, stash, g, workspace, workspace_bytes, stream, 7);
}

int wgnn_bwd_part(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const void* Y,
                  const float* dY, const void* stash, const wgnn_grads* g, void* workspace, size_t workspace_bytes,
                  void* stream, int which) {
  if (!dY) return WGNN_ERR_NULL;
  BwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.Y = Y; c.dY = dY; c.stash = stash; c.g = g; c.part = which;
  return bwd(d, c);
}

int wgnn_bwd_mse_part(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const void* Y,
                      const void* labels, float grad_scale, float* loss, const void* stash, const wgnn_grads* g,
                      void* workspace, size_t workspace_bytes, void* stream, int which) {
  if (!labels) return WGNN_ERR_NULL;
  BwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.Y = Y; c.labels = labels; c.grad_scale = grad_scale; c.loss = loss; c.stash = stash; c.g = g;
  c.part = which;
  return bwd(d, c);
}

int wgnn_bwd_state_part(const wgnn_dims* d, const float* A, const void* X, const wgnn_params* p, const void* Y,
                        const float* dY, const float* dh_n, const void* stash, const wgnn_grads* g, float* dh0,
                        void* workspace, size_t workspace_bytes, void* stream, int part) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!dY) return WGNN_ERR_NULL;
  // dh0 is written while dY, dh_n and the stash are read
  const size_t hb = (size_t)d->B * d->H * sizeof(float), yb = (size_t)d->B * d->T * d->H * sizeof(float);
  if (overlap(dh0, hb, dh_n, hb) || overlap(dh0, hb, dY, yb) || overlap(dh0, hb, stash, wgnn_state_stash_bytes(d)))
    return WGNN_ERR_UNSUPPORTED;
  BwdCall c(workspace, workspace_bytes, stream);
  c.A = A; c.X = X; c.p = p; c.Y = Y; c.dY = dY; c.stash = stash; c.g = g; c.part = part;
  c.sst = true; c.dhn = dh_n; c.dh0 = dh0;
  return bwd(d, c);
}

int wgnn_gru_bwd(const wgnn_dims* d, const float* g, const wgnn_params* p, const void* Y, const float* dY, const void* stash,
                 const wgnn_grads* grads, float* dg, void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !dY || !dg) return WGNN_ERR_NULL;
  BwdCall c(workspace, workspace_bytes, stream);
  c.p = p; c.Y = Y; c.dY = dY; c.stash = stash; c.g = grads; c.part = 7; c.dg_out = dg;
  return bwd(d, c);
}

int wgnn_bwd_rows_align(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  return rows_align(d, make_layout(d));
}

int wgnn_bwd_rows(const wgnn_dims* d, const void* Yv, const void* stash, const wgnn_grads* g, int which, int row0, int rows,
                  void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!Yv || !stash || !g || !workspace) return WGNN_ERR_NULL;
  const bool ih = (which & 3) == WGNN_ROWS_IH;
  if (ih ? (!g->w_ih || !g->b_ih) : (!g->w_hh || !g->b_hh)) return WGNN_ERR_NULL;
  const Layout L = make_layout(d);
  rc = check_rows(d, L, which, row0, rows);
  if (rc != WGNN_OK) return rc;
  if (workspace_bytes < sizeof(float) * L.bwd_floats) return WGNN_ERR_WORKSPACE;
  BwdCall c(workspace, workspace_bytes, stream);
  c.Y = Yv; c.stash = stash; c.g = g;
  // (the A operand is read from column row0 on; the last range's final tile reads columns past 3H exactly as the whole
  // product's does -- any finite data, inside the workspace -- and its rows are never stored)
  return bwd_weights(Bwd{d, c, L}, which & 3, row0, rows);
}

int wgnn_finish(const wgnn_dims* d, const wgnn_params* p, const wgnn_grads* g, int which, const wgnn_adam* adam,
                void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  const int only = which & (WGNN_FINISH_ADAM_GRU | WGNN_FINISH_ADAM_CONV);   // optimiser step of one tensor family
  if ((which & ~(6 | WGNN_FINISH_ADAM_GRU | WGNN_FINISH_ADAM_CONV)) != 0 || (which == 0 && !adam)) return WGNN_ERR_SHAPE;
  if (only && (!adam || (which & 6) != 0 || only == (WGNN_FINISH_ADAM_GRU | WGNN_FINISH_ADAM_CONV))) return WGNN_ERR_SHAPE;
  if (!g || !workspace || (adam && !p)) return WGNN_ERR_NULL;
  if (!complete(*g)) return WGNN_ERR_NULL;
  const Layout L = make_layout(d);
  if (workspace_bytes < sizeof(float) * L.bwd_floats) return WGNN_ERR_WORKSPACE;
  FinishArgs a = {};
  fill_reduce(L, d, g, (float*)workspace, which, a);
  if (adam) {
    if (!complete(*p)) return WGNN_ERR_NULL;
    if (adam->step < 1) return WGNN_ERR_SHAPE;
    if (!complete(adam->exp_avg) || !complete(adam->exp_avg_sq)) return WGNN_ERR_NULL;
    fill_adam(L, p, adam, a);
    a.elem_mask = ((which & 4) ? 0u : 0xF0u) | ((which & 2) ? 0u : 0x0Fu);   // tensors whose gradient is final in g
    if (only == WGNN_FINISH_ADAM_GRU) a.elem_mask = 0xF0u;
    if (only == WGNN_FINISH_ADAM_CONV) a.elem_mask = 0x0Fu;
  }
  return launch_finish(a, (hipStream_t)stream);
}

int wgnn_optim_version(void) { return WGNN_OPTIM_VERSION; }

// include/windgnn_sched.h
int wgnn_tn_split(const wgnn_dims* d, int state, wgnn_tn_split_info* out) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!out) return WGNN_ERR_NULL;
  const Layout L = make_layout(d, state != 0);
  out->sk_ih = L.sk_ih;
  out->sk_hh = L.sk_hh;
  out->kchunk_ih = cdiv_i(cdiv_i((int)L.BT, L.sk_ih), 32) * 32;
  out->kchunk_hh = cdiv_i(cdiv_i((int)L.BT, L.sk_hh), 32) * 32;
  out->merged = L.tn_merge ? 1 : 0;
  out->workgroups = 0;
  if (L.x3) {
    const int ni = L.sk_ih * pgemm_tn_tiles((int)L.G3, (int)L.I + 1), nh = L.sk_hh * pgemm_tn_tiles(L.m_hh, (int)L.H + 1);
    out->workgroups = L.tn_merge ? (ni > nh ? ni : nh) : ni + nh;
  }
  return WGNN_OK;
}

size_t wgnn_clip_bytes(const wgnn_dims* d) {
  if (check_dims(d) != WGNN_OK) return 0;
  return sizeof(float) * clip_floats(make_layout(d), d);
}

int wgnn_finish_norm(const wgnn_dims* d, const wgnn_grads* g, int which, float max_norm, void* clip, void* workspace,
                     size_t workspace_bytes, void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if ((which & ~6) != 0 || !(max_norm > 0.f)) return WGNN_ERR_SHAPE;   // (NaN fails the comparison)
  if (!g || !clip || !workspace) return WGNN_ERR_NULL;
  if (!complete(*g)) return WGNN_ERR_NULL;
  const Layout L = make_layout(d);
  if (workspace_bytes < sizeof(float) * L.bwd_floats) return WGNN_ERR_WORKSPACE;
  FinishArgs a = {};
  fill_norm(L, d, g, (float*)workspace, which, a);
  a.clip = (float*)clip;
  a.max_norm = max_norm;
  // (an internal consistency check of this launch against wgnn_clip_bytes' own arithmetic -- both depend on dims alone -- NOT a
  // check of the caller's buffer, whose real size the library cannot know: a clip shorter than wgnn_clip_bytes(d) is overrun)
  int64_t grid;
  if (finish_grid(a, &grid) != WGNN_OK || (size_t)CLIP_HDR + (size_t)grid > clip_floats(L, d)) return WGNN_ERR_SHAPE;
  return launch_finish_norm(a, (hipStream_t)stream);
}

int wgnn_finish_clipped(const wgnn_dims* d, const wgnn_params* p, const wgnn_grads* g, const wgnn_adam* adam, const void* clip,
                        void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!p || !g || !adam || !clip || !workspace) return WGNN_ERR_NULL;
  if (!complete(*g) || !complete(*p) || !complete(adam->exp_avg) || !complete(adam->exp_avg_sq)) return WGNN_ERR_NULL;
  if (adam->step < 1) return WGNN_ERR_SHAPE;
  const Layout L = make_layout(d);
  if (workspace_bytes < sizeof(float) * L.bwd_floats) return WGNN_ERR_WORKSPACE;
  FinishArgs a = {};
  fill_norm(L, d, g, (float*)workspace, 0, a);      // every tensor is read from g
  fill_adam(L, p, adam, a);
  a.clip = const_cast<float*>((const float*)clip);  // (read only: clip[1])
  return launch_finish_clipped(a, (hipStream_t)stream);
}

int wgnn_finish_rows(const wgnn_dims* d, const wgnn_params* p, const wgnn_grads* g, int which, int row0, int rows,
                     const wgnn_adam* adam, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_dims(d);
  if (rc != WGNN_OK) return rc;
  if (!p || !g || !adam || !workspace) return WGNN_ERR_NULL;
  const Layout L = make_layout(d);
  rc = check_rows(d, L, which, row0, rows);
  if (rc != WGNN_OK) return rc;
  if (adam->step < 1) return WGNN_ERR_SHAPE;
  if (workspace_bytes < WGNN_STATUS_BYTES) return WGNN_ERR_WORKSPACE;
  const bool ih = (which & 3) == WGNN_ROWS_IH;
  const wgnn_grads& m = adam->exp_avg;
  const wgnn_grads& v = adam->exp_avg_sq;
  RowsAdamArgs r = {};
  r.ncols = ih ? (int)L.I : (int)L.H;
  const size_t off = (size_t)row0 * r.ncols;
  r.p_w = const_cast<float*>(ih ? p->w_ih : p->w_hh);               // the optimiser updates the parameters in place
  r.m_w = ih ? m.w_ih : m.w_hh;
  r.v_w = ih ? v.w_ih : v.w_hh;
  r.g_w = ih ? g->w_ih : g->w_hh;
  r.p_b = const_cast<float*>(ih ? p->b_ih : p->b_hh);
  r.m_b = ih ? m.b_ih : m.b_hh;
  r.v_b = ih ? v.b_ih : v.b_hh;
  r.g_b = ih ? g->b_ih : g->b_hh;
  if (!r.p_w || !r.m_w || !r.v_w || !r.g_w || !r.p_b || !r.m_b || !r.v_b || !r.g_b) return WGNN_ERR_NULL;
  r.p_w += off; r.m_w += off; r.v_w += off; r.g_w += off;
  r.p_b += row0; r.m_b += row0; r.v_b += row0; r.g_b += row0;
  r.row0 = row0;
  r.rows = rows;
  set_adam(r, adam);
  r.status = (unsigned*)workspace;
  if (ih && p->prepared && L.prep_kind == 1) set_planes(r, L, p->prepared);
  return launch_adam_rows(r, (hipStream_t)stream);
}

// F == F_out == 13 (the reference's own layers, src/main.py:41): the MFMA kernels of gcn.hip; other widths up to 64: gcn_any.hip;
// max(F, F_out) > 64: gcn_wide.hip.  0 = fits none of them; WGNN_ERR_SHAPE / WGNN_ERR_UNSUPPORTED otherwise.
static int gcn_layer_route(int32_t ntiles, int32_t S, int32_t F, int32_t F_out, bool* wide) {
  if (ntiles < 1 || S < 1 || F < 1 || F_out < 1) return WGNN_ERR_SHAPE;
  // the tile loops of gcn.hip (base += gridDim.x * WAVES) and gcn_any.hip (t += gridDim.x) advance a 32-bit tile counter by their
  // grid past the last tile before they test it: it must not wrap (S = F = F_out = 1 reaches this with 8 GiB of X).  4096 = the
  // largest such step: grid_for() / ga_grid() cap the grid at 1024 workgroups and gcn.hip runs WAVES = 4 tiles per workgroup; a
  // larger grid cap or more waves per workgroup there raises this constant with it
  if ((int64_t)ntiles + 4096 > INT32_MAX) return WGNN_ERR_SHAPE;
  *wide = F > 64 || F_out > 64;
  if (*wide && !gcn_wide_countable(ntiles, S, F, F_out)) return WGNN_ERR_SHAPE;
  if (!(*wide ? gcn_wide_supported(S, F, F_out) : gcn_any_supported(S, F, F_out))) return WGNN_ERR_UNSUPPORTED;
  return WGNN_OK;
}

size_t wgnn_gcn_layer_workspace_bytes(int32_t ntiles, int32_t S, int32_t F, int32_t F_out) {
  bool wide = false;
  if (gcn_layer_route(ntiles, S, F, F_out, &wide) != WGNN_OK) return 0;
  if (wide) return sizeof(float) * gcn_wide_bwd_ws_floats(ntiles, S, F, F_out);
  if (F == 13 && F_out == 13) return sizeof(float) * gcn1_bwd_partial_floats(ntiles);
  return sizeof(float) * gcn_any_bwd_partial_floats(ntiles, F, F_out);
}

int wgnn_gcn_layer_fwd(int32_t ntiles, int32_t S, int32_t F, int32_t F_out, const float* A, const float* X, const float* W,
                       const float* b, float* out, void* stream) {
  bool wide = false;
  const int rc = gcn_layer_route(ntiles, S, F, F_out, &wide);
  if (rc != WGNN_OK) return rc;
  if (!A || !X || !W || !b || !out) return WGNN_ERR_NULL;
  if (wide) return launch_gcn_wide_fwd(ntiles, S, F, F_out, A, X, W, b, out, (hipStream_t)stream);
  if (F == 13 && F_out == 13) return launch_gcn1_fwd(ntiles, S, A, X, W, b, out, (hipStream_t)stream);
  return launch_gcn_any_fwd(ntiles, S, F, F_out, A, X, W, b, out, (hipStream_t)stream);
}

int wgnn_gcn_layer_bwd(int32_t ntiles, int32_t S, int32_t F, int32_t F_out, const float* A, const float* X, const float* W,
                       const float* out, const float* dout, float* dW, float* db, float* dX, void* workspace,
                       size_t workspace_bytes, void* stream) {
  bool wide = false;
  const int rc = gcn_layer_route(ntiles, S, F, F_out, &wide);
  if (rc != WGNN_OK) return rc;
  if (!A || !X || !W || !out || !dout || !dW || !db || !workspace) return WGNN_ERR_NULL;
  if (workspace_bytes < wgnn_gcn_layer_workspace_bytes(ntiles, S, F, F_out)) return WGNN_ERR_WORKSPACE;
  if (wide)
    return launch_gcn_wide_bwd(ntiles, S, F, F_out, A, X, W, out, dout, dW, db, dX, (float*)workspace, (hipStream_t)stream);
  if (F == 13 && F_out == 13)
    return launch_gcn1_bwd(ntiles, S, A, X, W, out, dout, dW, db, dX, (float*)workspace, (hipStream_t)stream);
  return launch_gcn_any_bwd(ntiles, S, F, F_out, A, X, W, out, dout, dW, db, dX, (float*)workspace, (hipStream_t)stream);
}

size_t wgnn_gcn_layer_csr_workspace_bytes(int32_t ntiles, int32_t S, int32_t F) {
  if (ntiles < 1 || S < 1 || F != 13 || (int64_t)ntiles * S * F >= (1ll << 31)) return 0;
  return sizeof(float) * gcn1_csr_bwd_ws_floats(ntiles, S);
}

int wgnn_gcn_layer_csr_fwd(int32_t ntiles, int32_t S, int32_t F, int32_t nnz, const void* csr, const float* X,
                           const float* W, const float* b, float* out, void* stream) {
  if (ntiles < 1 || S < 1 || F != 13 || nnz < 1 || (int64_t)ntiles * S * F >= (1ll << 31)) return WGNN_ERR_SHAPE;
  if (!csr || !X || !W || !b || !out) return WGNN_ERR_NULL;
  return launch_gcn1_csr_fwd(ntiles, S, nnz, csr, X, W, b, out, (hipStream_t)stream);
}

int wgnn_gcn_layer_csr_bwd(int32_t ntiles, int32_t S, int32_t F, int32_t nnz, const void* csr, const float* X,
                           const float* W, const float* out, const float* dout, float* dW, float* db, float* dX,
                           void* workspace, size_t workspace_bytes, void* stream) {
  if (ntiles < 1 || S < 1 || F != 13 || nnz < 1 || (int64_t)ntiles * S * F >= (1ll << 31)) return WGNN_ERR_SHAPE;
  if (!csr || !X || !W || !out || !dout || !dW || !db || !workspace) return WGNN_ERR_NULL;
  if (workspace_bytes < wgnn_gcn_layer_csr_workspace_bytes(ntiles, S, F)) return WGNN_ERR_WORKSPACE;
  return launch_gcn1_csr_bwd(ntiles, S, nnz, csr, X, W, out, dout, dW, db, dX, (float*)workspace, (hipStream_t)stream);
}

int wgnn_mse_loss_grad(const float* Y, const float* L, int64_t n, float grad_scale, float* dY, float* loss,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!Y || !L || !loss || !workspace) return WGNN_ERR_NULL;
  if (n < 1) return WGNN_ERR_SHAPE;
  if (workspace_bytes < 4096) return WGNN_ERR_WORKSPACE;
  return launch_mse(Y, L, n, grad_scale, dY, loss, (float*)workspace, (hipStream_t)stream);
}

int wgnn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t step,
                   float lr, float beta1, float beta2, float eps, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq) return WGNN_ERR_NULL;
  if (n < 1 || step < 1) return WGNN_ERR_SHAPE;
  return launch_adam(param, grad, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, (hipStream_t)stream);
}

}  // extern "C"
