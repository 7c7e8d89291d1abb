"""The per-instance parity table: which compile-time kernel instance each launcher of windgnn_amd/csrc selects for which
dims, and one case per instance (tests/test_gpu_instances.py proves each on the GPU, tests/test_instance_table_host.py checks
the table against the launcher sources).  A plain module: nothing here is collected.

An *instance key* is the profiler name of the launch plus, behind '|', the compile-time arguments (and the few run-time
switches that select another code path inside the kernel) the name does not show.  `plan()` is the dispatcher of
csrc/api.hip restated in Python: for the dims and the call form of a case it returns every key of the tabled families that
one step launches.  The GPU test compares the profiler's names with it, so the hidden arguments are fixed by the call form:
each family's section below says how.

A case is (family, key, S, T, B, H, math, io, state, route):
  math   'f32' | 'f16x3' | 'f16' | 'f16x3g';  io 'f32' | 'f16' | 'bf16' (type of X, Y and the labels);
  state  the carried-state entry points (wgnn_fwd_state_stash + wgnn_bwd_state_part with h0, dY, dh_n, dh0);
  route  'train'     wgnn_fwd_loss + wgnn_bwd_mse_part(7 | 8)          (state: the two state entry points)
         'unmerged'  the same with WGNN_OPT_TN_MERGED = 0               (one launch per weight-gradient product)
         'fused'     the same with WGNN_OPT_FUSED_FWD = 2               (gcngi_fwd_kernel writes the stash planes of g)
         'infer'     wgnn_fwd without a stash                           (gcngi_fwd_kernel, no plane of g written)
Shapes are the smallest that select the instance: T = 2 or 3, the smallest S / H of the wanted tile count, B = 17 (B = 1 mod 16:
the last workgroup of a recurrence is ragged), and the threshold itself where a threshold selects (see CASES).

The six window-major recurrence families have a second case per key at the other end of the bracket, EDGE_CASES: H at the TOP
of the key's width bracket (bracket_top()) and T = 5, so that interior time steps run on full tiles;
tests/test_gpu_instance_edges.py proves them on the GPU.

The two NT GEMM families (NT_FAMILIES) have a second case per key past a one-stage K loop, KLOOP_CASES: nt_products() restates
plan()'s NT launches with their contraction, and the product that carries the key runs seven K stages instead of one;
tests/test_gpu_instance_kloop.py proves them on the GPU.

gemm_f32_kernel has the same second half: gemm_f32_products() restates plan()'s gemm.hip launches with their contraction,
GEMM_F32_KLOOP_CASES runs every NT key at seven K steps of 16 columns instead of one and GEMM_F32_FOLD_CASES takes every tile past
the two-level fold (33 steps in one chunk); tests/test_general_loops_host.py re-derives them, tests/test_gpu_general_loops.py
proves them on the GPU (next to the CSR layers' item loop: tests/general_cases.py).

The three TN weight-gradient GEMM families (TN_FAMILIES) have theirs: tn_products() restates plan()'s TN launches with their
contraction over the B*T rows (split-K chunks walked in stages of 32 rows), and TN_KLOOP_CASES runs every key at seven stages a
chunk instead of two or three, both B sources of the merged launch included; tests/test_tn_kloop_host.py re-derives them,
tests/test_gpu_tn_kloop.py proves them on the GPU.

The series entry points (wgnn_series_*) have their own half: SERIES_FAMILIES, series_plan() and SERIES_CASES, whose cases are
(family, key, S, H, rows, T, stride, n, seed, route) with route 'series' (wgnn_series_fwd + wgnn_series_bwd with a signed
random dY), 'series_mse' (wgnn_series_fwd_loss + wgnn_series_bwd_mse) or 'series_last' (wgnn_series_fwd_last);
tests/test_gpu_series_instances.py proves them on the GPU."""
import re

MATHS = ("f32", "f16x3", "f16", "f16x3g")
ROUTES = ("train", "unmerged", "fused", "infer")


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


# ---- the integer lists of the launchers (test_instance_table_host.py extracts the same lists from the sources) ------------
GRUX_FWD_K = [1, 2, 3, 4]                                   # grux.hip launch_grux_fwd: switch (cdiv_i(H + 1, 32))
GRUX_BWD_K = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]        # grux.hip launch_grux_bwd: switch (ksb)
GRU_FWD_KS = [4, 8, 12, 16, 20, 24, 26, 28, 32]             # gru.hip FWD_KS and the FCASE list
GRU_BWD_KS3 = [12, 24, 36, 48, 60, 72, 78, 84, 96]          # gru.hip BWD_KS3 and the BCASE list
SMALL_HMAX = [32, 64, 96, 108, 112, 128]                    # gru_small.hip small_hmax's returns and SMALL_DISPATCH
SMALL_HMAX_UPTO = [32, 64, 96, 106, 112]                    # ... and its thresholds (H <= 106 -> 108), else 128
GCNX_NT = [1, 2, 3, 4]                                      # gcnx.hip launch_gcnx2_fwd / _bwd: switch ((S + 15) / 16)
GCNGI_NT = [1, 2, 3]                                        # gcngi.hip launch_gcngi_fwd
GCN32_NT = [1, 2, 3, 4]                                     # gcn32.hip launch_gcn32_fwd / _bwd
PGEMM_NT_T = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]   # pgemm.hip launch_pgemm_nt: NT_CASE
PGEMM_TN_T = [1, 2, 3, 4, 5, 6, 7]                          # pgemm.hip launch_pgemm_tn: TN_CASE
TN2_TI = [1, 2, 3, 4, 5, 6, 7]                              # pgemm.hip launch_pgemm_tn2: TN2_ROW
TN2_TH = [1, 2, 3, 4]                                       # ... and the TN2_CASEs of one row
GEMM32_NT_BIG_T = [1, 2, 3, 4, 5, 6, 7]                     # gemm32.hip launch_gemm32_nt: NT_CASE of the 128-row form
GEMM32_NT_SMALL_T = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]   # ... of the 32-row form
GEMM32_TN_T = [1, 2, 3, 4, 5, 6, 7]                         # gemm32.hip launch_gemm32_tn: TN_CASE


# ---- selection formulas (each restates the launcher named) ---------------------------------------------------------------
def grux_fwd_k(H):
    return cdiv(H + 1, 32)


def grux_bwd_k(H):
    return cdiv(8 * cdiv(2 * H, 8) + H, 32)


def pick_ks(need, ks):
    return next((k for k in ks if k >= need), -1)


def gru_fwd_k(H):
    return pick_ks(cdiv(H, 4), GRU_FWD_KS)


def gru_bwd_k(H):
    return pick_ks(cdiv(3 * H, 4), GRU_BWD_KS3)


def small_hmax(H):
    for upto, hmax in zip(SMALL_HMAX_UPTO, SMALL_HMAX):
        if H <= upto:
            return hmax
    return SMALL_HMAX[-1]


def gcn_nt(S):
    return (S + 15) // 16


def pgemm_nt_shape(M, N, nchunks=1):
    """pgemm.hip nt_shape: (slices, T, 'wide' | 'narrow'); narrow = N cut finer than it has to be, to fill the CUs."""
    nsl = cdiv(N, 448)
    T = cdiv(cdiv(N, nsl), 32)
    nm = cdiv(M, 192)
    if nm * nsl * nchunks < 192:
        want = min(cdiv(256, nm), cdiv(N, 32))
        T = cdiv(cdiv(N, want), 32)
        return cdiv(N, 32 * T), T, "narrow"
    return nsl, T, "wide"


def pgemm_nt_chunks(Kp):
    return cdiv(Kp, 4096) if Kp > 4096 + 2048 else 1


def pgemm_tn_shape(Nout):
    """pgemm.hip tn_shape: (N blocks, T)."""
    nNb = cdiv(Nout, 224)
    return nNb, cdiv(cdiv(Nout, nNb), 32)


def gemm32_nt_shape(N, big):
    t32 = cdiv(N, 32)
    nsl = cdiv(t32, 14)
    return nsl, (cdiv(cdiv(t32, nsl), 2) if big else cdiv(t32, nsl))


def gemm32_tn_shape(No):
    t16 = cdiv(No, 16)
    nNb = cdiv(t16, 14)
    return nNb, cdiv(cdiv(t16, nNb), 2)


def gemm_f32_tile(M, N):
    if cdiv(M, 128) * cdiv(N, 128) >= 1024:
        return 128, 128
    bn = 64 if rup(N, 64) < rup(N, 128) else 128
    bm = 64 if (rup(M, 64) < rup(M, 128) or cdiv(M, 128) * cdiv(N, bn) < 512) else 128
    return bm, bn


def gemm_f32_tiles(M, N):
    bm, bn = gemm_f32_tile(M, N)
    return cdiv(M, bm) * cdiv(N, bn)


def gemm_f32_nt_splitk(M, N, K):
    if gemm_f32_tiles(M, N) >= 64:
        return 1
    sk = K // 64
    return 1 if sk < 2 else min(sk, 8)


def gemm_f32_name(M, N, splitk, form):
    bm, bn = gemm_f32_tile(M, N)
    if bm == 128 and cdiv(M, 128) * cdiv(N, bn) * splitk < 256:
        bm = 64
    return "gemm_f32_kernel<%d,%d>[%s]" % (bm, bn, form)


def pick_splitk(BT, tiles, target, min_rows):
    sk = min(BT // min_rows, target // max(tiles, 1))
    if sk >= 8:
        sk -= sk % 8
    return max(sk, 1)


def gcngi_supported(S, H, x3):
    NT = gcn_nt(S)
    if NT < 1 or NT > 3 or 3 * H > 384:
        return False
    Ip = rup(S * 13 + 1, 32)
    ng, rows, pl = (8, 32, 2) if x3 else (12, 48, 1)
    smem = 2 * NT * ((NT + 1) // 2) * 64 * 16 + ng * 16 * NT * 20 * 4 + 2 * pl * rows * (2 * Ip + 16)
    return smem <= 160 * 1024


def refusal(S, T, B, H, math, io):
    """api.hip check_dims for a dense adjacency: None, or the reason the library refuses the dims."""
    if S > 64:
        return "dense adjacency: S <= 64 (api.hip check_dims)"
    if io != "f32" and (math == "f32" or H > 127):
        return "16-bit I/O: the fp16-plane family with the register-resident GRU only (api.hip check_dims)"
    return None


def g32_rows(BT, S, H):
    """api.hip make_layout, L.g32 (and L.g32tn: gemm32_tn_supported is the same threshold) of an exact-fp32 layout of BT rows
    with gru.hip's or gru_small.hip's recurrence: gemm32.hip's products instead of gemm.hip's."""
    return BT >= 4096 and rup(13 * S + 1, 32) <= 512 and rup(3 * H, 32) <= 512


def gemm32_nt_name(BT, N):
    big = cdiv(BT, 128) >= 192
    _, t = gemm32_nt_shape(N, big)
    return "gemm32_nt_kernel<%dx%d>" % ((128, 64 * t) if big else (32, 32 * t))


# The exact-fp32 family's parts of a step over a layout of BT rows (api.hip fwd_front, bwd_weights, bwd_dg); g32 = g32_rows of
# THAT layout.  plan() runs all four on B*T rows; series_plan() the front end, dW_ih and dg on the series' rows and dW_hh on n*T.
def f32_front(S, H, BT, g32):
    I, G3 = 13 * S, 3 * H
    if g32:
        return ["gcn32_fwd_kernel<%d>" % gcn_nt(S), gemm32_nt_name(BT, G3)]
    sk = gemm_f32_nt_splitk(BT, G3, I) if BT < 65536 else 1
    return ["gcn32_fwd_kernel<%d>" % gcn_nt(S), gemm_f32_name(BT, G3, sk, "kk")]


def f32_dw_hh(H, BT, g32, dghn, state):
    if g32:
        return "gemm32_tn_kernel<%d>|a2=%d" % (gemm32_tn_shape(H + 1)[1], dghn)
    sk_hh = pick_splitk(BT, gemm_f32_tiles(3 * H, H + 1), 1024, 128)
    return gemm_f32_name(3 * H, H + 1, sk_hh, "tn,ones" if state else "tn,ones,shift")


def f32_dw_ih(S, H, BT, g32):
    I, G3 = 13 * S, 3 * H
    if g32:
        return "gemm32_tn_kernel<%d>|a2=0" % gemm32_tn_shape(I + 1)[1]
    return gemm_f32_name(G3, I + 1, pick_splitk(BT, gemm_f32_tiles(G3, I + 1), 1024, 128), "tn,ones")


def f32_dg(S, H, BT, g32):
    I, G3 = 13 * S, 3 * H
    if g32:
        gemm = gemm32_nt_name(BT, I)
    else:
        gemm = gemm_f32_name(BT, I, gemm_f32_nt_splitk(BT, I, G3) if BT < 65536 else 1, "kn")
    return [gemm, "gcn32_bwd_kernel<%d>|w=%d" % (gcn_nt(S), 16 if (S <= 48 and BT >= 16384) else 12)]


def plan(S, T, B, H, math, io="f32", state=False, route="train"):
    """Every key of the tabled families that one step of this call form launches, in launch order (a dense adjacency)."""
    assert refusal(S, T, B, H, math, io) is None, (S, T, B, H, math, io)
    x3f = math != "f32"                                     # the fp16-plane kernel family (Layout::x3)
    full = math in ("f16x3", "f16x3g")                      # three_pass()
    io16 = io != "f32"
    gen = H > 127 if x3f else H > 128                       # gen_gru
    BT, I, G3 = B * T, 13 * S, 3 * H
    Ip, Gp, Hp = rup(I + 1, 32), rup(G3, 32), 32 * cdiv(H + 1, 32)
    g32 = not x3f and not gen and g32_rows(BT, S, H)
    small = not x3f and not gen and B <= 768
    rec32 = not x3f and not gen and not small
    dghn = (x3f and not gen) or (rec32 and g32)
    dgi1 = math == "f16x3g" and not gen and BT >= 4096
    gen2p = math == "f16x3g" and gen and BT >= 3072
    dg16 = dgi1 or (math == "f16" and not gen)
    gi16 = math == "f16" and not gen
    stash = route != "infer"
    st = "|st=%d" % state
    iok = "|io=%d" % (16 if io16 else 32)
    mode = "" if full else ",f16"
    out = []

    def nt(M, N, Kp, alo, out16, kpart=False):
        _, t, form = pgemm_nt_shape(M, N, pgemm_nt_chunks(Kp) if kpart else 1)
        sfx = "" if (full and alo) else (",x2" if full else ",f16")
        out.append("pgemm_nt_kernel<%d%s>|out16=%d|%s" % (t, sfx, out16, form))

    # ---- forward front end
    fmode = 2 if route == "fused" else 1
    if x3f and not gen and (fmode == 2 or not stash) and gcngi_supported(S, H, full):
        planes = (2 if (full and not dgi1) else 1) if stash else 0
        out.append("gcngi_fwd_kernel<%d%s>%s|planes=%d" % (gcn_nt(S), mode, iok, planes))
    elif x3f:
        out.append("gcnx_fwd_kernel<%d%s>%s" % (gcn_nt(S), mode, iok))
        nt(BT, G3, Ip, True, gi16)
    else:
        out += f32_front(S, H, BT, g32)
    # ---- forward recurrence
    h0 = state
    if x3f and not gen:
        out.append("grux_fwd_kernel<%d%s>%s%s" % (grux_fwd_k(H), mode, iok, st))
    elif rec32:
        out.append("gru_fwd_kernel<%d>%s" % (gru_fwd_k(H), st))
    elif small:
        out.append("gru_small_fwd_kernel|hmax=%d%s" % (small_hmax(H), st))
    elif x3f:
        for t in range(T):
            if t > 0 or h0:
                nt(B, G3, Hp, True, 0, kpart=True)
    else:
        for t in range(T):
            if t > 0 or h0:
                out.append(gemm_f32_name(B, G3, 1, "kk"))
    if not stash:
        return out
    # ---- BPTT recurrence
    if x3f and gen:
        for t in range(T):
            if t > 0 or state:
                nt(B, H, Gp, True, 0, kpart=True)
    elif x3f:
        lo = "|lo=%d" % (0 if dgi1 else 1) if full else ""
        out.append("grux_bwd_kernel<%d%s>%s%s%s" % (grux_bwd_k(H), mode, iok, st, lo))
    elif gen:
        for t in range(T):
            if t > 0 or state:
                out.append(gemm_f32_name(B, H, 1, "kn"))
    elif small:
        out.append("gru_small_bwd_kernel|hmax=%d%s" % (small_hmax(H), st))
    else:
        out.append("gru_bwd_kernel<%d>%s|%s" % (gru_bwd_k(H), st, "dGHn" if dghn else "dGH"))
    # ---- the two weight-gradient products
    pw = "|pw=%d" % state
    if x3f:
        _, ti = pgemm_tn_shape(I + 1)
        _, th = pgemm_tn_shape(H + 1)
        hh_alo = not (dgi1 if dghn else gen2p)
        ih_x3 = full and not (dgi1 or gen2p)
        hh_sfx = "" if (full and hh_alo) else (",x2" if full else ",f16")
        if dghn and route != "unmerged":
            assert th <= 4 and (hh_sfx == ",x2") == (full and not ih_x3)
            out.append("pgemm_tn_kernel<%d+%d%s>%s" % (ti, th, hh_sfx, pw))
        else:
            out.append("pgemm_tn_kernel<%d%s>|a2=%d%s" % (th, hh_sfx, dghn, pw))
            out.append("pgemm_tn_kernel<%d%s>|a2=0|pw=0" % (ti, "" if ih_x3 else ",f16"))
    else:
        out.append(f32_dw_hh(H, BT, g32, dghn, state))
        out.append(f32_dw_ih(S, H, BT, g32))
    # ---- dg and the GCN backward
    if x3f:
        nt(BT, I, Gp, not (dgi1 or gen2p), dg16)
        out.append("gcnx_bwd_kernel<%d%s>%s|dg16=%d" % (gcn_nt(S), mode, iok, dg16))
    else:
        out += f32_dg(S, H, BT, g32)
    return out


NT_FAMILIES = ("pgemm_nt_kernel", "gemm32_nt_kernel")
NT_ROLES = ("GI", "rec", "bptt", "dg")
NT_BK = 32                                                  # columns of the contraction per K stage (pgemm.hip, gemm32.hip: nk = Kp / 32)


def nt_products(S, T, B, H, math, io="f32", state=False, route="train"):
    """plan()'s NT launches of the two NT GEMM families restated with their contraction: (key, role, M, N, K stages) of every
    such launch of one step, in launch order.  role: 'GI' the input projection [g | 1] [W_ih | b_ih]^T (K = Ip), 'rec' / 'bptt'
    the per-step products of the wide-GRU path (K = Hp / Gp), 'dg' = dGI W_ih (K = Gp).  Stages = padded K / 32: the trip
    count of the kernel's K loop (of one K chunk's share where launch_pgemm_nt cuts K, which no tabled case reaches).
    plan() stays the authority for names: tests/test_instance_table_host.py holds the keys of the two together."""
    assert refusal(S, T, B, H, math, io) is None, (S, T, B, H, math, io)
    x3f, full = math != "f32", math in ("f16x3", "f16x3g")
    gen = H > 127 if x3f else H > 128
    BT, I, G3 = B * T, 13 * S, 3 * H
    Ip, Gp, Hp = rup(I + 1, 32), rup(G3, 32), 32 * cdiv(H + 1, 32)
    out = []
    if not x3f:
        if not gen and g32_rows(BT, S, H):
            out.append((gemm32_nt_name(BT, G3), "GI", BT, G3, Ip // NT_BK))
            if route != "infer":
                out.append((gemm32_nt_name(BT, I), "dg", BT, I, Gp // NT_BK))
        return out
    dgi1 = math == "f16x3g" and not gen and BT >= 4096
    gen2p = math == "f16x3g" and gen and BT >= 3072
    one16 = math == "f16" and not gen                       # GI and dg as ONE fp16 plane
    stash = route != "infer"

    def nt(role, M, N, Kp, alo, out16, kpart=False):
        nch = pgemm_nt_chunks(Kp) if kpart else 1
        _, t, form = pgemm_nt_shape(M, N, nch)
        sfx = "" if (full and alo) else (",x2" if full else ",f16")
        out.append(("pgemm_nt_kernel<%d%s>|out16=%d|%s" % (t, sfx, out16, form), role, M, N, cdiv(Kp // NT_BK, nch)))

    fused = not gen and (route == "fused" or not stash) and gcngi_supported(S, H, full)
    if not fused:
        nt("GI", BT, G3, Ip, True, one16)
    steps = T if state else T - 1
    if gen:
        for _ in range(steps):
            nt("rec", B, G3, Hp, True, 0, kpart=True)
    if not stash:
        return out
    if gen:
        for _ in range(steps):
            nt("bptt", B, H, Gp, True, 0, kpart=True)
    nt("dg", BT, I, Gp, not (dgi1 or gen2p), dgi1 or one16)
    return out


def keyed_product(key, S, T, B, H, math, io="f32", state=False, route="train", role=None):
    """The product of nt_products() that carries `key`: (role, M, N, stages) of the one with the most K stages, the first in
    launch order among equals (of that role alone where one is given); None where no such NT launch of the step has the key."""
    mine = [p for p in nt_products(S, T, B, H, math, io, state, route) if p[0] == key and role in (None, p[1])]
    return max(mine, key=lambda p: p[4])[1:] if mine else None


GEMM_F32_ROLES = ("GI", "rec", "bptt", "dg", "dW_hh", "dW_ih")
GEMM_F32_NT_ROLES = GEMM_F32_ROLES[:4]
GEMM_F32_BK = 16                                            # columns of the contraction per K step (gemm.hip: BK)
GEMM_F32_FOLD = 512 // GEMM_F32_BK                          # steps after which gemm.hip folds acc into tot (since == 512 / BK)


def gemm_f32_products(S, T, B, H, math, io="f32", state=False, route="train"):
    """plan()'s gemm_f32_kernel launches restated with their contraction: (key, role, M, N, K, split, steps) of every such
    launch of one step, in launch order.  role: 'GI' = g W_ih^T (K = 13 S; the bias is added in the epilogue), 'rec' / 'bptt'
    the per-step products of the wide-GRU path (K = H / 3 H), 'dg' = dGI W_ih (K = 3 H), 'dW_hh' / 'dW_ih' the two TN products
    (K = B*T rows, cut by pick_splitk).  steps = the trip count of the kernel's K loop in its first chunk: ceil(K / split) rounded
    up to 16 columns, over 16 (launch_gemm_f32's kchunk).  Nothing for the fp16-plane modes or where gemm32.hip's products run.
    plan() stays the authority for names: tests/test_general_loops_host.py holds the keys of the two together."""
    assert refusal(S, T, B, H, math, io) is None, (S, T, B, H, math, io)
    if math != "f32":
        return []
    gen = H > 128
    BT, I, G3 = B * T, 13 * S, 3 * H
    if not gen and g32_rows(BT, S, H):
        return []
    out = []

    def prod(role, M, N, K, sk, form):
        steps = cdiv(min(K, rup(cdiv(K, sk), GEMM_F32_BK)), GEMM_F32_BK)
        out.append((gemm_f32_name(M, N, sk, form), role, M, N, K, sk, steps))

    prod("GI", BT, G3, I, gemm_f32_nt_splitk(BT, G3, I) if BT < 65536 else 1, "kk")
    steps = T if state else T - 1
    if gen:
        for _ in range(steps):
            prod("rec", B, G3, H, 1, "kk")
    if route == "infer":
        return out
    if gen:
        for _ in range(steps):
            prod("bptt", B, H, G3, 1, "kn")
    prod("dW_hh", G3, H + 1, BT, pick_splitk(BT, gemm_f32_tiles(G3, H + 1), 1024, 128), "tn,ones" if state else "tn,ones,shift")
    prod("dW_ih", G3, I + 1, BT, pick_splitk(BT, gemm_f32_tiles(G3, I + 1), 1024, 128), "tn,ones")
    prod("dg", BT, I, G3, gemm_f32_nt_splitk(BT, I, G3) if BT < 65536 else 1, "kn")
    return out


def gemm_f32_keyed(key, S, T, B, H, math, io="f32", state=False, route="train", role=None):
    """The product of gemm_f32_products() that carries `key`: (role, M, N, K, split, steps) of the one with the most steps per
    chunk, the first in launch order among equals (of that role alone where one is given); None where none has the key."""
    mine = [p for p in gemm_f32_products(S, T, B, H, math, io, state, route) if p[0] == key and role in (None, p[1])]
    return max(mine, key=lambda p: p[6])[1:] if mine else None


TN_FAMILIES = ("pgemm_tn_kernel", "pgemm_tn2_kernel", "gemm32_tn_kernel")
TN_ROLES = ("dW_ih", "dW_hh")
TN_BK = 32                                                  # rows of the contraction per K stage (pgemm.hip: nk = (kend - kbeg + 31) / 32; gemm32.hip: T_BK)
TN_BM = 320                                                 # output rows per workgroup tile (common.h TN_BM, gemm32.hip T_BM)


def pgemm_tn_tiles(Mout, Nout):
    """pgemm.hip pgemm_tn_tiles: output tiles per K chunk."""
    return cdiv(Mout, TN_BM) * pgemm_tn_shape(Nout)[0]


def gemm32_tn_tiles(Mo, No):
    """gemm32.hip gemm32_tn_tiles."""
    return cdiv(Mo, TN_BM) * gemm32_tn_shape(No)[0]


def tn_m_hh(H, x3f, dghn):
    """api.hip make_layout, L.m_hh: GEMM rows of the dW_hh product -- [dGI_r | dGI_z | pad to msplit | dGHn] where the BPTT
    kernel stores the n third of dGH alone (grux.hip / gru.hip: msplit and hn in units of 8 halfs / 4 floats), else 3 H."""
    if not dghn:
        return 3 * H
    return 8 * cdiv(2 * H, 8) + 8 * cdiv(H, 8) if x3f else 4 * cdiv(2 * H, 4) + H


def tn_kchunk(K, sk):
    """pgemm.hip launch_tn_t / launch_tn2_t, gemm32.hip launch_tn_t: rows per split-K chunk, whole stages of 32."""
    return cdiv(cdiv(K, sk), TN_BK) * TN_BK


def tn_hh_from_y(math, io, state, route):
    """api.hip hh_from_y under pgemm_tn2_covers, at the library's defaults: the merged launch of the split modes' stateless
    fp32-I/O step forms dW_hh's [Hprev | 1] rows from the caller's fp32 Y (the caller knows the launch is the merged one)."""
    return math in ("f16x3", "f16x3g") and io == "f32" and not state and route != "unmerged"


def tn_products(S, T, B, H, math, io="f32", state=False, route="train"):
    """plan()'s launches of the three TN families restated with their contraction, in launch order: one dict per product --
    a merged launch '<TI+TH..>' gives two, role dW_ih then dW_hh, under the same key.
      key, role in TN_ROLES; Mout, Nout, tiles (per K chunk); rows = B*T, the contraction;
      sk, kchunk (rows per chunk) and stages = kchunk / 32, the trip count of the K loop in a full chunk;
      chunks = the non-empty ones (the splitter rounds kchunk up, so the last of the sk may start past the rows),
      last_stages / tail = stages of the last non-empty chunk and live rows of its final stage (32: not partial);
      shift_T = T where B row k is row k - 1 of the h rows and the stored start row where k % T == 0 (0: rows as they lie),
      per_window = the start row is window k / T's own [h0 | 1];
      source = where the B operand lies: 'planes' (fp16 hi / lo planes), 'Y' (the merged launch's fp32 Y form) or 'rows'
      (gemm32.hip's fp32 operand rows: g with its ones column, the [Hprev | 1] rows the forward recurrence wrote).
    Nothing for gemm.hip's exact-fp32 products (gemm_f32_products() has those) or the inference route.
    plan() stays the authority for names: tests/test_tn_kloop_host.py holds the keys of the two together, and sk / kchunk to
    wgnn_tn_split."""
    assert refusal(S, T, B, H, math, io) is None, (S, T, B, H, math, io)
    if route == "infer":
        return []
    x3f, full = math != "f32", math in ("f16x3", "f16x3g")
    gen = H > 127 if x3f else H > 128
    BT, I, G3 = B * T, 13 * S, 3 * H
    out = []

    def prod(key, role, Mout, Nout, tiles, shift_T, pw, source):
        sk = pick_splitk(BT, tiles, 256, 64)
        kchunk = tn_kchunk(BT, sk)
        chunks = cdiv(BT, kchunk)
        last = BT - (chunks - 1) * kchunk
        out.append(dict(key=key, role=role, Mout=Mout, Nout=Nout, tiles=tiles, rows=BT, sk=sk, kchunk=kchunk,
                        stages=kchunk // TN_BK, chunks=chunks, last_stages=cdiv(last, TN_BK), tail=last - (cdiv(last, TN_BK) - 1) * TN_BK,
                        shift_T=shift_T, per_window=pw, source=source))

    if not x3f:
        if gen or not g32_rows(BT, S, H):
            return out
        dghn = B > 768                                      # rec32 && g32tn
        m_hh = tn_m_hh(H, False, dghn)
        prod(f32_dw_hh(H, BT, True, dghn, state), "dW_hh", m_hh, H + 1, gemm32_tn_tiles(m_hh, H + 1), 0, False, "rows")
        prod(f32_dw_ih(S, H, BT, True), "dW_ih", G3, I + 1, gemm32_tn_tiles(G3, I + 1), 0, False, "rows")
        return out
    dgi1 = math == "f16x3g" and not gen and BT >= 4096
    gen2p = math == "f16x3g" and gen and BT >= 3072
    dghn = not gen
    _, ti = pgemm_tn_shape(I + 1)
    _, th = pgemm_tn_shape(H + 1)
    hh_sfx = "" if (full and not (dgi1 if dghn else gen2p)) else (",x2" if full else ",f16")
    ih_sfx = "" if (full and not (dgi1 or gen2p)) else ",f16"
    m_hh = tn_m_hh(H, True, dghn)
    hh = (m_hh, H + 1, pgemm_tn_tiles(m_hh, H + 1), T, bool(state))
    ih = (G3, I + 1, pgemm_tn_tiles(G3, I + 1), 0, False)
    if dghn and route != "unmerged":                        # tn_merge, WGNN_OPT_TN_MERGED, pgemm_tn2_covers
        key = "pgemm_tn_kernel<%d+%d%s>|pw=%d" % (ti, th, hh_sfx, state)
        prod(key, "dW_ih", *ih, "planes")
        prod(key, "dW_hh", *hh, "Y" if tn_hh_from_y(math, io, state, route) else "planes")
    else:
        prod("pgemm_tn_kernel<%d%s>|a2=%d|pw=%d" % (th, hh_sfx, dghn, state), "dW_hh", *hh, "planes")
        prod("pgemm_tn_kernel<%d%s>|a2=0|pw=0" % (ti, ih_sfx), "dW_ih", *ih, "planes")
    return out


def tn_carried(key, S, T, B, H, math, io="f32", state=False, route="train"):
    """The products of tn_products() launched under `key`: one for a plain key, both roles for a merged '<TI+TH..>' key; where
    a step launches a plain key twice (the same tile count for both products), both."""
    return [p for p in tn_products(S, T, B, H, math, io, state, route) if p["key"] == key]


H_SCAN = 128                                                # past it no register-resident recurrence runs (gen_gru)


def bracket_top(key, S, T, B, math, io="f32", state=False, route="train"):
    """The largest H for which plan() of this call form contains `key` (the top of the key's width bracket), scanning H upward
    over everything the call form accepts up to H_SCAN; None where no H selects it."""
    top = None
    for H in range(1, H_SCAN + 1):
        if refusal(S, T, B, H, math, io) is None and key in plan(S, T, B, H, math, io, state, route):
            top = H
    return top


SERIES_ROUTES = ("series", "series_mse", "series_last")


def fold_terms(T, stride):
    """How many windows cover an hour away from the two ends of the series: series_fold_kernel's trip count w_lo .. w_hi."""
    if stride == 1:
        return "T"
    return "%d..%d" % (T // stride, cdiv(T, stride))


def series_plan(S, H, rows, T, stride, n, route):
    """api.hip series_forward / series_backward restated: every tabled key one series step of `route` launches, in launch order.
    Two exact-fp32 layouts (series.hip plan): the front {B = 1, T = rows} -- both graph convolutions, the input projection, dW_ih,
    dg and the GCN backward, once per hour -- and the recurrence {B = n, T} -- gru.hip's kernels and dW_hh over the n*T
    window-major rows.  Each consults gemm32's threshold with its own row count; gru_small_supported is not consulted."""
    assert route in SERIES_ROUTES and (n - 1) * stride + T <= rows and 1 <= S <= 64 and 1 <= H <= 128, (S, H, rows, T, stride, n)
    g32_f, g32_r = g32_rows(rows, S, H), g32_rows(n * T, S, H)       # Lf.g32 = Lf.g32tn; Lr.g32tn = Lr.dghn = the [Hprev | 1] rows
    out = f32_front(S, H, rows, g32_f)
    out.append("gru_fwd_kernel<%d>|series|%s" % (gru_fwd_k(H), {"series": "y", "series_mse": "loss", "series_last": "last"}[route]))
    if route == "series_last":
        return out
    out.append("gru_bwd_kernel<%d>|series|%s|%s" % (gru_bwd_k(H), "dY" if route == "series" else "mse", "dGHn" if g32_r else "dGH"))
    out.append(f32_dw_hh(H, n * T, g32_r, g32_r, False))
    out.append("series_fold_kernel|terms=%s" % fold_terms(T, stride))
    out.append(f32_dw_ih(S, H, rows, g32_f))
    return out + f32_dg(S, H, rows, g32_f)


def name_of(key):
    """The profiler name of an instance key."""
    return key.split("|", 1)[0]


def family_of(key):
    """The family of a key: its kernel name with the template arguments of pgemm_tn's two launch forms told apart."""
    base = re.match(r"[a-z0-9_]+", key).group(0)
    if base == "pgemm_tn_kernel" and "+" in name_of(key):
        return "pgemm_tn2_kernel"
    return base


# gemm.hip launch_gemm_f32 builds its name at run time ("gemm_f32_kernel<%d,%d>[%s%s%s]": tile, operand forms); by emitted name,
# the names the public dims reach (the 128-row tiles need >= 512 tiles or a split-K that the exact-fp32 products of these
# dims never get: from B*T = 4096 they are gemm32.hip's)
GEMM_F32_NAMES = ["gemm_f32_kernel<%d,%d>[%s]" % (bm, bn, f) for bm, bn in ((64, 64), (64, 128))
                  for f in ("kk", "kn", "tn,ones", "tn,ones,shift")] + [
    "gemm_f32_kernel<128,64>[kk]", "gemm_f32_kernel<128,128>[kk]", "gemm_f32_kernel<128,128>[kn]"]


# ---- the families: every instance key a launcher can emit ----------------------------------------------------------------
def _keys(fmt, *axes):
    out = [()]
    for ax in axes:
        out = [o + (a,) for o in out for a in ax]
    return [fmt % o for o in out]


_MODE = ["", ",f16"]
_IO = [32, 16]
_BIT = [0, 1]
FAMILIES = {
    # grux.hip: <K, X3, IO, ST>.  The name shows K and the one-pass mode; IO = the dtype of X; ST = a state entry point.
    "grux_fwd_kernel": _keys("grux_fwd_kernel<%d%s>|io=%d|st=%d", GRUX_FWD_K, _MODE, _IO, _BIT),
    # grux.hip: <K, X3, IO, BwdState>, and under X3 the run-time write_lo (0: dGI / dGHn as ONE plane = f16x3g at B*T >= 4096,
    # which is also when the dg GEMM's name ends in ',x2>' and the merged weight-gradient launch's does)
    "grux_bwd_kernel": _keys("grux_bwd_kernel<%d>|io=%d|st=%d|lo=%d", GRUX_BWD_K, _IO, _BIT, _BIT)
                       + _keys("grux_bwd_kernel<%d,f16>|io=%d|st=%d", GRUX_BWD_K, _IO, _BIT),
    # gru.hip: <K, ST> / <K, BwdState>; exact fp32 with B > 768.  dGHn: the n third of dGH alone is stored, which is when the
    # dW_hh product is gemm32_tn_kernel with the two-source A operand (B*T >= 4096 and S <= 39)
    "gru_fwd_kernel": _keys("gru_fwd_kernel<%d>|st=%d", GRU_FWD_KS, _BIT),
    "gru_bwd_kernel": _keys("gru_bwd_kernel<%d>|st=%d|%s", GRU_BWD_KS3, _BIT, ["dGH", "dGHn"]),
    # gru_small.hip: <HMAX, 1, KSP, ST>; exact fp32 with B <= 768.  The name shows nothing: HMAX follows from H, ST from the route
    "gru_small_fwd_kernel": _keys("gru_small_fwd_kernel|hmax=%d|st=%d", SMALL_HMAX, _BIT),
    "gru_small_bwd_kernel": _keys("gru_small_bwd_kernel|hmax=%d|st=%d", SMALL_HMAX, _BIT),
    # gcnx.hip: <NT, X3, IO> / <NT, X3, IO, D16>; dg16 = the dg GEMM wrote ONE fp16 plane (its name ends in ',x2>' or ',f16>'
    # and it ran with fp16 C: the one-pass mode with H <= 127, f16x3g at B*T >= 4096)
    "gcnx_fwd_kernel": _keys("gcnx_fwd_kernel<%d%s>|io=%d", GCNX_NT, _MODE, _IO),
    "gcnx_bwd_kernel": _keys("gcnx_bwd_kernel<%d%s>|io=%d|dg16=%d", GCNX_NT, _MODE, _IO, _BIT),
    # gcngi.hip: <NT, X3, IO, ..>; planes = the stash planes of g it writes (0 inference, 2 split modes, 1 where the backward
    # reads the hi plane only: the one-pass mode, f16x3g at B*T >= 4096)
    "gcngi_fwd_kernel": _keys("gcngi_fwd_kernel<%d%s>|io=%d|planes=%d", GCNGI_NT, _MODE, _IO, [0, 1, 2]),
    # gcn32.hip: <NT> / <NT, W>; W = 16 waves from B*T >= 16384 with S <= 48 (<4, 16> is not built: LDS)
    "gcn32_fwd_kernel": _keys("gcn32_fwd_kernel<%d>", GCN32_NT),
    "gcn32_bwd_kernel": [k for k in _keys("gcn32_bwd_kernel<%d>|w=%d", GCN32_NT, [12, 16]) if k != "gcn32_bwd_kernel<4>|w=16"],
    # pgemm.hip: <T, X3, ALO, OUT16>.  ',x2>' = X3 with a single-plane A operand; out16 = fp16 C (GI in the one-pass mode, dg16);
    # wide / narrow = nt_shape's two tilings of N (the same instance run with few or many N slices)
    # (<T, true, true, true> does not exist: launch_nt_t refuses fp16 C with a two-plane A operand)
    "pgemm_nt_kernel": _keys("pgemm_nt_kernel<%d>|out16=0|%s", PGEMM_NT_T, ["wide", "narrow"])
                       + _keys("pgemm_nt_kernel<%d%s>|out16=%d|%s", PGEMM_NT_T, [",x2", ",f16"], _BIT, ["wide", "narrow"]),
    # pgemm.hip: <T, X3, A2, ALO, PW>: a2 = the two-source A operand (dW_hh behind the register-resident recurrence, T <= 4),
    # pw = per-window [h0 | 1] rows (dW_hh of a state entry point)
    "pgemm_tn_kernel": _keys("pgemm_tn_kernel<%d%s>|a2=0|pw=%d", PGEMM_TN_T, ["", ",x2", ",f16"], _BIT)
                       + _keys("pgemm_tn_kernel<%d%s>|a2=1|pw=%d", TN2_TH, ["", ",x2", ",f16"], _BIT),
    # pgemm.hip pgemm_tn2_kernel<TI, TH, MODE, PW>, named pgemm_tn_kernel<TI+TH..>: MODE 0 '' / 1 ',x2' / 2 ',f16'
    "pgemm_tn2_kernel": _keys("pgemm_tn_kernel<%d+%d%s>|pw=%d", TN2_TI, TN2_TH, ["", ",x2", ",f16"], _BIT),
    # gemm32.hip: <MW, NW, T32> named by its tile, <T16> with a2 = the two-source A operand (dGHn)
    "gemm32_nt_kernel": ["gemm32_nt_kernel<128x%d>" % (64 * t) for t in GEMM32_NT_BIG_T]
                        + ["gemm32_nt_kernel<32x%d>" % (32 * t) for t in GEMM32_NT_SMALL_T],
    "gemm32_tn_kernel": _keys("gemm32_tn_kernel<%d>|a2=%d", GEMM32_TN_T, _BIT),
    # gemm.hip: <bm / 64, bn / 64> and the operand forms of the name
    "gemm_f32_kernel": GEMM_F32_NAMES,
}

# The series entry points (include/windgnn_series.h, windgnn_series_train.h).  Their recurrences are further instances of
# gru.hip's two templates with the SAME profiler names as the window-major ones (FCASE / BCASE print K alone): the entry point
# fixes the SeriesRows argument -- every wgnn_series_* call passes a non-zero stride, no other call does -- and the call form the
# run-time paths behind it, so a name launched by a series route IS the series instance.
SERIES_FAMILIES = {
    # gru.hip gru_fwd_kernel<K, false, SeriesRows>: GI (and the labels) read at series rows w*stride + t.  y: wgnn_series_fwd
    # (Y and the gate records); loss: wgnn_series_fwd_loss (+ the label series and the statistics pair per workgroup);
    # last: wgnn_series_fwd_last (last_only: no Y, no records, the de-normalised last row).  The [Hprev | 1] rows are written
    # by y / loss when n*T >= 4096, which is when the BPTT kernel's key says dGHn
    "gru_fwd_kernel": _keys("gru_fwd_kernel<%d>|series|%s", GRU_FWD_KS, ["y", "loss", "last"]),
    # gru.hip gru_bwd_kernel<K3, SeriesRows>: dY: wgnn_series_bwd; mse: wgnn_series_bwd_mse (dY formed from Y and the label
    # series, the loss finalised); dGHn: the n third of dGH alone (n*T >= 4096 and S <= 39, dW_hh by gemm32_tn_kernel's
    # two-source form), dGH: all of it (dW_hh by gemm_f32_kernel[tn,ones,shift])
    "gru_bwd_kernel": _keys("gru_bwd_kernel<%d>|series|%s|%s", GRU_BWD_KS3, ["dY", "mse"], ["dGH", "dGHn"]),
    # series.hip: one kernel; terms = how many windows cover an interior hour (the loop's trip count): 0..1 with stride > T
    # (uncovered hours come out as zero rows), 1..2 with T = 3 at stride 2, T at stride 1
    "series_fold_kernel": ["series_fold_kernel|terms=%s" % t for t in ("0..1", "1..2", "T")],
}

# pgemm_tn2_kernel: 7 x 4 pairs per mode and per-window form; required: every TI and every TH at least once per mode and
# per-window form, with TI > TH and TI < TH both among them
TN2_PAIRS = [(1, 2), (2, 1), (3, 4), (4, 3), (5, 1), (6, 2), (7, 3)]
TN2_REQUIRED = ["pgemm_tn_kernel<%d+%d%s>|pw=%d" % (ti, th, m, pw) for (ti, th) in TN2_PAIRS for m in ("", ",x2", ",f16")
                for pw in _BIT]


# ---- what the public entry points can never select: key -> (why, the line of csrc/api.hip that excludes it and a word of it)
UNREACHABLE = {}


def _never(keys, why, line, word):
    for k in keys:
        assert k not in UNREACHABLE
        UNREACHABLE[k] = (why, line, word)


_never(_keys("gcnx_bwd_kernel<%d,f16>|io=16|dg16=0", GCNX_NT),
       "the one-pass mode has fp32 dg only behind the wide-GRU path (H > 127), where 16-bit I/O is refused", 163, "L.dg16 =")
_never(_keys("gcngi_fwd_kernel<%d,f16>|io=%d|planes=2", GCNGI_NT, _IO),
       "the lo plane of g is stashed for the three-pass modes only", 474, "const int planes =")
_never(_keys("pgemm_nt_kernel<%d%s>|out16=0|narrow", [11, 12, 13, 14], ["", ",f16"])
       + _keys("pgemm_nt_kernel<%d,x2>|out16=0|narrow", [10, 11, 12, 13, 14])
       + _keys("pgemm_nt_kernel<%d%s>|out16=1|narrow", [10, 11, 12, 13, 14], [",x2", ",f16"]),
       "nt_shape cuts N finer only below 192 workgroups, where N / (256 / ceil(M / 192)) stays within 10 tiles of 32 columns; "
       "the products with fp16 C or a single-plane A have N <= 13 S <= 832, which makes at most 9", 399, "d->S > 64")
_never(_keys("pgemm_tn_kernel<%d%s>|a2=0|pw=1", [1, 2, 3], ["", ",x2", ",f16"]) + _keys("pgemm_tn_kernel<%d,x2>|a2=0|pw=0", [1, 2, 3]),
       "a per-window or single-plane product without the two-source A operand is dW_hh of the wide-GRU path: H + 1 >= 129 "
       "columns, tiles of 4 to 7", 773, "hh.Ahi = dGHh")
_never(_keys("gemm32_tn_kernel<%d>|a2=1", [6, 7]),
       "the two-source A operand is dW_hh's: H + 1 <= 129 columns, tiles of at most 5", 803, "launch_gemm32_tn(b.dGI")

# Reachable, but only on the wide-GRU path at dims whose fp64 reference takes far longer than a test may: key -> dims
# (S, T, B, H, math).  plan() confirms the dims; no GPU case.
BEYOND_BUDGET = {
    "pgemm_nt_kernel<10>|out16=0|narrow": (1, 2, 4801, 961, "f16x3"),
    "pgemm_nt_kernel<10,f16>|out16=0|narrow": (1, 2, 4801, 961, "f16"),
}

# The model of a case is orc.init_params(S, 13, H, seed = S + H), except where that draw saturates the GRU (|Y| reaches 1.00,
# max |dW_hh| ~ 1e-5): there the reference's own fp32 CPU evaluation is off its fp64 one by more than any healthy draw's 5e-7
# relative to max -- S = 23, H = 4: 1.1e-4 on dW_hh, above the suite's bar by itself; S = 25, H = 4: 4.7e-6 -- and the seed
# is S + H + 1000 (2.7e-7 and 2.3e-7).  Measured on the reference alone, over every (S, H) of CASES.
# The edge half (EDGE_CASES) adds two entries, for another reason: at S = 1, H = 104 the default draw (seed 105) leaves hidden
# column 103 almost unused at B = 833 -- dropping it from the W_hh product moves Y by 5.1e-4, short of the 1e-3 the host test
# requires of each planted mistake -- and seed 1105 gives, at B = 833 / 17 / 769: wrong-parity h 9.9e-3 / 2.6e-2 / 2.2e-1,
# dropped column 3.9e-3 / 1.2e-2 / 4.0e-2, GI one step early 2.5e-2 / 1.7e-1 / 1.0 (fp32 against fp64 <= 3.0e-7).
# And (1, 84): 3085 -- at (1, 5, 65, 84), where grux_bwd_kernel<8,f16>|io=16|st=1 runs (EDGE_B_MOVED), GI one step early moves Y
# by 9.1e-4 with seed 85; with 3085, at B = 65 / 17 / 833: wrong-parity h 7.6e-3 / 9.3e-2 / 9.7e-3, dropped column 4.9e-3 /
# 2.1e-2 / 6.1e-3, GI one step early 2.2e-3 / 4.8e-1 / 5.5e-2 (fp32 against fp64 <= 5.8e-7).
PARAM_SEED = {(23, 4): 1027, (25, 4): 1029, (1, 104): 1105, (1, 84): 3085}


def param_seed(S, H):
    return PARAM_SEED.get((S, H), S + H)


# One-pass fp16 cases above F16_G_TOL, pinned as tests/test_gpu_parity.py's F16_SWEEP_EXCEPTIONS are: (key, tensor) ->
# measured value x 1.1, the measurement and the same shape's f16x3 error next to it
F16_EXCEPTIONS = {
    # S = 20, T = 3, B = 8161, H = 4 (B*T is above the 4096 cap of growing B): measured 6.23e-2; f16x3 at the same shape 2.73e-5
    ("pgemm_nt_kernel<5,f16>|out16=1|narrow", "gru.weight_hh_l0"): 6.9e-2,
    # S = 60, T = 3, B = 5473, H = 4: Y against F16_Y_TOL = 2e-2, measured 2.15e-2; f16x3 at the same shape 1.88e-5
    ("pgemm_nt_kernel<9,f16>|out16=1|narrow", "Y"): 2.4e-2,
}
# Five one-pass fp16 cases at S = 1, T = 2 run B = 33, not 17: at B = 17 a conv gradient measured 5.2e-2 ... 1.9e-1 of max
# (grux_fwd_kernel<3,f16>|io=16 st 0 / 1: 5.2e-2 / 9.3e-2; grux_bwd_kernel<7,f16>|io=16|st=1: 1.9e-1; grux_bwd_kernel<12,f16>|
# io=16|st=0: 7.4e-2; pgemm_tn_kernel<4,f16>|a2=0|pw=1: 1.9e-1) with f16x3 at 5e-7 ... 6e-6 on the same inputs -- rounding of
# 34 rows, not indexing -- and at B = 33 all five are below 1e-3

# (family, key, S, T, B, H, math, io, state, route)
# B*T thresholds: 2 x 2049 = 4098 >= 4096 (gemm32, dGHn, f16x3g's single plane); 3 x 1025 = 3075 >= 3072 (the wide-GRU path's);
# 3 x 5473 = 16 419 >= 16 384 (gcn32_bwd's 16 waves); 3 x 8161 = 24 483 >= 24 449 (gemm32_nt's 128-row tiles) and >= 18 241
# (wide pgemm_nt tiles over two N slices); 24 x 1537 = 36 888 >= 36 673 (wide pgemm_nt tiles over one N slice);
# B = 769: the first batch of gru.hip's recurrences.  The four per-window ',x2>' products of the wide-GRU path (f16x3g's single
# plane there starts at B*T = 3072) sit at 4098: the 1e-3 bar of single-plane state cases starts at 4096, and at 3 x 1025 they
# measured 1.3e-4 ... 4.9e-4 on conv1.weight (1.6e-4 ... 2.5e-4 is what the register-resident path's state cases show at 4098)
CASES = [
    # ---- grux_fwd_kernel
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=32|st=0", 1, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=32|st=1", 1, 2, 17, 4, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=16|st=0", 1, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=16|st=1", 1, 2, 17, 4, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=32|st=0", 1, 2, 17, 4, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=32|st=1", 1, 2, 17, 4, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=16|st=0", 1, 2, 17, 4, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=16|st=1", 1, 2, 17, 4, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=32|st=0", 1, 2, 17, 32, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=32|st=1", 1, 2, 17, 32, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=16|st=0", 1, 2, 17, 32, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=16|st=1", 1, 2, 17, 32, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=32|st=0", 1, 2, 17, 32, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=32|st=1", 1, 2, 17, 32, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=16|st=0", 1, 2, 17, 32, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=16|st=1", 1, 2, 17, 32, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=32|st=0", 1, 2, 17, 64, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=32|st=1", 1, 2, 17, 64, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=16|st=0", 1, 2, 17, 64, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=16|st=1", 1, 2, 17, 64, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=32|st=0", 1, 2, 17, 64, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=32|st=1", 1, 2, 17, 64, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=16|st=0", 1, 2, 33, 64, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=16|st=1", 1, 2, 33, 64, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=32|st=0", 1, 2, 17, 96, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=32|st=1", 1, 2, 17, 96, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=16|st=0", 1, 2, 17, 96, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=16|st=1", 1, 2, 17, 96, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=32|st=0", 1, 2, 17, 96, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=32|st=1", 1, 2, 17, 96, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=16|st=0", 1, 2, 17, 96, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=16|st=1", 1, 2, 17, 96, "f16", "bf16", True, "train"),
    # ---- grux_bwd_kernel
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=0|lo=0", 1, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=0|lo=1", 1, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=1|lo=0", 1, 2, 2049, 4, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=1|lo=1", 1, 2, 17, 4, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=0|lo=0", 1, 2, 2049, 4, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=0|lo=1", 1, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=1|lo=0", 1, 2, 2049, 4, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=1|lo=1", 1, 2, 17, 4, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=0|lo=0", 1, 2, 2049, 9, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=0|lo=1", 1, 2, 17, 9, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=1|lo=0", 1, 2, 2049, 9, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=1|lo=1", 1, 2, 17, 9, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=0|lo=0", 1, 2, 2049, 9, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=0|lo=1", 1, 2, 17, 9, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=1|lo=0", 1, 2, 2049, 9, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=1|lo=1", 1, 2, 17, 9, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=0|lo=0", 1, 2, 2049, 21, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=0|lo=1", 1, 2, 17, 21, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=1|lo=0", 1, 2, 2049, 21, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=1|lo=1", 1, 2, 17, 21, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=0|lo=0", 1, 2, 2049, 21, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=0|lo=1", 1, 2, 17, 21, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=1|lo=0", 1, 2, 2049, 21, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=1|lo=1", 1, 2, 17, 21, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=0|lo=0", 1, 2, 2049, 33, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=0|lo=1", 1, 2, 17, 33, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=1|lo=0", 1, 2, 2049, 33, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=1|lo=1", 1, 2, 17, 33, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=0|lo=0", 1, 2, 2049, 33, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=0|lo=1", 1, 2, 17, 33, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=1|lo=0", 1, 2, 2049, 33, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=1|lo=1", 1, 2, 17, 33, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=0|lo=0", 1, 2, 2049, 41, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=0|lo=1", 1, 2, 17, 41, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=1|lo=0", 1, 2, 2049, 41, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=1|lo=1", 1, 2, 17, 41, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=0|lo=0", 1, 2, 2049, 41, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=0|lo=1", 1, 2, 17, 41, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=1|lo=0", 1, 2, 2049, 41, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=1|lo=1", 1, 2, 17, 41, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=0|lo=0", 1, 2, 2049, 53, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=0|lo=1", 1, 2, 17, 53, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=1|lo=0", 1, 2, 2049, 53, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=1|lo=1", 1, 2, 17, 53, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=0|lo=0", 1, 2, 2049, 53, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=0|lo=1", 1, 2, 17, 53, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=1|lo=0", 1, 2, 2049, 53, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=1|lo=1", 1, 2, 17, 53, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=0|lo=0", 1, 2, 2049, 65, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=0|lo=1", 1, 2, 17, 65, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=1|lo=0", 1, 2, 2049, 65, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=1|lo=1", 1, 2, 17, 65, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=0|lo=0", 1, 2, 2049, 65, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=0|lo=1", 1, 2, 17, 65, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=1|lo=0", 1, 2, 2049, 65, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=1|lo=1", 1, 2, 17, 65, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=0|lo=0", 1, 2, 2049, 73, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=0|lo=1", 1, 2, 17, 73, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=1|lo=0", 1, 2, 2049, 73, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=1|lo=1", 1, 2, 17, 73, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=0|lo=0", 1, 2, 2049, 73, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=0|lo=1", 1, 2, 17, 73, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=1|lo=0", 1, 2, 2049, 73, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=1|lo=1", 1, 2, 17, 73, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=0|lo=0", 1, 2, 2049, 85, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=0|lo=1", 1, 2, 17, 85, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=1|lo=0", 1, 2, 2049, 85, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=1|lo=1", 1, 2, 17, 85, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=0|lo=0", 1, 2, 2049, 85, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=0|lo=1", 1, 2, 17, 85, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=1|lo=0", 1, 2, 2049, 85, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=1|lo=1", 1, 2, 17, 85, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=0|lo=0", 1, 2, 2049, 97, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=0|lo=1", 1, 2, 17, 97, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=1|lo=0", 1, 2, 2049, 97, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=1|lo=1", 1, 2, 17, 97, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=0|lo=0", 1, 2, 2049, 97, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=0|lo=1", 1, 2, 17, 97, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=1|lo=0", 1, 2, 2049, 97, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=1|lo=1", 1, 2, 17, 97, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=0|lo=0", 1, 2, 2049, 105, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=0|lo=1", 1, 2, 17, 105, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=1|lo=0", 1, 2, 2049, 105, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=1|lo=1", 1, 2, 17, 105, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=0|lo=0", 1, 2, 2049, 105, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=0|lo=1", 1, 2, 17, 105, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=1|lo=0", 1, 2, 2049, 105, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=1|lo=1", 1, 2, 17, 105, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=0|lo=0", 1, 2, 2049, 117, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=0|lo=1", 1, 2, 17, 117, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=1|lo=0", 1, 2, 2049, 117, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=1|lo=1", 1, 2, 17, 117, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=0|lo=0", 1, 2, 2049, 117, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=0|lo=1", 1, 2, 17, 117, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=1|lo=0", 1, 2, 2049, 117, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=1|lo=1", 1, 2, 17, 117, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=32|st=0", 1, 2, 17, 4, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=32|st=1", 1, 2, 17, 4, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=16|st=0", 1, 2, 17, 4, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=16|st=1", 1, 2, 17, 4, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=32|st=0", 1, 2, 17, 9, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=32|st=1", 1, 2, 17, 9, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=16|st=0", 1, 2, 17, 9, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=16|st=1", 1, 2, 17, 9, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=32|st=0", 1, 2, 17, 21, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=32|st=1", 1, 2, 17, 21, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=16|st=0", 1, 2, 17, 21, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=16|st=1", 1, 2, 17, 21, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=32|st=0", 1, 2, 17, 33, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=32|st=1", 1, 2, 17, 33, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=16|st=0", 1, 2, 17, 33, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=16|st=1", 1, 2, 17, 33, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=32|st=0", 1, 2, 17, 41, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=32|st=1", 1, 2, 17, 41, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=16|st=0", 1, 2, 17, 41, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=16|st=1", 1, 2, 17, 41, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=32|st=0", 1, 2, 17, 53, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=32|st=1", 1, 2, 17, 53, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=16|st=0", 1, 2, 17, 53, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=16|st=1", 1, 2, 17, 53, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=32|st=0", 1, 2, 17, 65, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=32|st=1", 1, 2, 17, 65, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=16|st=0", 1, 2, 17, 65, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=16|st=1", 1, 2, 33, 65, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=32|st=0", 1, 2, 17, 73, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=32|st=1", 1, 2, 17, 73, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=16|st=0", 1, 2, 17, 73, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=16|st=1", 1, 2, 17, 73, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=32|st=0", 1, 2, 17, 85, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=32|st=1", 1, 2, 17, 85, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=16|st=0", 1, 2, 17, 85, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=16|st=1", 1, 2, 17, 85, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=32|st=0", 1, 2, 17, 97, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=32|st=1", 1, 2, 17, 97, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=16|st=0", 1, 2, 17, 97, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=16|st=1", 1, 2, 17, 97, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=32|st=0", 1, 2, 17, 105, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=32|st=1", 1, 2, 17, 105, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=16|st=0", 1, 2, 17, 105, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=16|st=1", 1, 2, 17, 105, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=32|st=0", 1, 2, 17, 117, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=32|st=1", 1, 2, 17, 117, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=16|st=0", 1, 2, 33, 117, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=16|st=1", 1, 2, 17, 117, "f16", "bf16", True, "train"),
    # ---- gru_fwd_kernel
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|st=0", 1, 2, 769, 4, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|st=1", 1, 2, 769, 4, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|st=0", 1, 2, 769, 17, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|st=1", 1, 2, 769, 17, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|st=0", 1, 2, 769, 33, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|st=1", 1, 2, 769, 33, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|st=0", 1, 2, 769, 49, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|st=1", 1, 2, 769, 49, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|st=0", 1, 2, 769, 65, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|st=1", 1, 2, 769, 65, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|st=0", 1, 2, 769, 81, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|st=1", 1, 2, 769, 81, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|st=0", 1, 2, 769, 97, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|st=1", 1, 2, 769, 97, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|st=0", 1, 2, 769, 105, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|st=1", 1, 2, 769, 105, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|st=0", 1, 2, 769, 113, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|st=1", 1, 2, 769, 113, "f32", "f32", True, "train"),
    # ---- gru_bwd_kernel
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=0|dGH", 1, 2, 769, 4, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=0|dGHn", 1, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=1|dGH", 1, 2, 769, 4, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=1|dGHn", 1, 2, 2049, 4, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=0|dGH", 1, 2, 769, 17, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=0|dGHn", 1, 2, 2049, 17, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=1|dGH", 1, 2, 769, 17, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=1|dGHn", 1, 2, 2049, 17, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=0|dGH", 1, 2, 769, 33, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=0|dGHn", 1, 2, 2049, 33, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=1|dGH", 1, 2, 769, 33, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=1|dGHn", 1, 2, 2049, 33, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=0|dGH", 1, 2, 769, 49, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=0|dGHn", 1, 2, 2049, 49, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=1|dGH", 1, 2, 769, 49, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=1|dGHn", 1, 2, 2049, 49, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=0|dGH", 1, 2, 769, 65, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=0|dGHn", 1, 2, 2049, 65, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=1|dGH", 1, 2, 769, 65, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=1|dGHn", 1, 2, 2049, 65, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=0|dGH", 1, 2, 769, 81, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=0|dGHn", 1, 2, 2049, 81, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=1|dGH", 1, 2, 769, 81, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=1|dGHn", 1, 2, 2049, 81, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=0|dGH", 1, 2, 769, 97, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=0|dGHn", 1, 2, 2049, 97, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=1|dGH", 1, 2, 769, 97, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=1|dGHn", 1, 2, 2049, 97, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=0|dGH", 1, 2, 769, 105, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=0|dGHn", 1, 2, 2049, 105, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=1|dGH", 1, 2, 769, 105, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=1|dGHn", 1, 2, 2049, 105, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=0|dGH", 1, 2, 769, 113, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=0|dGHn", 1, 2, 2049, 113, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=1|dGH", 1, 2, 769, 113, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=1|dGHn", 1, 2, 2049, 113, "f32", "f32", True, "train"),
    # ---- gru_small_fwd_kernel
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=32|st=0", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=32|st=1", 1, 2, 17, 4, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=64|st=0", 1, 2, 17, 33, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=64|st=1", 1, 2, 17, 33, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=96|st=0", 1, 2, 17, 65, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=96|st=1", 1, 2, 17, 65, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=108|st=0", 1, 2, 17, 97, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=108|st=1", 1, 2, 17, 97, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=112|st=0", 1, 2, 17, 107, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=112|st=1", 1, 2, 17, 107, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=128|st=0", 1, 2, 17, 113, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=128|st=1", 1, 2, 17, 113, "f32", "f32", True, "train"),
    # ---- gru_small_bwd_kernel
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=32|st=0", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=32|st=1", 1, 2, 17, 4, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=64|st=0", 1, 2, 17, 33, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=64|st=1", 1, 2, 17, 33, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=96|st=0", 1, 2, 17, 65, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=96|st=1", 1, 2, 17, 65, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=108|st=0", 1, 2, 17, 97, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=108|st=1", 1, 2, 17, 97, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=112|st=0", 1, 2, 17, 107, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=112|st=1", 1, 2, 17, 107, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=128|st=0", 1, 2, 17, 113, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=128|st=1", 1, 2, 17, 113, "f32", "f32", True, "train"),
    # ---- gcnx_fwd_kernel
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<1>|io=32", 1, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<1>|io=16", 1, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<1,f16>|io=32", 1, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<1,f16>|io=16", 1, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<2>|io=32", 17, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<2>|io=16", 17, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<2,f16>|io=32", 17, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<2,f16>|io=16", 17, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<3>|io=32", 33, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<3>|io=16", 33, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<3,f16>|io=32", 33, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<3,f16>|io=16", 33, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<4>|io=32", 49, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<4>|io=16", 49, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<4,f16>|io=32", 49, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_fwd_kernel", "gcnx_fwd_kernel<4,f16>|io=16", 49, 2, 17, 4, "f16", "bf16", False, "train"),
    # ---- gcnx_bwd_kernel
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1>|io=32|dg16=0", 1, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1>|io=32|dg16=1", 1, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1>|io=16|dg16=0", 1, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1>|io=16|dg16=1", 1, 2, 2049, 4, "f16x3g", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1,f16>|io=32|dg16=0", 1, 2, 17, 128, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1,f16>|io=32|dg16=1", 1, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<1,f16>|io=16|dg16=1", 1, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2>|io=32|dg16=0", 17, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2>|io=32|dg16=1", 17, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2>|io=16|dg16=0", 17, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2>|io=16|dg16=1", 17, 2, 2049, 4, "f16x3g", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2,f16>|io=32|dg16=0", 17, 2, 17, 128, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2,f16>|io=32|dg16=1", 17, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<2,f16>|io=16|dg16=1", 17, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3>|io=32|dg16=0", 33, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3>|io=32|dg16=1", 33, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3>|io=16|dg16=0", 33, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3>|io=16|dg16=1", 33, 2, 2049, 4, "f16x3g", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3,f16>|io=32|dg16=0", 33, 2, 17, 128, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3,f16>|io=32|dg16=1", 33, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<3,f16>|io=16|dg16=1", 33, 2, 17, 4, "f16", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4>|io=32|dg16=0", 49, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4>|io=32|dg16=1", 49, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4>|io=16|dg16=0", 49, 2, 17, 4, "f16x3", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4>|io=16|dg16=1", 49, 2, 2049, 4, "f16x3g", "bf16", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4,f16>|io=32|dg16=0", 49, 2, 17, 128, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4,f16>|io=32|dg16=1", 49, 2, 17, 4, "f16", "f32", False, "train"),
    ("gcnx_bwd_kernel", "gcnx_bwd_kernel<4,f16>|io=16|dg16=1", 49, 2, 17, 4, "f16", "bf16", False, "train"),
    # ---- gcngi_fwd_kernel
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=32|planes=0", 1, 2, 17, 4, "f16x3", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=32|planes=1", 1, 2, 2049, 4, "f16x3g", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=32|planes=2", 1, 2, 17, 4, "f16x3", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=16|planes=0", 1, 2, 17, 4, "f16x3", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=16|planes=1", 1, 2, 2049, 4, "f16x3g", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1>|io=16|planes=2", 1, 2, 17, 4, "f16x3", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1,f16>|io=32|planes=0", 1, 2, 17, 4, "f16", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1,f16>|io=32|planes=1", 1, 2, 17, 4, "f16", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1,f16>|io=16|planes=0", 1, 2, 17, 4, "f16", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<1,f16>|io=16|planes=1", 1, 2, 17, 4, "f16", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=32|planes=0", 17, 2, 17, 4, "f16x3", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=32|planes=1", 17, 2, 2049, 4, "f16x3g", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=32|planes=2", 17, 2, 17, 4, "f16x3", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=16|planes=0", 17, 2, 17, 4, "f16x3", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=16|planes=1", 17, 2, 2049, 4, "f16x3g", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2>|io=16|planes=2", 17, 2, 17, 4, "f16x3", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2,f16>|io=32|planes=0", 17, 2, 17, 4, "f16", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2,f16>|io=32|planes=1", 17, 2, 17, 4, "f16", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2,f16>|io=16|planes=0", 17, 2, 17, 4, "f16", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<2,f16>|io=16|planes=1", 17, 2, 17, 4, "f16", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=32|planes=0", 33, 2, 17, 4, "f16x3", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=32|planes=1", 33, 2, 2049, 4, "f16x3g", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=32|planes=2", 33, 2, 17, 4, "f16x3", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=16|planes=0", 33, 2, 17, 4, "f16x3", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=16|planes=1", 33, 2, 2049, 4, "f16x3g", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3>|io=16|planes=2", 33, 2, 17, 4, "f16x3", "bf16", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3,f16>|io=32|planes=0", 33, 2, 17, 4, "f16", "f32", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3,f16>|io=32|planes=1", 33, 2, 17, 4, "f16", "f32", False, "fused"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3,f16>|io=16|planes=0", 33, 2, 17, 4, "f16", "bf16", False, "infer"),
    ("gcngi_fwd_kernel", "gcngi_fwd_kernel<3,f16>|io=16|planes=1", 33, 2, 17, 4, "f16", "bf16", False, "fused"),
    # ---- gcn32_fwd_kernel
    ("gcn32_fwd_kernel", "gcn32_fwd_kernel<1>", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_fwd_kernel", "gcn32_fwd_kernel<2>", 17, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_fwd_kernel", "gcn32_fwd_kernel<3>", 33, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_fwd_kernel", "gcn32_fwd_kernel<4>", 49, 2, 17, 4, "f32", "f32", False, "train"),
    # ---- gcn32_bwd_kernel
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<1>|w=12", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<1>|w=16", 1, 3, 5473, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<2>|w=12", 17, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<2>|w=16", 17, 3, 5473, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<3>|w=12", 33, 2, 17, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<3>|w=16", 33, 3, 5473, 4, "f32", "f32", False, "train"),
    ("gcn32_bwd_kernel", "gcn32_bwd_kernel<4>|w=12", 49, 2, 17, 4, "f32", "f32", False, "train"),
    # ---- pgemm_nt_kernel
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1>|out16=0|wide", 1, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1>|out16=0|narrow", 1, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2>|out16=0|wide", 3, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2>|out16=0|narrow", 5, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3>|out16=0|wide", 5, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3>|out16=0|narrow", 10, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4>|out16=0|wide", 8, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4>|out16=0|narrow", 15, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5>|out16=0|wide", 10, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5>|out16=0|narrow", 20, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6>|out16=0|wide", 13, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6>|out16=0|narrow", 25, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7>|out16=0|wide", 15, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7>|out16=0|narrow", 30, 3, 8161, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8>|out16=0|wide", 18, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8>|out16=0|narrow", 52, 3, 5473, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9>|out16=0|wide", 20, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9>|out16=0|narrow", 60, 3, 5473, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10>|out16=0|wide", 23, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11>|out16=0|wide", 25, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12>|out16=0|wide", 28, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13>|out16=0|wide", 30, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14>|out16=0|wide", 33, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=0|wide", 1, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=0|narrow", 1, 3, 1025, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=1|wide", 1, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=1|narrow", 1, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=0|wide", 1, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=0|narrow", 1, 2, 17, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=1|wide", 1, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=1|narrow", 1, 2, 17, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=0|wide", 3, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=0|narrow", 30, 2, 2049, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=1|wide", 3, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=1|narrow", 5, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=0|wide", 3, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=0|narrow", 1, 2, 2049, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=1|wide", 3, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=1|narrow", 5, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=0|wide", 5, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=0|narrow", 60, 2, 2049, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=1|wide", 5, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=1|narrow", 10, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=0|wide", 5, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=0|narrow", 1, 2, 3073, 192, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=1|wide", 5, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=1|narrow", 10, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=0|wide", 8, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=0|narrow", 60, 2, 3073, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=1|wide", 8, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=1|narrow", 15, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=0|wide", 8, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=0|narrow", 1, 3, 5473, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=1|wide", 8, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=1|narrow", 15, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=0|wide", 10, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=0|narrow", 30, 3, 5473, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=1|wide", 10, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=1|narrow", 20, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=0|wide", 10, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=0|narrow", 1, 3, 5473, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=1|wide", 10, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=1|narrow", 20, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=0|wide", 13, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=0|narrow", 39, 3, 5473, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=1|wide", 13, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=1|narrow", 25, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=0|wide", 13, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=0|narrow", 1, 3, 8161, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=1|wide", 13, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=1|narrow", 25, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=0|wide", 15, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=0|narrow", 45, 3, 5473, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=1|wide", 15, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=1|narrow", 30, 3, 8161, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=0|wide", 15, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=0|narrow", 1, 3, 8161, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=1|wide", 15, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=1|narrow", 30, 3, 8161, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=0|wide", 35, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=0|narrow", 52, 3, 5473, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=1|wide", 18, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=1|narrow", 52, 3, 5473, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=0|wide", 1, 3, 8161, 160, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=0|narrow", 1, 3, 5473, 225, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=1|wide", 18, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=1|narrow", 52, 3, 5473, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=0|wide", 40, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=0|narrow", 60, 3, 5473, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=1|wide", 20, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=1|narrow", 60, 3, 5473, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=0|wide", 1, 3, 8161, 192, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=0|narrow", 60, 3, 5473, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=1|wide", 20, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=1|narrow", 60, 3, 5473, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,x2>|out16=0|wide", 45, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,x2>|out16=1|wide", 23, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,f16>|out16=0|wide", 1, 3, 8161, 193, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,f16>|out16=1|wide", 23, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,x2>|out16=0|wide", 52, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,x2>|out16=1|wide", 25, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,f16>|out16=0|wide", 1, 3, 8161, 224, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,f16>|out16=1|wide", 25, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,x2>|out16=0|wide", 56, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,x2>|out16=1|wide", 28, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,f16>|out16=0|wide", 1, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,f16>|out16=1|wide", 28, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,x2>|out16=0|wide", 60, 3, 8161, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,x2>|out16=1|wide", 30, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,f16>|out16=0|wide", 1, 24, 1537, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,f16>|out16=1|wide", 30, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,x2>|out16=0|wide", 33, 24, 1537, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,x2>|out16=1|wide", 33, 24, 1537, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,f16>|out16=0|wide", 33, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,f16>|out16=1|wide", 33, 24, 1537, 4, "f16", "f32", False, "train"),
    # ---- pgemm_tn_kernel
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1>|a2=0|pw=0", 1, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,f16>|a2=0|pw=0", 1, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=0|pw=0", 3, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=0|pw=0", 3, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=0|pw=0", 5, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=0|pw=0", 5, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=0|pw=0", 8, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=0|pw=1", 1, 2, 17, 224, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=0|pw=0", 1, 3, 1025, 224, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=0|pw=1", 1, 2, 2049, 224, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=0|pw=0", 8, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=0|pw=1", 1, 2, 33, 224, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5>|a2=0|pw=0", 10, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5>|a2=0|pw=1", 1, 2, 17, 128, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,x2>|a2=0|pw=0", 1, 3, 1025, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,x2>|a2=0|pw=1", 1, 2, 2049, 128, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,f16>|a2=0|pw=0", 10, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,f16>|a2=0|pw=1", 1, 2, 17, 128, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6>|a2=0|pw=0", 13, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6>|a2=0|pw=1", 1, 2, 17, 160, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,x2>|a2=0|pw=0", 1, 3, 1025, 160, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,x2>|a2=0|pw=1", 1, 2, 2049, 160, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,f16>|a2=0|pw=0", 13, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,f16>|a2=0|pw=1", 1, 2, 17, 160, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7>|a2=0|pw=0", 15, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7>|a2=0|pw=1", 1, 2, 17, 192, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,x2>|a2=0|pw=0", 1, 3, 1025, 192, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,x2>|a2=0|pw=1", 1, 2, 2049, 192, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,f16>|a2=0|pw=0", 15, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,f16>|a2=0|pw=1", 1, 2, 17, 192, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1>|a2=1|pw=0", 1, 2, 17, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1>|a2=1|pw=1", 1, 2, 17, 4, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,x2>|a2=1|pw=0", 1, 2, 2049, 4, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,x2>|a2=1|pw=1", 1, 2, 2049, 4, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,f16>|a2=1|pw=0", 1, 2, 17, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,f16>|a2=1|pw=1", 1, 2, 17, 4, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=1|pw=0", 1, 2, 17, 32, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=1|pw=1", 1, 2, 17, 32, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,x2>|a2=1|pw=0", 1, 2, 2049, 32, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,x2>|a2=1|pw=1", 1, 2, 2049, 32, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=1|pw=0", 1, 2, 17, 32, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=1|pw=1", 1, 2, 17, 32, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=1|pw=0", 1, 2, 17, 64, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=1|pw=1", 1, 2, 17, 64, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,x2>|a2=1|pw=0", 1, 2, 2049, 64, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,x2>|a2=1|pw=1", 1, 2, 2049, 64, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=1|pw=0", 1, 2, 17, 64, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=1|pw=1", 1, 2, 17, 64, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=1|pw=0", 1, 2, 17, 96, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=1|pw=1", 1, 2, 17, 96, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=1|pw=0", 1, 2, 2049, 96, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=1|pw=1", 1, 2, 2049, 96, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=1|pw=0", 1, 2, 17, 96, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=1|pw=1", 1, 2, 17, 96, "f16", "f32", True, "unmerged"),
    # ---- pgemm_tn2_kernel
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2>|pw=0", 1, 2, 17, 32, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2>|pw=1", 1, 2, 17, 32, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,x2>|pw=0", 1, 2, 2049, 32, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,x2>|pw=1", 1, 2, 2049, 32, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,f16>|pw=0", 1, 2, 17, 32, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,f16>|pw=1", 1, 2, 17, 32, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1>|pw=0", 3, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1>|pw=1", 3, 2, 17, 4, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,x2>|pw=0", 3, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,x2>|pw=1", 3, 2, 2049, 4, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,f16>|pw=0", 3, 2, 17, 4, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,f16>|pw=1", 3, 2, 17, 4, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4>|pw=0", 5, 2, 17, 96, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4>|pw=1", 5, 2, 17, 96, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,x2>|pw=0", 5, 2, 2049, 96, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,x2>|pw=1", 5, 2, 2049, 96, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,f16>|pw=0", 5, 2, 17, 96, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,f16>|pw=1", 5, 2, 17, 96, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3>|pw=0", 8, 2, 17, 64, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3>|pw=1", 8, 2, 17, 64, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,x2>|pw=0", 8, 2, 2049, 64, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,x2>|pw=1", 8, 2, 2049, 64, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,f16>|pw=0", 8, 2, 17, 64, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,f16>|pw=1", 8, 2, 17, 64, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1>|pw=0", 10, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1>|pw=1", 10, 2, 17, 4, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,x2>|pw=0", 10, 2, 2049, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,x2>|pw=1", 10, 2, 2049, 4, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,f16>|pw=0", 10, 2, 17, 4, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,f16>|pw=1", 10, 2, 17, 4, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2>|pw=0", 13, 2, 17, 32, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2>|pw=1", 13, 2, 17, 32, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,x2>|pw=0", 13, 2, 2049, 32, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,x2>|pw=1", 13, 2, 2049, 32, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,f16>|pw=0", 13, 2, 17, 32, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,f16>|pw=1", 13, 2, 17, 32, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3>|pw=0", 15, 2, 17, 64, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3>|pw=1", 15, 2, 17, 64, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,x2>|pw=0", 15, 2, 2049, 64, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,x2>|pw=1", 15, 2, 2049, 64, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,f16>|pw=0", 15, 2, 17, 64, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,f16>|pw=1", 15, 2, 17, 64, "f16", "f32", True, "train"),
    # ---- gemm32_nt_kernel
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x64>", 1, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x128>", 5, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x192>", 10, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x256>", 15, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x320>", 20, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x384>", 25, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x448>", 30, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x32>", 1, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x64>", 3, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x96>", 5, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x128>", 8, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x160>", 10, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x192>", 13, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x224>", 15, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x256>", 18, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x288>", 20, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x320>", 23, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x352>", 25, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x384>", 28, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x416>", 30, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x448>", 33, 2, 2049, 4, "f32", "f32", False, "train"),
    # ---- gemm32_tn_kernel
    ("gemm32_tn_kernel", "gemm32_tn_kernel<1>|a2=0", 1, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<1>|a2=1", 1, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<2>|a2=0", 3, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<2>|a2=1", 1, 2, 2049, 32, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<3>|a2=0", 5, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<3>|a2=1", 1, 2, 2049, 64, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<4>|a2=0", 8, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<4>|a2=1", 1, 2, 2049, 96, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<5>|a2=0", 10, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<5>|a2=1", 1, 2, 2049, 128, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<6>|a2=0", 13, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<7>|a2=0", 15, 2, 2049, 4, "f32", "f32", False, "train"),
    # ---- gemm_f32_kernel
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[kk]", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[kn]", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[tn,ones]", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[tn,ones,shift]", 1, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[kk]", 1, 2, 17, 22, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[kn]", 5, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[tn,ones]", 5, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[tn,ones,shift]", 1, 2, 17, 64, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,64>[kk]", 1, 3, 8161, 192, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kk]", 1, 24, 1537, 129, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kn]", 52, 3, 8161, 4, "f32", "f32", False, "train"),
]

# ---- the edge half of the recurrence families ----------------------------------------------------------------------------
# A second case per key of the six window-major recurrence families (EDGE_FAMILIES), same tuple form, dims by rule:
#   H  the TOP of the key's width bracket: bracket_top() of the call form, the largest H whose plan() contains the key.  Every k
#      slot, hidden column and lane of the instance's last tile holds data, and the [h | 1] bias column lands on a tile edge
#      (grux_fwd: H = 31 / 63 / 95 / 127; gru: H = 4 K; gru_small: 32 / 64 / 96 / 106 / 112 / 128).
#   T  5: odd, so both parities of the double-buffered LDS state are used, and three interior steps -- a predecessor, a
#      successor and a prefetch in flight for a step that exists -- so each state buffer is rewritten after it was read, twice.
#   B  1 (mod 16) as in CASES: 17; 769 where gru.hip's kernels are selected; 833 where the key needs the B*T threshold
#      (5 x 833 = 4165 >= 4096: dGHn, lo=0 = f16x3g's single plane); the five one-pass cases CASES runs at B = 33 keep 33.
#   S, math, io, state and route are those of the key's case in CASES.
# One shape leaves the rule, on T (EDGE_T_OTHER): at (S, T, B, H) = (1, 5, 17, 106) the suite's draw has the 1 x 1 adjacency
# 0.0199, so g is of order 4e-4, GI is its bias at every step and consuming GI one step early moves Y by 2.4e-4 -- and by at
# most 6.9e-4 over the 600 parameter seeds 107 + 1000 k, k < 600: no PARAM_SEED entry reaches the 1e-3 the host test requires,
# the draw of A does not depend on it.  T = 7 (odd, five interior steps) draws A = 0.597: wrong-parity h 4.7e-2, dropped column
# 1.1e-2, GI one step early 2.1e-1.
# Two further one-pass fp16 cases run B = 33 (EDGE_B_MOVED), by the precedent of the five above CASES: at B = 17 a conv gradient
# of the carried-state step (a signed 1e-3 dY: the sums cancel) measured, relative to max, 7.1e-2 (grux_bwd_kernel<6,f16>|io=32|
# st=1, H = 64) and 1.1e-1 (grux_bwd_kernel<8,f16>|io=16|st=1, H = 84) against the imported 5e-2, with the GRU gradients of the
# same steps at 5.8e-4 / 1.5e-3 and the f16x3 siblings on the same inputs at 1.1e-6 / 9.4e-7 -- rounding of 85 rows, not
# indexing; at B = 33 they measured 4.8e-3 and 2.0e-3.  The second runs B = 65: the draw of (1, 5, 33, 84) has the 1 x 1
# adjacency 0.0192 and no parameter seed tried lifts "GI one step early" above 7.5e-4 there; (1, 5, 65, 84) draws 0.0301 and
# needs PARAM_SEED's entry for (1, 84) (see there); with it the case measured 4.6e-2 on the conv gradients (g is of order 1e-3
# on that draw, its products reach fp16's subnormals), 6.9e-4 on the GRU gradients, 1.9e-3 on Y (bf16 rounding).
# 254 keys on 49 distinct (S, T, B, H): 47 by the rule and these two; tests/test_instance_table_host.py re-derives every H and qualifies every shape on the
# oracle alone, tests/test_gpu_instance_edges.py runs them.
EDGE_FAMILIES = ("grux_fwd_kernel", "grux_bwd_kernel", "gru_fwd_kernel", "gru_bwd_kernel", "gru_small_fwd_kernel",
                 "gru_small_bwd_kernel")
EDGE_T = 5
EDGE_T_OTHER = {(1, 17, 106): 7}                            # (S, B, H) -> T
EDGE_B_MOVED = {"grux_bwd_kernel<6,f16>|io=32|st=1": 33, "grux_bwd_kernel<8,f16>|io=16|st=1": 65}
EDGE_CASES = [
    # ---- grux_fwd_kernel
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=32|st=0", 1, 5, 17, 31, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=32|st=1", 1, 5, 17, 31, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=16|st=0", 1, 5, 17, 31, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1>|io=16|st=1", 1, 5, 17, 31, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=32|st=0", 1, 5, 17, 31, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=32|st=1", 1, 5, 17, 31, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=16|st=0", 1, 5, 17, 31, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<1,f16>|io=16|st=1", 1, 5, 17, 31, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=32|st=0", 1, 5, 17, 63, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=32|st=1", 1, 5, 17, 63, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=16|st=0", 1, 5, 17, 63, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2>|io=16|st=1", 1, 5, 17, 63, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=32|st=0", 1, 5, 17, 63, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=32|st=1", 1, 5, 17, 63, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=16|st=0", 1, 5, 17, 63, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<2,f16>|io=16|st=1", 1, 5, 17, 63, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=32|st=0", 1, 5, 17, 95, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=32|st=1", 1, 5, 17, 95, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=16|st=0", 1, 5, 17, 95, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3>|io=16|st=1", 1, 5, 17, 95, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=32|st=0", 1, 5, 17, 95, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=32|st=1", 1, 5, 17, 95, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=16|st=0", 1, 5, 33, 95, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<3,f16>|io=16|st=1", 1, 5, 33, 95, "f16", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=32|st=0", 1, 5, 17, 127, "f16x3", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=32|st=1", 1, 5, 17, 127, "f16x3", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=16|st=0", 1, 5, 17, 127, "f16x3", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4>|io=16|st=1", 1, 5, 17, 127, "f16x3", "bf16", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=32|st=0", 1, 5, 17, 127, "f16", "f32", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=32|st=1", 1, 5, 17, 127, "f16", "f32", True, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=16|st=0", 1, 5, 17, 127, "f16", "bf16", False, "train"),
    ("grux_fwd_kernel", "grux_fwd_kernel<4,f16>|io=16|st=1", 1, 5, 17, 127, "f16", "bf16", True, "train"),
    # ---- grux_bwd_kernel
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=0|lo=0", 1, 5, 833, 8, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=0|lo=1", 1, 5, 17, 8, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=1|lo=0", 1, 5, 833, 8, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=32|st=1|lo=1", 1, 5, 17, 8, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=0|lo=0", 1, 5, 833, 8, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=0|lo=1", 1, 5, 17, 8, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=1|lo=0", 1, 5, 833, 8, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1>|io=16|st=1|lo=1", 1, 5, 17, 8, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=0|lo=0", 1, 5, 833, 20, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=0|lo=1", 1, 5, 17, 20, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=1|lo=0", 1, 5, 833, 20, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=32|st=1|lo=1", 1, 5, 17, 20, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=0|lo=0", 1, 5, 833, 20, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=0|lo=1", 1, 5, 17, 20, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=1|lo=0", 1, 5, 833, 20, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2>|io=16|st=1|lo=1", 1, 5, 17, 20, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=0|lo=0", 1, 5, 833, 32, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=0|lo=1", 1, 5, 17, 32, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=1|lo=0", 1, 5, 833, 32, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=32|st=1|lo=1", 1, 5, 17, 32, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=0|lo=0", 1, 5, 833, 32, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=0|lo=1", 1, 5, 17, 32, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=1|lo=0", 1, 5, 833, 32, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3>|io=16|st=1|lo=1", 1, 5, 17, 32, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=0|lo=0", 1, 5, 833, 40, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=0|lo=1", 1, 5, 17, 40, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=1|lo=0", 1, 5, 833, 40, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=32|st=1|lo=1", 1, 5, 17, 40, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=0|lo=0", 1, 5, 833, 40, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=0|lo=1", 1, 5, 17, 40, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=1|lo=0", 1, 5, 833, 40, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4>|io=16|st=1|lo=1", 1, 5, 17, 40, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=0|lo=0", 1, 5, 833, 52, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=0|lo=1", 1, 5, 17, 52, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=1|lo=0", 1, 5, 833, 52, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=32|st=1|lo=1", 1, 5, 17, 52, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=0|lo=0", 1, 5, 833, 52, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=0|lo=1", 1, 5, 17, 52, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=1|lo=0", 1, 5, 833, 52, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5>|io=16|st=1|lo=1", 1, 5, 17, 52, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=0|lo=0", 1, 5, 833, 64, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=0|lo=1", 1, 5, 17, 64, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=1|lo=0", 1, 5, 833, 64, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=32|st=1|lo=1", 1, 5, 17, 64, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=0|lo=0", 1, 5, 833, 64, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=0|lo=1", 1, 5, 17, 64, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=1|lo=0", 1, 5, 833, 64, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6>|io=16|st=1|lo=1", 1, 5, 17, 64, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=0|lo=0", 1, 5, 833, 72, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=0|lo=1", 1, 5, 17, 72, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=1|lo=0", 1, 5, 833, 72, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=32|st=1|lo=1", 1, 5, 17, 72, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=0|lo=0", 1, 5, 833, 72, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=0|lo=1", 1, 5, 17, 72, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=1|lo=0", 1, 5, 833, 72, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7>|io=16|st=1|lo=1", 1, 5, 17, 72, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=0|lo=0", 1, 5, 833, 84, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=0|lo=1", 1, 5, 17, 84, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=1|lo=0", 1, 5, 833, 84, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=32|st=1|lo=1", 1, 5, 17, 84, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=0|lo=0", 1, 5, 833, 84, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=0|lo=1", 1, 5, 17, 84, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=1|lo=0", 1, 5, 833, 84, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8>|io=16|st=1|lo=1", 1, 5, 17, 84, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=0|lo=0", 1, 5, 833, 96, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=0|lo=1", 1, 5, 17, 96, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=1|lo=0", 1, 5, 833, 96, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=32|st=1|lo=1", 1, 5, 17, 96, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=0|lo=0", 1, 5, 833, 96, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=0|lo=1", 1, 5, 17, 96, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=1|lo=0", 1, 5, 833, 96, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9>|io=16|st=1|lo=1", 1, 5, 17, 96, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=0|lo=0", 1, 5, 833, 104, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=0|lo=1", 1, 5, 17, 104, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=1|lo=0", 1, 5, 833, 104, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=32|st=1|lo=1", 1, 5, 17, 104, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=0|lo=0", 1, 5, 833, 104, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=0|lo=1", 1, 5, 17, 104, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=1|lo=0", 1, 5, 833, 104, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10>|io=16|st=1|lo=1", 1, 5, 17, 104, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=0|lo=0", 1, 5, 833, 116, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=0|lo=1", 1, 5, 17, 116, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=1|lo=0", 1, 5, 833, 116, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=32|st=1|lo=1", 1, 5, 17, 116, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=0|lo=0", 1, 5, 833, 116, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=0|lo=1", 1, 5, 17, 116, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=1|lo=0", 1, 5, 833, 116, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11>|io=16|st=1|lo=1", 1, 5, 17, 116, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=0|lo=0", 1, 5, 833, 127, "f16x3g", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=0|lo=1", 1, 5, 17, 127, "f16x3", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=1|lo=0", 1, 5, 833, 127, "f16x3g", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=32|st=1|lo=1", 1, 5, 17, 127, "f16x3", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=0|lo=0", 1, 5, 833, 127, "f16x3g", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=0|lo=1", 1, 5, 17, 127, "f16x3", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=1|lo=0", 1, 5, 833, 127, "f16x3g", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12>|io=16|st=1|lo=1", 1, 5, 17, 127, "f16x3", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=32|st=0", 1, 5, 17, 8, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=32|st=1", 1, 5, 17, 8, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=16|st=0", 1, 5, 17, 8, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<1,f16>|io=16|st=1", 1, 5, 17, 8, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=32|st=0", 1, 5, 17, 20, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=32|st=1", 1, 5, 17, 20, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=16|st=0", 1, 5, 17, 20, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<2,f16>|io=16|st=1", 1, 5, 17, 20, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=32|st=0", 1, 5, 17, 32, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=32|st=1", 1, 5, 17, 32, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=16|st=0", 1, 5, 17, 32, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<3,f16>|io=16|st=1", 1, 5, 17, 32, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=32|st=0", 1, 5, 17, 40, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=32|st=1", 1, 5, 17, 40, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=16|st=0", 1, 5, 17, 40, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<4,f16>|io=16|st=1", 1, 5, 17, 40, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=32|st=0", 1, 5, 17, 52, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=32|st=1", 1, 5, 17, 52, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=16|st=0", 1, 5, 17, 52, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<5,f16>|io=16|st=1", 1, 5, 17, 52, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=32|st=0", 1, 5, 17, 64, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=32|st=1", 1, 5, 33, 64, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=16|st=0", 1, 5, 17, 64, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<6,f16>|io=16|st=1", 1, 5, 17, 64, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=32|st=0", 1, 5, 17, 72, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=32|st=1", 1, 5, 17, 72, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=16|st=0", 1, 5, 17, 72, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<7,f16>|io=16|st=1", 1, 5, 33, 72, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=32|st=0", 1, 5, 17, 84, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=32|st=1", 1, 5, 17, 84, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=16|st=0", 1, 5, 17, 84, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<8,f16>|io=16|st=1", 1, 5, 65, 84, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=32|st=0", 1, 5, 17, 96, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=32|st=1", 1, 5, 17, 96, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=16|st=0", 1, 5, 17, 96, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<9,f16>|io=16|st=1", 1, 5, 17, 96, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=32|st=0", 1, 5, 17, 104, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=32|st=1", 1, 5, 17, 104, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=16|st=0", 1, 5, 17, 104, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<10,f16>|io=16|st=1", 1, 5, 17, 104, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=32|st=0", 1, 5, 17, 116, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=32|st=1", 1, 5, 17, 116, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=16|st=0", 1, 5, 17, 116, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<11,f16>|io=16|st=1", 1, 5, 17, 116, "f16", "bf16", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=32|st=0", 1, 5, 17, 127, "f16", "f32", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=32|st=1", 1, 5, 17, 127, "f16", "f32", True, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=16|st=0", 1, 5, 33, 127, "f16", "bf16", False, "train"),
    ("grux_bwd_kernel", "grux_bwd_kernel<12,f16>|io=16|st=1", 1, 5, 17, 127, "f16", "bf16", True, "train"),
    # ---- gru_fwd_kernel
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|st=0", 1, 5, 769, 16, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|st=1", 1, 5, 769, 16, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|st=0", 1, 5, 769, 32, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|st=1", 1, 5, 769, 32, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|st=0", 1, 5, 769, 48, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|st=1", 1, 5, 769, 48, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|st=0", 1, 5, 769, 64, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|st=1", 1, 5, 769, 64, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|st=0", 1, 5, 769, 80, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|st=1", 1, 5, 769, 80, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|st=0", 1, 5, 769, 96, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|st=1", 1, 5, 769, 96, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|st=0", 1, 5, 769, 104, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|st=1", 1, 5, 769, 104, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|st=0", 1, 5, 769, 112, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|st=1", 1, 5, 769, 112, "f32", "f32", True, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|st=0", 1, 5, 769, 128, "f32", "f32", False, "train"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|st=1", 1, 5, 769, 128, "f32", "f32", True, "train"),
    # ---- gru_bwd_kernel
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=0|dGH", 1, 5, 769, 16, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=0|dGHn", 1, 5, 833, 16, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=1|dGH", 1, 5, 769, 16, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|st=1|dGHn", 1, 5, 833, 16, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=0|dGH", 1, 5, 769, 32, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=0|dGHn", 1, 5, 833, 32, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=1|dGH", 1, 5, 769, 32, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|st=1|dGHn", 1, 5, 833, 32, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=0|dGH", 1, 5, 769, 48, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=0|dGHn", 1, 5, 833, 48, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=1|dGH", 1, 5, 769, 48, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|st=1|dGHn", 1, 5, 833, 48, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=0|dGH", 1, 5, 769, 64, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=0|dGHn", 1, 5, 833, 64, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=1|dGH", 1, 5, 769, 64, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|st=1|dGHn", 1, 5, 833, 64, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=0|dGH", 1, 5, 769, 80, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=0|dGHn", 1, 5, 833, 80, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=1|dGH", 1, 5, 769, 80, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|st=1|dGHn", 1, 5, 833, 80, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=0|dGH", 1, 5, 769, 96, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=0|dGHn", 1, 5, 833, 96, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=1|dGH", 1, 5, 769, 96, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|st=1|dGHn", 1, 5, 833, 96, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=0|dGH", 1, 5, 769, 104, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=0|dGHn", 1, 5, 833, 104, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=1|dGH", 1, 5, 769, 104, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|st=1|dGHn", 1, 5, 833, 104, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=0|dGH", 1, 5, 769, 112, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=0|dGHn", 1, 5, 833, 112, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=1|dGH", 1, 5, 769, 112, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|st=1|dGHn", 1, 5, 833, 112, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=0|dGH", 1, 5, 769, 128, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=0|dGHn", 1, 5, 833, 128, "f32", "f32", False, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=1|dGH", 1, 5, 769, 128, "f32", "f32", True, "train"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|st=1|dGHn", 1, 5, 833, 128, "f32", "f32", True, "train"),
    # ---- gru_small_fwd_kernel
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=32|st=0", 1, 5, 17, 32, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=32|st=1", 1, 5, 17, 32, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=64|st=0", 1, 5, 17, 64, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=64|st=1", 1, 5, 17, 64, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=96|st=0", 1, 5, 17, 96, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=96|st=1", 1, 5, 17, 96, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=108|st=0", 1, 7, 17, 106, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=108|st=1", 1, 7, 17, 106, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=112|st=0", 1, 5, 17, 112, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=112|st=1", 1, 5, 17, 112, "f32", "f32", True, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=128|st=0", 1, 5, 17, 128, "f32", "f32", False, "train"),
    ("gru_small_fwd_kernel", "gru_small_fwd_kernel|hmax=128|st=1", 1, 5, 17, 128, "f32", "f32", True, "train"),
    # ---- gru_small_bwd_kernel
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=32|st=0", 1, 5, 17, 32, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=32|st=1", 1, 5, 17, 32, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=64|st=0", 1, 5, 17, 64, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=64|st=1", 1, 5, 17, 64, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=96|st=0", 1, 5, 17, 96, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=96|st=1", 1, 5, 17, 96, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=108|st=0", 1, 7, 17, 106, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=108|st=1", 1, 7, 17, 106, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=112|st=0", 1, 5, 17, 112, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=112|st=1", 1, 5, 17, 112, "f32", "f32", True, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=128|st=0", 1, 5, 17, 128, "f32", "f32", False, "train"),
    ("gru_small_bwd_kernel", "gru_small_bwd_kernel|hmax=128|st=1", 1, 5, 17, 128, "f32", "f32", True, "train"),
]

# ---- the K-loop half of the two NT GEMM families --------------------------------------------------------------------------
# "The smallest dims that select it" keeps H = 4 where S selects the tile width and S = 1 where H does, so the product that
# carries a key of pgemm_nt_kernel or gemm32_nt_kernel contracts over 32 padded columns in CASES: ONE K stage -- no prefetch in
# flight under a compute phase, no ring slot used twice, no second barrier; gemm32's 128-row form runs its fused last step alone
# (nloop = nk - 1 = 0).  KLOOP_CASES gives a second case, same tuple form, to every key of NT_FAMILIES whose keyed product
# (keyed_product(): the NT launch of nt_products() that carries the key) runs fewer than KLOOP_STAGES stages in its CASES entry;
# dims by rule from that entry:
#   keyed through dg (N = 13 S selects the tile, K = Gp):  H = 74 -- 3 H = 222, Gp = 224: 7 stages, two zero pad columns in the last;
#   keyed through GI (N = 3 H selects it, K = Ip):         S = 17 -- 13 x 17 + 1 = 222, Ip = 224: 7 stages, the ones column and
#                                                          two pad columns in the last;
#   T, B, math, io, state and route are the entry's own: wide / narrow and every B*T threshold follow M and N alone.
# Seven: odd, so the two slots of a two-slot ring are used an unequal number of times; 7 = 2 x 3 + 1, so every slot of the
# three-slot A ring of the one-pass instances is rewritten after it was read, twice (slots 0 1 2 0 1 2 0); and gemm32's fused
# last step follows six ordinary iterations.  The keys CASES already runs past a one-stage loop (33 of the wide-GRU path, keyed
# through dg or the BPTT product with Gp = 384: 12 stages) get no second case.  103 cases on 53 distinct (S, T, B, H); no key
# leaves the rule.  tests/test_instance_table_host.py re-derives every entry and qualifies the inputs on the oracle alone,
# tests/test_gpu_instance_kloop.py runs them.
KLOOP_STAGES = 7
KLOOP_H, KLOOP_S = 74, 17                                   # the rule's H (keyed through dg) and S (keyed through GI)
KLOOP_CASES = [
    # ---- pgemm_nt_kernel
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1>|out16=0|wide", 17, 24, 1537, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1>|out16=0|narrow", 17, 2, 17, 4, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2>|out16=0|wide", 3, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2>|out16=0|narrow", 5, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3>|out16=0|wide", 5, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3>|out16=0|narrow", 10, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4>|out16=0|wide", 8, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4>|out16=0|narrow", 15, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5>|out16=0|wide", 10, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5>|out16=0|narrow", 20, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6>|out16=0|wide", 13, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6>|out16=0|narrow", 25, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7>|out16=0|wide", 15, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7>|out16=0|narrow", 30, 3, 8161, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8>|out16=0|wide", 18, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8>|out16=0|narrow", 52, 3, 5473, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9>|out16=0|wide", 20, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9>|out16=0|narrow", 60, 3, 5473, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10>|out16=0|wide", 23, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11>|out16=0|wide", 25, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12>|out16=0|wide", 28, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13>|out16=0|wide", 30, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14>|out16=0|wide", 33, 24, 1537, 74, "f16x3", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=1|wide", 1, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,x2>|out16=1|narrow", 1, 2, 2049, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=1|wide", 17, 24, 1537, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<1,f16>|out16=1|narrow", 17, 2, 17, 4, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=1|wide", 3, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,x2>|out16=1|narrow", 5, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=0|narrow", 17, 2, 2049, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=1|wide", 3, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<2,f16>|out16=1|narrow", 5, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=1|wide", 5, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,x2>|out16=1|narrow", 10, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=0|narrow", 17, 2, 3073, 192, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=1|wide", 5, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<3,f16>|out16=1|narrow", 10, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=1|wide", 8, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,x2>|out16=1|narrow", 15, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=0|narrow", 17, 3, 5473, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=1|wide", 8, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<4,f16>|out16=1|narrow", 15, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=1|wide", 10, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,x2>|out16=1|narrow", 20, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=0|narrow", 17, 3, 5473, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=1|wide", 10, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<5,f16>|out16=1|narrow", 20, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=1|wide", 13, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,x2>|out16=1|narrow", 25, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=0|narrow", 17, 3, 8161, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=1|wide", 13, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<6,f16>|out16=1|narrow", 25, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=1|wide", 15, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,x2>|out16=1|narrow", 30, 3, 8161, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=0|narrow", 17, 3, 8161, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=1|wide", 15, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<7,f16>|out16=1|narrow", 30, 3, 8161, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=1|wide", 18, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,x2>|out16=1|narrow", 52, 3, 5473, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=0|wide", 17, 3, 8161, 160, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=0|narrow", 17, 3, 5473, 225, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=1|wide", 18, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<8,f16>|out16=1|narrow", 52, 3, 5473, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=1|wide", 20, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,x2>|out16=1|narrow", 60, 3, 5473, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=0|wide", 17, 3, 8161, 192, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=1|wide", 20, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<9,f16>|out16=1|narrow", 60, 3, 5473, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,x2>|out16=1|wide", 23, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,f16>|out16=0|wide", 17, 3, 8161, 193, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<10,f16>|out16=1|wide", 23, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,x2>|out16=1|wide", 25, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,f16>|out16=0|wide", 17, 3, 8161, 224, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<11,f16>|out16=1|wide", 25, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,x2>|out16=1|wide", 28, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,f16>|out16=0|wide", 17, 24, 1537, 128, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<12,f16>|out16=1|wide", 28, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,x2>|out16=1|wide", 30, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,f16>|out16=0|wide", 17, 24, 1537, 129, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<13,f16>|out16=1|wide", 30, 24, 1537, 74, "f16", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,x2>|out16=1|wide", 33, 24, 1537, 74, "f16x3g", "f32", False, "train"),
    ("pgemm_nt_kernel", "pgemm_nt_kernel<14,f16>|out16=1|wide", 33, 24, 1537, 74, "f16", "f32", False, "train"),
    # ---- gemm32_nt_kernel
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x64>", 17, 3, 8161, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x128>", 5, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x192>", 10, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x256>", 15, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x320>", 20, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x384>", 25, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<128x448>", 30, 3, 8161, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x32>", 17, 2, 2049, 4, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x64>", 3, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x96>", 5, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x128>", 8, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x160>", 10, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x192>", 13, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x224>", 15, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x256>", 18, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x288>", 20, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x320>", 23, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x352>", 25, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x384>", 28, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x416>", 30, 2, 2049, 74, "f32", "f32", False, "train"),
    ("gemm32_nt_kernel", "gemm32_nt_kernel<32x448>", 33, 2, 2049, 74, "f32", "f32", False, "train"),
]

# One-pass fp16 K-loop cases above the imported bars, (key, tensor) -> bar: none.  The worst of the 36 one-pass cases measured
# 5.4e-3 on Y (pgemm_nt_kernel<8,f16>|out16=1|narrow: S = 52, 16 419 rows), 1.8e-4 on the loss and 1.4e-2 on a gradient
# (pgemm_nt_kernel<1,f16>|out16=1|narrow, conv1.weight at 34 rows) against 2e-2 / 2e-3 / 5e-2, with the f16x3 siblings at
# 3.7e-6 / 9.4e-8 / 2.1e-5.  An entry would be 1.5 x the figure of the fp64 step with the mode's operands rounded to fp16
# (lattice_inputs.fp64_step(f16_operands=True)) on the case's inputs, held by a host test as F16_FIGURES is.  Kept apart from
# F16_EXCEPTIONS: the keys are the same, the dims are not, and neither list may start applying to the other's cases.
KLOOP_F16_EXCEPTIONS = {}

# ---- gemm_f32_kernel past one K step ------------------------------------------------------------------------------------------
# The same question asked of gemm.hip's exact-fp32 products (gemm_f32_products()).  A K step is 16 columns; CASES keeps H = 4
# where S selects the key and S = 1 where H does, so the keyed product of an NT key contracts over 13 S = 13 or 3 H = 12 columns:
# ONE partial step -- no commit of step k + 1 into the other LDS stage, no refill of a register stage, and the 128 x 128 tile's
# one-register-stage pipeline (RS = 1) as little as the others' (RS = 2).  The exact count, over every launch of CASES, EDGE_CASES
# and KLOOP_CASES (the host test prints it): of the seven NT keys, FOUR never pass one step -- <64,128>[kk], <64,128>[kn],
# <128,128>[kk], <128,128>[kn]; <64,64>[kk] reaches 43 steps (GI of the <128,128>[kn] case, K = 676) and <64,64>[kn] 36 and
# <128,64>[kk] 12 as per-step products of the wide-GRU path (K = 3 H = 576, K = H = 192).  By the keyed product of its own CASES
# entry, six of seven run one step; <128,64>[kk] is keyed through `rec` at 12.  The four TN keys run 3 to 49 steps a chunk.
# GEMM_F32_KLOOP_CASES gives a second case, same tuple form, to every NT key whose keyed product (gemm_f32_keyed()) runs fewer
# than GEMM_F32_KLOOP_STEPS steps in one chunk in its CASES entry; dims by rule from that entry:
#   keyed through GI ([kk]: N = 3 H selects the tile, K = 13 S):  S = 8  -- K = 104: seven steps, the last with 8 live columns;
#   keyed through dg ([kn]: N = 13 S selects it, K = 3 H):        H = 35 -- K = 105: seven steps, the last with 9 live columns;
#   T, B and the rest are the entry's own: M, N, the tile and the split (1) do not depend on the dimension that moved.
# Seven: odd, so the two LDS stages are used an unequal number of times, and every register stage is refilled at least twice
# (RS = 2: at steps 0 to 3; RS = 1: at steps 0 to 4).  No key leaves the rule; no exact-fp32 layout here is gemm32.hip's (S = 52
# pads to 704 > 512 columns, H = 129 is the wide-GRU path) and no NT product is split.
GEMM_F32_KLOOP_STEPS = 7
GEMM_F32_KLOOP_S, GEMM_F32_KLOOP_H = 8, 35                  # the rule's S (keyed through GI) and H (keyed through dg)
GEMM_F32_KLOOP_CASES = [
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[kk]", 8, 2, 17, 4, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,64>[kn]", 1, 2, 17, 35, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[kk]", 8, 2, 17, 22, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[kn]", 5, 2, 17, 35, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kk]", 8, 24, 1537, 129, "f32", "f32", False, "train"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kn]", 52, 3, 8161, 35, "f32", "f32", False, "train"),
]

# The two-level fold (`since == 32`: after 512 columns acc is added into tot and cleared) needs 33 steps in ONE chunk.  One case
# per tile whose keyed product -- GI or dg: the role is tabled -- runs at least GEMM_F32_FOLD + 1 steps unsplit (so at least 64
# tiles) outside gemm32.hip's layouts (S >= 40, or the wide-GRU path):
#   <64,64>     an existing case does it and is named, not repeated: GI of CASES' <128,128>[kn] entry, K = 676, 43 steps;
#   <64,128>    (40, 2, 2017, 35):   GI, K = 520: 32 steps, the fold, one step of 8 live columns;
#   <128,64>    (40, 3, 2411, 192):  GI, K = 520 over 7233 rows x 576 columns (57 x 9 = 513 tiles of 128 x 64; in CASES the key is
#               carried by the wide-GRU path's per-step product, whose K = H could reach 513 only at N = 1539);
#   <128,128>   (40, 24, 1537, 129): GI [kk], K = 520;  (52, 3, 8161, 171): dg [kn], K = 513: ONE live column after the fold
#               (the same step runs <64,64>[kn] past the fold too, as the BPTT product: K = 513).
# (family, key, S, T, B, H, math, io, state, route, role): the case tuple and the role of the product that folds
GEMM_F32_FOLD_NAMED = ("gemm_f32_kernel<64,64>[kk]", "gemm_f32_kernel<128,128>[kn]", "GI")    # key, the CASES entry that runs it, role
GEMM_F32_FOLD_CASES = [
    ("gemm_f32_kernel", "gemm_f32_kernel<64,128>[kk]", 40, 2, 2017, 35, "f32", "f32", False, "train", "GI"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,64>[kk]", 40, 3, 2411, 192, "f32", "f32", False, "train", "GI"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kk]", 40, 24, 1537, 129, "f32", "f32", False, "train", "GI"),
    ("gemm_f32_kernel", "gemm_f32_kernel<128,128>[kn]", 52, 3, 8161, 171, "f32", "f32", False, "train", "dg"),
]

# ---- the K-loop half of the three TN families -----------------------------------------------------------------------------
# The weight-gradient products contract over the B*T rows, cut into split-K chunks of `kchunk` rows that are walked in stages of
# 32 rows through a two-slot LDS ring (tn_products()).  The splitter aims at 64 to 96 rows a chunk until sk reaches 256 / tiles,
# so at the smallest dims that select a key a chunk is two or three stages (CASES: 34 rows, sk = 1, kchunk = 64; the 4098-row
# keys sk = 64, kchunk = 96) and over every table above no launch of about 100 keys passes three (the exact count:
# tests/test_tn_kloop_host.py).  TN_KLOOP_CASES gives a second case, same tuple form, to the keys of TN_FAMILIES that CASES
# claims, walked in CASES order; a key gets one unless an earlier case of THIS table already launches it with every product it
# carries -- one role for a plain key, both for a merged '<TI+TH..>' key -- at seven stages (tn_seven()).  Dims by rule:
#   S, H, math, io, state and route are the CASES entry's own;
#   T = 3: 32 % 3 = 2, so the Y form's y_rem moves and wraps inside a chunk and the window-start mask meets every stage offset;
#   B = the smallest for which every carried product has kchunk >= 224 (TN_KLOOP_STAGES stages), B*T is no multiple of 32 (the
#       final stage is partial), the last non-empty chunk of every carried product has at least two stages (the partial stage
#       is zeroed in a slot that held an earlier one) and plan() still selects the key.
# One tile a chunk (sk = 256) gives B = 16 385: 49 155 rows, 220 chunks, the last of 99 rows -- four stages, three live rows in
# the fourth; two tiles (sk = 128: dW_hh of H = 128 ... 192) B = 8193; six (H = 224: sk = 40) B = 2561, 7683 rows.
# Seven: as KLOOP_STAGES -- odd, and each of the two slots is rewritten after it was read at least twice.
# Plane-form twins: every merged pw=0 key of the split modes forms dW_hh's B rows from fp32 Y at fp32 I/O (tn_hh_from_y());
# each has a second entry with bf16 I/O, which keeps the fp16 planes, so that both B sources of the same instantiation reach
# seven stages (tn_products()' `source`).  The rule skips three keys -- pgemm_tn_kernel<1>|a2=1|pw=0, <1,f16>|a2=1|pw=0 and
# gemm32_tn_kernel<1>|a2=1: the case of the <1>..|a2=0 key before each launches them at seven stages -- and no key leaves it:
# 105 keys and 14 twins, 119 cases on 39 distinct (S, T, B, H, io, state).  tests/test_tn_kloop_host.py re-derives every
# entry and qualifies the inputs on the oracle alone, tests/test_gpu_tn_kloop.py runs them.
#
# ONE deviation, TN_KLOOP_B_MOVED: the carried-state cases of six (S, H) run the first B ABOVE the rule's whose draw
# qualifies, because the rule's own draw does not -- a defect of the inputs, not of a kernel.  The carried-state step
# back-propagates a signed random dY, so every gradient is a sum of B*T (x S) cancelling terms, and two things that average
# out of the MSE step's coherent sums (no stateless case is touched) show at full size:
#   ReLU ties.  ONE term is ~1e-3 of a conv gradient's max.  A pre-activation of the fp64 reference within half an fp32 ulp of
#     zero (relative to the magnitudes of its 13 terms) has no sign to fp32 accuracy, and where a kernel -- or the reference itself
#     in fp32 -- lands on the other side the two differ by that whole term.  With 0.6 to 9.6 million pre-activations a case:
#     (8, 64)   B = 16 385: layer-2 element 1 665 318 is 1.6e-8 of its terms from zero (z = -2.8e-8).  Measured on the MI355X:
#               pgemm_tn_kernel<4+3>|pw=1 (f16x3) conv1.weight 9.41e-4, conv1.bias 8.70e-4, conv2.weight 1.18e-3, conv2.bias 6.75e-4
#               against the bar of 1e-4, every GRU gradient <= 4.9e-7; flipping that ONE mask element in the fp64 reference
#               moves the four by 9.29e-4, 8.58e-4, 1.17e-3, 6.74e-4.  (<4+3,x2>|pw=1: 1.25e-3 against 1e-3, the same element.)
#     (13, 32)  B = 16 385: the reference's own fp32 evaluation is 1.5e-4 / 1.6e-4 off its fp64 one on conv1.weight / conv1.bias
#     (5, 96), (10, 4), (15, 64)   elements at 5.2e-8, 1.4e-8 and 5.9e-9 whose flip costs 2.2e-3, 2.5e-4 and 1.7e-4 of max (the
#               MI355X happened to land on the reference's side of all three: <= 6.2e-5 measured)
#   f16x3g's single plane.  From 4096 rows that mode rounds dGI / dGHn to ONE fp16 plane and forms dW_ih as hi(dGI)^T hi(g):
#     2^-11 of each element, which the imported bar of such a case allows for (1e-3).  The fp64 step with those operands
#     rounded reproduces the MI355X's figures to two digits and depends on the draw: at (10, 4) it moves gru.weight_ih_l0 by
#     5.5e-4, 1.09e-3, 3.1e-4, 1.5e-3 and 2.4e-4 of max at B = 16 385 ... 16 389 (measured at 16 385 / 16 386: 5.61e-4 /
#     1.10e-3 -- above the bar with no kernel at fault), at (1, 96) conv2.weight by 5.1e-4, at (13, 32) and B = 16 386 conv1.bias
#     by 5.7e-4.  A draw qualifies where that rounding alone stays within half the bar.
# The moved B keeps every condition of the rule (49 158 ... 49 173 rows: tails of 6 to 21 live rows instead of 3); the host test
# shows that every B from the rule's up to the tabled one fails the qualification -- fp32 against fp64, the tie check or the
# single-plane check -- and that the tabled one passes.
TN_KLOOP_STAGES = 7
TN_KLOOP_T = 3
TN_KLOOP_TWIN_IO = "bf16"
TN_KLOOP_B_MOVED = {(1, 96): 16386, (5, 96): 16389, (8, 64): 16386, (10, 4): 16387, (13, 32): 16391, (15, 64): 16388}    # (S, H) of a carried-state case -> B


def tn_seven(p):
    """A product of tn_products() is taken to seven stages: full chunks of at least TN_KLOOP_STAGES stages, a partial final
    stage, and a last non-empty chunk of at least two stages."""
    return p["kchunk"] >= TN_KLOOP_STAGES * TN_BK and p["rows"] % TN_BK != 0 and p["last_stages"] >= 2


TN_KLOOP_CASES = [
    # ---- pgemm_tn_kernel
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1>|a2=0|pw=0", 1, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,f16>|a2=0|pw=0", 1, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=0|pw=0", 3, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=0|pw=0", 3, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=0|pw=0", 5, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=0|pw=0", 5, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=0|pw=0", 8, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=0|pw=1", 1, 3, 2561, 224, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=0|pw=0", 1, 3, 2561, 224, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=0|pw=1", 1, 3, 2561, 224, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=0|pw=0", 8, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=0|pw=1", 1, 3, 2561, 224, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5>|a2=0|pw=0", 10, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5>|a2=0|pw=1", 1, 3, 8193, 128, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,x2>|a2=0|pw=0", 1, 3, 8193, 128, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,x2>|a2=0|pw=1", 1, 3, 8193, 128, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,f16>|a2=0|pw=0", 10, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<5,f16>|a2=0|pw=1", 1, 3, 8193, 128, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6>|a2=0|pw=0", 13, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6>|a2=0|pw=1", 1, 3, 8193, 160, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,x2>|a2=0|pw=0", 1, 3, 8193, 160, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,x2>|a2=0|pw=1", 1, 3, 8193, 160, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,f16>|a2=0|pw=0", 13, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<6,f16>|a2=0|pw=1", 1, 3, 8193, 160, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7>|a2=0|pw=0", 15, 3, 16385, 4, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7>|a2=0|pw=1", 1, 3, 8193, 192, "f16x3", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,x2>|a2=0|pw=0", 1, 3, 8193, 192, "f16x3g", "f32", False, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,x2>|a2=0|pw=1", 1, 3, 8193, 192, "f16x3g", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,f16>|a2=0|pw=0", 15, 3, 16385, 4, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<7,f16>|a2=0|pw=1", 1, 3, 8193, 192, "f16", "f32", True, "train"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1>|a2=1|pw=1", 1, 3, 16385, 4, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,x2>|a2=1|pw=0", 1, 3, 16385, 4, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,x2>|a2=1|pw=1", 1, 3, 16385, 4, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<1,f16>|a2=1|pw=1", 1, 3, 16385, 4, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=1|pw=0", 1, 3, 16385, 32, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2>|a2=1|pw=1", 1, 3, 16385, 32, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,x2>|a2=1|pw=0", 1, 3, 16385, 32, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,x2>|a2=1|pw=1", 1, 3, 16385, 32, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=1|pw=0", 1, 3, 16385, 32, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<2,f16>|a2=1|pw=1", 1, 3, 16385, 32, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=1|pw=0", 1, 3, 16385, 64, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3>|a2=1|pw=1", 1, 3, 16385, 64, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,x2>|a2=1|pw=0", 1, 3, 16385, 64, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,x2>|a2=1|pw=1", 1, 3, 16385, 64, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=1|pw=0", 1, 3, 16385, 64, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<3,f16>|a2=1|pw=1", 1, 3, 16385, 64, "f16", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=1|pw=0", 1, 3, 16385, 96, "f16x3", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4>|a2=1|pw=1", 1, 3, 16386, 96, "f16x3", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=1|pw=0", 1, 3, 16385, 96, "f16x3g", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,x2>|a2=1|pw=1", 1, 3, 16386, 96, "f16x3g", "f32", True, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=1|pw=0", 1, 3, 16385, 96, "f16", "f32", False, "unmerged"),
    ("pgemm_tn_kernel", "pgemm_tn_kernel<4,f16>|a2=1|pw=1", 1, 3, 16386, 96, "f16", "f32", True, "unmerged"),
    # ---- pgemm_tn2_kernel (the bf16 entries: the plane-form twins)
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2>|pw=0", 1, 3, 16385, 32, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2>|pw=0", 1, 3, 16385, 32, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2>|pw=1", 1, 3, 16385, 32, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,x2>|pw=0", 1, 3, 16385, 32, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,x2>|pw=0", 1, 3, 16385, 32, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,x2>|pw=1", 1, 3, 16385, 32, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,f16>|pw=0", 1, 3, 16385, 32, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<1+2,f16>|pw=1", 1, 3, 16385, 32, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1>|pw=0", 3, 3, 16385, 4, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1>|pw=0", 3, 3, 16385, 4, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1>|pw=1", 3, 3, 16385, 4, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,x2>|pw=0", 3, 3, 16385, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,x2>|pw=0", 3, 3, 16385, 4, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,x2>|pw=1", 3, 3, 16385, 4, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,f16>|pw=0", 3, 3, 16385, 4, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<2+1,f16>|pw=1", 3, 3, 16385, 4, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4>|pw=0", 5, 3, 16385, 96, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4>|pw=0", 5, 3, 16385, 96, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4>|pw=1", 5, 3, 16389, 96, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,x2>|pw=0", 5, 3, 16385, 96, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,x2>|pw=0", 5, 3, 16385, 96, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,x2>|pw=1", 5, 3, 16389, 96, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,f16>|pw=0", 5, 3, 16385, 96, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<3+4,f16>|pw=1", 5, 3, 16389, 96, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3>|pw=0", 8, 3, 16385, 64, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3>|pw=0", 8, 3, 16385, 64, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3>|pw=1", 8, 3, 16386, 64, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,x2>|pw=0", 8, 3, 16385, 64, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,x2>|pw=0", 8, 3, 16385, 64, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,x2>|pw=1", 8, 3, 16386, 64, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,f16>|pw=0", 8, 3, 16385, 64, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<4+3,f16>|pw=1", 8, 3, 16386, 64, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1>|pw=0", 10, 3, 16385, 4, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1>|pw=0", 10, 3, 16385, 4, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1>|pw=1", 10, 3, 16387, 4, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,x2>|pw=0", 10, 3, 16385, 4, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,x2>|pw=0", 10, 3, 16385, 4, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,x2>|pw=1", 10, 3, 16387, 4, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,f16>|pw=0", 10, 3, 16385, 4, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<5+1,f16>|pw=1", 10, 3, 16387, 4, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2>|pw=0", 13, 3, 16385, 32, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2>|pw=0", 13, 3, 16385, 32, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2>|pw=1", 13, 3, 16391, 32, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,x2>|pw=0", 13, 3, 16385, 32, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,x2>|pw=0", 13, 3, 16385, 32, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,x2>|pw=1", 13, 3, 16391, 32, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,f16>|pw=0", 13, 3, 16385, 32, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<6+2,f16>|pw=1", 13, 3, 16391, 32, "f16", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3>|pw=0", 15, 3, 16385, 64, "f16x3", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3>|pw=0", 15, 3, 16385, 64, "f16x3", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3>|pw=1", 15, 3, 16388, 64, "f16x3", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,x2>|pw=0", 15, 3, 16385, 64, "f16x3g", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,x2>|pw=0", 15, 3, 16385, 64, "f16x3g", "bf16", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,x2>|pw=1", 15, 3, 16388, 64, "f16x3g", "f32", True, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,f16>|pw=0", 15, 3, 16385, 64, "f16", "f32", False, "train"),
    ("pgemm_tn2_kernel", "pgemm_tn_kernel<7+3,f16>|pw=1", 15, 3, 16388, 64, "f16", "f32", True, "train"),
    # ---- gemm32_tn_kernel
    ("gemm32_tn_kernel", "gemm32_tn_kernel<1>|a2=0", 1, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<2>|a2=0", 3, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<2>|a2=1", 1, 3, 16385, 32, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<3>|a2=0", 5, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<3>|a2=1", 1, 3, 16385, 64, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<4>|a2=0", 8, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<4>|a2=1", 1, 3, 16385, 96, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<5>|a2=0", 10, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<5>|a2=1", 1, 3, 8193, 128, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<6>|a2=0", 13, 3, 16385, 4, "f32", "f32", False, "train"),
    ("gemm32_tn_kernel", "gemm32_tn_kernel<7>|a2=0", 15, 3, 16385, 4, "f32", "f32", False, "train"),
]

# One-pass fp16 cases of TN_KLOOP_CASES above the imported bars, (key, tensor) -> bar: none (as KLOOP_F16_EXCEPTIONS; kept apart
# for the same reason)
TN_KLOOP_F16_EXCEPTIONS = {}

# ---- the series entry points -------------------------------------------------------------------------------------------
# (family, key, S, H, rows, T, stride, n, seed, route); the inputs are tests/test_gpu_series.py's _draw(S, H, rows, T, stride, n,
# seed).  n = 1 (mod 16): the last workgroup of a recurrence is ragged, with one valid window.
# Shape A: rows 36, T 3, stride 2, n 17 -- n*T = 51, both layouts below 4096: the full dGH, no [Hprev | 1] rows; coverage
#   alternates between 1 and 2, one spare row; H at the TOP of each K's range (4 K: every k slot of the instance in use).
# Shape B: rows 272, T 16, stride 1, n 257 -- n*T = 4112 >= 4096 with the front layout (272 rows) below: dGHn and the
#   [Hprev | 1] rows of rup(H + 1, 16) floats; H at the BOTTOM of each range (4 K_prev + 1).
# The fold's zero rows: tests/test_gpu_series.py's `gaps` shape (stride 5 > T 3: hours 3, 4, 8, 9 are covered by no window).
# Seeds: the smallest at which no ReLU pre-activation of the fp64 reference lies within 1e-5 (relative) of zero and the
# reference's own fp32 evaluation agrees with its fp64 one to 1e-5 (tests/test_instance_table_host.py asserts both).
SERIES_CASES = [
    # ---- gru_fwd_kernel
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|series|y", 2, 16, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|series|loss", 2, 16, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<4>|series|last", 2, 16, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|series|y", 2, 32, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|series|loss", 2, 32, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<8>|series|last", 2, 32, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|series|y", 2, 48, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|series|loss", 2, 48, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<12>|series|last", 2, 48, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|series|y", 2, 64, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|series|loss", 2, 64, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<16>|series|last", 2, 64, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|series|y", 2, 80, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|series|loss", 2, 80, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<20>|series|last", 2, 80, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|series|y", 2, 96, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|series|loss", 2, 96, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<24>|series|last", 2, 96, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|series|y", 2, 104, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|series|loss", 2, 104, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<26>|series|last", 2, 104, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|series|y", 2, 112, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|series|loss", 2, 112, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<28>|series|last", 2, 112, 36, 3, 2, 17, 0, "series_last"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|series|y", 2, 128, 36, 3, 2, 17, 0, "series"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|series|loss", 2, 128, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_fwd_kernel", "gru_fwd_kernel<32>|series|last", 2, 128, 36, 3, 2, 17, 0, "series_last"),
    # ---- gru_bwd_kernel
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|series|dY|dGH", 2, 16, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|series|dY|dGHn", 2, 4, 272, 16, 1, 257, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|series|mse|dGH", 2, 16, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<12>|series|mse|dGHn", 2, 4, 272, 16, 1, 257, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|series|dY|dGH", 2, 32, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|series|dY|dGHn", 2, 17, 272, 16, 1, 257, 7, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|series|mse|dGH", 2, 32, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<24>|series|mse|dGHn", 2, 17, 272, 16, 1, 257, 7, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|series|dY|dGH", 2, 48, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|series|dY|dGHn", 2, 33, 272, 16, 1, 257, 1, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|series|mse|dGH", 2, 48, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<36>|series|mse|dGHn", 2, 33, 272, 16, 1, 257, 1, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|series|dY|dGH", 2, 64, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|series|dY|dGHn", 2, 49, 272, 16, 1, 257, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|series|mse|dGH", 2, 64, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<48>|series|mse|dGHn", 2, 49, 272, 16, 1, 257, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|series|dY|dGH", 2, 80, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|series|dY|dGHn", 2, 65, 272, 16, 1, 257, 5, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|series|mse|dGH", 2, 80, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<60>|series|mse|dGHn", 2, 65, 272, 16, 1, 257, 5, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|series|dY|dGH", 2, 96, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|series|dY|dGHn", 2, 81, 272, 16, 1, 257, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|series|mse|dGH", 2, 96, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<72>|series|mse|dGHn", 2, 81, 272, 16, 1, 257, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|series|dY|dGH", 2, 104, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|series|dY|dGHn", 2, 97, 272, 16, 1, 257, 1, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|series|mse|dGH", 2, 104, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<78>|series|mse|dGHn", 2, 97, 272, 16, 1, 257, 1, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|series|dY|dGH", 2, 112, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|series|dY|dGHn", 2, 105, 272, 16, 1, 257, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|series|mse|dGH", 2, 112, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<84>|series|mse|dGHn", 2, 105, 272, 16, 1, 257, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|series|dY|dGH", 2, 128, 36, 3, 2, 17, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|series|dY|dGHn", 2, 113, 272, 16, 1, 257, 0, "series"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|series|mse|dGH", 2, 128, 36, 3, 2, 17, 0, "series_mse"),
    ("gru_bwd_kernel", "gru_bwd_kernel<96>|series|mse|dGHn", 2, 113, 272, 16, 1, 257, 0, "series_mse"),
    # ---- series_fold_kernel
    ("series_fold_kernel", "series_fold_kernel|terms=0..1", 7, 21, 13, 3, 5, 3, 0, "series"),
    ("series_fold_kernel", "series_fold_kernel|terms=1..2", 2, 16, 36, 3, 2, 17, 0, "series"),
    ("series_fold_kernel", "series_fold_kernel|terms=T", 2, 4, 272, 16, 1, 257, 0, "series"),
]
