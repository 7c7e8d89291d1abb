"""Host side of the fused step tail's loop regimes (no GPU): tests/finish_cases.py held to the text of csrc/finish.hip and of
api.hip's pick_splitk call sites, its split-K figures to wgnn_tn_split, the exact table of the regimes reachable with
B*T <= 4200 rows and which case claims each, what the nine shapes of the older finish tests reached, the (shift, seed) of every
draw re-derived, and reduction mistakes planted into the fp64 oracle's step: the weight gradients formed as sums over the K
chunks and the conv gradients as sums over the partial rows, as finish sums them.  tests/test_gpu_finish_regimes.py runs the
cases on the MI355X."""
import functools
import math as pymath
import re

import pytest
import torch

import finish_cases as fc
import gcn_loop_cases as gl
import instance_cases as ic
import lattice_inputs as li
import test_lattice_inputs_host as tli
from conftest import PARAM_KEYS, rel_to_max
from test_instance_table_host import MATH, _read
from test_tn_kloop_host import _lib, tn_step

BAR = 1e-4                                           # the fp32-grade gradient bar (tests/test_gpu_parity.py G_TOL)


# ---- 1. the restatement against the source text ------------------------------------------------------------------------------
def _one(pattern, text, flags=0):
    """The groups of the ONE match of `pattern` in `text` (as ints where they are digits)."""
    found = re.findall(pattern, text, flags)
    assert len(found) == 1, (pattern, found)
    g = found[0] if isinstance(found[0], tuple) else (found[0],)
    return tuple(int(x) if x.isdigit() else x for x in g)


def test_the_loop_heads_are_those_of_finish_hip():
    src = _read("finish.hip")
    tn = src[src.index("void seg_tn("):src.index("void seg_plain(")]
    plain = src[src.index("void seg_plain("):src.index("void seg_conv(")]
    conv = src[src.index("void seg_conv("):src.index("void seg_elem(")]
    # seg_tn: the flat branch, the four z phases, the 16-stride body of four loads, the tail, the fold
    assert _one(r"if \(s\.splitk < (\d+)\) \{", tn) == (fc.TN_FLAT_BELOW,)
    assert _one(r"for \(int z = 1; z < s\.splitk; \+\+z\) v \+= src\[\(size_t\)z \* slab4\];", tn)
    assert _one(r"const int tx = threadIdx\.x & 63, ty = threadIdx\.x >> (\d+);", tn) == (6,) and 256 >> 6 == fc.TN_PHASES
    assert _one(r"int z = ty;\s*for \(; z \+ (\d+) < s\.splitk; z \+= (\d+)\) \{", tn) == (fc.TN_BODY_REACH, fc.TN_BODY_STRIDE)
    body = tn[tn.index("z += 16) {"):tn.index("for (; z < s.splitk; z += 4)")]
    assert re.findall(r"s(\d) \+= src\[\(size_t\)\(?z(?: \+ (\d+))?\)? \* slab4\];", body) == [("0", ""), ("1", "4"), ("2", "8"), ("3", "12")]
    assert _one(r"for \(; z < s\.splitk; z \+= (\d+)\) s0 \+= src\[\(size_t\)z \* slab4\];", tn) == (fc.TN_TAIL_STRIDE,)
    assert fc.TN_BODY_STRIDE == 4 * fc.TN_TAIL_STRIDE and fc.TN_BODY_REACH == 3 * fc.TN_TAIL_STRIDE and fc.TN_TAIL_STRIDE == fc.TN_PHASES
    assert "    red[ty][tx] = (s0 + s1) + (s2 + s3);\n    __syncthreads();\n    if (ty != 0) return;\n" in tn
    assert "    v = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);\n" in tn
    # the wide-store predicate: W_ih, fp16-plane images, no row remap, 13 S and 3 H multiples of 4
    assert ("  if (ADAM && tw == T_WIH && a.prep_kind == 1 && s.msplit == 0 && (s.ncols & 3) == 0 && (s.Mout & 3) == 0 && n < s.ncols &&\n"
            "      m0 < s.Mout) {\n") in tn
    assert "using X1 = std::integral_constant<int, 0xB1>;" in tn and "using X2 = std::integral_constant<int, 0x4E>;" in tn
    api = _read("api.hip")
    assert "\n  L.prep_kind = x3 ? 1 : (g32_shape ? 2 : 0);\n" in api
    assert "\n    ih.Mout = ih.Mgemm = (int)L.G3; ih.Nout = (int)L.I + 1; ih.ncols = (int)L.I;\n" in api
    assert "\n    if (L.dghn) { hh.msplit = L.msplit; hh.rows1 = 2 * d->H; }" in api      # (ih never has a remap)
    assert [fc.wide_stores(S, H, m) for S, H, m in ((8, 12, "f16x3"), (8, 12, "f32"), (5, 12, "f16"), (8, 9, "f16x3g"), (4, 4, "f16"))] == [
        True, False, False, False, True]
    # seg_plain: body of eight loads, then single chunks
    assert _one(r"for \(; z \+ (\d+) <= s\.splitk; z \+= (\d+)\) \{", plain) == (fc.PLAIN_BODY, fc.PLAIN_BODY)
    assert re.findall(r"s(\d) \+= s\.partial\[\(size_t\)\(?z(?: \+ (\d+))?\)? \* MN \+ i\];", plain) == [
        ("0", "")] + [(str(k), str(k)) for k in range(1, 8)] + [("0", "")]
    assert _one(r"for \(; z < s\.splitk; \+\+z\) s0 \+= s\.partial\[\(size_t\)z \* MN \+ i\];", plain)
    assert "  if (n >= s.Nout) return;" in plain and "    if (m >= s.msplit) m = s.rows1 + (m - s.msplit);\n    else if (m >= s.rows1) return;\n" in plain
    # seg_conv: eight row phases, the 32-stride body of four loads, the tail, the fold
    assert _one(r"const int tx = threadIdx\.x & 31, ty = threadIdx\.x >> (\d+);", conv) == (5,) and 256 >> 5 == fc.CONV_PHASES
    assert _one(r"int b = ty;\s*for \(; b \+ (\d+) < a\.conv_rows; b \+= (\d+)\) \{", conv) == (fc.CONV_BODY_REACH, fc.CONV_BODY_STRIDE)
    assert re.findall(r"s(\d) \+= a\.conv_partial\[\(size_t\)\(?b(?: \+ (\d+))?\)? \* PART \+ i\];", conv) == [
        ("0", ""), ("1", "8"), ("2", "16"), ("3", "24"), ("0", "")]
    assert _one(r"for \(; b < a\.conv_rows; b \+= (\d+)\) s0 \+=", conv) == (fc.CONV_TAIL_STRIDE,)
    assert "  for (int k = 0; k < 8; ++k) s += sm[k][tx];\n" in conv
    # finish_norm_kernel runs the same segments
    norm = src[src.index("void __launch_bounds__(256) finish_norm_kernel("):src.index("void __launch_bounds__(1024) clip_coef_kernel(")]
    assert norm.count("seg_tn<0, 1>(") == 2 and norm.count("seg_plain<0, 1>(") == 2 and norm.count("seg_conv<0, 1>(") == 1


def test_the_split_k_and_row_counts_are_those_of_the_call_sites():
    api = _read("api.hip")
    sites = re.findall(r"pick_splitk\(L\.BT, (\w+)\(\(int\)L\.G3, \(int\)L\.[IH] \+ 1\)|pick_splitk\(L\.BT, (\w+)\(L\.m_hh, \(int\)L\.H \+ 1\)", api)
    assert len(sites) == 6
    divisors = re.findall(r"pick_splitk\(L\.BT, (\w+)\([^;:]*?\), (\d+), (\d+)\)", api)
    assert divisors == [("pgemm_tn_tiles", "256", "64")] * 2 + [("gemm32_tn_tiles", "256", "64"), ("gemm_f32_tiles", "1024", "128")] * 2
    assert api.count("pick_splitk(") == 7                                       # the six call sites and the definition
    for line in ("int pick_splitk(size_t BT, int tiles, int target_wgs, int min_rows) {", "  int by_rows = (int)(BT / (size_t)min_rows);",
                 "  int by_grid = target_wgs / (tiles > 0 ? tiles : 1);", "  int sk = by_rows < by_grid ? by_rows : by_grid;",
                 "  if (sk >= 8) sk -= sk % 8;       // multiples of 8 keep the tiles of one K chunk on one XCD", "  return sk < 1 ? 1 : sk;",
                 "    ih.splitk = L.sk_ih;", "    hh.splitk = L.sk_hh;", "    ih.kind = L.x3 ? 2 : 1;",
                 "    a.conv_rows = L.gen_gcn ? gcn_csr_bwd_rows()",
                 "                            : (L.x3 ? gcnx_bwd_grid((int)L.BT, d->S, three_pass(d)) : gcn32_bwd_grid((int)L.BT, d->S));"):
        assert "\n" + line + "\n" in api, line
    assert "\nconstexpr int CSR_BLOCKS = %d;" % fc.CSR_ROWS in _read("general.hip") and "\nint gcn_csr_bwd_rows() { return CSR_BLOCKS; }\n" in _read("general.hip")
    g32 = _read("gcn32.hip")
    assert "\nint bwd_waves_of(int S, int ntiles) { return (S <= 48 && ntiles >= 16384) ? 16 : 12; }\n" in g32
    assert "\n  int gx = cdiv_i(ntiles, bwd_waves_of(S, ntiles));\n  return gx < 1 ? 1 : (gx > 256 ? 256 : gx);" in g32
    assert "\nint gemm32_tn_pitch(int No) { return (No + 15) & ~15; }" in _read("gemm32.hip")
    assert "const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;" in _read("gcnx.hip") and "tile += nwaves" in _read("gcnx.hip")
    assert [ic.pick_splitk(bt, 1, 256, 64) for bt in (96, 128, 260, 320, 448, 520, 1040, 1552, 2580)] == [1, 2, 4, 5, 7, 8, 16, 24, 40]
    assert [ic.pick_splitk(bt, 1, 1024, 128) for bt in (128, 260, 448, 520, 660, 780, 900, 1040, 2580, 3080)] == [1, 2, 3, 4, 5, 6, 7, 8, 16, 24]
    # the walks count what the loops do
    assert fc.tn_trips(3) is None and fc.tn_trips(5) == [(0, 2), (0, 1), (0, 1), (0, 1)] and fc.tn_trips(7) == [(0, 2), (0, 2), (0, 2), (0, 1)]
    assert fc.tn_trips(16) == [(1, 0)] * 4 and fc.tn_trips(24) == [(1, 2)] * 4 and fc.tn_trips(40) == [(2, 2)] * 4 and fc.tn_trips(96) == [(6, 0)] * 4
    assert fc.plain_trips(7) == [(0, 7)] and fc.plain_trips(8) == [(1, 0)] and fc.plain_trips(24) == [(3, 0)] and fc.plain_trips(12) == [(1, 4)]
    assert fc.conv_trips(27) == [(1, 0)] * 3 + [(0, 3)] * 5 and fc.conv_trips(38) == [(1, 1)] * 6 + [(1, 0)] * 2 and fc.conv_trips(256) == [(8, 0)] * 8
    for n in range(1, 300):                          # every index is summed exactly once
        for trips, stride, bstride in ((fc.tn_trips(n), 4, 16), (fc.conv_trips(n), 8, 32)):
            if trips is not None:
                body = [ph + k * bstride + j * stride for ph, (b, _) in enumerate(trips) for k in range(b) for j in range(4)]
                assert sorted(body + fc.tail_chunks(trips, stride, bstride)) == list(range(n)), n
                assert max(fc.last_of_phase(trips, stride, bstride, ph) or 0 for ph in range(len(trips))) == n - 1
    assert fc.tail_chunks(fc.tn_trips(24), 4, 16) == list(range(16, 24)) and fc.last_of_phase(fc.tn_trips(16), 4, 16, 1) == 13


def _all_dims():
    return [c[:5] + (m,) for c in fc.SHAPES for m in fc.modes_of(c)] + [c + (m,) for c in fc.LEGACY_SHAPES for m in fc.LEGACY_MODES]


def test_split_k_and_kchunk_as_wgnn_tn_split_gives_them():
    """sk of both products in every mode, and kchunk where the TN splitters cut the rows (wgnn_tn_split reports their rounding;
    gemm.hip rounds its chunks to 16 rows itself), for every case and every legacy shape."""
    L = _lib()
    assert fc.CASES == [c for c in _all_dims() if c[:5] in fc.SHAPES]
    for S, T, B, H, csr, math in _all_dims():
        if csr and S > 64:
            continue                                 # (the restatement speaks of dense dims; api.hip takes sk from B*T, S and H alone)
        i = L.tn_split(L.Dims(B, T, S, 13, H, MATH[math], int(csr), 3 * S if csr else 0, 0), state=False)
        seg = fc.segments(S, T, B, H, math, csr)
        assert (seg["ih"]["sk"], seg["hh"]["sk"]) == (i.sk_ih, i.sk_hh), (S, T, B, H, math, seg, i.sk_ih, i.sk_hh)
        if seg["ih"]["family"] != "gemm":
            assert (seg["ih"]["kchunk"], seg["hh"]["kchunk"]) == (i.kchunk_ih, i.kchunk_hh), (S, T, B, H, math)
        for k in ("ih", "hh"):
            assert seg[k]["chunks"] == ic.cdiv(B * T, seg[k]["kchunk"]) <= seg[k]["sk"]


# ---- 2. the regime table ----------------------------------------------------------------------------------------------------
P = "phased"
# seg_tn: reachable split-K values are 1 .. 7 and the multiples of 8 up to 64 (B*T / 64 <= 65) -> regime
TN_REGIMES = {
    1: ("flat", 1), 2: ("flat", 2), 3: ("flat", 3),
    4: (P, (0, 0, 0, 0), (1, 1, 1, 1)), 5: (P, (0, 0, 0, 0), (2, 1, 1, 1)), 6: (P, (0, 0, 0, 0), (2, 2, 1, 1)),
    7: (P, (0, 0, 0, 0), (2, 2, 2, 1)), 8: (P, (0, 0, 0, 0), (2, 2, 2, 2)),
    16: (P, (1, 1, 1, 1), (0, 0, 0, 0)), 24: (P, (1, 1, 1, 1), (2, 2, 2, 2)),                  # 24: the body, then the tail
    32: (P, (2, 2, 2, 2), (0, 0, 0, 0)), 40: (P, (2, 2, 2, 2), (2, 2, 2, 2)),                  # 48, 64 as 32; 56 as 40
}
# seg_plain on gemm.hip's partials: 1 .. 7 (tail only) and 8, 16, 24, 32 (B*T / 128 <= 32): the tail never follows the body
GEMM_REGIMES = {1: (0, 1), 2: (0, 2), 3: (0, 3), 4: (0, 4), 5: (0, 5), 6: (0, 6), 7: (0, 7), 8: (1, 0), 16: (2, 0)}
# ... on gemm32.hip's (4096 <= B*T <= 4200: 64 or 65 by rows, 256 / tiles with at most six tiles): body only
GEMM32_REGIMES = {64: (2, 0)}
CONV_REGIMES = {(0, 0, "even"), (0, 0, "ragged"), (0, 1, "ragged"), (1, 1, "none"), (1, 1, "even"), (1, 1, "ragged"), (1, 2, "ragged"),
                (2, 2, "none"), (2, 2, "even"), (2, 2, "ragged")}


def _reachable():
    tn, gemm, gemm32, conv = set(), set(), set(), set()
    g32_tiles = ic.gemm32_tn_tiles(512, 513)         # g32_rows: rup(13 S + 1, 32) <= 512 and rup(3 H, 32) <= 512
    for BT in range(1, fc.ROWS_MAX + 1):
        for tiles in range(1, 257):
            tn.add(fc.tn_regime(ic.pick_splitk(BT, tiles, 256, 64)))
            if BT >= 4096 and tiles <= g32_tiles:
                gemm32.add(fc.plain_regime(ic.pick_splitk(BT, tiles, 256, 64)))
        for tiles in (1, 2, 3, 4, 6, 8, 12, 16, 32, 64, 100, 128, 200, 256, 500, 1024, 2000):
            gemm.add(fc.plain_regime(ic.pick_splitk(BT, tiles, 1024, 128)))      # (H > 128 runs gemm.hip at every B*T)
        for waves in (gl.BWD4_WAVES, gl.BWD_WAVES, gl.BWD_WAVES_ONE_PASS):
            conv.add(fc.conv_regime(max(1, min(ic.cdiv(BT, waves), gl.BWD_GRID_CAP))))
    conv.add(fc.conv_regime(fc.CSR_ROWS))
    return tn, gemm, gemm32, conv


def _claims():
    """(segment kind, family, wide stores, remap) x regime -> the cases that claim it."""
    out = {}
    for c in fc.CASES:
        S, T, B, H, csr, math = c
        seg = fc.segments(S, T, B, H, math, csr)
        for k in ("ih", "hh"):
            s = seg[k]
            out.setdefault((s["family"], seg["wide"] and k == "ih", s["remap"], s["regime"]), []).append(c)
        out.setdefault(("conv", False, False, seg["conv"]), []).append(c)
    return out


def test_every_reachable_regime_is_claimed():
    tn, gemm, gemm32, conv = _reachable()
    assert tn == set(TN_REGIMES.values()) and {fc.tn_regime(sk) for sk in TN_REGIMES} == tn
    assert {fc.tn_regime(sk) for sk in (48, 64)} == {TN_REGIMES[32]} and fc.tn_regime(56) == TN_REGIMES[40]
    assert gemm == set(GEMM_REGIMES.values()) and fc.plain_regime(24) == fc.plain_regime(32) == GEMM_REGIMES[16]
    assert gemm32 == set(GEMM32_REGIMES.values()) and conv == CONV_REGIMES
    assert all(TN_REGIMES[sk] == fc.tn_regime(sk) for sk in TN_REGIMES) and all(GEMM_REGIMES[sk] == fc.plain_regime(sk) for sk in GEMM_REGIMES)
    assert [sk for sk in TN_REGIMES if fc.tail_follows_body(fc.tn_trips(sk))] == [24, 40]
    assert [sk for sk in TN_REGIMES if fc.ragged(fc.tn_trips(sk))] == [5, 6, 7]
    assert not any(fc.tail_follows_body(fc.plain_trips(sk)) for sk in list(GEMM_REGIMES) + [24, 32, 64])
    claims = _claims()
    # seg_tn: every regime in dW_ih with the narrow (2-byte) and with the wide image stores, and in dW_hh with the row remap
    for r in TN_REGIMES.values():
        for wide, remap in ((False, False), (True, False), (False, True)):
            assert claims.get(("tn", wide, remap, r)), ("unclaimed", wide, remap, r)
    for r in GEMM_REGIMES.values():
        assert claims.get(("gemm", False, False, r)), ("unclaimed", r)
    for remap in (False, True):                      # gemm32.hip's padded rows, with and without the msplit remap
        assert claims.get(("gemm32", False, remap, GEMM32_REGIMES[64])), remap
    for r in CONV_REGIMES:
        assert claims.get(("conv", False, False, r)), ("unclaimed", r)
    # the wide-GRU path (no remap in dW_hh, two tiles a chunk) and the CSR rows at the body-then-tail split-K
    assert [c for c in claims[("tn", False, False, TN_REGIMES[24])] if c[3] == 200] and [c for c in claims[("tn", False, True, TN_REGIMES[24])] if c[4]]
    # the one-pass mode's 16-wave rows on the narrow ladder
    rows16 = [fc.conv_rows(*fc.NARROW[:1], fc.LADDER_T, B, fc.NARROW[1], "f16") for B in fc.LADDER_B]
    assert rows16 == [6, 8, 13, 17, 20, 24, 25, 28, 30, 33, 45, 54, 57, 65, 96, 97, 129, 160, 162, 193]
    rows12 = [fc.conv_rows(*fc.NARROW[:1], fc.LADDER_T, B, fc.NARROW[1], "f32") for B in fc.LADDER_B]
    assert rows12 == [8, 11, 17, 22, 27, 32, 34, 38, 40, 44, 60, 72, 75, 87, 128, 130, 172, 214, 215, 256]
    assert rows12 == [fc.conv_rows(*fc.WIDE[:1], fc.LADDER_T, B, fc.WIDE[1], "f16x3") for B in fc.LADDER_B]
    assert len(fc.CASES) == 158 and len(fc.SHAPES) == 46 and all(c[1] * c[2] <= fc.ROWS_MAX for c in fc.CASES)


def test_what_the_nine_legacy_shapes_reached():
    """The gap on record: the shapes of the two older finish tests reach seg_tn at split-K 1, 3, 6 and 96 only, seg_plain at 1, 3
    (gemm.hip) and 96 (gemm32.hip, no remap), ten conv_rows none of which puts the tail behind the body, and the wide stores
    in the flat branch alone."""
    tn, gemm, gemm32, rows, wide = set(), set(), set(), set(), set()
    for S, T, B, H, csr in fc.LEGACY_SHAPES:
        for math in fc.LEGACY_MODES:
            Sd = min(S, 64) if csr else S                                       # (sk comes from B*T and the tile counts alone)
            seg = fc.segments(Sd, T, B, H, math) if not csr else None
            if csr:
                i = _lib().tn_split(_lib().Dims(B, T, S, 13, H, MATH[math], 1, 6 * S, 0), state=False)
                (tn if math != "f32" else gemm).update({i.sk_ih, i.sk_hh})
                rows.add(fc.CSR_ROWS)
                continue
            for k in ("ih", "hh"):
                {"tn": tn, "gemm": gemm, "gemm32": gemm32}[seg[k]["family"]].add(seg[k]["sk"])
                if seg[k]["family"] == "gemm32":
                    assert not seg[k]["remap"]
            rows.add(seg["conv_rows"])
            if seg["wide"]:
                wide.add(((S, T, B, H), seg["ih"]["sk"]))
    assert tn == {1, 3, 6, 96} and gemm == {1, 3} and gemm32 == {96}
    assert rows == {1, 2, 3, 4, 5, 15, 20, 24, 32, 256}                        # (3 and 15: the one-pass mode's 16 waves)
    assert max(r for r in rows if r != 256) == 32 and {fc.conv_regime(r) for r in (32, 256)} == {(1, 1, "none"), (2, 2, "none")}
    assert not any(fc.tail_follows_body(fc.conv_trips(r)) for r in rows) and not any(fc.tail_follows_body(fc.tn_trips(sk)) for sk in tn)
    assert wide == {((4, 3, 5, 4), 1), ((8, 5, 9, 12), 1), ((20, 4, 6, 200), 1), ((28, 6, 40, 100), 3)}      # all in the flat branch
    legacy = {fc.tn_regime(sk) for sk in tn}
    assert sorted(sk for sk, r in TN_REGIMES.items() if r not in legacy) == [2, 4, 5, 7, 8, 16, 24, 40]


# ---- 3. the inputs ----------------------------------------------------------------------------------------------------------------
def _gi_max(d):
    from oracle import windgnn_oracle as orc
    _, cache = orc.forward(d.A.double(), d.X.double(), {k: v.double() for k, v in d.p.items()})
    return float(cache["GI"].abs().max())


def largest_shift(shape, seed):
    """The largest shift <= 0 on gru.weight_ih_l0 that brings max |GI| of the draw below fc.GI_MAX."""
    S, T, B, H, csr = shape
    gi0 = _gi_max(li.draw.__wrapped__(S, T, B, H, csr, 0, seed))
    if gi0 < fc.GI_MAX:
        return 0
    shift = min(0, 1 - pymath.ceil(pymath.log2(gi0 / fc.GI_MAX)))
    while not _gi_max(li.draw.__wrapped__(S, T, B, H, csr, shift, seed)) < fc.GI_MAX:
        shift -= 1
    return shift


def seed_figures(shape, seed, bar):
    """(the seed's largest shift, why its draw at that shift does not qualify: invariants (b), (d) and (f))."""
    S, T, B, H, csr = shape
    shift = largest_shift(shape, seed)
    d = li.draw.__wrapped__(S, T, B, H, csr, shift, seed)
    Zs, _ = li.preacts(d.A, d.X, d.p["conv1.weight"], d.p["conv1.bias"], d.p["conv2.weight"], d.p["conv2.bias"])
    why = []
    for layer, r in enumerate(li.measure(Zs, tli.STEPS), 1):
        if not r["margin"] > tli.MARGIN:
            why.append("(b): layer %d margin %.1e" % (layer, r["margin"]))
        if not r["varies"] >= tli.LIVENESS:
            why.append("(d): layer %d mask varies %.2f" % (layer, r["varies"]))
    if not why:
        why += ["(f): '%s' moves %.2g, not more than %.2g" % (name, e, 100 * bar)
                for name, e in li.mutation_effects(d.A, d.X, d.L, d.p).items() if not e > 100 * bar]
    return shift, why


def _bar(shape):
    S, T, B, H, csr = shape
    return tli._fp32_grade_bar((S, T, B, H, {(m, "f32") for m in fc.modes_of(shape) if m != "f16"}))


def test_the_input_table_is_what_the_rules_give():
    assert set(fc.INPUTS) == set(fc.SHAPES) and len(set(fc.SHAPES)) == len(fc.SHAPES)
    for shape in fc.SHAPES:
        shift, seed = fc.inputs_of(shape)
        assert 0 <= seed < fc.SEEDS
        for s in range(seed):
            assert seed_figures(shape, s, _bar(shape))[1], (shape, "seed %d already qualifies" % s)
        got, why = seed_figures(shape, seed, _bar(shape))
        assert (got, why) == (shift, []), (shape, got, why)
    # seeds other than 0 only where f16x3g's single-plane bar (1e-3 from 4096 rows) makes invariant (f) ask for 0.1
    assert {s: v for s, v in fc.INPUTS.items() if v[1]} == {(5, 2, 2049, 9, False): (-2, 7)}


# ---- 4. planted mistakes, on the oracle alone --------------------------------------------------------------------------------
def fold(parts, trips, stride, body_stride, plant=None, phase=0):
    """Sum parts[0 .. n) as a phased reduction of finish.hip does (fp64: the order does not matter here, the SET of indices does):
    every phase its body trips and its tail; plant = PLANTS[0] / [2] leaves out what the tail loops sum where a body ran before
    them, PLANTS[1] adds the last index of `phase` a second time."""
    n = parts.shape[0]
    idx = list(range(n))
    if plant in (fc.PLANTS[0], fc.PLANTS[2]):
        drop = set()
        for ph, (b, t) in enumerate(trips):
            if b:
                drop |= {ph + b * body_stride + k * stride for k in range(t)}
        idx = [i for i in idx if i not in drop]
    elif plant == fc.PLANTS[1]:
        idx.append(fc.last_of_phase(trips, stride, body_stride, phase))
    return parts[torch.tensor(idx, dtype=torch.long)].sum(0)


def chunk_partials(walk, kchunk, sk):
    """[sk][M][N + 1]: the partial of K chunk z = rows [z kchunk, (z + 1) kchunk) of Aop^T [Bop | 1]; chunks past the rows are zeros."""
    Aop, Bop = walk.Aop, torch.cat([walk.Bop, torch.ones(walk.Bop.shape[0], 1, dtype=walk.Bop.dtype)], 1)
    out = torch.zeros(sk, Aop.shape[1], Bop.shape[1], dtype=Aop.dtype)
    for z in range(sk):
        lo, hi = z * kchunk, min((z + 1) * kchunk, Aop.shape[0])
        if lo < hi:
            out[z] = Aop[lo:hi].t() @ Bop[lo:hi]
    return out


def conv_partials(gcn, waves, rows):
    """[rows][4 tensors flattened]: the partial row of workgroup r = the tiles t with (t % (waves rows)) // waves == r, each
    tile's contribution as orc.gcn2_backward forms it."""
    A, p, cache, dg = gcn
    B, T, S, F = dg.shape
    dZ2 = (dg * (cache["g"].reshape(B, T, S, F) > 0).to(dg.dtype)).reshape(B * T, S, F)
    dH1 = torch.matmul(A.t(), torch.matmul(dZ2, p["conv2.weight"].t()))
    dZ1 = dH1 * (cache["H1"].reshape(B * T, S, F) > 0).to(dg.dtype)
    per_tile = torch.cat([torch.matmul(cache["P1"].reshape(B * T, S, F).transpose(1, 2), dZ1).reshape(B * T, -1), dZ1.sum(1),
                          torch.matmul(cache["P2"].reshape(B * T, S, F).transpose(1, 2), dZ2).reshape(B * T, -1), dZ2.sum(1)], 1)
    row = (torch.arange(B * T) % (waves * rows)) // waves
    return torch.zeros(rows, per_tile.shape[1], dtype=dg.dtype).index_add_(0, row, per_tile)


def _conv_split(v, F=13):
    return {"conv1.weight": v[:F * F].reshape(F, F), "conv1.bias": v[F * F:F * F + F], "conv2.weight": v[F * F + F:2 * F * F + F].reshape(F, F),
            "conv2.bias": v[2 * F * F + F:]}


@functools.lru_cache(maxsize=2)
def _oracle_step(shape):
    S, T, B, H, csr = shape
    shift, seed = fc.inputs_of(shape)
    d = li.draw(S, T, B, H, csr, shift, seed)
    fig, grads, walks, gcn = tn_step(dict(A=d.A, X=d.X, L=d.L, p=d.p), 224, 224)
    _, _, g64 = li.fp64_step(d.A, d.X, d.L, d.p)
    assert max(rel_to_max(grads[k], g64[k]) for k in PARAM_KEYS) < 1e-12, shape
    return grads, walks, gcn


def plant_effects(shape, math):
    """{(plant, segment): (effect, live)} of one case, on the oracle: effect = the largest move of a gradient of the segment
    relative to its tensor's maximum; live = the planted indices hold rows (a dropped or doubled chunk of zeros moves nothing:
    the TN splitter rounds kchunk up to 32 rows, so the last of the split-K chunks may be empty)."""
    S, T, B, H, csr = shape
    seg = fc.segments(S, T, B, H, math, csr)
    grads, walks, gcn = _oracle_step(shape)
    out = {}
    for k, role, wk, bk in (("ih", "dW_ih", "gru.weight_ih_l0", "gru.bias_ih_l0"), ("hh", "dW_hh", "gru.weight_hh_l0", "gru.bias_hh_l0")):
        s = seg[k]
        parts = chunk_partials(walks[role], s["kchunk"], s["sk"])
        whole = parts.sum(0)
        assert rel_to_max(whole[:, :-1], grads[wk]) < 1e-12 and rel_to_max(whole[:, -1], grads[bk]) < 1e-12, (shape, math, k)
        if s["family"] != "tn":
            assert not fc.tail_follows_body(s["trips"])
            continue
        if s["trips"] is None:
            continue
        move = lambda P: max(rel_to_max(P[:, :-1], whole[:, :-1]), rel_to_max(P[:, -1], whole[:, -1]))
        assert move(fold(parts, s["trips"], 4, 16)) < 1e-12
        if fc.tail_follows_body(s["trips"]):
            live = any(z < s["chunks"] for z in fc.tail_chunks(s["trips"], 4, 16))
            out[(fc.PLANTS[0], k)] = (move(fold(parts, s["trips"], 4, 16, fc.PLANTS[0])), live)
        twice = [(move(fold(parts, s["trips"], 4, 16, fc.PLANTS[1], ph)), fc.last_of_phase(s["trips"], 4, 16, ph) < s["chunks"]) for ph in range(4)]
        lives = [e for e, live in twice if live]
        out[(fc.PLANTS[1], k)] = (min(lives), True) if lives else (max(e for e, _ in twice), False)
    if not csr:
        trips = fc.conv_trips(seg["conv_rows"])
        rows = conv_partials(gcn, fc.conv_waves(S, T, B, H, math), seg["conv_rows"])
        conv = [kk for kk in PARAM_KEYS if kk.startswith("conv")]
        whole = _conv_split(fold(rows, trips, 8, 32))
        assert max(rel_to_max(whole[kk], grads[kk]) for kk in conv) < 1e-12, (shape, math)
        if fc.tail_follows_body(trips):
            got = _conv_split(fold(rows, trips, 8, 32, fc.PLANTS[2]))
            out[(fc.PLANTS[2], "conv")] = (max(rel_to_max(got[kk], whole[kk]) for kk in conv), True)
    return out


# B*T -> the plants that fall on empty chunks there.  The TN splitter rounds kchunk up to whole stages of 32 rows, so the last of
# the split-K chunks may start past the rows and hold zeros: at 1552 rows (split-K 24, kchunk 96) 17 chunks hold rows -- the
# tail's chunk 16 does, the phases' last chunks 20 .. 23 do not; at 2580 (split-K 40) 27 do and the whole tail (32 .. 39) sums zeros.
# B = 768 and 1280 are the same two regimes with every chunk live (kchunk = 64 exactly), as are all rungs below split-K 16.
EMPTY_PLANTS = {1040: {fc.PLANTS[1]}, 1552: {fc.PLANTS[1]}, 2060: {fc.PLANTS[1]}, 2580: {fc.PLANTS[0], fc.PLANTS[1]}, 3080: {fc.PLANTS[1]},
                4098: {fc.PLANTS[1]}, 4200: {fc.PLANTS[1]}}


@pytest.mark.parametrize("shape", fc.SHAPES, ids=["S%d-T%d-B%d-H%d%s" % (s[:4] + ("-csr" if s[4] else "",)) for s in fc.SHAPES])
def test_the_inputs_can_tell_the_planted_mistakes(shape):
    bad, seen = [], set()
    for math in fc.modes_of(shape):
        eff = plant_effects(shape, math)
        key = tuple(sorted((k, round(e, 12)) for k, (e, _) in eff.items()))
        if key in seen:
            continue                                 # (f16x3g below 4096 rows, and f16 where its rows are f16x3's: the same sums)
        seen.add(key)
        for (plant, k), (e, live) in sorted(eff.items()):
            print("S%d T%d B%d H%d %s %s: '%s' moves a gradient by %.2e of max%s" % (shape[:4] + (math, k, plant, e, "" if live else " (empty chunks)")))
            if not live:
                if plant not in EMPTY_PLANTS.get(shape[1] * shape[2], ()) or e != 0.0:
                    bad.append("%s %s %s: '%s' falls on empty chunks and EMPTY_PLANTS does not say so" % (shape, math, k, plant))
            elif plant in EMPTY_PLANTS.get(shape[1] * shape[2], ()):
                bad.append("%s %s %s: '%s' is live, EMPTY_PLANTS says it is not" % (shape, math, k, plant))
            elif not e > fc.PLANT_FACTOR * BAR:
                bad.append("%s %s %s: '%s' moves no gradient by more than %.1e of max: pick another draw" % (shape, math, k, plant, e))
    assert bad == []


def test_every_body_plus_tail_regime_has_a_case_with_live_plants():
    """Every regime in which a tail follows an unrolled body is claimed by a case on which all of its planted mistakes fall on
    chunks (rows) that hold data -- and the fold notices a mistake at all."""
    need = {("tn", TN_REGIMES[24]): set(), ("tn", TN_REGIMES[40]): set()}
    for S, T, B, H, csr, math in fc.CASES:
        seg = fc.segments(S, T, B, H, math, csr)
        for k in ("ih", "hh"):
            s = seg[k]
            if (s["family"], s["regime"]) in need and s["chunks"] == s["sk"]:
                need[(s["family"], s["regime"])].add((B, k))
    assert need[("tn", TN_REGIMES[24])] == {(768, "ih"), (768, "hh")} and need[("tn", TN_REGIMES[40])] == {(1280, "ih"), (1280, "hh")}
    assert {r for r, v in EMPTY_PLANTS.items() if fc.PLANTS[0] in v} == {2580}
    g = torch.Generator().manual_seed(3)
    parts = torch.rand(24, 3, 5, generator=g, dtype=torch.float64)
    assert rel_to_max(fold(parts, fc.tn_trips(24), 4, 16), parts.sum(0)) < 1e-14
    assert torch.equal(fold(parts, fc.tn_trips(24), 4, 16, fc.PLANTS[0]), parts[:16].sum(0))
    assert rel_to_max(fold(parts, fc.tn_trips(24), 4, 16, fc.PLANTS[1], 2), parts.sum(0) + parts[22]) < 1e-14
    rows = torch.rand(38, 7, generator=g, dtype=torch.float64)
    assert rel_to_max(fold(rows, fc.conv_trips(38), 8, 32, fc.PLANTS[2]), rows[:32].sum(0)) < 1e-14
