"""The per-instance table of tests/instance_cases.py without a GPU: every instance key of every family is claimed by exactly
one case (or listed as unreachable, with the line of api.hip that excludes it), the integer lists of the table are the lists
in the launcher sources (extracted as text: a pattern that stops matching fails), and the Python selection formulas put every
case on the key it claims.  The library's host-only queries confirm what they can: it sizes a workspace for every case's
dims, refuses the refused ones, and its split-K counts are the formulas'.  The series half (SERIES_FAMILIES / SERIES_CASES) is
held to the same rules, and its inputs are measured on the fp64 oracle alone: tie-free, well conditioned in fp32, and able to
tell an off-by-one row.  The edge half of the recurrence families (EDGE_CASES) is re-derived -- every H the top of its
bracket, T odd and >= 5 -- and its inputs must tell three mistakes planted into a restated fp64 GRU.  The K-loop half of the two NT
GEMM families (KLOOP_CASES) likewise: nt_products() is held to plan(), every entry is re-derived -- on its key through the product
of the same role, seven K stages, dims by the rule -- and its inputs must tell three K-loop mistakes planted into the input
projection of a restated fp64 step."""
import ctypes
import os
import re

import pytest
import torch

import instance_cases as ic
from conftest import PARAM_KEYS, ROOT

CSRC = os.path.join(ROOT, "windgnn_amd", "csrc")
MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}
IO = {"f32": 0, "f16": 1, "bf16": 2}
# (T, B) of the cases: the plain pair, the first batch of gru.hip's recurrences, and the thresholds named above CASES
PLAIN_TB = {(2, 17), (3, 17), (2, 33)}          # (2, 33): one-pass fp16 cases grown once (see F16_EXCEPTIONS)
ALL_CASES = ic.CASES + ic.SERIES_CASES
THRESHOLD_TB = {(2, 769), (2, 2049), (2, 3073), (3, 1025), (3, 5473), (3, 8161), (24, 1537)}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, signature):
    """The text of the function whose definition starts with `signature`, up to its closing brace in column 0."""
    i = src.find(signature)
    assert i >= 0, "no %r in the source any more" % signature
    j = src.find("\n}\n", i)
    assert j > i, signature
    return src[i:j]


def _ints(pattern, text, what):
    found = re.findall(pattern, text)
    assert found, "the pattern for %s matches nothing any more: %r" % (what, pattern)
    return [int(x) for x in found]


def source_lists(read=_read):
    """name of a list of tests/instance_cases.py -> that list as the launcher sources have it."""
    gru, grux, small, gcnx, gcngi, gcn32, pgemm, gemm32 = (read(n + ".hip") for n in (
        "gru", "grux", "gru_small", "gcnx", "gcngi", "gcn32", "pgemm", "gemm32"))
    out = {}
    for name in ("FWD_KS", "BWD_KS3"):
        init = re.search(r"const int %s\[\] = \{([^}]*)\};" % name, gru)
        assert init, "no initialiser of %s in gru.hip any more" % name
        out["GRU_" + name] = [int(x) for x in init.group(1).split(",")]
    out["GRU_FWD_KS cases"] = _ints(r"FCASE\((\d+)\);", _body(gru, "int launch_gru_fwd("), "gru.hip FCASE")
    out["GRU_BWD_KS3 cases"] = _ints(r"BCASE\((\d+)\);", _body(gru, "int launch_gru_bwd("), "gru.hip BCASE")
    out["GRUX_FWD_K"] = _ints(r"case (\d+): FCASE\(\1\);", _body(grux, "int launch_grux_fwd("), "grux.hip FCASE")
    out["GRUX_BWD_K"] = _ints(r"case (\d+): BCASE\(\1\);", _body(grux, "int launch_grux_bwd("), "grux.hip BCASE")
    hmax = re.search(r"static int small_hmax\(int H\) \{ return ([^;]*); \}", small)
    assert hmax, "no one-line small_hmax in gru_small.hip any more"
    pairs = re.findall(r"H <= (\d+) \? (\d+) :", hmax.group(1))
    assert pairs and re.fullmatch(r"(?:H <= \d+ \? \d+ : )+\d+", hmax.group(1)), hmax.group(1)
    out["SMALL_HMAX_UPTO"] = [int(a) for a, _ in pairs]
    out["SMALL_HMAX"] = [int(b) for _, b in pairs] + [int(hmax.group(1).rsplit(":", 1)[1])]
    dispatch = _body(small, "#define SMALL_DISPATCH(KERNEL, ...)")
    out["SMALL_HMAX cases"] = (_ints(r"case (\d+): SMALL_GO\(KERNEL, \1,", dispatch, "gru_small.hip SMALL_GO")
                               + _ints(r"default: SMALL_GO\(KERNEL, (\d+),", dispatch, "gru_small.hip SMALL_GO default"))
    out["GCNX_NT"] = _ints(r"case (\d+): FWD_CASE\(\1\);", _body(gcnx, "int launch_gcnx2_fwd("), "gcnx.hip FWD_CASE")
    out["GCNX_NT bwd"] = _ints(r"case (\d+): BWD_CASE\(\1\);", _body(gcnx, "int launch_gcnx2_bwd("), "gcnx.hip BWD_CASE")
    out["GCNGI_NT"] = _ints(r"case (\d+): GG_CASE\(\1\);", _body(gcngi, "int launch_gcngi_fwd("), "gcngi.hip GG_CASE")
    out["GCN32_NT"] = _ints(r"case (\d+): FCASE\(\1\);", _body(gcn32, "int launch_gcn32_fwd("), "gcn32.hip FCASE")
    bwd32 = _body(gcn32, "int launch_gcn32_bwd(")
    out["GCN32_NT bwd"] = _ints(r"case (\d+): (?:BCASE\(\1\)|BLAUNCH\(\1, 12\));", bwd32, "gcn32.hip BCASE")
    out["GCN32 16 waves"] = _ints(r"case (\d+): BCASE\(\1\);", bwd32, "gcn32.hip BCASE")
    out["PGEMM_NT_T"] = _ints(r"NT_CASE\((\d+)\)", _body(pgemm, "int launch_pgemm_nt("), "pgemm.hip NT_CASE")
    out["PGEMM_TN_T"] = _ints(r"TN_CASE\((\d+)\)", _body(pgemm, "int launch_pgemm_tn("), "pgemm.hip TN_CASE")
    tn2 = _body(pgemm, "int launch_pgemm_tn2(")
    out["TN2_TI"] = _ints(r"TN2_ROW\((\d+)\)", tn2, "pgemm.hip TN2_ROW")
    out["TN2_TH"] = _ints(r"TN2_CASE\(ti, (\d+)\)", tn2, "pgemm.hip TN2_CASE")
    out["two-source A: T <="] = _ints(r"if constexpr \(T <= (\d+)\)", _body(pgemm, "static int launch_tn_t("), "pgemm.hip a2")
    nt32 = _body(gemm32, "int launch_gemm32_nt(")
    head, found, forms = nt32.partition("if (big) {")
    big, _, small32 = forms.partition("return WGNN_ERR_SHAPE;")
    assert found and "launch_nt_t<4, 2, t>" in big and "launch_nt_t<1, t, 1>" in small32
    out["GEMM32_NT_BIG_T"] = _ints(r"NT_CASE\((\d+)\)", big, "gemm32.hip NT_CASE (128 rows)")
    out["GEMM32_NT_SMALL_T"] = _ints(r"NT_CASE\((\d+)\)", small32, "gemm32.hip NT_CASE (32 rows)")
    out["GEMM32_TN_T"] = _ints(r"TN_CASE\((\d+)\)", _body(gemm32, "int launch_gemm32_tn("), "gemm32.hip TN_CASE")
    return out


def table_lists():
    """The same names from the table."""
    t = {n: getattr(ic, n) for n in ("GRU_FWD_KS", "GRU_BWD_KS3", "GRUX_FWD_K", "GRUX_BWD_K", "SMALL_HMAX_UPTO", "SMALL_HMAX",
                                     "GCNX_NT", "GCNGI_NT", "GCN32_NT", "PGEMM_NT_T", "PGEMM_TN_T", "TN2_TI", "TN2_TH",
                                     "GEMM32_NT_BIG_T", "GEMM32_NT_SMALL_T", "GEMM32_TN_T")}
    t["GRU_FWD_KS cases"], t["GRU_BWD_KS3 cases"] = ic.GRU_FWD_KS, ic.GRU_BWD_KS3
    t["SMALL_HMAX cases"], t["GCNX_NT bwd"], t["GCN32_NT bwd"] = ic.SMALL_HMAX, ic.GCNX_NT, ic.GCN32_NT
    t["GCN32 16 waves"] = sorted({int(re.search(r"<(\d+)>", k).group(1)) for k in ic.FAMILIES["gcn32_bwd_kernel"] if "w=16" in k})
    t["two-source A: T <="] = [max(int(re.search(r"<(\d+)", k).group(1)) for k in ic.FAMILIES["pgemm_tn_kernel"] if "a2=1" in k)]
    return t


def coverage_problems(cases):
    """What is wrong with `cases` (window-major and series cases together) as a cover of ic.FAMILIES and ic.SERIES_FAMILIES: a
    list of sentences, empty when every key is claimed once."""
    bad = []
    claimed = {}
    families = {fam: list(ic.FAMILIES.get(fam, ())) + list(ic.SERIES_FAMILIES.get(fam, ()))
                for fam in list(ic.FAMILIES) + [f for f in ic.SERIES_FAMILIES if f not in ic.FAMILIES]}
    for c in cases:
        fam, key = c[0], c[1]
        table = ic.SERIES_FAMILIES if c[-1] in ic.SERIES_ROUTES else ic.FAMILIES       # a case claims a key of its own table
        if ic.family_of(key) != fam or key not in table.get(fam, ()):
            bad.append("%s is no key of family %s" % (key, fam))
        if key in claimed:
            bad.append("%s is claimed twice" % key)
        claimed[key] = c
    for fam, keys in families.items():
        if len(set(keys)) != len(keys):
            bad.append("family %s lists a key twice" % fam)
        for key in keys:
            where = [n for n, d in (("CASES", claimed), ("UNREACHABLE", ic.UNREACHABLE), ("BEYOND_BUDGET", ic.BEYOND_BUDGET))
                     if key in d]
            if fam == "pgemm_tn2_kernel" and key not in ic.TN2_REQUIRED:
                continue                                           # all 28 pairs are not required (see below)
            if len(where) != 1:
                bad.append("%s is in %s" % (key, where or "no list"))
    for key in list(ic.UNREACHABLE) + list(ic.BEYOND_BUDGET):
        if not any(key in keys for keys in families.values()):
            bad.append("%s is excluded but no family lists it" % key)
    # the merged launch: every TI and every TH at least once per pass mode and per-window form, TI > TH and TI < TH among them
    for sfx in ("", ",x2", ",f16"):
        for pw in (0, 1):
            pairs = [tuple(int(x) for x in m.groups()) for m in
                     (re.fullmatch(r"pgemm_tn_kernel<(\d+)\+(\d+)%s>\|pw=%d" % (sfx, pw), k) for k in claimed) if m]
            if {a for a, _ in pairs} != set(ic.TN2_TI) or {b for _, b in pairs} != set(ic.TN2_TH):
                bad.append("merged launch %r pw=%d: not every TI and TH is run: %s" % (sfx, pw, pairs))
            if not any(a > b for a, b in pairs) or not any(a < b for a, b in pairs):
                bad.append("merged launch %r pw=%d: TI > TH and TI < TH must both occur" % (sfx, pw))
    return bad


def test_every_instance_key_is_claimed_by_exactly_one_case():
    assert coverage_problems(ALL_CASES) == []
    assert len(ALL_CASES) == len({c[1] for c in ALL_CASES})
    for fam, count in (("gru_fwd_kernel", 27), ("gru_bwd_kernel", 36), ("series_fold_kernel", 3)):
        assert len(ic.SERIES_FAMILIES[fam]) == count == len([c for c in ic.SERIES_CASES if c[0] == fam]), fam
    assert not {k for keys in ic.FAMILIES.values() for k in keys} & {k for keys in ic.SERIES_FAMILIES.values() for k in keys}
    assert set(ic.TN2_REQUIRED) <= set(ic.FAMILIES["pgemm_tn2_kernel"])


def test_the_integer_lists_are_those_of_the_launcher_sources():
    src, tab = source_lists(), table_lists()
    assert set(src) == set(tab)
    for name in src:
        assert src[name] == tab[name], (name, src[name], tab[name])
    # the name launch_gemm_f32 builds at run time
    assert '"gemm_f32_kernel<%d,%d>[%s%s%s]"' in _read("gemm.hip")
    for n in ic.GEMM_F32_NAMES:
        assert re.fullmatch(r"gemm_f32_kernel<(64|128),(64|128)>\[(kk|kn|tn)(,ones)?(,shift)?\]", n), n


def test_the_checks_notice_a_deleted_case_and_a_new_instantiation():
    for i in (0, len(ic.CASES) // 2, len(ic.CASES) - 1):
        assert coverage_problems(ic.CASES[:i] + ic.CASES[i + 1:] + ic.SERIES_CASES), ic.CASES[i]
    for i in range(len(ic.SERIES_CASES)):                        # every one of them: each is the only claim of its key
        gone = coverage_problems(ic.CASES + ic.SERIES_CASES[:i] + ic.SERIES_CASES[i + 1:])
        assert gone == ["%s is in no list" % ic.SERIES_CASES[i][1]], (ic.SERIES_CASES[i], gone)
    assert coverage_problems(ALL_CASES + [ic.CASES[0]]) and coverage_problems(ALL_CASES + [ic.SERIES_CASES[0]])
    assert coverage_problems(ic.CASES)                           # the window-major table alone no longer covers the keys
    moved = ("gru_fwd_kernel", "gru_fwd_kernel<4>|st=0") + ic.SERIES_CASES[0][2:]      # a series case claims no window-major key
    assert coverage_problems([c for c in ALL_CASES if c[1] != moved[1]] + [moved])

    def grown(name):                                             # gru.hip with one more entry in FWD_KS
        text = _read(name)
        return text.replace("26, 28, 32};", "26, 28, 32, 36};") if name == "gru.hip" else text
    assert grown("gru.hip") != _read("gru.hip")
    assert source_lists(grown)["GRU_FWD_KS"] != table_lists()["GRU_FWD_KS"]
    with pytest.raises(AssertionError):                          # a launcher that no longer reads as the pattern expects
        source_lists(lambda name: _read(name).replace("NT_CASE(", "NT_ROW("))


def test_selection_formulas_put_every_case_on_its_key():
    for fam, key, S, T, B, H, math, io, state, route in ic.CASES:
        assert ic.refusal(S, T, B, H, math, io) is None, key
        keys = ic.plan(S, T, B, H, math, io, state, route)
        assert key in keys, (key, keys)
        assert all(any(k in f for f in ic.FAMILIES.values()) for k in keys), (key, keys)
        assert not set(keys) & set(ic.UNREACHABLE), key
        # the shape rules: T = 2 or 3 and B = 17 unless a threshold selects; B = 1 (mod 16) always
        assert B % 16 == 1 and ((T, B) in PLAIN_TB or (T, B) in THRESHOLD_TB), key
        assert route in ic.ROUTES and not (state and route in ("fused", "infer")), key
    for key, (S, T, B, H, math) in ic.BEYOND_BUDGET.items():
        assert key in ic.plan(S, T, B, H, math), key
    # every H and S the fast kernels take selects an instance the launchers have
    for H in range(1, 129):
        assert ic.gru_fwd_k(H) in ic.GRU_FWD_KS and ic.gru_bwd_k(H) in ic.GRU_BWD_KS3 and ic.small_hmax(H) in ic.SMALL_HMAX
        if H <= 127:
            assert ic.grux_fwd_k(H) in ic.GRUX_FWD_K and ic.grux_bwd_k(H) in ic.GRUX_BWD_K
            assert ic.pgemm_tn_shape(H + 1)[1] in ic.TN2_TH
    for S in range(1, 65):
        assert ic.gcn_nt(S) in ic.GCNX_NT and ic.pgemm_tn_shape(13 * S + 1)[1] in ic.TN2_TI
        assert not ic.gcngi_supported(S, 4, False) or ic.gcn_nt(S) in ic.GCNGI_NT
        assert not ic.gcngi_supported(S, 4, True) or ic.gcngi_supported(S, 4, False)      # (the split modes' g rows are twice as long)


def test_no_call_form_reaches_an_excluded_key():
    """A grid over the thresholds of every selection: nothing plan() emits is listed as unreachable, and everything it emits
    is a key of a family.  The lines of api.hip the exclusions cite still say what they are cited for."""
    api = _read("api.hip").splitlines()
    for key, (why, line, word) in ic.UNREACHABLE.items():
        assert word in api[line - 1], (key, line, api[line - 1])
    allkeys = {k for keys in ic.FAMILIES.values() for k in keys}
    for T, B in sorted(PLAIN_TB | THRESHOLD_TB):
        for S in (1, 5, 17, 33, 34, 35, 49, 60, 64):
            for H in (4, 31, 64, 100, 127, 128, 129, 160, 225, 240):
                for math in ic.MATHS:
                    for io in ("f32", "bf16"):
                        if ic.refusal(S, T, B, H, math, io):
                            continue
                        for state, route in ((0, "train"), (0, "unmerged"), (0, "fused"), (0, "infer"), (1, "train"), (1, "unmerged")):
                            keys = set(ic.plan(S, T, B, H, math, io, bool(state), route))
                            assert keys <= allkeys and not keys & set(ic.UNREACHABLE), (S, T, B, H, math, io, state, route)


def test_the_library_accepts_every_case_and_splits_k_as_the_formulas_do():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    lib = L.load()
    seen = set()
    for fam, key, S, T, B, H, math, io, state, route in (ic.CASES + ic.KLOOP_CASES + ic.GEMM_F32_KLOOP_CASES
                                                          + [c[:10] for c in ic.GEMM_F32_FOLD_CASES]):
        dims = (S, T, B, H, math, io, state)
        if dims in seen:
            continue
        seen.add(dims)
        d = L.Dims(B, T, S, 13, H, MATH[math], 0, 0, IO[io])
        assert lib.wgnn_workspace_bytes(ctypes.byref(d)) > 0, key
        if math == "f32":
            continue
        i = L.tn_split(d, state=state)
        BT, I, G3 = B * T, 13 * S, 3 * H
        reg = H <= 127                                            # the register-resident recurrence: [dGI_r | dGI_z | pad | dGHn]
        m_hh = 8 * ic.cdiv(2 * H, 8) + 8 * ic.cdiv(H, 8) if reg else G3
        tiles_ih = ic.cdiv(G3, 320) * ic.pgemm_tn_shape(I + 1)[0]
        tiles_hh = ic.cdiv(m_hh, 320) * ic.pgemm_tn_shape(H + 1)[0]
        assert (i.sk_ih, i.sk_hh) == (ic.pick_splitk(BT, tiles_ih, 256, 64), ic.pick_splitk(BT, tiles_hh, 256, 64)), key
        assert i.merged == int(reg), key
    # refused by design: 16-bit I/O outside the fp16-plane family with the register-resident GRU, a dense graph above 64
    for S, T, B, H, math, io in ((1, 2, 17, 128, "f16", "bf16"), (1, 2, 17, 128, "f16x3", "f16"), (1, 2, 17, 4, "f32", "bf16"),
                                 (65, 2, 17, 4, "f16x3", "f32")):
        assert ic.refusal(S, T, B, H, math, io)
        assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(B, T, S, 13, H, MATH[math], 0, 0, IO[io]))) == 0


# ---- the series half of the table ------------------------------------------------------------------------------------------
FOLD_ZERO_ROWS = "series_fold_kernel|terms=0..1"
SHAPE_A = (2, 36, 3, 2, 17)          # (S, rows, T, stride, n): both layouts below gemm32's threshold
SHAPE_B = (2, 272, 16, 1, 257)       # the recurrence layout above it, the front layout below
TOPS = [4 * k for k in ic.GRU_FWD_KS]                                 # H with every k slot of the instance in use
BOTTOMS = [4] + [4 * k + 1 for k in ic.GRU_FWD_KS[:-1]]               # the first H of each instance


def test_series_plan_puts_every_series_case_on_its_key():
    allkeys = {k for keys in list(ic.FAMILIES.values()) + list(ic.SERIES_FAMILIES.values()) for k in keys}
    for fam, key, S, H, rows, T, stride, n, seed, route in ic.SERIES_CASES:
        keys = ic.series_plan(S, H, rows, T, stride, n, route)
        assert key in keys and set(keys) <= allkeys and not set(keys) & set(ic.UNREACHABLE), (key, keys)
        assert [k for k in keys if "|series|" in k or k.startswith("series_fold")] == \
            [k for k in keys if any(k in f for f in ic.SERIES_FAMILIES.values())], key
        assert (n - 1) * stride + T <= rows and route in ic.SERIES_ROUTES, key
        if key == FOLD_ZERO_ROWS:
            assert stride > T, key
            continue
        # the shape rules: n = 1 (mod 16), one of the two shapes, H at the top (A) or at the bottom (B) of its instance's range
        assert n % 16 == 1 and (S, rows, T, stride, n) in (SHAPE_A, SHAPE_B), key
        assert H in (TOPS if (S, rows, T, stride, n) == SHAPE_A else BOTTOMS), key
        assert ("dGHn" in key) == ((S, rows, T, stride, n) == SHAPE_B) or fam != "gru_bwd_kernel", key
    # shape A: a ragged second workgroup with one window, coverage 1 and 2, one spare row; shape B: on the two sides of 4096
    S, rows, T, stride, n = SHAPE_A
    assert n == 16 + 1 and rows == (n - 1) * stride + T + 1 and n * T < 4096 and ic.fold_terms(T, stride) == "1..2"
    S, rows, T, stride, n = SHAPE_B
    assert n % 16 == 1 and rows < 4096 <= n * T and (n - 16) * T < 4096 and ic.fold_terms(T, stride) == "T"   # the first such n
    assert TOPS == [16, 32, 48, 64, 80, 96, 104, 112, 128] and BOTTOMS == [4, 17, 33, 49, 65, 81, 97, 105, 113]
    for Ht, Hb, K, K3 in zip(TOPS, BOTTOMS, ic.GRU_FWD_KS, ic.GRU_BWD_KS3):
        assert ic.gru_fwd_k(Ht) == ic.gru_fwd_k(Hb) == K and ic.gru_bwd_k(Ht) == ic.gru_bwd_k(Hb) == K3
    # the two layouts decide apart: each product follows the row count of its own layout
    for rows, nT, want in ((4095, 4095, (0, 0)), (4096, 2048, (1, 0)), (2050, 4096, (0, 1)), (4097, 8192, (1, 1))):
        keys = ic.series_plan(7, 21, rows, 2, 1 if nT >= rows - 1 else 2, nT // 2, "series")
        assert ("gemm32_nt_kernel<32x64>" in keys, "gru_bwd_kernel<24>|series|dY|dGHn" in keys) == tuple(map(bool, want)), keys
        assert ("gemm32_tn_kernel<3>|a2=0" in keys, "gemm32_tn_kernel<1>|a2=1" in keys) == tuple(map(bool, want)), keys


def test_series_plan_decides_where_the_sources_do():
    gemm32, api, series, gru = (_read(n + ".hip") for n in ("gemm32", "api", "series", "gru"))
    nt = re.search(r"bool gemm32_nt_supported\(size_t BT, int Kp_f, int Kp_b\) \{\s*return ([^;]*);", gemm32)
    assert nt and nt.group(1) == "BT >= 4096 && Kp_f % 32 == 0 && Kp_b % 32 == 0 && Kp_f <= 512 && Kp_b <= 512", nt
    assert "bool gemm32_tn_supported(size_t BT) { return BT >= 4096; }" in gemm32
    assert ic.g32_rows(4096, 39, 128) and not ic.g32_rows(4095, 1, 4) and not ic.g32_rows(1 << 20, 40, 4)
    assert "constexpr int MB = 16;" in gru                         # 16 windows per workgroup: n = 1 (mod 16) is ragged
    # series mode never takes gru_small, and each layout is made with its own row count
    assert "L.small = !x3 && !L.gen_gru && !series && gru_small_supported(d->B, d->H);" in api
    assert "L.dghn = (x3 && !L.gen_gru) || (L.rec32 && L.g32tn);" in api
    assert "pl->front = wgnn_dims{1, sd->rows, sd->S," in series and "pl->rec = wgnn_dims{sd->n, sd->T, sd->S," in series
    # the launch order of series_bwd, and which layout each part runs on
    bwd = _body(api, "int series_bwd(")
    order = ["launch_gru_bwd(a, br.st)", "bwd_weights(br, WGNN_ROWS_HH", "launch_series_fold(br.dGI",
             "bwd_weights(bf, WGNN_ROWS_IH", "bwd_dg(bf)"]
    at = [bwd.find(x) for x in order]
    assert min(at) >= 0 and at == sorted(at), at
    assert "a.B = dr->B; a.T = dr->T; a.H = dr->H;" in bwd[:at[0]]         # BPTT runs on the rec layout's dims
    assert "a.dGHn = Lr.dghn ? br.dGH : nullptr; a.dGH = Lr.dghn ? nullptr : br.dGH;" in bwd
    fwd = _body(api, "int series_fwd(")
    assert "fwd_front(f)" in fwd and "a.hprev = sr && Lr.g32tn ? sr + Lr.st_hprev : nullptr;" in fwd
    # both launch_gru_fwd calls (last_only and Y) pass the stride: the one request they share takes the caller's map first
    go = [m.start() for m in re.finditer(re.escape("return launch_gru_fwd(a, f.st);"), fwd)]
    assert fwd.count("launch_gru_fwd(") == 2 == len(go) and fwd.count("GruFwdArgs a") == 1
    assert fwd.count("a.map = c.map;") == 1 and 0 <= fwd.find("a.map = c.map;") < go[0] and "a.map.stride" not in fwd
    assert bwd.count("a.map = c.map;") == 1 and 0 <= bwd.find("a.map = c.map;") < at[0] and "a.map.stride" not in bwd
    assert series.count("c.map.stride = sd->stride;") == 1 and "map.stride =" not in series.replace("c.map.stride = sd->stride;", "")
    # a non-zero stride selects the SeriesRows instances, under the window-major instances' names
    assert gru.count("if (m.stride) gru_fwd_go<K, false>(a, st, SeriesRows{m.stride});") == 1
    assert gru.count("if (m.stride) gru_bwd_go<K>(a, inv_n, coef, st, SeriesRows{m.stride});") == 1
    assert gru.count("const SeriesMap& m = a.map;") == 2
    assert 'PROF_LAUNCH("gru_fwd_kernel<" #K ">"' in gru and 'PROF_LAUNCH("gru_bwd_kernel<" #K ">"' in gru
    for d in ("fwd", "bwd"):                                       # ... and that name is the one the stride branch launches under
        assert re.search(r'PROF_LAUNCH\("gru_%s_kernel<" #K ">", fl, by, st, +\\\n +if \(m\.stride\) gru_%s_go<K' % (d, d), gru), d
    assert 'PROF_LAUNCH("series_fold_kernel"' in series
    assert "if (sd->rows < 1 || sd->T < 1 || sd->stride < 1" in series         # no entry point passes a zero stride on


def test_the_library_accepts_every_series_case():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    lib = L.load()
    for fam, key, S, H, rows, T, stride, n, seed, route in ic.SERIES_CASES:
        sd = L.SeriesDims(rows, T, stride, n, S, 13, H, 0, 0, 0, 0)
        for size in (lib.wgnn_series_workspace_bytes, lib.wgnn_series_stash_bytes, lib.wgnn_series_loss_bytes):
            assert size(ctypes.byref(sd)) > 0, key
    # ... and refuses H past the register-resident recurrence, which series_plan refuses too
    assert lib.wgnn_series_workspace_bytes(ctypes.byref(L.SeriesDims(36, 3, 2, 17, 2, 13, 129, 0, 0, 0, 0))) == 0
    with pytest.raises(AssertionError):
        ic.series_plan(2, 129, 36, 3, 2, 17, "series")


def _series_shapes():
    """The distinct (S, H, rows, T, stride, n, seed) of the series cases, in table order."""
    return list(dict.fromkeys(c[2:9] for c in ic.SERIES_CASES))


def input_problems(shape):
    """What is wrong with the inputs of a series shape, measured on the reference alone: a list of sentences."""
    from oracle import windgnn_oracle as orc
    from test_gpu_series_instances import reference
    from test_gpu_series import TOL
    from conftest import PARAM_KEYS, rel_to_max
    r = reference(*shape)
    if not r.margin > 1e-5:                                       # the series suites' tie rule
        return ["%s: a ReLU pre-activation within %.1e of zero (relative): pick another seed" % (shape, r.margin)]
    # the oracle in fp32 against itself in fp64: a draw on which rounding alone costs a tenth of the bar proves nothing
    Y32, cache = orc.forward(r.A, r.X, r.p)
    g32 = orc.backward(r.A, r.X, r.p, Y32, cache, r.dY)
    _, loss32, m32 = orc.train_step(r.A, r.X, r.L, r.p)
    gap = {"Y": rel_to_max(Y32, r.Yo), "loss": abs(float(loss32) - r.loss_o) / r.loss_o}
    for k in PARAM_KEYS:
        gap[k] = max(rel_to_max(g32[k], r.go[k]), rel_to_max(m32[k], r.gm[k]))
    worst = max(gap, key=gap.get)
    print("%s: margin %.1e, fp32 against fp64 at most %.1e (%s)" % (shape, r.margin, gap[worst], worst))
    return ["%s: %s in fp32 is %.1e off the fp64 oracle: pick another seed" % (shape, k, e) for k, e in gap.items() if e > TOL / 10]


def test_series_inputs_are_tie_free_and_well_conditioned():
    shapes = _series_shapes()
    assert len(shapes) == 9 + 9 + 1
    for shape in shapes:
        assert input_problems(shape) == []
    # the check notices a seed with a ReLU tie: shape B at H = 17 with seed 0 has a pre-activation 2e-6 (relative) from zero
    tied = (2, 17) + SHAPE_B[1:] + (0,)
    assert tied not in shapes and "ReLU" in input_problems(tied)[0]


def test_series_inputs_can_tell_an_off_by_one_row():
    """On the oracle alone, per shape of a series_mse case.  (a) Labels read one series row late move the loss and some gradient
    by more than 100 TOL (the SPARE row behind the last covered hour alone does).  (b) Windows started one hour late move Y, the
    de-normalised last rows and some gradient of the signed random dY by more than 100 TOL.  The MSE of (b) is printed, not
    asserted: against independent uniform labels it is the labels' own variance, and measured 1e-5 ... 2e-2 of the loss."""
    from oracle import windgnn_oracle as orc
    from test_gpu_series_instances import reference, windows
    from test_gpu_series import TOL
    from conftest import PARAM_KEYS, rel_to_max
    from windgnn_amd.series import series_coverage
    shapes = list(dict.fromkeys(c[2:9] for c in ic.SERIES_CASES if c[9] == "series_mse"))
    assert len(shapes) == 18
    for shape in shapes:
        S, H, rows, T, stride, n, seed = shape
        r = reference(*shape)
        A, p64 = r.A.double(), {k: v.double() for k, v in r.p.items()}
        _, loss, g = orc.train_step(A, r.X.double(), windows(r.Ls, T, stride, n, first=1).double(), p64)
        lab = (abs(float(loss) - r.loss_o) / r.loss_o, max(rel_to_max(g[k], r.gm[k]) for k in PARAM_KEYS))
        Xl = windows(r.feat, T, stride, n, first=1).double()         # (feat has three more hours than the series)
        Yl, cache = orc.forward(A, Xl, p64)
        gl = orc.backward(A, Xl, p64, Yl, cache, r.dY.double())
        _, loss_l, _ = orc.train_step(A, Xl, r.L.double(), p64)
        late = (rel_to_max(Yl, r.Yo), rel_to_max(Yl[:, -1], r.Yo[:, -1]), max(rel_to_max(gl[k], r.go[k]) for k in PARAM_KEYS))
        print("%s: labels one row late: loss %.1e grad %.1e; windows one hour late: Y %.1e last %.1e grad %.1e (loss %.1e)"
              % ((shape,) + lab + late + (abs(float(loss_l) - r.loss_o) / r.loss_o,)))
        assert min(lab) > 100 * TOL and min(late) > 100 * TOL, (shape, lab, late)
    # the fold's zero-row case: some hour inside the windows' span really is covered by no window
    fam, key, S, H, rows, T, stride, n, seed, route = next(c for c in ic.SERIES_CASES if c[1] == FOLD_ZERO_ROWS)
    cover = series_coverage(rows, T, stride, n)
    assert any(lo > hi for lo, hi in cover[:(n - 1) * stride + T]) and ic.fold_terms(T, stride) == "0..1"
    assert {hi - lo + 1 for lo, hi in series_coverage(*SHAPE_A[1:])[2:-1]} == {1, 2}


# ---- the edge half of the recurrence families ------------------------------------------------------------------------------
EDGE_B = {17: 17, 33: 33, 769: 769, 2049: 833}      # B of the key's CASES entry -> B of its edge case (see above EDGE_CASES)
Y_BAR = 1e-4                                         # the fp32-grade bar on Y (tests/test_gpu_parity.py Y_TOL), F16_Y_BAR the one-pass one
F16_Y_BAR = 2e-2


def edge_problems(edges):
    """What is wrong with `edges` as the edge half of the table: a list of sentences, empty when every key of the six recurrence
    families is claimed once, at the top of its bracket, at an odd T >= 5 and B = 1 (mod 16) by the rule."""
    bad = []
    base = {c[1]: c for c in ic.CASES if c[0] in ic.EDGE_FAMILIES}
    want = [k for fam in ic.EDGE_FAMILIES for k in ic.FAMILIES[fam]]
    assert sorted(base) == sorted(want)                           # (CASES claims every recurrence key: none is unreachable)
    claimed = [c[1] for c in edges]
    for key in want:
        if claimed.count(key) != 1:
            bad.append("%s is claimed %d times in EDGE_CASES" % (key, claimed.count(key)))
    for fam, key, S, T, B, H, math, io, state, route in edges:
        if key not in base:
            bad.append("%s is no key of a recurrence family" % key)
            continue
        _, _, S0, T0, B0, H0, math0, io0, state0, route0 = base[key]
        if (fam, S, math, io, state, route) != (base[key][0], S0, math0, io0, state0, route0):
            bad.append("%s: family, S, math, io, state and route are not those of its case in CASES" % key)
            continue
        if ic.refusal(S, T, B, H, math, io) is not None or key not in ic.plan(S, T, B, H, math, io, state, route):
            bad.append("%s: plan() at H = %d does not contain the key" % (key, H))
            continue
        if T < 5 or T % 2 == 0:
            bad.append("%s: T = %d is not odd and >= 5" % (key, T))
        elif T != ic.EDGE_T_OTHER.get((S, B, H), ic.EDGE_T):
            bad.append("%s: T = %d, the rule says %d" % (key, T, ic.EDGE_T_OTHER.get((S, B, H), ic.EDGE_T)))
        want_b = ic.EDGE_B_MOVED.get(key, EDGE_B[B0])
        if B % 16 != 1 or B != want_b:
            bad.append("%s: B = %d, the rule says %d" % (key, B, want_b))
        top = ic.bracket_top(key, S, T, B, math, io, state, route)
        beyond = H + 1 > ic.H_SCAN or ic.refusal(S, T, B, H + 1, math, io) is not None
        if H != top or not (beyond or key not in ic.plan(S, T, B, H + 1, math, io, state, route)):
            bad.append("%s: H = %d is not the top of its bracket (%s)" % (key, H, top))
        bottom = min(h for h in range(1, ic.H_SCAN + 1) if ic.refusal(S, T, B, h, math, io) is None
                     and key in ic.plan(S, T, B, h, math, io, state, route))
        if not (H > H0 or bottom == top):
            bad.append("%s: H = %d is not above the %d of its case in CASES" % (key, H, H0))
    return bad


def test_edge_cases_claim_every_recurrence_key_at_the_top_of_its_bracket():
    assert edge_problems(ic.EDGE_CASES) == []
    assert len(ic.EDGE_CASES) == 254 == sum(len(ic.FAMILIES[f]) for f in ic.EDGE_FAMILIES)
    assert len(_edge_shapes()) == 47 + 2 and ic.EDGE_T == 5 and ic.EDGE_T_OTHER == {(1, 17, 106): 7}
    assert [c[1] for c in ic.EDGE_CASES if c[3] != ic.EDGE_T] == ["gru_small_%s_kernel|hmax=108|st=%d" % (d, st)
                                                                 for d in ("fwd", "bwd") for st in (0, 1)]
    tops = lambda fam: sorted({c[5] for c in ic.EDGE_CASES if c[0] == fam})
    assert tops("grux_fwd_kernel") == [31, 63, 95, 127]
    assert tops("gru_fwd_kernel") == [4 * k for k in ic.GRU_FWD_KS] == tops("gru_bwd_kernel")
    assert tops("gru_small_fwd_kernel") == ic.SMALL_HMAX_UPTO + [128] == tops("gru_small_bwd_kernel")
    assert tops("grux_bwd_kernel") == [max(h for h in range(1, 128) if ic.grux_bwd_k(h) == k) for k in ic.GRUX_BWD_K]
    # the three thresholds B follows
    assert 5 * 833 >= 4096 > 5 * (833 - 16) and "L.small = !x3 && !L.gen_gru && !series && gru_small_supported(d->B, d->H);" in _read("api.hip")
    # only one-pass fp16 cases may leave B = 17 for more rows, to 33 or 65
    assert all(",f16>" in k and b in (33, 65) for k, b in ic.EDGE_B_MOVED.items()) and len(ic.EDGE_B_MOVED) == 2
    for c in ic.EDGE_CASES:
        assert (c[4] == 833) == any(w in c[1] for w in ("dGHn", "lo=0")), c[1]
        assert (c[4] == 769) == (c[0] in ("gru_fwd_kernel", "gru_bwd_kernel") and "dGHn" not in c[1]), c[1]
    # the library sizes a workspace for every edge shape
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    lib = L.load()
    for dims in dict.fromkeys((c[2:8]) for c in ic.EDGE_CASES):
        S, T, B, H, math, io = dims
        assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(B, T, S, 13, H, MATH[math], 0, 0, IO[io]))) > 0, dims


def test_the_edge_checks_notice_a_mis_tabled_entry():
    i = next(n for n, c in enumerate(ic.EDGE_CASES) if c[1] == "grux_bwd_kernel<10>|io=32|st=0|lo=1")

    def with_(**kw):
        c = dict(zip(("fam", "key", "S", "T", "B", "H", "math", "io", "state", "route"), ic.EDGE_CASES[i]))
        c.update(kw)
        return ic.EDGE_CASES[:i] + [tuple(c.values())] + ic.EDGE_CASES[i + 1:]
    H = ic.EDGE_CASES[i][5]
    assert H == 104
    assert edge_problems(with_(H=H - 1)) == ["grux_bwd_kernel<10>|io=32|st=0|lo=1: H = 103 is not the top of its bracket (104)"]
    assert edge_problems(with_(H=H + 1)) == ["grux_bwd_kernel<10>|io=32|st=0|lo=1: plan() at H = 105 does not contain the key"]
    assert edge_problems(with_(T=2)) == ["grux_bwd_kernel<10>|io=32|st=0|lo=1: T = 2 is not odd and >= 5"]
    assert edge_problems(with_(T=7)) == ["grux_bwd_kernel<10>|io=32|st=0|lo=1: T = 7, the rule says 5"]
    assert edge_problems(with_(T=6)) and edge_problems(with_(B=18)) and edge_problems(with_(B=33)) and edge_problems(with_(S=2))
    for j in (0, i, len(ic.EDGE_CASES) - 1):                      # a recurrence key left out, and one claimed twice
        gone = edge_problems(ic.EDGE_CASES[:j] + ic.EDGE_CASES[j + 1:])
        assert gone == ["%s is claimed 0 times in EDGE_CASES" % ic.EDGE_CASES[j][1]], gone
    assert edge_problems(ic.EDGE_CASES + [ic.EDGE_CASES[i]])
    assert edge_problems(ic.EDGE_CASES + [c for c in ic.CASES if c[0] == "gcnx_fwd_kernel"][:1])
    # a bracket of one width would be excused from "above the case in CASES", no other: the bottom-of-bracket entry is not
    assert edge_problems(ic.EDGE_CASES[:i] + [ic.EDGE_CASES[i][:3] + (5, 17, 97) + ic.EDGE_CASES[i][6:]] + ic.EDGE_CASES[i + 1:])


def _edge_shapes():
    """The distinct (S, T, B, H) of the edge cases, in table order."""
    return list(dict.fromkeys(c[2:6] for c in ic.EDGE_CASES))


def restated_gru(r, mistake=None):
    """Y of the fp64 GRU restated step by step on the oracle's own g, with one of three mistakes a recurrence kernel can make
    planted: 'parity' -- from t = 2 on the W_hh product reads h_{t-2} (the other parity's state buffer); 'column' -- hidden
    column H - 1 is dropped from the W_hh product; 'prefetch' -- on interior steps GI of step t + 1 is consumed at step t."""
    from oracle import windgnn_oracle as orc
    A, X, p = r["A"].double(), r["X"].double(), {k: v.double() for k, v in r["p"].items()}
    g, _ = orc.gcn2_forward(A, X, p)
    Wih, Whh, bih, bhh = (p["gru." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
    B, T, H = X.shape[0], X.shape[1], Whh.shape[1]
    GI = torch.matmul(g, Wih.t()) + bih
    hs = [torch.zeros(B, H, dtype=torch.float64)]                 # hs[t] = h_{t-1}
    for t in range(T):
        h = hs[t]
        hw = hs[t - 1] if (mistake == "parity" and t >= 2) else h
        if mistake == "column":
            gh = torch.matmul(hw[:, :H - 1], Whh[:, :H - 1].t()) + bhh
        else:
            gh = torch.matmul(hw, Whh.t()) + bhh
        gi = GI[:, t + 1] if (mistake == "prefetch" and 1 <= t <= T - 2) else GI[:, t]
        rg = torch.sigmoid(gi[:, 0:H] + gh[:, 0:H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + rg * gh[:, 2 * H:])
        hs.append((1.0 - z) * n + z * h)
    return torch.stack(hs[1:], 1)


def edge_input_problems(shape):
    """What is wrong with the inputs of an edge shape, measured on the oracle alone: a list of sentences."""
    from oracle import windgnn_oracle as orc
    from conftest import PARAM_KEYS, max_abs, rel_to_max
    from test_gpu_instances import _reference
    S, T, B, H = shape
    r = _reference(S, T, B, H, "f32", False)
    bad = []
    # the oracle in fp32 against itself in fp64: a draw on which rounding alone costs a tenth of the bar proves nothing
    Y32, _, g32 = orc.train_step(r["A"], r["X"], r["L"], r["p"])
    gap = {"Y": rel_to_max(Y32, r["Y"])}
    gap.update({k: rel_to_max(g32[k], r["grads"][k]) for k in PARAM_KEYS})
    bad += ["%s: %s in fp32 is %.1e off the fp64 oracle: pick another seed" % (shape, k, e) for k, e in gap.items() if e > 1e-5]
    # the restated GRU is the oracle's, bit for bit; each planted mistake moves Y by more than 10 fp32-grade bars
    assert torch.equal(restated_gru(r), r["Y"]), shape
    moved = {m: max_abs(restated_gru(r, m), r["Y"]) for m in ("parity", "column", "prefetch")}
    print("%s: seed %d, max|Y| %.2f, fp32 against fp64 at most %.1e; planted parity %.1e column %.1e prefetch %.1e "
          "(in one-pass bars of 2e-2: %.2f %.2f %.2f)" % ((shape, ic.param_seed(S, H), float(r["Y"].abs().max()), max(gap.values()))
                                                         + tuple(moved.values()) + tuple(v / F16_Y_BAR for v in moved.values())))
    bad += ["%s: the planted %s mistake moves Y by %.1e only: pick another seed" % (shape, m, v) for m, v in moved.items()
            if not v > 10 * Y_BAR]
    return bad


def test_edge_inputs_are_well_conditioned_and_can_tell_the_planted_mistakes():
    """Per distinct edge shape, on the oracle alone (the inputs are tests/test_gpu_instances.py's _reference draw, which the
    one-pass cases share with their f16x3 siblings): fp32 against fp64 within a tenth of the bar on Y and every gradient, and
    each planted mistake of restated_gru above 10 x 1e-4 on Y.  Against the one-pass bar of 2e-2 the mistakes are printed only."""
    shapes = _edge_shapes()
    assert len(shapes) == 49
    for shape in shapes:
        assert edge_input_problems(shape) == []


# ---- the K-loop half of the two NT GEMM families ---------------------------------------------------------------------------
G_BAR = 1e-3                                         # the widest fp32-grade gradient bar (single-plane f16x3g), F16_G_BAR the one-pass one
F16_G_BAR = 5e-2
ALL_WINDOW_TABLES = (("CASES", ic.CASES), ("EDGE_CASES", ic.EDGE_CASES), ("KLOOP_CASES", ic.KLOOP_CASES))


def _nt_keys(keys):
    return [k for k in keys if ic.family_of(k) in ic.NT_FAMILIES]


def test_nt_products_names_exactly_the_nt_launches_of_plan():
    """plan() is the authority for names; nt_products() restates its NT launches with their contraction.  For every case of
    every window-major table, and over a grid of the thresholds, the two give the same keys in the same order."""
    for name, table in ALL_WINDOW_TABLES:
        for fam, key, S, T, B, H, math, io, state, route in table:
            prods = ic.nt_products(S, T, B, H, math, io, state, route)
            assert [p[0] for p in prods] == _nt_keys(ic.plan(S, T, B, H, math, io, state, route)), (name, key)
            assert all(p[1] in ic.NT_ROLES and p[4] >= 1 for p in prods), (name, key, prods)
    for key, (S, T, B, H, math) in ic.BEYOND_BUDGET.items():
        assert [p[0] for p in ic.nt_products(S, T, B, H, math)] == _nt_keys(ic.plan(S, T, B, H, math)), key
    for T, B in sorted(PLAIN_TB | THRESHOLD_TB):
        for S in (1, 17, 34, 60):
            for H in (4, 74, 127, 128, 129, 225):
                for math in ic.MATHS:
                    for state, route in ((0, "train"), (0, "fused"), (0, "infer"), (1, "train"), (1, "unmerged")):
                        if ic.refusal(S, T, B, H, math, "f32"):
                            continue
                        prods = ic.nt_products(S, T, B, H, math, "f32", bool(state), route)
                        assert [p[0] for p in prods] == _nt_keys(ic.plan(S, T, B, H, math, "f32", bool(state), route)), (S, T, B, H, math, route)
    # the contraction: 32 columns a stage in both families, as the kernels count them
    assert "const int nk = Kp / 32;" in _read("pgemm.hip") and "const int nk = Kp / 32;" in _read("gemm32.hip")
    assert "const int nloop = FUSE_EPI ? nk - 1 : nk;" in _read("gemm32.hip")
    assert ic.nt_products(17, 2, 17, 74, "f16x3") == [("pgemm_nt_kernel<1>|out16=0|narrow", "GI", 34, 222, 7),
                                                       ("pgemm_nt_kernel<1>|out16=0|narrow", "dg", 34, 221, 7)]


def kloop_problems(kloops):
    """What is wrong with `kloops` as the K-loop half of the table: a list of sentences, empty when every key of the two NT GEMM
    families whose keyed product runs fewer than ic.KLOOP_STAGES stages in CASES is claimed once, on its key, through the product
    of the same role, at an odd count of at least ic.KLOOP_STAGES stages and at the rule's dims."""
    bad = []
    base = {c[1]: c for c in ic.CASES if c[0] in ic.NT_FAMILIES}
    claimed = [c[1] for c in kloops]
    bad += ["%s is claimed %d times in KLOOP_CASES" % (k, claimed.count(k)) for k in dict.fromkeys(claimed) if claimed.count(k) > 1]
    most = {key: ic.keyed_product(key, *c[2:])[3] for key, c in base.items()}      # the most stages the key's product runs anywhere
    for c in kloops:
        fam, key, S, T, B, H, math, io, state, route = c
        if key not in base:
            bad.append("%s is no key CASES claims for an NT GEMM family" % key)
            continue
        _, _, S0, T0, B0, H0, math0, io0, state0, route0 = base[key]
        if (fam, T, B, math, io, state, route) != (base[key][0], T0, B0, math0, io0, state0, route0):
            bad.append("%s: family, T, B, math, io, state and route are not those of its case in CASES" % key)
            continue
        if ic.refusal(S, T, B, H, math, io) is not None or key not in ic.plan(S, T, B, H, math, io, state, route):
            bad.append("%s: plan() at S = %d, H = %d does not contain the key" % (key, S, H))
            continue
        role0, _, _, stages0 = ic.keyed_product(key, *base[key][2:])
        if stages0 >= ic.KLOOP_STAGES:
            bad.append("%s: its case in CASES already runs %d K stages" % (key, stages0))
            continue
        mine = ic.keyed_product(key, S, T, B, H, math, io, state, route, role=role0)
        if mine is None:
            bad.append("%s: at S = %d, H = %d the key is not carried by the %s product that carries it in CASES" % (key, S, H, role0))
            continue
        stages = mine[3]
        if stages < ic.KLOOP_STAGES or stages % 2 == 0:
            bad.append("%s: the %s product runs %d K stages, not an odd count >= %d" % (key, role0, stages, ic.KLOOP_STAGES))
        want = (S0, ic.KLOOP_H) if role0 == "dg" else (ic.KLOOP_S, H0)
        if (S, H) != want:
            bad.append("%s: S = %d, H = %d, the rule says %d, %d" % ((key, S, H) + want))
        most[key] = max(most[key], stages)
    bad += ["%s runs at most %d K stages in CASES and KLOOP_CASES" % (k, n) for k, n in most.items() if n < ic.KLOOP_STAGES]
    return bad


def _kloop_shapes():
    """The distinct (S, T, B, H, io, state) of the K-loop cases, in table order, each with the roles of its keyed products."""
    out = {}
    for fam, key, S, T, B, H, math, io, state, route in ic.KLOOP_CASES:
        role = ic.keyed_product(key, *next(c for c in ic.CASES if c[1] == key)[2:])[0]
        out.setdefault((S, T, B, H, io, state), set()).add(role)
    return out


def test_kloop_cases_give_every_nt_key_a_k_loop_of_seven_stages():
    assert kloop_problems(ic.KLOOP_CASES) == []
    assert ic.KLOOP_STAGES == 7 and (ic.KLOOP_H, ic.KLOOP_S) == (74, 17) and ic.NT_BK == 32
    assert ic.rup(3 * ic.KLOOP_H, 32) == 7 * 32 == ic.rup(13 * ic.KLOOP_S + 1, 32) and 3 * ic.KLOOP_H == 222 == 13 * ic.KLOOP_S + 1
    # every reachable key of the two families is in CASES (the two BEYOND_BUDGET keys are the K-chunked form's), and no key
    # leaves the rule: kloop_problems() knows no exemption
    for fam in ic.NT_FAMILIES:
        assert {k for k in ic.FAMILIES[fam] if k not in ic.UNREACHABLE and k not in ic.BEYOND_BUDGET} == {c[1] for c in ic.CASES if c[0] == fam}
    # which half of which family needed the second case: by (family, wide-GRU path, role, stages of the CASES entry)
    census = {}
    for c in ic.CASES:
        if c[0] in ic.NT_FAMILIES:
            role, _, _, stages = ic.keyed_product(c[1], *c[2:])
            census.setdefault((c[0], c[5] > 127, role, stages), []).append(c[1])
    assert {k: len(v) for k, v in census.items()} == {
        ("pgemm_nt_kernel", False, "GI", 1): 4, ("pgemm_nt_kernel", False, "dg", 1): 65, ("pgemm_nt_kernel", True, "GI", 1): 13,
        ("pgemm_nt_kernel", True, "dg", 12): 32, ("pgemm_nt_kernel", True, "bptt", 12): 1,
        ("gemm32_nt_kernel", False, "GI", 1): 2, ("gemm32_nt_kernel", False, "dg", 1): 19}
    assert len(ic.KLOOP_CASES) == 4 + 65 + 13 + 2 + 19 == 103 and len(_kloop_shapes()) == 53
    assert {c[1] for c in ic.KLOOP_CASES} == {k for (_, _, _, stages), keys in census.items() for k in keys if stages < ic.KLOOP_STAGES}
    # one role per shape: H = 74 carries dg keys alone, S = 17 GI keys alone
    assert all(len(roles) == 1 for roles in _kloop_shapes().values())
    assert all((roles == {"dg"}) == (shape[3] == ic.KLOOP_H) and (roles == {"GI"}) == (shape[0] == ic.KLOOP_S and shape[3] != ic.KLOOP_H)
               for shape, roles in _kloop_shapes().items())
    # a pinned one-pass figure belongs to a one-pass K-loop case (none is pinned: every case is inside the imported bars)
    assert all(k in {c[1] for c in ic.KLOOP_CASES if c[6] == "f16"} and t in ["Y", "loss"] + list(PARAM_KEYS)
               for k, t in ic.KLOOP_F16_EXCEPTIONS) and ic.KLOOP_F16_EXCEPTIONS == {}
    # all fp32 I/O, no carried state, the training route -- as their cases in CASES; rows from 34 to 36 888
    assert {c[7:] for c in ic.KLOOP_CASES} == {("f32", False, "train")}
    assert sorted({c[3] * c[4] for c in ic.KLOOP_CASES}) == [34, 4098, 6146, 16419, 24483, 36888]


def test_the_kloop_checks_notice_a_mis_tabled_entry():
    dg_key, gi_key = "gemm32_nt_kernel<128x128>", "pgemm_nt_kernel<1>|out16=0|narrow"
    at = {k: next(n for n, c in enumerate(ic.KLOOP_CASES) if c[1] == k) for k in (dg_key, gi_key)}

    def with_(key, **kw):
        i = at[key]
        c = dict(zip(("fam", "key", "S", "T", "B", "H", "math", "io", "state", "route"), ic.KLOOP_CASES[i]))
        c.update(kw)
        return ic.KLOOP_CASES[:i] + [tuple(c.values())] + ic.KLOOP_CASES[i + 1:]
    assert ic.KLOOP_CASES[at[dg_key]][2:6] == (5, 3, 8161, 74) and ic.KLOOP_CASES[at[gi_key]][2:6] == (17, 2, 17, 4)
    # a deleted case: the first, one in the middle, the last
    for j in (0, at[dg_key], len(ic.KLOOP_CASES) - 1):
        gone = kloop_problems(ic.KLOOP_CASES[:j] + ic.KLOOP_CASES[j + 1:])
        assert gone == ["%s runs at most 1 K stages in CASES and KLOOP_CASES" % ic.KLOOP_CASES[j][1]], gone
    # H = 4 put back: the CASES entry itself
    assert kloop_problems(with_(dg_key, H=4)) == [
        "gemm32_nt_kernel<128x128>: the dg product runs 1 K stages, not an odd count >= 7",
        "gemm32_nt_kernel<128x128>: S = 5, H = 4, the rule says 5, 74",
        "gemm32_nt_kernel<128x128> runs at most 1 K stages in CASES and KLOOP_CASES"]
    # six stages: 3 H = 192
    assert kloop_problems(with_(dg_key, H=64)) == [
        "gemm32_nt_kernel<128x128>: the dg product runs 6 K stages, not an odd count >= 7",
        "gemm32_nt_kernel<128x128>: S = 5, H = 64, the rule says 5, 74",
        "gemm32_nt_kernel<128x128> runs at most 6 K stages in CASES and KLOOP_CASES"]
    # eight stages is past seven but even; nine is odd but not the rule's
    assert kloop_problems(with_(dg_key, H=85))[0] == "gemm32_nt_kernel<128x128>: the dg product runs 8 K stages, not an odd count >= 7"
    assert kloop_problems(with_(dg_key, H=96)) == ["gemm32_nt_kernel<128x128>: S = 5, H = 96, the rule says 5, 74"]
    # the wrong role: at S = 17, H = 32 the key is launched, with seven stages -- by GI (N = 96), where CASES keys it through dg
    wrong = with_(dg_key, S=17, H=32)
    assert dg_key in ic.plan(17, 3, 8161, 32, "f32") and ic.keyed_product(dg_key, 17, 3, 8161, 32, "f32") == ("GI", 24483, 96, 7)
    assert kloop_problems(wrong) == [
        "gemm32_nt_kernel<128x128>: at S = 17, H = 32 the key is not carried by the dg product that carries it in CASES",
        "gemm32_nt_kernel<128x128> runs at most 1 K stages in CASES and KLOOP_CASES"]
    # ... and a GI key moved along H instead of S: the GI product still carries it, for one stage
    assert kloop_problems(with_(gi_key, S=1, H=74))[0] == "pgemm_nt_kernel<1>|out16=0|narrow: the GI product runs 1 K stages, not an odd count >= 7"
    # a key lost, a key claimed twice, a key that needs no second case, another family's, another call form
    assert kloop_problems(with_(dg_key, S=17))[0] == "gemm32_nt_kernel<128x128>: plan() at S = 17, H = 74 does not contain the key"
    assert kloop_problems(ic.KLOOP_CASES + [ic.KLOOP_CASES[0]])[0] == "%s is claimed 2 times in KLOOP_CASES" % ic.KLOOP_CASES[0][1]
    twelve = next(c for c in ic.CASES if c[1] == "pgemm_nt_kernel<1,x2>|out16=0|wide")
    assert kloop_problems(ic.KLOOP_CASES + [twelve]) == ["pgemm_nt_kernel<1,x2>|out16=0|wide: its case in CASES already runs 12 K stages"]
    assert kloop_problems(ic.KLOOP_CASES + [c for c in ic.CASES if c[0] == "gcnx_fwd_kernel"][:1])
    assert kloop_problems(with_(dg_key, T=2)) and kloop_problems(with_(dg_key, B=8177)) and kloop_problems(with_(gi_key, math="f16"))


def test_the_tables_before_kloop_cases_ran_gemm32_128x128_for_one_stage():
    """The blind spot, asserted once: over CASES and EDGE_CASES together every launch of gemm32_nt_kernel<128x128> -- the keyed one
    or a sibling's -- contracts over 32 padded columns, so nloop = nk - 1 = 0 and the 128-row form's main loop never ran; the
    K-loop case runs it for six trips before the fused last step."""
    key = "gemm32_nt_kernel<128x128>"
    seen = [p for _, table in ALL_WINDOW_TABLES[:2] for c in table for p in ic.nt_products(*c[2:]) if p[0] == key]
    assert seen and {p[4] for p in seen} == {1}, seen
    case = next(c for c in ic.KLOOP_CASES if c[1] == key)
    assert ic.keyed_product(key, *case[2:]) == ("dg", 3 * 8161, 13 * 5, 7)
    # ... and so for most keys: those that NO launch of the two tables takes past one stage, by family and path (by the keyed
    # product of the CASES entry alone the count is 69 of 69, 21 of 21 and 13 of 46: the census of the test above; thirteen pgemm_nt
    # keys and two gemm32_nt keys get a longer loop as a sibling, mostly as GI of a case at S >= 30 and H = 4, where N = 12)
    most = {}
    for _, table in ALL_WINDOW_TABLES[:2]:
        for c in table:
            for k, role, M, N, stages in ic.nt_products(*c[2:]):
                most[k] = max(most.get(k, 0), stages)
    wide_gru = {c[1] for c in ic.CASES if c[0] == "pgemm_nt_kernel" and c[5] > 127}
    one = lambda keys: sum(most[k] == 1 for k in keys)
    reg = {c[1] for c in ic.CASES if c[0] == "pgemm_nt_kernel"} - wide_gru
    g32 = {c[1] for c in ic.CASES if c[0] == "gemm32_nt_kernel"}
    print("one-stage keys: pgemm_nt (H <= 127) %d of %d, gemm32_nt %d of %d, pgemm_nt (wide GRU) %d of %d"
          % (one(reg), len(reg), one(g32), len(g32), one(wide_gru), len(wide_gru)))
    assert (one(reg), len(reg)) == (60, 69) and (one(g32), len(g32)) == (19, 21) and (one(wide_gru), len(wide_gru)) == (9, 46)


KLOOP_WINDOWS = 64                                   # the inputs are qualified on the first min(B, 64) windows of the case's draw
KLOOP_MISTAKES = ("slab 3 of A from slab 2", "slab 3 of B from slab 2", "last slab left out")


def _slab_delta(Aop, Bop, mistake):
    """What a mistake of the K loop adds to C = Aop Bop^T, the operands [rows, K] cut into slabs of ic.NT_BK columns: an interior
    slab of one operand read from the slab before it (a stage consumed before its DMA landed: the slot still holds the stage
    two trips back in a two-slot ring; the previous slab stands for a stale one), or the last slab never accumulated."""
    K, bk = Aop.shape[1], ic.NT_BK
    assert K == Bop.shape[1] and K % bk == 0 and K // bk >= ic.KLOOP_STAGES          # slab 3 is interior
    s2, s3, last = slice(2 * bk, 3 * bk), slice(3 * bk, 4 * bk), slice(K - bk, K)
    if mistake == KLOOP_MISTAKES[0]:
        return torch.matmul(Aop[:, s2] - Aop[:, s3], Bop[:, s3].t())
    if mistake == KLOOP_MISTAKES[1]:
        return torch.matmul(Aop[:, s3], (Bop[:, s2] - Bop[:, s3]).t())
    assert mistake == KLOOP_MISTAKES[2]
    return -torch.matmul(Aop[:, last], Bop[:, last].t())


def _padded(t, K):
    return torch.cat([t, torch.zeros(t.shape[0], K - t.shape[1], dtype=t.dtype)], 1)


class _InputProjection(torch.autograd.Function):
    """The input projection as the oracle computes it -- forward GI = [g | 1] [W_ih | b_ih]^T, backward dg = dGI W_ih (and dW_ih,
    db_ih) -- with one mistake of KLOOP_MISTAKES planted into ONE of the two products: plant = (role, mistake) or None.  The
    operands are the kernels': K = Ip (g, the ones column, zero pad) for GI, K = Gp (the 3 H gate columns, zero pad) for dg."""

    @staticmethod
    def forward(ctx, g, Wih, bih, plant):
        ctx.save_for_backward(g, Wih)
        ctx.plant = plant
        GI = torch.matmul(g, Wih.t()) + bih
        if plant and plant[0] == "GI":
            g2 = g.reshape(-1, g.shape[-1])
            Ip = ic.rup(g2.shape[1] + 1, 32)
            Aop = _padded(torch.cat([g2, torch.ones(g2.shape[0], 1, dtype=g.dtype)], 1), Ip)
            Bop = _padded(torch.cat([Wih, bih[:, None]], 1), Ip)
            GI = GI + _slab_delta(Aop, Bop, plant[1]).reshape(GI.shape)
        return GI

    @staticmethod
    def backward(ctx, dGI):
        g, Wih = ctx.saved_tensors
        dGI2 = dGI.reshape(-1, dGI.shape[-1])
        dW = dGI2.t() @ g.reshape(-1, g.shape[-1])
        db = dGI2.sum(0)
        dg = dGI2 @ Wih
        if ctx.plant and ctx.plant[0] == "dg":
            Gp = ic.rup(dGI2.shape[1], 32)
            dg = dg + _slab_delta(_padded(dGI2, Gp), _padded(Wih.t(), Gp), ctx.plant[1])
        return dg.reshape(g.shape), dW, db, None


def kloop_step(r, plant=None, projection=None):
    """Y, the loss and the 8 gradients of the oracle's training step restated in fp64 around _InputProjection: the oracle's own
    graph convolutions, recurrence, BPTT and GCN backward, with GI and (dg, dW_ih, db_ih) taken from the Function (`projection`:
    another Function of the same signature, as tests/test_general_loops_host.py's for gemm.hip's operands)."""
    from oracle import windgnn_oracle as orc
    A, X, L = r["A"].double(), r["X"].double(), r["L"].double()
    p = {k: v.double() for k, v in r["p"].items()}
    Whh, bhh = p["gru.weight_hh_l0"], p["gru.bias_hh_l0"]
    B, T, S, F = X.shape
    H = Whh.shape[1]
    g, cache = orc.gcn2_forward(A, X, p)
    gl, Wl, bl = (t.detach().clone().requires_grad_(True) for t in (g, p["gru.weight_ih_l0"], p["gru.bias_ih_l0"]))
    GIa = (projection or _InputProjection).apply(gl, Wl, bl, plant)
    GI = GIa.detach()
    h = torch.zeros(B, H, dtype=torch.float64)
    Y, R, Z, N, GHN = (torch.empty(B, T, H, dtype=torch.float64) for _ in range(5))
    for t in range(T):                                            # orc.forward's loop
        gh = torch.matmul(h, Whh.t()) + bhh
        rg = torch.sigmoid(GI[:, t, 0:H] + gh[:, 0:H])
        z = torch.sigmoid(GI[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(GI[:, t, 2 * H:] + rg * gh[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        Y[:, t], R[:, t], Z[:, t], N[:, t], GHN[:, t] = h, rg, z, n, gh[:, 2 * H:]
    loss, dY = orc.mse_loss_and_grad(Y, L)
    dGI, dGH = (torch.empty(B, T, 3 * H, dtype=torch.float64) for _ in range(2))
    dh_next = torch.zeros(B, H, dtype=torch.float64)
    for t in range(T - 1, -1, -1):                                # orc.backward's loop
        hprev = Y[:, t - 1] if t > 0 else torch.zeros(B, H, dtype=torch.float64)
        rg, z, n = R[:, t], Z[:, t], N[:, t]
        dh = dY[:, t] + dh_next
        dn = dh * (1.0 - z)
        dz = dh * (hprev - n)
        dnt = dn * (1.0 - n * n)
        dr = dnt * GHN[:, t]
        dar = dr * rg * (1.0 - rg)
        daz = dz * z * (1.0 - z)
        dGI[:, t, 0:H], dGI[:, t, H:2 * H], dGI[:, t, 2 * H:] = dar, daz, dnt
        dGH[:, t, 0:H], dGH[:, t, H:2 * H], dGH[:, t, 2 * H:] = dar, daz, dnt * rg
        dh_next = dh * z + torch.matmul(dGH[:, t], Whh)
    GIa.backward(dGI)
    Hprev = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64), Y[:, :-1]], dim=1)
    dGH2 = dGH.reshape(B * T, 3 * H)
    grads = {"gru.weight_ih_l0": Wl.grad, "gru.bias_ih_l0": bl.grad,
             "gru.weight_hh_l0": dGH2.t() @ Hprev.reshape(B * T, H), "gru.bias_hh_l0": dGH2.sum(0)}
    grads.update(orc.gcn2_backward(A, p, cache, gl.grad.reshape(B, T, S, F)))
    return Y, float(loss), grads


def kloop_input_problems(shape, roles):
    """What is wrong with the inputs of a K-loop shape, measured on the oracle alone over the first KLOOP_WINDOWS windows of the
    case's own draw: a list of sentences."""
    from oracle import windgnn_oracle as orc
    from conftest import PARAM_KEYS, max_abs, rel_to_max
    from test_gpu_instances import _draw
    S, T, B, H, io, state = shape
    assert not state and io == "f32"                              # (the K-loop cases are the training route's)
    d = _draw(S, T, B, H, io, state)
    n = min(B, KLOOP_WINDOWS)
    r = dict(A=d["A"], X=d["X"][:n], L=d["L"][:n], p=d["p"])
    Y64, loss64, g64 = orc.train_step(r["A"].double(), r["X"].double(), r["L"].double(), {k: v.double() for k, v in r["p"].items()})
    bad = []
    # the oracle in fp32 against itself in fp64: a draw on which rounding alone costs a tenth of the bar proves nothing
    Y32, _, g32 = orc.train_step(r["A"], r["X"], r["L"], r["p"])
    gap = {"Y": rel_to_max(Y32, Y64)}
    gap.update({k: rel_to_max(g32[k], g64[k]) for k in PARAM_KEYS})
    bad += ["%s: %s in fp32 is %.1e off the fp64 oracle: pick another seed" % (shape, k, e) for k, e in gap.items() if e > 1e-5]
    # the restated step is the oracle's, bit for bit
    Yr, lossr, gr = kloop_step(r)
    assert torch.equal(Yr, Y64) and lossr == float(loss64) and all(torch.equal(gr[k], g64[k]) for k in PARAM_KEYS), shape
    # each mistake planted into the keyed product moves Y or a gradient by more than 10 fp32-grade bars
    for role in sorted(roles):
        moved = {}
        for m in KLOOP_MISTAKES:
            Ym, _, gm = kloop_step(r, (role, m))
            moved[m] = (max_abs(Ym, Y64), max(rel_to_max(gm[k], g64[k]) for k in PARAM_KEYS))
        print("%s %s: seed %d, %d windows, max|Y| %.2f, fp32 against fp64 at most %.1e; planted (Y, worst gradient): %s "
              "(in one-pass bars of 2e-2 / 5e-2: %s)"
              % (shape, role, ic.param_seed(S, H), n, float(Y64.abs().max()), max(gap.values()),
                 "  ".join("%.1e %.1e" % v for v in moved.values()),
                 "  ".join("%.2f %.2f" % (v[0] / F16_Y_BAR, v[1] / F16_G_BAR) for v in moved.values())))
        bad += ["%s: '%s' planted into %s moves Y by %.1e and no gradient by more than %.1e: pick another seed" % ((shape, m, role) + v)
                for m, v in moved.items() if not max(v) > 10 * Y_BAR]
    return bad


def test_kloop_inputs_are_well_conditioned_and_can_tell_the_planted_mistakes():
    """Per distinct K-loop shape, on the oracle alone and on the first 64 windows of the case's own draw (the conditioning is a
    property of (S, H) and the draw; 37 000 rows in fp64 several times over are not needed to see it): fp32 against fp64 within
    1e-5 on Y and every gradient; the step restated around _InputProjection equals the oracle's bit for bit; and each of the
    three K-loop mistakes, planted into the keyed product alone, moves Y or some gradient by more than 10 x 1e-4 (a mistake in
    dg leaves the forward alone and moves the four conv gradients).  Against the one-pass bars the figures are printed only."""
    shapes = _kloop_shapes()
    assert len(shapes) == 53
    problems = [p for shape, roles in shapes.items() for p in kloop_input_problems(shape, roles)]
    assert problems == []
    # the check notices a projection that is not the oracle's: the planted step differs from it
    S, T, B, H, io, state = next(iter(shapes))
    from test_gpu_instances import _draw
    d = _draw(S, T, B, H, io, state)
    r = dict(A=d["A"], X=d["X"][:4], L=d["L"][:4], p=d["p"])
    assert not torch.equal(kloop_step(r, ("GI", KLOOP_MISTAKES[2]))[0], kloop_step(r)[0])
