"""Host side of the K-loop half of the three TN weight-gradient GEMM families (no GPU): tests/instance_cases.py's tn_products()
held to its sources -- wgnn_tn_split, plan()'s names and the text of the launcher lines it restates --, the exact count of how
many K stages the tables before TN_KLOOP_CASES gave every TN key, TN_KLOOP_CASES re-derived entry by entry from its rule, and
the inputs of every case qualified on the oracle alone at the case's full shape (the contraction IS the rows: a sample of the
windows would not do): fp32 against fp64, and mistakes of the chunk / stage walk planted into the keyed product of a restated
fp64 step.  tests/test_gpu_tn_kloop.py runs the cases on the MI355X."""
import functools
import time

import torch

import instance_cases as ic
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_instance_table_host import IO, MATH, PLAIN_TB, THRESHOLD_TB, _read
from test_tn_split_host import _bt_sweep

G_BAR = 1e-4                                         # the split modes' gradient bar (tests/test_gpu_parity.py G_TOL)
F16_G_BAR = 5e-2                                     # the one-pass mode's
OLD_TABLES = (("CASES", ic.CASES), ("EDGE_CASES", ic.EDGE_CASES), ("KLOOP_CASES", ic.KLOOP_CASES),
              ("GEMM_F32_KLOOP_CASES", ic.GEMM_F32_KLOOP_CASES), ("GEMM_F32_FOLD_CASES", [c[:10] for c in ic.GEMM_F32_FOLD_CASES]))
ALL_TABLES = OLD_TABLES + (("TN_KLOOP_CASES", ic.TN_KLOOP_CASES),)


def _tn_keys(keys):
    return [k for k in keys if ic.family_of(k) in ic.TN_FAMILIES]


def _launches(prods):
    """The keys of tn_products() as plan() lists them: a merged launch once."""
    return [p["key"] for p in prods if not ("+" in ic.name_of(p["key"]) and p["role"] == "dW_hh")]


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    L.load()
    return L


# ---- 1. the restatement against its sources ---------------------------------------------------------------------------------
def test_tn_products_names_exactly_the_tn_launches_of_plan():
    """plan() is the authority for names.  For every case of every window-major table and over a grid of the thresholds,
    tn_products() gives plan()'s TN keys in plan()'s order, a merged launch as two products of one key."""
    for name, table in ALL_TABLES:
        for fam, key, S, T, B, H, math, io, state, route in table:
            prods = ic.tn_products(S, T, B, H, math, io, state, route)
            assert _launches(prods) == _tn_keys(ic.plan(S, T, B, H, math, io, state, route)), (name, key)
            for p in prods:
                merged = "+" in ic.name_of(p["key"])
                assert p["role"] in ic.TN_ROLES and p["rows"] == B * T and p["stages"] * ic.TN_BK == p["kchunk"], (name, key, p)
                assert (p["chunks"] - 1) * p["kchunk"] < B * T <= p["chunks"] * p["kchunk"] and p["chunks"] <= p["sk"], (name, key, p)
                assert 1 <= p["last_stages"] <= p["stages"] and 1 <= p["tail"] <= ic.TN_BK, (name, key, p)
                assert (p["source"] == "Y") <= (merged and p["role"] == "dW_hh" and p["shift_T"] == T and not p["per_window"]), (name, key, p)
                assert (p["source"] == "rows") == (ic.family_of(p["key"]) == "gemm32_tn_kernel"), (name, key, p)
                assert (p["shift_T"] > 0) == (p["role"] == "dW_hh" and p["source"] != "rows") and p["per_window"] <= (p["shift_T"] > 0)
            assert sum("+" in ic.name_of(p["key"]) for p in prods) in (0, 2), (name, key)
    for T, B in sorted(PLAIN_TB | THRESHOLD_TB | {(3, 16385)}):
        for S in (1, 17, 34, 60):
            for H in (4, 74, 127, 128, 129, 225):
                for math in ic.MATHS:
                    for io in ("f32", "bf16"):
                        for state, route in ((0, "train"), (0, "unmerged"), (0, "fused"), (0, "infer"), (1, "train"), (1, "unmerged")):
                            if ic.refusal(S, T, B, H, math, io):
                                continue
                            prods = ic.tn_products(S, T, B, H, math, io, bool(state), route)
                            assert _launches(prods) == _tn_keys(ic.plan(S, T, B, H, math, io, bool(state), route)), (S, T, B, H, math, io, route)
    # the issue's example: both roles at sk = 256, 221 chunks of seven stages, the last of seven with a one-row tail
    ih, hh = ic.tn_products(15, 3, 16491, 95, "f16x3")
    assert (ih["key"], ih["role"], hh["role"]) == ("pgemm_tn_kernel<7+3>|pw=0", "dW_ih", "dW_hh") == (hh["key"], "dW_ih", "dW_hh")
    for p in (ih, hh):
        assert (p["rows"], p["sk"], p["kchunk"], p["stages"], p["chunks"], p["last_stages"], p["tail"]) == (49473, 256, 224, 7, 221, 7, 1)
    assert (ih["source"], hh["source"], ih["shift_T"], hh["shift_T"]) == ("planes", "Y", 0, 3)
    # tests/test_gpu_tn_yfp32.py's shapes: 408 rows are five chunks of 96, not "more than one 384-row chunk"
    hh = ic.tn_products(34, 24, 17, 102, "f16x3")[1]
    assert (hh["sk"], hh["kchunk"], hh["chunks"], hh["last_stages"], hh["tail"], hh["source"]) == (6, 96, 5, 1, 24, "Y")
    for dims, tail in (((3, 3, 16491, 5), 1), ((3, 24, 2062, 101), 16)):
        hh = ic.tn_products(*dims, "f16x3")[1]
        assert ic.tn_seven(hh) and (hh["stages"], hh["tail"], hh["source"]) == (7, tail, "Y"), dims


def _split_problem(L, S, T, B, H, math, io, state):
    """tn_products() of the training route against wgnn_tn_split for the same dims: None, or what differs."""
    i = L.tn_split(L.Dims(B, T, S, 13, H, MATH[math], 0, 0, IO[io]), state=state)
    prods = ic.tn_products(S, T, B, H, math, io, state, "train")
    x3f = math != "f32"
    if i.merged != int(x3f and H <= 127) or i.merged != int(any("+" in ic.name_of(p["key"]) for p in prods)):
        return "merged = %d" % i.merged
    if not prods:                                                 # gemm.hip's exact-fp32 products: gemm_f32_products()
        return None if not x3f else "no product"
    by_role = {p["role"]: p for p in prods}
    got = (by_role["dW_ih"]["sk"], by_role["dW_hh"]["sk"], by_role["dW_ih"]["kchunk"], by_role["dW_hh"]["kchunk"])
    want = (i.sk_ih, i.sk_hh, i.kchunk_ih, i.kchunk_hh)
    return None if got == want else "tn_products %s, wgnn_tn_split %s" % (got, want)


def test_tn_products_split_k_as_wgnn_tn_split_does():
    """merged, sk and kchunk of both roles against the library's own layout function: over every case of every table, and over
    tests/test_tn_split_host.py's sweep of B*T from 1 to 131 072."""
    L = _lib()
    seen = set()
    for name, table in ALL_TABLES:
        for fam, key, S, T, B, H, math, io, state, route in table:
            dims = (S, T, B, H, math, io, state)
            if dims not in seen:
                seen.add(dims)
                assert _split_problem(L, *dims) is None, (name, key, _split_problem(L, *dims))
    for S, H in ((34, 102), (7, 20), (64, 102), (34, 127), (1, 1), (1, 128), (1, 224)):
        for math in ic.MATHS:
            for BT in _bt_sweep():
                T = 24 if BT % 24 == 0 else (3 if BT % 3 == 0 else 1)
                for state in (False, True):
                    assert _split_problem(L, S, T, BT // T, H, math, "f32", state) is None, (S, H, math, BT, state)


RESTATED = (
    # (file, the line tn_products() and its helpers restate)
    ("pgemm.hip", "  nNb = cdiv_i(Nout, 224);"),
    ("pgemm.hip", "  return cdiv_i(Mout, TN_BM) * nNb;"),
    ("pgemm.hip", "  const int kchunk = cdiv_i(cdiv_i(K, splitk), 32) * 32;"),
    ("pgemm.hip", "    r.kchunk = cdiv_i(cdiv_i(K, p.splitk), 32) * 32;"),
    ("pgemm.hip", "  const int nk = kend > kbeg ? (kend - kbeg + 31) / 32 : 0;"),
    ("pgemm.hip", "  if (hh.By && (tn2_mode(ih, hh) > 1 || hh.per_window || hh.shift_T < 1 || nNb != 1 || hh.ldb + 1 != hh.Nout)) return false;"),
    ("common.h", "constexpr int TN_BM = 320, TN_WAVES = 8;"),
    ("gemm32.hip", "constexpr int T_BM = 320, T_BK = 32;"),
    ("gemm32.hip", "  return cdiv_i(Mo, T_BM) * nNb;"),
    ("gemm32.hip", "  const int kchunk = cdiv_i(cdiv_i(K, splitk), T_BK) * T_BK;"),
    ("gemm32.hip", "  const int nk = (kend - kbeg + T_BK - 1) / T_BK;"),
    ("grux.hip", "int grux_hn(int H) { return 8 * cdiv_i(H, 8); }"),
    ("grux.hip", "int grux_msplit(int H) { return 8 * cdiv_i(2 * H, 8); }"),
    ("gru.hip", "int gru_msplit(int H) { return 4 * cdiv_i(2 * H, 4); }"),
    ("api.hip", "  L.m_hh = L.dghn ? (x3 ? L.msplit + L.hn : L.msplit + (int)L.H) : (int)L.G3;"),
    ("api.hip", "  L.dghn = (x3 && !L.gen_gru) || (L.rec32 && L.g32tn);"),
    ("api.hip", "    L.sk_ih = pick_splitk(L.BT, pgemm_tn_tiles((int)L.G3, (int)L.I + 1), 256, 64);"),
    ("api.hip", "    L.sk_hh = pick_splitk(L.BT, pgemm_tn_tiles(L.m_hh, (int)L.H + 1), 256, 64);"),
    ("api.hip", "    L.sk_ih = L.g32tn ? pick_splitk(L.BT, gemm32_tn_tiles((int)L.G3, (int)L.I + 1), 256, 64)"),
    ("api.hip", "    L.sk_hh = L.g32tn ? pick_splitk(L.BT, gemm32_tn_tiles(L.m_hh, (int)L.H + 1), 256, 64)"),
    ("api.hip", "  out->kchunk_ih = cdiv_i(cdiv_i((int)L.BT, L.sk_ih), 32) * 32;"),
    ("api.hip", "  out->kchunk_hh = cdiv_i(cdiv_i((int)L.BT, L.sk_hh), 32) * 32;"),
    ("api.hip", "  return tn_merge && three_pass(d) && d->io == WGNN_IO_F32 && !sst && from_env && opt(WGNN_OPT_TN_MERGED);"),
    ("api.hip", "    if (prods == (WGNN_ROWS_IH | WGNN_ROWS_HH) && L.tn_merge && opt(WGNN_OPT_TN_MERGED) && pgemm_tn2_covers(ih, hh)) {"),
    ("api.hip", "    hh.lda = (int)L.Gp; hh.Bhi = yph; hh.Blo = ypl; hh.ldb = (int)L.Hp; hh.shift_T = d->T; hh.splitk = L.sk_hh;"),
)


def test_the_restated_lines_are_in_the_sources():
    for name, line in RESTATED:
        assert "\n" + line in _read(name), (name, line)
    assert (ic.TN_BM, ic.TN_BK) == (320, 32)
    assert (ic.pgemm_tn_tiles(672, 225), ic.gemm32_tn_tiles(384, 129), ic.tn_m_hh(95, True, True), ic.tn_m_hh(95, False, True),
            ic.tn_m_hh(95, True, False), ic.tn_kchunk(49473, 256)) == (6, 2, 288, 287, 285, 224)


# ---- 2. what the tables before TN_KLOOP_CASES reached ------------------------------------------------------------------------
def _ran(p):
    """The longest K loop a product runs in any of its chunks."""
    return p["stages"] if p["chunks"] > 1 else p["last_stages"]


def stages_reached(tables):
    """Over every launch of `tables`: key -> the most stages a launch gives every product the key carries (the shorter role of
    a merged launch), and (key, role, source) -> the most stages that role runs from that B source."""
    by_key, by_role = {}, {}
    for _, table in tables:
        for c in table:
            launch = {}
            for p in ic.tn_products(*c[2:]):
                launch.setdefault(p["key"], []).append(_ran(p))
                k3 = (p["key"], p["role"], p["source"])
                by_role[k3] = max(by_role.get(k3, 0), _ran(p))
            for k, n in launch.items():
                by_key[k] = max(by_key.get(k, 0), min(n))
    return by_key, by_role


def _census(by_key):
    """(family, per-window, stages) -> keys."""
    out = {}
    for k, n in by_key.items():
        pw = "|pw=1" in k
        out[(ic.family_of(k), pw, n)] = out.get((ic.family_of(k), pw, n), 0) + 1
    return dict(sorted(out.items()))


# (family, per-window form, most stages) -> keys: 150 TN keys are launched by some case of the older tables (108 are claimed by
# CASES, the others run as siblings); 98 never pass three stages, 40 merged pw=0 keys reach five as by-products of the 36 888-row
# NT K-loop cases, eight unmerged pw=0 keys 10 to 24 and three gemm32 keys six, and no per-window key passes four
BLIND_SPOT = {
    ("gemm32_tn_kernel", False, 3): 9, ("gemm32_tn_kernel", False, 6): 3,
    ("pgemm_tn2_kernel", False, 2): 4, ("pgemm_tn2_kernel", False, 3): 10, ("pgemm_tn2_kernel", False, 5): 40,
    ("pgemm_tn2_kernel", True, 2): 12, ("pgemm_tn2_kernel", True, 3): 18,
    ("pgemm_tn_kernel", False, 2): 15, ("pgemm_tn_kernel", False, 3): 7, ("pgemm_tn_kernel", False, 10): 4,
    ("pgemm_tn_kernel", False, 20): 2, ("pgemm_tn_kernel", False, 24): 2,
    ("pgemm_tn_kernel", True, 2): 15, ("pgemm_tn_kernel", True, 3): 8, ("pgemm_tn_kernel", True, 4): 1,
}
# (role, B source, most stages) -> keys: the Y form of dW_hh (36 keys) never passed five stages, the plane form of 83 of its 102
# keys never three; 'rows' are gemm32.hip's fp32 operands
BLIND_SPOT_SOURCES = {
    ("dW_hh", "Y", 2): 2, ("dW_hh", "Y", 3): 7, ("dW_hh", "Y", 5): 27,
    ("dW_hh", "planes", 2): 38, ("dW_hh", "planes", 3): 45, ("dW_hh", "planes", 4): 1, ("dW_hh", "planes", 5): 13,
    ("dW_hh", "planes", 6): 2, ("dW_hh", "planes", 10): 2, ("dW_hh", "planes", 20): 1, ("dW_hh", "rows", 3): 5,
    ("dW_ih", "planes", 2): 23, ("dW_ih", "planes", 3): 28, ("dW_ih", "planes", 5): 16, ("dW_ih", "planes", 10): 28,
    ("dW_ih", "planes", 20): 1, ("dW_ih", "planes", 24): 2, ("dW_ih", "rows", 3): 4, ("dW_ih", "rows", 6): 3,
}


def test_the_tables_before_tn_kloop_cases_never_passed_a_few_stages():
    """The exact blind-spot table of DESIGN.md section 2c, "The TN half": over CASES, EDGE_CASES, KLOOP_CASES and the two
    gemm_f32 tables, how many reachable TN keys reach how many stages -- by (family, per-window form) -> {stages: keys}, and by
    (role, B source) -- and the old blind spot asserted once on one named key."""
    by_key, by_role = stages_reached(OLD_TABLES)
    census = _census(by_key)
    sources = {}
    for (k, role, src), n in by_role.items():
        sources[(role, src, n)] = sources.get((role, src, n), 0) + 1
    sources = dict(sorted(sources.items()))
    print("TN keys launched by the tables before TN_KLOOP_CASES: %d; (family, pw, most stages) -> keys: %s" % (len(by_key), census))
    print("(role, B source, most stages) -> keys: %s" % sources)
    assert census == BLIND_SPOT
    assert sources == BLIND_SPOT_SOURCES
    # every key CASES claims is among them, and none of those 108 passes three stages in its own entry -- but the six-tile dW_hh
    # of H = 224 at 4098 rows (sk = 40, kchunk = 128): four
    claimed = [c for c in ic.CASES if c[0] in ic.TN_FAMILIES]
    assert len(claimed) == 108 and {c[1] for c in claimed} <= set(by_key)
    own = {c[1]: max(_ran(p) for p in ic.tn_carried(c[1], *c[2:])) for c in claimed}
    assert {k for k, n in own.items() if n > 3} == {"pgemm_tn_kernel<4,x2>|a2=0|pw=1"} and max(own.values()) == 4
    # no per-window key, whoever launched it, ever ran more than four; 98 of the 150 keys never more than three
    assert max(n for k, n in by_key.items() if "|pw=1" in k) == 4 and len(by_key) == 150
    assert sum(n <= 3 for n in by_key.values()) == 98
    # the named key: the per-window merged launch at the bench's tile pair never ran a third stage -- each ring slot written
    # once -- and its stateless sibling five at most, in the Y form alone: its plane form never ran at all
    key, sib = "pgemm_tn_kernel<7+3>|pw=1", "pgemm_tn_kernel<7+3>|pw=0"
    assert by_key[key] == 2 and by_role[(key, "dW_ih", "planes")] == 2 == by_role[(key, "dW_hh", "planes")]
    assert by_key[sib] == 5 and by_role[(sib, "dW_hh", "Y")] == 5 and (sib, "dW_hh", "planes") not in by_role
    now_key, now_role = stages_reached(ALL_TABLES)
    assert now_key[key] == 7 == now_key[sib] and now_role[(sib, "dW_hh", "Y")] == 7 == now_role[(sib, "dW_hh", "planes")]
    # ... and with TN_KLOOP_CASES every key CASES claims reaches seven, in both B sources where it has two
    assert all(now_key[c[1]] >= ic.TN_KLOOP_STAGES for c in claimed)


# ---- 3. the table re-derived ----------------------------------------------------------------------------------------------
B_SCAN = 40000                                       # (the largest B of the rule is 16 385)


@functools.lru_cache(maxsize=None)
def smallest_b(key, S, H, math, io, state, route):
    """The rule's B: the smallest at which every product `key` carries is taken to seven stages (ic.tn_seven) at T = 3 and
    plan() still selects the key; None where no B up to B_SCAN does."""
    T = ic.TN_KLOOP_T
    for B in range(1, B_SCAN):
        if (B * T) % ic.TN_BK == 0 or B * T < ic.TN_KLOOP_STAGES * ic.TN_BK or ic.refusal(S, T, B, H, math, io):
            continue
        mine = ic.tn_carried(key, S, T, B, H, math, io, state, route)
        if mine and all(ic.tn_seven(p) for p in mine) and key in ic.plan(S, T, B, H, math, io, state, route):
            return B
    return None


def _wants_twin(case):
    """A merged pw=0 key of the split modes: its fp32-I/O case forms dW_hh's B rows from Y."""
    return case[0] == "pgemm_tn2_kernel" and case[6] in ("f16x3", "f16x3g") and not case[8]


def tn_kloop_problems(table):
    """What is wrong with `table` as TN_KLOOP_CASES: a list of sentences, empty when it is what the rule above the table gives."""
    bad = []
    base = [c for c in ic.CASES if c[0] in ic.TN_FAMILIES]
    known = {c[1]: c for c in base}
    ids = [(c[1], c[7]) for c in table]
    bad += ["%s (io = %s) is claimed %d times in TN_KLOOP_CASES" % (k + (ids.count(k),)) for k in dict.fromkeys(ids) if ids.count(k) > 1]
    bad += ["%s is no key CASES claims for a TN GEMM family" % c[1] for c in table if c[1] not in known]
    taken = {}                                                    # key -> roles an earlier case of the table takes to seven stages
    for c0 in base:
        fam, key, S0, T0, B0, H0, math0, io0, state0, route0 = c0
        roles0 = {p["role"] for p in ic.tn_carried(key, *c0[2:])}
        mine = [c for c in table if c[1] == key]
        need = not roles0 <= taken.get(key, set())
        if not need:
            bad += ["%s: an earlier case already takes every product it carries to seven stages" % key] if mine else []
            continue
        primary = [c for c in mine if c[7] == io0]
        if not primary:
            bad.append("%s has no case in TN_KLOOP_CASES and no earlier case takes its products to seven stages" % key)
        want_io = [io0] + ([ic.TN_KLOOP_TWIN_IO] if _wants_twin(c0) else [])
        if _wants_twin(c0) and primary and not [c for c in mine if c[7] == ic.TN_KLOOP_TWIN_IO]:
            bad.append("%s has no plane-form twin (io = %s): its case forms dW_hh's B rows from Y" % (key, ic.TN_KLOOP_TWIN_IO))
        bad += ["%s: io = %s is neither its CASES entry's nor the twin's" % (key, c[7]) for c in mine if c[7] not in want_io]
        for c in mine:
            fam, _, S, T, B, H, math, io, state, route = c
            if io not in want_io:
                continue
            if ic.refusal(S, T, B, H, math, io) is not None or key not in ic.plan(S, T, B, H, math, io, state, route):
                bad.append("%s: plan() at S = %d, B = %d, H = %d does not contain the key" % (key, S, B, H))
                continue
            prods = ic.tn_carried(key, *c[2:])
            if {p["role"] for p in prods} != roles0:
                bad.append("%s: at S = %d, H = %d the key is carried by %s alone, in CASES by %s"
                           % (key, S, H, " and ".join(sorted({p["role"] for p in prods})), " and ".join(sorted(roles0))))
                continue
            if (fam, S, H, math, state, route) != (c0[0], S0, H0, math0, state0, route0) or T != ic.TN_KLOOP_T:
                bad.append("%s: family, S, H, math, state and route are not those of its case in CASES, or T is not %d" % (key, ic.TN_KLOOP_T))
                continue
            if (B * T) % ic.TN_BK == 0:
                bad.append("%s: B*T = %d is a multiple of %d: no partial final stage" % (key, B * T, ic.TN_BK))
            for p in prods:
                if p["stages"] < ic.TN_KLOOP_STAGES:
                    bad.append("%s: the %s product runs %d stages a chunk (kchunk = %d), not %d or more" % (key, p["role"], p["stages"], p["kchunk"], ic.TN_KLOOP_STAGES))
                elif p["last_stages"] < 2:
                    bad.append("%s: the last non-empty chunk of the %s product has one stage" % (key, p["role"]))
                want_src = "rows" if fam == "gemm32_tn_kernel" else ("Y" if (p["role"] == "dW_hh" and _wants_twin(c0) and io == io0) else "planes")
                if p["source"] != want_src:
                    bad.append("%s (io = %s): the %s product reads its B rows from %s, not %s" % (key, io, p["role"], p["source"], want_src))
            rule = smallest_b(key, S, H, math, io, state, route)
            moved = ic.TN_KLOOP_B_MOVED.get((S, H)) if state else None
            if moved is not None and not moved > rule:
                bad.append("%s: TN_KLOOP_B_MOVED gives B = %d, not above the rule's %d" % (key, moved, rule))
            elif all(ic.tn_seven(p) for p in prods) and B != (moved or rule):
                bad.append("%s: B = %d, the rule's smallest is %s%s" % (key, B, rule, ", moved to %d by TN_KLOOP_B_MOVED" % moved if moved else ""))
        for c in primary[:1]:                                     # what this case takes to seven stages, for the keys after it
            for p in ic.tn_products(*c[2:]):
                if ic.tn_seven(p):
                    taken.setdefault(p["key"], set()).add(p["role"])
    return bad


def _shapes():
    """The distinct (S, T, B, H, io, state) of TN_KLOOP_CASES in table order, each with the distinct walks of its keyed products:
    (role, sk, kchunk, shift_T, per_window) -- shift_T = 0 where the B rows are read as they lie."""
    out = {}
    for c in ic.TN_KLOOP_CASES:
        for p in ic.tn_carried(c[1], *c[2:]):
            out.setdefault((c[2], c[3], c[4], c[5], c[7], c[8]), set()).add(
                (p["role"], p["sk"], p["kchunk"], p["shift_T"], p["per_window"]))
    return out


def test_tn_kloop_cases_are_what_the_rule_gives():
    assert tn_kloop_problems(ic.TN_KLOOP_CASES) == []
    assert (ic.TN_KLOOP_STAGES, ic.TN_KLOOP_T, ic.TN_KLOOP_TWIN_IO, 32 % ic.TN_KLOOP_T) == (7, 3, "bf16", 2)
    twins = [c for c in ic.TN_KLOOP_CASES if c[7] != "f32"]
    assert len(ic.TN_KLOOP_CASES) == 119 and len(twins) == 14 and len(_shapes()) == 39
    assert all(c[0] == "pgemm_tn2_kernel" and "|pw=0" in c[1] and ",f16" not in c[1] for c in twins)
    # the three keys the rule skips, and what took them to seven stages
    claimed = [c[1] for c in ic.CASES if c[0] in ic.TN_FAMILIES]
    skipped = [k for k in claimed if k not in {c[1] for c in ic.TN_KLOOP_CASES}]
    assert skipped == ["pgemm_tn_kernel<1>|a2=1|pw=0", "pgemm_tn_kernel<1,f16>|a2=1|pw=0", "gemm32_tn_kernel<1>|a2=1"]
    for k, by in zip(skipped, ("pgemm_tn_kernel<1>|a2=0|pw=0", "pgemm_tn_kernel<1,f16>|a2=0|pw=0", "gemm32_tn_kernel<1>|a2=0")):
        case = next(c for c in ic.TN_KLOOP_CASES if c[1] == by)
        assert [ic.tn_seven(p) for p in ic.tn_carried(k, *case[2:])] == [True], (k, by)
    # rows: one tile a chunk 49 155, two 24 579, six 7683 (the moved carried-state cases 49 158 ... 49 173); every case has a
    # partial final stage behind at least one full one: 3 live rows, or 6 ... 21
    assert sorted({c[3] * c[4] for c in ic.TN_KLOOP_CASES}) == [7683, 24579, 49155, 49158, 49161, 49164, 49167, 49173]
    tails = {c[4]: {p["tail"] for p in ic.tn_carried(c[1], *c[2:])} for c in ic.TN_KLOOP_CASES}
    assert tails == {2561: {3}, 8193: {3}, 16385: {3}, 16386: {6}, 16387: {9}, 16388: {12}, 16389: {15}, 16391: {21}}
    assert all(ic.tn_seven(p) and p["last_stages"] == {2561: 3, 8193: 6}.get(c[4], 4)
               for c in ic.TN_KLOOP_CASES for p in ic.tn_carried(c[1], *c[2:]))
    # the one deviation: 18 carried-state cases of six (S, H), none of them stateless
    assert ic.TN_KLOOP_B_MOVED == {(1, 96): 16386, (5, 96): 16389, (8, 64): 16386, (10, 4): 16387, (13, 32): 16391, (15, 64): 16388}
    at_moved = [c for c in ic.TN_KLOOP_CASES if c[8] and (c[2], c[5]) in ic.TN_KLOOP_B_MOVED]
    assert len(at_moved) == 18 and {c[4] for c in ic.TN_KLOOP_CASES} - {c[4] for c in at_moved} == {2561, 8193, 16385}
    assert ic.TN_KLOOP_F16_EXCEPTIONS == {}


def test_the_tn_kloop_checks_notice_a_mis_tabled_entry():
    one, both = "pgemm_tn_kernel<7>|a2=0|pw=0", "pgemm_tn_kernel<7+3>|pw=0"
    T = ic.TN_KLOOP_CASES
    at = {k: next(n for n, c in enumerate(T) if c[1] == k and c[7] == "f32") for k in (one, both)}

    def with_(key, **kw):
        i = at[key]
        c = dict(zip(("fam", "key", "S", "T", "B", "H", "math", "io", "state", "route"), T[i]))
        c.update(kw)
        return T[:i] + [tuple(c.values())] + T[i + 1:]
    assert T[at[one]][2:6] == (15, 3, 16385, 4) and T[at[both]][2:6] == (15, 3, 16385, 64)
    # a deleted case: the first, one in the middle, the last
    for j in (0, at[one], len(T) - 1):
        assert tn_kloop_problems(T[:j] + T[j + 1:]) == [
            "%s has no case in TN_KLOOP_CASES and no earlier case takes its products to seven stages" % T[j][1]], T[j]
    # B = 17 put back: 51 rows, two stages
    assert tn_kloop_problems(with_(one, B=17)) == ["%s: the dW_ih product runs 2 stages a chunk (kchunk = 64), not 7 or more" % one]
    assert tn_kloop_problems(with_(both, B=17)) == ["%s: the %s product runs 2 stages a chunk (kchunk = 64), not 7 or more" % (both, r)
                                                    for r in ic.TN_ROLES]
    # a six-stage case: 36 865 rows at sk = 256 are chunks of 160 rows ... 192 at 49 150
    six = with_(one, B=16383)
    assert ic.tn_carried(one, 15, 3, 16383, 4, "f16x3", "f32", False, "unmerged")[0]["stages"] == 6
    assert tn_kloop_problems(six) == ["%s: the dW_ih product runs 6 stages a chunk (kchunk = 192), not 7 or more" % one]
    # rows a multiple of 32: B = 16 416, 49 248 rows
    assert tn_kloop_problems(with_(one, B=16416)) == ["%s: B*T = 49248 is a multiple of 32: no partial final stage" % one]
    # a legal but larger B
    assert tn_kloop_problems(with_(one, B=16491)) == ["%s: B = 16491, the rule's smallest is 16385" % one]
    # a moved carried-state case put back on the rule's own B (whose draw has a ReLU tie: TN_KLOOP_B_MOVED)
    tie = next(n for n, c in enumerate(T) if c[1] == "pgemm_tn_kernel<4+3>|pw=1")
    assert T[tie][2:6] == (8, 3, 16386, 64)
    assert tn_kloop_problems(T[:tie] + [T[tie][:4] + (16385,) + T[tie][5:]] + T[tie + 1:]) == [
        "pgemm_tn_kernel<4+3>|pw=1: B = 16385, the rule's smallest is 16385, moved to 16386 by TN_KLOOP_B_MOVED"]
    # a last chunk of one stage: 49 281 + 3 rows = 220 chunks of 224 and one of 4 rows
    assert ic.tn_carried(one, 15, 3, 16428, 4, "f16x3", "f32", False, "unmerged")[0]["last_stages"] == 1
    assert tn_kloop_problems(with_(one, B=16428)) == ["%s: the last non-empty chunk of the dW_ih product has one stage" % one]
    # the other role only: at S = 1, H = 192 (merged launches off) pgemm_tn_kernel<7>|a2=0|pw=0 is dW_hh of the wide-GRU path
    other = with_(one, S=1, H=192)
    assert [p["role"] for p in ic.tn_carried(one, 1, 3, 16385, 192, "f16x3", "f32", False, "unmerged")] == ["dW_hh"]
    assert tn_kloop_problems(other) == ["%s: at S = 1, H = 192 the key is carried by dW_hh alone, in CASES by dW_ih" % one]
    # a missing plane-form twin, a twin at the wrong I/O type, a twin of a key that has none
    twin = next(n for n, c in enumerate(T) if c[1] == both and c[7] == "bf16")
    assert tn_kloop_problems(T[:twin] + T[twin + 1:]) == [
        "%s has no plane-form twin (io = bf16): its case forms dW_hh's B rows from Y" % both]
    assert tn_kloop_problems(T + [T[at[one]][:7] + ("bf16",) + T[at[one]][8:]]) == [
        "%s: io = bf16 is neither its CASES entry's nor the twin's" % one]
    # claimed twice, another family's key, a key that needs no case, T = 2
    assert tn_kloop_problems(T + [T[0]])[0] == "%s (io = f32) is claimed 2 times in TN_KLOOP_CASES" % T[0][1]
    assert tn_kloop_problems(T + [c for c in ic.CASES if c[0] == "gcnx_fwd_kernel"][:1])
    skipped = next(c for c in ic.CASES if c[1] == "pgemm_tn_kernel<1>|a2=1|pw=0")
    assert tn_kloop_problems(T + [skipped[:3] + (3, 16385) + skipped[5:]]) == [
        "pgemm_tn_kernel<1>|a2=1|pw=0: an earlier case already takes every product it carries to seven stages"]
    assert tn_kloop_problems(with_(one, T=2)) and tn_kloop_problems(with_(one, math="f16")) and tn_kloop_problems(with_(both, state=True))


# ---- 4, 5. the inputs, on the oracle alone --------------------------------------------------------------------------------
MISTAKES = ("stage kt >= 2 read from stage kt - 2", "the same on the B operand only", "window-start mask frozen at stage 0's",
            "per-window: the shared start row from stage 1 on")
TAIL = "partial last stage not zeroed"               # reported, never asserted (at most 31 of 7683 ... 49 167 rows)
# MISTAKES[0] swaps BOTH operands of a stage for those of the stage two back: the product then counts 64 rows twice in place of 64
# others, and where the rows' contributions are close to identically distributed the sum hardly moves.  Measured on the oracle, it
# stays below ten split-mode bars (but above one) on three shape / role pairs, all at H = 4; printed there, not asserted
# (DESIGN.md section 2c); the B-operand-only form of the same mistake moves the same products by 1.4e-1, 1.4e-1 and 2.4e-2
STALE_BOTH_FAINT = {((10, 3, 16385, 4, "f32", False), "dW_hh"): 6.0e-4, ((10, 3, 16385, 4, "bf16", False), "dW_hh"): 6.0e-4,
                    ((13, 3, 16385, 4, "f32", False), "dW_ih"): 9.2e-4}


def tn_walk(Aop, Bop, Y, starts, rows, kchunk, shift_T, per_window, mistake=None):
    """[dW | db] = Aop^T [B rows | 1] formed as the TN kernels form it: the `rows` rows of the contraction cut into chunks of
    `kchunk`, each walked in stages of ic.TN_BK rows, a partial sum per chunk, the chunks summed in order (finish.hip).
    Aop [rows, M] as it lies.  The B rows: with shift_T = 0 Bop [rows, N] as it lies; else row k is row k - 1 of Y [rows, N]
    unless k % shift_T == 0, a window start, where it is the start row -- starts[k / shift_T] ([windows, N]: per-window h0, or
    zeros for the one shared [0 | 1] row).  Rows past the end are zero in A (the kernel zeroes the dead rows of the partial
    stage; stages past it do not run).  mistake: one of MISTAKES or TAIL, planted into every chunk."""
    st = kchunk // ic.TN_BK
    chunks = ic.cdiv(rows, kchunk)
    k = torch.arange(chunks * kchunk)
    kt, r, kbeg = (k % kchunk) // ic.TN_BK, k % ic.TN_BK, (k // kchunk) * kchunk
    stale = (kt >= 2) if mistake in (MISTAKES[0], MISTAKES[1]) else torch.zeros_like(k, dtype=torch.bool)
    live = k < rows
    a_row = torch.where(stale, k - 2 * ic.TN_BK, k) if mistake == MISTAKES[0] else k
    if mistake == TAIL:                                           # the dead rows keep what the slot held: stage kt - 2
        dead = (~live) & (k < ic.rup(rows, ic.TN_BK)) & (kt >= 2)
        a_row = torch.where(dead, k - 2 * ic.TN_BK, a_row)
        live = live | dead
    A = Aop[a_row.clamp(max=rows - 1)] * live[:, None].to(Aop.dtype)
    b_row = torch.where(stale, k - 2 * ic.TN_BK, k).clamp(max=rows - 1)       # (the DMA clamps at the chunk's last row)
    if shift_T == 0:
        Bm = Bop[b_row]
    else:
        phase = kbeg + r if mistake == MISTAKES[2] else b_row     # the row whose k % shift_T decides "window start"
        start = phase % shift_T == 0
        win = b_row // shift_T
        if mistake == MISTAKES[3]:
            assert per_window
            win = torch.where(kt >= 1, torch.zeros_like(win), win)
        Bm = torch.where(start[:, None], starts[win if per_window else torch.zeros_like(win)], Y[(b_row - 1).clamp(min=0)])
    Bm = torch.cat([Bm, torch.ones(Bm.shape[0], 1, dtype=Bm.dtype)], 1)
    M, N = A.shape[1], Bm.shape[1]
    part = torch.bmm(A.reshape(chunks, st * ic.TN_BK, M).transpose(1, 2), Bm.reshape(chunks, st * ic.TN_BK, N))
    assert part.shape == (chunks, M, N) and st * ic.TN_BK == kchunk
    out = part[0].clone()
    for z in range(1, chunks):
        out += part[z]
    return out


class _Walk:
    """How one role's product is walked, and -- after a backward -- the operands it was walked on."""

    def __init__(self, rows, kchunk, shift_T=0, per_window=False, Y=None, starts=None):
        self.rows, self.kchunk, self.shift_T, self.per_window, self.Y, self.starts = rows, kchunk, shift_T, per_window, Y, starts
        self.Aop = self.Bop = None

    def product(self, mistake=None, kchunk=None):
        return tn_walk(self.Aop, self.Bop, self.Y, self.starts, self.rows, kchunk or self.kchunk, self.shift_T, self.per_window, mistake)


class _TnProduct(torch.autograd.Function):
    """out = Bop [W | b]^T as the oracle computes it (GI from g; the recurrent projection from the Hprev rows), whose backward
    forms [dW | db] = dOut^T [Bop | 1] by tn_walk -- chunks and stages -- and d Bop = dOut W as the oracle does."""

    @staticmethod
    def forward(ctx, Bop, W, b, walk):
        ctx.save_for_backward(Bop, W)
        ctx.walk = walk
        return torch.matmul(Bop, W.t()) + b

    @staticmethod
    def backward(ctx, dOut):
        Bop, W = ctx.saved_tensors
        ctx.walk.Aop, ctx.walk.Bop = dOut.detach(), Bop.detach()
        P = ctx.walk.product()
        return dOut @ W, P[:, :-1].contiguous(), P[:, -1].contiguous(), None


def tn_step(r, kchunk_ih, kchunk_hh, per_window=False, dtype=torch.float64):
    """One step of a case restated in `dtype` around _TnProduct: the oracle's graph convolutions, recurrence, BPTT and GCN
    backward (orc.forward / orc.backward, line for line), with both weight-gradient products formed by tn_walk.  r: the
    case's draw (tests/test_gpu_instances.py _draw) -- with h0, dY, dhn the carried-state step (Y, h_n, the 8 gradients, dh0),
    else the MSE step (Y, the loss, the 8 gradients).  Returns (figures, gradients, {role: _Walk}, what orc.gcn2_backward ran on)."""
    from oracle import windgnn_oracle as orc
    A, X = r["A"].to(dtype), r["X"].to(dtype)
    p = {k: v.to(dtype) for k, v in r["p"].items()}
    Whh, bhh = p["gru.weight_hh_l0"], p["gru.bias_hh_l0"]
    B, T, S, F = X.shape
    H = Whh.shape[1]
    state = "h0" in r
    g, cache = orc.gcn2_forward(A, X, p)
    gl, Wl, bl = (t.detach().clone().requires_grad_(True) for t in (g.reshape(B * T, S * F), p["gru.weight_ih_l0"], p["gru.bias_ih_l0"]))
    walk_ih = _Walk(B * T, kchunk_ih)
    GIa = _TnProduct.apply(gl, Wl, bl, walk_ih)
    GI = GIa.detach().reshape(B, T, 3 * H)
    h0 = r["h0"].to(dtype) if state else torch.zeros(B, H, dtype=dtype)
    h = h0
    Y, R, Z, N, GHN = (torch.empty(B, T, H, dtype=dtype) for _ in range(5))
    for t in range(T):
        gh = torch.matmul(h, Whh.t()) + bhh
        rg = torch.sigmoid(GI[:, t, 0:H] + gh[:, 0:H])
        z = torch.sigmoid(GI[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(GI[:, t, 2 * H:] + rg * gh[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        Y[:, t], R[:, t], Z[:, t], N[:, t], GHN[:, t] = h, rg, z, n, gh[:, 2 * H:]
    fig = {"Y": Y}
    if state:
        dY, dh_next = r["dY"].to(dtype), r["dhn"].to(dtype)
        fig["hn"] = h
    else:
        loss, dY = orc.mse_loss_and_grad(Y, r["L"].to(dtype))
        dh_next = torch.zeros(B, H, dtype=dtype)
        fig["loss"] = loss
    dGI, dGH = (torch.empty(B, T, 3 * H, dtype=dtype) for _ in range(2))
    for t in range(T - 1, -1, -1):
        hprev = Y[:, t - 1] if t > 0 else h0
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
    if state:
        fig["dh0"] = dh_next
    GIa.backward(dGI.reshape(B * T, 3 * H))
    Hprev = torch.cat([h0[:, None], Y[:, :-1]], dim=1).reshape(B * T, H)
    # the rows the plane kernels read: Y itself one row up, the start rows apart (h0 per window, or the one shared zero row)
    walk_hh = _Walk(B * T, kchunk_hh, T, per_window, Y.reshape(B * T, H), h0 if per_window else torch.zeros(1, H, dtype=dtype))
    Hl, Whl, bhl = Hprev.clone().requires_grad_(True), Whh.detach().clone().requires_grad_(True), bhh.detach().clone().requires_grad_(True)
    _TnProduct.apply(Hl, Whl, bhl, walk_hh).backward(dGH.reshape(B * T, 3 * H))
    grads = {"gru.weight_ih_l0": Wl.grad, "gru.bias_ih_l0": bl.grad, "gru.weight_hh_l0": Whl.grad, "gru.bias_hh_l0": bhl.grad}
    dg = gl.grad.reshape(B, T, S, F)
    grads.update(orc.gcn2_backward(A, p, cache, dg))
    return fig, grads, {"dW_ih": walk_ih, "dW_hh": walk_hh}, (A, p, cache, dg)


def _oracle(r, dtype):
    """The reference tests/test_gpu_instances.py holds the GPU to, in `dtype`: orc.train_step, or for a carried-state draw
    the autograd model of tests/test_gpu_state_train.py (fp64 only)."""
    from oracle import windgnn_oracle as orc
    if "h0" not in r:
        Yo, loss, go = orc.train_step(r["A"].to(dtype), r["X"].to(dtype), r["L"].to(dtype), {k: v.to(dtype) for k, v in r["p"].items()})
        return {"Y": Yo, "loss": loss}, go
    assert dtype == torch.float64
    from test_gpu_state_train import _fp64_model
    leaves, f = _fp64_model(r["p"])
    h0r = r["h0"].double().requires_grad_(True)
    Yr, hnr = f(r["A"], r["X"].float(), h0r)
    ((Yr * r["dY"].double()).sum() + (hnr * r["dhn"].double()).sum()).backward()
    return {"Y": Yr.detach(), "hn": hnr.detach(), "dh0": h0r.grad}, {k: leaves[k].grad for k in PARAM_KEYS}


def _gap(fa, ga, fb, gb):
    """Figures and gradients a against b: Y, h_n absolute; the loss, dh0 and the gradients relative to max."""
    out = {}
    for k in fb:
        out[k] = max_abs(fa[k], fb[k]) if k in ("Y", "hn") else rel_to_max(fa[k], fb[k])
    out.update({k: rel_to_max(ga[k], gb[k]) for k in PARAM_KEYS})
    return out


TIE_BAND = 2.0 ** -24                                # half an fp32 ulp of the sum of a pre-activation's term magnitudes
CONV_KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")


def relu_tie_problems(shape, gcn, grads):
    """ReLU ties of one draw, on the fp64 reference: sentences.  A pre-activation z = sum_f P[f] W[f, g] + b[g] of either layer
    whose |z| is below TIE_BAND x (sum_f |P[f] W[f, g]| + |b[g]|) has no sign to fp32 accuracy -- any fp32-grade evaluation, the
    reference's own in fp32 and every kernel mode, may put it on the other side of zero, whatever its order of sums -- and the
    reference then differs from a correct kernel by the whole term that mask element gates.  Where the conv gradients are
    coherent sums (the MSE step) one term is ~1e-6 of max; under the carried-state step's signed random dY they are sums of
    B*T*S cancelling terms and one term is ~1e-3 of max: ten split-mode bars.  A problem: such an element whose flip alone
    (computed exactly, on its own window and hour) moves a conv gradient by more than half of G_BAR."""
    from oracle import windgnn_oracle as orc
    A, p, cache, dg = gcn
    B, T, S, F = dg.shape
    bad = []
    for layer, Pk, Wk, bk, act in ((1, "P1", "conv1.weight", "conv1.bias", "H1"), (2, "P2", "conv2.weight", "conv2.bias", "g")):
        Z = torch.matmul(cache[Pk], p[Wk]) + p[bk]
        mag = torch.matmul(cache[Pk].abs(), p[Wk].abs()) + p[bk].abs()
        near = ((Z.abs() < TIE_BAND * mag) & (mag > 0)).reshape(-1).nonzero().flatten().tolist()
        for j in near:
            b, t = j // (T * S * F), (j // (S * F)) % T
            one = {k: cache[k][b:b + 1, t:t + 1] for k in ("P1", "H1", "P2", "g")}
            base = orc.gcn2_backward(A, p, one, dg[b:b + 1, t:t + 1])
            flipped = dict(one)
            a = one[act].clone().reshape(-1)
            e = j % (S * F)
            a[e] = 0.0 if a[e] > 0 else 1.0                      # (gcn2_backward reads the activations' sign alone)
            flipped[act] = a.reshape(one[act].shape)
            moved = orc.gcn2_backward(A, p, flipped, dg[b:b + 1, t:t + 1])
            cost = {k: float((moved[k] - base[k]).abs().max() / grads[k].abs().max()) for k in CONV_KEYS}
            k = max(cost, key=cost.get)
            if cost[k] > G_BAR / 2:
                bad.append("%s: layer-%d pre-activation %d is %.1e of its terms from zero and its flip moves %s by %.1e of max: "
                           "pick another draw" % (shape, layer, j, float(Z.reshape(-1)[j].abs() / mag.reshape(-1)[j]), k, cost[k]))
    return bad


X2_STATE_BAR = 1e-3                                  # the gradient bar of a single-plane f16x3g carried-state case from 4096 rows


def single_plane_problems(shape, w, gcn, grads):
    """What f16x3g's single plane costs by itself on one carried-state draw: sentences.  From 4096 rows that mode carries dGI and
    dGHn as ONE fp16 plane and forms dW_ih in one pass, hi(dGI)^T hi([g | 1]) (api.hip make_layout, L.dgi1; bwd_weights); dW_hh
    and dg take hi(dGI / dGH) against both planes of the other operand.  The rounding is 2^-11 of each element and averages
    out over coherent sums; the carried-state step's signed random dY leaves sums of cancelling terms, where it shows at full
    size.  The fp64 step with exactly those operands rounded to fp16 against itself unrounded: a problem where the rounding
    alone takes more than half of X2_STATE_BAR (as KLOOP_F16_EXCEPTIONS' rule for the one-pass mode: then the draw, not a
    kernel, decides whether the case passes)."""
    from oracle import windgnn_oracle as orc
    A, p, cache, dg = gcn
    h = lambda x: x.detach().half().double()
    one = lambda x: torch.cat([x, torch.ones(x.shape[0], 1, dtype=x.dtype)], 1)
    Pih = h(w["dW_ih"].Aop).t() @ h(one(w["dW_ih"].Bop))
    Phh = h(w["dW_hh"].Aop).t() @ one(w["dW_hh"].Bop.detach())
    got = {"gru.weight_ih_l0": Pih[:, :-1], "gru.bias_ih_l0": Pih[:, -1], "gru.weight_hh_l0": Phh[:, :-1], "gru.bias_hh_l0": Phh[:, -1]}
    got.update(orc.gcn2_backward(A, p, cache, (h(w["dW_ih"].Aop) @ p["gru.weight_ih_l0"]).reshape(dg.shape)))
    cost = {k: rel_to_max(got[k], grads[k]) for k in PARAM_KEYS}
    return ["%s: f16x3g's single fp16 plane of dGI / dGHn (and of g in dW_ih) alone moves %s by %.1e of max, more than half of the "
            "%.0e bar: pick another draw" % (shape, k, e, X2_STATE_BAR) for k, e in cost.items() if e > X2_STATE_BAR / 2], cost


def input_problems(shape, walks, report):
    """What is wrong with the inputs of one TN K-loop shape, measured on the oracle alone at the full shape: sentences.
    report: a list that receives (shape, role, mistake, effect on the role's weight / bias gradient relative to max)."""
    from test_gpu_instances import _draw
    S, T, B, H, io, state = shape
    r = _draw(S, T, B, H, io, state)
    kc = {role: kchunk for role, sk, kchunk, shift_T, pw in walks}
    f64, g64 = _oracle(r, torch.float64)
    bad = []
    # (a) rounding alone: the same step in fp32 against fp64 (the carried-state reference is fp64 only: the restated step stands in)
    f_r, g_r, w, gcn = tn_step(r, kc.get("dW_ih", 224), kc.get("dW_hh", 224), per_window=state)
    if state:
        f32, g32, _, _ = tn_step(r, kc.get("dW_ih", 224), kc.get("dW_hh", 224), per_window=state, dtype=torch.float32)
    else:
        f32, g32 = _oracle(r, torch.float32)
    gap = _gap(f32, g32, f64, g64)
    bad += ["%s: %s in fp32 is %.1e off the fp64 reference: pick another draw" % (shape, k, e) for k, e in gap.items() if e > 1e-5]
    bad += relu_tie_problems(shape, gcn, g64)
    if state:                                                     # (every carried-state shape has a ',x2>' case)
        bad += single_plane_problems(shape, w, gcn, g64)[0]
    # (b) the restated step is the reference's: the unplanted walk sums in another order, in fp64
    same = _gap(f_r, g_r, f64, g64)
    bad += ["%s: the restated step's %s is %.1e off the fp64 reference" % (shape, k, e) for k, e in same.items() if e > 1e-12]
    # (c) each mistake, planted into the keyed product alone, moves that product's two gradients
    for role, sk, kchunk, shift_T, pw in sorted(walks):
        walk = w[role]
        assert walk.per_window == (pw if role == "dW_hh" else False)
        if role == "dW_hh" and shift_T == 0:                      # gemm32.hip: the [Hprev | 1] rows as the forward wrote them
            walk = _Walk(walk.rows, kchunk)
            walk.Aop, walk.Bop = w[role].Aop, w[role].Bop
        ref = walk.product(kchunk=kchunk)
        names = [MISTAKES[0], MISTAKES[1]] + ([MISTAKES[2]] if shift_T else []) + ([MISTAKES[3]] if pw else []) + [TAIL]
        for m in names:
            P = walk.product(m, kchunk=kchunk)
            e = max(rel_to_max(P[:, :-1], ref[:, :-1]), rel_to_max(P[:, -1], ref[:, -1]))
            report.append((shape, role, m, e))
            if m == MISTAKES[0] and (shape, role) in STALE_BOTH_FAINT:
                if not G_BAR < e <= 10 * G_BAR:
                    bad.append("%s: '%s' planted into %s moves its gradients by %.1e of max: no entry of STALE_BOTH_FAINT" % (shape, m, role, e))
            elif m != TAIL and not e > 10 * G_BAR:
                bad.append("%s: '%s' planted into %s moves its gradients by %.1e of max: pick another draw" % (shape, m, role, e))
    return bad, gap, same


def test_tn_kloop_inputs_are_well_conditioned_and_can_tell_the_planted_mistakes():
    """Per distinct shape of TN_KLOOP_CASES, at the full shape, one reference each: (a) the reference in fp32 against fp64 within
    1e-5 on Y, the loss / h_n / dh0 and every gradient; (b) the step restated around _TnProduct, whose backward forms both
    weight-gradient products chunk by chunk and stage by stage, agrees with the reference to 1e-12 relative to max (not bit
    for bit: another order of fp64 sums); (c) each mistake of MISTAKES that applies to a keyed product of the shape, planted
    into that product alone, moves its weight or bias gradient by more than 10 x 1e-4 of max.  The un-zeroed tail (TAIL) and the
    effects in one-pass bars are printed, not asserted."""
    t0 = time.time()
    shapes = _shapes()
    report, problems, worst_gap, worst_same = [], [], {}, 0.0
    for shape, walks in shapes.items():
        bad, gap, same = input_problems(shape, walks, report)
        problems += bad
        for k, e in gap.items():
            k = k if k in ("Y", "hn", "loss", "dh0") else "gradients"
            worst_gap[k] = max(worst_gap.get(k, 0.0), e)
        worst_same = max(worst_same, max(same.values()))
    by_m = {}
    for shape, role, m, e in report:
        lo, hi, n = by_m.get((role, m), (1e30, 0.0, 0))
        by_m[(role, m)] = (min(lo, e), max(hi, e), n + 1)
    for (role, m), (lo, hi, n) in sorted(by_m.items()):
        print("%-6s %-50s %2d shapes: moves the product's gradients by %.1e ... %.1e of max (%.3g ... %.3g one-pass bars of %.0e)"
              % (role, m, n, lo, hi, lo / F16_G_BAR, hi / F16_G_BAR, F16_G_BAR))
    print("fp32 against fp64 at most %s; restated step against the reference at most %.1e; %d shapes in %.0f s"
          % (" ".join("%s=%.1e" % kv for kv in sorted(worst_gap.items())), worst_same, len(shapes), time.time() - t0))
    assert problems == []
    assert {m for _, _, m, _ in report} == set(MISTAKES) | {TAIL}
    # TN_KLOOP_B_MOVED: every B from the rule's up to the tabled one that keeps the rule's conditions fails (a), the tie check or the single-plane check
    for (S, H), moved in ic.TN_KLOOP_B_MOVED.items():
        mine = [c for c in ic.TN_KLOOP_CASES if c[8] and (c[2], c[5]) == (S, H)]
        rule = {smallest_b(c[1], S, H, c[6], c[7], c[8], c[9]) for c in mine}
        assert len(rule) == 1 and {c[4] for c in mine} == {moved}, (S, H)
        for B in range(rule.pop(), moved):
            if all(ic.tn_seven(p) for c in mine for p in ic.tn_carried(c[1], S, c[3], B, H, *c[6:])):
                shape = (S, ic.TN_KLOOP_T, B, H, "f32", True)
                bad = [b for b in input_problems(shape, shapes[(S, ic.TN_KLOOP_T, moved, H, "f32", True)], [])[0] if "planted into" not in b]
                print("not taken: %s" % bad[:1])
                assert bad, shape
    # the walk notices a mistake at all: on a small draw the planted product differs, the unplanted one is the plain product
    g = torch.Generator().manual_seed(5)
    Aop, Y, h0 = (torch.randn(n, m, generator=g, dtype=torch.float64) for n, m in ((300, 7), (300, 5), (100, 5)))
    Hprev = torch.cat([h0[:, None], Y.reshape(100, 3, 5)[:, :-1]], 1).reshape(300, 5)
    plain = Aop.t() @ torch.cat([Hprev, torch.ones(300, 1, dtype=torch.float64)], 1)
    assert rel_to_max(tn_walk(Aop, None, Y, h0, 300, 224, 3, True), plain) < 1e-14
    assert rel_to_max(tn_walk(Aop, Hprev, None, None, 300, 96, 0, False), plain) < 1e-14
    for m in MISTAKES + (TAIL,):
        assert rel_to_max(tn_walk(Aop, None, Y, h0, 300, 224, 3, True, m), plain) > 1e-3, m
