"""The general path's loops, checked without a GPU: tests/general_cases.py's restatement of the persistent CSR layers against
the text of csrc/general.hip, tests/instance_cases.py's gemm_f32_products() against plan(), both tables re-derived by rule, and the
inputs of tests/test_gpu_general_loops.py qualified on the fp64 oracle alone -- invariants (a) to (f) of
tests/test_lattice_inputs_host.py for the CSR shapes, fp32 against fp64 for the GEMM shapes, and for both a restated fp64 step
that equals the oracle's bit for bit and into which the mistakes a loop's second trip can make are planted: each must move Y or a
gradient by more than 10 x 1e-4.  A failure of a GPU case on these inputs is therefore a finding about the kernel."""

import pytest
import torch

import general_cases as gc
import instance_cases as ic
import lattice_inputs as li
import test_instance_table_host as tith
import test_lattice_inputs_host as tli
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_parity import G_TOL, Y_TOL

BAR = 1e-4                                          # the fp32-grade bar (Y_TOL, G_TOL); a planted mistake must exceed gc.PLANT_FACTOR x it
assert BAR == Y_TOL == G_TOL


# ==== A. the CSR layers ==========================================================================================================
def test_csr_plan_restates_the_source():
    src = tith._read("general.hip")
    const = lambda name: tith._ints(r"constexpr int %s = (\d+);" % name, src, name)
    assert const("CT") == [gc.CT] and const("CH") == [gc.CH] and const("CSR_BLOCKS") == [gc.CSR_BLOCKS]
    assert const("CSR_FWD_RPT") == [gc.CSR_FWD_RPT]
    fwd = tith._body(src, "__global__ void __launch_bounds__(CT) csr_layer_fwd_kernel(")
    bwd = tith._body(src, "__global__ void __launch_bounds__(CT) csr_layer_bwd_kernel(")
    assert "constexpr int RPT = CSR_FWD_RPT, RB = CT * RPT;" in fwd
    assert tith._ints(r"constexpr int RPT = (\d+), RB = CT \* RPT;", bwd, "the backward's RPT") == [gc.CSR_BWD_RPT]
    loop = "for (int item = blockIdx.x; item < nitems; item += gridDim.x) {"
    assert loop in fwd and loop in bwd and "const int nitems = csr_items(ntiles, S, RB);" in fwd and "double acc64[4]" in bwd
    # csr_item / csr_items / csr_grid, line by line
    for line in ("if (S >= RB) {", "const int nrb = (S + RB - 1) / RB;", "it.tile0 = item / nrb;", "it.row0 = (item - it.tile0 * nrb) * RB;",
                 "it.nrows = min(RB, S - it.row0);", "it.VC = S;", "const int G = RB / S;", "it.tile0 = item * G;",
                 "it.ng = min(G, ntiles - it.tile0);", "it.nrows = it.ng * S;", "it.VC = it.nrows;",
                 "return S >= RB ? ntiles * ((S + RB - 1) / RB) : (ntiles + RB / S - 1) / (RB / S);",
                 "const int n = csr_items(ntiles, S, CT * rpt);", "return n < CSR_BLOCKS ? (n < 1 ? 1 : n) : CSR_BLOCKS;",
                 "for (int c0 = 0; c0 < VC; c0 += CH) {",
                 "const dim3 grid(cdiv_i(S, ROWS), ntiles < %d ? ntiles : %d);" % (gc.SPMM_GRID_Y, gc.SPMM_GRID_Y),
                 "for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {"):
        assert line in src, "general.hip no longer has %r" % line
    # the items of a launch cover every (tile, row) exactly once, in every regime
    for S, ntiles in ((7, 1), (7, 293), (100, 41), (700, 5), (1024, 3), (1025, 3), (2047, 2), (2048, 3), (2049, 3), (4501, 2)):
        RB = gc.CT * gc.CSR_FWD_RPT
        seen = {}
        for item in range(gc.csr_items(ntiles, S, RB)):
            tile0, ng, row0, nrows, VC = gc.csr_item(item, ntiles, S, RB)
            assert 1 <= nrows <= RB and ng >= 1 and VC == (S if S >= RB else nrows)
            for v in range(nrows):
                g = 0 if ng == 1 else v // S
                key = (tile0 + g, row0 + v - g * S)
                assert key not in seen
                seen[key] = item
        assert len(seen) == ntiles * S and max(k[0] for k in seen) == ntiles - 1 and max(k[1] for k in seen) == S - 1
    assert gc.csr_plan(100, 5141) == dict(items=258, regime="group", tiles_per_item=20, ng_last=1, last_rows=100, row_blocks=1, chunks=1,
                                          grid=256, max_items_per_block=2, later=[256, 257])
    p = gc.csr_plan(2049, 130)
    assert (p["items"], p["regime"], p["row_blocks"], p["chunks"], p["last_rows"], p["later"]) == (260, "rowblock", 2, 2, 1, [256, 257, 258, 259])
    assert gc.spmm_trips(16384) == 1 and gc.spmm_trips(16385) == 2


def csr_loop_problems(shapes):
    """What is wrong with `shapes` as gc.CSR_LOOP_SHAPES: a list of sentences."""
    bad = []
    regimes = {}
    for S, T, B, H, shift, seed in shapes:
        p = gc.csr_plan(S, B * T)
        regimes.setdefault(gc.CSR_LOOP_REGIMES.get(S, p["regime"]), []).append(S)
        if p["items"] <= gc.CSR_BLOCKS:
            bad.append("S = %d: %d items on %d blocks: no block runs a second item" % (S, p["items"], gc.CSR_BLOCKS))
            continue
        if len(p["later"]) < 2:
            bad.append("S = %d: %d items: fewer than two blocks run two items" % (S, p["items"]))
        ragged = p["ng_last"] < p["tiles_per_item"] if p["regime"] == "group" else p["last_rows"] < gc.CT * gc.CSR_FWD_RPT
        if not ragged:
            bad.append("S = %d: the last item is full" % S)
        if p["regime"] != gc.CSR_LOOP_REGIMES.get(S):
            bad.append("S = %d runs the %s geometry, the table says %s" % (S, p["regime"], gc.CSR_LOOP_REGIMES.get(S)))
        if T not in (1, 2) or H != gc.CSR_LOOP_H:
            bad.append("S = %d: T = %d, H = %d; the table keeps T = 1 or 2 and H = %d" % (S, T, H, gc.CSR_LOOP_H))
        smaller = gc.csr_plan(S, (B - 1) * T) if B > 1 else None
        if smaller and len(smaller["later"]) >= 2 and smaller["items"] > gc.CSR_BLOCKS and (
                smaller["ng_last"] < smaller["tiles_per_item"] if smaller["regime"] == "group" else True):
            bad.append("S = %d: B = %d would do" % (S, B - 1))
    bad += ["no shape runs the %s geometry" % r for r in ("group", "tile", "rowblock") if r not in regimes]
    return bad


def test_csr_loop_shapes_run_two_items_per_block_in_every_geometry():
    assert csr_loop_problems(gc.CSR_LOOP_SHAPES) == []
    assert [(s[0], s[1] * s[2]) for s in gc.CSR_LOOP_SHAPES] == [(100, 5141), (700, 515), (1100, 258), (2049, 130)]
    plans = {s[0]: gc.csr_plan(s[0], s[1] * s[2]) for s in gc.CSR_LOOP_SHAPES}
    assert [plans[S]["items"] for S in (100, 700, 1100, 2049)] == [258, 258, 258, 260]
    assert [plans[S]["tiles_per_item"] for S in (100, 700, 1100, 2049)] == [20, 2, 1, 1]
    assert plans[700]["ng_last"] == 1 and 2 * 700 - gc.CT == 376 and 1100 - gc.CT == 76 and plans[2049]["last_rows"] == 1
    assert (100 * 13) % 4 == 0 and (2049 * 13) % 2 == 1                                # the 16-byte and the scalar copy-out
    # the cases: f32 and f16x3 on the training route everywhere, one-pass f16 at S = 700, the stash-less forward once per shape
    assert len(gc.CSR_LOOP_CASES) == 4 * 3 + 1
    by = {}
    for cid, S, T, B, H, shift, seed, mth, route in gc.CSR_LOOP_CASES:
        assert (S, T, B, H, shift, seed) in gc.CSR_LOOP_SHAPES
        by.setdefault(S, []).append((mth, route))
    assert all(sorted(v) == sorted([("f32", "train"), ("f16x3", "train"), ("f16x3", "infer")] + ([("f16", "train")] if S == 700 else []))
               for S, v in by.items()) and len(by) == 4
    assert gc.LAYER_LOOP_CASES == [(700, 515), (7, 16385)]
    assert gc.csr_plan(700, 515)["max_items_per_block"] == 2 and gc.spmm_trips(16385) == 2 and gc.csr_plan(7, 16385)["items"] == 57
    # ... and the checks notice: a deleted shape, 256 items, a full last item
    assert csr_loop_problems(gc.CSR_LOOP_SHAPES[:2] + gc.CSR_LOOP_SHAPES[3:]) == ["no shape runs the tile geometry"]
    assert csr_loop_problems(gc.CSR_LOOP_SHAPES[:3]) == ["no shape runs the rowblock geometry"]
    assert csr_loop_problems([(100, 1, 5120, 6, -4, 0)] + gc.CSR_LOOP_SHAPES[1:]) == ["S = 100: 256 items on 256 blocks: no block runs a second item"]
    assert csr_loop_problems([(100, 1, 5160, 6, -4, 0)] + gc.CSR_LOOP_SHAPES[1:])[0] == "S = 100: the last item is full"
    assert csr_loop_problems([(100, 1, 5121, 6, -4, 0)] + gc.CSR_LOOP_SHAPES[1:]) == ["S = 100: 257 items: fewer than two blocks run two items"]
    assert csr_loop_problems([(100, 1, 5142, 6, -4, 0)] + gc.CSR_LOOP_SHAPES[1:]) == ["S = 100: B = 5141 would do"]
    assert csr_loop_problems(gc.CSR_LOOP_SHAPES[:3] + [(2049, 2, 64, 6, -7, 9)]) == ["S = 2049: 256 items on 256 blocks: no block runs a second item"]


def test_no_earlier_csr_parity_shape_ran_two_items_per_block():
    """The blind spot, asserted once: every CSR shape that was compared with the fp64 oracle gives each block at most one item."""
    import test_gpu_parity as tgp
    marks = [m for m in tgp.test_csr_adjacency_against_oracle.pytestmark if m.name == "parametrize" and m.args[0] == "S,T,B,H,k"]
    literal = [(S, T * B) for S, T, B, H, k in marks[0].args[1]]
    assert len(literal) == 7 and (2500, 4) in literal
    lattice = [(S, T * B) for S, T, B, H, shift in li.CSR_SHAPES]
    tiles = sorted(n for _, n in literal + lattice)
    assert max(tiles) == 30 and max(n for _, n in lattice) == 15
    for S, n in literal + lattice:
        p = gc.csr_plan(S, n)
        assert p["max_items_per_block"] == 1 and p["items"] <= 30 and p["later"] == [], (S, n, p)
    # the random sweep (B <= 9, T <= 4, S <= 2600) and the finish test (12 tiles): at most 36 tiles, 72 items
    assert max(gc.csr_plan(S, 36)["items"] for S in (2, 64, 65, 700, 1023, 1025, 2047, 2048, 2600)) == 72 < gc.CSR_BLOCKS


# ---- the restated step and the three mistakes ---------------------------------------------------------------------------------
def _later_rows(S, ntiles):
    """Per mistake, what the second trips of a launch touch: the plan; src1: tile -> the tile whose source a stale LDS buffer
    holds (the same position of the item one grid stride earlier); first [ntiles, S]: rows of each two-item block's FIRST item;
    src3: tile -> the first tile of its item for the last tile of a later multi-tile item; chunk2: tiles of later row-block items."""
    RB = gc.CT * gc.CSR_FWD_RPT
    p = gc.csr_plan(S, ntiles)
    src1, src3 = torch.arange(ntiles), torch.arange(ntiles)
    first = torch.zeros(ntiles, S, dtype=torch.bool)
    chunk2 = []
    for item in p["later"]:
        tile0, ng, row0, nrows, VC = gc.csr_item(item, ntiles, S, RB)
        e0, eg, er0, enr, _ = gc.csr_item(item - p["grid"], ntiles, S, RB)
        assert er0 == row0                                            # (256 is a multiple of the row blocks per tile)
        for g in range(ng):
            src1[tile0 + g] = e0 + g
        if eg == 1:
            first[e0, er0:er0 + enr] = True
        else:
            first[e0:e0 + eg] = True
        if p["regime"] == "rowblock":
            chunk2.append(tile0)
        elif ng > 1:
            src3[tile0 + ng - 1] = tile0
    return p, src1, first, src3, sorted(set(chunk2))


def csr_loop_step(A, X, L, params, mistake=None):
    """lattice_inputs.fp64_step restated -- the same operations in the same order, so the same bits -- with one of gc.MISTAKES
    planted into both layers' launches."""
    leaves = {k: params[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}
    A, X, L = A.double(), X.double(), L.double()
    B, T, S, F = X.shape
    p, src1, first, src3, chunk2 = _later_rows(S, B * T)

    def layer(In, W, b):
        if mistake is None:
            return torch.relu(torch.matmul(torch.matmul(A, In), W) + b)
        tiles = In.reshape(B * T, S, F)
        if mistake == gc.MISTAKES[0]:
            tiles = tiles[src1]
        elif mistake == gc.MISTAKES[2] and p["regime"] != "rowblock":
            tiles = tiles[src3]
        P = torch.matmul(A, tiles)
        if mistake == gc.MISTAKES[2] and p["regime"] == "rowblock":
            keep = torch.ones(B * T, 1, 1, dtype=torch.float64)
            keep[chunk2] = 0.0
            P = keep * P + (1.0 - keep) * torch.matmul(A[:, :gc.CH], tiles[:, :gc.CH])
        Z = torch.matmul(P, W) + b
        if mistake == gc.MISTAKES[1]:
            Z = torch.where(first[:, :, None], torch.matmul(P, W.detach()) + b.detach(), Z)
        return torch.relu(Z).reshape(B, T, S, F)

    h = layer(X, leaves["conv1.weight"], leaves["conv1.bias"])
    h = layer(h, leaves["conv2.weight"], leaves["conv2.bias"])
    H = params["gru.weight_hh_l0"].shape[1]
    Y, _ = torch._VF.gru(h.reshape(B, T, S * F), torch.zeros(1, B, H, dtype=torch.float64),
                         [leaves[k] for k in PARAM_KEYS[4:]], True, 1, 0.0, False, False, True)
    loss = ((Y - L) ** 2).mean()
    loss.backward()
    return Y.detach(), float(loss), {k: leaves[k].grad for k in PARAM_KEYS}


def _margins(d):
    Zs, _ = li.preacts(d.A, d.X, d.p["conv1.weight"], d.p["conv1.bias"], d.p["conv2.weight"], d.p["conv2.bias"])
    return [r["margin"] for r in li.measure(Zs, tli.STEPS)]


def _gi_max(d):
    from oracle import windgnn_oracle as orc
    _, cache = orc.forward(d.A.double(), d.X.double(), {k: v.double() for k, v in d.p.items()})
    return float(cache["GI"].abs().max())


def csr_input_problems(shape, factor=gc.PLANT_FACTOR):
    """What is wrong with the inputs of one shape of gc.CSR_LOOP_SHAPES, on the oracle alone: a list of sentences."""
    S, T, B, H, shift, seed = shape
    bad = []
    d = li.draw(S, T, B, H, True, shift, seed)
    assert not torch.equal(d.A, d.A.t()) and bool((d.p["conv1.bias"] != 0).all()) and bool((d.p["conv2.bias"] != 0).all())
    # the tabled seed is the first of 0 .. 19 that meets invariant (b)
    assert 0 <= seed < gc.CSR_LOOP_SEEDS
    for s in range(seed):
        m = _margins(li.draw.__wrapped__(S, T, B, H, True, shift, s))
        if min(m) > tli.MARGIN:
            bad.append("S = %d: seed %d already meets invariant (b) (%.1e, %.1e); the table says %d" % (S, s, m[0], m[1], seed))
    # the tabled shift is the largest power of two that brings max |GI| below 8
    gi = _gi_max(d)
    if not gi < gc.CSR_LOOP_GI_MAX:
        bad.append("S = %d: max |GI| = %.1f at shift %d: the gates saturate" % (S, gi, shift))
    if shift < 0 and _gi_max(li.draw.__wrapped__(S, T, B, H, True, shift + 1, seed)) < gc.CSR_LOOP_GI_MAX:
        bad.append("S = %d: shift %d would do" % (S, shift + 1))
    # invariants (a) to (f), through the lattice test's own helper ((c) where a one-pass fp16 case runs on the shape)
    f16 = any(c[1] == S and c[7] == "f16" for c in gc.CSR_LOOP_CASES)
    tli._qualify("S%d T%d B%d H%d csr loop" % (S, T, B, H), d.A, d.X, d.L, d.p, G_TOL, f16)
    # the restated step is lattice_inputs.fp64_step, bit for bit
    Y, loss, g = li.fp64_step(d.A, d.X, d.L, d.p)
    Yr, lossr, gr = csr_loop_step(d.A, d.X, d.L, d.p)
    assert torch.equal(Yr, Y) and lossr == loss and all(torch.equal(gr[k], g[k]) for k in PARAM_KEYS), S
    regime = gc.csr_plan(S, B * T)["regime"]
    moved = {}
    for m in gc.MISTAKES:
        Ym, _, gm = csr_loop_step(d.A, d.X, d.L, d.p, m)
        moved[m] = (max_abs(Ym, Y), max(rel_to_max(gm[k], g[k]) for k in PARAM_KEYS))
        if m == gc.MISTAKES[2] and regime == "tile":
            # one tile per item and S <= CH: the item has neither a column offset (g = 0) nor a second chunk; nothing to plant
            assert moved[m] == (0.0, 0.0), (S, moved[m])
        elif not max(moved[m]) > factor * BAR:
            bad.append("S = %d: '%s' moves Y by %.1e and no gradient by more than %.1e: pick another seed" % ((S, m) + moved[m]))
        if m == gc.MISTAKES[1]:
            assert moved[m][0] == 0.0                                   # (a backward mistake: the forward is the oracle's)
    print("csr loop S%d T%d B%d (%s, seed %d, shift %d): max |GI| %.2f, max |Y| %.3f; planted (Y, worst gradient): %s"
          % (S, T, B, regime, seed, shift, gi, float(Y.abs().max()), "  ".join("%.1e %.1e" % v for v in moved.values())))
    if f16:
        Yh, lossh, gh = li.fp64_step(d.A, d.X, d.L, d.p, f16_operands=True)
        print("    one-pass fp16 operand rounding on the reference: Y %.2e  loss %.2e  gradients %.2e"
              % (max_abs(Yh, Y), abs(lossh - loss) / max(1.0, loss), max(rel_to_max(gh[k], g[k]) for k in PARAM_KEYS)))
    return bad


@pytest.mark.parametrize("shape", gc.CSR_LOOP_SHAPES, ids=["S%d" % s[0] for s in gc.CSR_LOOP_SHAPES])
def test_csr_loop_inputs_qualify_and_can_tell_the_planted_mistakes(shape):
    assert csr_input_problems(shape) == []


def test_the_csr_input_check_notices_a_mistake_that_stays_under_the_factor():
    """The smallest shape's own figures against a factor no mistake reaches, and an unshifted W_ih: both fail by message."""
    shape = gc.CSR_LOOP_SHAPES[0]
    got = csr_input_problems(shape, factor=1e9)
    assert len(got) == 3 and all("pick another seed" in s for s in got), got
    got = csr_input_problems(shape[:4] + (shape[4] + 1,) + shape[5:])
    assert any("the gates saturate" in s for s in got), got


def test_layer_loop_inputs_qualify():
    """The one-layer cases' draw: Z an odd multiple of 1/32 with live masks, and the tile one SpMM grid stride earlier (the dX
    loop's second trip reading its first trip's tile) differs from tile 16 384 itself."""
    for S, nt in gc.LAYER_LOOP_CASES:
        d = li.draw_layer(S, 13, 13, nt)
        (Z,), _ = li.preacts(d.A, d.X, d.W, d.b)
        (r,) = li.measure([Z], tli.STEPS[:1])
        assert r["odd"] and r["margin"] > tli.MARGIN and r["varies"] >= tli.LIVENESS, (S, nt, r)
        assert not torch.equal(d.A, d.A.t())
        dZ = d.dout.double() * (Z > 0)
        dX = torch.matmul(d.A.double().t(), torch.matmul(dZ, d.W.double().t()))
        stride = gc.SPMM_GRID_Y if nt > gc.SPMM_GRID_Y else gc.CSR_BLOCKS * gc.csr_plan(S, nt)["tiles_per_item"]
        wrong = dX.clone()
        wrong[stride:] = dX[:nt - stride]
        assert rel_to_max(wrong, dX) > 100 * 1e-5, (S, nt)


# ==== B. gemm_f32_kernel =========================================================================================================
WINDOW_TABLES = tith.ALL_WINDOW_TABLES + (("GEMM_F32_KLOOP_CASES", ic.GEMM_F32_KLOOP_CASES),
                                          ("GEMM_F32_FOLD_CASES", [c[:10] for c in ic.GEMM_F32_FOLD_CASES]))
NT_KEYS = [k for k in ic.GEMM_F32_NAMES if k.endswith("[kk]") or k.endswith("[kn]")]


def _f32_keys(keys):
    return [k for k in keys if ic.family_of(k) == "gemm_f32_kernel"]


def test_gemm_f32_products_names_exactly_the_gemm_f32_launches_of_plan():
    for name, table in WINDOW_TABLES:
        for fam, key, S, T, B, H, mth, io, state, route in table:
            prods = ic.gemm_f32_products(S, T, B, H, mth, io, state, route)
            assert [p[0] for p in prods] == _f32_keys(ic.plan(S, T, B, H, mth, io, state, route)), (name, key)
            assert all(p[1] in ic.GEMM_F32_ROLES and p[6] >= 1 for p in prods), (name, key, prods)
    for T, B in sorted(tith.PLAIN_TB | tith.THRESHOLD_TB):
        for S in (1, 8, 40, 52, 60):
            for H in (4, 35, 128, 129, 171, 192):
                for state, route in ((0, "train"), (0, "infer"), (1, "train"), (1, "unmerged")):
                    for mth in ("f32", "f16x3"):
                        prods = ic.gemm_f32_products(S, T, B, H, mth, "f32", bool(state), route)
                        assert [p[0] for p in prods] == _f32_keys(ic.plan(S, T, B, H, mth, "f32", bool(state), route)), (S, T, B, H, route)
    # the contraction as the kernel counts it
    src = tith._read("gemm.hip")
    assert "constexpr int BK = %d, LDT" % ic.GEMM_F32_BK in src and "if (since == 512 / BK) {" in src
    assert "p.kchunk = cdiv_i(cdiv_i(g.K, p.splitk), BK) * BK;" in src and "constexpr int RS = MI * NJ == 4 ? 1 : 2;" in src
    assert "if (k0 + (1 + RS) * BK < kend) {" in src and ic.GEMM_F32_FOLD == 32
    assert ic.gemm_f32_products(8, 2, 17, 35, "f32") == [
        ("gemm_f32_kernel<64,128>[kk]", "GI", 34, 105, 104, 1, 7), ("gemm_f32_kernel<64,64>[tn,ones,shift]", "dW_hh", 105, 36, 34, 1, 3),
        ("gemm_f32_kernel<64,128>[tn,ones]", "dW_ih", 105, 105, 34, 1, 3), ("gemm_f32_kernel<64,128>[kn]", "dg", 34, 104, 105, 1, 7)]


def test_the_tables_before_this_half_ran_four_nt_keys_of_gemm_f32_for_one_step():
    """The exact blind-spot table: the most steps any launch of CASES, EDGE_CASES and KLOOP_CASES takes each key of gemm_f32_kernel
    through in one chunk, and the steps of the keyed product of the key's own CASES entry."""
    most = {}
    for _, table in tith.ALL_WINDOW_TABLES:
        for c in table:
            for k, role, M, N, K, sk, steps in ic.gemm_f32_products(*c[2:]):
                if steps > most.get(k, (0,))[0]:
                    most[k] = (steps, role, c[2:6], K, sk)
    keyed = {c[1]: ic.gemm_f32_keyed(c[1], *c[2:]) for c in ic.CASES if c[0] == "gemm_f32_kernel"}
    for k in ic.GEMM_F32_NAMES:
        print("%-42s most steps %3d (%s of S T B H = %s, K = %d, split %d); keyed in CASES: %s, %d steps"
              % ((k,) + most[k] + (keyed[k][0], keyed[k][5])))
    assert {k: most[k][0] for k in NT_KEYS} == {
        "gemm_f32_kernel<64,64>[kk]": 43, "gemm_f32_kernel<64,64>[kn]": 36, "gemm_f32_kernel<64,128>[kk]": 1,
        "gemm_f32_kernel<64,128>[kn]": 1, "gemm_f32_kernel<128,64>[kk]": 12, "gemm_f32_kernel<128,128>[kk]": 1,
        "gemm_f32_kernel<128,128>[kn]": 1}
    assert {k: (keyed[k][0], keyed[k][5]) for k in NT_KEYS} == {
        "gemm_f32_kernel<64,64>[kk]": ("GI", 1), "gemm_f32_kernel<64,64>[kn]": ("dg", 1), "gemm_f32_kernel<64,128>[kk]": ("GI", 1),
        "gemm_f32_kernel<64,128>[kn]": ("dg", 1), "gemm_f32_kernel<128,64>[kk]": ("rec", 12), "gemm_f32_kernel<128,128>[kk]": ("GI", 1),
        "gemm_f32_kernel<128,128>[kn]": ("dg", 1)}
    # only <64,64> reached the fold, and the four TN keys run 3 to 49 steps a chunk
    assert [k for k in NT_KEYS if most[k][0] > ic.GEMM_F32_FOLD] == ["gemm_f32_kernel<64,64>[kk]", "gemm_f32_kernel<64,64>[kn]"]
    tn = [most[k][0] for k in ic.GEMM_F32_NAMES if k not in NT_KEYS]
    assert len(tn) == 4 and min(tn) >= 3 and max(tn) == 49


def _g32(S, T, B, H):
    return H <= 128 and ic.g32_rows(B * T, S, H)


def gemm_kloop_problems(kloops):
    """What is wrong with `kloops` as ic.GEMM_F32_KLOOP_CASES: a list of sentences, empty when every NT key of gemm_f32_kernel whose
    keyed product runs fewer than ic.GEMM_F32_KLOOP_STEPS steps in CASES is claimed once, on its key, through the product of the
    same role, unsplit, at an odd count of at least that many steps and at the rule's dims."""
    bad = []
    base = {c[1]: c for c in ic.CASES if c[0] == "gemm_f32_kernel" and c[1] in NT_KEYS}
    claimed = [c[1] for c in kloops]
    bad += ["%s is claimed %d times" % (k, claimed.count(k)) for k in dict.fromkeys(claimed) if claimed.count(k) > 1]
    most = {key: ic.gemm_f32_keyed(key, *c[2:])[5] for key, c in base.items()}
    for c in kloops:
        fam, key, S, T, B, H, mth, io, state, route = c
        if key not in base:
            bad.append("%s is no NT key CASES claims for gemm_f32_kernel" % key)
            continue
        S0, T0, B0, H0 = base[key][2:6]
        if (fam, T, B) + c[6:] != (base[key][0], T0, B0) + base[key][6:]:
            bad.append("%s: family, T, B, math, io, state and route are not those of its case in CASES" % key)
            continue
        if ic.refusal(S, T, B, H, mth, io) is not None or key not in ic.plan(S, T, B, H, mth, io, state, route):
            bad.append("%s: plan() at S = %d, H = %d does not contain the key" % (key, S, H))
            continue
        if _g32(S, T, B, H):
            bad.append("%s: at S = %d, H = %d the layout is gemm32.hip's" % (key, S, H))
            continue
        role0, steps0 = ic.gemm_f32_keyed(key, *base[key][2:])[0], ic.gemm_f32_keyed(key, *base[key][2:])[5]
        if steps0 >= ic.GEMM_F32_KLOOP_STEPS:
            bad.append("%s: its case in CASES already runs %d K steps" % (key, steps0))
            continue
        mine = ic.gemm_f32_keyed(key, S, T, B, H, mth, io, state, route, role=role0)
        if mine is None:
            bad.append("%s: at S = %d, H = %d the key is not carried by the %s product that carries it in CASES" % (key, S, H, role0))
            continue
        _, M, N, K, sk, steps = mine
        if sk != 1:
            bad.append("%s: the %s product is split %d ways" % (key, role0, sk))
        if steps < ic.GEMM_F32_KLOOP_STEPS or steps % 2 == 0:
            bad.append("%s: the %s product runs %d K steps, not an odd count >= %d" % (key, role0, steps, ic.GEMM_F32_KLOOP_STEPS))
        want = (S0, ic.GEMM_F32_KLOOP_H) if role0 == "dg" else (ic.GEMM_F32_KLOOP_S, H0)
        if (S, H) != want:
            bad.append("%s: S = %d, H = %d, the rule says %d, %d" % ((key, S, H) + want))
        most[key] = max(most[key], steps)
    bad += ["%s runs at most %d K steps in CASES and GEMM_F32_KLOOP_CASES" % (k, n) for k, n in most.items() if n < ic.GEMM_F32_KLOOP_STEPS]
    return bad


def gemm_fold_problems(folds, named=ic.GEMM_F32_FOLD_NAMED):
    """What is wrong with `folds` as ic.GEMM_F32_FOLD_CASES: every tile needs a product of more than ic.GEMM_F32_FOLD steps in one
    unsplit chunk over at least 64 tiles, outside gemm32.hip's layouts; one tile may be covered by naming an existing case."""
    bad = []
    tiles = {}
    key, entry, role = named
    case = next(c for c in ic.CASES if c[1] == entry)
    got = ic.gemm_f32_keyed(key, *case[2:], role=role)
    if got is None or got[5] <= ic.GEMM_F32_FOLD or got[4] != 1:
        bad.append("the named case %s does not run %s past the fold" % (entry, key))
    else:
        tiles[key.split("[")[0]] = entry
    for c in folds:
        fam, key, S, T, B, H, mth, io, state, route, role = c
        if ic.refusal(S, T, B, H, mth, io) is not None or key not in ic.plan(S, T, B, H, mth, io, state, route):
            bad.append("%s: plan() at S = %d, H = %d does not contain the key" % (key, S, H))
            continue
        if _g32(S, T, B, H):
            bad.append("%s: at S = %d, H = %d the layout is gemm32.hip's" % (key, S, H))
            continue
        mine = ic.gemm_f32_keyed(key, S, T, B, H, mth, io, state, route, role=role)
        if mine is None:
            bad.append("%s: at S = %d, H = %d the %s product does not carry the key" % (key, S, H, role))
            continue
        _, M, N, K, sk, steps = mine
        if sk != 1 or ic.gemm_f32_tiles(M, N) < 64:
            bad.append("%s: the %s product is split %d ways (%d tiles)" % (key, role, sk, ic.gemm_f32_tiles(M, N)))
        elif steps <= ic.GEMM_F32_FOLD or K <= 512:
            bad.append("%s: the %s product runs %d K steps: the fold needs %d" % (key, role, steps, ic.GEMM_F32_FOLD + 1))
        else:
            tiles[key.split("[")[0]] = key
    bad += ["no case takes gemm_f32_kernel<%d,%d> past the fold" % t for t in ((64, 64), (64, 128), (128, 64), (128, 128))
            if "gemm_f32_kernel<%d,%d>" % t not in tiles]
    return bad


def test_gemm_f32_kloop_and_fold_cases_follow_the_rule():
    assert gemm_kloop_problems(ic.GEMM_F32_KLOOP_CASES) == []
    assert gemm_fold_problems(ic.GEMM_F32_FOLD_CASES) == []
    assert (ic.GEMM_F32_KLOOP_STEPS, ic.GEMM_F32_KLOOP_S, ic.GEMM_F32_KLOOP_H, ic.GEMM_F32_BK) == (7, 8, 35, 16)
    assert 13 * 8 == 104 == 6 * 16 + 8 and 3 * 35 == 105 == 6 * 16 + 9
    assert [c[1] for c in ic.GEMM_F32_KLOOP_CASES] == [k for k in NT_KEYS if k != "gemm_f32_kernel<128,64>[kk]"]
    assert [(c[1], c[2:6]) for c in ic.GEMM_F32_KLOOP_CASES[-2:]] == [("gemm_f32_kernel<128,128>[kk]", (8, 24, 1537, 129)),
                                                                     ("gemm_f32_kernel<128,128>[kn]", (52, 3, 8161, 35))]
    # the dims the issue of this half confirmed with plan()
    for dims, keys in (((8, 2, 17, 35), ["gemm_f32_kernel<64,128>[kk]", "gemm_f32_kernel<64,128>[kn]"]),
                       ((8, 3, 8161, 192), ["gemm_f32_kernel<128,64>[kk]"]), ((8, 24, 1537, 129), ["gemm_f32_kernel<128,128>[kk]"]),
                       ((52, 3, 8161, 35), ["gemm_f32_kernel<128,128>[kn]"])):
        assert set(keys) <= set(ic.plan(*dims, "f32")), dims
    # K of the fold cases: 520, 520, 520 and 513 -- the last is ONE live column after the fold
    assert [ic.gemm_f32_keyed(c[1], *c[2:10], role=c[10])[3] for c in ic.GEMM_F32_FOLD_CASES] == [520, 520, 520, 513]
    assert {c[6:10] for c in ic.GEMM_F32_KLOOP_CASES + ic.GEMM_F32_FOLD_CASES} == {("f32", "f32", False, "train")}


def test_the_gemm_f32_checks_notice_a_mis_tabled_entry():
    K = ic.GEMM_F32_KLOOP_CASES
    kk, kn = "gemm_f32_kernel<64,128>[kk]", "gemm_f32_kernel<128,128>[kn]"
    at = {k: next(n for n, c in enumerate(K) if c[1] == k) for k in (kk, kn)}

    def with_(key, **kw):
        i = at[key]
        c = dict(zip(("fam", "key", "S", "T", "B", "H", "math", "io", "state", "route"), K[i]))
        c.update(kw)
        return K[:i] + [tuple(c.values())] + K[i + 1:]
    # a deleted case
    for j in (0, at[kn]):
        assert gemm_kloop_problems(K[:j] + K[j + 1:]) == ["%s runs at most 1 K steps in CASES and GEMM_F32_KLOOP_CASES" % K[j][1]]
    # S = 1 / H = 4 put back: the CASES entries themselves
    assert gemm_kloop_problems(with_(kk, S=1)) == [
        "%s: the GI product runs 1 K steps, not an odd count >= 7" % kk, "%s: S = 1, H = 22, the rule says 8, 22" % kk,
        "%s runs at most 1 K steps in CASES and GEMM_F32_KLOOP_CASES" % kk]
    assert gemm_kloop_problems(with_(kn, H=4)) == [
        "%s: the dg product runs 1 K steps, not an odd count >= 7" % kn, "%s: S = 52, H = 4, the rule says 52, 35" % kn,
        "%s runs at most 1 K steps in CASES and GEMM_F32_KLOOP_CASES" % kn]
    # six steps: 13 x 7 = 91, 3 x 32 = 96
    assert gemm_kloop_problems(with_(kk, S=7))[0] == "%s: the GI product runs 6 K steps, not an odd count >= 7" % kk
    assert gemm_kloop_problems(with_(kn, H=32))[0] == "%s: the dg product runs 6 K steps, not an odd count >= 7" % kn
    # eight is even; nine is odd but not the rule's; a split product; a key claimed twice; one that needs no second case
    assert gemm_kloop_problems(with_(kn, H=40))[0] == "%s: the dg product runs 8 K steps, not an odd count >= 7" % kn
    assert gemm_kloop_problems(with_(kn, H=48)) == ["%s: S = 52, H = 48, the rule says 52, 35" % kn]
    assert gemm_kloop_problems(with_(kk, S=10))[0] == "%s: the GI product is split 2 ways" % kk
    assert gemm_kloop_problems(K + [K[0]])[0] == "%s is claimed 2 times" % K[0][1]
    rec = next(c for c in ic.CASES if c[1] == "gemm_f32_kernel<128,64>[kk]")
    assert gemm_kloop_problems(K + [rec]) == ["gemm_f32_kernel<128,64>[kk]: its case in CASES already runs 12 K steps"]
    assert gemm_kloop_problems(with_(kn, T=2)) and gemm_kloop_problems(with_(kk, math="f16x3"))
    # the fold: a deleted case, a 32-step case (K = 512 needs no fold), a split one
    F = ic.GEMM_F32_FOLD_CASES
    assert gemm_fold_problems(F[1:]) == ["no case takes gemm_f32_kernel<64,128> past the fold"]
    assert gemm_fold_problems(F[:2] + F[3:]) == []                                  # <128,128> has two
    assert gemm_fold_problems(F[:2]) == ["no case takes gemm_f32_kernel<128,128> past the fold"]
    short = F[3][:5] + (170,) + F[3][6:]
    assert gemm_fold_problems(F[:2] + [short])[0] == "gemm_f32_kernel<128,128>[kn]: the dg product runs 32 K steps: the fold needs 33"
    few = F[0][:4] + (17,) + F[0][5:]
    assert gemm_fold_problems([few] + F[1:])[0].startswith("gemm_f32_kernel<64,128>[kk]: the GI product is split 8 ways")
    assert gemm_fold_problems(F, named=("gemm_f32_kernel<64,64>[kk]", "gemm_f32_kernel<64,64>[kk]", "GI"))[0].startswith("the named case")


# ---- the inputs of the GEMM cases ---------------------------------------------------------------------------------------------
GEMM_MISTAKES = ("step 3 read from the stage of step 1", "the last partial step left out", "the first 512 columns left out")


def _step_delta(Aop, Bop, mistake):
    """What a mistake of gemm_f32_kernel's K loop adds to C = Aop Bop^T, the operands [rows, K] as the kernel walks them, 16 columns
    a step (no padding: the tail step is masked): step 3 multiplied out of an LDS stage before step 3 was committed to it (the
    stage still holds step 1), the last, partial step never accumulated, or `tot` dropped (the 512 columns before the fold)."""
    K, bk = Aop.shape[1], ic.GEMM_F32_BK
    assert K == Bop.shape[1] and ic.cdiv(K, bk) >= ic.GEMM_F32_KLOOP_STEPS and K % bk != 0
    s1, s3, last = slice(bk, 2 * bk), slice(3 * bk, 4 * bk), slice((K // bk) * bk, K)
    if mistake == GEMM_MISTAKES[0]:
        return torch.matmul(Aop[:, s1], Bop[:, s1].t()) - torch.matmul(Aop[:, s3], Bop[:, s3].t())
    if mistake == GEMM_MISTAKES[1]:
        return -torch.matmul(Aop[:, last], Bop[:, last].t())
    assert mistake == GEMM_MISTAKES[2] and K > 512
    return -torch.matmul(Aop[:, :512], Bop[:, :512].t())


class _Projection32(torch.autograd.Function):
    """tith._InputProjection with gemm.hip's operands: GI = g W_ih^T over K = 13 S columns (b_ih is added in the epilogue),
    dg = dGI W_ih over K = 3 H; plant = (role, mistake of GEMM_MISTAKES) or None."""

    @staticmethod
    def forward(ctx, g, Wih, bih, plant):
        ctx.save_for_backward(g, Wih)
        ctx.plant = plant
        GI = torch.matmul(g, Wih.t()) + bih
        if plant and plant[0] == "GI":
            GI = GI + _step_delta(g.reshape(-1, g.shape[-1]), Wih, plant[1]).reshape(GI.shape)
        return GI

    @staticmethod
    def backward(ctx, dGI):
        g, Wih = ctx.saved_tensors
        dGI2 = dGI.reshape(-1, dGI.shape[-1])
        dW = dGI2.t() @ g.reshape(-1, g.shape[-1])
        db = dGI2.sum(0)
        dg = dGI2 @ Wih
        if ctx.plant and ctx.plant[0] == "dg":
            dg = dg + _step_delta(dGI2, Wih.t(), ctx.plant[1])
        return dg.reshape(g.shape), dW, db, None


def _gemm_shapes():
    """(S, T, B, H) -> the roles of the keyed products and whether a fold case runs on it, in table order."""
    out = {}
    for c in ic.GEMM_F32_KLOOP_CASES:
        role = ic.gemm_f32_keyed(c[1], *next(b for b in ic.CASES if b[1] == c[1])[2:])[0]
        out.setdefault(c[2:6], set()).add((role, False))
    for c in ic.GEMM_F32_FOLD_CASES:
        out.setdefault(c[2:6], set()).add((c[10], True))
    return out


def gemm_input_problems(shape, roles, factor=gc.PLANT_FACTOR):
    from oracle import windgnn_oracle as orc
    from test_gpu_instances import _draw
    S, T, B, H = shape
    d = _draw(S, T, B, H, "f32", False)
    n = min(B, tith.KLOOP_WINDOWS)
    r = dict(A=d["A"], X=d["X"][:n], L=d["L"][:n], p=d["p"])
    Y64, loss64, g64 = orc.train_step(r["A"].double(), r["X"].double(), r["L"].double(), {k: v.double() for k, v in r["p"].items()})
    Y32, _, g32 = orc.train_step(r["A"], r["X"], r["L"], r["p"])
    gap = {"Y": rel_to_max(Y32, Y64)}
    gap.update({k: rel_to_max(g32[k], g64[k]) for k in PARAM_KEYS})
    bad = ["%s: %s in fp32 is %.1e off the fp64 oracle: pick another seed" % (shape, k, e) for k, e in gap.items() if e > 1e-5]
    Yr, lossr, gr = tith.kloop_step(r, projection=_Projection32)
    assert torch.equal(Yr, Y64) and lossr == float(loss64) and all(torch.equal(gr[k], g64[k]) for k in PARAM_KEYS), shape
    for role, fold in sorted(roles):
        moved = {}
        for m in GEMM_MISTAKES[:3 if fold else 2]:
            Ym, _, gm = tith.kloop_step(r, (role, m), projection=_Projection32)
            moved[m] = (max_abs(Ym, Y64), max(rel_to_max(gm[k], g64[k]) for k in PARAM_KEYS))
        print("%s %s%s: seed %d, %d windows, max|Y| %.2f, fp32 against fp64 at most %.1e; planted (Y, worst gradient): %s"
              % (shape, role, " (fold)" if fold else "", ic.param_seed(S, H), n, float(Y64.abs().max()), max(gap.values()),
                 "  ".join("%.1e %.1e" % v for v in moved.values())))
        bad += ["%s: '%s' planted into %s moves Y by %.1e and no gradient by more than %.1e: pick another seed" % ((shape, m, role) + v)
                for m, v in moved.items() if not max(v) > factor * BAR]
    return bad


def test_gemm_f32_inputs_are_well_conditioned_and_can_tell_the_planted_mistakes():
    """Per distinct shape of the two GEMM tables, on the oracle alone and on the first 64 windows of the case's own draw: fp32
    against fp64 within 1e-5; the step restated around _Projection32 equals the oracle's bit for bit; and each K-loop mistake
    planted into the keyed product alone moves Y or some gradient by more than 10 x 1e-4."""
    shapes = _gemm_shapes()
    assert len(shapes) == 10 and sum(fold for roles in shapes.values() for _, fold in roles) == 4
    assert [p for shape, roles in shapes.items() for p in gemm_input_problems(shape, roles)] == []
    # a mistake that stays under the factor fails by message
    shape = next(iter(shapes))
    got = gemm_input_problems(shape, shapes[shape], factor=1e9)
    assert len(got) == 2 and all("pick another seed" in s for s in got), got
