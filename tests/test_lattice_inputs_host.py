"""The lattice draw of tests/lattice_inputs.py, qualified on the fp64 oracle alone (no GPU): for every distinct shape of
tests/test_gpu_lattice.py's cases the pre-activations are exact odd multiples of the grid step (so no ReLU tie exists at any
size and any summation order gives the same bits), the masks are live, the oracle's own fp32 evaluation stays within a tenth of
the bar of its fp64 one, and every wrong kernel of lattice_inputs.MUTATIONS -- a mask taken from the next station, a conv bias
dropped or mis-indexed, A where A^T belongs -- moves Y or a gradient by more than 100 bars.  A failure of a GPU case on these
inputs is therefore a finding about the kernel.  The figures are printed per shape."""
import numpy as np
import pytest
import torch

import instance_cases as ic
import lattice_inputs as li
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, Y_TOL
from test_gpu_series import TOL as SERIES_TOL
from test_gpu_series_instances import windows
from test_gpu_state_train import _tols

STEPS = (1 / 32, 1 / 512)
MARGIN = 5e-5             # five times the series suites' 1e-5 rule; an odd multiple of 1/512 below 30 gives >= 6.5e-5
LIVENESS = 0.20
IODT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _fp32_grade_bar(runs):
    """The gradient bar of a shape's cases, the one-pass fp16 ones aside (every shape has an fp32-grade case): what a mutation
    has to exceed a hundredfold."""
    S, T, B, H, maths = runs
    bars = [_tols("f16x3g_big" if (m == "f16x3g" and B * T >= 4096) else "", m, IODT[io])[1] for m, io in maths if m != "f16"]
    assert bars
    return max(bars)


def _qualify(tag, A, X, L, p, bar, f16_exact):
    """(a) .. (f) of one shape; returns the printed line's figures."""
    from oracle import windgnn_oracle as orc
    Zs, operands = li.preacts(A, X, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"])
    m = li.measure(Zs, STEPS)
    for layer, r in enumerate(m, 1):
        assert r["odd"] and r["qmax"] * (STEPS[layer - 1] * 512) < 2 ** 24, (tag, layer, r)      # (a): Z * 512 odd, below 2^24
        assert r["margin"] > MARGIN, (tag, layer, r)                                            # (b)
        assert r["varies"] >= LIVENESS, (tag, layer, r)                                         # (d)
    if f16_exact:                                                                               # (c)
        for t in operands:
            assert torch.equal(t.half().double(), t.double()), tag
    p64 = {k: v.double() for k, v in p.items()}
    Yo, loss_o, go = orc.train_step(A.double(), X.double(), L.double(), p64)
    Y32, loss32, g32 = orc.train_step(A, X, L, p)
    gap = {"Y": max_abs(Y32, Yo), "loss": abs(float(loss32) - float(loss_o)) / max(1.0, float(loss_o))}
    gap.update({k: rel_to_max(g32[k], go[k]) for k in PARAM_KEYS})
    worst = max(gap, key=gap.get)
    eff = li.mutation_effects(A, X, L, p)
    print("%s: margin %.1e / %.1e, mask varies %.2f / %.2f, live %.2f / %.2f, max g %.1f, fp32 - fp64 %.1e (%s); mutations: %s"
          % (tag, m[0]["margin"], m[1]["margin"], m[0]["varies"], m[1]["varies"], m[0]["live"], m[1]["live"],
             float(Zs[1].max()), gap[worst], worst, ", ".join("%s %.2g" % kv for kv in eff.items())))
    assert gap[worst] <= min(Y_TOL, G_TOL) / 10, (tag, gap)                                      # (e)
    for name, e in eff.items():                                                                 # (f)
        assert e > 100 * bar, (tag, name, e, bar)
    return eff


def test_window_shapes_qualify():
    shapes = li.window_shapes()
    assert len(shapes) == 4 + 2 + 3 + 3 + 6
    for (S, T, B, H, sparse, shift), maths in shapes.items():
        d = li.draw(S, T, B, H, sparse, shift)
        assert not torch.equal(d.A, d.A.t()) and bool((d.p["conv1.bias"] != 0).all()) and bool((d.p["conv2.bias"] != 0).all())
        assert float(d.X.min()) < 0 < float(d.X.max())
        bar = _fp32_grade_bar((S, T, B, H, maths))
        _qualify("S%d T%d B%d H%d%s" % (S, T, B, H, " csr" if sparse else ""), d.A, d.X, d.L, d.p, bar,
                 any(m == "f16" for m, _ in maths))


def test_series_shapes_qualify():
    shapes = list(dict.fromkeys(c[:7] for c in li.SERIES_CASES))
    assert len(shapes) == 2
    for S, H, rows, T, stride, n, seed in shapes:
        d = li.draw_series(S, H, rows, T, stride, n, seed)
        _qualify("series S%d H%d rows%d" % (S, H, rows), d.A, windows(d.Xs, T, stride, n), windows(d.Ls, T, stride, n), d.p,
                 SERIES_TOL, False)


def test_the_check_notices_a_missing_bias_and_a_symmetric_adjacency():
    """Deleting a conv bias from the draw, or symmetrising A, fails the qualification."""
    d = li.draw(34, li.T_, li.B_, li.H_)
    for k in ("conv1.bias", "conv2.bias"):
        with pytest.raises(AssertionError):
            _qualify("no " + k, d.A, d.X, d.L, dict(d.p, **{k: torch.zeros(13)}), G_TOL, False)
    with pytest.raises(AssertionError):
        _qualify("symmetric", (d.A + d.A.t()) / 2, d.X, d.L, d.p, G_TOL, False)


def test_the_instance_suites_draw_cannot_see_a_wrong_station_mask():
    """Why this file exists: at (S, T, B, H) = (5, 3, 17, 9) with tests/test_gpu_instances.py's draw the conv2 mask is the same
    at every station, so a backward that reads it from the next station computes the very same gradients."""
    from oracle import windgnn_oracle as orc
    S, T, B, H = 5, 3, 17, 9
    g = torch.Generator().manual_seed(31 * S + 7 * T + B + 101 * H)
    A = torch.rand(S, S, generator=g) / S + 0.01
    X = torch.rand(B, T, S, 13, generator=g)
    L = torch.rand(B, T, H, generator=g)
    p = orc.init_params(S, 13, H, seed=ic.param_seed(S, H))
    eff = li.mutation_effects(A, X, L, p)
    assert eff[li.MUTATIONS[1]] == 0.0 and eff[li.MUTATIONS[3]] == 0.0, eff


def _blob_halves(csr):
    """(A, AT) as dense fp64 matrices decoded from the words of a CsrAdjacency blob: rowptr | col | val, twice."""
    S, nnz = csr.S, csr.nnz
    w = csr.blob.cpu().numpy()
    out = []
    for base in (0, S + 1 + 2 * nnz):
        rowptr, col = w[base:base + S + 1], w[base + S + 1:base + S + 1 + nnz]
        val = w[base + S + 1 + nnz:base + S + 1 + 2 * nnz].view(np.float32)
        assert rowptr[0] == 0 and rowptr[-1] == nnz and (np.diff(rowptr) >= 0).all()
        M = np.zeros((S, S))
        rows = np.repeat(np.arange(S), np.diff(rowptr))
        assert all((np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(S))          # ascending inside a row
        M[rows, col] = val
        out.append((M, np.diff(rowptr)))
    return out


def test_csr_blob_holds_the_transpose_of_an_asymmetric_adjacency():
    """The second half of the blob is A^T -- not a copy of A -- with ragged rows and empty ones; and the oracle tells the two
    apart: the AT half replaced by A's own rowptr / col / val is mutation 'A in place of A^T' on csr.dense()."""
    from windgnn_amd.graph import CsrAdjacency
    for S, T, B, H, shift in li.CSR_SHAPES:
        d = li.draw(S, T, B, H, True, shift)
        csr = CsrAdjacency.from_dense(d.A)
        assert torch.equal(csr.dense(), d.A)
        (M, len_a), (MT, len_t) = _blob_halves(csr)
        A = d.A.double().numpy()
        assert (M == A).all() and (MT == A.T).all() and not (MT == A).all(), S
        assert len(set(len_a.tolist())) >= 4 and len_a.min() >= 1 and len_a.max() <= 6, S       # ragged rows
        assert len_t.min() == 0 or S < 100, S                                                  # A^T has empty rows
        assert float(d.A.sum(1).max()) <= 1.0 and float(d.A.min()) >= 0.0


def test_layer_shapes_qualify():
    """The general GraphConvLayer cases: Z an odd multiple of 1/32, live masks, and a dropped bias or A for A^T in dX shows."""
    for cid, S, Fi, Fo, nt in li.LAYER_CASES:
        d = li.draw_layer(S, Fi, Fo, nt)
        (Z,), _ = li.preacts(d.A, d.X, d.W, d.b)
        (r,) = li.measure([Z], STEPS[:1])
        assert r["odd"] and r["margin"] > MARGIN and r["varies"] >= LIVENESS, (cid, r)
        out = torch.relu(Z)
        no_bias = max_abs(torch.relu(Z - d.b.double()), out)
        dZ = d.dout.double() * (Z > 0)
        dP = torch.matmul(dZ, d.W.double().t())
        dX, dX_wrong = torch.matmul(d.A.double().t(), dP), torch.matmul(d.A.double(), dP)
        print("%s: margin %.1e, mask varies %.2f, live %.2f; bias dropped %.2g, A for A^T in dX %.2g"
              % (cid, r["margin"], r["varies"], r["live"], no_bias, rel_to_max(dX_wrong, dX)))
        assert no_bias > 100 * 1e-5 and rel_to_max(dX_wrong, dX) > 100 * 1e-5, cid


def test_every_dense_key_is_in_the_dispatchers_plan():
    for cid, keys, S, T, B, H, math, io, state, route, sparse, shift in li.CASES:
        if not sparse:
            expected = ic.plan(S, T, B, H, math, io, state, route)
            assert set(keys) <= set(expected), (cid, keys, expected)
    for S, H, rows, T, stride, n, seed, route in li.SERIES_CASES:
        assert ic.series_plan(S, H, rows, T, stride, n, route)


def test_one_pass_fp16_reference_figures():
    """The operand rounding of the one-pass fp16 mode on the reference alone, per 'f16' case: the table's figures are these."""
    seen = {}
    for cid, keys, S, T, B, H, math, io, state, route, sparse, shift in li.CASES:
        if math != "f16":
            continue
        d = li.draw(S, T, B, H, sparse, shift)
        Y, loss, g = li.fp64_step(d.A, d.X, d.L, d.p)
        Yr, loss_r, gr = li.fp64_step(d.A, d.X, d.L, d.p, f16_operands=True)
        fig = (max_abs(Yr, Y), abs(loss_r - loss) / max(1.0, loss), max(rel_to_max(gr[k], g[k]) for k in PARAM_KEYS))
        print("%s: Y %.2e (bar %.1e)  loss %.2e (2e-3)  gradients %.2e (%.1e)" % ((cid, fig[0], F16_Y_TOL, fig[1], fig[2], F16_G_TOL)))
        seen[cid] = fig
    assert set(seen) == set(li.F16_FIGURES), (sorted(seen), sorted(li.F16_FIGURES))
    for cid, fig in seen.items():
        for a, b in zip(fig, li.F16_FIGURES[cid]):
            assert abs(a - b) <= 0.05 * b, (cid, fig, li.F16_FIGURES[cid])
