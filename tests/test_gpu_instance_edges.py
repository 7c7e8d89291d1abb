"""The recurrence instances at their edges, on the MI355X.  tests/test_gpu_instances.py runs every key of the six window-major
recurrence families at the BOTTOM of its width bracket and at T = 2, where no kernel executes an interior time step; this module
runs tests/instance_cases.py's EDGE_CASES -- the same 254 keys at the TOP of the bracket (every k slot, hidden column and lane of
the last tile in use, the [h | 1] bias column on a tile edge) and at T = 5 (both parities of the double-buffered state, each
buffer rewritten after it was read) -- through the same _check: the same launched-name assertions, the same fp64 references and
the same imported tolerances.  tests/test_instance_table_host.py re-derives the table and qualifies its inputs without a GPU.

The second half is the one-launch hourly step (csrc/gru_step.hip) at its own edges: the hidden state split at lane 64, the
head / 16-byte body / tail split of a W_ih row by its 4-byte phase, and a ragged last group of four windows."""
import pytest
import torch

import instance_cases as ic
from conftest import PARAM_KEYS, max_abs
from test_gpu_instances import _check
from test_gpu_state import MATH, Y_TOL, _dev, _fp64_forward, _profiled, _setup

pytestmark = pytest.mark.gpu

# a shape's call forms run together: they share _reference's fp64 step (four per shape: two I/O types x the carried state),
# and keys of one call form share the GPU step
EDGES = sorted(ic.EDGE_CASES, key=lambda c: (c[2:6], c[7], c[8], ic.MATHS.index(c[6]), c[9], c[1]))


@pytest.mark.parametrize("case", EDGES, ids=[c[1] for c in EDGES])
def test_recurrence_edge(case):
    _check(case)


# H: one lane, the two sides of the lane-64 split of h (wh[q][0] / wh[q][1]) and of STEP_HMAX, the last unit alone in its
# workgroup of four (65) and a ragged last workgroup (63, 127).  S = 5: I = 65 = 1 (mod 4), so consecutive rows of W_ih start at
# all four 4-byte phases and every head (0..3) / tail combination of the row split occurs; S = 64 = STEP_SMAX: I = 832, every
# 16-byte body chunk slot in use (208 chunks: all STEP_MC = 4 slots of a lane) and the LDS tiles full.  B = 3: three of the
# four windows of a workgroup; B = 5: a full workgroup and one window.
# The model is init_params' draw; at S = 64 gru.weight_ih_l0 is scaled by 2^-5 (exact): its 832 inputs reach 19, and unscaled
# every gate saturates -- at H = 1 the step returns h0 whatever W_ih and W_hh hold (measured on the fp64 reference: zeroing
# either moves nothing).  Scaled, max |W_ih g| is 0.8 ... 2.3 and max |Y| 0.47 ... 0.85, as at S = 5 unscaled (0.9 ... 9.7, 0.66 ... 1.00).
W_IH_SCALE = {5: 1.0, 64: 2.0 ** -5}
STEP_CASES = [(S, B, H) for S in (5, 64) for B in (3, 5) for H in (1, 63, 64, 65, 127, 128)]


@pytest.mark.parametrize("S,B,H", STEP_CASES, ids=["S%d-B%d-H%d" % c for c in STEP_CASES])
def test_hourly_step_edge(S, B, H):
    """One hour from a signed random h0 through gcn_gru_state: ONE launch of gru_step_kernel, Y and h_n against the host fp64
    nn.GRU called with hx at the suite's Y bar."""
    from windgnn_amd.functional import gcn_gru_state
    dev = _dev()
    A_host, A, X, p, params, g = _setup(S, 1, B, H, torch.float32, 0)
    p["gru.weight_ih_l0"] *= W_IH_SCALE[S]
    params = [p[k].to(dev).contiguous() for k in PARAM_KEYS]
    h0 = (torch.rand(B, H, generator=g) * 2 - 1) * 0.8
    Yo, hno = _fp64_forward(A_host, X, p, h0)
    with torch.no_grad():
        (Y, hn), prof = _profiled(lambda: gcn_gru_state(A, X.to(dev), params, MATH["f32"], h0=h0.to(dev)))
    assert prof == {"gru_step_kernel": 1}, prof
    assert tuple(Y.shape) == (B, 1, H) and torch.equal(Y[:, 0], hn)
    e_y, e_h = max_abs(Y.cpu(), Yo), max_abs(hn.cpu(), hno)
    print("step S%d B%d H%d: max|Y| %.2f, against fp64 max|dY| = %.2e, max|dh_n| = %.2e" % (S, B, H, float(Yo.abs().max()), e_y, e_h))
    assert e_y <= Y_TOL and e_h <= Y_TOL, (S, B, H, e_y, e_h)
