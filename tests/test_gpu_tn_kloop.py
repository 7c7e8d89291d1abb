"""The three TN weight-gradient GEMM families past a three-stage K loop, on the MI355X.  tests/test_gpu_instances.py runs every
key of pgemm_tn_kernel, pgemm_tn2_kernel (named pgemm_tn_kernel<TI+TH..>) and gemm32_tn_kernel at the smallest dims that select
it, where a split-K chunk of the B*T rows is two or three stages of 32 rows: no slot of the two-slot LDS ring is rewritten after
it was read twice, the prefetch of stage kt + 1 never runs under compute() from the third stage on, and the window-start mask
never wraps.  This module runs tests/instance_cases.py's TN_KLOOP_CASES -- the same keys at T = 3 with B grown by rule until a
chunk of every product the key carries is seven stages, with a partial final stage in a slot that held an earlier one, and a
bf16-I/O twin of every merged key whose fp32-I/O case forms dW_hh's B rows from fp32 Y -- through the same _check: the same
launched-name assertions, the same fp64 references and the same imported tolerances.  ic.TN_KLOOP_F16_EXCEPTIONS is empty.
tests/test_tn_kloop_host.py re-derives the table and qualifies its inputs without a GPU.  A case reads nothing outside the
tree."""
import pytest

import instance_cases as ic
from test_gpu_instances import _check

pytestmark = pytest.mark.gpu

# a shape's call forms run together: they share _reference's fp64 step, and keys of one call form share the GPU step
TN_KLOOPS = sorted(ic.TN_KLOOP_CASES, key=lambda c: (c[2:6], c[7], c[8], ic.MATHS.index(c[6]), c[9], c[1]))


def _id(c):
    return c[1] if c[7] == "f32" else "%s|io=%s" % (c[1], c[7])


@pytest.mark.parametrize("case", TN_KLOOPS, ids=[_id(c) for c in TN_KLOOPS])
def test_tn_k_loop(case):
    _check(case, exceptions=ic.TN_KLOOP_F16_EXCEPTIONS)
