"""The two NT GEMM families past a one-stage K loop, on the MI355X.  tests/test_gpu_instances.py runs every key of
pgemm_nt_kernel and gemm32_nt_kernel at the smallest dims that select it, which for most keys leaves the product that carries
the key a contraction of 32 padded columns: one K stage, no prefetch in flight under a compute phase, no ring slot used twice,
and in gemm32's 128-row form no trip of the main loop at all.  This module runs tests/instance_cases.py's KLOOP_CASES -- the same
keys with the contraction grown to 224 padded columns by rule (H = 74 where the key is carried by dg, S = 17 where by GI): seven
stages, the last with pad columns -- through the same _check: the same launched-name assertions, the same fp64 references and
the same imported tolerances.  One-pass fp16 figures above the imported bars are pinned by ic.KLOOP_F16_EXCEPTIONS, apart from
the H = 4 cases' ic.F16_EXCEPTIONS.  tests/test_instance_table_host.py re-derives the table and qualifies its inputs without a
GPU.  A case reads nothing outside the tree."""
import pytest

import instance_cases as ic
from test_gpu_instances import _check

pytestmark = pytest.mark.gpu

# a shape's call forms run together: they share _reference's fp64 step, and keys of one call form share the GPU step
KLOOPS = sorted(ic.KLOOP_CASES, key=lambda c: (c[2:6], c[7], c[8], ic.MATHS.index(c[6]), c[9], c[1]))


@pytest.mark.parametrize("case", KLOOPS, ids=[c[1] for c in KLOOPS])
def test_nt_k_loop(case):
    _check(case, exceptions=ic.KLOOP_F16_EXCEPTIONS)
