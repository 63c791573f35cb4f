"""GPU: every graph rewrite on its forms and near misses -- the table of tests/fusion_cases.py on the device, at fusion levels 0, 1 and 2, one pushed sample; the
"fires" cases also with three samples at level 2.  Every output of every case, the extra outputs included:
  * comes back (never None) with the restatement's shape, finite;
  * err16 = max|got - ref16| / max|ref32| <= 1e-3 against tests/golden/fusion_cases.npz, the single-pattern rule of tests/test_golden.py, the same at every
    level (fusion_cases.EXCEPTIONS holds the figures on record, with 10 % headroom, where a case needs more: DESIGN 6.2);
  * where a case's `out` is ONE launch of a class the kernel tests name (fusion_cases' `rule` at its `cls_levels`), ALSO that class's rule against the float64
    restatement: the SiLU launch within one f16 ulp, Linear / Conv with bias, residual or per-image bias inside the contraction bound, GroupNorm [+ SiLU] and
    LayerNorm inside the bounds of their kernel-level tests, RMSNorm within one f16 ulp;
  * the level 2 plan is the one tests/test_fusion_cases_cpu.py pins on the stub backend;
  * sample k of the three-sample run equals the one-sample run of the same inputs bit for bit.
A "left" or "partial" case whose forbidden rewrite would compute other values is more than 50 tolerances away from them (checked on the CPU), so passing here
means the graph as written was computed.  The module reads tests/golden only.  The figures measured on an MI355X are in profiles/fusion_cases_table.txt
(tools/fusion_cases_table.py writes them)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fusion_cases as fc  # noqa: E402
import op_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu


def run(case, level, pushes=1, first=0):
    """a device fault ends the session: nothing more is launched on a device that has reported one"""
    from onnxstream_amd.bindings import OnnxStreamError
    try:
        return fc.run(case, level, pushes, first)
    except OnnxStreamError as e:
        if "memory access" in str(e) or "hipError" in str(e):
            pytest.exit(f"{case.name}: the device reported a fault: {e}", returncode=3)
        raise


def check(case, level, o, got, k, pushes):
    fig, bad = fc.check_output(case, level, o, got, k)
    print(f"{case.name} level {level} pushes {pushes} sample {k} {o}: {fig}")
    assert not bad, (level, o, pushes, k, bad)


@pytest.mark.parametrize("case", fc.planned(), ids=lambda c: c.name)
def test_case_on_the_device(case):
    for level in fc.LEVELS:
        got, kinds, what = run(case, level)
        for o in case.outs:
            assert len(got[o]) == 1, (level, o, "get_tensor returned None")
            check(case, level, o, got[o][0], 0, 1)
        exp = fc.expected_plan(case, level)
        if exp is not None:
            assert kinds == exp, (level, kinds, exp)


@pytest.mark.parametrize("case", [c for c in fc.planned() if c.expect == "fires"], ids=lambda c: c.name)
def test_fires_case_with_three_samples(case):
    three, kinds, _ = run(case, 2, 3)
    assert kinds == case.plan, (kinds, case.plan)
    for k in range(3):
        one = run(case, 2, 1, first=k)[0]
        for o in case.outs:
            assert len(three[o]) == 3, (o, len(three[o]))
            check(case, 2, o, three[o][k], k, 3)
            assert np.array_equal(oc.bits(one[o][0]), oc.bits(three[o][k])), (o, k, "sample k of the three-sample run differs from its one-sample run")
