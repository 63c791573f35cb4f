"""GPU: every operator's lowering per attribute form, layout and batch -- the table of tests/op_cases.py on the device, at fusion 0 and 2, with 1 and 3 pushed
samples, every sample checked:
  * "move" cases equal the float64 restatement bit for bit;
  * "elementwise" cases are within one f16 ulp of the float64 value rounded to f16 (osg_elementwise.hip: f32 arithmetic, one rounding); Add, Sub, Mul and Neg
    also equal numpy's f32 operation rounded once;
  * "reduce" cases stay inside the bound of the kernel-level test of the same kernel (op_cases.BOUNDS says which);
  * where the reference computes the case (tests/golden/op_cases.npz), err16 = max|got - ref16| / max|ref32| <= 1e-3, the single-pattern rule of
    tests/test_golden.py;
  * sample k of the 3-push run equals the 1-push run of the same inputs bit for bit.
Refusals and the empty-operand cases run on the stub only (tests/test_op_lowering_cpu.py): nothing here launches on invalid input.  The figures measured on an
MI355X are in profiles/op_lowering_table.txt (tools/op_lowering_table.py prints them)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import op_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu


def run(case, pushes, fusion, first=0):
    """a device fault ends the session: nothing more is launched on a device that has reported one"""
    from onnxstream_amd.bindings import OnnxStreamError
    try:
        return oc.run_case(case, pushes, fusion, first)
    except OnnxStreamError as e:
        if "memory access" in str(e) or "hipError" in str(e):
            pytest.exit(f"{case.name}: the device reported a fault: {e}", returncode=3)
        raise


@pytest.mark.parametrize("fusion", [0, 2])
@pytest.mark.parametrize("case", oc.device_cases(), ids=lambda c: c.name)
def test_case_on_the_device(case, fusion):
    three = run(case, 3, fusion)
    for o in case.outs:
        n = 1 if o in case.const_out else 3
        assert len(three[o]) == n, (o, len(three[o]))
    for k in range(3):
        one = run(case, 1, fusion, first=k)
        for o in case.outs:
            if o in case.const_out and k:
                continue
            for pushes, got in ((1, one[o][0]), (3, three[o][k])):
                fig, bad = oc.figures(case, o, got, k)
                print(f"{case.name} fusion {fusion} pushes {pushes} sample {k} {o}: {fig}")
                assert not bad, (o, pushes, k, bad)
                gold = oc.golden(case, o) if k == 0 else None
                if gold:
                    e = oc.err16(got, *gold)
                    print(f"{case.name} fusion {fusion} pushes {pushes} {o}: err16 {e:.2e}")
                    assert e <= 1e-3, (o, pushes, e)
            assert np.array_equal(oc.bits(one[o][0]), oc.bits(three[o][k])), (o, k, "sample k of the 3-push run differs from its 1-push run")
