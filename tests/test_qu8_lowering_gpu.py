"""GPU: the uint8-arithmetic lowering per operator form and both uint8 passes -- the table of tests/qu8_cases.py on the device, every planned case at fusion
levels 0 and 1, one thread.  Four passes per run, the protocol of tests/test_qu8_gpu.py::_run_vae_qu8: input A, A again, 0.37 A + 0.2, A again; from pass 2 on
everything behind the eager prefix (the steps that read per-pass quantisation parameters) is a replayed capture.
  * every pass equals the interpreter (qu8_cases.interpret over oracle/np_qu8.py) for ITS input bit for bit on every output -- integer arithmetic with a bit-exact
    specification, no tolerance -- and pass 3 differs from pass 1;
  * at level 0 once more with every intermediate as an extra output: every tensor equals the interpreter's;
  * at level 1 the plan shows exactly the rewrites the case expects (with the case's chosen extra outputs), at level 0 none;
  * where tests/golden/qu8_cases.npz holds the case, pass 1 also equals the reference's stored floats.
Reject cases run on the stub only (tests/test_qu8_lowering_cpu.py).  The module reads tests/golden only.  Launch counts and the number of codes compared on an
MI355X are in profiles/qu8_lowering_table.txt (tools/qu8_lowering_table.py writes them)."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import qu8_cases as qcs  # noqa: E402

pytestmark = pytest.mark.gpu

# Squeeze and Unsqueeze hand the codes on with scale 0 and zero point 0 (the reference's behaviour): the Sigmoid behind them sees 0 whatever was pushed
SAME_EVERY_PASS = {"move/squeeze_conv", "move/squeeze_pushed", "move/unsqueeze_conv", "move/unsqueeze_pushed"}
SAMPLE_OF_PASS = (0, 0, 1, 0)


def run(case, level, passes, extra=()):
    """a device fault ends the session: nothing more is launched on a device that has reported one"""
    from onnxstream_amd.bindings import OnnxStreamError
    try:
        return qcs.run(case, level, passes, extra)
    except OnnxStreamError as e:
        if "memory access" in str(e) or "hipError" in str(e):
            pytest.exit(f"{case.name}: the device reported a fault: {e}", returncode=3)
        raise


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def compare(case, level, what, got, want, names):
    """-> codes compared; asserts every named tensor equal to the interpreter's, dequantised with (float32)((int)q - zp) * scale on both sides"""
    n = 0
    for o in names:
        assert got[o] is not None, (level, what, o, "get_tensor returned None")
        w = qcs.deq(*want[o])
        assert got[o].shape == w.shape, (level, what, o, got[o].shape, w.shape)
        bad = int((bits(got[o]) != bits(w)).sum())
        assert not bad, (level, what, o, f"{bad} of {w.size} values differ from the interpreter's", want[o][1], want[o][2])
        n += w.size
    return n


def check_case(case, level):
    """-> (launches of a pass, codes compared): the whole protocol of one case at one level"""
    outs, what, launches = run(case, level, case.passes())
    compared = 0
    for p, k in enumerate(SAMPLE_OF_PASS):
        compared += compare(case, level, f"pass {p + 1}", outs[p], qcs.want(case, k), case.outs)
    differs = any(not np.array_equal(bits(outs[2][o]), bits(outs[0][o])) for o in case.outs)
    assert differs == (case.name not in SAME_EVERY_PASS), (level, "pass 3 against pass 1", differs)
    bad = qcs.check_plan(case, level, what)
    assert not bad, (level, case.expect, bad, what)
    if level == 0:
        names = case.intermediates()
        every, _, _ = run(case, 0, [case.sample(0)], extra=names)
        compared += compare(case, 0, "every intermediate", every[0], qcs.want(case, 0), names)
    for o in case.outs:
        gold = qcs.reference(case, o)
        assert (gold is None) == (case.name in qcs.REF_REFUSES), (case.name, o)
        if gold is not None:
            assert np.array_equal(bits(outs[0][o]), bits(gold[0])), (level, o, "differs from the reference's stored output")
    return launches, compared


@pytest.mark.parametrize("level", qcs.LEVELS)
@pytest.mark.parametrize("case", qcs.planned(), ids=lambda c: c.name)
def test_case_on_the_device(case, level):
    launches, compared = check_case(case, level)
    print(f"{case.name} level {level}: {launches} launches, {compared} codes compared")
