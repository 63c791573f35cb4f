"""CPU: every operator's lowering per attribute form, layout and batch (the table of tests/op_cases.py) through the stub backend (tests/stub/make_stub.py:
data movement is real, arithmetic launches compute nothing).  Checked here, without a GPU:
  * every case that is not a refusal plans at fusion 0 and 2 with 1 and 3 pushed samples, and get_tensor returns the restatement's shape for every sample;
  * every case whose launches are all data movement carries real values: they equal the float64 restatement bit for bit, the sign of zero included;
  * every refusal raises its message at plan time;
  * tests/golden/op_cases.npz (the reference's fp16 / fp32 outputs, tools/make_golden_ops.py) is what oracle/_ref computes, where it is built, and the
    restatement agrees with it: bit for bit for the movement cases, err16 <= 1e-3 (the single-pattern rule of tests/test_golden.py) for the others.
The same table runs on the device in tests/test_op_lowering_gpu.py."""
import os
import sys
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "stub"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import op_cases as oc  # noqa: E402

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(REPO, "tests", "golden", "op_cases.npz")


@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    with tempfile.TemporaryDirectory() as d:
        old = os.environ.get("OSGPU_LIB")
        os.environ["OSGPU_LIB"] = make_stub.build(d)
        try:
            yield
        finally:
            if old is None:
                os.environ.pop("OSGPU_LIB", None)
            else:
                os.environ["OSGPU_LIB"] = old


def test_table_is_well_formed():
    names = [c.name for c in oc.CASES]
    assert len(set(names)) == len(names)
    for c in oc.runnable():
        for k in range(3):
            w = c.want(k)
            assert {o for o in w if "@" not in o} == set(c.outs), c.name
            assert all(np.asarray(v).dtype == f64 for o, v in w.items() if "@" not in o), c.name
    assert set(oc.REF_REFUSES) <= set(names) and set(oc.REF_DIFFERS) <= set(names)


@pytest.mark.parametrize("pushes", [1, 3])
@pytest.mark.parametrize("fusion", [0, 2])
@pytest.mark.parametrize("case", oc.runnable(), ids=lambda c: c.name)
def test_plans_with_the_restated_shapes_and_moves_real_values(stub_backend, case, fusion, pushes):
    got = oc.run_case(case, pushes, fusion)
    for o in case.outs:
        n = 1 if o in case.const_out else pushes
        assert len(got[o]) == n, (o, len(got[o]))
        for k in range(n):
            want = case.want(k)[o]
            assert got[o][k].shape == want.shape, (o, k, got[o][k].shape, want.shape)
            if case.stub_values:
                assert np.array_equal(oc.bits(got[o][k]), oc.bits(want)), (o, k)


@pytest.mark.parametrize("case", [c for c in oc.CASES if c.cls == "reject"], ids=lambda c: c.name)
def test_refusals_are_raised_at_plan_time(stub_backend, case):
    from onnxstream_amd.bindings import OnnxStreamError
    for fusion in (0, 2):
        with pytest.raises(OnnxStreamError) as e:
            oc.run_case(case, 1, fusion)
        assert case.reject in str(e.value), str(e.value)


# ---- the reference's outputs --------------------------------------------------------------------------------------------------------------------------
def test_golden_file_covers_the_table():
    z = np.load(GOLDEN)
    have = {k.split("|")[0] for k in z.files}
    want = {c.name for c in oc.device_cases()} - set(oc.REF_REFUSES)
    assert have == want, (sorted(want - have), sorted(have - want))
    for c in oc.device_cases():
        if c.name not in oc.REF_REFUSES:
            assert all(f"{c.name}|{o}|{r}" in z.files for o in c.outs for r in ("ref16", "ref32")), c.name
    assert os.path.getsize(GOLDEN) < 400 * 1024          # (the single-pattern fixtures of tests/golden add up to more than 3 MiB)


def test_reference_reproduces_the_golden_file():
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref not built")
    import make_golden_ops as mg
    z = np.load(GOLDEN)
    for c in oc.device_cases():
        try:
            o16, o32 = mg.run_reference(c, True), mg.run_reference(c, False)
        except Exception as e:
            assert c.name in oc.REF_REFUSES and oc.REF_REFUSES[c.name] in str(e), (c.name, str(e))
            continue
        assert c.name not in oc.REF_REFUSES, c.name
        for o in c.outs:
            assert np.array_equal(oc.bits(o16[o]), oc.bits(z[f"{c.name}|{o}|ref16"].astype(f32))), (c.name, o)
            assert np.array_equal(oc.bits(o32[o]), oc.bits(z[f"{c.name}|{o}|ref32"])), (c.name, o)


@pytest.mark.parametrize("case", [c for c in oc.device_cases() if c.name not in oc.REF_REFUSES], ids=lambda c: c.name)
def test_restatement_agrees_with_the_reference(case):
    """pins the float64 restatement to the reference's semantics: shapes, and values on sample 0"""
    z = np.load(GOLDEN)
    want = case.want(0)
    for o in case.outs:
        r16, r32 = z[f"{case.name}|{o}|ref16"].astype(f32), z[f"{case.name}|{o}|ref32"]
        assert r16.shape == want[o].shape, (o, r16.shape, want[o].shape)
        w = want[o].astype(np.float16).astype(f32)
        if case.cls == "move":
            assert np.array_equal(oc.bits(w), oc.bits(r16)), o
        else:
            err16 = float(np.abs(w.astype(f64) - r16).max()) / float(np.abs(r32).max())
            assert err16 <= 1e-3, (o, err16)
