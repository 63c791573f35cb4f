"""CPU: every graph rewrite on its forms and near misses (the table of tests/fusion_cases.py) through the stub backend (tests/stub/make_stub.py: plan structure
only, arithmetic launches compute nothing).  Checked here, without a GPU:
  * every case plans at fusion levels 0, 1 and 2 under the options it names, and every output -- the extra outputs asked for through add_extra_output
    included -- comes back at every level with the restatement's shape: a rewrite never leaves a requested tensor unwritten;
  * the level 2 plan's arithmetic step kinds equal the case's `plan`: a "fires" case shows the rewrite, a "left" case names the surviving ops;
  * a near miss built on an operator form the lowering itself does not take is refused with that message at every level (the pass did not swallow it);
  * the value the forbidden rewrite would compute is more than 50 tolerances from the restatement on at least half of the elements, so that the device run
    of the same table (tests/test_fusion_cases_gpu.py) cannot pass over the defect -- or the case says why no value can show it;
  * tests/golden/fusion_cases.npz (the reference's fp16 / fp32 outputs, tools/make_golden_fusion.py) covers the table, is what oracle/_ref computes where it is
    built, and the restatement agrees with it under the single-pattern rule of tests/test_golden.py;
  * every fp16 pass of lowering_graph.inc has at least one "fires" case and two that are not: a pass added later without cases fails here."""
import os
import re
import sys
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "stub"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import fusion_cases as fc  # noqa: E402
import op_cases as oc  # noqa: E402

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(REPO, "tests", "golden", "fusion_cases.npz")


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


def want(case):
    """the restatement of sample 0 (fusion_cases computes it once per case and leaves it unchanged)"""
    return {o: v for o, v in fc.want(case).items() if "@" not in o}


def test_table_is_well_formed():
    names = [c.name for c in fc.CASES]
    assert len(set(names)) == len(names)
    for c in fc.CASES:
        w = want(c)
        assert set(w) == set(c.outs), (c.name, sorted(w), c.outs)
        assert all(v.dtype == f64 and np.isfinite(v).all() for v in w.values()), c.name
        assert c.pass_ in fc.PASSES, c.name
        assert c.refuse or c.plan, c.name
        if c.expect in ("left", "partial"):
            assert c.wrong is not None or c.why or c.refuse, c.name
    assert set(fc.REF_REFUSES) <= set(names)
    assert sum(c.pass_ == "fuse_tblock_tail" for c in fc.CASES) == 5        # (the only cases at the 320-wide sizes)


def test_every_pass_has_cases():
    src = open(os.path.join(REPO, "onnxstream_amd", "csrc", "host", "lowering_graph.inc")).read()
    passes = {m for m in re.findall(r"void ((?:fuse_|cse_)\w+)\(", src) if not m.startswith("fuse_u8_")}     # (the uint8 passes need range data: tests/qu8_cases.py)
    assert passes, "no pass found in lowering_graph.inc"
    assert passes <= set(fc.PASSES), sorted(passes - set(fc.PASSES))
    for p in sorted(passes | {"plan_linear_groups", "ln_fold"}):
        mine = [c for c in fc.CASES if c.pass_ == p]
        assert sum(c.expect == "fires" for c in mine) >= 1, p
        assert sum(c.expect != "fires" for c in mine) >= 2, p


@pytest.mark.parametrize("case", fc.planned(), ids=lambda c: c.name)
def test_plans_at_every_level_and_returns_every_output(stub_backend, case):
    w = want(case)
    for level in fc.LEVELS:
        got, kinds, what = fc.run(case, level)
        for o in case.outs:
            assert len(got[o]) == 1, (level, o, "get_tensor returned None")
            assert got[o][0].shape == w[o].shape, (level, o, got[o][0].shape, w[o].shape)
        exp = fc.expected_plan(case, level)
        if exp is not None:
            assert kinds == exp, (level, kinds, exp)
        if level == 2:
            text = "\n".join(what)
            for s in case.present:
                assert s in text, (case.expect, "not in the plan:", s, what)
            for s in case.absent:
                assert s not in text, (case.expect, "in the plan:", s, what)
        elif level == 0:
            assert not any(k.startswith("osg.") for k in kinds) or case.opts, (level, kinds)


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.expect == "fires" and not c.refuse], ids=lambda c: c.name)
def test_fires_cases_take_three_samples(stub_backend, case):
    got, kinds, _ = fc.run(case, 2, pushes=3)
    assert kinds == case.plan
    for o in case.outs:
        assert len(got[o]) == 3 and all(g.shape == want(case)[o].shape for g in got[o]), o


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.refuse], ids=lambda c: c.name)
def test_unsupported_operator_forms_are_refused_at_every_level(stub_backend, case):
    from onnxstream_amd.bindings import OnnxStreamError
    for level in fc.LEVELS:
        with pytest.raises(OnnxStreamError) as e:
            fc.run(case, level)
        assert case.refuse in str(e.value), (level, str(e.value))


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.wrong is not None], ids=lambda c: c.name)
def test_the_forbidden_rewrite_would_show(case):
    """|ref - wrong| > 50 tolerances on at least half of the elements of the outputs the rewrite would change (tolerance: 1e-3 max|ref|, the single-pattern rule)"""
    w, wv = want(case), case.wrong_values(0)
    assert wv, case.name
    for o, v in wv.items():
        assert v.shape == w[o].shape, (o, v.shape, w[o].shape)
        tol = 1e-3 * float(np.abs(w[o]).max())
        frac = float((np.abs(w[o] - v) > 50 * tol).mean())
        assert frac >= 0.5, (o, frac)


# ---- the reference's outputs --------------------------------------------------------------------------------------------------------------------------
def golden_cases():
    return [c for c in fc.planned() if c.name not in fc.REF_REFUSES]


def test_golden_file_covers_the_table():
    have = set(fc.load_golden(GOLDEN))
    want_keys = {f"{c.name}|{o}" for c in golden_cases() for o in c.outs}
    assert have == want_keys, (sorted(want_keys - have), sorted(have - want_keys))
    assert os.path.getsize(GOLDEN) < 400 * 1024
    assert set(k.split("|")[0] for k in fc.REF_NOISE) <= {c.name for c in fc.CASES} and all(k[0].split("|")[0] in {c.name for c in fc.CASES} for k in fc.EXCEPTIONS)


def test_reference_reproduces_the_golden_file():
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref not built")
    import make_golden_fusion as mg
    for c in fc.planned():
        try:
            o16, o32 = mg.run_reference(c, True), mg.run_reference(c, False)
        except Exception as e:
            assert c.name in fc.REF_REFUSES and fc.REF_REFUSES[c.name] in str(e), (c.name, str(e))
            continue
        assert c.name not in fc.REF_REFUSES, c.name
        for o in c.outs:
            ref16, m32, shape = fc.golden(c, o)
            assert o16[o].shape == shape, (c.name, o)
            assert np.array_equal(oc.bits(o16[o].reshape(-1)[::fc.golden_stride(o16[o].size)]), oc.bits(ref16)), (c.name, o)
            assert f32(np.abs(o32[o]).max()) == f32(m32), (c.name, o)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c.name)
def test_restatement_agrees_with_the_reference(case):
    """pins the float64 restatement to the reference's semantics: shapes, and values on sample 0 under the single-pattern rule"""
    w = want(case)
    for o in case.outs:
        gold = fc.golden(case, o)
        assert gold[2] == w[o].shape, (o, gold[2], w[o].shape)
        got = w[o].astype(np.float16).astype(f32)
        e = fc.err16(got, gold)
        assert e <= fc.bound16(case, o), (o, e)
