"""CPU: the uint8-arithmetic lowering per operator form and both uint8 passes on their forms and near misses (the table of tests/qu8_cases.py) through the stub
backend (tests/stub/make_stub.py: plan structure only, arithmetic launches compute nothing).  Checked here, without a GPU:
  * every planned case plans at fusion levels 0 and 1 (the uint8 passes run from level 1) and every named output comes back with the interpreter's shape; the
    level 1 plan shows exactly the rewrites the case's `expect` states, the level 0 plan none;
  * every reject case is refused with its message at both levels;
  * the interpreter (qu8_cases.interpret over oracle/np_qu8.py) reproduces tests/golden/qu8_cases.npz -- the reference's dequantised tensors, scale and zero point
    of every named tensor -- bit for bit; where oracle/_ref is built, a fresh reference run equals the stored one;
  * for every "left" / "partial" case the forbidden rewrite, computed as if it had fired, differs from the graph as written in at least one code of every
    sample (the share is printed), or the hand-written fused op is refused by its lowering -- or the case says why no code can show it;
  * coverage: every operator type lower_u8 dispatches on, every need( / throw message of lowering_u8.inc up to the end of lower_softmax_u8, and both passes
    (one firing case and two that do not fire, at least) are reached by a case.  The messages are read from the source text."""
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
import qu8_cases as qcs  # noqa: E402

SRC = os.path.join(REPO, "onnxstream_amd", "csrc", "host")


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
    names = [c.name for c in qcs.CASES]
    assert len(set(names)) == len(names)
    ranges, ref = qcs.golden()
    assert set(ranges) == set(names), (sorted(set(names) - set(ranges)), sorted(set(ranges) - set(names)))
    for c in qcs.planned():
        acts = c.intermediates()
        assert set(c.outs) <= set(acts), (c.name, c.outs, acts)
        assert set(c.extra) <= set(c.outs), c.name
        text = qcs.parse_ranges(qcs.range_text(c))
        assert all(np.isfinite(v).all() and v[0] < v[1] for v in text.values()), c.name
        if c.kind == "fusion":
            assert c.pass_ in qcs.PASSES and (c.present or c.absent), c.name
    assert set(qcs.REF_REFUSES) <= {c.name for c in qcs.planned()}
    assert not qcs.REF_DIFFERS, "where the reference and the interpreter disagree the reference is right: correct oracle/np_qu8.py or the interpreter"
    assert os.path.getsize(qcs.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("case", qcs.planned(), ids=lambda c: c.name)
def test_plans_at_both_levels(stub_backend, case):
    want = qcs.want(case, 0)
    for level in qcs.LEVELS:
        outs, what, _ = qcs.run(case, level)
        for o in case.outs:
            assert outs[0][o] is not None, (level, o, "get_tensor returned None")
            assert outs[0][o].shape == want[o][0].shape, (level, o, outs[0][o].shape, want[o][0].shape)
        bad = qcs.check_plan(case, level, what)
        assert not bad, (level, case.expect, bad, what)


def test_matmul_step_reads_the_operand_whose_parameters_it_takes(stub_backend):
    """activation x activation: the launch takes its [N,K] codes from the transposed copy and the PARAMETERS from the operand itself.  Plan::dyn_end goes by a step's
    reads, so the operand must be among them: with a pushed second operand behind a first one with parameters from range data, the launch otherwise lands in the
    captured part of the pass and replays the first pass's scale and zero point (found on the device by matmul/aa_static_a_pushed_b: 69 of 70 codes of pass 3)"""
    import re
    _, lines, _ = qcs.run(qcs.by_name("matmul/aa_static_a_pushed_b"), 0, step_lines=True)
    t_reads = next(set(re.search(r"reads=([\d,]*)", ln).group(1).split(",")) for ln in lines if "MatMul qu8/T" in ln)
    mm_reads = next(set(re.search(r"reads=([\d,]*)", ln).group(1).split(",")) for ln in lines if "MatMul qu8 mm" in ln)
    assert t_reads <= mm_reads and len(mm_reads) == 3, lines


_REFUSALS = {}


def refusal(case, level, body=None):
    """the message with which the lowering refuses the case (or the hand-written form `body`), None where it plans"""
    from onnxstream_amd.bindings import OnnxStreamError
    key = (case.name, level, body is not None)
    if key not in _REFUSALS:
        try:
            qcs.run(case, level, body=body, ranges=None if body is None else _hand_ranges(case, body))
            _REFUSALS[key] = None
        except OnnxStreamError as e:
            _REFUSALS[key] = str(e)
    return _REFUSALS[key]


def _hand_ranges(case, body):
    """range data of a hand-written form: the case's own, plus what the body states for its fused op"""
    from onnxstream_amd.synth import graph as sg
    have = qcs.parse_ranges(qcs.range_text(case))
    have.update(case.write(sg.MemSink(), body).ranges)
    return "".join(f"{n},{lo:.6f},{hi:.6f}\r\n" for n, (lo, hi) in have.items())


@pytest.mark.parametrize("case", qcs.rejects(), ids=lambda c: c.name)
def test_refused_with_its_message_at_both_levels(stub_backend, case):
    for level in qcs.LEVELS:
        msg = refusal(case, level)
        assert msg is not None and case.reject in msg, (level, msg)


# ---- the interpreter against the reference ------------------------------------------------------------------------------------------------------------------
def golden_cases():
    return [c for c in qcs.planned() if c.name not in qcs.REF_REFUSES]


def test_golden_file_covers_the_table():
    have = set(qcs.golden()[1])
    want_keys = {f"{c.name}|{n}" for c in golden_cases() for n in c.intermediates()}
    assert have == want_keys, (sorted(want_keys - have), sorted(have - want_keys))


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c.name)
def test_interpreter_reproduces_the_reference(case):
    want = qcs.want(case, 0)
    for n in case.intermediates():
        ref, scale, zp = qcs.reference(case, n)
        codes, s, z = want[n]
        assert codes.shape == ref.shape, (n, codes.shape, ref.shape)
        assert (np.float32(s), int(z)) == (scale, zp), (n, s, z, scale, zp)
        got = qcs.deq(codes, s, z)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (n, int((got != ref).sum()), got.size)


def test_reference_reproduces_the_golden_file():
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref not built")
    import make_golden_qu8_cases as mg
    from onnxstream_amd.bindings import OnnxStreamError
    for c in qcs.planned():
        try:
            ref = mg.run_reference(c, qcs.range_text(c))
        except (OnnxStreamError, RuntimeError) as e:
            assert c.name in qcs.REF_REFUSES and qcs.REF_REFUSES[c.name] in str(e), (c.name, str(e))
            continue
        assert c.name not in qcs.REF_REFUSES, c.name
        for n in c.intermediates():
            stored = qcs.reference(c, n)
            assert n in ref and ref[n][0].shape == stored[0].shape, (c.name, n)
            assert np.array_equal(ref[n][0], stored[0]) and (ref[n][1], ref[n][2]) == (stored[1], stored[2]), (c.name, n)


# ---- near misses: the forbidden rewrite would show ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in qcs.planned() if c.expect in ("left", "partial")], ids=lambda c: c.name)
def test_the_forbidden_rewrite_would_show(stub_backend, case):
    if case.wrong is None:
        assert case.why, case.name
        print(f"{case.name}: held on plan structure -- {case.why}")
        return
    if isinstance(case.wrong, tuple):
        kind, body, msg = case.wrong
        assert kind == "refused"
        for level in qcs.LEVELS:
            got = refusal(case, level, body)
            assert got is not None and msg in got, (level, got)
        print(f"{case.name}: the fused op written by hand is refused: {refusal(case, 0, body)}")
        return
    for k in (0, 1):
        want = qcs.want(case, k)
        if isinstance(case.wrong, dict):
            for o, v in case.wrong.items():
                assert v == "unwritten" and o in case.outs, (case.name, o)
                w = qcs.deq(*want[o])
                share = float((w != 0).mean())
                print(f"{case.name} sample {k} {o}: {share:.3f} of the values differ from an unwritten tensor's")
                assert share > 0, (o, k)
        else:
            wrong = qcs.want(case, k, body=case.wrong)
            differs = 0
            for o in case.outs:
                assert wrong[o][0].shape == want[o][0].shape, (o, wrong[o][0].shape, want[o][0].shape)
                share = float((qcs.deq(*wrong[o]) != qcs.deq(*want[o])).mean())
                print(f"{case.name} sample {k} {o}: {share:.3f} of the codes differ under the forbidden rewrite")
                differs += share > 0
            assert differs, k


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------------------
def _lowering_text():
    text = open(os.path.join(SRC, "lowering_u8.inc")).read()
    end = text.index("void lower_softmax_u8")
    return text[:text.index("\n    }\n", end) + 7]


def _functions(text):
    """[(function name, body text)] of the member functions, in order"""
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"^    [\w:<>\*& ]+? (\w+)\([^;{]*\) \{$", text, flags=re.M)]
    return [(name, text[at:(heads[i + 1][0] if i + 1 < len(heads) else len(text))]) for i, (at, name) in enumerate(heads)]


# the operator types a function of lowering_u8.inc serves (None: any -- the helpers)
SERVES = {"lower_conv_u8": ("Conv",), "lower_matmul_u8": ("MatMul",), "lower_binary_u8": ("Add", "Mul"), "lower_sigmoid_u8": ("Sigmoid",),
          "lower_instance_norm_u8": ("InstanceNormalization",), "lower_instance_norm_u8_nhwc": ("osg.qu8.InstanceNormNHWC", "InstanceNormalization"),
          "lower_affine_act_u8": ("osg.qu8.AffineAct", "osg.qu8.NormAffineAct"), "lower_softmax_u8": ("Softmax",), "out_q": None, "range_q": None, "need_u8": None,
          "lower_u8": None, "out_val_u8": None, "lut_alloc": None}
# (function, message) that no graph can reach, with the reason
UNREACHABLE = {
    ("lower_matmul_u8", "uint8 arithmetic runs one sample per pass (every pushed sample has its own scale)."):
        "the plan refuses more than one pushed sample under uint8 arithmetic before any op is lowered (reject/three_pushed_samples), and a MatMul has no image count of its own",
}


def source_messages():
    """(function, the longest string literal of the message) for every need( and throw of lowering_u8.inc from line 1 to the end of lower_softmax_u8"""
    out = []
    for name, body in _functions(_lowering_text()):
        for m in re.finditer(r"(?:\bneed\(|throw std::invalid_argument\()(.*?)\);", body, flags=re.S):
            lits = re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))
            assert lits, (name, m.group(0))
            out.append((name, max(lits, key=len)))
    return out


def test_coverage_of_the_uint8_lowering(stub_backend):
    text = _lowering_text()
    missing = []
    # operator types
    body = dict(_functions(text))["lower_u8"]
    types = set(re.findall(r't == "([\w\.]+)"', body))
    assert {"Conv", "MatMul", "Softmax", "osg.qu8.NormAffineAct", "Resize"} <= types, types
    reached = set()
    for c in qcs.planned():
        for level in qcs.LEVELS:
            _, what, _ = qcs.run(c, level)
            for w in what:
                k = w.split(" ", 1)[0]
                reached.add({"InstanceNorm": "InstanceNormalization" if "nhwc" not in w else "osg.qu8.InstanceNormNHWC", "AffineAct": "osg.qu8.AffineAct",
                             "NormAffineAct": "osg.qu8.NormAffineAct"}.get(k, k.split("/")[0]))
        with tempfile.TemporaryDirectory() as d:
            c.emit(d + "/")
            from oracle import qu8_check as qc
            reached |= {op["type"] for op in qc.parse_model(d + "/model.txt")}            # (Reshape, Flatten, Squeeze, Unsqueeze leave no step: they are aliases)
    missing += [f"operator type {t}" for t in sorted(types - reached)]
    # messages
    msgs = source_messages()
    assert len(msgs) > 40 and all(fn in SERVES for fn, _ in msgs), sorted({fn for fn, _ in msgs} - set(SERVES))
    refusals = []
    for c in qcs.rejects():
        refusals += [refusal(c, lv) for lv in qcs.LEVELS]
    for c in qcs.planned():
        if isinstance(c.wrong, tuple):
            refusals += [refusal(c, lv, c.wrong[1]) for lv in qcs.LEVELS]
    refusals = [r for r in refusals if r]
    for fn, lit in msgs:
        if (fn, lit) in UNREACHABLE:
            continue
        serves = SERVES[fn]
        if not any(lit in r and (serves is None or r.startswith(tuple(t + ":" for t in serves))) for r in refusals):
            missing.append(f"message of {fn}: {lit!r}")
    # passes
    src = open(os.path.join(SRC, "lowering_graph.inc")).read()
    passes = set(re.findall(r"void (fuse_u8_\w+)\(", src))
    assert passes == set(qcs.PASSES), (passes, qcs.PASSES)
    for p in sorted(passes):
        mine = [c for c in qcs.CASES if c.pass_ == p]
        if sum(c.expect == "fires" for c in mine) < 1 or sum(c.expect != "fires" for c in mine) < 2:
            missing.append(f"pass {p}: one firing case and two that do not fire")
    assert not missing, missing
