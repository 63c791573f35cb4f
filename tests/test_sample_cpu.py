"""Sampling in the device token loop (osg_decode_sample, model_hip_generate_sampled), CPU side.

* tests/sample_rule.py, the restatement the GPU tests hold the kernel to, is itself checked: its Philox4x32-10 against known answers, its draws against
  a float64 softmax with float64 top-k / top-p truncation (every kept token's frequency within 4 standard deviations of its binomial expectation over
  20 000 draws, nothing outside the kept set ever drawn), and the rule's edge cases on rows small enough to work out by hand.
* The host side over the no-op stand-in for libosgpu.so (tests/stub/make_stub.py: its launches compute nothing, so no token is ever taken): every
  refusal of model_hip_generate_sampled with its message, a sampled call that reports 0 tokens and leaves the Model's tensors alone, and a decode plan
  whose text is the greedy call's."""
import dataclasses
import math
import os
import sys
import tempfile

import numpy as np
import pytest

import sample_rule as S
from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))
f32 = np.float32
CFG = dataclasses.replace(llama.TINY, max_pos=256, name="llama_tiny_long")
PROMPT = [3, 17, 42, 5, 9]
NC = 2 * CFG.layers


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    ones = 0xFFFFFFFF
    assert S.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert S.philox4x32_10((ones,) * 4, (ones,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert S.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # the draw takes key = (seed low, seed high), counter = (n low, n high, 0, 0), r = word 0 | word 1 << 32
    assert S.draw_r(0, 0) == 0x6627E8D5 | (0xE169C58D << 32)
    seed, n = 0x299F31D0A4093822, 0x85A308D3243F6A88
    out = S.philox4x32_10((0x243F6A88, 0x85A308D3, 0, 0), (0xA4093822, 0x299F31D0))
    assert S.draw_r(seed, n) == out[0] | (out[1] << 32)


@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (0.8, 12, 0.9), (1.5, 5, 1.0), (0.7, 0, 0.6)])
def test_restatement_draws_the_float64_softmax(T, top_k, top_p):
    V, N = 16, 20000
    row = (np.random.default_rng(16).standard_normal(V) * 1.5).astype(f32)
    # float64: order, top-k, softmax of the kept logits at the temperature, the shortest prefix that reaches top_p
    order = np.lexsort((-np.arange(V), -row.astype(np.float64)))
    if top_k:
        order = order[:top_k]
    w = np.exp((row[order].astype(np.float64) - float(row[order[0]])) / T)
    if top_p < 1:
        share = np.cumsum(w) / w.sum()
        j = int(np.argmax(share >= top_p))
        assert abs(share[j] - top_p) > 1e-6 and (j == 0 or abs(share[j - 1] - top_p) > 1e-6)        # (the float64 cut is not a near-tie)
        order, w = order[:j + 1], w[:j + 1]
    expect = dict(zip((int(i) for i in order), w / w.sum()))
    prep = S.Prepared(row, T, top_k, top_p)
    assert not prep.stop and sorted(expect) == [int(i) for i in prep.kept]
    counts = np.zeros(V, np.int64)
    for n in range(N):
        counts[prep.draw(0x5EED, n)[0]] += 1
    for i in range(V):
        if i not in expect:
            assert counts[i] == 0, i
        else:
            p = expect[i]
            assert abs(counts[i] - N * p) <= 4 * math.sqrt(N * p * (1 - p)), (i, counts[i], N * p)


def test_restatement_edge_cases():
    # all equal: the order is index descending, top-k keeps the LARGEST indices, each kept token has q = 2^32
    p = S.Prepared(np.zeros(10, f32), 1.0, 3, 1.0)
    assert p.first == 9 and list(p.kept) == [7, 8, 9] and p.Q == 3 << 32
    # -0.0 equals +0.0
    p = S.Prepared(np.array([0.0, -0.0, -1.0], f32), 1.0, 1, 1.0)
    assert list(p.kept) == [1]
    # ties across the top-p cut: four equal tokens carry the mass, half of it needs the two largest indices
    p = S.Prepared(np.array([2.0, -40.0, 2.0, 2.0, 2.0], f32), 1.0, 0, 0.5)
    assert list(p.kept) == [3, 4] and p.widened == {2, 3, 4}
    # NaN is left out, at the maximum's place too; -inf has q = 0 and drops out
    p = S.Prepared(np.array([np.nan, 1.0, -np.inf, 1.0, np.nan], f32), 1.0, 0, 1.0)
    assert p.first == 3 and list(p.kept) == [1, 3]
    # the rows that stop the loop
    assert S.Prepared(np.full(4, np.nan, f32), 1.0).stop and S.Prepared(np.array([0.0, np.inf], f32), 1.0).stop
    assert S.Prepared(np.full(4, -np.inf, f32), 1.0).stop
    assert S.sample(np.full(4, np.nan, f32), 1.0, 0, 1.0, 0, 0)[0] is None
    # logits below -1 are sampled (the argmax's "start from -1.0f" is not part of the rule); top_k = 1 is the first token whatever the draw
    row = np.array([-5.0, -3.0, -7.0, -3.0], f32)
    for n in range(8):
        assert S.sample(row, 0.3, 1, 0.2, 77, n)[:2] == (3, math.inf)
    # a tiny top_p still keeps one token; one dominant logit leaves the others at q = 0
    assert list(S.Prepared(row, 1.0, 0, 1e-30).kept) == [3]
    p = S.Prepared(np.array([0.0, 30.0, 1.0], f32), 1.0)
    assert list(p.kept) == [1] and p.Q == 1 << 32
    # the threshold is floor(p * Qtot) with the fp32 p taken exactly: fp32(2/3) = 11184811 / 2^24 lies ABOVE 2/3, so two of three equal tokens fall
    # short of it by 256 (the double 2/3 would have kept two)
    p = S.Prepared(np.zeros(3, f32), 1.0, 0, 2.0 / 3.0)
    thr = (3 << 32) * 11184811 // 2 ** 24
    assert thr == (2 << 32) + 256 and list(p.kept) == [0, 1, 2] and p.topp_margin == 256 / (3 << 32)


def test_draws_of_one_row_depend_on_seed_and_index_only():
    row = (np.random.default_rng(3).standard_normal(200) * 2).astype(f32)
    p = S.Prepared(row, 0.9, 50, 0.95)
    a = [p.draw(11, n)[0] for n in range(32)]
    assert a == [p.draw(11, n)[0] for n in range(32)]
    assert a != [p.draw(12, n)[0] for n in range(32)]
    assert a[5:] == [p.draw(11, 5 + n)[0] for n in range(27)]          # draw_base = 5 at n_tokens = n is draw index 5 + n


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host side through the stub
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    with tempfile.TemporaryDirectory() as d:
        so = make_stub.build(d)
        old = os.environ.get("OSGPU_LIB")
        os.environ["OSGPU_LIB"] = so
        try:
            yield so
        finally:
            if old is None:
                os.environ.pop("OSGPU_LIB", None)
            else:
                os.environ["OSGPU_LIB"] = old


@pytest.fixture(scope="module")
def model_dir():
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        llama.build_llama(DirSink(d), CFG)
        yield d


def _model(model_dir):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    m.add_outputs_convert("logits")
    llama.configure(m, CFG, model_dir, sdpa=True, upcast=True)
    llama.forward_resident(m, CFG, PROMPT, True, 0, keep_logits=True)
    return m


def test_sampled_refusals(stub_backend, model_dir):
    from onnxstream_amd.bindings import OnnxStreamError
    m = _model(model_dir)
    m.set_use_fp16_arithmetic(True)
    built = m.hip_plans_built()
    for kw, msg in (({"temperature": -0.5}, "temperature must be finite and >= 0"),
                    ({"temperature": float("nan")}, "temperature must be finite and >= 0"),
                    ({"temperature": float("inf")}, "temperature must be finite and >= 0"),
                    ({"temperature": float("-inf")}, "temperature must be finite and >= 0"),
                    ({"temperature": 1e-42}, "temperature is too small"),
                    ({"temperature": 0.8, "top_k": -1}, "top_k must be >= 0"),
                    ({"temperature": 0.8, "top_p": float("nan")}, r"top_p must be in \(0, 1\]"),
                    ({"temperature": 0.8, "top_p": 0.0}, r"top_p must be in \(0, 1\]"),
                    ({"temperature": 0.8, "top_p": -0.1}, r"top_p must be in \(0, 1\]"),
                    ({"temperature": 0.8, "top_p": 1.0000001}, r"top_p must be in \(0, 1\]")):
        with pytest.raises(OnnxStreamError, match="^Model::hip_generate: " + msg):
            m.generate(4, NC, **kw)
    # the refusals of the greedy call hold for the sampled one, under the same prefix
    with pytest.raises(OnnxStreamError, match="^Model::hip_generate: max_new must be >= 0"):
        m.generate(-1, NC, temperature=0.8)
    with pytest.raises(OnnxStreamError, match="^Model::hip_generate: tensor not found: nologits"):
        m.generate(4, NC, logits="nologits", temperature=0.8)
    assert m.hip_plans_built() == built          # nothing was built on the way to a refusal
    m.close()


def test_sampled_call_through_the_stub(stub_backend, model_dir):
    m = _model(model_dir)
    P = len(PROMPT)
    names = sorted(m.get_all_tensor_names())
    logits = m.get_tensor("logits")[0].copy()
    cache = m.get_tensor_f16("opkv0").copy()
    built = m.hip_plans_built()
    toks, stop, trace, ms = llama.generate(m, CFG, 4, trace=True, temperature=0.8, top_k=40, top_p=0.9, seed=2 ** 64 - 1, draw_base=2 ** 63)
    assert list(toks) == [] and stop == 0 and trace.shape == (0, CFG.vocab)         # (the stub takes no token)
    assert m.hip_plans_built() == built + 1
    sampled_info = m.hip_decode_plan_info()
    # the Model's tensors are as they were
    assert sorted(m.get_all_tensor_names()) == names
    assert m.get_tensor("logits")[0].shape == (1, P, CFG.vocab) and m.get_tensor("logits")[0].tobytes() == logits.tobytes()
    assert m.get_tensor_f16("opkv0").tobytes() == cache.tobytes()
    # a greedy call shares the plan the sampled call built, and so does the next sampled one
    llama.generate(m, CFG, 4)
    llama.generate(m, CFG, 4, temperature=1.0)
    assert m.hip_plans_built() == built + 1 and m.hip_decode_plan_info() == sampled_info
    m.close()
    # a Model that only ever decodes greedily builds the same plan, to the letter
    m = _model(model_dir)
    llama.generate(m, CFG, 4)
    assert m.hip_decode_plan_info() == sampled_info
    m.close()
