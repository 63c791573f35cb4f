"""One chat turn on the device (model_hip_turn), CPU side: the host logic over the no-op stand-in for libosgpu.so (tests/stub/make_stub.py -- its
launches compute nothing, so no token is ever picked: a turn reports 0 tokens and leaves the prefill's caches of P + n rows).

* every refusal, with its message;
* the chunk plan: one row-append per cache, one chunk-form attention per layer, no mask, no cache copy -- and everything else the launches of an ordinary
  T = chunk run();
* a mask that is not exactly the causal one (a padding term that is not all zeros; no key barred) is refused by name;
* the shapes a turn leaves in m_data, the capacity rule (as given and as derived), and the decode plan being the one `generate` alone builds."""
import dataclasses
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))
CFG = dataclasses.replace(llama.TINY, max_pos=256, name="llama_tiny_long")
PROMPT = [3, 17, 42, 5, 9]
NC = 2 * CFG.layers


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


def _model(model_dir, sdpa=True, upcast=True, options=(), prefill=True):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    for k, v in options:
        m._set_option(k, v)
    m.add_outputs_convert("logits")
    llama.configure(m, CFG, model_dir, sdpa=sdpa, upcast=upcast)
    if prefill:
        llama.forward_resident(m, CFG, PROMPT, True, 0, keep_logits=True)
    return m


def _steps(info):
    return [ln.split(" | ", 1)[1] for ln in info.splitlines() if ln.startswith("step ")]


def test_refusals(stub_backend, model_dir):
    from onnxstream_amd.bindings import OnnxStreamError
    m = _model(model_dir, prefill=False)
    m.set_use_fp16_arithmetic(True)
    with pytest.raises(OnnxStreamError, match=r"Model::hip_turn: run\(\) once first"):
        m.turn([1, 2], 4, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_prefill_plan_info: no chunk plan"):
        m.hip_prefill_plan_info()
    m.close()

    m = _model(model_dir)
    for bad in ([], ):
        with pytest.raises(OnnxStreamError, match="Model::hip_turn: n_prompt must be >= 1"):
            m.turn(bad, 4, NC)
    for chunk in (0, -1, 513):
        with pytest.raises(OnnxStreamError, match=r"Model::hip_turn: chunk must be in \[1, 512\]"):
            m.turn([1, 2], 4, NC, chunk=chunk)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: capacity must be >= 0"):
        m.turn([1, 2], 4, NC, capacity=-1)
    # what generate refuses
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: max_new must be >= 0"):
        m.turn([1, 2], -1, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: temperature must be finite and >= 0"):
        m.turn([1, 2], 4, NC, temperature=-1.0)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: temperature must be finite and >= 0"):
        m.turn([1, 2], 4, NC, temperature=float("nan"))
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: temperature is too small"):
        m.turn([1, 2], 4, NC, temperature=1e-45)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: top_k must be >= 0"):
        m.turn([1, 2], 4, NC, temperature=1.0, top_k=-1)
    for top_p in (0.0, 1.5, float("nan")):
        with pytest.raises(OnnxStreamError, match=r"Model::hip_turn: top_p must be in \(0, 1\]"):
            m.turn([1, 2], 4, NC, temperature=1.0, top_p=top_p)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: needs at least one key/value cache"):
        m.turn([1, 2], 4, 0)
    # neither the caches a run() left nor pushed ones
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: tensor not found: nopkv0"):
        m.turn([1, 2], 4, NC, cache_in="nopkv", cache_out="nokv")
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: tensor not found: opkv4"):
        m.turn([1, 2], 4, NC + 1)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: cache 'logits0' must be float16"):
        m.set_use_fp16_arithmetic(False)
        m.add_tensor("logits0", np.zeros((1, 2, 5, 16), np.float32))
        m.set_use_fp16_arithmetic(True)
        m.turn([1, 2], 4, 1, cache_out="logits")
    for opt, msg in (("use_uint8_arithmetic", "not available with uint8 arithmetic"), ("hip_stream_weights", "not available in streamed-weights mode"),
                     ("use_fp16_arithmetic", "needs fp16 arithmetic")):
        m._set_option(opt, opt != "use_fp16_arithmetic")
        with pytest.raises(OnnxStreamError, match="Model::hip_turn: " + msg):
            m.turn([1, 2], 4, NC)
        m._set_option(opt, opt == "use_fp16_arithmetic")
    m.set_use_scaled_dp_attn_op(False)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: needs m_use_scaled_dp_attn_op"):
        m.turn([1, 2], 4, NC)
    m.set_use_scaled_dp_attn_op(True)
    # names the graph does not know: the chunk plan cannot be built, and none is kept
    with pytest.raises(OnnxStreamError, match="input tensor not found: input.*ids"):
        m.turn([1, 2], 4, NC, ids="noids")
    with pytest.raises(OnnxStreamError, match="no chunk plan"):
        m.hip_prefill_plan_info()
    # the logits output must be an fp32 output of the graph
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: the graph has no fp32 output 'nologits'"):
        m.turn([1, 2], 4, NC, logits="nologits")
    # positions and token ids beyond the tables they index
    P = len(PROMPT)
    with pytest.raises(OnnxStreamError, match=f"Model::hip_turn: positions up to {P + 2 + 256 - 1} are needed, the smallest table indexed by 'position.*ids' has 256 rows"):
        m.turn([1, 2], 256, NC)
    with pytest.raises(OnnxStreamError, match=f"Model::hip_turn: positions up to 256 are needed"):
        m.turn(list(range(1, 253)), 0, NC, chunk=64)          # 5 + 252 rows: the last position is 256
    with pytest.raises(OnnxStreamError, match=f"Model::hip_turn: prompt token {CFG.vocab} at 1 is outside the smallest table indexed by 'input.*ids' \\({CFG.vocab} rows\\)"):
        m.turn([1, CFG.vocab], 4, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_turn: prompt token -1 at 0 is outside"):
        m.turn([-1, 2], 4, NC)
    # nothing of the above touched the conversation
    assert m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, P, CFG.head_dim)
    m.close()


def test_a_host_evaluation_of_the_tokens_or_positions_is_refused(stub_backend, model_dir):
    from onnxstream_amd.bindings import OnnxStreamError
    m = _model(model_dir)
    with pytest.raises(OnnxStreamError, match=r"Model::hip_turn: Cast \(.*\) needs the value of 'attention.*mask' while the plan is built"):
        m.turn([1, 2], 4, NC, pos="attention_mask", mask="position_ids")
    m.close()


@pytest.mark.parametrize("upcast,fusion", [(False, 2), (True, 2), (True, 0)])
def test_chunk_plan_shape(stub_backend, model_dir, upcast, fusion):
    C = 8
    m = _model(model_dir, upcast=upcast, options=(("hip_fusion_level", fusion),))
    toks, stop, trace, ms = llama.turn(m, CFG, [7, 8, 9], 4, chunk=C, trace=True)
    assert list(toks) == [] and stop == 0 and trace.shape == (0, CFG.vocab)         # (the stub picks nothing)
    info = m.hip_prefill_plan_info()
    assert info.splitlines()[0] == f"prefill chunk {C} capacity 64"
    whats = _steps(info)
    appends = [w for w in whats if w.startswith("KVAppend(rows) ")]
    assert sorted(appends) == sorted(f"KVAppend(rows) /model/layers.{l}/self_attn/Concat{s}" for l in range(CFG.layers) for s in ("", "_1"))
    assert sum(w.startswith("ScaledDotProductAttention(chunk) ") for w in whats) == CFG.layers
    assert not any(w.startswith("ScaledDotProductAttention ") for w in whats)
    cache_concat = re.compile(r"Concat /model/layers\.\d+/self_attn/Concat(_1)?$")
    assert not any(cache_concat.match(w) or w.startswith(("output opkv", "Expand")) for w in whats)
    assert sum(w.startswith("output ") for w in whats) == 1 and "output logits" in whats
    # tokens and positions: the three Gathers read them on the device; nothing of the mask / shape subgraphs is a launch
    assert sorted(w for w in whats if w.startswith("Gather ")) == ["Gather /model/embed_tokens/Gather", "Gather /rotary/Gather", "Gather /rotary/Gather_1"]
    assert not any(w.split(" ")[0] in ("Range", "Less", "Where", "Cast", "Shape", "ConstantOfShape") for w in whats)
    # everything else is the T = chunk pass the ordinary plan would be: same launches, attention and cache movement apart
    def rest(ws):
        return [w for w in ws if not (cache_concat.match(w) or w.startswith(("KVAppend", "ScaledDotProductAttention", "output opkv")))]
    rows = len(PROMPT) + 3
    m.drop_tensor("logits")
    llama.forward_resident(m, CFG, list(range(1, C + 1)), False, rows)
    ordinary = _steps(m.hip_plan_info())
    assert len(rest(ordinary)) > 20 and rest(ordinary) == rest(whats)
    m.close()


@pytest.mark.parametrize("file,value,why", [("mask_2E_onef.bin", 2.0, "a key at or before its query row is barred"),
                                             ("mask_2E_min.bin", 0.0, "a key behind its query row is not barred")],
                         ids=["padding_term", "nothing_barred"])
def test_a_mask_that_is_not_exactly_causal_is_refused_by_name(stub_backend, file, value, why):
    """the chunk attention works the causal bound out of the device-side row and reads no mask, so the plan-time mask must say exactly that.  Two graphs
    whose mask says something else, made by rewriting one scalar of the mask subgraph: `1 - attention_mask` computed from 2 (a padding term that is not
    all zeros: it bars every key), and the barred value 0 (no key barred)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model, OnnxStreamError
    cfg = dataclasses.replace(CFG, name="llama_tiny_other_mask")
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        llama.build_llama(DirSink(d), cfg)
        assert os.path.getsize(d + file) == 2          # (one float16)
        with open(d + file, "wb") as f:
            f.write(np.float16(value).tobytes())
        m = Model(b.LIB_HOST, 1, "ram+nocache")
        m.add_outputs_convert("logits")
        llama.configure(m, cfg, d, sdpa=True, upcast=True)
        llama.forward_resident(m, cfg, PROMPT, True, 0, keep_logits=True)
        with pytest.raises(OnnxStreamError, match=r"Model::hip_turn: ScaledDotProductAttention \(.*\): the attention mask is not the causal mask of a chunk of 4 rows "
                                                  r"behind 60 cached rows \(" + why + r"\)"):
            llama.turn(m, cfg, [1, 2, 3], 2, chunk=4)
        with pytest.raises(OnnxStreamError, match="no chunk plan"):
            m.hip_prefill_plan_info()
        m.close()


def test_shapes_left_in_the_model_and_the_capacity_rule(stub_backend, model_dir):
    m = _model(model_dir)
    P = len(PROMPT)
    built = m.hip_plans_built()
    # max_new = 0: the prefill alone; no decode plan is needed
    llama.turn(m, CFG, [1, 2, 3], 0, chunk=2)
    assert m.hip_plans_built() == built + 1
    assert m.hip_prefill_plan_info().startswith("prefill chunk 2 capacity 64\n")
    assert m.get_tensor("logits")[0].shape == (1, 1, CFG.vocab)
    for i in range(NC):
        assert m.get_tensor_f16(f"opkv{i}").shape == (1, CFG.kv_heads, P + 3, CFG.head_dim)
    assert sorted(m.get_all_tensor_names()) == sorted(["logits"] + [f"opkv{i}" for i in range(NC)])
    P += 3
    # derived: max(P + ceil(n / chunk) * chunk, P + n + max_new), rounded up to 64 -- here the padded chunk decides: 8 + 64 > 64, while 8 + 1 + 4 is not
    llama.turn(m, CFG, [4], 4, chunk=64)
    assert m.hip_prefill_plan_info().startswith("prefill chunk 64 capacity 128\n")
    assert m.hip_decode_plan_info().startswith("decode capacity 64\n")          # (the loop's own rule: P + n + max_new)
    P += 1
    assert m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, P, CFG.head_dim)
    # ... and here the new tokens decide
    built = m.hip_plans_built()
    llama.turn(m, CFG, [5, 6], 120, chunk=64)
    assert m.hip_plans_built() == built + 2          # 9 + 2 + 120 = 131 rows: beyond the 128 of the chunk plan and the 64 of the decode plan
    assert m.hip_prefill_plan_info().startswith("prefill chunk 64 capacity 192\n") and m.hip_decode_plan_info().startswith("decode capacity 192\n")
    built = m.hip_plans_built()
    llama.turn(m, CFG, [5], 4, chunk=64)             # 11 + 64 and 11 + 1 + 4 fit: nothing is built
    assert m.hip_plans_built() == built
    P += 1
    P += 2
    # as given: at least that many rows, for both plans; the turns that follow build nothing
    llama.turn(m, CFG, [7], 1, chunk=4, capacity=200)
    assert m.hip_prefill_plan_info().startswith("prefill chunk 4 capacity 256\n") and m.hip_decode_plan_info().startswith("decode capacity 256\n")
    built = m.hip_plans_built()
    llama.turn(m, CFG, [8, 9, 10], 1, chunk=4)
    llama.turn(m, CFG, [8], 100, chunk=4, capacity=256)
    assert m.hip_plans_built() == built
    P += 1 + 3 + 1
    assert m.get_tensor_f16(f"opkv{NC - 1}").shape == (1, CFG.kv_heads, P, CFG.head_dim)
    # the first turn of the app: zero-length caches as pushed, consumed by the turn
    m.clear_tensors()
    llama.turn(m, CFG, [1, 2, 3, 4, 5], 2, chunk=4, first=True)
    assert sorted(m.get_all_tensor_names()) == sorted(["logits"] + [f"opkv{i}" for i in range(NC)])
    assert m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, 5, CFG.head_dim)
    m.close()


@pytest.mark.parametrize("upcast,fusion", [(True, 2), (True, 0)])
def test_the_decode_plan_is_the_one_generate_builds(stub_backend, model_dir, upcast, fusion):
    def strip(info):          # (the arena placement depends on what the pool handed out before: the steps are the plan)
        return [info.splitlines()[0]] + _steps(info)
    m = _model(model_dir, upcast=upcast, options=(("hip_fusion_level", fusion),))
    llama.turn(m, CFG, [7, 8, 9], 4, chunk=8)
    got = strip(m.hip_decode_plan_info())
    m.close()
    m = _model(model_dir, upcast=upcast, options=(("hip_fusion_level", fusion),))
    m.drop_tensor("logits")
    llama.forward_resident(m, CFG, [7, 8, 9], False, len(PROMPT), keep_logits=True)
    llama.generate(m, CFG, 4)
    assert strip(m.hip_decode_plan_info()) == got
    m.close()
