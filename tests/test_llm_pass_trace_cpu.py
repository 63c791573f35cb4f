"""The two steps the device token loop (model_hip_generate) and the chat turn (model_hip_turn) share with each other, seen from the backend's side.

The stand-in for libosgpu.so is generated with its opt-in trace (tests/stub/make_stub.py, OSGPU_STUB_TRACE) over the graph entry points, osg_prefill_stage
(which stands in front of every pass of the chunk plan), osg_decode_pick (in front of every pass of the decode plan) and osg_copy_2d.  The stub's pick is
replaced by the state machine of include/osgpu.h with a token that is always 1, so that a loop takes tokens and `generate` reaches the exit that leaves its
caches in the Model; nothing else of the stub changes.  Checked against the contract (plan.h), never against a recorded run:

* the pass (Plan::run_pass): successive passes of either resident plan go eager, then osg_graph_begin .. osg_graph_end plus osg_graph_launch, then
  osg_graph_launch of that graph alone, across calls; with hip_use_graph off no graph entry point is reached;
* publishing the caches (generate after tokens were taken, a turn with max_new = 0, a turn whose loop took tokens), device-resident and host-side: behind the
  last pass exactly one osg_copy_2d per cache, fp16, from a capacity buffer (pitch cap * d) into a dense one (pitch rows * d), Hkv rows of rows * d elements,
  rows being the cache length the Model then reports and cap the capacity of the plan whose buffers hold it."""
import dataclasses
import os
import sys
import tempfile

import pytest

from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))
CFG = dataclasses.replace(llama.TINY, max_pos=256, name="llama_tiny_long")
NC = 2 * CFG.layers
STAGE, PICK = "osg_prefill_stage", "osg_decode_pick"

PICK_BODY = """{
    (void)ctx; (void)logits; (void)T; (void)V; (void)eos_id;
    stub_trace("osg_decode_pick\\n");
    if (!state[3] && state[2] < max_tokens) { tokens[state[2]++] = 1; input_ids[0] = 1; position_ids[0] = state[1]; state[0] = state[1]; state[1]++; }
    return 0;
}"""
COPY_TRACE = ('{ stub_trace("osg_copy_2d elem_size=%d src=%p src_pitch=%ld src_off=%ld dst=%p dst_pitch=%ld dst_off=%ld outer=%ld inner=%ld\\n", elem_size, (void*)src, '
              "src_pitch, src_off, dst, dst_pitch, dst_off, outer, inner);")
GRAPH_END_BODY = '{ (void)ctx; *out = (osg_graph*)calloc(1, 16); stub_trace("osg_graph_end g=%p\\n", (void*)*out); return 0; }'


@pytest.fixture(scope="module")
def trace_path():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    old_env = {k: os.environ.get(k) for k in ("OSGPU_LIB", make_stub.TRACE_ENV)}
    old_special, old_traced = dict(make_stub.SPECIAL), make_stub.traced
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        os.environ[make_stub.TRACE_ENV] = d + "trace.txt"
        make_stub.SPECIAL[PICK] = PICK_BODY
        make_stub.SPECIAL["osg_copy_2d"] = COPY_TRACE + old_special["osg_copy_2d"].strip()[1:]
        make_stub.SPECIAL["osg_graph_begin"] = '{ (void)ctx; stub_trace("osg_graph_begin\\n"); return 0; }'          # (no parameter to trace but ctx)
        make_stub.SPECIAL["osg_graph_end"] = GRAPH_END_BODY
        make_stub.traced = lambda name: name in ("osg_graph_launch", STAGE)
        try:
            so = make_stub.build(d + "stub")
        finally:
            make_stub.SPECIAL.clear()
            make_stub.SPECIAL.update(old_special)
            make_stub.traced = old_traced
        os.environ["OSGPU_LIB"] = so
        try:
            llama.build_llama(DirSink(d), CFG)
            yield d
        finally:
            for k, v in old_env.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def _model(d, resident=True, graph=True):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    m._set_option("hip_resident_outputs", int(resident))
    m._set_option("hip_use_graph", int(graph))
    m.add_outputs_convert("logits")
    llama.configure(m, CFG, d, sdpa=True, upcast=True)
    return m


def _call(d, fn):
    """the trace lines of fn(): [(entry point, {param: int})], pointers as integers"""
    path = d + "trace.txt"
    start = os.path.getsize(path) if os.path.exists(path) else 0
    fn()
    with open(path) as f:
        f.seek(start)
        lines = f.read().splitlines()
    out = []
    for ln in lines:
        name, *kv = ln.split(" ")
        out.append((name, {k: 0 if v == "(nil)" else int(v, 16) if v.startswith("0x") else int(v) for k, v in (item.split("=") for item in kv)}))
    return out


def _passes(lines, marker):
    """the graph entry points between each `marker` and the marker (of either plan) that follows it: one list per pass of that plan"""
    out = []
    for i, (name, _) in enumerate(lines):
        if name != marker:
            continue
        j = i + 1
        while j < len(lines) and lines[j][0] not in (STAGE, PICK):
            j += 1
        out.append([(n, a) for n, a in lines[i + 1:j] if n.startswith("osg_graph_")])
    return out


def _capacity(info):
    return int(info.splitlines()[0].split("capacity ")[1].split()[0])


def test_a_pass_goes_eager_then_captured_then_replayed(trace_path):
    d = trace_path
    m = _model(d)
    llama.forward_resident(m, CFG, [1], True, 0)          # the weight-loading pass
    m.clear_tensors()
    # a first turn builds both plans: 9 prompt tokens in chunks of 4 are three passes of the chunk plan, three new tokens three passes of the decode plan
    lines = _call(d, lambda: llama.turn(m, CFG, list(range(1, 10)), 3, chunk=4, first=True))
    graphs = {}
    for marker in (STAGE, PICK):
        eager, captured, replayed = _passes(lines, marker)
        assert eager == []
        assert [n for n, _ in captured] == ["osg_graph_begin", "osg_graph_end", "osg_graph_launch"]
        g = captured[1][1]["g"]
        assert g and captured[2][1]["g"] == g
        assert replayed == [("osg_graph_launch", {"g": g})]
        graphs[marker] = g
    assert graphs[STAGE] != graphs[PICK]
    # from then on every pass of either plan is a launch of its graph, whichever call makes it
    lines = _call(d, lambda: llama.turn(m, CFG, [4, 5, 6, 7, 8], 2, chunk=4))
    assert _passes(lines, STAGE) == [[("osg_graph_launch", {"g": graphs[STAGE]})]] * 2
    assert _passes(lines, PICK) == [[("osg_graph_launch", {"g": graphs[PICK]})]] * 2
    lines = _call(d, lambda: llama.generate(m, CFG, 2))
    assert _passes(lines, PICK) == [[("osg_graph_launch", {"g": graphs[PICK]})]] * 2 and _passes(lines, STAGE) == []
    m.close()


def test_without_hip_use_graph_no_pass_reaches_a_graph_entry_point(trace_path):
    d = trace_path
    m = _model(d, graph=False)
    llama.forward_resident(m, CFG, [1], True, 0)
    m.clear_tensors()
    lines = _call(d, lambda: (llama.turn(m, CFG, list(range(1, 10)), 3, chunk=4, first=True), llama.turn(m, CFG, [4, 5, 6], 3, chunk=4), llama.generate(m, CFG, 3)))
    assert [n for n, _ in lines].count(STAGE) == 4 and [n for n, _ in lines].count(PICK) == 9
    assert not [n for n, _ in lines if n.startswith("osg_graph_")]
    m.close()


def _check_published(m, lines, cap, rows):
    """behind the last pass (a replay: nothing of a pass's own steps follows it) one compacting copy per cache"""
    last = max(i for i, (n, _) in enumerate(lines) if n == "osg_graph_launch")
    assert all(n == "osg_copy_2d" for n, _ in lines[last + 1:])
    copies = [a for _, a in lines[last + 1:]]
    assert len(copies) == NC
    Hkv, hd = CFG.kv_heads, CFG.head_dim
    for i, a in enumerate(copies):
        assert m.get_tensor_f16(f"opkv{i}").shape == (1, Hkv, rows, hd)
        assert a["elem_size"] == 2 and a["src_pitch"] == cap * hd and a["dst_pitch"] == rows * hd and a["outer"] == Hkv and a["inner"] == rows * hd
        assert a["src_off"] == 0 and a["dst_off"] == 0 and a["src"] and a["dst"]
    assert len({a["src"] for a in copies}) == NC and len({a["dst"] for a in copies}) == NC


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_generate_publishes_each_cache_with_one_copy(trace_path, resident):
    d = trace_path
    m = _model(d, resident=resident)
    prompt = [3, 17, 42, 5, 9]
    llama.forward_resident(m, CFG, prompt, True, 0, keep_logits=True)
    res = []
    lines = _call(d, lambda: res.append(llama.generate(m, CFG, 4)))
    assert list(res[0][0]) == [1, 1, 1, 1]
    _check_published(m, lines, _capacity(m.hip_decode_plan_info()), len(prompt) + 4)
    assert m.get_tensor("logits")[0].shape == (1, 1, CFG.vocab)
    m.close()


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_turn_publishes_each_cache_with_one_copy(trace_path, resident):
    d = trace_path
    m = _model(d, resident=resident)
    llama.forward_resident(m, CFG, [1], True, 0)
    m.clear_tensors()
    # max_new = 0: the prefill's caches, out of the chunk plan's buffers
    lines = _call(d, lambda: llama.turn(m, CFG, list(range(1, 10)), 0, chunk=4, first=True))
    assert PICK not in [n for n, _ in lines]
    _check_published(m, lines, _capacity(m.hip_prefill_plan_info()), 9)
    lines = _call(d, lambda: llama.turn(m, CFG, [4, 5, 6, 7, 8], 0, chunk=4, capacity=100))          # (from cache_out, in a chunk plan of another capacity)
    assert _capacity(m.hip_prefill_plan_info()) == 128
    _check_published(m, lines, 128, 14)
    # the loop took tokens: published once, by the loop, out of the decode plan's buffers (a capacity of its own)
    res = []
    lines = _call(d, lambda: res.append(llama.turn(m, CFG, [9, 10, 11], 4, chunk=4)))
    assert list(res[0][0]) == [1, 1, 1, 1]
    assert _capacity(m.hip_decode_plan_info()) == 64
    _check_published(m, lines, 64, 14 + 3 + 4)
    assert sorted(m.get_all_tensor_names()) == sorted(["logits"] + [f"opkv{i}" for i in range(NC)])
    m.close()
