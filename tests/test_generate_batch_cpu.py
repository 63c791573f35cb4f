"""Several sampled sequences per prompt in the device token loop (model_hip_generate_batch), CPU side: the host logic over the no-op stand-in for
libosgpu.so (tests/stub/make_stub.py).  Its launches compute nothing, so no sequence ever draws a token; what can be checked here is what the host
does around the loop:

* include/osgpu.h declares the three batch entry points and the host library exports the call;
* every refusal, with its prefix -- and model_hip_generate's own refusal of a batch of two, unchanged;
* the plumbing: the n_seq states and the seeds as the first osg_decode_sample_batch launch finds them on the "device" (the stand-in built here records
  them -- the one entry point given a body of its own for this file), the decode plan rebuilt when n_seq changes and kept when it does not, its text, and
  m_data byte for byte as before the call."""
import ctypes
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
PFX = "Model::hip_generate_batch: "

# the stand-in's osg_decode_sample_batch: computes nothing, like every arithmetic launch, but keeps what the FIRST launch after a reset was handed
RECORDER_GLOBALS = """
int stub_rec_calls = 0, stub_rec_n_seq = 0, stub_rec_state[4 * 64];
unsigned long long stub_rec_seeds[64], stub_rec_draw_base = 0;
long stub_rec_max_tokens = 0;
"""
RECORDER_BODY = """{
    (void)ctx; (void)logits; (void)V; (void)eos_id; (void)input_ids; (void)position_ids; (void)tokens; (void)temperature; (void)top_k; (void)top_p;
    if (stub_rec_calls++ == 0 && n_seq <= 64) {
        stub_rec_n_seq = n_seq;
        stub_rec_max_tokens = max_tokens;
        stub_rec_draw_base = draw_base;
        memcpy(stub_rec_state, state, (size_t)n_seq * 16);
        memcpy(stub_rec_seeds, seeds, (size_t)n_seq * 8);
    }
    return 0;
}"""


@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    with tempfile.TemporaryDirectory() as d:
        old_special, old_helpers = dict(make_stub.SPECIAL), make_stub.HALF_HELPERS
        make_stub.SPECIAL["osg_decode_sample_batch"] = RECORDER_BODY
        make_stub.HALF_HELPERS = old_helpers + RECORDER_GLOBALS
        try:
            so = make_stub.build(d)
        finally:
            make_stub.SPECIAL.clear()
            make_stub.SPECIAL.update(old_special)
            make_stub.HALF_HELPERS = old_helpers
        old = os.environ.get("OSGPU_LIB")
        os.environ["OSGPU_LIB"] = so
        try:
            yield ctypes.CDLL(so)          # (the same loaded image the host library binds: its globals are the ones read below)
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


def _model(model_dir, prefill=True):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    m.add_outputs_convert("logits")
    llama.configure(m, CFG, model_dir, sdpa=True, upcast=True)
    if prefill:
        llama.forward_resident(m, CFG, PROMPT, True, 0, keep_logits=True)
    return m


def _steps(info):
    return [ln.split(" | ", 1)[1] for ln in info.splitlines() if ln.startswith("step ")]


def _recorded(lib):
    g = lambda ty, name: ty.in_dll(lib, name)
    n = g(ctypes.c_int, "stub_rec_n_seq").value
    state = np.array(g(ctypes.c_int * 256, "stub_rec_state")[:4 * n], np.int32).reshape(n, 4)
    seeds = [int(x) for x in g(ctypes.c_ulonglong * 64, "stub_rec_seeds")[:n]]
    return dict(calls=g(ctypes.c_int, "stub_rec_calls").value, n_seq=n, state=state, seeds=seeds, max_tokens=g(ctypes.c_long, "stub_rec_max_tokens").value,
                draw_base=g(ctypes.c_ulonglong, "stub_rec_draw_base").value)


def _reset(lib):
    ctypes.c_int.in_dll(lib, "stub_rec_calls").value = 0
    ctypes.c_int.in_dll(lib, "stub_rec_n_seq").value = 0


def test_the_entry_points_are_declared_and_the_call_is_exported():
    from onnxstream_amd import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "osgpu.h")).read(), flags=re.S)
    for name in ("osg_decode_sample_batch", "osg_kv_append_at_batch", "osg_sdpa_len_batch"):
        assert re.search(r"^int " + name + r"\(osg_ctx\* ctx,", src, flags=re.M), name
    # the single-sequence entry points are still there, with the signatures they had
    assert "int osg_kv_append_at(osg_ctx* ctx, const void* src, void* cache, const int* row, int kv_heads, long cap, int d);" in src
    assert re.search(r"int osg_sdpa_len\(osg_ctx\* ctx, osg_dtype dtype, const void\* q, const void\* k, const void\* v, const void\* mask, void\* o, const int\* tkv,\s+"
                     r"long kv_head_stride, long kv_batch_stride, long cap, int batch, int q_heads, int kv_heads, int D, float scale\);", src)
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    lib = ctypes.CDLL(b.LIB_HOST)
    for name in ("model_hip_generate_batch", "model_hip_generate_sampled", "model_hip_generate"):
        assert hasattr(lib, name), name


def test_refusals(stub_backend, model_dir):
    from onnxstream_amd.bindings import OnnxStreamError
    m = _model(model_dir, prefill=False)
    m.set_use_fp16_arithmetic(True)
    with pytest.raises(OnnxStreamError, match=PFX + r"run\(\) once first"):
        m.generate_batch(2, 4, NC, [1, 2], 1.0)
    m.close()

    m = _model(model_dir)
    gb = lambda n_seq=2, max_new=4, nc=NC, seeds=(1, 2), t=1.0, **kw: m.generate_batch(n_seq, max_new, nc, seeds, t, **kw)
    # what is new in this call
    with pytest.raises(OnnxStreamError, match=PFX + "n_seq must be >= 1"):
        gb(n_seq=0, seeds=())
    with pytest.raises(OnnxStreamError, match=PFX + "n_seq must be >= 1"):
        gb(n_seq=-3, seeds=())
    with pytest.raises(OnnxStreamError, match=PFX + "no seeds"):
        gb(seeds=None)
    with pytest.raises(OnnxStreamError, match=PFX + "temperature must be > 0: greedy sequences from one prompt are all the same sequence"):
        gb(t=0.0)
    # everything model_hip_generate_sampled refuses
    for t in (-1.0, float("nan"), float("inf")):
        with pytest.raises(OnnxStreamError, match=PFX + "temperature must be finite and >= 0"):
            gb(t=t)
    with pytest.raises(OnnxStreamError, match=PFX + "temperature is too small"):
        gb(t=1e-42)
    with pytest.raises(OnnxStreamError, match=PFX + "top_k must be >= 0"):
        gb(top_k=-1)
    for p in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(OnnxStreamError, match=PFX + r"top_p must be in \(0, 1\]"):
            gb(top_p=p)
    with pytest.raises(OnnxStreamError, match=PFX + "max_new must be >= 0"):
        gb(max_new=-1)
    with pytest.raises(OnnxStreamError, match=PFX + "needs at least one key/value cache"):
        gb(nc=0)
    with pytest.raises(OnnxStreamError, match=PFX + "tensor not found: nologits"):
        gb(logits="nologits")
    with pytest.raises(OnnxStreamError, match=PFX + "tensor not found: nokv0"):
        gb(cache_out="nokv")
    with pytest.raises(OnnxStreamError, match=PFX + "tensor not found: opkv4"):
        gb(nc=NC + 1)
    with pytest.raises(OnnxStreamError, match=PFX + "the logits tensor 'opkv0' must be float32"):
        gb(logits="opkv0")
    for opt, msg in (("use_uint8_arithmetic", "not available with uint8 arithmetic"), ("hip_stream_weights", "not available in streamed-weights mode"),
                     ("use_fp16_arithmetic", "needs fp16 arithmetic")):
        m._set_option(opt, opt != "use_fp16_arithmetic")
        with pytest.raises(OnnxStreamError, match=PFX + msg):
            gb()
        m._set_option(opt, opt == "use_fp16_arithmetic")
    m.set_use_scaled_dp_attn_op(False)
    with pytest.raises(OnnxStreamError, match=PFX + "needs m_use_scaled_dp_attn_op"):
        gb()
    m.set_use_scaled_dp_attn_op(True)
    with pytest.raises(OnnxStreamError, match=PFX + "positions up to 260 are needed"):
        gb(max_new=256)
    # the prefill is a batch-1 run(): logits of two samples are refused here as in the single call, whose message has not changed
    m.drop_tensor("logits")
    m.set_use_fp16_arithmetic(False)
    m.add_tensor("logits", np.zeros((2, 1, CFG.vocab), np.float32))
    m.set_use_fp16_arithmetic(True)
    with pytest.raises(OnnxStreamError, match=PFX + "the batch must be 1"):
        gb()
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: the batch must be 1"):
        m.generate(4, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: the batch must be 1"):
        m.generate(4, NC, temperature=0.8, seed=3)
    m.close()


def test_states_seeds_plan_and_m_data(stub_backend, model_dir):
    lib = stub_backend
    m = _model(model_dir)
    P = len(PROMPT)
    names = sorted(m.get_all_tensor_names())
    lg0 = m.get_tensor("logits")[0].copy()
    kv0 = [m.get_tensor_f16(f"opkv{i}").copy() for i in range(NC)]
    built = m.hip_plans_built()

    # ---- three sequences: three states (-1, P, 0, 0), the seeds in order, the shared arguments ----
    seeds = [2 ** 64 - 1, 5, 0x0123456789ABCDEF]
    _reset(lib)
    toks, stop, trace, ms = m.generate_batch(3, 6, NC, seeds, 0.8, top_k=7, top_p=0.9, draw_base=100, trace=True)
    assert [len(t) for t in toks] == [0, 0, 0] and list(stop) == [0, 0, 0] and [t.shape for t in trace] == [(0, CFG.vocab)] * 3      # (the stub draws nothing)
    r = _recorded(lib)
    assert r["calls"] == 6 and r["n_seq"] == 3 and r["max_tokens"] == 6 and r["draw_base"] == 100
    assert r["state"].tolist() == [[-1, P, 0, 0]] * 3
    assert r["seeds"] == seeds
    assert m.hip_plans_built() == built + 1
    info = m.hip_decode_plan_info()
    assert info.splitlines()[0] == "decode capacity 64 sequences 3"
    whats = _steps(info)
    assert sorted(w for w in whats if w.startswith("KVAppend")) == sorted(f"KVAppend(batch) /model/layers.{l}/self_attn/Concat{s}" for l in range(CFG.layers) for s in ("", "_1"))
    assert sum(w.startswith("ScaledDotProductAttention(len, batch) ") for w in whats) == CFG.layers
    assert not any(w.startswith(("ScaledDotProductAttention ", "ScaledDotProductAttention(len) ", "KVAppend ", "output opkv", "Expand")) for w in whats)
    assert sorted(w for w in whats if w.startswith("Gather ")) == ["Gather /model/embed_tokens/Gather", "Gather /rotary/Gather", "Gather /rotary/Gather_1"]
    assert sum(w.startswith("output ") for w in whats) == 1 and "output logits" in whats

    # ---- the same n_seq: the plan is kept (other seeds, another rule, another budget within the capacity) ----
    _reset(lib)
    llama.generate_batch(m, CFG, 3, 64 - P, temperature=1.3, seed=2 ** 64 - 2)
    assert m.hip_plans_built() == built + 1
    r = _recorded(lib)
    assert r["seeds"] == [2 ** 64 - 2, 2 ** 64 - 1, 0] and r["state"].tolist() == [[-1, P, 0, 0]] * 3 and r["calls"] == 64 - P      # (seed + s modulo 2^64)
    # ---- another n_seq: rebuilt; a larger capacity: rebuilt ----
    _reset(lib)
    llama.generate_batch(m, CFG, 5, 4, seed=9)
    assert m.hip_plans_built() == built + 2 and m.hip_decode_plan_info().startswith("decode capacity 64 sequences 5\n")
    r = _recorded(lib)
    assert r["n_seq"] == 5 and r["seeds"] == [9, 10, 11, 12, 13] and r["state"].tolist() == [[-1, P, 0, 0]] * 5
    llama.generate_batch(m, CFG, 5, 4, seed=9, sync_every=1)
    assert m.hip_plans_built() == built + 2
    llama.generate_batch(m, CFG, 5, 64 - P + 1, seed=9)
    assert m.hip_plans_built() == built + 3 and m.hip_decode_plan_info().startswith("decode capacity 128 sequences 5\n")
    # ---- n_seq = 1 is the plan of the single-sequence calls, with their step texts: one of them after the other builds nothing ----
    llama.generate_batch(m, CFG, 1, 4, seed=1)
    assert m.hip_plans_built() == built + 4
    info1 = m.hip_decode_plan_info()
    assert info1.splitlines()[0] == "decode capacity 64"
    llama.generate(m, CFG, 4, temperature=0.8, seed=1)
    llama.generate(m, CFG, 4)
    assert m.hip_plans_built() == built + 4 and m.hip_decode_plan_info() == info1
    w1 = _steps(info1)
    assert sum(w.startswith("KVAppend ") for w in w1) == NC and sum(w.startswith("ScaledDotProductAttention(len) ") for w in w1) == CFG.layers
    assert not any("batch" in w for w in w1)
    # (the batched plan is the same pass, launch for launch, but for the three batch forms)
    norm = lambda ws: [w.replace("KVAppend(batch) ", "KVAppend ").replace("(len, batch) ", "(len) ").replace("RoPE(batch) ", "RoPE ") for w in ws]
    assert norm(whats) == w1
    # max_new = 0: nothing runs, nothing is built
    toks, stop, trace, ms = llama.generate_batch(m, CFG, 4, 0, trace=True)
    assert [len(t) for t in toks] == [0] * 4 and ms == 0.0 and m.hip_plans_built() == built + 4

    # ---- m_data is as it was: names, the prompt's logits, the caches ----
    assert sorted(m.get_all_tensor_names()) == names
    assert m.get_tensor("logits")[0].tobytes() == lg0.tobytes() and m.get_tensor("logits")[0].shape == (1, P, CFG.vocab)
    for i in range(NC):
        c = m.get_tensor_f16(f"opkv{i}")
        assert c.shape == (1, CFG.kv_heads, P, CFG.head_dim) and c.tobytes() == kv0[i].tobytes(), i
    # and the app goes on through run()
    m.drop_tensor("logits")
    lg = llama.forward_resident(m, CFG, [1, 2, 3], False, P)
    assert lg.shape == (1, 3, CFG.vocab) and m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, P + 3, CFG.head_dim)
    m.close()
