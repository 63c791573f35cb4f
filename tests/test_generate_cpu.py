"""The LLM app's token loop on the device (model_hip_generate), CPU side: the host logic over the no-op stand-in for libosgpu.so
(tests/stub/make_stub.py -- its launches compute nothing, so osg_decode_pick never picks a token: every call reports 0 tokens and leaves the Model's
tensors as they were, which is what the contract says of a loop in which no pass ran).

* every refusal, with its message;
* the decode plan: one in-place append per cache, one length-form attention per layer, the token and the position read by Gathers only -- and a
  refusal when anything else would need their values while the plan is built;
* the plan is kept across calls while its capacity suffices, rebuilt beyond it; run()'s own plan goes on working;
* the fixtures themselves: at every step the reference's top-1 logit leads the runner-up by far more than the bound the device loop's logits are
  held to (tests/test_generate_gpu.py), so that the token identity asserted there cannot hinge on a near-tie."""
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
CFG = dataclasses.replace(llama.TINY, max_pos=256, name="llama_tiny_long")      # (room for positions beyond the first plan's capacity)
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
    with pytest.raises(OnnxStreamError, match=r"Model::hip_generate: run\(\) once first"):
        m.generate(4, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_decode_plan_info: no decode plan"):
        m.hip_decode_plan_info()
    m.close()

    m = _model(model_dir)
    built = m.hip_plans_built()
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: max_new must be >= 0"):
        m.generate(-1, NC)
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: tensor not found: nologits"):
        m.generate(4, NC, logits="nologits")
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: tensor not found: nokv0"):
        m.generate(4, NC, cache_out="nokv")
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: tensor not found: opkv4"):
        m.generate(4, NC + 1)
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: the logits tensor 'opkv0' must be float32"):
        m.generate(4, NC, logits="opkv0")
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: cache 'logits0' must be float16"):
        m.set_use_fp16_arithmetic(False)
        m.add_tensor("logits0", np.zeros((1, 2, 5, 16), np.float32))
        m.set_use_fp16_arithmetic(True)
        m.generate(4, 1, cache_out="logits")
    for opt, msg in (("use_uint8_arithmetic", "not available with uint8 arithmetic"), ("hip_stream_weights", "not available in streamed-weights mode"),
                     ("use_fp16_arithmetic", "needs fp16 arithmetic")):
        m._set_option(opt, opt != "use_fp16_arithmetic")
        with pytest.raises(OnnxStreamError, match="Model::hip_generate: " + msg):
            m.generate(4, NC)
        m._set_option(opt, opt == "use_fp16_arithmetic")
    m.set_use_scaled_dp_attn_op(False)
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: needs m_use_scaled_dp_attn_op"):
        m.generate(4, NC)
    m.set_use_scaled_dp_attn_op(True)
    # names the graph does not know: the plan cannot be built, and none is kept
    with pytest.raises(OnnxStreamError, match="input tensor not found: input.*ids"):          # (tensor names travel mangled: _ is _5F_)
        m.generate(4, NC, ids="noids")
    with pytest.raises(OnnxStreamError, match="input tensor not found: pkv0"):
        m.generate(4, NC, cache_in="nopkv")
    with pytest.raises(OnnxStreamError, match="no decode plan"):
        m.hip_decode_plan_info()
    # a batch of two
    m.drop_tensor("logits")
    m.set_use_fp16_arithmetic(False)
    m.add_tensor("logits", np.zeros((2, 1, CFG.vocab), np.float32))
    m.set_use_fp16_arithmetic(True)
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: the batch must be 1"):
        m.generate(4, NC)
    assert m.hip_plans_built() >= built
    m.close()


def test_a_host_evaluation_of_the_token_or_position_is_refused(stub_backend, model_dir):
    """the loop's token and position exist on the device only.  Handing the attention mask over as if it were the position input makes the mask subgraph
    (Cast -> Sub -> Mul, folded while the plan is built) need a device value: refused, by name"""
    from onnxstream_amd.bindings import OnnxStreamError
    m = _model(model_dir)
    with pytest.raises(OnnxStreamError, match=r"Model::hip_generate: Cast \(.*\) needs the value of 'attention.*mask' while the plan is built"):
        m.generate(4, NC, pos="attention_mask", mask="position_ids")
    m.close()


@pytest.mark.parametrize("upcast,fusion", [(False, 2), (True, 2), (True, 0)])
def test_decode_plan_shape(stub_backend, model_dir, upcast, fusion):
    m = _model(model_dir, upcast=upcast, options=(("hip_fusion_level", fusion),))
    ordinary = _steps(m.hip_plan_info())
    toks, stop, trace, ms = llama.generate(m, CFG, 4, trace=True)
    assert list(toks) == [] and stop == 0 and trace.shape == (0, CFG.vocab)         # (the stub picks nothing)
    info = m.hip_decode_plan_info()
    assert info.splitlines()[0] == "decode capacity 64"
    whats = _steps(info)
    appends = [w for w in whats if w.startswith("KVAppend ")]
    assert sorted(appends) == sorted(f"KVAppend /model/layers.{l}/self_attn/Concat{s}" for l in range(CFG.layers) for s in ("", "_1"))
    assert sum(w.startswith("ScaledDotProductAttention(len) ") for w in whats) == CFG.layers
    assert not any(w.startswith("ScaledDotProductAttention ") for w in whats)
    # the caches are neither copied in (Concat) nor out ("output opkv*") per pass, and repeat_kv stays virtual
    cache_concat = re.compile(r"Concat /model/layers\.\d+/self_attn/Concat(_1)?$")
    assert not any(cache_concat.match(w) or w.startswith(("output opkv", "Expand")) for w in whats)
    assert sum(w.startswith("output ") for w in whats) == 1 and "output logits" in whats
    # token and position: the three Gathers read them on the device; nothing of the mask / shape subgraphs is a launch
    assert sorted(w for w in whats if w.startswith("Gather ")) == ["Gather /model/embed_tokens/Gather", "Gather /rotary/Gather", "Gather /rotary/Gather_1"]
    assert not any(w.split(" ")[0] in ("Range", "Less", "Where", "Cast", "Shape", "ConstantOfShape") for w in whats)
    # everything else is the T = 1 pass the ordinary plan would be: same launches, attention and cache movement apart
    def rest(ws):
        return [w for w in ws if not (cache_concat.match(w) or w.startswith(("KVAppend", "ScaledDotProductAttention", "output opkv")))]
    llama.forward_resident(m, CFG, [7], False, len(PROMPT))
    assert rest(_steps(m.hip_plan_info())) == rest(whats)
    assert len(ordinary) > 0
    m.close()


def test_plan_is_kept_within_capacity_and_rebuilt_beyond(stub_backend, model_dir):
    m = _model(model_dir)
    P = len(PROMPT)
    built = m.hip_plans_built()
    # max_new = 0: nothing happens, nothing is built
    toks, stop, trace, ms = llama.generate(m, CFG, 0, trace=True)
    assert list(toks) == [] and stop == 0 and ms == 0.0 and m.hip_plans_built() == built
    from onnxstream_amd.bindings import OnnxStreamError
    with pytest.raises(OnnxStreamError, match="no decode plan"):
        m.hip_decode_plan_info()
    names = sorted(m.get_all_tensor_names())
    llama.generate(m, CFG, 4)
    assert m.hip_plans_built() == built + 1 and m.hip_decode_plan_info().startswith("decode capacity 64\n")
    llama.generate(m, CFG, 64 - P)                    # fills the capacity exactly
    llama.generate(m, CFG, 1, sync_every=1)
    assert m.hip_plans_built() == built + 1
    llama.generate(m, CFG, 64 - P + 1)                # one row more than it holds
    assert m.hip_plans_built() == built + 2 and m.hip_decode_plan_info().startswith("decode capacity 128\n")
    llama.generate(m, CFG, 4)                         # the larger plan serves the smaller call
    assert m.hip_plans_built() == built + 2
    # another option set: another plan
    m._set_option("hip_fusion_level", 0)
    llama.generate(m, CFG, 4)
    assert m.hip_plans_built() == built + 3
    m._set_option("hip_fusion_level", 2)
    # positions past the rotary table are refused before anything runs
    with pytest.raises(OnnxStreamError, match="Model::hip_generate: positions up to 260 are needed, the smallest table indexed by 'position.*ids' has 256 rows"):
        llama.generate(m, CFG, 256)
    # no pass ran (the stub picks nothing): the Model's tensors are as they were, and the app goes on through the ordinary run()
    assert sorted(m.get_all_tensor_names()) == names
    assert m.get_tensor("logits")[0].shape == (1, P, CFG.vocab)
    assert m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, P, CFG.head_dim)
    m.drop_tensor("logits")
    before = m.hip_plans_built()
    lg = llama.forward_resident(m, CFG, [1, 2, 3], False, P)
    assert lg.shape == (1, 3, CFG.vocab) and m.hip_plans_built() == before + 1
    assert m.get_tensor_f16("opkv0").shape == (1, CFG.kv_heads, P + 3, CFG.head_dim)
    assert sum(w.startswith("ScaledDotProductAttention ") for w in _steps(m.hip_plan_info())) == CFG.layers
    m.close()


@pytest.mark.parametrize("fixture", ["llama_tiny", "llama_tiny_wide"])
def test_fixture_tokens_do_not_hinge_on_a_near_tie(fixture):
    """tests/test_generate_gpu.py holds every logit of the device loop within 2e-3 of the largest fp32 logit of the reference's fp16 run.  Two logits
    can each move by that much, so greedy tokens are guaranteed equal where top-1 leads top-2 by more than 4e-3 of it -- at every step of both fixtures
    (measured: 3.0e-2 at the least), and with a single maximum, so that the app's last-of-equals rule does not come into play either."""
    z = np.load(os.path.join(HERE, "golden", fixture + ".npz"))
    toks = [int(t) for t in z["tokens"]]
    steps = len(toks) + 1
    mx = max(float(np.abs(z[f"logits32_{s}"]).max()) for s in range(steps))
    for tag in ("16", "16u"):
        for s in range(steps):
            row = z[f"logits{tag}_{s}"][0, -1]
            top = np.sort(row)[::-1]
            assert (top[0] - top[1]) / mx > 2 * 2e-3, (tag, s, (top[0] - top[1]) / mx)
            assert top[0] >= -1.0          # (the app's scan starts at -1)
            if s < len(toks):
                assert int(np.argmax(row)) == toks[s]
