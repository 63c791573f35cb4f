"""One chat turn on the device (model_hip_turn; reference src/llm.cpp:456-497), GPU side.

* The device turn against the host-driven chunked flow of the same backend, bit for bit: every piece of the prompt through llama.forward (the last
  one padded with token 0 up to the chunk, the caches then cut back to the real rows), then the host token loop -- tokens, the logits of every decode
  pass, the final logits and every cache, over two turns; a follow-up prompt through the ordinary run(); max_new = 0; an end-of-sequence token; the
  sampled rule against forward_resident + generate; the plans kept within capacity and rebuilt beyond it.
* Against the reference's fixture (tests/golden/llama_tiny*.npz) with the prompt fed in chunks of 4, within the bounds tests/test_llm_flow.py and
  tests/test_generate_gpu.py::test_device_loop_vs_reference hold the per-call path to."""
import os
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
f16, f32 = np.float16, np.float32
FIX = {"tiny": (llama.TINY, np.load(os.path.join(HERE, "golden", "llama_tiny.npz"))),
       "wide": (llama.TINY_WIDE, np.load(os.path.join(HERE, "golden", "llama_tiny_wide.npz")))}
pytestmark = pytest.mark.gpu
MAX_NEW = 4
# (n_prompt, chunk): one padded piece; exact; three pieces, the last padded.  Each from P = 0, then a second turn of 5 tokens in chunks of 8 on top.
CASES = [(5, 16), (16, 16), (21, 8)]
TURN2 = (5, 8)


def prompt_of(cfg, n, salt):
    return [int(t) for t in np.random.default_rng(1000 * salt + n).integers(1, cfg.vocab, n)]


def ref_argmax(row):
    """src/llm.cpp:355-370: prev = -1.0f; an element is taken when v >= prev"""
    prev, best = f32(-1.0), -1
    for i, v in enumerate(row):
        if v >= prev:
            prev, best = v, i
    return best


def _model(model_dir, cfg, upcast, fusion, graph, resident, convert=True):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    for k, v in (("hip_autotune", 0), ("hip_fusion_level", fusion), ("hip_use_graph", graph), ("hip_resident_outputs", resident)):
        m._set_option(k, v)
    if convert:
        m.add_outputs_convert("logits")
    llama.configure(m, cfg, model_dir, sdpa=True, upcast=upcast)
    return m


def _caches(m, cfg):
    return [m.get_tensor_f16(f"opkv{i}") for i in range(2 * cfg.layers)]


def _host_turn(m, cfg, prompt, past, chunk, max_new, eos=-1):
    """the specification: the prompt in pieces of `chunk` tokens through llama.forward (existing public functions only), the last piece padded with
    token 0, the caches cut back to the real rows and logits row r - 1 taken; then the app's token loop (src/llm.cpp:472-496), one run() per token.
    Returns (tokens, stop, logits of every decode pass, the logits row of the last pass that ran, the caches)."""
    P = past[0].shape[2] if past is not None else 0
    assert P + -(-len(prompt) // chunk) * chunk <= cfg.max_pos          # (the oracle's padded rows carry real positions: they must exist in the rotary table)
    row = None
    for at in range(0, len(prompt), chunk):
        piece = prompt[at:at + chunk]
        r = len(piece)
        lg, new_past = llama.forward(m, cfg, piece + [0] * (chunk - r), past)
        past = [np.ascontiguousarray(c[:, :, :P + r]) for c in new_past]
        row = lg[0, r - 1].copy()
        P += r
    toks, trace, stop = [], [], 0
    for _ in range(max_new):
        tok = ref_argmax(row)
        if tok < 0:
            stop = 2
            break
        if tok == eos:
            stop = 1
            break
        toks.append(tok)
        lg, past = llama.forward(m, cfg, [tok], past)
        row = lg[0, -1].copy()
        trace.append(row)
        P += 1
    return toks, stop, trace, row, past


@pytest.fixture(scope="module")
def model_dirs():
    with tempfile.TemporaryDirectory() as d:
        dirs = {}
        for name, (cfg, _) in FIX.items():
            dirs[name] = os.path.join(d, name) + "/"
            os.makedirs(dirs[name])
            llama.build_llama(DirSink(dirs[name]), cfg)
        yield dirs


_host_cache = {}


def host_flow(model_dirs, which, upcast, fusion):
    """the host-driven flow of every case, computed once per (model, upcast, fusion) and shared (hip_use_graph and hip_resident_outputs do not change
    the host flow's bits: tests/test_llm_flow.py, tests/test_planner_cpu.py)"""
    key = (which, upcast, fusion)
    if key not in _host_cache:
        cfg, _ = FIX[which]
        m = _model(model_dirs[which], cfg, upcast, fusion, 1, 0, convert=False)
        out = {}
        for n, chunk in CASES:
            p1, p2 = prompt_of(cfg, n, 1), prompt_of(cfg, TURN2[0], 2)
            t1 = _host_turn(m, cfg, p1, None, chunk, MAX_NEW)
            t2 = _host_turn(m, cfg, p2, t1[4], TURN2[1], MAX_NEW)
            follow, _ = llama.forward(m, cfg, [1, 2, 3], t2[4])
            out[(n, chunk)] = (t1, t2, follow)
        m.close()
        _host_cache[key] = out
    return _host_cache[key]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_turn(m, cfg, got, want, rows):
    toks, stop, trace, _ = got
    w_toks, w_stop, w_trace, w_row, w_past = want
    assert list(toks) == w_toks and stop == w_stop
    assert trace.shape == (len(w_toks), cfg.vocab)
    for n in range(len(w_toks)):
        assert bits(trace[n]) == bits(w_trace[n]), n
    lg = m.get_tensor("logits")[0]
    assert lg.shape == (1, 1, cfg.vocab) and bits(lg[0, 0]) == bits(w_row)
    for i, c in enumerate(_caches(m, cfg)):
        assert c.shape == (1, cfg.kv_heads, rows, cfg.head_dim), (i, c.shape)
        assert bits(c) == bits(w_past[i].astype(f16)), i          # (the oracle's caches are the fp16 values as fp32)


def first_run(m, cfg):
    """a run() must have happened (the app's weight-loading pass); its tensors are dropped: the conversation starts empty"""
    llama.forward_resident(m, cfg, [1], True, 0)
    m.clear_tensors()


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("fusion", [0, 2])
@pytest.mark.parametrize("upcast", [False, True])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_device_turn_equals_the_host_driven_chunked_flow(model_dirs, which, upcast, fusion, graph, resident):
    cfg, _ = FIX[which]
    H = host_flow(model_dirs, which, upcast, fusion)
    for n, chunk in CASES:
        t1, t2, follow = H[(n, chunk)]
        assert len(t1[0]) == MAX_NEW and len(t2[0]) == MAX_NEW          # (no invalid argmax on the way: every pass of the table is compared)
        m = _model(model_dirs[which], cfg, upcast, fusion, graph, resident)
        first_run(m, cfg)
        got = llama.turn(m, cfg, prompt_of(cfg, n, 1), MAX_NEW, chunk=chunk, trace=True, first=True)
        check_turn(m, cfg, got, t1, n + MAX_NEW)
        got = llama.turn(m, cfg, prompt_of(cfg, TURN2[0], 2), MAX_NEW, chunk=TURN2[1], trace=True)
        check_turn(m, cfg, got, t2, n + MAX_NEW + TURN2[0] + MAX_NEW)
        # the app goes on with its next prompt through the ordinary run()
        m.drop_tensor("logits")
        lg = llama.forward_resident(m, cfg, [1, 2, 3], False, n + 2 * MAX_NEW + TURN2[0])
        assert bits(lg) == bits(follow), (n, chunk)
        m.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_a_turn_without_new_tokens_leaves_the_prefill(model_dirs, graph):
    cfg, _ = FIX["tiny"]
    n, chunk = CASES[2]
    prompt = prompt_of(cfg, n, 1)
    mh = _model(model_dirs["tiny"], cfg, True, 2, 1, 0, convert=False)
    _, _, _, w_row, w_past = _host_turn(mh, cfg, prompt, None, chunk, 0)
    mh.close()
    for resident in (0, 1):
        m = _model(model_dirs["tiny"], cfg, True, 2, graph, resident)
        first_run(m, cfg)
        toks, stop, trace, _ = llama.turn(m, cfg, prompt, 0, chunk=chunk, trace=True, first=True)
        assert list(toks) == [] and stop == 0
        lg = m.get_tensor("logits")[0]
        assert lg.shape == (1, 1, cfg.vocab) and bits(lg[0, 0]) == bits(w_row)
        for i, c in enumerate(_caches(m, cfg)):
            assert c.shape == (1, cfg.kv_heads, n, cfg.head_dim) and bits(c) == bits(w_past[i].astype(f16)), i
        assert "pkv0" not in m.get_all_tensor_names()          # (consumed, as run() consumes its inputs)
        m.close()


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_an_end_of_sequence_token_stops_the_turn_where_the_host_loop_stops(model_dirs, which):
    cfg, _ = FIX[which]
    n, chunk = CASES[0]
    prompt = prompt_of(cfg, n, 1)
    mh = _model(model_dirs[which], cfg, True, 2, 1, 0, convert=False)
    free = _host_turn(mh, cfg, prompt, None, chunk, MAX_NEW)
    for k in (0, 2):          # the first pick already, and the third
        eos = free[0][k]
        want = _host_turn(mh, cfg, prompt, None, chunk, MAX_NEW, eos=eos)
        want_n = free[0].index(eos)
        assert want[1] == 1 and len(want[0]) == want_n <= k
        for sync_every in (1, 0):
            m = _model(model_dirs[which], cfg, True, 2, 1, 1)
            first_run(m, cfg)
            got = llama.turn(m, cfg, prompt, MAX_NEW, chunk=chunk, eos_id=eos, sync_every=sync_every, trace=True, first=True)
            check_turn(m, cfg, got, want, n + want_n)
            m.close()
    mh.close()


def test_sampled_turn_gives_the_tokens_of_forward_and_generate(model_dirs):
    """chunk == n_prompt: the prefill is the very pass forward_resident runs, so the sampled loops start from equal logits and equal caches"""
    cfg, _ = FIX["tiny"]
    prompt = prompt_of(cfg, 16, 1)
    rule = dict(temperature=0.8, top_k=5, seed=1234)
    m = _model(model_dirs["tiny"], cfg, True, 2, 1, 1)
    llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    w_toks, w_stop, w_trace, _ = llama.generate(m, cfg, MAX_NEW, trace=True, **rule)
    w_caches = _caches(m, cfg)
    m.close()
    m = _model(model_dirs["tiny"], cfg, True, 2, 1, 1)
    first_run(m, cfg)
    toks, stop, trace, _ = llama.turn(m, cfg, prompt, MAX_NEW, chunk=16, trace=True, first=True, **rule)
    assert len(w_toks) == MAX_NEW and list(toks) == list(w_toks) and stop == w_stop
    assert bits(trace) == bits(w_trace)
    for i, c in enumerate(_caches(m, cfg)):
        assert bits(c) == bits(w_caches[i]), i
    m.close()


def test_plans_are_kept_within_capacity_and_rebuilt_beyond(model_dirs):
    cfg, _ = FIX["tiny"]
    m = _model(model_dirs["tiny"], cfg, True, 2, 1, 1)
    first_run(m, cfg)
    llama.turn(m, cfg, prompt_of(cfg, 5, 1), 2, chunk=8, first=True)
    assert m.hip_prefill_plan_info().startswith("prefill chunk 8 capacity 64\n") and m.hip_decode_plan_info().startswith("decode capacity 64\n")
    built = m.hip_plans_built()
    llama.turn(m, cfg, prompt_of(cfg, 5, 2), 2, chunk=8)          # 7 + 8 <= 64 and 7 + 5 + 2 <= 64: nothing is built
    assert m.hip_plans_built() == built
    # beyond 64 rows (the rotary table of this model ends at 64 positions, so the capacity is asked for): both plans are built again
    llama.turn(m, cfg, prompt_of(cfg, 5, 3), 2, chunk=8, capacity=65)
    assert m.hip_plans_built() == built + 2
    assert m.hip_prefill_plan_info().startswith("prefill chunk 8 capacity 128\n") and m.hip_decode_plan_info().startswith("decode capacity 128\n")
    m.close()


@pytest.mark.parametrize("which,upcast", [("tiny", False), ("tiny", True), ("wide", True)])
def test_device_turn_vs_reference(model_dirs, which, upcast):
    """Against the reference's own run of the flow (the fixture), the prompt fed in chunks of 4 (two pieces, the second padded): the tokens are the
    fixture's greedy tokens; the logits of every pass and the caches within the bounds of tests/test_generate_gpu.py::test_device_loop_vs_reference
    and test_llm_flow.py's sdpa modes (2e-3 of the largest fp32 logit, and within 1e-3 or at least as close to the fp32 reference as the reference's
    own fp16 run + 1e-4; caches 1e-3).  tests/test_generate_cpu.py shows that the fixture's tokens do not hinge on a near-tie."""
    cfg, z = FIX[which]
    prompt, toks_fix = [int(t) for t in z["prompt"]], [int(t) for t in z["tokens"]]
    tag = "16u" if upcast else "16"
    n_ref = len(toks_fix)
    m = _model(model_dirs[which], cfg, upcast, 2, 1, 0)
    first_run(m, cfg)
    toks, stop, trace, _ = llama.turn(m, cfg, prompt, n_ref, chunk=4, trace=True, first=True)
    caches = _caches(m, cfg)
    m.close()
    assert list(toks) == toks_fix and stop == 0
    mx = max(float(np.abs(z[f"logits32_{s}"]).max()) for s in range(n_ref + 1))
    for n in range(n_ref):
        lg, r16, r32 = trace[n], z[f"logits{tag}_{n + 1}"][0, -1], z[f"logits32_{n + 1}"][0, -1]
        e16, e32, drift = np.abs(lg - r16).max() / mx, np.abs(lg - r32).max() / mx, np.abs(r16 - r32).max() / mx
        print(f"{which} upcast={upcast} pass {n}: err16 {e16:.2e} err32 {e32:.2e} (reference drift {drift:.2e})")
        assert e16 <= 2e-3 and (e16 <= 1e-3 or e32 <= drift + 1e-4), (n, e16, e32, drift)
    if which == "tiny":          # (the wide fixture's flow test holds no caches either)
        pm = max(float(np.abs(z[f"past32_{i}"]).max()) for i in range(len(caches)))
        rows = len(prompt) + n_ref
        for i, c in enumerate(caches):
            assert c.shape[2] == rows
            err = np.abs(c[:, :, :rows] - z[f"past{tag}_{i}"]).max() / pm
            print(f"cache {i}: {err:.2e}")
            assert err <= 1e-3, (i, err)
