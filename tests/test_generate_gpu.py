"""The LLM app's token loop on the device (model_hip_generate; reference loop src/llm.cpp:472-496), GPU side.

* The three entry points behind it against what include/osgpu.h says of them: osg_decode_pick against a Python restatement of the app's argmax
  (src/llm.cpp:355-370) and of the state advance, osg_kv_append_at row by row, osg_sdpa_len bit for bit against osg_sdpa on compacted copies.
* The device loop against the host-driven loop of the same backend (synth.llama.forward_resident, one run() per token), bit for bit: tokens, the
  logits of every pass, the final logits and caches, the stop at an end-of-sequence token, and a following prompt through the ordinary run().
* The device loop against the reference's fixture (tests/golden/llama_tiny*.npz), within the bounds tests/test_llm_flow.py holds the per-call
  path to in its sdpa modes."""
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_decode_pick
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref_argmax(row):
    """src/llm.cpp:355-370: prev = -1.0f; an element is taken when v >= prev"""
    prev, best = f32(-1.0), -1
    for i, v in enumerate(row):
        if v >= prev:          # (False for a NaN)
            prev, best = v, i
    return best


def ref_pick(row, eos, state, ids, pos, tokens):
    """the state advance of osg_decode_pick (include/osgpu.h) on host copies; state = [row, len, n_tokens, stop]"""
    state, ids, pos, tokens = state.copy(), ids.copy(), pos.copy(), tokens.copy()
    if state[3] != 0 or state[2] >= len(tokens):
        return state, ids, pos, tokens
    tok = ref_argmax(row)
    if tok < 0:
        state[3] = 2
    elif eos >= 0 and tok == eos:
        state[3] = 1
    else:
        tokens[state[2]] = tok
        ids[0], pos[0] = tok, state[1]
        state[0], state[1], state[2] = state[1], state[1] + 1, state[2] + 1
    return state, ids, pos, tokens


def pick_rows(V):
    """rows of V logits that exercise the scan: the maximum at either end, duplicates (the LAST wins), exactly -1.0, NaNs, nothing >= -1"""
    rng = np.random.default_rng(V)
    base = rng.standard_normal(V).astype(f32)
    rows = {}
    r = base.copy(); r[0] = 9.0; rows["max_first"] = r
    r = base.copy(); r[V - 1] = 9.0; rows["max_last"] = r
    r = base.copy(); r[[0, V // 3, V // 2, V - 1]] = 7.5; rows["duplicates"] = r
    r = np.full(V, -3.0, f32); r[V // 2] = -1.0; rows["minus_one_counts"] = r
    r = np.full(V, -1.0, f32); rows["all_minus_one"] = r
    r = (-1.5 - np.abs(base)).astype(f32); rows["all_below"] = r
    r = base.copy(); r[::2] = np.nan; r[V - 1] = np.nan; rows["nans"] = r
    r = np.full(V, np.nan, f32); rows["all_nan"] = r
    r = base.copy(); r[V // 2] = 0.0; r[0] = -0.0; r[r > 0] = -0.5; rows["zeros_of_both_signs"] = r
    return rows


@pytest.mark.parametrize("V", [1, 96, 1000, 32003])
def test_decode_pick_equals_the_apps_argmax(gpu, V):
    T = 3
    for name, row in pick_rows(V).items():
        want_tok = ref_argmax(row)
        if name in ("all_below", "all_nan"):
            assert want_tok == -1
        if name == "duplicates" and V > 1:
            assert want_tok == V - 1
        logits = np.full((T, V), 50.0, f32)       # (only the LAST row counts)
        logits[T - 1] = row
        state = np.array([0, 7, 1, 0], np.int32)
        ids, pos, tokens = np.array([-5], np.int64), np.array([-6], np.int64), np.full(4, -7, np.int64)
        for eos in (-1, want_tok):
            d_state, d_ids, d_pos, d_tok = gpu.to_dev(state), gpu.to_dev(ids), gpu.to_dev(pos), gpu.to_dev(tokens)
            gpu.decode_pick(gpu.to_dev(logits), eos, d_state, d_ids, d_pos, d_tok)
            want = ref_pick(row, eos, state, ids, pos, tokens)
            got = (d_state.numpy(), d_ids.numpy(), d_pos.numpy(), d_tok.numpy())
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, eos, got, want)
            if want[0][3] != 0:
                # stopped: further launches, whatever the logits say, change nothing
                gpu.decode_pick(gpu.to_dev(np.full((1, V), 3.0, f32)), -1, d_state, d_ids, d_pos, d_tok)
                again = (d_state.numpy(), d_ids.numpy(), d_pos.numpy(), d_tok.numpy())
                for g, w in zip(again, got):
                    assert g.tobytes() == w.tobytes(), (name, eos)


def test_decode_pick_stops_writing_at_the_token_budget(gpu):
    row = np.arange(96, dtype=f32).reshape(1, 96)
    state = np.array([4, 5, 2, 0], np.int32)
    d_state, d_ids, d_pos, d_tok = gpu.to_dev(state), gpu.to_dev(np.array([1], np.int64)), gpu.to_dev(np.array([4], np.int64)), gpu.to_dev(np.array([8, 9], np.int64))
    gpu.decode_pick(gpu.to_dev(row), -1, d_state, d_ids, d_pos, d_tok)
    assert np.array_equal(d_state.numpy(), state) and d_ids.numpy()[0] == 1 and d_pos.numpy()[0] == 4 and list(d_tok.numpy()) == [8, 9]


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_kv_append_at
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hkv,cap,d", [(2, 192, 16), (3, 5, 128), (1, 1, 8)])
def test_kv_append_at_writes_one_row_per_head(gpu, Hkv, cap, d):
    rng = np.random.default_rng(cap)
    cache = rng.integers(0, 65536, (Hkv, cap, d)).astype(np.uint16)
    src = rng.integers(0, 65536, (Hkv, d)).astype(np.uint16)
    for row in sorted({0, cap // 2, cap - 1}):
        dev = gpu.to_dev(cache)
        gpu.kv_append_at(gpu.to_dev(src), dev, gpu.to_dev(np.array([row, 0, 0, 0], np.int32)))
        want = cache.copy()
        want[:, row, :] = src
        assert np.array_equal(dev.numpy(), want), row
    for row in (-1, cap):      # outside the buffer: nothing is written
        dev = gpu.to_dev(cache)
        gpu.kv_append_at(gpu.to_dev(src), dev, gpu.to_dev(np.array([row, 0, 0, 0], np.int32)))
        assert np.array_equal(dev.numpy(), cache), row


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_sdpa_len
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (4, 2), (2, 2)])
def test_sdpa_len_has_the_bits_of_sdpa_on_compacted_copies(gpu, D, Hq, Hkv):
    CAP = 192
    rng = np.random.default_rng(D * 10 + Hq)
    q = rng.standard_normal((1, Hq, 1, D)).astype(f16)
    k = rng.standard_normal((1, Hkv, CAP, D)).astype(f16)
    v = rng.standard_normal((1, Hkv, CAP, D)).astype(f16)
    mask = (rng.standard_normal(CAP) * 0.5).astype(f16)
    scale = float(f16(1.0 / np.sqrt(D)))
    dq = gpu.to_dev(q)
    for L in (1, 63, 64, 65, 130, CAP):
        ref = gpu.sdpa(dq, gpu.to_dev(k[:, :, :L]), gpu.to_dev(v[:, :, :L]), gpu.to_dev(mask[:L].reshape(1, L)), scale).numpy()
        assert np.isfinite(ref.astype(f32)).all()
        state = gpu.to_dev(np.array([L - 1, L, 0, 0], np.int32))
        got = gpu.sdpa_len(dq, gpu.to_dev(k), gpu.to_dev(v), gpu.to_dev(mask), state, scale).numpy()
        assert got.tobytes() == ref.tobytes(), L
        # rows at and past the length (and the mask there) are never read: NaN bit patterns in them change nothing
        kn, vn, mn = k.copy(), v.copy(), mask.copy()
        kn.view(np.uint16)[:, :, L:] = 0x7E01
        vn.view(np.uint16)[:, :, L:] = 0xFFFF
        mn.view(np.uint16)[L:] = 0x7C01
        got = gpu.sdpa_len(dq, gpu.to_dev(kn), gpu.to_dev(vn), gpu.to_dev(mn), state, scale).numpy()
        assert got.tobytes() == ref.tobytes(), ("nan tail", L)


def test_sdpa_len_refuses_what_it_does_not_implement(gpu):
    from onnxstream_amd.osgpu import OsgError
    q, kv, mask = gpu.to_dev(np.zeros((1, 2, 1, 16), f16)), gpu.to_dev(np.zeros((1, 1, 8, 16), f16)), gpu.to_dev(np.zeros(8, f16))
    state = gpu.to_dev(np.array([0, 1, 0, 0], np.int32))
    with pytest.raises(OsgError, match="osg_sdpa_len: a mask"):
        gpu.sdpa_len(q, kv, kv, None, state, 0.25)
    with pytest.raises(OsgError, match="osg_sdpa_len: .*scale > 0"):
        gpu.sdpa_len(q, kv, kv, mask, state, 0.0)
    with pytest.raises(OsgError, match="osg_sdpa_len: query heads"):
        gpu.sdpa_len(gpu.to_dev(np.zeros((1, 3, 1, 16), f16)), gpu.to_dev(np.zeros((1, 2, 8, 16), f16)), gpu.to_dev(np.zeros((1, 2, 8, 16), f16)), mask, state, 0.25)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
MAX_NEW = 5


def _model(model_dir, cfg, upcast, fusion, graph, resident):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    for k, v in (("hip_autotune", 0), ("hip_fusion_level", fusion), ("hip_use_graph", graph), ("hip_resident_outputs", resident)):
        m._set_option(k, v)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, model_dir, sdpa=True, upcast=upcast)
    return m


def _caches(m, cfg):
    return [m.get_tensor_f16(f"opkv{i}") for i in range(2 * cfg.layers)]       # (fp16 bits, read where they are: host or device)


def _host_loop(m, cfg, prompt, max_new, eos=-1):
    """the specification: src/llm.cpp:472-496 driven from the host, one run() per token"""
    lg = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    P, toks, trace, stop = len(prompt), [], [], 0
    for _ in range(max_new):
        tok = ref_argmax(lg[0, -1])
        if tok < 0:
            stop = 2
            break
        if tok == eos:
            stop = 1
            break
        toks.append(tok)
        lg = llama.forward_resident(m, cfg, [tok], False, P, keep_logits=True)
        trace.append(lg[0, -1].copy())
        P += 1
    return toks, stop, trace, lg


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
    """the host-driven loop, the EOS variant and the follow-up prompt, computed once per (model, upcast, fusion) and shared (hip_use_graph and
    hip_resident_outputs do not change the host flow's bits: tests/test_llm_flow.py, tests/test_planner_cpu.py)"""
    key = (which, upcast, fusion)
    if key not in _host_cache:
        cfg, z = FIX[which]
        prompt, toks_fix = [int(t) for t in z["prompt"]], [int(t) for t in z["tokens"]]
        m = _model(model_dirs[which], cfg, upcast, fusion, 1, 0)
        toks, stop, trace, lg = _host_loop(m, cfg, prompt, MAX_NEW)
        caches = _caches(m, cfg)
        m.drop_tensor("logits")
        follow = llama.forward_resident(m, cfg, [1, 2, 3], False, len(prompt) + len(toks))
        m.close()
        m = _model(model_dirs[which], cfg, upcast, fusion, 1, 0)
        e_toks, e_stop, _, e_lg = _host_loop(m, cfg, prompt, MAX_NEW, eos=toks_fix[2])
        e_caches = _caches(m, cfg)
        m.close()
        _host_cache[key] = dict(toks=toks, stop=stop, trace=trace, lg=lg, caches=caches, follow=follow, e_toks=e_toks, e_stop=e_stop, e_lg=e_lg, e_caches=e_caches)
    return _host_cache[key]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("fusion", [0, 2])
@pytest.mark.parametrize("upcast", [False, True])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_device_loop_equals_the_host_driven_loop(model_dirs, which, upcast, fusion, graph, resident):
    cfg, z = FIX[which]
    prompt, toks_fix = [int(t) for t in z["prompt"]], [int(t) for t in z["tokens"]]
    H = host_flow(model_dirs, which, upcast, fusion)
    assert H["toks"][:len(toks_fix)] == toks_fix and H["stop"] == 0 and len(H["toks"]) == MAX_NEW
    P = len(prompt)
    # ---- MAX_NEW tokens in one call: tokens, every pass's logits, the final logits and caches ----
    m = _model(model_dirs[which], cfg, upcast, fusion, graph, resident)
    llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    built = m.hip_plans_built()
    toks, stop, trace, _ = llama.generate(m, cfg, MAX_NEW, trace=True)
    assert m.hip_plans_built() == built + 1
    assert list(toks) == H["toks"] and stop == 0
    assert trace.shape == (MAX_NEW, cfg.vocab)
    for n in range(MAX_NEW):
        assert bits(trace[n]) == bits(H["trace"][n]), n
    lg = m.get_tensor("logits")[0]
    assert lg.shape == (1, 1, cfg.vocab) and bits(lg) == bits(H["lg"])
    caches = _caches(m, cfg)
    for i, c in enumerate(caches):
        assert c.shape == (1, cfg.kv_heads, P + MAX_NEW, cfg.head_dim) and bits(c) == bits(H["caches"][i]), i
    # ---- the app goes on with its next prompt through the ordinary run() ----
    m.drop_tensor("logits")
    follow = llama.forward_resident(m, cfg, [1, 2, 3], False, P + MAX_NEW)
    assert bits(follow) == bits(H["follow"])
    m.close()
    # ---- an end-of-sequence token: the loop stops where the host loop stops; sync_every 1 (the host ends the call early) and 0 agree ----
    eos = toks_fix[2]
    want_n = toks_fix.index(eos)
    assert H["e_toks"] == toks_fix[:want_n] and H["e_stop"] == 1
    if which == "wide":
        assert want_n == 2          # (llama_tiny's third token repeats its first: there the host loop stops before any pass)
    for sync_every in (1, 0):
        m = _model(model_dirs[which], cfg, upcast, fusion, graph, resident)
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        toks, stop, trace, _ = llama.generate(m, cfg, MAX_NEW, eos_id=eos, sync_every=sync_every, trace=True)
        assert list(toks) == H["e_toks"] and len(toks) == want_n and stop == 1 and trace.shape == (want_n, cfg.vocab)
        assert bits(m.get_tensor("logits")[0]) == bits(H["e_lg"])
        for i, c in enumerate(_caches(m, cfg)):
            assert c.shape == (1, cfg.kv_heads, P + want_n, cfg.head_dim) and bits(c) == bits(H["e_caches"][i]), i
        m.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_second_call_continues_in_the_kept_plan(model_dirs, graph):
    """two calls of 2 and 3 tokens give what one call of 5 gives, and the second builds no plan"""
    cfg, z = FIX["tiny"]
    prompt = [int(t) for t in z["prompt"]]
    H = host_flow(model_dirs, "tiny", True, 2)
    m = _model(model_dirs["tiny"], cfg, True, 2, graph, 1)
    llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    t1, s1, tr1, _ = llama.generate(m, cfg, 2, trace=True)
    built = m.hip_plans_built()
    t2, s2, tr2, _ = llama.generate(m, cfg, 3, trace=True)
    assert m.hip_plans_built() == built
    assert list(t1) + list(t2) == H["toks"] and s1 == 0 and s2 == 0
    for n, row in enumerate(list(tr1) + list(tr2)):
        assert bits(row) == bits(H["trace"][n]), n
    for i, c in enumerate(_caches(m, cfg)):
        assert bits(c) == bits(H["caches"][i]), i
    m.close()


@pytest.mark.parametrize("which,upcast", [("tiny", False), ("tiny", True), ("wide", True)])
def test_device_loop_vs_reference(model_dirs, which, upcast):
    """Against the reference's own run of the flow (the fixture): the tokens are the fixture's greedy tokens followed by the argmax of its last logits;
    the logits of every pass and the caches within the bounds of test_llm_flow.py's sdpa modes (2e-3 of the largest fp32 logit, and within 1e-3 or
    at least as close to the fp32 reference as the reference's own fp16 run + 1e-4; caches 1e-3).  tests/test_generate_cpu.py asserts on the
    fixture that the top-1 to top-2 gap at every step exceeds twice that bound, so the token identity cannot hinge on a near-tie."""
    cfg, z = FIX[which]
    prompt, toks_fix = [int(t) for t in z["prompt"]], [int(t) for t in z["tokens"]]
    tag = "16u" if upcast else "16"
    m = _model(model_dirs[which], cfg, upcast, 2, 1, 0)
    llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    toks, stop, trace, _ = llama.generate(m, cfg, MAX_NEW, trace=True)
    caches = _caches(m, cfg)
    m.close()
    n_ref = len(toks_fix)
    assert list(toks) == toks_fix + [int(np.argmax(z[f"logits{tag}_{n_ref}"][0, -1]))] and stop == 0
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
            err = np.abs(c[:, :, :rows] - z[f"past{tag}_{i}"]).max() / pm
            print(f"cache {i}: {err:.2e}")
            assert err <= 1e-3, (i, err)
