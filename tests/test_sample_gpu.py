"""Sampling in the device token loop, GPU side: osg_decode_sample against the restatement of its rule (tests/sample_rule.py, include/osgpu.h) draw by
draw, on random rows at every size at which the kernel's work is laid out differently and on rows built to hit the rule's edges; the launches that must
stop or do nothing; repeatability; and the loop itself (model_hip_generate_sampled) on the two Llama fixtures, each step checked against the logits the
device had at that step, and the passes against the host-driven run() loop fed the device's tokens.

The device's fp32 exp is the one place where kernel and restatement may differ (last bits of q).  A draw whose margin (sample_rule.check) is under
2^-16 is ambiguous: the device's token must then lie in the restatement's kept set, widened by one token at the top-p cut; every other draw must be
equal.  At most 5 % of a case's draws may be ambiguous -- a condition on the case, which depends on the restatement alone, never on the device."""
import os
import tempfile

import numpy as np
import pytest

import sample_rule as S
from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
pytestmark = pytest.mark.gpu
RULES = [(0.8, 40, 0.9), (1.0, 0, 0.9), (1.5, 0, 1.0), (0.7, 1000, 0.5)]
DRAWS = 64
CAP = 0.05


def run_draws(gpu, row, rule, seed, n_draws, eos=-1, draw_base=0, n0=0, extra_rows=2):
    """n_draws launches over one row (the LAST of 1 + extra_rows), the state advancing as the loop's would: (tokens, state, ids, pos)"""
    T, top_k, top_p = rule
    logits = np.full((1 + extra_rows, len(row)), 50.0, f32)
    logits[-1] = row
    d_lg = gpu.to_dev(logits)
    d_state = gpu.to_dev(np.array([6, 7, n0, 0], np.int32))
    d_ids, d_pos, d_tok = gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(n0 + n_draws, -7, np.int64))
    for _ in range(n_draws):
        gpu.decode_sample(d_lg, eos, d_state, d_ids, d_pos, d_tok, T, top_k, top_p, seed, draw_base)
    return d_tok.numpy(), d_state.numpy(), d_ids.numpy(), d_pos.numpy()


def check_draws(prep, seed, got, base=0):
    """every draw under the ambiguity rule; the case must keep to the cap"""
    ambiguous = sum(S.check(prep, seed, base + n, int(t)) for n, t in enumerate(got))
    assert ambiguous <= CAP * len(got), f"{ambiguous} of {len(got)} draws are ambiguous: choose another seed for this case"
    return ambiguous


def ambiguous_count(prep, seed, draws=DRAWS):
    """how many of a case's draws the restatement calls ambiguous: a property of row, rule and seed, not of the device"""
    return sum(min(prep.draw(seed, n)[1], prep.topp_margin) < S.AMBIGUOUS for n in range(draws))


def random_row(V, rule, seed):
    """N(0, 3^2) logits and the first of four seeds at which the case keeps to the cap.  Where no seed can -- a wide rule over a large vocabulary puts
    much of its mass on tokens lighter than 2^-16, each an ambiguous draw by definition, whatever the seed -- the row is drawn more peaked, sigma 5,
    then 8.  Decided by the restatement alone; returns (row, prep, seed, sigma).  test_flat_rows_outside_the_cap runs the sigma 3 rows given up here."""
    z = np.random.default_rng(V).standard_normal(V)
    for sigma in (3.0, 5.0, 8.0):
        row = (z * sigma).astype(f32)
        prep = S.Prepared(row, *rule)
        for s in range(4):
            if ambiguous_count(prep, seed + s) <= CAP * DRAWS:
                return row, prep, seed + s, sigma
    return row, prep, seed, sigma          # (the test then fails on the cap)


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "T%g-k%d-p%g" % r)
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1024, 1025, 4097, 32000, 128256])
def test_decode_sample_equals_the_restatement(gpu, V, rule):
    row, prep, seed, sigma = random_row(V, rule, 0x9E3779B97F4A7C15 ^ V)
    toks, state, ids, pos = run_draws(gpu, row, rule, seed, DRAWS)
    ambiguous = check_draws(prep, seed, toks)
    print(f"V {V} rule {rule}: sigma {sigma:g}, seed {seed:#x}, kept {len(prep.kept)}, top-p margin {prep.topp_margin:.3g}, {ambiguous} ambiguous of {DRAWS}")
    assert list(state) == [7 + DRAWS - 1, 7 + DRAWS, DRAWS, 0] and ids[0] == toks[-1] and pos[0] == 7 + DRAWS - 1


@pytest.mark.parametrize("rule", [(1.0, 0, 0.9), (1.5, 0, 1.0)], ids=lambda r: "T%g-k%d-p%g" % r)
@pytest.mark.parametrize("V", [32000, 128256])
def test_flat_rows_outside_the_cap(gpu, V, rule):
    """The N(0, 3^2) rows that random_row had to give up: thousands of kept tokens, most of them lighter than 2^-16, so no seed keeps the case to the
    cap and it cannot stand among the capped cases.  Run IN ADDITION to them, under the same rule draw by draw -- an unambiguous draw must be equal, an
    ambiguous one must lie in the (widened) kept set -- and without the cap, which these rows cannot meet; the count is printed."""
    seed = 0x51A7 + V
    row = (np.random.default_rng(V).standard_normal(V) * 3.0).astype(f32)
    prep = S.Prepared(row, *rule)
    assert len(prep.kept) > 1000
    toks = run_draws(gpu, row, rule, seed, DRAWS)[0]
    ambiguous = sum(S.check(prep, seed, n, int(t)) for n, t in enumerate(toks))
    print(f"V {V} rule {rule}: sigma 3, kept {len(prep.kept)}, top-p margin {prep.topp_margin:.3g}, {ambiguous} ambiguous of {DRAWS}")


@pytest.mark.parametrize("V,extra_rows,head", [(1, 1, 1), (2, 1, 2), (3, 1, 1), (3, 3, 3), (5, 1, 3), (7, 1, 1), (1025, 1, 3), (4099, 1, 1), (4098, 1, 2)])
def test_rows_that_start_off_a_16_byte_boundary(gpu, V, extra_rows, head):
    """The kernel reads the row with 16-byte loads from its first aligned element on; the 0-3 tokens before it (`head`) go their own way through every
    pass and through the draw.  The row is the last of 1 + extra_rows, so it starts extra_rows * V elements into a 16-byte-aligned buffer: every head
    of 1, 2 and 3 tokens, a head that is the whole row, and heads that carry enough mass to be drawn."""
    assert min(V, (-(extra_rows * V)) % 4) == head
    row = (np.random.default_rng(V + extra_rows).standard_normal(V) * 2).astype(f32)
    n_heavy = min(V, 6)
    row[:n_heavy] = 8.0 + 0.01 * np.arange(n_heavy, dtype=f32)          # the first six tokens are heavy: the head is drawn, and so is what follows it
    for rule in ((1.0, 0, 1.0), (0.8, 40, 0.9), (1.0, 2, 1.0)):
        prep = S.Prepared(row, *rule)
        seed = next((0xA11C + V + k for k in range(4) if ambiguous_count(prep, 0xA11C + V + k, 48) <= CAP * 48), 0xA11C + V)
        toks = run_draws(gpu, row, rule, seed, 48, extra_rows=extra_rows)[0]
        ambiguous = check_draws(prep, seed, toks)
        in_head = sum(int(t) < head for t in toks)
        print(f"V {V} head {head} rule {rule}: kept {len(prep.kept)}, {in_head} of 48 draws in the head, {ambiguous} ambiguous")
        if V > head and rule[1] == 0:
            assert 0 < in_head < 48


# ---------------------------------------------------------------------------------------------------------------------------------------
# rows built to hit the edges
# ---------------------------------------------------------------------------------------------------------------------------------------
VE = 2500          # (three passes of the 1024 threads over the row, twelve of the sixteen index ranges of the draw in use)


def edge_cases():
    rng = np.random.default_rng(2500)
    base = rng.standard_normal(VE).astype(f32)
    cases = {}
    cases["all_equal_topk"] = (np.full(VE, 1.25, f32), (1.0, 5, 1.0))
    cases["all_equal_topp"] = (np.full(VE, -3.0, f32), (0.5, 0, 0.0102))          # 25.5 of 2500 equal masses: 26 tokens
    r = base.copy()
    big = rng.permutation(VE)[:45]
    r[big[:35]] = 4.0 + np.arange(35, dtype=f32) * 0.25             # 35 distinct leaders ...
    r[big[35:]] = 3.5                                               # ... and ten equals across the k = 40 boundary: the five largest indices stay
    cases["ties_across_k"] = (r, (2.0, 40, 1.0))
    r = np.full(VE, -30.0, f32)
    r[rng.permutation(VE)[:8]] = 5.0                                # eight equals carry all the mass: 0.45 of it is 3.6 tokens, so the four largest indices
    cases["ties_across_p"] = (r, (1.0, 0, 0.45))
    r = base.copy()
    r[rng.permutation(VE)[:12]] = 2.75                              # both cuts inside one run of equals: top-k takes 7 of the 12, top-p fewer
    r[r > 2.75] = 2.0
    cases["ties_across_k_and_p"] = (r, (0.25, 7, 0.6))
    r = base.copy()
    r[::7] = np.nan
    r[int(np.nanargmax(base))] = np.nan
    cases["nan_scattered_and_at_the_maximum"] = (r, (1.0, 0, 0.95))
    r = base.copy()
    r[::5] = -np.inf
    cases["minus_inf"] = (r, (1.0, 0, 1.0))
    r = base.copy()
    r[1777] = 100.0
    cases["one_dominant"] = (r, (1.0, 0, 1.0))
    cases["top_k_equals_V"] = (base * 2, (1.0, VE, 1.0))
    cases["top_k_beyond_V"] = (base * 2, (1.0, VE + 100, 0.9))
    cases["below_minus_one"] = (base - 20.0, (1.0, 50, 1.0))
    r = base.copy()
    r[[3, 900]] = 0.0
    r[[4, 2400]] = -0.0
    r[r > 0] = -0.5
    cases["zeros_of_both_signs"] = (r, (0.05, 2, 1.0))
    return cases


@pytest.mark.parametrize("name", list(edge_cases()))
def test_decode_sample_on_edge_rows(gpu, name):
    row, rule = edge_cases()[name]
    seed, draws = 0xC0FFEE, 40
    prep = S.Prepared(row, *rule)
    toks, state, _, _ = run_draws(gpu, row, rule, seed, draws)
    assert state[2] == draws and state[3] == 0
    kept = [int(i) for i in prep.kept]
    if name == "all_equal_topk":
        assert kept == list(range(VE - 5, VE))
    if name == "all_equal_topp":
        assert kept == list(range(VE - 26, VE))
    if name == "ties_across_k":
        ties = np.flatnonzero(row == f32(3.5))
        assert len(kept) == 40 and sorted(set(kept) & set(ties)) == sorted(ties)[-5:]
    if name == "ties_across_p":
        assert kept == sorted(np.flatnonzero(row == f32(5.0)))[-4:]
    if name == "ties_across_k_and_p":
        ties = sorted(np.flatnonzero(row == f32(2.75)))
        assert 1 <= len(kept) < 7 and kept == ties[-len(kept):]
    if name == "one_dominant":
        assert kept == [1777]
    if name in ("top_k_equals_V", "top_k_beyond_V"):
        assert kept == [int(i) for i in S.Prepared(row, rule[0], 0, rule[2]).kept]
    if name == "zeros_of_both_signs":
        assert kept == [900, 2400]
    if name == "minus_inf":
        assert not np.isinf(row[kept]).any()
    check_draws(prep, seed, toks)
    assert set(int(t) for t in toks) <= prep.widened
    if len(kept) > 1:
        assert len(set(int(t) for t in toks)) > 1          # (a draw, not a pick)


@pytest.mark.parametrize("V", [1, 700, 4097])
def test_top_k_one_is_the_first_token_of_the_order(gpu, V):
    """whatever the temperature, top_p and seed: the largest value, among equals the largest index; no margin is allowed"""
    rng = np.random.default_rng(V)
    row = rng.standard_normal(V).astype(f32)
    row[::11] = np.nan
    row[rng.permutation(V)[:3]] = 6.5          # three equal maxima
    first = S.Prepared(row, 1.0).first
    assert first == max(i for i in range(V) if row[i] == row[first])
    for T, top_p, seed in ((0.01, 1.0, 1), (1.0, 0.3, 2), (50.0, 1.0, 2 ** 64 - 1), (3e38, 1e-30, 12345)):
        toks, state, _, _ = run_draws(gpu, row, (T, 1, top_p), seed, 6)
        assert list(toks) == [first] * 6 and state[2] == 6, (T, top_p, seed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# launches that stop, or do nothing
# ---------------------------------------------------------------------------------------------------------------------------------------
def _launch(gpu, row, state, eos=-1, rule=(1.0, 0, 1.0), seed=3):
    ids, pos, tokens = np.array([-5], np.int64), np.array([-6], np.int64), np.full(4, -7, np.int64)
    d = [gpu.to_dev(np.asarray(state, np.int32)), gpu.to_dev(ids), gpu.to_dev(pos), gpu.to_dev(tokens)]
    gpu.decode_sample(gpu.to_dev(np.asarray(row, f32).reshape(1, -1)), eos, d[0], d[1], d[2], d[3], rule[0], rule[1], rule[2], seed, 0)
    return d, (ids, pos, tokens)


@pytest.mark.parametrize("V", [1, 96, 3000])
def test_rows_that_stop(gpu, V):
    rng = np.random.default_rng(V)
    base = rng.standard_normal(V).astype(f32)
    inf_row = base.copy()
    inf_row[V // 2] = np.inf
    nan_and_minus_inf = np.full(V, np.nan, f32)
    nan_and_minus_inf[::2] = -np.inf
    for name, row in (("all_nan", np.full(V, np.nan, f32)), ("plus_inf", inf_row), ("nothing_finite", nan_and_minus_inf)):
        for rule in ((1.0, 0, 1.0), (0.8, 40, 0.9)):
            d, host = _launch(gpu, row, [0, 7, 1, 0], rule=rule)
            assert list(d[0].numpy()) == [0, 7, 1, 2], (name, rule)
            for dev, h in zip(d[1:], host):
                assert np.array_equal(dev.numpy(), h), (name, rule)
            # stopped: a further launch over a good row changes nothing
            gpu.decode_sample(gpu.to_dev(base.reshape(1, V)), -1, d[0], d[1], d[2], d[3], 1.0, 0, 1.0, 3, 0)
            assert list(d[0].numpy()) == [0, 7, 1, 2] and all(np.array_equal(dev.numpy(), h) for dev, h in zip(d[1:], host))
    # the end-of-sequence token drawn: stop = 1, nothing else written
    row = base.copy()
    row[V // 3] = 90.0
    d, host = _launch(gpu, row, [0, 7, 1, 0], eos=V // 3)
    assert list(d[0].numpy()) == [0, 7, 1, 1] and all(np.array_equal(dev.numpy(), h) for dev, h in zip(d[1:], host))
    # ... and another eos_id lets it through, as the restatement's state advance says
    d, host = _launch(gpu, row, [0, 7, 1, 0], eos=V // 3 + 1)
    want = S.advance(V // 3, V // 3 + 1, np.array([0, 7, 1, 0], np.int32), *host)
    for dev, w in zip(d, want):
        assert np.array_equal(dev.numpy(), w)


def test_decode_sample_stops_writing_at_the_token_budget(gpu):
    row = np.arange(96, dtype=f32)
    for state in ([4, 5, 4, 0], [4, 5, 9, 0], [4, 5, 2, 1], [4, 5, 2, 2]):          # the budget (tokens has 4 slots) spent or exceeded; stopped
        d, host = _launch(gpu, row, state)
        assert list(d[0].numpy()) == state and all(np.array_equal(dev.numpy(), h) for dev, h in zip(d[1:], host)), state


def test_decode_sample_refuses_invalid_arguments(gpu):
    from onnxstream_amd.osgpu import OsgError
    row = np.zeros(8, f32)
    for rule, msg in (((0.0, 0, 1.0), "temperature"), ((-1.0, 0, 1.0), "temperature"), ((float("nan"), 0, 1.0), "temperature"),
                      ((float("inf"), 0, 1.0), "temperature"), ((1e-42, 0, 1.0), "temperature"), ((1.0, -1, 1.0), "top_k must be >= 0"),
                      ((1.0, 0, 0.0), "top_p must be in"), ((1.0, 0, 1.5), "top_p must be in"), ((1.0, 0, float("nan")), "top_p must be in")):
        with pytest.raises(OsgError, match="osg_decode_sample: .*" + msg):
            _launch(gpu, row, [0, 7, 0, 0], rule=rule)


# ---------------------------------------------------------------------------------------------------------------------------------------
# repeatability and seeds
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_same_arguments_same_bits(gpu):
    row = (np.random.default_rng(5).standard_normal(50000) * 3).astype(f32)
    rule = (0.9, 300, 0.97)
    a = run_draws(gpu, row, rule, 77, 32)
    b = run_draws(gpu, row, rule, 77, 32)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_seeds_and_draw_base(gpu):
    row = np.zeros(4096, f32)          # flat: 4096 tokens of q = 2^32 each
    rule = (1.0, 0, 1.0)
    a = run_draws(gpu, row, rule, 1, 32)[0]
    b = run_draws(gpu, row, rule, 2, 32)[0]
    assert (a != b).any() and len(set(a)) > 16
    prep = S.Prepared(row, *rule)
    assert list(a) == [prep.draw(1, n)[0] for n in range(32)]          # (equal masses of 2^32: nothing here depends on exp)
    # draw_base = b at n_tokens = 0 is draw_base = 0 at n_tokens = b
    for base in (1, 7, 31):
        assert run_draws(gpu, row, rule, 1, 1, draw_base=base)[0][0] == a[base]
        assert run_draws(gpu, row, rule, 1, 1, n0=base)[0][base] == a[base]
    # the draw index is 64 bits wide, and wraps
    hi = run_draws(gpu, row, rule, 1, 2, draw_base=2 ** 64 - 1)[0]
    assert list(hi) == [prep.draw(1, 2 ** 64 - 1)[0], a[0]]
    assert run_draws(gpu, row, rule, 1 << 40, 1, draw_base=1 << 33)[0][0] == prep.draw(1 << 40, 1 << 33)[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
FIX = {"tiny": (llama.TINY, np.load(os.path.join(HERE, "golden", "llama_tiny.npz"))),
       "wide": (llama.TINY_WIDE, np.load(os.path.join(HERE, "golden", "llama_tiny_wide.npz")))}
LOOP_RULE = dict(temperature=0.8, top_k=40, top_p=0.9, seed=0xDECADE)
N_NEW = 8


@pytest.fixture(scope="module")
def model_dirs():
    with tempfile.TemporaryDirectory() as d:
        dirs = {}
        for name, (cfg, _) in FIX.items():
            dirs[name] = os.path.join(d, name) + "/"
            os.makedirs(dirs[name])
            llama.build_llama(DirSink(dirs[name]), cfg)
        yield dirs


def _model(model_dir, cfg, graph):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    for k, v in (("hip_autotune", 0), ("hip_fusion_level", 2), ("hip_use_graph", graph), ("hip_resident_outputs", 1)):
        m._set_option(k, v)
    m.add_outputs_convert("logits")
    llama.configure(m, cfg, model_dir, sdpa=True, upcast=True)
    return m


def _caches(m, cfg):
    return [m.get_tensor_f16(f"opkv{i}") for i in range(2 * cfg.layers)]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_sampled_device_loop(model_dirs, which, graph):
    cfg, z = FIX[which]
    prompt = [int(t) for t in z["prompt"]]
    P = len(prompt)
    rule = (LOOP_RULE["temperature"], LOOP_RULE["top_k"], LOOP_RULE["top_p"])
    # ---- N_NEW sampled tokens in one call; every step against the logits the device had at that step ----
    m = _model(model_dirs[which], cfg, graph)
    lg0 = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)[0, -1].copy()
    greedy_plan = None
    toks, stop, trace, _ = llama.generate(m, cfg, N_NEW, trace=True, **LOOP_RULE)
    assert stop == 0 and len(toks) == N_NEW and trace.shape == (N_NEW, cfg.vocab)
    ambiguous = 0
    for n in range(N_NEW):
        prep = S.Prepared(lg0 if n == 0 else trace[n - 1], *rule)
        ambiguous += S.check(prep, LOOP_RULE["seed"], n, int(toks[n]))
    assert ambiguous <= CAP * N_NEW, f"{ambiguous} ambiguous draws: choose another seed"
    assert len(set(int(t) for t in toks)) > 1
    lg_end, caches = m.get_tensor("logits")[0], _caches(m, cfg)
    sampled_plan = m.hip_decode_plan_info()
    m.close()
    # ---- the passes: the device's tokens one by one through the host-driven run() loop ----
    m = _model(model_dirs[which], cfg, graph)
    lg = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    assert bits(lg[0, -1]) == bits(lg0)
    for n, tok in enumerate(toks):
        lg = llama.forward_resident(m, cfg, [int(tok)], False, P + n, keep_logits=True)
        assert bits(lg[0, -1]) == bits(trace[n]), n
    assert lg.shape == (1, 1, cfg.vocab) and bits(lg) == bits(lg_end)
    for i, c in enumerate(_caches(m, cfg)):
        assert c.shape == (1, cfg.kv_heads, P + N_NEW, cfg.head_dim) and bits(c) == bits(caches[i]), i
    m.close()
    # ---- one call of N_NEW = a call of 4, then a call of 4 with draw_base = 4 ----
    m = _model(model_dirs[which], cfg, graph)
    llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
    t1, s1, tr1, _ = llama.generate(m, cfg, 4, trace=True, **LOOP_RULE)
    built = m.hip_plans_built()
    t2, s2, tr2, _ = llama.generate(m, cfg, N_NEW - 4, trace=True, draw_base=4, **LOOP_RULE)
    assert m.hip_plans_built() == built and s1 == 0 and s2 == 0
    assert list(t1) + list(t2) == list(toks) and bits(np.concatenate([tr1, tr2])) == bits(trace)
    assert bits(m.get_tensor("logits")[0]) == bits(lg_end)
    for i, c in enumerate(_caches(m, cfg)):
        assert bits(c) == bits(caches[i]), i
    m.close()
    # ---- temperature = 0 is the greedy call: tokens, trace, caches, and the same plan text as the sampled call's ----
    out = []
    for kw in ({}, dict(temperature=0.0, top_k=3, top_p=0.5, seed=9, draw_base=2)):
        m = _model(model_dirs[which], cfg, graph)
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        g_toks, g_stop, g_trace, _ = llama.generate(m, cfg, 5, trace=True, **kw)
        out.append((bits(g_toks), g_stop, bits(g_trace), bits(m.get_tensor("logits")[0]), [bits(c) for c in _caches(m, cfg)]))
        greedy_plan = m.hip_decode_plan_info()
        m.close()
    assert out[0] == out[1]
    assert [int(t) for t in np.frombuffer(out[0][0], np.int64)][:len(z["tokens"])] == [int(t) for t in z["tokens"]]
    assert greedy_plan == sampled_plan
