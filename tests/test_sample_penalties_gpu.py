"""Repetition, presence and frequency penalties and min-p in the device token loop, GPU side: osg_decode_count, osg_decode_penalize and the three _ext
entry points against the restatement of steps 0 and 3b (tests/sample_rule_ext.py, include/osgpu.h) in front of the restatement of steps 1-6
(tests/sample_rule.py); the identity of the _ext entry points with the old ones; the launches that must leave the counts alone; and the three loops
(model_hip_generate_sampled_ext, model_hip_generate_batch_ext, model_hip_turn_ext) on the two Llama fixtures.

Steps 0 and 3b are exact, so osg_decode_penalize is held to the restatement bit for bit and min-p adds no margin: the ambiguity rule of sample_rule.check
and its 2^-16 threshold stand as they are, and at most 5 % of a case's draws may be ambiguous -- a condition on the case, decided by the restatement
alone.  Where a draw is ambiguous the device may take the neighbouring token, so the counts of every later draw are rebuilt from the DEVICE's tokens."""
import numpy as np
import pytest

import sample_rule as S
import sample_rule_ext as X
from onnxstream_amd.synth import llama
from test_sample_gpu import FIX, RULES, _caches, _model, bits, model_dirs  # noqa: F401  (model_dirs: the module-scoped fixture of the two Llama fixtures)

f32 = np.float32
pytestmark = pytest.mark.gpu
PENALTIES = [(1.3, 0.0, 0.0), (1.0, 0.5, 0.25), (1.1, 0.2, 0.1)]          # (repetition, presence, frequency)
MIN_PS = [0.0, 0.05]
DRAWS = 64
CAP = 0.05


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_decode_penalize and osg_decode_count
# ---------------------------------------------------------------------------------------------------------------------------------------
def same_bits(got, want, counts):
    """bit for bit; where a count is > 0 and the restatement gives a NaN, any NaN (the payload of a NaN that went through arithmetic is not the rule's)"""
    got, want = np.asarray(got, f32).reshape(-1), np.asarray(want, f32).reshape(-1)
    eq = got.view(np.uint32) == want.view(np.uint32)
    nan_ok = np.isnan(got) & np.isnan(want) & (np.asarray(counts).reshape(-1) > 0)
    return bool((eq | nan_ok).all())


def penalize_case(gpu, rows, counts, extra_rows, pen):
    """rows [n_seq, V] as rows extra_rows .. of a logits buffer, counts [n_seq, V]: the device's adjusted rows against the restatement's"""
    n_seq, V = rows.shape
    logits = np.full((extra_rows + n_seq, V), 50.0, f32)
    logits[extra_rows:] = rows
    out = gpu.decode_penalize(gpu.to_dev(logits), gpu.to_dev(counts.astype(np.int32)), *pen, row=extra_rows, n_seq=n_seq).numpy()
    for s in range(n_seq):
        want = X.penalize(rows[s], counts[s], *pen)
        assert same_bits(out[s], want, counts[s]), (V, extra_rows, pen, s, np.flatnonzero(out[s].view(np.uint32) != want.view(np.uint32))[:8])
    assert bits(out[counts == 0]) == bits(rows[counts == 0])          # (a count of 0: the logit's own bits, a NaN's included)


@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("V", [1, 3, 63, 65, 1025, 4099])
def test_decode_penalize_equals_the_restatement(gpu, V, n_seq):
    """random rows, counts of 0, 1 and 70 000 mixed and different per sequence; extra_rows 0-3 puts the first row at every offset from a 16-byte boundary
    that V allows (an odd V: all four), and the rows of the other sequences, of the counts and of the output at offsets of their own"""
    rng = np.random.default_rng(100 * V + n_seq)
    for extra_rows in range(4):
        rows = (rng.standard_normal((n_seq, V)) * 4).astype(f32)
        counts = rng.choice(np.array([0, 0, 1, 1, 2, 70000]), size=(n_seq, V))
        for pen in PENALTIES + [(0.5, -0.75, -0.125), (1.0, 0.0, 0.0)]:
            penalize_case(gpu, rows, counts, extra_rows, pen)


@pytest.mark.parametrize("frequency", [0.25, -0.25])
@pytest.mark.parametrize("r", [0.5, 1.3])
def test_decode_penalize_on_an_edge_row(gpu, r, frequency):
    """+-0, +-inf, NaN, the largest finite values and subnormals, each under a count of 0, 1 and 70 000"""
    tiny, big = np.finfo(f32).smallest_subnormal, np.finfo(f32).max
    edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, big, -big, tiny, -tiny, f32(1e-39), f32(-1e-39), np.finfo(f32).tiny, 1.0, -1.0, 17500.0, -17500.0], f32)
    rows = np.tile(edge, 3).reshape(1, -1)
    counts = np.repeat(np.array([0, 1, 70000]), len(edge)).reshape(1, -1)
    for extra_rows in (0, 1):
        for presence in (0.0, 0.5, -3.0):
            penalize_case(gpu, rows, counts, extra_rows, (r, presence, frequency))
    a = X.penalize(rows[0], counts[0], r, 0.5, frequency)
    assert np.isnan(a[4::len(edge)]).all() and np.isposinf(a[2::len(edge)]).all() and np.isneginf(a[3::len(edge)]).all()


def test_decode_count(gpu):
    V = 1000
    rng = np.random.default_rng(7)
    toks = rng.integers(0, V, 5000).astype(np.int64)
    toks[:700] = 3                                                      # one token many times over: the atomics add up
    toks[700:720] = [-1, V, V + 5, -2 ** 40, 2 ** 40] * 4                # outside [0, V): ignored
    inside = toks[(toks >= 0) & (toks < V)]
    start = rng.integers(0, 9, V).astype(np.int32)
    d_cnt = gpu.to_dev(start)
    gpu.decode_count(gpu.to_dev(toks), d_cnt)
    assert np.array_equal(d_cnt.numpy(), start + np.bincount(inside, minlength=V))
    gpu.decode_count(gpu.to_dev(toks), d_cnt, n=0)                       # n = 0: nothing
    gpu.decode_count(gpu.to_dev(np.zeros(0, np.int64)), d_cnt)
    assert np.array_equal(d_cnt.numpy(), start + np.bincount(inside, minlength=V))
    gpu.decode_count(gpu.to_dev(toks), d_cnt, n=650)                     # a prefix
    assert np.array_equal(d_cnt.numpy(), start + np.bincount(inside, minlength=V) + np.bincount(toks[:650], minlength=V))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the _ext pick and sample, draw by draw with the counts advancing
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_ext(gpu, row, rule, pen, min_p, seed, n_draws, history, eos=-1, extra_rows=2, greedy=False):
    """n_draws x (osg_decode_penalize + the _ext pick or sample) over one raw row, the counts starting from the history: (tokens, state, ids, pos, counts)"""
    V = len(row)
    logits = np.full((1 + extra_rows, V), 50.0, f32)
    logits[-1] = row
    d_lg, d_adj = gpu.to_dev(logits), gpu.empty((1, V), np.float32)
    d_cnt = gpu.to_dev(np.zeros(V, np.int32))
    gpu.decode_count(gpu.to_dev(np.asarray(history, np.int64)), d_cnt)
    d_state = gpu.to_dev(np.array([6, 7, 0, 0], np.int32))
    d_ids, d_pos, d_tok = gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(n_draws, -7, np.int64))
    for _ in range(n_draws):
        gpu.decode_penalize(d_lg, d_cnt, *pen, row=extra_rows, out=d_adj)
        if greedy:
            gpu.decode_pick_ext(d_adj, eos, d_state, d_ids, d_pos, d_tok, d_cnt)
        else:
            gpu.decode_sample_ext(d_adj, eos, d_state, d_ids, d_pos, d_tok, rule[0], rule[1], rule[2], seed, 0, min_p, d_cnt)
    return d_tok.numpy(), d_state.numpy(), d_ids.numpy(), d_pos.numpy(), d_cnt.numpy()


def simulate(row, rule, pen, min_p, seed, history, draws=DRAWS):
    """the restatement's own sequence of draws, the counts advancing with ITS tokens: (tokens, how many draws it calls ambiguous); it gives a seed up
    (fewer tokens than draws) as soon as the case is past the cap"""
    counts = X.counts_of(history, [], len(row))
    toks, ambiguous = [], 0
    for n in range(draws):
        prep = X.prepared(row, counts, *rule, *pen, min_p)
        if prep.stop:
            break
        tok, margin = prep.draw(seed, n)
        ambiguous += min(margin, prep.topp_margin) < S.AMBIGUOUS
        if ambiguous > CAP * draws:
            break
        toks.append(tok)
        counts[tok] += 1
    return toks, ambiguous


def random_case(V, rule, pen, min_p, seed):
    """as test_sample_gpu.random_row: N(0, sigma^2) logits with sigma 3, then 5, then 8, and the first of four seeds at which the case keeps to the cap;
    the history holds the row's four largest tokens, so the penalty reorders the top.  Decided by the restatement alone."""
    z = np.random.default_rng(V).standard_normal(V)
    for sigma in (3.0, 5.0, 8.0):
        row = (z * sigma).astype(f32)
        history = [int(i) for i in np.argsort(row, kind="stable")[-4:]]
        for s in range(4):
            toks, ambiguous = simulate(row, rule, pen, min_p, seed + s, history)
            if len(toks) == DRAWS and ambiguous <= CAP * DRAWS:
                return row, history, seed + s, sigma
    return row, history, seed, sigma          # (the test then fails on the cap)


def check_path(row, rule, pen, min_p, seed, history, got):
    """every device token under the ambiguity rule, the counts rebuilt from the history and the device's earlier tokens: (ambiguous draws, final counts)"""
    counts = X.counts_of(history, [], len(row))
    ambiguous = 0
    for n, t in enumerate(got):
        prep = X.prepared(row, counts, *rule, *pen, min_p)
        assert not prep.stop
        ambiguous += S.check(prep, seed, n, int(t))
        counts[int(t)] += 1
    assert ambiguous <= CAP * len(got), f"{ambiguous} of {len(got)} draws are ambiguous: choose another seed for this case"
    return ambiguous, counts


@pytest.mark.parametrize("min_p", MIN_PS, ids=lambda p: "minp%g" % p)
@pytest.mark.parametrize("pen", PENALTIES, ids=lambda p: "r%g-pr%g-fr%g" % p)
@pytest.mark.parametrize("rule", RULES, ids=lambda r: "T%g-k%d-p%g" % r)
@pytest.mark.parametrize("V", [1, 65, 1025, 4097, 32000])
def test_decode_sample_ext_equals_the_restatement(gpu, V, rule, pen, min_p):
    row, history, seed, sigma = random_case(V, rule, pen, min_p, 0x9E3779B97F4A7C15 ^ V)
    toks, state, ids, pos, counts = run_ext(gpu, row, rule, pen, min_p, seed, DRAWS, history)
    assert list(state) == [7 + DRAWS - 1, 7 + DRAWS, DRAWS, 0] and ids[0] == toks[-1] and pos[0] == 7 + DRAWS - 1
    ambiguous, want_counts = check_path(row, rule, pen, min_p, seed, history, toks)
    print(f"V {V} rule {rule} penalties {pen} min_p {min_p}: sigma {sigma:g}, seed {seed:#x}, {len(set(toks.tolist()))} distinct tokens, {ambiguous} ambiguous of {DRAWS}")
    assert np.array_equal(counts, want_counts)


@pytest.mark.parametrize("pen", PENALTIES, ids=lambda p: "r%g-pr%g-fr%g" % p)
@pytest.mark.parametrize("V", [1, 65, 1025, 4097, 32000])
def test_decode_pick_ext_equals_the_restatement(gpu, V, pen):
    """greedy with penalties: the app's argmax over the adjusted row, pick by pick; where the adjusted maximum falls under -1 the loop stops with 2"""
    row = (np.random.default_rng(V).standard_normal(V) * 3.0).astype(f32)
    history = [int(i) for i in np.argsort(row, kind="stable")[-4:]]
    toks, state, ids, pos, counts = run_ext(gpu, row, None, pen, 0.0, 0, DRAWS, history, greedy=True)
    want_counts = X.counts_of(history, [], V)
    want = []
    for _ in range(DRAWS):
        t = X.pick(X.penalize(row, want_counts, *pen))
        if t is None:
            break
        want.append(t)
        want_counts[t] += 1
    n = len(want)
    assert list(toks[:n]) == want and (toks[n:] == -7).all()
    assert list(state) == ([7 + n - 1, 7 + n, n, 0 if n == DRAWS else 2] if n else [6, 7, 0, 2])
    assert np.array_equal(counts, want_counts)
    print(f"V {V} penalties {pen}: {n} picks, {len(set(want))} distinct tokens, stop {state[3]}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact cases: no ambiguity rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_top_k_one_under_a_large_presence_penalty_never_repeats(gpu):
    V, draws = 64, 32
    row = np.random.default_rng(64).standard_normal(V).astype(f32)
    pen = (1.0, 100.0, 0.0)
    for T, top_p, seed in ((1.0, 1.0, 1), (0.3, 0.5, 2 ** 64 - 1)):
        toks, state, _, _, counts = run_ext(gpu, row, (T, 1, top_p), pen, 0.0, seed, draws, [])
        assert len(set(toks.tolist())) == draws and state[2] == draws
        c = np.zeros(V, np.int64)
        for t in toks:
            assert int(t) == X.prepared(row, c, T, 1, top_p, *pen).first          # the first of the order over the adjusted row: no margin is allowed
            c[int(t)] += 1
        assert list(toks) == [int(i) for i in np.argsort(-row.astype(np.float64), kind="stable")[:draws]]          # (distinct values: the raw order)
        assert np.array_equal(counts, c)


def test_greedy_ext_stops_where_the_adjusted_maximum_falls_below_minus_one(gpu):
    row = np.full(65, -5.0, f32)
    row[7], row[9], row[64] = 0.5, 0.4, 0.4          # 9 and 64 are equal: the LAST of equal maxima wins
    toks, state, ids, pos, counts = run_ext(gpu, row, None, (1.0, 2.0, 0.0), 0.0, 0, 6, [], greedy=True)
    assert list(toks) == [7, 64, 9, -7, -7, -7] and list(state) == [9, 10, 3, 2] and ids[0] == 9 and pos[0] == 9
    assert np.array_equal(counts, np.bincount([7, 64, 9], minlength=65))
    # the repetition penalty alone: a positive logit is divided, a negative one multiplied, a zero stays
    row = np.array([-0.75, 0.0, 3.0, 2.0, -0.6], f32)
    toks, state, _, _, _ = run_ext(gpu, row, None, (2.0, 0.0, 0.0), 0.0, 0, 4, [0, 4], greedy=True)
    assert list(toks) == [2, 3, 2, 2] and state[3] == 0          # 3.0, then 2.0 > 1.5, then 1.5 > 1.0; -0.75 * 2 and -0.6 * 2 are out of the scan
    toks, state, _, _, _ = run_ext(gpu, row[[0, 1, 4]], None, (2.0, 0.0, 0.0), 0.0, 0, 3, [1], greedy=True)
    assert list(toks) == [1, 1, 1]                                # 0 * r = 0: still the maximum


def test_min_p_one_keeps_exactly_the_tokens_equal_to_the_maximum(gpu):
    V = 3000
    row = np.random.default_rng(3).standard_normal(V).astype(f32)
    top = [11, 1500, 2999]
    row[top] = 5.0
    row[12] = np.nextafter(f32(5.0), f32(0.0))          # one ulp under the maximum: dropped
    prep = S.Prepared(X.min_p_drop(row, 0.7, 1.0), 0.7)
    assert [int(i) for i in prep.kept] == top
    logits = gpu.to_dev(row.reshape(1, V))
    d_state = gpu.to_dev(np.array([6, 7, 0, 0], np.int32))
    d_ids, d_pos, d_tok = gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(48, -7, np.int64))
    for _ in range(48):
        gpu.decode_sample_ext(logits, -1, d_state, d_ids, d_pos, d_tok, 0.7, 0, 1.0, 99, 0, 1.0, None)
    toks = d_tok.numpy()
    assert list(toks) == [prep.draw(99, n)[0] for n in range(48)]          # (three masses of exactly 2^32: nothing here depends on exp)
    assert set(toks.tolist()) == set(top)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the old path
# ---------------------------------------------------------------------------------------------------------------------------------------
def _operands(gpu, n_tok, n_seq=1):
    state = np.tile(np.array([6, 7, 0, 0], np.int32), n_seq)
    return [gpu.to_dev(state), gpu.to_dev(np.full(n_seq, -5, np.int64)), gpu.to_dev(np.full(n_seq, -6, np.int64)), gpu.to_dev(np.full((n_seq, n_tok), -7, np.int64))]


def _read(ops):
    return [bits(o.numpy()) for o in ops]


@pytest.mark.parametrize("V", [65, 4097, 32000])
def test_ext_without_controls_is_the_old_entry_point(gpu, V):
    rng = np.random.default_rng(V + 1)
    row = (rng.standard_normal(V) * 3).astype(f32)
    lg = gpu.to_dev(np.stack([np.full(V, 50.0, f32), row]))
    n = 24
    for rule in RULES:
        old, new, cnt = _operands(gpu, n), _operands(gpu, n), _operands(gpu, n)
        d_cnt = gpu.to_dev(np.zeros(V, np.int32))
        for _ in range(n):
            gpu.decode_sample(lg, -1, old[0], old[1], old[2], old[3].view(0, (n,)), *rule, 5, 3)
            gpu.decode_sample_ext(lg, -1, new[0], new[1], new[2], new[3].view(0, (n,)), *rule, 5, 3, 0.0, None)
            gpu.decode_sample_ext(lg, -1, cnt[0], cnt[1], cnt[2], cnt[3].view(0, (n,)), *rule, 5, 3, 0.0, d_cnt)
        assert _read(old) == _read(new) == _read(cnt), rule          # tokens, state, staging: bit for bit
        assert np.array_equal(d_cnt.numpy(), np.bincount(old[3].numpy().reshape(-1), minlength=V))
    # the pick
    old, new, cnt = _operands(gpu, 3), _operands(gpu, 3), _operands(gpu, 3)
    d_cnt = gpu.to_dev(np.zeros(V, np.int32))
    for _ in range(3):
        gpu.decode_pick(lg, -1, old[0], old[1], old[2], old[3].view(0, (3,)))
        gpu.decode_pick_ext(lg, -1, new[0], new[1], new[2], new[3].view(0, (3,)), None)
        gpu.decode_pick_ext(lg, -1, cnt[0], cnt[1], cnt[2], cnt[3].view(0, (3,)), d_cnt)
    assert _read(old) == _read(new) == _read(cnt) and list(old[3].numpy()[0]) == [int(np.argmax(row))] * 3
    assert np.array_equal(d_cnt.numpy(), 3 * np.bincount([int(np.argmax(row))], minlength=V))
    # the batch form: three sequences
    rows = gpu.to_dev((rng.standard_normal((3, V)) * 3).astype(f32))
    seeds = gpu.to_dev(np.array([1, 2 ** 64 - 1, 77], np.uint64))
    old, new, cnt = _operands(gpu, n, 3), _operands(gpu, n, 3), _operands(gpu, n, 3)
    d_cnt = gpu.to_dev(np.zeros((3, V), np.int32))
    for _ in range(n):
        gpu.decode_sample_batch(rows, -1, *old, seeds, 0.8, 40, 0.9, 2)
        gpu.decode_sample_batch_ext(rows, -1, *new, seeds, 0.8, 40, 0.9, 2, 0.0, None)
        gpu.decode_sample_batch_ext(rows, -1, *cnt, seeds, 0.8, 40, 0.9, 2, 0.0, d_cnt)
    assert _read(old) == _read(new) == _read(cnt)
    toks = old[3].numpy()
    assert np.array_equal(d_cnt.numpy(), np.stack([np.bincount(toks[s], minlength=V) for s in range(3)]))


def test_batch_ext_sequence_is_the_single_ext_call(gpu):
    """n_seq = 3 over an odd V (every row, count row and output row at another offset from a 16-byte boundary), different counts per sequence: sequence s
    is osg_decode_penalize + osg_decode_sample_ext over its row, its counts and its seed"""
    V, n = 1025, 32
    rng = np.random.default_rng(1025)
    rows = (rng.standard_normal((3, V)) * 4).astype(f32)
    start = rng.choice(np.array([0, 0, 0, 1, 3]), size=(3, V)).astype(np.int32)
    seeds = [5, 2 ** 63, 12345]
    pen, rule, min_p = (1.1, 0.2, 0.1), (0.8, 40, 0.9), 0.05
    lg, d_cnt, d_adj = gpu.to_dev(rows), gpu.to_dev(start), gpu.empty((3, V), np.float32)
    ops = _operands(gpu, n, 3)
    d_seeds = gpu.to_dev(np.array(seeds, np.uint64))
    for _ in range(n):
        gpu.decode_penalize(lg, d_cnt, *pen, n_seq=3, out=d_adj)
        gpu.decode_sample_batch_ext(d_adj, -1, *ops, d_seeds, *rule, 0, min_p, d_cnt)
    toks, counts = ops[3].numpy(), d_cnt.numpy()
    for s in range(3):
        one, c1, a1 = _operands(gpu, n), gpu.to_dev(start[s]), gpu.empty((1, V), np.float32)
        for _ in range(n):
            gpu.decode_penalize(lg, c1, *pen, row=s, out=a1)
            gpu.decode_sample_ext(a1, -1, one[0], one[1], one[2], one[3].view(0, (n,)), *rule, seeds[s], 0, min_p, c1)
        assert bits(one[3].numpy()[0]) == bits(toks[s]) and bits(c1.numpy()) == bits(counts[s]), s
        assert np.array_equal(counts[s], start[s] + np.bincount(toks[s], minlength=V))
    assert len({tuple(t) for t in toks.tolist()}) == 3


def test_launches_that_append_nothing_change_no_count(gpu):
    V = 96
    good = np.arange(V, dtype=f32)
    start = (np.arange(V) % 5).astype(np.int32)
    cases = [("stopped by eos", good, [4, 5, 2, 1], -1), ("stopped as invalid", good, [4, 5, 2, 2], -1), ("budget spent", good, [4, 5, 4, 0], -1),
             ("budget exceeded", good, [4, 5, 9, 0], -1), ("eos drawn", np.where(np.arange(V) == 40, 90.0, -90.0).astype(f32), [4, 5, 1, 0], 40),
             ("invalid row", np.full(V, np.nan, f32), [4, 5, 1, 0], -1), ("infinite top", np.where(np.arange(V) == 3, np.inf, 0.0).astype(f32), [4, 5, 1, 0], -1)]
    for name, row, state, eos in cases:
        for greedy in (False, True):
            if greedy and name == "infinite top":
                continue          # (the argmax takes +inf: no invalid row for the pick)
            if greedy and name == "invalid row":
                row = np.full(V, -2.0, f32)          # nothing >= -1: the pick's invalid argmax
            d_cnt = gpu.to_dev(start)
            ops = [gpu.to_dev(np.asarray(state, np.int32)), gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(4, -7, np.int64))]
            lg = gpu.to_dev(row.reshape(1, V))
            if greedy:
                gpu.decode_pick_ext(lg, eos, *ops, d_cnt)
            else:
                gpu.decode_sample_ext(lg, eos, *ops, 1.0, 0, 1.0, 3, 0, 0.0, d_cnt)
            assert np.array_equal(d_cnt.numpy(), start), (name, greedy)
            assert ops[0].numpy()[2] == state[2] and (ops[3].numpy() == -7).all(), (name, greedy)
            assert ops[0].numpy()[3] == (state[3] or (1 if name == "eos drawn" else 2 if name in ("invalid row", "infinite top") else 0)), (name, greedy)
    # ... and one that appends does
    d_cnt = gpu.to_dev(start)
    ops = [gpu.to_dev(np.array([4, 5, 1, 0], np.int32)), gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(4, -7, np.int64))]
    gpu.decode_pick_ext(gpu.to_dev(good.reshape(1, V)), -1, *ops, d_cnt)
    assert np.array_equal(d_cnt.numpy(), start + np.bincount([V - 1], minlength=V)) and ops[3].numpy()[1] == V - 1


def test_ext_entry_points_refuse_an_invalid_min_p(gpu):
    from onnxstream_amd.osgpu import OsgError
    ops = _operands(gpu, 4)
    lg = gpu.to_dev(np.zeros((1, 8), f32))
    for min_p in (-0.1, 1.5, float("nan")):
        with pytest.raises(OsgError, match=r"osg_decode_sample: min_p must be in \[0, 1\]"):
            gpu.decode_sample_ext(lg, -1, ops[0], ops[1], ops[2], ops[3].view(0, (4,)), 1.0, 0, 1.0, 0, 0, min_p, None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loops
# ---------------------------------------------------------------------------------------------------------------------------------------
LOOP_RULE = dict(temperature=0.8, top_k=40, top_p=0.9, seed=0xDECADE)
LOOP_EXT = dict(repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=0.1, min_p=0.05)
N_NEW = 8


def _check_loop(lg0, trace, toks, history, seed, draw_base=0, ext=LOOP_EXT):
    """every token of a sampled loop against the restatement over that step's RAW traced logits and the counts rebuilt from history and earlier tokens"""
    rule = (LOOP_RULE["temperature"], LOOP_RULE["top_k"], LOOP_RULE["top_p"])
    pen = (ext["repetition_penalty"], ext["presence_penalty"], ext["frequency_penalty"])
    counts = X.counts_of(history, [], len(lg0))
    ambiguous = 0
    for n, t in enumerate(toks):
        prep = X.prepared(lg0 if n == 0 else trace[n - 1], counts, *rule, *pen, ext["min_p"])
        ambiguous += S.check(prep, seed, draw_base + n, int(t))
        counts[int(t)] += 1
    assert ambiguous <= CAP * len(toks), f"{ambiguous} ambiguous draws: choose another seed"


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_generate_with_history_and_penalties(model_dirs, which, graph):
    cfg, z = FIX[which]
    prompt = [int(t) for t in z["prompt"]]
    history = prompt + prompt[:2]
    out = []
    for sync_every in (0, 1):
        m = _model(model_dirs[which], cfg, graph)
        lg0 = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)[0, -1].copy()
        plain = None
        if sync_every == 0:          # the controls change neither the decode plan's text nor its key: a plain call first, then the _ext call on its plan
            llama.generate(m, cfg, 1, **LOOP_RULE)
            plain = m.hip_decode_plan_info()
            m.close()
            m = _model(model_dirs[which], cfg, graph)
            llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        toks, stop, trace, _ = llama.generate(m, cfg, N_NEW, trace=True, sync_every=sync_every, history=history, **LOOP_RULE, **LOOP_EXT)
        assert stop == 0 and len(toks) == N_NEW and trace.shape == (N_NEW, cfg.vocab)
        if plain is not None:
            assert m.hip_decode_plan_info() == plain
            _check_loop(lg0, trace, toks, history, LOOP_RULE["seed"])
        out.append((bits(toks), bits(trace), bits(m.get_tensor("logits")[0]), [bits(c) for c in _caches(m, cfg)]))
        if sync_every == 1:
            # the trace is the model's: the passes through the host-driven run() loop fed the device's tokens give the same rows
            m2 = _model(model_dirs[which], cfg, graph)
            llama.forward_resident(m2, cfg, prompt, True, 0, keep_logits=True)
            for n, tok in enumerate(toks):
                lg = llama.forward_resident(m2, cfg, [int(tok)], False, len(prompt) + n, keep_logits=True)
                assert bits(lg[0, -1]) == bits(trace[n]), n
            m2.close()
            # a call of 4 and a call of 4 with draw_base = 4 and the first four tokens added to the history: the same eight tokens
            m3 = _model(model_dirs[which], cfg, graph)
            llama.forward_resident(m3, cfg, prompt, True, 0, keep_logits=True)
            t1 = llama.generate(m3, cfg, 4, history=history, **LOOP_RULE, **LOOP_EXT)[0]
            t2 = llama.generate(m3, cfg, N_NEW - 4, history=history + [int(t) for t in t1], draw_base=4, **LOOP_RULE, **LOOP_EXT)[0]
            assert list(t1) + list(t2) == list(toks)
            m3.close()
        m.close()
    assert out[0] == out[1]
    # ---- greedy with penalties: the app's argmax over the adjusted logits of every step ----
    m = _model(model_dirs[which], cfg, graph)
    lg0 = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)[0, -1].copy()
    pen = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25)
    toks, stop, trace, _ = llama.generate(m, cfg, N_NEW, trace=True, history=history, **pen)
    counts = X.counts_of(history, [], cfg.vocab)
    for n in range(N_NEW):
        want = X.pick(X.penalize(lg0 if n == 0 else trace[n - 1], counts, 1.3, 0.5, 0.25))
        if want is None:
            assert stop == 2 and len(toks) == n
            break
        assert int(toks[n]) == want, n
        counts[want] += 1
    else:
        assert stop == 0 and len(toks) == N_NEW
    m.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_generate_batch_sequence_is_the_single_call(model_dirs, which, graph):
    cfg, z = FIX[which]
    prompt = [int(t) for t in z["prompt"]]
    seeds = [0x1234, 2 ** 63 + 5, 99]
    rule = {k: v for k, v in LOOP_RULE.items() if k != "seed"}
    m = _model(model_dirs[which], cfg, graph)
    lg0 = llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)[0, -1].copy()
    toks, stop, trace, _ = llama.generate_batch(m, cfg, 3, N_NEW, trace=True, seeds=seeds, draw_base=7, history=prompt, **rule, **LOOP_EXT)
    m.close()
    assert list(stop) == [0, 0, 0] and len({tuple(t.tolist()) for t in toks}) > 1
    for s in range(3):
        m = _model(model_dirs[which], cfg, graph)
        llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
        t1, s1, tr1, _ = llama.generate(m, cfg, N_NEW, trace=True, seed=seeds[s], draw_base=7, history=prompt, **rule, **LOOP_EXT)
        m.close()
        assert s1 == 0 and list(t1) == list(toks[s]) and trace[s].shape == tr1.shape == (N_NEW, cfg.vocab), s
        for n in range(N_NEW):
            assert bits(trace[s][n]) == bits(tr1[n]), (s, n)
        _check_loop(lg0, trace[s], toks[s], prompt, seeds[s], draw_base=7)


@pytest.mark.parametrize("chunk", [8, 16])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_turn_counts_its_prompt(model_dirs, which, graph, chunk):
    """history=None is the prompt for a turn: the turn equals the host-driven chunked flow (the prompt's pieces through run()) followed by generate with
    history = the prompt -- tokens, trace, logits and caches bit for bit"""
    cfg, _ = FIX[which]
    prompt = [int(t) for t in np.random.default_rng(16).integers(1, cfg.vocab, 16)]
    m = _model(model_dirs[which], cfg, graph)
    for at in range(0, 16, chunk):
        llama.forward_resident(m, cfg, prompt[at:at + chunk], at == 0, at, keep_logits=at + chunk == 16)
    want = llama.generate(m, cfg, N_NEW, trace=True, history=prompt, **LOOP_RULE, **LOOP_EXT)
    w_lg, w_caches = m.get_tensor("logits")[0], _caches(m, cfg)
    m.close()
    m = _model(model_dirs[which], cfg, graph)
    llama.forward_resident(m, cfg, [1], True, 0)          # (a run() must have happened; its tensors are dropped: the conversation starts empty)
    m.clear_tensors()
    got = llama.turn(m, cfg, prompt, N_NEW, chunk=chunk, trace=True, first=True, **LOOP_RULE, **LOOP_EXT)
    assert len(want[0]) == N_NEW and list(got[0]) == list(want[0]) and got[1] == want[1] and bits(got[2]) == bits(want[2])
    assert bits(m.get_tensor("logits")[0]) == bits(w_lg)
    for i, c in enumerate(_caches(m, cfg)):
        assert bits(c) == bits(w_caches[i]), i
    # another history than the prompt gives other tokens here, and an explicit history equal to the prompt the same ones
    m.close()
    m = _model(model_dirs[which], cfg, graph)
    llama.forward_resident(m, cfg, [1], True, 0)
    m.clear_tensors()
    again = llama.turn(m, cfg, prompt, N_NEW, chunk=chunk, trace=True, first=True, history=list(prompt), **LOOP_RULE, **LOOP_EXT)
    assert list(again[0]) == list(want[0]) and bits(again[2]) == bits(want[2])
    m.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_ext_exports_with_all_controls_off_are_the_old_exports(model_dirs, which, graph):
    """history=[] takes the call through the _ext export with every control at its default: the bits of the export without the suffix"""
    cfg, z = FIX[which]
    prompt = [int(t) for t in z["prompt"]]

    def once(kind, **kw):
        m = _model(model_dirs[which], cfg, graph)
        if kind == "turn":
            llama.forward_resident(m, cfg, [1], True, 0)
            m.clear_tensors()
            r = llama.turn(m, cfg, prompt, 5, chunk=8, trace=True, first=True, **kw)
        else:
            llama.forward_resident(m, cfg, prompt, True, 0, keep_logits=True)
            r = (llama.generate_batch if kind == "batch" else llama.generate)(m, cfg, *([2] if kind == "batch" else []), 5, trace=True, **kw)
        if kind == "batch":
            res = ([bits(t) for t in r[0]], bits(r[1]), [bits(t) for t in r[2]])
        else:
            res = (bits(r[0]), r[1], bits(r[2]), bits(m.get_tensor("logits")[0]), [bits(c) for c in _caches(m, cfg)])
        m.close()
        return res

    for kind, kw in (("generate", LOOP_RULE), ("generate", {}), ("turn", LOOP_RULE), ("turn", {}), ("batch", dict(temperature=0.8, top_k=40, top_p=0.9, seeds=[3, 4]))):
        assert once(kind, **kw) == once(kind, history=[], **kw), (kind, kw)
