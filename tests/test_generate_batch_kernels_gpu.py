"""The three batch entry points of the device token loop (include/osgpu.h), GPU side:

* osg_decode_sample_batch row by row against the restatement of the rule (tests/sample_rule.py: sample / advance under the ambiguity rule of `check`),
  with guard bands round everything it may write, on batches that mix running, stopped, spent, ending and invalid rows, and against osg_decode_sample
  on the same row with the same seed, which must give the same token;
* osg_kv_append_at_batch against the definition, every other byte of the caches unchanged;
* osg_sdpa_len_batch bit for bit against osg_sdpa on dense copies of each batch's first tkv_b rows, the rows past each length filled with NaN."""
import numpy as np
import pytest

import sample_rule as S

f16, f32 = np.float16, np.float32
pytestmark = pytest.mark.gpu
RULES = [(1.0, 0, 1.0), (0.7, 40, 0.9)]
GUARD = -7777


class Batch:
    """device buffers of n_seq sequences with one guard row before and one after each of them: state, ids, pos, tokens"""

    def __init__(self, gpu, logits, states, max_tokens, seeds, tokens=None):
        self.gpu, self.n, self.V, self.max_tokens = gpu, logits.shape[0], logits.shape[1], max_tokens
        n = self.n
        self.h_state = np.full((n + 2, 4), GUARD, np.int32)
        self.h_state[1:-1] = states
        self.h_ids = np.full(n + 2, GUARD, np.int64)
        self.h_pos = np.full(n + 2, GUARD, np.int64)
        self.h_tok = np.full((n + 2, max(max_tokens, 1)), GUARD, np.int64)
        if tokens is not None:
            self.h_tok[1:-1] = tokens
        self.logits = gpu.to_dev(np.ascontiguousarray(logits, f32))
        self.state, self.ids, self.pos, self.tok = gpu.to_dev(self.h_state), gpu.to_dev(self.h_ids), gpu.to_dev(self.h_pos), gpu.to_dev(self.h_tok)
        self.seeds = gpu.to_dev(np.array([s & (2 ** 64 - 1) for s in seeds], np.uint64))

    def launch(self, rule, eos=-1, draw_base=0):
        g = self.gpu
        g._ck(g.lib.osg_decode_sample_batch(g.ctx, self.logits.ptr, self.V, self.n, int(eos), self.state.ptr + 16, self.ids.ptr + 8, self.pos.ptr + 8,
                                            self.tok.ptr + 8 * self.h_tok.shape[1], self.max_tokens, float(rule[0]), int(rule[1]), float(rule[2]), self.seeds.ptr,
                                            int(draw_base)))

    def read(self):
        """(state [n,4], ids [n], pos [n], tokens [n, max_tokens]) after checking that the guard rows are as they were"""
        st, ids, pos, tok = self.state.numpy(), self.ids.numpy(), self.pos.numpy(), self.tok.numpy()
        for a in (st, tok):
            assert (a[0] == GUARD).all() and (a[-1] == GUARD).all()
        for a in (ids, pos):
            assert a[0] == GUARD and a[-1] == GUARD
        return st[1:-1].copy(), ids[1:-1].copy(), pos[1:-1].copy(), tok[1:-1].copy()


def expect_step(preps, rule, seeds, eos, draw_base, before, after, max_tokens):
    """one launch, row by row: `after` must be what S.advance makes of `before` with the token the restatement draws (an ambiguous draw: with the device's
    own token, which S.check holds to the widened kept set).  Returns the number of ambiguous draws."""
    ambiguous = 0
    for s, prep in enumerate(preps):
        st, ids, pos, tok = (a[s] for a in before)
        got = tuple(a[s] for a in after)
        if st[3] != 0 or st[2] >= max_tokens:
            want = (st, ids, pos, tok)                       # stopped or spent: nothing changes
        elif prep.stop:
            want = S.advance(None, eos, st, ids[None], pos[None], tok)
            want = (want[0], want[1][0], want[2][0], want[3])
        else:
            n = draw_base + int(st[2])
            if got[0][3] == 0:
                dev_tok = int(got[3][st[2]])
            else:
                assert got[0][3] == 1 and eos >= 0
                dev_tok = eos
            ambiguous += S.check(prep, seeds[s], n, dev_tok)
            want = S.advance(dev_tok, eos, st, ids[None], pos[None], tok)
            want = (want[0], want[1][0], want[2][0], want[3])
        for g, w in zip(got, want):
            assert np.array_equal(np.asarray(g), np.asarray(w)), (s, got, want)
    return ambiguous


def rows_for(V, n_seq, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_seq, V)) * 3.0).astype(f32)


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "T%g-k%d-p%g" % r)
@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("V", [1, 65, 4097])
def test_decode_sample_batch_equals_the_restatement_row_by_row(gpu, V, n_seq, rule):
    DRAWS = 16
    logits = rows_for(V, n_seq, V * 10 + n_seq)
    seeds = [0x9E3779B97F4A7C15 + 977 * s for s in range(n_seq)]
    preps = [S.Prepared(logits[s], *rule) for s in range(n_seq)]
    states = np.array([[6 + s, 7 + s, 0, 0] for s in range(n_seq)], np.int32)       # (every sequence at a length of its own)
    b = Batch(gpu, logits, states, DRAWS, seeds)
    ambiguous = 0
    before = b.read()
    for _ in range(DRAWS):
        b.launch(rule, draw_base=5)
        after = b.read()
        ambiguous += expect_step(preps, rule, seeds, -1, 5, before, after, DRAWS)
        before = after
    st = before[0]
    assert st.tolist() == [[7 + s + DRAWS - 1, 7 + s + DRAWS, DRAWS, 0] for s in range(n_seq)]
    print(f"V {V} n_seq {n_seq} rule {rule}: {ambiguous} ambiguous of {DRAWS * n_seq}")
    # one launch more: every row is at its budget, nothing changes
    b.launch(rule, draw_base=5)
    for a, w in zip(b.read(), before):
        assert a.tobytes() == w.tobytes()


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "T%g-k%d-p%g" % r)
@pytest.mark.parametrize("V", [65, 4097])
def test_mixed_batches_every_row_goes_its_own_way(gpu, V, rule):
    """rows: 0 runs; 1 has stopped already (nothing of it may change); 2 is at the token budget; 3 draws the end-of-sequence token (a logit that holds all
    the mass; row 0 and row 5 cannot draw it: a NaN stands there); 4 is all NaN (stop 2); 5 runs"""
    MAXT = 4
    eos = V // 2
    logits = rows_for(V, 6, V + 1)
    logits[0, eos] = np.nan
    logits[5, eos] = np.nan
    logits[3, eos] = 200.0
    logits[4, :] = np.nan
    seeds = [11, 12, 13, 14, 15, 2 ** 64 - 1]
    preps = [S.Prepared(logits[s], *rule) for s in range(6)]
    assert preps[4].stop and not any(preps[s].stop for s in (0, 1, 2, 3, 5)) and preps[3].draw(14, 1)[0] == eos
    states = np.array([[9, 10, 1, 0], [3, 4, 1, 1], [20, 21, MAXT, 0], [30, 31, 1, 0], [40, 41, 2, 0], [-1, 50, 0, 0]], np.int32)
    tokens = np.arange(6 * MAXT, dtype=np.int64).reshape(6, MAXT) + 1000
    b = Batch(gpu, logits, states, MAXT, seeds, tokens)
    before = b.read()
    for step in range(MAXT + 1):
        b.launch(rule, eos=eos)
        after = b.read()
        expect_step(preps, rule, seeds, eos, 0, before, after, MAXT)
        before = after
    st, ids, pos, tok = before
    assert st[1].tolist() == [3, 4, 1, 1] and tok[1].tolist() == tokens[1].tolist()          # the stopped row: as it was
    assert st[2].tolist() == [20, 21, MAXT, 0] and tok[2].tolist() == tokens[2].tolist()      # the spent row: as it was
    assert st[3].tolist() == [30, 31, 1, 1] and tok[3].tolist() == tokens[3].tolist()         # end of sequence at its first draw
    assert st[4].tolist() == [40, 41, 2, 2] and tok[4].tolist() == tokens[4].tolist()         # the invalid row
    assert st[0].tolist() == [9 + MAXT - 1, 10 + MAXT - 1, MAXT, 0] and st[5].tolist() == [50 + MAXT - 1, 50 + MAXT, MAXT, 0]
    assert ids[1] == GUARD and pos[1] == GUARD and ids[3] == GUARD and ids[4] == GUARD and ids[2] == GUARD      # rows that never picked wrote no staging slot
    assert ids[0] == tok[0][MAXT - 1] and pos[0] == 9 + MAXT - 1 and ids[5] == tok[5][MAXT - 1] and pos[5] == 50 + MAXT - 1


@pytest.mark.parametrize("V", [65, 4097])
def test_a_row_draws_what_osg_decode_sample_draws_with_its_seed(gpu, V):
    """same device code, same row, same state, same seed: the same token, wherever the row stands in the batch -- and two rows with equal logits and
    equal seeds draw equal tokens"""
    rule, DRAWS = (0.7, 40, 0.9), 8
    logits = rows_for(V, 3, V + 2)
    logits[2] = logits[0]
    seeds = [0xABCDEF0123, 77, 0xABCDEF0123]
    states = np.array([[4, 5, 0, 0]] * 3, np.int32)
    b = Batch(gpu, logits, states, DRAWS, seeds)
    for _ in range(DRAWS):
        b.launch(rule, draw_base=3)
    st, ids, pos, tok = b.read()
    assert tok[0].tolist() == tok[2].tolist() and st[0].tolist() == st[2].tolist()
    for s in range(3):
        d_lg = gpu.to_dev(logits[s:s + 1])
        d_state, d_ids, d_pos, d_tok = gpu.to_dev(states[s]), gpu.to_dev(np.array([-5], np.int64)), gpu.to_dev(np.array([-6], np.int64)), gpu.to_dev(np.full(DRAWS, -7, np.int64))
        for _ in range(DRAWS):
            gpu.decode_sample(d_lg, -1, d_state, d_ids, d_pos, d_tok, *rule, seeds[s], 3)
        assert d_tok.numpy().tolist() == tok[s].tolist(), s
        assert d_state.numpy().tolist() == st[s].tolist() and d_ids.numpy()[0] == ids[s] and d_pos.numpy()[0] == pos[s]


def test_decode_sample_batch_refuses_what_the_single_launch_refuses(gpu):
    from onnxstream_amd.osgpu import OsgError
    b = Batch(gpu, np.zeros((2, 8), f32), np.array([[0, 1, 0, 0]] * 2, np.int32), 2, [1, 2])
    for rule, msg in (((0.0, 0, 1.0), "temperature"), ((1.0, -1, 1.0), "top_k"), ((1.0, 0, 0.0), "top_p"), ((1.0, 0, 1.5), "top_p")):
        with pytest.raises(OsgError, match="osg_decode_sample_batch: .*" + msg):
            b.launch(rule)


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_kv_append_at_batch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Hkv", [1, 4])
def test_kv_append_at_batch_writes_each_batch_at_its_own_row(gpu, Hkv, d):
    B, cap = 3, 128
    rng = np.random.default_rng(Hkv * 1000 + d)
    cache = rng.integers(0, 65536, (B, Hkv, cap, d)).astype(np.uint16)
    src = rng.integers(0, 65536, (B, Hkv, d)).astype(np.uint16)
    for rows in ((0, 127, 64), (5, -1, 6), (cap, 3, cap - 1), (-1, cap, cap + 7)):
        state = np.full((B, 4), 99, np.int32)
        state[:, 0] = rows
        dev = gpu.to_dev(cache)
        gpu.kv_append_at_batch(gpu.to_dev(src), dev, gpu.to_dev(state))
        want = cache.copy()
        for b, r in enumerate(rows):
            if 0 <= r < cap:
                want[b, :, r, :] = src[b]
        assert dev.numpy().tobytes() == want.tobytes(), rows


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_sdpa_len_batch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (2, 1, 128), (8, 4, 64)])
def test_sdpa_len_batch_has_the_bits_of_sdpa_on_dense_copies(gpu, Hq, Hkv, D):
    B, CAP = 3, 128
    rng = np.random.default_rng(D * 10 + Hq)
    q = rng.standard_normal((B, Hq, 1, D)).astype(f16)
    k = rng.standard_normal((B, Hkv, CAP, D)).astype(f16)
    v = rng.standard_normal((B, Hkv, CAP, D)).astype(f16)
    mask = (rng.standard_normal(CAP) * 0.5).astype(f16)
    scale = float(f16(1.0 / np.sqrt(D)))
    for lens in ((1, 64, 65), (128, 2, 63)):
        ref = np.zeros((B, Hq, 1, D), f16)
        kn, vn = k.copy(), v.copy()
        for b, L in enumerate(lens):
            ref[b] = gpu.sdpa(gpu.to_dev(q[b:b + 1]), gpu.to_dev(k[b:b + 1, :, :L]), gpu.to_dev(v[b:b + 1, :, :L]), gpu.to_dev(mask[:L].reshape(1, L)), scale).numpy()[0]
            kn.view(np.uint16)[b, :, L:] = 0x7E01          # rows at and past the length of THIS batch: NaN bit patterns, so any read of them shows
            vn.view(np.uint16)[b, :, L:] = 0xFFFF
        assert np.isfinite(ref.astype(f32)).all()
        state = np.zeros((B, 4), np.int32)
        state[:, 0] = [L - 1 for L in lens]
        state[:, 1] = lens
        state[:, 2:] = 12345                               # (not lengths: the stride over the states must be the one asked for)
        got = gpu.sdpa_len_batch(gpu.to_dev(q), gpu.to_dev(kn), gpu.to_dev(vn), gpu.to_dev(mask), gpu.to_dev(state), scale).numpy()
        for b in range(B):
            assert got[b].tobytes() == ref[b].tobytes(), (lens, b)
        # batch b alone through osg_sdpa_len: the same bits again
        for b, L in enumerate(lens):
            one = gpu.sdpa_len(gpu.to_dev(q[b:b + 1]), gpu.to_dev(kn[b:b + 1]), gpu.to_dev(vn[b:b + 1]), gpu.to_dev(mask), gpu.to_dev(state[b]), scale).numpy()
            assert one[0].tobytes() == got[b].tobytes(), (lens, b)
    # lengths outside [1, cap] are clamped into it
    state = np.zeros((B, 4), np.int32)
    state[:, 1] = [0, -5, CAP + 9]
    got = gpu.sdpa_len_batch(gpu.to_dev(q), gpu.to_dev(k), gpu.to_dev(v), gpu.to_dev(mask), gpu.to_dev(state), scale).numpy()
    for b, L in enumerate((1, 1, CAP)):
        ref = gpu.sdpa(gpu.to_dev(q[b:b + 1]), gpu.to_dev(k[b:b + 1, :, :L]), gpu.to_dev(v[b:b + 1, :, :L]), gpu.to_dev(mask[:L].reshape(1, L)), scale).numpy()[0]
        assert got[b].tobytes() == ref.tobytes(), b


def test_sdpa_len_batch_refuses_what_it_does_not_implement(gpu):
    from onnxstream_amd.osgpu import OsgError
    q, kv, mask = gpu.to_dev(np.zeros((2, 2, 1, 16), f16)), gpu.to_dev(np.zeros((2, 1, 8, 16), f16)), gpu.to_dev(np.zeros(8, f16))
    state = gpu.to_dev(np.array([[0, 1, 0, 0]] * 2, np.int32))
    with pytest.raises(OsgError, match="osg_sdpa_len_batch: a mask"):
        gpu.sdpa_len_batch(q, kv, kv, None, state, 0.25)
    with pytest.raises(OsgError, match="osg_sdpa_len_batch: .*scale > 0"):
        gpu.sdpa_len_batch(q, kv, kv, mask, state, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# osg_rope_batch (the rotary step of a batched pass: every sequence at a position of its own)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,T,d", [(3, 4, 1, 16), (5, 2, 1, 128), (2, 3, 2, 64)])
def test_rope_batch_is_rope_per_batch(gpu, B, H, T, d):
    rng = np.random.default_rng(B * 100 + d)
    x = rng.standard_normal((B, H, T, d)).astype(f16)
    cos, sin = rng.uniform(-1, 1, (B, T, d)).astype(f16), rng.uniform(-1, 1, (B, T, d)).astype(f16)
    got = gpu.rope_batch(gpu.to_dev(x), gpu.to_dev(cos), gpu.to_dev(sin)).numpy()
    for b in range(B):
        one = gpu.rope(gpu.to_dev(x[b]), gpu.to_dev(cos[b]), gpu.to_dev(sin[b])).numpy()
        assert got[b].tobytes() == one.tobytes(), b
