"""The sampling rule of osg_decode_sample (include/osgpu.h, steps 1-6) restated in numpy and Python integers: what tests/test_sample_cpu.py and
tests/test_sample_gpu.py hold the device to.

Everything after the weights is integer arithmetic, so there is exactly one place where the device and this file can differ: w = exp(x) in fp32 is
not correctly rounded on either side, and q = floor(min(w, 1) * 2^32) can differ in its last bits (a few 1e-7 relative).  Two margins say how far a
draw is from where such a difference could change it:
  * the draw's margin: the distance of t from the nearest running-sum boundary BETWEEN two kept tokens, over Q (infinite with one kept token);
  * the top-p margin of the row: the distance of the prefix sum from the threshold on either side of the cut, over Qtot (infinite when top-p is off).
`check` below is the rule the tests apply: a draw with a margin under 2^-16 is ambiguous -- the device's token must then lie in the kept set widened by
one token at the top-p cut --, every other draw must give the restatement's token."""
import math

import numpy as np

f32 = np.float32
MASK32 = 0xFFFFFFFF
AMBIGUOUS = 2.0 ** -16


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", 2011): counter 4 words, key 2 words -> 4 words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def draw_r(seed, n):
    """step 5's 64-bit r for draw index n"""
    seed, n = seed & (2 ** 64 - 1), n & (2 ** 64 - 1)
    out = philox4x32_10((n & MASK32, n >> 32, 0, 0), (seed & MASK32, seed >> 32))
    return out[0] | (out[1] << 32)


def weights_q(values, m, temperature, perturb=None):
    """step 3: q of fp32 `values` against the maximum m; perturb: a relative error per element put on w (a stand-in for another exp)"""
    inv_t = f32(1.0) / f32(temperature)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        w = np.exp((values.astype(f32) - f32(m)) * inv_t).astype(np.float64)
    if perturb is not None:
        w = w * (1.0 + perturb)
    return np.floor(np.minimum(w, 1.0) * 4294967296.0).astype(np.uint64)


class Prepared:
    """steps 1-4 on one row under one rule: everything a draw needs"""

    def __init__(self, row, temperature, top_k=0, top_p=1.0, perturb=None):
        row = np.asarray(row, f32)
        idx = np.flatnonzero(~np.isnan(row))
        order = idx[np.lexsort((-idx, -row[idx].astype(np.float64)))]        # value descending, index descending among equals
        self.stop = len(order) == 0 or bool(np.isinf(row[order[0]]))         # the invalid argmax: stop = 2
        self.topp_margin = math.inf
        if self.stop:
            return
        self.first = int(order[0])
        if top_k > 0:
            order = order[:top_k]
        q = weights_q(row[order], row[self.first], temperature, None if perturb is None else perturb[order])
        order, q = order[q > 0], q[q > 0]
        widened = order
        if f32(top_p) < 1:
            cum = np.cumsum(q, dtype=np.uint64)                              # (exact: below 2^53)
            qtot = int(cum[-1])
            num, den = float(f32(top_p)).as_integer_ratio()                  # the fp32 value, exactly
            thr = max(1, qtot * num // den)
            j = int(np.searchsorted(cum, np.uint64(thr), side="left"))       # the shortest prefix with a sum >= thr
            below = thr - int(cum[j - 1]) if j > 0 else math.inf             # (one token is always kept)
            self.topp_margin = min(below, int(cum[j]) - thr) / qtot
            widened = order[:j + 2]
            order, q = order[:j + 1], q[:j + 1]
        by_index = np.argsort(order)
        self.kept = order[by_index]
        self.cum = np.cumsum(q[by_index], dtype=np.uint64)
        self.Q = int(self.cum[-1])
        self.widened = set(int(i) for i in widened)

    def draw(self, seed, n):
        """step 5: (token, the draw's margin)"""
        t = (draw_r(seed, n) * self.Q) >> 64
        pos = int(np.searchsorted(self.cum, np.uint64(t), side="right"))     # the first running sum that exceeds t
        margin = math.inf
        if pos > 0:
            margin = min(margin, (t - int(self.cum[pos - 1])) / self.Q)
        if pos + 1 < len(self.cum):
            margin = min(margin, (int(self.cum[pos]) - t) / self.Q)
        return int(self.kept[pos]), margin


def sample(row, temperature, top_k, top_p, seed, n):
    """steps 1-5 for one draw: (token or None when the row stops the loop, the draw's margin, the top-p margin)"""
    p = Prepared(row, temperature, top_k, top_p)
    if p.stop:
        return None, math.inf, math.inf
    tok, margin = p.draw(seed, n)
    return tok, margin, p.topp_margin


def advance(tok, eos, state, ids, pos, tokens):
    """step 6 on host copies, state = [row, len, n_tokens, stop]; tok None: the row stops the loop.  The caller has checked that the loop runs."""
    state, ids, pos, tokens = state.copy(), ids.copy(), pos.copy(), tokens.copy()
    if tok is None:
        state[3] = 2
    elif eos >= 0 and tok == eos:
        state[3] = 1
    else:
        tokens[state[2]] = tok
        ids[0], pos[0] = tok, state[1]
        state[0], state[1], state[2] = state[1], state[1] + 1, state[2] + 1
    return state, ids, pos, tokens


def check(prep, seed, n, got):
    """The tests' rule for one draw: returns True when the draw is ambiguous (a margin under 2^-16), and asserts what holds either way."""
    want, margin = prep.draw(seed, n)
    if min(margin, prep.topp_margin) < AMBIGUOUS:
        assert got in prep.widened, (n, got, want, margin, prep.topp_margin)
        return True
    assert got == want, (n, got, want, margin, prep.topp_margin)
    return False
