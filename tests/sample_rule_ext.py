"""Steps 0 and 3b of the sampling rule (include/osgpu.h: repetition, presence and frequency penalties over a count per token, and min-p) restated in
numpy, one operation per rounding, in front of the restatement of steps 1-6 (tests/sample_rule.py): what tests/test_sample_penalties_gpu.py holds
the device to.

Both steps are exact -- fp32 products, sums and one compare, no exp -- so they add no ambiguity of their own: the margins and the 2^-16 threshold of
sample_rule.check stay as they are.  A token that min-p drops is handed to sample_rule.Prepared as a NaN: min-p keeps a prefix of step 1's order, as
top-k does, so dropping its tail before or after top-k is the same set, and the first token (x = 0 >= x_min) always stays."""
import math

import numpy as np

import sample_rule as S

f32 = np.float32


def penalize(row, counts, r=1.0, presence=0.0, frequency=0.0):
    """step 0: the adjusted row a of raw fp32 logits under int counts; a has the bits of the row where the count is 0"""
    row = np.asarray(row, f32)
    counts = np.asarray(counts)
    assert row.shape == counts.shape and (counts >= 0).all() and (counts < 2 ** 24).all()
    r, presence, frequency = f32(r), f32(presence), f32(frequency)
    with np.errstate(all="ignore"):
        inv_r = f32(1.0) / r                                            # once, in fp32
        b = np.where(row > 0, row * inv_r, row * r).astype(f32)          # one fp32 multiply; +-0 and NaN take the second branch
        prod = (frequency * counts.astype(f32)).astype(f32)              # the product rounded ...
        u = (presence + prod).astype(f32)                                # ... then the sum
        a = (b - u).astype(f32)                                          # one rounding
    return np.where(counts > 0, a, row).astype(f32)


def x_min(min_p):
    """step 3b's threshold: the fp32 nearest to the double-precision log of min_p's fp32 value; -inf when min_p = 0"""
    p = float(f32(min_p))
    return f32(-math.inf) if p == 0.0 else f32(math.log(p))


def min_p_drop(a, temperature, min_p):
    """the adjusted row with every token of x < x_min replaced by a NaN (= no token); x = (a - m) * inv_t as step 3 forms it"""
    a = np.asarray(a, f32)
    valid = ~np.isnan(a)
    if f32(min_p) == 0 or not valid.any():
        return a
    m = a[valid].max()                                                   # step 1's first value (which of its equals holds it does not matter here)
    if np.isinf(m):
        return a                                                         # (the row stops the loop: steps 1-6 say so)
    inv_t = f32(1.0) / f32(temperature)
    with np.errstate(all="ignore"):
        x = ((a - m).astype(f32) * inv_t).astype(f32)
        drop = x < x_min(min_p)                                          # (a NaN compares false and is no token anyway)
    out = a.copy()
    out[drop] = np.nan
    return out


def prepared(row, counts, temperature, top_k=0, top_p=1.0, r=1.0, presence=0.0, frequency=0.0, min_p=0.0):
    """steps 0-4 on one raw row under the counts: a sample_rule.Prepared to draw from and to check against"""
    a = penalize(row, counts, r, presence, frequency)
    return S.Prepared(min_p_drop(a, temperature, min_p), temperature, top_k, top_p)


def pick(a):
    """the app's argmax over an (adjusted) row: the scan starts at -1.0f and takes v >= prev -- the last of the equal maxima among the elements >= -1,
    None when nothing qualifies (stop = 2)"""
    a = np.asarray(a, f32)
    ok = np.flatnonzero(a >= f32(-1.0))
    if len(ok) == 0:
        return None
    top = a[ok].max()
    return int(ok[a[ok] == top][-1])


def counts_of(history, tokens, V):
    """c of the rule: occurrences among the history plus the tokens appended so far"""
    both = np.concatenate([np.asarray(history, np.int64).reshape(-1), np.asarray(tokens, np.int64).reshape(-1)])
    return np.bincount(both, minlength=V).astype(np.int64)
