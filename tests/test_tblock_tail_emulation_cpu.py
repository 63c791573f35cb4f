"""CPU: the per-element bounds and FAR caps of tests/test_tblock_tail_float64.py hold for numpy emulations of the arithmetic osg_tblock_tail declares, over
the inputs of every case of that module with M <= 128: f32 accumulation for the contractions, ln_rows' split of a row over 4 / 8 lanes for the LayerNorms,
f16 probabilities against an f32 row sum of the unrounded exponentials for the cross-attention, osg_gelu_erf's polynomial on f32 for the GEGLU.  A bound that
the declared arithmetic alone can exceed would fail here, without a GPU.  Each stage is emulated from the emulation's own previous stage, as the device test
checks each stage against the device's own dump."""
import numpy as np

import test_tblock_tail_float64 as m

f16, f32, f64 = np.float16, np.float32, np.float64


def emu_contraction(a, w, bias=None, res=None):
    acc = a.astype(f32) @ w.astype(f32).T
    acc = acc + (bias.astype(f32) if bias is not None else f32(0))
    acc = acc + (res.astype(f32) if res is not None else f32(0))
    return acc.astype(f16)


def lane_split_sum(v, lpr):
    """[M, C] f32 -> [M, 1]: lane `part` of a row adds its chunks part + lpr i (8 values each) in order, then the xor butterfly over the lpr lanes"""
    M, C = v.shape
    per = C // 8 // lpr
    lanes = v.reshape(M, per, lpr, 8).transpose(0, 2, 1, 3).reshape(M, lpr, per * 8)
    s = np.cumsum(lanes, axis=2, dtype=f32)[:, :, -1]
    step = 1
    while step < lpr:
        s = (s + s[:, np.arange(lpr) ^ step]).astype(f32)
        step *= 2
    return s[:, :1]


def emu_ln(x, gam, bet, eps, rows):
    lpr = 4 if rows == 64 else 8
    v = x.astype(f32)
    mean = (lane_split_sum(v, lpr) / f32(v.shape[1])).astype(f32)
    d = (v - mean).astype(f32)
    var = (lane_split_sum((d * d).astype(f32), lpr) / f32(v.shape[1])).astype(f32)
    rstd = (f32(1) / np.sqrt((var + f32(eps)).astype(f32), dtype=f32)).astype(f32)
    return ((((d * rstd).astype(f32) * gam.astype(f32)).astype(f32)) + bet.astype(f32)).astype(f32).astype(f16)


def emu_attention(q, k, v, scale, imgs):
    M = q.shape[0]
    c = f32(f32(scale) * f32(m.LOG2E))
    qh, kh, vh = m.heads_of(q, imgs), m.heads_of(k, imgs), m.heads_of(v, imgs)
    out = np.empty(qh.shape, f16)
    for b in range(imgs):
        for h in range(m.HEADS):
            t = ((qh[b, h].astype(f32) @ kh[b, h].astype(f32).T).astype(f32) * c).astype(f32)
            e = np.exp2((t - t.max(axis=1, keepdims=True)).astype(f32).astype(f64)).astype(f32)
            l = e.sum(axis=1, dtype=f32)
            o = e.astype(f16).astype(f32) @ vh[b, h].astype(f32)
            out[b, h] = (o * (f32(1) / l)[:, None]).astype(f32).astype(f16)
    return out.transpose(0, 2, 1, 3).reshape(M, m.C)


def emu_gelu(g):
    """osg_gelu_erf (osg_common.h) on f32: Abramowitz-Stegun 7.1.26"""
    xs = (g * f32(0.70710678118654752440)).astype(f32)
    ax = np.abs(xs)
    t = (f32(1) / (f32(0.3275911) * ax + f32(1)).astype(f32)).astype(f32)
    poly = ((((f32(1.061405429) * t - f32(1.453152027)) * t + f32(1.421413741)) * t - f32(0.284496736)) * t + f32(0.254829592)) * t
    e = np.exp2(((ax * ax).astype(f32) * f32(-1.44269504088896341)).astype(f32).astype(f64)).astype(f32)
    er = np.copysign((f32(1) - (poly * e).astype(f32)).astype(f32), xs)
    return (f32(0.5) * g * (f32(1) + er)).astype(f32)


def emulate(c, inp, rows):
    w, F = inp["w"], 4 * m.C
    st = {}
    st["x1"] = emu_contraction(inp["a1"], w["wo1"], w.get("bo1"), inp["x0"])
    st["ln2"] = emu_ln(st["x1"], w["g2"], w["be2"], m.EPS, rows)
    st["q"] = emu_contraction(st["ln2"], w["wq2"], w.get("bq2"))
    st["a2"] = emu_attention(st["q"], inp["k"], inp["v"], inp["scale"], c["imgs"])
    st["x2"] = emu_contraction(st["a2"], w["wo2"], w.get("bo2"), st["x1"])
    st["ln3"] = emu_ln(st["x2"], w["g3"], w["be3"], m.EPS, rows)
    hp = st["ln3"].astype(f32) @ w["w1"].astype(f32).T
    hp = hp + (w["b1"].astype(f32) if w.get("b1") is not None else f32(0))
    h = (hp[:, :F] * emu_gelu(hp[:, F:])).astype(f32).astype(f16)
    x3 = emu_contraction(h, w["w2"], w.get("b2"), st["x2"])
    if c["proj"]:
        st["x3"] = x3
        st["out"] = emu_contraction(x3, w["wpo"], w.get("bpo"), inp["xin"])
    else:
        st["out"] = x3
    return st


def test_bounds_hold_for_the_cpu_emulations():
    m.WORST.clear()
    m.CEFF[:] = [0.0, ""]
    n = 0
    for c in m.CASES:
        if c["M"] > 128:
            continue
        m.verify(c, m.inputs(c), emulate(c, m.inputs(c), c["rows"]), c["rows"])      # (asserts every bound, every FAR cap, c_eff <= 4.1, the score range)
        n += 1
    m.print_worst()                                                                  # (-s)
    assert n == 26 and set(m.WORST) == set(m.STAGES) | {"y"}
    assert m.CEFF[0] <= 4.1, m.CEFF
