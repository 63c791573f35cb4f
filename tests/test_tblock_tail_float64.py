"""-m gpu: the transformer-block tail (osg_tblock_tail, onnxstream_amd/csrc/osg_tchain.hip) stage by stage, per element, against float64.

What is pinned.  Every case asserts the launch record (osg_last_kernel family 4: rows per block, NS, row blocks, prefetch workgroups, proj_out, second
destination); `out` (and `out2`) lie between guard bands of a 0xFF-filled allocation, and where `out` is a column view the columns outside it must come back
0xFF; every case is seeded and frees its buffers.  Stage s is compared with float64 applied to the DEVICE'S OWN dump of the stage before it (x1, LN(x1), q,
a2, x2, LN(x2), x3; the host operands feed x1), so every stage is one rounding deep and no error compounds; the end-to-end assertion stays in
tests/test_tblock_tail.py.  test_coverage fails, naming what is missing, unless the records include rows {32, 64} x prefetch workgroups {0, 8} x proj_out
{0, 1} and a second destination.

Left out: the NS = 3 instantiation (tblock_tail_kernel<2, 320, 40, 5, 3>) is reached only through OSG_TBLOCK_NS, and OSG_TBLOCK_ROWS, OSG_TBLOCK_PREFETCH and
the two OSG_TBLOCK_PF_SLEEP knobs are read once per process as well: under the session-wide `gpu` fixture they stay at their defaults.  C = 320 with 8 heads
is all the kernel takes.

Bounds (u = 2^-24, H = 2^-11).
  x1, q, x2, y   one contraction over K = 320 in f32, bias and residual added in f32, one RNE to f16: the bound and the check of
                 tests/test_contraction_instantiations.py, |got - want| <= H |want| + (1 + H)(K + 3) u S + 2^-25, S the sum of the absolute terms; at most
                 FAR = 0.02 of the elements more than one f16 ulp from the correctly rounded float64 result.
  LN(x1), LN(x2) section C of tests/test_unet_attention_norm.py (norm_exact, two passes) with the chain of ln_rows: a lane adds 8 PER values, then
                 log2(lanes per row) shuffles: g = 8 PER + 3, PER = 10 with 64-row blocks (4 lanes a row), 5 with 32-row blocks (8 lanes).  FAR applies.
  a2             one pass over at most 80 keys, no running maximum, no rescale.  With p~_j = 2^((s_j - m) c), P = sum p~_j, want = sum p~_j v_jd / P and
                 A = sum p~_j |v_jd| / P the kernel computes
                   s_j   D = 40 f16 products in f32 (16x16x16 MFMAs):                              |ds_j| <= D u sum_d |q_d k_jd|
                   t_j   = f32(s_j c) - f32(m c), c = f32(scale) f32(log2 e): an error of the maximum shifts every t_j alike and cancels in p / P, so
                         per key                                                                   |dt_j| <= u (D c Sabs + 3 |t|max + 3 |m c|)
                   e_j   = v_exp_f32(t_j): 2^-23 relative, ln2 |dt_j| from the argument:           eps = ln2 u (...) + 2^-23
                   p^_j  = f16(e_j) multiplies V: H relative where p~_j is a normal f16, 2^-25 absolute below 2^-14; 80 products in five MFMAs: 85 u
                   l     = the sum of the UNROUNDED e_j (attn2_kernel adds the f16 values: there the rounding of p^ enters numerator and denominator, here
                         the numerator alone): 20 additions in a lane and two shuffles, 22 u; 1 / l and the product: 3 u
                 o / l - want = (sum p~_j e'_j v_jd + sum u_j v_jd) / P - want delta, |e'_j| <= H + eps + 85 u, |delta| <= eps + 25 u:
                   E = (H + eps + 85 u) A + (eps + 25 u) |want| + 2^-25 sum_{p~_j < 2^-14} |v_jd| / P,    |got - want| <= (1 + 2^-8) E + ulp16(|want| + E) / 2.
                 Since |want| <= A this is ulp16 / 2 + c H A with c = (1 + 2^-8)(1 + (2 eps + 110 u) / H): c_eff is printed and asserted <= 4.1 (it stays
                 near 1: the row sum is not rounded to f16).  No FAR cap on zero-mean V (|want| << A: an f32 emulation already leaves 8 - 11 % of the
                 elements more than an ulp off); with V offset by 3 FAR applies.  Tk = 1: p = 1, the sum is 1, the product exact -- a2 equals V's row bit for bit.
  x3             two contractions with the f16 rounding of the GEGLU hidden h between them (h is not dumped): want = ff.net.2 in float64 over
                 h_ref = f16(float64 GEGLU of ff.net.0.proj(LN(x2) dump)), + b2 + the x2 dump; bound = the contraction bound of ff.net.2 (K = 1280) +
                 sum_k |w2_nk| (E_h,k + H |h_k| + 2^-25), E_h from act_apply(..., ACT_GEGLU) on ff.net.0.proj's bound.  The worst case is loose; the FAR cap
                 is the part with teeth.

Per stage, over all cases: worst error / bound, the largest share of the allowance beyond the last rounding that is used (arith_share), the largest share of
elements more than one f16 ulp from the correctly rounded result.  The emulation column is tests/test_tblock_tail_emulation_cpu.py (numpy restatement of the
declared arithmetic, the cases with M <= 128); the MI355X column holds what `-s` printed on the device when the module was added ("not measured": no device run
was possible then; the first run's `-s` output belongs here).  The contractions and LayerNorms reach ~0.9 - 1.0 of
their bounds because the half-ulp term of the last rounding is sharp; x3's worst case is loose, as said above.
                 emulation                   MI355X
  x1             0.890 / 0.008 / 0.0002   not measured
  LN(x1)         0.994 / 0.034 / 0.0000   not measured
  q              0.842 / 0.004 / 0.0003   not measured
  a2             0.656 / 0.534 / 0.1077   not measured
  x2             0.925 / 0.006 / 0.0001   not measured
  LN(x2)         0.994 / 0.023 / 0.0000   not measured
  x3             0.315 / 0.014 / 0.0023   not measured
  y              0.882 / 0.004 / 0.0002   not measured
  c_eff of the a2 bound: at most 1.49 (inputs and bound alone).
"""
import math
import os
from functools import lru_cache

import numpy as np
import pytest

import test_contraction_instantiations as ci
import test_unet_attention_norm as an
from test_tblock_tail import make_block, rnd

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
U24, H11 = 2.0 ** -24, 2.0 ** -11
LOG2E = 1.4426950408889634
C, HEADS, D = 320, 8, 40
TBLOCK = 4                                   # osg_last_kernel family
STAGES = ["x1", "ln2", "q", "a2", "x2", "ln3", "x3"]
FAMILIES = ("normal", "offset", "bigscore", "bq2", "nobias")
RECORDS = {}                                 # case id -> launch record (test_coverage reads it)
WORST = {}                                   # stage -> [error / bound, arith_share, far, case id of the worst ratio]
CEFF = [0.0, ""]


@pytest.fixture
def dev(gpu):
    """device buffers of one case, freed when it ends: uploads, 0xFF-filled outputs and whatever a wrapper allocated (keep)"""
    held = []

    class Dev:
        def __call__(self, arr):
            return self.keep(gpu.to_dev(arr))

        def nan(self, n, dtype=f16):
            return self.keep(gpu.empty((n,), dtype))          # every byte 0xFF

        def keep(self, b):
            held.append(b)
            return b

    yield Dev()
    for b in held:
        b.free()


@lru_cache(maxsize=None)
def num_cu():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256                             # (the MI355X; the prefetch cases then assert the record a 256-CU device gives)


# =====================================================================================================================================
# cases and inputs
# =====================================================================================================================================
def tcase(M, imgs, Tk, proj, rows, family="normal"):
    return dict(id=f"M{M}-img{imgs}-Tk{Tk}-{'proj' if proj else 'noproj'}-rows{rows}-{family}", M=M, imgs=imgs, Tk=Tk, proj=proj, rows=rows, family=family)


def cases():
    cs = [tcase(32, 1, 77, True, 32), tcase(96, 3, 77, True, 32)]                # one block; every block reads another image's K / V
    for rows in (32, 64):
        cs.append(tcase(128, 2, 77, False, rows))                                # out is x3
        cs += [tcase(128, 1, tk, True, rows) for tk in (1, 15, 16, 17, 64, 80)]  # the boundaries of the 16-token tiles
        cs += [tcase(128, 2, 77, True, rows, fam) for fam in FAMILIES]
    # the weight-prefetching workgroups (row blocks >= 64 and row blocks + 8 <= CUs); the two marked + complete rows x proj_out for test_coverage
    cs += [tcase(2048, 1, 77, True, 32), tcase(2048, 1, 77, False, 32),          # +
           tcase(4096, 1, 77, False, 64), tcase(4096, 1, 77, True, 64),          # +
           tcase(4096, 1, 77, True, 0)]                                          # the library's own choice: 32 rows, 128 blocks
    return cs


CASES = cases()
EPS = 1e-5


def inputs(c):
    """host operands of a case: w (dict, weights [N, K]), a1, x0, xin [M, C], k, v [imgs, Tk, C], scale"""
    M, imgs, Tk, fam = c["M"], c["imgs"], c["Tk"], c["family"]
    rng = np.random.default_rng(M * 1000 + Tk * 7 + imgs + 101 * FAMILIES.index(fam))
    w = make_block(rng, C)
    a1, x0, xin = rnd(rng, (M, C)), rnd(rng, (M, C)), rnd(rng, (M, C))
    k, v = rnd(rng, (imgs, Tk, C)), rnd(rng, (imgs, Tk, C))
    scale = float(f32(D ** -0.5))
    if fam == "offset":            # rows of the residual stream with a mean of +-4 (LayerNorm's cancellation), V with a mean of 3 (sum p v large)
        x0 = (x0.astype(f32) + np.where(np.arange(M) % 2, -4.0, 4.0).astype(f32)[:, None]).astype(f16)
        v = (v.astype(f32) + 3).astype(f16)
    elif fam == "bigscore":        # K scaled so that max |scale q k| ~ 25 (q from the float64 chain): probabilities that underflow f16
        x1 = a1.astype(f64) @ w["wo1"].astype(f64).T + w["bo1"].astype(f64) + x0.astype(f64)
        n2 = (x1 - x1.mean(1, keepdims=True)) / np.sqrt(x1.var(1, keepdims=True) + EPS) * w["g2"].astype(f64) + w["be2"].astype(f64)
        q = n2 @ w["wq2"].astype(f64).T
        k = (k.astype(f64) * (25.0 / max_score(q, k, scale, imgs))).astype(f16)
    elif fam == "bq2":
        w["bq2"] = rnd(rng, (C,), 0.1)
    elif fam == "nobias":
        for n in ("bo1", "bo2", "b1", "b2", "bpo"):
            w[n] = None
    return dict(w=w, a1=a1, x0=x0, xin=xin, k=k, v=v, scale=scale)


def heads_of(t, imgs):
    """[imgs * T, C] or [imgs, T, C] -> [imgs, heads, T, D]"""
    return t.reshape(imgs, -1, HEADS, D).transpose(0, 2, 1, 3)


def max_score(q, k, scale, imgs):
    s = np.einsum("bhqd,bhkd->bhqk", heads_of(np.asarray(q, f64), imgs), heads_of(np.asarray(k, f64), imgs))
    return float(np.abs(s).max() * scale)


# =====================================================================================================================================
# float64 references and bounds, one stage at a time
# =====================================================================================================================================
def xattn_exact(q, k, v, scale):
    """one head: q [R, D], k, v [Tk, D] (f16) -> float64 want, bound, c_eff [R, D] (module docstring, a2)"""
    q, k, v = q.astype(f64), k.astype(f64), v.astype(f64)
    c = scale * LOG2E
    s = q @ k.T
    sabs = (np.abs(q) @ np.abs(k).T).max(axis=1)
    m = s.max(axis=1)
    t = (s - m[:, None]) * c
    pt = np.exp2(t)
    P = pt.sum(axis=1, keepdims=True)
    want = (pt @ v) / P
    A = (pt @ np.abs(v)) / P
    sub = (pt < 2.0 ** -14 * (1 + 2.0 ** -9)).astype(f64)
    eps = (math.log(2) * U24 * (D * c * sabs + 3 * np.abs(t).max(axis=1) + 3 * np.abs(m) * c) + 2.0 ** -23)[:, None]
    E = (H11 + eps + 85 * U24) * A + (eps + 25 * U24) * np.abs(want) + 2.0 ** -25 * (sub @ np.abs(v)) / P
    E = E * (1 + 2.0 ** -8)
    bound = E + an.ulp16(np.abs(want) + E) / 2
    ceff = (1 + 2.0 ** -8) * ((H11 + eps + 85 * U24) * A + (eps + 25 * U24) * np.abs(want)) / (H11 * A)
    return want, bound, ceff


def attention_reference(q, k, v, scale, imgs):
    """q [M, C] (a stage dump), k, v [imgs, Tk, C] -> want, bound [M, C], the largest c_eff"""
    M = q.shape[0]
    qh, kh, vh = heads_of(q, imgs), heads_of(k, imgs), heads_of(v, imgs)
    want, bound = np.empty((imgs, HEADS, M // imgs, D)), np.empty((imgs, HEADS, M // imgs, D))
    ceff = 0.0
    for b in range(imgs):
        for h in range(HEADS):
            want[b, h], bound[b, h], ce = xattn_exact(qh[b, h], kh[b, h], vh[b, h], scale)
            ceff = max(ceff, float(ce.max()))
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(M, C)
    return back(want), back(bound), ceff


def ln_reference(x, gam, bet, rows):
    per = 10 if rows == 64 else 5
    return an.norm_exact(x.astype(f64), gam.astype(f64), bet.astype(f64), float(f32(EPS)), 8 * per + 3, False, 0, f16)


def contraction_bound(want, E):
    return H11 * np.abs(want) + (1 + H11) * E + ci.TINY


def x3_reference(ln3, x2, w):
    """want and E (the allowance in front of the last rounding) of x3 from the dumps of LN(x2) and x2"""
    pre, E1 = ci.contraction(ln3, w["w1"], w["b1"])
    hval, Eh = ci.act_apply(pre, E1, ci.ACT_GEGLU)
    h_ref = hval.astype(f16)
    want, E2 = ci.contraction(h_ref, w["w2"], w["b2"], x2)
    return want, E2 + (Eh + H11 * np.abs(hval) + ci.TINY) @ np.abs(w["w2"].astype(f64)).T


def report(stage, cid, got, want, bound):
    """print worst error / bound, arith_share and the share of elements more than an ulp off; keep the worst of the module; -> (ratio array, far)"""
    ratio = np.abs(got.astype(f64) - want) / bound
    worst, share, far = float(ratio.max()), an.arith_share(got, want, bound), float((ci.ulps_off(got, want) > 1).mean())
    print(f"[{stage}] {cid}: worst error / bound {worst:.3f} (beyond the last rounding: {share:.3f} of the allowance; {far:.4f} of the elements more than an ulp off)")
    wst = WORST.setdefault(stage, [0.0, 0.0, 0.0, ""])
    if worst > wst[0]:
        wst[0], wst[3] = worst, cid
    wst[1], wst[2] = max(wst[1], share), max(wst[2], far)
    return ratio, far


def assert_bound(stage, cid, got, want, bound, ratio):
    if ratio.max() > 1.0:
        i = tuple(int(x) for x in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        raise AssertionError(f"{cid} {stage}: {int((ratio > 1).sum())} of {ratio.size} elements outside the bound; worst at {i}: got {float(got[i])!r}, want {want[i]!r}, "
                             f"bound {bound[i]!r} (error / bound {float(ratio.max()):.2f}); first at {tuple(int(x) for x in np.argwhere(ratio > 1.0)[0])}")


def verify(c, inp, st, rows):
    """st: stage name -> f16 [M, C] (x1, ln2, q, a2, x2, ln3, x3 with proj_out, and `out`), each checked against float64 of the stage before it"""
    cid, w, imgs = c["id"], inp["w"], c["imgs"]
    for n, t in st.items():
        assert np.isfinite(t.astype(f32)).all(), f"{cid}: {n} not finite"

    def contraction_stage(stage, got, a, wn, bias, res):
        want, E = ci.contraction(a, w[wn], w.get(bias), res)
        report(stage, cid, got, want, contraction_bound(want, E))
        ci.check(got, want, E, f"{cid} {stage}")

    def ln_stage(stage, got, x, gam, bet):
        want, bound = ln_reference(x, w[gam], w[bet], rows)
        ratio, far = report(stage, cid, got, want, bound)
        assert_bound(stage, cid, got, want, bound, ratio)
        assert far <= ci.FAR, f"{cid} {stage}: {far:.4f} of the elements more than one f16 ulp from the correctly rounded result"

    contraction_stage("x1", st["x1"], inp["a1"], "wo1", "bo1", inp["x0"])
    ln_stage("ln2", st["ln2"], st["x1"], "g2", "be2")
    contraction_stage("q", st["q"], st["ln2"], "wq2", "bq2", None)
    if c["family"] == "bigscore":
        s = max_score(st["q"], inp["k"], inp["scale"], imgs)
        assert 20.0 <= s <= 30.0, f"{cid}: max |scale q k| = {s:.1f}"
    want, bound, ceff = attention_reference(st["q"], inp["k"], inp["v"], inp["scale"], imgs)
    if ceff > CEFF[0]:
        CEFF[:] = [ceff, cid]
    ratio, far = report("a2", cid, st["a2"], want, bound)
    print(f"[a2] {cid}: c_eff {ceff:.3f}")
    assert_bound("a2", cid, st["a2"], want, bound, ratio)
    assert ceff <= 4.1, f"{cid}: c_eff {ceff:.2f}"
    if c["family"] == "offset":
        assert far <= ci.FAR, f"{cid} a2: {far:.4f} of the elements more than one f16 ulp from the correctly rounded result"
    if c["Tk"] == 1:
        rows_v = np.repeat(inp["v"][:, 0, :], c["M"] // imgs, axis=0)
        assert np.array_equal(st["a2"].view(np.uint16), rows_v.view(np.uint16)), f"{cid}: with one key a2 is V's row, bit for bit"
    contraction_stage("x2", st["x2"], st["a2"], "wo2", "bo2", st["x1"])
    ln_stage("ln3", st["ln3"], st["x2"], "g3", "be3")
    x3 = st["x3"] if c["proj"] else st["out"]
    want, E = x3_reference(st["ln3"], st["x2"], w)
    report("x3", cid, x3, want, contraction_bound(want, E))
    ci.check(x3, want, E, f"{cid} x3")
    if c["proj"]:
        contraction_stage("y", st["out"], st["x3"], "wpo", "bpo", inp["xin"])


# =====================================================================================================================================
# the device
# =====================================================================================================================================
def upload(gpu, dev, inp, proj):
    """-> device operands of gpu.tblock_tail: the weight dict (packed), a1, x0, xin, kp, vtp -- all freed with the case"""
    dw = {}
    for n, t in inp["w"].items():
        if t is None or (not proj and n in ("wpo", "bpo")):
            dw[n] = None
        elif n in gpu.TBLOCK_WEIGHTS:
            dw[n] = dev.keep(gpu.tblock_pack_weight(dev(t)))
        else:
            dw[n] = dev(t)
    kp, vtp = gpu.tblock_kv_pack(dev(inp["k"]), dev(inp["v"]), HEADS)
    return dw, dev(inp["a1"]), dev(inp["x0"]), dev(inp["xin"]) if proj else None, dev.keep(kp), dev.keep(vtp)


def expected_record(c, rows, out2=0):
    nblk = c["M"] // rows
    ns = 3 if rows == 32 and os.environ.get("OSG_TBLOCK_NS", "").strip() == "3" else 2
    return (TBLOCK, rows, ns, nblk, 8 if nblk >= 64 and nblk + 8 <= num_cu() else 0, int(c["proj"]), out2, 0)


def launch(gpu, dev, c, ops, debug, **kw):
    dw, a1, x0, xin, kp, vtp = ops
    out, dumps = gpu.tblock_tail(a1, x0, dw, kp, vtp, c["Tk"], HEADS, float(f32(D ** -0.5)), c["M"] // c["imgs"], EPS, xin=xin, debug=debug, rows_per_block=c["rows"], **kw)
    for d in dumps:
        dev.keep(d)
    return dumps, gpu.last_kernel()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_stage_by_stage(gpu, dev, c):
    M = c["M"]
    rows = c["rows"] or 32                          # (rows_per_block = 0 at M = 4096: M / 64 < 2 CUs, the library takes 32-row blocks)
    want_rec = expected_record(c, rows)
    if M >= 2048 and want_rec[4] != 8:
        pytest.skip(f"{M // rows} row blocks + 8 prefetching workgroups do not fit the {num_cu()} CUs of this device")
    inp = inputs(c)
    assert gpu.lib.osg_tblock_tail_supported(M, M // c["imgs"], C, HEADS, c["Tk"]) == 1
    ops = upload(gpu, dev, inp, c["proj"])
    buf, out = an.guarded(dev, (M, C))
    dumps, rec = launch(gpu, dev, c, ops, True, out=out)
    RECORDS[c["id"]] = rec
    assert rec == want_rec, (rec, want_rec)
    st = {n: dumps[i].numpy() for i, n in enumerate(STAGES) if n != "x3" or c["proj"]}
    if not c["proj"]:
        assert (dumps[6].numpy().view(np.uint16) == 0xFFFF).all(), "x3 has no dump without proj_out"
    st["out"] = an.read_guarded(buf, (M, C))
    verify(c, inp, st, rows)


ABI = [tcase(128, 2, 77, proj, rows) for rows in (32, 64) for proj in (True, False)]


@pytest.mark.parametrize("c", ABI, ids=[c["id"] for c in ABI])
def test_out_is_the_same_with_and_without_stage_dumps(gpu, dev, c):
    """the production launch (dbg all NULL) writes the bits of the launch the stage checks read"""
    inp = inputs(c)
    ops = upload(gpu, dev, inp, c["proj"])
    res = []
    for debug in (True, False):
        buf, out = an.guarded(dev, (c["M"], C))
        _, rec = launch(gpu, dev, c, ops, debug, out=out)
        assert rec == expected_record(c, c["rows"]), rec
        res.append(an.read_guarded(buf, (c["M"], C)))
    assert np.array_equal(res[0].view(np.uint16), res[1].view(np.uint16))


@pytest.mark.parametrize("c", ABI[::2], ids=[c["id"] for c in ABI[::2]])
def test_out_as_a_column_view_with_a_second_destination(gpu, dev, c):
    """out at a row pitch into a Concat slot (the planner's a.ldo = dst_ld) and out2 at another pitch in the same launch: the same bits, nothing else written"""
    M = c["M"]
    inp = inputs(c)
    ops = upload(gpu, dev, inp, True)
    P1, C1, P2, C2 = 2 * C + 64, C, C + 24, 8
    buf1, wide1 = an.guarded(dev, (M, P1))
    buf2, wide2 = an.guarded(dev, (M, P2))
    _, rec = launch(gpu, dev, c, ops, False, out=wide1, out_col=C1, out2=wide2, out2_col=C2)
    RECORDS["view:" + c["id"]] = rec
    assert rec == expected_record(c, c["rows"], out2=1), rec
    got = []
    for buf, pitch, col in ((buf1, P1, C1), (buf2, P2, C2)):
        raw = buf.numpy()
        inside = np.zeros((M, pitch), bool)
        inside[:, col:col + C] = True
        mask = np.concatenate([np.zeros(an.GUARD, bool), inside.ravel(), np.zeros(an.GUARD, bool)])
        assert (raw.view(np.uint16)[~mask] == 0xFFFF).all(), "a store landed outside the column view (guard band or the columns beside it)"
        got.append(raw[mask].reshape(M, C))
        assert np.isfinite(got[-1].astype(f32)).all()
    assert np.array_equal(got[0].view(np.uint16), got[1].view(np.uint16)), "out and out2 differ"
    bufd, dense = an.guarded(dev, (M, C))
    launch(gpu, dev, c, ops, False, out=dense)
    assert np.array_equal(an.read_guarded(bufd, (M, C)).view(np.uint16), got[0].view(np.uint16)), "the column view holds other bits than a dense out"


# ---- the packs: pure data movement, bit exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tk", [1, 17, 77, 80])
def test_kv_pack_jobs(gpu, dev, Tk):
    """three jobs (head dims 40, 80, 160: the three levels of the UNet) at distinct column pairs of one [imgs * Tk][ld] matrix wider than the columns used"""
    imgs = 2
    rng = np.random.default_rng(Tk)
    jobs = [(8, 2272, 40), (2600, 336, 80), (3248, 984, 160)]            # (k_col, v_col, D); 8 D columns each, in the order K0 V1 V2 V0 K1 K2, 8 columns between them
    ld = 4544
    base = rnd(rng, (imgs * Tk, ld))
    total = sum(2 * imgs * HEADS * 80 * ((d + 15) // 16 * 16) for _, _, d in jobs)
    buf, dst = an.guarded(dev, (total,))
    _, offs = gpu.tblock_kv_pack_jobs(dev(base), ld, imgs, Tk, HEADS, jobs, out=dst)
    got = an.read_guarded(buf, (total,))
    b3 = base.reshape(imgs, Tk, ld)
    for (kc, vc, d), off in zip(jobs, offs):
        dp = (d + 15) // 16 * 16
        n = imgs * HEADS * 80 * dp
        assert n == gpu.lib.osg_tblock_kv_pack_elems(imgs, HEADS, d)
        want_kp = np.zeros((imgs, HEADS, 80, dp), f16)
        want_kp[:, :, :Tk, :d] = b3[:, :, kc:kc + HEADS * d].reshape(imgs, Tk, HEADS, d).transpose(0, 2, 1, 3)
        want_vt = np.zeros((imgs, HEADS, dp, 80), f16)
        want_vt[:, :, :d, :Tk] = b3[:, :, vc:vc + HEADS * d].reshape(imgs, Tk, HEADS, d).transpose(0, 2, 3, 1)
        assert np.array_equal(got[off:off + n].view(np.uint16), want_kp.ravel().view(np.uint16)), f"K pack of job {(kc, vc, d)}"
        assert np.array_equal(got[off + n:off + 2 * n].view(np.uint16), want_vt.ravel().view(np.uint16)), f"V^T pack of job {(kc, vc, d)}"


@pytest.mark.parametrize("N,K", [(320, 320), (2560, 320), (320, 1280), (1, 8), (3, 24)])
def test_pack_weight(gpu, dev, N, K):
    w = rnd(np.random.default_rng(N + K), (N, K))
    buf, out = an.guarded(dev, (K // 8, N, 8))
    gpu.tblock_pack_weight(dev(w), out=out)
    got = an.read_guarded(buf, (K // 8, N, 8))
    assert np.array_equal(got.view(np.uint16), w.reshape(N, K // 8, 8).transpose(1, 0, 2).view(np.uint16))


def print_worst():
    for stage in STAGES + ["y"]:
        if stage in WORST:
            r, share, far, cid = WORST[stage]
            print(f"[{stage}] over the module: worst error / bound {r:.3f} ({cid}), beyond the last rounding {share:.3f} of the allowance, at most {far:.4f} of the elements more than an ulp off")
    print(f"[a2] the largest c of c 2^-11 A: {CEFF[0]:.3f} ({CEFF[1]})")


def test_coverage():
    """the records of the cases above: fails, naming what is missing, unless every rows x prefetch workgroups x proj_out combination and a second destination
    were launched.  It reads RECORDS, which the cases fill as they run: it has to run after them in the same process, and fails, on purpose, under a selection
    that gives it less than the whole module.  On a device whose CU count rules the prefetching workgroups out those combinations are not asked for."""
    have = {r[1:2] + r[4:6] for r in RECORDS.values() if r[0] == TBLOCK}
    pfs = (0, 8) if 64 + 8 <= num_cu() else (0,)
    missing = [f"rows {rows} prefetch workgroups {pf} proj_out {po}" for rows in (32, 64) for pf in pfs for po in (0, 1) if (rows, pf, po) not in have]
    if not any(r[6] == 1 for r in RECORDS.values()):
        missing.append("a second destination")
    print_worst()
    assert not missing, "not reached: " + "; ".join(missing)
