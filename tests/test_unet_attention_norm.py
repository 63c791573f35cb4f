"""-m gpu: the UNet's attention and normalisation kernels, per route, per element, against float64 restatements written here.

What is pinned.  Every case asserts through osg_last_kernel (include/osgpu.h) which kernel the entry point launched; every output is a view between two
guard bands of one 0xFF-filled allocation (NaN in f16 and f32) and, for the strided attention layouts, every element of that allocation the call must not
write has to come back 0xFF; every case is seeded and frees its buffers.  The last test fails, naming what is missing, unless the records collected by the
cases include all 8 attn2_kernel instantiations, the GroupNorm routes / (NV, threads) / groups per block / cluster sizes listed at GN_WANTED, LayerNorm
NV 1-4 + both generic kernels and InstanceNorm with 256 / 1024 threads in both dtypes.

Left out: the knobs OSG_ATTN_QT, OSG_ATTN_BKV, OSG_ATTN_V1 and OSG_GN_STATS_APPLY_V2 are read once per process, so under the session-wide `gpu` fixture the
v2 producer-statistics kernel (gn_apply_stats_kernel), the 128-key attn_kernel and a forced QT stay untested here; QT = 2 is reached by shape.  attn_kernel,
RMSNorm, softmax and reduce-mean are the decoder module's (tests/test_decoder_kernels.py).

A. attn2_kernel<D, QT, NST>.  Reference: float64 softmax(scale q k^T) v on the f16 operands.  With p~_j = 2^((s_j - m) c) the unnormalised probabilities
   (m the row maximum, c = scale log2 e), P = sum p~_j, p_j = p~_j / P, want = sum p_j v_jd and A = sum p_j |v_jd|, the kernel computes
     s_j     f16 products (exact in f32) accumulated in f32 over D terms:                   |ds_j| <= D u sum_d |q_d k_jd|            (u = 2^-24)
     t_j     = fma(s_j, c, -m c) in f32, c = f32(scale) * f32(log2 e) (1.5 u relative), -m c rounded once, the fma once:
                                                                                            |dt_j| <= u (D c Sabs + 3 |t|max + 3 |m c|)
     p^_j    = f16(v_exp_f32(t_j)): 2^-23 relative for v_exp_f32, ln2 |dt_j| from the argument, then RNE to f16 -- 2^-11 relative where p~_j is a normal
             f16 and 2^-25 absolute below 2^-14 (an earlier tile's p^ is relative to the running maximum of its time, so it is no smaller than p~_j:
             subnormal then implies p~_j < 2^-14; the later rescale by alpha <= 1 only shrinks the absolute term).  alpha itself is a v_exp_f32 of an
             f32 product: 2^-22 per rescale, at most one per key tile.
     l, o_d  the row sum is the sum of the SAME f16 values p^_j that multiply v (the all-ones MFMA), both accumulated in f32: 32 products inside an
             MFMA, two MFMAs and at most one rescale per key tile: (32 + 3 ntiles) u relative to sum p^ |v| resp. sum p^.
     got     = f16(o_d * (1 / l)): two f32 roundings, one RNE to f16.
   With p^_j = p~_j (1 + e_j) + u_j, |e_j| <= 2^-11 + eps, |u_j| <= 2^-25 [p~_j < 2^-14]:
     o/l - want = (sum p~_j e_j v_jd + sum u_j v_jd) / P - want (sum p~_j e_j + sum u_j) / P + second order, so
     E = (2^-11 + eps + (35 + 3 ntiles) u) (A + |want|) + 2^-25 (sum_{p~_j < 2^-14} |v_jd| + |want| #{p~_j < 2^-14}) / P
     eps = ln2 u (D c Sabs + 3 |t|max + 3 |m c|) + 2^-22 (1 + ntiles),           |got - want| <= (1 + 2^-8) E + ulp16(|want| + E) / 2.
   Since |want| <= A this is the issue's form ulp16 / 2 + c 2^-11 A with c = 2 (1 + eps 2^11 + ...): the worst c_eff over the cases is printed (-s) next to
   the worst error / bound.  To keep c_eff below 4 the large-score family reaches |scale q k| ~ 30 for D <= 80 and ~ 20 for D = 160 (eps grows with
   D c Sabs, the worst-case f32 accumulation of the scores).
B. GroupNorm.  Reference: float64 mean / variance / affine / SiLU on the stored operands.  The kernels add x and x^2 (fma: the squares are exact) in f32
   along chains of at most g additions (then in f64), g from the launch record: NV + 16 for the slab kernels (NV row vectors, 8 elements, a 6-level wave
   tree), rows per thread + (channels of a group in a sweep) * R + 4 for the three-pass statistics (R = 256 / vector columns), and form
   mean = S1 icnt, var = f32(S2 icnt - mean^2) in f64 with icnt an f32 reciprocal (2 u), rstd = 1 / sqrtf(var + eps):
     dmean <= u (g E|x| + 2 |mean|),   dvar <= u ((g + 4) E[x^2] + 2 |mean| (g E|x| + 2 |mean|)),   E[x^2] = var + mean^2,
     rho (relative error of rstd) <= 1 / sqrt(1 - min(dvar, var) / (var + eps)) - 1 + 3 u  ~  (1.5 g + 4) u (1 + mean^2 / var): the conditioning term.
   a = rstd gamma, b = beta - mean a, y = x a + b in f32 (fma or not), pre = (x - mean) a + beta:
     E_pre = |pre - beta| (rho + 2 u) + |a| (dmean + 3 u |mean|) + 2 u (|beta| + |pre|)
   (the second term is the cancellation of x a against mean a); SiLU (slope <= 1.1, osg_sigmoid accurate to (3 + 0.65 |pre|) 2^-23 relative, see the
   decoder module): E = 1.1 E_pre + (3.5 + 0.65 |pre|) 2^-23 |want|.  |got - want| <= (1 + 2^-8) E + ulp16(|want| + E) / 2 (f32 output: no ulp term).
   The producer-statistics form reads int64 fixed-point sums of the producer's per-wave f32 partials: each partial is rounded to 2^-20 (sum) resp.
   1 / stat_q_scale (squares), at most HW / 8 partials per group (a wave covers at least 16 rows; a group's columns lie in at most two waves), g = 256.
C. LayerNorm / InstanceNorm compute the variance from the deviations (two passes): dmean as above, var^ = var + dmean^2 exactly up to (g + 4) u var,
   g = 8 NV + 6 (layer_norm_kernel), C / 256 + 12 (generic), L / threads + 24 (InstanceNorm);  E_pre = |pre - beta| (rho + 4 u) + |a| dmean + 2 u (|pre| + |beta|).

CPU emulations of that arithmetic (emulate_attn2, emulate_onepass, emulate_twopass below; `python tests/test_unet_attention_norm.py` runs them over the
inputs of every case of this module, no GPU needed; tests/test_unet_attention_norm_emulation_cpu.py asserts it) stay inside the bounds.  Worst
error / bound of the emulations, with the figure measured on an MI355X when the module was added beside it:
  A  N(0,1) / N(0,2) inputs 0.454 (Tkv = 4096: 0.075), dominating keys 0.299, maxima in tile 0 0.422, |scale q k| ~ 30 0.378, V with an offset 0.302;
     the emulation must stay below 0.67.  MI355X: 0.454 over the section.  The c of c 2^-11 A depends on the bound and the inputs alone: at most 4.01
     (D = 160, |scale q k| ~ 20); the CPU test asserts c <= 4.1.
  B, C  the half-ulp term of the last rounding is sharp -- an f32 result next to a rounding boundary is half an ulp off however exact it is -- so
     error / bound reaches 1.000 in every family, on the emulation and on the device alike.  Of the REST of the bound, the allowance E for the arithmetic in
     front of that rounding (arith_share), the emulation uses at most 0.323 (B) and 0.245 (C), the MI355X 0.356 (B) and 0.245 (C).
     The emulation leaves out the two GroupNorm tensors of more than 2^23 elements; three-C8-G1-HW16385 has the chain length (g ~ 2000) of the larger one,
     and for the three-pass cases the emulation's running sums are as long as g.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
U24, H11 = 2.0 ** -24, 2.0 ** -11
LOG2E = 1.4426950408889634
GUARD = 256                     # elements of guard before and after an output (keeps 16-byte alignment)
OSG_F16, OSG_F32 = 2, 3
ATTENTION, GROUPNORM, LAYERNORM, INSTANCENORM = 0, 1, 2, 3          # osg_last_kernel families
SLAB, CLUSTER, THREE_FOLD, THREE_FINALIZE, THREE_F32, STATS_V1 = 0, 1, 2, 3, 4, 5     # GroupNorm routes; the shapes below were chosen for a device of 256 CUs
RECORDS = {}                    # case id -> osg_last_kernel record (test_coverage reads it)
WORST = {}                      # section -> (error / bound, case id)


def ulp16(x):
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f16)).astype(f64)


def note(section, cid, ratio, extra=""):
    print(f"[{section}] {cid}: worst error / bound {ratio:.3f} {extra}")
    if ratio > WORST.get(section, (0.0, ""))[0]:
        WORST[section] = (ratio, cid)


@pytest.fixture
def dev(gpu):
    """device buffers of one case, freed when it ends: uploads and 0xFF-filled outputs"""
    held = []

    class Dev:
        def __call__(self, arr):
            b = gpu.to_dev(arr)
            held.append(b)
            return b

        def nan(self, n, dtype=f16):
            b = gpu.empty((n,), dtype)          # every byte 0xFF
            held.append(b)
            return b

    yield Dev()
    for b in held:
        b.free()


def guarded(dev, shape, dtype=f16):
    """(whole allocation, view of `shape` between two GUARD bands)"""
    n = int(np.prod(shape))
    buf = dev.nan(n + 2 * GUARD, dtype)
    return buf, buf.view(GUARD, shape)


def read_guarded(buf, shape):
    raw = buf.numpy()
    n = int(np.prod(shape))
    edge = np.concatenate([raw[:GUARD], raw[GUARD + n:]])
    assert (edge.view(np.uint8) == 0xFF).all(), "a store landed in a guard band"
    out = raw[GUARD:GUARD + n].reshape(shape)
    bad = ~np.isfinite(out.astype(f64))
    assert not bad.any(), f"{int(bad.sum())} of {out.size} output elements not finite (first at {tuple(np.argwhere(bad)[0])}): never written, or NaN / inf computed"
    return out


def arith_share(got, want, bound):
    """the normalisations' error / bound reaches 1 wherever the last rounding alone costs half an ulp; this is the share of the REST of the bound, the
    allowance for the arithmetic in front of that rounding, that the error uses: max (err - ulp16(want) / 2) / (bound - ulp16(want) / 2), f16 outputs"""
    if got.dtype != f16:
        return float((np.abs(got.astype(f64) - want) / bound).max())
    half = ulp16(want) / 2
    rest = bound - half                    # (0 where the arithmetic has no allowance: gamma = beta = 0 in a constant group)
    over = np.maximum(np.abs(got.astype(f64) - want) - half, 0.0)
    return float(np.where(rest > 0, over / np.where(rest > 0, rest, 1.0), 0.0).max())


def check(section, cid, got, want, bound, extra=""):
    err = np.abs(got.astype(f64) - want)
    ratio = err / bound
    worst = float(ratio.max())
    share = arith_share(got, want, bound)
    note(section, cid, worst, extra + f"(beyond the last rounding: {share:.3f} of the allowance)")
    if share > WORST.get(section + " beyond the last rounding", (0.0, ""))[0]:
        WORST[section + " beyond the last rounding"] = (share, cid)
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        n = int((ratio > 1.0).sum())
        raise AssertionError(f"{cid}: {n} of {ratio.size} elements outside the bound; worst at {tuple(int(x) for x in i)}: got {float(got[i])!r}, want {want[i]!r}, "
                             f"bound {bound[i]!r} (error / bound {worst:.2f}); first at {tuple(int(x) for x in np.argwhere(ratio > 1.0)[0])}")


# =====================================================================================================================================
# A. attn2_kernel
# =====================================================================================================================================
NST = {40: 4, 64: 3, 80: 3, 160: 3}
UNROLL = {40: 4, 64: 6, 80: 6, 160: 6}
DS = (40, 64, 80, 160)
LAYOUTS = ("heads", "tokens", "kv", "owide", "qkv", "sdpa")


def acase(cid, D, B, H, Tq, Tkv, layout="heads", family="normal", qt=1, seed=0):
    return dict(id=f"D{D}-QT{qt}-{cid}", D=D, B=B, H=H, Tq=Tq, Tkv=Tkv, layout=layout, family=family, qt=qt, seed=seed)


def attn_cases():
    cs = []
    for D in DS:
        u = UNROLL[D]
        # the end of the sweep at every remainder position, full and ragged last tiles; small Tq, a few heads, the layouts in turn
        tiles = list(range(1, u + 3)) + [2 * u, 2 * u + 1]
        i = 0
        for n in tiles:
            for tkv in (64 * n, 64 * n - 63, 64 * n - 1):
                lay = ("heads", "tokens", "kv", "owide")[i % 4]
                tq = (17, 65, 1, 63, 15)[i % 5]
                cs.append(acase(f"tiles{n}-Tkv{tkv}-Tq{tq}-{lay}", D, 1 + i % 2, 2 + i % 3, tq, tkv, lay, seed=i))
                i += 1
        for tkv in (77, 4096):
            cs.append(acase(f"Tkv{tkv}-Tq65-heads", D, 1, 2, 65, tkv, "heads", seed=tkv))
        # QT = 2 (Tq >= 1024 and ceil(Tq / 128) * B * H >= 2 * 256): a subset of the tile counts, Tq = 1024, 64 heads
        for j, n in enumerate(sorted({1, NST[D] - 1, NST[D], u, u + 1, 2 * u + 1})):
            tkv = (64 * n, 64 * n - 63, 64 * n - 1)[j % 3]
            lay = ("tokens", "heads", "kv", "owide")[j % 4]
            cs.append(acase(f"tiles{n}-Tkv{tkv}-Tq1024-{lay}", D, 2, 32, 1024, tkv, lay, qt=2, seed=100 + j))
        # query edges: QT = 1 in the dense and the token layout; QT = 2 with a grid of 8 q + r workgroups, r = 1, 3, 7 (9 * 57, 9 * 59, 9 * 63)
        for tq in (1, 15, 17, 63, 65):
            for lay in ("heads", "tokens"):
                cs.append(acase(f"edge-Tq{tq}-Tkv130-{lay}", D, 2, 3, tq, 130, lay, seed=tq))
        for tq, (b, h) in zip((1025, 1039, 1151), ((1, 57), (1, 59), (3, 21))):
            cs.append(acase(f"edge-Tq{tq}-Tkv77-grid{9 * b * h}-{'tokens' if b > 1 else 'heads'}", D, b, h, tq, 77, "tokens" if b > 1 else "heads", qt=2, seed=tq))
        # grid sizes total = 8 q + r (and total in {1, 7}): which (head, query block) a workgroup computes
        for total, (b, h, tq) in {1: (1, 1, 64), 7: (1, 7, 33), 9: (3, 3, 64), 11: (1, 11, 50), 15: (3, 5, 64), 17: (1, 17, 20), 23: (1, 23, 64), 27: (3, 3, 130),
                                  33: (1, 11, 190), 35: (1, 7, 300)}.items():
            cs.append(acase(f"grid{total}-B{b}-H{h}-Tq{tq}", D, b, h, tq, 100, "tokens" if b > 1 else "heads", seed=total))
        # layouts of the planner: merged QKV (self-attention), merged KV (cross-attention, 77 keys), an output column range, batch 2 and 3; osg_sdpa with Hq / Hkv = 4
        cs.append(acase("qkv-self-T200-B2", D, 2, 4, 200, 200, "qkv", seed=1))
        cs.append(acase("qkv-self-T70-B3", D, 3, 2, 70, 70, "qkv", seed=2))
        cs.append(acase("kv-cross-Tq256-Tkv77-B3", D, 3, 4, 256, 77, "kv", seed=3))
        cs.append(acase("owide-Tq100-Tkv77-B2", D, 2, 4, 100, 77, "owide", seed=4))
        cs.append(acase("sdpa-gqa4-Tq70-Tkv129-B2", D, 2, 8, 70, 129, "sdpa", seed=5))
        cs.append(acase("sdpa-gqa4-Tq1024-Tkv200-B2", D, 2, 32, 1024, 200, "sdpa", qt=2, seed=6))
        # the online softmax
        for fam in ("spike", "max0", "big", "voffset"):
            cs.append(acase(f"{fam}-Tq80-Tkv333", D, 1, 3, 80, 333, "heads", fam, seed=8))
        cs.append(acase("spike-Tq1024-Tkv333", D, 2, 32, 1024, 333, "tokens", "spike", qt=2, seed=8))
        cs.append(acase("voffset-Tq1024-Tkv200", D, 2, 32, 1024, 200, "heads", "voffset", qt=2, seed=9))
    cs.append(acase("qkv-self-T1024-B2", 40, 2, 32, 1024, 1024, "qkv", qt=2, seed=10))
    cs.append(acase("qkv-self-T1024-B2", 64, 2, 32, 1024, 1024, "qkv", qt=2, seed=11))
    return cs


ATTN_CASES = attn_cases()
SPIKE_ROWS = {3: 5, 21: 150, 40: 330, 41: 331, 70: 150}        # query row -> the key that dominates it (first, a middle, the ragged last tile)


def attn_inputs(c):
    """q [B,H,Tq,D], k, v [B,Hkv,Tkv,D] (f16), scale"""
    D, B, H, Tq, Tkv = c["D"], c["B"], c["H"], c["Tq"], c["Tkv"]
    rng = np.random.default_rng(D * 1000 + c["seed"] + Tq + 7 * Tkv)
    hkv = H // 4 if c["layout"] == "sdpa" else H
    sig = 2.0 if c["seed"] % 2 else 1.0
    q = (rng.standard_normal((B, H, Tq, D), dtype=f32) * f32(sig)).astype(f16)
    k = rng.standard_normal((B, hkv, Tkv, D), dtype=f32).astype(f16)
    v = rng.standard_normal((B, hkv, Tkv, D), dtype=f32).astype(f16)
    scale = float(f32(D ** -0.5))
    fam = c["family"]
    if fam == "spike":         # some rows of a wave get a dominating key, their neighbours do not: the rescale sits behind a wave-wide ballot
        for r, j in SPIKE_ROWS.items():
            k[:, :, j] = (q[:, :hkv, r].astype(f32) * (12.0 / (sig ** 2 * D ** 0.5))).astype(f16)       # scale q k ~ 12 on that key
    elif fam == "max0":        # the maxima fall after tile 0: no rescale from tile 1 on
        k[:, :, :64] = (k[:, :, :64].astype(f32) * 4).astype(f16)
    elif fam == "big":         # |scale q k| up to ~30 (20 for D = 160): probabilities that underflow f16
        s = np.abs(np.einsum("bhqd,bhkd->bhqk", q.astype(f64), k.astype(f64))).max() * scale
        q = (q.astype(f64) * ((20.0 if D == 160 else 30.0) / s)).astype(f16)
    elif fam == "voffset":     # sum p v is large while the errors of p matter
        v = (v.astype(f32) + (12.0 if c["seed"] % 2 else -9.0)).astype(f16)
    return q, k, v, scale


def attn_layout(c):
    """operand -> (buffer name, offset, token / head / batch stride) in elements, buffer sizes"""
    D, B, H, Tq, Tkv, lay = c["D"], c["B"], c["H"], c["Tq"], c["Tkv"], c["layout"]
    C = H * D
    dense = lambda T: (D, T * D, H * T * D)
    tok = lambda T: (C, D, T * C)
    if lay in ("heads", "sdpa"):
        hkv = H // 4 if lay == "sdpa" else H
        L = dict(q=("q", 0) + dense(Tq), k=("k", 0, D, Tkv * D, hkv * Tkv * D), v=("v", 0, D, Tkv * D, hkv * Tkv * D), o=("o", GUARD) + dense(Tq))
        return L, dict(q=B * H * Tq * D, k=B * hkv * Tkv * D, v=B * hkv * Tkv * D, o=B * H * Tq * D + 2 * GUARD)
    L = dict(q=("q", 0) + tok(Tq), k=("k", 0) + tok(Tkv), v=("v", 0) + tok(Tkv), o=("o", GUARD) + tok(Tq))
    sizes = dict(q=B * Tq * C, k=B * Tkv * C, v=B * Tkv * C, o=B * Tq * C + 2 * GUARD)
    if lay == "qkv":
        L.update(q=("qkv", 0, 3 * C, D, Tq * 3 * C), k=("qkv", C, 3 * C, D, Tq * 3 * C), v=("qkv", 2 * C, 3 * C, D, Tq * 3 * C))
        sizes = dict(qkv=B * Tq * 3 * C, o=sizes["o"])
    elif lay == "kv":
        L.update(k=("kv", 0, 2 * C, D, Tkv * 2 * C), v=("kv", C, 2 * C, D, Tkv * 2 * C))
        sizes = dict(q=sizes["q"], kv=B * Tkv * 2 * C, o=sizes["o"])
    elif lay == "owide":
        W = C + 24
        L.update(o=("o", GUARD + 8, W, D, Tq * W))
        sizes["o"] = B * Tq * W + 2 * GUARD
    return L, sizes


def strided_index(shape, off, tok, head, batch):
    B, H, T, D = shape
    return (off + np.arange(B)[:, None, None, None] * batch + np.arange(H)[None, :, None, None] * head + np.arange(T)[None, None, :, None] * tok + np.arange(D))


def run_attention(gpu, dev, c, q, k, v, scale):
    L, sizes = attn_layout(c)
    rng = np.random.default_rng(c["seed"])
    host = {n: rng.standard_normal(sz, dtype=f32).astype(f16) for n, sz in sizes.items() if n != "o"}      # (what lies between the operands is finite noise)
    for name, x in (("q", q), ("k", k), ("v", v)):
        buf, off, tok, head, batch = L[name]
        host[buf][strided_index(x.shape, off, tok, head, batch)] = x
    d = {n: dev(a) for n, a in host.items()}
    obuf = dev.nan(sizes["o"])
    B, H, Tq, D = q.shape
    if c["layout"] == "sdpa":
        gpu.sdpa(d["q"].view(0, q.shape), d["k"].view(0, k.shape), d["v"].view(0, v.shape), None, scale, out=obuf.view(GUARD, q.shape))
    else:
        arg = lambda n, b: (b.ptr + 2 * L[n][1],) + L[n][2:]
        gpu.attention_strided(arg("q", d[L["q"][0]]), arg("k", d[L["k"][0]]), arg("v", d[L["v"][0]]), arg("o", obuf), B, H, Tq, k.shape[2], D, scale)
    rec = gpu.last_kernel()
    raw = obuf.numpy()
    idx = strided_index(q.shape, *L["o"][1:])
    untouched = np.ones(raw.shape, bool)
    untouched[idx] = False
    assert (raw.view(np.uint16)[untouched] == 0xFFFF).all(), "a store landed outside the output (guard band, column gap, rows past Tq or columns past D)"
    got = raw[idx]
    bad = ~np.isfinite(got.astype(f64))
    assert not bad.any(), f"{int(bad.sum())} of {got.size} output elements not finite (first at {tuple(np.argwhere(bad)[0])}): never written, or NaN / inf computed"
    return got, rec


def attn_rows(T):
    """all rows of a small case; else the rows either side of every 16-, 64- and 128-row boundary, the first and the last ones"""
    if T <= 320:
        return np.arange(T)
    r = set(range(8)) | set(range(T - 40, T))
    for b in range(16, T, 16):
        r |= {b - 1, b}
    return np.array(sorted(r))


def attn_heads(B, H, Tq):
    """every head of a small case (at most 8192 query rows in all); else the first and the last head of every image and one in between"""
    if B * H * Tq <= 8192:
        return [(b, h) for b in range(B) for h in range(H)]
    return sorted({(b, h) for b in range(B) for h in (0, H // 2 + b, H - 1)})


def attn_exact(q, k, v, scale, ntiles):
    """one head: q [R,D], k, v [S,D] (f16) -> float64 want [R,D], bound [R,D], c_eff [R,D] (see the module docstring, A)"""
    D = q.shape[1]
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
    eps = math.log(2) * U24 * (D * c * sabs + 3 * np.abs(t).max(axis=1) + 3 * np.abs(m) * c) + 2.0 ** -22 * (1 + ntiles)
    aw = A + np.abs(want)
    E = (H11 + eps[:, None] + (35 + 3 * ntiles) * U24) * aw + 2.0 ** -25 * (sub @ np.abs(v) + np.abs(want) * sub.sum(axis=1, keepdims=True)) / P
    E = E * (1 + 2.0 ** -8)
    bound = E + ulp16(np.abs(want) + E) / 2
    return want, bound, (1 + 2.0 ** -8) * (H11 + eps[:, None] + (35 + 3 * ntiles) * U24) * aw / (H11 * A)      # the c of c 2^-11 A (without the underflow term)


def emulate_attn2(q, k, v, scale):
    """the arithmetic attn2_kernel declares, one head, in numpy: f32 scores, 64-key tiles, running maximum, f16 probabilities summed as they are"""
    c = f32(f32(scale) * f32(LOG2E))
    s = q.astype(f32) @ k.astype(f32).T
    R, S = s.shape
    m_run = np.full(R, -np.inf, f32)
    l = np.zeros(R, f32)
    o = np.zeros((R, v.shape[1]), f32)
    with np.errstate(invalid="ignore"):
        for kv0 in range(0, S, 64):
            st = s[:, kv0:kv0 + 64]
            m_new = np.maximum(m_run, st.max(axis=1))
            mc = (-m_new * c).astype(f32)
            alpha = np.where(np.isinf(m_run), 0.0, np.exp2(((m_run - m_new) * c).astype(f32).astype(f64))).astype(f32)
            p = np.exp2((st.astype(f64) * f64(c) + mc[:, None].astype(f64)).astype(f32).astype(f64)).astype(f32).astype(f16)
            l = (l * alpha + p.astype(f32).sum(axis=1, dtype=f32)).astype(f32)
            o = (o * alpha[:, None] + p.astype(f32) @ v[kv0:kv0 + 64].astype(f32)).astype(f32)
            m_run = m_new
    return (o * (f32(1) / l)[:, None]).astype(f16)


def attn_compare(c, q, k, v, scale, fn):
    """fn(b, h, rows) -> f16 [rows, D] of head (b, h); compared with float64 per element.  -> worst error / bound, worst c_eff"""
    B, H, Tq, D = q.shape
    r = H // k.shape[1]
    rows = attn_rows(Tq)
    ntiles = -(-k.shape[2] // 64)
    worst, ceff, fail = 0.0, 0.0, None
    for b, h in attn_heads(B, H, Tq):
        want, bound, ce = attn_exact(q[b, h, rows], k[b, h // r], v[b, h // r], scale, ntiles)
        ratio = np.abs(fn(b, h, rows).astype(f64) - want) / bound
        ceff = max(ceff, float(ce.max()))
        if ratio.max() > worst:
            worst = float(ratio.max())
            i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            fail = f"image {b} head {h} row {int(rows[i])} d {int(j)}: want {want[i, j]!r}, bound {bound[i, j]!r}, {int((ratio > 1).sum())} elements of this head outside"
    return worst, ceff, fail


@pytest.mark.parametrize("c", ATTN_CASES, ids=[c["id"] for c in ATTN_CASES])
def test_attn2(gpu, dev, c):
    q, k, v, scale = attn_inputs(c)
    got, rec = run_attention(gpu, dev, c, q, k, v, scale)
    RECORDS["attn:" + c["id"]] = rec
    nqb = -(-c["Tq"] // (64 * c["qt"]))
    assert rec[:7] == (ATTENTION, 2, c["D"], NST[c["D"]], c["qt"], 64, nqb * c["B"] * c["H"]), rec
    worst, ceff, fail = attn_compare(c, q, k, v, scale, lambda b, h, rows: got[b, h][rows])
    note("A", c["id"], worst, f"c_eff {ceff:.2f}")
    assert worst <= 1.0, f"{c['id']}: error / bound {worst:.2f} at {fail}"


# =====================================================================================================================================
# B / C. normalisation: inputs, float64 references and bounds
# =====================================================================================================================================
def family_rows(rng, n_rows, n, dtype, first=0):
    """[n_rows, n] values, the family by row (first + row) % 5: N(0,1); N(mu, s) with |mu| / s = 8; = 32; constant; N(0,1) with one outlier of +-60000"""
    x = rng.standard_normal((n_rows, n))
    for r in range(n_rows):
        fam = (first + r) % 5
        sgn = -1.0 if (r // 5) % 2 else 1.0
        s = (0.25, 0.5, 1.0)[r % 3]
        if fam == 1:
            x[r] = x[r] * s + sgn * 8 * s
        elif fam == 2:
            x[r] = x[r] * s + sgn * 32 * s
        elif fam == 3:
            x[r] = sgn * (0.25, 0.75, -0.5)[r % 3]
        elif fam == 4:
            x[r, int(rng.integers(n))] = sgn * 60000.0
    return x.astype(dtype)


def affine(rng, C, dtype):
    """gamma with negative and zero entries, beta up to +-4"""
    g = rng.standard_normal(C) * 1.0
    g[rng.random(C) < 0.1] = 0.0
    b = rng.uniform(-4, 4, C)
    return g.astype(dtype), b.astype(dtype)


def silu64(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def rstd_error(dvar, var, eps):
    lo = np.minimum(dvar, var) / (var + eps)            # (the kernels clamp the variance at 0)
    return np.maximum(1.0 / np.sqrt(1.0 - lo) - 1.0, 1.0 - 1.0 / np.sqrt(1.0 + dvar / (var + eps))) + 3 * U24


def finish_bound(want, pre, E_pre, act, out_dtype):
    E = 1.1 * E_pre + (3.5 + 0.65 * np.abs(pre)) * 2.0 ** -23 * np.abs(want) if act else E_pre
    E = E * (1 + 2.0 ** -8)
    return E + ulp16(np.abs(want) + E) / 2 if out_dtype == f16 else E + 2.0 ** -149


def norm_exact(xg, gam, bet, eps, g, onepass, act=0, out_dtype=f16, extra_s1=0.0, extra_s2=0.0):
    """xg [..., groups, n] float64 rows to normalise, gam / bet broadcastable to it -> want, bound (module docstring B, C).
    extra_s1 / extra_s2: further absolute errors of mean and E[x^2] (the fixed-point partials of the producer statistics)"""
    mean = xg.mean(axis=-1, keepdims=True)
    var = xg.var(axis=-1, keepdims=True)
    eabs = np.abs(xg).mean(axis=-1, keepdims=True)
    dmean = U24 * (g * eabs + 2 * np.abs(mean)) + extra_s1
    if onepass:
        dvar = U24 * ((g + 4) * (var + mean * mean) + 2 * np.abs(mean) * (g * eabs + 2 * np.abs(mean))) + extra_s2 + 2 * np.abs(mean) * extra_s1
    else:
        dvar = U24 * (g + 4) * var + dmean * dmean
    rho = rstd_error(dvar, var, eps)
    a = gam / np.sqrt(var + eps)
    pre = (xg - mean) * a + bet
    if onepass:
        E_pre = np.abs(pre - bet) * (rho + 2 * U24) + np.abs(a) * (dmean + 3 * U24 * np.abs(mean)) + 2 * U24 * (np.abs(bet) + np.abs(pre))
    else:
        E_pre = np.abs(pre - bet) * (rho + 4 * U24) + np.abs(a) * dmean + 2 * U24 * (np.abs(bet) + np.abs(pre))
    want = silu64(pre) if act else pre
    return want, finish_bound(want, pre, E_pre, act, out_dtype)


def lane_sums(x, lanes):
    """sum over the last axis as `lanes` strided f32 running sums (sequential), the lanes added in float64"""
    n = x.shape[-1]
    pad = (-n) % lanes
    xp = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), x.dtype)], axis=-1).reshape(x.shape[:-1] + (-1, lanes))
    return np.cumsum(xp, axis=-2, dtype=f32)[..., -1, :].astype(f64).sum(axis=-1, keepdims=True)


def emulate_onepass(xg, gam, bet, eps, act, out_dtype=f16, lanes=256):
    """GroupNorm as the kernels declare it: f32 running sums of x and x^2, E[x^2] - mean^2 in f64, f32 from there on"""
    x32 = xg.astype(f32)
    n = xg.shape[-1]
    icnt = f64(f32(1.0) / f32(n))
    mean = lane_sums(x32, lanes) * icnt
    q = lane_sums((x32.astype(f64) ** 2).astype(f32), lanes) * icnt          # (per-term rounding instead of the fma: no better than the kernel)
    var = np.maximum((q - mean * mean).astype(f32), f32(0))
    rstd = (f32(1) / np.sqrt(var + f32(eps), dtype=f32)).astype(f32)
    a = (rstd * gam.astype(f32)).astype(f32)
    b = (bet.astype(f32) - (mean.astype(f32) * a).astype(f32)).astype(f32)
    y = (x32.astype(f64) * a.astype(f64) + b.astype(f64)).astype(f32)
    if act:
        y = (y.astype(f64) * (1.0 / (1.0 + np.exp(-y.astype(f64)))).astype(f32).astype(f64)).astype(f32)
    return y.astype(out_dtype)


def emulate_twopass(xg, gam, bet, eps, out_dtype=f16, lanes=64):
    x32 = xg.astype(f32)
    n = xg.shape[-1]
    mean = (lane_sums(x32, lanes).astype(f32) / f32(n)).astype(f32)
    d = (x32 - mean).astype(f32)
    var = (lane_sums((d * d).astype(f32), lanes).astype(f32) / f32(n)).astype(f32)
    rstd = (f32(1) / np.sqrt(var + f32(eps), dtype=f32)).astype(f32)
    return ((((d * rstd).astype(f32) * gam.astype(f32)).astype(f32)) + bet.astype(f32)).astype(f32).astype(out_dtype)


# ---- B. GroupNorm -------------------------------------------------------------------------------------------------------------------
def gcase(cid, C, G, N, HW, route, nv=0, nt=256, gb=0, S=None, act=1, dtype=f16, env=None, first=0):
    return dict(id=cid, C=C, G=G, N=N, HW=HW, route=route, nv=nv, nt=nt, gb=gb, S=S, act=act, dtype=dtype, env=env or {}, first=first)


OFF = {"OSG_GN_SLAB_OFF": "1", "OSG_GN_CLUSTER_OFF": "1"}
MIN_NV = {"OSG_GN_CLUSTER_MIN_NV": "1"}
GN_CASES = [
    # one-block slab kernel: (NV, threads) over the block sizes, groups per block 1 / 2 / 4 / 8 (cpg 8; 12, 20; 10, 30; 9), HW in {1, 2, RT - 1, RT + 1, prime, odd * 2}
    gcase("slab-C64-G8-HW1", 64, 8, 1, 1, SLAB, 1, 256, 1, act=0),                               # G = C / 8
    gcase("slab-C512-G64-HW2-N3", 512, 64, 3, 2, SLAB, 1, 256, 1),
    gcase("slab-C8-G1-HW255", 8, 1, 2, 255, SLAB, 1, 256, 1, first=2),                           # RT - 1 (RT = 256)
    gcase("slab-C8-G1-HW257", 8, 1, 1, 257, SLAB, 2, 256, 1, act=0, first=1),                     # RT + 1
    gcase("slab-C8-G1-HW4096", 8, 1, 1, 4096, SLAB, 4, 1024, 1, first=4),
    gcase("slab-C96-G8-HW84", 96, 8, 2, 84, SLAB, 1, 256, 2),                                    # cpg 12: RT = 85
    gcase("slab-C96-G8-HW86", 96, 8, 1, 86, SLAB, 2, 256, 2, act=0),
    gcase("slab-C96-G8-HW681", 96, 8, 1, 681, SLAB, 2, 1024, 2),                                 # (the integer division of RT lets 1024 threads take 2 vectors)
    gcase("slab-C192-G16-HW2", 192, 16, 3, 2, SLAB, 1, 256, 2),
    gcase("slab-C160-G8-HW101", 160, 8, 1, 101, SLAB, 2, 256, 2),                                # cpg 20, a prime
    gcase("slab-C160-G8-HW103", 160, 8, 2, 103, SLAB, 4, 256, 2, act=0),
    gcase("slab-C1280-G64-HW202", 1280, 64, 1, 202, SLAB, 4, 256, 2),                            # odd * 2
    gcase("slab-C320-G32-HW64", 320, 32, 2, 64, SLAB, 2, 256, 4),                                # cpg 10: the UNet's 8x8
    gcase("slab-C320-G32-HW256", 320, 32, 2, 256, SLAB, 4, 512, 4),                              # 16x16
    gcase("slab-C320-G32-HW1024", 320, 32, 1, 1024, SLAB, 8, 1024, 4),                           # 32x32
    gcase("slab-C640-G64-HW50", 640, 64, 3, 50, SLAB, 1, 256, 4, act=0),                         # RT - 1 (RT = 51)
    gcase("slab-C640-G64-HW52", 640, 64, 1, 52, SLAB, 2, 256, 4),
    gcase("slab-C960-G32-HW34", 960, 32, 1, 34, SLAB, 2, 256, 4),                                # cpg 30, odd * 2
    gcase("slab-C960-G32-HW67", 960, 32, 2, 67, SLAB, 4, 256, 4, act=0),                         # a prime
    gcase("slab-C960-G32-HW544", 960, 32, 1, 544, SLAB, 8, 1024, 4),
    gcase("slab-C240-G8-HW271", 240, 8, 1, 271, SLAB, 4, 1024, 4),                               # a prime
    gcase("slab-C72-G8-HW27", 72, 8, 3, 27, SLAB, 1, 256, 8),                                    # cpg 9: RT = 28
    gcase("slab-C72-G8-HW29", 72, 8, 1, 29, SLAB, 2, 256, 8, act=0),
    gcase("slab-C576-G64-HW113", 576, 64, 1, 113, SLAB, 4, 512, 8),                              # a prime
    gcase("slab-C72-G8-HW227", 72, 8, 2, 227, SLAB, 4, 1024, 8),
    gcase("slab-C576-G64-HW454", 576, 64, 1, 454, SLAB, 8, 1024, 8, act=0),                      # odd * 2
    gcase("slab-C56-G1-HW145", 56, 1, 1, 145, SLAB, 2, 512, 1, first=1),
    # cluster kernel: S = 16, 8, 4, 2 as the CU count allows
    gcase("cluster-C320-G32-N2-HW4096", 320, 32, 2, 4096, CLUSTER, 4, 512, 4, 16),               # the UNet's 64x64
    gcase("cluster-C320-G32-N3-HW4096", 320, 32, 3, 4096, CLUSTER, 4, 1024, 4, 8, act=0),
    gcase("cluster-C640-G64-N3-HW1640", 640, 64, 3, 1640, CLUSTER, 4, 1024, 4, 4),
    gcase("cluster-C1280-G64-N3-HW1634", 1280, 64, 3, 1634, CLUSTER, 8, 1024, 2, 2),
    gcase("cluster-C72-G8-N1-HW7248", 72, 8, 1, 7248, CLUSTER, 8, 1024, 8, 16, act=0),
    gcase("cluster-C72-G8-N1-HW912", 72, 8, 1, 912, CLUSTER, 4, 256, 8, 16),
    gcase("cluster-C8-G1-N1-HW8194", 8, 1, 1, 8194, CLUSTER, 8, 1024, 1, 2, first=2),
    # ... and, with OSG_GN_CLUSTER_MIN_NV = 1, the slabs the one-block kernel would take: NV = 1 and 2
    gcase("cluster-minnv-C72-G8-HW16", 72, 8, 1, 16, CLUSTER, 1, 256, 8, 16, env=MIN_NV),
    gcase("cluster-minnv-C96-G8-HW1376", 96, 8, 1, 1376, CLUSTER, 2, 256, 2, 16, env=MIN_NV, act=0),
    gcase("cluster-minnv-C80-G8-HW8", 80, 8, 1, 8, CLUSTER, 1, 256, 4, 8, env=MIN_NV),
    gcase("cluster-minnv-C8-G1-HW1028", 8, 1, 1, 1028, CLUSTER, 2, 256, 1, 4, env=MIN_NV, first=1),
    gcase("cluster-minnv-C1280-G64-N3-HW102", 1280, 64, 3, 102, CLUSTER, 1, 256, 2, 2, env=MIN_NV),
    # three passes
    gcase("three-C64-G32-HW15", 64, 32, 2, 15, THREE_FOLD, S=1),                                 # cpg 2 < 8
    gcase("three-C64-G32-HW4099", 64, 32, 1, 4099, THREE_FOLD, S=16, act=0),
    gcase("three-off-C2560-G32-HW64", 2560, 32, 1, 64, THREE_FOLD, S=8, env=OFF),                # C > 2048: the second channel sweep of the statistics
    gcase("three-off-C2560-G32-N3-HW2801", 2560, 32, 3, 2801, THREE_FINALIZE, S=64, env=OFF, act=0),   # slabs * N = 1050 > 1024: gn_finalize_kernel
    gcase("three-off-C320-G32-HW77", 320, 32, 2, 77, THREE_FOLD, S=1, env=OFF),                  # a vector that straddles two groups
    gcase("three-C8-G1-HW1048577", 8, 1, 1, (1 << 20) + 1, THREE_FOLD, S=64),                  # past the slab plans' HW limit; 64 statistics slabs
    gcase("three-C8-G1-HW16385", 8, 1, 1, 16385, THREE_FOLD, S=8, first=2),                      # the same chain of ~2000 additions in the fold, small enough for the CPU emulation
    gcase("three-f32-C320-G32-HW77", 320, 32, 2, 77, THREE_F32, S=3, dtype=f32),
    gcase("three-f32-C36-G3-HW1000", 36, 3, 1, 1000, THREE_F32, S=4, dtype=f32, act=0),
]
GN_EPS = 1e-5


def gn_inputs(c):
    C, G, N, HW = c["C"], c["G"], c["N"], c["HW"]
    rng = np.random.default_rng(C * 7 + G + N * 3 + HW)
    cpg = C // G
    rows = family_rows(rng, N * G, HW * cpg, c["dtype"], c["first"])                       # one row per (image, group)
    x = np.ascontiguousarray(rows.reshape(N, G, HW, cpg).transpose(0, 2, 1, 3)).reshape(N, HW, C)
    gam, bet = affine(rng, C, c["dtype"])
    return x, gam, bet


def gn_chain(c, rec):
    """the longest chain of f32 additions behind a group's sums, from the launch record (module docstring, B)"""
    if rec[1] in (SLAB, CLUSTER):
        return rec[2] + 16
    V = 8 if c["dtype"] == f16 else 4
    cols = min(c["C"] // V, 256)
    R = 256 // cols
    rows = -(-c["HW"] // (rec[5] * R)) + 1
    return rows + min(c["C"] // c["G"], cols * V) * R + 4 + (2 if c["dtype"] == f32 else 0)


def gn_reference(c, x, gam, bet, g, **kw):
    N, HW, C = x.shape
    G = c["G"]
    cpg = C // G
    xg = x.astype(f64).reshape(N, HW, G, cpg).transpose(0, 2, 1, 3).reshape(N, G, HW * cpg)
    gg = np.broadcast_to(gam.astype(f64).reshape(1, G, 1, cpg), (N, G, HW, cpg)).reshape(N, G, HW * cpg)
    bb = np.broadcast_to(bet.astype(f64).reshape(1, G, 1, cpg), (N, G, HW, cpg)).reshape(N, G, HW * cpg)
    want, bound = norm_exact(xg, gg, bb, float(f32(GN_EPS)), g, True, c["act"], x.dtype, **kw)
    back = lambda t: t.reshape(N, G, HW, cpg).transpose(0, 2, 1, 3).reshape(N, HW, C)
    return back(want), back(bound)


@pytest.mark.parametrize("c", GN_CASES, ids=[c["id"] for c in GN_CASES])
def test_group_norm(gpu, dev, c, monkeypatch):
    for kn in ("OSG_GN_SLAB_OFF", "OSG_GN_CLUSTER_OFF", "OSG_GN_CLUSTER_WAIT", "OSG_GN_CLUSTER_MIN_NV"):
        monkeypatch.delenv(kn, raising=False)
    for kn, val in c["env"].items():
        monkeypatch.setenv(kn, val)
    x, gam, bet = gn_inputs(c)
    N, HW, C = x.shape
    dx, dg, db = dev(x.reshape(N, HW, 1, C)), dev(gam), dev(bet)
    buf, out = guarded(dev, (N, HW, 1, C), x.dtype)
    gpu.group_norm_nhwc(dx, dg, db, c["G"], GN_EPS, c["act"], out=out)
    rec = gpu.last_kernel()
    RECORDS["gn:" + c["id"]] = rec
    got = read_guarded(buf, (N, HW, C))
    if c["route"] in (SLAB, CLUSTER):
        assert rec[:6] == (GROUPNORM, c["route"], c["nv"], c["nt"], c["gb"], c["S"] or 1), rec
    else:
        assert rec[:4] == (GROUPNORM, c["route"], 0, 256) and rec[5] == c["S"], rec
    want, bound = gn_reference(c, x, gam, bet, gn_chain(c, rec))
    check("B", c["id"], got, want, bound)
    if c["route"] == CLUSTER:      # nobody waits: every block recomputes its peers' partials -- the same bits
        monkeypatch.setenv("OSG_GN_CLUSTER_WAIT", "0")
        buf2, out2 = guarded(dev, (N, HW, 1, C), x.dtype)
        gpu.group_norm_nhwc(dx, dg, db, c["G"], GN_EPS, c["act"], out=out2)
        assert gpu.last_kernel() == rec
        solo = read_guarded(buf2, (N, HW, C))
        assert np.array_equal(solo.view(np.uint16), got.view(np.uint16)), "OSG_GN_CLUSTER_WAIT=0 gave other bits"


STATS_CASES = [(1, 16, 16, 64, 96, 3, 8, 0), (2, 32, 32, 320, 640, 1, 32, 1), (2, 64, 64, 320, 320, 3, 32, 1)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,G,act", STATS_CASES, ids=[f"stats-v1-N{s[0]}-{s[1]}x{s[2]}-C{s[3]}-{s[4]}-k{s[5]}-G{s[6]}" for s in STATS_CASES])
def test_group_norm_producer_statistics(gpu, dev, N, H, W, Cin, Cout, k, G, act):
    """gn_apply_kernel<f16, 2>: the statistics are the int64 fixed-point sums the producing convolution's epilogue left (osg_set_stat_sinks); the reference
    is float64 GroupNorm of the tensor the convolution stored"""
    cid = f"stats-v1-{H}x{W}-C{Cout}-G{G}"
    rng = np.random.default_rng(N + H + Cin + Cout + k)
    x = rng.standard_normal((N, H, W, Cin)).astype(f16)
    w = (rng.standard_normal((Cout, k, k, Cin)) * (k * k * Cin) ** -0.5).astype(f16)
    bias = (rng.standard_normal(Cout) * 0.3 + np.repeat(rng.uniform(-6, 6, G), Cout // G)).astype(f16)      # (groups with a common offset)
    gam, bet = affine(rng, Cout, f16)
    table = dev(np.zeros((8, N, G, 2), np.int64))
    wide = dev(np.zeros((N, H, W, Cout), f16))
    gpu.set_stat_sinks(H * W, table, G, Cout // G, 0)
    gpu.conv2d_nhwc_view(dev(x), dev(w), dev(bias), wide, 0, None, 1, (k // 2,) * 4)
    y = wide.numpy().reshape(N, H * W, Cout)
    buf, out = guarded(dev, (N, H, W, Cout))
    gpu.group_norm_stats_nhwc(wide, dev(gam), dev(bet), G, GN_EPS, table, act=act, out=out)
    rec = gpu.last_kernel()
    RECORDS["gn:" + cid] = rec
    assert rec[:6] == (GROUPNORM, STATS_V1, 0, 256, 0, 1), rec
    got = read_guarded(buf, (N, H * W, Cout))
    n = H * W * (Cout // G)
    qscale = 2.0 ** min(20, max(10, 36 - int(np.ceil(np.log2(n)))))
    parts = H * W / 8
    c = dict(G=G, act=act)
    want, bound = gn_reference(c, y, gam, bet, 256, extra_s1=parts * 2.0 ** -21 / n, extra_s2=parts * 0.5 / qscale / n)
    check("B", cid, got, want, bound)


# ---- C. LayerNorm, InstanceNorm --------------------------------------------------------------------------------------------------------
LN_CS = (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2040, 2048, 2056, 30)
LN_CASES = [(C, rows, f16) for C in LN_CS for rows in (1, 3, 4, 5)] + [(C, 4097, f16) for C in (8, 520, 1024, 1544, 2048, 2056, 30)] + \
           [(C, rows, f32) for C, rows in ((30, 3), (512, 5), (2052, 4), (320, 4097))]


@pytest.mark.parametrize("C,rows,dtype", LN_CASES, ids=[f"ln-C{c}-rows{r}-{np.dtype(d).name}" for c, r, d in LN_CASES])
def test_layer_norm(gpu, dev, C, rows, dtype):
    cid = f"ln-C{C}-rows{rows}-{np.dtype(dtype).name}"
    rng = np.random.default_rng(C * 5 + rows + (dtype == f32))
    x = family_rows(rng, rows, C, dtype, first=C % 5)
    gam, bet = affine(rng, C, dtype)
    buf, out = guarded(dev, (rows, C), dtype)
    gpu.layer_norm(dev(x), dev(gam), dev(bet), GN_EPS, out=out)
    rec = gpu.last_kernel()
    RECORDS["ln:" + cid] = rec
    nv = -(-C // 512) if dtype == f16 and C % 8 == 0 and C <= 2048 else 0
    assert rec[:3] == (LAYERNORM, nv, OSG_F16 if dtype == f16 else OSG_F32), rec
    got = read_guarded(buf, (rows, C))
    g = 8 * nv + 6 if nv else -(-C // 256) + 12
    want, bound = norm_exact(x.astype(f64), gam.astype(f64), bet.astype(f64), float(f32(GN_EPS)), g, False, 0, dtype)
    check("C", cid, got, want, bound)


IN_OPTS = ("scale-bias", "bias-only", "scale-only", "plain")
# the full product: each of the four operand options with N = 1 and N = 3 (rows = N * G > n_scale = G), in both dtypes, at every L (both block sizes)
IN_CASES = [(L, N, dtype, opt) for L in (1, 255, 8191, 8192, 40960) for N in (1, 3) for dtype in (f16, f32) for opt in range(4)]


IN_G = 5


def in_first(L, N, opt):
    return L + N + opt


def in_inputs(L, N, dtype, opt):
    """x [N * G, L], scale [G] or None, bias [G] or None (opt: an index into IN_OPTS), and the float64 per-row gamma / beta they mean: row r takes
    scale[r % G] and bias[r % G]"""
    rng = np.random.default_rng(L * 16 + N * 8 + opt * 2 + (dtype == f32))
    x = family_rows(rng, N * IN_G, L, dtype, first=in_first(L, N, opt))
    sc = (rng.standard_normal(IN_G) * 1.5).astype(f32) if opt in (0, 2) else None
    bi = rng.uniform(-4, 4, IN_G).astype(f32) if opt in (0, 1) else None
    gam = np.tile(sc if sc is not None else np.ones(IN_G), N).astype(f64)[:, None]
    bet = np.tile(bi if bi is not None else np.zeros(IN_G), N).astype(f64)[:, None]
    return x, sc, bi, gam, bet


@pytest.mark.parametrize("L,N,dtype,opt", IN_CASES, ids=[f"in-L{L}-N{N}-{np.dtype(d).name}-{IN_OPTS[o]}" for L, N, d, o in IN_CASES])
def test_instance_norm(gpu, dev, L, N, dtype, opt):
    """rows = N * G with n_scale = G, as the host calls it for a GroupNorm over N images: row r takes scale[r % G] and bias[r % G] where the case has
    them (with neither operand there is nothing to index and the wrapper passes n_scale = 1)"""
    cid = f"in-L{L}-N{N}-{np.dtype(dtype).name}-{IN_OPTS[opt]}"
    x, sc, bi, gam, bet = in_inputs(L, N, dtype, opt)
    buf, out = guarded(dev, (N * IN_G, L), dtype)
    gpu.instance_norm(dev(x), dev(sc) if sc is not None else None, dev(bi) if bi is not None else None, GN_EPS, out=out)
    rec = gpu.last_kernel()
    RECORDS["in:" + cid] = rec
    threads = 1024 if L >= 8192 else 256
    assert rec[:3] == (INSTANCENORM, threads, OSG_F16 if dtype == f16 else OSG_F32), rec
    got = read_guarded(buf, (N * IN_G, L))
    want, bound = norm_exact(x.astype(f64), gam, bet, float(f32(GN_EPS)), -(-L // threads) + 24, False, 0, dtype)
    check("C", cid, got, want, bound)


# =====================================================================================================================================
# D. coverage
# =====================================================================================================================================
GN_WANTED = ([("slab (NV, threads)", (SLAB, nv, nt)) for nv, nt in ((1, 256), (2, 256), (4, 256), (2, 512), (4, 512), (2, 1024), (4, 1024), (8, 1024))] +
             [("slab groups per block", (SLAB, "gb", gb)) for gb in (1, 2, 4, 8)] +
             [("cluster NV", (CLUSTER, "nv", nv)) for nv in (1, 2, 4, 8)] + [("cluster S", (CLUSTER, "S", s)) for s in (16, 8, 4, 2)] +
             [("route", (r,)) for r in (THREE_FOLD, THREE_FINALIZE, THREE_F32, STATS_V1)])


def test_coverage():
    """the records of the cases above: fails, naming what is missing, where a listed kernel or plan was not reached on this device.
    It reads RECORDS, which the cases of this module fill as they run: it has to run after them in the same process (file order, as pytest runs a module),
    and it fails, on purpose, under a -k selection, a reordering or a distribution over processes that gives it less than the whole module"""
    missing = []
    attn = {r[2:5] for k, r in RECORDS.items() if k.startswith("attn:") and r[:2] == (ATTENTION, 2)}
    missing += [f"attn2_kernel<{D}, {qt}, {NST[D]}>" for D in DS for qt in (1, 2) if (D, NST[D], qt) not in attn]
    gn = [r for k, r in RECORDS.items() if k.startswith("gn:")]
    have = set()
    for r in gn:
        have |= {(r[1],), (r[1], r[2], r[3]), (r[1], "gb", r[4]), (r[1], "nv", r[2]), (r[1], "S", r[5])}
    missing += [f"GroupNorm {what} {key}" for what, key in GN_WANTED if key not in have]
    ln = {r[1:3] for k, r in RECORDS.items() if k.startswith("ln:")}
    missing += [f"LayerNorm NV {nv} dtype {dt}" for nv, dt in ((1, OSG_F16), (2, OSG_F16), (3, OSG_F16), (4, OSG_F16), (0, OSG_F16), (0, OSG_F32)) if (nv, dt) not in ln]
    inn = {r[1:3] for k, r in RECORDS.items() if k.startswith("in:")}
    missing += [f"InstanceNorm {t} threads dtype {dt}" for t in (256, 1024) for dt in (OSG_F16, OSG_F32) if (t, dt) not in inn]
    for sec, (ratio, cid) in sorted(WORST.items()):
        print(f"[{sec}] worst error / bound over the section: {ratio:.3f} ({cid})")
    assert not missing, "not reached: " + "; ".join(missing)


# =====================================================================================================================================
# the CPU emulations over the inputs of every case (no GPU): `python tests/test_unet_attention_norm.py`
# =====================================================================================================================================
def emulate_all():
    worst, c_max = {}, [0.0, ""]

    def keep(fam, ratio, cid):
        if ratio > worst.get(fam, (0, ""))[0]:
            worst[fam] = (ratio, cid)

    for c in ATTN_CASES:
        q, k, v, scale = attn_inputs(c)
        r = q.shape[1] // k.shape[1]
        w, ceff, fail = attn_compare(c, q, k, v, scale, lambda b, h, rows: emulate_attn2(q[b, h, rows], k[b, h // r], v[b, h // r], scale))
        keep("A " + c["family"] + (" Tkv4096" if c["Tkv"] == 4096 else ""), w, c["id"] + f" c_eff {ceff:.2f}")
        assert w <= 1.0, (c["id"], w, fail)
        if ceff > c_max[0]:
            c_max[:] = [ceff, c["id"]]
    for c in GN_CASES:
        if c["HW"] * c["C"] * c["N"] > 1 << 23:
            continue
        x, gam, bet = gn_inputs(c)
        N, HW, C = x.shape
        G, cpg = c["G"], C // c["G"]
        rec = (GROUPNORM, c["route"], c["nv"], c["nt"], c["gb"], c["S"] or 1)
        want, bound = gn_reference(c, x, gam, bet, gn_chain(c, rec))
        xg = x.reshape(N, HW, G, cpg).transpose(0, 2, 1, 3).reshape(N, G, HW * cpg)
        gg = np.broadcast_to(gam.reshape(1, G, 1, cpg), (N, G, HW, cpg)).reshape(N, G, HW * cpg)
        bb = np.broadcast_to(bet.reshape(1, G, 1, cpg), (N, G, HW, cpg)).reshape(N, G, HW * cpg)
        # (three passes: as many running sums as make each as long as the kernel's longest chain; the slab kernels' chains are shorter than n / 256)
        lanes = 256 if c["route"] in (SLAB, CLUSTER) else max(1, HW * cpg // gn_chain(c, rec))
        got = emulate_onepass(xg, gg, bb, GN_EPS, c["act"], x.dtype, lanes).reshape(N, G, HW, cpg).transpose(0, 2, 1, 3).reshape(N, HW, C)
        ratio = np.abs(got.astype(f64) - want) / bound
        fam = np.broadcast_to(((np.arange(N * G) + c["first"]) % 5).reshape(N, 1, G, 1), (N, HW, G, cpg)).reshape(N, HW, C)
        for f_ in range(5):
            keep(f"B family {f_}", float(ratio[fam == f_].max()) if (fam == f_).any() else 0.0, c["id"])
        keep("B beyond the last rounding", arith_share(got, want, bound), c["id"])
        assert ratio.max() <= 1.0, (c["id"], float(ratio.max()))
    for C, rows, dtype in LN_CASES:
        rng = np.random.default_rng(C * 5 + rows + (dtype == f32))
        x = family_rows(rng, rows, C, dtype, first=C % 5)
        gam, bet = affine(rng, C, dtype)
        nv = -(-C // 512) if dtype == f16 and C % 8 == 0 and C <= 2048 else 0
        want, bound = norm_exact(x.astype(f64), gam.astype(f64), bet.astype(f64), float(f32(GN_EPS)), 8 * nv + 6 if nv else -(-C // 256) + 12, False, 0, dtype)
        got = emulate_twopass(x, gam, bet, GN_EPS, dtype)
        ratio = np.abs(got.astype(f64) - want) / bound
        keep("C beyond the last rounding", arith_share(got, want, bound), f"ln-C{C}-rows{rows}")
        fam = (np.arange(rows) + C % 5) % 5
        for f_ in range(5):
            keep(f"C family {f_}", float(ratio[fam == f_].max()) if (fam == f_).any() else 0.0, f"ln-C{C}-rows{rows}")
        assert ratio.max() <= 1.0, (C, rows, float(ratio.max()))
    for L, N, dtype, opt in IN_CASES:
        x, sc, bi, gam, bet = in_inputs(L, N, dtype, opt)
        threads = 1024 if L >= 8192 else 256
        want, bound = norm_exact(x.astype(f64), gam, bet, float(f32(GN_EPS)), -(-L // threads) + 24, False, 0, dtype)
        got = emulate_twopass(x, gam, bet, GN_EPS, dtype, lanes=threads)
        ratio = np.abs(got.astype(f64) - want) / bound
        keep("C beyond the last rounding", arith_share(got, want, bound), f"in-L{L}-N{N}-{np.dtype(dtype).name}")
        fam = (np.arange(N * IN_G) + in_first(L, N, opt)) % 5
        for f_ in range(5):
            keep(f"C family {f_}", float(ratio[fam == f_].max()) if (fam == f_).any() else 0.0, f"in-L{L}-N{N}-{np.dtype(dtype).name}")
        assert ratio.max() <= 1.0, (L, N, dtype, float(ratio.max()))
    for name, (ratio, cid) in sorted(worst.items()):
        print(f"  {name:24s} {ratio:.3f}   ({cid})")
    print(f"  the largest c of c 2^-11 A: {c_max[0]:.2f} ({c_max[1]})")
    return worst, c_max[0]


if __name__ == "__main__":
    emulate_all()
