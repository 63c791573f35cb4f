"""-m gpu: the kernels of the decoder (LLM) flow against float64 restatements written here, at TinyLlama / Mistral shapes and at the
edges where the kernels branch.

A. Attention (osg_sdpa, osg_attention_strided -> dispatch_attn / launch_attn in osg_attention.hip): the 128-row (QT=2) form of
   attn_kernel, every attn_kernel instantiation <DP, DT>, grouped-query heads, decode, and masks whose first key tile is fully masked
   (-65504 and -inf).  Reference: softmax(scale q k^T + mask) v in float64, query head h reading key/value head h // (Hq / Hkv).
B. The fp32 ("upcast") elementwise and row-reduction kernels the host lowers a flagged RMSNorm chain onto (osg_binary, osg_unary,
   osg_reduce_mean_last with OSG_F32), the grid-stride loops and tails of the elementwise kernels, osg_rms_norm and osg_softmax_last (f16).

Every output is pre-filled with NaN (all bytes 0xFF) before the call, so an element the kernel never writes fails the comparison.  Every
case is seeded and frees its device buffers when it ends.
"""
import math

import numpy as np
import pytest

from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
U24 = 2.0 ** -24          # unit roundoff of f32 (half an ulp at 1.0)
NEG = f16(-65504.0)       # the f16 minimum, as the exporters write a causal mask

# launch_attn takes the 128-row form (QT=2) when Tq >= 1024 and ceil(Tq / 128) * batch * heads >= 2 * num_cu.  The cases meant to reach it
# satisfy that for any device of up to 512 CUs (MI355X has 256): ceil(2048 / 128) * 2 * 32 = 16 * 64 = 1024 = 2 * 512.
MAX_CU = 512


def reaches_qt2(T, B, H):
    return T >= 1024 and -(-T // 128) * B * H >= 2 * MAX_CU


@pytest.fixture
def dev(gpu):
    """device buffers of one case: uploads, NaN-filled outputs; all freed when the case ends"""
    held = []

    class Dev:
        def __call__(self, arr):
            b = gpu.to_dev(arr)
            held.append(b)
            return b

        def nan(self, shape, dtype):
            b = gpu.empty(shape, dtype)
            held.append(b)
            gpu.memset(b, 0xFF)     # f16 0xFFFF / f32 0xFFFFFFFF: NaN
            return b

    yield Dev()
    for b in held:
        b.free()


def ulp16(x):
    """spacing of f16 at |x| (subnormal spacing 2^-24 near 0)"""
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f16)).astype(f64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    u = np.uint16 if got.dtype == f16 else np.uint32
    return np.array_equal(got.view(u), want.view(u))


# =====================================================================================================================================
# A. attention
# =====================================================================================================================================
def attn_exact(q, k, v, mask, scale, heads, rows):
    """float64 softmax(scale q k^T + mask) v of q [B,Hq,T,D], k / v [B,Hkv,S,D], mask [T,S] (or None), for the query heads `heads`
    ((b, h) pairs) and the query rows `rows`, over ALL keys -> [len(heads), len(rows), D]"""
    r = q.shape[1] // k.shape[1]
    out = []
    for b, h in heads:
        kv = h // r
        s = scale * (q[b, h, rows].astype(f64) @ k[b, kv].astype(f64).T)
        if mask is not None:
            s = s + mask[rows].astype(f64)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        out.append((e / e.sum(axis=1, keepdims=True)) @ v[b, kv].astype(f64))
    return np.stack(out)


def sample_rows(T):
    """all rows of a small case; else the first 256, both sides of every 128-row block boundary and the last 300"""
    if T <= 600:
        return np.arange(T)
    r = set(range(256)) | set(range(T - 300, T))
    for b in range(128, T, 128):
        r |= {b - 1, b}
    return np.array(sorted(r))


def sample_heads(B, Hq, Hkv, full):
    """every head of a small case; else every query head of two key/value groups (the first of image 0, the last of the last image)"""
    if full:
        return [(b, h) for b in range(B) for h in range(Hq)]
    r = Hq // Hkv
    return [(0, h) for h in range(r)] + [(B - 1, h) for h in range(Hq - r, Hq)]


def check_attention(got, q, k, v, mask, scale, valid=None, bound=2e-3):
    """got, q: [B,Hq,T,D]; valid: query rows with at least one visible key (others have no softmax and are not compared)"""
    B, Hq, T, D = q.shape
    S = k.shape[2]
    valid = np.ones(T, bool) if valid is None else valid
    assert np.isfinite(got[:, :, valid]).all(), "non-finite (or unwritten) output on a row with a visible key"
    full = B * Hq * T * S * D <= (1 << 28)
    rows = sample_rows(T) if not full else np.arange(T)
    rows = rows[valid[rows]]
    heads = sample_heads(B, Hq, k.shape[1], full)
    want = attn_exact(q, k, v, mask, scale, heads, rows)
    g = np.stack([got[b, h][rows] for b, h in heads]).astype(f64)
    err = np.abs(g - want).max() / np.abs(want).max()
    assert err <= bound, err


def qkv(rng, B, Hq, Hkv, T, S, D):
    q = rng.standard_normal((B, Hq, T, D), dtype=f32).astype(f16)
    k = rng.standard_normal((B, Hkv, S, D), dtype=f32).astype(f16)
    v = rng.standard_normal((B, Hkv, S, D), dtype=f32).astype(f16)
    return q, k, v


def causal_mask(rng, T, S, neg=NEG, window=None, left_pad=0):
    """additive [T,S] mask as test_osg_sdpa_kernel writes it: causal over the last T of S positions (query i sees keys j <= S - T + i),
    a finite bias (0.5 N(0,1)) on the visible keys, `neg` elsewhere; optionally only the last `window` keys of each row, and the first
    `left_pad` keys of every row masked.  -> mask, visible rows"""
    i = np.arange(T)[:, None]
    j = np.arange(S)[None, :]
    vis = j <= S - T + i
    if window is not None:
        vis &= j > S - T + i - window
    vis &= j >= left_pad
    mask = np.where(vis, (rng.standard_normal((T, S), dtype=f32) * 0.5).astype(f16), f16(neg)).astype(f16)
    return mask, vis.any(axis=1)


def run_sdpa(gpu, dev, q, k, v, mask, scale):
    o = dev.nan(q.shape, f16)
    gpu.sdpa(dev(q), dev(k), dev(v), dev(mask) if mask is not None else None, scale, out=o)
    return o.numpy()


def scale_of(D):
    return float(f32(D ** -0.5))


# ---- QT=2 masked prefill --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hq,Hkv,T,S,D", [
    pytest.param(2, 32, 8, 2048, 2048, 128, id="attn_kernel<128,8,QT2>-mistral-gqa4"),
    pytest.param(2, 32, 4, 2048, 2048, 64, id="attn_kernel<64,4,QT2>-tinyllama-gqa8"),
    pytest.param(2, 32, 8, 1921, 1921 + 37, 128, id="attn_kernel<128,8,QT2>-ragged-T1921-past37"),
])
def test_sdpa_qt2_masked_prefill(gpu, dev, B, Hq, Hkv, T, S, D):
    """masked prefill long enough for the 128-row form: the QT=2 mask-row indexing (q0 + qt*16 + lq), its GQA head mapping and its
    online-softmax rescale; the ragged case has partial last query and key tiles"""
    assert reaches_qt2(T, B, Hq)
    rng = np.random.default_rng(B * 7 + Hq + Hkv * 3 + T + S + D)
    q, k, v = qkv(rng, B, Hq, Hkv, T, S, D)
    mask, valid = causal_mask(rng, T, S)
    got = run_sdpa(gpu, dev, q, k, v, mask, scale_of(D))
    check_attention(got, q, k, v, mask, scale_of(D), valid)


# ---- QT=2 unmasked, token layout --------------------------------------------------------------------------------------------------
def tokens(x):
    """[B,H,T,D] -> [B,T,H*D] (the projections' layout)"""
    B, H, T, D = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(B, T, H * D))


def heads_of(x, H):
    B, T, C = x.shape
    return x.reshape(B, T, H, C // H).transpose(0, 2, 1, 3)


def run_tokens(gpu, dev, q, k, v, scale):
    """attention_tokens on [B,T,H*D]: a store past D lands in the neighbouring head (or the next token's head 0)"""
    H = q.shape[1]
    qt = tokens(q)
    o = dev.nan(qt.shape, f16)
    gpu.attention_tokens(dev(qt), dev(tokens(k)), dev(tokens(v)), H, scale, out=o)
    return heads_of(o.numpy(), H)


def test_tokens_qt2_unmasked(gpu, dev):
    """attn_kernel<128,8,QT2>, no mask, token layout: B=2, 32 heads, Tq = Tkv = 2048, D = 128"""
    B, H, T, D = 2, 32, 2048, 128
    assert reaches_qt2(T, B, H)
    rng = np.random.default_rng(2048)
    q, k, v = qkv(rng, B, H, H, T, T, D)
    got = run_tokens(gpu, dev, q, k, v, scale_of(D))
    check_attention(got, q, k, v, None, scale_of(D))


# ---- every attn_kernel instantiation ----------------------------------------------------------------------------------------------
# dispatch_attn: D <= 32 -> <32,2>, <= 48 -> <64,3>, <= 64 -> <64,4>, <= 80 -> <96,5>, <= 96 -> <96,6>, <= 128 -> <128,8>, <= 160 -> <160,10>;
# unmasked D in {40, 64, 80, 160} go to attn2_kernel instead, so none of these head dims is one of them.  Tq = 70 < 1024: QT=1.
INST = {8: "<32,2>", 24: "<32,2>", 48: "<64,3>", 56: "<64,4>", 72: "<96,5>", 88: "<96,6>", 96: "<96,6>", 112: "<128,8>", 136: "<160,10>",
        152: "<160,10>"}
VARIANTS = ["sdpa-mask-gqa1", "sdpa-mask-gqa4", "sdpa-nomask-gqa4", "tokens-nomask"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", list(INST), ids=[f"D{d}-attn_kernel{i}-QT1" for d, i in INST.items()])
def test_attn_kernel_instantiations(gpu, dev, D, variant):
    """ragged Tq = 70, Tkv = 129 (a partial query tile and a 1-key last key tile) for every instantiation, masked and unmasked"""
    B, Tq, Tkv = 2, 70, 129
    Hq, Hkv = (4, 4) if variant in ("sdpa-mask-gqa1", "tokens-nomask") else (8, 2)
    rng = np.random.default_rng(D * 10 + VARIANTS.index(variant))
    q, k, v = qkv(rng, B, Hq, Hkv, Tq, Tkv, D)
    scale = scale_of(D)
    if variant == "tokens-nomask":
        got = run_tokens(gpu, dev, q, k, v, scale)
        check_attention(got, q, k, v, None, scale)
        return
    mask, valid = causal_mask(rng, Tq, Tkv) if "nomask" not in variant else (None, None)
    got = run_sdpa(gpu, dev, q, k, v, mask, scale)
    check_attention(got, q, k, v, mask, scale, valid)


# ---- decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("S", [1, 64, 65, 4097])
@pytest.mark.parametrize("Hq,Hkv,D", [pytest.param(32, 8, 128, id="mistral-attn_kernel<128,8,QT1>"),
                                      pytest.param(32, 4, 64, id="tinyllama-attn_kernel<64,4,QT1>-masked-or-attn2<64,QT1>-unmasked")])
def test_sdpa_decode(gpu, dev, Hq, Hkv, D, S, masked):
    """one query row against S keys (the KV cache), finite additive bias when masked"""
    rng = np.random.default_rng(S * 3 + D + masked)
    q, k, v = qkv(rng, 1, Hq, Hkv, 1, S, D)
    mask = (rng.standard_normal((1, S), dtype=f32) * 0.5).astype(f16) if masked else None
    got = run_sdpa(gpu, dev, q, k, v, mask, scale_of(D))
    check_attention(got, q, k, v, mask, scale_of(D))


# ---- rows whose first key tile is fully masked ------------------------------------------------------------------------------------
# Before the safe maximum in attn_kernel's online softmax, a -inf mask gave NaN on these rows: m_run = m_new = -inf made
# alpha = exp2(NaN) and fma(-inf, c, +inf) = NaN.  -65504 takes the finite path.
MASKED_SHAPES = [
    pytest.param(1, 8, 2, 600, 64, id="attn_kernel<64,4,QT1>-T600"),
    pytest.param(1, 8, 2, 600, 128, id="attn_kernel<128,8,QT1>-T600"),
    pytest.param(2, 32, 8, 2048, 64, id="attn_kernel<64,4,QT2>-T2048"),
]


@pytest.mark.parametrize("neg", [float(NEG), -math.inf], ids=["neg65504", "neginf"])
@pytest.mark.parametrize("kind", ["window100", "leftpad70"])
@pytest.mark.parametrize("B,Hq,Hkv,T,D", MASKED_SHAPES)
def test_sdpa_first_key_tile_fully_masked(gpu, dev, B, Hq, Hkv, T, D, kind, neg):
    """causal + a sliding window of 100 keys (rows >= 164 see none of keys 0-63), or causal + 70 left-padding keys (every row's first
    tile is masked; rows < 70 see no key at all and are excluded)"""
    if T >= 1024:
        assert reaches_qt2(T, B, Hq)
    rng = np.random.default_rng(T + D + len(kind) + (neg == -math.inf))
    q, k, v = qkv(rng, B, Hq, Hkv, T, T, D)
    mask, valid = causal_mask(rng, T, T, neg=neg, window=100 if kind == "window100" else None, left_pad=70 if kind == "leftpad70" else 0)
    assert (mask[valid][:, :64] <= NEG).all(axis=1).sum() >= T // 2      # most compared rows start with a fully masked tile
    got = run_sdpa(gpu, dev, q, k, v, mask, scale_of(D))
    check_attention(got, q, k, v, mask, scale_of(D), valid)


# =====================================================================================================================================
# B. fp32 elementwise / row reductions, loops, RMSNorm, softmax
# =====================================================================================================================================
def f32_normal(rng, shape, lo=-8, hi=8):
    """normal f32 numbers with random signs and binary exponents in [lo, hi): no zeros, subnormals, overflow in add / mul / div"""
    m = rng.uniform(1.0, 2.0, shape)
    e = rng.integers(lo, hi, shape)
    s = rng.choice([-1.0, 1.0], shape)
    return (s * m * np.exp2(e)).astype(f32)


def np_binary(kind, a, b):
    """f32 operands, one IEEE op (numpy rounds f32 add / sub / mul / div correctly), one RNE rounding to the storage type"""
    a32, b32 = a.astype(f32), b.astype(f32)
    y = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[kind](a32, b32)
    return y.astype(a.dtype)


def binary_operands(rng, kind, ash, bsh, dtype=f32):
    lo, hi = (-8, 8) if dtype == f32 else (-6, 6)      # (f16: products and quotients stay inside the f16 range)
    a = f32_normal(rng, ash, lo, hi)
    b = f32_normal(rng, bsh, lo, hi)
    if kind == "div":
        b = np.abs(b)           # |b| >= 2^lo: bounded away from 0
    return a.astype(dtype), b.astype(dtype)


def run_binary(gpu, dev, kind, a, b):
    osh = np.broadcast_shapes(a.shape, b.shape)
    y = dev.nan(osh, a.dtype)
    gpu.binary(kind, dev(a), dev(b), out=y)
    return y.numpy()


# which branch of run_binary (osg_elementwise.hip) each f32 shape pair takes (V = 4 f32 per 16-byte vector)
BIN_F32_SHAPES = [
    pytest.param((1, 77, 2048), (1, 77, 2048), id="mode0-same"),
    pytest.param((7,), (7,), id="mode0-same-n7-tail3"),
    pytest.param((2, 77, 5), (), id="mode1-b-scalar"),
    pytest.param((), (7, 1), id="mode3-a-scalar-div1-sqrt"),
    pytest.param((333, 4), (4,), id="mode2-per4(f16-bcast)"),
    pytest.param((100, 12), (12,), id="mode2-per12(f16-bcast)"),
    pytest.param((9, 4096), (4096,), id="mode2-per4096"),
    pytest.param((4,), (333, 4), id="mode4-per4(f16-bcast)"),
    pytest.param((12,), (100, 12), id="mode4-per12(f16-bcast)"),
    pytest.param((4096,), (9, 4096), id="mode4-per4096"),
    pytest.param((1, 77, 2048), (1, 77, 1), id="bcast-row-scale"),
    pytest.param((3, 1, 5), (1, 4, 1), id="bcast-both"),
    pytest.param((50, 6), (6,), id="bcast-per6"),
]


@pytest.mark.parametrize("kind", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("ash,bsh", BIN_F32_SHAPES)
def test_binary_f32_bit_exact(gpu, dev, kind, ash, bsh):
    rng = np.random.default_rng(len(ash) * 100 + len(bsh) * 10 + int(np.prod(ash)) + int(np.prod(bsh)))
    a, b = binary_operands(rng, kind, ash, bsh)
    got = run_binary(gpu, dev, kind, a, b)
    assert bits_equal(got, np_binary(kind, a, b))


@pytest.mark.parametrize("kind", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("which", ["a", "y"])
def test_binary_f32_misaligned_falls_back_to_bcast(gpu, dev, kind, which):
    """a or y 4 bytes off a 16-byte boundary: run_binary leaves the vector kernels for binary_bcast_kernel (same shape, per 4)"""
    rng = np.random.default_rng(7 + len(kind) + (which == "y"))
    n = 4099
    a, b = binary_operands(rng, kind, (n,), (n,))
    abuf = dev(np.concatenate([f32_normal(rng, (1,)), a]))     # a lives at offset 4 bytes when which == "a"
    bbuf = dev(b)
    ybuf = dev.nan((n + 1,), f32)
    a_ptr = abuf.ptr + 4 if which == "a" else dev(a).ptr
    y_ptr = ybuf.ptr + 4 if which == "y" else ybuf.ptr
    gpu.binary_at(kind, f32, a_ptr, (n,), bbuf.ptr, (n,), y_ptr)
    y = ybuf.numpy()
    got = y[1:] if which == "y" else y[:n]
    assert bits_equal(got, np_binary(kind, a, b))
    if which == "y":
        assert np.isnan(y[0])           # nothing written in front of y
    else:
        assert np.isnan(y[n])           # nothing written past y


# ---- fp32 unary -------------------------------------------------------------------------------------------------------------------
def run_unary(gpu, dev, kind, x, param=0.0):
    y = dev.nan(x.shape, x.dtype)
    gpu.unary(kind, dev(x), param, out=y)
    return y.numpy()


@pytest.mark.parametrize("kind,param", [("sqrt", 0.0), ("neg", 0.0), ("pow", 2.0)])
def test_unary_f32_bit_exact(gpu, dev, kind, param):
    """sqrtf is correctly rounded (hipcc's default), neg is exact, pow with 2 is one multiply"""
    rng = np.random.default_rng(11 + len(kind))
    x = f32_normal(rng, (100003,), -20, 20)
    if kind == "sqrt":
        x = np.abs(x)
    want = {"sqrt": lambda: np.sqrt(x), "neg": lambda: -x, "pow": lambda: x * x}[kind]()
    assert bits_equal(run_unary(gpu, dev, kind, x, param), want)


@pytest.mark.parametrize("kind,param", [("pow", 3.0), ("pow", 0.5), ("erf", 0.0), ("sin", 0.0), ("cos", 0.0)])
def test_unary_f32_within_4_ulps(gpu, dev, kind, param):
    """libm-class functions: within 4 f32 ulps of the float64 value rounded to f32, for 2^-10 <= |x| <= 100"""
    rng = np.random.default_rng(13 + int(param * 4) + len(kind))
    x = (rng.choice([-1.0, 1.0], 200000) * np.exp2(rng.uniform(-10, math.log2(100), 200000))).astype(f32)
    if kind == "pow" and param == 0.5:
        x = np.abs(x)
    x64 = x.astype(f64)
    want = {"pow": lambda: x64 ** param, "erf": lambda: np.vectorize(math.erf)(x64), "sin": lambda: np.sin(x64),
            "cos": lambda: np.cos(x64)}[kind]()
    got = run_unary(gpu, dev, kind, x, param).astype(f64)
    w32 = want.astype(f32).astype(f64)
    ulps = np.abs(got - w32) / ulp32(w32)
    assert np.isfinite(got).all() and ulps.max() <= 4, (ulps.max(), x[np.argmax(ulps)])


# osg_sigmoid(x) = v_rcp_f32(1 + v_exp_f32(x * -1.44269504f)).  Relative errors, first order, in units of 2^-23:
#   the exponent t = x * c: c is log2(e) rounded to f32 (relative error 1.34e-8 = 0.11 * 2^-23) and the product rounds once (<= 0.5 * 2^-23),
#   so |dt| <= 0.61 * 2^-23 * |x| * log2(e), and 2^(t + dt) = 2^t (1 + ln2 dt) moves e by <= 0.61 |x| * 2^-23 relative;
#   v_exp_f32 and v_rcp_f32 are each accurate to 1 ulp (<= 2^-23 relative); 1 + e rounds once (<= 0.5 * 2^-23); a relative error r of e
#   moves 1 / (1 + e) by r * e / (1 + e) <= r.  Sum: (2.5 + 0.61 |x|) * 2^-23; the test allows (3 + 0.65 |x|) * 2^-23 for the second-order terms.
#   |x| <= 80 keeps sigmoid(x) >= 1.8e-35 a normal f32 (below x = -87.3 the true value is subnormal and the kernel returns 0).
# silu = x * sigmoid(x): one more rounding, + 0.5 * 2^-23.
# gelu_erf = (0.5 x) * (1 + erff(x * 0.70710678f)): 0.5 x is exact; the argument's two roundings move erf by <= 0.63 * 2^-24 absolute
#   (max of (2 / sqrt(pi)) z exp(-z^2) times 1.3 * 2^-24); erff within 4 ulps of a value below 1 is <= 4 * 2^-24 absolute; the add and the
#   final multiply round once each (<= 2^-24 relative of the result).  |err| <= 0.5 |x| * 4.7 * 2^-24 + 2 * 2^-24 |y|
#   = (1.18 |x| + |y|) * 2^-23: absolute in |x|, because 1 + erf cancels for negative x.  The test allows (1.25 |x| + 1.5 |y|) * 2^-23.
def _sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))       # (|x| <= 100: no overflow in float64, no cancellation)


@pytest.mark.parametrize("kind", ["sigmoid", "silu", "gelu_erf"])
def test_unary_f32_activation_bounds(gpu, dev, kind):
    rng = np.random.default_rng(17 + len(kind))
    lim = 80.0 if kind != "gelu_erf" else 100.0
    x = np.concatenate([rng.uniform(-lim, lim, 100000), rng.standard_normal(100000) * 3]).astype(f32)
    x64 = x.astype(f64)
    erf = np.vectorize(math.erf)
    want = {"sigmoid": lambda: _sigmoid64(x64), "silu": lambda: x64 * _sigmoid64(x64),
            "gelu_erf": lambda: 0.5 * x64 * (1.0 + erf(x64 / math.sqrt(2.0)))}[kind]()
    got = run_unary(gpu, dev, kind, x).astype(f64)
    ax = np.abs(x64)
    if kind == "gelu_erf":
        tol = (1.25 * ax + 1.5 * np.abs(want)) * 2.0 ** -23
    else:
        tol = (3.0 + 0.65 * ax + (0.5 if kind == "silu" else 0.0)) * 2.0 ** -23 * np.abs(want)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= tol).all(), (float((err / tol).max()), x[np.argmax(err / tol)])


# ---- grid-stride loops and vector tails -------------------------------------------------------------------------------------------
# grid_for caps a launch at 2048 blocks x 256 threads: one sweep of the vector kernels covers 2048 * 256 * V elements (V = 8 f16, 4 f32),
# so n = 2 sweeps + r runs the loop twice and leaves r elements to the scalar tail; the broadcast kernel sweeps 2048 * 256 elements.
def vec(dtype):
    return 8 if dtype == f16 else 4


def loop_sizes(dtype):
    V = vec(dtype)
    sweep = 2048 * 256 * V
    return [2 * sweep + 1, 2 * sweep + V - 1, 1, V - 1, V + 1]


SIZE_CASES = [pytest.param(dt, i, id=f"{np.dtype(dt).name}-{['2sweeps+1', '2sweeps+V-1', 'n1', 'nV-1', 'nV+1'][i]}")
              for dt in (f16, f32) for i in range(5)]


@pytest.mark.parametrize("dtype,which", SIZE_CASES)
def test_unary_loop_and_tail(gpu, dev, dtype, which):
    n = loop_sizes(dtype)[which]
    rng = np.random.default_rng(n)
    x = np.abs(f32_normal(rng, (n,), -6, 6)).astype(dtype)
    want = np.sqrt(x.astype(f32)).astype(dtype)         # the kernel's contract: f32 op, one RNE rounding
    assert bits_equal(run_unary(gpu, dev, "sqrt", x), want)


@pytest.mark.parametrize("mode", ["mode0", "mode1", "mode3", "bcast-misaligned-y"])
@pytest.mark.parametrize("dtype,which", SIZE_CASES)
def test_binary_loop_and_tail(gpu, dev, dtype, which, mode):
    """the fast kernel's modes 0 / 1 / 3 at the loop sizes, and binary_bcast_kernel at the same n (y one element off a 16-byte boundary)"""
    n = loop_sizes(dtype)[which]
    rng = np.random.default_rng(n + len(mode))
    ash, bsh = {"mode0": ((n,), (n,)), "mode1": ((n,), (1,)), "mode3": ((1,), (n,)), "bcast-misaligned-y": ((n,), (n,))}[mode]
    a, b = binary_operands(rng, "mul", ash, bsh, dtype)
    if mode != "bcast-misaligned-y":
        assert bits_equal(run_binary(gpu, dev, "mul", a, b), np_binary("mul", a, b))
        return
    ybuf = dev.nan((n + 1,), dtype)
    gpu.binary_at("mul", dtype, dev(a).ptr, ash, dev(b).ptr, bsh, ybuf.ptr + np.dtype(dtype).itemsize)
    y = ybuf.numpy()
    assert np.isnan(y[0]) and bits_equal(y[1:], np_binary("mul", a, b))


@pytest.mark.parametrize("dtype", [f16, f32], ids=["f16", "f32"])
@pytest.mark.parametrize("case", ["mode2-per4096", "mode4-per4096", "bcast-row"])
def test_binary_large_periodic_and_bcast(gpu, dev, dtype, case):
    """periodic operands over 2.5 vector sweeps (a partial third sweep); the broadcast kernel over 16 sweeps"""
    V = vec(dtype)
    rows = (5 * 2048 * 256 * V) // (2 * 4096) + 3
    ash, bsh = {"mode2-per4096": ((rows, 4096), (4096,)), "mode4-per4096": ((4096,), (rows, 4096)),
                "bcast-row": ((1, 4097, 2049), (1, 4097, 1))}[case]
    rng = np.random.default_rng(rows + len(case))
    a, b = binary_operands(rng, "sub", ash, bsh, dtype)
    assert bits_equal(run_binary(gpu, dev, "sub", a, b), np_binary("sub", a, b))


# ---- osg_reduce_mean_last ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 2048])
@pytest.mark.parametrize("C", [1, 63, 2048, 4096, 11008])
@pytest.mark.parametrize("dtype", [f32, f16], ids=["f32", "f16"])
def test_reduce_mean_last(gpu, dev, dtype, C, rows):
    """one wave per row: lane l sums x[l], x[l + 64], ... in order, then a 6-level xor tree, then / C.
    f32 bound: ceil(C/64) - 1 roundings in a lane, 6 in the tree, 1 in the division, each <= 2^-24 of a partial sum bounded by
    sum|x|: |err| <= (ceil(C/64) + 6) * 2^-24 * mean|x| (first order); allowed (ceil(C/64) + 8) * 2^-24 * mean|x|, with cancelling rows.
    f16: the f32 mean is ~1e-5 relative off at worst here (rows offset away from 0), then one RNE rounding: <= 1 f16 ulp."""
    rng = np.random.default_rng(C * 10 + rows + (dtype == f16))
    if dtype == f32:
        x = (rng.standard_normal((rows, C)) * np.exp2(rng.integers(-4, 4, (rows, 1)))).astype(f32)   # means near 0: cancellation
    else:
        off = rng.choice([-1.0, 1.0], (rows, 1)) * rng.uniform(0.5, 4.0, (rows, 1))
        x = (off + 0.5 * rng.standard_normal((rows, C))).astype(f16)
    y = dev.nan((rows, 1), dtype)
    gpu.reduce_mean_last(dev(x), out=y)
    got = y.numpy()[:, 0].astype(f64)
    x64 = x.astype(f64)
    want = x64.mean(axis=1)
    assert np.isfinite(got).all()
    if dtype == f32:
        tol = (math.ceil(C / 64) + 8) * U24 * np.abs(x64).mean(axis=1)
    else:
        tol = ulp16(want)
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())


# ---- RMSNorm ----------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


def rms_exact(x, w, eps):
    x64 = x.astype(f64)
    return w.astype(f64) * x64 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + eps)


def rms_inputs(rng, rows, C):
    x = (rng.standard_normal((rows, C), dtype=f32) * 3.0).astype(f16)
    w = (1 + rng.standard_normal(C, dtype=f32) * 0.1).astype(f16)
    return x, w


@pytest.mark.parametrize("rows", [1, 7, 2048])
@pytest.mark.parametrize("C", [2048, 4096])
def test_rms_norm_chain_f32(gpu, dev, C, rows):
    """The seven-op chain the host lowers a flagged RMSNorm onto with m_requires_upcast (fp32 operands from the f16 input):
        p = Pow(x, 2)            osg_unary pow 2
        m = ReduceMean(p, -1)    osg_reduce_mean_last f32
        a = Add(m, eps)          osg_binary mode 1 (b scalar)
        s = Sqrt(a)              osg_unary sqrt
        r = Div(1, s)            osg_binary mode 3 (a scalar)
        t = Mul(x, r)            osg_binary bcast [rows,C] x [rows,1] (mode 1 when rows = 1)
        y = Mul(w, t)            osg_binary mode 4 (a periodic, period C)
    Bound, relative to float64, u = 2^-24: the squares round once (u) and the mean adds (ceil(C/64) + 6) u (test_reduce_mean_last; all
    terms positive, so relative to the mean itself); + eps: u; sqrt halves that and rounds once: u; Div, Mul, Mul: u each.  First order:
    ((ceil(C/64) + 8) / 2 + 4) u = (ceil(C/64) / 2 + 8) u; allowed (ceil(C/64) / 2 + 9) u: 41 u = 20.5 f32 ulps at worst for C = 4096."""
    rng = np.random.default_rng(C + rows)
    x16, w16 = rms_inputs(rng, rows, C)
    x, w = x16.astype(f32), w16.astype(f32)
    dx, dw = dev(x), dev(w)
    p = dev.nan((rows, C), f32)
    gpu.unary("pow", dx, 2.0, out=p)
    m = dev.nan((rows, 1), f32)
    gpu.reduce_mean_last(p, out=m)
    a = dev.nan((rows, 1), f32)
    gpu.binary("add", m, dev(np.array(EPS, f32)), out=a)
    s = dev.nan((rows, 1), f32)
    gpu.unary("sqrt", a, out=s)
    r = dev.nan((rows, 1), f32)
    gpu.binary("div", dev(np.array(1.0, f32)), s, out=r)
    t = dev.nan((rows, C), f32)
    gpu.binary("mul", dx, r, out=t)
    y = dev.nan((rows, C), f32)
    gpu.binary("mul", dw, t, out=y)
    got = y.numpy().astype(f64)
    want = rms_exact(x, w, float(f32(EPS)))
    tol = (math.ceil(C / 64) / 2 + 9) * U24 * np.abs(want)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("rows", [1, 7, 2048])
@pytest.mark.parametrize("C", [2048, 4096])
def test_rms_norm_f16_within_one_ulp(gpu, dev, C, rows):
    """osg_rms_norm: the f32 result is within ~(C/256 + 12) 2^-24 relative of float64 (sum of squares, mean, eps, sqrt, 1/, two multiplies),
    far below half an f16 ulp (2^-11 relative): one RNE rounding leaves it within 1 f16 ulp of float64"""
    rng = np.random.default_rng(C * 3 + rows)
    x, w = rms_inputs(rng, rows, C)
    y = dev.nan((rows, C), f16)
    gpu.rms_norm(dev(x), dev(w), EPS, out=y)
    got = y.numpy().astype(f64)
    want = rms_exact(x, w, float(f32(EPS)))
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= ulp16(want)).all(), float((err / ulp16(want)).max())


# ---- osg_softmax_last (f16) -------------------------------------------------------------------------------------------------------
def softmax_exact(x):
    x64 = x.astype(f64)
    e = np.exp(x64 - x64.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("special", [False, True], ids=["plain", "neg65504-neginf"])
@pytest.mark.parametrize("S", [1, 77, 2049, 4097])
def test_softmax_last_f16(gpu, dev, S, special):
    """decoder-like rows; `special` rows also hold -65504 and -inf entries (at least one entry finite, -65504 counting as finite).
    f16(e) * f16(1/sum) rounds three times (<= 1.5 ulp relative to the product, all below 1): allowed 1 f16 ulp + 2^-11 absolute"""
    rows = 64
    rng = np.random.default_rng(S * 2 + special)
    x = (rng.standard_normal((rows, S), dtype=f32) * 3.0).astype(f16)
    if special:
        x[rng.random((rows, S)) < 0.3] = NEG
        x[rng.random((rows, S)) < 0.3] = -np.inf
        x[np.arange(rows), rng.integers(0, S, rows)] = f16(1.5)      # one finite entry per row at least
        x[0, :] = NEG                                                 # only -65504 (and -inf): uniform over the -65504 entries
        x[0, rng.random(S) < 0.5] = -np.inf
        x[0, 0] = NEG
        if S > 1:
            x[1, :] = -np.inf
            x[1, S // 2] = f16(0.25)                                  # one visible entry: probability 1
    y = dev.nan((rows, S), f16)
    gpu.softmax_last(dev(x), out=y)
    got = y.numpy()
    assert np.isfinite(got).all()
    want = ref.softmax_last(x)
    assert np.abs(got.astype(f64) - want.astype(f64)).max() <= 2e-3 * np.abs(want.astype(f64)).max()
    p = softmax_exact(x)
    assert (np.abs(got.astype(f64) - p) <= ulp16(p) + 2.0 ** -11).all()
