"""-m gpu: every instantiation of the contraction kernels against float64, element by element -- each gemm2_kernel entry (kV2Entries) and conv3x3_kernel
entry (kV3Entries) of onnxstream_amd/csrc/osg_gemm_routes.h, every tile of the round-1 gemm_kernel that launch_cfg picks, and conv_cin4_mfma_kernel.

* The entries are read from the header through tests/cpp/contraction_routes.cpp (the driver of the CPU test): one case per entry, named after it, reached by
  a request that the driver's resolution maps onto it.  Every launch asserts with osg_last_route that exactly that entry ran, with the k-slices, fold and
  reduce kernel the case asks for: an entry added to the table without a working case here fails the suite.
* Each output lies inside one Gpu.empty allocation (every byte 0xFF: NaN in f16 and f32) between guard bands; output views leave a column gap.  Guards and
  gap must come back bit-identical, every output element finite.
* Bounds, per element.  A kernel forms each output as one f32 sum of K f16 products (exact in f32; uint8 codes enter as the exact q - zp) and the epilogue
  operands, in some order (k-slices, wave groups and the reduce launch only change the tree), then rounds once to f16.  A sum of n terms in f32 errs by at
  most (n - 1) 2^-24 S, S the sum of their absolute values: with bias and residual E = (K + 3) 2^-24 S (one slack term); a per-image bias and the scale of
  uint8 codes add one rounding each.  The f16 rounding (relative 2^-11) of a value within E of want gives
      |got - want| <= 2^-11 |want| + (1 + 2^-11) E + 2^-25          (2^-25: half the smallest f16 subnormal).
  act_apply widens E for SiLU and GEGLU, ln_reference derives it for the folded LayerNorm.  The worst case admits small systematic errors, so at most FAR
  of the elements may lie more than one f16 ulp from the correctly rounded float64 result.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f16, f32, f64 = np.float16, np.float32, np.float64
U, H, TINY = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
# A correct kernel's f32 error is a random walk, ~sqrt(K) 2^-24 |partial sums|: it moves a unit-scale result by more than one f16 ulp only within ~2^-10 of
# zero, about 0.1 % of the elements of these operands.  A systematic error (a term dropped or added twice, a wrong rounding) moves far more than 2 %: the
# constant test_rms_norm uses.
FAR = 0.02
CONV, LN1, LN2, W8 = 1, 2, 4, 32                   # form bits of the driver
GEMM2, CONV3X3, GEMM_V1, CIN4 = 0, 1, 2, 3         # osg_last_route families
OSG_F16, OSG_F32 = 2, 3
ACT_NONE, ACT_SILU, ACT_GEGLU = 0, 1, 3
GUARD = 256                                        # elements of guard before and after an output (keeps 16-byte alignment)
KNOBS = ("OSG_GEMM_CFG", "OSG_GEMM_NST", "OSG_GEMM_SPLITS", "OSG_GEMM_KS", "OSG_GEMM_SPEC", "OSG_GEMM_FOLD", "OSG_CONV3X3_BN", "OSG_CONV3X3_NL",
         "OSG_CONV3X3_SPLITS", "OSG_CONV3X3_FOLD", "OSG_SPLITK_FOLD")


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def driver():
    """{mode: what tests/cpp/contraction_routes.cpp prints in it} for the modes entries and resolve"""
    d = tempfile.mkdtemp(prefix="osg_routes_")
    try:
        exe = os.path.join(d, "routes")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"), os.path.join(REPO, "tests", "cpp", "contraction_routes.cpp"),
                        "-o", exe], check=True)
        return {m: subprocess.run([exe, m], stdout=subprocess.PIPE, text=True, check=True).stdout for m in ("entries", "resolve")}
    finally:
        shutil.rmtree(d, ignore_errors=True)


@lru_cache(maxsize=None)
def table():
    """(kV2Entries, kV3Entries, {v2 entry: (cfg, nst, ks, spec) of a request of the entry's own form that resolves to it})"""
    out = driver()
    v2, v3 = [], []
    for line in out["entries"].splitlines():
        f = line.split()
        if f[0] == "v2":
            bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, tile, fold = map(int, f[1:])
            v2.append(dict(bm=bm, bn=bn, nst=nst, conv=conv, spec=spec, ln=ln, nch=nch, ks=ks, wgn=wgn, wq=wq, tile=tile, fold=fold))
        else:
            w, bn, wgm, wgn, nlw, wq = map(int, f[1:])
            v3.append(dict(w=w, bn=bn, nlw=nlw, wq=wq))
    own = [(CONV if e["conv"] else 0) | (W8 if e["wq"] else 0) | (LN1 if e["ln"] == 1 else LN2 if e["ln"] == 2 else 0) for e in v2]
    req = {}
    for line in out["resolve"].splitlines():
        f = line.split()
        if f[0] != "r":
            continue
        form, nch, cfg, nst, ks, fold, spec, entry, _ = map(int, f[1:])
        if entry < 0 or fold or form != own[entry]:
            continue
        e = v2[entry]
        direct = (cfg, nst, ks, spec) == (e["tile"], e["nst"], e["ks"], e["spec"])     # (the tile, ring, KS and spec of the entry itself, where that reaches it)
        if entry not in req or (direct and not req[entry][1]):
            req[entry] = ((cfg, nst, ks, spec), direct)
    return v2, v3, {i: r for i, (r, _) in req.items()}


def v2_id(e):
    s = f"v2-{e['bm']:03d}x{e['bn']:03d}-n{e['nst']}"
    if e["conv"]:
        s += "-conv"
    if e["spec"]:
        s += "-spec"
    if e["ln"]:
        s += f"-ln{e['ln']}" + (f"-nch{e['nch']}" if e["ln"] == 2 else "")
    if e["ks"] == 2:
        s += "-ks2"
    return s + ("-w8" if e["wq"] else "")


def v3_id(e):
    return f"v3-w{e['w']:02d}-{e['bn']:03d}-nl{e['nlw']}" + ("-w8" if e["wq"] else "")


FOLD_TIMEOUT = pytest.mark.timeout(180, method="thread")   # (a fold protocol error would spin on the device: bound it, as the fold tests of test_gpu_kernels do)


def v2_params():
    return [pytest.param(i, id=v2_id(e), marks=[FOLD_TIMEOUT] if e["fold"] else []) for i, e in enumerate(table()[0])]


def v3_params():
    return [pytest.param(i, id=v3_id(e), marks=[FOLD_TIMEOUT]) for i, e in enumerate(table()[1])]


def knobs(mp, **kv):
    for k in KNOBS:
        mp.delenv(k, raising=False)
    for k, v in kv.items():
        mp.setenv(k, str(int(v)))


def slices(ktiles, asked):
    """the k-slices a split of `ktiles` k-tiles into `asked` runs as (no empty slice)"""
    per = -(-ktiles // asked)
    return -(-ktiles // per)


def reduce_kernel(splits, fold, n):
    """osg_last_route's reduce code for a launch of n columns (dense output, aligned operands, no statistics sinks)"""
    if splits == 1 or fold:
        return 0
    return 1 if n % 4 else 2 if splits <= 4 else 3


# ---- outputs inside guard bands ------------------------------------------------------------------------------------------------------------------------
class Out:
    """`rows` x `cols` elements, rows `ld` apart from column `col` on, inside one Gpu.empty allocation (0xFF bytes) with GUARD elements before and after"""

    def __init__(self, gpu, rows, cols, dtype=f16, ld=None, col=0):
        self.rows, self.cols, self.ld, self.col, self.dtype = rows, cols, ld or cols, col, np.dtype(dtype)
        self.buf = gpu.empty((2 * GUARD + rows * self.ld,), dtype)
        self.ptr = self.buf.ptr + (GUARD + col) * self.dtype.itemsize

    def read(self):
        raw = self.buf.numpy()
        region = raw[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)
        gap = np.ones(region.shape, bool)
        gap[:, self.col:self.col + self.cols] = False
        untouched = np.concatenate([raw[:GUARD], raw[GUARD + self.rows * self.ld:], region[gap]])
        assert (untouched.view(np.uint8) == 0xFF).all(), "a store landed outside the output (guard band or column gap changed)"
        out = region[:, self.col:self.col + self.cols].copy()
        bad = ~np.isfinite(out)
        assert not bad.any(), f"{int(bad.sum())} of {out.size} output elements not finite (first at {tuple(np.argwhere(bad)[0])}): never written, or NaN / inf computed"
        return out


def ptr(b):
    return b.ptr if b is not None else None


def bias_dtype(bias):
    return OSG_F32 if bias is not None and bias.dtype == f32 else OSG_F16


def dev(gpu, *arrays):
    return [gpu.to_dev(a) if a is not None else None for a in arrays]


# ---- float64 references and bounds ---------------------------------------------------------------------------------------------------------------------
def rnd(rng, shape, std=1.0, dtype=f16):
    return (rng.standard_normal(shape, dtype=f32) * std).astype(dtype)


def contraction(a, b, bias=None, res=None, rowbias=None, scale=None):
    """a . b^T (* scale[n]) + bias + per-image bias + residual in float64 on the exact operands (a: [..., M, K]; b: [N, K] f16 values or q - zp) and its f32
    error bound E = (K + 3 (+ 1 per-image bias) (+ 1 scale)) 2^-24 S"""
    a64, b64 = a.astype(f64), b.astype(f64)
    return epilogue(a64 @ b64.T, np.abs(a64) @ np.abs(b64).T, a.shape[-1], bias, res, rowbias, scale)


def epilogue(pre, S, k, bias=None, res=None, rowbias=None, scale=None):
    """contraction's second half, on the float64 products pre = a . b^T and S = |a| . |b|^T of k terms each (tuned_rows.py forms them blockwise)"""
    n = k + 3 + (rowbias is not None) + (scale is not None)
    if scale is not None:
        pre, S = pre * scale, S * np.abs(scale)
    for t in (bias, rowbias, res):
        if t is not None:
            pre, S = pre + t.astype(f64), S + np.abs(t.astype(f64))
    return pre, n * U * S


def geglu_logical(x):
    """columns of a pair-interleaved GEGLU projection (blocks of 16 value columns, then 16 gate columns) -> [values | gates]"""
    n = x.shape[-1]
    d = np.arange(n)
    to = np.where(d % 32 < 16, 16 * (d // 32) + d % 32, n // 2 + 16 * (d // 32) + d % 32 - 16)
    out = np.empty_like(x)
    out[..., to] = x
    return out


def act_apply(pre, E, act):
    """the activation of the float64 pre-activation values and the propagation of their bound E"""
    if act == ACT_NONE:
        return pre, E
    if act == ACT_SILU:
        # device: v * rcp(1 + exp2(-v log2 e)).  The rounding of v log2 e moves exp2's result by |v| 2^-24 relative, exp2, the addition and rcp by ~1 ulp each:
        # the sigmoid errs by (|v| + 5) 2^-24 relative, the product adds 2^-24.  |silu'| <= 1.1.
        y = pre / (1.0 + np.exp(-pre))
        return y, 1.1 * E + (np.abs(pre) + 8) * U * np.abs(y)
    assert act == ACT_GEGLU
    from scipy.special import erf
    c = pre.shape[-1] // 2
    v, g, ev, eg = pre[..., :c], pre[..., c:], E[..., :c], E[..., c:]
    ge = 0.5 * g * (1.0 + erf(g / np.sqrt(2.0)))
    # d(v gelu(g)) = gelu(g) dv + v gelu'(g) dg with |gelu'| <= 1.13; the device erf (Abramowitz-Stegun 7.1.26) errs by 1.5e-7, its f32 evaluation on the
    # hardware rcp / exp2 by less than 2^-20; 0.5 g (1 + erf) and the product by a few roundings
    return v * ge, np.abs(ge) * ev + 1.13 * (np.abs(v) + ev) * eg + np.abs(v) * (0.5 * np.abs(g) * (1.5e-7 + 2.0 ** -20) + 4 * U * (np.abs(g) + np.abs(ge)))


def ulps_off(got, want):
    """distance in f16 ulps between got and the correctly rounded want"""
    def order(h):
        i = h.view(np.uint16).astype(np.int32)
        return np.where(i & 0x8000, -(i & 0x7FFF), i)
    return np.abs(order(got.astype(f16)) - order(want.astype(f16)))


def bound_of(want, E):
    return H * np.abs(want) + (1 + H) * E + TINY


def check(got, want, E, what):
    g = got.astype(f64)
    bound = bound_of(want, E)
    bad = np.abs(g - want) > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; first at {i}: got {g[i]!r} want {want[i]!r} bound {bound[i]!r}")
    far = (ulps_off(got, want) > 1).mean()
    assert far <= FAR, f"{what}: {far:.4f} of the elements more than one f16 ulp from the correctly rounded result"


def check_rowstats(got, rs, what):
    """osg_gemm_rowstats sums the STORED f16 outputs of each 32-column slot (osg_gemm_common.h): 32 terms in f32, squares of f16 values exact in f32"""
    g = got.astype(f64).reshape(got.shape[0], -1, 32)
    rs = rs.astype(f64).reshape(got.shape[0], -1, 2)
    for k, t in ((0, g), (1, g * g)):
        bad = np.abs(rs[..., k] - t.sum(-1)) > 31 * U * np.abs(t).sum(-1)
        assert not bad.any(), f"{what}: row statistic {k} of slot {tuple(np.argwhere(bad)[0])} is not the sum of the stored outputs"


def ln_reference(x, wf, c1, c2, eps, res):
    """rstd (x . wf^T - mean c1) + c2 (+ residual) in float64 on the operands osg_gemm_ln receives, and its bound.  The kernel: s = sum x and q = sum x^2 in f32
    (single pass, or the producer's slot sums added up: at most K - 1 additions either way); mean = s / K, var = q / K - mean^2 formed in f64 from them and
    rounded to f32; rstd = 1 / sqrtf(var + eps) (three roundings); acc = x . wf as in the plain GEMM; rstd (acc - mean c1) + c2 + residual (five roundings)."""
    k = x.shape[1]
    x64, wf64, c1, c2 = x.astype(f64), wf.astype(f64), c1.astype(f64), c2.astype(f64)
    s, q = x64.sum(1), (x64 * x64).sum(1)
    mean = s / k
    var = np.maximum(q / k - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    acc = x64 @ wf64.T
    D = acc - mean[:, None] * c1
    pre = rstd[:, None] * D + c2
    r64 = res.astype(f64) if res is not None else 0.0
    pre = pre + r64
    e_s, e_q = (k - 1) * U * np.abs(x64).sum(1), (k - 1) * U * q
    e_mean = e_s / k + 2 * U * np.abs(mean)                                   # (+ the f32 1 / K, the f32 mean)
    e_var0 = (e_q + U * q) / k + (2 * np.abs(mean) + e_mean) * e_mean
    e_var = e_var0 + U * (var + e_var0)
    e_rstd = 0.5 * e_var * np.maximum(var + eps - e_var, eps) ** -1.5 + 4 * U * rstd
    e_D = (k + 3) * U * (np.abs(x64) @ np.abs(wf64).T) + e_mean[:, None] * np.abs(c1) + 2 * U * (np.abs(acc) + np.abs(mean)[:, None] * np.abs(c1))
    E = e_rstd[:, None] * (np.abs(D) + e_D) + rstd[:, None] * e_D + U * (3 * rstd[:, None] * np.abs(D) + 2 * np.abs(c2) + np.abs(r64))
    return pre, E


def im2col(x, k, stride, pad):
    """NHWC x -> [n ho wo, (kh, kw, cin)] rows in float64 (the OHWI weight's K order), ho, wo"""
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c), f64)
    xp[:, pad:pad + h, pad:pad + w] = x
    taps = [xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :] for i in range(k) for j in range(k)]
    return np.concatenate(taps, axis=-1).reshape(n * ho * wo, k * k * c), ho, wo


def quant(rng, shape):
    """uint8 codes over the whole range, a zero point and a scale that make the weights ~N(0, 1 / K)"""
    q = rng.integers(0, 256, shape, dtype=np.uint8)
    return q, 128 + int(rng.integers(-8, 9)), float(np.float32(2.0 / np.sqrt(np.prod(shape[1:])) / 74.0))


def quant_vectors(rng, n, scale):
    return (scale * rng.uniform(0.5, 2.0, n)).astype(f32), rng.integers(100, 156, n).astype(f32)


# ---- the entry points --------------------------------------------------------------------------------------------------------------------------------
def gemm(gpu, a, w, bias, res, act, batch=1):
    """osg_gemm with the [N, K] weight w; a: [M, K] or [batch, M, K]"""
    m, k = a.shape[-2:]
    n = w.shape[0]
    out = Out(gpu, batch * m, n // 2 if act == ACT_GEGLU else n)
    da, dw, db, dr = keep = dev(gpu, a, w, bias, res)
    gpu._ck(gpu.lib.osg_gemm(gpu.ctx, OSG_F16, da.ptr, dw.ptr, 1, ptr(db), bias_dtype(bias), ptr(dr), out.ptr, m, n, k, batch, m * k if batch > 1 else 0, 0,
                             m * n if batch > 1 else 0, act))
    got = out.read()
    del keep
    return got, gpu.last_route()


def gemm_rowstats(gpu, a, w, bias, res, act):
    m, k = a.shape
    n = w.shape[0]
    out, rs = Out(gpu, m, n), Out(gpu, m, n // 32 * 2, f32)
    da, dw, db, dr = keep = dev(gpu, a, w, bias, res)
    gpu._ck(gpu.lib.osg_gemm_rowstats(gpu.ctx, da.ptr, dw.ptr, ptr(db), bias_dtype(bias), ptr(dr), out.ptr, m, n, k, act, rs.ptr))
    got, stats = out.read(), rs.read()
    del keep
    return got, stats, gpu.last_route()


def gemm_w8(gpu, a, q, scale, zp, vec, bias, res, act):
    """osg_gemm_w8, or osg_gemm_w8_v with vec = (scale[N], zero point[N])"""
    m, k = a.shape
    n = q.shape[0]
    out = Out(gpu, m, n // 2 if act == ACT_GEGLU else n)
    da, dq, db, dr, dv = keep = dev(gpu, a, q, bias, res, np.concatenate(vec) if vec is not None else None)
    if dv is None:
        gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dq.ptr, scale, zp, ptr(db), bias_dtype(bias), ptr(dr), out.ptr, m, n, k, act))
    else:
        gpu._ck(gpu.lib.osg_gemm_w8_v(gpu.ctx, da.ptr, dq.ptr, 0.0, 0, dv.ptr, dv.ptr + 4 * n, ptr(db), bias_dtype(bias), ptr(dr), out.ptr, m, n, k, act))
    got = out.read()
    del keep
    return got, gpu.last_route()


def conv(gpu, x, w, bias, res, ib, act, stride, pad, w8=None, ld=None, col=0):
    """osg_conv2d_nhwc_v (f16 OHWI weight), or osg_conv2d_nhwc_w8_v with w the codes and w8 = (scale, zero point, vectors or None); res: [pixels, Cout];
    ib: [images, Cout]; ld / col: the output as a column view of a wider buffer"""
    n, h, wd, cin = x.shape
    cout, kh, kw, _ = w.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    out = Out(gpu, n * ho * wo, cout, ld=ld, col=col)
    vec = w8[2] if w8 is not None else None
    dx, dw, db, dr, di, dv = keep = dev(gpu, x, w, bias, res, ib, np.concatenate(vec) if vec is not None else None)
    geo = (n, h, wd, cin, cout, kh, kw, stride, stride, pad, pad, pad, pad, act)
    if w8 is None:
        gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, OSG_F16, dx.ptr, dw.ptr, ptr(db), bias_dtype(bias), ptr(di), cout if ib is not None else 0, ptr(dr), out.ptr,
                                          ld or 0, None, 0, *geo))
    else:
        gpu._ck(gpu.lib.osg_conv2d_nhwc_w8_v(gpu.ctx, dx.ptr, dw.ptr, w8[0], w8[1], ptr(dv), dv.ptr + 4 * cout if dv is not None else None, ptr(db),
                                             bias_dtype(bias), ptr(di), cout if ib is not None else 0, ptr(dr), out.ptr, ld or 0, None, 0, *geo))
    got = out.read()
    del keep
    return got, gpu.last_route()


def ln_fold(w, gamma, beta, bias):
    """the folded operands Gpu.gemm_ln builds: W' = f16(gamma W), c1 = sum_k W', c2 = W . beta + bias"""
    wf = (gamma.astype(f32)[None, :] * w.astype(f32)).astype(f16)
    return wf, wf.astype(f64).sum(axis=1).astype(f32), (w.astype(f64) @ beta.astype(f64) + bias.astype(f64)).astype(f32)


def gemm_ln(gpu, x, w, gamma, beta, bias, res, act, with_rowstats):
    """osg_gemm_ln with the folded operands Gpu.gemm_ln builds (W' = f16(gamma W), c1 = sum_k W', c2 = W . beta + bias); with_rowstats: the producer's
    [M][K/32][2] slot sums handed over, built here in float32 from float64 sums (the consumer tested alone)"""
    m, k = x.shape
    n = w.shape[0]
    wf, c1, c2 = ln_fold(w, gamma, beta, bias)
    rs = None
    if with_rowstats:
        x3 = x.astype(f64).reshape(m, k // 32, 32)
        rs = np.stack([x3.sum(-1), (x3 * x3).sum(-1)], -1).astype(f32)
    out = Out(gpu, m, n // 2 if act == ACT_GEGLU else n)
    dx, dwf, d1, d2, drs, dr = keep = dev(gpu, x, wf, c1, c2, rs, res)
    gpu._ck(gpu.lib.osg_gemm_ln(gpu.ctx, dx.ptr, dwf.ptr, d1.ptr, d2.ptr, 1e-5, ptr(drs), ptr(dr), out.ptr, m, n, k, act))
    got = out.read()
    del keep
    return got, gpu.last_route(), (wf, c1, c2)


# ---- gemm2_kernel ------------------------------------------------------------------------------------------------------------------------------------
K_PLAIN = 960            # 15 k-tiles: at least NST + 1 for every ring, a multiple of none of 2 / 4 / 6 / 8 (the ring wraps mid-way), odd for KS = 2
K_LN2 = {5: 320, 10: 576, 20: 1216}    # K / 64 chunks of handed-over statistics: 5, 9, 19 -> the NCH = 5 / 10 / 20 instantiations (k-tiles odd as well)


@pytest.mark.parametrize("idx", v2_params())
def test_gemm2_instantiation(gpu, idx, monkeypatch):
    v2, _, req = table()
    e = v2[idx]
    assert idx in req, f"no launch request resolves to entry {idx}"
    cfg, nst, ks, spec = req[idx]
    rng = np.random.default_rng(7919 * (idx + 1))

    def force(**kv):
        knobs(monkeypatch, OSG_GEMM_CFG=cfg, OSG_GEMM_NST=nst, OSG_GEMM_KS=ks, OSG_GEMM_SPEC=spec, **kv)

    pairs = (e["bn"] // e["wgn"]) % 32 == 0          # GEGLU value / gate pairs and row-statistics slots: a wave's columns a multiple of 32
    if e["ln"]:
        ln_entry(gpu, idx, e, force, pairs, rng)
    elif e["conv"]:
        conv_entry(gpu, idx, e, force, rng)
    else:
        gemm_entry(gpu, idx, e, force, pairs, rng)


def splits_asked(e):
    """(k-slices, fold) of the tall case: 1; 3 (the reduce launch); 5 (splitk_reduce4_kernel<8>); the fold where the entry takes it.  Four loader waves: 1."""
    return [(1, 0)] if e["spec"] else [(1, 0), (3, 0), (5, 0)] + ([(3, 1)] if e["fold"] else [])


def gemm_entry(gpu, idx, e, force, pairs, rng):
    K = K_PLAIN
    kt = K // 64
    w8 = bool(e["wq"])
    if w8:
        q, zp, scale = quant(rng, (400, K))
        wmat = q.astype(f64) - zp
    else:
        w = rnd(rng, (400, K), K ** -0.5)

    def route(s, fold, n):
        s = slices(kt, s)
        return (GEMM2, idx, s, fold, reduce_kernel(s, fold, n))

    def run(a, n, bias, res, act, vec=None, batch=1):
        if not w8:
            return gemm(gpu, a, w[:n], bias, res, act, batch)
        return gemm_w8(gpu, a, q[:n], scale, zp, vec, bias, res, act)

    def want(a, n, bias, res=None, vec=None):
        if not w8:
            return contraction(a, w[:n], bias, res)
        if vec is None:
            return contraction(a, wmat[:n], bias, res, scale=scale)
        return contraction(a, q[:n].astype(f64) - vec[1][:, None], bias, res, scale=vec[0].astype(f64))

    # tall (the m-major tile walk): 300 x 200 -- ragged for every BM / BN, tile totals no multiple of 8 --, f16 bias + residual
    M, N = 300, 200
    a, bias, res = rnd(rng, (M, K)), rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    pre, E = want(a, N, bias, res)
    for s, fold in splits_asked(e):
        force(OSG_GEMM_SPLITS=s, OSG_GEMM_FOLD=fold)
        got, r = run(a, N, bias, res, ACT_NONE)
        check(got, pre, E, f"tall, {s} k-slices, fold {fold}")
        assert r == route(s, fold, N), r
    # wide (n-major): 136 x 372, f32 bias, SiLU; uint8 codes with per-column (scale, zero point) vectors
    M, N = 136, 372
    a, bias = rnd(rng, (M, K)), rnd(rng, (N,), 0.1, f32)
    vec = quant_vectors(rng, N, scale) if w8 else None
    force(OSG_GEMM_SPLITS=1)
    got, r = run(a, N, bias, None, ACT_SILU, vec)
    check(got, *act_apply(*want(a, N, bias, vec=vec), ACT_SILU), "wide, f32 bias, SiLU")
    assert r == route(1, 0, N), r
    if not w8:
        # batch 2 over a shared weight with N % 4 != 0 (the general epilogue); split in 3: the scalar reduce launch
        M, N = 97, 150
        a, bias, res = rnd(rng, (2, M, K)), rnd(rng, (N,), 0.1), rnd(rng, (2, M, N))
        pre, E = want(a, N, bias, res)
        for s in (1,) if e["spec"] else (1, 3):
            force(OSG_GEMM_SPLITS=s)
            got, r = run(a, N, bias, res, ACT_NONE, batch=2)
            check(got, pre.reshape(2 * M, N), E.reshape(2 * M, N), f"batch 2, N % 4 != 0, {s} k-slices")
            assert r == route(s, 0, N), r
    if pairs:
        # GEGLU: 384 pair-interleaved columns -> 192
        M, N = 300, 384
        a, bias = rnd(rng, (M, K)), rnd(rng, (N,), 0.1)
        force(OSG_GEMM_SPLITS=1)
        got, r = run(a, N, bias, None, ACT_GEGLU)
        pre, E = want(a, N, bias)
        check(got, *act_apply(geglu_logical(pre), geglu_logical(E), ACT_GEGLU), "GEGLU")
        assert r == route(1, 0, N), r
        if not w8:
            # the row-statistics producer: 352 columns (11 slots), bias + residual, SiLU
            M, N = 300, 352
            a, bias, res = rnd(rng, (M, K)), rnd(rng, (N,), 0.1), rnd(rng, (M, N))
            got, rs, r = gemm_rowstats(gpu, a, w[:N], bias, res, ACT_SILU)
            check(got, *act_apply(*want(a, N, bias, res), ACT_SILU), "row-statistics producer")
            check_rowstats(got, rs, "row-statistics producer")
            assert r == route(1, 0, N), r
    # a 1 x 1 convolution (the GEMM over the pixels) into a column view: columns 12 .. 211 of rows 224 wide, the gap must stay untouched
    M, N = 300, 200
    x, bias, res = rnd(rng, (1, 15, 20, K)), rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    force(OSG_GEMM_SPLITS=1)
    if w8:
        got, r = conv(gpu, x, q[:N].reshape(N, 1, 1, K), bias, res, None, ACT_NONE, 1, 0, w8=(scale, zp, None), ld=N + 24, col=12)
    else:
        got, r = conv(gpu, x, w[:N].reshape(N, 1, 1, K), bias, res, None, ACT_NONE, 1, 0, ld=N + 24, col=12)
    check(got, *want(x.reshape(M, K), N, bias, res), "1x1 convolution into a column view")
    assert r == route(1, 0, N), r


def conv_entry(gpu, idx, e, force, rng):
    """the implicit-GEMM convolution: stride 2, or a width the halo kernel does not take (it claims every 3 x 3 / stride 1 request at W in 8 .. 64)"""
    w8 = bool(e["wq"])
    cin = 64
    K = 9 * cin                                       # 9 k-tiles: NST + 1 for 8 stages, odd, a multiple of no ring; 3 and 5 slices
    kt = K // 64

    def weights(cout):
        if not w8:
            w = rnd(rng, (cout, 3, 3, cin), K ** -0.5)
            return w, w.reshape(cout, K), None
        q, zp, scale = quant(rng, (cout, 3, 3, cin))
        return q, q.reshape(cout, K).astype(f64) - zp, (scale, zp)

    # tall: 4 images 34 x 34 at stride 2 -> 4 x 17 x 17 pixels, 200 channels; bias, per-image bias, residual; 1 / 3 / 5 slices, the fold
    cout = 200
    wt, wmat, qs = weights(cout)
    x = rnd(rng, (4, 34, 34, cin))
    cols, ho, wo = im2col(x, 3, 2, 1)
    M = cols.shape[0]
    bias, ib, res = rnd(rng, (cout,), 0.1), rnd(rng, (4, cout), 0.5), rnd(rng, (M, cout))
    pre, E = contraction(cols, wmat, bias, res, np.repeat(ib, ho * wo, axis=0), scale=qs[0] if w8 else None)
    for s, fold in splits_asked(e):
        force(OSG_GEMM_SPLITS=s, OSG_GEMM_FOLD=fold)
        got, r = conv(gpu, x, wt, bias, res, ib, ACT_NONE, 2, 1, w8=(qs[0], qs[1], None) if w8 else None)
        check(got, pre, E, f"stride 2, {s} k-slices, fold {fold}")
        s = slices(kt, s)
        assert r == (GEMM2, idx, s, fold, reduce_kernel(s, fold, cout)), r
    # wide: one 11 x 12 image at stride 1, 372 channels, f32 bias, SiLU; uint8 codes with per-column vectors
    cout = 372
    wt, wmat, qs = weights(cout)
    x = rnd(rng, (1, 11, 12, cin))
    cols, _, _ = im2col(x, 3, 1, 1)
    bias = rnd(rng, (cout,), 0.1, f32)
    force(OSG_GEMM_SPLITS=1)
    if w8:
        vec = quant_vectors(rng, cout, qs[0])
        pre, E = contraction(cols, wt.reshape(cout, K).astype(f64) - vec[1][:, None], bias, scale=vec[0].astype(f64))
        got, r = conv(gpu, x, wt, bias, None, None, ACT_SILU, 1, 1, w8=(0.0, 0, vec))
    else:
        pre, E = contraction(cols, wmat, bias)
        got, r = conv(gpu, x, wt, bias, None, None, ACT_SILU, 1, 1)
    check(got, *act_apply(pre, E, ACT_SILU), "width 12, f32 bias, SiLU")
    assert r == (GEMM2, idx, 1, 0, 0), r


def ln_entry(gpu, idx, e, force, pairs, rng):
    """LayerNorm folded in: LN = 1 row statistics beside the MFMAs, LN = 2 handed over; rows with a large common offset (the single-pass variance cancels)"""
    K = K_LN2[e["nch"]] if e["ln"] == 2 else K_PLAIN
    force(OSG_GEMM_SPLITS=1)
    cases = [(300, 200, ACT_NONE, True), (136, 372, ACT_SILU, False)] + ([(300, 384, ACT_GEGLU, False)] if pairs else [])
    for M, N, act, with_res in cases:
        x = (rnd(rng, (M, K), 1.5).astype(f32) + rng.standard_normal((M, 1), dtype=f32) * 3.0).astype(f16)
        gamma, beta = (1 + rnd(rng, (K,), 0.2).astype(f32)).astype(f16), rnd(rng, (K,), 0.2)
        w, bias = rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1)
        res = rnd(rng, (M, N)) if with_res else None
        got, r, ops = gemm_ln(gpu, x, w, gamma, beta, bias, res, act, e["ln"] == 2)
        pre, E = ln_reference(x, *ops, 1e-5, res)
        if act == ACT_GEGLU:
            pre, E = geglu_logical(pre), geglu_logical(E)
        check(got, *act_apply(pre, E, act), f"{M} x {N} x {K}, act {act}")
        assert r == (GEMM2, idx, 1, 0, 0), r


# ---- conv3x3_kernel (the halo-reuse 3 x 3 convolution) --------------------------------------------------------------------------------------------------
HALO_IMAGES = {64: (1, 6), 32: (2, 4), 16: (1, 16), 8: (3, 8)}   # (images, rows) at each width: whole 128-pixel tiles; at W = 8 two 8 x 8 images a tile (3: half a tile)


@pytest.mark.parametrize("idx", v3_params())
def test_conv3x3_instantiation(gpu, idx, monkeypatch):
    """320 input channels = 5 slabs: 1 / 3 / 5 k-slices and the fold; 196 output channels: a ragged last tile at 80, 128 and 160 columns"""
    _, v3, _ = table()
    e = v3[idx]
    n, h = HALO_IMAGES[e["w"]]
    cin, cout = 320, 196
    rng = np.random.default_rng(104729 * (idx + 1))
    x = rnd(rng, (n, h, e["w"], cin))
    cols, _, _ = im2col(x, 3, 1, 1)
    if e["wq"]:
        wt, zp, scale = quant(rng, (cout, 3, 3, cin))
        wmat = wt.reshape(cout, -1).astype(f64) - zp
    else:
        wt = rnd(rng, (cout, 3, 3, cin), (9 * cin) ** -0.5)
        wmat, scale, zp = wt.reshape(cout, -1), None, None
    w8 = (scale, zp, None) if e["wq"] else None
    bias, ib, res = rnd(rng, (cout,), 0.1), rnd(rng, (n, cout), 0.5), rnd(rng, (cols.shape[0], cout))
    pre, E = contraction(cols, wmat, bias, res, np.repeat(ib, h * e["w"], axis=0), scale=scale)
    for s, fold in ((1, 0), (3, 0), (5, 0), (3, 1)):
        knobs(monkeypatch, OSG_CONV3X3_BN=e["bn"], OSG_CONV3X3_NL=e["nlw"], OSG_CONV3X3_SPLITS=s, OSG_CONV3X3_FOLD=fold)
        got, r = conv(gpu, x, wt, bias, res, ib, ACT_NONE, 1, 1, w8=w8)
        check(got, pre, E, f"{s} k-slices, fold {fold}")
        sl = slices(cin // 64, s)
        assert r == (CONV3X3, idx, sl, fold, reduce_kernel(sl, fold, cout)), r
    # f32 bias, SiLU, no residual; uint8 codes with per-column vectors
    bias = rnd(rng, (cout,), 0.1, f32)
    knobs(monkeypatch, OSG_CONV3X3_BN=e["bn"], OSG_CONV3X3_NL=e["nlw"], OSG_CONV3X3_SPLITS=1)
    if e["wq"]:
        vec = quant_vectors(rng, cout, scale)
        pre, E = contraction(cols, wt.reshape(cout, -1).astype(f64) - vec[1][:, None], bias, scale=vec[0].astype(f64))
        w8 = (0.0, 0, vec)
    else:
        pre, E = contraction(cols, wmat, bias)
    got, r = conv(gpu, x, wt, bias, None, None, ACT_SILU, 1, 1, w8=w8)
    check(got, *act_apply(pre, E, ACT_SILU), "f32 bias, SiLU")
    assert r == (CONV3X3, idx, 1, 0, 0), r


# ---- the round-1 kernels -----------------------------------------------------------------------------------------------------------------------------
# launch_cfg's tiles (0: 128 x 128 when 128 x 128 tiles fill the CUs and N % 128 == 0, 1: 128 x 64 when those do and M >= 128, 2: 64 x 64) x the vector /
# scalar A loads (K % 8 == 0 / Cin % 8 == 0) x GEMM / convolution, reached with K (Cin) no multiple of 64; the 64 x 64 cases with K >= 1024 on few tiles split.
# GEMM: (M, N, K); convolution 3 x 3, stride 1, pad 1: (images, H = W, Cin, Cout).
V1_CASES = [(0, 0, 1, (2560, 2048, 72)), (0, 0, 0, (2560, 2048, 70)), (0, 1, 1, (4096, 1000, 72)), (0, 1, 0, (4096, 1000, 70)),
            (0, 2, 1, (300, 200, 1032)), (0, 2, 0, (300, 200, 1030)),
            (1, 0, 1, (10, 16, 8, 2048)), (1, 0, 0, (10, 16, 6, 2048)), (1, 1, 1, (16, 16, 8, 1000)), (1, 1, 0, (16, 16, 6, 1000)),
            (1, 2, 1, (1, 17, 120, 200)), (1, 2, 0, (1, 17, 118, 200))]


def v1_id(c):
    is_conv, tile, vec, _ = c
    return f"v1-{('128x128', '128x064', '064x064')[tile]}" + ("-vec" if vec else "") + ("-conv" if is_conv else "")


@pytest.mark.parametrize("case", V1_CASES, ids=[v1_id(c) for c in V1_CASES])
def test_round1_gemm_kernel(gpu, case, monkeypatch):
    is_conv, tile, vec, shape = case
    knobs(monkeypatch)
    rng = np.random.default_rng(sum(shape) + 31 * tile + 7 * vec + is_conv)
    if is_conv:
        n, hw, cin, N = shape
        K = 9 * cin
        x = rnd(rng, (n, hw, hw, cin))
        w = rnd(rng, (N, 3, 3, cin), K ** -0.5)
        a, _, _ = im2col(x, 3, 1, 1)
        M = a.shape[0]
        bias, res = rnd(rng, (N,), 0.1), rnd(rng, (M, N))
        got, r = conv(gpu, x, w, bias, res, None, ACT_NONE, 1, 1)
        pre, E = contraction(a, w.reshape(N, K), bias, res)
    else:
        M, N, K = shape
        a, w = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5)
        bias, res = rnd(rng, (N,), 0.1), rnd(rng, (M, N))
        got, r = gemm(gpu, a, w, bias, res, ACT_NONE)
        pre, E = contraction(a, w, bias, res)
    check(got, pre, E, v1_id(case))
    # the split of the 64 x 64 cases: as many slices as K / 256 allows (few tiles, K >= 1024), over 32-deep k-tiles
    s = min(K // 256, 32) if tile == 2 else 1
    s = slices(-(-K // 32), s)
    assert r == (GEMM_V1, tile | vec << 2 | is_conv << 3, s, 0, reduce_kernel(s, 0, N)), r


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_cin4_kernel(gpu, stride, monkeypatch):
    """conv_cin4_mfma_kernel (3 x 3, Cin = 4: the SD conv_in / VAE post-quant convolution): ragged pixel count, f32 bias, per-image bias, residual, SiLU"""
    knobs(monkeypatch)
    rng = np.random.default_rng(4 + stride)
    n, hw, cout = 2, 23, 320
    x = rnd(rng, (n, hw, hw, 4))
    w = rnd(rng, (cout, 3, 3, 4), 36 ** -0.5)
    a, ho, wo = im2col(x, 3, stride, 1)
    bias, ib, res = rnd(rng, (cout,), 0.1, f32), rnd(rng, (n, cout), 0.5), rnd(rng, (a.shape[0], cout))
    got, r = conv(gpu, x, w, bias, res, ib, ACT_SILU, stride, 1)
    check(got, *act_apply(*contraction(a, w.reshape(cout, 36), bias, res, np.repeat(ib, ho * wo, axis=0)), ACT_SILU), f"cin4, stride {stride}")
    assert r == (CIN4, 0, 1, 0, 0), r
