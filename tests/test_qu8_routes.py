"""-m gpu: the uint8-arithmetic kernels (onnxstream_amd/csrc/osg_qu8.hip) per route, bit exact against the specification oracle/np_qu8.py.

What is pinned.  Every case asserts through osg_last_kernel (include/osgpu.h, families 5 and 6) which kernel / route the entry point launched BEFORE it compares
codes; every output is a view between two 0xFF guard bands of one allocation (Gpu.empty), and the bands -- with every gap a batch stride or a misaligned view
leaves -- must come back 0xFF; every case is seeded and frees its buffers.  Every comparison is array_equal against oracle/np_qu8.py evaluated on the host, never
against another device launch; the fused ops are composed from the specification's functions (mul_u8 -> add_u8 -> sigmoid_u8 table -> mul_u8; instance_norm_u8 on
the rows gathered from NHWC with numpy).  The codes are integers: there is no tolerance.  The environment knobs OSG_QU8_V2, _NST, _V2_TILE, _TILE and _WGM are
read per launch and set per case.  The last test fails, naming what is missing, unless the records seen include all 6 q8_gemm_kernel and all 16 non-debug
q8_gemm2_kernel instantiations and every family-6 route listed at E_WANTED.

  contractions, register-staged (OSG_QU8_V2=0): GEMM (70, 37, 72) lda 75 (scalar staging, a partial second k-tile), (130, 132, 80) lda 96 at tiles 64 and 128
      (16-byte staging, partial last k-tile), each dense and as a batch of 3 with stride_a > M lda, one shared weight (stride_b 0) and stride_c > M N, each
      with and without a bias of both signs whose b / (sx sw) is no integer; every convolution below; a Cin = 20 convolution (scalar staging).
  contractions, pipelined (OSG_QU8_V2=2): GEMM (200, 132, 256) lda 272, batch 2 with all three strides beyond dense, a bias, on every tile / ring depth;
      K = 128 on a ring of depth 4 (more slots than k-tiles).  Convolutions on 2 x 9 x 11 x 128 -> 68 channels (M and N tile tails, N % 4 == 0): 3 x 3 stride 2
      pads (0, 0, 1, 1) -- the halo rule's bottom / right clauses alone --, 3 x 3 pads (1, 0, 0, 2), 1 x 3, 3 x 1, stride (2, 1), 1 x 1 without pads (record: no halo
      correction), 7 x 7 (49 taps > 32: record says the register-staged kernel); input zero points 0, 117, 255 on the padded ones, weight zero points 0 and 255
      once each; tap sums from the caller (record 1) and built by the call (record 2), osg_qu8_conv_tap_sums itself against w.sum(-1).
  requantisation: a GEMM and a Mul with sx sw / so exactly 0.5 (half of the accumulators are round-to-even ties), output zero points 0, 128, 255.  Every
      contraction case checks on the host, before the launch, that both ends of the code range are reached (min < 30, max > 220; 0 and 255 where built for it).
  osg_qu8_lut: n = 1, 255, 257, 524288 + 77 (second trip of the grid-stride loop), all 256 codes present, table from the host and placed on the device.
  osg_qu8_binary (Add, Mul): same shape n = 16 k + 5; per-channel against NHWC and against NCHW with H W = 35; a scalar on either side; a periodic operand on
      the left (operands swapped); rank 6; same shape through views at byte offset 1 (generic kernel); (1100, 1, 5) x (1, 100, 1) = 550 000 outputs (second trip of
      the generic loop); same shape with 2^23 + 53 codes (second trip + tail of the fast kernel); zero points 0 / 255 with both ends reached; an Add whose scale
      ratio puts the shift outside [1, 31] is refused, osg_last_error names it, the output stays 0xFF.
  osg_qu8_affine_act: ACT on / off, NHWC and NCHW with odd H W, n no multiple of 16, x or y at byte offset 1 (the scalar branch).
  osg_qu8_instance_norm: 3 rows of 65536 + 77 (two pieces; rows 1 and 2 start misaligned); [2, 4, 1000] with four scales (row % n_scale), one constant row
      (variance 0), one row of codes 0 and 255 alone.
  osg_qu8_instance_norm_nhwc: (C, G) = (48, 48), (64, 16), (128, 8), (256, 8) (sh 0, 2, 4, 5), (96, 8) (the division on the 16-byte path), (40, 5) (scalar),
      H W = 700 at C = 96 (the second piece starts at channel 64), C = 64 at byte offset 8 (scalar), G = 56, G = 57 refused.
  osg_qu8_norm_affine_act_nhwc: channel tables at C = 96 and 320 (a channel block with cb0 > 0 and 64 channels), H W = 5, 64, 231; per-group tables at (40, 5)
      and at C = 64 through a misaligned view; ACT on / off on both.
  osg_qu8_softmax_last: C = 1, 3, 255, 256, 257, 4096, 5000; a row of zeros, a row of 255s (C <= 512), one 255 among zeros; the constant rows at C = 513 and 600
      whose 32-bit sum wraps (to 32 and 104): the codes of the corrected specification, 255 in every column.  Before each launch the helper forms the 32-bit
      sum of every row on the host and asserts it is not 0.

Left out: OSG_QU8_DBG (wrong results by design); OSG_QU8_NORM_CHAIN (read once per process); the a_bytes >= 2^31 refusal of the pipelined kernel; softmax rows
whose table sum is 0 modulo 2^32 (a constant row at 1024 or 4096 channels): every implementation divides by zero there and np_qu8.softmax_u8 refuses them.
The softmax rows are pinned against np_qu8 alone: oracle/qu8_check.py runs whole model directories through the reference and offers no single-Softmax entry.
"""
import numpy as np
import pytest

import test_unet_attention_norm as an
from oracle import np_qu8 as Q
from onnxstream_amd.osgpu import OsgError

pytestmark = pytest.mark.gpu
dev = an.dev
GUARD = an.GUARD
f32 = np.float32
u8 = np.uint8
Q8C, Q8E = 5, 6                                   # osg_last_kernel families
LUT, BINARY, AFFINE_ACT, INORM, INORM_NHWC, NORM_AFFINE, SOFTMAX = 1, 2, 3, 4, 5, 6, 7          # family 6: the entry points
RECORDS = {}                                      # case id -> osg_last_kernel record (test_coverage reads it)


def codes(rng, shape):
    return np.asarray(rng.integers(0, 256, shape, dtype=u8))


def bell(rng, shape):
    """codes with structure (a bell around a per-row centre), like real activations"""
    centre = rng.integers(60, 190, tuple(shape[:-1]) + (1,))
    return np.clip(np.rint(rng.standard_normal(shape) * 35 + centre), 0, 255).astype(u8)


class Out:
    """an output of `shape` codes at byte `off` behind the first guard band of one 0xFF-filled allocation"""

    def __init__(self, dev, shape, off=0):
        self.shape, self.off = tuple(shape), off
        self.n = int(np.prod(shape))
        self.buf = dev.nan(self.n + 2 * GUARD + 16, u8)
        self.view = self.buf.view(GUARD + off, self.shape)

    def read(self):
        raw = self.buf.numpy()
        lo = GUARD + self.off
        assert (raw[:lo] == 0xFF).all() and (raw[lo + self.n:] == 0xFF).all(), "a store landed in a guard band"
        return raw[lo:lo + self.n].reshape(self.shape)

    def untouched(self):
        assert (self.buf.numpy() == 0xFF).all(), "a refused call wrote to its output"


def at(dev, arr, off):
    """arr on the device at byte offset `off` of an allocation (off = 0: aligned)"""
    arr = np.ascontiguousarray(arr)
    if not off:
        return dev(arr)
    flat = np.concatenate([np.full(off, 0xEE, u8), arr.reshape(-1).view(u8)])
    return dev(flat).view(off, arr.shape)


def same(got, want, what):
    want = np.broadcast_to(want, got.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {want.size} codes differ; first at {i}: got {int(got[i])}, want {int(want[i])}")


def record(gpu, cid, want):
    rec = gpu.last_kernel()
    assert rec[:len(want)] == tuple(want), f"{cid}: osg_last_kernel {rec}, wanted {tuple(want)}"
    RECORDS[cid] = rec
    return rec


def ceil_div(a, b):
    return -(-a // b)


def grid_for(items):
    return min(max(ceil_div(items, 256), 1), 2048)


def both_ends(want, strict=False):
    if strict:
        assert want.min() == 0 and want.max() == 255, (want.min(), want.max())
    else:
        assert want.min() < 30 and want.max() > 220, (want.min(), want.max())


# =====================================================================================================================================
# contractions
# =====================================================================================================================================
def set_env(monkeypatch, v2, nst=None, v2_tile=None, tile=None, wgm=None):
    for k, v in (("OSG_QU8_V2", v2), ("OSG_QU8_NST", nst), ("OSG_QU8_V2_TILE", v2_tile), ("OSG_QU8_TILE", tile), ("OSG_QU8_WGM", wgm)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    monkeypatch.delenv("OSG_QU8_DBG", raising=False)


V2_CONFIGS = [(64, 64, 2), (64, 64, 3), (64, 64, 4), (128, 128, 2), (128, 128, 3), (128, 128, 4), (256, 128, 2), (256, 128, 3)]      # (BM, BN, NST)


def set_v2(monkeypatch, bm, bn, nst):
    set_env(monkeypatch, 2, nst=nst, v2_tile=bn if bm != 256 else 128, wgm=4 if bm == 256 else 2)


def gemm_operands(rng, batch, M, N, K, lda, stride_a, stride_b, a_codes=None, b_codes=None):
    """(a [batch, M, K], its pitched device image, b [batch or 1, N, K], its device image): the gaps of the pitched images hold random codes"""
    sa = stride_a if batch > 1 else M * lda
    abuf = codes(rng, (batch * sa,))
    a = np.stack([abuf[z * sa:z * sa + M * lda].reshape(M, lda)[:, :K] for z in range(batch)])
    if a_codes is not None:
        for z in range(batch):
            abuf[z * sa:z * sa + M * lda].reshape(M, lda)[:, :K] = a_codes[z]
        a = a_codes
    nb = batch if stride_b else 1
    sb = stride_b if stride_b else N * K
    bbuf = codes(rng, (nb * sb,))
    if b_codes is not None:
        bbuf[:N * K] = b_codes.reshape(-1)
    b = np.stack([bbuf[z * sb:z * sb + N * K].reshape(N, K) for z in range(nb)])
    return a, abuf, b, bbuf


def gemm_bias(rng, N, aq, bq):
    """a bias of both signs whose b / (sx sw) lies a quarter to three quarters of the way between two integers: the truncation of the epilogue shows"""
    ab = f32(aq[0]) * f32(bq[0])
    bias = ((np.trunc(rng.standard_normal(N) * 9000.0) + rng.uniform(0.25, 0.75, N) * np.where(rng.random(N) < 0.5, -1, 1)) * float(ab)).astype(f32)
    r = bias / ab
    assert (bias > 0).any() and (bias < 0).any() and (np.abs(r - np.rint(r)) > 0.2).all()
    return bias


def run_gemm(gpu, dev, cid, rec_want, batch, M, N, K, lda, stride_a, stride_b, stride_c, aq, bq, oq, bias, a, abuf, b, bbuf, strict=False):
    """one osg_qu8_gemm launch on pitched operands against matmul_u8 (+ the truncated bias); the output's gaps must stay 0xFF"""
    acc = np.matmul(a.astype(np.int64) - aq[1], np.swapaxes(b, -1, -2).astype(np.int64) - bq[1])
    if bias is not None:
        acc = acc + Q.conv_bias_i32(bias, aq[0], bq[0]).astype(np.int64)
    want = Q.requant_fp32(acc.astype(np.int32), f32(f32(aq[0]) * f32(bq[0])) / f32(oq[0]), oq[1])
    if bias is None:
        assert np.array_equal(want, Q.matmul_u8(a, aq[0], aq[1], np.swapaxes(b, -1, -2), bq[0], bq[1], oq[0], oq[1]))
    both_ends(want, strict)
    sc = stride_c if batch > 1 else M * N
    span = (batch - 1) * sc + M * N
    out = Out(dev, (span,))
    dA = dev(abuf).view(0, (batch, M, K) if batch > 1 else (M, K))
    dB = dev(bbuf).view(0, (batch, N, K) if stride_b and batch > 1 else (N, K))
    gpu.qu8_gemm(dA, aq, dB, bq, dev(bias) if bias is not None else None, oq, out=out.view, lda=lda, stride_a=stride_a if batch > 1 else 0,
                 stride_b=stride_b if batch > 1 else 0, stride_c=sc if batch > 1 else 0)
    record(gpu, cid, rec_want)
    full = np.full(span, 0xFF, u8)
    for z in range(batch):
        full[z * sc:z * sc + M * N] = want[z].reshape(-1)
    same(out.read(), full, cid)


GEMM_V1 = [("scalar", 70, 37, 72, 75, None, (64, 64, 0)), ("vec-t64", 130, 132, 80, 96, 64, (64, 64, 2)), ("vec-t128", 130, 132, 80, 96, 128, (128, 128, 2))]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("batch", [1, 3], ids=["dense", "batch3-strided"])
@pytest.mark.parametrize("name,M,N,K,lda,tile,inst", GEMM_V1, ids=[g[0] for g in GEMM_V1])
def test_gemm_register_staged(gpu, dev, monkeypatch, name, M, N, K, lda, tile, inst, batch, with_bias):
    set_env(monkeypatch, 0, tile=tile)
    rng = np.random.default_rng(M * 1000 + N + batch * 7 + with_bias)
    vec = inst[2] == 2
    stride_a = M * lda + (32 if vec else 7)            # (the 16-byte staging needs strides that keep the alignment; the scalar one gets an odd stride)
    stride_c = M * N + (8 if N % 4 == 0 else 5)        # (with N % 4 == 0 the epilogue stores four codes at a time: the stride keeps them aligned)
    a, abuf, b, bbuf = gemm_operands(rng, batch, M, N, K, lda, stride_a, 0)
    aq, bq = (f32(0.021), 140), (f32(0.0105), 99)
    oq = (f32(float(aq[0]) * float(bq[0]) * np.sqrt(K) * 75.0 / 2.0), 128)
    bias = gemm_bias(rng, N, aq, bq) if with_bias else None
    bm, bn, flags = inst
    cid = f"gemm-v1-{name}-b{batch}-{'bias' if with_bias else 'nobias'}"
    run_gemm(gpu, dev, cid, (Q8C, 1, bm, bn, 0, flags, ceil_div(M, bm) * ceil_div(N, bn) * batch, 0), batch, M, N, K, lda, stride_a, 0, stride_c, aq, bq, oq,
             bias, a, abuf, b, bbuf)


@pytest.mark.parametrize("bm,bn,nst", V2_CONFIGS, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in V2_CONFIGS])
def test_gemm_pipelined(gpu, dev, monkeypatch, bm, bn, nst):
    set_v2(monkeypatch, bm, bn, nst)
    batch, M, N, K, lda = 2, 200, 132, 256, 272
    rng = np.random.default_rng(bm + nst)
    stride_a, stride_b, stride_c = M * lda + 48, N * K + 32, M * N + 8
    a, abuf, b, bbuf = gemm_operands(rng, batch, M, N, K, lda, stride_a, stride_b)
    aq, bq = (f32(0.021), 140), (f32(0.0105), 99)
    oq = (f32(float(aq[0]) * float(bq[0]) * np.sqrt(K) * 75.0 / 2.0), 128)
    bias = gemm_bias(rng, N, aq, bq)
    flags = 2 | (4 if bm == 256 else 0)
    run_gemm(gpu, dev, f"gemm-v2-{bm}x{bn}x{nst}", (Q8C, 2, bm, bn, nst, flags, ceil_div(M, bm) * ceil_div(N, bn) * batch, 0), batch, M, N, K, lda, stride_a,
             stride_b, stride_c, aq, bq, oq, bias, a, abuf, b, bbuf)


@pytest.mark.parametrize("bm", [64, 128])
def test_gemm_pipelined_one_k_tile_on_a_ring_of_four(gpu, dev, monkeypatch, bm):
    set_v2(monkeypatch, bm, bm, 4)
    M, N, K = 200, 132, 128
    rng = np.random.default_rng(bm)
    a, abuf, b, bbuf = gemm_operands(rng, 1, M, N, K, K, 0, 0)
    aq, bq = (f32(0.021), 140), (f32(0.0105), 99)
    oq = (f32(float(aq[0]) * float(bq[0]) * np.sqrt(K) * 75.0 / 2.0), 128)
    run_gemm(gpu, dev, f"gemm-v2-{bm}-k128-nst4", (Q8C, 2, bm, bm, 4, 2, ceil_div(M, bm) * ceil_div(N, bm), 0), 1, M, N, K, K, 0, 0, 0, aq, bq, oq, None, a, abuf, b,
             bbuf)


@pytest.mark.parametrize("zo", [0, 128, 255])
def test_gemm_requantisation_ties(gpu, dev, monkeypatch, zo):
    """sx sw / so = 0.25 * 0.5 / 0.25 = 0.5 exactly: every odd accumulator is a tie, rounded to the even code"""
    set_env(monkeypatch, 0)
    M, N, K = 70, 37, 64
    rng = np.random.default_rng(zo)
    za, zb = 140, 99
    a = (za + rng.integers(-10, 11, (1, M, K))).astype(u8)
    b = (zb + rng.integers(-10, 11, (1, N, K))).astype(u8)
    acc = np.matmul(a[0].astype(np.int64) - za, b[0].T.astype(np.int64) - zb)
    ties = (acc % 2 != 0) & (acc // 2 + zo > 0) & (acc // 2 + zo < 254)
    assert ties.sum() > 100 and (acc[ties] % 4 == 1).any() and (acc[ties] % 4 == 3).any()          # ties that round down and ties that round up
    _, abuf, _, bbuf = gemm_operands(rng, 1, M, N, K, K, 0, 0, a_codes=a, b_codes=b)
    run_gemm(gpu, dev, f"gemm-ties-zo{zo}", (Q8C, 1, 64, 64, 0, 2, 2, 0), 1, M, N, K, K, 0, 0, 0, (f32(0.25), za), (f32(0.5), zb), (f32(0.25), zo), None, a, abuf,
             b, bbuf, strict=True)


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------
CONVS = {   # name: (H, W, KH, KW, (sh, sw), (pt, pl, pb, pr), weight zero point, halo correction of the pipelined kernel)
    "3x3-s2-pads-bottom-right": (10, 12, 3, 3, (2, 2), (0, 0, 1, 1), 255, True),       # even H, W: the last window reaches into the bottom / right pad
    "3x3-s2-pad-bottom": (10, 11, 3, 3, (2, 2), (0, 0, 1, 0), 131, True),               # the halo rule's second clause alone
    "3x3-s2-pad-right": (9, 12, 3, 3, (2, 2), (0, 0, 0, 1), 131, True),                 # its third clause alone
    "3x3-pads-1002": (9, 11, 3, 3, (1, 1), (1, 0, 0, 2), 0, True),
    "1x3": (9, 11, 1, 3, (1, 1), (0, 1, 0, 1), 131, True),
    "3x1": (9, 11, 3, 1, (1, 1), (1, 0, 1, 0), 131, True),
    "3x3-stride-2-1": (9, 11, 3, 3, (2, 1), (1, 1, 1, 1), 131, True),
    "1x1-nopads": (9, 11, 1, 1, (1, 1), (0, 0, 0, 0), 131, False),
}
CN, CH, CW, CIN, COUT = 2, 9, 11, 128, 68


def halo_rule(H, W, KH, KW, stride, pads):
    """try_q8v2's: a tap of some output pixel falls outside the image"""
    Ho, Wo = (H + pads[0] + pads[2] - KH) // stride[0] + 1, (W + pads[1] + pads[3] - KW) // stride[1] + 1
    return bool(pads[0] or pads[1] or (Ho - 1) * stride[0] - pads[0] + KH > H or (Wo - 1) * stride[1] - pads[1] + KW > W)
SX, SW = f32(0.0173), f32(0.0042)


def conv_case(rng, KH, KW, zx, zw, cin=CIN, with_bias=True, H=CH, W=CW):
    """inputs of one convolution and output parameters under which both ends of the code range are reached whatever the zero points: the bias takes the mean
    of the accumulators out (it depends on the zero points alone), the output scale follows their spread"""
    x, w = codes(rng, (CN, H, W, cin)), codes(rng, (COUT, KH, KW, cin))
    K = KH * KW * cin
    rx, rw = np.hypot(73.9, 127.5 - zx), np.hypot(73.9, 127.5 - zw)
    sxw = float(SX) * float(SW)
    bias = None
    if with_bias:
        bias = (-K * (127.5 - zx) * (127.5 - zw) * sxw + rng.standard_normal(COUT) * 0.5).astype(f32)
    oq = (f32(sxw * np.sqrt(K) * rx * rw / 100.0), 120)
    return x, w, bias, oq


def conv_launch(gpu, dev, cid, rec_want, x, zx, w, zw, bias, oq, stride, pads, want, dw=None, dx=None, taps=None):
    out = Out(dev, want.shape)
    gpu.qu8_conv2d_nhwc(dx if dx is not None else dev(x), (SX, zx), dw if dw is not None else dev(w), (SW, zw), dev(bias) if bias is not None else None, oq, stride, pads,
                        tap_sums=taps, out=out.view)
    record(gpu, cid, rec_want)
    same(out.read(), want, cid)


@pytest.mark.parametrize("name", list(CONVS))
def test_conv_every_instantiation(gpu, dev, monkeypatch, name):
    """one convolution shape on all 8 pipelined instantiations and on both tiles of the register-staged kernel; the padded ones at input zero points 0, 117, 255"""
    H, W, KH, KW, stride, pads, zw, halo = CONVS[name]
    Ho, Wo = (H + pads[0] + pads[2] - KH) // stride[0] + 1, (W + pads[1] + pads[3] - KW) // stride[1] + 1
    M = CN * Ho * Wo
    assert halo == halo_rule(H, W, KH, KW, stride, pads)
    if name == "3x3-s2-pad-bottom":
        assert (Ho - 1) * 2 + 3 > H and (Wo - 1) * 2 + 3 <= W
    if name == "3x3-s2-pad-right":
        assert (Ho - 1) * 2 + 3 <= H and (Wo - 1) * 2 + 3 > W
    for zx in ((117, 0, 255) if halo else (117,)):
        if zw in (0, 255) and zx != 117:
            continue                       # (the weight zero points 0 and 255 run once each, at the ordinary input zero point)
        rng = np.random.default_rng(KH * 100 + KW * 10 + zx)
        x, w, bias, oq = conv_case(rng, KH, KW, zx, zw, H=H, W=W)
        dx, dw = dev(x), dev(w)
        for b in ((bias, None) if zx == 117 and zw == 131 else (bias,)):
            want = Q.conv2d_nhwc_u8(x, SX, zx, w, SW, zw, b, pads, stride, oq[0], oq[1])
            assert want.shape == (CN, Ho, Wo, COUT)
            if b is not None:
                both_ends(want)
            for bm, bn, nst in V2_CONFIGS:
                set_v2(monkeypatch, bm, bn, nst)
                cid = f"conv-v2-{name}-zx{zx}-{bm}x{bn}x{nst}-{'bias' if b is not None else 'nobias'}"
                conv_launch(gpu, dev, cid, (Q8C, 2, bm, bn, nst, 3 | (4 if bm == 256 else 0), ceil_div(M, bm) * ceil_div(COUT, bn), 2 if halo else 0), x, zx, w, zw, b,
                            oq, stride, pads, want, dw, dx)
            for tile in (64, 128):
                set_env(monkeypatch, 0, tile=tile)
                conv_launch(gpu, dev, f"conv-v1-{name}-zx{zx}-t{tile}-{'bias' if b is not None else 'nobias'}",
                            (Q8C, 1, tile, tile, 0, 3, ceil_div(M, tile) * ceil_div(COUT, tile), 0), x, zx, w, zw, b, oq, stride, pads, want, dw, dx)


def test_conv_7x7_falls_back_to_the_register_staged_kernel(gpu, dev, monkeypatch):
    set_v2(monkeypatch, 64, 64, 4)
    rng = np.random.default_rng(77)
    x, w, bias, oq = conv_case(rng, 7, 7, 117, 131)
    pads = (3, 3, 3, 3)
    want = Q.conv2d_nhwc_u8(x, SX, 117, w, SW, 131, bias, pads, (1, 1), oq[0], oq[1])
    both_ends(want)
    M = CN * CH * CW
    conv_launch(gpu, dev, "conv-7x7", (Q8C, 1, 64, 64, 0, 3, ceil_div(M, 64) * ceil_div(COUT, 64), 0), x, 117, w, 131, bias, oq, 1, pads, want)


def test_conv_scalar_staging(gpu, dev, monkeypatch):
    """Cin = 20: a 16-code chunk straddles filter taps, q8_gemm_kernel<true, false, 64, 64>"""
    set_env(monkeypatch, 0)
    rng = np.random.default_rng(20)
    x, w, bias, oq = conv_case(rng, 3, 3, 117, 131, cin=20)
    pads = (1, 0, 0, 2)
    want = Q.conv2d_nhwc_u8(x, SX, 117, w, SW, 131, bias, pads, (1, 1), oq[0], oq[1])
    both_ends(want)
    conv_launch(gpu, dev, "conv-v1-cin20", (Q8C, 1, 64, 64, 0, 1, ceil_div(want.size // COUT, 64) * ceil_div(COUT, 64), 0), x, 117, w, 131, bias, oq, 1, pads, want)


def test_conv_tap_sums_from_the_caller(gpu, dev, monkeypatch):
    rng = np.random.default_rng(5)
    x, w, bias, oq = conv_case(rng, 3, 3, 117, 131)
    pads, stride = (1, 0, 0, 2), (1, 1)
    assert halo_rule(CH, CW, 3, 3, stride, pads)
    want = Q.conv2d_nhwc_u8(x, SX, 117, w, SW, 131, bias, pads, stride, oq[0], oq[1])
    both_ends(want)
    dw = dev(w)
    tbuf = dev.nan(COUT * 9 + 2 * GUARD, np.int32)
    taps = gpu.qu8_conv_tap_sums(dw, out=tbuf.view(GUARD, (COUT, 9)))
    raw = tbuf.numpy()
    assert (raw[:GUARD] == -1).all() and (raw[GUARD + COUT * 9:] == -1).all(), "a store landed in a guard band"
    same(raw[GUARD:GUARD + COUT * 9].reshape(COUT, 9), w.astype(np.int32).sum(-1).reshape(COUT, 9), "osg_qu8_conv_tap_sums")
    set_v2(monkeypatch, 64, 64, 4)
    wg = ceil_div(want.size // COUT, 64) * ceil_div(COUT, 64)
    conv_launch(gpu, dev, "conv-v2-taps-from-caller", (Q8C, 2, 64, 64, 4, 3, wg, 1), x, 117, w, 131, bias, oq, stride, pads, want, dw, taps=taps)
    conv_launch(gpu, dev, "conv-v2-taps-built", (Q8C, 2, 64, 64, 4, 3, wg, 2), x, 117, w, 131, bias, oq, stride, pads, want, dw)


# =====================================================================================================================================
# elementwise
# =====================================================================================================================================
SIG_IN, SIG_OUT = (f32(0.0713), 130), (f32(1.0 / 255), 0)


@pytest.mark.parametrize("n", [1, 255, 257, 524288 + 77])
@pytest.mark.parametrize("placed", [False, True], ids=["host-table", "device-table"])
def test_lut(gpu, dev, n, placed):
    rng = np.random.default_rng(n)
    x = codes(rng, (n,))
    if n >= 256:
        x[rng.permutation(n)[:256]] = np.arange(256, dtype=u8)
        assert len(np.unique(x)) == 256
    table = Q.sigmoid_u8(np.arange(256, dtype=u8), *SIG_IN, *SIG_OUT)
    out = Out(dev, (n,))
    gpu.qu8_lut(dev(x), dev(table) if placed else table, out=out.view)
    record(gpu, f"lut-{n}-{placed}", (Q8E, LUT, 0, grid_for(n)))
    assert n <= grid_for(n) * 256 or n == 524288 + 77          # only the last size takes a second trip of the loop
    same(out.read(), Q.sigmoid_u8(x, *SIG_IN, *SIG_OUT), f"lut n {n}")


GENERIC, SAME, PERIODIC, SWAPPED = 0, 1, 2, 3
BIN_SHAPES = [   # (id, a shape, b shape, byte offset of a / b / y, route)
    ("same-16k+5", (645,), (645,), 0, SAME),
    ("channel-nhwc", (1, 9, 7, 48), (48,), 0, PERIODIC),
    ("channel-nchw-hw35", (1, 20, 5, 7), (20, 1, 1), 0, PERIODIC),
    ("scalar-right", (3, 77), (), 0, PERIODIC),
    ("scalar-left", (1,), (3, 77), 0, SWAPPED),
    ("periodic-left", (32, 1, 1), (1, 32, 9, 7), 0, SWAPPED),
    ("rank6", (2, 3, 1, 5, 1, 4), (1, 3, 2, 1, 6, 4), 0, GENERIC),
    ("same-offset1", (645,), (645,), 1, GENERIC),
]
BIN_PARAMS = {   # kind: [(sa, za, sb, zb, so, zo, both ends exactly 0 and 255)]
    "add": [(0.031, 120, 0.017, 131, 0.045, 125, False), (0.02, 0, 0.02, 255, 0.012, 0, True), (0.02, 255, 0.013, 0, 0.012, 255, True)],
    "mul": [(0.031, 120, 0.017, 131, 0.0125, 125, False), (0.0042826, 0, 0.00154, 255, 0.00007, 255, True), (0.0042826, 255, 0.00154, 255, 0.00007, 0, True)],
}


def run_binary(gpu, dev, cid, kind, a, b, off, route, params, grid=None):
    fn = Q.add_u8 if kind == "add" else Q.mul_u8
    da, db = at(dev, a, off), at(dev, b, off)
    oshape = np.broadcast_shapes(a.shape, b.shape)
    n = int(np.prod(oshape))
    for sa, za, sb, zb, so, zo, strict in params:
        want = np.broadcast_to(fn(a, f32(sa), za, b, f32(sb), zb, f32(so), zo), oshape)
        if n > 1000:
            both_ends(want, strict)
        out = Out(dev, oshape, off)
        gpu.qu8_binary(kind, da, (f32(sa), za), db, (f32(sb), zb), (f32(so), zo), out=out.view)
        record(gpu, f"{cid}-za{za}-zo{zo}", (Q8E, BINARY, route | (4 if kind == "mul" else 0), grid_for(n) if route == GENERIC else grid_for(n // 16 + 1)))
        same(out.read(), want, f"{cid} zero points {za} {zb} {zo}")


@pytest.mark.parametrize("kind", ["add", "mul"])
@pytest.mark.parametrize("cid,ash,bsh,off,route", BIN_SHAPES, ids=[s[0] for s in BIN_SHAPES])
def test_binary(gpu, dev, kind, cid, ash, bsh, off, route):
    rng = np.random.default_rng(len(cid) * 31 + len(ash))
    run_binary(gpu, dev, f"binary-{kind}-{cid}", kind, codes(rng, ash), codes(rng, bsh), off, route, BIN_PARAMS[kind])


@pytest.mark.parametrize("kind", ["add", "mul"])
def test_binary_second_trip_of_the_generic_loop(gpu, dev, kind):
    rng = np.random.default_rng(55)
    assert 1100 * 100 * 5 > 2048 * 256
    run_binary(gpu, dev, f"binary-{kind}-generic-550000", kind, codes(rng, (1100, 1, 5)), codes(rng, (1, 100, 1)), 0, GENERIC, BIN_PARAMS[kind][:1])


@pytest.mark.parametrize("kind", ["add", "mul"])
def test_binary_second_trip_and_tail_of_the_fast_kernel(gpu, dev, kind):
    n = (1 << 23) + 53
    assert n // 16 > 2048 * 256 and n % 16
    rng = np.random.default_rng(23)
    run_binary(gpu, dev, f"binary-{kind}-same-2^23+53", kind, codes(rng, (n,)), codes(rng, (n,)), 0, SAME, BIN_PARAMS[kind][:1])


def test_binary_mul_requantisation_ties(gpu, dev):
    """sa sb / so = 0.5 exactly: every odd product is a tie"""
    rng = np.random.default_rng(9)
    za, zb = 120, 131
    a, b = (za + rng.integers(-20, 21, (645,))).astype(u8), (zb + rng.integers(-20, 21, (645,))).astype(u8)
    prod = (a.astype(int) - za) * (b.astype(int) - zb)
    assert ((prod % 4 == 1) & (abs(prod) < 200)).any() and ((prod % 4 == 3) & (abs(prod) < 200)).any()
    run_binary(gpu, dev, "binary-mul-ties", "mul", a, b, 0, SAME, [(0.25, za, 0.5, zb, 0.25, zo, zo != 128) for zo in (0, 128, 255)])


def test_binary_add_refuses_a_shift_outside_1_to_31(gpu, dev):
    rng = np.random.default_rng(4)
    a, b = codes(rng, (645,)), codes(rng, (645,))
    before = gpu.last_kernel()
    for sa, so in ((2.0, 2.0 ** -20), (2.0 ** -12, 1.0)):            # the larger ratio 2^21 -> shift -1; 2^-12 -> shift 32
        out = Out(dev, (645,))
        with pytest.raises(OsgError, match="scale ratio out of the range of the fixed-point add"):
            gpu.qu8_binary("add", dev(a), (f32(sa), 3), dev(b), (f32(sa), 5), (f32(so), 7), out=out.view)
        out.untouched()
    assert gpu.last_kernel() == before


AQ = dict(xq=(f32(0.021), 118), gq=(f32(0.011), 90), mq=(f32(0.024), 121), bq=(f32(0.013), 140), aq=(f32(0.027), 117), sq=(f32(1 / 256), 0), oq=(f32(0.012), 15))


def affine_spec(x, g, b, act, xq):
    """Mul(x, g) -> Add(., b) [-> Sigmoid -> Mul] composed from the specification's ops; g, b broadcast against x"""
    m = Q.mul_u8(x, *xq, g, *AQ["gq"], *AQ["mq"])
    a = Q.add_u8(m, *AQ["mq"], b, *AQ["bq"], *AQ["aq"])
    if not act:
        return a
    return Q.mul_u8(a, *AQ["aq"], Q.sigmoid_u8(a, *AQ["aq"], *AQ["sq"]), *AQ["sq"], *AQ["oq"])


def sig_table():
    return Q.sigmoid_u8(np.arange(256, dtype=u8), *AQ["aq"], *AQ["sq"])


AFFINE_CASES = [("nhwc-77x48", 77, 48, False, 0, 0), ("nhwc-7x5", 7, 5, False, 0, 0), ("nchw-40x63", 63, 40, True, 0, 0), ("nhwc-x-offset1", 77, 48, False, 1, 0),
          ("nchw-y-offset1", 63, 40, True, 0, 1)]


@pytest.mark.parametrize("act", [False, True], ids=["affine", "affine-silu"])
@pytest.mark.parametrize("cid,HW,C,nchw,xoff,yoff", AFFINE_CASES, ids=[c[0] for c in AFFINE_CASES])
def test_affine_act(gpu, dev, cid, HW, C, nchw, xoff, yoff, act):
    rng = np.random.default_rng(HW * C + act)
    shape = (C, HW) if nchw else (HW, C)
    x, g, b = codes(rng, shape), codes(rng, (C,)), codes(rng, (C,))
    cs = (C, 1) if nchw else (C,)
    want = affine_spec(x, g.reshape(cs), b.reshape(cs), act, AQ["xq"])
    n = HW * C
    if n > 1000:
        both_ends(want)
    assert (n % 16 != 0) == (cid in ("nhwc-7x5", "nchw-40x63", "nchw-y-offset1"))
    out = Out(dev, shape, yoff)
    gpu.qu8_affine_act(at(dev, x, xoff), AQ["xq"], dev(g), AQ["gq"], AQ["mq"], dev(b), AQ["bq"], AQ["aq"], dev(sig_table()) if act else None, AQ["sq"], AQ["oq"], C,
                       HW if nchw else 1, out=out.view)
    record(gpu, f"affine-{cid}-{act}", (Q8E, AFFINE_ACT, int(act), grid_for(n // 16 + 1)))
    same(out.read(), want, f"affine_act {cid} act {act}")


# =====================================================================================================================================
# normalisation
# =====================================================================================================================================
NQ_IN, NQ_OUT = (f32(0.0193), 113), (f32(0.0291), 128)


def norm_rows_spec(rows, scale, bias, eps, xq, oq):
    """instance_norm_u8 on [R, L] rows with scale / bias of n_scale entries: row r takes entry r % n_scale"""
    ns = len(scale)
    assert rows.shape[0] % ns == 0
    return np.concatenate([Q.instance_norm_u8(rows[i:i + ns][None], xq[0], xq[1], scale, bias, eps, oq[0], oq[1])[0] for i in range(0, rows.shape[0], ns)])


def test_instance_norm_pieces_and_misaligned_rows(gpu, dev):
    rows, L = 3, 65536 + 77
    rng = np.random.default_rng(rows + L)
    x = bell(rng, (rows, L))
    scale, bias = (1.0 + 0.1 * rng.standard_normal(rows)).astype(f32), (0.1 * rng.standard_normal(rows)).astype(f32)
    want = norm_rows_spec(x, scale, bias, 1e-6, NQ_IN, NQ_OUT)
    out = Out(dev, (rows, L))
    gpu.qu8_instance_norm(dev(x), NQ_IN, dev(scale), dev(bias), 1e-6, NQ_OUT, out=out.view)
    record(gpu, "inorm-3x65613", (Q8E, INORM, 0, 2 * rows, 2))
    same(out.read(), want, "instance_norm 3 x 65613")


def test_instance_norm_row_modulo_scales_constant_and_two_valued_rows(gpu, dev):
    rng = np.random.default_rng(2418)
    x = bell(rng, (2, 4, 1000))
    x[0, 1] = 77                                                   # variance 0
    x[1, 2] = np.where(rng.random(1000) < 0.4, 0, 255)             # codes 0 and 255 alone
    scale, bias = (1.0 + 0.1 * rng.standard_normal(4)).astype(f32), (0.1 * rng.standard_normal(4)).astype(f32)
    want = norm_rows_spec(x.reshape(8, 1000), scale, bias, 1e-6, NQ_IN, NQ_OUT).reshape(2, 4, 1000)
    assert len(np.unique(want[0, 1])) == 1 and len(np.unique(want[1, 2])) == 2
    out = Out(dev, (2, 4, 1000))
    gpu.qu8_instance_norm(dev(x), NQ_IN, dev(scale), dev(bias), 1e-6, NQ_OUT, out=out.view)
    record(gpu, "inorm-2x4x1000", (Q8E, INORM, 0, 8, 1))
    same(out.read(), want, "instance_norm [2, 4, 1000], four scales")


def nhwc_rows(x, G):
    """[HW, C] NHWC codes -> the [G, HW * cpg] rows of the [1, G, L] InstanceNormalization, in (pixel, channel) order"""
    HW, C = x.shape
    return np.ascontiguousarray(x.reshape(HW, G, C // G).transpose(1, 0, 2)).reshape(G, HW * (C // G))


def rows_nhwc(rows, HW, C):
    G = rows.shape[0]
    return np.ascontiguousarray(rows.reshape(G, HW, C // G).transpose(1, 0, 2)).reshape(HW, C)


def norm_nhwc_spec(x, G, scale, bias, eps, xq, oq):
    return rows_nhwc(norm_rows_spec(nhwc_rows(x, G), scale, bias, eps, xq, oq), *x.shape)


def sh_of(cpg):
    return cpg.bit_length() - 1 if (cpg & (cpg - 1)) == 0 else -1


NHWC = [("C48-G48", 35, 48, 48, 0), ("C64-G16", 35, 64, 16, 0), ("C128-G8", 35, 128, 8, 0), ("C256-G8", 35, 256, 8, 0), ("C96-G8", 35, 96, 8, 0), ("C40-G5", 35, 40, 5, 0),
        ("C96-HW700", 700, 96, 8, 0), ("C64-offset8", 35, 64, 16, 8), ("C112-G56", 35, 112, 56, 0)]


@pytest.mark.parametrize("cid,HW,C,G,off", NHWC, ids=[c[0] for c in NHWC])
def test_instance_norm_nhwc(gpu, dev, cid, HW, C, G, off):
    rng = np.random.default_rng(HW + C + G)
    x = np.ascontiguousarray(bell(rng, (C, HW)).T)                 # a bell per channel
    scale, bias = (1 + rng.standard_normal(G) * 0.1).astype(f32), (rng.standard_normal(G) * 0.1).astype(f32)
    xq, oq = (f32(0.031), 121), (f32(0.024), 118)
    want = norm_nhwc_spec(x, G, scale, bias, 1e-5, xq, oq)
    n = HW * C
    if cid == "C96-HW700":
        assert n > 65536 and 65536 % C == 64
    out = Out(dev, (HW, C), off)
    gpu.qu8_instance_norm_nhwc(at(dev, x, off), G, xq, dev(scale), dev(bias), 1e-5, oq, out=out.view)
    record(gpu, f"inorm-nhwc-{cid}", (Q8E, INORM_NHWC, sh_of(C // G), ceil_div(n, 65536), 3 if C % 16 == 0 and off % 16 == 0 else 0))
    same(out.read(), want, f"instance_norm_nhwc {cid}")


@pytest.mark.parametrize("fused", [False, True], ids=["norm", "norm-affine"])
def test_nhwc_norms_refuse_57_groups(gpu, dev, fused):
    rng = np.random.default_rng(57)
    x, g, b = codes(rng, (35, 114)), codes(rng, (114,)), codes(rng, (114,))
    scale, bias = np.ones(57, f32), np.zeros(57, f32)
    out = Out(dev, (35, 114))
    before = gpu.last_kernel()
    with pytest.raises(OsgError, match="more than 56 groups"):
        if fused:
            gpu.qu8_norm_affine_act_nhwc(dev(x), 57, NQ_IN, dev(scale), dev(bias), 1e-5, AQ["xq"], dev(g), AQ["gq"], AQ["mq"], dev(b), AQ["bq"], AQ["aq"], None, AQ["sq"],
                                         AQ["oq"], out=out.view)
        else:
            gpu.qu8_instance_norm_nhwc(dev(x), 57, NQ_IN, dev(scale), dev(bias), 1e-5, NQ_OUT, out=out.view)
    out.untouched()
    assert gpu.last_kernel() == before


CHANNEL_TABLES, GROUP_TABLES = 0, 1
NORM_AFFINE_CASES = [("C96-HW5", 5, 96, 8, 0), ("C96-HW64", 64, 96, 8, 0), ("C96-HW231", 231, 96, 8, 0), ("C320-HW5", 5, 320, 32, 0), ("C320-HW64", 64, 320, 32, 0),
                     ("C320-HW231", 231, 320, 32, 0), ("C40-G5", 77, 40, 5, 0), ("C64-offset1", 35, 64, 16, 1)]


@pytest.mark.parametrize("act", [False, True], ids=["affine", "affine-silu"])
@pytest.mark.parametrize("cid,HW,C,G,off", NORM_AFFINE_CASES, ids=[c[0] for c in NORM_AFFINE_CASES])
def test_norm_affine_act_nhwc(gpu, dev, cid, HW, C, G, off, act):
    rng = np.random.default_rng(HW * C + G + act)
    x = np.ascontiguousarray(bell(rng, (C, HW)).T)
    scale, bias = (1 + rng.standard_normal(G) * 0.1).astype(f32), (rng.standard_normal(G) * 0.1).astype(f32)
    g, b = codes(rng, (C,)), codes(rng, (C,))
    xq, nq = (f32(0.031), 121), (f32(0.024), 118)
    want = affine_spec(norm_nhwc_spec(x, G, scale, bias, 1e-5, xq, nq), g, b, act, nq)
    if HW * C > 1000:
        both_ends(want)
    route = CHANNEL_TABLES if C % 16 == 0 and off % 16 == 0 else GROUP_TABLES
    wg = ceil_div(HW, 64) * ceil_div(C, 128) if route == CHANNEL_TABLES else grid_for(HW * C // 16 + 1)
    out = Out(dev, (HW, C), off)
    gpu.qu8_norm_affine_act_nhwc(at(dev, x, off), G, xq, dev(scale), dev(bias), 1e-5, nq, dev(g), AQ["gq"], AQ["mq"], dev(b), AQ["bq"], AQ["aq"],
                                 dev(sig_table()) if act else None, AQ["sq"], AQ["oq"], out=out.view)
    record(gpu, f"norm-affine-{cid}-{act}", (Q8E, NORM_AFFINE, route | (2 if act else 0), wg, sh_of(C // G)))
    same(out.read(), want, f"norm_affine_act_nhwc {cid} act {act}")


# =====================================================================================================================================
# softmax
# =====================================================================================================================================
SOFTMAX_IN = f32(0.0625)


def softmax_table(C):
    qscale = min(float(np.iinfo(np.uint32).max) / C, 8388607.0)
    return np.rint(qscale * np.exp((np.arange(256, dtype=np.float64) - 255.0) * float(SOFTMAX_IN))).astype(np.uint32)


def run_softmax(gpu, dev, cid, x, placed=False):
    rows, C = x.shape
    table = softmax_table(C)
    sums = table.astype(np.uint64)[x.astype(np.int64) + 255 - x.max(-1, keepdims=True).astype(np.int64)].sum(-1) % (1 << 32)
    assert (sums != 0).all(), f"{cid}: the 32-bit table sum of row {int(np.argmin(sums))} is 0"
    want, so, zo = Q.softmax_u8(x, SOFTMAX_IN, -1)
    out = Out(dev, (rows, C))
    gpu.qu8_softmax_last(dev(x), dev(table) if placed else table, out=out.view)
    record(gpu, cid, (Q8E, SOFTMAX, 0, rows))
    same(out.read(), want, cid)
    return want, sums


@pytest.mark.parametrize("C", [1, 3, 255, 256, 257, 4096, 5000])
def test_softmax(gpu, dev, C):
    rng = np.random.default_rng(C)
    rows = [np.clip(np.rint(rng.standard_normal((3, C)) * 30 + 120), 0, 255).astype(u8)]
    one = np.zeros((1, C), u8)
    one[0, C // 2] = 255
    rows.append(one)                                               # one code 255 among zeros
    if C != 4096:
        rows.append(np.zeros((1, C), u8))                          # (at 4096 channels a constant row sums to 0 modulo 2^32: left out, see the module docstring)
    if C <= 512:
        rows.append(np.full((1, C), 255, u8))
    run_softmax(gpu, dev, f"softmax-C{C}", np.concatenate(rows), placed=C % 2 == 0)


@pytest.mark.parametrize("C,wrapped", [(513, 32), (600, 104)])
def test_softmax_constant_rows_whose_sum_wraps(gpu, dev, C, wrapped):
    x = np.stack([np.zeros(C, u8), np.full(C, 255, u8), np.full(C, 91, u8), (np.arange(C) % 256).astype(u8)])
    want, sums = run_softmax(gpu, dev, f"softmax-wrap-C{C}", x)
    assert (sums[:3] == wrapped).all() and (want[:3] == 255).all()


# =====================================================================================================================================
def test_coverage():
    """every instantiation / route the dispatch can take without OSG_QU8_DBG has been seen by the cases above"""
    seen5 = {r[1:6] for r in RECORDS.values() if r[0] == Q8C}
    want5 = {(1, 64, 64, 0, 0), (1, 64, 64, 0, 2), (1, 128, 128, 0, 2), (1, 64, 64, 0, 1), (1, 64, 64, 0, 3), (1, 128, 128, 0, 3)}
    want5 |= {(2, bm, bn, nst, conv | 2 | (4 if bm == 256 else 0)) for bm, bn, nst in V2_CONFIGS for conv in (0, 1)}
    assert len(want5) == 22
    missing = sorted(want5 - seen5)
    assert not missing, f"contraction instantiations (kernel, BM, BN, NST, flags) never launched: {missing}"
    halo = {r[7] for r in RECORDS.values() if r[0] == Q8C and r[1] == 2 and r[5] & 1}
    assert halo == {0, 1, 2}, f"halo corrections seen: {sorted(halo)}"
    seen6 = {r[1:3] for r in RECORDS.values() if r[0] == Q8E}
    E_WANTED = {(LUT, 0), (INORM, 0), (SOFTMAX, 0), (AFFINE_ACT, 0), (AFFINE_ACT, 1)}
    E_WANTED |= {(BINARY, route | mul) for route in (GENERIC, SAME, PERIODIC, SWAPPED) for mul in (0, 4)}
    E_WANTED |= {(INORM_NHWC, sh) for sh in (0, 1, 2, 3, 4, 5, -1)}
    E_WANTED |= {(NORM_AFFINE, route | act) for route in (CHANNEL_TABLES, GROUP_TABLES) for act in (0, 2)}
    missing = sorted(E_WANTED - seen6)
    assert not missing, f"elementwise / normalisation routes (entry point, route) never launched: {missing}"
    paths = {r[4] for r in RECORDS.values() if r[0] == Q8E and r[1] == INORM_NHWC}
    assert paths == {0, 3}, f"NHWC norm: 16-byte / scalar paths seen: {sorted(paths)}"
    pieces = {r[4] for r in RECORDS.values() if r[0] == Q8E and r[1] == INORM}
    assert pieces == {1, 2}, f"instance norm: pieces per row seen: {sorted(pieces)}"
