"""-m gpu: the argument values of the contraction kernels' leading scalar parameters that tests/test_contraction_instantiations.py does not reach.

gemm2_kernel and conv3x3_kernel take what their first DMA requests depend on as flat leading parameters (preloaded into scalar registers), derive the tile grid
(mt, nt) from M, N and the tile's size inside the kernel and unpack the k-slices and the walk order from one word; batch strides, the convolution geometry and
the epilogue come from the GemmParams behind them (onnxstream_amd/csrc/osg_gemm_common.h kernarg_pack).  The instantiation module runs every instantiation
through these signatures at 2 - 5 tiles per side; the cases here, with tiny K and N:

* more than 255 tiles down (mt) and across (nt): a tile count that a byte-wide field would wrap;
* 2 k-slices (the vector reduce launch), 4 (folded in the kernel) and 12 (the 8-wide reduce launch), each with the m-major (M > N) and the n-major (N > M) walk;
* batch 3 (strideA / strideB / strideC come from the struct);
* an output view (ldc: columns 12 .. of rows 24 elements wider) of a 1 x 1 convolution;
* one 3 x 3 / stride 1 convolution through conv3x3_kernel and one stride-2 convolution through gemm2_kernel<CONV>, both with a ragged last row tile;
* host only, no launch: one past each packed field's limit is refused (osg_gemm_kernarg_check, osg_attention_kernarg_check), the limit itself is taken.

Not here: a row pitch of A other than K.  No entry point of include/osgpu.h hands gemm2_kernel one (osg_gemm, osg_gemm_ln, osg_gemm_rowstats and osg_gemm_w8 set
lda = K, a 1 x 1 convolution lda = Cin = K), so such a launch cannot be built from a test; the 32-bit pitch parameter carries K in every GEMM case of this file and of
the instantiation module, and its range check is among the host-only cases.

Every output element against float64 on the exact operands, under the bound and the cap on elements more than one f16 ulp off that
tests/test_contraction_instantiations.py derives (its helpers are imported, not copied); osg_last_route confirms the instantiation, k-slices, fold and reduce kernel.
"""
import numpy as np
import pytest

import test_contraction_instantiations as ci
from test_contraction_instantiations import ACT_NONE, CONV3X3, GEMM2, check, contraction, conv, gemm, im2col, knobs, reduce_kernel, rnd, slices, table

pytestmark = pytest.mark.gpu


def plain_entry():
    """the 64 x 64 f16 GEMM instantiation with the shallowest ring that also folds its split: (index, (cfg, nst, ks, spec) of a request that resolves to it)"""
    v2, _, req = table()
    own = [i for i, e in enumerate(v2) if (e["bm"], e["bn"]) == (64, 64) and not (e["conv"] or e["spec"] or e["ln"] or e["wq"]) and e["ks"] == 1 and e["fold"] and i in req]
    assert own, "no plain 64 x 64 entry"
    i = min(own, key=lambda i: v2[i]["nst"])
    return i, req[i]


def conv_entry64():
    v2, _, req = table()
    own = [i for i, e in enumerate(v2) if (e["bm"], e["bn"]) == (64, 64) and e["conv"] and not (e["spec"] or e["wq"]) and i in req]
    assert own, "no 64 x 64 convolution entry"
    i = min(own, key=lambda i: v2[i]["nst"])
    return i, req[i]


def force(mp, req, **kv):
    cfg, nst, ks, spec = req
    knobs(mp, OSG_GEMM_CFG=cfg, OSG_GEMM_NST=nst, OSG_GEMM_KS=ks, OSG_GEMM_SPEC=spec, **kv)


@pytest.mark.parametrize("M,N", [(64 * 256 + 1, 8), (8, 64 * 256 + 4)], ids=["mt257", "nt257"])
def test_more_than_255_tiles_per_side(gpu, monkeypatch, M, N):
    idx, req = plain_entry()
    K = 192
    rng = np.random.default_rng(31 * M + N)
    a, w, bias = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1)
    force(monkeypatch, req, OSG_GEMM_SPLITS=1)
    got, r = gemm(gpu, a, w, bias, None, ACT_NONE)
    assert r == (GEMM2, idx, 1, 0, 0), r
    check(got, *contraction(a, w, bias), f"{-(-M // 64)} x {-(-N // 64)} tiles")


@ci.FOLD_TIMEOUT
@pytest.mark.parametrize("M,N", [(200, 72), (72, 200)], ids=["m_major", "n_major"])
def test_k_slices_and_walk_order(gpu, monkeypatch, M, N):
    idx, req = plain_entry()
    K = 768                                            # 12 k-tiles
    rng = np.random.default_rng(977 * M + N)
    a, w, bias, res = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    pre, E = contraction(a, w, bias, res)
    for s, fold in ((2, 0), (4, 1), (12, 0)):
        force(monkeypatch, req, OSG_GEMM_SPLITS=s, OSG_GEMM_FOLD=fold)
        got, r = gemm(gpu, a, w, bias, res, ACT_NONE)
        assert r == (GEMM2, idx, slices(K // 64, s), fold, reduce_kernel(s, fold, N)), r
        check(got, pre, E, f"{s} k-slices, fold {fold}")


def test_batch_strides_come_from_the_struct(gpu, monkeypatch):
    idx, req = plain_entry()
    M, N, K = 70, 72, 192
    rng = np.random.default_rng(5)
    a, w, bias, res = rnd(rng, (3, M, K)), rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1), rnd(rng, (3, M, N))
    pre, E = contraction(a, w, bias, res)
    force(monkeypatch, req, OSG_GEMM_SPLITS=1)
    got, r = gemm(gpu, a, w, bias, res, ACT_NONE, batch=3)
    assert r == (GEMM2, idx, 1, 0, 0), r
    check(got, pre.reshape(3 * M, N), E.reshape(3 * M, N), "batch 3")


def test_output_view(gpu, monkeypatch):
    idx, req = plain_entry()
    M, N, K = 100, 72, 192
    rng = np.random.default_rng(6)
    x, w, bias, res = rnd(rng, (1, 10, 10, K)), rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    force(monkeypatch, req, OSG_GEMM_SPLITS=1)
    got, r = conv(gpu, x, w.reshape(N, 1, 1, K), bias, res, None, ACT_NONE, 1, 0, ld=N + 24, col=12)      # (Out.read: the 24 columns of the gap come back untouched)
    assert r == (GEMM2, idx, 1, 0, 0), r
    check(got, *contraction(x.reshape(M, K), w, bias, res), "1 x 1 convolution into a column view")


def test_halo_convolution_ragged_rows(gpu, monkeypatch):
    """3 x 3 / stride 1 at W = 8: three 8 x 8 images = 192 output rows, one and a half 128-row tiles of conv3x3_kernel"""
    _, v3, _ = table()
    idx = next(i for i, e in enumerate(v3) if e["w"] == 8 and e["bn"] == 80 and e["nlw"] == 4 and not e["wq"])
    cin, cout = 128, 72                                # (two 64-channel slabs)
    rng = np.random.default_rng(7)
    x, w = rnd(rng, (3, 8, 8, cin)), rnd(rng, (cout, 3, 3, cin), (9 * cin) ** -0.5)
    bias, ib = rnd(rng, (cout,), 0.1), rnd(rng, (3, cout), 0.5)
    cols, _, _ = im2col(x, 3, 1, 1)
    res = rnd(rng, (cols.shape[0], cout))
    knobs(monkeypatch, OSG_CONV3X3_BN=80, OSG_CONV3X3_NL=4, OSG_CONV3X3_SPLITS=1)
    got, r = conv(gpu, x, w, bias, res, ib, ACT_NONE, 1, 1)
    assert r == (CONV3X3, idx, 1, 0, 0), r
    check(got, *contraction(cols, w.reshape(cout, -1), bias, res, np.repeat(ib, 64, axis=0)), "3 x 3, 192 rows")


def test_strided_convolution_ragged_rows(gpu, monkeypatch):
    """3 x 3 / stride 2 over one 18 x 18 image: 81 output rows, a 64-row tile and 17 rows of gemm2_kernel<CONV> (H, W, Ho, Wo, strides and pads from the struct)"""
    idx, req = conv_entry64()
    cin, cout = 64, 72
    rng = np.random.default_rng(8)
    x, w, bias = rnd(rng, (1, 18, 18, cin)), rnd(rng, (cout, 3, 3, cin), (9 * cin) ** -0.5), rnd(rng, (cout,), 0.1)
    cols, ho, wo = im2col(x, 3, 2, 1)
    assert (ho, wo) == (9, 9)
    force(monkeypatch, req, OSG_GEMM_SPLITS=1)
    got, r = conv(gpu, x, w, bias, None, None, ACT_NONE, 2, 1)
    assert r == (GEMM2, idx, 1, 0, 0), r
    check(got, *contraction(cols, w.reshape(cout, -1), bias), "3 x 3 / stride 2, 81 rows")


# ---- host only: the range checks of the packed parameters, no launch ---------------------------------------------------------------------------------------
def refused(gpu, rc, what):
    assert rc == 1, f"{what}: accepted"
    msg = gpu.lib.osg_last_error(gpu.ctx).decode()
    assert "kernel parameter" in msg, msg


def test_contraction_fields_one_past_the_limit(gpu):
    chk = gpu.lib.osg_gemm_kernarg_check
    assert chk(gpu.ctx, 2 ** 31 - 1, 2 ** 16 - 1) == 0            # the limits themselves fit: a 32-bit signed pitch, 16 bits of k-slices
    assert chk(gpu.ctx, 0, 1) == 0                                # (a convolution has no pitch)
    refused(gpu, chk(gpu.ctx, 2 ** 31, 1), "a row pitch of 2^31 elements")
    refused(gpu, chk(gpu.ctx, -1, 1), "a negative row pitch")
    refused(gpu, chk(gpu.ctx, 64, 2 ** 16), "2^16 k-slices")
    refused(gpu, chk(gpu.ctx, 64, 0), "no k-slice")


def test_attention_fields_one_past_the_limit(gpu):
    chk = gpu.lib.osg_attention_kernarg_check
    assert chk(gpu.ctx, 2 ** 31 - 1, 2 ** 16 - 1, 2 ** 16 - 1) == 0
    refused(gpu, chk(gpu.ctx, 2 ** 31, 8, 1), "a key / value stride of 2^31 elements")
    refused(gpu, chk(gpu.ctx, 320, 2 ** 16, 1), "2^16 heads")
    refused(gpu, chk(gpu.ctx, 320, 8, 2 ** 16), "2^16 query heads per key / value head")
