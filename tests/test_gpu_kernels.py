"""-m gpu: every C-ABI entry point of libosgpu vs the numpy restatement of the reference arithmetic (oracle/np_ops.py).

Tolerances (written per test): integer/byte work bit-exact; f16 outputs within a few f16 ulps of the restatement
(summation order / polynomial-vs-libm exp), quoted relative to max|reference| as north_star asks (<= 1e-3).
"""
import numpy as np
import pytest

from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rnd(rng, shape, std=1.0, dtype=f16):
    return (rng.standard_normal(shape, dtype=f32) * std).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (4096, 320, 320), (77, 320, 768), (1, 1280, 320), (256, 1280, 1280),
                                   (64, 1280, 5120), (130, 72, 40), (33, 7, 36)])
def test_gemm(gpu, M, N, K):
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    a, b = rnd(rng, (M, K)), rnd(rng, (K, N), K ** -0.5)
    bias = rnd(rng, (N,), 0.1)
    res = rnd(rng, (M, N))
    want = ref.matmul(a, b, bias, res)
    da, db = gpu.to_dev(a), gpu.to_dev(b)
    got = gpu.gemm(da, db, gpu.to_dev(bias), gpu.to_dev(res)).numpy()
    assert rel_max(got, want) <= 1e-3
    # resident-weight layout [N,K]
    dbt = gpu.transpose_kn_to_nk(db)
    assert np.array_equal(dbt.numpy(), b.T)
    got2 = gpu.gemm(da, dbt, gpu.to_dev(bias.astype(f32)), gpu.to_dev(res), b_is_nk=True).numpy()
    assert rel_max(got2, want) <= 1e-3
    # asymmetric-operand transpose check: A = I must reproduce B exactly
    if M == K:
        eye = np.eye(M, dtype=f16)
        assert np.array_equal(gpu.gemm(gpu.to_dev(eye), db).numpy(), b)


@pytest.mark.parametrize("M,K,C", [(300, 128, 128), (8192, 320, 1280), (64, 1280, 5120)])
def test_gemm_geglu_epilogue(gpu, M, K, C):
    """Linear + GEGLU fused in the GEMM epilogue (pair-interleaved [N,K] weight) vs x[:, :C] * gelu_erf(x[:, C:])."""
    from scipy.special import erf
    rng = np.random.default_rng(M + K + C)
    a, w = rnd(rng, (M, K)), rnd(rng, (K, 2 * C), K ** -0.5)
    b = rnd(rng, (2 * C,), 0.1)
    x = a.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    v, g = x[:, :C], x[:, C:]
    want = v * 0.5 * g * (1.0 + erf(g / np.sqrt(2.0)))
    wt = w.T.copy()                                   # [N, K]
    wi = np.empty_like(wt)
    bi = np.empty_like(b)
    for k in range(C // 16):
        wi[32 * k:32 * k + 16] = wt[16 * k:16 * k + 16]
        wi[32 * k + 16:32 * k + 32] = wt[C + 16 * k:C + 16 * k + 16]
        bi[32 * k:32 * k + 16] = b[16 * k:16 * k + 16]
        bi[32 * k + 16:32 * k + 32] = b[C + 16 * k:C + 16 * k + 16]
    y = gpu.empty((M, C), f16)
    da, dw, db = gpu.to_dev(a), gpu.to_dev(wi), gpu.to_dev(bi)
    gpu._ck(gpu.lib.osg_gemm(gpu.ctx, 2, da.ptr, dw.ptr, 1, db.ptr, 2, None, y.ptr, M, 2 * C, K, 1, 0, 0, 0, 3))
    assert rel_max(y.numpy(), want) <= 1e-3


@pytest.mark.parametrize("M,K,N,geglu", [(300, 320, 320, False), (8192, 320, 960, False), (2048, 640, 640, False), (512, 1280, 1280, False),
                                          (130, 64, 36, False), (1024, 640, 5120, True), (128, 1280, 10240, True), (77, 1536, 64, True)])
def test_gemm_ln_folded_layer_norm(gpu, M, K, N, geglu):
    """LayerNorm folded into its consuming GEMM (osg_gemm_ln: gamma in the weight, row sums / sums of squares accumulated beside the MFMAs,
    beta and the mean correction in two fp32 epilogue vectors) vs LayerNorm -> Linear (+GEGLU) in float64.  Rows with a large common
    offset exercise the mean-correction and the single-pass variance cancellation."""
    from scipy.special import erf
    rng = np.random.default_rng(M + K + N)
    x = (rnd(rng, (M, K), 1.5).astype(f32) + rng.standard_normal((M, 1), dtype=f32) * 3.0).astype(f16)
    gamma, beta = (1 + rnd(rng, (K,), 0.2).astype(f32)).astype(f16), rnd(rng, (K,), 0.2)
    w = rnd(rng, (N, K), K ** -0.5)
    bias = rnd(rng, (N,), 0.1)
    x64 = x.astype(np.float64)
    ln = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * gamma.astype(np.float64) + beta.astype(np.float64)
    want = ln @ w.astype(np.float64).T + bias.astype(np.float64)
    wk, bk = w, bias
    if geglu:
        C = N // 2
        v, g = want[:, :C], want[:, C:]
        want = v * 0.5 * g * (1.0 + erf(g / np.sqrt(2.0)))
        wk, bk = np.empty_like(w), np.empty_like(bias)
        for k in range(C // 16):
            wk[32 * k:32 * k + 16] = w[16 * k:16 * k + 16]
            wk[32 * k + 16:32 * k + 32] = w[C + 16 * k:C + 16 * k + 16]
            bk[32 * k:32 * k + 16] = bias[16 * k:16 * k + 16]
            bk[32 * k + 16:32 * k + 32] = bias[C + 16 * k:C + 16 * k + 16]
    got = gpu.gemm_ln(gpu.to_dev(x), wk, gamma, beta, bk, 1e-5, act=3 if geglu else 0).numpy()
    assert rel_max(got, want) <= 1e-3
    if K % 32 == 0 and K <= 1280:
        # hand-over variant: x = the output of a GEMM that also emits partial row statistics (osg_gemm_rowstats); the consumer does no
        # statistics work of its own.  x = x0 . I + 0 reproduces x exactly, so `want` still applies.
        eye = gpu.to_dev(np.eye(K, dtype=f16))
        xd, rs = gpu.gemm_rowstats(gpu.to_dev(x), eye)
        assert np.array_equal(xd.numpy(), x)
        rsn = rs.numpy()
        x3 = x.astype(np.float64).reshape(M, K // 32, 32)
        assert np.allclose(rsn[..., 0], x3.sum(-1), rtol=1e-5, atol=1e-3) and np.allclose(rsn[..., 1], (x3 ** 2).sum(-1), rtol=1e-5, atol=1e-3)
        got2 = gpu.gemm_ln(xd, wk, gamma, beta, bk, 1e-5, act=3 if geglu else 0, rowstats=rs).numpy()
        assert rel_max(got2, want) <= 1e-3
    # against the unfused device sequence (LayerNorm rounds to f16 first): within the two paths' roundings
    if not geglu:
        lnd = gpu.layer_norm(gpu.to_dev(x), gpu.to_dev(gamma), gpu.to_dev(beta), 1e-5)
        two = gpu.gemm(lnd, gpu.to_dev(w), gpu.to_dev(bias), b_is_nk=True).numpy()
        assert rel_max(got, two.astype(np.float64)) <= 2e-3


@pytest.mark.parametrize("M,N,K,cfg,nst,splits", [(8192, 320, 320, 2, 2, 1), (8192, 320, 320, 2, 4, 1), (512, 1280, 1280, 2, 4, 1), (2048, 640, 640, 1, 2, 1), (8192, 320, 1280, 2, 4, 1),
                                                  (512, 1280, 5120, 2, 4, 3), (300, 200, 192, 2, 2, 1), (130, 72, 64, 2, 4, 1), (77, 320, 768, 1, 2, 1)])
def test_gemm_two_wave_groups_on_alternating_k_tiles(gpu, M, N, K, cfg, nst, splits, monkeypatch):
    """gemm2_kernel KS = 2 (round 3: 512 threads, group g of four waves takes the k-tiles g, g + 2, ..., partial accumulators added through LDS; a
    measured candidate of the tuner): odd and even tile counts, a single k-tile (group 1 runs only its zero-filled dummy), ragged M / N, bias +
    residual, split-K on top -- against the float64 product and against the one-group kernel (same value class, not the same fp32 summation order)."""
    rng = np.random.default_rng(M + N + K + nst)
    a, w = rnd(rng, (M, K)), rnd(rng, (K, N), K ** -0.5)
    bias, res = rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    da, dw, db, dr = gpu.to_dev(a), gpu.transpose_kn_to_nk(gpu.to_dev(w)), gpu.to_dev(bias), gpu.to_dev(res)
    monkeypatch.setenv("OSG_GEMM_CFG", str(cfg)); monkeypatch.setenv("OSG_GEMM_NST", str(nst)); monkeypatch.setenv("OSG_GEMM_SPLITS", str(splits))
    monkeypatch.setenv("OSG_GEMM_KS", "1")
    one = gpu.gemm(da, dw, db, dr, b_is_nk=True).numpy()
    monkeypatch.setenv("OSG_GEMM_KS", "2")
    two = gpu.gemm(da, dw, db, dr, b_is_nk=True).numpy()
    again = gpu.gemm(da, dw, db, dr, b_is_nk=True).numpy()
    want = ref.matmul(a, w, bias, res)
    assert np.array_equal(two, again)
    assert rel_max(two, want) <= 1e-3 and rel_max(one, want) <= 1e-3
    assert rel_max(two, one.astype(np.float64)) <= 1e-3


@pytest.mark.parametrize("tile", [4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K,nst,splits,fold", [(2048, 640, 640, 2, 1, 0), (512, 1280, 1280, 4, 1, 0), (8192, 320, 320, 4, 1, 0), (512, 1280, 5120, 4, 2, 0), (512, 1280, 5120, 4, 2, 1),
                                                 (300, 200, 192, 2, 1, 0), (130, 72, 64, 4, 1, 0), (77, 960, 768, 2, 1, 0), (1000, 2560, 320, 4, 1, 0)])
def test_gemm_160_and_80_column_tiles_give_the_bits_of_the_64x64_tile(gpu, tile, M, N, K, nst, splits, fold, monkeypatch):
    """Round 6 (osg_gemm_wide.hip): the 128x160 / 128x80 / 64x80 / 64x160 tiles of gemm2_kernel -- the waves as 4 x 1 (tiles 4 .. 6), a B stage padded to 96 rows
    for the 80-column tiles (pad rows never requested, never read), ragged M and N (N no multiple of 80 included: the tuner never picks the tiles there, the kernel
    must still be right), split-K with the reduce launch and folded by the last arriver.  Every output element is the same MFMA sequence whatever the tile (k
    ascending in steps of 32, f32 accumulate, one rounding), so at the same split of K the result must equal the 64x64 tile's BIT FOR BIT, bias + residual included."""
    if fold and tile in (4, 7):
        pytest.skip("the in-kernel fold is not offered for the 160-column tiles (20 accumulator quads per lane)")
    rng = np.random.default_rng(M + N + K + tile)
    a, w = rnd(rng, (M, K)), rnd(rng, (K, N), K ** -0.5)
    bias, res = rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    da, dw, db, dr = gpu.to_dev(a), gpu.transpose_kn_to_nk(gpu.to_dev(w)), gpu.to_dev(bias), gpu.to_dev(res)
    monkeypatch.setenv("OSG_GEMM_NST", str(nst)); monkeypatch.setenv("OSG_GEMM_SPLITS", str(splits)); monkeypatch.setenv("OSG_GEMM_KS", "1")
    monkeypatch.setenv("OSG_GEMM_FOLD", str(fold))
    monkeypatch.setenv("OSG_GEMM_CFG", "2")
    base = gpu.gemm(da, dw, db, dr, b_is_nk=True).numpy()
    monkeypatch.setenv("OSG_GEMM_CFG", str(tile))
    got = gpu.gemm(da, dw, db, dr, b_is_nk=True).numpy()
    assert rel_max(base, ref.matmul(a, w, bias, res)) <= 1e-3
    assert np.array_equal(got, base), (int((got != base).sum()), rel_max(got, base.astype(np.float64)))


def test_160_column_tiles_geglu_layer_norm_fold_and_convolution(gpu, monkeypatch):
    """... the forms osg_gemm_wide.hip holds beside the plain GEMM: the GEGLU epilogue on the 128x160 tile (10 column blocks per wave: value / gate pairs stay inside
    a wave), the LayerNorm-folding GEMM with handed-over row statistics on the 128x160 and 64x160 tiles, the implicit-GEMM convolution (3x3 stride 2) on tiles
    4 .. 6 -- each against the 128x64 / 64x64 tile's bits."""
    rng = np.random.default_rng(606)
    # GEGLU, plain and LayerNorm-folded (weights in any order: both tiles read the same interleaved matrix)
    M, K, N = 1024, 640, 5120
    a, w, b = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5), rnd(rng, (N,), 0.1)
    da, dw, db = gpu.to_dev(a), gpu.to_dev(w), gpu.to_dev(b)
    def geglu():
        y = gpu.empty((M, N // 2), f16)
        gpu._ck(gpu.lib.osg_gemm(gpu.ctx, 2, da.ptr, dw.ptr, 1, db.ptr, 2, None, y.ptr, M, N, K, 1, 0, 0, 0, 3))
        return y.numpy()
    monkeypatch.setenv("OSG_GEMM_NST", "2"); monkeypatch.setenv("OSG_GEMM_SPLITS", "1"); monkeypatch.setenv("OSG_GEMM_KS", "1")
    monkeypatch.setenv("OSG_GEMM_CFG", "1")
    base = geglu()
    monkeypatch.setenv("OSG_GEMM_CFG", "4")
    assert np.array_equal(geglu(), base)
    gamma, beta = (1 + rnd(rng, (K,), 0.2).astype(f32)).astype(f16), rnd(rng, (K,), 0.2)
    eye = gpu.to_dev(np.eye(K, dtype=f16))
    for act, n_out in ((3, N), (0, 1920)):
        wk, bk = w[:n_out], b[:n_out]
        for nst in (2, 4):
            monkeypatch.setenv("OSG_GEMM_NST", str(nst))
            monkeypatch.setenv("OSG_GEMM_CFG", "1")
            xd, rs = gpu.gemm_rowstats(da, eye)
            base = gpu.gemm_ln(xd, wk, gamma, beta, bk, 1e-5, act=act, rowstats=rs).numpy()
            for tile in ((4,) if act == 3 else (4, 7)):
                monkeypatch.setenv("OSG_GEMM_CFG", str(tile))
                got = gpu.gemm_ln(xd, wk, gamma, beta, bk, 1e-5, act=act, rowstats=rs).numpy()
                assert np.array_equal(got, base), (tile, act, nst, rel_max(got, base.astype(np.float64)))
    # a GEMM that also emits its output's partial row statistics (32-column slots): the 128x160 tile serves them (a wave's 160 columns = 5 whole slots from a
    # multiple of 32), the 80-column tiles and the 2 x 2 form of 64x160 do not and hand the launch back to a round-2 tile
    monkeypatch.setenv("OSG_GEMM_NST", "4")
    monkeypatch.setenv("OSG_GEMM_CFG", "2")
    wq = gpu.to_dev(rnd(rng, (640, K), K ** -0.5))
    yb, rb = gpu.gemm_rowstats(da, wq)
    for tile in (4, 5, 6, 7):
        monkeypatch.setenv("OSG_GEMM_CFG", str(tile))
        yt, rt = gpu.gemm_rowstats(da, wq)
        assert np.array_equal(yt.numpy(), yb.numpy()) and np.array_equal(rt.numpy(), rb.numpy()), tile
    # the downsampling convolution of the 32 x 32 level through the implicit-GEMM kernel
    x = rnd(rng, (2, 32, 32, 640))
    wc = rnd(rng, (640, 3, 3, 640), (640 * 9) ** -0.5)
    bc = rnd(rng, (640,), 0.1)
    dx, dwc, dbc = gpu.to_dev(x), gpu.to_dev(wc), gpu.to_dev(bc)
    monkeypatch.setenv("OSG_GEMM_NST", "4")
    monkeypatch.setenv("OSG_GEMM_CFG", "2")
    base = gpu.conv2d_nhwc(dx, dwc, dbc, 2, (1, 1, 1, 1)).numpy()
    assert rel_max(base, ref.conv2d_nhwc(x, wc, bc, (2, 2), (1,) * 4)) <= 1e-3
    for tile in (4, 5, 6):
        monkeypatch.setenv("OSG_GEMM_CFG", str(tile))
        got = gpu.conv2d_nhwc(dx, dwc, dbc, 2, (1, 1, 1, 1)).numpy()
        assert np.array_equal(got, base), (tile, rel_max(got, base.astype(np.float64)))
    # 64 x 80 with a 2-stage ring is no convolution instantiation: the 64 x 64 tile runs, and a folded split is sized for it (osg_gemm_routes.h resolve_v2)
    monkeypatch.setenv("OSG_GEMM_SPLITS", "2"); monkeypatch.setenv("OSG_GEMM_FOLD", "0"); monkeypatch.setenv("OSG_GEMM_CFG", "2")
    base = gpu.conv2d_nhwc(dx, dwc, dbc, 2, (1, 1, 1, 1)).numpy()
    monkeypatch.setenv("OSG_GEMM_NST", "2"); monkeypatch.setenv("OSG_GEMM_FOLD", "1"); monkeypatch.setenv("OSG_GEMM_CFG", "6")
    got = gpu.conv2d_nhwc(dx, dwc, dbc, 2, (1, 1, 1, 1)).numpy()
    assert np.array_equal(got.view(np.uint16), base.view(np.uint16))


def test_two_wave_groups_conv_and_folded_layer_norm(gpu, monkeypatch):
    """KS = 2 through the implicit-GEMM convolution (tap / channel position advanced by two k-tiles per step) and through the LayerNorm-folding GEMM with
    handed-over row statistics"""
    rng = np.random.default_rng(9)
    monkeypatch.setenv("OSG_GEMM_CFG", "2"); monkeypatch.setenv("OSG_GEMM_NST", "4"); monkeypatch.setenv("OSG_GEMM_SPLITS", "1")
    for (N, H, Cin, Cout, k, stride) in ((2, 32, 64, 128, 3, 2), (1, 24, 192, 96, 3, 1), (2, 16, 320, 64, 1, 1)):   # (stride 2, a width the halo kernel does not take, 1x1)
        x, w = rnd(rng, (N, H, H, Cin)), rnd(rng, (Cout, k, k, Cin), (k * k * Cin) ** -0.5)
        bias = rnd(rng, (Cout,), 0.1)
        dx, dw, db = gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias)
        pad = k // 2
        monkeypatch.setenv("OSG_GEMM_KS", "1")
        one = gpu.conv2d_nhwc(dx, dw, db, stride, (pad,) * 4).numpy()
        monkeypatch.setenv("OSG_GEMM_KS", "2")
        two = gpu.conv2d_nhwc(dx, dw, db, stride, (pad,) * 4).numpy()
        want = ref.conv2d_nhwc(x, w, bias, (stride, stride), (pad,) * 4)
        assert rel_max(two, want) <= 2e-3 and rel_max(two, one.astype(np.float64)) <= 1e-3
    M, K, Nn = 2048, 640, 640
    x = (rnd(rng, (M, K), 1.5).astype(f32) + rng.standard_normal((M, 1), dtype=f32) * 3.0).astype(f16)
    gamma, beta = (1 + rnd(rng, (K,), 0.2).astype(f32)).astype(f16), rnd(rng, (K,), 0.2)
    w, bias = rnd(rng, (Nn, K), K ** -0.5), rnd(rng, (Nn,), 0.1)
    x64 = x.astype(np.float64)
    ln = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * gamma.astype(np.float64) + beta.astype(np.float64)
    want = ln @ w.astype(np.float64).T + bias.astype(np.float64)
    monkeypatch.setenv("OSG_GEMM_KS", "1")
    xd, rs = gpu.gemm_rowstats(gpu.to_dev(x), gpu.to_dev(np.eye(K, dtype=f16)))
    monkeypatch.setenv("OSG_GEMM_KS", "2")
    got = gpu.gemm_ln(xd, w, gamma, beta, bias, 1e-5, act=0, rowstats=rs).numpy()
    assert rel_max(got, want) <= 1e-3


def _quant(rng, shape, std):
    w = (rng.standard_normal(shape, dtype=f32) * std).astype(f32)
    lo, hi = min(float(w.min()), 0.0), max(float(w.max()), 0.0)
    scale = np.float32((hi - lo) / 255.0)
    zp = int(abs(lo) / scale)
    q = np.clip(np.rint(w / scale) + zp, 0, 255).astype(np.uint8)
    wd = ref.dequantize_u8(q, scale, zp, f16)          # what the reference holds after loading the uint8 weight
    return q, float(scale), zp, wd


@pytest.mark.parametrize("M,N,K", [(300, 200, 128), (8192, 320, 320), (154, 1280, 768), (64, 1280, 5120), (2048, 72, 640)])
def test_gemm_w8(gpu, M, N, K):
    """uint8 weights dequantised on chip == the f16 GEMM on the reference's load-time dequantised weights."""
    rng = np.random.default_rng(M + N + K)
    a = rnd(rng, (M, K))
    q, scale, zp, wd = _quant(rng, (N, K), K ** -0.5)
    bias = rnd(rng, (N,), 0.1)
    res = rnd(rng, (M, N))
    want = ref.matmul(a, wd.T, bias, res)
    y = gpu.empty((M, N), f16)
    da, dq, db, dr = gpu.to_dev(a), gpu.to_dev(q), gpu.to_dev(bias), gpu.to_dev(res)
    gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dq.ptr, scale, zp, db.ptr, 2, dr.ptr, y.ptr, M, N, K, 0))
    assert rel_max(y.numpy(), want) <= 1e-3
    # and bit-identical to the f16 kernel fed with the dequantised weights when both take the same tile path (no split-K: small K)
    if K <= 512:
        y2 = gpu.gemm(da, gpu.to_dev(wd), db, dr, b_is_nk=True).numpy()
        assert rel_max(y.numpy(), y2) <= 2e-3


@pytest.mark.parametrize("N,H,Cin,Cout,k,stride", [(2, 16, 64, 96, 3, 1), (1, 32, 128, 320, 3, 1), (2, 8, 192, 64, 1, 1), (1, 16, 64, 128, 3, 2)])
def test_conv_w8(gpu, N, H, Cin, Cout, k, stride):
    rng = np.random.default_rng(N + H + Cin + Cout)
    x = rnd(rng, (N, H, H, Cin))
    q, scale, zp, wd = _quant(rng, (Cout, k, k, Cin), (k * k * Cin) ** -0.5)
    bias = rnd(rng, (Cout,), 0.1)
    pad = k // 2
    want = ref.conv2d_nhwc(x, wd, bias, (stride, stride), (pad,) * 4)
    y = gpu.empty(want.shape, f16)
    dx, dq, db = gpu.to_dev(x), gpu.to_dev(q), gpu.to_dev(bias)
    gpu._ck(gpu.lib.osg_conv2d_nhwc_w8(gpu.ctx, dx.ptr, dq.ptr, scale, zp, db.ptr, 2, None, 0, None, y.ptr, N, H, H, Cin, Cout, k, k,
                                       stride, stride, pad, pad, pad, pad, 0))
    assert rel_max(y.numpy(), want) <= 1e-3


def _exact_w8(a, q, scale, zp, bias=None, res=None):
    """what the resident-codes kernels compute: sum_k a (q - zp) exactly, times scale[n], in float64"""
    y = (a.astype(np.float64) @ (q.astype(np.float64) - np.asarray(zp, np.float64).reshape(-1, 1)).T) * np.asarray(scale, np.float64).reshape(1, -1)
    if bias is not None:
        y = y + bias.astype(np.float64)
    if res is not None:
        y = y + res.astype(np.float64)
    return y


def test_w8_fragment_conversion_is_exact(gpu):
    """every code 0 .. 255 against every zero point class through the byte-permute / packed-subtract conversion (w8_frag): A = identity picks the weight rows
    out one by one, scale 1 -- the output must be q - zp EXACTLY."""
    K = N = 256
    a = np.eye(K, dtype=f16)
    rng = np.random.default_rng(1)
    q = np.stack([np.roll(np.arange(256, dtype=np.uint8), r) for r in range(N)])          # every row holds every code
    da, dq = gpu.to_dev(a), gpu.to_dev(q)
    for zp in (0, 1, 127, 128, 255):
        y = gpu.empty((K, N), f16)
        gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dq.ptr, 1.0, zp, None, 2, None, y.ptr, K, N, K, 0))
        assert np.array_equal(y.numpy().astype(np.int32), (q.astype(np.int32) - zp).T)
    # per-column zero points and scales (the merged projections): powers of two keep the product exact
    zv = rng.integers(0, 256, N).astype(np.float32)
    sv = (2.0 ** rng.integers(-3, 3, N)).astype(np.float32)
    y = gpu.empty((K, N), f16)
    dsz = gpu.to_dev(np.concatenate([sv, zv]))
    gpu._ck(gpu.lib.osg_gemm_w8_v(gpu.ctx, da.ptr, dq.ptr, 0.0, 0, dsz.ptr, dsz.ptr + 4 * N, None, 2, None, y.ptr, K, N, K, 0))
    assert np.array_equal(y.numpy().astype(np.float64), ((q.astype(np.float64) - zv[:, None]) * sv[:, None]).T)


@pytest.mark.parametrize("M,N,K,cfg,nst,splits", [(300, 200, 128, 0, 2, 1), (8192, 320, 320, 2, 4, 1), (2048, 640, 640, 1, 2, 1), (2048, 640, 640, 3, 4, 1), (512, 1280, 1280, 2, 8, 1),
                                                  (512, 1280, 5120, 2, 4, 3), (8192, 320, 1280, 4, 4, 1), (2048, 640, 2560, 5, 2, 2), (2048, 640, 640, 6, 6, 1), (512, 1280, 1280, 7, 4, 1),
                                                  (154, 960, 768, 6, 4, 1), (130, 72, 64, 2, 2, 1), (2, 1280, 320, 2, 4, 1)])
def test_gemm_w8_every_tile(gpu, M, N, K, cfg, nst, splits, monkeypatch):
    """the WQ = 1 instantiations of gemm2_kernel, tile by tile (64-byte code rows, 16 rows per wave-load, the 4-slot XOR swizzle, pad rows of the 80 / 160-column
    tiles, split-K slabs of scaled sums): against the exact contraction in float64, and against the reference's order (dequantise to f16, then the f16 GEMM)."""
    rng = np.random.default_rng(M + N + K + cfg)
    a = rnd(rng, (M, K))
    q, scale, zp, wd = _quant(rng, (N, K), K ** -0.5)
    bias, res = rnd(rng, (N,), 0.1), rnd(rng, (M, N))
    monkeypatch.setenv("OSG_GEMM_CFG", str(cfg)); monkeypatch.setenv("OSG_GEMM_NST", str(nst)); monkeypatch.setenv("OSG_GEMM_SPLITS", str(splits))
    y = gpu.empty((M, N), f16)
    da, dq, db, dr = gpu.to_dev(a), gpu.to_dev(q), gpu.to_dev(bias), gpu.to_dev(res)
    gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dq.ptr, scale, zp, db.ptr, 2, dr.ptr, y.ptr, M, N, K, 0))
    got = y.numpy()
    assert rel_max(got, _exact_w8(a, q, [scale] * N, [zp] * N, bias, res)) <= 6e-4
    assert rel_max(got, ref.matmul(a, wd.T, bias, res)) <= 1e-3
    y2 = gpu.empty((M, N), f16)
    gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dq.ptr, scale, zp, db.ptr, 2, dr.ptr, y2.ptr, M, N, K, 0))
    assert np.array_equal(got, y2.numpy())


def test_gemm_w8_merged_projection_vectors_and_geglu(gpu):
    """per-column (scale, zero point) vectors -- three weights quantised one by one, concatenated as codes (the merged Q|K|V projection) -- and the GEGLU epilogue
    on pair-interleaved codes"""
    from scipy.special import erf
    rng = np.random.default_rng(11)
    M, K = 2048, 640
    a = rnd(rng, (M, K))
    parts = [_quant(rng, (n, K), s * K ** -0.5) for n, s in ((640, 1.0), (640, 0.3), (640, 2.0))]
    q = np.concatenate([p_[0] for p_ in parts])
    sv = np.concatenate([np.full(p_[0].shape[0], p_[1], np.float32) for p_ in parts])
    zv = np.concatenate([np.full(p_[0].shape[0], p_[2], np.float32) for p_ in parts])
    wd = np.concatenate([p_[3] for p_ in parts])
    N = q.shape[0]
    bias = rnd(rng, (N,), 0.1)
    y = gpu.empty((M, N), f16)
    dsz = gpu.to_dev(np.concatenate([sv, zv]))
    da, dq, db = gpu.to_dev(a), gpu.to_dev(q), gpu.to_dev(bias)
    gpu._ck(gpu.lib.osg_gemm_w8_v(gpu.ctx, da.ptr, dq.ptr, 0.0, 0, dsz.ptr, dsz.ptr + 4 * N, db.ptr, 2, None, y.ptr, M, N, K, 0))
    assert rel_max(y.numpy(), _exact_w8(a, q, sv, zv, bias)) <= 6e-4
    assert rel_max(y.numpy(), ref.matmul(a, wd.T, bias)) <= 1e-3
    # GEGLU: value columns 0 .. C-1, gate columns C .. 2C-1, rows interleaved in blocks of 16
    C = 1280
    q, scale, zp, wd = _quant(rng, (2 * C, K), K ** -0.5)
    b = rnd(rng, (2 * C,), 0.1)
    x = _exact_w8(a, q, [scale] * (2 * C), [zp] * (2 * C), b)
    v, g = x[:, :C], x[:, C:]
    want = v * 0.5 * g * (1.0 + erf(g / np.sqrt(2.0)))
    qi, bi = np.empty_like(q), np.empty_like(b)
    for k in range(C // 16):
        qi[32 * k:32 * k + 16] = q[16 * k:16 * k + 16]
        qi[32 * k + 16:32 * k + 32] = q[C + 16 * k:C + 16 * k + 16]
        bi[32 * k:32 * k + 16] = b[16 * k:16 * k + 16]
        bi[32 * k + 16:32 * k + 32] = b[C + 16 * k:C + 16 * k + 16]
    y = gpu.empty((M, C), f16)
    dqi, dbi = gpu.to_dev(qi), gpu.to_dev(bi)
    gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, da.ptr, dqi.ptr, scale, zp, dbi.ptr, 2, None, y.ptr, M, 2 * C, K, 3))
    assert rel_max(y.numpy(), want) <= 1e-3


@pytest.mark.parametrize("N,H,Cin,Cout,bn,splits", [(2, 64, 320, 320, 80, 1), (2, 32, 640, 640, 128, 1), (2, 16, 1280, 1280, 160, 2), (2, 8, 1280, 1280, 80, 4),
                                                    (2, 8, 2560, 1280, 128, 3), (2, 32, 960, 640, 160, 1), (1, 16, 64, 100, 128, 1)])
def test_conv3x3_w8_halo_kernel(gpu, N, H, Cin, Cout, bn, splits, monkeypatch):
    """the WQ = 1 instantiations of the halo-reuse 3x3 kernel (every image width, every tile width, split-K over slabs) with bias, per-image bias and residual"""
    rng = np.random.default_rng(N + H + Cin + Cout)
    x = rnd(rng, (N, H, H, Cin))
    q, scale, zp, wd = _quant(rng, (Cout, 3, 3, Cin), (9 * Cin) ** -0.5)
    bias, res = rnd(rng, (Cout,), 0.1), rnd(rng, (N, H, H, Cout))
    want = ref.conv2d_nhwc(x, wd, bias, (1, 1), (1,) * 4).astype(np.float64) + res.astype(np.float64)
    monkeypatch.setenv("OSG_CONV3X3_BN", str(bn)); monkeypatch.setenv("OSG_CONV3X3_SPLITS", str(splits))
    y = gpu.empty(want.shape, f16)
    dx, dq, db, dr = gpu.to_dev(x), gpu.to_dev(q), gpu.to_dev(bias), gpu.to_dev(res)
    gpu._ck(gpu.lib.osg_conv2d_nhwc_w8(gpu.ctx, dx.ptr, dq.ptr, scale, zp, db.ptr, 2, None, 0, dr.ptr, y.ptr, N, H, H, Cin, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 0))
    assert rel_max(y.numpy(), want) <= 1e-3
    # the same convolution into a column slice of a wider buffer + a dense second destination (the skip connections' output views)
    wide = gpu.to_dev(np.zeros((N, H, H, Cout + 64), f16))
    dense = gpu.empty(want.shape, f16)
    gpu._ck(gpu.lib.osg_conv2d_nhwc_w8_v(gpu.ctx, dx.ptr, dq.ptr, scale, zp, None, None, db.ptr, 2, None, 0, dr.ptr, dense.ptr, Cout, wide.ptr + 2 * 32, Cout + 64,
                                          N, H, H, Cin, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 0)) if Cout % 4 == 0 else None
    if Cout % 4 == 0:
        assert np.array_equal(dense.numpy(), y.numpy())
        wv = wide.numpy()
        assert np.array_equal(wv[..., 32:32 + Cout], y.numpy()) and not wv[..., :32].any() and not wv[..., 32 + Cout:].any()


@pytest.mark.timeout(180, method="thread")
def test_conv3x3_w8_halo_kernel_folds_the_tile_it_runs(gpu, monkeypatch):
    """uint8 codes with 160 columns at W = 64 run the 80-column tile (osg_gemm_routes.h resolve3): a split folded in the kernel is sized for that tile and gives the
    bits of the reduce launch"""
    rng = np.random.default_rng(64160)
    N, H, Cin, Cout = 1, 64, 128, 320
    x = rnd(rng, (N, H, H, Cin))
    q, scale, zp, wd = _quant(rng, (Cout, 3, 3, Cin), (9 * Cin) ** -0.5)
    bias, res = rnd(rng, (Cout,), 0.1), rnd(rng, (N, H, H, Cout))
    dx, dq, db, dr = gpu.to_dev(x), gpu.to_dev(q), gpu.to_dev(bias), gpu.to_dev(res)
    monkeypatch.setenv("OSG_CONV3X3_BN", "160"); monkeypatch.setenv("OSG_CONV3X3_SPLITS", "2")

    def conv(fold):
        monkeypatch.setenv("OSG_CONV3X3_FOLD", fold)
        y = gpu.empty((N, H, H, Cout), f16)
        gpu._ck(gpu.lib.osg_conv2d_nhwc_w8(gpu.ctx, dx.ptr, dq.ptr, scale, zp, db.ptr, 2, None, 0, dr.ptr, y.ptr, N, H, H, Cin, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 0))
        return y.numpy()
    want = conv("0")
    assert rel_max(want, ref.conv2d_nhwc(x, wd, bias, (1, 1), (1,) * 4).astype(np.float64) + res.astype(np.float64)) <= 1e-3
    for _ in range(2):
        assert np.array_equal(conv("1").view(np.uint16), want.view(np.uint16))


def test_gemm_batched(gpu):
    rng = np.random.default_rng(5)
    a, b = rnd(rng, (8, 256, 160)), rnd(rng, (8, 160, 77), 0.1)
    want = np.stack([ref.matmul(a[i], b[i]) for i in range(8)])
    got = gpu.gemm(gpu.to_dev(a), gpu.to_dev(b)).numpy()
    assert rel_max(got, want) <= 1e-3
    # shared weight across the batch (the reference's per-op batch loop)
    w = rnd(rng, (160, 96), 0.1)
    want = np.stack([ref.matmul(a[i], w) for i in range(8)])
    assert rel_max(gpu.gemm(gpu.to_dev(a), gpu.to_dev(w)).numpy(), want) <= 1e-3


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,pad", [
    (1, 16, 16, 32, 64, 3, 1, 1), (2, 64, 64, 320, 320, 3, 1, 1), (1, 64, 64, 4, 320, 3, 1, 1), (1, 64, 64, 320, 4, 3, 1, 1),
    (1, 32, 32, 640, 640, 3, 2, 1), (1, 8, 8, 1280, 1280, 3, 1, 1), (1, 16, 16, 640, 1280, 1, 1, 0), (1, 9, 7, 24, 40, 3, 2, 1),
    (2, 8, 8, 2560, 1280, 3, 1, 1)])
def test_conv2d(gpu, N, H, W, Cin, Cout, k, stride, pad):
    rng = np.random.default_rng(H * 31 + Cin + Cout)
    x = rnd(rng, (N, H, W, Cin))
    w = rnd(rng, (Cout, k, k, Cin), (Cin * k * k) ** -0.5)
    b = rnd(rng, (Cout,), 0.1)
    want = ref.conv2d_nhwc(x, w, b, (stride, stride), (pad,) * 4)
    got = gpu.conv2d_nhwc(gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(b), stride, (pad,) * 4).numpy()
    assert got.shape == want.shape
    assert rel_max(got, want) <= 1e-3
    res = rnd(rng, want.shape)
    want2 = ref.conv2d_nhwc(x, w, b.astype(f32), (stride, stride), (pad,) * 4, residual=res)
    got2 = gpu.conv2d_nhwc(gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(b.astype(f32)), stride, (pad,) * 4, residual=gpu.to_dev(res)).numpy()
    assert rel_max(got2, want2) <= 1e-3


@pytest.mark.parametrize("N,H,Cin,Cout,bn,splits", [
    (2, 64, 64, 320, 80, 1), (1, 64, 128, 160, 160, 2), (2, 32, 192, 128, 128, 3), (1, 32, 64, 640, 160, 1), (2, 16, 128, 320, 80, 2),
    (1, 16, 64, 96, 128, 1), (2, 8, 128, 160, 80, 1), (1, 8, 64, 160, 160, 1), (3, 8, 192, 128, 128, 3), (2, 64, 64, 320, 0, 0)])
def test_conv3x3_halo_kernel(gpu, N, H, Cin, Cout, bn, splits, monkeypatch):
    """The halo-reuse 3x3 kernel (osg_conv3x3.hip) at every tile geometry (W = 64/32/16/8), channel tile and split-K setting,
    incl. partial tiles (1 image of 8x8 = 64 pixels; 3 images of 8x8), bias + per-image bias + residual epilogue."""
    monkeypatch.setenv("OSG_GN_SLAB_OFF", "1")   # the fused path takes its statistics from the three-pass kernels: compare like with like
    if bn:
        monkeypatch.setenv("OSG_CONV3X3_BN", str(bn))
        monkeypatch.setenv("OSG_CONV3X3_SPLITS", str(splits))
    rng = np.random.default_rng(N * 131 + H * 7 + Cin + Cout)
    x = rnd(rng, (N, H, H, Cin))
    w = rnd(rng, (Cout, 3, 3, Cin), (9 * Cin) ** -0.5)
    bias = rnd(rng, (Cout,), 0.1)
    res = rnd(rng, (N, H, H, Cout))
    ib = rnd(rng, (N, Cout), 0.5)
    want = ref.conv2d_nhwc(x, w, bias, (1, 1), (1, 1, 1, 1), res.astype(f32) + ib.astype(f32)[:, None, None, :])
    got = gpu.conv2d_nhwc(gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias), 1, (1, 1, 1, 1), gpu.to_dev(res), image_bias=gpu.to_dev(ib)).numpy()
    assert rel_max(got, want) <= 1e-3


@pytest.mark.timeout(180, method="thread")   # (a protocol error would spin on the device: bound it)
@pytest.mark.parametrize("mode", ["1"])
@pytest.mark.parametrize("M,N,K,splits,cfg,batch", [(512, 1280, 5120, 4, 2, 1), (128, 1280, 1280, 4, 2, 1), (2048, 320, 1280, 2, 1, 1), (300, 100, 2048, 3, 1, 1),
                                                    (64, 640, 10240, 4, 2, 1), (77, 320, 2048, 3, 3, 2), (16384, 320, 1280, 2, 2, 1), (512, 1280, 5120, 8, 2, 1)])
def test_splitk_fold_in_the_kernel_equals_the_reduce_launch(gpu, M, N, K, splits, cfg, batch, mode, monkeypatch):
    """Round 5: split-K finished by the LAST k-slice workgroup to arrive at each tile (osg_gemm_common.h splitk_fold_acc: the others publish their accumulators in
    lane layout, the last one adds the slices in slice order and runs the fused epilogue) gives the bits of the separate reduce launch -- slabs through memory -- on every tile the fold takes, 2 .. 4 slices, ragged M / N, bias + residual, the
    batched form, and again on the next launches (the tile words are left zeroed); one case has more workgroups than the GPU holds at once (nobody waits for a
    workgroup that has not arrived); 8 slices: the launch falls back to the reduce launch."""
    monkeypatch.setenv("OSG_GEMM_SPLITS", str(splits))
    monkeypatch.setenv("OSG_GEMM_CFG", str(cfg))
    rng = np.random.default_rng(M + N + K)
    a = rnd(rng, (batch, M, K)) if batch > 1 else rnd(rng, (M, K))
    w, bias, res = rnd(rng, (K, N), K ** -0.5), rnd(rng, (N,), 0.1), rnd(rng, a.shape[:-1] + (N,))
    da, dw, db, dr = gpu.to_dev(a), gpu.to_dev(w), gpu.to_dev(bias), gpu.to_dev(res)
    monkeypatch.setenv("OSG_GEMM_FOLD", "0")
    want = gpu.gemm(da, dw, db, dr).numpy()
    assert rel_max(want, ref.matmul(a.reshape(-1, K), w, bias, residual=res.reshape(-1, N)).reshape(want.shape)) <= 1e-3
    monkeypatch.setenv("OSG_GEMM_FOLD", "1")
    monkeypatch.setenv("OSG_SPLITK_FOLD", mode)
    for _ in range(4):
        got = gpu.gemm(da, dw, db, dr).numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


@pytest.mark.timeout(180, method="thread")
@pytest.mark.parametrize("N,H,Cin,Cout,bn,splits", [(1, 64, 128, 160, 160, 2), (2, 32, 192, 128, 128, 3), (2, 16, 1280, 320, 80, 4), (1, 8, 2560, 1280, 80, 4),
                                                    (3, 8, 192, 128, 128, 3), (2, 16, 1280, 320, 80, 10)])
@pytest.mark.parametrize("mode", ["1"])
def test_conv3x3_splitk_fold_in_the_kernel_equals_the_reduce_launch(gpu, N, H, Cin, Cout, bn, splits, mode, monkeypatch):
    monkeypatch.setenv("OSG_CONV3X3_BN", str(bn))
    monkeypatch.setenv("OSG_CONV3X3_SPLITS", str(splits))
    rng = np.random.default_rng(N * 131 + H * 7 + Cin + Cout)
    x, w = rnd(rng, (N, H, H, Cin)), rnd(rng, (Cout, 3, 3, Cin), (9 * Cin) ** -0.5)
    bias, res, ib = rnd(rng, (Cout,), 0.1), rnd(rng, (N, H, H, Cout)), rnd(rng, (N, Cout), 0.5)
    dx, dw, db, dr, di = gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias), gpu.to_dev(res), gpu.to_dev(ib)
    monkeypatch.setenv("OSG_CONV3X3_FOLD", "0")
    want = gpu.conv2d_nhwc(dx, dw, db, 1, (1, 1, 1, 1), dr, image_bias=di).numpy()
    monkeypatch.setenv("OSG_CONV3X3_FOLD", "1")
    monkeypatch.setenv("OSG_SPLITK_FOLD", mode)
    for _ in range(4):
        got = gpu.conv2d_nhwc(dx, dw, db, 1, (1, 1, 1, 1), dr, image_bias=di).numpy()
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("N,H,Cin,Cout,bn,splits", [(2, 64, 320, 320, 80, 1), (2, 64, 640, 320, 160, 1), (2, 32, 640, 640, 128, 2), (2, 32, 1280, 640, 80, 3),
                                                    (2, 16, 1280, 1280, 160, 4), (2, 16, 640, 1280, 128, 2), (2, 8, 1280, 1280, 80, 5), (2, 8, 2560, 1280, 128, 8),
                                                    (2, 8, 1280, 1280, 160, 4), (3, 8, 192, 128, 128, 1)])
def test_conv3x3_halo_kernel_with_eight_loader_waves_gives_the_same_bits(gpu, N, H, Cin, Cout, bn, splits, monkeypatch):
    """round 3: the halo-reuse kernel with 8 DMA-issuing waves (768-thread workgroups, a measured candidate of the tuner): the same patch / weight
    images in LDS, the same MFMA order => bit-identical to the 4-loader kernel for every tile width, slab split and image size (W = 8 with
    BN = 160 has no room for the wider stages and runs the 4-loader kernel)."""
    monkeypatch.setenv("OSG_CONV3X3_BN", str(bn))
    monkeypatch.setenv("OSG_CONV3X3_SPLITS", str(splits))
    rng = np.random.default_rng(N + H + Cin + Cout + bn)
    x, w = rnd(rng, (N, H, H, Cin)), rnd(rng, (Cout, 3, 3, Cin), (9 * Cin) ** -0.5)
    bias, res = rnd(rng, (Cout,), 0.1), rnd(rng, (N, H, H, Cout))
    dx, dw, db, dr = gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias), gpu.to_dev(res)
    monkeypatch.setenv("OSG_CONV3X3_NL", "4")
    want = gpu.conv2d_nhwc(dx, dw, db, 1, (1, 1, 1, 1), dr).numpy()
    monkeypatch.setenv("OSG_CONV3X3_NL", "8")
    for _ in range(2):
        got = gpu.conv2d_nhwc(dx, dw, db, 1, (1, 1, 1, 1), dr).numpy()
        assert np.array_equal(got, want)
    assert rel_max(want, ref.conv2d_nhwc(x, w, bias, (1, 1), (1, 1, 1, 1), res)) <= 2e-3


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,stride,env", [
    (2, 64, 64, 4, 320, 3, 1, {}),                                      # conv_in: the small-Cin vector kernel
    (2, 64, 64, 320, 320, 1, 1, {}),                                    # 1x1 = plain GEMM (proj_out / shortcut)
    (2, 64, 64, 320, 320, 3, 1, {}),                                    # halo-reuse kernel, one tile per CU
    (2, 32, 32, 640, 640, 3, 1, {"OSG_CONV3X3_SPLITS": "2"}),           # ... split over slabs + reduce launch
    (2, 8, 8, 1280, 1280, 3, 1, {"OSG_CONV3X3_SPLITS": "4", "OSG_CONV3X3_FOLD": "1"}),   # ... folded in the kernel
    (2, 64, 64, 320, 320, 3, 2, {}),                                    # downsampler: implicit GEMM
    (2, 16, 16, 1280, 640, 1, 1, {"OSG_GEMM_SPLITS": "4"}),             # split-K GEMM + reduce launch
    (1, 12, 10, 20, 36, 3, 1, {}),                                      # ragged shape: the register-staged v1 kernel
])
def test_conv_output_views_equal_the_dense_result(gpu, N, H, W, Cin, Cout, k, stride, env, monkeypatch):
    """osg_conv2d_nhwc_v (round 3: skip tensors written straight into their Concat slot): the column slice of a wider NHWC buffer, and the
    dense tensor + the slice in one launch, hold exactly the bits the plain launch stores; the neighbouring columns stay untouched."""
    for kk, vv in env.items():
        monkeypatch.setenv(kk, vv)
    rng = np.random.default_rng(N + H + Cin + Cout + k)
    pad = k // 2
    x, w = rnd(rng, (N, H, W, Cin)), rnd(rng, (Cout, k, k, Cin), (k * k * Cin) ** -0.5)
    bias = rnd(rng, (Cout,), 0.1)
    dx, dw, db = gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = gpu.to_dev(rnd(rng, (N, Ho, Wo, Cout)))
    ib = gpu.to_dev(rnd(rng, (N, Cout), 0.2))
    want = gpu.conv2d_nhwc(dx, dw, db, stride, (pad,) * 4, res, image_bias=ib).numpy()
    left, right = 8, 12
    wide0 = rnd(rng, (N, Ho, Wo, left + Cout + right))
    for dual, swap in ((False, False), (True, False), (True, True)):
        wide = gpu.to_dev(wide0)
        dense = gpu.to_dev(np.zeros((N, Ho, Wo, Cout), f16)) if dual else None
        gpu.conv2d_nhwc_view(dx, dw, db, wide, left, dense, stride, (pad,) * 4, res, image_bias=ib, swap=swap)
        got = wide.numpy()
        assert np.array_equal(got[..., left:left + Cout], want), (dual, swap)
        assert np.array_equal(got[..., :left], wide0[..., :left]) and np.array_equal(got[..., left + Cout:], wide0[..., left + Cout:])
        if dual:
            assert np.array_equal(dense.numpy(), want)


@pytest.mark.parametrize("N,H,W,Cin,Cout,k,G,env", [
    (2, 64, 64, 320, 320, 3, 32, {}),                                   # halo kernel, 128 x 160 tiles: a wave's 80 columns hold 8 groups of 10 channels and straddle two more
    (2, 32, 32, 640, 640, 3, 32, {}),                                   # halo kernel at W = 32
    (2, 32, 32, 320, 640, 1, 32, {}),                                   # 1x1 = plain GEMM (gemm2_kernel's epilogue)
    (1, 48, 48, 320, 320, 3, 32, {}),                                   # a width the halo kernel does not take: the implicit-GEMM kernel
    (2, 16, 16, 1280, 640, 1, 32, {"OSG_GEMM_SPLITS": "4"}),            # split-K GEMM: the reduce launch finishes the values and adds them up
    (2, 32, 32, 640, 640, 3, 32, {"OSG_CONV3X3_SPLITS": "2"}),          # split-K halo kernel: the same
    (2, 32, 32, 320, 640, 1, 32, {"OSG_GEMM_KS": "2", "OSG_GEMM_CFG": "2", "OSG_GEMM_NST": "2"}),   # two wave groups per tile: group 0's epilogue serves the sinks
    (1, 16, 16, 64, 96, 3, 8, {}),                                      # small shapes: whatever kernel runs, whichever way the statistics are made
    (2, 64, 64, 320, 320, 3, 32, {"SCALE": "1e-3"}),                    # a small-magnitude tensor (|y| ~ 1e-3: a wave's partial sum of squares is ~ 1e-4; advisor, round 3)
    (1, 64, 64, 64, 256, 3, 1, {"SCALE": "3000"}),                      # one group of 2^20 elements of |y| ~ 4e3 (sum of squares ~ 2^44: the fixed 2^20 scale of round 4 wrapped the int64; advisor, round 4)
])
def test_group_norm_statistics_from_the_producing_convolution(gpu, N, H, W, Cin, Cout, k, G, env, monkeypatch):
    """osg_set_stat_sinks + osg_group_norm_stats_nhwc (round 3): the convolution's epilogue adds the per-(image, group) sums of what it stores to an int64
    fixed-point table -- for its own output and, at a channel offset, for the Concat slot it stores a second time -- and the normalisation is one streaming
    launch reading the table.  The table against numpy on the stored values, the normalised tensors against the GroupNorm launch, twice the same bits."""
    env = dict(env)
    sc = float(env.pop("SCALE", "1"))
    for kk, vv in env.items():
        monkeypatch.setenv(kk, vv)
    rng = np.random.default_rng(N + H + Cin + Cout + k)
    pad = k // 2
    x, w = rnd(rng, (N, H, W, Cin), sc), rnd(rng, (Cout, k, k, Cin), (k * k * Cin) ** -0.5)
    bias = rnd(rng, (Cout,), 0.3 * sc)
    dx, dw, db = gpu.to_dev(x), gpu.to_dev(w), gpu.to_dev(bias)
    res = gpu.to_dev(rnd(rng, (N, H, W, Cout), sc))
    left = 2 * (Cout // G) + 8                     # the slot starts in the middle of a group of the concatenated tensor
    left += (-left) % 4                            # (slices of a wider buffer start at multiples of 4 elements)
    Cw = left + Cout + 16
    Cw += (-Cw) % 8
    Gw = 8
    assert Cw % Gw == 0 and Cw % 8 == 0
    wide0 = rnd(rng, (N, H, W, Cw))
    gam, bet = gpu.to_dev(rnd(rng, (Cout,), 1.0)), gpu.to_dev(rnd(rng, (Cout,), 0.5))
    runs = []
    for rep in range(2):
        t0, t1 = gpu.to_dev(np.zeros((8, N, G, 2), np.int64)), gpu.to_dev(np.zeros((8, N, Gw, 2), np.int64))   # (one copy per XCD)
        wide, dense = gpu.to_dev(wide0), gpu.to_dev(np.zeros((N, H, W, Cout), f16))
        gpu.set_stat_sinks(H * W, t0, G, Cout // G, 0, t1, Gw, Cw // Gw, left)
        gpu.conv2d_nhwc_view(dx, dw, db, wide, left, dense, 1, (pad,) * 4, res, swap=True)     # dense = the primary destination, the slot the second
        y = dense.numpy().astype(np.float64)
        tab0, tab1 = t0.numpy().sum(0), t1.numpy().sum(0)
        yg = y.reshape(N, H * W, G, Cout // G)
        # the scale of the sums of squares follows the group's size (osg_gemm_common.h stat_q_shift): 2^(36 - ceil(log2(elements))) clamped to [2^10, 2^20]
        qs = lambda elems: 2.0 ** min(20, max(10, 36 - int(np.ceil(np.log2(elems)))))
        q0, q1 = qs(H * W * (Cout // G)), qs(H * W * (Cw // Gw))
        assert (tab0[..., 1] >= 0).all() and (tab1[..., 1] >= 0).all()          # (a wrapped int64 sum of squares shows up negative)
        assert np.allclose(tab0[..., 0] / 2.0 ** 20, yg.sum((1, 3)), rtol=1e-5, atol=2e-2 * max(sc, 1))
        assert np.allclose(tab0[..., 1] / q0, (yg * yg).sum((1, 3)), rtol=1e-4 if sc < 1 else 1e-5, atol=2.0 * sc * sc)
        # the slot's share of the concatenated tensor's groups (the other columns are not this launch's business)
        full = np.zeros((N, H * W, Cw)); full[..., left:left + Cout] = y.reshape(N, H * W, Cout)
        fg = full.reshape(N, H * W, Gw, Cw // Gw)
        assert np.allclose(tab1[..., 0] / 2.0 ** 20, fg.sum((1, 3)), rtol=1e-5, atol=2e-2 * max(sc, 1))
        assert np.allclose(tab1[..., 1] / q1, (fg * fg).sum((1, 3)), rtol=1e-4 if sc < 1 else 1e-5, atol=2.0 * sc * sc)
        got = gpu.group_norm_stats_nhwc(dense, gam, bet, G, 1e-5, t0, act=1).numpy()
        want = gpu.group_norm_nhwc(dense, gam, bet, G, 1e-5, act=1).numpy()
        assert rel_max(want.astype(f32), got.astype(f32)) <= 2e-3
        runs.append((tab0.copy(), tab1.copy(), got.copy()))
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))        # integer atomics: the arrival order of the workgroups leaves no trace


def test_conv_linearity_full_size(gpu):
    """Size-independent property at SD1.5 full size: conv(a*x) + conv(b*y) == conv(a*x + b*y) up to f16 rounding."""
    rng = np.random.default_rng(11)
    x, y = rnd(rng, (2, 64, 64, 320)), rnd(rng, (2, 64, 64, 320))
    w = rnd(rng, (320, 3, 3, 320), 2880 ** -0.5)
    dw = gpu.to_dev(w)
    cx = gpu.conv2d_nhwc(gpu.to_dev(x), dw, None).numpy().astype(f32)
    cy = gpu.conv2d_nhwc(gpu.to_dev(y), dw, None).numpy().astype(f32)
    cxy = gpu.conv2d_nhwc(gpu.to_dev((x.astype(f32) + y.astype(f32)).astype(f16)), dw, None).numpy().astype(f32)
    assert rel_max(cx + cy, cxy) <= 4e-3


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,Tq,Tkv,D", [(8, 64, 64, 160), (8, 256, 77, 160), (8, 1024, 1024, 80), (4, 2048, 77, 40),
                                            (2, 4096, 4096, 40), (10, 256, 256, 64), (3, 50, 11, 16), (2, 130, 200, 24)])
def test_attention(gpu, heads, Tq, Tkv, D):
    rng = np.random.default_rng(Tq + Tkv + D)
    q, k, v = rnd(rng, (heads, Tq, D)), rnd(rng, (heads, Tkv, D)), rnd(rng, (heads, Tkv, D))
    scale = D ** -0.5
    want = ref.attention_exact(q, k, v, scale)
    got = gpu.attention(gpu.to_dev(q), gpu.to_dev(k), gpu.to_dev(v), scale, k_is_dt=False).numpy()
    assert rel_max(got, want) <= 2e-3
    kdt = np.ascontiguousarray(k.transpose(0, 2, 1))
    got2 = gpu.attention(gpu.to_dev(q), gpu.to_dev(kdt), gpu.to_dev(v), scale, k_is_dt=True).numpy()
    assert np.array_equal(got, got2)
    if Tq * Tkv <= 256 * 256:
        # the reference's sliced path (f16 scores / probabilities) agrees within its own rounding noise
        sliced = ref.attention_fused_ops(q, kdt, v, f16(scale), parts=2)
        assert rel_max(got, sliced) <= 6e-3


@pytest.mark.parametrize("heads,Tq,Tkv,D", [(64, 1030, 200, 40), (64, 1024, 77, 64), (72, 1024, 130, 80), (64, 1030, 70, 160), (3, 100, 130, 40), (2, 70, 1, 80),
                                            (2, 200, 129, 64), (1, 17, 300, 160)])
def test_attention_dma_kernel_ragged_shapes(gpu, heads, Tq, Tkv, D):
    """attn2_kernel (round 5: K / V through LDS-DMA, transposing V reads, row sums on the matrix pipe): the 128-row form (>= 512 blocks of 128 rows) and the
    64-row form on ragged query / key counts -- partial last key tile (rows past Tkv zero-filled by the DMA), query rows past Tq, one key only."""
    rng = np.random.default_rng(Tq * 7 + Tkv + D)
    q, k, v = rnd(rng, (heads, Tq, D)), rnd(rng, (heads, Tkv, D)), rnd(rng, (heads, Tkv, D))
    want = ref.attention_exact(q, k, v, D ** -0.5)
    got = gpu.attention(gpu.to_dev(q), gpu.to_dev(k), gpu.to_dev(v), D ** -0.5, k_is_dt=False).numpy()
    assert rel_max(got, want) <= 2e-3


def test_attention_spike_rows(gpu):
    """Force the online-softmax rescale branch: one key dominates a late tile for some query rows."""
    rng = np.random.default_rng(3)
    heads, T, D = 2, 512, 64
    q, k, v = rnd(rng, (heads, T, D)), rnd(rng, (heads, T, D)), rnd(rng, (heads, T, D))
    k[:, 300] = q[:, 7] * 4
    k[:, 450] = q[:, 100] * 6
    want = ref.attention_exact(q, k, v, D ** -0.5)
    got = gpu.attention(gpu.to_dev(q), gpu.to_dev(k), gpu.to_dev(v), D ** -0.5, k_is_dt=False).numpy()
    assert rel_max(got, want) <= 2e-3


def test_attention_token_layout(gpu):
    rng = np.random.default_rng(4)
    B, heads, Tq, Tkv, D = 2, 8, 256, 77, 40
    q, k, v = rnd(rng, (B, Tq, heads * D)), rnd(rng, (B, Tkv, heads * D)), rnd(rng, (B, Tkv, heads * D))
    got = gpu.attention_tokens(gpu.to_dev(q), gpu.to_dev(k), gpu.to_dev(v), heads, D ** -0.5).numpy()
    sp = lambda t, T: t.reshape(B, T, heads, D).transpose(0, 2, 1, 3).reshape(B * heads, T, D)
    want = ref.attention_exact(sp(q, Tq), sp(k, Tkv), sp(v, Tkv), D ** -0.5)
    want = want.reshape(B, heads, Tq, D).transpose(0, 2, 1, 3).reshape(B, Tq, heads * D)
    assert rel_max(got, want) <= 2e-3


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L", [(32, 40960), (32, 5120), (64, 640), (3, 17)])
def test_instance_norm(gpu, rows, L):
    rng = np.random.default_rng(rows + L)
    x = rnd(rng, (1, rows, L), 2.0) + f16(0.5)
    sc, bi = rnd(rng, (rows,), 1.0, f32), rnd(rng, (rows,), 1.0, f32)
    want = ref.instance_norm(x, sc, bi, 1e-5)
    got = gpu.instance_norm(gpu.to_dev(x), gpu.to_dev(sc), gpu.to_dev(bi), 1e-5).numpy()
    assert rel_max(got, want) <= 1e-3


@pytest.mark.parametrize("N,H,W,C,act", [(2, 64, 64, 320, 1), (1, 8, 8, 2560, 0), (2, 16, 16, 1280, 1), (1, 5, 3, 64, 0),
                                         # single-launch slab kernel: every vectors-per-thread instantiation, ragged HW, groups straddling a vector
                                         (2, 32, 32, 640, 1), (2, 32, 32, 1920, 1), (1, 32, 32, 960, 0), (2, 16, 16, 2560, 1), (2, 8, 8, 1280, 1),
                                         (1, 7, 9, 320, 1), (1, 3, 3, 256, 0), (1, 16, 16, 1920, 0), (3, 1, 1, 384, 1),
                                         # cluster kernel (pixel rows of a slab split over co-resident blocks): the 64x64 level, P = 4, the wide concat inputs
                                         (2, 64, 64, 640, 1), (2, 64, 64, 960, 1), (8, 64, 64, 320, 1), (1, 64, 64, 320, 0), (2, 32, 32, 1280, 1),
                                         (1, 128, 128, 256, 1), (1, 64, 64, 512, 1), (40, 64, 64, 320, 1)])
def test_group_norm_nhwc(gpu, N, H, W, C, act):
    rng = np.random.default_rng(C + H)
    x = rnd(rng, (N, H, W, C), 1.5) + f16(0.3)
    g, b = (1 + rnd(rng, (C,), 0.1).astype(f32)).astype(f16), rnd(rng, (C,), 0.1)
    want = ref.group_norm_nhwc_exact(x, g, b, 32, 1e-5, bool(act))
    got = gpu.group_norm_nhwc(gpu.to_dev(x), gpu.to_dev(g), gpu.to_dev(b), 32, 1e-5, act).numpy()
    assert rel_max(got, want) <= 1e-3
    if N == 1 and not act:
        # the decomposed reference chain (Reshape/InstanceNorm/Reshape/Mul/Add on NCHW) agrees within its extra roundings
        dec = ref.group_norm_decomposed_nchw(x.transpose(0, 3, 1, 2), g, b, 32, 1e-5).transpose(0, 2, 3, 1)
        assert rel_max(got, dec) <= 2e-3


@pytest.mark.parametrize("rows,C", [(4096, 320), (1024, 640), (256, 1280), (7, 48), (5, 30)])
def test_layer_norm(gpu, rows, C):
    rng = np.random.default_rng(rows + C)
    x = rnd(rng, (1, rows, C), 1.5) + f16(0.2)
    g, b = (1 + rnd(rng, (C,), 0.1).astype(f32)).astype(f16), rnd(rng, (C,), 0.1)
    got = gpu.layer_norm(gpu.to_dev(x), gpu.to_dev(g), gpu.to_dev(b), 1e-5).numpy()
    assert rel_max(got, ref.layer_norm_exact(x, g, b, 1e-5)) <= 1e-3
    assert rel_max(got, ref.layer_norm_decomposed(x, g, b, 1e-5)) <= 4e-3


@pytest.mark.parametrize("rows,C", [(5, 64), (1, 2048), (33, 320), (7, 100)])
def test_rms_norm(gpu, rows, C):
    """fp32 from the f16 input to one rounding, in the op order of the graph chain (Pow, ReduceMean, Add, Sqrt, Div, Mul, Mul)"""
    rng = np.random.default_rng(rows + C)
    x = rnd(rng, (rows, C), 3.0)
    w = (1 + rnd(rng, (C,), 0.1).astype(f32)).astype(f16)
    xf = x.astype(f32)
    r = f32(1.0) / np.sqrt((xf * xf).mean(axis=-1, keepdims=True, dtype=f32) + f32(1e-5))
    want = (w.astype(f32) * (xf * r)).astype(f16)
    got = gpu.rms_norm(gpu.to_dev(x), gpu.to_dev(w), 1e-5).numpy()
    assert rel_max(got, want) <= 1e-3
    assert (got != want).mean() <= 0.02        # (the f32 sum order may move a value across an f16 rounding boundary, nothing more)


@pytest.mark.parametrize("BH,T,d", [(4, 5, 16), (32, 1, 64), (6, 37, 128), (1, 300, 8)])
def test_rope_is_bit_identical_to_the_op_chain(gpu, BH, T, d):
    rng = np.random.default_rng(BH + T + d)
    x = rnd(rng, (BH, T, d), 2.0)
    cs, sn = rnd(rng, (T, d), 1.0), rnd(rng, (T, d), 1.0)
    half = d // 2
    rot = np.concatenate([-x[..., half:], x[..., :half]], axis=-1)
    a = (x.astype(f32) * cs.astype(f32)).astype(f16)
    b = (rot.astype(f32) * sn.astype(f32)).astype(f16)
    want = (a.astype(f32) + b.astype(f32)).astype(f16)
    got = gpu.rope(gpu.to_dev(x), gpu.to_dev(cs), gpu.to_dev(sn)).numpy()
    assert np.array_equal(got, want)


def test_reduce_mean_softmax(gpu):
    rng = np.random.default_rng(9)
    x = rnd(rng, (3, 77, 333), 2.0)
    assert rel_max(gpu.reduce_mean_last(gpu.to_dev(x)).numpy(), ref.reduce_mean_last(x)) <= 1e-3
    want = ref.softmax_last(x)
    got = gpu.softmax_last(gpu.to_dev(x)).numpy()
    assert rel_max(got, want) <= 2e-3
    xl = rnd(rng, (16, 4096), 3.0)
    assert rel_max(gpu.softmax_last(gpu.to_dev(xl)).numpy(), ref.softmax_last(xl)) <= 2e-3


def test_group_norm_cluster_relaunch_is_bit_stable(gpu):
    """The cluster kernel's arrival / departure counters reset themselves: ten launches in a row (two shapes interleaved) give the same bits."""
    rng = np.random.default_rng(5)
    xs = [rnd(rng, (2, 64, 64, 320), 1.5), rnd(rng, (2, 32, 32, 1920), 1.5)]
    gs = [(1 + rnd(rng, (x.shape[-1],), 0.1).astype(f32)).astype(f16) for x in xs]
    bs = [rnd(rng, (x.shape[-1],), 0.1) for x in xs]
    dev = [(gpu.to_dev(x), gpu.to_dev(g), gpu.to_dev(b)) for x, g, b in zip(xs, gs, bs)]
    first = [gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy() for d in dev]
    for _ in range(10):
        for d, f in zip(dev, first):
            assert np.array_equal(gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy(), f)
    for x, g, b, f in zip(xs, gs, bs, first):
        assert rel_max(f, ref.group_norm_nhwc_exact(x, g, b, 32, 1e-5, True)) <= 1e-3


def test_group_norm_cluster_bounded_wait_solo_path_gives_the_same_bits(gpu, monkeypatch):
    """The cluster kernel never waits without a bound (advisor, round 2: two contexts / two streams on one GPU can each hold part of a slab's
    blocks): a block whose peers do not arrive in time recomputes their partials from x with the same reduction tree.  OSG_GN_CLUSTER_WAIT=0
    makes EVERY block take that path -- same bits as the co-operative path, counters back to zero (the launches after it still agree)."""
    rng = np.random.default_rng(11)
    cases = [rnd(rng, (2, 64, 64, 320), 1.5), rnd(rng, (2, 32, 32, 1920), 1.5), rnd(rng, (1, 64, 64, 640), 1.5)]
    for x in cases:
        C = x.shape[-1]
        g, b = (1 + rnd(rng, (C,), 0.1).astype(f32)).astype(f16), rnd(rng, (C,), 0.1)
        d = (gpu.to_dev(x), gpu.to_dev(g), gpu.to_dev(b))
        monkeypatch.delenv("OSG_GN_CLUSTER_WAIT", raising=False)
        coop = gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy()
        monkeypatch.setenv("OSG_GN_CLUSTER_WAIT", "0")
        solo = gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy()
        solo2 = gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy()
        monkeypatch.delenv("OSG_GN_CLUSTER_WAIT", raising=False)
        again = gpu.group_norm_nhwc(*d, 32, 1e-5, 1).numpy()
        assert np.array_equal(solo, coop) and np.array_equal(solo2, coop) and np.array_equal(again, coop)
        assert rel_max(coop, ref.group_norm_nhwc_exact(x, g, b, 32, 1e-5, True)) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sigmoid", "erf", "sqrt", "sin", "cos", "neg", "pow", "silu", "gelu_erf"])
def test_unary(gpu, kind):
    rng = np.random.default_rng(1)
    x = rnd(rng, (1000, 37), 3.0)
    if kind == "sqrt":
        x = np.abs(x)
    got = gpu.unary(kind, gpu.to_dev(x), 2.0).numpy()
    want = ref.unary(kind, x, 2.0)
    if kind == "neg":
        assert np.array_equal(got, want)
    else:
        # <= 1 f16 ulp of the correctly rounded value
        assert np.abs(got.astype(f32) - want.astype(f32)).max() <= np.abs(want.astype(f32)).max() * 1e-3


@pytest.mark.parametrize("kind", ["add", "sub", "mul", "div"])
@pytest.mark.parametrize("ash,bsh", [((1, 4096, 320), (1, 4096, 320)), ((1, 4096, 320), (320,)), ((1, 320, 64, 64), (320, 1, 1)),
                                     ((1, 64, 64, 320), (1, 1, 1, 320)), ((2, 77, 5), ()), ((1, 1280, 1, 1), (1, 1280, 8, 8)),
                                     ((3, 1, 5), (1, 4, 1)), ((7,), (7,))])
def test_binary(gpu, kind, ash, bsh):
    rng = np.random.default_rng(len(ash) * 10 + len(bsh))
    a, b = rnd(rng, ash, 2.0), rnd(rng, bsh, 2.0)
    if kind == "div":
        b = (np.abs(b.astype(f32)) + 0.5).astype(f16)
    got = gpu.binary(kind, gpu.to_dev(a), gpu.to_dev(b)).numpy()
    want = ref.binary(kind, a, b)
    assert got.shape == want.shape
    # f32 math + one rounding on both sides: bit-exact except f32->f16 double rounding in div
    assert np.array_equal(got, want) or (kind == "div" and rel_max(got, want) <= 1e-3)


def test_geglu(gpu):
    rng = np.random.default_rng(2)
    x = rnd(rng, (1, 256, 2 * 1280), 1.5)
    want = ref.r16(x[..., :1280].astype(f32) * ref.unary("gelu_erf", x[..., 1280:]).astype(f32))
    assert rel_max(gpu.geglu(gpu.to_dev(x)).numpy(), want) <= 2e-3


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,perm", [((1, 320, 64, 64), (0, 2, 3, 1)), ((1, 64, 64, 320), (0, 3, 1, 2)), ((1, 4096, 8, 40), (0, 2, 1, 3)),
                                        ((8, 77, 160), (0, 2, 1)), ((2, 3, 4, 5, 6), (4, 0, 3, 1, 2)), ((5, 1, 7), (2, 1, 0)), ((6, 9), (1, 0)),
                                        ((3, 4, 5), (0, 1, 2))])
@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
def test_transpose(gpu, shape, perm, dtype):
    rng = np.random.default_rng(sum(shape))
    x = rng.integers(0, 255, size=shape).astype(dtype)
    assert np.array_equal(gpu.transpose(gpu.to_dev(x), perm).numpy(), x.transpose(perm))


def test_copy2d_concat_slice(gpu):
    rng = np.random.default_rng(8)
    a, b = rnd(rng, (4096, 320)), rnd(rng, (4096, 640))
    out = gpu.empty((4096, 960), f16)
    gpu.copy_2d(gpu.to_dev(a), 320, 0, out, 960, 0, 4096, 320)
    gpu.copy_2d(gpu.to_dev(b), 640, 0, out, 960, 320, 4096, 640)
    assert np.array_equal(out.numpy(), np.concatenate([a, b], 1))
    sl = gpu.empty((4096, 100), f16)
    gpu.copy_2d(out, 960, 33, sl, 100, 0, 4096, 100)
    assert np.array_equal(sl.numpy(), out.numpy()[:, 33:133])


@pytest.mark.parametrize("nhwc", [True, False])
def test_resize_nearest(gpu, nhwc):
    rng = np.random.default_rng(6)
    x = rnd(rng, (1, 16, 16, 64) if nhwc else (1, 64, 16, 16))
    got = gpu.resize_nearest(gpu.to_dev(x), 32, 32, nhwc).numpy()
    want = x.repeat(2, axis=1 if nhwc else 2).repeat(2, axis=2 if nhwc else 3)
    assert np.array_equal(got, want)


def test_gather_maxpool(gpu):
    rng = np.random.default_rng(7)
    x = rnd(rng, (100, 33))
    idx = np.array([5, 99, 0, -1, 42], np.int64)
    assert np.array_equal(gpu.gather_rows(gpu.to_dev(x), gpu.to_dev(idx)).numpy(), x[idx])
    img = rnd(rng, (1, 20, 20, 128))
    got = gpu.maxpool_nhwc(gpu.to_dev(img), (5, 5), (1, 1), (2, 2, 2, 2)).numpy()
    pad = np.full((1, 24, 24, 128), -np.inf, f32)
    pad[:, 2:22, 2:22] = img
    want = np.max([pad[:, i:i + 20, j:j + 20] for i in range(5) for j in range(5)], axis=0).astype(f16)
    assert np.array_equal(got, want)


def test_convert_quant_bit_exact(gpu):
    """Integer path: u8 codes and dequantised values must be BIT-EXACT (SURVEY A13 formulas)."""
    rng = np.random.default_rng(10)
    x = (rng.standard_normal(1 << 20, dtype=f32) * 3).astype(f32)
    scale, zp = ref.range_to_scale(float(x.min()) * 0.7, float(x.max()) * 0.7)
    q = gpu.convert(gpu.to_dev(x), np.uint8, scale, zp).numpy()
    assert np.array_equal(q, ref.quantize_u8(x, scale, zp))
    dq = gpu.convert(gpu.to_dev(q), np.float32, scale, zp).numpy()
    assert np.array_equal(dq, ref.dequantize_u8(q, scale, zp))
    dq16 = gpu.convert(gpu.to_dev(q), np.float16, scale, zp).numpy()
    assert np.array_equal(dq16, ref.dequantize_u8(q, scale, zp, f16))
    h = x.astype(f16)
    assert np.array_equal(gpu.convert(gpu.to_dev(h), np.float32).numpy(), h.astype(f32))
    assert np.array_equal(gpu.convert(gpu.to_dev(x), np.float16).numpy(), h)


def test_upload_staged_roundtrip(gpu):
    rng = np.random.default_rng(12)
    x = rng.integers(0, 255, size=(150 << 20) + 13, dtype=np.uint8)   # > 2 staging chunks, ragged tail
    d = gpu.to_dev(x, staged=True)
    assert np.array_equal(d.numpy(), x)


@pytest.mark.parametrize("outer,ia,ib,dt", [(8192, 320, 320, f16), (2048, 1280, 640, f16), (7, 5, 3, f16), (3, 160, 160, f32), (1, 1, 9, np.uint8), (64, 8, 24, f16)])
def test_concat2_single_launch(gpu, outer, ia, ib, dt):
    """The skip-connection Concat as ONE launch (osg_concat2) == numpy.concatenate, bit for bit, for 16-byte and odd-sized runs."""
    rng = np.random.default_rng(outer + ia + ib)
    a = (rng.standard_normal((outer, ia)) * 50).astype(dt)
    b = (rng.standard_normal((outer, ib)) * 50).astype(dt)
    got = gpu.concat2(gpu.to_dev(a), gpu.to_dev(b)).numpy()
    assert np.array_equal(got, np.concatenate([a, b], axis=-1))
