"""-m gpu: the contraction entry points on tensors at and past 2 and 4 GiB, against the float64 restatement (oracle/np_ops.py) on sampled rows.

The epilogue of gemm2_kernel / conv3x3_kernel / gemm_kernel stores through buffer descriptors with 32-bit offsets: an output, residual or per-image bias
whose byte offsets do not fit them loses stores past 2 GiB or wraps them onto its first rows past 4 GiB.  Every case here
  * fills the output with 0xFF first (every f16 reads NaN): a dropped store shows up as NaN, not as a leftover zero;
  * builds its large operands ON THE DEVICE with osg_gather_rows from small seeded tables whose periods are pairwise coprime (A row m = TA[m % 4099],
    residual row m = TR[m % 4093], input pixel p = TX[p % 4091]): no two rows below ~16.7 M expect the same value, so a store that landed on another
    row cannot pass -- and checks sampled rows of those gathered tensors bit for bit against the tables (gather_rows_kernel at this size);
  * compares the first 256 rows, ~300 rows around the byte 2^31 and 2^32 of the output (when it reaches them) and its last 300 rows with the
    reference computed from the table rows those outputs need.
Row widths are chosen so that byte 2^31 falls inside a row and inside a column tile.  Up to ~11 GiB of device memory per case, freed at its end.
"""
import numpy as np
import pytest

from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
f16, f32 = np.float16, np.float32
F16, F32 = 2, 3
P_A, P_R, P_X = 4099, 4093, 4091      # periods of the A-row, residual-row and input-pixel tables (pairwise coprime)


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rnd(rng, shape, std=1.0, dtype=f16):
    return (rng.standard_normal(shape, dtype=f32) * std).astype(dtype)


class Bufs:
    """the device buffers of one case: freed when it ends, pass or fail (the GPU is shared)"""

    def __init__(self, gpu):
        self.gpu, self.live = gpu, []

    def add(self, b):
        self.live.append(b)
        return b

    def empty(self, shape, dtype=f16):
        return self.add(self.gpu.empty(shape, dtype))

    def to_dev(self, a):
        return self.add(self.gpu.to_dev(a))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.live:
            b.free()
        self.gpu.sync()


def big(bufs, table, shape):
    """device tensor of `shape` whose row r (over the last axis) is table[r % len(table)], gathered on the device 8 bytes at a time"""
    gpu = bufs.gpu
    p, row = table.shape
    assert row == shape[-1] and row % 4 == 0
    n = int(np.prod(shape[:-1], dtype=np.int64))
    tab = gpu.to_dev(table)
    idx = gpu.to_dev(np.arange(n, dtype=np.int64) % p)
    y = bufs.empty(shape)
    gpu._ck(gpu.lib.osg_gather_rows(gpu.ctx, 8, tab.ptr, idx.ptr, y.ptr, n, row // 4, p))
    gpu.sync()
    tab.free()
    idx.free()
    return y


def blocks(n_rows, row_bytes):
    """row ranges to compare: the first 256, ~300 around the bytes 2^31 and 2^32 (when the tensor reaches them), the last 300"""
    out = [(0, min(256, n_rows))]
    for b in (1 << 31, 1 << 32):
        if n_rows * row_bytes > b:
            r = b // row_bytes
            out.append((max(r - 150, 0), min(r + 150, n_rows)))
    out.append((max(n_rows - 300, 0), n_rows))
    return out


def sentinel(gpu, buf):
    gpu._ck(gpu.lib.osg_memset(gpu.ctx, buf.ptr, 0xFF, buf.nbytes))


def check_gathered(buf, table, n_rows, row_bytes):
    for lo, hi in blocks(n_rows, row_bytes):
        got = buf.read_rows(lo, hi)
        assert np.array_equal(got.view(np.uint16), table[np.arange(lo, hi) % len(table)].view(np.uint16)), f"gathered rows {lo}..{hi}"


def compare(got, want, what):
    bad = np.isnan(got.astype(f32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} rows hold the 0xFF sentinel (NaN), first at offset {int(np.argmax(bad))}: stores dropped"
    e = rel_max(got, want)
    assert e <= 1e-3, f"{what}: rel_max {e:.3g}"


def check_rows(out, n_rows, pitch, want_fn, what, col0=0, ncol=None):
    """every block of `out` (rows `pitch` elements wide; the compared columns col0 .. col0 + ncol) against want_fn(rows)"""
    ncol = ncol if ncol is not None else pitch
    for lo, hi in blocks(n_rows, pitch * 2):
        got = out.read_rows(lo, hi)[:, col0:col0 + ncol]
        compare(got, want_fn(np.arange(lo, hi)), f"{what} rows {lo}..{hi}")


def conv_ref(tx, n_img, H, W, w_ohwi, bias, stride, pads, pix, rb=None, tr=None):
    """ref.conv2d_nhwc restricted to the output pixels `pix` (flat n * Ho * Wo index) of an input whose pixel q is tx[q % len(tx)]"""
    cout, kh, kw, cin = w_ohwi.shape
    sh, sw = stride
    pt, pl, pb, pr = pads
    ho_n, wo_n = (H + pt + pb - kh) // sh + 1, (W + pl + pr - kw) // sw + 1
    n, rem = pix // (ho_n * wo_n), pix % (ho_n * wo_n)
    ho, wo = rem // wo_n, rem % wo_n
    cols = np.zeros((len(pix), kh, kw, cin), f32)
    for i in range(kh):
        for j in range(kw):
            h, w = ho * sh - pt + i, wo * sw - pl + j
            ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            q = (n * H + np.clip(h, 0, H - 1)) * W + np.clip(w, 0, W - 1)
            cols[ok, i, j] = tx[q[ok] % len(tx)]
    extra = np.zeros((len(pix), cout))
    if rb is not None:
        extra += rb[n].astype(np.float64)
    if tr is not None:
        extra += tr[pix % len(tr)].astype(np.float64)
    return ref.matmul(cols.reshape(len(pix), -1), w_ohwi.reshape(cout, -1).T, bias, extra)


# ---- plain GEMM: C and residual past 2 / 4 GiB ------------------------------------------------------------------------------------------------------------
M1 = 1_048_639


def _gemm_case(gpu, monkeypatch, M, N, K, cfg, seed, batch=1):
    rng = np.random.default_rng(seed)
    ta, tr = rnd(rng, (P_A, K)), rnd(rng, (P_R, N))
    w = rnd(rng, (N, K), K ** -0.5)
    bias = rnd(rng, (N,), 0.1, f32)
    if cfg is not None:
        monkeypatch.setenv("OSG_GEMM_CFG", str(cfg)); monkeypatch.setenv("OSG_GEMM_SPLITS", "1"); monkeypatch.setenv("OSG_GEMM_NST", "4")
    rows = M * batch
    with Bufs(gpu) as bufs:
        a, res = big(bufs, ta, (rows, K)), big(bufs, tr, (rows, N))
        dw, db = bufs.to_dev(w), bufs.to_dev(bias)
        c = bufs.empty((rows, N))
        sentinel(gpu, c)
        gpu._ck(gpu.lib.osg_gemm(gpu.ctx, F16, a.ptr, dw.ptr, 1, db.ptr, F32, res.ptr, c.ptr, M, N, K, batch,
                                 M * K if batch > 1 else 0, 0, M * N if batch > 1 else 0, 0))
        check_gathered(a, ta, rows, K * 2)
        check_gathered(res, tr, rows, N * 2)
        check_rows(c, rows, N, lambda r: ref.matmul(ta[r % P_A], w.T, bias, tr[r % P_R]), f"gemm M={M} N={N} x{batch} cfg {cfg}")


@pytest.mark.timeout(120, method="thread")
def test_gemm_output_past_2gib(gpu, monkeypatch):
    """G1: C and residual of 2.5 GiB (64 x 64 tiles: residual prefetched through a pointer, C through the store descriptor)"""
    _gemm_case(gpu, monkeypatch, M1, 1256, 64, 2, 1)


@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("cfg", [2, 0])
def test_gemm_output_past_4gib(gpu, monkeypatch, cfg):
    """G2: C and residual of 4.9 GiB, N = 2504 (ragged for every tile width).  cfg 0 (128 x 128) loads the residual on demand through its descriptor"""
    _gemm_case(gpu, monkeypatch, M1, 2504, 64, cfg, 2)


@pytest.mark.timeout(120, method="thread")
def test_gemm_batched_images_past_4gib(gpu, monkeypatch):
    """G3: three images of 1.2 GiB each (strideC): every image's base pointer is 64-bit already"""
    _gemm_case(gpu, monkeypatch, 503_317, 1280, 64, None, 3, batch=3)


@pytest.mark.timeout(120, method="thread")
def test_gemm_w8_output_past_2gib(gpu):
    """G4: osg_gemm_w8 (uint8 weight codes, the WQ = 1 instantiations) into 2.5 GiB, f16 bias + residual"""
    M, N, K = M1, 1256, 64
    rng = np.random.default_rng(4)
    ta, tr = rnd(rng, (P_A, K)), rnd(rng, (P_R, N))
    q = rng.integers(0, 256, (N, K), dtype=np.uint8)
    scale, zp = 0.02, 131
    wd = (q.astype(np.float64) - zp) * scale
    bias = rnd(rng, (N,), 0.1)
    with Bufs(gpu) as bufs:
        a, res = big(bufs, ta, (M, K)), big(bufs, tr, (M, N))
        dq, db = bufs.to_dev(q), bufs.to_dev(bias)
        c = bufs.empty((M, N))
        sentinel(gpu, c)
        gpu._ck(gpu.lib.osg_gemm_w8(gpu.ctx, a.ptr, dq.ptr, scale, zp, db.ptr, F16, res.ptr, c.ptr, M, N, K, 0))
        check_rows(c, M, N, lambda r: ref.matmul(ta[r % P_A], wd.T, bias, tr[r % P_R]), "gemm_w8")


@pytest.mark.timeout(120, method="thread")
def test_gemm_ln_and_rowstats_past_2gib(gpu):
    """G5: osg_gemm_rowstats (output + its [M][N/32][2] row statistics) and osg_gemm_ln (LayerNorm over K folded in), outputs of 2.7 GiB"""
    M, N, K, eps = M1, 1376, 64, 1e-5
    rng = np.random.default_rng(5)
    ta, tr = rnd(rng, (P_A, K)), rnd(rng, (P_R, N))
    w = rnd(rng, (N, K), K ** -0.5)
    bias = rnd(rng, (N,), 0.1)
    gamma, beta = (1 + rnd(rng, (K,), 0.2).astype(f32)).astype(f16), rnd(rng, (K,), 0.2)
    with Bufs(gpu) as bufs:
        a, res = big(bufs, ta, (M, K)), big(bufs, tr, (M, N))
        dw, db = bufs.to_dev(w), bufs.to_dev(bias)
        c = bufs.empty((M, N))
        rs = bufs.empty((M, N // 16), f32)
        sentinel(gpu, c)
        sentinel(gpu, rs)
        gpu._ck(gpu.lib.osg_gemm_rowstats(gpu.ctx, a.ptr, dw.ptr, db.ptr, F16, res.ptr, c.ptr, M, N, K, 0, rs.ptr))
        check_rows(c, M, N, lambda r: ref.matmul(ta[r % P_A], w.T, bias, tr[r % P_R]), "gemm_rowstats")
        for lo, hi in blocks(M, N * 2):     # the statistics of the rows the kernel stored, 32 columns per slot
            y = c.read_rows(lo, hi).astype(np.float64).reshape(hi - lo, N // 32, 32)
            want = np.stack([y.sum(axis=2), (y * y).sum(axis=2)], axis=2).reshape(hi - lo, N // 16)
            got = rs.read_rows(lo, hi)
            assert not np.isnan(got).any(), f"rowstats rows {lo}..{hi}: sentinel left"
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-3, err_msg=f"rowstats rows {lo}..{hi}")
        rs.free()
        # LayerNorm(A) . W^T + bias + residual, gamma folded into the weight as the planner does (osgpu.Gpu.gemm_ln)
        wf = (gamma.astype(f32)[None, :] * w.astype(f32)).astype(f16)
        c1 = wf.astype(np.float64).sum(axis=1).astype(f32)
        c2 = (w.astype(np.float64) @ beta.astype(np.float64) + bias.astype(np.float64)).astype(f32)
        dwf, d1, d2 = bufs.to_dev(wf), bufs.to_dev(c1), bufs.to_dev(c2)
        sentinel(gpu, c)
        gpu._ck(gpu.lib.osg_gemm_ln(gpu.ctx, a.ptr, dwf.ptr, d1.ptr, d2.ptr, eps, None, res.ptr, c.ptr, M, N, K, 0))

        def want_ln(r):
            x = ta[r % P_A].astype(np.float64)
            xn = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + eps) * gamma.astype(np.float64) + beta.astype(np.float64)
            return ref.matmul(xn, w.T, bias, tr[r % P_R])
        check_rows(c, M, N, want_ln, "gemm_ln")


@pytest.mark.timeout(120, method="thread")
def test_gemm_geglu_output_past_2gib(gpu):
    """G6: GEGLU epilogue (pair-interleaved weight, 2C = 2560) writing a [M, 1280] output of 2.5 GiB"""
    from scipy.special import erf
    M, C, K = M1, 1280, 64
    rng = np.random.default_rng(6)
    ta = rnd(rng, (P_A, K))
    w = rnd(rng, (2 * C, K), K ** -0.5)        # [N, K]: value rows 0 .. C - 1, gate rows C .. 2C - 1
    b = rnd(rng, (2 * C,), 0.1)
    order = np.concatenate([np.r_[16 * k:16 * k + 16, C + 16 * k:C + 16 * k + 16] for k in range(C // 16)])
    with Bufs(gpu) as bufs:
        a = big(bufs, ta, (M, K))
        dw, db = bufs.to_dev(w[order]), bufs.to_dev(b[order])
        y = bufs.empty((M, C))
        sentinel(gpu, y)
        gpu._ck(gpu.lib.osg_gemm(gpu.ctx, F16, a.ptr, dw.ptr, 1, db.ptr, F16, None, y.ptr, M, 2 * C, K, 1, 0, 0, 0, 3))

        def want(r):
            x = ta[r % P_A].astype(np.float64) @ w.T.astype(np.float64) + b.astype(np.float64)
            v, g = x[:, :C], x[:, C:]
            return v * 0.5 * g * (1.0 + erf(g / np.sqrt(2.0)))
        check_rows(y, M, C, want, "gemm geglu")


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------------------------
def _conv_case(gpu, n, H, W, Cin, Cout, k, stride, pads, seed, image_bias=True, residual=True, view_pitch=0):
    rng = np.random.default_rng(seed)
    tx = rnd(rng, (P_X, Cin))
    w = rnd(rng, (Cout, k, k, Cin), (k * k * Cin) ** -0.5)
    bias = rnd(rng, (Cout,), 0.1)
    # (one spare row behind the per-image bias: the base tree's epilogue read up to a tile width past its end on the last column tile -- invisible in the
    # output, whose stores there are dropped -- and an over-read must not leave the allocation)
    rb = rnd(rng, (n, Cout), 0.5) if image_bias else None
    sh, sw = stride
    pt, pl, pb, pr = pads
    Ho, Wo = (H + pt + pb - k) // sh + 1, (W + pl + pr - k) // sw + 1
    M = n * Ho * Wo
    tr = rnd(rng, (P_R, Cout)) if residual else None
    with Bufs(gpu) as bufs:
        x = big(bufs, tx, (n, H, W, Cin))
        res = big(bufs, tr, (n, Ho, Wo, Cout)) if residual else None
        dw, db = bufs.to_dev(w), bufs.to_dev(bias)
        drb = bufs.to_dev(np.concatenate([rb, np.zeros((1, Cout), f16)])) if image_bias else None
        check_gathered(x, tx, n * H * W, Cin * 2)
        want = lambda r: conv_ref(tx, n, H, W, w, bias, stride, pads, r, rb, tr)   # noqa: E731
        args = (n, H, W, Cin, Cout, k, k, sh, sw, pt, pl, pb, pr, 0)
        what = f"conv {n}x{H}x{W}x{Cin} -> {Cout} k{k} s{sh}"
        if view_pitch:
            # osg_conv2d_nhwc_v: columns [Cout, 2 Cout) of a [M, view_pitch] buffer, and a dense [M, Cout] second destination
            wide, dense = bufs.empty((n, Ho, Wo, view_pitch)), bufs.empty((n, Ho, Wo, Cout))
            sentinel(gpu, wide)
            sentinel(gpu, dense)
            gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, F16, x.ptr, dw.ptr, db.ptr, F16, drb.ptr if image_bias else None, Cout if image_bias else 0,
                                              res.ptr if residual else None, wide.ptr + Cout * 2, view_pitch, dense.ptr, Cout, *args))
            check_rows(wide, M, view_pitch, want, what + " (view)", col0=Cout, ncol=Cout)
            check_rows(dense, M, Cout, want, what + " (dense)")
            return
        y = bufs.empty((n, Ho, Wo, Cout))
        sentinel(gpu, y)
        if image_bias:
            gpu._ck(gpu.lib.osg_conv2d_nhwc_rb(gpu.ctx, F16, x.ptr, dw.ptr, db.ptr, F16, drb.ptr, Cout, res.ptr if residual else None, y.ptr, *args))
        else:
            gpu._ck(gpu.lib.osg_conv2d_nhwc(gpu.ctx, F16, x.ptr, dw.ptr, db.ptr, F16, res.ptr if residual else None, y.ptr, *args))
        check_rows(y, M, Cout, want, what)


@pytest.mark.timeout(120, method="thread")
def test_conv3x3_halo_output_past_2gib(gpu, monkeypatch):
    """C1: the halo-reuse 3x3 kernel (W = 64, forced 128-wide tile, one slab range) with per-image bias + residual into 2.5 GiB: the !BATCH epilogue"""
    monkeypatch.setenv("OSG_CONV3X3_BN", "128"); monkeypatch.setenv("OSG_CONV3X3_SPLITS", "1")
    _conv_case(gpu, 1, 16384, 64, 64, 1256, 3, (1, 1), (1, 1, 1, 1), 11)


@pytest.mark.timeout(120, method="thread")
def test_conv3x3_implicit_gemm_output_past_2gib(gpu, monkeypatch):
    """C1b: a 3x3 convolution the halo kernel declines (W = 128) through gemm2_kernel<CONV>, 128 x 128 tiles (on-demand per-image bias + residual)"""
    monkeypatch.setenv("OSG_GEMM_CFG", "0"); monkeypatch.setenv("OSG_GEMM_SPLITS", "1"); monkeypatch.setenv("OSG_GEMM_NST", "4")
    _conv_case(gpu, 1, 8192, 128, 64, 1256, 3, (1, 1), (1, 1, 1, 1), 12)


@pytest.mark.timeout(120, method="thread")
def test_conv1x1_batched_output_past_4gib(gpu, monkeypatch):
    """C2: 1x1 convolution of two images (a GEMM over the pixels), 128 x 128 tiles, per-image bias with N % 128 != 0, C and residual of 4.9 GiB"""
    monkeypatch.setenv("OSG_GEMM_CFG", "0"); monkeypatch.setenv("OSG_GEMM_SPLITS", "1"); monkeypatch.setenv("OSG_GEMM_NST", "4")
    _conv_case(gpu, 2, 1024, 1024, 64, 1256, 1, (1, 1), (0, 0, 0, 0), 13)


@pytest.mark.timeout(120, method="thread")
def test_conv_view_past_4gib(gpu):
    """C3: osg_conv2d_nhwc_v into the upper half of a buffer of pitch 2 Cout (4.9 GiB) plus a dense second destination of 2.5 GiB"""
    _conv_case(gpu, 1, 1024, 1024, 64, 1256, 1, (1, 1), (0, 0, 0, 0), 14, view_pitch=2 * 1256)


@pytest.mark.timeout(120, method="thread")
def test_conv3x3_stride2_output_past_2gib(gpu):
    """C4: stride-2 3x3 convolution (implicit GEMM) with bias + residual into 2.1 GiB"""
    _conv_case(gpu, 1, 2048, 2048, 64, 1096, 3, (2, 2), (1, 1, 1, 1), 15, image_bias=False)


# ---- operands of 2 GiB or more: the pointer-based fallback kernel -------------------------------------------------------------------------------------------
@pytest.mark.timeout(120, method="thread")
@pytest.mark.parametrize("M,K,N", [(900_001, 1280, 64), (17_000_000, 64, 76)])
def test_gemm_operand_past_2gib(gpu, M, K, N):
    """I1: A of 2 GiB or more takes gemm_kernel (M tiles in grid.y); the second shape has ~133 000 row tiles and a 2.4 GiB output"""
    rng = np.random.default_rng(M + K)
    ta, tr = rnd(rng, (P_A, K)), rnd(rng, (P_R, N))
    w = rnd(rng, (N, K), K ** -0.5)
    bias = rnd(rng, (N,), 0.1)
    with Bufs(gpu) as bufs:
        a, res = big(bufs, ta, (M, K)), big(bufs, tr, (M, N))
        dw, db = bufs.to_dev(w), bufs.to_dev(bias)
        c = bufs.empty((M, N))
        sentinel(gpu, c)
        gpu._ck(gpu.lib.osg_gemm(gpu.ctx, F16, a.ptr, dw.ptr, 1, db.ptr, F16, res.ptr, c.ptr, M, N, K, 1, 0, 0, 0, 0))
        check_gathered(a, ta, M, K * 2)
        check_rows(c, M, N, lambda r: ref.matmul(ta[r % P_A], w.T, bias, tr[r % P_R]), f"gemm fallback M={M} K={K}")


@pytest.mark.timeout(120, method="thread")
def test_conv_input_past_2gib(gpu):
    """I2: a 3x3 convolution whose input is 2.2 GiB (1 x 1900 x 1900 x 320): past the halo kernel's and gemm2_kernel's operand limit"""
    _conv_case(gpu, 1, 1900, 1900, 320, 64, 3, (1, 1), (1, 1, 1, 1), 16, image_bias=False)
