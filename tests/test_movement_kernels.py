"""-m gpu: the data-movement kernels (onnxstream_amd/csrc/osg_move.hip) and osg_convert, bit exact against numpy indexing.

Every destination is a view between two guard bands of one 0xFF-filled allocation (Gpu.empty); the bands, and every gap a pitch leaves inside the
destination, must come back 0xFF.  No source element consists of 0xFF bytes alone (integers below the all-ones pattern, floats that are not NaN), so an element
the kernel never wrote shows as a mismatch.  Every case is seeded and frees its buffers.

  osg_transpose      every permutation of every shape of rank 1 to 4 with dims drawn from {1, 2, 33} (33 crosses the 32 x 32 LDS tile; the 1s and the
                     permutations that keep neighbours together walk the dimension merging of run_transpose: plain copies, the batched 2-D LDS kernel,
                     transpose_nd_kernel at canonical ranks 2 to 4), 2-byte elements; a tenth of them, by a seeded draw, at 1, 4 and 8 bytes as well;
                     twenty seeded shape / permutation pairs each at ranks 5 and 6; the two fallbacks of the LDS kernel onto transpose_nd_kernel
                     (batch > 65535, rows / 32 > 65535).
  osg_copy_2d,       per element size one case for every vector width the entry point can pick (16, 8, 4, 2, 1 bytes, not below the element): pitches,
  osg_concat2        offsets and inner lengths are odd multiples of that width, so the next width is ruled out; outer 1 and 7.
  osg_resize_nearest element sizes 1, 2, 4; NHWC on the 16-byte path, NHWC with C = 5 (scalar), NCHW; 2x (the UNet's), identity, 3x / 2x, a fractional
                     upscale and a downscale.  Reference index: the contract min(floor(f32(o) * (f32(H) / f32(Ho))), H - 1) in numpy float32, which for
                     integer factors must equal o // factor.
  osg_gather_rows    element sizes 1, 2, 4, 8; repeated and negative indices, rows of 1 and 33 elements, a single index.
  osg_maxpool_nhwc   f16 and f32; 5 / 1 / pads 2, 3 / 2 / pads 1, 2 / 2 / no pads, 3 / 1 / pads (0, 1, 0, 1); C = 3 and 128; -inf and the largest finite value
                     in the input.
  osg_convert        f16 -> u8 and f32 -> u8 at exact half-code ties and beyond both ends of the range (oracle/np_ops.quantize_u8), f32 -> f16 at overflow
                     and at subnormals; n = 1, 255, 257, 2^20 + 3 (the grid-stride loop: more elements than threads launched).
"""
import itertools

import numpy as np
import pytest

import test_unet_attention_norm as an
from oracle import np_ops as ref

pytestmark = pytest.mark.gpu
dev = an.dev
GUARD = an.GUARD
f16, f32 = np.float16, np.float32
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def source(rng, shape, es):
    """unsigned integers of es bytes, none of them the all-ones pattern"""
    hi = 2 ** 63 if es == 8 else 2 ** (8 * es) - 1
    return rng.integers(0, hi, size=shape, dtype=np.uint64).astype(UINT[es])


def bits(a):
    return np.ascontiguousarray(a).view(UINT[a.dtype.itemsize])


def read(buf, shape):
    """the view of `shape` behind the first guard band of buf, after checking both bands"""
    raw = bits(buf.numpy())
    n = int(np.prod(shape))
    ones = UINT[raw.dtype.itemsize](~UINT[raw.dtype.itemsize](0))
    assert (raw[:GUARD] == ones).all() and (raw[GUARD + n:] == ones).all(), "a store landed in a guard band"
    return raw[GUARD:GUARD + n].reshape(shape)


def same(got, want, what):
    want = bits(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {want.size} elements differ; first at {tuple(int(x) for x in bad[0])}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}")


# ---- osg_transpose -------------------------------------------------------------------------------------------------------------------------------------
def transpose_sweep(gpu, dev, pairs_by_shape, sizes_of):
    """pairs_by_shape: shape -> [perm]; sizes_of(shape, perm) -> element sizes to run.  One upload per (shape, element size), one destination per shape."""
    launches = 0
    for shape, perms in pairs_by_shape.items():
        n = int(np.prod(shape))
        rng = np.random.default_rng(sum(d * 37 ** i for i, d in enumerate(shape)))
        src, dsrc, dbuf = {}, {}, {}
        for perm in perms:
            for es in sizes_of(shape, perm):
                if es not in src:
                    src[es] = source(rng, shape, es)
                    dsrc[es] = dev(src[es])
                    dbuf[es] = dev.nan(n + 2 * GUARD, UINT[es])
                else:
                    gpu.memset(dbuf[es], 0xFF)
                oshape = tuple(shape[p] for p in perm)
                gpu.transpose(dsrc[es], perm, out=dbuf[es].view(GUARD, oshape))
                same(read(dbuf[es], oshape), np.transpose(src[es], perm), f"transpose {shape} perm {perm} element size {es}")
                launches += 1
    return launches


@pytest.mark.parametrize("rank", [1, 2, 3, 4])
def test_transpose_every_permutation(gpu, dev, rank):
    draw = np.random.default_rng(rank)
    wide = {}                                       # (shape, perm) -> also at 1, 4 and 8 bytes: a tenth, by a seeded draw
    pairs = {}
    for shape in itertools.product((1, 2, 33), repeat=rank):
        pairs[shape] = list(itertools.permutations(range(rank)))
        for perm in pairs[shape]:
            wide[(shape, perm)] = draw.random() < 0.1
    n = transpose_sweep(gpu, dev, pairs, lambda s, p: (2, 1, 4, 8) if wide[(s, p)] else (2,))
    assert n >= 3 ** rank * len(list(itertools.permutations(range(rank))))


@pytest.mark.parametrize("rank", [5, 6])
def test_transpose_rank_5_and_6(gpu, dev, rank):
    rng = np.random.default_rng(rank)
    pairs = {}
    while sum(len(v) for v in pairs.values()) < 20:
        shape = tuple(int(x) for x in rng.choice((1, 2, 3, 5, 33), size=rank))
        if np.prod(shape) > 1 << 20:
            continue
        pairs.setdefault(shape, []).append(tuple(int(x) for x in rng.permutation(rank)))
    transpose_sweep(gpu, dev, pairs, lambda s, p: (2, 8) if sum(p) % 2 else (2, 4))


@pytest.mark.parametrize("shape,perm", [((65536, 2, 3), (0, 2, 1)), ((2097153, 2), (1, 0))], ids=["batch-65536", "rows-2097153"])
def test_transpose_lds_kernel_fallbacks(gpu, dev, shape, perm):
    """a batched 2-D transpose whose grid the LDS kernel cannot take (blockIdx.z / blockIdx.y limits) runs on transpose_nd_kernel"""
    transpose_sweep(gpu, dev, {shape: [perm]}, lambda s, p: (2,))


# ---- osg_copy_2d, osg_concat2 --------------------------------------------------------------------------------------------------------------------------
WIDTHS = [(es, w) for es in (1, 2, 4, 8) for w in (16, 8, 4, 2, 1) if w >= es]


@pytest.mark.parametrize("outer", [1, 7])
@pytest.mark.parametrize("es,w", WIDTHS, ids=[f"es{es}-w{w}" for es, w in WIDTHS])
def test_copy_2d(gpu, dev, es, w, outer):
    u = w // es                                    # elements per vector: every quantity below an odd multiple of it
    sp, so, dp, do, inner = 41 * u, 3 * u, 45 * u, 5 * u, 35 * u
    rng = np.random.default_rng(es * 100 + w + outer)
    src = source(rng, (outer * sp,), es)
    buf = dev.nan(outer * dp + 2 * GUARD, UINT[es])
    gpu.copy_2d(dev(src), sp, so, buf.view(GUARD, (outer * dp,)), dp, do, outer, inner)
    want = np.full((outer, dp), ~UINT[es](0), UINT[es])
    want[:, do:do + inner] = src.reshape(outer, sp)[:, so:so + inner]
    same(read(buf, (outer, dp)), want, f"copy_2d element size {es} width {w} outer {outer}")


@pytest.mark.parametrize("outer", [1, 7])
@pytest.mark.parametrize("es,w", [p for p in WIDTHS if p[0] != 8], ids=[f"es{es}-w{w}" for es, w in WIDTHS if es != 8])
def test_concat2(gpu, dev, es, w, outer):
    u = w // es
    ia, ib = 35 * u, 9 * u
    rng = np.random.default_rng(es * 100 + w + outer)
    a, b = source(rng, (outer, ia), es), source(rng, (outer, ib), es)
    buf = dev.nan(outer * (ia + ib) + 2 * GUARD, UINT[es])
    gpu.concat2(dev(a), dev(b), out=buf.view(GUARD, (outer, ia + ib)))
    same(read(buf, (outer, ia + ib)), np.concatenate([a, b], axis=1), f"concat2 element size {es} width {w} outer {outer}")


# ---- osg_resize_nearest --------------------------------------------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out):
    idx = np.minimum(np.floor(np.arange(n_out, dtype=f32) * (f32(n_in) / f32(n_out))).astype(np.int64), n_in - 1)
    if n_out % n_in == 0:
        assert np.array_equal(idx, np.arange(n_out) // (n_out // n_in)), "an integer factor: the contract is o // factor"
    return idx


SIZES = [(16, 16, 32, 32), (6, 7, 6, 7), (4, 6, 12, 12), (5, 7, 8, 9), (8, 9, 3, 4)]


@pytest.mark.parametrize("H,W,Ho,Wo", SIZES, ids=[f"{s[0]}x{s[1]}-to-{s[2]}x{s[3]}" for s in SIZES])
@pytest.mark.parametrize("layout", ["nhwc16", "nhwc5", "nchw"])
@pytest.mark.parametrize("es", [1, 2, 4])
def test_resize_nearest(gpu, dev, es, layout, H, W, Ho, Wo):
    N = 2
    C = {"nhwc16": 48 // es, "nhwc5": 5, "nchw": 3}[layout]
    nhwc = layout != "nchw"
    rng = np.random.default_rng(es + H * 7 + Wo + len(layout))
    x = source(rng, (N, H, W, C) if nhwc else (N, C, H, W), es)
    hi, wi = nearest_index(H, Ho), nearest_index(W, Wo)
    want = x[:, hi][:, :, wi] if nhwc else x[:, :, hi][:, :, :, wi]
    buf = dev.nan(want.size + 2 * GUARD, UINT[es])
    gpu.resize_nearest(dev(x), Ho, Wo, nhwc, out=buf.view(GUARD, want.shape))
    same(read(buf, want.shape), want, f"resize {layout} element size {es}")


# ---- osg_gather_rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [[3, 3, -1, 0, -7, 6, 3, 3], [-2]], ids=["repeated-negative", "single"])
@pytest.mark.parametrize("row", [1, 33])
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_gather_rows(gpu, dev, es, row, idx):
    x = source(np.random.default_rng(es + row), (7, row), es)
    buf = dev.nan(len(idx) * row + 2 * GUARD, UINT[es])
    gpu.gather_rows(dev(x), dev(np.array(idx, np.int64)), out=buf.view(GUARD, (len(idx), row)))
    same(read(buf, (len(idx), row)), x[idx], f"gather_rows element size {es} row {row}")


# ---- osg_maxpool_nhwc ----------------------------------------------------------------------------------------------------------------------------------
POOLS = [(5, 1, (2, 2, 2, 2)), (3, 2, (1, 1, 1, 1)), (2, 2, (0, 0, 0, 0)), (3, 1, (0, 1, 0, 1))]       # (k, stride, (top, left, bottom, right))


@pytest.mark.parametrize("k,stride,pads", POOLS, ids=[f"k{k}-s{s}-p{''.join(map(str, p))}" for k, s, p in POOLS])
@pytest.mark.parametrize("C", [3, 128])
@pytest.mark.parametrize("dtype", [f16, f32], ids=["f16", "f32"])
def test_maxpool(gpu, dev, dtype, C, k, stride, pads):
    N, H, W = 2, 9, 11
    rng = np.random.default_rng(C + k * 10 + stride)
    x = rng.standard_normal((N, H, W, C)).astype(dtype)
    x[rng.random(x.shape) < 0.2] = -np.inf                       # (windows of -inf alone at C = 3 ... )
    x[0, :3, :3] = -np.inf
    x[rng.random(x.shape) < 0.02] = np.finfo(dtype).max
    pt, pl, pb, pr = pads
    xp = np.full((N, H + pt + pb, W + pl + pr, C), -np.inf, dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    want = np.stack([np.stack([xp[:, i * stride:i * stride + k, j * stride:j * stride + k].max(axis=(1, 2)) for j in range(Wo)], axis=1) for i in range(Ho)], axis=1)
    assert want.shape == (N, Ho, Wo, C) and np.isinf(want).any() and (want == np.finfo(dtype).max).any()
    buf = dev.nan(want.size + 2 * GUARD, dtype)
    gpu.maxpool_nhwc(dev(x), (k, k), (stride, stride), pads, out=buf.view(GUARD, want.shape))
    same(read(buf, want.shape), want, f"maxpool {np.dtype(dtype).name} C {C} k {k} stride {stride} pads {pads}")


# ---- osg_convert ---------------------------------------------------------------------------------------------------------------------------------------
NS = [1, 255, 257, (1 << 20) + 3]


def tiled(values, n):
    return np.resize(np.asarray(values), n)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", [f16, f32], ids=["f16", "f32"])
def test_convert_to_u8(gpu, dev, dtype, n):
    """x / scale exactly half way between two codes (scale a power of two: the product is exact) rounds to the even code; the ends of the range clamp"""
    scale, zp = 0.25, 7
    codes = np.array([-9, -8, -7, -1, 0, 1, 2, 100, 101, 253, 254, 255, 256, 257, 300])
    big = [1000.0, -1000.0, 60000.0, -60000.0] + ([1e30, -1e30, 3e38, -3e38] if dtype == f32 else [65504.0, -65504.0])
    vals = np.concatenate([(codes - zp + 0.5) * scale, (codes - zp) * scale, (codes - zp + 0.25) * scale, big]).astype(dtype)
    x = tiled(vals, n)
    if n > 1 << 20:                # ... and a scale whose reciprocal is inexact, on ordinary values
        scale, zp = 0.1, 128
        x = (np.random.default_rng(n).standard_normal(n) * 8).astype(dtype)
        x[:vals.size] = vals
    want = ref.quantize_u8(x.astype(f32), scale, zp)
    buf = dev.nan(n + 2 * GUARD, np.uint8)
    gpu.convert(dev(x), np.uint8, scale, zp, out=buf.view(GUARD, (n,)))
    same(read(buf, (n,)), want, f"convert {np.dtype(dtype).name} -> u8 n {n}")


@pytest.mark.parametrize("n", NS)
def test_convert_f32_to_f16_overflow_and_subnormals(gpu, dev, n):
    t = 2.0 ** -24                                  # the smallest f16 subnormal
    vals = [65504.0, 65519.996, 65520.0, 65536.0, 1e10, 3e38, t, t / 2, t / 2 * (1 + 2.0 ** -20), 1.5 * t, 2.5 * t, t / 4, 1e-30, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
            2.0 ** -14 - t / 2, 1023.5 * t, 0.0]
    vals = np.array(vals + [-v for v in vals], f32)
    x = tiled(vals, n)
    if n > 1 << 20:
        x = np.concatenate([vals, (np.random.default_rng(n).standard_normal(n - vals.size) * 2.0 ** np.random.default_rng(n + 1).integers(-30, 18, n - vals.size)).astype(f32)])
    with np.errstate(over="ignore"):
        want = x.astype(f16)
    assert n == 1 or (np.isinf(want).any() and (want == 0).any())
    buf = dev.nan(n + 2 * GUARD, f16)
    gpu.convert(dev(x), f16, out=buf.view(GUARD, (n,)))
    same(read(buf, (n,)), want, f"convert f32 -> f16 n {n}")
