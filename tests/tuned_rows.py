"""The shipped tune table (onnxstream_amd/tune/mi355x.txt) row by row: each row as the call it describes, the route osg_last_route must report for its choice,
and a float64 reference of every output element.  No GPU in here: tests/test_tuned_rows_cpu.py exercises it on the host, tests/tuned_rows_worker.py
launches the rows (tests/test_tuned_rows.py).

* Row -> call.  The 13 key fields as tune_key (osg_gemm_select.h) forms them: kind 0 osg_gemm (lda == K; flags 128 osg_gemm_ln, with 256 on handed-over row
  statistics; 512 osg_gemm_rowstats; 1024 osg_gemm_w8 / osg_gemm_w8_v), kind 1 the 3 x 3 / stride 1 / pad 1 convolution, kind 2 any other convolution
  (KH = KW, pad KW // 2); low flag bits the activation, 16 a residual, 32 a per-image bias, 64 an f32 bias.  A bias is always passed.  uint8 rows on even
  table lines take scalar (scale, zero point), on odd lines with N % 4 == 0 per-column vectors.
* Row -> route.  Family 0: the entry tests/cpp/contraction_routes.cpp's resolve mode gives for the row's (cfg & 7, nst, KS, fold, spec) under the row's own
  form; family 1: resolve3 of (W, bn, loader waves, uint8).  The k-slices that run (no empty slice), the fold bit as splitk_fold_route grants it, the reduce kernel.
* Reference.  Operands, bounds and the comparison are those of tests/test_contraction_instantiations.py (imported, not restated): every element against
  float64 within 2^-11 |want| + (1 + 2^-11) E + 2^-25, at most FAR of the elements more than one f16 ulp from the correctly rounded result.  The bounds depend on
  K and the operands only.  Where the float64 [M, K] operand fits LIMIT the operands are plain random and the reference is the brute-force product, formed in
  chunks of rows (and of columns for a very wide weight) so that no float64 array passes LIMIT.  The larger rows get a STRUCTURED activation whose reference is
  exact without the [M, K] product:
    GEMM         A[i] = block[i mod P] with P an odd prime >= 131 (coprime to every tile height, chosen by the table line), the marker columns -- the first
                 k-tile of the first, middle and last k-slice of the row's split and the first, middle and last k-tile -- hold (i mod 64, i / 64 mod 64,
                 i / 4096 mod 64) / 32 instead: no two of any 4096 consecutive rows are equal.  want and S = |a| . |b| are the block's float64 product plus the
                 markers' rank-one terms.
    convolution  x[n, h, w] = T[h mod Ph, w mod Pw] with one channel holding a per-pixel marker instead.  Interior pixels: the torus convolution of one
                 period plus the single-channel 3 x 3 sum of the markers; pixels whose window touches the padding: the direct product of their own patches.
  (No folded-LayerNorm or row-statistics row is that large; their statistics would need a structured form of their own.)
"""
import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np

import test_contraction_instantiations as ci

f16, f32, f64, U = ci.f16, ci.f32, ci.f64, ci.U
TABLE = os.path.join(ci.REPO, "onnxstream_amd", "tune", "mi355x.txt")
LIMIT = 512 << 20                 # bytes of the largest float64 array
CHUNK = LIMIT // 8 // 4           # elements of a working array (several are alive at a time)
THREADS = 4                        # blocks of the comparison in flight
K_TICKETS = 1 << 16               # osg_ctx::kTickets (osg_common.h); the split-K fold owns the lower half
PRIMES = (131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199, 211)
CONV_PERIODS = ((5, 7), (7, 5), (5, 9), (9, 7), (7, 11), (11, 5))
ACT_NONE, ACT_SILU, ACT_GEGLU = ci.ACT_NONE, ci.ACT_SILU, ci.ACT_GEGLU


# ---- a row ---------------------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    line: int
    kind: int
    device: int
    M: int
    N: int
    K: int
    batch: int
    H: int
    W: int
    Cin: int
    KW: int
    sh: int
    sw: int
    flags: int
    family: int
    cfg: int
    nst: int
    splits: int
    bn: int
    us: float = 0.0

    # the form
    act = property(lambda s: s.flags & 15)
    residual = property(lambda s: bool(s.flags & 16))
    rowbias = property(lambda s: bool(s.flags & 32))
    bias_f32 = property(lambda s: bool(s.flags & 64))
    ln = property(lambda s: bool(s.flags & 128))
    rs_in = property(lambda s: bool(s.flags & 256))
    rs_out = property(lambda s: bool(s.flags & 512))
    w8 = property(lambda s: bool(s.flags & 1024))
    vec = property(lambda s: s.w8 and s.line % 2 == 1 and s.N % 4 == 0)
    conv = property(lambda s: s.kind != 0)
    no_split = property(lambda s: s.act == ACT_GEGLU or s.ln or s.rs_out)          # run_gemm_v2's allow_split, negated
    # the convolution's geometry
    k = property(lambda s: 3 if s.kind == 1 else s.KW)
    stride = property(lambda s: 1 if s.kind == 1 else s.sh)
    pad = property(lambda s: s.k // 2)
    Ho = property(lambda s: (s.H + 2 * s.pad - s.k) // s.stride + 1)
    Wo = property(lambda s: (s.W + 2 * s.pad - s.k) // s.stride + 1)
    images = property(lambda s: s.M // (s.Ho * s.Wo))
    rows = property(lambda s: s.M * s.batch)                                        # rows of the output
    cols = property(lambda s: s.N // 2 if s.act == ACT_GEGLU else s.N)              # columns of the output
    # the choice
    tile = property(lambda s: s.cfg & 7)
    ks = property(lambda s: 2 if s.cfg & 8 else 1)
    fold = property(lambda s: (s.cfg >> 4) & 1)
    spec = property(lambda s: (s.cfg >> 5) & 1)

    @property
    def op(self):
        if self.conv:
            return "conv_w8" if self.w8 else "conv"
        return "gemm_ln" if self.ln else "gemm_rowstats" if self.rs_out else "gemm_w8" if self.w8 else "gemm"

    @property
    def id(self):
        what = {0: "gemm", 1: "conv3x3", 2: "conv"}[self.kind]
        if self.ln:
            what = "ln"
        elif self.rs_out:
            what = "rowstats"
        return f"L{self.line:03d}-{what}-{self.M}x{self.N}x{self.K}-{'w8' if self.w8 else 'f16'}"

    def check_decodes(self):
        """the row describes a call the entry points accept and tune_key maps back onto it"""
        where = f"table line {self.line}"
        assert self.kind in (0, 1, 2) and self.device == 0 and min(self.M, self.N, self.K, self.batch) > 0, where
        assert self.flags & ~2047 == 0 and self.act in (ACT_NONE, ACT_SILU, ACT_GEGLU), f"{where}: flags {self.flags}"
        if self.act == ACT_GEGLU:
            assert self.N % 32 == 0 and not self.residual and self.batch == 1 and not self.conv, f"{where}: GEGLU needs N % 32 == 0, no residual, a GEMM"
        if self.kind == 0:
            assert self.H == self.K and (self.W, self.Cin, self.KW, self.sh, self.sw) == (0,) * 5, f"{where}: a GEMM row carries lda == K and no geometry"
            assert not self.rowbias, f"{where}: the per-image bias exists on convolution rows only"
            assert not self.rs_in or self.ln, f"{where}: handed-over row statistics without the folded LayerNorm"
            assert not self.ln or (self.bias_f32 and not self.rs_out and not self.w8 and self.N % 4 == 0), f"{where}: osg_gemm_ln passes c2 as an f32 bias"
            assert not self.rs_out or (self.N % 32 == 0 and not self.w8), f"{where}: osg_gemm_rowstats needs N % 32 == 0"
            assert self.batch == 1 or self.op == "gemm", f"{where}: only osg_gemm takes a batch"
        else:
            assert self.batch == 1 and not (self.ln or self.rs_in or self.rs_out), f"{where}: a convolution row is one plain launch"
            assert (self.k == 3 and self.sh == self.sw == 1 and self.KW == 3) if self.kind == 1 else (self.sh == self.sw and self.KW % 2 == 1), where
            assert self.K == self.k * self.k * self.Cin and self.M == self.images * self.Ho * self.Wo and self.images > 0, f"{where}: M, K do not follow from the geometry"
            assert not (self.Cin == 4 and self.k == 3 and not self.w8), f"{where}: conv_cin4_mfma_kernel takes this shape before the table is asked"
            assert self.k > 1, f"{where}: a 1 x 1 convolution looks its row up as a GEMM"
            halo = self.k == 3 and self.stride == 1 and self.W in (8, 16, 32, 64) and self.N % 4 == 0 and self.H % (128 // (self.W * (2 if self.W == 8 else 1))) == 0 and \
                (self.W != 8 or self.H == 8)
            assert halo == (self.kind == 1), f"{where}: kind {self.kind}, but osg_conv3x3_prepare {'takes' if halo else 'refuses'} the shape"


@lru_cache(maxsize=None)
def rows():
    out = []
    for i, text in enumerate(open(TABLE).read().splitlines(), 1):
        f = text.split()
        assert len(f) == 19, f"table line {i}: {len(f)} fields"
        out.append(Row(i, *map(int, f[:18]), float(f[18])))
    return out


# ---- the route a row's choice runs -----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def resolutions():
    """({(form bits, nch, cfg, nst, ks, fold, spec): (entry, fold)}, {(w, bn, loader waves, w8): entry}) of the driver's resolve mode"""
    v2, v3 = {}, {}
    for line in ci.driver()["resolve"].splitlines():
        f = line.split()
        if f[0] == "r":
            v2[tuple(map(int, f[1:8]))] = (int(f[8]), int(f[9]))
        else:
            v3[tuple(map(int, f[1:5]))] = int(f[5])
    return v2, v3


def form_bits(r):
    return (ci.CONV if r.conv else 0) | (ci.LN1 if r.ln and not r.rs_in else 0) | (ci.LN2 if r.ln and r.rs_in else 0) | (8 if r.act == ACT_GEGLU else 0) | \
        (16 if r.rs_out else 0) | (ci.W8 if r.w8 else 0)


@dataclasses.dataclass(frozen=True)
class Route:
    route: tuple          # what osg_last_route reports: (family, entry, k-slices, fold, reduce kernel)
    bm: int
    bn: int
    tiles: int            # output tiles of the launch
    ktiles: int           # units the split divides: 64-deep k-tiles (family 0), 64-channel slabs (family 1)
    fold_asked: bool      # the row asks for the fold and its entry can fold

    workgroups = property(lambda s: s.tiles * s.route[2])


def expected_route(r):
    v2e, v3e, _ = ci.table()
    v2, v3 = resolutions()
    if r.family == 0:
        nch = 5 if not (r.ln and r.rs_in) else 5 if r.K // 64 <= 5 else 10 if r.K // 64 <= 10 else 20       # v2_nch of the K / 32 slots
        entry, fold = v2[(form_bits(r), nch, r.tile, r.nst, r.ks, r.fold, r.spec)]
        if entry < 0:
            return Route((0, entry, 0, 0, 0), 0, 0, 0, 0, False)
        bm, bn, ktiles = v2e[entry]["bm"], v2e[entry]["bn"], r.K // 64
        tiles = r.batch * -(-r.M // bm) * -(-r.N // bn)
    else:
        entry, fold = v3[(r.W, r.bn, 8 if r.nst == 8 else 4, int(r.w8))], r.fold
        if entry < 0:
            return Route((1, entry, 0, 0, 0), 0, 0, 0, 0, False)
        bm, bn, ktiles = 128, v3e[entry]["bn"], r.Cin // 64
        tiles = -(-r.M // 128) * -(-r.N // bn)
    s = ci.slices(ktiles, max(r.splits, 1))
    # splitk_fold_route
    folded = int(bool(fold) and 2 <= s <= 4 and 2 * tiles + 16 <= K_TICKETS // 2 and r.N % 4 == 0 and not r.no_split)
    return Route((r.family, entry, s, folded, ci.reduce_kernel(s, folded, r.N)), bm, bn, tiles, ktiles, bool(fold))


def check_legal(r):
    """the row's choice is legal for the form that looks it up: what run_gemm_v2, splitk_fold_route and conv2d_route take for granted, restated"""
    where = f"table line {r.line} ({r.id})"
    assert r.family in (0, 1) and (r.family == 0 or r.kind == 1), f"{where}: the halo kernel serves kind 1 only"
    e = expected_route(r)
    assert e.route[1] >= 0, f"{where}: no instantiation takes the choice under the row's own form"
    assert r.splits >= 1 and (not r.no_split or r.splits == 1), f"{where}: GEGLU, folded LayerNorm and row statistics live in the tile epilogue: splits {r.splits}"
    assert (r.Cin if r.conv else r.K) % 64 == 0, f"{where}: K (Cin) must be a multiple of 64"
    if r.fold:
        assert e.fold_asked and 2 <= e.route[2] <= 4, f"{where}: a fold row runs 2 .. 4 k-slices on a fold-capable entry, not {e.route[2]}"
        assert 2 * e.tiles + 16 <= K_TICKETS // 2, f"{where}: {e.tiles} tiles do not fit the fold's half of the ticket array"
        assert e.route[3] == 1, f"{where}: the fold is not granted (N % 4, epilogue form)"
    if r.family == 1:
        assert r.nst in (0, 4, 8) and not (r.w8 and r.nst == 8), f"{where}: uint8 codes run the 4-loader kernel only"
        assert r.cfg in (0, 16), f"{where}: a halo-kernel row's cfg holds the fold bit only"
    if r.w8:
        assert not (r.ks == 2 or r.spec), f"{where}: uint8 codes have no KS = 2 / four-loader-wave instantiation"
    if r.ln and r.rs_in:
        assert r.K <= 1280 and r.K % 32 == 0, f"{where}: handed-over row statistics need K <= 1280"
    return e


# ---- operands and references -------------------------------------------------------------------------------------------------------------------------
def markers(i):
    """three small-integer markers (exact in f16) of row / pixel index i: equal only for indices 2^18 apart"""
    return [((i >> s) & 63).astype(f64) / 32.0 for s in (0, 6, 12)]


def marker_columns(ktiles, slices_, unit=64):
    """columns in the first k-tile of the first, middle and last k-slice and in the first, middle and last k-tile, each with the marker it holds"""
    per = -(-ktiles // slices_)
    tiles = sorted({0, (slices_ // 2) * per, (slices_ - 1) * per, ktiles // 2, ktiles - 1})
    if len(tiles) < 3:
        return [(t * unit + 5 + 11 * j, j) for t in tiles for j in range(3)][:3] if len(tiles) == 1 else [(tiles[0] * unit + 5, 0), (tiles[1] * unit + 5, 1), (tiles[1] * unit + 21, 2)]
    return [(t * unit + 5 + 3 * j, j % 3) for j, t in enumerate(tiles)]


class Case:
    """the operands of a row's call and the float64 reference of any block of its output"""

    def __init__(self, r, structured=None):
        self.r = r
        self.route = expected_route(r)
        rng = self.rng = np.random.default_rng(1000003 * r.line + 17)
        self.structured = (r.rows * r.K * 8 > LIMIT) if structured is None else structured
        assert not (self.structured and (r.ln or r.rs_out)), "no structured form of the row statistics"
        N, K = r.N, r.K
        # the weight: f16 values ~ N(0, 1 / K), or uint8 codes with scalar or per-column (scale, zero point)
        shape = (N, r.k, r.k, r.Cin) if r.conv else (N, K)
        self.scale = self.zp = self.vecs = None
        if r.w8:
            self.w, self.zp, self.scale = ci.quant(rng, shape)
            if r.vec:
                self.vecs = ci.quant_vectors(rng, N, self.scale)
        else:
            self.w = ci.rnd(rng, shape, K ** -0.5)
        self.bias = ci.rnd(rng, (N,), 0.1, f32 if r.bias_f32 else f16)
        self.ib = ci.rnd(rng, (r.images, N), 0.5) if r.rowbias else None
        if r.ln:
            self.gamma, self.beta = (1 + ci.rnd(rng, (K,), 0.2).astype(f32)).astype(f16), ci.rnd(rng, (K,), 0.2)
            self.folded = ci.ln_fold(self.w, self.gamma, self.beta, self.bias)
        # the residual: random; for a structured (large) row a random block repeated with an odd period of its own
        self.res = None
        if r.residual:
            self.res = ci.rnd(rng, (r.rows, r.cols)) if not self.structured else np.take(ci.rnd(rng, (251, r.cols)), np.arange(r.rows) % 251, axis=0)
        self._cache = {}
        if r.conv:
            self._conv_operand()
        else:
            self._gemm_operand()

    # -- the activation operand
    def _gemm_operand(self):
        r, rng = self.r, self.rng
        if r.ln:      # rows with a large common offset (the single-pass variance cancels), as ln_entry
            self.a = (ci.rnd(rng, (r.rows, r.K), 1.5).astype(f32) + rng.standard_normal((r.rows, 1), dtype=f32) * 3.0).astype(f16)
        elif not self.structured:
            self.a = ci.rnd(rng, (r.rows, r.K))
        else:
            self.P = PRIMES[r.line % len(PRIMES)]
            self.mcols = marker_columns(self.route.ktiles, self.route.route[2])
            self.block = ci.rnd(rng, (self.P, r.K))
            self.block[:, [c for c, _ in self.mcols]] = 0
            i = np.arange(r.rows)
            self.a = np.take(self.block, i % self.P, axis=0)
            mk = markers(i)
            for c, j in self.mcols:
                self.a[:, c] = mk[j].astype(f16)

    def _conv_operand(self):
        r, rng = self.r, self.rng
        if not self.structured:
            self.x = ci.rnd(rng, (r.images, r.H, r.W, r.Cin))
            return
        self.Ph, self.Pw = CONV_PERIODS[r.line % len(CONV_PERIODS)]
        self.mch = (7 * r.line + 3) % r.Cin
        self.T = ci.rnd(rng, (self.Ph, self.Pw, r.Cin))
        self.T[:, :, self.mch] = 0
        self.x = np.empty((r.images, r.H, r.W, r.Cin), f16)
        self.x[:] = self.T[np.arange(r.H)[:, None] % self.Ph, np.arange(r.W)[None, :] % self.Pw][None]
        n, h, w = np.meshgrid(np.arange(r.images), np.arange(r.H), np.arange(r.W), indexing="ij")
        self.x[..., self.mch] = self._pixel_marker(n, h, w).astype(f16)

    def _pixel_marker(self, n, h, w):
        return ((h * 31 + w * 7 + n * 13) & 63).astype(f64) / 32.0

    # -- the weight as the float64 [columns, K] matrix the products use, and its scale
    def _wmat(self, n0, n1):
        w = self.w[n0:n1].reshape(n1 - n0, -1)
        if not self.r.w8:
            return w.astype(f64), None
        if self.vecs is None:
            return w.astype(f64) - self.zp, self.scale
        return w.astype(f64) - self.vecs[1][n0:n1, None].astype(f64), self.vecs[0][n0:n1].astype(f64)

    def chunks(self):
        """(r0, r1, n0, n1) blocks of the output in its PHYSICAL columns (GEGLU: whole rows, the pairs sit apart), no float64 array of more than CHUNK elements"""
        r = self.r
        nc = r.N if (r.act == ACT_GEGLU or r.ln) else max(32, min(r.N, CHUNK // r.K // 32 * 32))
        rc = max(1, min(r.rows, CHUNK // max(r.K if not self.structured else 1, nc)))
        return [(r0, min(r0 + rc, r.rows), n0, min(n0 + nc, r.N)) for n0 in range(0, r.N, nc) for r0 in range(0, r.rows, rc)]

    def _im2col(self):
        if "cols" not in self._cache:
            self._cache["cols"] = ci.im2col(self.x, self.r.k, self.r.stride, self.r.pad)[0]
        return self._cache["cols"]

    def _products(self, r0, r1, n0, n1):
        """pre = a . b^T and S = |a| . |b|^T of the block, float64"""
        r = self.r
        b, _ = self._wmat(n0, n1)
        if not self.structured:
            a = (self._im2col() if r.conv else self.a)[r0:r1].astype(f64)
            return a @ b.T, np.abs(a) @ np.abs(b).T
        if not r.conv:
            key = ("block", n0, n1)
            if key not in self._cache:
                self._cache = {k: v for k, v in self._cache.items() if k[0] != "block"}
                blk = self.block.astype(f64)
                self._cache[key] = (blk @ b.T, np.abs(blk) @ np.abs(b).T)
            bp, bs = self._cache[key]
            i = np.arange(r0, r1)
            pre, S = bp[i % self.P], bs[i % self.P]
            mk = markers(i)
            mk, bc = np.stack([mk[j] for _, j in self.mcols], axis=1), b[:, [c for c, _ in self.mcols]]      # the rank-one terms as one small product
            return pre + mk @ bc.T, S + mk @ np.abs(bc).T
        return self._conv_structured(r0, r1, n0, n1, b)

    def _conv_structured(self, r0, r1, n0, n1, b):
        r, k, s, pad, C = self.r, self.r.k, self.r.stride, self.r.pad, self.r.Cin
        key = ("torus", n0, n1)
        if key not in self._cache:
            self._cache = {kk: v for kk, v in self._cache.items() if kk[0] != "torus"}
            # the torus convolution of one period: the window's top-left input pixel at (p, q), taps wrapping round
            T = self.T.astype(f64)
            taps = [np.roll(T, (-i, -j), axis=(0, 1)).reshape(self.Ph * self.Pw, C) for i in range(k) for j in range(k)]
            cols = np.concatenate(taps, axis=1)
            self._cache[key] = (cols @ b.T, np.abs(cols) @ np.abs(b).T)
        tp, ts = self._cache[key]
        i = np.arange(r0, r1)
        n, ho, wo = i // (r.Ho * r.Wo), i // r.Wo % r.Ho, i % r.Wo
        h0, w0 = ho * s - pad, wo * s - pad
        t = (h0 % self.Ph) * self.Pw + w0 % self.Pw
        pre, S = tp[t], ts[t]
        # the markers: a single-channel k x k sum
        bm = b.reshape(n1 - n0, k * k, C)[..., self.mch]
        v = np.empty((i.size, k * k))
        for di in range(k):
            for dj in range(k):
                hh, ww = h0 + di, w0 + dj
                v[:, di * k + dj] = np.where((hh >= 0) & (hh < r.H) & (ww >= 0) & (ww < r.W), self._pixel_marker(n, hh, ww), 0.0)
        pre += v @ bm.T
        S += v @ np.abs(bm).T
        # the pixels whose window touches the padding: their own patches, directly
        edge = np.flatnonzero((h0 < 0) | (w0 < 0) | (h0 + k > r.H) | (w0 + k > r.W))
        if edge.size:
            patch = np.zeros((edge.size, k, k, C), f64)
            for di in range(k):
                for dj in range(k):
                    hh, ww = h0[edge] + di, w0[edge] + dj
                    ok = (hh >= 0) & (hh < r.H) & (ww >= 0) & (ww < r.W)
                    patch[ok, di, dj] = self.x[n[edge][ok], hh[ok], ww[ok]]
            patch = patch.reshape(edge.size, k * k * C)
            pre[edge], S[edge] = patch @ b.T, np.abs(patch) @ np.abs(b).T
        return pre, S

    def reference(self, r0, r1, n0, n1):
        """(want, E, c0, c1): the float64 result and f32-error bound of output rows r0 .. r1, and the OUTPUT columns c0 .. c1 the block covers"""
        r = self.r
        res = self.res[r0:r1] if self.res is not None else None
        if r.ln:
            pre, E = ci.ln_reference(self.a[r0:r1], *self.folded, 1e-5, res)
        else:
            _, scale = self._wmat(n0, n1)
            rb = self.ib[np.arange(r0, r1) // (r.Ho * r.Wo), n0:n1] if self.ib is not None else None
            pre, E = ci.epilogue(*self._products(r0, r1, n0, n1), r.K, self.bias[n0:n1], res[:, n0:n1] if res is not None else None, rb, scale)
        if r.act == ACT_GEGLU:
            pre, E = ci.geglu_logical(pre), ci.geglu_logical(E)
            return (*ci.act_apply(pre, E, ACT_GEGLU), 0, r.cols)
        return (*ci.act_apply(pre, E, r.act), n0, n1)

    # -- the comparison of a whole output
    def compare(self, got):
        """every element of got against the reference: (worst |got - want| / bound, share of elements more than one f16 ulp off); raises as ci.check does"""
        r = self.r
        assert got.shape == (r.rows, r.cols), (got.shape, r.rows, r.cols)
        def block(blk):
            r0, r1, n0, n1 = blk
            want, E, c0, c1 = self.reference(r0, r1, n0, n1)
            g = got[r0:r1, c0:c1]
            bound = ci.bound_of(want, E)
            ratio = np.abs(g.astype(f64) - want) / bound
            first = None
            if ratio.max() > 1.0:
                i = tuple(np.argwhere(ratio > 1.0)[0])
                first = f"first at {(r0 + i[0], c0 + i[1])}: got {float(g[i])!r} want {want[i]!r} bound {bound[i]!r}"
            return float(ratio.max()), int((ci.ulps_off(g, want) > 1).sum()), first

        # the blocks of one column range share the products of the block / the period (formed by the first of them); the rest on a few threads (numpy
        # releases the lock in its loops)
        blocks, out = self.chunks(), []
        with ThreadPoolExecutor(THREADS) as pool:
            for cr in sorted({b[2:] for b in blocks}):
                mine = [b for b in blocks if b[2:] == cr]
                out.append(block(mine[0]))
                out += list(pool.map(block, mine[1:]))
        worst, far = max(o[0] for o in out), sum(o[1] for o in out) / got.size
        first = next((o[2] for o in out if o[2]), None)
        assert worst <= 1.0, f"{r.id}: elements outside the bound, worst {worst:.3f} x the bound; {first}"
        assert far <= ci.FAR, f"{r.id}: {far:.4f} of the elements more than one f16 ulp from the correctly rounded result"
        return worst, far

    # -- the launch
    def launch(self, gpu):
        """the row's call through the public entry point: (output, osg_last_route)"""
        r = self.r
        if r.op == "gemm":
            return ci.gemm(gpu, self.a.reshape(r.batch, r.M, r.K) if r.batch > 1 else self.a, self.w, self.bias, self.res, r.act, r.batch)
        if r.op == "gemm_w8":
            return ci.gemm_w8(gpu, self.a, self.w, self.scale, self.zp, self.vecs, self.bias, self.res, r.act)
        if r.op == "gemm_rowstats":
            got, rs, route = ci.gemm_rowstats(gpu, self.a, self.w, self.bias, self.res, r.act)
            ci.check_rowstats(got, rs, r.id)
            return got, route
        if r.op == "gemm_ln":
            got, route, ops = ci.gemm_ln(gpu, self.a, self.w, self.gamma, self.beta, self.bias, self.res, r.act, r.rs_in)
            assert all(np.array_equal(x, y) for x, y in zip(ops, self.folded))
            return got, route
        w8 = None
        if r.w8:
            w8 = (self.scale, self.zp, None) if self.vecs is None else (0.0, 0, self.vecs)
        return ci.conv(gpu, self.x, self.w, self.bias, self.res, self.ib, r.act, r.stride, r.pad, w8=w8)

    # -- the declared arithmetic in numpy (the host's stand-in for a kernel): f32 accumulation per k-slice, the slices added in f32, one f16 rounding
    def emulate(self, drop_tile=None, short_last=False):
        """drop_tile: that k-tile (family 1: (slab, tap) unit) contributes nothing; short_last: the last k-slice stops one k-tile early"""
        r, e = self.r, self.route
        a = (ci.im2col(self.x, r.k, r.stride, r.pad)[0] if r.conv else self.a).astype(f32)
        b, scale = (self.folded[0], None) if r.ln else self._wmat(0, r.N)
        b = b.astype(f32)
        # the columns of each unit, in the order the kernel walks them
        if r.family == 0:
            units = [np.arange(64 * t, 64 * t + 64) for t in range(r.K // 64)]
            per = -(-e.ktiles // e.route[2])
        else:
            units = [tap * r.Cin + 64 * slab + np.arange(64) for slab in range(r.Cin // 64) for tap in range(9)]
            per = 9 * -(-e.ktiles // e.route[2])
        gone = {len(units) - 1} if short_last else {drop_tile} if drop_tile is not None else set()
        acc = np.zeros((r.rows, r.N), f32)
        for s0 in range(0, len(units), per):
            cols = [units[u] for u in range(s0, min(s0 + per, len(units))) if u not in gone]
            if cols:
                cols = np.concatenate(cols)
                acc += a[:, cols] @ b[:, cols].T
        if scale is not None:
            acc *= np.asarray(scale, f32)
        if r.ln:      # the folded LayerNorm: single-pass row statistics in f32, rstd (acc - mean c1) + c2
            mean = a.sum(1, dtype=f32) / f32(r.K)
            var = np.maximum((a * a).sum(1, dtype=f32) / f32(r.K) - mean * mean, f32(0))
            acc = (f32(1) / np.sqrt(var + f32(1e-5)))[:, None] * (acc - mean[:, None] * self.folded[1]) + self.folded[2]
        else:
            acc += self.bias.astype(f32)
        if self.ib is not None:
            acc += np.repeat(self.ib, r.Ho * r.Wo, axis=0).astype(f32)
        if self.res is not None:
            acc += self.res.astype(f32)
        if r.act == ACT_SILU:
            acc = acc / (1 + np.exp(-acc))
        elif r.act == ACT_GEGLU:
            from scipy.special import erf
            p = ci.geglu_logical(acc).astype(f64)
            v, g = p[:, :r.N // 2], p[:, r.N // 2:]
            acc = v * 0.5 * g * (1 + erf(g / np.sqrt(2.0)))
        return acc.astype(f16)


def reduced(r, M=None, N=None, hw=None, images=None, **kw):
    """a copy of row r at a smaller size (the same form, K, choice): M rows / N columns for a GEMM, `images` images of hw x hw pixels for a convolution"""
    if not r.conv:
        return dataclasses.replace(r, M=M or r.M, N=N or r.N, **kw)
    hw, images = hw or r.H, images or r.images
    t = dataclasses.replace(r, H=hw, W=hw, N=N or r.N, **kw)
    return dataclasses.replace(t, M=images * t.Ho * t.Wo)


# ---- the groups the device test runs, one child process each ---------------------------------------------------------------------------------------------
GROUPS = {"sd15-unet": (1, 61), "sd15-decoder": (62, 80), "sdxl": (81, 133), "decoder-1024": (134, 143), "p4-unet": (144, 180), "p4-decoder": (181, 191),
          "w8a16": (192, 250)}


def group_rows(name):
    lo, hi = GROUPS[name]
    return [r for r in rows() if lo <= r.line <= hi]
