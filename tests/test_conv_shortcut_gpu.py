"""-m gpu: the halo-reuse 3x3 convolution with a second K segment (osg_conv2d_nhwc_cat, osg_conv3x3_cat.hip) against float64, and the plans that
use it (option hip_fuse_shortcut) against the reference.

* The kernel entry: out = f16(conv3x3(x, W) + x2 . W2^T + bias) with bias the f32 sum of two f16 bias vectors.  Reference, bound and the FAR cap are those of
  tests/test_contraction_instantiations.py (contraction / epilogue / check / im2col), with K = 9 Cin + Cin2 and one more bias term: the sum of the two biases
  is rounded once more on the host.  Outputs lie between guard bands (Out).
* Shapes: the smallest at which each path can still go wrong -- one image per width (two 8 x 8 images at W = 8: one tile), Cin in {64, 128} (one / two slabs),
  Cin2 in {64, 192} (one / three k-tiles: the three-tile case fills the ring's prologue short of its depth, the split cases wrap the slices), Cout in {80, 96}
  (96: a partial last n-tile at every tile width).  Every instantiation runs 1, 2 and 3 k-slices: with one slab and three k-tiles, 2 slices are (the slab | the
  k-tiles) and 3 slices are (nothing | the slab | the k-tiles).  A split ends in the reduce launch; the in-kernel fold is asked for as well and must not be taken
  (this kernel does not offer it: DESIGN.md 4.2.1).  Cin2 = 448 (seven k-tiles) wraps the ring on the read side at every tile width.
* The plans: the miniature UNets with the option on through the legs of tests/parity.py against the reference goldens, and the full-size SD 1.5 UNet with the
  key and pinned references of tests/test_fullsize.py."""
import os
import shutil
import subprocess
import tempfile
from functools import lru_cache

import numpy as np
import pytest

import parity
from test_contraction_instantiations import (ACT_NONE, ACT_SILU, Out, act_apply, check, dev, epilogue, im2col, knobs, ptr, reduce_kernel, rnd)

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64
CAT = 4                       # osg_last_route family
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@lru_cache(maxsize=None)
def cat_entries():
    """the entry list of osg_conv3x3_cat.hip, in its order, as (image width, output channels per tile, loader waves): read from osg_conv3x3_cat_plan.h through
    tools/conv_cat_plan_check.cpp, the way tests/test_contraction_instantiations.py reads the other tables"""
    d = tempfile.mkdtemp(prefix="osg_cat_")
    try:
        exe = os.path.join(d, "entries")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"), os.path.join(REPO, "tools", "conv_cat_plan_check.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe, "entries"], stdout=subprocess.PIPE, text=True, check=True).stdout
        return [(int(f[0]), int(f[1]), int(f[4])) for f in (ln.split() for ln in out.splitlines())]
    finally:
        shutil.rmtree(d, ignore_errors=True)


IMAGES = {64: (1, 64), 32: (1, 32), 16: (1, 16), 8: (2, 8)}      # (images, rows) per width


def cat_slices(cin, cin2, asked):
    total = 9 * (cin // 64) + cin2 // 64
    q = -(-total // asked)
    return -(-total // q)


class Case:
    """operands of one fused launch and its float64 reference"""

    def __init__(self, rng, n, h, w, cin, cin2, cout, act=ACT_NONE, biases=True):
        self.n, self.h, self.w, self.cin, self.cin2, self.cout, self.act = n, h, w, cin, cin2, cout, act
        K = 9 * cin + cin2
        self.x, self.x2 = rnd(rng, (n, h, w, cin)), rnd(rng, (n, h, w, cin2))
        self.wt, self.w2 = rnd(rng, (cout, 3, 3, cin), K ** -0.5), rnd(rng, (cout, cin2), K ** -0.5)
        self.b, self.bs = rnd(rng, (cout,), 0.1), rnd(rng, (cout,), 0.1)
        self.bias32 = self.b.astype(f32) + self.bs.astype(f32)          # what the planner hands over: the two biases added in f32 on the host
        cols, _, _ = im2col(self.x, 3, 1, 1)
        a = np.concatenate([cols, self.x2.reshape(-1, cin2).astype(f64)], axis=1)
        bm = np.concatenate([self.wt.reshape(cout, -1), self.w2], axis=1).astype(f64)
        bs64 = self.bs.astype(f64)
        # (K + 3) terms of the plain launch, one more for the second bias: its absolute value joins S, the rounding of the host's sum the count
        pre, E = epilogue(a @ bm.T + bs64, np.abs(a) @ np.abs(bm).T + np.abs(bs64), K + 1, self.b)
        if not biases:                                                  # neither convolution has a bias: the launch takes a NULL bias operand
            self.bias32 = None
            pre, E = epilogue(a @ bm.T, np.abs(a) @ np.abs(bm).T, K)
        self.want, self.E = act_apply(pre, E, act)
        for v in (self.want, self.E):
            v.setflags(write=False)

    def run(self, gpu, ld=None, col=0, second=False):
        m = self.n * self.h * self.w
        out = Out(gpu, m, self.cout, ld=ld, col=col)
        out2 = Out(gpu, m, self.cout) if second else None
        dx, dw, dx2, dw2, db = keep = dev(gpu, self.x, self.wt, self.x2, self.w2, self.bias32)
        gpu._ck(gpu.lib.osg_conv2d_nhwc_cat(gpu.ctx, dx.ptr, dw.ptr, dx2.ptr, dw2.ptr, self.cin2, ptr(db), out.ptr, ld or 0, out2.ptr if second else None,
                                            self.cout if second else 0, self.n, self.h, self.w, self.cin, self.cout, self.act))
        got = out.read()
        got2 = out2.read() if second else None
        del keep
        return got, got2, gpu.last_route()


def entry_params():
    return [pytest.param(i, id=f"cat-w{w:02d}-{bn:03d}-nl{nl}") for i, (w, bn, nl) in enumerate(cat_entries())]


def test_entry_list_is_the_one_this_file_walks(gpu):
    assert gpu.lib.osg_conv3x3_cat_entries() == len(cat_entries()) == 22


@pytest.mark.parametrize("idx", entry_params())
def test_cat_instantiation(gpu, idx, monkeypatch):
    w, bn, nl = cat_entries()[idx]
    n, h = IMAGES[w]
    rng = np.random.default_rng(15485863 * (idx + 1))
    # one slab + three k-tiles, a partial last n-tile: 1 / 2 / 3 slices.  A split is always finished by the reduce launch: a request for the in-kernel fold is not
    # honoured (osg_conv3x3_cat_launch says why), which the route shows
    c = Case(rng, n, h, w, 64, 192, 96)
    for s, fold in ((1, 0), (2, 0), (3, 0), (2, 1), (3, 1)):
        knobs(monkeypatch, OSG_CONV3X3_BN=bn, OSG_CONV3X3_NL=nl, OSG_CONV3X3_SPLITS=s, OSG_CONV3X3_FOLD=fold)
        got, _, r = c.run(gpu)
        check(got, c.want, c.E, f"Cin 64, Cin2 192, Cout 96: {s} k-slices, fold asked {fold}")
        sl = cat_slices(64, 192, s)
        assert sl == s and r == (CAT, idx, sl, 0, reduce_kernel(sl, 0, 96)), r
    # two slabs + one k-tile, whole n-tiles of 80, SiLU: 1 slice, and 2 slices of which the second holds a slab AND the k-tile
    c = Case(rng, n, h, w, 128, 64, 80, ACT_SILU)
    for s in (1, 2):
        knobs(monkeypatch, OSG_CONV3X3_BN=bn, OSG_CONV3X3_NL=nl, OSG_CONV3X3_SPLITS=s)
        got, _, r = c.run(gpu)
        check(got, c.want, c.E, f"Cin 128, Cin2 64, Cout 80, SiLU: {s} k-slices")
        assert r == (CAT, idx, s, 0, reduce_kernel(s, 0, 80)), r


@pytest.mark.parametrize("w,bn,nl", [(8, 80, 4), (8, 128, 4), (8, 160, 4), (16, 128, 8), (16, 160, 8)])
def test_ring_wraps_on_the_read_side(gpu, w, bn, nl, monkeypatch):
    """Cin2 = 448: seven k-tiles, two more than the deepest ring (5 stages at 80 / 128 columns, 4 at 160) -- the math waves' stage index wraps and the loaders'
    counted wait runs past one lap, in one slice and in a slice that holds k-tiles only"""
    n, h = IMAGES[w]
    rng = np.random.default_rng(977 * w + bn + nl)
    c = Case(rng, n, h, w, 64, 448, 96)
    for s in (1, 2):
        knobs(monkeypatch, OSG_CONV3X3_BN=bn, OSG_CONV3X3_NL=nl, OSG_CONV3X3_SPLITS=s)
        got, _, r = c.run(gpu)
        check(got, c.want, c.E, f"Cin2 448, {s} k-slices")
        assert r == (CAT, cat_entries().index((w, bn, nl)), s, 0, reduce_kernel(s, 0, 96)), r


def test_no_bias_operand(gpu, monkeypatch):
    knobs(monkeypatch)
    c = Case(np.random.default_rng(31), 2, 8, 8, 64, 128, 80, biases=False)
    got, _, r = c.run(gpu)
    check(got, c.want, c.E, "no bias")
    assert r[0] == CAT, r


def test_two_m_tiles_at_width_8_views_and_a_second_destination(gpu, monkeypatch):
    """four 8 x 8 images = two m-tiles; the output as a column view of a wider buffer (ldc > N: a `>concat` slot), then with a second dense destination"""
    rng = np.random.default_rng(4242)
    c = Case(rng, 4, 8, 8, 128, 192, 96)
    for s, fold in ((1, 0), (3, 0), (2, 1)):
        knobs(monkeypatch, OSG_CONV3X3_BN=80, OSG_CONV3X3_NL=4, OSG_CONV3X3_SPLITS=s, OSG_CONV3X3_FOLD=fold)
        got, _, r = c.run(gpu)
        check(got, c.want, c.E, f"two m-tiles, {s} k-slices, fold {fold}")
        assert r[0] == CAT and r[2:4] == (s, 0), r
        got, got2, r = c.run(gpu, ld=96 + 24, col=12, second=True)
        check(got, c.want, c.E, f"column view, {s} k-slices, fold {fold}")
        assert np.array_equal(got, got2)                          # the second destination receives the same f16 values
    knobs(monkeypatch, OSG_CONV3X3_BN=128, OSG_CONV3X3_NL=8, OSG_CONV3X3_SPLITS=1)
    got, _, r = c.run(gpu, ld=96 + 8, col=4)
    check(got, c.want, c.E, "column view alone")


def test_statistics_sink_against_the_unfused_pair(gpu, monkeypatch):
    """the GroupNorm-statistics sink armed: the table of the fused launch holds the sums of what IT stored, and differs from the table the un-fused pair
    (1x1 convolution, then the 3x3 one with its output as residual) fills by no more than the stored values differ"""
    knobs(monkeypatch)
    rng = np.random.default_rng(77)
    n, h, w, cout, G = 2, 16, 16, 96, 8
    c = Case(rng, n, h, w, 64, 192, cout)
    dx, dw, dx2, dw2, db32, db, dbs = dev(gpu, c.x, c.wt, c.x2, c.w2.reshape(cout, 1, 1, -1), c.bias32, c.b, c.bs)
    tabs, ys = [], []
    for fused in (True, False):
        t0 = gpu.to_dev(np.zeros((8, n, G, 2), np.int64))
        y = gpu.to_dev(np.zeros((n, h, w, cout), f16))
        if fused:
            gpu.set_stat_sinks(h * w, t0, G, cout // G, 0)
            gpu._ck(gpu.lib.osg_conv2d_nhwc_cat(gpu.ctx, dx.ptr, dw.ptr, dx2.ptr, dw2.ptr, c.cin2, db32.ptr, y.ptr, 0, None, 0, n, h, w, c.cin, cout, ACT_NONE))
        else:
            s = gpu.conv2d_nhwc(dx2, dw2, dbs, 1, (0, 0, 0, 0))
            gpu.set_stat_sinks(h * w, t0, G, cout // G, 0)
            gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, 2, dx.ptr, dw.ptr, db.ptr, 2, None, 0, s.ptr, y.ptr, 0, None, 0, n, h, w, c.cin, cout, 3, 3, 1, 1, 1, 1, 1, 1, ACT_NONE))
        ys.append(y.numpy().astype(f64).reshape(n, h * w, G, cout // G))
        tabs.append(t0.numpy().sum(0).astype(f64))
    qs = 2.0 ** min(20, max(10, 36 - int(np.ceil(np.log2(h * w * (cout // G))))))
    for y, t in zip(ys, tabs):                                     # each table is the sum of what its launch stored (the tolerances of tests/test_gpu_kernels.py)
        assert np.allclose(t[..., 0] / 2.0 ** 20, y.sum((1, 3)), rtol=1e-5, atol=2e-2)
        assert np.allclose(t[..., 1] / qs, (y * y).sum((1, 3)), rtol=1e-5, atol=2.0)
    check(ys[0].reshape(-1, cout), c.want, c.E, "fused launch with the sink armed")
    d1 = np.abs(ys[0] - ys[1]).sum((1, 3))
    d2 = np.abs(ys[0] * ys[0] - ys[1] * ys[1]).sum((1, 3))
    assert (np.abs(tabs[0][..., 0] - tabs[1][..., 0]) / 2.0 ** 20 <= d1 + 4e-2).all()
    assert (np.abs(tabs[0][..., 1] - tabs[1][..., 1]) / qs <= d2 + 4.0).all()


def test_shapes_the_entry_does_not_take_fail_with_a_clear_error(gpu, monkeypatch):
    knobs(monkeypatch)
    rng = np.random.default_rng(5)
    for n, h, w, cin, cin2 in ((1, 16, 16, 64, 96), (1, 16, 16, 96, 64), (1, 24, 24, 64, 64), (1, 6, 16, 64, 64)):
        x, x2 = rnd(rng, (n, h, w, cin)), rnd(rng, (n, h, w, cin2))
        wt, w2 = rnd(rng, (80, 3, 3, cin), 0.05), rnd(rng, (80, cin2), 0.05)
        out = Out(gpu, n * h * w, 80)
        dx, dw, dx2, dw2 = keep = dev(gpu, x, wt, x2, w2)
        rc = gpu.lib.osg_conv2d_nhwc_cat(gpu.ctx, dx.ptr, dw.ptr, dx2.ptr, dw2.ptr, cin2, None, out.ptr, 0, None, 0, n, h, w, cin, 80, ACT_NONE)
        assert rc != 0 and b"osg_conv2d_nhwc_cat" in gpu.lib.osg_last_error(gpu.ctx), (n, h, w, cin, cin2)
        del keep


# ---- the plans --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unet_tiny", "unet_tinyxl"])
def test_miniature_unets_with_the_option_on(name):
    """the option off is the default plan of tests/test_golden.py; the option on passes the same legs against the same goldens, fuses at least one pair, and stays
    within f16 noise of the option off"""
    import test_golden as tg
    ins, oname, r16, r32 = tg.load(name)
    off = tg._run_hip(name, ins, oname, 2, True)
    on = tg._run_hip(name, ins, oname, 2, True, options=(("hip_fuse_shortcut", 1),))
    assert list(on.shape) == list(r16.shape) and np.isfinite(on).all()
    tg._check_net(name, off, f"{name}@f2 (option off)", key=f"{name}@f2")
    tg._check_net(name, on, f"{name}@f2 +shortcut", key=f"{name}@f2")
    assert not np.array_equal(on, off)                             # (a pair fused: one f16 rounding fewer per fused ResNet)
    assert float(np.abs(on - off).max()) / float(np.abs(r32).max()) <= 5e-3


def test_full_size_sd15_with_the_option_on():
    import test_fullsize as tf
    from onnxstream_amd import build as b
    from onnxstream_amd.synth import sd_unet
    from onnxstream_amd.synth.graph import DirSink
    from oracle import ref as oref
    d = os.path.join(os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth"), "sd15") + "/"
    if not os.path.exists(d + ".complete"):
        os.makedirs(d, exist_ok=True)
        sd_unet.build_unet(DirSink(d), sd_unet.SD15)
        open(d + ".complete", "w").write("ok")
    a, c = sd_unet.unet_inputs(sd_unet.SD15, 42), sd_unet.unet_inputs(sd_unet.SD15, 43)
    on = tf._run(b.LIB_HOST, d, [a, c], runs=3, options=(("hip_fuse_shortcut", 1),))
    for o in on[1:]:
        assert np.array_equal(on[0][0], o[0]) and np.array_equal(on[0][1], o[1])      # eager == captured == replayed, bit for bit
    assert np.isfinite(on[0][0]).all() and np.isfinite(on[0][1]).all()
    if not oref.available():
        pytest.skip("oracle/_ref not present: reproducibility checked, reference parity skipped")
    tf._triangulated(on[0][0], d, a, "SD1.5 UNet full size", "sd15")
