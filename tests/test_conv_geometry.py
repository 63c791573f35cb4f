"""-m gpu: the convolution entry points off the diagonal -- KH != KW, stride_h != stride_w, four different pads, H != W -- on every route of conv2d_route,
element by element against float64 (the table: tests/conv_geometry_cases.py; its own claims: tests/test_conv_geometry_cpu.py).

* Reference: conv_geometry_cases.im2col (every geometry parameter on its own axis) on the f16-rounded operands, then contraction / act_apply / check of
  tests/test_contraction_instantiations.py with K = KH KW Cin: |got - want| <= 2^-11 |want| + (1 + 2^-11)(K + 3) 2^-24 S + 2^-25, at most 2 % of the elements
  more than one f16 ulp from the correctly rounded value.  No tolerance of this file's own.
* Every launch asserts with osg_last_route the family the table names (and, on family 0, the instantiation, k-slices and fold the forced request resolves to).
* Outputs lie in guarded allocations (test_contraction_instantiations.Out: 0xFF bytes, guard bands, the column gap of a view): a store outside the output fails.
* test_coverage, last, fails where a (route, form) pair of the table was not reached, and prints the worst error / bound per route.
"""
import numpy as np
import pytest

import conv_geometry_cases as cg
import test_contraction_instantiations as ci
from onnxstream_amd.osgpu import OsgError

pytestmark = pytest.mark.gpu
f16, f32, f64 = np.float16, np.float32, np.float64

REACHED = {}     # (route, form) -> the route osg_last_route reported
WORST = {}       # route -> (worst error / bound, case)


def entry_of(tile_bm, tile_bn, nst, conv, w8):
    """index in kV2Entries of the plain (KS = 1, no loader waves, no LayerNorm) instantiation"""
    v2, _, _ = ci.table()
    return next(i for i, e in enumerate(v2) if (e["bm"], e["bn"], e["nst"], e["conv"], e["wq"], e["spec"], e["ln"], e["ks"]) == (tile_bm, tile_bn, nst, int(conv), int(w8), 0, 0, 1))


def launch(gpu, c, o):
    """the case through osg_conv2d_nhwc_v / osg_conv2d_nhwc_w8_v -> (primary output, second destination or None, osg_last_route)"""
    ho, wo = c.out_hw()
    rows = c.n * ho * wo
    e = c.epi
    view, dst2 = e.get("view"), e.get("dst2")
    out = ci.Out(gpu, rows, c.cout, ld=c.cout + view[0] if view else None, col=view[1] if view else 0)
    out2 = ci.Out(gpu, rows, c.cout, ld=c.cout + dst2[0], col=dst2[1]) if dst2 else None
    dx, dw, db, dr, di = keep = ci.dev(gpu, o["x"], o["w"], o["bias"], o["res"], o["ib"])
    tail = (ci.ptr(db), ci.bias_dtype(o["bias"]), ci.ptr(di), c.cout if di is not None else 0, ci.ptr(dr), out.ptr, out.ld if view else 0,
            out2.ptr if out2 else None, out2.ld if out2 else 0, c.n, c.h, c.w, c.cin, c.cout, c.kh, c.kw, c.sh, c.sw, *c.pads, e["act"])
    if c.w8:
        gpu._ck(gpu.lib.osg_conv2d_nhwc_w8_v(gpu.ctx, dx.ptr, dw.ptr, o["scale"], o["zp"], None, None, *tail))
    else:
        gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, ci.OSG_F16, dx.ptr, dw.ptr, *tail))
    got, got2 = out.read(), out2.read() if out2 else None
    del keep
    return got, got2, gpu.last_route()


def reference(c, o):
    cols, ho, wo = cg.columns(c, o)
    assert (ho, wo) == c.out_hw()
    pre, E = ci.contraction(cols, o["wmat"], o["bias"], o["res"], np.repeat(o["ib"], ho * wo, axis=0) if o["ib"] is not None else None, scale=o["scale"])
    return ci.act_apply(pre, E, c.epi["act"])


def expected_route(c, r):
    """what osg_last_route must report for the case; None where only the family is claimed"""
    if c.family == cg.CIN4:
        return (cg.CIN4, 0, 1, 0, 0)
    if c.family == cg.GEMM2 and c.knobs:
        s = ci.slices(c.K // 64, c.knobs["OSG_GEMM_SPLITS"])
        fold = c.knobs["OSG_GEMM_FOLD"]
        red = r[4] if c.epi.get("view") else ci.reduce_kernel(s, fold, c.cout)     # (reduce_kernel names the code of a dense output)
        return (cg.GEMM2, entry_of(64, 64, 4, True, c.w8), s, fold, red)
    if c.family == cg.GEMM_V1:
        # choose_v1: 64 x 64 tiles (few of them); K >= 1024 splits into min(K / 256, 32) slices of 32-deep k-tiles
        s = ci.slices(-(-c.K // 32), min(c.K // 256, 32) if c.K >= 1024 else 1)
        return (cg.GEMM_V1, 2 | (c.cin % 8 == 0) << 2 | 1 << 3, s, 0, ci.reduce_kernel(s, 0, c.cout))
    return None


def case_params():
    return [pytest.param(c, id=c.name, marks=[ci.FOLD_TIMEOUT] if c.knobs.get("OSG_GEMM_FOLD") else []) for c in cg.device_cases()]


@pytest.mark.parametrize("c", case_params())
def test_conv_geometry(gpu, c, monkeypatch):
    ci.knobs(monkeypatch, **c.knobs)
    o = cg.operands(c)
    want, E = reference(c, o)
    got, got2, r = launch(gpu, c, o)
    # the route first: a result that is right on another kernel says nothing about this one
    assert r[0] == c.family, f"{c.name}: family {r[0]} ran (route {r}), the table names {c.family}"
    exp = expected_route(c, r)
    if exp is not None:
        assert r == exp, (c.name, r, exp)
    elif c.family == cg.GEMM2:
        v2, _, _ = ci.table()
        assert bool(v2[r[1]]["conv"]) == c.conv_entry, f"{c.name}: entry {r[1]} is {'an implicit-GEMM' if v2[r[1]]['conv'] else 'a plain GEMM'} instantiation"
    if c.route == "f" and c.form == "k7x7":
        assert r[2] > 1, r                                  # (the one shape of the register-staged kernel that splits K inside a tap)
    ratio = float((np.abs(got.astype(f64) - want) / ci.bound_of(want, E)).max())
    print(f"{c.name}: route {r}, worst error / bound {ratio:.3f}")
    if ratio > WORST.get(c.route, (0.0, ""))[0]:
        WORST[c.route] = (ratio, c.name)
    ci.check(got, want, E, c.name)
    if got2 is not None:
        assert np.array_equal(got2.view(np.uint16), got.view(np.uint16)), f"{c.name}: the second destination differs from the first"
    if c.form == "p3101_top_eq_kh":
        # pt == KH: the first output row of the image lies wholly in the padding -- the bias, bit for bit
        wo = c.out_hw()[1]
        assert np.array_equal(got[:wo].view(np.uint16), np.broadcast_to(o["bias"], (wo, c.cout)).view(np.uint16)), f"{c.name}: a padding-only output row is not the bias"
    REACHED[(c.route, c.form)] = r


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in cg.refusals()])
def test_conv_geometry_refused(gpu, c, monkeypatch):
    """the entry point's error, nothing launched: osg_last_route as the launch before left it, the output untouched"""
    ci.knobs(monkeypatch)
    taken = cg.by_name("b/n1")
    launch(gpu, taken, cg.operands(taken))
    before = gpu.last_route()
    o = cg.operands(c)
    out = ci.Out(gpu, 64, c.cout)
    dx, dw, db = keep = ci.dev(gpu, o["x"], o["w"], o["bias"])
    with pytest.raises(OsgError, match=c.error):
        gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, ci.OSG_F16, dx.ptr, dw.ptr, db.ptr, ci.OSG_F16, None, 0, None, out.ptr, 0, None, 0,
                                          c.n, c.h, c.w, c.cin, c.cout, c.kh, c.kw, c.sh, c.sw, *c.pads, cg.ACT_NONE))
    assert gpu.last_route() == before
    assert (out.buf.numpy().view(np.uint8) == 0xFF).all(), f"{c.name}: a refused call wrote to the output"
    del keep


def test_coverage():
    """fails, naming what is missing, where a (route, form) pair of the table was not reached on the device; prints the worst error / bound per route and the
    family each near miss ran on.  It reads what test_conv_geometry recorded: it has to run after it in the same process, and fails, on purpose, under a
    selection that gives it less than the whole module"""
    for route, (ratio, name) in sorted(WORST.items()):
        print(f"[route {route}] worst error / bound {ratio:.3f} ({name})")
    for c in cg.device_cases():
        if c.cls == "near" and (c.route, c.form) in REACHED:
            print(f"[near miss] {c.name}: family {REACHED[(c.route, c.form)][0]}")
    missing = [f"{r}/{f}" for r, f in cg.wanted_pairs() if (r, f) not in REACHED]
    assert not missing, "not reached: " + "; ".join(missing)
