"""CPU: the claims of tests/conv_geometry_cases.py that tests/test_conv_geometry.py relies on, and GraphBuilder.conv's extended signature.

  * the float64 im2col reference of every case equals torch.nn.functional.conv2d in float64 behind torch.nn.functional.pad (an independent restatement: torch
    pads, strides and walks taps in its own code) to 1e-12 relative;
  * every form appears on every route that can legally take it, the forms the issue lists are all there, every near miss differs from its partner in
    exactly one parameter (the four pads count as one) and the partner chain ends at a taken case, every refusal names a geometry without an output or a
    stride of 0;
  * the 2 % cap of `check` (elements more than one f16 ulp from the correctly rounded value) holds BY CONSTRUCTION for the reference rounded to f16: that
    value IS the correctly rounded one, 0 ulps away everywhere.  So the cap is a statement about the kernel alone, and this file does not measure it on one;
  * GraphBuilder.conv writes byte-identical model.txt text for the square / symmetric calls, spelt the old way or the new."""
import numpy as np
import pytest

import conv_geometry_cases as cg
import test_contraction_instantiations as ci

f16, f32, f64 = np.float16, np.float32, np.float64
# (test_contraction_instantiations is marked gpu as a module: importing its reference functions runs nothing of it, and this module carries no mark)


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in cg.device_cases()])
def test_im2col_reference_is_torch_conv2d(c):
    import torch
    import torch.nn.functional as F
    o = cg.operands(c)
    cols, ho, wo = cg.columns(c, o)
    assert (ho, wo) == c.out_hw() and cols.shape == (c.n * ho * wo, c.K)
    mine = cols @ o["wmat"].T
    pt, pl, pb, pr = c.pads
    x = torch.from_numpy(o["x"].astype(f64)).permute(0, 3, 1, 2)                                         # NHWC -> NCHW
    w = torch.from_numpy(o["wmat"].reshape(c.cout, c.kh, c.kw, c.cin)).permute(0, 3, 1, 2)               # OHWI -> OIHW
    y = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, stride=(c.sh, c.sw))
    assert tuple(y.shape) == (c.n, c.cout, ho, wo)
    theirs = y.permute(0, 2, 3, 1).reshape(c.n * ho * wo, c.cout).numpy()
    assert np.abs(mine - theirs).max() <= 1e-12 * np.abs(theirs).max()


def test_every_form_on_every_legal_route():
    have = {(c.route, c.form) for c in cg.CASES}
    for r in cg.ROUTES:
        for f in list(cg.FORMS) + list(cg.EPILOGUES):
            assert ((r, f) in have) == cg.legal(r, f), (r, f)
    # the forms the table must hold
    geo = {(c.kh, c.kw) for c in cg.CASES if c.cls == "kernel"}
    assert geo == {(1, 3), (3, 1), (3, 5), (5, 3), (2, 4), (7, 7)}
    assert {(c.sh, c.sw) for c in cg.CASES if c.cls == "stride"} >= {(1, 2), (2, 1), (3, 2)}
    assert any((c.h + c.pads[0] + c.pads[2] - c.kh) % c.sh for c in cg.CASES if c.cls == "stride")
    pads = {(c.pads, (c.sh, c.sw)) for c in cg.CASES if c.cls == "pad"}
    assert pads >= {((0, 0, 1, 1), (2, 2)), ((1, 1, 0, 0), (1, 1)), ((2, 0, 0, 1), (1, 1)), ((1, 2, 0, 3), (1, 1))}
    assert any(c.pads[0] == c.kh for c in cg.CASES if c.cls == "pad")
    for c in cg.device_cases():
        assert c.h <= 20 and c.w <= 20 or c.route == "halo", c.name       # (the halo kernel's widths are 8 .. 64 by definition)
        assert c.cin <= 128 and c.cout <= 96 and min(c.pads) >= 0, c.name
        if c.route in cg.ROUTES:
            assert c.h != c.w and c.h % 2 and c.w % 2, c.name
            spec = cg.ROUTES[c.route]
            assert (c.cin == 4 and (c.kh, c.kw) == (3, 3) and c.cout % 16 == 0) if c.route == "a" else (c.cin % 64 == 0) if spec["family"] == cg.GEMM2 else \
                (c.cin % 8 == 0 and c.cin % 64) if c.route == "e" else c.cin % 8 != 0, c.name
            if c.route in ("e", "f"):
                assert c.cout % 4, c.name
            if spec["knobs"].get("OSG_GEMM_SPLITS", 1) == 3:
                assert ci.slices(c.K // 64, 3) == 3, c.name
    # three images whose pixel count per image is a multiple of no tile height: a row tile spans images
    for c in cg.CASES:
        if c.form == "n3" or c.cls == "epilogue":
            ho, wo = c.out_hw()
            assert c.n == 3 and all((ho * wo) % t for t in cg.TILE_HEIGHTS), c.name
        if c.cls == "epilogue":
            assert c.sh != c.sw and len(set(c.pads)) > 1, c.name
    # the one shape of the element-wise gather that splits K: few tiles, K >= 1024
    c = cg.by_name("f/k7x7")
    assert c.K >= 1024 and c.K // 256 > 1 and c.cin % 8


def test_near_misses_differ_in_one_parameter():
    near = [c for c in cg.CASES if c.cls == "near"]
    taken = [c for c in near if c.partner is None]
    assert {(c.route, c.family) for c in taken} == {("halo", cg.CONV3X3), ("one", cg.GEMM2)} and len(taken) == 5
    for c in near:
        if c.partner is None:
            continue
        p = cg.by_name(c.partner)
        d = c.differs(p)
        assert len(d) == 1, (c.name, c.partner, d)
        hops = 0
        while p.partner is not None and p.cls == "near":
            p, hops = cg.by_name(p.partner), hops + 1
        assert hops <= 1, c.name
        # the chain ends at a case its kernel takes: the halo kernel's, the plain GEMM's, or the Cin = 4 kernel's own stride form
        assert (p.cls == "near" and p.form == "taken") or (c.route == "cin4" and p.route == "a"), c.name
    halo = {c.w for c in taken if c.route == "halo"}
    assert halo == {8, 16, 32, 64}
    for w in halo:
        forms = {(c.kh, c.kw, c.sh, c.sw, c.pads) for c in near if c.route == "halo" and c.w == w and c.partner}
        assert forms >= {(3, 3, 1, 1, (0, 0, 2, 2)), (3, 3, 1, 1, (2, 2, 0, 0)), (3, 1, 1, 1, (1, 0, 1, 0)), (3, 5, 1, 1, (1, 2, 1, 2)), (3, 3, 1, 2, (1, 1, 1, 1))}
    for c in near:
        if c.route == "halo" and c.pads in ((0, 0, 2, 2), (2, 2, 0, 0), (1, 0, 1, 0), (1, 2, 1, 2)):
            assert c.out_hw() == (c.h, c.w), c.name            # the near misses that keep Ho == H, Wo == W
    ones = {(c.sh, c.sw, c.pads) for c in near if c.route == "one" and c.partner}
    assert ones == {(1, 2, (0, 0, 0, 0)), (2, 2, (0, 0, 0, 0)), (1, 1, (1, 1, 1, 1)), (1, 1, (0, 1, 0, 0))}


def test_refusals_have_no_output():
    for c in cg.refusals():
        pt, pl, pb, pr = c.pads
        assert c.sh == 0 or c.sw == 0 or c.h + pt + pb < c.kh or c.w + pl + pr < c.kw, c.name
    assert any(c.sh > 1 and c.h + c.pads[0] + c.pads[2] < c.kh for c in cg.refusals())      # (a negative extent that C's division truncates to 0)


@pytest.mark.parametrize("route", list(cg.ROUTES))
def test_far_cap_holds_for_the_rounded_reference(route):
    """by construction: the reference rounded to f16 is 0 ulps from the correctly rounded reference, and inside the bound (2^-11 |want| covers the rounding)"""
    c = cg.by_name(f"{route}/e_f32_ib_silu")
    o = cg.operands(c)
    cols, ho, wo = cg.columns(c, o)
    pre, E = ci.contraction(cols, o["wmat"], o["bias"], o["res"], np.repeat(o["ib"], ho * wo, axis=0), scale=o["scale"])
    want, E = ci.act_apply(pre, E, c.epi["act"])
    assert not ci.ulps_off(want.astype(f16), want).any()
    ci.check(want.astype(f16), want, E, c.name)


@pytest.mark.parametrize("route", list(cg.ROUTES))
def test_a_padding_tap_read_as_data_leaves_the_bound(route):
    """why the activations carry a mean: with the border pixel standing where a pad belongs (a clamped index for a bounds check) the border outputs leave the
    bound by far -- the check on the device can see one such tap"""
    c = cg.by_name(f"{route}/p2001")
    o = cg.operands(c)
    cols, ho, wo = cg.columns(c, o)
    want, E = ci.contraction(cols, o["wmat"], o["bias"], scale=o["scale"])
    pt, pl, pb, pr = c.pads
    clamped = np.pad(o["x"].astype(f64), ((0, 0), (pt, pb), (pl, pr), (0, 0)), mode="edge")
    wrong, _ = ci.contraction(cg.im2col(clamped, c.kh, c.kw, c.sh, c.sw, 0, 0, 0, 0)[0], o["wmat"], o["bias"], scale=o["scale"])
    border = np.zeros((c.n, ho, wo), bool)
    border[:, :pt], border[:, :, wo - pr:] = True, True
    off = (np.abs(wrong - want) > 8 * ci.bound_of(want, E)).reshape(c.n, ho, wo, c.cout)
    assert off[border].mean() > 0.9 and not off[~border & ~np.roll(border, 1, 1) & ~np.roll(border, -1, 2)].any()


def test_graphbuilder_conv_square_calls_write_the_same_text():
    """the scalar spelling of GraphBuilder.conv and the (kh, kw) / (sh, sw) / four-pad spelling write the same model.txt and the same weight files, and the golden
    case conv3x3_stride2 still writes the text and the weights tests/golden/conv3x3_stride2.npz was recorded from"""
    import hashlib

    import golden_cases
    from onnxstream_amd.synth.graph import GraphBuilder, MemSink

    def emit(fn, shape=None):
        sink = MemSink()
        g = GraphBuilder(sink)
        fn(g, g.input("x", shape)) if shape else fn(g)
        return g.finish(), sink

    def files(sink):
        return {k: v if isinstance(v, str) else np.asarray(v).tobytes() for k, v in sink.files.items()}

    for shape, old, new, attrs in [
            ((1, 64, 12, 12), lambda g, x: g.conv("/c", x, 64, 3, stride=2, pad=1), lambda g, x: g.conv("/c", x, 64, (3, 3), stride=(2, 2), pad=(1, 1, 1, 1)),
             "dilations:1,1;group:1;kernel_shape:3,3;pads:1,1,1,1;strides:2,2"),
            ((1, 64, 8, 8), lambda g, x: g.conv("/c", x, 32, 1, bias=False), lambda g, x: g.conv("/c", x, 32, (1, 1), stride=(1, 1), pad=(0, 0, 0, 0), bias=False),
             "dilations:1,1;group:1;kernel_shape:1,1;pads:0,0,0,0;strides:1,1"),
            ((1, 8, 5, 7), lambda g, x: g.conv("/c", x, 16, 5), lambda g, x: g.conv("/c", x, 16, (5, 5), pad=(2, 2, 2, 2)),
             "dilations:1,1;group:1;kernel_shape:5,5;pads:2,2,2,2;strides:1,1")]:
        (t_old, s_old), (t_new, s_new) = emit(old, shape), emit(new, shape)
        assert t_old == t_new
        assert t_old.rstrip("\n").endswith("*" + attrs), t_old
        assert files(s_old) == files(s_new)
    # the golden case as it was written before the signature grew (text, and a digest of each weight file)
    txt, sink = emit(golden_cases.conv3x3_stride2)
    assert txt == ("/c:Conv*input:x(1,64,12,12);_2F_c_2E_weight_nchw.bin(float16:64,64,3,3);_2F_c_2E_bias.bin(float16:64)*output:_2F_c_5F_out0_1(1,64,6,6)"
                   "*dilations:1,1;group:1;kernel_shape:3,3;pads:1,1,1,1;strides:2,2\n"), txt
    digest = {k: hashlib.sha256(v).hexdigest()[:16] for k, v in files(sink).items() if k != "model.txt"}
    assert digest == {"_2F_c_2E_bias.bin": "81317a71bee11dea", "_2F_c_2E_weight_nhwc.bin": "8faa4438fdadedc7"}, digest
    # and the new forms name what they were given, with the output shape ONNX derives from the pads as given
    txt, _ = emit(lambda g, x: g.conv("/c", x, 16, (3, 5), stride=(2, 1), pad=(0, 1, 1, 2)), (1, 8, 6, 7))
    assert txt.rstrip("\n").endswith("(1,16,3,6)*dilations:1,1;group:1;kernel_shape:3,5;pads:0,1,1,2;strides:2,1"), txt
