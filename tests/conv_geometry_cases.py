"""The case table of tests/test_conv_geometry.py (device) and tests/test_conv_geometry_cpu.py (the table's own claims): the f16 / W8A16 convolution entry points
off the diagonal KH == KW, stride_h == stride_w, four equal pads -- every geometry form on every route of conv2d_route that can legally take it.

  route   how a case reaches it                                                        what runs
  a       Cin = 4, 3 x 3, Cout % 16 == 0                                               conv_cin4_mfma_kernel (family 3)
  b       Cin % 64 == 0, the 64 x 64 tile with a 4-stage ring forced, one k-slice      gemm2_kernel<CONV> (family 0)
  c-red   as b, 3 k-slices finished by the reduce launch                               gemm2_kernel<CONV> + splitk_reduce
  c-fold  as b, 3 k-slices folded by the last arriver of each tile                     gemm2_kernel<CONV>, fold
  d       as b with uint8 weight codes (osg_conv2d_nhwc_w8_v)                          gemm2_kernel<CONV, WQ>
  e       Cin % 8 == 0, Cin % 64 != 0                                                  gemm_kernel<CONV, VEC> (family 2): the 16-byte gather
  f       Cin % 8 != 0                                                                 gemm_kernel<CONV>: the element-wise gather

A form is one geometry (kernel, stride, pads, images) of a class (`kernel`, `stride`, `pad`, `images`, `epilogue`); route a takes the 3 x 3 forms only.  Images
are 13 x 9 (H != W, both odd): 117 pixels an image with 3 x 3 / stride 1 / pad 1, a multiple of no tile height (16, 32, 64, 128), so with three images a row tile
spans images.  Activations carry a mean of +0.5: a padding tap read as data, or data read as padding, moves an output by ~0.5 |w| ~ 0.5 / sqrt(K) against a
bound of ~2^-11 |want|.

Near misses (`near`) name a partner that differs in exactly one parameter -- one of N, H, W, Cin, Cout, KH, KW, sh, sw, or the four pads taken as one -- and the
family each must run on; where the issue's form differs from the taken case in two (KH = 3, KW = 1 with the pads that keep Wo == W) the table steps through the
form in between.  Refusals (`refuse`) must fail in the entry point with nothing launched.

Plain numpy: nothing here needs a device, and nothing here is read from the code under test."""
import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64
GEMM2, CONV3X3, GEMM_V1, CIN4 = 0, 1, 2, 3         # osg_last_route families
ACT_NONE, ACT_SILU = 0, 1
TILE_HEIGHTS = (16, 32, 64, 128)                    # pixel rows per block of the four kernels (the Cin = 4 kernel: 32)
V2_TILE = dict(OSG_GEMM_CFG=2, OSG_GEMM_NST=4, OSG_GEMM_KS=1, OSG_GEMM_SPEC=0)   # the 64 x 64 tile: fold-capable, three row tiles and two column tiles here

ROUTES = {
    "a": dict(cin=4, cout=48, w8=False, family=CIN4, knobs={}),
    "b": dict(cin=64, cout=72, w8=False, family=GEMM2, knobs=dict(V2_TILE, OSG_GEMM_SPLITS=1, OSG_GEMM_FOLD=0)),
    "c-red": dict(cin=64, cout=72, w8=False, family=GEMM2, knobs=dict(V2_TILE, OSG_GEMM_SPLITS=3, OSG_GEMM_FOLD=0)),
    "c-fold": dict(cin=64, cout=72, w8=False, family=GEMM2, knobs=dict(V2_TILE, OSG_GEMM_SPLITS=3, OSG_GEMM_FOLD=1)),
    "d": dict(cin=64, cout=72, w8=True, family=GEMM2, knobs=dict(V2_TILE, OSG_GEMM_SPLITS=1, OSG_GEMM_FOLD=0)),
    "e": dict(cin=24, cout=70, w8=False, family=GEMM_V1, knobs={}),
    "f": dict(cin=6, cout=70, w8=False, family=GEMM_V1, knobs={}),
}
H0, W0 = 13, 9

# form -> (class, geometry): k = (KH, KW), s = (sh, sw), p = (top, left, bottom, right), n = images; what is not named is 3 x 3, stride 1, pad 1, one image
FORMS = {
    "k1x3": ("kernel", dict(k=(1, 3), p=(0, 1, 0, 1))),
    "k3x1": ("kernel", dict(k=(3, 1), p=(1, 0, 1, 0))),
    "k3x5": ("kernel", dict(k=(3, 5), p=(1, 2, 1, 2))),
    "k5x3": ("kernel", dict(k=(5, 3), p=(2, 1, 2, 1))),
    "k2x4": ("kernel", dict(k=(2, 4), p=(0, 1, 1, 2))),
    "k7x7": ("kernel", dict(k=(7, 7), p=(3, 3, 3, 3))),
    "s1x2": ("stride", dict(s=(1, 2))),
    "s2x1": ("stride", dict(s=(2, 1))),
    "s3x2": ("stride", dict(s=(3, 2))),
    "s5x4_rows_unused": ("stride", dict(s=(5, 4))),              # (13 + 2 - 3) % 5 == 2: the last two padded rows feed no output
    "p0011_s2": ("pad", dict(p=(0, 0, 1, 1), s=(2, 2))),         # a VAE encoder's down-sampling convolution
    "p1100": ("pad", dict(p=(1, 1, 0, 0))),
    "p2001": ("pad", dict(p=(2, 0, 0, 1))),
    "p1203": ("pad", dict(p=(1, 2, 0, 3))),
    "p3101_top_eq_kh": ("pad", dict(p=(3, 1, 0, 1))),            # pt == KH: output row 0 sees padding only and equals the bias
    "n1": ("images", dict()),
    "n3": ("images", dict(n=3)),
}
# the epilogue forms, each at three images under stride (2, 1), pads (0, 0, 1, 0): Ho x Wo = 6 x 7 = 42 pixels an image
EPI_GEO = dict(n=3, s=(2, 1), p=(0, 0, 1, 0))
EPILOGUES = {
    "e_f16_ib_res": dict(bias=f16, ib=True, res=True, act=ACT_NONE),
    "e_f32_ib_silu": dict(bias=f32, ib=True, res=False, act=ACT_SILU),
    "e_view_dst2": dict(bias=f16, ib=True, res=True, act=ACT_SILU, view=(24, 12), dst2=(8, 4)),   # (pitch - Cout, first column) of the view and of the second destination
}
PLAIN_EPI = dict(bias=f16, ib=False, res=False, act=ACT_NONE)


def legal(route, form):
    """can the route take the form?  Route a is the 3 x 3 kernel; output views need Cout % 4 == 0 (routes a to d)"""
    if form in EPILOGUES:
        return form != "e_view_dst2" or ROUTES[route]["cout"] % 4 == 0
    return route != "a" or FORMS[form][1].get("k", (3, 3)) == (3, 3)


class Case:
    FIELDS = ("n", "h", "w", "cin", "cout", "kh", "kw", "sh", "sw", "pads")

    def __init__(self, name, route, form, cls, n=1, h=H0, w=W0, cin=64, cout=72, k=(3, 3), s=(1, 1), p=(1, 1, 1, 1), w8=False, knobs=None, epi=None, family=None,
                 conv_entry=None, partner=None, error=None):
        self.name, self.route, self.form, self.cls = name, route, form, cls
        self.n, self.h, self.w, self.cin, self.cout = n, h, w, cin, cout
        (self.kh, self.kw), (self.sh, self.sw), self.pads = k, s, tuple(p)
        self.w8, self.knobs, self.epi, self.family, self.conv_entry, self.partner, self.error = w8, dict(knobs or {}), dict(epi or PLAIN_EPI), family, conv_entry, partner, error

    @property
    def K(self):
        return self.kh * self.kw * self.cin

    def out_hw(self):
        pt, pl, pb, pr = self.pads
        return (self.h + pt + pb - self.kh) // self.sh + 1, (self.w + pl + pr - self.kw) // self.sw + 1

    def differs(self, other):
        return sorted(f for f in self.FIELDS if getattr(self, f) != getattr(other, f))


CASES = []


def add(*a, **kw):
    c = Case(*a, **kw)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)
    return c


def by_name(name):
    return next(c for c in CASES if c.name == name)


for _r, _spec in ROUTES.items():
    for _f, (_cls, _geo) in FORMS.items():
        if not legal(_r, _f):
            continue
        cin = _spec["cin"]
        if _spec["family"] == GEMM2 and _cls == "pad":
            cin = 128                                     # (two k-tiles a tap: the tap walk advances every other tile)
        if _r == "f" and _f == "k7x7":
            cin = 22                                      # K = 1078 on 4 tiles: choose_v1 asks for 4 k-slices, whose bounds fall inside a tap
        add(f"{_r}/{_f}", _r, _f, _cls, cin=cin, cout=_spec["cout"], w8=_spec["w8"], knobs=_spec["knobs"], family=_spec["family"], conv_entry=True, **_geo)
    for _f, _epi in EPILOGUES.items():
        if legal(_r, _f):
            add(f"{_r}/{_f}", _r, _f, "epilogue", cin=_spec["cin"], cout=_spec["cout"], w8=_spec["w8"], knobs=_spec["knobs"], family=_spec["family"], conv_entry=True,
                epi=_epi, **EPI_GEO)

# ---- near misses ---------------------------------------------------------------------------------------------------------------------------------------
# the halo-reuse kernel takes 3 x 3 / stride 1 / pads (1,1,1,1) at W in {8, 16, 32, 64} over whole 128-pixel tiles; everything one step away runs the implicit GEMM
HALO_IMAGES = {8: (2, 8), 16: (1, 8), 32: (1, 4), 64: (1, 2)}       # W -> (images, H)
for _w, (_n, _h) in HALO_IMAGES.items():
    g = dict(n=_n, h=_h, w=_w, cin=64, cout=24)
    t = f"near/halo_w{_w}"
    add(t, "halo", "taken", "near", family=CONV3X3, **g)
    add(t + "/p0022", "halo", "p0022", "near", p=(0, 0, 2, 2), family=GEMM2, conv_entry=True, partner=t, **g)
    add(t + "/p2200", "halo", "p2200", "near", p=(2, 2, 0, 0), family=GEMM2, conv_entry=True, partner=t, **g)
    add(t + "/s1x2", "halo", "s1x2", "near", s=(1, 2), family=GEMM2, conv_entry=True, partner=t, **g)
    add(t + "/k3x1", "halo", "k3x1", "near", k=(3, 1), family=GEMM2, conv_entry=True, partner=t, **g)
    add(t + "/k3x1_p1010", "halo", "k3x1_p1010", "near", k=(3, 1), p=(1, 0, 1, 0), family=GEMM2, conv_entry=True, partner=t + "/k3x1", **g)   # Ho == H, Wo == W again
    add(t + "/k3x5", "halo", "k3x5", "near", k=(3, 5), family=GEMM2, conv_entry=True, partner=t, **g)
    add(t + "/k3x5_p1212", "halo", "k3x5_p1212", "near", k=(3, 5), p=(1, 2, 1, 2), family=GEMM2, conv_entry=True, partner=t + "/k3x5", **g)
# 1 x 1 is the plain GEMM over the pixels only at stride 1 without pads
g = dict(cin=64, cout=72, k=(1, 1))
add("near/one", "one", "taken", "near", p=(0, 0, 0, 0), family=GEMM2, conv_entry=False, **g)
add("near/one/s1x2", "one", "s1x2", "near", p=(0, 0, 0, 0), s=(1, 2), family=GEMM2, conv_entry=True, partner="near/one", **g)
add("near/one/s2x2", "one", "s2x2", "near", p=(0, 0, 0, 0), s=(2, 2), family=GEMM2, conv_entry=True, partner="near/one/s1x2", **g)
add("near/one/p1111", "one", "p1111", "near", p=(1, 1, 1, 1), family=GEMM2, conv_entry=True, partner="near/one", **g)
add("near/one/p0100", "one", "p0100", "near", p=(0, 1, 0, 0), family=GEMM2, conv_entry=True, partner="near/one", **g)
# Cin = 4, 3 x 3 stays on its kernel whatever the stride and the pads
add("near/cin4/s2x1_p0110", "cin4", "s2x1_p0110", "near", cin=4, cout=48, s=(2, 1), p=(0, 1, 1, 0), family=CIN4, partner="a/s2x1")

# ---- refusals: (the entry point's message) ---------------------------------------------------------------------------------------------------------------
add("refuse/kh_gt_padded_h", "refuse", "kh", "refuse", h=5, k=(8, 3), error="empty output")                           # 5 + 2 < 8
add("refuse/kh_gt_padded_h_s2", "refuse", "kh_s2", "refuse", h=5, k=(8, 3), s=(2, 1), error="empty output")           # (5 + 2 - 8) / 2 truncates to 0 in C
add("refuse/kw_gt_padded_w_s3", "refuse", "kw_s3", "refuse", w=3, k=(3, 7), s=(1, 3), error="empty output")
add("refuse/stride_h_0", "refuse", "sh0", "refuse", s=(0, 1), error="invalid argument")
add("refuse/stride_w_0", "refuse", "sw0", "refuse", s=(1, 0), error="invalid argument")


def device_cases():
    return [c for c in CASES if c.cls != "refuse"]


def refusals():
    return [c for c in CASES if c.cls == "refuse"]


def wanted_pairs():
    """the (route, form) pairs test_coverage wants reached on the device"""
    return [(c.route, c.form) for c in device_cases()]


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 1000003


def im2col(x, KH, KW, sh, sw, pt, pl, pb, pr):
    """NHWC x -> [n ho wo, (kh, kw, cin)] rows in float64 (the OHWI weight's K order), ho, wo: every geometry parameter on its own axis"""
    n, h, w, c = x.shape
    ho, wo = (h + pt + pb - KH) // sh + 1, (w + pl + pr - KW) // sw + 1
    xp = np.zeros((n, h + pt + pb, w + pl + pr, c), f64)
    xp[:, pt:pt + h, pl:pl + w] = x
    taps = [xp[:, i:i + sh * (ho - 1) + 1:sh, j:j + sw * (wo - 1) + 1:sw, :] for i in range(KH) for j in range(KW)]
    return np.concatenate(taps, axis=-1).reshape(n * ho * wo, KH * KW * c), ho, wo


def operands(c):
    """the f16-rounded operands of a case, seeded by its name: x [n, h, w, cin] (mean +0.5), the OHWI weight `w` (f16 values, or uint8 codes with `scale` and
    `zp`), `wmat` the exact [Cout, K] float64 weight matrix before the scale, and the epilogue operands the case's form names (None otherwise)"""
    rng = np.random.default_rng(_seed(c.name))
    x = (rng.standard_normal((c.n, c.h, c.w, c.cin), dtype=f32) + f32(0.5)).astype(f16)
    shape = (c.cout, c.kh, c.kw, c.cin)
    o = dict(x=x, scale=None, zp=None)
    if c.w8:
        o["w"] = rng.integers(0, 256, shape, dtype=np.uint8)
        o["zp"] = 128 + int(rng.integers(-8, 9))
        o["scale"] = float(f32(2.0 / np.sqrt(c.K) / 74.0))               # (codes uniform over the range: weights ~N(0, 1 / K))
        o["wmat"] = o["w"].reshape(c.cout, c.K).astype(f64) - o["zp"]
    else:
        o["w"] = (rng.standard_normal(shape, dtype=f32) * f32(c.K ** -0.5)).astype(f16)
        o["wmat"] = o["w"].reshape(c.cout, c.K).astype(f64)
    e = c.epi
    ho, wo = c.out_hw() if e["res"] else (0, 0)             # (a refusal has no output extent to speak of: stride 0)
    o["bias"] = (rng.standard_normal(c.cout, dtype=f32) * f32(0.1)).astype(e["bias"]) if e["bias"] is not None else None
    o["ib"] = (rng.standard_normal((c.n, c.cout), dtype=f32) * f32(0.5)).astype(f16) if e["ib"] else None
    o["res"] = rng.standard_normal((c.n * ho * wo, c.cout), dtype=f32).astype(f16) if e["res"] else None
    return o


def columns(c, o):
    return im2col(o["x"], c.kh, c.kw, c.sh, c.sw, *c.pads)
