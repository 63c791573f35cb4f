"""The case table of the per-operator lowering tests (tests/test_op_lowering_cpu.py on the stub backend, tests/test_op_lowering_gpu.py on the device,
tools/make_golden_ops.py for the reference's outputs in tests/golden/op_cases.npz).

One case = one operator in one attribute form / layout / broadcast form:
  build(g)     emits the graph over onnxstream_amd.synth.graph.GraphBuilder: inputs, the operator under test through g.op(...), named outputs
  inputs       name -> shape as pushed (seeded values, three samples) or name -> callable(k) for a special sample k
  ref(i)       the float64 numpy restatement: i maps each input name to the float64 image of its f16-rounded sample; returns output name -> float64 array.
               Plain numpy written for this table: nothing here calls oracle/np_ops.py.  An entry `"<out>@f32"` holds numpy's f32 operation rounded once to
               f16 where the device must reproduce it bit for bit (Add, Sub, Mul, Neg).
  cls          "move"        bit-exact
               "elementwise" within one f16 ulp of the float64 value rounded to f16 (osg_elementwise.hip: f32 arithmetic, one rounding)
               "reduce"      the bound of the kernel-level test of the same kernel, named in `bound` (BOUNDS below cites where each comes from)
               "reject"      refused at plan time with a message that contains `reject`
               "chain"       several launches, no per-operator class (the graphs of tests/fusion_cases.py, which name a class per level where one launch remains)
  upcast       substrings for Model.set_upcast_substrings
  stub_values  the stub backend carries this case's values (every launch of it is data movement)
  const_out    outputs that depend on constants only: they have one sample however many were pushed

A channels-last operand is Transpose(0,3,1,2) of a plain [1,H,W,C] input (an alias in Lay::nhwc, no arithmetic); a shared operand is a weight; a per-sample
operand is an input.  REF_REFUSES lists the cases the reference itself refuses (restatement-only), REF_DIFFERS the ones where its form differs in kind."""
import math

import numpy as np

f16, f32, f64 = np.float16, np.float32, np.float64
I64MAX = 2 ** 63 - 1

# bound name -> where it is taken from (the kernel-level test of the same kernel)
BOUNDS = {
    "mean_f16": "tests/test_decoder_kernels.py::test_reduce_mean_last (f16): |got - want| <= ulp16(want)",
    "softmax_f16": "tests/test_decoder_kernels.py::test_softmax_last_f16: |got - p| <= ulp16(p) + 2^-11",
    "instance_norm": "tests/test_unet_attention_norm.py::test_instance_norm: norm_exact(x, gamma, beta, eps, ceil(L / 256) + 24, two-pass)",
    "contraction": "tests/test_contraction_instantiations.py::check: |got - want| <= 2^-11 |want| + (1 + 2^-11) (K + 3) 2^-24 S + 2^-25, at most 2 % of "
                   "the elements more than one f16 ulp from the correctly rounded value",
    "rms_chain": "tests/test_decoder_kernels.py::test_rms_norm_chain_f32 + test_rms_norm_f16_within_one_ulp: the fp32 chain is (ceil(C/64)/2 + 9) 2^-24 "
                 "relative off at worst, far below half an f16 ulp, so one rounding leaves it within one f16 ulp of float64",
}


class Case:
    def __init__(self, name, cls, build, inputs, ref, outs=("out",), reject=None, upcast=None, bound=None, stub_values=None, const_out=(), extra=None,
                 dynamic=False):
        self.name, self.cls, self.build, self.inputs, self.ref, self.outs = name, cls, build, inputs, ref, tuple(outs)
        self.reject, self.upcast, self.bound, self.const_out, self.extra, self.dynamic = reject, upcast, bound, tuple(const_out), extra or {}, dynamic
        self.stub_values = (cls == "move") if stub_values is None else stub_values
        assert cls in ("move", "elementwise", "reduce", "reject", "chain") and (cls != "reduce" or bound in BOUNDS) and (cls != "reject" or reject), name

    def sample(self, k):
        """fp32 inputs of pushed sample k (0..2)"""
        out = {}
        for j, (n, s) in enumerate(self.inputs.items()):
            out[n] = np.ascontiguousarray(s(k), f32) if callable(s) else rnd(_seed(self.name) + 10 * j + k, s)
        return out

    def want(self, k):
        return self.ref({n: r16(v) for n, v in self.sample(k).items()})


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100000


def r16(x):
    """float64 image of the f16 rounding of x"""
    return np.asarray(x, f32).astype(f16).astype(f64)


def rnd(seed, shape):
    """magnitudes in [0.25, 4] with either sign: no overflow, no cancellation to 0, safe as a divisor"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 4.0, shape)).astype(f32)


def pos(seed, shape):
    return np.abs(rnd(seed, shape))


def wt(name, shape, positive=False):
    """values of a weight: already f16-representable, so the graph and the restatement hold the same numbers"""
    v = rnd(_seed("w" + name), shape)
    return (np.abs(v) if positive else v).astype(f16).astype(f32)


CASES = []


def add(*a, **k):
    c = Case(*a, **k)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def nhwc_in(g, name, shape):
    """logical [1,C,H,W] tensor held channels-last: the input is pushed as [1,H,W,C]"""
    n, c, h, w = shape
    return g.transpose("/cl_" + name, g.input(name, (n, h, w, c)), (0, 3, 1, 2))


def cf(x):
    """the logical image of an input pushed as [1,H,W,C]"""
    return x.transpose(0, 3, 1, 2)


def cl_out(g, t, name="out"):
    n, c, h, w = t.shape
    return g.op("/rb_" + name, "Transpose", [t], (n, h, w, c), {"perm": "0,2,3,1"}, out_names=[name])


def i64(g, name, vals):
    return g.weight(name, np.asarray(vals, np.int64), dtype="int64")


# ======================================================================================================================================
# Add, Sub, Mul, Div: one graph holds the four kinds of one form (outputs Add, Sub, Mul, Div), each form with the operands in both orders
# ======================================================================================================================================
KINDS = {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": np.divide}


def _bin_ref(fa, fb):
    def ref(i):
        a, b = fa(i), fb(i)
        out = {}
        for kind, fn in KINDS.items():
            out[kind] = fn(a, b)
            if kind != "Div":
                out[kind + "@f32"] = fn(a.astype(f32), b.astype(f32)).astype(f16)
        return out
    return ref


def _bin(name, inputs, ea, eb, fa, fb, oshape, nhwc_out=False, both=True, **kw):
    """ea / eb(g) emit the operands (called once per graph), fa / fb(i) restate them"""
    for order in (("ab", "ba") if both else ("ab",)):
        def build(g, order=order):
            a, b = ea(g), eb(g)
            if order == "ba":
                a, b = b, a
            for kind in KINDS:
                if nhwc_out:
                    cl_out(g, g.op("/" + kind, kind, [a, b], oshape), kind)
                else:
                    g.op("/" + kind, kind, [a, b], oshape, out_names=[kind])
        ref = _bin_ref(fa, fb) if order == "ab" else _bin_ref(fb, fa)
        if nhwc_out:
            ref = (lambda r: lambda i: {k: (v.transpose(0, 2, 3, 1)) for k, v in r(i).items()})(ref)
        add(f"bin/{name}/{order}", "elementwise", build, inputs, ref, outs=tuple(KINDS), **kw)


def _w(name, shape):
    v = wt(name, shape)
    return (lambda g: g.weight(name, v, allow_quant=False)), (lambda i: v.astype(f64))


def _x(name, shape):
    return (lambda g: g.input(name, shape)), (lambda i: i[name])


def _xn(name, shape):
    return (lambda g: nhwc_in(g, name, shape)), (lambda i: cf(i[name]))


def _pl(shape):      # pushed shape of a channels-last input
    return (shape[0], shape[2], shape[3], shape[1])


T, C8, C5 = 3, 8, 5
ex, fx = _x("x", (1, T, C5))
ey, fy = _x("y", (1, T, C5))
_bin("plain_same", {"x": (1, T, C5), "y": (1, T, C5)}, ex, ey, fx, fy, (1, T, C5), both=False)
for nm, ws, xs in [("scalar", (), (1, T, C5)), ("vecC8", (C8,), (1, T, C8)), ("vecC5", (C5,), (1, T, C5)), ("col", (1, T, 1), (1, T, C5)),
                   ("rank2_rank4", (T, C5), (1, 2, T, C5)), ("rank5", (1, 2, 1, 2, C5), (1, 2, 3, 2, C5))]:
    ew, fw = _w("/c_" + nm, ws)
    ex, fx = _x("x", xs)
    _bin("plain_" + nm, {"x": xs}, ex, ew, fx, fw, xs)
ew, fw = _w("/c_row", (1, 1, C5))
ex, fx = _x("x", (1, T, 1))
_bin("plain_col_row", {"x": (1, T, 1)}, ex, ew, fx, fw, (1, T, C5))                      # [1,T,1] against [1,1,C]: both operands stretch

XS = (1, C8, 2, 4)                                                                         # C = H * W: a [1,1,H,W] operand has C elements and is NOT per-channel
ex, fx = _xn("x", XS)
ey, fy = _xn("y", XS)
_bin("nhwc_same", {"x": _pl(XS), "y": _pl(XS)}, ex, ey, fx, fy, XS, nhwc_out=True, both=False)
for nm, ws in [("c11", (C8, 1, 1)), ("1c11", (1, C8, 1, 1)), ("scalar", ())]:
    ew, fw = _w("/n_" + nm, ws)
    _bin("nhwc_" + nm, {"x": _pl(XS)}, ex, ew, fx, fw, XS, nhwc_out=True)
et, ft = _x("t", (1, C8, 1, 1))
_bin("nhwc_temb", {"x": _pl(XS), "t": (1, C8, 1, 1)}, ex, et, fx, ft, XS, nhwc_out=True)   # the time-embedding add: a per-sample [1,C,1,1] input
ep, fp = _x("p", XS)
_bin("nhwc_plain_same", {"x": _pl(XS), "p": XS}, ex, ep, fx, fp, XS)
ew, fw = _w("/n_11hw", (1, 1, 2, 4))
_bin("nhwc_11hw", {"x": _pl(XS)}, ex, ew, fx, fw, XS)
XC = (1, C8, C8, C8)
ex, fx = _xn("x", XC)
ew, fw = _w("/n_w", (C8,))
_bin("nhwc_vecW", {"x": _pl(XC)}, ex, ew, fx, fw, XC)                                      # [W] with W == C == H broadcasts along W
XF = (1, C5, 3, 2)
ex, fx = _xn("x", XF)
ew, fw = _w("/n_c11_5", (C5, 1, 1))
_bin("nhwc_c11_C5", {"x": _pl(XF)}, ex, ew, fx, fw, XF, nhwc_out=True)
ea, fa = _x("a", (1, T, C5))
eb, fb = _x("b", (1, 1, C5))
_bin("persample_persample", {"a": (1, T, C5), "b": (1, 1, C5)}, ea, eb, fa, fb, (1, T, C5))
ew, fw = _w("/shared", (1, T, C8))
ex, fx = _x("x", (1, T, C8))
_bin("shared_persample", {"x": (1, T, C8)}, ew, ex, fw, fx, (1, T, C8))
for kind in KINDS:
    v6 = wt("/c_rank6", (1, 2, 1, 3, 2, 4))
    add(f"bin/rank6/{kind}", "reject", (lambda g, kind=kind, v6=v6: g.op("/" + kind, kind, [g.input("x", (1, 2, 2, 3, 2, 4)), g.weight("/c6", v6, allow_quant=False)],
                                                                      (1, 2, 2, 3, 2, 4), out_names=["out"])),
        {"x": (1, 2, 2, 3, 2, 4)}, None, reject="rank too large")


# ======================================================================================================================================
# Sigmoid, Erf, Sqrt, Sin, Cos, Neg, Pow
# ======================================================================================================================================
UNARY = {"Sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)), "Erf": np.vectorize(math.erf, otypes=[f64]), "Sqrt": np.sqrt, "Sin": np.sin, "Cos": np.cos,
         "Neg": np.negative}
US = (1, 5, 413)                  # 2065 elements: no multiple of 8, more than one block
UN = (1, C8, 3, 5)


def _un_ref(fn, kind, src):
    def ref(i):
        x = src(i)
        out = {"out": fn(x)}
        if kind == "Neg":
            out["out@f32"] = (-x.astype(f32)).astype(f16)
        return out
    return ref


for kind, fn in UNARY.items():
    gen = (lambda k, kind=kind: pos(_seed(kind) + k, US)) if kind == "Sqrt" else US
    add(f"unary/{kind}/odd_count", "elementwise", (lambda g, kind=kind: g.op("/" + kind, kind, [g.input("x", US)], US, out_names=["out"])), {"x": gen},
        _un_ref(fn, kind, lambda i: i["x"]))
    gen = (lambda k, kind=kind: pos(_seed(kind) + 7 + k, _pl(UN))) if kind == "Sqrt" else _pl(UN)
    add(f"unary/{kind}/nhwc", "elementwise", (lambda g, kind=kind: cl_out(g, g.op("/" + kind, kind, [nhwc_in(g, "x", UN)], UN))), {"x": gen},
        _un_ref(fn, kind, lambda i: i["x"]))          # (elementwise on the channels-last image, read back channels-last: the pushed layout again)
for p in (2.0, 3.0, 0.5, -1.0):
    gen = (lambda k, p=p: pos(_seed("pow") + k, US)) if p == 0.5 else US
    add(f"unary/Pow/{p:g}", "elementwise", (lambda g, p=p: g.op("/Pow", "Pow", [g.input("x", US), g.scalar("/Pow.e", p)], US, out_names=["out"])), {"x": gen},
        (lambda i, p=p: {"out": np.power(i["x"], p)}))
add("unary/Pow/nhwc", "elementwise", (lambda g: cl_out(g, g.op("/Pow", "Pow", [nhwc_in(g, "x", UN), g.scalar("/Pow.e", 3.0)], UN))), {"x": _pl(UN)},
    lambda i: {"out": np.power(i["x"], 3.0)})
add("unary/Pow/exponent_shape1", "reject",
    (lambda g: g.op("/Pow", "Pow", [g.input("x", US), g.weight("/Pow.e", np.asarray([2.0], f32), allow_quant=False)], US, out_names=["out"])), {"x": US}, None,
    reject="power must be a scalar")


# ======================================================================================================================================
# The upcast chain: the six-operation spelling of RMS norm under m_requires_upcast (push_tensor's rule: a flagged operation's fp32 result stays fp32 only
# while the NEXT operation is its sole consumer; otherwise it is rounded to f16).  In every variant below exactly one f16 rounding lies between the input and
# `out`, or two where the variant says so, and the restatement rounds at those points only.
# ======================================================================================================================================
RC, RT, REPS = 48, 3, 1e-5
EPS16 = float(f16(REPS))           # a 0-d f16 weight holds eps


def _rms(g, pow_name, second_consumer=None):
    x = g.input("x", (1, RT, RC))
    p = g.op(pow_name, "Pow", [x, g.scalar("/norm.two", 2.0)], (1, RT, RC))
    m = g.op("/norm/ReduceMean", "ReduceMean", [p], (1, RT, 1), {"axes": "-1", "keepdims": "1"})
    e = g.op("/norm/Add", "Add", [m, g.scalar("/norm.eps", REPS)], (1, RT, 1))
    s = g.op("/norm/Sqrt", "Sqrt", [e], (1, RT, 1))
    r = g.op("/norm/Div", "Div", [g.scalar("/norm.one", 1.0), s], (1, RT, 1))
    g.op("/norm/Mul", "Mul", [x, r], (1, RT, RC), out_names=["out"])
    if second_consumer:
        g.op("/plain/Neg", "Neg", [m], (1, RT, 1), out_names=["neg_mean"])     # the second consumer of the flagged ReduceMean's output, at the queue's end


def _rms_ref(i):
    x = i["x"]
    return {"out": x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS16)}          # fp32 from the f16 input to `out`: one rounding, at `out`


def _rms_ref_plain_pow(i):
    x = i["x"]
    p = r16(x * x)                                                                 # Pow is not flagged: f16 arithmetic (x * x is exact in f32: correctly rounded)
    return {"out": x / np.sqrt(p.mean(-1, keepdims=True) + EPS16)}


def _rms_ref_two(i):
    x = i["x"]
    m = r16((x * x).mean(-1, keepdims=True))                                       # two consumers: rounded to f16 before both
    return {"out": x / np.sqrt(m + EPS16), "neg_mean": -m}


RW = (1.0 + wt("/norm_w", (RC,)) / 16).astype(f16).astype(f32)


def _rms7(g):
    """the seven-operation spelling, fully flagged: at fusion 2 fuse_rms_norm takes it as one osg.RMSNorm launch, at fusion 0 it runs op by op in fp32"""
    x = g.input("x", (1, RT, RC))
    p = g.op("/norm/Pow", "Pow", [x, g.scalar("/norm.two", 2.0)], (1, RT, RC))
    m = g.op("/norm/ReduceMean", "ReduceMean", [p], (1, RT, 1), {"axes": "-1", "keepdims": "1"})
    e = g.op("/norm/Add", "Add", [m, g.scalar("/norm.eps", REPS)], (1, RT, 1))
    s = g.op("/norm/Sqrt", "Sqrt", [e], (1, RT, 1))
    r = g.op("/norm/Div", "Div", [g.scalar("/norm.one", 1.0), s], (1, RT, 1))
    xn = g.op("/norm/Mul", "Mul", [x, r], (1, RT, RC))
    g.op("/norm/Mul_1", "Mul", [g.weight("/norm.weight", RW, allow_quant=False), xn], (1, RT, RC), out_names=["out"])


add("upcast/rms7_weight", "reduce", _rms7, {"x": (1, RT, RC)},
    lambda i: {"out": RW.astype(f64) * i["x"] / np.sqrt((i["x"] * i["x"]).mean(-1, keepdims=True) + EPS16)}, upcast=["/norm/"], bound="rms_chain")
add("upcast/rms6", "reduce", lambda g: _rms(g, "/norm/Pow"), {"x": (1, RT, RC)}, _rms_ref, upcast=["/norm/"], bound="rms_chain")
add("upcast/rms6_plain_pow", "reduce", lambda g: _rms(g, "/plain/Pow"), {"x": (1, RT, RC)}, _rms_ref_plain_pow, upcast=["/norm/"], bound="rms_chain")
add("upcast/rms6_two_consumers", "reduce", lambda g: _rms(g, "/norm/Pow", True), {"x": (1, RT, RC)}, _rms_ref_two, outs=("out", "neg_mean"), upcast=["/norm/"],
    bound="rms_chain")


# ======================================================================================================================================
# ReduceMean (rows offset away from 0, as in the kernel-level f16 test: the bound is relative to the mean)
# ======================================================================================================================================
def _mean_in(shape, name):
    return lambda k: 2.0 + 0.5 * np.random.default_rng(_seed(name) + k).standard_normal(shape)


for C in (1, 7, 320):
    for ax in ("-1", "2"):
        s = (1, T, C)
        add(f"mean/C{C}/axes{ax}", "reduce", (lambda g, s=s, ax=ax: g.op("/m", "ReduceMean", [g.input("x", s)], s[:-1] + (1,), {"axes": ax, "keepdims": "1"},
                                                                   out_names=["out"])), {"x": _mean_in(s, f"mean{C}")},
            lambda i: {"out": i["x"].mean(-1, keepdims=True)}, bound="mean_f16")
add("mean/no_attributes", "reduce", (lambda g: g.op("/m", "ReduceMean", [g.input("x", (1, T, 7))], (1, T, 1), out_names=["out"])), {"x": _mean_in((1, T, 7), "meanna")},
    lambda i: {"out": i["x"].mean(-1, keepdims=True)}, bound="mean_f16")
add("mean/nhwc", "reduce", (lambda g: g.op("/m", "ReduceMean", [nhwc_in(g, "x", XS)], (1, C8, 2, 1), {"axes": "-1", "keepdims": "1"}, out_names=["out"])),
    {"x": _mean_in(_pl(XS), "meannhwc")}, lambda i: {"out": cf(i["x"]).mean(-1, keepdims=True)}, bound="mean_f16")
add("mean/axes1_rank3", "reject", (lambda g: g.op("/m", "ReduceMean", [g.input("x", (1, T, 7))], (1, 1, 7), {"axes": "1", "keepdims": "1"}, out_names=["out"])),
    {"x": (1, T, 7)}, None, reject="reduction supported on the last axis only")
add("mean/keepdims0", "reject", (lambda g: g.op("/m", "ReduceMean", [g.input("x", (1, T, 7))], (1, T), {"axes": "-1", "keepdims": "0"}, out_names=["out"])),
    {"x": (1, T, 7)}, None, reject="keepdims must be 1")


# ======================================================================================================================================
# Softmax
# ======================================================================================================================================
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _sm(name, shape, axis, gen=None, src=None, emit=None):
    attrs = None if axis is None else {"axis": str(axis)}
    emit = emit or (lambda g: g.input("x", shape))
    src = src or (lambda i: i["x"])
    add("softmax/" + name, "reduce", (lambda g: g.op("/sm", "Softmax", [emit(g)], shape, attrs, out_names=["out"])), {"x": gen or shape},
        (lambda i: {"out": _softmax(src(i), -1 if axis is None else axis)}), bound="softmax_f16")


_sm("no_axis", (1, 4, 7), None)
_sm("axis-1", (1, 4, 7), -1)
_sm("axis1_rank3", (1, 5, 7), 1)
_sm("axis1_rank4", (1, 3, 4, 5), 1)
_sm("axis-2", (1, 3, 4, 5), -2)
_sm("nhwc", XS, -1, gen=_pl(XS), src=lambda i: cf(i["x"]), emit=lambda g: nhwc_in(g, "x", XS))
_sm("nhwc_axis1", XS, 1, gen=_pl(XS), src=lambda i: cf(i["x"]), emit=lambda g: nhwc_in(g, "x", XS))


def _big_row(k):
    x = rnd(900 + k, (1, 4, 7)) * 3
    x[0, 1] = [6e4, 5.9e4, -6e4, 6e4, 0.0, 100.0, 5.99e4]
    return x


_sm("row_6e4", (1, 4, 7), -1, gen=_big_row)


# ======================================================================================================================================
# MatMul, Gemm
# ======================================================================================================================================
def _mm_ref(fa, fb, so=None):
    """the product, and what the contraction bound needs: S = |a| . |b| and K"""
    def ref(i):
        a, b = fa(i), fb(i)
        out, S = a @ b, np.abs(a) @ np.abs(b)
        return {"out": out.reshape(so or out.shape), "out@S": S.reshape(so or S.shape), "out@K": np.asarray(a.shape[-1])}
    return ref


def _mm(name, sa, sb, so, **kw):
    add("matmul/" + name, "reduce", (lambda g: g.op("/mm", "MatMul", [g.input("a", sa), g.input("b", sb)], so, out_names=["out"])), {"a": sa, "b": sb},
        _mm_ref(lambda i: i["a"], lambda i: i["b"], so), bound="contraction", **kw)


_mm("nMK_nKN", (2, 3, 8), (2, 8, 5), (2, 3, 5))
_mm("1nMK_nKN", (1, 2, 3, 8), (2, 8, 5), (1, 2, 3, 5))
_mm("1nMK_1nKN", (1, 2, 3, 8), (1, 2, 8, 5), (1, 2, 3, 5))
_mm("nMK_1nKN", (2, 3, 8), (1, 2, 8, 5), (2, 3, 5))                 # the lead 1 on the right only: the result keeps the LEFT operand's rank (see REF_DIFFERS)
_mm("M1", (2, 1, 8), (2, 8, 5), (2, 1, 5))
_mm("K11", (2, 3, 11), (2, 11, 5), (2, 3, 5))
for nm, sa in [("rank2", (3, 8)), ("rank3", (1, 3, 8)), ("rank4", (1, 2, 3, 8))]:
    for N in (8, 5):
        w = wt(f"/mm_w{nm}{N}", (8, N)) / 2
        add(f"matmul/const_{nm}_N{N}", "reduce", (lambda g, sa=sa, w=w, N=N: g.op("/mm", "MatMul", [g.input("a", sa), g.weight("/mm.weight", w)], sa[:-1] + (N,),
                                                                            out_names=["out"])), {"a": sa},
            _mm_ref(lambda i: i["a"], lambda i, w=w: w.astype(f64)), bound="contraction")
GW, GB = wt("/gemm_w", (11, 5)) / 2, wt("/gemm_b", (5,))


def _gemm(g, attrs=None, bias=True):
    ins = [g.input("a", (1, 11)), g.weight("/gemm.weight", GW)] + ([g.weight("/gemm.bias", GB, allow_quant=False)] if bias else [])
    g.op("/gemm", "Gemm", ins, (1, 5), attrs, out_names=["out"])


add("gemm/M1_bias", "reduce", _gemm, {"a": (1, 11)},
    lambda i: {"out": i["a"] @ GW.astype(f64) + GB, "out@S": np.abs(i["a"]) @ np.abs(GW.astype(f64)) + np.abs(GB), "out@K": np.asarray(11)}, bound="contraction")
add("gemm/attributes_1", "reduce", lambda g: _gemm(g, {"alpha": "1.0", "beta": "1.0", "transA": "0", "transB": "0"}), {"a": (1, 11)},
    lambda i: {"out": i["a"] @ GW.astype(f64) + GB, "out@S": np.abs(i["a"]) @ np.abs(GW.astype(f64)) + np.abs(GB), "out@K": np.asarray(11)}, bound="contraction")
add("gemm/transB1", "reject", lambda g: _gemm(g, {"transB": "1"}), {"a": (1, 11)}, None, reject="transB != 0 case not implemented")
add("gemm/alpha0.5", "reject", lambda g: _gemm(g, {"alpha": "0.5"}), {"a": (1, 11)}, None, reject="alpha != 1 case not implemented")
add("gemm/two_inputs", "reject", lambda g: _gemm(g, bias=False), {"a": (1, 11)}, None, reject="wrong number of inputs")


# ======================================================================================================================================
# Expand (x * ones on the device: exact, the sign of zero included; an arithmetic launch, so the stub carries shapes only)
# ======================================================================================================================================
def _ex(name, sx, target, so, gen=None, emit=None, src=None):
    emit = emit or (lambda g: g.input("x", sx))
    src = src or (lambda i: i["x"])
    add("expand/" + name, "move", (lambda g: g.op("/ex", "Expand", [emit(g), i64(g, "/ex.shape", target)], so, out_names=["out"])), {"x": gen or sx},
        (lambda i: {"out": np.broadcast_to(src(i), so).copy()}), stub_values=False)


_ex("leading", (1, 3, 4), [2, 3, 4], (2, 3, 4))
_ex("middle", (2, 1, 4), [2, 3, 4], (2, 3, 4))
_ex("trailing", (2, 3, 1), [2, 3, 4], (2, 3, 4))
_ex("rank_growth", (3, 4), [2, 3, 4], (2, 3, 4))
_ex("target1_input4", (2, 4), [2, 1], (2, 4))
_ex("nhwc", (1, C8, 1, 3), [1, C8, 2, 3], (1, C8, 2, 3), gen=(1, 1, 3, C8), emit=lambda g: nhwc_in(g, "x", (1, C8, 1, 3)), src=lambda i: cf(i["x"]))


def _neg_zero(k):
    x = rnd(77 + k, (2, 1, 4))
    x[0, 0, 1], x[1, 0, 2], x[1, 0, 0] = -0.0, -0.0, 0.0
    return x


_ex("negative_zero", (2, 1, 4), [2, 3, 4], (2, 3, 4), gen=_neg_zero)


# ======================================================================================================================================
# InstanceNormalization
# ======================================================================================================================================
ING, INL = 4, 35
IN_S, IN_B = wt("/in_scale", (ING,)), wt("/in_bias", (ING,))


def _inorm(g):
    x = g.input("x", (1, ING, INL))
    g.op("/in", "InstanceNormalization", [x, g.weight("/in.scale", IN_S, dtype="float32", allow_quant=False), g.weight("/in.bias", IN_B, dtype="float32", allow_quant=False)],
         (1, ING, INL), {"epsilon": "1e-05"}, out_names=["out"])


def _inorm_ref(i):
    x = i["x"]
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return {"out": (x - mu) / np.sqrt(var + float(f32(1e-5))) * IN_S.astype(f64)[None, :, None] + IN_B.astype(f64)[None, :, None]}


add("instance_norm/odd_L", "reduce", _inorm, {"x": (1, ING, INL)}, _inorm_ref, bound="instance_norm", extra={"gamma": IN_S, "beta": IN_B, "L": INL})


# ======================================================================================================================================
# Concat
# ======================================================================================================================================
def _cat(name, shapes, axis, so, same=False, **kw):
    names = [f"x{j}" for j in range(len(shapes))]

    def build(g):
        ts = [g.input(n, s) for n, s in zip(names, shapes)]
        if same:
            ts = ts + ts
        g.op("/cat", "Concat", ts, so, {"axis": str(axis)}, out_names=["out"])
    add("concat/" + name, "move", build, dict(zip(names, shapes)), (lambda i: {"out": np.concatenate([i[n] for n in names] * (2 if same else 1), axis)}), **kw)


_cat("axis0", [(2, 3), (1, 3)], 0, (3, 3))
_cat("middle_run3", [(1, 2, 3), (1, 4, 3)], 1, (1, 6, 3))
_cat("last_run1", [(1, 2, 3), (1, 2, 1)], 2, (1, 2, 4))
_cat("last_run3", [(1, 2, 1), (1, 2, 3)], -1, (1, 2, 4))
_cat("axis-2", [(1, 2, 3), (1, 1, 3)], -2, (1, 3, 3))
_cat("one_operand", [(1, 2, 3)], 1, (1, 2, 3))
_cat("three_operands", [(1, 2, 3), (1, 1, 3), (1, 4, 3)], 1, (1, 7, 3))
_cat("four_operands", [(1, 2, 2), (1, 2, 1), (1, 2, 3), (1, 2, 1)], 2, (1, 2, 7))
_cat("same_tensor_twice", [(1, 2, 3)], 1, (1, 4, 3), same=True)
_cat("empty_between_live", [(1, 2, 3), (1, 0, 3), (1, 1, 3)], 1, (1, 3, 3), dynamic=True)    # (a 0 in model.txt needs support_dynamic_shapes)


def _cat_nhwc(name, chans, axis, plain=(), same=False):
    H, W = 2, 3
    shapes = [(1, c, H, W) for c in chans] if axis == 1 else [(1, 4, h, W) for h in chans]
    names = [f"x{j}" for j in range(len(shapes))]
    so = list(shapes[0])
    so[axis] = sum(s[axis] for s in shapes) * (2 if same else 1)

    def build(g):
        ts = [g.input(n, s) if j in plain else nhwc_in(g, n, s) for j, (n, s) in enumerate(zip(names, shapes))]
        if same:
            ts = ts + ts
        g.op("/cat", "Concat", ts, tuple(so), {"axis": str(axis)}, out_names=["out"])
    add("concat/" + name, "move", build, {n: (s if j in plain else _pl(s)) for j, (n, s) in enumerate(zip(names, shapes))},
        (lambda i: {"out": np.concatenate([i[n] if j in plain else cf(i[n]) for j, n in enumerate(names)] * (2 if same else 1), axis)}))


_cat_nhwc("nhwc_axis1_C8", [8, 8], 1)
_cat_nhwc("nhwc_axis1_C5_3", [5, 3], 1)
_cat_nhwc("nhwc_axis1_three", [8, 4, 12], 1)
_cat_nhwc("nhwc_axis1_same_twice", [8], 1, same=True)
_cat_nhwc("nhwc_plain_axis1", [8, 4], 1, plain=(1,))
_cat_nhwc("nhwc_axis2", [2, 3], 2)


# ======================================================================================================================================
# Split
# ======================================================================================================================================
def _split(name, sx, axis, sizes, nhwc=False):
    outs = [f"o{j}" for j in range(len(sizes))]
    ax = axis % len(sx)
    shapes = [sx[:ax] + (n,) + sx[ax + 1:] for n in sizes]

    def build(g):
        x = nhwc_in(g, "x", sx) if nhwc else g.input("x", sx)
        g.op("/split", "Split", [x, i64(g, "/split.sizes", sizes)], shapes, {"axis": str(axis)}, out_names=outs)
    add("split/" + name, "move", build, {"x": _pl(sx) if nhwc else sx},
        (lambda i: dict(zip(outs, np.split(cf(i["x"]) if nhwc else i["x"], np.cumsum(sizes)[:-1], ax)))), outs=outs)


_split("axis0", (4, 3), 0, [1, 3])
_split("axis1_size1", (1, 5, 3), 1, [2, 1, 2])
_split("last", (1, 2, 7), 2, [3, 4])
_split("axis-1", (1, 2, 7), -1, [1, 5, 1])
_split("axis-2", (1, 5, 3), -2, [4, 1])
_split("nhwc_axis1", (1, C8, 2, 3), 1, [3, 5], nhwc=True)
_split("nhwc_axis2", (1, C8, 3, 2), 2, [1, 2], nhwc=True)


# ======================================================================================================================================
# Slice (the reference's rules: a start past the end is clamped to dim - 1, an end to dim; last or last-but-one axis; step 1)
# ======================================================================================================================================
SX = (1, 3, 6, 7)


def _slice(name, starts, ends, axes=None, steps=None, want=None, reject=None, sx=SX):
    cut = want if callable(want) else (lambda x: x[want])

    def build(g):
        ins = [g.input("x", sx), i64(g, "/sl.starts", starts), i64(g, "/sl.ends", ends)]
        if axes is not None:
            ins.append(i64(g, "/sl.axes", axes))
        if steps is not None:
            ins.append(i64(g, "/sl.steps", steps))
        so = cut(np.zeros(sx)).shape if want is not None else sx
        g.op("/sl", "Slice", ins, so, out_names=["out"])
    if reject:
        add("slice/" + name, "reject", build, {"x": sx}, None, reject=reject)
    else:
        add("slice/" + name, "move", build, {"x": sx}, lambda i: {"out": cut(i["x"])})


_ = slice
_slice("one_axis_no_axes", [1], [5], want=(_(None), _(None), _(None), _(1, 5)))
_slice("two_axes_no_axes", [1, 2], [6, 4], want=lambda x: x[..., 1:6][..., 2:4])      # the reference's form: see REF_DIFFERS
_slice("axes-1", [2], [7], [-1], want=(_(None), _(None), _(None), _(2, 7)))
_slice("axes-2", [0], [4], [-2], want=(_(None), _(None), _(0, 4)))
_slice("axes-2-1", [1, 3], [5, 6], [-2, -1], want=(_(None), _(None), _(1, 5), _(3, 6)))
_slice("axes-1-2", [3, 1], [6, 5], [-1, -2], want=(_(None), _(None), _(1, 5), _(3, 6)))
_slice("axes_positive", [2], [5], [3], want=(_(None), _(None), _(None), _(2, 5)))
_slice("negative_start_end", [-5], [-1], [-1], want=(_(None), _(None), _(None), _(2, 6)))
_slice("end_int64_max", [3], [I64MAX], [-1], want=(_(None), _(None), _(None), _(3, 7)))
_slice("start_past_end_clamped", [7 + 3], [I64MAX], [-1], want=(_(None), _(None), _(None), _(6, 7)))
_slice("steps1", [1], [4], [-1], [1], want=(_(None), _(None), _(None), _(1, 4)))
_slice("step2", [1], [5], [-1], [2], reject="unsupported steps value(s)")
_slice("axis_rank-3", [1], [2], [1], reject="slice supported on last or last but one axis only")
_slice("start_ge_end", [4], [4], [-1], reject="invalid value(s) in starts and/or ends")
del _


# ======================================================================================================================================
# Gather (the reference's shape rules: leading 1-dims of the table are stripped and given back, a 0-d index on a >2-D table drops the axis)
# ======================================================================================================================================
def _gather(name, sx, idx, axis, so, const_table=False, reject=None):
    idx = np.asarray(idx, np.int64)
    tab = wt("/tab_" + name, sx) if const_table else None

    def build(g):
        if const_table:
            x = g.weight("/g.table", tab)
            d = g.input("d", (1, 2))
            g.op("/d", "Reshape", [d, i64(g, "/d.shape", [2, 1])], (2, 1), {"allowzero": "0"}, out_names=["d_out"])
        else:
            x = g.input("x", sx)
        g.op("/g", "Gather", [x, g.weight("/g.idx", idx, dtype="int64")], [so], {"axis": str(axis)}, out_names=["out"])     # ([so]: a 0-d output is an empty tuple)

    def ref(i):
        x = tab.astype(f64) if const_table else i["x"]
        out = {"out": np.take(x, idx, axis).reshape(so)}
        if const_table:
            out["d_out"] = i["d"].reshape(2, 1)
        return out
    ins = {"d": (1, 2)} if const_table else {"x": sx}
    if reject:
        add("gather/" + name, "reject", build, ins, None, reject=reject)
    else:
        add("gather/" + name, "move", build, ins, ref, outs=("out", "d_out") if const_table else ("out",), const_out=("out",) if const_table else ())


_gather("table2d_idx1D", (9, 4), [[4, 0, -1, 8, -9]], 0, (1, 5, 4), const_table=True)
_gather("idx0d_on_1d", (5,), 3, 0, ())
_gather("axis1_1VE", (1, 6, 4), [[5, 0, -2]], 1, (1, 1, 3, 4))
_gather("idx0d_on_3d", (4, 2, 3), 2, 0, (2, 3))
_gather("persample_table", (6, 4), [[1, -1, 3]], 0, (1, 3, 4))
_gather("idx1d", (6, 4), [2, 5], 0, (2, 4))
_gather("axis_nonzero", (2, 6, 4), [[1]], 1, (2, 1, 1, 4), reject="axis must be 0")


# ======================================================================================================================================
# Transpose, Reshape, Flatten, Unsqueeze, Squeeze
# ======================================================================================================================================
def _mv(name, typ, sx, so, attrs=None, const=None, fn=None):
    def build(g):
        ins = [g.input("x", sx)] + ([i64(g, "/mv.c", const)] if const is not None else [])
        g.op("/mv", typ, ins, so, attrs, out_names=["out"])
    add(f"{typ.lower()}/{name}", "move", build, {"x": sx}, (lambda i: {"out": fn(i["x"]) if fn else i["x"].reshape(so)}))


_mv("unit_dims_11Hd", "Transpose", (1, 1, 5, 4), (1, 5, 1, 4), {"perm": "0,2,1,3"}, fn=lambda x: x.transpose(0, 2, 1, 3))
_mv("unit_dims_1H1d", "Transpose", (1, 5, 1, 4), (1, 1, 5, 4), {"perm": "0,2,1,3"}, fn=lambda x: x.transpose(0, 2, 1, 3))
_mv("same_perm_no_unit", "Transpose", (1, 3, 5, 4), (1, 5, 3, 4), {"perm": "0,2,1,3"}, fn=lambda x: x.transpose(0, 2, 1, 3))
_mv("unit_dim_moves_past_two", "Transpose", (3, 1, 4), (1, 3, 4), {"perm": "1,0,2"}, fn=lambda x: x.transpose(1, 0, 2))
_mv("zero_and_minus1", "Reshape", (1, 4, 6), (1, 8, 3), {"allowzero": "0"}, const=[0, -1, 3])
_mv("minus1_first", "Reshape", (2, 3, 4), (6, 4), None, const=[-1, 4])
for ax, so in [(0, (1, 24)), (1, (2, 12)), (-1, (6, 4)), (3, (24, 1))]:
    _mv(f"axis{ax}", "Flatten", (2, 3, 4), so, {"axis": str(ax)})
_mv("default_axis", "Flatten", (2, 3, 4), (2, 12))
_mv("axes_0_-1", "Unsqueeze", (3, 4), (1, 3, 4, 1), const=[0, -1])
_mv("two_axes", "Squeeze", (1, 3, 1, 4), (3, 4), const=[0, 2])
_mv("negative_axis", "Squeeze", (1, 3, 1, 4), (1, 3, 4), const=[-2])


# ======================================================================================================================================
# Resize (nearest, asymmetric, floor; the reference's rules: out = floor((float)in * scale), source index = (size_t)(o / scale) clamped, with
# scale = (float)size / (float)in in the `sizes` form)
# ======================================================================================================================================
RATTR = {"coordinate_transformation_mode": "asymmetric", "mode": "nearest", "nearest_mode": "floor"}


def _nearest(x, Ho, Wo, sh, sw):
    H, W = x.shape[2:]
    hi = np.minimum((np.arange(Ho, dtype=f32) / f32(sh)).astype(np.int64), H - 1)
    wi = np.minimum((np.arange(Wo, dtype=f32) / f32(sw)).astype(np.int64), W - 1)
    return x[:, :, hi][:, :, :, wi]


def _resize(name, sx, scale=None, sizes=None, nhwc=False):
    if sizes:
        Ho, Wo = sizes
        sh, sw = f32(Ho) / f32(sx[2]), f32(Wo) / f32(sx[3])
    else:
        sh = sw = f32(scale)
        Ho, Wo = int(np.floor(f32(sx[2]) * sh)), int(np.floor(f32(sx[3]) * sw))
    so = (1, sx[1], Ho, Wo)

    def build(g):
        x = nhwc_in(g, "x", sx) if nhwc else g.input("x", sx)
        if sizes:
            ins = [x, None, None, i64(g, "/rs.sizes", [1, sx[1], Ho, Wo])]
        else:
            ins = [x, None, g.weight("/rs.scales", np.asarray([1, 1, scale, scale], f32), dtype="float32")]
        y = g.op("/rs", "Resize", ins, so, RATTR, out_names=None if nhwc else ["out"])
        if nhwc:
            cl_out(g, y)
    add("resize/" + name, "move", build, {"x": _pl(sx) if nhwc else sx},
        (lambda i: {"out": _nearest(cf(i["x"]), Ho, Wo, sh, sw).transpose(0, 2, 3, 1) if nhwc else _nearest(i["x"], Ho, Wo, sh, sw)}))


for sc in (2, 1.5, 0.5):
    _resize(f"scale{sc}_nhwc", (1, C8, 5, 6), scale=sc, nhwc=True)
    _resize(f"scale{sc}_plain", (1, 3, 5, 6), scale=sc)
_resize("sizes_nhwc", (1, C8, 4, 6), sizes=(7, 5), nhwc=True)
_resize("sizes_plain", (1, 3, 4, 6), sizes=(7, 5))


# ======================================================================================================================================
# MaxPool (an arithmetic launch: the stub carries shapes only)
# ======================================================================================================================================
def _pool_ref(x, k, s, pads):
    ph, pw = pads[0] + pads[2], pads[1] + pads[3]              # re-centred, the reference's form: see REF_DIFFERS
    pt, pl = ph // 2, pw // 2
    pb, pr = ph - pt, pw - pl
    xp = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)), constant_values=-np.inf)
    Ho, Wo = (xp.shape[2] - k) // s + 1, (xp.shape[3] - k) // s + 1
    out = np.full(x.shape[:2] + (Ho, Wo), -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, xp[:, :, dy:dy + s * Ho:s, dx:dx + s * Wo:s][:, :, :Ho, :Wo])
    return out


def _pool(name, sx, k, s, pads, nhwc=True, gen=None, dilations=True):
    Ho, Wo = (sx[2] + pads[0] + pads[2] - k) // s + 1, (sx[3] + pads[1] + pads[3] - k) // s + 1
    so = (1, sx[1], Ho, Wo)
    attrs = {"ceil_mode": "0", "kernel_shape": f"{k},{k}", "pads": ",".join(map(str, pads)), "strides": f"{s},{s}"}
    if dilations:
        attrs["dilations"] = "1,1"

    def build(g):
        x = nhwc_in(g, "x", sx) if nhwc else g.input("x", sx)
        g.op("/mp", "MaxPool", [x], so, attrs, out_names=["out"])
    add("maxpool/" + name, "move", build, {"x": gen or (_pl(sx) if nhwc else sx)}, (lambda i: {"out": _pool_ref(cf(i["x"]) if nhwc else i["x"], k, s, pads)}),
        stub_values=False)


_pool("k2s2", (1, C8, 6, 6), 2, 2, (0, 0, 0, 0))
_pool("k3s1p1", (1, C8, 5, 6), 3, 1, (1, 1, 1, 1))
_pool("k5s1p2", (1, C8, 5, 6), 5, 1, (2, 2, 2, 2))
_pool("pads0110", (1, C8, 5, 6), 2, 1, (0, 1, 1, 0))
_pool("pads1001", (1, C8, 5, 6), 2, 1, (1, 0, 0, 1))
_pool("pads2000", (1, C8, 5, 6), 3, 1, (2, 0, 0, 0))
_pool("no_dilations_attribute", (1, C8, 6, 6), 2, 2, (0, 0, 0, 0), dilations=False)
_pool("plain_C5", (1, C5, 6, 6), 3, 2, (1, 1, 1, 1), nhwc=False)
_pool("all_negative", (1, C8, 5, 6), 3, 1, (1, 1, 1, 1), gen=lambda k: -pos(55 + k, (1, 5, 6, C8)))


# ======================================================================================================================================
# Conv (f16): every attribute form of lower_conv -- one-sided pads (re-centred as the reference does: top = (top + bottom) / 2, the odd cell at the bottom, and
# the same from left to right), non-square kernels, strides per axis, attribute presence, layout, Conv1D.  Shapes pairwise distinct: C 8, H 7, W 6 -> 12 channels.
# ======================================================================================================================================
KC, KH_, KW_, KO = 8, 7, 6, 12
KX = (1, KC, KH_, KW_)
KB = wt("/conv_b", (KO,))


def _conv_restate(x, w, b, pads, strides):
    """float64 convolution of x [1,C,H,W] (or [1,C,L]: Conv1D over [1,C,L,1]) with w [O,I,kh,kw], the pads re-centred; and S, K of the contraction bound"""
    if x.ndim == 3:
        r = _conv_restate(x[..., None], w, b, (pads[0], 0, pads[1], 0), (strides[0], strides[0]))
        return {k: (v[..., 0] if v.ndim == 4 else v) for k, v in r.items()}
    O, I, kh, kw = w.shape
    ph, pw = pads[0] + pads[2], pads[1] + pads[3]
    pt, pl = ph // 2, pw // 2
    xp = np.pad(x, ((0, 0), (0, 0), (pt, ph - pt), (pl, pw - pl)))
    sh, sw = strides
    Ho, Wo = (xp.shape[2] - kh) // sh + 1, (xp.shape[3] - kw) // sw + 1
    out, S = np.zeros((1, O, Ho, Wo)), np.zeros((1, O, Ho, Wo))
    for dy in range(kh):
        for dx in range(kw):
            patch = xp[:, :, dy:dy + sh * (Ho - 1) + 1:sh, dx:dx + sw * (Wo - 1) + 1:sw]
            out += np.einsum("nchw,oc->nohw", patch, w[:, :, dy, dx])
            S += np.einsum("nchw,oc->nohw", np.abs(patch), np.abs(w[:, :, dy, dx]))
    if b is not None:
        out, S = out + b[None, :, None, None], S + np.abs(b)[None, :, None, None]
    return {"out": out, "out@S": S, "out@K": np.asarray(I * kh * kw)}


def _conv_case(name, k=(3, 3), pads=(1, 1, 1, 1), strides=(1, 1), attrs="all", bias="given", nhwc=True, sx=KX, wshape=None, bshape=None, reject=None, more=None, neg=False, **kw):
    """attrs: "all" (dilations, group, kernel_shape, pads, strides), "none" (dilations and group only: the defaults apply, the kernel size comes from the weights)
    or a dict as it stands; bias: "given", "absent" (two inputs) or "empty" (three inputs, the third an empty name); more: further attributes; neg: `out` is Neg of the
    convolution (exact on the device: the bound is the convolution's) -- the reference cannot hand a Conv1D's 3-D channels-last result out as a graph output"""
    one_d = len(sx) == 3
    wshape = wshape or ((KO, sx[1]) + tuple(k) + ((1,) if one_d else ()))
    wgt = wt("/conv_w" + name, wshape) / 16
    bvals = KB if bshape is None else wt("/conv_b" + name, bshape)
    join = lambda v: ",".join(map(str, v))       # noqa: E731
    if attrs == "all":
        a = {"dilations": "1" if one_d else "1,1", "group": "1", "kernel_shape": join(k), "pads": join(pads), "strides": join(strides)}
    elif attrs == "none":
        a = {"dilations": "1" if one_d else "1,1", "group": "1"}
    else:
        a = dict(attrs)
    a.update(more or {})
    p4 = tuple(pads) if not one_d else (pads[0], 0, pads[1], 0)
    s2 = tuple(strides) if not one_d else (strides[0], strides[0])
    k2 = tuple(k) if not one_d else (k[0], 1)
    ext = lambda n, p, kk, s: max((n + p - kk) // max(s, 1) + 1, 1)       # noqa: E731  (a refusal's graph still names an output shape)
    so = (1, wshape[0], ext(sx[2], p4[0] + p4[2], k2[0], s2[0])) + (() if one_d else (ext(sx[3], p4[1] + p4[3], k2[1], s2[1]),))

    def build(g):
        x = nhwc_in(g, "x", sx) if nhwc and not one_d else g.input("x", sx)
        ins = [x, g.weight("/conv.weight", wgt, conv=True, allow_quant=False)]
        if bias == "given":
            ins.append(g.weight("/conv.bias", bvals, allow_quant=False))
        elif bias == "empty":
            ins.append(None)
        y = g.op("/conv", "Conv", ins, so, a or None, out_names=None if neg else ["out"])
        if neg:
            g.op("/neg", "Neg", [y], so, out_names=["out"])
    inputs = {"x": _pl(sx) if nhwc and not one_d else sx}
    if reject:
        add("conv/" + name, "reject", build, inputs, None, reject=reject, **kw)
        return
    src = (lambda i: cf(i["x"])) if nhwc and not one_d else (lambda i: i["x"])

    def ref(i):
        r = _conv_restate(src(i), wgt.astype(f64), KB.astype(f64) if bias == "given" else None, pads, strides)
        if neg:
            r["out"] = -r["out"]
        return r
    add("conv/" + name, "reduce", build, inputs, ref, bound="contraction", stub_values=False, **kw)


_conv_case("k3_pad1")
_conv_case("plain_input", nhwc=False)
_conv_case("k1", k=(1, 1), pads=(0, 0, 0, 0))
_conv_case("pads_0011", pads=(0, 0, 1, 1))
_conv_case("pads_1100", pads=(1, 1, 0, 0))
_conv_case("pads_2000", pads=(2, 0, 0, 0))
_conv_case("pads_1021", pads=(1, 0, 2, 1))
_conv_case("stride2_pads_0011", pads=(0, 0, 1, 1), strides=(2, 2))
_conv_case("stride_2_1", strides=(2, 1))
_conv_case("k1x3", k=(1, 3), pads=(0, 1, 0, 1))
_conv_case("k3x1", k=(3, 1), pads=(1, 0, 1, 0))
_conv_case("k3x5", k=(3, 5), pads=(1, 2, 1, 2))
_conv_case("k5x7_pads_2323", k=(5, 7), pads=(2, 3, 2, 3))
_conv_case("no_pads_strides_kernel_shape", pads=(0, 0, 0, 0), attrs="none")
_conv_case("no_attributes", pads=(0, 0, 0, 0), attrs={})
_conv_case("no_bias", bias="absent")
_conv_case("bias_empty_name", bias="empty")
KL = (1, KC, 11)
_conv_case("conv1d_k3_stride2_pads_11", k=(3,), pads=(1, 1), strides=(2,), sx=KL, neg=True)
_conv_case("conv1d_pads_20", k=(3,), pads=(2, 0), strides=(1,), sx=KL, neg=True)
_conv_case("conv1d_no_attributes", k=(3,), pads=(0, 0), strides=(1,), sx=KL, attrs={})
_conv_case("group2", reject="group != 1 not supported", more={"group": "2"})
_conv_case("dilations2", reject="dilations != 1 not supported", more={"dilations": "2,2"})
_conv_case("two_pads_rank4", reject="invalid pads/strides", more={"pads": "1,1"})
_conv_case("kernel_shape_contradicts_weights", reject="kernel_shape does not match the weights", more={"kernel_shape": "3,5"})
_conv_case("auto_pad", reject="unrecognized attribute: auto_pad", more={"auto_pad": "SAME_UPPER"})
_conv_case("dilations_length_contradicts_rank", reject="invalid dilations attribute value", more={"dilations": "1"})
_conv_case("wrong_cin", reject="invalid shape of weights", wshape=(KO, KC // 2, 3, 3))
_conv_case("bias_of_another_length", reject="invalid shape of bias", bshape=(KO - 1,))
_conv_case("batch2", reject="batch size must be 1", sx=(2, KC, KH_, KW_), nhwc=False)
_conv_case("stride0", reject="invalid pads/strides", more={"strides": "0,1"})
# 7 + 2 < 10: (7 + 2 - 10) / 2 truncates to 0 in C, which would plan one output row of a kernel that fits nowhere
_conv_case("kernel_larger_than_padded_input_stride2", k=(10, 3), strides=(2, 1), reject="kernel larger than the padded input")


# ======================================================================================================================================
# An operand without elements against an extent of 1 (support_dynamic_shapes: the declared 0 is a wildcard, so the computed shape is not checked against
# it): the output is empty and nothing is launched.  Stub only.
# ======================================================================================================================================
for kind in KINDS:
    add(f"bin/empty_operand/{kind}", "move",
        (lambda g, kind=kind: g.op("/" + kind, kind, [g.input("x", (1, 2, 0, 4)), g.weight("/e.w", wt("/e_w", (1, 2, 1, 4)), allow_quant=False)], (1, 2, 0, 4),
                                  out_names=["out"])), {"x": (1, 2, 0, 4)}, lambda i: {"out": np.zeros((1, 2, 0, 4))}, dynamic=True)
STUB_ONLY = {c.name for c in CASES if c.name.startswith("bin/empty_operand/")}


# ---- what the reference says about these cases (tools/make_golden_ops.py prints both lists; tests/test_op_lowering_cpu.py checks them where oracle/_ref
# is built) -------------------------------------------------------------------------------------------------------------------------------------------
# case -> a substring of the reference's refusal: restatement-only cases, accepted by the device
REF_REFUSES = {
    "mean/no_attributes": "reduce supported on 1 axis only",
    "matmul/1nMK_nKN": "shape of input 0 must have 3 dimensions",
    "matmul/nMK_1nKN": "shape of input 1 must have 2 or 3 dimensions",
    "matmul/const_rank4_N8": "shape of input 0 must have 3 dimensions",
    "matmul/const_rank4_N5": "shape of input 0 must have 3 dimensions",
    "expand/target1_input4": "input dimension > output dimension",
    "flatten/axis3": "invalid axis attribute",
    "maxpool/no_dilations_attribute": "invalid dilations attribute value",
    # Conv: the reference wants strides[0] == strides[1] and every attribute present; lower_conv takes a stride per axis, applies the ONNX defaults and reads the
    # kernel size from the weights, and skips a bias whose name is empty
    "conv/stride_2_1": "XnnPack::convolution_nhwc_fp32: one or more arguments are invalid",
    "conv/no_pads_strides_kernel_shape": "invalid shape of W or invalid kernel_shape",
    "conv/no_attributes": "invalid dilations attribute value",
    "conv/bias_empty_name": "input tensor not found",
    "conv/conv1d_no_attributes": "invalid dilations attribute value",
}
# case -> note: the reference's form differs from the first restatement in kind; resolved in favour of the reference
REF_DIFFERS = {
    "maxpool/pads0110": "pads that differ between the two sides of a direction: the first restatement (and the lowering) padded as ONNX names them (top, left, "
                        "bottom, right); the reference re-centres them as it does for Conv, top = (top + bottom) / 2 with the odd cell at the bottom, and the same "
                        "from left to right.  The restatement and the lowering follow the reference (also maxpool/pads1001, maxpool/pads2000).",
    "conv/pads_1100": "pads (1,1,0,0): ONNX pads the top and the left; the reference re-centres, top = (1 + 0) / 2 = 0 with the odd cell at the bottom, left = 0 with the "
                      "odd cell at the right -- the same convolution as conv/pads_0011 (the two cases hold different weights, so their outputs differ).  The restatement "
                      "and lower_conv follow the reference (also conv/pads_2000: one cell at the top, one at the bottom; conv/pads_1021; conv/conv1d_pads_20).",
    "slice/two_axes_no_axes": "two starts / ends without an `axes` input: the first restatement (and the lowering) took the last two axes, ONNX would take axes 0 and "
                              "1; the reference slices the LAST axis twice, the second time on the result of the first (its `last_but_one` is only ever set from "
                              "`axes`).  The restatement and the lowering follow the reference.",
}


def runnable():
    """the cases that compute something (not refused here)"""
    return [c for c in CASES if c.cls != "reject"]


def device_cases():
    return [c for c in runnable() if c.name not in STUB_ONLY]


# ---- running a case through the product library (the stub backend where OSGPU_LIB names it, the device otherwise) --------------------------------------
def emit(case, sink):
    from onnxstream_amd.synth.graph import GraphBuilder
    g = GraphBuilder(sink)
    case.build(g)
    g.finish()


def plan_steps(info):
    """the `what` of every step of Model.hip_plan_info()"""
    return [line.split(" | ", 1)[1] for line in info.splitlines() if line.startswith("step ")]


def run_case(case, pushes=1, fusion=2, first=0, options=None, extra_outputs=(), plan=False):
    """pushes samples first .. first + pushes - 1 -> output name -> list of fp32 arrays, one per pushed sample (one only for an output that depends on constants alone); raises
    onnxstream_amd.bindings.OnnxStreamError with the refusal's message.  options: Model options set before the graph is read (hip_fusion_level among them overrides `fusion`);
    extra_outputs: names for add_extra_output; plan: return (outputs, the `what` of every plan step) instead"""
    import tempfile

    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    from onnxstream_amd.synth.graph import DirSink
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        emit(case, DirSink(d))
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        try:
            m._set_option("hip_fusion_level", fusion)
            for name, value in (options or {}).items():
                m._set_option(name, value)
            for name in extra_outputs:
                m.add_extra_output(name)
            if case.dynamic:
                m.set_support_dynamic_shapes(True)
            if case.upcast:
                m.set_upcast_substrings(case.upcast)
            m.read_file(d + "model.txt")
            m.set_use_fp16_arithmetic(True)
            for k in range(pushes):
                for name, arr in case.sample(first + k).items():
                    m.add_tensor(name, arr)
            m.run()
            got = {}
            for o in case.outs:
                res = [m.get_tensor(o, i) for i in range(pushes)]
                got[o] = [r[0] for r in res if r is not None]
            steps = plan_steps(m.hip_plan_info()) if plan else None
        finally:
            m.close()
    return (got, steps) if plan else got


def bits(x):
    """the bit image of fp32 values: equality of these tells -0.0 from 0.0"""
    return np.ascontiguousarray(x, f32).view(np.uint32)


def ulps16(got, want):
    """distance in f16 ulps between got (f16-representable) and the float64 want rounded to f16"""
    def order(h):
        i = h.view(np.uint16).astype(np.int32)
        return np.where(i & 0x8000, -(i & 0x7FFF), i)
    return np.abs(order(np.asarray(got).astype(f16)) - order(np.asarray(want, f64).astype(f16)))


# ---- the figures of one output of one sample, and what its class allows ---------------------------------------------------------------------------------
def ulp16(x):
    """spacing of f16 at |x|, as the kernel-level tests define it"""
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f16)).astype(f64)


def figures(case, o, got, k):
    """-> (figures, failures): `figures` holds `ulps`, the largest distance in f16 ulps to the float64 restatement rounded to f16, and for a "reduce" case `ratio`,
    the largest error / bound of its kernel-level bound; `failures` lists what the case's class does not allow (empty: the output passes)"""
    w = case.want(k)
    want = w[o]
    if got.shape != want.shape:
        return {}, [f"shape {got.shape}, restated {want.shape}"]
    if got.size == 0:
        return {"ulps": 0}, []
    fig, bad = {"ulps": int(ulps16(got, want).max())}, []
    g = got.astype(f64)
    if not np.isfinite(g).all():
        bad.append("not finite")
    if case.cls == "move":
        if not np.array_equal(bits(got), bits(want)):
            bad.append(f"not the restatement bit for bit ({int((bits(got) != bits(want)).sum())} of {got.size} elements differ)")
    elif case.cls == "elementwise":
        if fig["ulps"] > 1:
            bad.append(f"{fig['ulps']} f16 ulps from the correctly rounded float64 value")
        if o + "@f32" in w and not np.array_equal(bits(got), bits(w[o + "@f32"].astype(f32))):
            bad.append("not numpy's f32 operation rounded once")
    else:
        err = np.abs(g - want)
        if case.bound in ("mean_f16", "rms_chain"):
            bound = ulp16(want)
        elif case.bound == "softmax_f16":
            bound = ulp16(want) + 2.0 ** -11
        elif case.bound == "contraction":
            E = (int(w[o + "@K"]) + 3) * 2.0 ** -24 * w[o + "@S"]
            bound = 2.0 ** -11 * np.abs(want) + (1 + 2.0 ** -11) * E + 2.0 ** -25
            fig["far"] = float((ulps16(got, want) > 1).mean())
            if fig["far"] > 0.02:
                bad.append(f"{fig['far']:.3f} of the elements more than one f16 ulp from the correctly rounded value")
        else:
            assert case.bound == "instance_norm"
            from test_unet_attention_norm import norm_exact          # the bound of the kernel-level test itself
            x = r16(case.sample(k)["x"])[0]
            L = x.shape[-1]
            want2, bound = norm_exact(x, case.extra["gamma"].astype(f64)[:, None], case.extra["beta"].astype(f64)[:, None], float(f32(1e-5)), -(-L // 256) + 24,
                                      False, 0, f16)
            assert np.allclose(want2[None], want, rtol=1e-12, atol=1e-12)
            bound = bound[None]
        fig["ratio"] = float((err / bound).max())
        if fig["ratio"] > 1.0:
            bad.append(f"error / bound {fig['ratio']:.3f} ({case.bound})")
    return fig, bad


_GOLDEN = None


def golden(case, o):
    """(ref16, ref32) of sample 0 from tests/golden/op_cases.npz, or None for a case the reference refuses"""
    global _GOLDEN
    import os
    if _GOLDEN is None:
        _GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_cases.npz"))
    if case.name in REF_REFUSES:
        return None
    return _GOLDEN[f"{case.name}|{o}|ref16"].astype(f32), _GOLDEN[f"{case.name}|{o}|ref32"]


def err16(got, ref16, ref32):
    """the single-pattern figure of tests/test_golden.py: max|got - ref16| / max|ref32|"""
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(f64) - ref16)
    d = np.where(bits(got) == bits(ref16), 0.0, d)            # (inf - inf)
    return float(d.max()) / float(np.abs(ref32).max())
