"""The case table of the graph-fusion tests (tests/test_fusion_cases_cpu.py on the stub backend, tests/test_fusion_cases_gpu.py on the device,
tools/make_golden_fusion.py for the reference's outputs in tests/golden/fusion_cases.npz).  It sits between the kernel tables and tests/op_cases.py
(one operator each): one case = one small graph aimed at ONE rewrite of run_fusions() (csrc/host/lowering_graph.inc) or one of the two lowering-time
merges (plan_linear_groups, the LayerNorm fold), in a form the project's own exporter never writes.

A case's `body(w)` writes the graph op by op through the writer W below.  W hands every op to GraphBuilder.op(...) AND evaluates it in float64 numpy on
the spot, so the graph as written and its restatement are one description: `ref(i)` is that evaluation on the f16-rounded inputs, nothing is rounded in
between.  No layer helper of GraphBuilder (group_norm, layer_norm) or of synth/sd_unet.py is used: the forms here are the ones they never emit.

  pass_    the rewrite the case aims at (the name of the function in lowering_graph.inc / lowering_ops.inc)
  expect   "fires"    the pass must take the graph
           "left"     the pass must leave it: the ops survive (`plan` names them)
           "partial"  a weaker rewrite is right (AttentionFusedOps instead of osg.Attention, GroupNorm without the SiLU, ...)
           "extra"    the positive form with an interior tensor of the pattern asked for through add_extra_output: the pass leaves the pattern or keeps that
                      tensor right; it never returns None or stale bytes
  plan     the arithmetic step kinds (first word of `what` in Model.hip_plan_info, data movement left out: MOVES) of the fusion level 2 plan
  fused    a substring of a step's `what` that shows the (full) rewrite: in the level 2 plan for "fires", not in it for "left" and "partial"; `present` / `absent` add
           further substrings (the weaker rewrite of a "partial" case).  An epilogue fusion leaves no mark in `what`: there the missing Add / osg.SiLU step of `plan` is the mark
  wrong    for "left" / "partial": body of the graph the FORBIDDEN rewrite would compute (the residual dropped, the activation after the bias, the heads
           interleaved, ...), or output name -> "unwritten" for a tensor the rewrite would delete.  tests/test_fusion_cases_cpu.py asserts that it is more
           than 50 tolerances away from `ref` on at least half of the elements, so a device pass cannot hide the defect.  Where the forbidden rewrite would
           compute the SAME values (a guard on the number of readers, on an operand's rank) or differs below f16 resolution, `why` says so and the case is
           held on plan structure.
  opts     Model options of the case; extra: names for add_extra_output; upcast: substrings for set_upcast_substrings
  refuse   the message with which the lowering refuses the graph at EVERY level (a near miss built on an operator form the lowering does not take: the pass
           must not swallow it either)
  rule     every output of every case is held to the single-pattern rule of tests/test_golden.py, max|got - ref16| / max|ref32| <= 1e-3 (also the tolerance of the `wrong`
           check).  Where `out` is ONE launch of a class the kernel tests name, at the levels in `cls_levels`, it is ALSO held to that class's rule against the float64
           restatement, which sees the small elements that a rule relative to the maximum cannot:
             "elementwise"  within one f16 ulp (op_cases.figures)
             "contraction"  op_cases.figures' contraction bound; K and S = |a| . |w| + |bias| + |residual| come from the writer (the addends are exact in front of the one rounding)
             "rms_chain"    within one f16 ulp (op_cases.BOUNDS)
             "group_norm"   tests/test_unet_attention_norm.py::test_group_norm: norm_exact(x, gamma, beta, eps, 24, one-pass, silu) -- the one-block kernel takes these shapes
                            (8 channels per group), its longest chain of additions is NV + 16 with NV <= 8
             "layer_norm"   tests/test_unet_attention_norm.py::test_layer_norm: norm_exact(x, gamma, beta, eps, ceil(C / 256) + 12, two-pass)
           `norm` holds gamma, beta, eps, act for the last two.
"""
import math

import numpy as np

import op_cases as oc
from op_cases import f16, f32, f64, r16, rnd, pos, wt, _seed

# (to_nhwc / to_nchw: layout changes; upcast / downcast: f16 <-> f32 conversions of the upcast chain; Softmax/T0, /T1: the transposes around a Softmax over another axis)
MOVES = {"input", "output", "to_nhwc", "to_nchw", "upcast", "downcast", "Softmax/T0", "Softmax/T1", "Transpose", "Copy", "Concat", "Slice", "Reshape", "Unsqueeze", "Squeeze", "Gather", "Split", "Resize", "KVPack", "Expand"}
SQRT2_F32 = float(f32(math.sqrt(2.0)))


# ======================================================================================================================================
# the writer: one call = one op in model.txt + its float64 value
# ======================================================================================================================================
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _conv(x, wgt, b, pads, strides):
    if x.ndim == 3:                                                   # Conv1D: [1,C,L] with a [O,I,k,1] filter bank
        return _conv(x[..., None], wgt, b, (pads[0], 0, pads[1], 0), (strides[0], strides[0]))[..., 0]
    O, I, kh, kw = wgt.shape
    ph, pw = pads[0] + pads[2], pads[1] + pads[3]                      # re-centred, the reference's form (op_cases.REF_DIFFERS, conv/pads_1100)
    xp = np.pad(x, ((0, 0), (0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2)))
    Ho, Wo = (xp.shape[2] - kh) // strides[0] + 1, (xp.shape[3] - kw) // strides[1] + 1
    out = np.zeros((x.shape[0], O, Ho, Wo))
    for dy in range(kh):
        for dx in range(kw):
            out += np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + strides[0] * Ho:strides[0], dx:dx + strides[1] * Wo:strides[1]], wgt[:, :, dy, dx])
    return out if b is None else out + b[None, :, None, None]


def _ints(s):
    return [int(v) for v in str(s).split(",")]


def _np_op(typ, v, a):
    """float64 numpy semantics of one ONNX op as the reference reads it; v: operand values (int64 arrays for shape operands), a: attributes"""
    if typ in ("Add", "Sub", "Mul", "Div"):
        return oc.KINDS[typ](v[0], v[1])
    if typ == "Pow":
        return np.power(v[0], v[1])
    if typ in oc.UNARY:
        return oc.UNARY[typ](v[0])
    if typ == "MatMul":
        return v[0] @ v[1]
    if typ == "Gemm":
        return v[0] @ v[1] + (v[2] if len(v) > 2 else 0.0)
    if typ == "Softmax":
        return _softmax(v[0], int(a.get("axis", -1)))
    if typ == "ReduceMean":
        return v[0].mean(axis=tuple(_ints(a["axes"])), keepdims=bool(int(a.get("keepdims", 1))))
    if typ == "Reshape":
        tgt = [v[0].shape[k] if d == 0 else int(d) for k, d in enumerate(v[1])]
        return v[0].reshape(tgt)
    if typ == "Transpose":
        return v[0].transpose(_ints(a["perm"]))
    if typ == "Unsqueeze":
        out = v[0]
        for ax in sorted(int(x) for x in v[1]):
            out = np.expand_dims(out, ax)
        return out
    if typ == "Slice":
        ax = int(v[3][0]) if len(v) > 3 else -1
        sl = [slice(None)] * v[0].ndim
        sl[ax] = slice(int(v[1][0]), min(int(v[2][0]), v[0].shape[ax]))
        return v[0][tuple(sl)]
    if typ == "Concat":
        return np.concatenate(v, int(a["axis"]))
    if typ == "InstanceNormalization":
        x = v[0]
        mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + float(f32(float(a.get("epsilon", 1e-5))))) * v[1][None, :, None] + v[2][None, :, None]
    if typ == "Conv":
        k = len(_ints(a["kernel_shape"]))
        return _conv(v[0], v[1], v[2] if len(v) > 2 else None, _ints(a.get("pads", "0,0,0,0" if k == 2 else "0,0")), _ints(a.get("strides", "1,1" if k == 2 else "1")))
    raise KeyError(typ)


class W:
    def __init__(self, g, i):
        self.g, self.i, self.val = g, i, {}
        self.SK = {}               # tensor name -> (S, K) of the contraction launch that writes it: S = |a| . |w| + |bias| + |residual|, K its contraction length (op_cases' bound)

    def inp(self, name, shape):
        t = self.g.input(name, shape)
        self.val[t.name] = np.asarray(self.i[name], f64).reshape(shape)
        return t

    def c(self, name, arr, dtype=None, conv=False):
        """a float weight: the operator sees its f16 rounding under fp16 arithmetic (InstanceNormalization's operands, kept f32, hold f16-exact values here)"""
        arr = np.asarray(arr, f32)
        t = self.g.weight(name, arr, dtype=dtype, conv=conv, allow_quant=False)
        self.val[t.name] = r16(arr)
        return t

    def s(self, name, val, dtype=None):
        return self.c(name, np.asarray(val, f32).reshape(()), dtype)

    def i64(self, name, vals):
        t = self.g.weight(name, np.asarray(vals, np.int64), dtype="int64")
        self.val[t.name] = np.asarray(vals, np.int64)
        return t

    def op(self, name, typ, ins, attrs=None, out=None):
        attrs = {k: str(v) for k, v in (attrs or {}).items()}
        v = _np_op(typ, [self.val[t.name] for t in ins], attrs)
        t = self.g.op(name, typ, ins, v.shape if v.shape else [()], attrs or None, out_names=[out] if out else None)
        t = t if v.shape else t[0]
        self.val[t.name] = v
        if typ in ("MatMul", "Gemm", "Conv"):
            wv = self.val[ins[1].name]
            self.SK[t.name] = (_np_op(typ, [np.abs(self.val[x.name]) for x in ins], attrs), int(np.prod(wv.shape[1:])) if typ == "Conv" else int(wv.shape[0]))
        elif typ == "Add" and sum(x.name in self.SK for x in ins) == 1:          # a bias, a residual or a per-image bias: an exact addend in front of the one rounding
            k = 0 if ins[0].name in self.SK else 1
            self.SK[t.name] = (self.SK[ins[k].name][0] + np.abs(self.val[ins[1 - k].name]), self.SK[ins[k].name][1])
        return t

    # single ops with their constant operand
    def reshape(self, name, x, shape, out=None):
        return self.op(name, "Reshape", [x, self.i64(name + ".shape", shape)], {"allowzero": 0}, out)

    def transpose(self, name, x, perm, out=None):
        return self.op(name, "Transpose", [x], {"perm": ",".join(map(str, perm))}, out)

    def unsqueeze(self, name, x, axis):
        return self.op(name, "Unsqueeze", [x, self.i64(name + ".axes", [axis])])

    def slice_last(self, name, x, a, b):
        return self.op(name, "Slice", [x, self.i64(name + ".starts", [a]), self.i64(name + ".ends", [b]), self.i64(name + ".axes", [-1]), self.i64(name + ".steps", [1])])


RULES = {"elementwise": ("elementwise", None), "contraction": ("reduce", "contraction"), "rms_chain": ("reduce", "rms_chain"), "group_norm": None, "layer_norm": None}


class FCase(oc.Case):
    def __init__(self, name, pass_, expect, body, inputs, outs=("out",), plan=None, fused=None, wrong=None, why=None, opts=None, extra=(), upcast=None, refuse=None,
                 rule=None, cls_levels=(), plan_low=None, present=(), absent=(), wrong_outs=None, norm=None):
        assert expect in ("fires", "left", "partial", "extra") and (rule is None or (rule in RULES and cls_levels)), name
        assert expect not in ("left", "partial") or wrong is not None or why or refuse, name
        oc.Case.__init__(self, name, "chain", self._emit, inputs, self._ref, outs=tuple(outs) + tuple(extra), upcast=upcast, stub_values=False, extra=norm)
        self.pass_, self.expect, self.body, self.plan, self.fused, self.wrong, self.why = pass_, expect, body, plan, fused, wrong, why
        self.wrong_outs = wrong_outs               # the outputs the forbidden rewrite would change (default: every output its body writes)
        self.present = tuple(present) + ((fused,) if fused and expect == "fires" else ())
        self.absent = tuple(absent) + ((fused,) if fused and expect in ("left", "partial") else ())
        self.opts, self.extra_outs, self.refuse, self.rule, self.cls_levels, self.plan_low = dict(opts or {}), tuple(extra), refuse, rule, tuple(cls_levels), plan_low

    def _run(self, body, g, i):
        w = W(g, i)
        named = body(w) or {}
        return w, named

    def _emit(self, g):
        self._run(self.body, g, {n: r16(v) for n, v in self.sample(0).items()})

    def _ref(self, i, body=None):
        from onnxstream_amd.synth.graph import GraphBuilder, MemSink, mangle
        w, _ = self._run(body or self.body, GraphBuilder(MemSink()), i)
        out = {o: np.asarray(w.val[mangle(o)], f64) for o in self.outs if mangle(o) in w.val}
        for o in self.outs:
            if mangle(o) in w.SK:
                out[o + "@S"], out[o + "@K"] = w.SK[mangle(o)][0], np.asarray(w.SK[mangle(o)][1])
        return out

    def wrong_values(self, k=0):
        """output name -> float64 value of the forbidden rewrite (zeros for a tensor it would leave unwritten)"""
        i = {n: r16(v) for n, v in self.sample(k).items()}
        if callable(self.wrong):
            return {o: v for o, v in self._ref(i, self.wrong).items() if "@" not in o and (self.wrong_outs is None or o in self.wrong_outs)}
        want = self.ref(i)
        return {o: np.zeros_like(want[o]) for o, v in self.wrong.items() if v == "unwritten"}

    def as_class(self):
        """the view of this case that op_cases.figures judges at the levels where `out` is one launch of a class it names"""
        import copy
        c = copy.copy(self)
        c.cls, c.bound = RULES[self.rule]
        return c


CASES = []


def add(*a, **k):
    c = FCase(*a, **k)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)


def by_name(name):
    return next(c for c in CASES if c.name == name)


# shapes: the smallest the kernels take
T, C, H, D = 16, 64, 2, 32
XS = (1, T, C)
IMG = (1, C, 8, 8)          # what a convolution reads: 64 channels on 8 x 8
CO = 16                     # ... and writes: 16 channels, so that a recorded output is 1024 values
OIMG = (1, CO, 8, 8)
GIMG = (1, C, 4, 4)         # what a GroupNorm of 8 groups reads


def lw(name, shape, scale):
    """a weight of magnitudes scale * [0.25, 4], f16-exact (scale a power of two)"""
    return wt(name, shape) * f32(scale)


def near1(name, shape):
    return (1.0 + wt(name, shape) / 16).astype(f16).astype(f32)


# ======================================================================================================================================
# fuse_silu
# ======================================================================================================================================
def _silu(w, x, nm="/act", order="xs", y=None, out=None):
    s = w.op(nm + "/Sigmoid", "Sigmoid", [x])
    a = y if y is not None else x
    return w.op(nm + "/Mul", "Mul", [a, s] if order == "xs" else [s, a], out=out)


def _normal(name, shape, scale=1.5, shift=-0.3):
    """normal values, as activations have them: few elements sit in the binade of the largest one (where one f16 ulp is up to 9.8e-4 of it)"""
    return lambda k: (scale * np.random.default_rng(_seed(name) + k).standard_normal(shape) + shift).astype(f32)


SX, SXY = {"x": _normal("silu_x", XS)}, {"x": _normal("silu_x", XS), "y": _normal("silu_y", XS)}
for order in ("xs", "sx"):
    add(f"silu/{order}", "fuse_silu", "fires", (lambda w, order=order: _silu(w, w.inp("x", XS), order=order, out="out")), SX, plan=["osg.SiLU"], fused="osg.SiLU",
        rule="elementwise", cls_levels=(1, 2))


def _silu_extra(w):
    x = w.inp("x", XS)
    s = w.op("/act/Sigmoid", "Sigmoid", [x], out="sig")
    w.op("/act/Mul", "Mul", [x, s], out="out")


add("silu/sigmoid_is_extra_output", "fuse_silu", "extra", _silu_extra, SX, extra=("sig",), plan=["Sigmoid", "Mul"])
add("silu/mul_of_another_tensor", "fuse_silu", "left", (lambda w: _silu(w, w.inp("x", XS), y=w.inp("y", XS), out="out")), SXY, plan=["Sigmoid", "Mul"], fused="osg.SiLU",
    wrong=lambda w: _silu(w, w.inp("x", XS), out="out"))


def _silu_sig_twice(w):
    x = w.inp("x", XS)
    s = w.op("/act/Sigmoid", "Sigmoid", [x])
    w.op("/act/Mul", "Mul", [x, s], out="out")
    w.op("/other/Neg", "Neg", [s], out="neg")


add("silu/sigmoid_read_twice", "fuse_silu", "left", _silu_sig_twice, SX, outs=("out", "neg"), plan=["Sigmoid", "Mul", "Neg"], fused="osg.SiLU", wrong={"neg": "unwritten"})


def _silu_sig_sig(w, wrong=False):
    x = w.inp("x", XS)
    s = w.op("/act/Sigmoid", "Sigmoid", [x])
    w.op("/act/Mul", "Mul", [x if wrong else s, s], out="out")


add("silu/sigmoid_times_itself", "fuse_silu", "left", _silu_sig_sig, SX, plan=["Sigmoid", "Mul"], fused="osg.SiLU", wrong=lambda w: _silu_sig_sig(w, True))


# ======================================================================================================================================
# fuse_group_norm: Reshape[1,G,L] -> InstanceNormalization(1, 0) -> Reshape[x.shape] -> Mul(gamma) -> Add(beta) [-> SiLU]
# ======================================================================================================================================
GG = 8
GX = {"x": _normal("gn_x", GIMG, 2.0, 0.5)}
GN_G, GN_B = near1("/gn_g", (C,)), wt("/gn_b", (C,)) / 16


def _gn(w, x=None, gshape=(C, 1, 1), order="xg", eps=1e-5, silu=False, scale=1.0, bias=0.0, shape2=None, gamma=None, mul_twice=False, r0_twice=False, add_twice=False,
        out="out", nm="/gn", extra_name=None, xshape=GIMG):
    x = x if x is not None else w.inp("x", xshape)
    n, Cc = int(np.prod(xshape)), xshape[1]
    gshape = tuple(Cc if d == C else d for d in gshape)
    r0 = w.reshape(nm + "/Reshape", x, (1, GG, n // GG))
    i = w.op(nm + "/InstanceNormalization", "InstanceNormalization",
             [r0, w.c(nm + ".in_scale", np.full((GG,), scale), "float32"), w.c(nm + ".in_bias", np.full((GG,), bias), "float32")], None if eps is None else {"epsilon": repr(eps)})
    r1 = w.reshape(nm + "/Reshape_1", i, shape2 or xshape, out=extra_name)
    g = w.c(nm + ".weight", (GN_G[:Cc] if gamma is None else gamma).reshape(gshape))
    b = w.c(nm + ".bias", GN_B[:Cc].reshape(gshape if gamma is None else (Cc, 1, 1)))
    last = not (silu or add_twice)
    m = w.op(nm + "/Mul", "Mul", [r1, g] if order == "xg" else [g, r1])
    a = w.op(nm + "/Add", "Add", [m, b] if order == "xg" else [b, m], out=out if last else None)
    if mul_twice:
        w.op("/other/Neg", "Neg", [m], out="neg")
    if r0_twice:
        w.op("/other/Neg", "Neg", [r0], out="neg")
    if add_twice:
        w.op("/other/Neg", "Neg", [a], out="neg")
    if silu or add_twice:
        a = _silu(w, a, out=out)
    return a


for gs, gn in (((C, 1, 1), "c11"), ((1, C, 1, 1), "1c11")):
    for order in ("xg", "gx"):
        add(f"group_norm/{gn}/{order}", "fuse_group_norm", "fires", (lambda w, gs=gs, order=order: _gn(w, gshape=gs, order=order)), GX, plan=["GroupNorm"], fused="GroupNorm",
            rule="group_norm", cls_levels=(1, 2), norm=dict(gamma=GN_G, beta=GN_B, eps=f32(1e-5), act=0))
add("group_norm/silu", "fuse_group_norm", "fires", (lambda w: _gn(w, silu=True)), GX, plan=["GroupNorm"], fused="GroupNorm", rule="group_norm", cls_levels=(1, 2), norm=dict(gamma=GN_G, beta=GN_B, eps=f32(1e-5), act=1))                      # (one launch: the SiLU rides in it)
add("group_norm/no_epsilon_attribute", "fuse_group_norm", "fires", (lambda w: _gn(w, eps=None)), GX, plan=["GroupNorm"], fused="GroupNorm",
    rule="group_norm", cls_levels=(1, 2), norm=dict(gamma=GN_G, beta=GN_B, eps=f32(1e-5), act=0))
add("group_norm/epsilon_1e-6", "fuse_group_norm", "fires", (lambda w: _gn(w, eps=1e-6)), GX, plan=["GroupNorm"], fused="GroupNorm",
    rule="group_norm", cls_levels=(1, 2), norm=dict(gamma=GN_G, beta=GN_B, eps=f32(1e-6), act=0))
add("group_norm/reshape_is_extra_output", "fuse_group_norm", "extra", (lambda w: _gn(w, extra_name="normed")), GX, extra=("normed",),
    plan=["InstanceNorm", "Mul", "Add"])
add("group_norm/in_scale_2", "fuse_group_norm", "left", (lambda w: _gn(w, scale=2.0)), GX, plan=["InstanceNorm", "Mul", "Add"], fused="GroupNorm",
    wrong=lambda w: _gn(w))
add("group_norm/in_bias_2", "fuse_group_norm", "left", (lambda w: _gn(w, bias=2.0)), GX, plan=["InstanceNorm", "Mul", "Add"], fused="GroupNorm",
    wrong=lambda w: _gn(w))
add("group_norm/second_reshape_to_another_shape", "fuse_group_norm", "left", (lambda w: _gn(w, shape2=(1, C, 2, 8))), GX, plan=["InstanceNorm", "Mul", "Add"],
    fused="GroupNorm", why="per-channel gamma / beta apply the same way to [1,C,2,8]: the rewrite would compute these values under x's shape [1,C,4,4], which the "
                           "declared output shape refuses; a guard on the shape, held on plan structure")
GN_HW = near1("/gn_hw", (CO,)) * np.where(np.arange(CO) % 2, f32(2), f32(0.5))
HWIMG = (1, CO, 4, 4)       # H * W == C: a [1,1,H,W] operand has C elements and is NOT per-channel
add("group_norm/gamma_11HW_with_HW_eq_C", "fuse_group_norm", "left", (lambda w: _gn(w, gshape=(1, 1, 4, 4), gamma=GN_HW, xshape=HWIMG)), {"x": _normal("gn_xhw", HWIMG, 2.0, 0.5)}, plan=["InstanceNorm", "Mul", "Add"],
    fused="GroupNorm", wrong=lambda w: _gn(w, gshape=(CO, 1, 1), gamma=GN_HW, xshape=HWIMG))          # (the rewrite would take the C values per channel)
add("group_norm/mul_read_twice", "fuse_group_norm", "left", (lambda w: _gn(w, mul_twice=True)), GX, outs=("out", "neg"), plan=["InstanceNorm", "Mul", "Add", "Neg"],
    fused="GroupNorm", wrong={"neg": "unwritten"})
add("group_norm/first_reshape_read_twice", "fuse_group_norm", "left", (lambda w: _gn(w, r0_twice=True)), GX, outs=("out", "neg"),
    plan=["InstanceNorm", "Mul", "Add", "Neg"], fused="GroupNorm", wrong={"neg": "unwritten"})
add("group_norm/add_read_by_silu_and_another", "fuse_group_norm", "partial", (lambda w: _gn(w, add_twice=True)), GX, outs=("out", "neg"), plan=["GroupNorm", "Neg", "osg.SiLU"],
    present=("GroupNorm", "osg.SiLU"), wrong={"neg": "unwritten"})


# ======================================================================================================================================
# fuse_layer_norm: ReduceMean -> Sub -> Pow(2) -> ReduceMean -> Add(eps) -> Sqrt -> Div -> Mul(gamma) -> Add(beta)
# ======================================================================================================================================
LN_G, LN_B = near1("/ln_g", (C,)), wt("/ln_b", (C,)) / 16
RED = {"axes": -1, "keepdims": 1}


def _ln(w, x=None, eps_first=False, gorder="dg", border="mb", p=2.0, sub_swapped=False, red1=None, red2=None, div_swapped=False, third_reader=False, gshape=(C,), gamma=None,
        out="out", nm="/ln", xshape=XS, extra_name=None, eps=1e-5, beta=None):
    x = x if x is not None else w.inp("x", xshape)
    mean = w.op(nm + "/ReduceMean", "ReduceMean", [x], red1 or RED)
    d = w.op(nm + "/Sub", "Sub", [mean, x] if sub_swapped else [x, mean], out=extra_name)
    pw = w.op(nm + "/Pow", "Pow", [d, w.s(nm + ".pow_exp", p)])
    var = w.op(nm + "/ReduceMean_1", "ReduceMean", [pw], red2 or RED)
    e = w.s(nm + ".eps", eps)
    ve = w.op(nm + "/Add", "Add", [e, var] if eps_first else [var, e])
    sd = w.op(nm + "/Sqrt", "Sqrt", [ve])
    q = w.op(nm + "/Div", "Div", [sd, d] if div_swapped else [d, sd])
    g = w.c(nm + ".weight", (LN_G if gamma is None else gamma).reshape(gshape))
    b = w.c(nm + ".bias", LN_B if beta is None else beta)
    m = w.op(nm + "/Mul", "Mul", [q, g] if gorder == "dg" else [g, q])
    a = w.op(nm + "/Add_1", "Add", [m, b] if border == "mb" else [b, m], out=out)
    if third_reader:
        w.op("/other/Neg", "Neg", [d], out="neg")
    return a


def _x_pm(lo, hi, name, shape=XS):
    """magnitudes in [lo, hi], either sign: x - mean stays away from 0"""
    def gen(k):
        rng = np.random.default_rng(_seed(name) + k)
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(lo, hi, shape)).astype(f32)
    return gen


def _x_skew(name, shape=XS):
    """log-normal rows: the third central moment is positive, so Sqrt(mean((x - m)^3) + eps) is real"""
    return lambda k: (4 * np.exp(0.5 * np.random.default_rng(_seed(name) + k).standard_normal(shape))).astype(f32)


def _x_normal(name, shape=XS):
    """normal rows, as an activation in front of a LayerNorm has them (tests/golden_cases.layer_norm): few elements sit near the largest one"""
    return lambda k: (1.5 * np.random.default_rng(_seed(name) + k).standard_normal(shape) - 0.3).astype(f32)


LNX = {"x": _x_normal("ln_x")}
LN_RULE = dict(rule="layer_norm", cls_levels=(1, 2), norm=dict(gamma=LN_G, beta=LN_B, eps=float(f16(1e-5)), act=0))      # (eps: the f16 the Add's constant holds)


add("layer_norm/nine_ops", "fuse_layer_norm", "fires", (lambda w: _ln(w)), LNX, plan=["LayerNorm"], fused="LayerNorm", **LN_RULE)
add("layer_norm/eps_first", "fuse_layer_norm", "fires", (lambda w: _ln(w, eps_first=True)), LNX, plan=["LayerNorm"], fused="LayerNorm", **LN_RULE)
add("layer_norm/gamma_first", "fuse_layer_norm", "fires", (lambda w: _ln(w, gorder="gd")), LNX, plan=["LayerNorm"], fused="LayerNorm", **LN_RULE)
add("layer_norm/beta_first", "fuse_layer_norm", "fires", (lambda w: _ln(w, border="bm")), LNX, plan=["LayerNorm"], fused="LayerNorm", **LN_RULE)
add("layer_norm/centred_is_extra_output", "fuse_layer_norm", "extra", (lambda w: _ln(w, extra_name="centred")), LNX, extra=("centred",),
    plan=["ReduceMean", "Sub", "Pow", "ReduceMean", "Add", "Sqrt", "Div", "Mul", "Add"])
LN_OPS = ["ReduceMean", "Sub", "Pow", "ReduceMean", "Add", "Sqrt", "Div", "Mul", "Add"]
add("layer_norm/pow_3", "fuse_layer_norm", "left", (lambda w: _ln(w, p=3.0)), {"x": _x_skew("ln3")}, plan=LN_OPS, fused="LayerNorm", wrong=lambda w: _ln(w))
add("layer_norm/sub_mean_minus_x", "fuse_layer_norm", "left", (lambda w: _ln(w, sub_swapped=True)), LNX, plan=LN_OPS, fused="LayerNorm", wrong=lambda w: _ln(w))
add("layer_norm/first_mean_over_axis_1", "fuse_layer_norm", "left", (lambda w: _ln(w, red1={"axes": 1, "keepdims": 1})), LNX, fused="LayerNorm",
    refuse="reduction supported on the last axis only")
add("layer_norm/keepdims_0", "fuse_layer_norm", "left", (lambda w: _ln(w, red1={"axes": -1, "keepdims": 0}, red2={"axes": -1, "keepdims": 0}, xshape=(C,))), {"x": (C,)}, fused="LayerNorm", refuse="keepdims must be 1")
add("layer_norm/second_mean_over_axis_1", "fuse_layer_norm", "left", (lambda w: _ln(w, red2={"axes": 1, "keepdims": 1})), LNX, fused="LayerNorm",
    refuse="reduction supported on the last axis only")
add("layer_norm/div_sqrt_by_centred", "fuse_layer_norm", "left", (lambda w: _ln(w, div_swapped=True)), {"x": _x_pm(1.0, 2.0, "lndiv")}, plan=LN_OPS, fused="LayerNorm",
    wrong=lambda w: _ln(w))
add("layer_norm/centred_read_three_times", "fuse_layer_norm", "left", (lambda w: _ln(w, third_reader=True)), LNX, outs=("out", "neg"), plan=LN_OPS + ["Neg"], fused="LayerNorm",
    wrong={"neg": "unwritten"})
LN_GT = near1("/ln_gt", (C,)) * np.asarray([1, -1, 2, -2], f32)[np.arange(C) % 4]        # (four levels: a row's gain differs from its column's on 3 / 4 of the elements)
add("layer_norm/gamma_T1_with_T_eq_C", "fuse_layer_norm", "left", (lambda w: _ln(w, gshape=(C, 1), gamma=LN_GT, xshape=(1, C, C))), {"x": _x_normal("ln_xcc", (1, C, C))}, plan=LN_OPS, fused="LayerNorm",
    wrong=lambda w: _ln(w, gamma=LN_GT, xshape=(1, C, C)))


# ======================================================================================================================================
# fuse_geglu: p -> Slice(0:C) = value, Slice(C:2C) = gate; value * (0.5 * gate * (1 + Erf(gate / sqrt 2)))
# ======================================================================================================================================
PS = (1, T, 2 * C)


def _geglu(w, p=None, div=SQRT2_F32, div_dtype="float32", swapped=False, one=1.0, half=0.5, cut=(0, C, C, 2 * C), third_reader=False, out="out", nm="/ff", extra_name=None):
    p = p if p is not None else w.inp("p", PS)
    a, b = w.slice_last(nm + "/Slice", p, cut[0], cut[1]), w.slice_last(nm + "/Slice_1", p, cut[2], cut[3])
    val, gate = (b, a) if swapped else (a, b)
    d = w.op(nm + "/Div", "Div", [gate, w.s(nm + ".sqrt2", div, div_dtype)])
    e = w.op(nm + "/Erf", "Erf", [d], out=extra_name)
    s = w.op(nm + "/Add", "Add", [e, w.s(nm + ".one", one)])
    m = w.op(nm + "/Mul", "Mul", [gate, s])
    m = w.op(nm + "/Mul_1", "Mul", [m, w.s(nm + ".half", half)])
    y = w.op(nm + "/Mul_2", "Mul", [val, m], out=out)
    if third_reader:
        w.op("/other/Neg", "Neg", [p], out="neg")
    return y


def _p_neg_pos(k):
    """value half in -[1, 2], gate half in [1, 2]: value * gelu(gate) is large everywhere, gate * gelu(value) small"""
    m = np.random.default_rng(_seed("geglu_np") + k).uniform(1.0, 2.0, PS).astype(f32)
    m[..., :C] *= -1
    return m


def _p_pos_neg(k):
    return -_p_neg_pos(k)


GE_OPS = ["Div", "Erf", "Add", "Mul", "Mul", "Mul"]
add("geglu/sqrt2_f32", "fuse_geglu", "fires", (lambda w: _geglu(w)), {"p": PS}, plan=["GEGLU"], fused="GEGLU")
add("geglu/sqrt2_f16", "fuse_geglu", "fires", (lambda w: _geglu(w, div=1.4140625, div_dtype="float16")), {"p": PS}, plan=["GEGLU"], fused="GEGLU")
add("geglu/erf_is_extra_output", "fuse_geglu", "extra", (lambda w: _geglu(w, extra_name="erf")), {"p": PS}, extra=("erf",), plan=GE_OPS)
add("geglu/halves_swapped", "fuse_geglu", "left", (lambda w: _geglu(w, swapped=True)), {"p": _p_pos_neg}, plan=GE_OPS, fused="GEGLU", wrong=lambda w: _geglu(w))
add("geglu/add_2", "fuse_geglu", "left", (lambda w: _geglu(w, one=2.0)), {"p": _p_neg_pos}, plan=GE_OPS, fused="GEGLU", wrong=lambda w: _geglu(w))
add("geglu/mul_0.25", "fuse_geglu", "left", (lambda w: _geglu(w, half=0.25)), {"p": _p_neg_pos}, plan=GE_OPS, fused="GEGLU", wrong=lambda w: _geglu(w))
add("geglu/slices_do_not_meet", "fuse_geglu", "left", (lambda w: _geglu(w, cut=(0, C - 8, C + 8, 2 * C))), {"p": PS}, plan=GE_OPS, fused="GEGLU",
    why="the rewrite would write [1,T,C] where the graph declares [1,T,C-8]: refused by the declared shape; held on plan structure")
for dv in (1.413, 1.416):
    add(f"geglu/divisor_{dv}", "fuse_geglu", "left", (lambda w, dv=dv: _geglu(w, div=dv)), {"p": PS}, plan=GE_OPS, fused="GEGLU",
        why="another function than the exact GELU, but d/dc [x/2 erf(x/c)] (c - sqrt 2) stays below 2.6e-4 |gelu(x)| at every x: under half an f16 ulp, so no "
            "f16 output can show it; held on plan structure")
add("geglu/projection_read_three_times", "fuse_geglu", "left", (lambda w: _geglu(w, third_reader=True)), {"p": PS}, outs=("out", "neg"), plan=GE_OPS + ["Neg"], fused="GEGLU",
    why="a guard on the readers of the projection: the rewrite reads the same tensor, computes the same values and deletes nothing the third reader needs (the projection "
        "is the pattern's input); held on plan structure")


# ======================================================================================================================================
# fuse_attention(true): the UNet form, heads 2 x 32.  fuse_attention(false) is the same score chain under fuse_ops_in_attention at level < 2
# ======================================================================================================================================
# The attention inputs are chosen so that the reference's own f16 chain stays well inside the single-pattern rule AND a wrong head / token order shows:
#   * x is positive and WV = (s_h + r) / 128 with s_h = +1 for the columns of head 0, -1 for head 1: V = s_h mean(x) / 2 + a per-token part of about a third of it.  The
#     output of a head does not cancel (its error is measured against its own size), the heads differ in sign, the tokens by tens of per cent;
#   * WQ, WK / 64: the raw scores stay under 8 (their f16 rounding, 2^-9 at most, is what the softmax amplifies), the probabilities of a row still spread over a decade.
SIGN_H = np.repeat(np.asarray([1.0, -1.0], f32), D)
WQ, WK, WV = lw("/wq", (C, C), 1 / 64), lw("/wk", (C, C), 1 / 64), ((SIGN_H[None, :] + wt("/wv", (C, C))) / 128).astype(f16).astype(f32)
XPOS = {"x": lambda k: pos(_seed("attn_x") + k, XS)}
SCALE = D ** -0.5


def _heads(w, nm, t, tokens, h=H, d=D):
    r = w.reshape(nm + "/Reshape", t, (1, tokens, h, d))
    p = w.transpose(nm + "/Transpose", r, (0, 2, 1, 3))
    return w.reshape(nm + "/Reshape_1", p, (h, tokens, d))


def _proj(w, nm, x, wgt, bias=None):
    y = w.op(nm + "/MatMul", "MatMul", [x, w.c(nm + ".weight", wgt)])
    return y if bias is None else w.op(nm + "/Add", "Add", [y, w.c(nm + ".bias", bias)])


def _attn(w, x=None, scale="mul", kform="plain", merge="1hTd", mperm=(0, 2, 1, 3), sm_axis=-1, sm_twice=False, out="out", nm="/attn", q=None, k=None, v=None, extra_name=None, wts=None):
    """q, k, v: the [1,T,C] projections (made from x here unless given)"""
    x = x if x is not None or q is not None else w.inp("x", XS)
    wq, wk, wv = wts or (WQ, WK, WV)
    q = q if q is not None else _proj(w, nm + "/to_q", x, wq)
    k = k if k is not None else _proj(w, nm + "/to_k", x, wk)
    v = v if v is not None else _proj(w, nm + "/to_v", x, wv)
    qh, vh = _heads(w, nm + "/q", q, T), _heads(w, nm + "/v", v, T)
    if kform == "plain":
        kt = w.transpose(nm + "/k/Transpose_1", _heads(w, nm + "/k", k, T), (0, 2, 1))
    elif kform == "transposed_in_split":                      # [1,T,h,d] -> Transpose(0,2,3,1) -> Reshape[h,d,T]: the key arrives transposed, no Transpose(0,2,1)
        r = w.reshape(nm + "/k/Reshape", k, (1, T, H, D))
        kt = w.reshape(nm + "/k/Reshape_1", w.transpose(nm + "/k/Transpose", r, (0, 2, 3, 1)), (H, D, T))
    else:                                                     # "4x16_regrouped": split into 4 heads of 16, read as 2 x 32: the head counts of q and k differ
        r = w.transpose(nm + "/k/Transpose", w.reshape(nm + "/k/Reshape", k, (1, T, 4, 16)), (0, 2, 1, 3))
        kt = w.transpose(nm + "/k/Transpose_1", w.reshape(nm + "/k/Reshape_1", r, (H, T, D)), (0, 2, 1))
    s = w.op(nm + "/MatMul", "MatMul", [qh, kt])
    if scale == "mul":
        s = w.op(nm + "/Mul", "Mul", [s, w.s(nm + ".scale", SCALE)])
    elif scale == "mul_const_first":
        s = w.op(nm + "/Mul", "Mul", [w.s(nm + ".scale", SCALE), s])
    elif scale == "shape1":
        s = w.op(nm + "/Mul", "Mul", [s, w.c(nm + ".scale", np.asarray([SCALE]))])
    p = w.op(nm + "/Softmax", "Softmax", [s], {"axis": sm_axis}, out=extra_name)
    o = w.op(nm + "/MatMul_1", "MatMul", [p, vh])
    if sm_twice:
        w.op("/other/Neg", "Neg", [p], out="neg")
    o = w.reshape(nm + "/Reshape_o", o, (1, H, T, D) if merge == "1hTd" else (H, 1, T, D))
    o = w.transpose(nm + "/Transpose_o", o, mperm)
    return w.reshape(nm + "/Reshape_o1", o, (1, T, C), out=out)


QKV = ["Linear", "Linear", "Linear"]
for sc in ("mul", "none"):
    add(f"attention/full/{sc}", "fuse_attention", "fires", (lambda w, sc=sc: _attn(w, scale=sc)), XPOS, plan=["Linear", "Attention"], fused="Attention /")
add("attention/softmax_is_extra_output", "fuse_attention", "extra", (lambda w: _attn(w, extra_name="probs")), XPOS, extra=("probs",),
    plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul"])
add("attention/key_transposed_in_head_split", "fuse_attention", "partial", (lambda w: _attn(w, kform="transposed_in_split")), XPOS, plan=QKV + ["AttentionFusedOps"],
    fused="Attention /", why="the key arrives transposed by another route: the same values; the full rewrite reads K through the Transpose(0,2,1) it folds, held on plan structure")
# (a case of its own inputs: x of either sign, sharper scores and a V without a common part, so that the scores decide the output and the regrouped key shows)
W_SHARP = (lw("/wq_s", (C, C), 1 / 32), lw("/wk_s", (C, C), 1 / 32), lw("/wv_s", (C, C), 1 / 16))
add("attention/key_heads_4x16_regrouped", "fuse_attention", "partial", (lambda w: _attn(w, kform="4x16_regrouped", wts=W_SHARP)), {"x": XS}, plan=QKV + ["AttentionFusedOps"],
    fused="Attention /", wrong=lambda w: _attn(w, wts=W_SHARP))
for nm, kw in [("merge_perm_0123", dict(mperm=(0, 1, 2, 3))), ("merge_reshape_h1Td", dict(merge="h1Td"))]:
    add(f"attention/{nm}", "fuse_attention", "partial", (lambda w, kw=kw: _attn(w, **kw)), XPOS, plan=QKV + ["AttentionFusedOps"], fused="Attention /",
        wrong=lambda w: _attn(w))
add("attention/scale_of_shape_1", "fuse_attention", "left", (lambda w: _attn(w, scale="shape1")), XPOS, plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul"], fused="Attention /",
    why="a one-element scale multiplies like a scalar: the same values; the reference's fused operator wants a 0-d scale (\"s must be a scalar\"), held on plan structure")
add("attention/scale_constant_first", "fuse_attention", "left", (lambda w: _attn(w, scale="mul_const_first")), XPOS, plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul"],
    fused="Attention /", why="Mul commutes: the same values; the reference's rewrite reads the scale from input 1 only, held on plan structure")
add("attention/softmax_axis_1", "fuse_attention", "left", (lambda w: _attn(w, sm_axis=1)), XPOS, plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul"], fused="Attention /",
    wrong=lambda w: _attn(w))
add("attention/softmax_read_twice", "fuse_attention", "left", (lambda w: _attn(w, sm_twice=True)), XPOS, outs=("out", "neg"),
    plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul", "Neg"], fused="Attention /", why="the rewrite would leave the probabilities unwritten; a row of 16 probabilities has most of them under 50 tolerances (5 %) of the largest "
                         "whatever the inputs, so `unwritten` cannot meet the half-of-the-elements form: held on the tensor coming back at every level with the restated shape, "
                         "and on its values on the device")
# fuse_attention(false): the reference's own AttentionFusedOps rewrite, below level 2
for sc in ("mul", "none"):
    add(f"attention_plain/{sc}", "fuse_attention", "fires", (lambda w, sc=sc: _attn(w, scale=sc)), XPOS, opts={"fuse_ops_in_attention": 1}, plan=["Linear", "Attention"],
        plan_low=QKV + ["AttentionFusedOps"], fused="Attention /")
add("attention_plain/softmax_axis_1", "fuse_attention", "left", (lambda w: _attn(w, sm_axis=1)), XPOS, opts={"fuse_ops_in_attention": 1},
    plan=QKV + ["MatMul", "Mul", "Softmax", "MatMul"], plan_low=QKV + ["MatMul", "Mul", "Softmax", "MatMul"], fused="Attention /", wrong=lambda w: _attn(w))


# ======================================================================================================================================
# fuse_sdpa (use_scaled_dp_attn_op): the llama form, operands [1,h,T,d], a causal mask
# ======================================================================================================================================
def _causal(neg=-65504.0):
    m = np.zeros((1, 1, T, T), f32)
    for r in range(T):
        m[0, 0, r, r + 1:] = neg
    return m


def _sdpa(w, form="div", mask_first=False, scale_shape=(), kperm=(0, 1, 3, 2), out="out", nm="/attn", extra_name=None):
    x = w.inp("x", XS)

    def split(n, wgt):
        return w.transpose(f"{nm}/{n}/Transpose", w.reshape(f"{nm}/{n}/Reshape", _proj(w, f"{nm}/{n}_proj", x, wgt), (1, T, H, D)), (0, 2, 1, 3))
    q, v = split("q", WQ), split("v", WV)
    if kperm == (0, 1, 3, 2):
        kt = w.transpose(nm + "/Transpose_3", split("k", WK), kperm)
    else:                                                     # the key leaves its head split transposed: [1,T,h,d] -> Transpose(0,2,3,1) = [1,h,d,T]
        kt = w.transpose(nm + "/Transpose_3", w.reshape(nm + "/k/Reshape", _proj(w, nm + "/k_proj", x, WK), (1, T, H, D)), kperm)
    mask = w.c("attn.mask", _causal())
    if form == "div":
        s = w.op(nm + "/MatMul", "MatMul", [q, kt])
        s = w.op(nm + "/Div", "Div", [s, w.c("attn.sqrt_d", np.full(scale_shape, math.sqrt(D)))])
    else:
        q2 = w.op(nm + "/Mul", "Mul", [q, w.c("attn.s", np.full(scale_shape, D ** -0.25))])
        k2 = w.op(nm + "/Mul_1", "Mul", [kt, w.c("attn.s2", np.full(scale_shape, D ** -0.25))])
        s = w.op(nm + "/MatMul", "MatMul", [q2, k2])
    s = w.op(nm + "/Add", "Add", [mask, s] if mask_first else [s, mask])
    p = w.op(nm + "/Softmax", "Softmax", [s], {"axis": -1}, out=extra_name)
    o = w.op(nm + "/MatMul_1", "MatMul", [p, v])
    o = w.transpose(nm + "/Transpose_4", o, (0, 2, 1, 3))
    return w.reshape(nm + "/Reshape_3", o, (1, T, C), out=out)


SD = {"use_scaled_dp_attn_op": 1}
SD_WHY = "the ScaledDotProductAttention operator computes the chain's own function: the guard keeps the rewrite to the operand order and ranks the reference's rewrite reads; "\
         "held on plan structure, and on the values at every level"
SD_DIV, SD_MM = ["MatMul", "Div", "Add", "Softmax", "MatMul"], ["Mul", "Mul", "MatMul", "Add", "Softmax", "MatMul"]
for form in ("div", "mulmul"):
    add(f"sdpa/{form}", "fuse_sdpa", "fires", (lambda w, form=form: _sdpa(w, form)), XPOS, opts=SD, plan=QKV + ["ScaledDotProductAttention"], fused="ScaledDotProductAttention")
add("sdpa/softmax_is_extra_output", "fuse_sdpa", "extra", (lambda w: _sdpa(w, extra_name="probs")), XPOS, opts=SD, extra=("probs",), plan=QKV + SD_DIV)
add("sdpa/mask_first", "fuse_sdpa", "left", (lambda w: _sdpa(w, mask_first=True)), XPOS, opts=SD, plan=QKV + SD_DIV, fused="ScaledDotProductAttention", why=SD_WHY)
add("sdpa/scale_of_rank_2", "fuse_sdpa", "left", (lambda w: _sdpa(w, scale_shape=(1, 1))), XPOS, opts=SD, plan=QKV + SD_DIV, fused="ScaledDotProductAttention", why=SD_WHY)
add("sdpa/scale_of_rank_2_mulmul", "fuse_sdpa", "left", (lambda w: _sdpa(w, "mulmul", scale_shape=(1, 1))), XPOS, opts=SD, plan=QKV + SD_MM, fused="ScaledDotProductAttention",
    why=SD_WHY)
add("sdpa/key_perm_0231", "fuse_sdpa", "left", (lambda w: _sdpa(w, kperm=(0, 2, 3, 1))), XPOS, opts=SD, plan=QKV + SD_DIV, fused="ScaledDotProductAttention", why=SD_WHY)


# ======================================================================================================================================
# fuse_linear / fuse_residual
# ======================================================================================================================================
WL, BL = lw("/wl", (C, C), 1 / 16), wt("/bl", (C,))
WC3, BC = lw("/wc3", (CO, C, 3, 3), 1 / 64), wt("/bc", (CO,)) / 4
CONV3 = {"dilations": "1,1", "group": 1, "kernel_shape": "3,3", "pads": "1,1,1,1", "strides": "1,1"}


def _linear(w, x, bias="N", border="yb", res=None, rorder="yr", res2=None, out="out", nm="/l", wgt=None):
    y = w.op(nm + "/MatMul", "MatMul", [x, w.c(nm + ".weight", WL if wgt is None else wgt)], out=out if (bias is None and res is None) else None)
    if bias is not None:
        b = w.c(nm + ".bias", {"N": BL, "1N": BL.reshape(1, C), "1": BL[:1]}[bias])
        y = w.op(nm + "/Add", "Add", [y, b] if border == "yb" else [b, y], out=out if res is None else None)
    if res is not None:
        r = y if res == "self" else res
        y = w.op(nm + "/Add_r", "Add", [y, r] if rorder == "yr" else [r, y], out=out if res2 is None else None)
    if res2 is not None:
        y = w.op(nm + "/Add_r2", "Add", [y, res2], out=out)
    return y


# a VAE encoder's down-sampling convolution: stride 2, pad on the bottom and the right only (8 x 8 -> 4 x 4)
CONV3_DOWN = {"dilations": "1,1", "group": 1, "kernel_shape": "3,3", "pads": "0,0,1,1", "strides": "2,2"}
DIMG = (1, CO, 4, 4)


def _conv3(w, x, bias=True, nm="/c", out=None, wgt=None, attrs=None):
    ins = [x, w.c(nm + ".weight", WC3 if wgt is None else wgt, conv=True)] + ([w.c(nm + ".bias", BC)] if bias else [])
    return w.op(nm, "Conv", ins, attrs or CONV3, out=out)


for border in ("yb", "by"):
    add(f"linear/bias_N/{border}", "fuse_linear", "fires", (lambda w, border=border: _linear(w, w.inp("x", XS), border=border)), {"x": XS}, plan=["Linear"], rule="contraction", cls_levels=(2,))
add("linear/matmul_is_extra_output", "fuse_linear", "extra",
    (lambda w: w.op("/l/Add", "Add", [w.op("/l/MatMul", "MatMul", [w.inp("x", XS), w.c("/l.weight", WL)], out="mm"), w.c("/l.bias", BL)], out="out")), {"x": XS}, extra=("mm",),
    plan=["Linear", "Add"])
add("linear/bias_1N", "fuse_linear", "left", (lambda w: _linear(w, w.inp("x", XS), bias="1N")), {"x": XS}, plan=["Linear", "Add"],
    why="a [1,N] bias adds like an [N] one: the same values; the epilogue takes a vector, held on plan structure (the Add survives)")
add("linear/bias_of_length_1", "fuse_linear", "left", (lambda w: _linear(w, w.inp("x", XS), bias="1")), {"x": XS}, plan=["Linear", "Add"],
    wrong=lambda w: _linear(w, w.inp("x", XS), bias=None))                                     # (an [N] read of a one-element bias; the least the rewrite does is lose it)
for rorder in ("yr", "ry"):
    add(f"residual/linear/{rorder}", "fuse_residual", "fires", (lambda w, rorder=rorder: _linear(w, w.inp("x", XS), res=w.inp("a", XS), rorder=rorder)), {"x": XS, "a": XS},
        plan=["Linear"], rule="contraction", cls_levels=(2,))


def _x_plus_linear(w):
    x = w.inp("x", XS)
    _linear(w, x, res=x, rorder="ry")


add("residual/x_plus_linear_of_x", "fuse_residual", "fires", _x_plus_linear, {"x": XS}, plan=["Linear"], rule="contraction", cls_levels=(2,))
for bias in (True, False):
    add(f"residual/conv/{'bias' if bias else 'nobias'}", "fuse_residual", "fires",
        (lambda w, bias=bias: w.op("/Add", "Add", [_conv3(w, w.inp("x", IMG), bias), w.inp("a", OIMG)], out="out")), {"x": IMG, "a": OIMG}, plan=["Conv"], rule="contraction", cls_levels=(2,))
add("residual/conv_is_extra_output", "fuse_residual", "extra", (lambda w: w.op("/Add", "Add", [_conv3(w, w.inp("x", IMG), out="conv"), w.inp("a", OIMG)], out="out")),
    {"x": IMG, "a": OIMG}, extra=("conv",), plan=["Conv", "Add"])
add("residual/broadcast_11N", "fuse_residual", "left", (lambda w: _linear(w, w.inp("x", XS), res=w.inp("a", (1, 1, C)))), {"x": XS, "a": (1, 1, C)}, plan=["Linear", "Add"],
    wrong=lambda w: _linear(w, w.inp("x", XS)))         # (the epilogue would read T rows where one exists; the least it does is lose the row)
add("residual/add_y_y", "fuse_residual", "left", (lambda w: _linear(w, w.inp("x", XS), res="self")), {"x": XS}, plan=["Linear", "Add"],
    wrong=lambda w: _linear(w, w.inp("x", XS)))                                                # (a residual that is the op's own output does not exist when the op runs)


def _conv1d_res(w, wrong=False):
    x, a = w.inp("x", (1, C, 40)), w.inp("a", (1, CO, 40))
    y = w.op("/c1", "Conv", [x, w.c("/c1.weight", lw("/wc1", (CO, C, 3, 1), 1 / 32), conv=True), w.c("/c1.bias", BC)],
             {"dilations": "1", "group": 1, "kernel_shape": "3", "pads": "1,1", "strides": "1"}, out="out" if wrong else None)
    if not wrong:
        w.op("/Add", "Add", [y, a], out="out")


add("residual/conv1d", "fuse_residual", "left", _conv1d_res, {"x": (1, C, 40), "a": (1, CO, 40)}, plan=["Conv", "Add"], wrong=lambda w: _conv1d_res(w, True))
add("residual/linear_two_in_a_row", "fuse_residual", "partial", (lambda w: _linear(w, w.inp("x", XS), res=w.inp("a", XS), res2=w.inp("c", XS))), {"x": XS, "a": XS, "c": XS},
    plan=["Linear", "Add"], wrong=lambda w: _linear(w, w.inp("x", XS), res=w.inp("a", XS)))      # defect 1: the second residual dropped


def _conv_two_res(w, wrong=False):
    x, a, c = w.inp("x", IMG), w.inp("a", OIMG), w.inp("c", OIMG)
    y = w.op("/Add", "Add", [_conv3(w, x), a], out="out" if wrong else None)
    if not wrong:
        w.op("/Add_1", "Add", [y, c], out="out")


add("residual/conv_two_in_a_row", "fuse_residual", "partial", _conv_two_res, {"x": IMG, "a": OIMG, "c": OIMG}, plan=["Conv", "Add"],
    wrong=lambda w: _conv_two_res(w, True))                                                     # defect 2


# ======================================================================================================================================
# fuse_conv_act / fuse_gemm_act / fuse_image_bias
# ======================================================================================================================================
WG, BG = lw("/wg", (C, C), 1 / 16), wt("/bg", (C,))


def _temb(w, t, nm="/t"):
    return w.unsqueeze(nm + "/Unsqueeze_1", w.unsqueeze(nm + "/Unsqueeze", t, 2), 3)


def _conv_chain(w, steps, out="out", conv_extra=None, conv_twice=False, t_twice=False, t_const=False, down=False):
    """steps: a string over s (SiLU), r (Add of an image), t (Add of Unsqueeze(Unsqueeze(t[1,C]))) applied to the convolution in that order; down: the convolution
    is the one-sided-pad stride-2 form"""
    x = w.inp("x", IMG)
    r = w.inp("r", DIMG if down else OIMG) if "r" in steps else None
    t = None
    if "t" in steps:
        t = w.c("/t.const", wt("/tconst", (1, CO))) if t_const else w.inp("t", (1, CO))
    y = _conv3(w, x, out=conv_extra, attrs=CONV3_DOWN if down else None)
    y0 = y
    for n, st in enumerate(steps):
        o = out if n == len(steps) - 1 else None
        if st == "s":
            y = _silu(w, y, nm=f"/act{n}", out=o)
        elif st == "r":
            y = w.op(f"/Add{n}", "Add", [y, r], out=o)
        else:
            y = w.op(f"/Add{n}", "Add", [y, _temb(w, t)], out=o)
    if conv_twice:
        w.op("/other/Neg", "Neg", [y0], out="neg")
    if t_twice:
        w.op("/other/Neg", "Neg", [t], out="neg")
    return y


def _gemm(w, bias=True, out="out", extra_name=None):
    x = w.inp("x", (1, C))
    y = w.op("/g", "Gemm", [x, w.c("/g.weight", WG)] + ([w.c("/g.bias", BG)] if bias else []), out=extra_name)
    return _silu(w, y, out=out)


IM, IMR, IMT = {"x": IMG}, {"x": IMG, "r": OIMG}, {"x": IMG, "t": (1, CO)}
add("conv_act/conv_silu", "fuse_conv_act", "fires", (lambda w: _conv_chain(w, "s")), IM, plan=["Conv"])
add("conv_act/conv_residual_silu", "fuse_conv_act", "fires", (lambda w: _conv_chain(w, "rs")), IMR, plan=["Conv"])
add("conv_act/conv_is_extra_output", "fuse_conv_act", "extra", (lambda w: _conv_chain(w, "s", conv_extra="conv")), IM, extra=("conv",), plan=["Conv", "osg.SiLU"])
add("conv_act/silu_then_residual", "fuse_conv_act", "partial", (lambda w: _conv_chain(w, "sr")), IMR, plan=["Conv", "Add"],
    wrong=lambda w: _conv_chain(w, "rs"))                                                       # (the epilogue adds the residual BEFORE the activation)
add("conv_act/conv_read_by_silu_and_another", "fuse_conv_act", "left", (lambda w: _conv_chain(w, "s", conv_twice=True)), IM, outs=("out", "neg"), plan=["Conv", "osg.SiLU", "Neg"],
    wrong={"neg": "unwritten"})
# the three epilogue fusions behind the one-sided-pad stride-2 convolution: the residual's and the per-image bias's rows follow Ho x Wo = 4 x 4, not H x W
add("conv_act/stride2_pads_0011_silu", "fuse_conv_act", "fires", (lambda w: _conv_chain(w, "s", down=True)), IM, plan=["Conv"])
add("residual/conv_stride2_pads_0011", "fuse_residual", "fires", (lambda w: _conv_chain(w, "r", down=True)), {"x": IMG, "r": DIMG}, plan=["Conv"], rule="contraction",
    cls_levels=(2,))
add("image_bias/conv_stride2_pads_0011_add_t", "fuse_image_bias", "fires", (lambda w: _conv_chain(w, "t", down=True)), IMT, plan=["Conv"], rule="contraction", cls_levels=(2,))
add("gemm_act/gemm_silu", "fuse_gemm_act", "fires", (lambda w: _gemm(w)), {"x": (1, C)}, plan=["Gemm"])
add("gemm_act/gemm_is_extra_output", "fuse_gemm_act", "extra", (lambda w: _gemm(w, extra_name="gemm")), {"x": (1, C)}, extra=("gemm",), plan=["Gemm", "osg.SiLU"])
add("gemm_act/no_bias", "fuse_gemm_act", "left", (lambda w: _gemm(w, bias=False)), {"x": (1, C)}, refuse="wrong number of inputs")


def _gemm_twice(w):
    x = w.inp("x", (1, C))
    y = w.op("/g", "Gemm", [x, w.c("/g.weight", WG), w.c("/g.bias", BG)])
    _silu(w, y, out="out")
    w.op("/other/Neg", "Neg", [y], out="neg")


add("gemm_act/gemm_read_by_silu_and_another", "fuse_gemm_act", "left", _gemm_twice, {"x": (1, C)}, outs=("out", "neg"), plan=["Gemm", "osg.SiLU", "Neg"],
    wrong={"neg": "unwritten"})
add("image_bias/conv_add_t", "fuse_image_bias", "fires", (lambda w: _conv_chain(w, "t")), IMT, plan=["Conv"], rule="contraction", cls_levels=(2,))
add("image_bias/conv_is_extra_output", "fuse_image_bias", "extra", (lambda w: _conv_chain(w, "t", conv_extra="conv")), IMT, extra=("conv",), plan=["Conv", "Add"])
add("image_bias/silu_then_add_t", "fuse_image_bias", "left", (lambda w: _conv_chain(w, "st")), IMT, plan=["Conv", "Add"],
    wrong=lambda w: _conv_chain(w, "ts"))                                                       # defect 3: silu(conv + t) where the graph says silu(conv) + t
add("image_bias/t_read_twice", "fuse_image_bias", "left", (lambda w: _conv_chain(w, "t", t_twice=True)), IMT, outs=("out", "neg"), plan=["Conv", "Add", "Neg"],
    why="a guard on the readers of t: the same values either way; held on plan structure")
add("image_bias/t_constant", "fuse_image_bias", "left", (lambda w: _conv_chain(w, "t", t_const=True)), IM, plan=["Conv", "Add"],
    why="a constant t gives the same sum: the epilogue input is per pushed sample, a weight is not; held on plan structure")


# ======================================================================================================================================
# cse_silu
# ======================================================================================================================================
def _cse(w, n=2, second="consumed"):
    x = w.inp("x", XS)
    for k in range(n):
        s = _silu(w, x, nm=f"/act{k}", out="second" if (k == 1 and second != "consumed") else None)
        if not (k == 1 and second == "graph_output"):
            w.op(f"/use{k}", "Mul", [s, w.c(f"/use{k}.c", wt(f"/cse{k}", (C,)))], out=f"out{k}")


add("cse_silu/two", "cse_silu", "fires", (lambda w: _cse(w, 2)), {"x": XS}, outs=("out0", "out1"), plan=["osg.SiLU", "Mul", "Mul"])
add("cse_silu/three", "cse_silu", "fires", (lambda w: _cse(w, 3)), {"x": XS}, outs=("out0", "out1", "out2"), plan=["osg.SiLU", "Mul", "Mul", "Mul"])
add("cse_silu/second_is_graph_output", "cse_silu", "left", (lambda w: _cse(w, 2, "graph_output")), {"x": XS}, outs=("out0", "second"), plan=["osg.SiLU", "Mul", "osg.SiLU"],
    wrong={"second": "unwritten"})                                                              # defect 4
add("cse_silu/second_is_extra_output", "cse_silu", "extra", (lambda w: _cse(w, 2, "extra")), {"x": XS}, outs=("out0", "out1"), extra=("second",),
    plan=["osg.SiLU", "Mul", "osg.SiLU", "Mul"])


def _cse_two_tensors(w, wrong=False):
    x, y = w.inp("x", XS), w.inp("y", XS)
    for n, src in (("x", x), ("y", x if wrong else y)):
        w.op(f"/use_{n}", "Mul", [_silu(w, src, nm="/act_" + n), w.c(f"/use_{n}.c", wt("/cse_" + n, (C,)))], out="out_" + n)


add("cse_silu/silus_of_two_tensors", "cse_silu", "left", _cse_two_tensors, {"x": XS, "y": XS}, outs=("out_x", "out_y"), plan=["osg.SiLU", "Mul", "osg.SiLU", "Mul"],
    wrong=lambda w: _cse_two_tensors(w, True), wrong_outs=("out_y",))                      # (the second SiLU replaced by the first: silu(x) where the graph says silu(y))


# ======================================================================================================================================
# fuse_linear_geglu: osg.Linear(x, W[K,2C], b) -> osg.GEGLU
# ======================================================================================================================================
WP, BP = lw("/wp", (C, 2 * C), 1 / 32), wt("/bp", (2 * C,)) / 8
WP96 = lw("/wp96", (96, 2 * C), 1 / 32)


def _lin_geglu(w, K=C, res=False, twice=False, extra_name=None):
    x = w.inp("x", (1, T, K))
    p = w.op("/ff/proj/MatMul", "MatMul", [x, w.c("/ff/proj.weight", WP if K == C else WP96)])
    p = w.op("/ff/proj/Add", "Add", [p, w.c("/ff/proj.bias", BP)], out=extra_name)
    if res:
        p = w.op("/ff/proj/Add_r", "Add", [p, w.inp("a", PS)])
    _geglu(w, p, third_reader=twice)


add("linear_geglu/K64", "fuse_linear_geglu", "fires", (lambda w: _lin_geglu(w)), {"x": XS}, plan=["Linear+GEGLU"], fused="Linear+GEGLU")
add("linear_geglu/projection_is_extra_output", "fuse_linear_geglu", "extra", (lambda w: _lin_geglu(w, extra_name="proj")), {"x": XS}, extra=("proj",), plan=["Linear"] + GE_OPS)
LG_WHY = "the epilogue computes the GEGLU's own function: the guard keeps the rewrite to the shapes the interleaved weight copy takes and to a projection nobody else reads; "\
         "held on plan structure, and on the values at every level"
add("linear_geglu/K96", "fuse_linear_geglu", "left", (lambda w: _lin_geglu(w, K=96)), {"x": (1, T, 96)}, plan=["Linear", "GEGLU"], fused="Linear+GEGLU", why=LG_WHY)
add("linear_geglu/residual_on_the_linear", "fuse_linear_geglu", "left", (lambda w: _lin_geglu(w, res=True)), {"x": XS, "a": PS}, plan=["Linear", "GEGLU"], fused="Linear+GEGLU", why=LG_WHY)
add("linear_geglu/projection_read_twice", "fuse_linear_geglu", "left", (lambda w: _lin_geglu(w, twice=True)), {"x": XS}, outs=("out", "neg"), plan=["Linear"] + GE_OPS + ["Neg"],
    fused="Linear+GEGLU", wrong={"neg": "unwritten"})


# ======================================================================================================================================
# plan_linear_groups (Q|K|V off one input into one GEMM) and the LayerNorm fold (hip_fuse_ln_gemm)
# ======================================================================================================================================
BQ = wt("/bq", (C,)) / 8
MG_WHY = "the merged launch computes each member's own product: the guard keeps members apart that one launch cannot serve; held on plan structure, and on the values at every level"


LN_B1 = (1.0 + wt("/ln_b1", (C,)) / 16).astype(f16).astype(f32)          # (a LayerNorm output of mean 1: V keeps its sign per head behind it, see WV)


def _qkv(w, qbias=False, q_read=False, q_res=False, ln=False, ln_add=False, ln_extra=None, q_extra=None):
    x = w.inp("x", XS)
    n = _ln(w, x, out=ln_extra, nm="/norm1", beta=LN_B1) if ln else x
    q = _proj(w, "/attn/to_q", n, WQ, BQ if qbias else None) if not q_extra else w.op("/attn/to_q/MatMul", "MatMul", [n, w.c("/attn/to_q.weight", WQ)], out=q_extra)
    if q_res:
        q = w.op("/attn/to_q/Add_r", "Add", [q, w.inp("a", XS)])
    if q_read:
        w.op("/other/Neg", "Neg", [q], out="neg")
    o = _attn(w, q=q, k=_proj(w, "/attn/to_k", n, WK), v=_proj(w, "/attn/to_v", n, WV), out=None if ln_add else "out")
    if ln_add:
        w.op("/Add", "Add", [o, n], out="out")


add("linear_groups/qkv", "plan_linear_groups", "fires", (lambda w: _qkv(w)), XPOS, plan=["Linear", "Attention"], fused="merged(3)")
add("linear_groups/q_with_bias", "plan_linear_groups", "partial", (lambda w: _qkv(w, qbias=True)), XPOS, plan=["Linear", "Linear", "Attention"], present=("merged(2)",), absent=("merged(3)",), why=MG_WHY)
add("linear_groups/q_also_read_by_neg", "plan_linear_groups", "partial", (lambda w: _qkv(w, q_read=True)), XPOS, outs=("out", "neg"), plan=["Linear", "Neg", "Linear", "Attention"],
    present=("merged(2)",), absent=("merged(3)",), why=MG_WHY)
add("linear_groups/q_with_residual", "plan_linear_groups", "partial", (lambda w: _qkv(w, q_res=True)), dict(XPOS, a=XS), plan=["Linear", "Linear", "Attention"], present=("merged(2)",),
    absent=("merged(3)",), why=MG_WHY)
add("linear_groups/q_is_extra_output", "plan_linear_groups", "extra", (lambda w: _qkv(w, q_extra="q")), XPOS, extra=("q",), plan=["Linear", "Linear", "Attention"],
    present=("merged(2)",))
LF_WHY = "the folded GEMM computes LayerNorm then Linear: the guard keeps the fold to a LayerNorm that nothing but the Linears of one launch read; held on plan structure, and on "\
         "the values at every level"
add("ln_fold/read_by_linears_only", "ln_fold", "fires", (lambda w: _qkv(w, ln=True)), XPOS, plan=["Linear", "Attention"], fused="ln+")
add("ln_fold/switched_off", "ln_fold", "left", (lambda w: _qkv(w, ln=True)), XPOS, opts={"hip_fuse_ln_gemm": 0}, plan=["LayerNorm", "Linear", "Attention"], fused="ln+", why=LF_WHY)
add("ln_fold/read_by_a_linear_and_an_add", "ln_fold", "left", (lambda w: _qkv(w, ln=True, ln_add=True)), XPOS, plan=["LayerNorm", "Linear", "Attention", "Add"], fused="ln+",
    why=LF_WHY)
add("ln_fold/layer_norm_is_extra_output", "ln_fold", "extra", (lambda w: _qkv(w, ln=True, ln_extra="normed")), XPOS, extra=("normed",), plan=["LayerNorm", "Linear", "Attention"])


# ======================================================================================================================================
# fuse_rms_norm (under set_upcast_substrings(["/norm/"])) and fuse_rope: the forms of synth/llama.py
# ======================================================================================================================================
RW = near1("/rms_w", (C,))


def _rms(w, p=2.0, plain=None, out="out", extra_name=None):
    """plain: the op written under a name the upcast substrings do not flag"""
    def nm(op):
        return ("/plain/" if plain == op else "/norm/") + op
    x = w.inp("x", XS)
    pw = w.op(nm("Pow"), "Pow", [x, w.s("/norm.two", p)])
    m = w.op(nm("ReduceMean"), "ReduceMean", [pw], RED, out=extra_name)
    e = w.op(nm("Add"), "Add", [m, w.s("/norm.eps", 1e-5)])
    s = w.op(nm("Sqrt"), "Sqrt", [e])
    r = w.op(nm("Div"), "Div", [w.s("/norm.one", 1.0), s])
    xn = w.op(nm("Mul"), "Mul", [x, r])
    return w.op(nm("Mul_1"), "Mul", [w.c("/norm.weight", RW), xn], out=out)


RMS_OPS = ["Pow", "ReduceMean", "Add", "Sqrt", "Div", "Mul", "Mul"]
UP = ["/norm/"]
add("rms_norm/seven_ops", "fuse_rms_norm", "fires", (lambda w: _rms(w)), {"x": XS}, upcast=UP, plan=["RMSNorm"], fused="RMSNorm", rule="rms_chain", cls_levels=(1, 2))
add("rms_norm/mean_is_extra_output", "fuse_rms_norm", "extra", (lambda w: _rms(w, extra_name="mean")), {"x": XS}, upcast=UP, extra=("mean",), plan=RMS_OPS)
add("rms_norm/pow_3", "fuse_rms_norm", "left", (lambda w: _rms(w, p=3.0)), {"x": lambda k: pos(_seed("rms3") + k, XS)}, upcast=UP, plan=RMS_OPS, fused="RMSNorm", wrong=lambda w: _rms(w))
RMS_WHY = "the same function with one more f16 rounding inside the chain (the unflagged op's result): under the chain tolerance; held on plan structure"
add("rms_norm/sqrt_not_flagged", "fuse_rms_norm", "left", (lambda w: _rms(w, plain="Sqrt")), {"x": XS}, upcast=UP, plan=RMS_OPS, fused="RMSNorm", why=RMS_WHY)
add("rms_norm/last_mul_not_flagged", "fuse_rms_norm", "left", (lambda w: _rms(w, plain="Mul_1")), {"x": XS}, upcast=UP, plan=RMS_OPS, fused="RMSNorm", why=RMS_WHY)

RS = (1, H, T, D)
_ang = 0.37 * (np.arange(T, dtype=f64)[:, None] + 1) * (np.arange(D // 2, dtype=f64)[None, :] + 1)       # (angles spread over the circle: neither table is near 0 in a whole column)
COS = np.concatenate([np.cos(_ang), np.cos(_ang)], -1).reshape(1, 1, T, D).astype(f16).astype(f32)
SIN = np.concatenate([np.sin(_ang), np.sin(_ang)], -1).reshape(1, 1, T, D).astype(f16).astype(f32)


def _rope(w, cut=(0, D // 2, D // 2, D), cos_first=False, sin_first=False, rot_first=False, neg_first_half=False, out="out", extra_name=None, other=False):
    x = w.inp("x", RS)
    y = w.inp("y", RS) if other else x
    x1, x2 = w.slice_last("/rope/Slice", x, cut[0], cut[1]), w.slice_last("/rope/Slice_1", x, cut[2], cut[3])
    if neg_first_half:                                        # Concat(Neg(x1), x2): not a rotation
        rot = w.op("/rope/Concat", "Concat", [w.op("/rope/Neg", "Neg", [x1]), x2], {"axis": -1}, out=extra_name)
    else:
        rot = w.op("/rope/Concat", "Concat", [w.op("/rope/Neg", "Neg", [x2]), x1], {"axis": -1}, out=extra_name)
    cos, sin = w.c("/rope.cos", COS), w.c("/rope.sin", SIN)
    a = w.op("/rope/Mul", "Mul", [cos, y] if cos_first else [y, cos])
    b = w.op("/rope/Mul_1", "Mul", [sin, rot] if sin_first else [rot, sin])
    return w.op("/rope/Add", "Add", [b, a] if rot_first else [a, b], out=out)


ROPE_OPS = ["Neg", "Mul", "Mul", "Add"]
add("rope/llama_form", "fuse_rope", "fires", (lambda w: _rope(w)), {"x": RS}, plan=["RoPE"], fused="RoPE")
add("rope/cos_sin_first", "fuse_rope", "fires", (lambda w: _rope(w, cos_first=True, sin_first=True)), {"x": RS}, plan=["RoPE"], fused="RoPE")
add("rope/rotated_term_first", "fuse_rope", "fires", (lambda w: _rope(w, rot_first=True)), {"x": RS}, plan=["RoPE"], fused="RoPE")
add("rope/rotated_is_extra_output", "fuse_rope", "extra", (lambda w: _rope(w, extra_name="rot")), {"x": RS}, extra=("rot",), plan=ROPE_OPS)
add("rope/slices_do_not_meet", "fuse_rope", "left", (lambda w: _rope(w, cut=(0, D // 2 + 4, D // 2 + 4, D))), {"x": RS}, plan=ROPE_OPS, fused="RoPE", wrong=lambda w: _rope(w))
add("rope/cos_times_another_tensor", "fuse_rope", "left", (lambda w: _rope(w, other=True)), {"x": RS, "y": RS}, plan=ROPE_OPS, fused="RoPE", wrong=lambda w: _rope(w))
add("rope/first_half_negated", "fuse_rope", "left", (lambda w: _rope(w, neg_first_half=True)), {"x": RS}, plan=ROPE_OPS, fused="RoPE", wrong=lambda w: _rope(w))


# ======================================================================================================================================
# fuse_tblock_tail: the transformer_block_320 sizes (C = 320, T = 64, heads 8 x 40, context 77 x 768): osg_tblock_tail_supported takes nothing smaller
# ======================================================================================================================================
C3, T3, H3, D3, TK3, CK3 = 320, 64, 8, 40, 77, 768
X3, CTX3, IMG3 = (1, T3, C3), (1, TK3, CK3), (1, C3, 8, 8)


def _attn3(w, nm, x, ctx, tk, kin):
    def heads(n, t, tokens):
        r = w.reshape(f"{nm}/{n}/Reshape", t, (1, tokens, H3, D3))
        return w.reshape(f"{nm}/{n}/Reshape_1", w.transpose(f"{nm}/{n}/Transpose", r, (0, 2, 1, 3)), (H3, tokens, D3))
    q = heads("q", x, T3)
    k = heads("k", _proj(w, nm + "/to_k", ctx, lw(nm + "wk", (kin, C3), 1 / 128)), tk)
    v = heads("v", _proj(w, nm + "/to_v", ctx, lw(nm + "wv", (kin, C3), 1 / 64)), tk)
    s = w.op(nm + "/MatMul", "MatMul", [q, w.transpose(nm + "/k/Transpose_1", k, (0, 2, 1))])
    s = w.op(nm + "/Mul", "Mul", [s, w.s(nm + ".scale", D3 ** -0.5)])
    o = w.op(nm + "/MatMul_1", "MatMul", [w.op(nm + "/Softmax", "Softmax", [s], {"axis": -1}), v])
    o = w.transpose(nm + "/Transpose_o", w.reshape(nm + "/Reshape_o", o, (1, H3, T3, D3)), (0, 2, 1, 3))
    return w.reshape(nm + "/Reshape_o1", o, (1, T3, C3))


def _ln3(w, nm, x):
    mean = w.op(nm + "/ReduceMean", "ReduceMean", [x], RED)
    d = w.op(nm + "/Sub", "Sub", [x, mean])
    var = w.op(nm + "/ReduceMean_1", "ReduceMean", [w.op(nm + "/Pow", "Pow", [d, w.s(nm + ".pow_exp", 2.0)])], RED)
    q = w.op(nm + "/Div", "Div", [d, w.op(nm + "/Sqrt", "Sqrt", [w.op(nm + "/Add", "Add", [var, w.s(nm + ".eps", 1e-5)])])])
    m = w.op(nm + "/Mul", "Mul", [q, w.c(nm + ".weight", near1(nm + "g", (C3,)))])
    return w.op(nm + "/Add_1", "Add", [m, w.c(nm + ".bias", wt(nm + "b", (C3,)) / 16)])


def _lin3(w, nm, x, kin, nout, scale, bias=True):
    return _proj(w, nm, x, lw(nm + "w", (kin, nout), scale), wt(nm + "b", (nout,)) / 16 if bias else None)


def _tblock(w, x1_third=False, q_res=False, pads=0, cross=True):
    x0, ctx = w.inp("x", X3), w.inp("ctx", CTX3)
    res_img = w.inp("img", IMG3)
    n1 = _ln3(w, "/norm1", x0)
    a1 = _attn3(w, "/attn1", _lin3(w, "/attn1/to_q", n1, C3, C3, 1 / 64, False), n1, T3, C3)
    x1 = w.op("/Add", "Add", [_lin3(w, "/attn1/to_out.0", a1, C3, C3, 1 / 64), x0])
    if x1_third:
        w.op("/other/Neg", "Neg", [x1], out="neg")
    x2 = x1
    if cross:
        q = _lin3(w, "/attn2/to_q", _ln3(w, "/norm2", x1), C3, C3, 1 / 64, False)
        if q_res:
            q = w.op("/attn2/to_q/Add_r", "Add", [q, w.inp("a", X3)])
        a2 = _attn3(w, "/attn2", q, ctx, TK3, CK3)
        x2 = w.op("/Add_1", "Add", [_lin3(w, "/attn2/to_out.0", a2, C3, C3, 1 / 64), x1])
    p = _lin3(w, "/ff/net.0/proj", _ln3(w, "/norm3", x2), C3, 8 * C3, 1 / 64)
    gl = _geglu_n(w, p, 4 * C3)
    x3 = w.op("/Add_2", "Add", [_lin3(w, "/ff/net.2", gl, 4 * C3, C3, 1 / 256), x2])
    y = w.transpose("/Transpose_1", w.reshape("/Reshape_1", x3, (1, 8, 8, C3)), (0, 3, 1, 2))
    k = 1 + 2 * pads
    y = w.op("/proj_out", "Conv", [y, w.c("/proj_out.weight", lw("/pow", (C3, C3, k, k), 1 / 64 / k), conv=True), w.c("/proj_out.bias", wt("/pob", (C3,)) / 16)],
             {"dilations": "1,1", "group": 1, "kernel_shape": f"{k},{k}", "pads": ",".join([str(pads)] * 4), "strides": "1,1"})
    w.op("/Add_3", "Add", [y, res_img], out="out")


def _geglu_n(w, p, n, nm="/ff/net.0"):
    val, gate = w.slice_last(nm + "/Slice", p, 0, n), w.slice_last(nm + "/Slice_1", p, n, 2 * n)
    e = w.op(nm + "/Erf", "Erf", [w.op(nm + "/Div", "Div", [gate, w.s(nm + ".sqrt2", SQRT2_F32, "float32")])])
    m = w.op(nm + "/Mul", "Mul", [gate, w.op(nm + "/Add", "Add", [e, w.s(nm + ".one", 1.0)])])
    return w.op(nm + "/Mul_2", "Mul", [val, w.op(nm + "/Mul_1", "Mul", [m, w.s(nm + ".half", 0.5)])])


def _x3(name, shape, s):
    return lambda k: rnd(_seed(name) + k, shape) * f32(s)


TB_IN = {"x": _x3("tbx", X3, 0.5), "ctx": _x3("tbc", CTX3, 0.5), "img": _x3("tbi", IMG3, 0.5)}
TB_WHY = "the one-launch tail computes the chain's own function: the guard keeps it to a chain whose interior nobody else reads and to a 1x1 projection; held on plan structure, and on "\
         "the values at every level"
TB_OFF = ["Linear", "Attention", "Linear", "Linear", "Linear", "Attention", "Linear", "Linear+GEGLU", "Linear", "Conv"]      # Q|K|V, attn1, to_out + x0, to_q, K|V, attn2, to_out + x1, proj + GEGLU, net.2 + x2, proj_out + image
add("tblock_tail/positive", "fuse_tblock_tail", "fires", (lambda w: _tblock(w)), TB_IN, plan=["Linear", "Attention", "Linear", "TBlockTail+proj_out"], fused="TBlockTail+proj_out")
add("tblock_tail/x1_read_three_times", "fuse_tblock_tail", "left", (lambda w: _tblock(w, x1_third=True)), TB_IN, outs=("out", "neg"), plan=TB_OFF[:3] + ["Neg"] + TB_OFF[3:], fused="TBlockTail", wrong={"neg": "unwritten"})
add("tblock_tail/to_q_with_residual", "fuse_tblock_tail", "left", (lambda w: _tblock(w, q_res=True)), dict(TB_IN, a=_x3("tba", X3, 0.5)), plan=TB_OFF, fused="TBlockTail", why=TB_WHY)
add("tblock_tail/proj_out_pads_1", "fuse_tblock_tail", "partial", (lambda w: _tblock(w, pads=1)), TB_IN, plan=["Linear", "Attention", "Linear", "TBlockTail", "Conv"],
    fused="TBlockTail+proj_out", present=("TBlockTail ",), why=TB_WHY)
add("tblock_tail/self_attention_only", "fuse_tblock_tail", "left", (lambda w: _tblock(w, cross=False)), TB_IN, plan=["Linear", "Attention", "Linear", "Linear+GEGLU", "Linear", "Conv"], fused="TBlockTail", why=TB_WHY)


# ---- figures on record, each held with 10 % headroom (the form of parity.EXCEPTIONS) ------------------------------------------------------------------------------
# REF_NOISE: "<case>|<output>" -> max|f16(restatement) - ref16| / max|ref32| where the REFERENCE'S OWN op-by-op f16 chain is more than 1e-3 from float64 (a cube, a
# probability tensor, a product of two rounded factors: no fused launch is involved).  tests/test_fusion_cases_cpu.py holds the restatement to these instead of 1e-3.
REF_NOISE = {
    "group_norm/silu|out": 1.03e-3,
    "group_norm/add_read_by_silu_and_another|out": 1.03e-3,
    "layer_norm/pow_3|out": 1.59e-3,
    "layer_norm/gamma_T1_with_T_eq_C|out": 1.03e-3,
    "attention/softmax_is_extra_output|probs": 1.10e-3,
    "attention/softmax_read_twice|neg": 1.10e-3,
    "linear_geglu/projection_is_extra_output|out": 1.02e-3,
}
# EXCEPTIONS: ("<case>|<output>", level) -> err16 measured on an MI355X where the device is more than 1e-3 from the reference's f16 output (profiles/fusion_cases_table.txt).
# Every one is one or two f16 ulps at the largest elements of an output (one ulp at the bottom of the top binade is 2^-10 = 9.8e-4 of it): a chain that runs op by op on
# both sides and rounds an intermediate the other way (levels 0 / 1, or the same figure at all three), or a launch that saves one of the reference's roundings (level 2).
# None comes near the 50 tolerances that separate a case from its forbidden rewrite.
EXCEPTIONS = {
    ("silu/sigmoid_times_itself|out", 0): 1.01e-03, ("silu/sigmoid_times_itself|out", 1): 1.01e-03, ("silu/sigmoid_times_itself|out", 2): 1.01e-03,
    # (the two below: the device is 0 / 1 f16 ulps from float64 at levels 1 and 2; the figure is the reference's own, REF_NOISE)
    ("group_norm/silu|out", 0): 1.03e-03, ("group_norm/silu|out", 1): 1.03e-03, ("group_norm/silu|out", 2): 1.03e-03,
    ("group_norm/add_read_by_silu_and_another|out", 0): 1.03e-03, ("group_norm/add_read_by_silu_and_another|out", 1): 1.03e-03,
    ("group_norm/add_read_by_silu_and_another|out", 2): 1.03e-03,
    ("layer_norm/div_sqrt_by_centred|out", 0): 1.46e-03, ("layer_norm/div_sqrt_by_centred|out", 1): 1.46e-03, ("layer_norm/div_sqrt_by_centred|out", 2): 1.46e-03,
    ("layer_norm/gamma_T1_with_T_eq_C|out", 0): 1.03e-03, ("layer_norm/gamma_T1_with_T_eq_C|out", 1): 1.03e-03, ("layer_norm/gamma_T1_with_T_eq_C|out", 2): 1.03e-03,
    ("attention/key_heads_4x16_regrouped|out", 2): 1.01e-03,
    ("residual/broadcast_11N|out", 2): 1.02e-03,
    ("linear_geglu/K96|out", 2): 1.19e-03,
    ("linear_geglu/projection_read_twice|out", 2): 1.37e-03,
    ("ln_fold/read_by_linears_only|out", 1): 1.19e-03, ("ln_fold/switched_off|out", 1): 1.19e-03, ("ln_fold/layer_norm_is_extra_output|out", 1): 1.19e-03,
}


def bound16(case, o, level=None):
    """what err16 of `o` is held to: 1e-3, or a figure on record with 10 % headroom"""
    m = REF_NOISE.get(f"{case.name}|{o}") if level is None else EXCEPTIONS.get((f"{case.name}|{o}", level))
    return 1e-3 if m is None else 1.1 * m


# ---- what the reference says about these cases (tools/make_golden_fusion.py prints the list) ----------------------------------------------------------------
# case -> a substring of the reference's refusal: restatement-only cases
REF_REFUSES = {}

# the fp16 passes of run_fusions() and the two lowering-time merges; the uint8 passes (fuse_u8_*) need range data: their table is tests/qu8_cases.py
PASSES = ("fuse_sdpa", "fuse_rms_norm", "fuse_rope", "fuse_silu", "fuse_group_norm", "fuse_layer_norm", "fuse_geglu", "fuse_attention", "fuse_linear", "fuse_residual",
          "fuse_conv_act", "fuse_linear_geglu", "fuse_tblock_tail", "cse_silu", "fuse_gemm_act", "fuse_image_bias", "plan_linear_groups", "ln_fold")
LEVELS = (0, 1, 2)


def planned():
    """the cases that plan (not refused by the lowering at every level)"""
    return [c for c in CASES if not c.refuse]


# ---- running a case ------------------------------------------------------------------------------------------------------------------------------------------
def run(case, level, pushes=1, first=0):
    """-> (output name -> list of fp32 arrays, [] where get_tensor returned None; the plan's arithmetic step kinds; every step's `what`)"""
    got, what = oc.run_case(case, pushes, level, first, options=case.opts, extra_outputs=case.extra_outs, plan=True)
    return got, kinds(what), what


def kinds(what):
    return [k for k in (w.split(" ", 1)[0] for w in what) if k not in MOVES]


def expected_plan(case, level):
    if level == 2:
        return case.plan
    return case.plan_low if (case.plan_low and case.opts.get("fuse_ops_in_attention")) else None


# ---- tests/golden/fusion_cases.npz: the reference's outputs of sample 0, packed (three entries, so that the archive's per-entry overhead stays out of the 400 KiB cap):
#   ref16     every output of the fp16-arithmetic run as f16 values, one after the other; an output of more than GOLDEN_FULL values (the five 320-wide cases) at every
#             GOLDEN_STRIDE-th value of its flattened form
#   ref32max  max|ref32| of the fp32-arithmetic run per output: all that the single-pattern rule takes from it
#   index     "<case>|<output>" per output, in order, with its shape
GOLDEN_FULL, GOLDEN_STRIDE = 4096, 8
_GOLDEN = None


def golden_stride(n):
    return GOLDEN_STRIDE if n > GOLDEN_FULL else 1


def load_golden(path=None):
    import json
    import os
    z = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_cases.npz"))
    out, at = {}, 0
    for (key, shape), m in zip(json.loads(bytes(z["index"]).decode()), z["ref32max"]):
        n = int(np.prod(shape, dtype=np.int64))
        kept = -(-n // golden_stride(n))
        out[key] = (z["ref16"][at:at + kept].astype(f32), float(m), tuple(shape))
        at += kept
    assert at == z["ref16"].size
    return out


def golden(case, o):
    """(ref16 values kept, max|ref32|, shape) of sample 0, or None for a case the reference refuses"""
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden()
    if case.name in REF_REFUSES or case.refuse:
        return None
    return _GOLDEN[f"{case.name}|{o}"]


def err16(got, gold):
    """the single-pattern figure of tests/test_golden.py, max|got - ref16| / max|ref32|, over the values the golden file keeps"""
    ref16, m32, shape = gold
    assert tuple(got.shape) == shape, (got.shape, shape)
    g = np.ascontiguousarray(got, f32).reshape(-1)[::golden_stride(got.size)]
    return oc.err16(g, ref16, np.asarray([m32]))


# ---- the figures of one output of one sample on the device, and what its case allows (tests/test_fusion_cases_gpu.py asserts, tools/fusion_cases_table.py prints) ------
_WANT = {}


def want(case, k=0):
    """the float64 restatement of sample k (with the @S / @K of a contraction output), computed once and left unchanged"""
    if (case.name, k) not in _WANT:
        _WANT[(case.name, k)] = case.want(k)
        for v in _WANT[(case.name, k)].values():
            v.setflags(write=False)
    return _WANT[(case.name, k)]


def norm_bound(case, k):
    """(want, bound) of the kernel-level GroupNorm / LayerNorm test for this case's `out`"""
    from test_unet_attention_norm import norm_exact          # the bound of the kernel-level test itself
    x, n = r16(case.sample(k)["x"]), case.extra
    gam, bet, eps = n["gamma"].astype(f64), n["beta"].astype(f64), float(n["eps"])
    if case.rule == "layer_norm":
        return norm_exact(x, gam, bet, eps, -(-x.shape[-1] // 256) + 12, False, 0, f16)
    per = lambda v: np.broadcast_to(v.reshape(1, -1, 1, 1), x.shape).reshape(1, GG, -1)      # (NCHW: the channels of a group lie together)
    w, b = norm_exact(x.reshape(1, GG, -1), per(gam), per(bet), eps, 24, True, n["act"], f16)
    return w.reshape(x.shape), b.reshape(x.shape)


def check_output(case, level, o, got, k=0):
    """-> (figures, failures) as op_cases.figures: `ulps` (largest distance in f16 ulps to the float64 restatement rounded to f16), for sample 0 `err16` against the golden
    file, `ratio` (error / bound) where a class rule applies; `failures` lists what the case does not allow (empty: the output passes)"""
    w = want(case, k)[o]
    if got.shape != w.shape:
        return {}, [f"shape {got.shape}, restated {w.shape}"]
    fig, bad = {"ulps": int(oc.ulps16(got, w).max())}, ([] if np.isfinite(got).all() else ["not finite"])
    if case.rule and o == "out" and level in case.cls_levels:
        if case.rule in ("group_norm", "layer_norm"):
            w2, bound = norm_bound(case, k)
            assert np.allclose(w2, w, rtol=1e-9, atol=1e-9), case.name
            fig["ratio"] = float((np.abs(got.astype(f64) - w) / bound).max())
            if fig["ratio"] > 1.0:
                bad.append(f"error / bound {fig['ratio']:.3f} ({case.rule})")
        else:
            f2, b2 = oc.figures(case.as_class(), o, got, k)
            fig.update(f2)
            bad += b2
    gold = golden(case, o) if k == 0 else None
    if gold:
        fig["err16"] = err16(got, gold)
        if fig["err16"] > bound16(case, o, level):
            bad.append(f"err16 {fig['err16']:.2e} > {bound16(case, o, level):.2e}")
    return fig, bad
