"""The case table of the uint8-arithmetic lowering tests (tests/test_qu8_lowering_cpu.py on the stub backend, tests/test_qu8_lowering_gpu.py on the device,
tools/make_golden_qu8_cases.py for the reference's outputs in tests/golden/qu8_cases.npz).  It is the uint8 sister of tests/op_cases.py and
tests/fusion_cases.py: one case = one small graph aimed at ONE branch of csrc/host/lowering_u8.inc, of the two uint8 passes of lowering_graph.inc
(fuse_u8_instance_norm_nhwc, fuse_u8_affine_act) or of the run-time protocol for inputs whose (scale, zero point) change per pass (qdyn, dyn_end).

A case's `body(w)` writes the graph op by op through the writer QW.  QW hands every op to GraphBuilder(quant_all=True).op(...) AND evaluates it in float64
numpy on every sample of the case, so that the case's range data -- (min, max) of each op's float64 output over the samples, in the reference's text
format -- comes from the same description.  The text the tests READ is the one stored in tests/golden/qu8_cases.npz: every machine reads the same bytes.

`interpret` runs a parsed model.txt forward on CODES with oracle/np_qu8.py (the bit-exact specification, pinned against the reference by
oracle/qu8_check.py): pushed inputs through quantize_dynamic, every op through its np_qu8 function with the output parameters range_to_scale gives for its
range, movement ops copy codes and carry (scale, zero point), Conv pads re-centred as the reference does.  Everything is in the logical layout.

  kind     "lower"   a branch of lowering_u8.inc;  "fusion"  a form or near miss of a uint8 pass;  "reject"  refused at plan time with `reject` in the message
  expect   (fusion) "fires" / "partial" (Mul + Add fuse, the SiLU stays) / "left"
  present  substrings of Model.hip_plan_info step names the fusion level 1 plan shows; `absent` the ones it must not show.  The level 0 plan shows no
           FUSED mark at all
  wrong    for "left" / "partial": what the forbidden rewrite would do --
             a body             the graph it would compute (same op names, so the same range data): its codes must differ from the graph as written
             {name: "unwritten"} a tensor it would delete: the named OUTPUT that reads it differs from zeros
             ("refused", body, message)  the fused op written by hand: the lowering refuses it with `message`
           or `why`: the rewrite would compute the same codes (the guard keeps the pass to operands it can prove constant, or to what a kernel holds);
           such a case is held on plan structure alone and says so
  extra    tensors asked for through add_extra_output at level 1 (the fusion expectation is stated WITH them)
  opts     vram_budget: Model.hip_set_vram_budget before the graph is read;  pushes: samples pushed before one run (uint8 arithmetic takes one)
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from onnxstream_amd.synth import graph as sg  # noqa: E402
from oracle import np_qu8 as Q  # noqa: E402
from oracle.np_ops import range_to_scale  # noqa: E402

f32, f64 = np.float32, np.float64
MOVE_TYPES = ("Reshape", "Flatten", "Squeeze", "Unsqueeze", "Transpose", "Resize")
FUSED = ("InstanceNorm qu8 nhwc", "AffineAct qu8", "NormAffineAct qu8")          # the marks of a uint8 rewrite in a step's name ("AffineAct qu8" is in "NormAffineAct qu8" too)
RATTR = {"coordinate_transformation_mode": "asymmetric", "mode": "nearest", "nearest_mode": "floor"}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100000


def recentre(pads):
    """(top, left, bottom, right) as the reference hands them to the convolution: the total per axis split in halves, the odd cell at the bottom / right"""
    ph, pw = pads[0] + pads[2], pads[1] + pads[3]
    return ph // 2, pw // 2, ph - ph // 2, pw - pw // 2


def _ints(s):
    return [int(v) for v in str(s).split(",")]


def reshape_target(shape, tgt):
    out = [shape[k] if int(d) == 0 else int(d) for k, d in enumerate(tgt)]
    if -1 in out:
        out[out.index(-1)] = int(np.prod(shape)) // int(-np.prod(out))
    return out


def move(typ, x, attrs, consts):
    """the movement operators on any array (codes or float64): consts are the values of the constant operands (None where absent)"""
    if typ == "Reshape":
        return np.ascontiguousarray(x).reshape(reshape_target(x.shape, consts[1]))
    if typ == "Flatten":
        ax = int(attrs.get("axis", 1))
        ax += x.ndim if ax < 0 else 0
        return np.ascontiguousarray(x).reshape(int(np.prod(x.shape[:ax], dtype=np.int64)), -1)
    if typ == "Squeeze":
        return np.squeeze(x, tuple(int(a) for a in consts[1]))
    if typ == "Unsqueeze":
        out = x
        rank = x.ndim + len(consts[1])
        for ax in sorted(int(a) % rank for a in consts[1]):
            out = np.expand_dims(out, ax)
        return out
    if typ == "Transpose":
        return x.transpose(_ints(attrs["perm"]))
    if typ == "Resize":
        sc = consts[2]
        return Q.resize_nearest_u8(x, float(sc[2]), float(sc[3]))
    raise KeyError(typ)


# ======================================================================================================================================
# the float64 restatement (for the range data only: the codes come from `interpret`)
# ======================================================================================================================================
def _fconv(x, w_oihw, b, pads, strides):
    pt, pl, pb, pr = recentre(pads)
    O, _, kh, kw = w_oihw.shape
    xp = np.pad(x, ((0, 0), (0, 0), (pt, pb), (pl, pr)))
    Ho, Wo = (xp.shape[2] - kh) // strides[0] + 1, (xp.shape[3] - kw) // strides[1] + 1
    out = np.zeros((x.shape[0], O, Ho, Wo))
    for dy in range(kh):
        for dx in range(kw):
            out += np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + strides[0] * (Ho - 1) + 1:strides[0], dx:dx + strides[1] * (Wo - 1) + 1:strides[1]], w_oihw[:, :, dy, dx])
    return out if b is None else out + b[None, :, None, None]


def _fop(typ, v, a):
    if typ == "Conv":
        return _fconv(v[0], v[1], v[2] if len(v) > 2 else None, _ints(a.get("pads", "0,0,0,0")), _ints(a.get("strides", "1,1")))
    if typ == "MatMul":
        return v[0] @ v[1]
    if typ in ("Add", "Sub"):
        return v[0] + v[1] if typ == "Add" else v[0] - v[1]
    if typ in ("Mul", "Div"):
        return v[0] * v[1] if typ == "Mul" else v[0] / v[1]
    if typ == "Concat":
        return np.concatenate(v, int(a["axis"]))
    if typ == "Sigmoid":
        return 1.0 / (1.0 + np.exp(-v[0]))
    if typ == "Softmax":
        ax = int(a.get("axis", -1))
        e = np.exp(v[0] - v[0].max(axis=ax, keepdims=True))
        return e / e.sum(axis=ax, keepdims=True)
    if typ == "InstanceNormalization":
        x = v[0]
        red = tuple(range(2, x.ndim))
        mu, var = x.mean(red, keepdims=True), x.var(red, keepdims=True)
        sh = (1, -1) + (1,) * (x.ndim - 2)
        return (x - mu) / np.sqrt(var + float(f32(float(a.get("epsilon", 1e-5))))) * v[1].reshape(sh) + v[2].reshape(sh)
    return move(typ, v[0], a, v)


class QW:
    """one call = one op in model.txt + its float64 value on every sample"""

    def __init__(self, g, samples):
        self.g, self.samples, self.val, self.ranges, self.acts, self.lenient = g, samples, {}, {}, [], False

    def inp(self, name, shape):
        t = self.g.input(name, shape)
        self.val[t.name] = [np.asarray(s[name], f64).reshape(shape) for s in self.samples]
        return t

    def _const(self, t, arr):
        self.val[t.name] = [arr] * len(self.samples)
        return t

    def cq(self, name, arr, conv=False):
        """a float initializer: uint8[scale, zero point] in the file, its dequantised value here"""
        arr = np.asarray(arr, f32)
        q, sc, zp = sg.quantize_u8(arr)
        return self._const(self.g.weight(name, arr, conv=conv, allow_quant=False), (q.astype(f64) - zp) * float(f32(sc)))

    def c32(self, name, arr):
        """what the exporter leaves fp32: Conv biases, InstanceNormalization scale / bias, Resize scales"""
        arr = np.asarray(arr, f32)
        return self._const(self.g.weight(name, arr, dtype="float32", allow_quant=False, q8_exempt=True), arr.astype(f64))

    def c16(self, name, arr, conv=False):
        arr = np.asarray(arr, f32)
        return self._const(self.g.weight(name, arr, dtype="float16", allow_quant=False, q8_exempt=True, conv=conv), arr.astype(f64))

    def i64(self, name, vals):
        return self._const(self.g.weight(name, np.asarray(vals, np.int64), dtype="int64"), np.asarray(vals, np.int64))

    def op(self, name, typ, ins, attrs=None, out=None, shape=None):
        attrs = {k: str(v) for k, v in (attrs or {}).items()}
        try:
            vals = [_fop(typ, [None if t is None else self.val[t.name][k] for t in ins], attrs) for k in range(len(self.samples))]
        except Exception:
            if not self.lenient:
                raise
            return self.raw(name, typ, ins, shape if shape is not None else ins[0].shape, attrs, out)          # (a form no restatement takes: a reject case)
        t = self.g.op(name, typ, ins, tuple(shape if shape is not None else vals[0].shape), attrs or None, out_names=[out or name + "o"])
        self.val[t.name] = vals
        self.acts.append(t.name)
        self.ranges[name] = (min(float(v.min()) for v in vals), max(float(v.max()) for v in vals))
        return t

    def raw(self, name, typ, ins, shape, attrs=None, out=None, rng=(-1.0, 1.0), second_out=None):
        """an op written by hand (the fused forms of the uint8 passes, forms no restatement takes): no value, the range given"""
        a = {k: str(v) for k, v in (attrs or {}).items()} or None
        if second_out:
            t = self.g.op(name, typ, ins, [tuple(shape), tuple(shape)], a, out_names=[out or name + "o", second_out])[0]
        else:
            t = self.g.op(name, typ, ins, tuple(shape), a, out_names=[out or name + "o"])
        self.acts.append(t.name)
        if rng:
            self.ranges[name] = rng
        return t

    # single ops with their constant operand
    def conv(self, name, x, cout, k=(3, 3), pads=(1, 1, 1, 1), strides=(1, 1), bias=True, ks=True, out=None, attrs=None, wdt=None, bdt=None, kshape=None):
        cin = x.shape[1]
        rng = np.random.default_rng(_seed("w" + name))
        wv = (rng.standard_normal((cout, cin, k[0], k[1])) / np.sqrt(cin * k[0] * k[1])).astype(f32)
        ins = [x, self.c16(name + "w", wv, conv=True) if wdt == "float16" else self.cq(name + "w", wv, conv=True)]
        if bias:
            bv = (rng.standard_normal(cout) * 0.3).astype(f32)
            ins.append(self.c16(name + "b", bv) if bdt == "float16" else self.c32(name + "b", bv))
        a = {"dilations": "1,1", "group": "1"}
        if ks:
            a["kernel_shape"] = kshape or f"{k[0]},{k[1]}"
        a["pads"] = ",".join(map(str, pads))
        a["strides"] = ",".join(map(str, strides))
        a.update(attrs or {})
        return self.op(name, "Conv", ins, a, out)

    def reshape(self, name, x, shape, out=None):
        return self.op(name, "Reshape", [x, self.i64(name + "s", shape)], {"allowzero": 0}, out)

    def transpose(self, name, x, perm, out=None):
        return self.op(name, "Transpose", [x], {"perm": ",".join(map(str, perm))}, out)

    def sigmoid(self, name, x, out=None):
        return self.op(name, "Sigmoid", [x], None, out)

    def wq(self, name, shape, scale=1.0, shift=0.0):
        rng = np.random.default_rng(_seed("w" + name))
        return self.cq(name, (rng.standard_normal(shape) * scale + shift).astype(f32))


# ======================================================================================================================================
# cases
# ======================================================================================================================================
class QCase:
    def __init__(self, name, kind, body, inputs, outs=("out",), reject=None, pass_=None, expect=None, present=(), absent=(), wrong=None, why=None, extra=(), opts=None,
                 drop_range=()):
        assert kind in ("lower", "fusion", "reject") and (kind != "reject" or reject) and (kind != "fusion" or expect in ("fires", "partial", "left")), name
        assert expect not in ("left", "partial") or wrong is not None or why, name
        self.name, self.kind, self.body, self.inputs, self.outs, self.reject = name, kind, body, dict(inputs), tuple(outs), reject
        self.pass_, self.expect, self.present, self.absent, self.wrong, self.why = pass_, expect, tuple(present), tuple(absent), wrong, why
        self.extra, self.opts, self.drop_range = tuple(extra), dict(opts or {}), tuple(drop_range)
        self._acts = None

    def sample(self, k):
        """pass inputs: sample 0 = A (seeded), sample 1 = 0.37 A + 0.2 -- another range, so another (scale, zero point) for every pushed input"""
        out = {}
        for j, (n, s) in enumerate(self.inputs.items()):
            a = (np.random.default_rng(_seed(self.name) + 10 * j).standard_normal(s) * 1.2 + 0.15).astype(f32)
            out[n] = a if k == 0 else (a * f32(0.37) + f32(0.2)).astype(f32)
        return out

    def passes(self):
        """the four passes of the device protocol: A, A, 0.37 A + 0.2, A"""
        return [self.sample(0), self.sample(0), self.sample(1), self.sample(0)]

    def write(self, sink, body=None):
        g = sg.GraphBuilder(sink, quant_all=True)
        w = QW(g, [self.sample(0), self.sample(1)])
        w.lenient = self.kind == "reject" or body is not None
        (body or self.body)(w)
        g.finish()
        return w

    def emit(self, d, body=None):
        return self.write(sg.DirSink(d), body)

    def computed_range_text(self):
        w = self.write(sg.MemSink())
        return "".join(f"{n},{lo:.6f},{hi:.6f}\r\n" for n, (lo, hi) in w.ranges.items() if n not in self.drop_range)

    def intermediates(self):
        """every activation an op writes, in graph order (the outputs included)"""
        if self._acts is None:
            self._acts = tuple(self.write(sg.MemSink()).acts)
        return self._acts


CASES = []


def add(*a, **k):
    c = QCase(*a, **k)
    assert all(c.name != o.name for o in CASES), c.name
    CASES.append(c)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def planned():
    return [c for c in CASES if c.kind != "reject"]


def rejects():
    return [c for c in CASES if c.kind == "reject"]


# shapes: small, non-square, pairwise distinct (a swapped extent cannot pass)
H, W, CI, CO = 5, 7, 8, 12
X = (1, CI, H, W)
Y = (1, CO, H, W)
INX = {"x": X}


def pre(w, name="pre", cout=CI, x=None):
    """a 1x1 Conv in front: what follows reads a channels-last tensor with parameters from range data"""
    return w.conv(name, x if x is not None else w.inp("x", X), cout, k=(1, 1), pads=(0, 0, 0, 0))


# ---- Conv ------------------------------------------------------------------------------------------------------------------------------------------
def _conv_case(name, **kw):
    add("conv/" + name, "lower", (lambda w: w.conv("conv", pre(w), CO, out="out", **kw)), INX)


_conv_case("k3_pad1")
_conv_case("k1", k=(1, 1), pads=(0, 0, 0, 0))
_conv_case("pads_0011", pads=(0, 0, 1, 1))
_conv_case("pads_1100", pads=(1, 1, 0, 0))
_conv_case("pads_2000", pads=(2, 0, 0, 0))
_conv_case("stride2_pads_0011", pads=(0, 0, 1, 1), strides=(2, 2))
_conv_case("stride_2_1", strides=(2, 1))
_conv_case("no_bias", bias=False)
_conv_case("k3x5", k=(3, 5), pads=(1, 2, 1, 2))
_conv_case("k5x7_pads_2323", k=(5, 7), pads=(2, 3, 2, 3))
_conv_case("no_kernel_shape", ks=False)
# an fp16 bias file: the loader hands every floating-point constant of a uint8 plan over as fp32, so the bias arrives as the fp32 the launch wants
_conv_case("fp16_bias", bdt="float16")
add("conv/plain_pushed", "lower", (lambda w: w.conv("conv", w.inp("x", X), CO, out="out")), INX)
add("conv/plain_from_reshape", "lower", (lambda w: w.conv("conv", w.reshape("rs", w.inp("x", (1, CI * H, W)), X), CO, out="out")), {"x": (1, CI * H, W)})
add("conv/plain_from_add", "lower", (lambda w: w.conv("conv", w.op("add", "Add", [w.inp("x", X), w.inp("y", X)]), CO, out="out")), {"x": X, "y": X})
# the weight of `conv` (864 bytes) does not fit behind `pre`'s: it travels through the streaming ring, so the plan holds no tap-sum table for it
add("conv/k3_pad1_streamed", "lower", (lambda w: w.conv("conv", pre(w), CO, out="out")), INX, opts={"vram_budget": 256})


# ---- MatMul ----------------------------------------------------------------------------------------------------------------------------------------
MN, MM, MK, MNN = 2, 5, 8, 7
for nm, sh in (("w_MK", (MM, MK)), ("w_1MK", (1, MM, MK)), ("w_1nMK", (1, MN, MM, MK))):
    add("matmul/" + nm, "lower", (lambda w, sh=sh: w.op("mm", "MatMul", [w.inp("x", sh), w.wq("mmw", (MK, MNN), 0.5)], out="out")), {"x": sh})
for n in (1, 2):
    for nm, lead in (("aa_nMK", ()), ("aa_1nMK", (1,))):
        sa, sb = lead + (n, MM, MK), lead + (n, MK, MNN)
        add(f"matmul/{nm}_n{n}", "lower", (lambda w, sa=sa, sb=sb: w.op("mm", "MatMul", [w.inp("a", sa), w.inp("b", sb)], out="out")), {"a": sa, "b": sb})
# one operand with parameters from range data, the other pushed: the launch reads the PUSHED operand's per-pass parameters whichever side it is on
add("matmul/aa_static_a_pushed_b", "lower", (lambda w: w.op("mm", "MatMul", [w.sigmoid("sa", w.inp("a", (MN, MM, MK))), w.inp("b", (MN, MK, MNN))], out="out")),
    {"a": (MN, MM, MK), "b": (MN, MK, MNN)})
add("matmul/aa_pushed_a_static_b", "lower", (lambda w: w.op("mm", "MatMul", [w.inp("a", (MN, MM, MK)), w.sigmoid("sb", w.inp("b", (MN, MK, MNN)))], out="out")),
    {"a": (MN, MM, MK), "b": (MN, MK, MNN)})


# ---- Add / Mul -------------------------------------------------------------------------------------------------------------------------------------
def _bin(name, fn, inputs):
    for typ in ("Add", "Mul"):
        for order in ("ab", "ba"):
            def body(w, typ=typ, order=order):
                a, b = fn(w)
                w.op("bin", typ, [a, b] if order == "ab" else [b, a], out="out")
            add(f"{typ.lower()}/{name}_{order}", "lower", body, inputs)


_bin("nhwc_nhwc", lambda w: (lambda x: (pre(w, "ca", CO, x), pre(w, "cb", CO, x)))(w.inp("x", X)), INX)
_bin("nhwc_plain", lambda w: (pre(w, "ca", CO), w.reshape("rs", w.inp("y", (1, CO, H * W)), Y)), {"x": X, "y": (1, CO, H * W)})
_bin("chan_C11", lambda w: (pre(w, "ca", CO), w.wq("g", (CO, 1, 1), 0.8, 0.3)), INX)
_bin("chan_1C11", lambda w: (pre(w, "ca", CO), w.wq("g", (1, CO, 1, 1), 0.8, 0.3)), INX)
_bin("scalar", lambda w: (pre(w, "ca", CO), w.cq("g", np.asarray(0.7, f32).reshape(()))), INX)
_bin("lastaxis_W", lambda w: (w.inp("x", (3, 4, W)), w.wq("g", (W,), 0.8, 0.3)), {"x": (3, 4, W)})
_bin("b315_141", lambda w: (w.inp("x", (3, 1, 5)), w.wq("g", (1, 4, 1), 0.8, 0.3)), {"x": (3, 1, 5)})
_bin("rank2_rank4", lambda w: (w.wq("g", (H, W), 0.8, 0.3), w.inp("x", (1, 3, H, W))), {"x": (1, 3, H, W)})
_bin("two_pushed", lambda w: (w.inp("x", (1, 3, H, W)), w.inp("y", (1, 3, H, W))), {"x": (1, 3, H, W), "y": (1, 3, H, W)})
_bin("nhwc_lastaxis_W", lambda w: (pre(w, "ca", CO), w.wq("g", (W,), 0.8, 0.3)), INX)          # the general fall-back: both operands made plain


# ---- Sigmoid, Softmax, InstanceNormalization ---------------------------------------------------------------------------------------------------------
add("sigmoid/conv", "lower", (lambda w: w.sigmoid("sig", pre(w, "ca", CO), out="out")), INX)
add("sigmoid/pushed", "lower", (lambda w: w.sigmoid("sig", w.inp("x", X), out="out")), INX)
add("sigmoid/pushed_reshape_transpose", "lower", (lambda w: w.sigmoid("sig", w.transpose("tr", w.reshape("rs", w.inp("x", X), (CI, H, W)), (2, 0, 1)), out="out")), INX)

add("softmax/conv_axis_m1_row7", "lower", (lambda w: w.op("sm", "Softmax", [pre(w, "ca", CO)], {"axis": -1}, out="out")), INX)
add("softmax/matmul_axis_rank_row33", "lower", (lambda w: w.op("sm", "Softmax", [w.op("mm", "MatMul", [w.inp("x", (1, MM, MK)), w.wq("mmw", (MK, 33), 0.5)])], {"axis": 2}, out="out")),
    {"x": (1, MM, MK)})
add("softmax/pushed_row7", "lower", (lambda w: w.op("sm", "Softmax", [w.inp("x", (3, 4, W))], {"axis": 2}, out="out")), {"x": (3, 4, W)})
add("softmax/pushed_row33_default_axis", "lower", (lambda w: w.op("sm", "Softmax", [w.inp("x", (2, 5, 33))], out="out")), {"x": (2, 5, 33)})


def _in(w, x, G, eps=1e-5, name="inorm", out=None):
    rng = np.random.default_rng(_seed("in" + name) + G)
    sc, bi = w.c32(name + "sc", 1.0 + 0.2 * rng.standard_normal(G)), w.c32(name + "bi", 0.2 * rng.standard_normal(G))
    return w.op(name, "InstanceNormalization", [x, sc, bi], None if eps is None else {"epsilon": repr(eps)}, out)


add("instancenorm/G1_pushed_eps", "lower", (lambda w: _in(w, w.inp("x", (1, 1, 35)), 1, 1e-3, out="out")), {"x": (1, 1, 35)})
add("instancenorm/G2_pushed_default_eps", "lower", (lambda w: _in(w, w.inp("x", (1, 2, 35)), 2, None, out="out")), {"x": (1, 2, 35)})
add("instancenorm/G8_conv_eps", "lower", (lambda w: _in(w, w.reshape("rs", pre(w), (1, CI, H * W)), CI, 1e-6, out="out")), INX)


# ---- movement: codes re-arranged, (scale, zero point) carried; a Sigmoid behind each uses the carried parameters -------------------------------------
def _mv_op(w, typ, x):
    if typ == "Reshape":
        return w.reshape("mv", x, (1, x.shape[1], H * W))
    if typ == "Flatten":
        return w.op("mv", "Flatten", [x], {"axis": 1})
    if typ == "Squeeze":
        return w.op("mv", "Squeeze", [x, w.i64("mvax", [0])])
    if typ == "Unsqueeze":
        return w.op("mv", "Unsqueeze", [x, w.i64("mvax", [0])])
    if typ.startswith("Transpose"):
        return w.transpose("mv", x, [int(c) for c in typ[-4:]])
    return w.op("mv", "Resize", [x, None, w.c32("mvsc", [1, 1, int(typ[-1]), int(typ[-1])])], RATTR)


for typ in ("Reshape", "Flatten", "Squeeze", "Unsqueeze", "Transpose0231", "Transpose0312", "Transpose0213", "Resize2", "Resize3"):
    add(f"move/{typ.lower()}_conv", "lower", (lambda w, typ=typ: w.sigmoid("sig", _mv_op(w, typ, pre(w, "ca", CO)), out="out")), INX)
    add(f"move/{typ.lower()}_pushed", "lower", (lambda w, typ=typ: w.sigmoid("sig", _mv_op(w, typ, w.inp("x", X)), out="out")), INX)


# ---- dyn_end: a pushed input read late -----------------------------------------------------------------------------------------------------------------
def _dyn_residual(w):
    x = w.inp("x", X)
    w.op("add", "Add", [w.conv("c1", w.conv("c0", x, CI), CI), x], out="out")


def _dyn_mul(w):
    x = w.inp("x", X)
    w.op("mul", "Mul", [w.sigmoid("sig", x), pre(w, "ca", CI, x)], out="out")


add("dyn/residual_add_at_the_end", "lower", _dyn_residual, INX)
add("dyn/mul_sigmoid_conv", "lower", _dyn_mul, INX)
add("dyn/rearrangement_only", "lower", (lambda w: w.transpose("tr", w.reshape("rs", w.inp("x", X), (CI, H, W)), (1, 2, 0), out="out")), INX)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
NOT_IMPL = "operation not implemented with uint8 arithmetic on the HIP backend: "


def rej(name, body, msg, inputs=INX, **kw):
    add("reject/" + name, "reject", body, inputs, reject=msg, **kw)


rej("sub", lambda w: w.op("bin", "Sub", [pre(w), w.inp("y", X)], out="out"), NOT_IMPL + "Sub", {"x": X, "y": X})
rej("div", lambda w: w.op("bin", "Div", [pre(w), w.inp("y", X)], out="out"), NOT_IMPL + "Div", {"x": X, "y": X})
rej("concat", lambda w: w.op("cat", "Concat", [pre(w), w.inp("y", X)], {"axis": 1}, out="out"), NOT_IMPL + "Concat", {"x": X, "y": X})
rej("softmax_non_last_axis", lambda w: w.op("sm", "Softmax", [w.inp("x", (3, 4, W))], {"axis": 1}, out="out"), "uint8 softmax over a non-last axis", {"x": (3, 4, W)})
rej("conv_group2", lambda w: w.conv("conv", pre(w), CO, attrs={"group": 2}, out="out"), "group != 1 not supported")
rej("conv_dilation2", lambda w: w.conv("conv", pre(w), CO, attrs={"dilations": "2,2"}, out="out"), "dilations != 1 not supported")
rej("conv_3d_input", lambda w: w.op("conv", "Conv", [w.inp("x", (1, CI, W)), w.cq("convw", np.ones((CO, CI, 3, 1), f32), conv=True)],
                                    {"dilations": "1", "group": "1", "kernel_shape": "3", "pads": "1,1", "strides": "1"}, out="out", shape=(1, CO, W)),
    "Conv1D / non 4-D input not implemented", {"x": (1, CI, W)})
rej("conv_kernel_shape_contradicts", lambda w: w.conv("conv", pre(w), CO, kshape="5,3", out="out"), "kernel_shape does not match the weights")
rej("conv_fp16_weight", lambda w: w.conv("conv", pre(w), CO, wdt="float16", out="out"), "wrong data type of W")
rej("conv_bias_of_another_length", lambda w: w.raw("conv", "Conv", [pre(w), w.cq("convw", np.ones((CO, CI, 3, 3), f32), conv=True), w.c32("convb", np.zeros(CO + 1))], Y,
                                                   {"pads": "1,1,1,1"}, out="out"), "wrong data type of B")
rej("conv_bad_pads", lambda w: w.conv("conv", pre(w), CO, attrs={"pads": "1,1"}, out="out"), "invalid pads/strides")
rej("conv_wrong_cin", lambda w: w.op("conv", "Conv", [pre(w), w.cq("convw", np.ones((CO, CI + 1, 3, 3), f32), conv=True)],
                                     {"dilations": "1,1", "group": "1", "kernel_shape": "3,3", "pads": "1,1,1,1", "strides": "1,1"}, out="out", shape=Y), "invalid shape of weights")
rej("conv_one_input", lambda w: w.raw("conv", "Conv", [pre(w)], Y, {"kernel_shape": "3,3"}, out="out"), "wrong number of inputs")
rej("conv_weight_is_activation", lambda w: w.raw("conv", "Conv", [pre(w), w.inp("y", (CO, CI, 3, 3))], Y, {"pads": "1,1,1,1"}, out="out"),
    "weights must be a static *_nchw.bin tensor", {"x": X, "y": (CO, CI, 3, 3)})
rej("conv_unrecognized_attribute", lambda w: w.conv("conv", pre(w), CO, attrs={"auto_pad": "NOTSET"}, out="out"), "Conv: unrecognized attribute: auto_pad")
rej("instancenorm_unrecognized_attribute", lambda w: w.op("inorm", "InstanceNormalization", [w.inp("x", (1, 2, 35)), w.c32("sc", np.ones(2)), w.c32("bi", np.zeros(2))],
                                                          {"epsilon": "1e-05", "momentum": "0.9"}, out="out"), "InstanceNormalization: unrecognized attribute: momentum", {"x": (1, 2, 35)})
rej("softmax_unrecognized_attribute", lambda w: w.raw("sm", "Softmax", [w.inp("x", (3, 4, W))], (3, 4, W), {"axis": "-1", "temperature": "2"}, out="out"),
    "Softmax: unrecognized attribute: temperature", {"x": (3, 4, W)})
rej("instancenorm_4d_input", lambda w: _in(w, pre(w), CI, out="out"), "input shape must be [1,G,L]")
rej("instancenorm_two_inputs", lambda w: w.raw("inorm", "InstanceNormalization", [w.inp("x", (1, 2, 35)), w.c32("sc", np.ones(2))], (1, 2, 35), out="out"), "wrong number of inputs",
    {"x": (1, 2, 35)})
rej("instancenorm_scale_of_another_length", lambda w: w.raw("inorm", "InstanceNormalization", [w.inp("x", (1, 2, 35)), w.c32("sc", np.ones(3)), w.c32("bi", np.zeros(2))], (1, 2, 35),
                                                            out="out"), "invalid scale/bias", {"x": (1, 2, 35)})
rej("broadcast_rank7", lambda w: w.op("bin", "Add", [w.inp("x", (1, 1, 1, 1, 2, 3, 4)), w.wq("g", (4,), 0.8)], out="out"), "rank too large for the device broadcast kernel",
    {"x": (1, 1, 1, 1, 2, 3, 4)})
rej("not_broadcastable", lambda w: w.raw("bin", "Add", [w.inp("x", (3, 4, W)), w.wq("g", (5,), 0.8)], (3, 4, W), out="out"), "shapes are not broadcastable", {"x": (3, 4, W)})
rej("binary_one_input", lambda w: w.raw("bin", "Add", [w.inp("x", (3, 4, W))], (3, 4, W), out="out"), "Add: wrong number of inputs", {"x": (3, 4, W)})
rej("binary_fp32_operand", lambda w: w.raw("bin", "Mul", [w.inp("x", (3, 4, W)), w.c32("g", np.ones(W))], (3, 4, W), out="out"), "Mul: wrong data type of inputs", {"x": (3, 4, W)})
rej("matmul_inner_extents_differ", lambda w: w.raw("mm", "MatMul", [w.inp("x", (MM, MK)), w.wq("mmw", (MK + 1, MNN), 0.5)], (MM, MNN), out="out"), "invalid shape of inputs",
    {"x": (MM, MK)})
rej("matmul_batches_differ", lambda w: w.raw("mm", "MatMul", [w.inp("a", (2, MM, MK)), w.inp("b", (3, MK, MNN))], (2, MM, MNN), out="out"), "invalid shape of inputs",
    {"a": (2, MM, MK), "b": (3, MK, MNN)})
rej("matmul_one_input", lambda w: w.raw("mm", "MatMul", [w.inp("x", (MM, MK))], (MM, MNN), out="out"), "MatMul: wrong number of inputs", {"x": (MM, MK)})
rej("matmul_fp32_operand", lambda w: w.raw("mm", "MatMul", [w.inp("x", (MM, MK)), w.c32("mmw", np.ones((MK, MNN)))], (MM, MNN), out="out"), "MatMul: wrong data type of input",
    {"x": (MM, MK)})
rej("sigmoid_two_inputs", lambda w: w.raw("sig", "Sigmoid", [w.inp("x", X), w.inp("y", X)], X, out="out"), "Sigmoid: wrong number of inputs", {"x": X, "y": X})
rej("softmax_two_inputs", lambda w: w.raw("sm", "Softmax", [w.inp("x", X), w.inp("y", X)], X, out="out"), "Softmax: wrong number of inputs", {"x": X, "y": X})
rej("conv_two_outputs", lambda w: w.raw("conv", "Conv", [pre(w), w.cq("convw", np.ones((CO, CI, 3, 3), f32), conv=True)], Y, {"pads": "1,1,1,1"}, out="out", second_out="out2"),
    "Conv: wrong number of outputs")
rej("matmul_two_outputs", lambda w: w.raw("mm", "MatMul", [w.inp("x", (MM, MK)), w.wq("mmw", (MK, MNN), 0.5)], (MM, MNN), out="out", second_out="out2"),
    "MatMul: wrong number of outputs", {"x": (MM, MK)})
rej("binary_two_outputs", lambda w: w.raw("bin", "Mul", [w.inp("x", (3, 4, W)), w.wq("g", (W,), 0.8)], (3, 4, W), out="out", second_out="out2"), "Mul: wrong number of outputs",
    {"x": (3, 4, W)})
rej("sigmoid_two_outputs", lambda w: w.raw("sig", "Sigmoid", [w.inp("x", X)], X, out="out", second_out="out2"), "Sigmoid: wrong number of outputs")
rej("sigmoid_fp32_input", lambda w: (w.inp("x", X), w.raw("sig", "Sigmoid", [w.c32("c", np.ones(X))], X, out="out"))[1], "Sigmoid: wrong data type of input")
rej("conv_fp32_x", lambda w: (w.inp("x", X), w.raw("conv", "Conv", [w.c32("c", np.ones(X)), w.cq("convw", np.ones((CO, CI, 3, 3), f32), conv=True)], Y, {"pads": "1,1,1,1"}, out="out"))[1],
    "Conv: wrong data type of X")
rej("no_range_data_conv", lambda w: w.conv("conv", pre(w), CO, out="out"), "Conv: range data not found", drop_range=("conv",))
rej("no_range_data_sigmoid", lambda w: w.sigmoid("sig", pre(w), out="out"), "Sigmoid: range data not found", drop_range=("sig",))
rej("three_pushed_samples", lambda w: w.conv("conv", pre(w), CO, out="out"), "Model::run: uint8 arithmetic runs one sample per pass on the HIP backend", opts={"pushes": 3})
rej("conv_two_images", lambda w: w.conv("conv", w.inp("x", (2, CI, H, W)), CO, out="out"), "Conv: uint8 arithmetic runs one sample per pass", {"x": (2, CI, H, W)})


# ======================================================================================================================================
# fuse_u8_instance_norm_nhwc: Reshape[1,G,L] -> InstanceNormalization -> Reshape[x.shape] over a 4-D tensor
# ======================================================================================================================================
P_IN, P_AF = "fuse_u8_instance_norm_nhwc", "fuse_u8_affine_act"
NHWC_MARK, AFF_MARK, NAA_MARK = "InstanceNorm qu8 nhwc inorm", "AffineAct qu8 ", "NormAffineAct qu8 "


def _gn(w, C=CO, G=2, x=None, r0_twice=False, in_extra=None, shape2=None, out="out", L=None, xshape=None):
    x = x if x is not None else pre(w, "ca", C)
    xs = xshape or (1, C, H, W)
    r0 = w.reshape("r0", x, (1, G, L or C * H * W // G))
    i = _in(w, r0, G, out=in_extra)
    y = w.reshape("r1", i, shape2 or xs, out=out)
    if r0_twice:
        w.sigmoid("other", r0, out="out2")
    return y


def _fused_in(w, C=CO, G=2, x=None, xs=None):
    """osg.qu8.InstanceNormNHWC written by hand: what the pass would leave if it took the graph"""
    x = x if x is not None else pre(w, "ca", C)
    rng = np.random.default_rng(_seed("ininorm") + G)
    sc, bi = w.c32("inormsc", 1.0 + 0.2 * rng.standard_normal(G)), w.c32("inormbi", 0.2 * rng.standard_normal(G))
    return w.raw("inorm", "osg.qu8.InstanceNormNHWC", [x, sc, bi], xs or x.shape, {"epsilon": "1e-05", "groups": G}, out="out")


for G, C in ((2, CO), (CO, CO), (56, 56)):
    add(f"u8_in/fires_G{G}_C{C}", "fusion", (lambda w, G=G, C=C: _gn(w, C, G)), INX, pass_=P_IN, expect="fires", present=(NHWC_MARK,))
add("u8_in/G57", "fusion", (lambda w: _gn(w, 57, 57)), INX, pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    why="the NHWC kernel keeps one 256-bin histogram per group in LDS and refuses more than 56 groups (osg_qu8_instance_norm_nhwc): the rewrite would end the run with that "
        "error, not with other codes; held on plan structure")
add("u8_in/first_reshape_read_twice", "fusion", (lambda w: _gn(w, r0_twice=True)), INX, outs=("out", "out2"), pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    wrong={"out2": "unwritten"})
add("u8_in/norm_output_is_extra_output", "fusion", (lambda w: _gn(w, in_extra="normed")), INX, outs=("out", "normed"), pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    wrong={"normed": "unwritten"}, extra=("normed",))
add("u8_in/second_reshape_to_another_shape", "fusion", (lambda w: _gn(w, shape2=(1, CO, W, H))), INX, pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    wrong=("refused", lambda w: _fused_in(w, xs=(1, CO, W, H)), "unexpected shape of output"))
# 6 channels in 4 groups of 6 x 35 / 4 ... does not divide: [1,4,L] with L = 6 * 35 / 4 is no integer.  8 channels on 5 x 6 in 3 groups: L = 80, C % G != 0
add("u8_in/groups_do_not_divide_channels", "fusion", (lambda w: _gn(w, CI, 3, x=pre(w, "ca", CI, w.inp("x", (1, CI, H, 6))), L=80, xshape=(1, CI, H, 6))), {"x": (1, CI, H, 6)},
    pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    wrong=("refused", lambda w: _fused_in(w, CI, 3, x=pre(w, "ca", CI, w.inp("x", (1, CI, H, 6)))), "invalid number of groups"))
add("u8_in/input_of_rank_3", "fusion", (lambda w: _gn(w, CO, 2, x=w.reshape("sq", pre(w, "ca", CO), (CO, H, W)), xshape=(CO, H, W))), INX, pass_=P_IN, expect="left", absent=(NHWC_MARK,),
    wrong=("refused", lambda w: _fused_in(w, CO, 2, x=w.reshape("sq", pre(w, "ca", CO), (CO, H, W))), "input shape must be [1,C,H,W]"))


def _plain_x(w, C=CO):
    """a 4-D tensor in the logical layout with parameters from range data: Add of a pushed input and a reshaped one"""
    return w.op("padd", "Add", [w.inp("x", (1, C, H, W)), w.reshape("prs", w.inp("y", (1, C, H * W)), (1, C, H, W))])


PLAIN_IN = {"x": Y, "y": (1, CO, H * W)}
# the pass fires (the two Reshape steps are gone), the lowering takes the plain [G][L] branch: no "nhwc" launch, no layout copy
add("u8_in/fires_plain_input", "fusion", (lambda w: _gn(w, x=_plain_x(w))), PLAIN_IN, pass_=P_IN, expect="fires", present=("InstanceNorm qu8 inorm",), absent=(NHWC_MARK, "to_nhwc"))


# the fused operator written by hand on a plain input: the [G][L] branch of lower_instance_norm_u8_nhwc, whose plan has the steps of the graph as written
add("u8_in/hand_written_on_plain_input", "lower", (lambda w: _fused_in(w, x=_plain_x(w))), PLAIN_IN)


# ======================================================================================================================================
# fuse_u8_affine_act: Mul(x, gamma[C]) -> Add(., beta[C]) [-> Sigmoid -> Mul(., sigmoid)] over a 4-D tensor
# ======================================================================================================================================
def _aff(w, x=None, gshape=(CO, 1, 1), bshape=None, order="xg", silu=False, sorder="as", gamma=None, beta=None, add_third=False, add_extra=None, mul_extra=None, mul_twice=False,
         other_y=False, add_mm=False, C=CO, out="out"):
    x = x if x is not None else pre(w, "ca", C)
    g = gamma if gamma is not None else w.wq("gam", gshape, 0.4, 1.0)
    b = beta if beta is not None else w.wq("bet", bshape or gshape, 0.5, 0.1)
    last = not silu
    m = w.op("amul", "Mul", [x, g] if order == "xg" else [g, x], out=mul_extra)
    a = w.op("aadd", "Add", ([m, m] if add_mm else [m, b] if order == "xg" else [b, m]), out=(out if last else add_extra))
    if mul_twice:
        w.sigmoid("other", m, out="out2")
    if add_third:
        w.sigmoid("other", a, out="out2")
    if silu:
        s = w.sigmoid("asig", a)
        y = w.sigmoid("ysig", w.inp("y", Y)) if other_y else a
        a = w.op("amul2", "Mul", [y, s] if sorder == "as" else [s, y], out=out)
    return a


def _fused_aff(w, x, g, b, typ="osg.qu8.AffineAct", attrs=None, extra_ins=(), rng_names=("amul", "aadd")):
    for n in rng_names:
        w.ranges[n] = (-2.0, 2.0)
    return w.raw("aadd", typ, [x, g, b] + list(extra_ins), x.shape, attrs if attrs is not None else {"mul": "amul", "add": "aadd"}, out="out", rng=None)


add("u8_affine/mul_add", "fusion", _aff, INX, pass_=P_AF, expect="fires", present=(AFF_MARK + "aadd",), absent=("Mul qu8", "Add qu8"))
for order in ("xg", "gx"):
    for sorder in ("as", "sa"):
        add(f"u8_affine/silu_{order}_{sorder}", "fusion", (lambda w, order=order, sorder=sorder: _aff(w, order=order, silu=True, sorder=sorder)), INX, pass_=P_AF, expect="fires",
            present=(AFF_MARK + "amul2",), absent=("Mul qu8", "Add qu8", "Sigmoid qu8"))
add("u8_affine/gamma_1C11", "fusion", (lambda w: _aff(w, gshape=(1, CO, 1, 1), silu=True)), INX, pass_=P_AF, expect="fires", present=(AFF_MARK + "amul2",), absent=("Mul qu8", "Add qu8"))
add("u8_affine/plain_input", "fusion", (lambda w: _aff(w, x=_plain_x(w), silu=True)), PLAIN_IN, pass_=P_AF, expect="fires", present=(AFF_MARK + "amul2",), absent=("Mul qu8", "Sigmoid qu8"))
add("u8_affine/norm_nhwc", "fusion", (lambda w: _aff(w, x=_gn(w, out=None), silu=True)), INX, pass_=P_AF, expect="fires", present=(NAA_MARK + "amul2",),
    absent=(NHWC_MARK, "Mul qu8", "Add qu8", "Sigmoid qu8"))
add("u8_affine/norm_nhwc_no_silu", "fusion", (lambda w: _aff(w, x=_gn(w, out=None))), INX, pass_=P_AF, expect="fires", present=(NAA_MARK + "aadd",), absent=(NHWC_MARK, "Mul qu8", "Add qu8"))
add("u8_affine/norm_plain", "fusion", (lambda w: _aff(w, x=_gn(w, x=_plain_x(w), out=None), silu=True)), PLAIN_IN, pass_=P_AF, expect="fires",
    present=("InstanceNorm qu8 inorm", AFF_MARK + "amul2"), absent=(NHWC_MARK, NAA_MARK, "Mul qu8", "Sigmoid qu8", "to_nhwc"))

# partial: Mul + Add fuse, the SiLU stays
add("u8_affine/add_read_by_a_third_op", "fusion", (lambda w: _aff(w, silu=True, add_third=True)), INX, outs=("out", "out2"), pass_=P_AF, expect="partial",
    present=(AFF_MARK + "aadd", "Sigmoid qu8 asig", "Mul qu8 amul2"), absent=(AFF_MARK + "amul2",), wrong={"out2": "unwritten"})
add("u8_affine/add_is_extra_output", "fusion", (lambda w: _aff(w, silu=True, add_extra="added")), INX, outs=("out", "added"), pass_=P_AF, expect="partial",
    present=(AFF_MARK + "aadd", "Sigmoid qu8 asig", "Mul qu8 amul2"), absent=(AFF_MARK + "amul2",), wrong={"added": "unwritten"}, extra=("added",))
add("u8_affine/last_mul_of_another_tensor", "fusion", (lambda w: _aff(w, silu=True, other_y=True)), {"x": X, "y": Y}, pass_=P_AF, expect="partial",
    present=(AFF_MARK + "aadd", "Sigmoid qu8 asig", "Mul qu8 amul2"), absent=(AFF_MARK + "amul2",), wrong=lambda w: (w.inp("y", Y), _aff(w, silu=True))[1])

# left
add("u8_affine/gamma_is_an_activation", "fusion", (lambda w: _aff(w, gamma=w.inp("g", (1, CO, 1, 1)))), {"x": X, "g": (1, CO, 1, 1)}, pass_=P_AF, expect="left",
    present=("Mul qu8 amul", "Add qu8 aadd"), absent=(AFF_MARK,),
    why="the one-pass kernel reads gamma's parameters at run time like the Mul launch does and would give the same codes: the guard keeps the pass to operands the planner "
        "knows to be constants; held on plan structure")
# (C == W below: a [W] operand has C elements and is NOT per-channel)
add("u8_affine/gamma_lastaxis_W_equals_C", "fusion", (lambda w: _aff(w, x=pre(w, "ca", W), gshape=(W,), bshape=(W, 1, 1), C=W)), INX, pass_=P_AF, expect="left",
    present=("Mul qu8 amul", "Add qu8 aadd"), absent=(AFF_MARK,), wrong=lambda w: _aff(w, x=pre(w, "ca", W), gshape=(W, 1, 1), bshape=(W, 1, 1), C=W))
add("u8_affine/beta_not_per_channel", "fusion", (lambda w: _aff(w, x=pre(w, "ca", W), gshape=(W, 1, 1), bshape=(W,), C=W)), INX, pass_=P_AF, expect="left",
    present=("Mul qu8 amul", "Add qu8 aadd"), absent=(AFF_MARK,), wrong=lambda w: _aff(w, x=pre(w, "ca", W), gshape=(W, 1, 1), bshape=(W, 1, 1), C=W))
add("u8_affine/gamma_C11_against_rank3", "fusion", (lambda w: _aff(w, x=w.reshape("sq", pre(w, "ca", CO), (CO, H, W)))), INX, pass_=P_AF, expect="left",
    present=("Mul qu8 amul", "Add qu8 aadd"), absent=(AFF_MARK,),
    wrong=("refused", lambda w: _fused_aff(w, w.reshape("sq", pre(w, "ca", CO), (CO, H, W)), w.wq("gam", (CO, 1, 1), 0.4, 1.0), w.wq("bet", (CO, 1, 1), 0.5, 0.1)),
           "input shape must be [1,C,H,W]"))
add("u8_affine/mul_read_twice", "fusion", (lambda w: _aff(w, mul_twice=True)), INX, outs=("out", "out2"), pass_=P_AF, expect="left", present=("Mul qu8 amul", "Add qu8 aadd"),
    absent=(AFF_MARK,), wrong={"out2": "unwritten"})
add("u8_affine/mul_is_extra_output", "fusion", (lambda w: _aff(w, mul_extra="mulled")), INX, outs=("out", "mulled"), pass_=P_AF, expect="left", present=("Mul qu8 amul", "Add qu8 aadd"),
    absent=(AFF_MARK,), wrong={"mulled": "unwritten"}, extra=("mulled",))
add("u8_affine/add_m_m", "fusion", (lambda w: _aff(w, add_mm=True)), INX, pass_=P_AF, expect="left", present=("Mul qu8 amul", "Add qu8 aadd"), absent=(AFF_MARK,),
    wrong=("refused", lambda w: (lambda x: _fused_aff(w, x, w.wq("gam", (CO, 1, 1), 0.4, 1.0), x))(pre(w, "ca", CO)), "invalid shape of the per-channel operands"))


def _norm_twice(w):
    n = _gn(w, out=None)
    w.sigmoid("other", n, out="out2")
    return _aff(w, x=n, silu=True)


add("u8_affine/norm_output_read_twice", "fusion", _norm_twice, INX, outs=("out", "out2"), pass_=P_AF, expect="partial", present=(NHWC_MARK, AFF_MARK + "amul2"), absent=(NAA_MARK,),
    wrong={"out2": "unwritten"})


# ---- the fused operators written by hand: the refusals of their lowerings that no graph of plain operators reaches -----------------------------------------
def _hand(w, **kw):
    x = pre(w, "ca", CO)
    return _fused_aff(w, x, w.wq("gam", (CO, 1, 1), 0.4, 1.0), w.wq("bet", (CO, 1, 1), 0.5, 0.1), **kw)


rej("affine_act_mul_range_missing", lambda w: _hand(w, rng_names=("aadd",)), "osg.qu8.AffineAct: range data not found")
rej("affine_act_add_range_missing", lambda w: _hand(w, rng_names=("amul",)), "osg.qu8.AffineAct: range data not found")
rej("affine_act_fp32_gamma", lambda w: _fused_aff(w, pre(w, "ca", CO), w.c32("gam", np.ones((CO, 1, 1))), w.wq("bet", (CO, 1, 1), 0.5, 0.1)), "osg.qu8.AffineAct: wrong data type of inputs")
rej("norm_affine_act_groups_do_not_divide", lambda w: _hand(w, typ="osg.qu8.NormAffineAct", extra_ins=[w.c32("sc", np.ones(5)), w.c32("bi", np.zeros(5))],
                                                             attrs={"mul": "amul", "add": "aadd", "norm": "aadd", "norm_groups": 5}), "osg.qu8.NormAffineAct: invalid scale/bias")
rej("instance_norm_nhwc_fp32_input_scale_length", lambda w: w.raw("inorm", "osg.qu8.InstanceNormNHWC", [pre(w, "ca", CO), w.c32("sc", np.ones(3)), w.c32("bi", np.zeros(2))], Y,
                                                                   {"groups": 2}, out="out"), "invalid scale/bias")
rej("instance_norm_nhwc_unrecognized_attribute", lambda w: w.raw("inorm", "osg.qu8.InstanceNormNHWC", [pre(w, "ca", CO), w.c32("sc", np.ones(2)), w.c32("bi", np.zeros(2))], Y,
                                                                  {"groups": 2, "momentum": 1}, out="out"), "InstanceNormalization: unrecognized attribute: momentum")
rej("instance_norm_nhwc_range_missing", lambda w: w.raw("inorm", "osg.qu8.InstanceNormNHWC", [pre(w, "ca", CO), w.c32("sc", np.ones(2)), w.c32("bi", np.zeros(2))], Y,
                                                         {"groups": 2}, out="out", rng=None), "osg.qu8.InstanceNormNHWC: range data not found")

PASSES = (P_IN, P_AF)
LEVELS = (0, 1)

# ---- what the reference says about these cases (tools/make_golden_qu8_cases.py prints both lists) ---------------------------------------------------------------
# case -> a substring of the reference's refusal: restatement-only cases
REF_REFUSES = {
    "conv/stride_2_1": "XnnPack::convolution_nhwc_fp32: one or more arguments are invalid.",
    "conv/no_kernel_shape": "Conv: invalid shape of W or invalid kernel_shape (not implemented?).",
    "matmul/w_1nMK": "MatMul: shape of input 0 must have 3 dimensions (not implemented).",
    "u8_in/hand_written_on_plain_input": "Operator not implemented: osg.qu8.InstanceNormNHWC.",
}
# cases where the reference's codes and the interpreter's disagree: must be empty
REF_DIFFERS = {}


# ======================================================================================================================================
# the forward interpreter on codes
# ======================================================================================================================================
def parse_ranges(text):
    out = {}
    for line in text.replace("\r", "\n").split("\n"):
        if line:
            n, lo, hi = line.rsplit(",", 2)
            out[n] = (f32(float(lo)), f32(float(hi)))
    return out


def interpret(d, ranges, inputs, ops=None):
    """d: directory of model.txt and the weight files; ranges: op name -> (lo, hi); inputs: name -> fp32 array as pushed.
    -> tensor name -> (codes in the logical layout, scale, zero point) for every activation of the graph"""
    from oracle import qu8_check as qc
    ops = ops or qc.parse_model(d + "model.txt")
    T = {n: Q.quantize_dynamic(np.asarray(a, f32), threads=1) for n, a in inputs.items()}

    def get(tok):
        if not tok:
            return None
        nm = qc.tname(tok)
        return T[nm] if nm in T else qc.weights_of(d, tok)

    for op in ops:
        t, a = op["type"], op["attrs"]
        v = [get(tok) for tok in op["inputs"]]
        if t in MOVE_TYPES:
            res = (move(t, v[0][0], a, [None if x is None else x[0] for x in v]), v[0][1], v[0][2])
            if t in ("Squeeze", "Unsqueeze"):
                # the reference's Squeeze and Unsqueeze hand on type and data only (src/onnxstream.cpp:3901, :7470): the output tensor keeps scale 0 and zero point 0,
                # and whatever reads it dequantises every code to 0 (tools/make_golden_qu8_cases.py found it; pinned in tests/test_qu8_oracle.py)
                res = (res[0], f32(0.0), 0)
        elif t == "Softmax":
            res = Q.softmax_u8(v[0][0], v[0][1], int(a.get("axis", -1)))
        else:
            so, zo = range_to_scale(*ranges[op["name"]])
            if t == "Conv":
                (x, sx, zx), (wgt, sw, zw) = v[0], v[1]
                y = Q.conv2d_nhwc_u8(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), sx, zx, wgt, sw, zw, v[2][0] if len(v) > 2 and v[2] is not None else None,
                                     recentre(_ints(a.get("pads", "0,0,0,0"))), _ints(a.get("strides", "1,1")), so, zo)
                res = (np.ascontiguousarray(y.transpose(0, 3, 1, 2)), so, zo)
            elif t == "MatMul":
                res = (Q.matmul_u8(*v[0], *v[1], so, zo), so, zo)
            elif t in ("Add", "Mul"):
                y = (Q.add_u8 if t == "Add" else Q.mul_u8)(*v[0], *v[1], so, zo)
                res = (np.broadcast_to(y, np.broadcast_shapes(v[0][0].shape, v[1][0].shape)), so, zo)
            elif t == "Sigmoid":
                res = (Q.sigmoid_u8(*v[0], so, zo), so, zo)
            elif t == "InstanceNormalization":
                res = (Q.instance_norm_u8(*v[0], v[1][0], v[2][0], float(a.get("epsilon", 1e-5)), so, zo), so, zo)
            elif t == "osg.qu8.InstanceNormNHWC":          # (written by hand: Reshape[1,G,L] -> InstanceNormalization -> Reshape back, which is what the pass replaces)
                x = v[0][0]
                y = Q.instance_norm_u8(np.ascontiguousarray(x).reshape(1, int(a["groups"]), -1), v[0][1], v[0][2], v[1][0], v[2][0], float(a.get("epsilon", 1e-5)), so, zo)
                res = (y.reshape(x.shape), so, zo)
            else:
                raise KeyError(t)
        T[qc.tname(op["outputs"][0])] = (np.ascontiguousarray(res[0]), f32(res[1]), int(res[2]))
    return T


def deq(codes, scale, zp):
    """(float32)((int)q - zp) * scale: what both the device and the reference hand back for a uint8 tensor"""
    return ((codes.astype(np.int32) - int(zp)).astype(f32) * f32(scale)).astype(f32)


# ---- tests/golden/qu8_cases.npz: "ranges|<case>" the range-data text of EVERY case; "index" [[<case>|<tensor>, shape, scale, zero point], ...] and "ref" the reference's
# dequantised values of these tensors (sample 0, logical layout), fp32, one after the other
_GOLDEN = None
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qu8_cases.npz")


def load_golden(path=None):
    import json
    z = np.load(path or GOLDEN)
    ranges = {k.split("|", 1)[1]: str(z[k]) for k in z.files if k.startswith("ranges|")}
    ref, at = {}, 0
    for key, shape, scale, zp in json.loads(bytes(z["index"]).decode()):
        n = int(np.prod(shape, dtype=np.int64))
        ref[key] = (z["ref"][at:at + n].reshape(shape), f32(scale), int(zp))
        at += n
    assert at == z["ref"].size
    return ranges, ref


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden()
    return _GOLDEN


def range_text(case):
    return golden()[0][case.name]


def reference(case, name):
    """(the reference's dequantised tensor, scale, zero point) of sample 0, or None where the file does not hold it"""
    return golden()[1].get(f"{case.name}|{name}")


_WANT = {}


def want(case, k=0, body=None):
    """the interpreter's {tensor: (codes, scale, zp)} for sample k under the stored range data; computed once per case and sample, left unchanged"""
    key = (case.name, k)
    if body is None and key in _WANT:
        return _WANT[key]
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        case.emit(d, body)
        res = interpret(d, parse_ranges(range_text(case)), case.sample(k))
    for v in res.values():
        v[0].setflags(write=False)
    if body is None:
        _WANT[key] = res
    return res


# ---- running a case through the product library (the stub backend where OSGPU_LIB names it, the device otherwise) --------------------------------------
def run(case, level, passes=None, extra=(), body=None, ranges=None, step_lines=False):
    """-> (one {name: fp32 array or None} per pass, the `what` of every plan step -- step_lines: the whole line, reads and writes included --, launches of the last pass);
    raises OnnxStreamError with the refusal's message"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    passes = passes if passes is not None else [case.sample(0)]
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        case.emit(d, body)
        open(d + "range_data.txt", "w", newline="").write(ranges if ranges is not None else range_text(case))
        m = Model(b.LIB_HOST, 1, "ram+nocache")          # threads = 1: the chunking of a pushed input's percentiles follows the thread count
        try:
            m.hip_read_range_data(d + "range_data.txt")
            m.set_use_uint8_arithmetic(True)
            m._set_option("hip_fusion_level", level)
            if "vram_budget" in case.opts:
                m.hip_set_vram_budget(case.opts["vram_budget"])
            m.read_file(d + "model.txt")
            m.mangle_tensor_names = False
            names = tuple(case.outs) + tuple(e for e in extra if e not in case.outs)
            for e in names:
                if e not in case.outs or e in case.extra:
                    m.add_extra_output(e)
            outs = []
            for ins in passes:
                for _ in range(case.opts.get("pushes", 1)):
                    for n, a in ins.items():
                        m.add_tensor(n, a)
                m.run()
                got = {n: m.get_tensor(n) for n in names}
                outs.append({n: (None if v is None else v[0]) for n, v in got.items()})
                m.clear_tensors()
            what = [line if step_lines else line.split(" | ", 1)[1] for line in m.hip_plan_info().splitlines() if line.startswith("step ")]
            launches = m.hip_last_kernel_count()
            assert "vram_budget" not in case.opts or m.hip_streamed_bytes() > 0, (case.name, "no weight travelled through the streaming ring")
        finally:
            m.close()
    return outs, what, launches


def check_plan(case, level, what, with_extra=True):
    """-> the failures of the plan's step names against the case's expectation (empty: as expected)"""
    text, bad = "\n".join(what), []
    if level == 0 or case.kind != "fusion":
        bad += [f"level {level}: fused step in the plan: {s}" for s in what if any(m in s for m in FUSED) and (level == 0 or case.kind != "fusion")]
        return bad
    bad += [f"not in the plan: {s}" for s in case.present if s not in text]
    bad += [f"in the plan: {s}" for s in case.absent if s in text]
    return bad
