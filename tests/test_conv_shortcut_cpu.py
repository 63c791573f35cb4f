"""CPU: fuse_conv_shortcut (option hip_fuse_shortcut) -- a ResNet's 3x3 conv2 and its 1x1 conv_shortcut planned as ONE launch of
osg_conv2d_nhwc_cat -- on the no-op stand-in for libosgpu.so (tests/stub/make_stub.py).  Structure only: which pairs fuse at full size, what the fused step
declares, which near misses stay two launches, how the sampler-loop frame classifies the fused steps, and the host-only arithmetic of the kernel's second K
segment (osg_conv3x3_cat_plan.h) through a stand-alone program built with the host sanitizers.  The numbers are tests/test_conv_shortcut_gpu.py's business."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import sd_unet
from onnxstream_amd.synth.graph import DirSink, GraphBuilder

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "stub"))

f32 = np.float32
ON = (("hip_fuse_shortcut", 1),)

# the 14 ResNets of SD 1.5 whose channel count changes
FUSED_SD15 = sorted(["/down_blocks.1/resnets.0/conv2", "/down_blocks.2/resnets.0/conv2"] + [f"/up_blocks.{b}/resnets.{r}/conv2" for b in range(4) for r in range(3)])


@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    old = {k: os.environ.get(k) for k in ("OSGPU_LIB", make_stub.TRACE_ENV)}
    with tempfile.TemporaryDirectory() as d:
        os.environ.pop(make_stub.TRACE_ENV, None)
        os.environ["OSGPU_LIB"] = make_stub.build(d)
        try:
            yield d
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def _plan(model_dir, inputs, options=(), pushes=1, outs=()):
    """-> (Model, plan steps, the named outputs as the stub leaves them)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m.read_file(model_dir + "model.txt")
    for k, v in options:
        m._set_option(k, v)
    for _ in range(pushes):
        for k, v in inputs.items():
            m.add_tensor(k, v)
    m.set_use_fp16_arithmetic(True)
    m.set_fuse_ops_in_attention(True)
    m.run()
    got = [m.get_tensor(o)[0] for o in outs]
    return m, _steps(m.hip_plan_info()), got


def _steps(info):
    steps = []
    for line in info.splitlines():
        if line.startswith("step "):
            head, what = line.split(" | ", 1)
            f = dict(kv.split("=") for kv in head.split()[2:])
            steps.append(dict(i=int(head.split()[1]), what=what, reads=[int(v) for v in f["reads"].split(",") if v], writes=[int(v) for v in f["writes"].split(",") if v]))
    return steps


def _sd15_dir():
    d = os.path.join(os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth"), "sd15") + "/"
    if not os.path.exists(d + ".complete"):
        os.makedirs(d, exist_ok=True)
        sd_unet.build_unet(DirSink(d), sd_unet.SD15)
        open(d + ".complete", "w").write("ok")
    return d


def test_full_size_sd15_fuses_the_14_shortcuts_and_the_default_plan_is_the_parents(stub_backend):
    d = _sd15_dir()
    ins = sd_unet.unet_inputs(sd_unet.SD15, 42)
    m, off, _ = _plan(d, ins, (), pushes=2)
    m.close()
    m, on, _ = _plan(d, ins, ON, pushes=2)
    m.close()
    assert len(off) == 275 and not any("+shortcut" in s["what"] for s in off)
    assert sum("conv_shortcut" in s["what"] for s in off) == 14
    assert len(on) == 261 and not any("conv_shortcut" in s["what"] for s in on)
    fused = [s for s in on if "+shortcut" in s["what"]]
    assert sorted(s["what"].split(" ")[1] for s in fused) == FUSED_SD15
    assert all(s["what"].startswith("Conv ") and s["what"].split(" ")[2] == "+shortcut" for s in fused)
    # with the option off the launch list is the one without it; with it on, only the 28 launches of the 14 pairs differ
    gone = [s["what"] for s in off if "conv_shortcut" in s["what"]]
    rest_on = [s["what"].replace(" +shortcut", "") for s in on]
    assert [w for w in (s["what"] for s in off) if w not in gone] == rest_on
    # each fused step reads x, the tensor its shortcut read: the value is written by an earlier step and stays allocated until the fused step has run
    off_by = {s["what"].split(" ")[1]: s for s in off if s["what"].startswith("Conv ")}
    for s in fused:
        name = s["what"].split(" ")[1]
        sc_off = off_by[name.replace("/conv2", "/conv_shortcut")]
        x_writer_off = [t["what"] for t in off if sc_off["reads"][0] in t["writes"]]
        x_writers_on = [t for t in on if t["i"] < s["i"] and t["what"] in x_writer_off]
        assert x_writers_on, name
        assert any(w in s["reads"] for t in x_writers_on for w in t["writes"]), (name, s["reads"])
        assert len(s["reads"]) == 5                                   # h, W2, x, Ws, the f32 sum of the two biases


# ---- one ResNet tail in miniature: out = conv3x3(h) + conv1x1(x), at the 8 x 8 level of sd_unet.TINY (64 channels, concatenated input of 128) -------------------
C_TINY = sd_unet.TINY.block_out[2]


def _pair(sink, cin2=2 * C_TINY, sc_stride=1, k=3, dil=1, twice=False, quant=False):
    g = GraphBuilder(sink, quant_weights=quant)
    hw = 8
    x = g.input("x", (1, cin2, hw * sc_stride, hw * sc_stride))
    h = g.input("h", (1, C_TINY, hw, hw))
    c = g.conv("/res/conv2", h, C_TINY, k, pad=dil * (k // 2))     # (the order of sd_unet's resnet: conv2, then the shortcut, then the Add)
    if dil != 1:
        g.lines[-1] = g.lines[-1].replace("dilations:1,1", f"dilations:{dil},{dil}")
    s = g.conv("/res/conv_shortcut", x, C_TINY, 1, stride=sc_stride)
    y = g.op("/res/Add_1", "Add", [s, c], (1, C_TINY, hw, hw), out_names=None if twice else ["out"])
    if twice:
        g.op("/res/Add_2", "Add", [y, s], (1, C_TINY, hw, hw), out_names=["out"])
    g.finish()
    rng = np.random.default_rng(7)
    return {"x": rng.standard_normal((1, cin2, hw * sc_stride, hw * sc_stride)).astype(f32), "h": rng.standard_normal((1, C_TINY, hw, hw)).astype(f32)}


def _both(stub_dir, extra=(), **kw):
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        ins = _pair(DirSink(d), **kw)
        res = []
        for opts in (extra, extra + ON):
            m, steps, got = _plan(d, ins, opts, outs=("out",))
            m.close()
            res.append(([s["what"] for s in steps], got[0]))
        return res


def test_the_miniature_pair_fuses(stub_backend):
    (off, y0), (on, y1) = _both(stub_backend)
    assert sorted(w for w in off if w.startswith("Conv")) == ["Conv /res/conv2", "Conv /res/conv_shortcut"]
    assert [w for w in on if w.startswith("Conv")] == ["Conv /res/conv2 +shortcut"]
    assert len(on) == len(off) - 1 and np.array_equal(y0, y1)


@pytest.mark.parametrize("case,kw,extra", [
    ("shortcut_stride_2", dict(sc_stride=2), ()),
    ("shortcut_read_twice", dict(twice=True), ()),
    ("conv2_is_1x1", dict(k=1), ()),
    ("cin2_96", dict(cin2=96), ()),
    ("w8_resident", dict(quant=True), (("hip_w8_resident", 1),)),
    ("fusion_level_1", dict(), (("hip_fusion_level", 1),)),
])
def test_near_misses_stay_two_launches(stub_backend, case, kw, extra):
    (off, y0), (on, y1) = _both(stub_backend, extra=extra, **kw)
    assert on == off, case
    assert sum(w.split(" ")[0] == "Conv" for w in on) == 2 and not any("+shortcut" in w for w in on)
    assert np.array_equal(y0, y1)


def _two_pairs(sink, bias):
    """two ResNet tails of different widths in one graph: out = conv3x3(h) + conv1x1(x) with 64 channels, out2 the same with 128"""
    g = GraphBuilder(sink)
    x = g.input("x", (1, 2 * C_TINY, 8, 8))
    h = g.input("h", (1, C_TINY, 8, 8))
    h2 = g.input("h2", (1, 2 * C_TINY, 8, 8))
    for nm, hh, cout, out in (("/a", h, C_TINY, "out"), ("/b", h2, 2 * C_TINY, "out2")):
        c = g.conv(nm + "/conv2", hh, cout, 3, bias=bias)
        s = g.conv(nm + "/conv_shortcut", x, cout, 1, bias=bias)
        g.op(nm + "/Add_1", "Add", [s, c], (1, cout, 8, 8), out_names=[out])
    g.finish()
    rng = np.random.default_rng(8)
    return {k: rng.standard_normal(sh).astype(f32) for k, sh in (("x", (1, 2 * C_TINY, 8, 8)), ("h", (1, C_TINY, 8, 8)), ("h2", (1, 2 * C_TINY, 8, 8)))}


@pytest.mark.parametrize("bias", [False, True])
def test_two_fused_pairs_of_different_widths_keep_their_own_bias(stub_backend, bias):
    """without biases a fused launch takes NO bias operand (no derived constant, so two pairs cannot meet in one); with them each pair reads a constant of its own"""
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        ins = _two_pairs(DirSink(d), bias)
        m, steps, got = _plan(d, ins, ON, outs=("out", "out2"))
        m.close()
    fused = [s for s in steps if "+shortcut" in s["what"]]
    assert [s["what"] for s in fused] == ["Conv /a/conv2 +shortcut", "Conv /b/conv2 +shortcut"]
    assert [len(s["reads"]) for s in fused] == [5 if bias else 4] * 2                 # h, W2, x, Ws (+ the f32 bias sum)
    if bias:
        assert fused[0]["reads"][4] != fused[1]["reads"][4]
    assert got[0].shape[1] == C_TINY and got[1].shape[1] == 2 * C_TINY


def test_dilation_2_is_refused_by_the_lowering_either_way(stub_backend):
    """the backend lowers no dilated convolution at all: the pair is not fused into something that would hide the refusal"""
    msgs = []
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        ins = _pair(DirSink(d), dil=2)
        for opts in ((), ON):
            with pytest.raises(Exception) as e:
                m, _, _ = _plan(d, ins, opts)
                m.close()
            msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "dilations" in msgs[0]


def test_fused_steps_are_sample_dependent_in_the_sampler_loop_frame(stub_backend):
    import test_loop_hoist_cpu as lh
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_unet.build_unet(DirSink(d), sd_unet.TINY)
        ins = sd_unet.unet_inputs(sd_unet.TINY, 42)
        m = lh._model(d, ins, ON)
        steps = lh._steps(m.hip_plan_info())
        fused = [i for i, s in enumerate(steps) if "+shortcut" in s["what"]]
        assert len(fused) == 2                                       # up_blocks.2 resnets.0 / .1: 128 -> 64 channels at 8 x 8 (resnets.2 reads 96 channels: left alone)
        lh._loop(m, ins)
        head, cls, st = lh._check_classes_and_homes(m, steps)
        m.close()
        taint = lh._taint(steps)
        for i in fused:
            assert i not in cls and taint[i] & 1, steps[i]["what"]     # the sample reaches it: it stays in the per-step graph
        assert st["step_launches"] == len(steps) - len(cls)


def test_slice_partition_and_barrier_counts_under_the_host_sanitizers():
    """tools/conv_cat_plan_check.cpp: for every entry x splits 1..5 x Cin2 / 64 in 1..40 the slices cover the unit list exactly once and both roles count
    the same barriers -- a stand-alone program with its own main, built with -fsanitize=address,undefined"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "conv_cat_plan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"),
                               os.path.join(REPO, "tools", "conv_cat_plan_check.cpp"), "-o", exe])
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0, out.stdout
        assert "OK" in out.stdout
