"""CPU: the loop hoist of the device sampler loops (option hip_loop_hoist) -- which plan steps leave the sampler step, where their
results live, what the loops still hand the backend -- on the no-op stand-in for libosgpu.so (tests/stub/make_stub.py, generated with its opt-in
trace as tests/test_sampler_loop_trace_cpu.py does).  Structure only: the numbers are the GPU tests' business (tests/test_loop_hoist_gpu.py).

The classes are re-derived here from the plan's own step list (Model.hip_plan_info: reads / writes per step) and compared with what the host
library reports (Model.hip_loop_hoist_info), so the test does not take the library's word for the dependence analysis."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import sd_unet
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))

f32 = np.float32
IO = ("sample", "timestep", "out_sample")
T5 = np.array([901.0, 702.5, 500.25, 901.0, 702.5], f32)


@pytest.fixture(scope="module")
def traced_stub():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    old = {k: os.environ.get(k) for k in ("OSGPU_LIB", make_stub.TRACE_ENV)}
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        os.environ[make_stub.TRACE_ENV] = d + "trace.txt"
        os.environ["OSGPU_LIB"] = make_stub.build(d + "stub")
        try:
            yield d + "trace.txt"
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def _model(model_dir, ins, options=()):
    """a Model whose plan of two samples has run twice: the second run() records the pass"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m.read_file(model_dir + "model.txt")
    for k, v in options:
        m._set_option(k, v)
    for _ in range(2):
        for _ in range(2):
            for k, v in ins.items():
                m.add_tensor(k, v)
        m.set_use_fp16_arithmetic(True)
        m.set_fuse_ops_in_attention(True)
        m.run()
        m.clear_tensors()
    return m


def _loop(m, ins, t=T5):
    n = len(t)
    x = np.zeros((1,) + ins["sample"].shape[1:], f32)
    s = [np.linspace(0.5 + k, 1.5 + k, n).astype(f32) for k in range(5)]
    assert m.hip_sampler_loop(*IO, x, np.ones((n,) + x.shape, f32), s[0], s[1], np.asarray(t, f32), s[2], s[3], s[4], 7.0, None) == 0.0


def _trace_since(path, start):
    with open(path) as f:
        f.seek(start)
        return [ln.split(" ") for ln in f.read().splitlines()]


def _steps(plan_info):
    steps = []
    for line in plan_info.splitlines():
        if line.startswith("step "):
            head, what = line.split(" | ", 1)
            f = dict(kv.split("=") for kv in head.split()[2:])
            steps.append(dict(what=what, reads=[int(v) for v in f["reads"].split(",") if v], writes=[int(v) for v in f["writes"].split(",") if v]))
    return steps


def _hoist(info):
    cls, vals, head = {}, {}, {}
    for line in info.splitlines():
        w = line.split()
        if line.startswith("hoist ready="):
            head = {k: int(v) for k, v in (kv.split("=") for kv in w[1:])}
        elif line.startswith("arena "):
            head["arena"] = tuple(int(kv.split("=")[1]) for kv in w[1:])
        elif line.startswith("hoist P step ") or line.startswith("hoist T step "):
            cls[int(w[3])] = (w[1], line.split(" | ", 1)[1])
        elif line.startswith("hoist val "):
            f = {k: int(v) for k, v in (kv.split("=") for kv in w[5:])}
            vals[int(w[2])] = (f["base"], f["bytes"], int(w[4]))
    return head, cls, vals


def _taint(steps):
    """the two bits per step, from the step list alone: 1 = the sample reaches it, 2 = the timestep does"""
    (s_in,) = [s for s in steps if s["what"] == "input sample"]
    (t_in,) = [s for s in steps if s["what"] == "input timestep"]
    bits = {s_in["reads"][0]: 1, t_in["reads"][0]: 2}
    out = []
    for s in steps:
        b = 0
        for r in s["reads"]:
            b |= bits.get(r, 0)
        for w in s["writes"]:
            bits[w] = bits.get(w, 0) | b
        out.append(b)
    return out


def _check_classes_and_homes(m, steps):
    head, cls, vals = _hoist(m.hip_loop_hoist_info())
    taint = _taint(steps)
    writers = {}
    for i, s in enumerate(steps):
        for w in set(s["writes"]):
            writers.setdefault(w, []).append(i)
    for i, (c, what) in cls.items():
        assert what == steps[i]["what"]
        assert taint[i] & 1 == 0 and c == ("T" if taint[i] & 2 else "P"), (i, what, taint[i], c)
        for w in steps[i]["writes"]:
            assert writers[w] == [i] and w in vals, (i, what, w)
        for r in steps[i]["reads"]:           # what a hoisted step reads is never computed by the per-step part
            assert all(j in cls for j in writers.get(r, [])), (i, what, r)
    # every value a hoisted step writes: outside the arena, and no two share a byte
    a0, an = head["arena"]
    spans = sorted((b, b + n) for b, n, _ in vals.values())
    for lo, hi in spans:
        assert hi <= a0 or lo >= a0 + an, (lo, hi, a0, an)
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo
    st = m.hip_loop_hoist_stats()
    assert st["p_steps"] == sum(c == "P" for c, _ in cls.values()) and st["t_steps"] == sum(c == "T" for c, _ in cls.values())
    assert st["step_launches"] == m.hip_last_kernel_count() - len(cls) == len(steps) - len(cls)
    return head, cls, st


def test_full_size_sd15_hoists_the_prompt_and_timestep_launches(traced_stub):
    d = os.path.join(os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth"), "sd15") + "/"
    if not os.path.exists(d + ".complete"):
        os.makedirs(d, exist_ok=True)
        sd_unet.build_unet(DirSink(d), sd_unet.SD15)
        open(d + ".complete", "w").write("ok")
    ins = sd_unet.unet_inputs(sd_unet.SD15, 42)
    m = _model(d, ins)
    steps = _steps(m.hip_plan_info())
    assert m.hip_loop_hoist_stats()["step_launches"] == 0          # nothing is classified before a loop call names the two inputs
    _loop(m, ins)
    head, cls, st = _check_classes_and_homes(m, steps)
    m.close()
    names = {c: sorted(w for k, w in cls.values() if k == c) for c in "PT"}
    att = "/down_blocks.0/attentions.0/transformer_blocks.0/attn2/"
    assert names["P"] == sorted(["input encoder_5F_hidden_5F_states", "Linear merged(32) " + att + "to_k", "KVPack x5 " + att + "MatMul_Attention_TBlockTail"])
    assert names["T"] == sorted(["input timestep", "Mul /time_proj/Mul", "Sin /time_proj/Sin", "Cos /time_proj/Cos", "Concat /time_proj/Concat",
                                 "Gemm /time_embedding/linear_1", "Gemm /time_embedding/linear_2", "Linear merged(22) /down_blocks.0/resnets.0/time_emb_proj"])
    assert len(steps) == 275 and st["step_launches"] == 264
    assert head["row_bytes"] == 2 * 20160 * 2 and head["epoch_keyed"] == 0     # a row is the merged time_emb_proj output; the timestep is all it depends on
    assert st["extra_bytes"] < 20 << 20


@pytest.fixture(scope="module")
def tiny(traced_stub):
    with tempfile.TemporaryDirectory() as d:
        out = {}
        for cfg in (sd_unet.TINY, sd_unet.TINY_XL):
            sub = d + "/" + cfg.name + "/"
            os.makedirs(sub)
            sd_unet.build_unet(DirSink(sub), cfg)
            out[cfg.name] = (sub, sd_unet.unet_inputs(cfg, 42))
        yield out


def test_xl_added_embedding_is_prompt_class_and_keys_the_rows_by_epoch(tiny):
    d, ins = tiny["tinyxl"]
    m = _model(d, ins)
    steps = _steps(m.hip_plan_info())
    _loop(m, ins)
    head, cls, st = _check_classes_and_homes(m, steps)
    kind = {w: c for c, w in cls.values()}
    for w in ("input text_5F_embeds", "input time_5F_ids", "Concat /add_embedding/Concat", "Gemm /add_embedding/linear_1", "Gemm /add_embedding/linear_2"):
        assert kind[w] == "P", w
    assert kind["Add /Add_emb"] == "T"                              # time embedding + added embedding: what time_emb_proj reads
    assert [w for w in kind if w.startswith("Linear merged") and w.endswith("time_emb_proj")] and all(
        kind[w] == "T" for w in kind if w.endswith("time_emb_proj"))
    assert head["epoch_keyed"] == 1
    e0 = m.hip_loop_hoist_stats()
    assert e0["rows"] == 3
    m.hip_set_input("text_embeds", 0, ins["text_embeds"])
    e1 = m.hip_loop_hoist_stats()
    assert e1["epoch"] == e0["epoch"] + 1
    m.hip_set_input("sample", 0, ins["sample"])                     # the loop's own inputs are no reason to drop rows
    assert m.hip_loop_hoist_stats()["epoch"] == e1["epoch"]
    _loop(m, ins)
    e2 = m.hip_loop_hoist_stats()
    m.close()
    assert (e0["t_hits"], e0["t_misses"]) == (2, 3) and (e2["t_hits"], e2["t_misses"], e2["rows"]) == (2, 3, 3)   # the rows of the old epoch were dropped


def test_primed_loop_call_still_traces_three_lines_per_step(tiny, traced_stub):
    d, ins = tiny["tiny"]
    m = _model(d, ins)
    m.hip_sampler_schedule(T5)
    for call in range(2):
        start = os.path.getsize(traced_stub)
        _loop(m, ins)
        lines = _trace_since(traced_stub, start)
        st = m.hip_loop_hoist_stats()
        assert (st["t_hits"], st["t_misses"], st["rows"]) == (5, 0, 3)
        assert len(lines) == 3 * len(T5), [ln[0] for ln in lines]
        for i in range(len(T5)):
            assert [ln[0] for ln in lines[3 * i:3 * i + 3]] == ["osg_sampler_prepare", "osg_graph_launch", "osg_sampler_cfg_euler_a"]
        assert len({ln[1] for ln in lines[1::3]}) == 1 and lines[1][1].startswith("g=0x")
    m.close()


def test_option_off_is_the_plan_and_the_loop_of_before(tiny, traced_stub):
    d, ins = tiny["tiny"]
    infos, traces = [], []
    for opts in ((), (("hip_loop_hoist", 0),)):
        m = _model(d, ins, opts)
        infos.append(m.hip_plan_info())
        start = os.path.getsize(traced_stub)
        _loop(m, ins)
        lines = _trace_since(traced_stub, start)
        # pointers differ from Model to Model: entry points and every scalar argument are compared
        traces.append([[f for f in ln if "=0x" not in f or "p" in f.split("=")[1]] for ln in lines])
        st = m.hip_loop_hoist_stats()
        after = m.hip_plan_info()
        m.close()
        if opts:
            assert st["p_steps"] == st["t_steps"] == st["step_launches"] == st["extra_bytes"] == st["rows"] == 0
            assert after == infos[-1]                               # no value left the arena
    assert infos[0] == infos[1]                                     # launch list, arena placement and size
    assert traces[0] == traces[1] and len(traces[0]) == 3 * len(T5)


def test_changing_the_option_rebuilds_the_plan(tiny):
    d, ins = tiny["tiny"]
    m = _model(d, ins)
    built = m.hip_plans_built()
    m._set_option("hip_loop_hoist", 0)
    for _ in range(2):
        for k, v in ins.items():
            m.add_tensor(k, v)
    m.run()
    assert m.hip_plans_built() == built + 1
    m.close()
