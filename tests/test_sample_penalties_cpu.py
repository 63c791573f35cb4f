"""Repetition, presence and frequency penalties and min-p in the device token loop, CPU side: the host logic over the no-op stand-in for libosgpu.so
(tests/stub/make_stub.py).  Its launches compute nothing, so no token is ever drawn; what can be checked here is what the host does around the loop:

* include/osgpu.h declares the five new entry points beside the old ones, whose signatures stand, and the host library exports the three _ext calls;
* every refusal of the three calls, each with its own prefix;
* the launches of a call, as the stand-in built here records them (the token-loop entry points are given bodies that note their name and the arguments
  that matter): with the controls off -- through the old exports, through the _ext exports with a NULL struct, and through the _ext exports with a
  struct of defaults -- exactly the launches the loop always made; with them on, the count of the history, step 0 before every pick, the _ext pick or
  sample with the count table; min-p alone: the _ext sample without a table and without step 0;
* the decode plan: not rebuilt, and its text unchanged, by the controls;
* the Python defaults route to the exports without the suffix."""
import ctypes
import dataclasses
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import llama
from onnxstream_amd.synth.graph import DirSink

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))
CFG = dataclasses.replace(llama.TINY, max_pos=256, name="llama_tiny_long")
PROMPT = [3, 17, 42, 5, 9]
NC = 2 * CFG.layers
PREFIXES = {"generate": "Model::hip_generate: ", "batch": "Model::hip_generate_batch: ", "turn": "Model::hip_turn: "}

NOTE_HELPERS = r"""
#include <stdio.h>
char stub_log[1 << 16];
int stub_log_len = 0;
static void stub_note(const char* s) {
    const size_t n = strlen(s);
    if (stub_log_len + n + 2 >= sizeof stub_log) return;
    memcpy(stub_log + stub_log_len, s, n);
    stub_log_len += (int)n;
    stub_log[stub_log_len++] = '\n';
    stub_log[stub_log_len] = 0;
}
"""
BODIES = {
    "osg_decode_pick": '{ stub_note("pick"); return 0; }',
    "osg_decode_sample": '{ stub_note("sample"); return 0; }',
    "osg_decode_sample_batch": '{ stub_note("sample_batch"); return 0; }',
    "osg_decode_pick_ext": '{ stub_note(counts ? "pick_ext counts" : "pick_ext"); return 0; }',
    "osg_decode_sample_ext": '{ char b[128]; snprintf(b, sizeof b, "sample_ext min_p=%a%s", (double)min_p, counts ? " counts" : ""); stub_note(b); return 0; }',
    "osg_decode_sample_batch_ext": '{ char b[128]; snprintf(b, sizeof b, "sample_batch_ext n_seq=%d min_p=%a%s", n_seq, (double)min_p, counts ? " counts" : ""); '
                                   'stub_note(b); return 0; }',
    "osg_decode_penalize": '{ char b[256]; snprintf(b, sizeof b, "penalize n_seq=%d V=%ld stride=%ld r=%a inv_r=%a presence=%a frequency=%a zero=%d", n_seq, V, '
                           'row_stride, (double)r, (double)inv_r, (double)presence, (double)frequency, counts[0] == 0 && counts[(long)n_seq * V - 1] == 0); '
                           'stub_note(b); return 0; }',
    "osg_decode_count": '{ char b[512]; int k = snprintf(b, sizeof b, "count V=%ld tokens", V); for (long i = 0; i < n && k < 480; i++) '
                        'k += snprintf(b + k, sizeof b - k, " %lld", (long long)tokens[i]); stub_note(b); return 0; }',
}


@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    with tempfile.TemporaryDirectory() as d:
        old_special, old_helpers = dict(make_stub.SPECIAL), make_stub.HALF_HELPERS
        make_stub.SPECIAL.update(BODIES)
        make_stub.HALF_HELPERS = old_helpers + NOTE_HELPERS
        try:
            so = make_stub.build(d)
        finally:
            make_stub.SPECIAL.clear()
            make_stub.SPECIAL.update(old_special)
            make_stub.HALF_HELPERS = old_helpers
        old = os.environ.get("OSGPU_LIB")
        os.environ["OSGPU_LIB"] = so
        try:
            yield ctypes.CDLL(so)          # (the same loaded image the host library binds: its log is the one read below)
        finally:
            if old is None:
                os.environ.pop("OSGPU_LIB", None)
            else:
                os.environ["OSGPU_LIB"] = old


@pytest.fixture(scope="module")
def model_dir():
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        llama.build_llama(DirSink(d), CFG)
        yield d


def _model(model_dir, prefill=True):
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    m = Model(b.LIB_HOST, 1, "ram+nocache")
    m.add_outputs_convert("logits")
    llama.configure(m, CFG, model_dir, sdpa=True, upcast=True)
    if prefill:
        llama.forward_resident(m, CFG, PROMPT, True, 0, keep_logits=True)
    return m


def _log(lib, reset=True):
    text = ctypes.string_at(ctypes.addressof(ctypes.c_char.in_dll(lib, "stub_log")), ctypes.c_int.in_dll(lib, "stub_log_len").value).decode()
    if reset:
        ctypes.c_int.in_dll(lib, "stub_log_len").value = 0
    return text.splitlines()


def _parse(line):
    """a noted launch as (name, {argument: value}): %a floats come back exactly, bare words are flags"""
    name, *rest = line.split()
    if name == "count":
        return name, dict(V=int(rest[0][2:]), tokens=[int(t) for t in rest[2:]])
    args = {}
    for w in rest:
        k, _, v = w.partition("=")
        args[k] = True if not _ else float.fromhex(v) if "x" in v or v in ("inf", "nan") else int(v)
    return name, args


def f32v(x):
    return float(np.float32(x))


def test_the_entry_points_are_declared_and_the_calls_are_exported():
    from onnxstream_amd import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "osgpu.h")).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int osg_decode_count(osg_ctx* ctx, const int64_t* tokens, long n, int* counts, long V);" in flat
    assert ("int osg_decode_penalize(osg_ctx* ctx, const float* rows, long row_stride, long V, int n_seq, const int* counts, float* out, float r, float inv_r, "
            "float presence, float frequency);") in flat
    old = {"osg_decode_pick": "int osg_decode_pick(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, "
                              "int64_t* position_ids, int64_t* tokens, long max_tokens",
           "osg_decode_sample": "int osg_decode_sample(osg_ctx* ctx, const float* logits, long T, long V, long long eos_id, int* state, int64_t* input_ids, "
                                "int64_t* position_ids, int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p, unsigned long long seed, "
                                "unsigned long long draw_base",
           "osg_decode_sample_batch": "int osg_decode_sample_batch(osg_ctx* ctx, const float* logits, long V, int n_seq, long long eos_id, int* state, "
                                      "int64_t* input_ids, int64_t* position_ids, int64_t* tokens, long max_tokens, float temperature, long top_k, float top_p, "
                                      "const unsigned long long* seeds, unsigned long long draw_base"}
    for name, decl in old.items():
        assert decl + ");" in flat, name                                               # the old signature stands
        tail = ", int* counts);" if name == "osg_decode_pick" else ", float min_p, int* counts);"
        assert decl.replace(name + "(", name + "_ext(") + tail in flat, name              # the _ext one is the old one plus min_p and the counts
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    lib = ctypes.CDLL(b.LIB_HOST)
    for name in ("model_hip_generate", "model_hip_generate_sampled", "model_hip_generate_batch", "model_hip_turn", "model_hip_generate_sampled_ext",
                 "model_hip_generate_batch_ext", "model_hip_turn_ext"):
        assert hasattr(lib, name), name


def _call(m, kind, **kw):
    if kind == "generate":
        kw.setdefault("temperature", 0.8)
        return m.generate(kw.pop("max_new", 4), NC, **kw)
    if kind == "batch":
        return m.generate_batch(2, kw.pop("max_new", 4), NC, [1, 2], kw.pop("temperature", 0.8), **kw)
    kw.setdefault("temperature", 0.8)
    return m.turn([1, 2], kw.pop("max_new", 4), NC, **kw)


@pytest.mark.parametrize("kind", ["generate", "batch", "turn"])
def test_refusals(stub_backend, model_dir, kind):
    from onnxstream_amd.bindings import OnnxStreamError
    pfx = re.escape(PREFIXES[kind])
    m = _model(model_dir)
    for r in (float("nan"), 0.0, -1.5, float("inf"), float("-inf"), 1e-45, 1e39):          # (the reciprocal of the subnormal is infinite in fp32; 1e39 is inf in fp32)
        with pytest.raises(OnnxStreamError, match=pfx + "repetition_penalty must be > 0 and finite"):
            _call(m, kind, repetition_penalty=r)
    for name in ("presence_penalty", "frequency_penalty"):
        for v in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(OnnxStreamError, match=pfx + name + " must be finite"):
                _call(m, kind, **{name: v})
    for p in (float("nan"), -0.01, 1.01, float("inf")):
        with pytest.raises(OnnxStreamError, match=pfx + r"min_p must be in \[0, 1\]"):
            _call(m, kind, min_p=p)
    if kind != "batch":          # (a batch refuses temperature == 0 by itself, before it looks at min_p)
        with pytest.raises(OnnxStreamError, match=pfx + "min_p needs temperature > 0"):
            _call(m, kind, min_p=0.1, temperature=0.0)
    for bad in ([CFG.vocab], [0, 1, -1], [2 ** 40]):
        with pytest.raises(OnnxStreamError, match=pfx + "history token " + str(bad[-1]) + " at " + str(len(bad) - 1) + r" is outside \[0, " + str(CFG.vocab) + r"\)"):
            _call(m, kind, history=bad)
    with pytest.raises(OnnxStreamError, match=pfx + r"n_history \+ max_new must be below 2\^24"):
        _call(m, kind, history=np.zeros(2 ** 24 - 4, np.int64), presence_penalty=0.5)
    # negative presence and frequency penalties are allowed, and so are the boundaries of min_p
    _call(m, kind, presence_penalty=-0.5, frequency_penalty=-0.25, min_p=1.0, history=[0, CFG.vocab - 1])
    _call(m, kind, min_p=0.0, repetition_penalty=0.5)
    m.close()


def _raw_ext(m, kind, ext, **over):
    """the three _ext exports called directly, as a C caller would: `ext` a bindings.SampleExt or None (NULL)"""
    from onnxstream_amd.bindings import SampleExt
    cp, ip, llp = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    names = [m._name(x) for x in ("input_ids", "position_ids", "attention_mask", "logits", "pkv", "opkv")]
    toks = (ctypes.c_longlong * 16)()
    n, stop, ms = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), ctypes.c_double(0)
    head = [ctypes.c_void_p, cp, cp, cp, cp, cp, cp, ctypes.c_int]
    tail = [ctypes.c_float, ctypes.c_longlong, ctypes.c_float]
    extp = ctypes.byref(ext) if ext is not None else None
    temperature = over.get("temperature", 0.8)
    m.set_use_fp16_arithmetic(True)
    if kind == "generate":
        f = m._lib.model_hip_generate_sampled_ext
        f.argtypes = head + [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, llp, ip, ip, fp, dp] + tail + [ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(SampleExt)]
        args = [4, -1, 0, toks, n, stop, None, ctypes.byref(ms), temperature, 0, 1.0, 5, 0, extp]
    elif kind == "batch":
        f = m._lib.model_hip_generate_batch_ext
        f.argtypes = head + [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, llp, ip, ip, fp, dp] + tail + [ctypes.POINTER(ctypes.c_ulonglong),
                                                                                                                    ctypes.c_ulonglong, ctypes.POINTER(SampleExt)]
        args = [2, 4, -1, 0, toks, n, stop, None, ctypes.byref(ms), temperature, 0, 1.0, (ctypes.c_ulonglong * 2)(1, 2), 0, extp]
    else:
        f = m._lib.model_hip_turn_ext
        f.argtypes = head + [llp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, llp, ip, ip, fp, dp] + tail + [
            ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(SampleExt)]
        args = [(ctypes.c_longlong * 2)(1, 2), 2, 32, 0, 4, -1, 0, toks, n, stop, None, ctypes.byref(ms), temperature, 0, 1.0, 5, 0, extp]
    f.restype = ctypes.c_void_p
    m._err(f(m._h, *names, NC, *args))


@pytest.mark.parametrize("kind", ["generate", "batch", "turn"])
def test_launches_plan_and_the_null_struct(stub_backend, model_dir, kind):
    from onnxstream_amd.bindings import OnnxStreamError, SampleExt
    lib = stub_backend
    V = CFG.vocab
    old_launch = {"generate": "sample", "batch": "sample_batch", "turn": "sample"}[kind]
    n_seq = 2 if kind == "batch" else 1
    m = _model(model_dir)
    _log(lib)
    # ---- the parent's call: four launches of the old entry point, nothing else of the token loop's ----
    _call(m, kind)
    parent = _log(lib)
    assert parent == [old_launch] * 4
    built, info = m.hip_plans_built(), m.hip_decode_plan_info()
    # ---- the _ext export with NULL, and with a struct of defaults (and an empty, and a non-empty history): the same launches ----
    _raw_ext(m, kind, None)
    assert _log(lib) == parent
    _raw_ext(m, kind, SampleExt(1.0, 0.0, 0.0, 0.0, None, 0))
    assert _log(lib) == parent
    _call(m, kind, history=[1, 2, 3])          # (a history without a penalty: checked, then unused -- no table is built)
    assert _log(lib) == parent
    if kind != "batch":
        _call(m, kind, temperature=0.0, history=[])
        assert _log(lib) == ["pick"] * 4
    # NULL history with n_history > 0, n_history < 0: only a C caller can say that
    for ext, msg in ((SampleExt(1.0, 0.0, 0.0, 0.0, None, 3), r"no history tokens \(n_history > 0\)"), (SampleExt(1.0, 0.0, 0.0, 0.0, None, -1), "n_history must be >= 0")):
        with pytest.raises(OnnxStreamError, match=re.escape(PREFIXES[kind]) + msg):
            _raw_ext(m, kind, ext)
    _log(lib)
    # ---- min-p alone: the _ext sample, no table, no step 0 ----
    _call(m, kind, min_p=0.05)
    sample = ("sample_batch_ext", dict(n_seq=2, min_p=f32v(0.05))) if kind == "batch" else ("sample_ext", dict(min_p=f32v(0.05)))
    assert [_parse(ln) for ln in _log(lib)] == [sample] * 4
    # ---- penalties: the history counted once per sequence into a zeroed table, then step 0 and the _ext sample with the table, four times ----
    history = [7, 7, 9, V - 1]
    _call(m, kind, repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=-0.1, min_p=0.05, history=history)
    got = [_parse(ln) for ln in _log(lib)]
    pen = ("penalize", dict(n_seq=n_seq, V=V, stride=V, r=f32v(1.1), inv_r=f32v(np.float32(1.0) / np.float32(1.1)), presence=f32v(0.2), frequency=f32v(-0.1), zero=1))
    assert got[:n_seq] == [("count", dict(V=V, tokens=history))] * n_seq
    with_table = (sample[0], dict(sample[1], counts=True))
    assert got[n_seq:] == [pen, with_table] * 4          # (zero=1: the stand-in counts nothing, so the table is as the host zeroed it)
    # ---- a turn counts its prompt when no history is given (the Python surface; the export adds nothing by itself) ----
    if kind == "turn":
        m.turn([4, 5, 6], 2, NC, temperature=0.8, presence_penalty=1.0)
        assert _log(lib)[0] == f"count V={V} tokens 4 5 6"
        ext = SampleExt(1.0, 1.0, 0.0, 0.0, None, 0)
        _raw_ext(m, kind, ext)
        assert [ln.split()[0] for ln in _log(lib)] == ["penalize", "sample_ext"] * 4
    else:
        _call(m, kind, presence_penalty=1.0)          # generate / generate_batch: history=None is nothing
        assert [ln.split()[0] for ln in _log(lib)] == ["penalize", "sample_batch_ext" if kind == "batch" else "sample_ext"] * 4
    # ---- greedy with a penalty: the _ext pick over the adjusted row ----
    if kind != "batch":
        _call(m, kind, temperature=0.0, repetition_penalty=1.3, history=[5])
        pen = ("penalize", dict(n_seq=1, V=V, stride=V, r=f32v(1.3), inv_r=f32v(np.float32(1.0) / np.float32(1.3)), presence=0.0, frequency=0.0, zero=1))
        assert [_parse(ln) for ln in _log(lib)] == [("count", dict(V=V, tokens=[5]))] + [pen, ("pick_ext", dict(counts=True))] * 4
    # ---- none of this has touched the decode plan: not rebuilt, the same text ----
    if kind != "turn":          # (a turn's prompts lengthen the conversation: its plans grow with it, controls or none)
        assert m.hip_plans_built() == built
    assert m.hip_decode_plan_info() == info
    m.close()


def test_the_python_defaults_route_to_the_old_exports(stub_backend, model_dir):
    m = _model(model_dir)

    class Spy:
        def __init__(self, lib):
            self._lib, self.seen = lib, []

        def __getattr__(self, name):
            if name.startswith("model_hip_generate") or name.startswith("model_hip_turn"):
                self.seen.append(name)
            return getattr(self._lib, name)

    spy = Spy(m._lib)
    m._lib = spy
    try:
        llama.generate(m, CFG, 2)
        llama.generate(m, CFG, 2, temperature=0.8)
        llama.generate_batch(m, CFG, 2, 2, temperature=0.8, seed=3)
        llama.turn(m, CFG, [1, 2], 2, temperature=0.8)
        assert spy.seen == ["model_hip_generate", "model_hip_generate_sampled", "model_hip_generate_batch", "model_hip_turn"]
        del spy.seen[:]
        llama.generate(m, CFG, 2, repetition_penalty=1.2)          # greedy with a penalty goes through the sampled _ext export, temperature 0
        llama.generate(m, CFG, 2, temperature=0.8, min_p=0.1)
        llama.generate_batch(m, CFG, 2, 2, temperature=0.8, seed=3, frequency_penalty=0.1)
        llama.turn(m, CFG, [1, 2], 2, temperature=0.8, presence_penalty=0.1)
        llama.generate(m, CFG, 2, history=[1])
        assert spy.seen == ["model_hip_generate_sampled_ext", "model_hip_generate_sampled_ext", "model_hip_generate_batch_ext", "model_hip_turn_ext",
                            "model_hip_generate_sampled_ext"]
    finally:
        m._lib = spy._lib
    m.close()
