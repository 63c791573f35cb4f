"""GPU: the device sampler loops with the loop hoist (option hip_loop_hoist) against the same loops without it, bit for bit.

With the hoist on, a loop call launches per step only the plan steps that depend on the latent; the prompt-only steps run once per call and the
timestep-only steps once per timestep value, their results kept in a table of rows.  Every launch that runs is one of the full pass's launches with the
same arguments on the same data, so nothing may differ: each case runs two Models that differ in hip_loop_hoist alone, on the same inputs, and compares
the latents the loop returns -- and the pass's output tensor where a case is about run() -- as bit patterns.  TINY and TINY_XL (whose timestep branch
also reads text_embeds / time_ids through the added embedding: the table is keyed by the input epoch) with two samples per pass."""
import os
import tempfile

import numpy as np
import pytest

from onnxstream_amd.synth import sd_unet
from onnxstream_amd.synth.graph import DirSink

pytestmark = pytest.mark.gpu

f32 = np.float32
IO = ("sample", "timestep", "out_sample")
STEPS = 5
# timestep values per step: the fourth and fifth repeat the first two, so a table of two rows sees stored misses, an unstored miss and hits
T5 = np.array([901.0, 702.5, 500.25, 901.0, 702.5], f32)
MS_DPMPP_2M_ORDERS = [0, 1, 1, 1, 1]
ST_EULER, ST_SDE0, ST_SDE1, ST_SDE2 = 2, 5, 6, 7


@pytest.fixture(scope="module")
def graphs():
    with tempfile.TemporaryDirectory() as d:
        out = {}
        for cfg in (sd_unet.TINY, sd_unet.TINY_XL):
            sub = d + "/" + cfg.name + "/"
            os.makedirs(sub)
            sd_unet.build_unet(DirSink(sub), cfg)
            out[cfg.name] = (sub, cfg)
        yield out


def _inputs(cfg, seeds=(42, 43)):
    return [sd_unet.unet_inputs(cfg, s) for s in seeds]


def _run(m, pushes):
    for ins in pushes:
        for k, v in ins.items():
            m.add_tensor(k, v)
    m.set_use_fp16_arithmetic(True)
    m.set_fuse_ops_in_attention(True)
    m.run()
    out = np.stack([m.get_tensor("out_sample", i)[0] for i in range(len(pushes))])
    m.clear_tensors()
    return out


def _model(graph, hoist, rows=None, pushes=None):
    """a Model whose plan of two samples has run twice (the second run() captures the pass)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    d, cfg = graph
    m = Model(b.LIB_HOST, 0, "ram+nocache")
    m.read_file(d + "model.txt")
    m._set_option("hip_loop_hoist", hoist)
    if rows is not None:
        m._set_option("hip_loop_hoist_rows", rows)
    for _ in range(2):
        _run(m, pushes or _inputs(cfg))
    return m


def _scal(seed, n):
    return np.random.default_rng(seed).uniform(0.4, 1.2, n).astype(f32)


def _x(cfg, prompts, seed=7):
    return np.random.default_rng(seed).standard_normal((prompts, cfg.in_ch, cfg.latent, cfg.latent)).astype(f32)


def _euler_pair(m, cfg, t, seed=0):
    n = len(t)
    x = _x(cfg, 1, 7 + seed)
    noise = np.random.default_rng(100 + seed).standard_normal((n,) + x.shape).astype(f32)
    m.hip_sampler_loop(*IO, x, noise, _scal(1, n), -_scal(2, n), np.asarray(t, f32), _scal(3, n), -0.1 * _scal(4, n), 0.05 * _scal(5, n), 7.3, None)
    return x


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def reference(graphs):
    """the Euler-A pair loop over T5 without the hoist: computed once, read by every case that runs the same call"""
    m = _model(graphs["tiny"], 0)
    x = _euler_pair(m, graphs["tiny"][1], T5)
    st = m.hip_loop_hoist_stats()
    m.close()
    assert np.isfinite(x).all() and x.any()
    assert st["p_steps"] == st["t_steps"] == st["step_launches"] == st["extra_bytes"] == 0
    return x


@pytest.mark.parametrize("variant", ["unprimed", "primed", "two_rows"])
def test_euler_a_pair_matches_the_full_pass_per_step(graphs, reference, variant):
    g = graphs["tiny"]
    m = _model(g, 1, rows=2 if variant == "two_rows" else None)
    if variant == "primed":
        m.hip_sampler_schedule(T5)
    x = _euler_pair(m, g[1], T5)
    st = m.hip_loop_hoist_stats()
    kernels = m.hip_last_kernel_count()
    m.close()
    assert _same(x, reference)
    assert st["p_steps"] > 0 and st["t_steps"] > 0 and st["step_launches"] == kernels - st["p_steps"] - st["t_steps"]
    # unprimed: three distinct values miss, their repeats hit; primed: nothing misses; two rows: the third value misses and is not kept
    assert (st["t_hits"], st["t_misses"], st["rows"]) == {"unprimed": (2, 3, 3), "primed": (5, 0, 3), "two_rows": (2, 3, 2)}[variant]


@pytest.mark.parametrize("how", ["run", "set_input"])
def test_a_changed_context_reaches_the_next_loop_call(graphs, how):
    """the prompt-only launches (context conversion, merged K|V projection, K/V packs) are not kept across calls"""
    g = graphs["tiny"]
    cfg = g[1]
    first, other = _inputs(cfg), _inputs(cfg, (52, 53))
    got = []
    for hoist in (0, 1):
        m = _model(g, hoist, pushes=first)
        m.hip_sampler_schedule(T5)
        a = _euler_pair(m, cfg, T5)
        if how == "run":
            _run(m, [dict(ins, encoder_hidden_states=o["encoder_hidden_states"]) for ins, o in zip(first, other)])
        else:
            for i, o in enumerate(other):
                m.hip_set_input("encoder_hidden_states", i, o["encoder_hidden_states"])
        b = _euler_pair(m, cfg, T5, seed=1)
        m.close()
        got.append((a, b))
    assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])
    assert not _same(got[0][0], got[0][1])


def test_one_step_call_then_four_step_call(graphs, reference):
    """a loop cut at an image boundary: the chunks see the rows and the prompt-only values of their own call"""
    g = graphs["tiny"]
    got = []
    for hoist in (0, 1):
        m = _model(g, hoist)
        a = _euler_pair(m, g[1], T5[:1])
        b = _euler_pair(m, g[1], T5[1:], seed=1)
        m.close()
        got.append((a, b))
    assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])


@pytest.mark.parametrize("family", ["multistep", "stochastic"])
def test_single_forms_of_the_other_loop_families(graphs, family):
    """DPM++ 2M and a stochastic loop (SDE forms with history, noise on some steps), one sample per prompt, two prompts"""
    g = graphs["tiny"]
    cfg = g[1]
    got = []
    for hoist in (0, 1):
        m = _model(g, hoist)
        m.hip_sampler_schedule(T5[:3])
        x = _x(cfg, 2)
        if family == "multistep":
            coef = (0.3 * _scal(20, STEPS * 6)).reshape(STEPS, 6)
            dcoef = _scal(21, STEPS * 2).astype(np.float64).reshape(STEPS, 2)
            m.hip_sampler_loop_multistep_single(*IO, x, 0, _scal(1, STEPS), -_scal(2, STEPS), T5, _scal(3, STEPS), MS_DPMPP_2M_ORDERS, coef, dcoef)
        else:
            coef = (0.3 * _scal(40, STEPS * 10)).reshape(STEPS, 10)
            coef[:, 9] = [1, 1.5, 1, 0.75, 1]
            noise = np.random.default_rng(9).standard_normal((STEPS,) + x.shape).astype(f32)
            m.hip_sampler_loop_stochastic_single(*IO, x, _scal(1, STEPS), -_scal(2, STEPS), T5, _scal(3, STEPS), [ST_SDE0, ST_SDE1, ST_SDE2, ST_SDE2, ST_EULER],
                                                 [1, 0, 1, 1, 0], coef, noise)
        st = m.hip_loop_hoist_stats()
        m.close()
        assert np.isfinite(x).all() and x.any()
        assert (st["t_steps"] > 0) == bool(hoist)
        got.append(x)
    assert _same(got[0], got[1])


def test_xl_rows_follow_the_added_embedding_inputs(graphs):
    """TINY_XL: the timestep branch adds the embedding of text_embeds / time_ids, so a row is only valid for the inputs it was computed from"""
    g = graphs["tinyxl"]
    cfg = g[1]
    first, other = _inputs(cfg), _inputs(cfg, (52, 53))
    got = []
    for hoist in (0, 1):
        m = _model(g, hoist, pushes=first)
        m.hip_sampler_schedule(T5)
        a = _euler_pair(m, cfg, T5)
        e0 = m.hip_loop_hoist_stats()
        for i, o in enumerate(other):
            m.hip_set_input("text_embeds", i, o["text_embeds"])
        b = _euler_pair(m, cfg, T5, seed=1)
        e1 = m.hip_loop_hoist_stats()
        info = m.hip_loop_hoist_info()
        m.close()
        if hoist:
            assert "epoch_keyed=1" in info
            assert e1["epoch"] > e0["epoch"]
            assert (e0["t_hits"], e0["t_misses"]) == (5, 0) and (e1["t_hits"], e1["t_misses"]) == (2, 3)      # the primed rows were dropped
        got.append((a, b))
    assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])
    assert not _same(got[0][0], got[0][1])


def test_run_after_a_loop_call_is_the_pass_of_a_fresh_model(graphs):
    """the full captured pass, recorded anew on the moved buffers, computes what it computed before"""
    g = graphs["tiny"]
    cfg = g[1]
    probe = _inputs(cfg, (62, 63))
    fresh = _model(g, 1)
    want = _run(fresh, probe)
    fresh.close()
    m = _model(g, 1)
    m.hip_sampler_schedule(T5)
    _euler_pair(m, cfg, T5)
    got = _run(m, probe)
    m.hip_replay(1)
    m.close()
    assert np.isfinite(want).all() and _same(got, want)
