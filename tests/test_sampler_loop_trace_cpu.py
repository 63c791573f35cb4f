"""What the three device sampler loops (model_hip_sampler_loop, _multistep, _stochastic and their *_single forms) hand the backend, step by step.

The no-op stand-in for libosgpu.so computes nothing, so the plumbing tests cannot see which pointers and scalars a loop passes to the kernels.  Here the
stand-in is generated with its opt-in trace (tests/stub/make_stub.py, OSGPU_STUB_TRACE): every osg_sampler_* call and every osg_graph_launch appends
one line with its arguments, floats as %a.  Each case runs once as the guidance pair (one prompt) and once as the single form (two prompts) on a plan
of two samples over the TINY UNet, and the trace is checked against the documented contract of the loops (plan.h, exports.cpp, include/osgpu.h) --
never against a recorded run:

* per step exactly one prepare entry (which one: the rules of the loop family), the captured pass, one update entry with the step's form;
* every per-step scalar is the caller's array entry, bit for bit;
* x, sample, timestep, eps and the graph are the same pointers at every step; prompts, L and t_per_sample are constant;
* the noise pointer is NULL at a step that draws none, else a fixed base + i * prompts * L * 4;
* history, relationally: a pointer h_k the form reads is the h0 of step i - k and nothing wrote over it since, a pointer it does not read is NULL, and
  h0 differs from every h_k of its own step (but for DPM++ 2M, whose ring has one slot by design); DDIM passes no history."""
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
STEPS = 5
GUIDANCE = 7.3
# osg_multistep_form and osg_stochastic_form, include/osgpu.h
MS_DPMPP_FIRST, MS_DPMPP_2M, MS_EULER_D, MS_IPNDM1, MS_IPNDM_V1, MS_IPNDM2, MS_IPNDM3, MS_IPNDM_VO1, MS_IPNDM_VO2, MS_IPNDM_VO3, MS_TAYLOR1, MS_TAYLOR2, \
    MS_DDIM = range(13)
ST_EULER, ST_SDE0, ST_SDE1, ST_SDE2 = 2, 5, 6, 7
# the update form of each (sampler, order) of model_hip_sampler_loop_multistep
MS_FORMS = {
    0: [MS_DPMPP_FIRST, MS_DPMPP_2M, MS_EULER_D],
    1: [MS_EULER_D, MS_IPNDM1, MS_IPNDM2, MS_IPNDM3],
    2: [MS_EULER_D, MS_IPNDM_V1, MS_IPNDM2, MS_IPNDM3],
    3: [MS_EULER_D, MS_IPNDM_VO1, MS_IPNDM_VO2, MS_IPNDM_VO3],
    4: [MS_EULER_D, MS_TAYLOR1, MS_TAYLOR2],
    5: [MS_DDIM],
}
# orders that reach each sampler's deepest form (sampler 0: order 2 is the last-step Euler form, which reads no history)
MS_ORDERS = {0: [0, 1, 1, 1, 2], 1: [0, 1, 2, 3, 3], 2: [0, 1, 2, 3, 3], 3: [0, 1, 2, 3, 3], 4: [0, 1, 2, 2, 2], 5: [0, 0, 0, 0, 0]}


def _scalars(seed, n=STEPS, dtype=f32):
    """n distinct values that no shorter format holds exactly: a scalar taken from another step, or rounded on the way, shows"""
    return (np.random.default_rng(seed).uniform(0.1, 3.0, n)).astype(dtype)


class Traced:
    def __init__(self, model, path, sample_shape):
        self.m, self.path, self.shape = model, path, sample_shape
        self.L = int(np.prod(sample_shape[1:]))

    def x(self, prompts):
        return np.zeros((prompts,) + tuple(self.shape[1:]), f32)

    def call(self, fn, *args, **kw):
        """the trace lines of one loop call: [(entry point, {param: value})]; pointers and integers as int (NULL = 0), floats exactly"""
        start = os.path.getsize(self.path) if os.path.exists(self.path) else 0
        assert fn(*args, **kw) == 0.0
        with open(self.path) as f:
            f.seek(start)
            lines = f.read().splitlines()
        out = []
        for ln in lines:
            name, *kv = ln.split(" ")
            d = {}
            for item in kv:
                k, v = item.split("=")
                d[k] = 0 if v == "(nil)" else float.fromhex(v) if "p" in v else int(v, 16) if v.startswith("0x") else int(v)
            out.append((name, d))
        return out


@pytest.fixture(scope="module")
def traced():
    import make_stub
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    old = {k: os.environ.get(k) for k in ("OSGPU_LIB", make_stub.TRACE_ENV)}
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        os.environ[make_stub.TRACE_ENV] = d + "trace.txt"
        os.environ["OSGPU_LIB"] = make_stub.build(d + "stub")
        try:
            ins = sd_unet.unet_inputs(sd_unet.TINY, 42)
            sd_unet.build_unet(DirSink(d), sd_unet.TINY)
            m = Model(b.LIB_HOST, 0, "ram+nocache")
            m.read_file(d + "model.txt")
            for _ in range(2):                       # a plan of TWO samples; the second run() captures the pass the loops then launch
                for _ in range(2):
                    for k, v in ins.items():
                        m.add_tensor(k, v)
                m.set_use_fp16_arithmetic(True)
                m.set_fuse_ops_in_attention(True)
                m.run()
                m.clear_tensors()
            yield Traced(m, d + "trace.txt", ins["sample"].shape)
            m.close()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def _eq(got, want):
    """bit for bit: the traced double is the float the entry point received"""
    return got == float(want) and np.signbit(got) == np.signbit(want)


def check_frame(tr, lines, prompts, pair, c_in, t, prepare, update, draws):
    """The contract every loop shares.  prepare(i) -> (entry point, x_scale or None); update(i) -> (entry point, {scalar: value}); draws[i]: the step
    is handed noise.  Returns the update entries for the loop's own (history) checks."""
    assert len(lines) == 3 * STEPS, [n for n, _ in lines]
    ups = []
    for i in range(STEPS):
        (pn, pa), (gn, ga), (un, ua) = lines[3 * i:3 * i + 3]
        want_p, x_scale = prepare(i)
        assert pn == want_p and gn == "osg_graph_launch", (i, pn, gn, un)
        assert ("x_scale" in pa) == (x_scale is not None)
        if x_scale is not None:
            assert _eq(pa["x_scale"], x_scale), (i, pa["x_scale"], x_scale)
        assert _eq(pa["c_in"], c_in[i]) and _eq(pa["t"], t[i]), (i, pa)
        want_u, scal = update(i)
        assert un == want_u, (i, un)
        for k, v in scal.items():
            assert _eq(ua[k], v), (i, k, ua[k], v)
        assert ("guidance" in ua) == pair
        if pair:
            assert _eq(ua["guidance"], f32(GUIDANCE))
        for a in (pa, ua):
            assert a["prompts"] == prompts and a["L"] == tr.L
        ups.append(ua)
    p0, g0, u0 = lines[0][1], lines[1][1], lines[2][1]
    assert p0["x"] and p0["sample"] and p0["timestep"] and u0["eps"] and g0["g"] and p0["t_per_sample"] > 0
    assert len({p0["x"], p0["sample"], p0["timestep"], u0["eps"]}) == 4
    for i in range(STEPS):
        pa, ga, ua = lines[3 * i][1], lines[3 * i + 1][1], lines[3 * i + 2][1]
        assert all(pa[k] == p0[k] for k in ("x", "sample", "timestep", "t_per_sample")) and ga["g"] == g0["g"]
        assert ua["x"] == p0["x"] and ua["eps"] == u0["eps"]
    if draws is not None:
        bases = set()
        for i, ua in enumerate(ups):
            if draws[i]:
                assert ua["noise"]
                bases.add(ua["noise"] - i * prompts * tr.L * 4)
            else:
                assert ua["noise"] == 0
        assert len(bases) <= 1
    return ups


def check_history(ups, hs, reads, writes, one_slot=False):
    """hs: the update's history parameters, h0 first; reads[i]: how many earlier entries step i's form reads; writes[i]: whether it writes h0"""
    for i, ua in enumerate(ups):
        assert bool(ua[hs[0]]) == bool(writes[i]), (i, ua)
        for k in range(1, len(hs)):
            if k > reads[i]:
                assert ua[hs[k]] == 0, (i, k)
                continue
            assert ua[hs[k]] and ua[hs[k]] == ups[i - k][hs[0]], (i, k)
            for j in range(i - k + 1, i + 1):          # ... and no step since, this one included, has written over it
                if not (one_slot and j == i):
                    assert ups[j][hs[0]] != ua[hs[k]], (i, k, j)


PAIRS = [pytest.param(True, id="pair"), pytest.param(False, id="single")]


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("with_noise_and_clip", [True, False])
def test_euler_a(traced, pair, with_noise_and_clip):
    tr, prompts = traced, 1 if pair else 2
    x = tr.x(prompts)
    c_in, c_out, t, sigma, d_sigma, sigma_up = (_scalars(s) for s in range(6))
    noise = np.ones((STEPS,) + x.shape, f32) if with_noise_and_clip else None
    clip = _scalars(6) if with_noise_and_clip else None
    if pair:
        lines = tr.call(tr.m.hip_sampler_loop, *IO, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, GUIDANCE, clip)
    else:
        lines = tr.call(tr.m.hip_sampler_loop_single, *IO, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, clip)

    def update(i):
        return ("osg_sampler_cfg_euler_a" if pair else "osg_sampler_euler_a_single",
                {"c_out": c_out[i], "sigma": sigma[i], "d_sigma": d_sigma[i], "sigma_up": sigma_up[i], "clip": clip[i] if clip is not None else f32(0)})

    # Euler-A never rescales x: the pair takes the plain prepare, the single form is handed x_scale = 1
    check_frame(tr, lines, prompts, pair, c_in, t, lambda i: ("osg_sampler_prepare", None) if pair else ("osg_sampler_prepare_single", f32(1)), update,
                [with_noise_and_clip] * STEPS)
    assert not x.any()


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("sampler", range(6))
def test_multistep(traced, pair, sampler):
    tr, prompts = traced, 1 if pair else 2
    x = tr.x(prompts)
    c_in, c_out, t, sigma = (_scalars(10 + s) for s in range(4))
    order = MS_ORDERS[sampler]
    coef = _scalars(20, STEPS * 6).reshape(STEPS, 6)
    if sampler == 5:
        coef[:, 5] = [1, 1.5, 1, 1.5, 1]             # DDIM's pair rescales at every step, also where the factor is 1
    dcoef = _scalars(21, STEPS * 2, np.float64).reshape(STEPS, 2)
    if pair:
        lines = tr.call(tr.m.hip_sampler_loop_multistep, *IO, x, sampler, c_in, c_out, t, sigma, order, coef, dcoef, GUIDANCE)
    else:
        lines = tr.call(tr.m.hip_sampler_loop_multistep_single, *IO, x, sampler, c_in, c_out, t, sigma, order, coef, dcoef)

    def prepare(i):
        if not pair:
            return "osg_sampler_prepare_single", coef[i, 5] if sampler == 5 else f32(1)      # (the other samplers' column 5 is not a prescale)
        return ("osg_sampler_prepare_rescale", coef[i, 5]) if sampler == 5 else ("osg_sampler_prepare", None)

    def update(i):
        scal = {"c_out": c_out[i], "sigma": sigma[i], "da": dcoef[i, 0], "db": dcoef[i, 1]}
        scal.update({f"k{j}": coef[i, j] for j in range(5)})
        return "osg_sampler_cfg_multistep" if pair else "osg_sampler_multistep_single", scal

    ups = check_frame(tr, lines, prompts, pair, c_in, t, prepare, update, None)
    assert [u["form"] for u in ups] == [MS_FORMS[sampler][o] for o in order]
    assert all("noise" not in u for u in ups)
    reads = [0 if sampler == 0 and o == 2 else o for o in order]
    check_history(ups, ("h0", "h1", "h2", "h3"), reads, [sampler != 5] * STEPS, one_slot=sampler == 0)
    assert max(reads) == {0: 1, 1: 3, 2: 3, 3: 3, 4: 2, 5: 0}[sampler]      # the case reaches the sampler's deepest form
    assert not x.any()


@pytest.mark.parametrize("pair", PAIRS)
def test_stochastic(traced, pair):
    tr, prompts = traced, 1 if pair else 2
    x = tr.x(prompts)
    c_in, c_out, t, sigma = (_scalars(30 + s) for s in range(4))
    form = [ST_SDE0, ST_SDE1, ST_SDE2, ST_SDE2, ST_EULER]
    draws = [1, 0, 1, 1, 0]
    coef = _scalars(40, STEPS * 10).reshape(STEPS, 10)
    coef[:, 9] = [1, 1.5, 1, 1.5, 1]
    noise = np.ones((STEPS,) + x.shape, f32)
    if pair:
        lines = tr.call(tr.m.hip_sampler_loop_stochastic, *IO, x, c_in, c_out, t, sigma, form, draws, coef, noise, GUIDANCE)
    else:
        lines = tr.call(tr.m.hip_sampler_loop_stochastic_single, *IO, x, c_in, c_out, t, sigma, form, draws, coef, noise)

    def prepare(i):
        if not pair:
            return "osg_sampler_prepare_single", coef[i, 9]
        return ("osg_sampler_prepare_rescale", coef[i, 9]) if coef[i, 9] != 1 else ("osg_sampler_prepare", None)

    def update(i):
        scal = {"c_out": c_out[i], "sigma": sigma[i], "n0": coef[i, 7], "n1": coef[i, 8]}
        scal.update({f"k{j}": coef[i, j] for j in range(7)})
        return "osg_sampler_cfg_stochastic" if pair else "osg_sampler_stochastic_single", scal

    ups = check_frame(tr, lines, prompts, pair, c_in, t, prepare, update, draws)
    assert [u["form"] for u in ups] == form
    sde = [f in (ST_SDE0, ST_SDE1, ST_SDE2) for f in form]
    check_history(ups, ("h0", "h1", "h2"), [{ST_SDE1: 1, ST_SDE2: 2}.get(f, 0) for f in form], sde)
    assert not x.any()
