"""SDXL (`xl`) and SDXL Turbo (`turbo`) in the sampler loop, CPU side.

* Reference pin: the harness's host loop (Txt2Img.sample with xl / turbo, the extras, the reference's initial latent and noise walk) driving the
  REFERENCE library for a micro UNet with the SDXL interface lands on the reference application's own latents bit for bit, for every entry of
  tests/golden/sdxl_loop.npz (tools/make_golden_sdxl_loop.py: src/sd.cpp + src/samplers.h compiled as they lie and run through the SDXL branch).  That
  pins the SDXL last-step rule, sigma_reshaper / sigma_reshaper_sharp, DDIM's softened prescale and the single-branch denoiser to compiled reference code.
* The switches do something; the Turbo tables are finite at 1-4 steps and read no history older than the image; the defaults change nothing.
* model_hip_sampler_loop_single / model_hip_sampler_loop_multistep_single: argument checks over the no-op stand-in for libosgpu.so."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.pipeline import _MS_LOOP, MULTISTEP, SAMPLERS, Txt2Img, log_sigmas_table, sigma_reshaper, sigma_reshaper_sharp, sigma_schedule
from onnxstream_amd.synth.graph import DirSink
from oracle import ref as oref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sdxl_loop.npz")
LOG_SIGMAS = os.path.join(HERE, "golden", "log_sigmas.npz")
sys.path.insert(0, os.path.join(HERE, "stub"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import make_golden_sdxl_loop as t  # noqa: E402

f32 = np.float32
SHAPE = (1, 4, t.LAT_H, t.LAT_W)
CASES = [("xl", s, t.XL_STEPS) for s in t.XL_SAMPLERS] + [("turbo", s, n) for n in t.TURBO_STEPS for s in SAMPLERS] + [("turbo", s, n) for s, n in t.TURBO_EXTRA]
# osg_multistep_form -> how many entries of earlier steps (h1..h3) it reads
READS = {0: 0, 1: 1, 2: 0, 3: 1, 4: 1, 5: 2, 6: 3, 7: 1, 8: 2, 9: 3, 10: 1, 11: 2, 12: 0}


def _bare():
    p = Txt2Img.__new__(Txt2Img)
    p.log_sigmas, p._t_cache = log_sigmas_table(), {}
    return p


@pytest.fixture(scope="module")
def ref_pipeline():
    """Txt2Img over the reference library and the micro SDXL UNet, with the application's own log-sigma table"""
    if not oref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_sdxl_unet(DirSink(d + "sdxl_unet_fp16/"))
        p = Txt2Img(oref.REF_LIB, d + "sdxl_unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = np.load(LOG_SIGMAS)["log_sigmas"]
        yield p
        p.close()


def _ref_sample(p, z, sampler, steps, **kw):
    emb, emb_neg, pooled, pooled_neg = t.contexts()
    return p.sample(emb[None], emb_neg[None], steps=steps, latent_shape=SHAPE, init_latent=z["init"], step_noise=lambda i: z["noise"][i], sampler=sampler,
                    extra_cond=t.extras(pooled), extra_uncond=t.extras(pooled_neg), **kw)


def test_fixture_holds_every_case():
    z = np.load(GOLD)
    assert sorted(z["cases"]) == sorted(f"{m}_{s}_{n}" for m, s, n in CASES)
    assert z["init"].shape == SHAPE and z["noise"].shape == (max(t.XL_STEPS, *t.TURBO_STEPS),) + SHAPE
    for c in z["cases"]:
        assert z["latents_" + c].shape == SHAPE and np.isfinite(z["latents_" + c]).all()
    assert os.path.getsize(GOLD) < 512 * 1024


@pytest.mark.parametrize("mode,sampler,steps", CASES)
def test_harness_equals_the_reference_application_bit_for_bit(ref_pipeline, mode, sampler, steps):
    z = np.load(GOLD)
    got = _ref_sample(ref_pipeline, z, sampler, steps, xl=True, turbo=mode == "turbo")
    want = z[f"latents_{mode}_{sampler}_{steps}"]
    assert np.isfinite(got).all() and np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_turbo_changes_the_result(ref_pipeline, sampler):
    z = np.load(GOLD)
    assert not np.array_equal(_ref_sample(ref_pipeline, z, sampler, 4, xl=True), z[f"latents_turbo_{sampler}_4"])


def test_xl_changes_dpmpp2m(ref_pipeline):
    z = np.load(GOLD)
    assert not np.array_equal(_ref_sample(ref_pipeline, z, "dpm++2m", t.XL_STEPS), z[f"latents_xl_dpm++2m_{t.XL_STEPS}"])


@pytest.mark.parametrize("sampler", SAMPLERS[1:])
def test_switches_change_the_tables(sampler):
    """without a UNet: turbo moves the scalars of every sampler but Euler-Ancestral (which Turbo leaves alone), xl the last step of the DPM++ pair"""
    p = _bare()
    sig = sigma_schedule(4, p.log_sigmas)
    if sampler == "euler":
        assert not np.array_equal(p.loop_scalars(sig, "euler")[4], p.loop_scalars(sig, "euler", turbo=True)[4])
        return
    _, order, coef, dcoef = p.multistep_table(sig, sampler)
    _, order_t, coef_t, dcoef_t = p.multistep_table(sig, sampler, turbo=True)
    assert not (np.array_equal(coef, coef_t) and np.array_equal(dcoef, dcoef_t))
    _, order_x, coef_x, _ = p.multistep_table(sig, sampler, xl=True)
    if sampler.startswith("dpm"):
        assert order[-1] == 0 and order_x[-1] == 2 and np.array_equal(order[:-1], order_x[:-1]) and np.array_equal(coef[:-1], coef_x[:-1])
        assert coef_x[-1, 0] == -sig[3]              # the Euler step to sigma = 0: k0 = 0 - sigma_i
    else:
        assert np.array_equal(order, order_x) and np.array_equal(coef, coef_x)
    assert np.array_equal(p.loop_scalars(sig, "euler_a")[4:], p.loop_scalars(sig, "euler_a", turbo=True)[4:])


def test_reshapers():
    s = f32(3.0)
    for i, steps in ((0, 1), (0, 4), (3, 4), (2, 3)):
        assert sigma_reshaper(s, i, steps, False) == s and sigma_reshaper_sharp(s, i, steps, False) == s
        assert 0 < sigma_reshaper(s, i, steps, True) <= s
        assert sigma_reshaper(f32(0), i, steps, True) == 0 and sigma_reshaper_sharp(f32(0), i, steps, True) == 0
    assert sigma_reshaper(s, 0, 1, True) == s                           # one step: both powers are 1 ** e
    # 3 / (steps - 2.5) is negative below 3 steps: the sharp form then moves AWAY from the plain one
    plain = sigma_reshaper(s, 0, 2, True)
    assert plain < s < sigma_reshaper_sharp(s, 0, 2, True)
    assert sigma_reshaper(s, 0, 3, True) < s and sigma_reshaper_sharp(s, 0, 3, True) < s


@pytest.mark.parametrize("steps", [1, 2, 3, 4])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_turbo_tables_are_finite_and_ordered(sampler, steps):
    """every device argument is finite and no step reads a history entry older than the image -- at one step the image is first and last step at once"""
    p = _bare()
    sig = sigma_schedule(steps, p.log_sigmas)
    assert sig.shape == (steps + 1,) and np.isfinite(sig).all() and sig[-1] == 0
    for a in p.loop_scalars(sig, "euler" if sampler in MULTISTEP else sampler, turbo=True):
        assert a.shape == (steps,) and np.isfinite(a).all()
    if sampler not in MULTISTEP:
        return
    loop, order, coef, dcoef = p.multistep_table(sig, sampler, turbo=True)
    assert loop == MULTISTEP[sampler] and order.shape == (steps,) and coef.shape == (steps, 6) and dcoef.shape == (steps, 2)
    assert np.isfinite(coef).all() and np.isfinite(dcoef).all()
    forms = _MS_LOOP[loop][1]
    assert all(0 <= order[i] < len(forms) and READS[forms[order[i]]] <= i for i in range(steps))
    if sampler.startswith("dpm"):
        assert order[-1] == 2                        # turbo implies xl


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_defaults_reproduce_the_tables(sampler):
    p = _bare()
    sig = sigma_schedule(20, p.log_sigmas)
    name = "euler" if sampler in MULTISTEP else sampler
    for a, b in zip(p.loop_scalars(sig, name), p.loop_scalars(sig, name, turbo=False)):
        assert np.array_equal(a, b)
    if sampler in MULTISTEP:
        old, new = p.multistep_table(sig, sampler), p.multistep_table(sig, sampler, xl=False, turbo=False)
        assert old[0] == new[0] and all(np.array_equal(a, b) for a, b in zip(old[1:], new[1:]))
        assert old[1].max() <= (1 if sampler.startswith("dpm") else 3) and (old[2][:, 5] == 1).all() == (sampler != "ddim")


@pytest.fixture(scope="module")
def stub_backend():
    import make_stub
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_HOST):
        pytest.skip("host library not built")
    with tempfile.TemporaryDirectory() as d:
        so = make_stub.build(d)
        old = os.environ.get("OSGPU_LIB")
        os.environ["OSGPU_LIB"] = so
        try:
            yield so
        finally:
            if old is None:
                os.environ.pop("OSGPU_LIB", None)
            else:
                os.environ["OSGPU_LIB"] = old


def test_single_loop_plumbing(stub_backend):
    """the *_single loops want a plan of `prompts` samples, the CFG loops one of 2 * prompts; the table and order checks carry over, and order 2 of the
    DPM++ loop (the Euler step of the SDXL rule) is legal at step 0 (the stub computes nothing: eps stays 0, so x stays 0)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model, OnnxStreamError
    emb, _, pooled, _ = t.contexts()
    steps = 4
    sc = [np.full(steps, v, f32) for v in (0.5, -2.0, 900.0, 2.0)]
    eu = sc + [np.full(steps, -0.5, f32), np.zeros(steps, f32)]
    order = np.minimum(np.arange(steps), 3).astype(np.int32)
    coef, dcoef = np.ones((steps, 6), f32), np.ones((steps, 2), np.float64)
    io = ("sample", "timestep", "out_sample")
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_sdxl_unet(DirSink(d))
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.read_file(d + "model.txt")
        x1, x2 = np.zeros(SHAPE, f32), np.zeros((2,) + SHAPE[1:], f32)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_single: no plan"):
            m.hip_sampler_loop_single(*io, x1, None, *eu)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_multistep_single: no plan"):
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, order, coef, dcoef)

        def run(pushes):
            for _ in range(pushes):
                m.add_tensor("timestep", np.asarray([900.0], f32))
                m.add_tensor("sample", x1)
                m.add_tensor("encoder_hidden_states", emb[None])
                for k, v in t.extras(pooled).items():
                    m.add_tensor(k, v)
            m.set_use_fp16_arithmetic(True)
            m.set_fuse_ops_in_attention(True)
            m.run()
            m.clear_tensors()

        run(1)                                           # a plan of ONE sample: one prompt for the single loops, none for the CFG loops
        noise = np.ones((steps,) + SHAPE, f32)
        assert m.hip_sampler_loop_single(*io, x1, None, *eu) == 0.0 and not x1.any()
        for loop in range(6):
            o = np.minimum(order, [1, 3, 3, 3, 2, 0][loop]).astype(np.int32)
            assert m.hip_sampler_loop_multistep_single(*io, x1, loop, *sc, o, coef, dcoef) == 0.0 and np.isfinite(x1).all() and not x1.any()
        assert m.hip_sampler_loop_multistep_single(*io, x1, 0, *sc, np.full(steps, 2, np.int32), coef, dcoef) == 0.0      # Euler at every step, step 0 too
        assert m.hip_sampler_loop_multistep_single(*io, x1, 0, sc[0][:1], sc[1][:1], sc[2][:1], sc[3][:1], [2], coef[:1], dcoef[:1]) == 0.0
        with pytest.raises(OnnxStreamError, match="2 \\* prompts"):
            m.hip_sampler_loop(*io, x1, noise, *eu)
        with pytest.raises(OnnxStreamError, match="2 \\* prompts"):
            m.hip_sampler_loop_multistep(*io, x1, 1, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_single: the plan's batch must be prompts"):
            m.hip_sampler_loop_single(*io, x2, None, *eu)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_multistep_single: the plan's batch must be prompts"):
            m.hip_sampler_loop_multistep_single(*io, x2, 1, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="unknown sampler form 6"):
            m.hip_sampler_loop_multistep_single(*io, x1, 6, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="steps \\* 6 floats"):
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, order, coef[:-1], dcoef)
        with pytest.raises(OnnxStreamError, match="steps \\* 2 doubles"):
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, order, coef, dcoef[:, :1])
        with pytest.raises(OnnxStreamError, match="order 1 at step 0"):       # history that this image has not written yet
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, np.ones(steps, np.int32), coef, dcoef)
        with pytest.raises(OnnxStreamError, match="order 3 at step 3"):       # Taylor3 has orders 0-2 only
            m.hip_sampler_loop_multistep_single(*io, x1, 4, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="order 2 at step 2"):       # the Euler order belongs to the DPM++ loop alone: DDIM has one form
            m.hip_sampler_loop_multistep_single(*io, x1, 5, *sc, np.asarray([0, 0, 2, 0], np.int32), coef, dcoef)
        with pytest.raises(OnnxStreamError, match="one entry per step"):
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, order[:-1], coef, dcoef)
        with pytest.raises(OnnxStreamError, match="not found"):
            m.hip_sampler_loop_multistep_single("sample", "timestep", "nope", x1, 1, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="not found"):
            m.hip_sampler_loop_single("sample", "nope", "out_sample", x1, None, *eu)

        run(2)                                           # a plan of TWO samples: one prompt for the CFG loops, two for the single loops
        assert m.hip_sampler_loop(*io, x1, noise, *eu) == 0.0 and not x1.any()
        assert m.hip_sampler_loop_multistep(*io, x1, 0, *sc, np.asarray([0, 1, 1, 2], np.int32), coef, dcoef) == 0.0 and not x1.any()
        assert m.hip_sampler_loop_multistep(*io, x1, 0, *sc, np.full(steps, 2, np.int32), coef, dcoef) == 0.0
        assert m.hip_sampler_loop_single(*io, x2, None, *eu) == 0.0 and not x2.any()
        assert m.hip_sampler_loop_multistep_single(*io, x2, 3, *sc, order, coef, dcoef) == 0.0 and not x2.any()
        with pytest.raises(OnnxStreamError, match="must be prompts"):
            m.hip_sampler_loop_single(*io, x1, None, *eu)
        with pytest.raises(OnnxStreamError, match="must be prompts"):
            m.hip_sampler_loop_multistep_single(*io, x1, 1, *sc, order, coef, dcoef)
        m.close()
