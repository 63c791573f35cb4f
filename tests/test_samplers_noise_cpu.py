"""The samplers of the device loop that add fresh noise per step (pipeline.STOCHASTIC: DDPM(-a), DDIM-a, TCD(-a), LCM, DPM++ 3M SDE(-a)), CPU side.

* Names: the eight are accepted, SAMPLERS and MULTISTEP are what they were, the two-evaluation samplers and lms are still refused.
* stochastic_table: finite scalars, the drawing steps a prefix of the image, no SDE form earlier than its order, SDXL's last-step rule.
* Reference pin: the harness's host loop (Txt2Img.sample: stochastic_table's scalars + stochastic_update, the host restatement of
  osg_sampler_cfg_stochastic) driving the REFERENCE library for the UNet, with the application's own initial latent and noise walk, lands on the
  reference application's latents bit for bit -- tests/golden/sd_samplers_noise.npz (SD 1.5 micro UNet) and tests/golden/sdxl_loop_noise.npz (SDXL and
  Turbo on the 12 x 20 micro SDXL UNet), both written by tools/make_golden_samplers_noise.py from src/sd.cpp + src/samplers.h compiled as they lie.
* model_hip_sampler_loop_stochastic[_single]: argument checks over the no-op stand-in for libosgpu.so (tests/stub/make_stub.py)."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd import pipeline
from onnxstream_amd.pipeline import MULTISTEP, SAMPLERS, Txt2Img, log_sigmas_table, sigma_schedule
from onnxstream_amd.synth import sd_unet
from onnxstream_amd.synth.graph import DirSink
from oracle import ref as oref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_SD = os.path.join(HERE, "golden", "sd_samplers_noise.npz")
GOLD_XL = os.path.join(HERE, "golden", "sdxl_loop_noise.npz")
LOG_SIGMAS = os.path.join(HERE, "golden", "log_sigmas.npz")
sys.path.insert(0, os.path.join(HERE, "stub"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import make_golden_sd_loop as sdl  # noqa: E402
import make_golden_sdxl_loop as xll  # noqa: E402

f32 = np.float32
EIGHT = ("ddpm", "ddpm_a", "ddim_a", "tcd", "tcd_a", "lcm", "dpm++3msde", "dpm++3msde_a")
SILENT = ("ddpm", "tcd", "dpm++3msde")                   # eta = 0: they draw nothing
ST_LINEAR, ST_DEN, ST_EULER, ST_DDIM_A, ST_TCD, ST_SDE0, ST_SDE1, ST_SDE2 = range(8)       # osg_stochastic_form, include/osgpu.h
XL_SHAPE = (1, 4, xll.LAT_H, xll.LAT_W)
XL_CASES = [("xl", "dpm++3msde_a", 5), ("xl", "tcd_a", 5)] + [("turbo", s, n) for n in (1, 4) for s in EIGHT]


def _stochastic():
    """pipeline.STOCHASTIC, looked up at run time: a tree without the feature fails every test here instead of failing the module's import"""
    return pipeline.STOCHASTIC


def _bare():
    p = Txt2Img.__new__(Txt2Img)
    p.log_sigmas, p._t_cache = log_sigmas_table(), {}
    return p


def test_names():
    assert set(_stochastic()) == set(EIGHT)
    assert SAMPLERS == ("euler_a", "euler", "dpm++2m", "dpm++2mv2", "ipndm", "ipndm_v", "ipndm_vo", "taylor3", "ddim")
    assert MULTISTEP == {"dpm++2m": 0, "dpm++2mv2": 0, "ipndm": 1, "ipndm_v": 2, "ipndm_vo": 3, "taylor3": 4, "ddim": 5}
    assert not set(EIGHT) & set(SAMPLERS)
    p = Txt2Img.__new__(Txt2Img)
    for name in EIGHT:
        pipeline._check_sampler(name)
    for bad in ("heun", "dpm2", "dpm++2s", "dpm++2s_a", "lms"):
        with pytest.raises(ValueError, match="valid names: euler_a, euler, dpm\\+\\+2m"):
            p.sample(None, None, sampler=bad)
        with pytest.raises(ValueError, match="valid names"):
            p.sample_device(None, None, sampler=bad)
    with pytest.raises(ValueError, match="not a stochastic sampler"):
        _bare().stochastic_table(sigma_schedule(4, log_sigmas_table()), "euler_a")


def _check_table(sampler, steps, xl, turbo):
    p = _bare()
    sig = sigma_schedule(steps, p.log_sigmas)
    form, draws, coef = p.stochastic_table(sig, sampler, xl=xl, turbo=turbo)
    assert form.shape == (steps,) and draws.shape == (steps,) and coef.shape == (steps, 10)
    assert form.dtype == np.int32 and draws.dtype == np.int32 and coef.dtype == f32
    assert np.isfinite(coef).all()
    assert ((form >= 0) & (form < 8)).all() and set(draws.tolist()) <= {0, 1}
    nd = int(draws.sum())
    assert draws[:nd].all() and not draws[nd:].any()                     # a prefix: noise i of the application's walk belongs to step i
    if sampler in SILENT:
        assert nd == 0
    if sampler == "ddim_a":
        assert nd == steps and coef[-1, 7] == 0                          # the add stays on the last step, times 0
    else:
        assert not draws[-1]
    if sampler not in SILENT and steps > 1:
        assert nd == steps - (sampler != "ddim_a") and (coef[:nd - 1, 7] > 0).all()
    # no SDE form earlier than its order, and each behind steps that wrote history
    for i, f in enumerate(form):
        for k in range(1, {ST_SDE1: 1, ST_SDE2: 2}.get(int(f), 0) + 1):
            assert i - k >= 0 and form[i - k] in (ST_SDE0, ST_SDE1, ST_SDE2)
    if sampler.startswith("dpm"):
        assert form[-1] == (ST_EULER if xl or turbo else ST_DEN)
        assert form[:-1].tolist() == [ST_SDE0, ST_SDE1, ST_SDE2][:steps - 1] + [ST_SDE2] * max(steps - 4, 0)
        if xl or turbo:
            assert coef[-1, 0] < 0
    else:
        assert (form == {"ddpm": ST_LINEAR, "ddpm_a": ST_LINEAR, "ddim_a": ST_DDIM_A, "tcd": ST_TCD, "tcd_a": ST_TCD, "lcm": ST_DEN}[sampler]).all()
    # the prescale of x is DDIM's: DDIM-a and TCD have it on every step, nobody else
    assert (coef[:, 9] > 1).all() if sampler in ("ddim_a", "tcd", "tcd_a") else (coef[:, 9] == 1).all()
    # n1 multiplies x only in TCD's noise add
    assert (coef[draws == 0, 8] == 1).all() and (sampler == "tcd_a" or (coef[:, 8] == 1).all())
    return form, draws, coef


@pytest.mark.parametrize("sampler", EIGHT)
def test_stochastic_table_20_steps(sampler):
    _check_table(sampler, 20, False, False)
    f_xl, d_xl, c_xl = _check_table(sampler, 20, True, False)
    f, d, c = _bare().stochastic_table(sigma_schedule(20, log_sigmas_table()), sampler)
    assert np.array_equal(f[:-1], f_xl[:-1]) and np.array_equal(c[:-1], c_xl[:-1]) and np.array_equal(d, d_xl)     # xl moves the last DPM++ step alone
    assert np.array_equal(f, f_xl) != sampler.startswith("dpm")


@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("sampler", EIGHT)
def test_stochastic_table_turbo(sampler, steps):
    _, _, coef_t = _check_table(sampler, steps, True, True)
    _, _, coef = _bare().stochastic_table(sigma_schedule(steps, log_sigmas_table()), sampler, xl=True)
    if steps == 4 and sampler not in ("ddpm", "ddpm_a", "lcm"):          # those three read the raw sigma[i + 1] and have no prescale
        assert not np.array_equal(coef, coef_t)
    if sampler in ("ddpm", "ddpm_a", "lcm"):
        assert np.array_equal(coef, coef_t)


def test_eta():
    """the randomness each name sets, and that it reaches the scalars (dpm++3msde_a's 0.5 of Turbo mode, src/samplers.h:414-417, is pinned by the
    Turbo fixtures)"""
    p = _bare()
    sig = sigma_schedule(4, p.log_sigmas)
    assert _stochastic()["tcd_a"] == 0.5 and _stochastic()["ddpm_a"] == 1 and _stochastic()["ddim_a"] == 1 and _stochastic()["dpm++3msde_a"] == 1
    assert all(_stochastic()[s] == 0 for s in SILENT)
    # TCD's si3 = sigma[(size_t)((steps - i - 1) * eta + i + 1)] and si4 = si1 * (1 - eta): eta 0 reads sigma[i + 1] twice, eta 0.5 a later (smaller)
    # sigma and half of si1, so alpha_s = 1 / (si2 * si2 + 1) is larger; on the last step both reach sigma = 0 and alpha_s = 1
    _, _, c = p.stochastic_table(sig, "tcd")
    _, _, ca = p.stochastic_table(sig, "tcd_a")
    assert (c[:-1, 1] < ca[:-1, 1]).all() and (ca[:-1, 1] < 1).all() and (c[:-1, 2] > ca[:-1, 2]).all() and (ca[:-1, 2] > 0).all()
    assert c[-1, 1] == 1 and ca[-1, 1] == 1 and c[-1, 2] == 0 and ca[-1, 2] == 0
    # dpm++3msde_a: eta 1, or 0.5 in Turbo mode -- k0 = exp(-h * (eta + 1)) at step 0 (one Turbo step reshapes nothing, so only eta differs)
    sig2 = sigma_schedule(2, p.log_sigmas)
    k_plain, k_a = (p.stochastic_table(sig2, s)[2][0, 0] for s in ("dpm++3msde", "dpm++3msde_a"))
    assert 0 < k_a < k_plain < 1 and abs(float(k_a) - float(k_plain) ** 2) < 1e-6 * float(k_a)


def test_fixtures_hold_the_eight():
    z = np.load(GOLD_SD)
    lat = [z["latents_" + s] for s in EIGHT]
    assert all(a.shape == (1, 4, 64, 64) and a.dtype == f32 and np.isfinite(a).all() for a in lat)
    assert all(5 <= int(z["steps_" + s]) <= 20 for s in EIGHT)
    assert all(not np.array_equal(lat[i], lat[j]) for i in range(8) for j in range(i + 1, 8))
    x = np.load(GOLD_XL)
    assert sorted(x["cases"]) == sorted(f"{m}_{s}_{n}" for m, s, n in XL_CASES)
    assert x["init"].shape == XL_SHAPE and x["noise"].shape == (5,) + XL_SHAPE and int(x["seed"]) == xll.SEED
    assert all(x["latents_" + c].shape == XL_SHAPE and np.isfinite(x["latents_" + c]).all() for c in x["cases"])
    for keys in (["xl_dpm++3msde_a_5", "xl_tcd_a_5"], [f"turbo_{s}_4" for s in EIGHT]):      # (one Turbo step draws nothing: twins coincide there)
        assert all(not np.array_equal(x["latents_" + a], x["latents_" + b]) for i, a in enumerate(keys) for b in keys[i + 1:])
    assert os.path.getsize(GOLD_SD) < 1024 * 1024 and os.path.getsize(GOLD_XL) < 512 * 1024


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs the reference sources)")
@pytest.mark.parametrize("sampler", EIGHT)
def test_harness_equals_the_reference_application_bit_for_bit(sampler):
    z = np.load(GOLD_SD)
    steps = int(z["steps_" + sampler])
    lib = sdl.ref_lib()
    cond, uncond = sdl.contexts()
    init, noise = sdl.ref_noise_walk(lib, sdl.SEED, steps)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        p = Txt2Img(oref.REF_LIB, d + "unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = np.load(LOG_SIGMAS)["log_sigmas"]
        got = p.sample(cond[None], uncond[None], steps=steps, latent_shape=(1, 4, 64, 64), init_latent=init, step_noise=lambda i: noise[i], sampler=sampler)
        p.close()
    want = z["latents_" + sampler]
    assert np.isfinite(got).all() and np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.fixture(scope="module")
def ref_xl_pipeline():
    """Txt2Img over the reference library and the micro SDXL UNet, with the application's own log-sigma table"""
    if not oref.available():
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        xll.build_micro_sdxl_unet(DirSink(d + "sdxl_unet_fp16/"))
        p = Txt2Img(oref.REF_LIB, d + "sdxl_unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = np.load(LOG_SIGMAS)["log_sigmas"]
        yield p
        p.close()


@pytest.mark.parametrize("mode,sampler,steps", XL_CASES)
def test_harness_equals_the_reference_application_sdxl_bit_for_bit(ref_xl_pipeline, mode, sampler, steps):
    z = np.load(GOLD_XL)
    emb, emb_neg, pooled, pooled_neg = xll.contexts()
    got = ref_xl_pipeline.sample(emb[None], emb_neg[None], steps=steps, latent_shape=XL_SHAPE, init_latent=z["init"], step_noise=lambda i: z["noise"][i],
                                 sampler=sampler, extra_cond=xll.extras(pooled), extra_uncond=xll.extras(pooled_neg), xl=True, turbo=mode == "turbo")
    want = z[f"latents_{mode}_{sampler}_{steps}"]
    assert np.isfinite(got).all() and np.array_equal(got, want), float(np.abs(got - want).max())


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


def test_device_stochastic_loop_plumbing(stub_backend):
    """model_hip_sampler_loop_stochastic[_single]: the checks of model_hip_sampler_loop plus unknown form, SDE forms ahead of their history, table
    sizes and a drawing step without noise (the stub computes nothing: eps stays 0, so x stays 0)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model, OnnxStreamError
    ins = sd_unet.unet_inputs(sd_unet.TINY, 42)
    L = ins["sample"].shape
    steps = 4
    sc = [np.full(steps, v, f32) for v in (0.5, -2.0, 900.0, 2.0)]
    coef = np.ones((steps, 10), f32)
    io = ("sample", "timestep", "out_sample")
    none, all_ = np.zeros(steps, np.int32), np.ones(steps, np.int32)
    sde = np.asarray([ST_SDE0, ST_SDE1, ST_SDE2, ST_SDE2], np.int32)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_unet.build_unet(DirSink(d), sd_unet.TINY)
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.read_file(d + "model.txt")
        x = np.zeros(L, f32)
        x2 = np.zeros((2,) + L[1:], f32)
        noise = np.ones((steps,) + L, f32)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_stochastic: no plan"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, none, coef)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_stochastic_single: no plan"):
            m.hip_sampler_loop_stochastic_single(*io, x, *sc, sde, none, coef)

        def run():
            for _ in range(2):
                for k, v in ins.items():
                    m.add_tensor(k, v)
            m.set_use_fp16_arithmetic(True)
            m.set_fuse_ops_in_attention(True)
            m.run()
            m.clear_tensors()

        run()                                            # a plan of TWO samples: one prompt for the CFG loop, two for the single loop
        for f in range(5):                               # every history-free form at every step, with and without noise; prescale on and off
            form = np.full(steps, f, np.int32)
            for dr, nz in ((none, None), (all_, noise), (np.asarray([1, 1, 0, 0], np.int32), noise)):
                for c in (coef, coef * np.asarray([1] * 9 + [1.5], f32)):
                    assert m.hip_sampler_loop_stochastic(*io, x, *sc, form, dr, c, nz) == 0.0 and np.isfinite(x).all() and not x.any()
        assert m.hip_sampler_loop_stochastic(*io, x, *sc, sde, none, coef) == 0.0 and not x.any()
        assert m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([ST_SDE0, ST_SDE1, ST_SDE2, ST_EULER], np.int32), all_, coef, noise) == 0.0 and not x.any()
        assert m.hip_sampler_loop_stochastic(*io, x, sc[0][:1], sc[1][:1], sc[2][:1], sc[3][:1], [ST_EULER], [0], coef[:1]) == 0.0      # a one-step image
        assert m.hip_sampler_loop_stochastic_single(*io, x2, *sc, sde, all_, coef, np.ones((steps,) + x2.shape, f32)) == 0.0 and not x2.any()
        with pytest.raises(OnnxStreamError, match="unknown form 8 at step 2"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([0, 0, 8, 0], np.int32), none, coef)
        with pytest.raises(OnnxStreamError, match="unknown form -1 at step 0"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([-1, 0, 0, 0], np.int32), none, coef)
        with pytest.raises(OnnxStreamError, match="form 6 at step 0 is not available"):      # history that this image has not written yet
            m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([ST_SDE1, ST_SDE1, ST_SDE2, ST_SDE2], np.int32), none, coef)
        with pytest.raises(OnnxStreamError, match="form 7 at step 1 is not available"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([ST_SDE0, ST_SDE2, ST_SDE2, ST_SDE2], np.int32), none, coef)
        with pytest.raises(OnnxStreamError, match="form 6 at step 3 is not available"):      # the step before wrote no history
            m.hip_sampler_loop_stochastic(*io, x, *sc, np.asarray([ST_SDE0, ST_SDE1, ST_DEN, ST_SDE1], np.int32), none, coef)
        with pytest.raises(OnnxStreamError, match="steps \\* 10 floats"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, none, coef[:-1])
        with pytest.raises(OnnxStreamError, match="steps \\* 10 floats"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, none, coef[:, :9])
        with pytest.raises(OnnxStreamError, match="draws noise but no noise was given"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, np.asarray([0, 1, 0, 0], np.int32), coef)
        with pytest.raises(OnnxStreamError, match="noise must hold steps \\* x.size"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, all_, coef, noise[:-1])
        with pytest.raises(OnnxStreamError, match="one entry per step"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde[:-1], none, coef)
        with pytest.raises(OnnxStreamError, match="one entry per step"):
            m.hip_sampler_loop_stochastic(*io, x, *sc, sde, none[:-1], coef)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_stochastic: the plan's batch must be 2 \\* prompts"):
            m.hip_sampler_loop_stochastic(*io, x2, *sc, sde, none, coef)
        with pytest.raises(OnnxStreamError, match="hip_sampler_loop_stochastic_single: the plan's batch must be prompts"):
            m.hip_sampler_loop_stochastic_single(*io, x, *sc, sde, none, coef)
        with pytest.raises(OnnxStreamError, match="not found"):
            m.hip_sampler_loop_stochastic("sample", "timestep", "nope", x, *sc, sde, none, coef)
        assert not x.any() and not x2.any()
        m.close()
