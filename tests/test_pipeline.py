"""End-to-end harness (onnxstream_amd/pipeline.py = the reference app's denoising loop + VAE decode, host side).

CPU: the schedule arithmetic against known answers taken from the reference's hard-coded table (src/sd.cpp:1591) and against
the golden end-to-end run generated THROUGH THE REFERENCE LIBRARY (tools/make_golden.py); GPU: the HIP backend through the
very same harness against that golden run (3 Euler-Ancestral steps with CFG 7 + VAE decode on miniature graphs)."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.pipeline import Txt2Img, log_sigmas_table, sigma_schedule, sigma_to_t
from onnxstream_amd.synth import sd_unet, sd_vae
from onnxstream_amd.synth.graph import DirSink
from oracle import ref as oref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_tiny.npz")


def test_latents_file_round_trip(tmp_path):
    """--save-latents / --decode-latents: raw float32 of the first sample (src/sd.cpp:2325-2327, :3212-3245)"""
    from onnxstream_amd.pipeline import load_latents, save_latents
    x = np.random.default_rng(1).standard_normal((2, 4, 64, 64)).astype(np.float32)
    f = str(tmp_path / "lat.bin")
    save_latents(f, x)
    assert os.path.getsize(f) == 4 * 64 * 64 * 4
    assert np.array_equal(load_latents(f), x[0:1])
    with pytest.raises(ValueError):
        load_latents(f, 32, 32)


def test_schedule_known_answers():
    ls = log_sigmas_table()
    # first / last three entries of the reference's table (src/sd.cpp:1591)
    assert np.allclose(ls[:3], [-3.534698963, -3.186542273, -2.982215166], atol=2e-5)
    assert np.allclose(ls[-3:], [2.66990304, 2.67595911, 2.682024002], atol=2e-5)
    assert np.all(np.diff(ls) > 0)
    sig = sigma_schedule(20, ls)
    assert sig.shape == (21,) and sig[-1] == 0 and np.all(np.diff(sig) < 0)
    assert abs(sig[0] - np.exp(2.682024002)) < 1e-3               # t = 999
    assert abs(sigma_to_t(float(sig[0]), ls) - 999.0) < 1e-3      # sigma_to_t inverts t_to_sigma on the grid
    assert abs(sigma_to_t(float(np.exp(ls[500])), ls) - 500.0) < 1e-2


def _emit(d):
    du, dv = d + "/unet/", d + "/vae/"
    sd_unet.build_unet(DirSink(du), sd_unet.TINY)
    sd_vae.build_vae_decoder(DirSink(dv), sd_vae.TINY_VAE)
    return du, dv


def _emit_tiled(d):
    import dataclasses
    dt = d + "/vae_t/"
    sd_vae.build_vae_decoder(DirSink(dt), dataclasses.replace(sd_vae.TINY_VAE, latent=8, in_name="latent_sample"))
    return dt


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs /root/reference)")
def test_reference_reproduces_pipeline_golden():
    z = np.load(GOLD)
    with tempfile.TemporaryDirectory() as d:
        du, dv = _emit(d)
        p = Txt2Img(oref.REF_LIB, du, dv, batched=False, threads=1)
        lat = p.sample(z["cond"], z["uncond"], steps=3, seed=9, latent_shape=(1, 4, 16, 16))
        img = p.decode(lat)
        p.close()
        pt = Txt2Img(oref.REF_LIB, du, _emit_tiled(d), batched=False, threads=1)
        img_t = pt.decode_tiled(lat, tile=8)
        pt.close()
    assert np.array_equal(lat, z["latents"]) and np.array_equal(img, z["image"]) and np.array_equal(img_t, z["image_tiled"])


@pytest.mark.gpu
def test_hip_pipeline_vs_reference_golden():
    from onnxstream_amd import build as b
    z = np.load(GOLD)
    with tempfile.TemporaryDirectory() as d:
        du, dv = _emit(d)
        p = Txt2Img(b.LIB_HOST, du, dv, batched=True)
        lat = p.sample(z["cond"], z["uncond"], steps=3, seed=9, latent_shape=(1, 4, 16, 16))
        img = p.decode(lat)
        # the VAE on the REFERENCE's latents isolates the decoder from the (chaotic) accumulated sampler drift
        img_ref_lat = p.decode(z["latents"])
        p.close()
        pt = Txt2Img(b.LIB_HOST, du, _emit_tiled(d), batched=True)       # 9 overlapping tiles as ONE batch-9 pass
        img_t = pt.decode_tiled(z["latents"], tile=8)
        pt.close()
    e_tiled = float(np.abs(img_t - z["image_tiled"]).max() / np.abs(z["image_tiled"]).max())
    assert e_tiled <= 5e-3, e_tiled
    e_lat = float(np.abs(lat - z["latents"]).max() / np.abs(z["latents"]).max())
    e_img = float(np.abs(img_ref_lat - z["image"]).max() / np.abs(z["image"]).max())
    e_e2e = float(np.abs(img - z["image"]).max() / np.abs(z["image"]).max())
    print(f"pipeline: latents {e_lat:.2e}  decode(ref latents) {e_img:.2e}  end-to-end image {e_e2e:.2e}")
    # three CFG-7 steps through a random-weight UNet amplify rounding differences; the per-pass bound is in test_golden.py
    assert e_lat <= 2e-2 and e_img <= 5e-3 and e_e2e <= 5e-2


@pytest.mark.gpu
@pytest.mark.parametrize("prompts", [1, 3])
def test_device_sampler_loop_matches_host_loop_bitwise(prompts):
    """The loop with CFG + Euler-Ancestral on the device (osg_sampler_prepare / osg_sampler_cfg_euler_a around the captured pass, no host
    round trips) against the host loop driving the same backend: same schedule, same random stream, same fp32 operation order => the
    latents are identical bit for bit, for one prompt and for several prompts batched into one pass; a second image on new contexts
    (resident plan, only model_hip_set_input) stays identical too."""
    from onnxstream_amd import build as b
    z = np.load(GOLD)
    rng = np.random.default_rng(5)
    shape = (prompts, 4, 16, 16)
    with tempfile.TemporaryDirectory() as d:
        du, _ = _emit(d)
        for round_ in range(2):
            conds = [z["cond"] + np.float32(0.01 * (k + 3 * round_)) * rng.standard_normal(z["cond"].shape, dtype=np.float32) for k in range(prompts)]
            unconds = [z["uncond"]] * prompts
            if round_ == 0:
                ph = Txt2Img(b.LIB_HOST, du, None, batched=True)
                pd = Txt2Img(b.LIB_HOST, du, None, batched=True)
            if prompts == 1:
                want = ph.sample(conds[0], unconds[0], steps=4, seed=21 + round_, latent_shape=shape)
                got = pd.sample_device(conds[0], unconds[0], steps=4, seed=21 + round_, latent_shape=shape)
            else:
                want = ph.sample(conds, unconds, steps=4, seed=21 + round_, latent_shape=shape)
                got = pd.sample_device(conds, unconds, steps=4, seed=21 + round_, latent_shape=shape)
            assert np.isfinite(want).all() and np.abs(want).max() > 0
            assert np.array_equal(got, want), float(np.abs(got - want).max())
        ph.close()
        pd.close()


# ---- the sampler / CFG arithmetic pinned against COMPILED REFERENCE CODE ------------------------------------------------------------------
# oracle/ref_sd.cpp #includes the reference application (src/sd.cpp + src/samplers.h) where it lies: diffusion_solver, CFGDenoiser_CompVisDenoiser
# and the Euler-Ancestral branch the shipped samplers.h selects run as the reference compiled them; tests/golden/sd_loop.npz holds that
# loop's output (tools/make_golden_sd_loop.py).  The harness (pipeline.py: schedule, sigma_to_t, c_in / c_out, CFG 7, ancestral update)
# driving the SAME reference library for the UNet must land on the same bits -- nothing of the sampler is restated on the oracle side.
SD_LOOP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sd_loop.npz")


def _sd_loop_tools():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_golden_sd_loop as t
    return t


LOG_SIGMAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "log_sigmas.npz")


def _reference_log_sigmas():
    """the reference application's log-sigma table literals (src/sd.cpp), as float32 (tools/make_golden_log_sigmas.py)"""
    return np.load(LOG_SIGMAS)["log_sigmas"]


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs /root/reference)")
def test_harness_loop_equals_the_reference_application_bit_for_bit():
    t = _sd_loop_tools()
    z = np.load(SD_LOOP)
    lib = t.ref_lib()
    cond, uncond = t.contexts()
    steps = int(z["steps"])
    init, noises = t.ref_noise_walk(lib, int(z["seed"]), steps)
    assert np.array_equal(init, z["init"][0:1]) and all(np.array_equal(noises[i], z["noise"][i][0:1]) for i in range(steps))
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_unet.build_unet(DirSink(d + "unet_fp16/"), t.IFACE)
        live = t.ref_loop(lib, d, 1, threads=1)                        # the reference application itself, here and now
        assert np.array_equal(live[0], z["latents"][0])                # ... reproduces the committed fixture
        p = Txt2Img(oref.REF_LIB, d + "unet_fp16/", None, batched=False, threads=1)
        # the one input of the loop that is DATA in the reference's source: the log-sigma table literals (src/sd.cpp:1591).  The product
        # recomputes the table (<= 1 float32 ulp off in 173 of the 1000 entries, see log_sigmas_table); for the bit-for-bit comparison of
        # the ARITHMETIC the literals themselves are parsed from the source here
        ref_table = _reference_log_sigmas()
        assert np.abs(p.log_sigmas.astype(np.float64) - ref_table.astype(np.float64)).max() <= 2.4e-7 and int((p.log_sigmas == ref_table).sum()) >= 800
        p.log_sigmas = ref_table
        got = p.sample(cond[None], uncond[None], steps=steps, latent_shape=(1, 4, 64, 64), init_latent=z["init"][0:1],
                       step_noise=lambda i: z["noise"][i][0:1])
        p.close()
    assert np.array_equal(got[0], z["latents"][0]), float(np.abs(got[0] - z["latents"][0]).max())


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs /root/reference)")
def test_harness_20_step_schedule_equals_the_reference_application_bit_for_bit():
    """the full 20-step schedule (float delta, 20 interpolated sigmas, 20 sigma_to_t, the app's srand/rand noise walk) on a micro UNet with
    the app's interface: milliseconds per pass, every scalar of the loop has to be the reference's to the last bit"""
    t = _sd_loop_tools()
    z = np.load(SD_LOOP)
    lib = t.ref_lib()
    cond, uncond = t.contexts()
    init, noises = t.ref_noise_walk(lib, int(z["seed"]), 20)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_unet(DirSink(d + "unet_fp16/"))
        live = t.ref_loop(lib, d, 1, threads=1, steps=20)
        assert np.array_equal(live, z["latents20_micro"])
        p = Txt2Img(oref.REF_LIB, d + "unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = _reference_log_sigmas()
        got = p.sample(cond[None], uncond[None], steps=20, latent_shape=(1, 4, 64, 64), init_latent=init, step_noise=lambda i: noises[i])
        p.close()
    assert np.isfinite(got).all() and np.array_equal(got, z["latents20_micro"]), float(np.abs(got - z["latents20_micro"]).max())


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs /root/reference)")
def test_harness_euler_sampler_equals_the_reference_application_bit_for_bit():
    """--sampler euler (src/samplers.h:116-126, the ORIGINAL_SAMPLER_ALGORITHMS branch): 20 steps on the micro UNet, harness == the reference app"""
    t = _sd_loop_tools()
    z = np.load(SD_LOOP)
    lib = t.ref_lib()
    cond, uncond = t.contexts()
    init, _ = t.ref_noise_walk(lib, int(z["seed"]), 20)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_unet(DirSink(d + "unet_fp16/"))
        lib.ref_sd_set_sampler(1)
        try:
            live = t.ref_loop(lib, d, 1, threads=1, steps=20)
        finally:
            lib.ref_sd_set_sampler(0)
        assert not np.array_equal(live, z["latents20_micro"])          # (it really is another sampler)
        p = Txt2Img(oref.REF_LIB, d + "unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = _reference_log_sigmas()
        got = p.sample(cond[None], uncond[None], steps=20, latent_shape=(1, 4, 64, 64), init_latent=init, sampler="euler")
        p.close()
    assert np.isfinite(got).all() and np.array_equal(got, live), float(np.abs(got - live).max())


@pytest.mark.gpu
def test_device_euler_loop_matches_host_loop_bitwise():
    from onnxstream_amd import build as b
    t = _sd_loop_tools()
    z = np.load(SD_LOOP)
    cond, uncond = t.contexts()
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_unet(DirSink(d + "unet_fp16/"))
        p = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        kw = dict(steps=20, latent_shape=(1, 4, 64, 64), init_latent=z["init"][0:1], sampler="euler")
        host = p.sample(cond[None], uncond[None], **kw)
        dev = p.sample_device(cond[None], uncond[None], **kw)
        p.close()
    assert np.isfinite(host).all() and np.array_equal(host, dev)


@pytest.mark.gpu
def test_hip_device_loop_vs_the_reference_application():
    """the product's device loop (2 prompts batched, like the app's --num 2) against the reference application's latents after 3 CFG-7
    steps; and bit-identical to the host loop over the same backend"""
    from onnxstream_amd import build as b
    t = _sd_loop_tools()
    z = np.load(SD_LOOP)
    cond, uncond = t.contexts()
    steps = int(z["steps"])
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_unet.build_unet(DirSink(d + "unet_fp16/"), t.IFACE)
        kw = dict(steps=steps, latent_shape=(2, 4, 64, 64), init_latent=z["init"], step_noise=lambda i: z["noise"][i])
        pd = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        got = pd.sample_device([cond[None]] * 2, [uncond[None]] * 2, **kw)
        pd.close()
        ph = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        host = ph.sample([cond[None]] * 2, [uncond[None]] * 2, **kw)
        ph.close()
    assert np.array_equal(got, host)
    err = float(np.abs(got - z["latents"]).max() / np.abs(z["latents"]).max())
    print(f"device loop vs reference application after {steps} steps: {err:.2e}")
    assert err <= 2e-2     # three CFG-7 steps through a random-weight UNet amplify the per-pass f16 differences (bounded in test_golden.py)
