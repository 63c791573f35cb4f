"""The multistep samplers of the device loop (pipeline.MULTISTEP: DPM++ 2M / 2M v2, iPNDM, iPNDM_v, iPNDM_vo, Taylor3, DDIM), CPU side.

* The harness's host loop (Txt2Img.sample: multistep_table's scalars + multistep_update, the host restatement of osg_sampler_cfg_multistep)
  driving the REFERENCE library for the UNet lands on the reference application's own latents bit for bit (tests/golden/sd_samplers.npz,
  tools/make_golden_samplers.py: src/sd.cpp + src/samplers.h compiled as they lie, sampler chosen by name).
* model_hip_sampler_loop_multistep's argument checks, over the no-op stand-in for libosgpu.so (tests/stub/make_stub.py)."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.pipeline import MULTISTEP, SAMPLERS, Txt2Img, sigma_schedule
from onnxstream_amd.synth import sd_unet
from onnxstream_amd.synth.graph import DirSink
from oracle import ref as oref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sd_samplers.npz")
LOG_SIGMAS = os.path.join(HERE, "golden", "log_sigmas.npz")
sys.path.insert(0, os.path.join(HERE, "stub"))


def _sd_loop_tools():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import make_golden_sd_loop as t
    return t


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


def test_sampler_names():
    assert SAMPLERS == ("euler_a", "euler", "dpm++2m", "dpm++2mv2", "ipndm", "ipndm_v", "ipndm_vo", "taylor3", "ddim")
    assert set(MULTISTEP) == set(SAMPLERS[2:])
    p = Txt2Img.__new__(Txt2Img)
    for bad in ("heun", "lms", "DPM++2M"):
        with pytest.raises(ValueError, match="valid names: euler_a, euler, dpm\\+\\+2m"):
            p.sample(None, None, sampler=bad)
        with pytest.raises(ValueError, match="valid names"):
            p.sample_device(None, None, sampler=bad)


@pytest.mark.parametrize("sampler", list(MULTISTEP))
def test_multistep_table_is_finite_and_ordered(sampler):
    """every device argument is finite (Taylor3's first step would read the reference's unset sampler_history_dt: it must not leak) and no
    step reads a history entry older than the image"""
    from onnxstream_amd.pipeline import log_sigmas_table
    p = Txt2Img.__new__(Txt2Img)
    sig = sigma_schedule(20, log_sigmas_table())
    loop, order, coef, dcoef = p.multistep_table(sig, sampler)
    assert loop == MULTISTEP[sampler] and order.shape == (20,) and coef.shape == (20, 6) and dcoef.shape == (20, 2)
    assert np.isfinite(coef).all() and np.isfinite(dcoef).all()
    assert all(0 <= order[i] <= i for i in range(20))
    if sampler.startswith("dpm"):
        assert order[0] == 0 and order[-1] == 0 and (order[1:-1] == 1).all() and coef[-1, 1] == -1   # expm1(log(0) - log(s)) = -1
    if sampler == "ddim":
        assert (coef[:, 5] > 1).all() and dcoef[-1, 0] == 0 and dcoef[-1, 1] == 1


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("sampler", list(MULTISTEP))
def test_harness_multistep_sampler_equals_the_reference_application_bit_for_bit(sampler):
    t = _sd_loop_tools()
    z = np.load(GOLD)
    steps = int(z["steps_" + sampler])
    assert steps >= 5
    lib = t.ref_lib()
    cond, uncond = t.contexts()
    init, _ = t.ref_noise_walk(lib, t.SEED, steps)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_unet(DirSink(d + "unet_fp16/"))
        p = Txt2Img(oref.REF_LIB, d + "unet_fp16/", None, batched=False, threads=1)
        p.log_sigmas = np.load(LOG_SIGMAS)["log_sigmas"]
        got = p.sample(cond[None], uncond[None], steps=steps, latent_shape=(1, 4, 64, 64), init_latent=init, sampler=sampler)
        p.close()
    want = z["latents_" + sampler]
    assert np.isfinite(got).all() and np.array_equal(got, want), float(np.abs(got - want).max())


def test_device_multistep_loop_plumbing(stub_backend):
    """model_hip_sampler_loop_multistep: the checks of model_hip_sampler_loop plus unknown loop form, table sizes and orders (the stub computes
    nothing: eps stays 0, so x stays 0)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model, OnnxStreamError
    ins = sd_unet.unet_inputs(sd_unet.TINY, 42)
    L = ins["sample"].shape
    steps = 4
    sc = [np.full(steps, v, np.float32) for v in (0.5, -2.0, 900.0, 2.0)]
    order = np.minimum(np.arange(steps), 3).astype(np.int32)
    coef, dcoef = np.ones((steps, 6), np.float32), np.ones((steps, 2), np.float64)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_unet.build_unet(DirSink(d), sd_unet.TINY)
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.read_file(d + "model.txt")
        x = np.zeros(L, np.float32)
        with pytest.raises(OnnxStreamError, match="no plan"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 1, *sc, order, coef, dcoef)
        for _ in range(2):
            for k, v in ins.items():
                m.add_tensor(k, v)
        m.set_use_fp16_arithmetic(True)
        m.set_fuse_ops_in_attention(True)
        m.run()
        m.clear_tensors()
        for loop in range(6):
            o = np.minimum(order, [1, 3, 3, 3, 2, 0][loop]).astype(np.int32)
            ms = m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, loop, *sc, o, coef, dcoef)
            assert ms == 0.0 and np.isfinite(x).all() and not x.any()
        with pytest.raises(OnnxStreamError, match="unknown sampler form 6"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 6, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="unknown sampler form -1"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, -1, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="steps \\* 6 floats"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 1, *sc, order, coef[:-1], dcoef)
        with pytest.raises(OnnxStreamError, match="steps \\* 2 doubles"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 1, *sc, order, coef, dcoef[:, :1])
        with pytest.raises(OnnxStreamError, match="order 1 at step 0"):       # history that this image has not written yet
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 1, *sc, np.ones(steps, np.int32), coef, dcoef)
        with pytest.raises(OnnxStreamError, match="order 3 at step 3"):       # Taylor3 has orders 0-2 only
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 4, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="one entry per step"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", x, 1, *sc, order[:-1], coef, dcoef)
        with pytest.raises(OnnxStreamError, match="2 \\* prompts"):
            m.hip_sampler_loop_multistep("sample", "timestep", "out_sample", np.zeros((2,) + L[1:], np.float32), 1, *sc, order, coef, dcoef)
        with pytest.raises(OnnxStreamError, match="not found"):
            m.hip_sampler_loop_multistep("sample", "timestep", "nope", x, 1, *sc, order, coef, dcoef)
        m.close()
