"""SDXL and SDXL Turbo in the device sampler loop (osg_sampler_*_single, Plan::sampler_loop / sampler_loop_multistep with one sample per prompt).

(a) every guidance-free entry point against the host restatement (pipeline.multistep_update with den = eps*c_out + x, which tests/test_sdxl_turbo_cpu.py
    pins to the reference application), bit for bit; prompts 1 and 3 -- an odd count is the smallest that tells eps[p] from eps[2p] -- and a latent
    length that is not a multiple of the 256-thread block;
(b) Txt2Img.sample_device against Txt2Img.sample on the same HIP backend, bit for bit, on a micro UNet with the SDXL interface (12 x 20 latents):
    Turbo with every sampler at 1 and 4 steps, SDXL with CFG at 5 steps, 1 and 3 prompts with extras of their own, and a second image on new
    contexts and extras with the plan kept resident;
(c) a Turbo plan and a CFG plan in sequence on one Txt2Img; SD 1.5 without the new arguments as before."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.pipeline import SAMPLERS, Txt2Img, multistep_update
from onnxstream_amd.synth.graph import DirSink

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_golden_sdxl_loop as t  # noqa: E402

f32 = np.float32
L_ODD = 1000                  # 3 full blocks of 256 and a tail of 232
# form -> how many history entries it reads (h1..h3); every form but DDIM writes h0
READS = {0: 0, 1: 1, 2: 0, 3: 1, 4: 1, 5: 2, 6: 3, 7: 1, 8: 2, 9: 3, 10: 1, 11: 2, 12: 0}


@pytest.fixture(scope="module")
def gpu():
    from onnxstream_amd import osgpu
    g = osgpu.Gpu(0)
    yield g
    g.close()


@pytest.mark.parametrize("prompts", [1, 3])
@pytest.mark.parametrize("form", sorted(READS))
def test_multistep_single_kernel_matches_host_restatement(gpu, form, prompts):
    rng = np.random.default_rng(200 + 7 * form + prompts)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(3)
    eps = rng.standard_normal((prompts, L_ODD), dtype=f32)
    hist_in = [rng.standard_normal((prompts, L_ODD), dtype=f32) for _ in range(4)]
    c_out, sigma = f32(-2.5), f32(2.5)
    k = rng.standard_normal(5, dtype=f32)
    dk = (0.93125, 0.0731) if form == 12 else (0.0, 0.0)
    n = READS[form]
    # device: h0 pre-filled with NaN (it must be overwritten), except for DPM++ 2M, whose h1 IS h0 (one slot, read before it is overwritten)
    aliased = form == 1
    bufs = [gpu.to_dev(hist_in[0] if aliased else np.full((prompts, L_ODD), np.nan, f32))] + [gpu.to_dev(h) for h in hist_in[1:]]
    xd, ed = gpu.to_dev(x), gpu.to_dev(eps)
    hp = [bufs[0].ptr if form != 12 else None, bufs[0].ptr if aliased else (bufs[1].ptr if n >= 1 else None),
          bufs[2].ptr if n >= 2 else None, bufs[3].ptr if n >= 3 else None]
    gpu._ck(gpu.lib.osg_sampler_multistep_single(gpu.ctx, form, xd.ptr, ed.ptr, *hp, prompts, L_ODD, c_out, sigma, *[float(v) for v in k], *dk))
    got_x, got_h0 = xd.numpy(), bufs[0].numpy()
    den = (eps * c_out) + x                                                        # CFGDenoiser_CompVisDenoiser's cond branch alone
    h0 = np.full((prompts, L_ODD), np.nan, f32) if not aliased else hist_in[0].copy()
    hist = [h0, h0 if aliased else hist_in[1], hist_in[2], hist_in[3]]
    want_x = multistep_update(form, x, den, hist, sigma, k, dk)
    assert np.isfinite(want_x).all()
    assert np.array_equal(got_x, want_x), float(np.abs(got_x.astype(np.float64) - want_x).max())
    if form == 12:
        assert np.isnan(got_h0).all()                                              # DDIM keeps no history
    else:
        assert np.isfinite(got_h0).all() and np.array_equal(got_h0, h0)
    for j in (1, 2, 3):
        assert np.array_equal(bufs[j].numpy(), hist_in[j])                         # the older entries are only read


@pytest.mark.parametrize("prompts", [1, 3])
@pytest.mark.parametrize("with_noise", [False, True])
def test_euler_a_single_kernel(gpu, prompts, with_noise):
    rng = np.random.default_rng(10 * prompts + with_noise)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(3)
    eps = rng.standard_normal((prompts, L_ODD), dtype=f32)
    noise = rng.standard_normal((prompts, L_ODD), dtype=f32)
    c_out, sigma, d_sigma, sigma_up = f32(-2.5), f32(2.5), f32(-0.8125), f32(0.7)
    xd, ed, nd = gpu.to_dev(x), gpu.to_dev(eps), gpu.to_dev(noise)
    gpu._ck(gpu.lib.osg_sampler_euler_a_single(gpu.ctx, xd.ptr, ed.ptr, nd.ptr if with_noise else None, prompts, L_ODD, c_out, sigma, d_sigma, sigma_up, 0.0))
    den = (eps * c_out) + x
    want = x + (((x - den) / sigma) * d_sigma)
    if with_noise:
        want = want + (noise * sigma_up)
    assert np.array_equal(xd.numpy(), want)
    gpu._ck(gpu.lib.osg_sampler_euler_a_single(gpu.ctx, xd.ptr, ed.ptr, None, prompts, L_ODD, c_out, sigma, d_sigma, sigma_up, 0.5))
    assert np.abs(xd.numpy()).max() <= 0.5                                         # clip, as in the CFG kernel


@pytest.mark.parametrize("prompts", [1, 3])
@pytest.mark.parametrize("scale", [1.0, 1.0717734])
def test_prepare_single_kernel(gpu, prompts, scale):
    rng = np.random.default_rng(prompts)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(14)
    scale, c_in, tv = f32(scale), f32(0.0682), f32(999.0)
    xd = gpu.to_dev(x)
    sample = gpu.to_dev(np.full((prompts + 1, L_ODD), np.nan, f32))               # one row more than the kernel may touch
    ts = gpu.to_dev(np.full(prompts + 1, np.nan, f32))
    gpu._ck(gpu.lib.osg_sampler_prepare_single(gpu.ctx, xd.ptr, sample.ptr, ts.ptr, prompts, L_ODD, scale, c_in, tv, 1))
    xs = x * scale
    assert np.array_equal(xd.numpy(), xs)                                          # (scale 1: x untouched)
    s, tt = sample.numpy(), ts.numpy()
    assert np.array_equal(s[:prompts], xs * c_in) and np.isnan(s[prompts]).all()
    assert (tt[:prompts] == tv).all() and np.isnan(tt[prompts])


def test_multistep_single_kernel_argument_errors(gpu):
    from onnxstream_amd import osgpu
    xd, ed = gpu.to_dev(np.zeros((1, 16), f32)), gpu.to_dev(np.ones((1, 16), f32))
    h = gpu.to_dev(np.zeros((1, 16), f32))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_multistep_single: unknown form 13"):
        gpu._ck(gpu.lib.osg_sampler_multistep_single(gpu.ctx, 13, xd.ptr, ed.ptr, h.ptr, h.ptr, h.ptr, h.ptr, 1, 16, 1.0, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_multistep_single: form 5 needs history pointer h2"):
        gpu._ck(gpu.lib.osg_sampler_multistep_single(gpu.ctx, 5, xd.ptr, ed.ptr, h.ptr, h.ptr, None, None, 1, 16, 1.0, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0))
    assert np.array_equal(xd.numpy(), np.zeros((1, 16), f32))


def _prompt_inputs(rng, prompts, round_):
    """contexts and extras that differ per prompt and per round"""
    emb, emb_neg, pooled, pooled_neg = t.contexts()
    conds = [(emb + f32(0.05 * (k + 3 * round_ + 1)) * rng.standard_normal(emb.shape, dtype=f32))[None] for k in range(prompts)]
    unconds = [(emb_neg + f32(0.02 * (k + 3 * round_)) * rng.standard_normal(emb.shape, dtype=f32))[None] for k in range(prompts)]
    ec = [t.extras(pooled + f32(0.3 * (k + 2 * round_)) * rng.standard_normal(pooled.shape, dtype=f32)) for k in range(prompts)]
    eu = [t.extras(pooled_neg + f32(0.2 * (k + 2 * round_ + 1)) * rng.standard_normal(pooled.shape, dtype=f32)) for k in range(prompts)]
    for k in range(prompts):          # the application pushes one constant time_ids; a test of the plumbing wants them to differ
        ec[k][t.NAMES["time_ids"]] = t.TIME_IDS + f32(64 * (k + round_))
        eu[k][t.NAMES["time_ids"]] = t.TIME_IDS - f32(32 * (k + round_ + 1))
    return conds, unconds, ec, eu


def _one(v, prompts):
    return v[0] if prompts == 1 else v


CASES = [("turbo", s, n) for s in SAMPLERS for n in (1, 4)] + [("xl", s, 5) for s in ("euler_a", "dpm++2m", "ddim")]


@pytest.mark.parametrize("prompts", [1, 3])
def test_device_sdxl_loops_match_host_loop_bitwise(prompts):
    from onnxstream_amd import build as b
    rng = np.random.default_rng(12)
    shape = (prompts, 4, t.LAT_H, t.LAT_W)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_sdxl_unet(DirSink(d))
        ph = Txt2Img(b.LIB_HOST, d, None, batched=True)
        pd = {m: Txt2Img(b.LIB_HOST, d, None, batched=True) for m in ("turbo", "xl")}        # one resident plan per mode: P and 2P samples
        try:
            for mode, sampler, steps in CASES:
                for round_ in range(2):          # round 1: new contexts and extras, the plan and the history ring stay resident
                    conds, unconds, ec, eu = _prompt_inputs(rng, prompts, round_)
                    kw = dict(steps=steps, seed=31 + round_, latent_shape=shape, sampler=sampler, extra_cond=_one(ec, prompts),
                              extra_uncond=_one(eu, prompts), xl=True, turbo=mode == "turbo")
                    want = ph.sample(_one(conds, prompts), _one(unconds, prompts), **kw)
                    built = pd[mode].unet.hip_plans_built()
                    got = pd[mode].sample_device(_one(conds, prompts), None if mode == "turbo" else _one(unconds, prompts), **kw)
                    assert np.isfinite(want).all() and np.abs(want).max() > 0, (mode, sampler, steps)
                    assert np.array_equal(got, want), (mode, sampler, steps, round_, float(np.abs(got - want).max()))
                    assert built == 0 or pd[mode].unet.hip_plans_built() == built          # only the first image of a mode plans
            # the extras reach the UNet: the same image with prompt 0's pooled embedding of the other branch is another image
            conds, unconds, ec, eu = _prompt_inputs(rng, prompts, 0)
            kw = dict(steps=2, seed=5, latent_shape=shape, sampler="euler", turbo=True)
            a = pd["turbo"].sample_device(_one(conds, prompts), None, extra_cond=_one(ec, prompts), **kw)
            b2 = pd["turbo"].sample_device(_one(conds, prompts), None, extra_cond=_one([eu[0]] + ec[1:], prompts), **kw)
            assert not np.array_equal(a[0], b2[0]) and np.array_equal(a[1:], b2[1:])
        finally:
            ph.close()
            for p in pd.values():
                p.close()


def test_turbo_then_cfg_on_one_pipeline():
    """a plan of P samples and a plan of 2P samples in sequence on ONE Txt2Img (a Model keeps one plan): each call must find or rebuild its own"""
    from onnxstream_amd import build as b
    rng = np.random.default_rng(13)
    prompts = 2
    shape = (prompts, 4, t.LAT_H, t.LAT_W)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_sdxl_unet(DirSink(d))
        ph = Txt2Img(b.LIB_HOST, d, None, batched=True)
        pd = Txt2Img(b.LIB_HOST, d, None, batched=True)
        try:
            for k, (turbo, sampler) in enumerate([(True, "dpm++2m"), (False, "dpm++2m"), (True, "euler_a"), (False, "ipndm"), (False, "euler_a")]):
                conds, unconds, ec, eu = _prompt_inputs(rng, prompts, k)
                kw = dict(steps=3, seed=40 + k, latent_shape=shape, sampler=sampler, extra_cond=ec, extra_uncond=eu, xl=True, turbo=turbo)
                want = ph.sample(conds, unconds, **kw)
                got = pd.sample_device(conds, None if turbo else unconds, **kw)
                assert np.array_equal(got, want), (k, turbo, sampler, float(np.abs(got - want).max()))
            assert pd.unet.hip_plans_built() == 4        # P, 2P, P, 2P -- and the fifth image reused the fourth's
        finally:
            ph.close()
            pd.close()


def test_sd15_device_loop_unchanged():
    """sample_device() without the new arguments on the SD 1.5 micro UNet still equals sample()"""
    from onnxstream_amd import build as b
    import make_golden_sd_loop as sdl
    cond, uncond = sdl.contexts()
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        ph = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        pd = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        try:
            for sampler in ("euler_a", "dpm++2m", "ddim"):
                kw = dict(steps=5, seed=3, latent_shape=(1, 4, 64, 64), sampler=sampler)
                want = ph.sample(cond[None], uncond[None], **kw)
                assert np.array_equal(pd.sample_device(cond[None], uncond[None], **kw), want), sampler
            assert pd.unet.hip_plans_built() == 1
        finally:
            ph.close()
            pd.close()
