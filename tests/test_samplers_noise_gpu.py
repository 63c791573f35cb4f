"""The samplers that add fresh noise per step on the device (osg_sampler_cfg_stochastic / osg_sampler_stochastic_single, Plan::sampler_loop_stochastic).

(a) every update form of the kernel against pipeline.stochastic_update (the host restatement that tests/test_samplers_noise_cpu.py pins to the
    reference application), bit for bit, for the pair entry and the single entry, with and without a noise pointer; prompts 1 and 3 -- an odd count
    tells eps[p] from eps[2p] -- and a latent length that is not a multiple of the 256-thread block;
(b) the launcher's argument errors;
(c) Txt2Img.sample_device against Txt2Img.sample on the same HIP backend, bit for bit, for all eight samplers: 20 steps on the micro UNet, 1 and 3
    prompts, and a second image on new contexts with the plan kept resident (history ring and noise buffer must not carry over);
(d) the same in Turbo mode on the 12 x 20 micro SDXL UNet at 1 and 4 steps, and dpm++3msde_a with CFG and the SDXL last-step rule at 5 steps."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd import pipeline
from onnxstream_amd.pipeline import Txt2Img
from onnxstream_amd.synth.graph import DirSink

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_golden_sd_loop as sdl  # noqa: E402
import make_golden_sdxl_loop as xll  # noqa: E402

f32 = np.float32
L_ODD = 1000                  # 3 full blocks of 256 and a tail of 232
EIGHT = ("ddpm", "ddpm_a", "ddim_a", "tcd", "tcd_a", "lcm", "dpm++3msde", "dpm++3msde_a")
# osg_stochastic_form -> how many history entries it reads (h1, h2); the SDE forms (5, 6, 7) write h0
READS = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 1, 7: 2}
SDE = (5, 6, 7)


@pytest.fixture(scope="module")
def gpu():
    from onnxstream_amd import osgpu
    g = osgpu.Gpu(0)
    yield g
    g.close()


def _den(x, eps, c_out, guidance, pair):
    """the kernel's den: the CFG combine of the pair eps[2p], eps[2p+1] (as Txt2Img.denoise), or eps[p]*c_out + x alone"""
    if not pair:
        return (eps * c_out) + x
    den_c = (eps[0::2] * c_out) + x
    den_u = (eps[1::2] * c_out) + x
    return den_u + (f32(guidance) * (den_c - den_u))


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("prompts", [1, 3])
@pytest.mark.parametrize("pair", [True, False], ids=["cfg", "single"])
@pytest.mark.parametrize("form", sorted(READS))
def test_stochastic_kernel_matches_host_restatement(gpu, form, pair, prompts, with_noise):
    rng = np.random.default_rng(300 + 16 * form + 4 * prompts + 2 * pair + with_noise)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(3)
    eps = rng.standard_normal(((2 if pair else 1) * prompts, L_ODD), dtype=f32)
    noise = rng.standard_normal((prompts, L_ODD), dtype=f32)
    hist_in = [None] + [rng.standard_normal((prompts, L_ODD), dtype=f32) for _ in range(2)]
    c_out, guidance, sigma = f32(-2.5), 7.0, f32(2.5)
    k = rng.standard_normal(9, dtype=f32)
    k[1:5] = np.abs(k[1:5]) + f32(0.5)                           # divisors (DDIM-a's k1, the SDE forms' k2..k4) stay away from 0
    n = READS[form]
    bufs = [gpu.to_dev(np.full((prompts, L_ODD), np.nan, f32))] + [gpu.to_dev(h) for h in hist_in[1:]]      # h0 pre-filled with NaN
    xd, ed, nd = gpu.to_dev(x), gpu.to_dev(eps), gpu.to_dev(noise)
    hp = [bufs[0].ptr if form in SDE else None, bufs[1].ptr if n >= 1 else None, bufs[2].ptr if n >= 2 else None]
    args = [form, xd.ptr, ed.ptr, nd.ptr if with_noise else None, *hp, prompts, L_ODD, c_out] + ([guidance] if pair else []) + [sigma] + [float(v) for v in k]
    gpu._ck((gpu.lib.osg_sampler_cfg_stochastic if pair else gpu.lib.osg_sampler_stochastic_single)(gpu.ctx, *args))
    got_x, got_h0 = xd.numpy(), bufs[0].numpy()
    # host
    den = _den(x, eps, c_out, guidance, pair)
    h0 = np.full((prompts, L_ODD), np.nan, f32)
    want_x = pipeline.stochastic_update(form, x, den, [h0, hist_in[1], hist_in[2]], sigma, k, noise if with_noise else None)
    assert np.isfinite(want_x).all()
    assert np.array_equal(got_x, want_x), float(np.abs(got_x.astype(np.float64) - want_x).max())
    if with_noise:                                               # the tail did something: without the pointer the result is another
        assert not np.array_equal(want_x, pipeline.stochastic_update(form, x, den, [h0.copy(), hist_in[1], hist_in[2]], sigma, k, None))
    if form in SDE:
        assert np.array_equal(got_h0, den) and np.array_equal(h0, den)                 # history holds den
    else:
        assert np.isnan(got_h0).all() and np.isnan(h0).all()
    for j in (1, 2):
        assert np.array_equal(bufs[j].numpy(), hist_in[j])                             # the older entries are only read
    assert np.array_equal(nd.numpy(), noise) and np.array_equal(ed.numpy(), eps)


def test_tcd_tail_is_the_shared_tail_at_n1_equal_1(gpu):
    """x = (n1*x') + (n0*noise) with n1 = 1 has the bits of x' + (noise*n0): multiplying by 1 is exact and the product commutes"""
    rng = np.random.default_rng(7)
    x, eps, noise = (rng.standard_normal((1, L_ODD), dtype=f32) for _ in range(3))
    k = np.asarray([0.7, 0.9, 0.3, 0, 0, 0, 0, 0.45, 1.0], f32)
    xd, ed, nd = gpu.to_dev(x), gpu.to_dev(eps), gpu.to_dev(noise)
    gpu._ck(gpu.lib.osg_sampler_stochastic_single(gpu.ctx, 4, xd.ptr, ed.ptr, nd.ptr, None, None, None, 1, L_ODD, -2.5, 2.5, *[float(v) for v in k]))
    plain = pipeline.stochastic_update(4, x, (eps * f32(-2.5)) + x, [None] * 3, f32(2.5), k, None)
    assert np.array_equal(xd.numpy(), plain + (noise * k[7]))


def test_stochastic_kernel_argument_errors(gpu):
    from onnxstream_amd import osgpu
    xd, e2, e1 = gpu.to_dev(np.zeros((1, 16), f32)), gpu.to_dev(np.ones((2, 16), f32)), gpu.to_dev(np.ones((1, 16), f32))
    h = [gpu.to_dev(np.zeros((1, 16), f32)) for _ in range(3)]
    z9 = [0.0] * 9
    with pytest.raises(osgpu.OsgError, match="osg_sampler_cfg_stochastic: unknown form 8"):
        gpu._ck(gpu.lib.osg_sampler_cfg_stochastic(gpu.ctx, 8, xd.ptr, e2.ptr, None, h[0].ptr, h[1].ptr, h[2].ptr, 1, 16, 1.0, 7.0, 1.0, *z9))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_stochastic_single: unknown form -1"):
        gpu._ck(gpu.lib.osg_sampler_stochastic_single(gpu.ctx, -1, xd.ptr, e1.ptr, None, h[0].ptr, h[1].ptr, h[2].ptr, 1, 16, 1.0, 1.0, *z9))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_cfg_stochastic: form 7 needs history pointer h2"):
        gpu._ck(gpu.lib.osg_sampler_cfg_stochastic(gpu.ctx, 7, xd.ptr, e2.ptr, None, h[0].ptr, h[1].ptr, None, 1, 16, 1.0, 7.0, 1.0, *z9))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_stochastic_single: form 6 needs history pointer h1"):
        gpu._ck(gpu.lib.osg_sampler_stochastic_single(gpu.ctx, 6, xd.ptr, e1.ptr, None, h[0].ptr, None, None, 1, 16, 1.0, 1.0, *z9))
    with pytest.raises(osgpu.OsgError, match="osg_sampler_cfg_stochastic: form 5 needs history pointer h0"):
        gpu._ck(gpu.lib.osg_sampler_cfg_stochastic(gpu.ctx, 5, xd.ptr, e2.ptr, None, None, None, None, 1, 16, 1.0, 7.0, 1.0, *z9))
    gpu._ck(gpu.lib.osg_sampler_cfg_stochastic(gpu.ctx, 1, xd.ptr, e2.ptr, None, None, None, None, 0, 16, 1.0, 7.0, 1.0, *z9))       # no prompts: a no-op
    gpu._ck(gpu.lib.osg_sampler_stochastic_single(gpu.ctx, 1, xd.ptr, e1.ptr, None, None, None, None, 1, 0, 1.0, 1.0, *z9))
    assert np.array_equal(xd.numpy(), np.zeros((1, 16), f32))


@pytest.mark.parametrize("prompts", [1, 3])
def test_device_stochastic_loops_match_host_loop_bitwise(prompts):
    from onnxstream_amd import build as b
    cond, uncond = sdl.contexts()
    rng = np.random.default_rng(21)
    shape = (prompts, 4, 64, 64)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        ph = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        pd = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        try:
            for sampler in EIGHT:
                for round_ in range(2):          # round 1: new contexts, the plan, the history ring and the noise buffer stay resident
                    conds = [(cond + f32(0.05 * (k + 3 * round_)) * rng.standard_normal(cond.shape, dtype=f32))[None] for k in range(prompts)]
                    unconds = [uncond[None]] * prompts
                    c, u = (conds[0], unconds[0]) if prompts == 1 else (conds, unconds)
                    kw = dict(steps=20, seed=51 + round_, latent_shape=shape, sampler=sampler)
                    want = ph.sample(c, u, **kw)
                    got = pd.sample_device(c, u, **kw)
                    assert np.array_equal(got, want, equal_nan=True), (sampler, round_)
                    if not np.isfinite(want).all():
                        # the micro UNet does not denoise and this trajectory overflowed (the reference's own lcm run does, past 17 steps): a NaN
                        # agrees with anything that made it, so the comparison that counts is the longest image that stays finite
                        kw["steps"] = 10
                        want = ph.sample(c, u, **kw)
                        got = pd.sample_device(c, u, **kw)
                        assert np.array_equal(got, want), (sampler, round_, float(np.abs(got - want).max()))
                    assert np.isfinite(want).all() and np.abs(want).max() > 0, sampler
            assert pd.unet.hip_plans_built() == 1
        finally:
            ph.close()
            pd.close()


def _prompt_inputs(rng, prompts, round_):
    """contexts and extras that differ per prompt and per round"""
    emb, emb_neg, pooled, pooled_neg = xll.contexts()
    conds = [(emb + f32(0.05 * (k + 3 * round_ + 1)) * rng.standard_normal(emb.shape, dtype=f32))[None] for k in range(prompts)]
    unconds = [(emb_neg + f32(0.02 * (k + 3 * round_)) * rng.standard_normal(emb.shape, dtype=f32))[None] for k in range(prompts)]
    ec = [xll.extras(pooled + f32(0.3 * (k + 2 * round_)) * rng.standard_normal(pooled.shape, dtype=f32)) for k in range(prompts)]
    eu = [xll.extras(pooled_neg + f32(0.2 * (k + 2 * round_ + 1)) * rng.standard_normal(pooled.shape, dtype=f32)) for k in range(prompts)]
    return conds, unconds, ec, eu


def _one(v, prompts):
    return v[0] if prompts == 1 else v


XL_CASES = [("turbo", s, n) for s in EIGHT for n in (1, 4)] + [("xl", "dpm++3msde_a", 5)]


@pytest.mark.parametrize("prompts", [1, 3])
def test_device_stochastic_sdxl_loops_match_host_loop_bitwise(prompts):
    from onnxstream_amd import build as b
    rng = np.random.default_rng(22)
    shape = (prompts, 4, xll.LAT_H, xll.LAT_W)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        xll.build_micro_sdxl_unet(DirSink(d))
        ph = Txt2Img(b.LIB_HOST, d, None, batched=True)
        pd = {m: Txt2Img(b.LIB_HOST, d, None, batched=True) for m in ("turbo", "xl")}        # one resident plan per mode: P and 2P samples
        try:
            for mode, sampler, steps in XL_CASES:
                for round_ in range(2):          # round 1: new contexts and extras, the plan stays resident
                    conds, unconds, ec, eu = _prompt_inputs(rng, prompts, round_)
                    kw = dict(steps=steps, seed=61 + round_, latent_shape=shape, sampler=sampler, extra_cond=_one(ec, prompts),
                              extra_uncond=_one(eu, prompts), xl=True, turbo=mode == "turbo")
                    want = ph.sample(_one(conds, prompts), _one(unconds, prompts), **kw)
                    got = pd[mode].sample_device(_one(conds, prompts), None if mode == "turbo" else _one(unconds, prompts), **kw)
                    assert np.isfinite(want).all() and np.abs(want).max() > 0, (mode, sampler, steps)
                    assert np.array_equal(got, want), (mode, sampler, steps, round_, float(np.abs(got - want).max()))
            assert pd["turbo"].unet.hip_plans_built() == 1 and pd["xl"].unet.hip_plans_built() == 1
        finally:
            ph.close()
            for p in pd.values():
                p.close()
