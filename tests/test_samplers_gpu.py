"""The multistep samplers on the device (osg_sampler_cfg_multistep / osg_sampler_prepare_rescale, Plan::sampler_loop_multistep).

(a) every update form and order of the kernel against pipeline.multistep_update (the host restatement that tests/test_samplers_cpu.py pins to the
    reference application), bit for bit; prompts 1 and 3 and a latent length that is not a multiple of the 256-thread block;
(b) Txt2Img.sample_device against Txt2Img.sample on the same HIP backend, bit for bit, for every multistep sampler: 20 steps on the micro UNet,
    1 and 3 prompts, and a second image on new contexts with the plan kept resident (the history ring must not carry over)."""
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd.pipeline import MULTISTEP, Txt2Img, multistep_update
from onnxstream_amd.synth.graph import DirSink

pytestmark = pytest.mark.gpu

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


def _den(x, eps, c_out, guidance):
    """the CFG combine of the kernel (and of Txt2Img.denoise): den_c = eps[2p]*c_out + x, den_u = eps[2p+1]*c_out + x, den_u + g*(den_c - den_u)"""
    den_c = (eps[0::2] * c_out) + x
    den_u = (eps[1::2] * c_out) + x
    return den_u + (f32(guidance) * (den_c - den_u))


@pytest.mark.parametrize("prompts", [1, 3])
@pytest.mark.parametrize("form", sorted(READS))
def test_multistep_kernel_matches_host_restatement(gpu, form, prompts):
    rng = np.random.default_rng(100 + 7 * form + prompts)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(3)
    eps = rng.standard_normal((2 * prompts, L_ODD), dtype=f32)
    hist_in = [rng.standard_normal((prompts, L_ODD), dtype=f32) for _ in range(4)]
    c_out, guidance, sigma = f32(-2.5), 7.0, f32(2.5)
    k = rng.standard_normal(5, dtype=f32)
    dk = (0.93125, 0.0731) if form == 12 else (0.0, 0.0)
    n = READS[form]
    # device: h0 pre-filled with NaN (it must be overwritten), except for DPM++ 2M, whose h1 IS h0 (one slot, read before it is overwritten)
    aliased = form == 1
    bufs = [gpu.to_dev(hist_in[0] if aliased else np.full((prompts, L_ODD), np.nan, f32))] + [gpu.to_dev(h) for h in hist_in[1:]]
    xd, ed = gpu.to_dev(x), gpu.to_dev(eps)
    hp = [bufs[0].ptr if form != 12 else None, bufs[0].ptr if aliased else (bufs[1].ptr if n >= 1 else None),
          bufs[2].ptr if n >= 2 else None, bufs[3].ptr if n >= 3 else None]
    gpu._ck(gpu.lib.osg_sampler_cfg_multistep(gpu.ctx, form, xd.ptr, ed.ptr, *hp, prompts, L_ODD, c_out, guidance, sigma, *[float(v) for v in k], *dk))
    got_x, got_h0 = xd.numpy(), bufs[0].numpy()
    # host
    den = _den(x, eps, c_out, guidance)
    h0 = np.full((prompts, L_ODD), np.nan, f32) if not aliased else hist_in[0].copy()
    hist = [h0, h0 if aliased else hist_in[1], hist_in[2], hist_in[3]]
    want_x = multistep_update(form, x, den, hist, sigma, k, dk)
    assert np.isfinite(want_x).all()
    assert np.array_equal(got_x, want_x), float(np.abs(got_x.astype(np.float64) - want_x).max())
    if form == 12:
        want64 = x.astype(np.float64) * dk[0] + den.astype(np.float64) * dk[1]     # DDIM: double arithmetic, one rounding at the store
        assert np.array_equal(got_x, want64.astype(f32))
        assert np.isnan(got_h0).all()                                              # DDIM keeps no history
    else:
        assert np.isfinite(got_h0).all() and np.array_equal(got_h0, h0)
    for j in (1, 2, 3):
        assert np.array_equal(bufs[j].numpy(), hist_in[j])                         # the older entries are only read


@pytest.mark.parametrize("prompts", [1, 3])
def test_prepare_rescale_kernel(gpu, prompts):
    rng = np.random.default_rng(prompts)
    x = rng.standard_normal((prompts, L_ODD), dtype=f32) * f32(14)
    scale, c_in, t = f32(1.0717734), f32(0.0682), f32(999.0)
    xd = gpu.to_dev(x)
    sample = gpu.to_dev(np.full((2 * prompts, L_ODD), np.nan, f32))
    ts = gpu.to_dev(np.full(2 * prompts, np.nan, f32))
    gpu._ck(gpu.lib.osg_sampler_prepare_rescale(gpu.ctx, xd.ptr, sample.ptr, ts.ptr, prompts, L_ODD, scale, c_in, t, 1))
    xs = x * scale
    assert np.array_equal(xd.numpy(), xs)
    s = sample.numpy()
    assert np.array_equal(s[0::2], xs * c_in) and np.array_equal(s[1::2], xs * c_in)
    assert (ts.numpy() == t).all()


def test_multistep_kernel_argument_errors(gpu):
    from onnxstream_amd import osgpu
    xd, ed = gpu.to_dev(np.zeros((1, 16), f32)), gpu.to_dev(np.zeros((2, 16), f32))
    h = gpu.to_dev(np.zeros((1, 16), f32))
    with pytest.raises(osgpu.OsgError, match="unknown form 13"):
        gpu._ck(gpu.lib.osg_sampler_cfg_multistep(gpu.ctx, 13, xd.ptr, ed.ptr, h.ptr, h.ptr, h.ptr, h.ptr, 1, 16, 1.0, 7.0, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0))
    with pytest.raises(osgpu.OsgError, match="needs history pointer h2"):
        gpu._ck(gpu.lib.osg_sampler_cfg_multistep(gpu.ctx, 5, xd.ptr, ed.ptr, h.ptr, h.ptr, None, None, 1, 16, 1.0, 7.0, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0))
    assert np.array_equal(xd.numpy(), np.zeros((1, 16), f32))


def _sd_loop_tools():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_golden_sd_loop as t
    return t


@pytest.mark.parametrize("prompts", [1, 3])
def test_device_multistep_loops_match_host_loop_bitwise(prompts):
    from onnxstream_amd import build as b
    t = _sd_loop_tools()
    cond, uncond = t.contexts()
    rng = np.random.default_rng(11)
    shape = (prompts, 4, 64, 64)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        t.build_micro_unet(DirSink(d + "unet_fp16/"))
        ph = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        pd = Txt2Img(b.LIB_HOST, d + "unet_fp16/", None, batched=True)
        try:
            for sampler in MULTISTEP:
                for round_ in range(2):          # round 1: new contexts, the plan and the history ring stay resident
                    conds = [(cond + f32(0.05 * (k + 3 * round_)) * rng.standard_normal(cond.shape, dtype=f32))[None] for k in range(prompts)]
                    unconds = [uncond[None]] * prompts
                    kw = dict(steps=20, seed=31 + round_, latent_shape=shape, sampler=sampler)
                    if prompts == 1:
                        want = ph.sample(conds[0], unconds[0], **kw)
                        got = pd.sample_device(conds[0], unconds[0], **kw)
                    else:
                        want = ph.sample(conds, unconds, **kw)
                        got = pd.sample_device(conds, unconds, **kw)
                    assert np.isfinite(want).all() and np.abs(want).max() > 0, sampler
                    assert np.array_equal(got, want), (sampler, round_, float(np.abs(got - want).max()))
        finally:
            ph.close()
            pd.close()
