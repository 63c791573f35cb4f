"""-m gpu: latents -> image on the device.

* osg_decode_gather / osg_decode_blend alone (Gpu.decode_gather / Gpu.decode_blend) against the numpy statements of pipeline.py, bit for bit, between guard
  bands, on both access widths (16-byte aligned operands: four pixels per thread; operands pushed off that alignment: one per thread).
* Txt2Img.decode_device / txt2img_device against decode() / decode_tiled() of the same object on the HIP library, bit for bit, and against the reference's
  golden images with the bounds tests/test_pipeline.py::test_hip_pipeline_vs_reference_golden applies to the same pass.
* the full-size decoders: SD_VAE untiled at 64 x 64, its 32-latent form over 64 x 64 (9 tiles) and over 128 x 128 with the SDXL factor (25 tiles)."""
import dataclasses
import os
import tempfile

import numpy as np
import pytest

from onnxstream_amd import pipeline
from onnxstream_amd.pipeline import Txt2Img
from onnxstream_amd.synth import sd_unet, sd_vae
from onnxstream_amd.synth.graph import DirSink

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "pipeline_tiny.npz")
f32 = np.float32
SIZES = [(64, 64, 32, 8), (128, 96, 32, 8), (15, 20, 8, 4), (16, 16, 16, 8)]      # (H, W, tile, up); (15, 20, 8) has origins 0/6/7: three-fold overlaps


def same_bits(a, b):
    """equal bit for bit; a NaN matches a NaN (its sign and payload are the machine's: the host makes -NaN of inf * 0, the device +NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != f32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def special(rng, shape, big):
    """normal values, values `big` times as large (far outside what lands in [0, 255]), zeros of both signs and one infinity"""
    t = rng.standard_normal(shape, dtype=f32)
    flat = t.reshape(-1)
    idx = rng.permutation(flat.size)
    n = max(flat.size // 50, 4)
    flat[idx[:n]] = 0.0
    flat[idx[n:2 * n]] = -0.0
    flat[idx[2 * n:3 * n]] = f32(big) * rng.standard_normal(n, dtype=f32)
    flat[idx[3 * n]] = np.inf
    return t


def banded(gpu, shape, dtype, guard):
    """a fresh 0xFF-filled buffer with `guard` elements before and after the view a kernel is to write"""
    n = int(np.prod(shape))
    whole = gpu.empty((n + 2 * guard,), dtype)
    return whole, whole.view(guard, shape)


def bands_untouched(whole, guard):
    raw = whole.numpy().view(np.uint8)
    g = guard * whole.dtype.itemsize
    return bool((raw[:g] == 0xFF).all() and (raw[-g:] == 0xFF).all())


@pytest.mark.parametrize("guard", [64, 3])          # 64 elements keep every operand 16-byte aligned; 3 push it off: the one-element-per-thread kernels
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("H,W,tile,up", SIZES)
def test_decode_gather_kernel(gpu, H, W, tile, up, P, guard):
    rng = np.random.default_rng(H * 131 + W * 7 + P)
    lat = special(rng, (P, 4, H, W), 1e4)
    factor = f32(7.67754 if P == 3 else 5.48998)
    oy, ox = pipeline.tile_origins(H, tile), pipeline.tile_origins(W, tile)
    want = np.stack([lat[p, :, y:y + tile, x:x + tile] * factor for p in range(P) for y in oy for x in ox]).astype(f32)
    whole, out = banded(gpu, want.shape, f32, guard)
    src_whole = gpu.to_dev(np.concatenate([np.zeros(guard, f32), lat.reshape(-1), np.zeros(guard, f32)]))
    got = gpu.decode_gather(src_whole.view(guard, lat.shape), tile, float(factor), out=out).numpy()
    assert np.isinf(want).any() and (want == 0).any()
    assert same_bits(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert bands_untouched(whole, guard)


@pytest.mark.parametrize("guard", [64, 3])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("H,W,tile,up", SIZES)
def test_decode_blend_kernel(gpu, H, W, tile, up, P, guard):
    rng = np.random.default_rng(H * 17 + W * 5 + P)
    T = len(pipeline.tile_origins(H, tile)) * len(pipeline.tile_origins(W, tile))
    tiles = special(rng, (P * T, 3, tile * up, tile * up), 1e3)
    want = pipeline.blend_fold(tiles, H, W, tile, up)
    want_px = pipeline.to_pixels(want)
    assert (~np.isfinite(want)).any() and (want_px == 0).any() and (want_px == 255).any() and ((want_px > 0) & (want_px < 255)).any()
    src_whole = gpu.to_dev(np.concatenate([np.zeros(guard, f32), tiles.reshape(-1), np.zeros(guard, f32)]))
    src = src_whole.view(guard, tiles.shape)
    for form in ("f32", "u8", "both"):
        wi, image = banded(gpu, want.shape, f32, guard)
        wp, pixels = banded(gpu, want_px.shape, np.uint8, guard)
        img, pix = gpu.decode_blend(src, P, H, W, tile, want=form, image=image if form != "u8" else None, pixels=pixels if form != "f32" else None)
        assert (img is None) == (form == "u8") and (pix is None) == (form == "f32")
        if img is not None:
            assert same_bits(img.numpy(), want), form
        else:
            assert (wi.numpy().view(np.uint8) == 0xFF).all()
        if pix is not None:
            assert np.array_equal(pix.numpy(), want_px), form
        else:
            assert (wp.numpy() == 0xFF).all()
        assert bands_untouched(wi, guard) and bands_untouched(wp, guard)


def test_decode_kernels_refuse_bad_extents(gpu):
    from onnxstream_amd.osgpu import OsgError
    lat = gpu.to_dev(np.zeros((1, 4, 8, 8), f32))
    with pytest.raises(OsgError, match="osg_decode_gather"):
        gpu._ck(gpu.lib.osg_decode_gather(gpu.ctx, lat.ptr, lat.ptr, 1, 8, 8, 16, 1.0))
    with pytest.raises(OsgError, match="osg_decode_blend"):
        gpu._ck(gpu.lib.osg_decode_blend(gpu.ctx, lat.ptr, lat.ptr, None, 1, 8, 8, 16, 8))


def _emit(d):
    du, dv, dt = d + "/unet/", d + "/vae/", d + "/vae_t/"
    sd_unet.build_unet(DirSink(du), sd_unet.TINY)
    sd_vae.build_vae_decoder(DirSink(dv), sd_vae.TINY_VAE)
    sd_vae.build_vae_decoder(DirSink(dt), dataclasses.replace(sd_vae.TINY_VAE, latent=8, in_name="latent_sample"))
    return du, dv, dt


TILED = ("latent_sample", "out_image")


def _check_against_host(p, lats, host, **kw):
    """decode_device in its three forms on two sets of latents (the second one on the resident plan), then the host method of the same object"""
    got = []
    for i, lat in enumerate(lats):
        img = p.decode_device(lat, want="f32", **kw)
        if i == 0:
            built = p.vae.hip_plans_built()
        px = p.decode_device(lat, want="u8", **kw)
        both = p.decode_device(lat, want="both", **kw)
        assert p.last_decode_ms > 0
        assert img.dtype == f32 and px.dtype == np.uint8 and px.shape == (img.shape[0],) + img.shape[2:] + (3,)
        assert np.array_equal(both[0], img) and np.array_equal(both[1], px)
        assert np.array_equal(px, pipeline.to_pixels(img))
        got.append(img)
    assert p.vae.hip_plans_built() == built                 # the second image reused plan and captured pass
    for lat, img in zip(lats, got):
        want = host(lat)
        assert np.isfinite(want).all() and float(np.abs(want).max()) > 0
        assert same_bits(img, want), float(np.abs(img - want).max())
    return got


def test_decode_device_matches_the_host_methods_and_the_reference_golden():
    from onnxstream_amd import build as b
    z = np.load(GOLD)
    rng = np.random.default_rng(11)
    other = rng.standard_normal(z["latents"].shape, dtype=f32)
    with tempfile.TemporaryDirectory() as d:
        du, dv, dt = _emit(d)
        p = Txt2Img(b.LIB_HOST, du, dv, batched=True)
        img = _check_against_host(p, [z["latents"], other], p.decode)[0]
        # a 2-image batch: one pass of batch 2
        two = np.concatenate([other, z["latents"]])
        _check_against_host(p, [two, two[::-1]], p.decode)
        # txt2img_device == decode(sample_device(...))
        kw = dict(steps=3, seed=9, latent_shape=(1, 4, 16, 16))
        e2e = p.txt2img_device(z["cond"], z["uncond"], **kw)
        assert same_bits(e2e, p.decode(p.sample_device(z["cond"], z["uncond"], **kw)))
        p.close()
        pt = Txt2Img(b.LIB_HOST, du, dt, batched=True)      # the 8-wide decoder over 16 x 16 latents: 9 tiles, one pass of batch 9
        img_t = _check_against_host(pt, [z["latents"], other], lambda lat: pt.decode_tiled(lat, tile=8), names=TILED)[0]
        # two images through the tiled decoder are ONE pass of batch 18, which no host method runs (decode_tiled() takes one image): the host side is
        # the same 18 pushes through the same library, folded by blend_fold
        def tiled2(lat):
            o = pipeline.tile_origins(16, 8)
            z = (lat * f32(5.48998)).astype(f32)
            pushes = [{TILED[0]: np.ascontiguousarray(z[i:i + 1, :, y:y + 8, x:x + 8])} for i in range(lat.shape[0]) for y in o for x in o]
            outs = np.concatenate(pt._run(pt.vae, pushes, TILED[1]))
            return pipeline.blend_fold(outs, 16, 16, 8, outs.shape[-1] // 8)
        _check_against_host(pt, [two, two[::-1]], tiled2, names=TILED)
        # the SDXL factor reaches the kernel
        assert same_bits(pt.decode_device(other, factor=7.67754, names=TILED), pt.decode_tiled(other, tile=8, factor=7.67754))
        pt.close()
    # the bounds of tests/test_pipeline.py::test_hip_pipeline_vs_reference_golden: the pass is the same
    e_img = float(np.abs(img - z["image"]).max() / np.abs(z["image"]).max())
    e_tiled = float(np.abs(img_t - z["image_tiled"]).max() / np.abs(z["image_tiled"]).max())
    print(f"decode_device vs the reference: image {e_img:.2e}  tiled image {e_tiled:.2e}")
    assert e_img <= 5e-3 and e_tiled <= 5e-3


def _synth(cfg):
    d = os.path.join(os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth"), cfg.name) + "/"
    if not os.path.exists(d + ".complete"):
        os.makedirs(d, exist_ok=True)
        sd_vae.build_vae_decoder(DirSink(d), cfg)
        open(d + ".complete", "w").write("ok")
    return d


FULL = {"untiled64": (sd_vae.SD_VAE, 64, 5.48998),
        "tiled64": (dataclasses.replace(sd_vae.SD_VAE, latent=32, in_name="latent_sample", name="sd_vae_l32"), 64, 5.48998),
        "tiled128": (dataclasses.replace(sd_vae.SD_VAE, latent=32, in_name="latent_sample", name="sd_vae_l32"), 128, 7.67754)}


@pytest.mark.parametrize("case", list(FULL))
def test_decode_device_full_size(case):
    from onnxstream_amd import build as b
    cfg, n, factor = FULL[case]
    d = _synth(cfg)
    lat = np.random.default_rng(n).standard_normal((1, 4, n, n), dtype=f32)
    p = Txt2Img(b.LIB_HOST, d, d, batched=True, names=dict(vae_in=cfg.in_name))
    names = (cfg.in_name, "out_image")
    host = (lambda v: p.decode(v, factor=factor)) if cfg.latent == n else (lambda v: p.decode_tiled(v, tile=cfg.latent, names=names, factor=factor))
    # the first call plans with these latents (the input staging then holds their tiles already); the second set goes through the gather alone
    other = np.random.default_rng(n + 1).standard_normal((1, 4, n, n), dtype=f32)
    for v in (lat, other):
        img, px = p.decode_device(v, factor=factor, names=names, want="both")
        assert img.shape == (1, 3, 8 * n, 8 * n) and np.array_equal(px, pipeline.to_pixels(img))
        want = host(v)
        assert np.isfinite(want).all() and float(np.abs(want).max()) > 0 and same_bits(img, want), float(np.abs(img - want).max())
    assert not np.array_equal(host(lat), want)
    assert p.vae.hip_plans_built() == 1
    p.close()
