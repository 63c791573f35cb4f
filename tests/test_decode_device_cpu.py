"""Latents -> image on the device (Txt2Img.decode_device, model_hip_decode, osg_decode_gather / osg_decode_blend), CPU side.

* tile_origins, blend_fold and to_pixels -- the numpy statements the device kernels are pinned to (tests/test_decode_device_gpu.py) -- against known
  answers and against decode_tiled()'s own blend, bit for bit: on random tiles (three-fold overlaps, zeros of both signs, an infinity) and on the
  golden tiled decode through the reference library.
* model_hip_decode's argument checks, over the no-op stand-in for libosgpu.so (tests/stub/make_stub.py)."""
import ctypes
import dataclasses
import os
import sys
import tempfile

import numpy as np
import pytest

from onnxstream_amd import pipeline
from onnxstream_amd.pipeline import Txt2Img
from onnxstream_amd.synth import sd_vae
from onnxstream_amd.synth.graph import DirSink, GraphBuilder
from oracle import ref as oref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "pipeline_tiny.npz")
sys.path.insert(0, os.path.join(HERE, "stub"))
f32 = np.float32


def same_bits(a, b):
    """equal bit for bit; a NaN matches a NaN (its sign and payload are the machine's: x86 makes -NaN of inf * 0)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != f32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


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


def test_tile_origins():
    assert pipeline.tile_origins(64, 32) == [0, 24, 32]
    assert pipeline.tile_origins(128, 32) == [0, 24, 48, 72, 96]
    assert pipeline.tile_origins(60, 32) == [0, 24, 28]
    assert pipeline.tile_origins(32, 32) == [0]
    assert pipeline.tile_origins(15, 8) == [0, 6, 7] and pipeline.tile_origins(20, 8) == [0, 6, 12]
    with pytest.raises(ValueError):
        pipeline.tile_origins(16, 32)


def special_tiles(rng, shape):
    """normal values, values far outside what lands in [0, 255], zeros of both signs and one infinity"""
    t = rng.standard_normal(shape, dtype=f32)
    flat = t.reshape(-1)
    idx = rng.permutation(flat.size)
    n = max(flat.size // 50, 4)
    flat[idx[:n]] = 0.0
    flat[idx[n:2 * n]] = -0.0
    flat[idx[2 * n:3 * n]] = f32(1e4) * rng.standard_normal(n, dtype=f32)
    flat[idx[3 * n]] = np.inf
    return t


def host_tiled(tiles, H, W, tile):
    """decode_tiled()'s blend on given decoder outputs: the method itself, its decoder pass replaced by `tiles`"""
    p = Txt2Img.__new__(Txt2Img)
    p.vae = None
    p._run = lambda m, pushes, out: [tiles[k:k + 1] for k in range(len(pushes))]
    with np.errstate(invalid="ignore"):
        return p.decode_tiled(np.zeros((1, 4, H, W), f32), tile=tile)


@pytest.mark.parametrize("H,W,tile,up", [(64, 64, 32, 2), (15, 20, 8, 4), (60, 32, 32, 1), (16, 16, 16, 8), (128, 96, 32, 1)])
def test_blend_fold_equals_decode_tiled_on_random_tiles(H, W, tile, up):
    rng = np.random.default_rng(H * 1000 + W)
    T = len(pipeline.tile_origins(H, tile)) * len(pipeline.tile_origins(W, tile))
    tiles = special_tiles(rng, (T, 3, tile * up, tile * up))
    want = host_tiled(tiles, H, W, tile)
    got = pipeline.blend_fold(tiles, H, W, tile, up)
    assert got.shape == (1, 3, H * up, W * up) and got.dtype == f32
    assert (~np.isfinite(want)).any() and same_bits(got, want)
    if (H, W, tile) == (15, 20, 8):         # rows 7*up .. 8*up-1 lie in the tiles at 0, 6 and 7: the three-fold overlap is really there
        oy = pipeline.tile_origins(H, tile)
        assert sum(o <= 7 < o + tile for o in oy) == 3
    # several images: image p folds the tiles p*T .. p*T + T - 1
    two = np.concatenate([tiles, tiles[::-1]])
    got2 = pipeline.blend_fold(two, H, W, tile, up)
    assert same_bits(got2[0:1], want) and same_bits(got2[1:2], host_tiled(tiles[::-1], H, W, tile))


@pytest.mark.skipif(not oref.available(), reason="oracle/_ref not built")
def test_blend_fold_equals_decode_tiled_on_the_golden_tiled_decode():
    z = np.load(GOLD)
    with tempfile.TemporaryDirectory() as d:
        dt = d + "/vae_t/"
        sd_vae.build_vae_decoder(DirSink(dt), dataclasses.replace(sd_vae.TINY_VAE, latent=8, in_name="latent_sample"))
        pt = Txt2Img(oref.REF_LIB, dt, dt, batched=False, threads=1)
        seen = []
        run = pt._run
        pt._run = lambda m, pushes, out: seen.append(run(m, pushes, out)) or seen[-1]
        img = pt.decode_tiled(z["latents"], tile=8)
        pt.close()
    assert np.array_equal(img, z["image_tiled"])
    tiles = np.concatenate(seen[0])
    assert tiles.shape[0] == 9
    assert same_bits(pipeline.blend_fold(tiles, 16, 16, 8, tiles.shape[-1] // 8), z["image_tiled"])


def test_to_pixels():
    v = np.array([-1e9, -1.0, -0.5, -0.0, 0.0, 0.99, 1.0, 127.5, 254.99, 255.0, 255.5, 256.0, 1e9, np.inf, -np.inf, np.nan], f32)
    want = np.array([0, 0, 0, 0, 0, 0, 1, 127, 254, 255, 255, 255, 255, 255, 0, 0], np.uint8)
    img = np.stack([v, v[::-1], np.full_like(v, 7.9)]).reshape(1, 3, 1, v.size)
    px = pipeline.to_pixels(img)
    assert px.shape == (1, 1, v.size, 3) and px.dtype == np.uint8 and px.flags.c_contiguous
    assert np.array_equal(px[0, 0, :, 0], want) and np.array_equal(px[0, 0, :, 1], want[::-1]) and (px[0, 0, :, 2] == 7).all()
    # min(max((int)v, 0), 255) wherever (int)v is defined
    r = (np.random.default_rng(3).standard_normal(3072) * 200 + 128).astype(f32)
    assert np.array_equal(pipeline.to_pixels(r.reshape(1, 3, 1, -1))[0, 0].T.reshape(-1), np.clip(np.trunc(r.astype(np.float64)), 0, 255).astype(np.uint8))


def test_decode_and_decode_tiled_take_a_factor():
    """the keyword `factor` scales the latents (SDXL: 7.67754); the default is the SD 1.5 value"""
    for factor in (None, 7.67754):
        seen = []
        p = Txt2Img.__new__(Txt2Img)
        p.vae, p.names = None, dict(vae_in="input.1", vae_out="out_image")
        p._run = lambda m, pushes, out: [seen.append(next(iter(q.values()))) or np.zeros((1, 3, 64, 64), f32) for q in pushes]
        lat = np.random.default_rng(1).standard_normal((1, 4, 8, 8), dtype=f32)
        kw = {} if factor is None else dict(factor=factor)
        p.decode(lat, **kw)
        p.decode_tiled(lat, tile=8, **kw)
        assert all(np.array_equal(s, lat * f32(5.48998 if factor is None else factor)) for s in seen) and len(seen) == 2


def _run_once(m, name, z, n):
    for _ in range(n):
        m.add_tensor(name, z)
    m.run()
    m.clear_tensors()


def test_model_hip_decode_plumbing(stub_backend):
    """model_hip_decode exists and refuses, each with its message: no plan, streamed weights, uint8 arithmetic, an output kept out of the fp32 conversion,
    unknown names, a batch that is not images * tiles, latents smaller than the tile, an output that is no integer multiple of the tile (the stub
    computes nothing: what comes back is the zeroed device buffer)"""
    from onnxstream_amd import build as b
    from onnxstream_amd.bindings import Model, OnnxStreamError
    assert hasattr(ctypes.CDLL(b.LIB_HOST), "model_hip_decode")
    cfg = dataclasses.replace(sd_vae.TINY_VAE, latent=8, in_name="latent_sample")
    names = (cfg.in_name, "out_image")
    z = sd_vae.vae_inputs(cfg)[cfg.in_name]
    lat16 = np.random.default_rng(2).standard_normal((1, 4, 16, 16), dtype=f32)
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        sd_vae.build_vae_decoder(DirSink(d), cfg)
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.set_use_fp16_arithmetic(True)
        m.read_file(d + "model.txt")
        img = np.full((1, 3, 64, 64), 5, f32)              # (the miniature decoder upscales 4x)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: no plan"):
            m.hip_decode(*names, lat16, 5.48998, img)
        _run_once(m, cfg.in_name, z, 9)
        pix = np.full((1, 64, 64, 3), 5, np.uint8)
        assert m.hip_decode(*names, lat16, 5.48998, img, pix) == 0.0
        assert not img.any() and not pix.any()
        assert m.hip_plans_built() == 1
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: input/output tensor not found"):
            m.hip_decode("nope", "out_image", lat16, 5.48998, img)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: input/output tensor not found"):
            m.hip_decode(cfg.in_name, "nope", lat16, 5.48998, img)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the plan's batch is 9, the decode needs images \\* tiles = 2 \\* 9 = 18 samples"):
            m.hip_decode(*names, np.concatenate([lat16, lat16]), 5.48998, np.empty((2, 3, 64, 64), f32))
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the plan's batch is 9, the decode needs images \\* tiles = 1 \\* 1 = 1 samples"):
            m.hip_decode(*names, lat16[:, :, :8, :8], 5.48998, np.empty((1, 3, 32, 32), f32))
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: latents of 4 x 16 are smaller than the tile 8"):
            m.hip_decode(*names, lat16[:, :, :4], 5.48998, np.empty((1, 3, 16, 64), f32))
        # u is the plan's to know (4 for this decoder): a buffer sized for another u is refused, not overrun
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the image buffer holds 768 elements, the decode writes 12288 \\(upscale factor 4\\)"):
            m.hip_decode(*names, lat16, 5.48998, np.empty((1, 3, 16, 16), f32))
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the pixel buffer holds 49152 elements, the decode writes 12288"):
            m.hip_decode(*names, lat16, 5.48998, None, np.empty((1, 128, 128, 3), np.uint8))
        with pytest.raises(OnnxStreamError, match="hip_decode: image must be"):
            m.hip_decode(*names, lat16, 5.48998, np.empty((1, 3, 64, 64), np.float64))
        m.close()

        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.set_use_fp16_arithmetic(True)
        m.read_file(d + "model.txt")
        m._set_option("hip_stream_weights", 1)
        _run_once(m, cfg.in_name, z, 9)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: not available in streamed-weights mode"):
            m.hip_decode(*names, lat16, 5.48998, img)
        m.close()

        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.set_use_fp16_arithmetic(True)
        m.read_file(d + "model.txt")
        m.add_outputs_convert("something_else")
        _run_once(m, cfg.in_name, z, 9)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the output is excluded from the fp32 conversion"):
            m.hip_decode(*names, lat16, 5.48998, img)
        m.close()

    with tempfile.TemporaryDirectory() as d:      # uint8 arithmetic (the golden uint8 case's ranges: a calibration through the stub would measure nothing)
        d += "/"
        cfg16 = sd_vae.TINY_VAE
        sd_vae.build_vae_decoder(DirSink(d), cfg16, quant_all=True)
        open(d + "range_data.txt", "w", newline="").write(str(np.load(os.path.join(HERE, "golden", "vae_tiny_qu8.npz"))["ranges"]))
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.hip_read_range_data(d + "range_data.txt")
        m.set_use_uint8_arithmetic(True)
        m.read_file(d + "model.txt")
        _run_once(m, cfg16.in_name, sd_vae.vae_inputs(cfg16)[cfg16.in_name], 1)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: not available with uint8 arithmetic"):
            m.hip_decode(cfg16.in_name, "out_image", lat16, 5.48998, img)
        m.close()

    with tempfile.TemporaryDirectory() as d:      # [1, 4, 8, 8] -> an unpadded 3 x 3 convolution -> [1, 3, 6, 6]: 6 is no multiple of 8
        d += "/"
        g = GraphBuilder(DirSink(d))
        out = g.conv("c", g.input("z", (1, 4, 8, 8)), 3, 3, pad=0)
        g.finish()
        assert out.shape == (1, 3, 6, 6)
        m = Model(b.LIB_HOST, 0, "ram+nocache")
        m.mangle_tensor_names = False
        m.set_use_fp16_arithmetic(True)
        m.read_file(d + "model.txt")
        _run_once(m, "z", np.zeros((1, 4, 8, 8), f32), 1)
        with pytest.raises(OnnxStreamError, match="Model::hip_decode: the output's spatial size 6 is not an integer multiple of the tile 8"):
            m.hip_decode("z", out.name, np.zeros((1, 4, 8, 8), f32), 5.48998, np.empty((1, 3, 8, 8), f32))
        m.close()


def test_decode_device_refuses_what_it_cannot_do():
    p = Txt2Img.__new__(Txt2Img)
    p.batched, p.vae = False, None
    with pytest.raises(ValueError, match="valid: f32, u8, both"):
        p.decode_device(np.zeros((1, 4, 8, 8), f32), want="rgb")
    with pytest.raises(RuntimeError, match="needs the HIP backend"):
        p.decode_device(np.zeros((1, 4, 8, 8), f32))
