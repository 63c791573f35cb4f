"""Generate tests/golden/sdxl_loop.npz: the reference APPLICATION's denoising loop (src/sd.cpp diffusion_solver + CFGDenoiser_CompVisDenoiser +
src/samplers.h) run through its SDXL branch -- `--xl` (CFG 7, the DPM++ last-step rule) and `--turbo` (one UNet sample per step, the Turbo sigma
reshapers, DDIM's softened prescale, any step count) -- on a micro UNet with the SDXL interface the application pushes, one image, one thread.
tools/ref_sdxl_loop.cpp (the application #included where it lies) is compiled here into a temporary directory with oracle/Makefile's CXXFLAGS and
linked against the oracle objects build() leaves in oracle/_ref/; before anything is recorded the compile re-derives a committed fixture of the
oracle's own build (sd_loop.npz's latents20_micro, the SD 1.5 branch).

Stored: latents_<mode>_<sampler>_<steps> [1,4,12,20] float32 for mode xl (euler_a, dpm++2m, dpm++2mv2 at 5 steps) and mode turbo (every sampler of
pipeline.SAMPLERS at 1 and 4 steps, ddim and dpm++2mv2 at 3 -- where 3 / (steps - 2.5) changes sign); cases (the list of those keys without the
prefix); init [1,4,12,20] and noise [5,1,4,12,20], the application's initial latent and ancestral noise walk for that latent size; seed."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from onnxstream_amd.synth.graph import DirSink, GraphBuilder  # noqa: E402

ORACLE = os.path.join(REPO, "oracle")
REF_OBJS = ("onnxstream_ref.o", "exports_ref.o", "xnn_shim.o", "ref_extra.o")     # oracle/_ref/ objects; ref_sd.o is replaced by the shim
OUT = os.path.join(REPO, "tests", "golden", "sdxl_loop.npz")
# not square: a swapped w / h shows; 4 * 12 * 20 = 960 floats per prompt is no multiple of the sampler kernels' 256-thread block
LAT_H, LAT_W = 12, 20
SEED = 9
XL_STEPS = 5
XL_SAMPLERS = ("euler_a", "dpm++2m", "dpm++2mv2")
TURBO_STEPS = (1, 4)
TURBO_EXTRA = (("ddim", 3), ("dpm++2mv2", 3))
NAMES = dict(time_ids="time_ids", text_embeds="text_embeds")
TIME_IDS = np.asarray([[1024, 1024, 0, 0, 1024, 1024]], np.float32)       # what the application pushes for every image (src/sd.cpp:1481)


def build_micro_sdxl_unet(sink, h=LAT_H, w=LAT_W):
    """make_golden_sd_loop.build_micro_unet's idea with the SDXL interface the application pushes (timestep [1], time_ids [1,6], text_embeds [1,1280],
    sample [1,4,h,w], encoder_hidden_states [1,77,2048] -> [1,4,h,w]): conv3x3(sample) + timestep * a[4,1,1] + mean_tokens(ctx W)[1,4,1,1], plus one
    small term per extra input -- (text_embeds V)[1,4,1,1] and mean(time_ids * b)[1,1,1,1] -- so that a dropped or swapped extra changes the output"""
    g = GraphBuilder(sink, seed=78)
    t = g.input("timestep", (1,))
    ids = g.input("time_ids", (1, 6))
    te = g.input("text_embeds", (1, 1280))
    x = g.input("sample", (1, 4, h, w))
    c = g.input("encoder_hidden_states", (1, 77, 2048))
    y = g.conv("/conv", x, 4, 3, std=0.15)
    a = g.weight("/t.scale", g.randn((4, 1, 1), 1e-4), allow_quant=False)
    y = g.binary("/add_t", "Add", y, g.binary("/mul_t", "Mul", t, a))
    m = g.matmul_w("/ctx/MatMul", c, 4)
    m = g.transpose("/ctx/T", m, (0, 2, 1))
    m = g.op("/ctx/ReduceMean", "ReduceMean", [m], (1, 4, 1), {"axes": "-1", "keepdims": "1"})
    m = g.reshape("/ctx/Reshape", m, (1, 4, 1, 1))
    y = g.binary("/add_ctx", "Add", y, m)
    e = g.matmul_w("/te/MatMul", te, 4, std=0.3 / np.sqrt(1280))
    e = g.reshape("/te/Reshape", e, (1, 4, 1, 1))
    y = g.binary("/add_te", "Add", y, e)
    b = g.weight("/ids.scale", np.abs(g.randn((1, 6), 2e-4)) + np.float32(1e-4), allow_quant=False)
    i = g.binary("/ids/Mul", "Mul", ids, b)
    i = g.op("/ids/ReduceMean", "ReduceMean", [i], (1, 1), {"axes": "-1", "keepdims": "1"})
    i = g.reshape("/ids/Reshape", i, (1, 1, 1, 1))
    g.op("/out", "Add", [y, i], (1, 4, h, w), out_names=["out_sample"])
    g.finish()


def contexts():
    """(embeds, embeds_neg) [77,2048] and (pooled, pooled_neg) [1280]: what the application's two text encoders would hand to diffusion_solver"""
    rng = np.random.default_rng(6)
    emb = rng.standard_normal((2, 77, 2048), dtype=np.float32)
    pooled = rng.standard_normal((2, 1280), dtype=np.float32)
    return emb[0], emb[1], pooled[0], pooled[1]


def extras(pooled):
    """the per-branch extras of Txt2Img.denoise for a pooled embedding"""
    return {NAMES["text_embeds"]: np.ascontiguousarray(pooled, np.float32).reshape(1, 1280), NAMES["time_ids"]: TIME_IDS}


def _make_var(name):
    """a variable of oracle/Makefile as make expands it"""
    out = subprocess.run(["make", "-s", "-C", ORACLE, "--no-print-directory", "--eval", f"print-var: ; @echo $({name})", "print-var"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return out.strip()


def build_shim(tmp):
    cxx, flags, tl = _make_var("CXX"), _make_var("CXXFLAGS").split(), _make_var("TL")
    obj, so = os.path.join(tmp, "ref_sdxl_loop.o"), os.path.join(tmp, "libref_sdxl_loop.so")
    subprocess.run([cxx] + flags + ["-w", "-c", os.path.join(REPO, "tools", "ref_sdxl_loop.cpp"), "-o", obj], check=True)
    objs = [os.path.join(ORACLE, "_ref", o) for o in REF_OBJS]
    subprocess.run([cxx, "-shared", "-o", so, obj] + objs + ["-L" + tl, "-ltorch_cpu", "-lc10", "-Wl,-rpath," + tl, "-lpthread", "-ldl"], check=True)
    lib = ctypes.CDLL(so)
    lib.ref_sdxl_solve.restype = ctypes.c_char_p
    lib.ref_sdxl_solve.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_int] * 4 + [ctypes.c_uint] * 3 + [ctypes.c_void_p] * 5
    lib.ref_sdxl_randn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.ref_sdxl_step_noise_seed.argtypes = [ctypes.c_int]
    lib.ref_sdxl_step_noise_seed.restype = ctypes.c_int
    return lib


def solve(lib, name, models_dir, steps, xl, turbo):
    emb, emb_neg, pooled, pooled_neg = contexts()
    out = np.zeros((1, 4, LAT_H, LAT_W), np.float32)
    err = lib.ref_sdxl_solve(name.encode(), models_dir.encode(), int(xl), int(turbo), SEED, steps, LAT_W, LAT_H, 1, emb.ctypes.data, emb_neg.ctypes.data,
                             pooled.ctypes.data, pooled_neg.ctypes.data, out.ctypes.data)
    if err:
        raise RuntimeError(err.decode())
    return out


def solve_sd15(lib, name, models_dir, steps):
    import make_golden_sd_loop as sdl
    cond, uncond = sdl.contexts()
    out = np.zeros((1, 4, 64, 64), np.float32)
    err = lib.ref_sdxl_solve(name.encode(), models_dir.encode(), 0, 0, sdl.SEED, steps, 64, 64, 1, cond.ctypes.data, uncond.ctypes.data, None, None,
                             out.ctypes.data)
    if err:
        raise RuntimeError(err.decode())
    return out


def noise_walk(lib, seed, steps):
    """initial latent + ancestral noises as diffusion_solver / process_sample draw them for an image started with `seed`"""
    def randn(s):
        out = np.empty((1, 4, LAT_H, LAT_W), np.float32)
        lib.ref_sdxl_randn(s, LAT_W, LAT_H, out.ctypes.data)
        return out
    return randn(seed % 1000), np.stack([randn(lib.ref_sdxl_step_noise_seed(seed + i)) for i in range(steps)])


if __name__ == "__main__":
    import make_golden_sd_loop as sdl
    from onnxstream_amd.pipeline import SAMPLERS
    from oracle import ref as oref
    assert oref.available() and all(os.path.exists(os.path.join(ORACLE, "_ref", o)) for o in REF_OBJS), "build the oracle first (build())"
    res, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        d = tmp + "/models/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        # this compile reproduces the oracle's: euler_a through the shim's SD 1.5 branch == the committed 20-step fixture of the oracle's own build
        assert np.array_equal(solve_sd15(lib, "euler_a", d, 20), np.load(os.path.join(REPO, "tests", "golden", "sd_loop.npz"))["latents20_micro"])
        for sub in ("sdxl_unet_fp16/", "sdxl_unet_anyshape_fp16/"):       # the two directories the application reads (src/sd.cpp:1674-1681)
            build_micro_sdxl_unet(DirSink(d + sub))
        todo = [("xl", s, XL_STEPS) for s in XL_SAMPLERS] + [("turbo", s, n) for n in TURBO_STEPS for s in SAMPLERS] + [("turbo", s, n) for s, n in TURBO_EXTRA]
        for mode, name, steps in todo:
            lat = solve(lib, name, d, steps, xl=True, turbo=mode == "turbo")
            assert np.isfinite(lat).all(), (mode, name, steps)
            case = f"{mode}_{name}_{steps}"
            cases.append(case)
            res["latents_" + case] = lat
            print(f"{case:22s} max|x| {float(np.abs(lat).max()):.4g}  std {float(lat.std()):.4g}")
        # the switches do something: SDXL's last-step rule against plain SD for DPM++ 2M, Turbo against SDXL for the same sampler and step count
        plain = solve(lib, "dpm++2m", d, XL_STEPS, xl=False, turbo=False)
        assert not np.array_equal(plain, res[f"latents_xl_dpm++2m_{XL_STEPS}"])
        assert not np.array_equal(solve(lib, "euler_a", d, XL_STEPS, xl=True, turbo=True), res[f"latents_xl_euler_a_{XL_STEPS}"])
        init, noise = noise_walk(lib, SEED, max(XL_STEPS, *TURBO_STEPS))
    np.savez_compressed(OUT, init=init, noise=noise, seed=np.asarray(SEED), cases=np.asarray(cases), **res)
    print(OUT, os.path.getsize(OUT), "bytes")
