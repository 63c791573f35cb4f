"""Generate tests/golden/sd_samplers_noise.npz and tests/golden/sdxl_loop_noise.npz: the reference APPLICATION's denoising loop (src/sd.cpp
diffusion_solver + CFGDenoiser_CompVisDenoiser + src/samplers.h) run with each of the one-evaluation samplers that add fresh noise per step
(pipeline.STOCHASTIC: ddpm, ddpm_a, ddim_a, tcd, tcd_a, lcm, dpm++3msde, dpm++3msde_a), one image, one thread.  Python only: the committed shims
tools/ref_sd_samplers.cpp and tools/ref_sdxl_loop.cpp are compiled by the build steps of make_golden_samplers.py and make_golden_sdxl_loop.py, and
before anything is recorded each compile re-derives a committed fixture of the oracle's own build (sd_loop.npz's latents20_micro).

sd_samplers_noise.npz, on the SD 1.5 micro UNet of make_golden_sd_loop.py (CFG 7, seed make_golden_sd_loop.SEED): per sampler S latents_S
[1,4,64,64] float32 and steps_S (20, or the largest count >= 5 that stays finite).
sdxl_loop_noise.npz, on the 12 x 20 micro SDXL UNet of make_golden_sdxl_loop.py (its seed and contexts): latents_<mode>_<sampler>_<steps> for mode
xl (dpm++3msde_a and tcd_a at 5 steps) and mode turbo (all eight at 1 and 4 steps); cases (those keys without the prefix); init and noise [5,1,4,12,20],
the application's initial latent and noise walk; seed."""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden_samplers as mgs  # noqa: E402
import make_golden_sd_loop as sdl  # noqa: E402
import make_golden_sdxl_loop as xll  # noqa: E402
from onnxstream_amd.pipeline import STOCHASTIC  # noqa: E402
from onnxstream_amd.synth.graph import DirSink  # noqa: E402
from oracle import ref as oref  # noqa: E402

OUT_SD = os.path.join(REPO, "tests", "golden", "sd_samplers_noise.npz")
OUT_XL = os.path.join(REPO, "tests", "golden", "sdxl_loop_noise.npz")
XL_STEPS = 5
XL_SAMPLERS = ("dpm++3msde_a", "tcd_a")
TURBO_STEPS = (1, 4)
TWINS = (("ddpm", "ddpm_a"), ("tcd", "tcd_a"), ("dpm++3msde", "dpm++3msde_a"))


def check_distinct(res, keys, what):
    """all latents finite and pairwise distinct"""
    for i, a in enumerate(keys):
        assert np.isfinite(res[a]).all(), (what, a)
        for b in keys[i + 1:]:
            assert not np.array_equal(res[a], res[b]), (what, a, b)


if __name__ == "__main__":
    assert oref.available() and all(os.path.exists(os.path.join(mgs.ORACLE, "_ref", o)) for o in mgs.REF_OBJS), "build the oracle first (build())"
    gold20 = np.load(os.path.join(REPO, "tests", "golden", "sd_loop.npz"))["latents20_micro"]
    with tempfile.TemporaryDirectory() as tmp:
        d = tmp + "/models/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        for sub in ("sdxl_unet_fp16/", "sdxl_unet_anyshape_fp16/"):       # the two directories the application reads (src/sd.cpp:1674-1681)
            xll.build_micro_sdxl_unet(DirSink(d + sub))

        # SD 1.5: each compile reproduces the oracle's -- euler_a through the shim == the committed 20-step fixture of the oracle's own build
        lib = mgs.build_shim(tmp)
        assert np.array_equal(mgs.solve(lib, "euler_a", d, 20), gold20)
        sd = {}
        for name in STOCHASTIC:
            for steps in range(20, 4, -1):
                lat = mgs.solve(lib, name, d, steps)
                if np.isfinite(lat).all():
                    break
            assert np.isfinite(lat).all(), name
            sd["latents_" + name], sd["steps_" + name] = lat, np.asarray(steps)
            print(f"{name:14s} steps {steps:2d}  max|x| {float(np.abs(lat).max()):.4g}  std {float(lat.std()):.4g}")
        check_distinct(sd, ["latents_" + s for s in STOCHASTIC], "sd")
        for plain, anc in TWINS:
            assert not np.array_equal(sd["latents_" + plain], sd["latents_" + anc]), (plain, anc)     # the noise does something

        # SDXL and SDXL Turbo
        xlib = xll.build_shim(tmp)
        assert np.array_equal(xll.solve_sd15(xlib, "euler_a", d, 20), gold20)
        xl, cases = {}, []
        todo = [("xl", s, XL_STEPS) for s in XL_SAMPLERS] + [("turbo", s, n) for n in TURBO_STEPS for s in STOCHASTIC]
        for mode, name, steps in todo:
            lat = xll.solve(xlib, name, d, steps, xl=True, turbo=mode == "turbo")
            case = f"{mode}_{name}_{steps}"
            cases.append(case)
            xl["latents_" + case] = lat
            print(f"{case:26s} max|x| {float(np.abs(lat).max()):.4g}  std {float(lat.std()):.4g}")
        for keys in ([f"latents_xl_{s}_{XL_STEPS}" for s in XL_SAMPLERS], [f"latents_turbo_{s}_4" for s in STOCHASTIC]):
            check_distinct(xl, keys, "sdxl")
        # one Turbo step is first and last step at once: no sampler draws (ddim_a adds its noise times 0), and samplers that share a rule coincide there
        assert all(np.isfinite(xl[f"latents_turbo_{s}_1"]).all() for s in STOCHASTIC)
        init, noise = xll.noise_walk(xlib, xll.SEED, max(XL_STEPS, *TURBO_STEPS))
    np.savez_compressed(OUT_SD, **sd)
    np.savez_compressed(OUT_XL, init=init, noise=noise, seed=np.asarray(xll.SEED), cases=np.asarray(cases), **xl)
    for out in (OUT_SD, OUT_XL):
        print(out, os.path.getsize(out), "bytes")
