"""Generate tests/golden/sd_samplers.npz: the reference APPLICATION's denoising loop (src/sd.cpp diffusion_solver + CFGDenoiser_CompVisDenoiser +
src/samplers.h) run with each of the one-evaluation multistep samplers the device loop supports (pipeline.MULTISTEP), on the micro UNet of
make_golden_sd_loop.py, CFG 7, seed make_golden_sd_loop.SEED, one image, one thread.  The oracle's ref_sd_set_sampler knows euler_a / euler only,
so tools/ref_sd_samplers.cpp (the reference application #included where it lies, sampler chosen by name through its own sampler_name[]) is
compiled here into a temporary directory with oracle/Makefile's CXXFLAGS and linked against the oracle objects build() leaves in oracle/_ref/.

Stored per sampler S: latents_S [1,4,64,64] float32 and steps_S (20, or the largest count >= 5 that stays finite on the micro UNet)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden_sd_loop as sdl  # noqa: E402
from onnxstream_amd.pipeline import MULTISTEP  # noqa: E402
from onnxstream_amd.synth.graph import DirSink  # noqa: E402
from oracle import ref as oref  # noqa: E402

ORACLE = os.path.join(REPO, "oracle")
REF_OBJS = ("onnxstream_ref.o", "exports_ref.o", "xnn_shim.o", "ref_extra.o")     # oracle/_ref/ objects; ref_sd.o is replaced by the shim
OUT = os.path.join(REPO, "tests", "golden", "sd_samplers.npz")


def _make_var(name):
    """a variable of oracle/Makefile as make expands it"""
    out = subprocess.run(["make", "-s", "-C", ORACLE, "--no-print-directory", "--eval", f"print-var: ; @echo $({name})", "print-var"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return out.strip()


def build_shim(tmp):
    cxx, flags, tl = _make_var("CXX"), _make_var("CXXFLAGS").split(), _make_var("TL")
    obj, so = os.path.join(tmp, "ref_sd_samplers.o"), os.path.join(tmp, "libref_sd_samplers.so")
    subprocess.run([cxx] + flags + ["-w", "-c", os.path.join(REPO, "tools", "ref_sd_samplers.cpp"), "-o", obj], check=True)
    objs = [os.path.join(ORACLE, "_ref", o) for o in REF_OBJS]
    subprocess.run([cxx, "-shared", "-o", so, obj] + objs + ["-L" + tl, "-ltorch_cpu", "-lc10", "-Wl,-rpath," + tl, "-lpthread", "-ldl"], check=True)
    lib = ctypes.CDLL(so)
    lib.ref_sd_samplers_solve.restype = ctypes.c_char_p
    lib.ref_sd_samplers_solve.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_void_p] * 3
    return lib


def solve(lib, name, models_dir, steps):
    cond, uncond = sdl.contexts()
    out = np.zeros((1, 4, 64, 64), np.float32)
    err = lib.ref_sd_samplers_solve(name.encode(), models_dir.encode(), sdl.SEED, steps, 1, 1, cond.ctypes.data, uncond.ctypes.data, out.ctypes.data)
    if err:
        raise RuntimeError(err.decode())
    return out


if __name__ == "__main__":
    assert oref.available() and all(os.path.exists(os.path.join(ORACLE, "_ref", o)) for o in REF_OBJS), "build the oracle first (build())"
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        d = tmp + "/models/"
        sdl.build_micro_unet(DirSink(d + "unet_fp16/"))
        # this compile reproduces the oracle's: euler_a through the shim == the committed 20-step fixture of the oracle's own build
        assert np.array_equal(solve(lib, "euler_a", d, 20), np.load(os.path.join(REPO, "tests", "golden", "sd_loop.npz"))["latents20_micro"])
        for name in MULTISTEP:
            for steps in range(20, 4, -1):
                lat = solve(lib, name, d, steps)
                if np.isfinite(lat).all():
                    break
            assert np.isfinite(lat).all(), name
            res["latents_" + name], res["steps_" + name] = lat, np.asarray(steps)
            print(f"{name:10s} steps {steps:2d}  max|x| {float(np.abs(lat).max()):.4g}  std {float(lat.std()):.4g}")
    names = list(MULTISTEP)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(res["latents_" + a], res["latents_" + b]), (a, b)
    np.savez_compressed(OUT, **res)
    print(OUT, os.path.getsize(OUT), "bytes")
