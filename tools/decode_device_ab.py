"""Dev tool (GPU box): latents -> image on the host (Txt2Img.decode / decode_tiled) against the same on the device (Txt2Img.decode_device), A/B inside one process.

Three full-size decoders (synthetic weights, as bench.py builds them): SD_VAE untiled at 64 x 64 latents, its 32-latent form over 64 x 64 (9 tiles) and over
128 x 128 with the SDXL factor (25 tiles).  Per case the host method, decode_device(want="u8") and decode_device(want="f32") ALTERNATE, REPS times each after
a warm-up (all three run the same resident plan and captured pass), on fresh latents per repetition.  Reported: wall ms per decode (median, min .. max) and the
device ms model_hip_decode returns; the images are compared bit for bit on the way.  The condition printed at the end: the device path is no slower than the host
path in any case, and in the 25-tile case faster by more than the spread between repetitions (the larger max - min of the two series compared).

    python tools/decode_device_ab.py [out.txt] [reps]          (default profiles/decode_device_ab.txt, 7 repetitions)
"""
import dataclasses
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from onnxstream_amd import build as b
from onnxstream_amd.pipeline import Txt2Img, to_pixels
from onnxstream_amd.synth import sd_vae
from onnxstream_amd.synth.graph import DirSink

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "decode_device_ab.txt")
REPS = max(int(sys.argv[2]) if len(sys.argv) > 2 else 7, 5)
root = os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth")
L32 = dataclasses.replace(sd_vae.SD_VAE, latent=32, in_name="latent_sample", name="sd_vae_l32")
CASES = [("untiled 64x64 (1 tile)", sd_vae.SD_VAE, 64, 5.48998), ("tiled 64x64 (9 tiles)", L32, 64, 5.48998), ("tiled 128x128 (25 tiles)", L32, 128, 7.67754)]


def synth(cfg):
    d = os.path.join(root, cfg.name) + "/"
    if not os.path.exists(d + ".complete"):
        os.makedirs(d, exist_ok=True)
        sd_vae.build_vae_decoder(DirSink(d), cfg)
        open(d + ".complete", "w").write("ok")
    return d


def stats(v):
    return float(np.median(v)), float(min(v)), float(max(v))


lines = ["# latents -> image: Txt2Img.decode / decode_tiled (host) vs Txt2Img.decode_device (device), alternating in one process",
         f"# wall ms per decode over {REPS} repetitions: median (min .. max); device ms: what model_hip_decode returns (gather + pass + blend), median",
         "# case\tpath\twall_median\twall_min\twall_max\tdevice_ms"]
verdict, ok = [], True
rng = np.random.default_rng(0)
for label, cfg, n, factor in CASES:
    d = synth(cfg)
    names = (cfg.in_name, "out_image")
    p = Txt2Img(b.LIB_HOST, d, d, batched=True, names=dict(vae_in=cfg.in_name))
    host = (lambda lat: p.decode(lat, factor=factor)) if cfg.latent == n else (lambda lat: p.decode_tiled(lat, tile=cfg.latent, names=names, factor=factor))
    lat = rng.standard_normal((1, 4, n, n), dtype=np.float32)
    for _ in range(3):                                   # plan, capture, and one replay of each path
        host(lat)
        p.decode_device(lat, factor, names, "both")
    wall = {"host": [], "device u8": [], "device f32": []}
    dev_ms = {"device u8": [], "device f32": []}
    for rep in range(REPS):
        lat = rng.standard_normal((1, 4, n, n), dtype=np.float32)
        t0 = time.perf_counter()
        want = host(lat)
        t1 = time.perf_counter()
        px = p.decode_device(lat, factor, names, "u8")
        t2 = time.perf_counter()
        dev_ms["device u8"].append(p.last_decode_ms)
        t3 = time.perf_counter()
        img = p.decode_device(lat, factor, names, "f32")
        t4 = time.perf_counter()
        dev_ms["device f32"].append(p.last_decode_ms)
        wall["host"].append((t1 - t0) * 1e3)
        wall["device u8"].append((t2 - t1) * 1e3)
        wall["device f32"].append((t4 - t3) * 1e3)
        if not (np.array_equal(img, want) and np.array_equal(px, to_pixels(want))):
            raise SystemExit(f"{label}: the device image differs from the host image")
    p.close()
    for k, v in wall.items():
        med, lo, hi = stats(v)
        lines.append(f"{label}\t{k}\t{med:.3f}\t{lo:.3f}\t{hi:.3f}\t" + (f"{float(np.median(dev_ms[k])):.3f}" if k in dev_ms else "-"))
    h = stats(wall["host"])
    for k in ("device u8", "device f32"):
        m = stats(wall[k])
        spread = max(h[2] - h[1], m[2] - m[1])
        gain = h[0] - m[0]
        good = gain > spread if n == 128 else gain >= 0
        ok &= good
        verdict.append(f"# {label}: {k} {m[0]:.3f} ms vs host {h[0]:.3f} ms: {gain:+.3f} ms ({h[0] / m[0]:.2f}x), spread between repetitions {spread:.3f} ms -> "
                       + ("OK" if good else "NOT MET") + (" (must exceed the spread)" if n == 128 else " (must not be slower)"))
lines += verdict + ["# condition " + ("met" if ok else "NOT met")]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
sys.exit(0 if ok else 1)
