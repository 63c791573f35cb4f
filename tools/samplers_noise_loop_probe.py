"""Dev tool (GPU): device ms per step of the sampler loop for the samplers that add fresh noise per step, against euler_a as the control.
Full-size SD 1.5 UNet (synthetic weights, as bench.py builds it), 2 prompts, 20 steps; tcd_a, lcm, ddpm_a, dpm++3msde_a and euler_a alternate in ONE
process on one resident plan for ROUNDS rounds, so drift hits all five alike.  Reported: last_loop_ms / steps per sampler (median, min..max) and, for
tcd_a, the wall time per step of the host loop sample() next to its device loop.  The bar is euler_a's own spread in the same run: the update launch is
one of ~277 launches per step.  (The synthetic UNet does not denoise, so some trajectories overflow; the launches and their cost are the same.)
    python tools/samplers_noise_loop_probe.py [out.txt] [rounds]      (tile choices from the cost model: one plan for all five, nothing is tuned)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onnxstream_amd import build as b  # noqa: E402
from onnxstream_amd.pipeline import Txt2Img  # noqa: E402
from onnxstream_amd.synth import sd_unet  # noqa: E402
from onnxstream_amd.synth.graph import DirSink  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "profiles/samplers_noise_device_loop.txt"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
SAMPLERS = ("euler_a", "tcd_a", "lcm", "ddpm_a", "dpm++3msde_a")
HOST = "tcd_a"
STEPS, P = 20, 2
root = os.environ.get("OSA_SYNTH_DIR", "/tmp/onnxstream_amd_synth")
cfg = sd_unet.SD15
ud = os.path.join(root, cfg.name) + "/"
if not os.path.exists(ud + ".complete"):
    os.makedirs(ud, exist_ok=True)
    sd_unet.build_unet(DirSink(ud), cfg)
    open(ud + ".complete", "w").write("ok")

pipe = Txt2Img(b.LIB_HOST, ud, None, batched=True, device=0, autotune=False)
rng = np.random.default_rng(0)
conds = [rng.standard_normal((1, 77, cfg.ctx_dim), dtype=np.float32) for _ in range(P)]
unconds = [rng.standard_normal((1, 77, cfg.ctx_dim), dtype=np.float32) for _ in range(P)]
lat = (P, 4, cfg.latent, cfg.latent)
for s in SAMPLERS:                      # plan, capture, and every update kernel's code object loaded before anything is timed
    pipe.sample_device(conds, unconds, steps=STEPS, seed=1, latent_shape=lat, sampler=s)
dev = {s: [] for s in SAMPLERS}
dev_wall = []
for r in range(ROUNDS):
    for s in SAMPLERS:
        t0 = time.perf_counter()
        pipe.sample_device(conds, unconds, steps=STEPS, seed=2 + r, latent_shape=lat, sampler=s)
        if s == HOST:
            dev_wall.append((time.perf_counter() - t0) * 1e3 / STEPS)
        dev[s].append(pipe.last_loop_ms / STEPS)
host_wall = []
for r in range(3):
    t0 = time.perf_counter()
    pipe.sample(conds, unconds, steps=STEPS, seed=2 + r, latent_shape=lat, sampler=HOST)
    host_wall.append((time.perf_counter() - t0) * 1e3 / STEPS)

fmt = lambda v: f"median {np.median(v):.4f}  min..max {min(v):.4f}..{max(v):.4f}"
lines = [f"# device ms per step of the sampler loop (last_loop_ms / {STEPS}): SD 1.5 UNet full size, {P} prompts (batch {2 * P}), {STEPS} steps, {ROUNDS} rounds,",
         "# the five samplers alternating in one process on one resident plan; tile choices from the cost model (no tuning)"]
for s in SAMPLERS:
    lines.append(f"{s:14s} {fmt(dev[s])}   rounds: " + " ".join(f"{v:.4f}" for v in dev[s]))
e = dev["euler_a"]
lines.append(f"# euler_a's own spread in this run: {max(e) - min(e):.4f} ms; medians minus euler_a's: " +
             "  ".join(f"{s} {np.median(dev[s]) - np.median(e):+.4f}" for s in SAMPLERS[1:]))
lines.append(f"# {HOST}, wall ms per step: sample_device() {fmt(dev_wall)};  sample() (host loop, one round trip per step, 3 images) {fmt(host_wall)}")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
pipe.close()
