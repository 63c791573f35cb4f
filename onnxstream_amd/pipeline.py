"""txt2img harness: the denoising loop + VAE decode of the reference app, host side (reference src/sd.cpp ``diffusion_solver``
:1574-1780, ``CFGDenoiser_CompVisDenoiser`` :1397-1559, Euler-Ancestral ``src/samplers.h`` :1430-1472, ``decoder_solver`` :1174-1256).

It drives ANY library that exports the reference's model_* C API through ``bindings.Model`` -- the HIP backend
(``libonnxstream_amd.so``) or the reference oracle -- which is what makes it a parity harness: same schedule, same CFG
combine (scale 7, hard-coded in the reference), same sampler arithmetic, only the UNet/VAE executor differs.
With the HIP backend the cond and uncond samples are pushed under the same names and run as ONE batch-2 pass
(the reference's ``m_batch``); with the reference library they run back to back, as ``sd.cpp`` does without ``--num``.

Out of scope (host glue of the app): tokenizer, text encoder, PNG writer.  The text context is an input.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, Optional

import numpy as np

from .bindings import Model

f32 = np.float32


def _libm_float_fn(name, nargs=1):
    """The reference app computes its schedule with the C library's FLOAT functions (std::exp / std::log on float: expf / logf, src/sd.cpp:1402,
    :1608).  numpy's float32 exp / log are its own SIMD kernels and differ from glibc's in the last bit for a third of the table
    (sigma[0] = 14.614644 vs 14.614643) -- one ulp of sigma flips f16 roundings of the UNet input and moves a whole pass by 1e-3.  So the
    harness calls the same libm; without one, the correctly rounded value (double function, rounded once) stands in."""
    import ctypes
    import ctypes.util
    import math
    try:
        fn = getattr(ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6"), name + "f")
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float] * nargs
        return lambda *v: f32(fn(*[float(a) for a in v]))
    except (OSError, AttributeError):
        dbl = getattr(math, name)
        return lambda *v: f32(dbl(*[float(a) for a in v]))


expf, logf = _libm_float_fn("exp"), _libm_float_fn("log")
expm1f, sqrtf = _libm_float_fn("expm1"), _libm_float_fn("sqrt")
powf = _libm_float_fn("pow", 2)

# samplers of the reference's --sampler (src/sd.cpp:41-63) that sample() and sample_device() run: the default Euler-Ancestral, Euler, and the
# one-evaluation, noise-free multistep samplers of src/samplers.h (the ORIGINAL_SAMPLER_ALGORITHMS branch); STOCHASTIC below holds eight more
SAMPLERS = ("euler_a", "euler", "dpm++2m", "dpm++2mv2", "ipndm", "ipndm_v", "ipndm_vo", "taylor3", "ddim")
# multistep sampler -> loop form of model_hip_sampler_loop_multistep (exports.cpp)
MULTISTEP = {"dpm++2m": 0, "dpm++2mv2": 0, "ipndm": 1, "ipndm_v": 2, "ipndm_vo": 3, "taylor3": 4, "ddim": 5}
# loop form -> (history depth as src/samplers.h create_buffers, the osg_multistep_form of each order); the table of Plan::sampler_loop_multistep
# (order 2 of loop form 0 is the plain Euler step the reference substitutes on the last step of an SDXL image, src/sd.cpp:1705-1719)
_MS_LOOP = {0: (1, (0, 1, 2)), 1: (4, (2, 3, 5, 6)), 2: (4, (2, 4, 5, 6)), 3: (4, (2, 7, 8, 9)), 4: (3, (2, 10, 11)), 5: (0, (12,))}
# the one-evaluation samplers that add fresh noise per step (src/samplers.h:1039-1223, :1406-1428, :412-541) -> eta, the randomness the reference sets
# for the name (0: the sampler draws nothing; dpm++3msde_a takes 0.5 in Turbo mode, :414-417).  lcm has no eta; it draws on every step but the last.
STOCHASTIC = {"ddpm": 0.0, "ddpm_a": 1.0, "ddim_a": 1.0, "tcd": 0.0, "tcd_a": 0.5, "lcm": 0.0, "dpm++3msde": 0.0, "dpm++3msde_a": 1.0}
# osg_stochastic_form (include/osgpu.h)
ST_LINEAR, ST_DEN, ST_EULER, ST_DDIM_A, ST_TCD, ST_SDE0, ST_SDE1, ST_SDE2 = range(8)
_ST_SDE = (ST_SDE0, ST_SDE1, ST_SDE2)


def _check_sampler(sampler: str) -> None:
    if sampler not in SAMPLERS + tuple(STOCHASTIC):
        raise ValueError(f"unknown sampler {sampler!r}; valid names: {', '.join(SAMPLERS + tuple(STOCHASTIC))}")


# pow(2.f, -p - .5f) with the reference's constexpr p = 0 (src/samplers.h:101-103), stated as the constant the compiler folds it to: the correctly
# rounded float of 2 ** -0.5 (glibc's powf returns the same value at run time)
_RESHAPER_BASE = f32(0.70710677)


def sigma_reshaper(si1, i: int, steps: int, turbo: bool):
    """sigma_reshaper of process_sample (src/samplers.h:97-106): what the non-ancestral samplers read in place of sigma[i + 1] for the Turbo model;
    the identity outside Turbo mode.  Float arithmetic in the reference's expression tree, pow = powf."""
    si1 = f32(si1)
    if not turbo:
        return si1
    e = f32(_RESHAPER_BASE / f32(steps))
    curve = f32(f32(powf(f32(f32(steps - i) / f32(steps)), e) + powf(f32(f32(i + 1) / f32(steps)), e)) / f32(2))
    return f32(si1 * (max(f32(0.0001), curve) if curve else f32(0)))


def sigma_reshaper_sharp(si1, i: int, steps: int, turbo: bool):
    """sigma_reshaper_sharp (src/samplers.h:109-113): the correction of sigma_reshaper scaled by the signed cube root of 3 / (steps - 2.5)."""
    si1 = f32(si1)
    pre = sigma_reshaper(si1, i, steps, turbo)
    if pre == si1:
        return si1
    smooth = f32(f32(3) / f32(f32(steps) - f32(2.5)))
    return f32(si1 + f32(f32(f32(smooth / abs(smooth)) * powf(abs(smooth), f32(f32(1) / f32(3)))) * f32(pre - si1)))


def _per_prompt(v, P: int) -> list:
    """an argument given once per call, or as a list with one entry per prompt -> the list"""
    return list(v) if isinstance(v, (list, tuple)) else [v] * P


def multistep_update(form: int, x: np.ndarray, den: np.ndarray, hist, sigma, k, dk) -> np.ndarray:
    """One step of osg_multistep_form `form` (include/osgpu.h) on the host, in the kernel's operation order: every fp32 operation rounded on its
    own, DDIM in float64 with one rounding at the end.  hist = [h0, h1, h2, h3] (arrays or None); h0 is overwritten.  Returns the new x."""
    k0, k1, k2, k3, k4 = (f32(v) for v in k[:5])
    if form == 12:
        return ((x.astype(np.float64) * float(dk[0])) + (den.astype(np.float64) * float(dk[1]))).astype(f32)
    if form in (0, 1):
        dv = den if form == 0 else (k2 * den) - (k3 * hist[1])
        nx = (k0 * x) - (k1 * dv)
        hist[0][...] = den
        return nx.astype(f32)
    d = (x - den) / f32(sigma)
    h1, h2, h3 = hist[1], hist[2], hist[3]
    if form == 2:
        s = k0 * d
    elif form == 3:
        s = (k0 * ((f32(3) * d) - h1)) / f32(2)
    elif form == 4:
        s = (k0 * ((k1 * d) - (k2 * h1))) / f32(2)
    elif form == 5:
        s = (k0 * (((f32(23) * d) - (f32(16) * h1)) + (f32(5) * h2))) / f32(12)
    elif form == 6:
        s = (k0 * ((((f32(55) * d) - (f32(59) * h1)) + (f32(37) * h2)) - (f32(9) * h3))) / f32(24)
    elif form == 7:
        s = k0 * ((k1 * d) + (k2 * h1))
    elif form == 8:
        s = k0 * (((k1 * d) + (k2 * h1)) + (k3 * h2))
    elif form == 9:
        s = k0 * ((((k1 * d) + (k2 * h1)) + (k3 * h2)) + (k4 * h3))
    elif form == 10:
        d2 = (d - h1) * k1
        s = (k0 * d) + (k2 * d2)
    elif form == 11:
        d2 = (d - h1) * k1
        d3 = (d2 - h2) * k1
        s = ((k0 * d) + (k2 * d2)) + (k3 * d3)
    else:
        raise ValueError(f"unknown multistep form {form}")
    hist[0][...] = d
    return (x + s).astype(f32)


def stochastic_update(form: int, x: np.ndarray, den: np.ndarray, hist, sigma, k, noise) -> np.ndarray:
    """One step of osg_stochastic_form `form` (include/osgpu.h) on the host, in the kernel's operation order: every fp32 operation rounded on its own.
    hist = [h0, h1, h2] (arrays or None); the SDE forms overwrite h0 with den.  k = k0..k6, n0, n1; noise: the step's draw, or None.  Returns the new x."""
    k0, k1, k2, k3, k4, k5, k6, n0, n1 = (f32(v) for v in k[:9])
    sigma = f32(sigma)
    if form == ST_LINEAR:
        nx = (x * k0) + (den * k1)
    elif form == ST_DEN:
        nx = den
    elif form == ST_EULER:
        nx = x + (((x - den) / sigma) * k0)
    elif form == ST_DDIM_A:
        mo = ((k0 + x) - den) / sigma
        po = ((x * k1) - (mo * k2)) / k1
        nx = (k3 * po) + (mo * k4)
    elif form == ST_TCD:
        mo = (x - den) / sigma
        po = x - (k0 * mo)
        nx = (k1 * po) + (k2 * mo)
    elif form in _ST_SDE:
        hist[0][...] = den
        nx = (k0 * x) - (k1 * den)
        if form == ST_SDE1:
            nx = nx + (k3 * ((den - hist[1]) / k2))
        elif form == ST_SDE2:
            d10 = (den - hist[1]) / k2
            d11 = (hist[1] - hist[2]) / k3
            df = d10 - d11
            d1 = d10 + ((df * k2) / k4)
            d2 = df / k4
            nx = nx + ((k5 * d1) - (k6 * d2))
    else:
        raise ValueError(f"unknown stochastic form {form}")
    if noise is not None:
        nx = ((n1 * nx) + (n0 * noise)) if form == ST_TCD else (nx + (noise * n0))
    return nx.astype(f32)


def log_sigmas_table() -> np.ndarray:
    """The 1000-entry table hard-coded at src/sd.cpp:1591: log(sqrt((1-acp)/acp)) of SD's scaled-linear beta schedule
    (beta 0.00085 -> 0.012 over 1000 steps), recomputed the way it was made -- alphas_cumprod in float64, stored as float32, sigma and log
    in float32.  The reference's literals are the float32 results of whatever libm produced them: this recomputation hits 827 of the
    1000 entries exactly and is 1 float32 ulp (<= 2.4e-7) off in the others (tests/test_pipeline.py checks that against the source)."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    acp = np.cumprod(1.0 - betas).astype(f32)
    return np.log(np.sqrt((f32(1) - acp) / acp)).astype(f32)


def sigma_schedule(steps: int, log_sigmas: np.ndarray) -> np.ndarray:
    """t_to_sigma over linspace(999, 0, steps) + a trailing 0 (src/sd.cpp:1597-1612)."""
    sig = np.empty(steps + 1, f32)
    delta = f32(-999.0) / f32(steps - 1) if steps > 1 else f32(0)      # float delta = -999.0f / (step - 1)
    for i in range(steps):
        t = f32(999.0 + float(f32(f32(i) * delta)))                   # float t = 999.0 + i * delta  (float product, double sum, one rounding)
        lo, hi = int(np.floor(t)), int(np.ceil(t))
        w = f32(t - lo)
        sig[i] = expf(f32(f32(f32(1) - w) * log_sigmas[lo]) + f32(w * log_sigmas[hi]))
    sig[steps] = 0.0
    return sig


def sigma_to_t(sigma: float, log_sigmas: np.ndarray) -> float:
    """src/sd.cpp:1403-1425."""
    ls = logf(f32(sigma))
    dists = np.cumsum((ls - log_sigmas >= 0).astype(np.int64))
    low = min(int(np.argmax(dists)), 1000 - 2)
    high = low + 1
    lo, hi = log_sigmas[low], log_sigmas[high]
    w = f32(f32(lo - ls) / f32(lo - hi))                      # float arithmetic throughout, as :1420-1422
    w = max(f32(0), min(f32(1), w))
    return float(f32(f32(f32(1) - w) * f32(low)) + f32(w * f32(high)))


def save_latents(path: str, latents: np.ndarray) -> None:
    """`sd --save-latents FILE` (src/sd.cpp:2325-2327): the first sample's latents as raw little-endian float32, [4, h, w]."""
    np.ascontiguousarray(np.asarray(latents, f32).reshape((-1,) + tuple(np.asarray(latents).shape[-3:]))[0], "<f4").tofile(path)


def load_latents(path: str, h: int = 64, w: int = 64) -> np.ndarray:
    """`sd --decode-latents FILE` (src/sd.cpp:3212-3245): a raw float32 file back as [1, 4, h, w] (the app checks the size against 4*h*w too)."""
    v = np.fromfile(path, "<f4")
    if v.size != 4 * h * w:
        raise ValueError("Invalid size of latents file.")
    return v.reshape(1, 4, h, w).astype(f32)


def tile_origins(n: int, tile: int) -> List[int]:
    """Origins of the decoder tiles along an axis of n latent pixels (sd_tiled_decoder's loop, src/sd.cpp:1328-1340, for any n and tile): 0, step,
    2 * step, ... with step = 3 * tile / 4, and a last one flush with the border -- [0, 24, 32] for (64, 32), [0, 24, 28] for (60, 32), where three
    tiles overlap."""
    if n < tile or tile < 1 or (tile < 2 and n != tile):
        raise ValueError(f"no tiles of {tile} over {n} latent pixels")
    step, o, v = (tile * 3) // 4, [], 0
    while True:
        v = min(v, n - tile)
        o.append(v)
        if v == n - tile:
            return o
        v += step


def blend_fold(tiles: np.ndarray, H: int, W: int, tile: int, up: int) -> np.ndarray:
    """The blend of decode_tiled() stated per OUTPUT PIXEL, as osg_decode_blend computes it (include/osgpu.h): tiles [P*T, C, up*tile, up*tile] (tile k of
    image p = entry p*T + k, raster order) -> image [P, C, up*H, up*W].  Every pixel starts from d = 0 and folds the tiles that cover it in raster order:
    f = qy * qx with qy = ly / ramp where the tile's y origin != 0 and its local row ly < ramp (else 1), qx alike, ramp = 2 * tile * up / 8;
    d = s * f + d * (1 - f); at the end (d + 1) * 127.5.  Every operation is rounded to float32 on its own; f == 1 goes through the same arithmetic."""
    tiles = np.asarray(tiles, f32)
    oy, ox = tile_origins(H, tile), tile_origins(W, tile)
    T, ts, ramp = len(oy) * len(ox), tile * up, 2 * tile * up // 8
    P, C = tiles.shape[0] // T, tiles.shape[1]
    if tiles.shape != (P * T, C, ts, ts):
        raise ValueError(f"blend_fold: {tiles.shape} is not [P * {T}, C, {ts}, {ts}]")
    Y, X = np.arange(H * up)[:, None], np.arange(W * up)[None, :]
    d = np.zeros((P, C, H * up, W * up), f32)
    s = np.zeros_like(d)
    with np.errstate(invalid="ignore", divide="ignore"):     # (inf * 0 is a NaN on the device too; ramp = 0 below 4 output pixels per tile: no ramp)
        for ky, y0 in enumerate(oy):
            ly = Y - y0 * up
            qy = np.where((ky != 0) & (ly < ramp), ly.astype(f32) / f32(ramp), f32(1.0)).astype(f32)
            for kx, x0 in enumerate(ox):
                lx = X - x0 * up
                qx = np.where((kx != 0) & (lx < ramp), lx.astype(f32) / f32(ramp), f32(1.0)).astype(f32)
                f = (qy * qx).astype(f32)
                s[:, :, y0 * up:y0 * up + ts, x0 * up:x0 * up + ts] = tiles[ky * len(ox) + kx::T]
                cover = (ly >= 0) & (ly < ts) & (lx >= 0) & (lx < ts)
                d = np.where(cover, s * f + d * (f32(1.0) - f), d)
        return ((d + f32(1.0)) * f32(127.5)).astype(f32)


def to_pixels(img: np.ndarray) -> np.ndarray:
    """Mat::to_pixels (src/sd.cpp:340-364): float image [..., 3, h, w] -> packed 8-bit RGB [..., h, w, 3], each value min(max((int)v, 0), 255) --
    truncated toward zero, then clamped.  Clamping in float first gives the same for every v whose (int) is defined and settles the rest as
    osg_decode_blend does: +inf -> 255, -inf -> 0, NaN -> 0."""
    v = np.asarray(img, f32)
    v = np.where(np.isnan(v), f32(0.0), np.clip(v, f32(0.0), f32(255.0)))
    return np.ascontiguousarray(np.moveaxis(v.astype(np.int32).astype(np.uint8), -3, -1))


class Txt2Img:
    def __init__(self, library: str, unet_dir: str, vae_dir: Optional[str], batched: bool = True, device: int = 0,
                 names: Dict[str, str] = None, fusion: Optional[int] = None, threads: int = 0, autotune: Optional[bool] = None):
        self.batched = batched
        self.names = dict(timestep="timestep", sample="sample", ctx="encoder_hidden_states", out="out_sample", vae_in="input.1",
                          vae_out="out_image")
        if names:
            self.names.update(names)
        self.log_sigmas = log_sigmas_table()
        self._t_cache: Dict[float, float] = {}
        self.unet = Model(library, threads, "ram+nocache")
        self.vae = Model(library, threads, "ram+nocache") if vae_dir else None
        for m, d in ((self.unet, unet_dir), (self.vae, vae_dir)):
            if m is None:
                continue
            if batched:
                m._set_option("hip_device", device)
                if fusion is not None:
                    m._set_option("hip_fusion_level", fusion)
                if m is self.unet:      # conv2 + conv_shortcut of the channel-changing ResNets as one launch (OSA_FUSE_SHORTCUT=0: A/B runs against the un-fused plan)
                    m._set_option("hip_fuse_shortcut", int(os.environ.get("OSA_FUSE_SHORTCUT", "1") != "0"))
                if autotune is not None:
                    m._set_option("hip_autotune", int(bool(autotune)))
            m.read_file(d + "model.txt")
        self._configured: Dict[int, bool] = {}
        self._dev_ready: Dict[tuple, int] = {}       # sample_device: (model, prompts[, samples per prompt]) -> hip_plans_built() when that plan was captured
        self.last_loop_ms = 0.0
        self._vae_dir = vae_dir
        self._dec_ready = None        # decode_device: (key, upscale factor, plans built) of the decoder plan that is resident and captured
        self.last_decode_ms = 0.0

    def close(self):
        self.unet.close()
        if self.vae:
            self.vae.close()

    def _run(self, m: Model, pushes: List[Dict[str, np.ndarray]], out: str) -> List[np.ndarray]:
        if self.batched:
            for ins in pushes:
                for k, v in ins.items():
                    m.add_tensor(k, v if (v.dtype == f32 and v.flags.c_contiguous) else np.ascontiguousarray(v, f32))
            if not self._configured.get(id(m)):
                m.set_use_fp16_arithmetic(True)
                m.set_fuse_ops_in_attention(True)
                self._configured[id(m)] = True
            m.run()
            res = [m.get_tensor(out, i)[0] for i in range(len(pushes))]
            m.clear_tensors()
            return res
        res = []
        for ins in pushes:            # the reference C API takes fp32 inputs only while fp16 arithmetic is off (see oracle/ref.py)
            m.set_use_fp16_arithmetic(False)
            for k, v in ins.items():
                m.add_tensor(k, np.ascontiguousarray(v, f32))
            m.set_use_fp16_arithmetic(True)
            m.set_fuse_ops_in_attention(True)
            m.run()
            res.append(m.get_tensor(out)[0])
            m.clear_tensors()
        return res

    def denoise(self, x: np.ndarray, sigma: float, cond: np.ndarray, uncond: np.ndarray, guidance: float = 7.0,
                extra_cond=None, extra_uncond=None, turbo: bool = False) -> np.ndarray:
        """CFGDenoiser_CompVisDenoiser: eps-prediction wrapped as a denoiser, then the CFG combine (src/sd.cpp:1397-1559).  extra_cond / extra_uncond:
        SDXL's micro-conditioning (text_embeds [1,1280], time_ids [1,6]; src/sd.cpp:1488-1516) pushed along with each branch -- a dict, or a list
        with one dict per prompt.  turbo: the cond branch alone (:1537-1541), one UNet sample per prompt; uncond is not read."""
        n = self.names
        c_out = f32(-1.0 * sigma)
        c_in = f32(1.0 / np.sqrt(f32(sigma) * f32(sigma) + 1))
        if sigma not in self._t_cache:            # the schedule revisits the same 20 sigmas for every image
            self._t_cache[sigma] = sigma_to_t(sigma, self.log_sigmas)
        t = f32(self._t_cache[sigma])
        xin = (x * c_in).astype(f32)
        B = 1 if turbo else 2
        if xin.shape[0] > 1 and isinstance(cond, (list, tuple)):
            # several prompts at the same step of the schedule (the reference's `--num N` batching, src/sd.cpp:1098-1161): 2N samples
            # pushed under the same names -> ONE batched pass; prompt p = pushes 2p (cond) and 2p+1 (uncond); in Turbo mode N samples, prompt p = push p
            P = xin.shape[0]
            extras = (_per_prompt(extra_cond, P), _per_prompt(extra_uncond, P))
            pushes = []
            for p_i in range(P):
                for br, c in enumerate((cond[p_i],) if turbo else (cond[p_i], uncond[p_i])):
                    pushes.append({n["timestep"]: np.asarray([t], f32), n["sample"]: xin[p_i:p_i + 1], n["ctx"]: c})
                    if extras[br][p_i]:
                        pushes[-1].update(extras[br][p_i])
            eps = self._run(self.unet, pushes, n["out"])
            den_c = np.concatenate(eps[0::B]) * c_out + x
            if turbo:
                return den_c.astype(f32)
            den_u = np.concatenate(eps[1::2]) * c_out + x
            return (den_u + f32(guidance) * (den_c - den_u)).astype(f32)
        pushes = [{n["timestep"]: np.asarray([t], f32), n["sample"]: xin, n["ctx"]: c} for c in ((cond,) if turbo else (cond, uncond))]
        # SDXL micro-conditioning (text_embeds [1,1280], time_ids [1,6]; reference src/sd.cpp:1488-1516) rides along per branch
        for push, extra in zip(pushes, (extra_cond, extra_uncond)):
            if isinstance(extra, (list, tuple)):
                extra = extra[0]
            if extra:
                push.update(extra)
        eps = self._run(self.unet, pushes, n["out"])
        den_c = eps[0] * c_out + x
        if turbo:
            return den_c.astype(f32)
        den_u = eps[1] * c_out + x
        return (den_u + f32(guidance) * (den_c - den_u)).astype(f32)

    @staticmethod
    def ancestral_step_scalars(s_i, s_n):
        """(sigma_up, sigma_down) of one Euler-Ancestral step exactly as the reference's ACTIVE branch computes them -- samplers.h:66
        ships `#define ORIGINAL_SAMPLER_ALGORITHMS 1`, i.e. src/samplers.h:1431-1433, all in float:
            sigma_up   = min(s1, sqrt(s1 * s1 * (s0 * s0 - s1 * s1) / (s0 * s0)));   sigma_down = sqrt(s1 * s1 - sigma_up * sigma_up)"""
        s0, s1 = f32(s_i), f32(s_n)
        with np.errstate(invalid="ignore"):
            sigma_up = min(s1, np.sqrt(f32(f32(f32(s1 * s1) * f32(f32(s0 * s0) - f32(s1 * s1))) / f32(s0 * s0))))
            sigma_down = np.sqrt(f32(f32(s1 * s1) - f32(sigma_up * sigma_up)))
        return f32(sigma_up), f32(sigma_down)

    def sample(self, cond: np.ndarray, uncond: np.ndarray, steps: int = 20, seed: int = 42, latent_shape=(1, 4, 64, 64),
               on_step: Optional[Callable[[int, np.ndarray], None]] = None, init_latent: Optional[np.ndarray] = None,
               step_noise: Optional[Callable[[int], np.ndarray]] = None, sampler: str = "euler_a", extra_cond=None, extra_uncond=None,
               xl: bool = False, turbo: bool = False) -> np.ndarray:
        """diffusion_solver (src/sd.cpp:1574-1780) with the default sampler, Euler Ancestral as the shipped reference runs it
        (src/samplers.h:1431-1449, ORIGINAL_SAMPLER_ALGORITHMS):  x += ((x - d) / sigma_i) * (sigma_down - sigma_i) + r * sigma_up,
        every operation rounded to float on its own.  init_latent: N(0,1) start (default: numpy stream; the reference draws
        randn_4_w_h(seed % 1000), :1595) -- it is scaled by sigma[0] here as :1611-1612 does; step_noise(i): the ancestral noise of step i.
        sampler="euler": the plain Euler step of the same branch (src/samplers.h:116-126): x += (x - d) / sigma_i * (sigma_{i+1} - sigma_i), no noise.
        The multistep samplers of MULTISTEP (DPM++ 2M / 2M v2, iPNDM, iPNDM_v, iPNDM_vo, Taylor3, DDIM) take their per-step scalars from
        multistep_table() and step with multistep_update(), the host restatement of the device kernel; they draw no noise.
        The samplers of STOCHASTIC (DDPM(-a), DDIM-a, TCD(-a), LCM, DPM++ 3M SDE(-a)) take theirs from stochastic_table() and step with
        stochastic_update(); step_noise(i) is asked for on the steps that draw, which are a prefix of the image.
        extra_cond / extra_uncond: SDXL's micro-conditioning, as denoise() takes it.  xl: the reference's `--xl` (the DPM++ pair takes the Euler step on
        the last step, multistep_table()).  turbo: `--turbo` -- implies xl; one UNet sample per prompt and no guidance (uncond may be None), the
        Turbo forms of sigma_reshaper / sigma_reshaper_sharp and of DDIM's prescale, any steps >= 1 (src/sd.cpp:2923)."""
        _check_sampler(sampler)
        xl = xl or turbo
        dn = dict(extra_cond=extra_cond, extra_uncond=extra_uncond, turbo=turbo)
        sig = sigma_schedule(steps, self.log_sigmas)
        rng = np.random.default_rng(seed)     # the reference draws mt19937 normals; any N(0,1) stream is equivalent for the harness
        x0 = rng.standard_normal(latent_shape, dtype=f32) if init_latent is None else np.asarray(init_latent, f32).reshape(latent_shape)
        x = (x0 * f32(sig[0])).astype(f32)
        if sampler in MULTISTEP:
            loop, order, coef, dcoef = self.multistep_table(sig, sampler, xl=xl, turbo=turbo)
            depth, forms = _MS_LOOP[loop]
            ring = [np.zeros(x.shape, f32) for _ in range(depth)]
            for i in range(steps):
                if loop == 5:         # DDIM's prescale_sample (src/samplers.h:27-59), before the denoiser sees x
                    x = (x * coef[i, 5]).astype(f32)
                den = self.denoise(x, float(sig[i]), cond, uncond, **dn)
                hist = [ring[(i - k) % depth] if depth and k <= order[i] else None for k in range(4)]
                x = multistep_update(forms[order[i]], x, den, hist, sig[i], coef[i], dcoef[i])
                if on_step:
                    on_step(i, x)
            return x
        if sampler in STOCHASTIC:
            form, draws, coef = self.stochastic_table(sig, sampler, xl=xl, turbo=turbo)
            depth = 3 if any(f in _ST_SDE for f in form) else 0       # create_buffers, src/samplers.h:14
            ring = [np.zeros(x.shape, f32) for _ in range(depth)]
            for i in range(steps):
                if coef[i, 9] != 1:       # prescale_sample (src/samplers.h:27-59), before the denoiser sees x
                    x = (x * coef[i, 9]).astype(f32)
                den = self.denoise(x, float(sig[i]), cond, uncond, **dn)
                hist = [ring[(i - k) % depth] if depth else None for k in range(3)]
                noise = None
                if draws[i]:
                    noise = rng.standard_normal(latent_shape, dtype=f32) if step_noise is None else np.asarray(step_noise(i), f32).reshape(latent_shape)
                x = stochastic_update(form[i], x, den, hist, sig[i], coef[i], noise)
                if on_step:
                    on_step(i, x)
            return x
        for i in range(steps):
            den = self.denoise(x, float(sig[i]), cond, uncond, **dn)
            if sampler == "euler":
                x = (x + f32(f32(x - den) / f32(sig[i])) * f32(sigma_reshaper(sig[i + 1], i, steps, turbo) - f32(sig[i]))).astype(f32)
                if on_step:
                    on_step(i, x)
                continue
            sigma_up, sigma_down = self.ancestral_step_scalars(sig[i], sig[i + 1])
            noise = rng.standard_normal(latent_shape, dtype=f32) if step_noise is None else np.asarray(step_noise(i), f32).reshape(latent_shape)
            x = (x + f32(f32(x - den) / f32(sig[i])) * f32(sigma_down - f32(sig[i])) + noise * sigma_up).astype(f32)
            if on_step:
                on_step(i, x)
        return x

    def loop_scalars(self, sig: np.ndarray, sampler: str = "euler_a", turbo: bool = False):
        """Per-step fp32 scalars of the loop, computed exactly as denoise()/sample() do: c_in, c_out, t (sigma_to_t), sigma_i, d_sigma =
        sigma_down - sigma_i and sigma_up of the Euler-Ancestral update.  turbo: Euler reads sigma_{i+1} through sigma_reshaper (src/samplers.h:119);
        Euler-Ancestral does not."""
        steps = len(sig) - 1
        c_in, c_out, ts, s_arr, d_sigma, s_up = (np.empty(steps, f32) for _ in range(6))
        for i in range(steps):
            sigma = float(sig[i])
            c_out[i] = f32(-1.0 * sigma)
            c_in[i] = f32(1.0 / np.sqrt(f32(sigma) * f32(sigma) + 1))
            if sigma not in self._t_cache:
                self._t_cache[sigma] = sigma_to_t(sigma, self.log_sigmas)
            ts[i] = f32(self._t_cache[sigma])
            sigma_up, sigma_down = self.ancestral_step_scalars(sig[i], sig[i + 1])
            if sampler == "euler":      # (the Euler step is the ancestral one with sigma_down = sigma_{i+1} and no noise, src/samplers.h:116-126)
                sigma_up, sigma_down = f32(0.0), sigma_reshaper(sig[i + 1], i, steps, turbo)
            s_arr[i] = f32(sig[i])
            d_sigma[i] = f32(sigma_down - f32(sig[i]))
            s_up[i] = sigma_up
        if getattr(self, "batched", False) and getattr(self, "unet", None) is not None:      # the schedule's timesteps: the device loops compute what depends on them alone once per value, ahead of step 0
            self.unet.hip_sampler_schedule(ts)
        return c_in, c_out, ts, s_arr, d_sigma, s_up

    def multistep_table(self, sig: np.ndarray, sampler: str, xl: bool = False, turbo: bool = False):
        """Per-step scalars of a multistep sampler, as the reference's process_sample computes them (src/samplers.h, ORIGINAL_SAMPLER_ALGORITHMS;
        the loop-invariant per-element coefficients hoisted with the same expression tree, every operation rounded to float).  Every sampler reads
        sigma[i + 1] -- and no other sigma -- through a reshaper: sigma_reshaper for DPM++ 2M and the iPNDM family, sigma_reshaper_sharp for DPM++ 2M v2,
        Taylor3 and DDIM; both are the identity unless `turbo`, which also softens DDIM's prescale after the first step (src/samplers.h:50-59).
        xl (implied by turbo): the reference's SDXL rule (src/sd.cpp:1705-1719) -- the DPM++ pair takes the plain Euler step of src/samplers.h:116-126
        on the last step, order 2 of loop form 0, which reads no history.  Returns (loop form, order [steps] int32, coef [steps, 6] float32 = k0..k4 of
        the step's osg_multistep_form and DDIM's prescale factor of x, dcoef [steps, 2] float64 = DDIM's (a, b))."""
        _check_sampler(sampler)
        if sampler not in MULTISTEP:
            raise ValueError(f"{sampler!r} is not a multistep sampler; those are: {', '.join(MULTISTEP)}")
        steps = len(sig) - 1
        order = np.zeros(steps, np.int32)
        coef = np.zeros((steps, 6), f32)
        coef[:, 5] = 1
        dcoef = np.zeros((steps, 2), np.float64)
        one, two = f32(1), f32(2)
        dt_prev = None
        xl = xl or turbo
        reshape = sigma_reshaper_sharp if sampler in ("dpm++2mv2", "taylor3", "ddim") else sigma_reshaper
        for i in range(steps):
            s, s1 = f32(sig[i]), reshape(sig[i + 1], i, steps, turbo)
            sp = f32(sig[i - 1]) if i else None
            if xl and i == steps - 1 and sampler in ("dpm++2m", "dpm++2mv2"):      # the sampler IS Euler for this step: sigma_reshaper, src/samplers.h:119-125
                order[i] = 2
                coef[i, 0] = f32(sigma_reshaper(sig[i + 1], i, steps, turbo) - s)
            elif sampler in ("dpm++2m", "dpm++2mv2"):             # src/samplers.h:339-377, :543-582
                if i == 0 or s1 == 0:
                    with np.errstate(divide="ignore"):
                        coef[i, :2] = f32(s1 / s), expm1f(f32(logf(s1) - logf(s)))       # log(0) = -inf, expm1(-inf) = -1 on the last step
                    continue
                t, t_next = f32(-logf(s)), f32(-logf(s1))
                h = f32(t_next - t)
                h_last = f32(t + logf(sp))
                if sampler == "dpm++2m":
                    b = expm1f(f32(-h))
                    r = f32(h_last / h)
                else:
                    h_min = h if h < h_last else h_last                   # std::min / std::max
                    h_max = h if h_last < h else h_last
                    r = f32(h_max / h_min)
                    b = expm1f(f32(-f32(f32(h_max + h_min) / two)))
                inv = f32(one / f32(two * r))
                order[i] = 1
                coef[i, :4] = f32(s1 / s), b, f32(one + inv), inv
            elif sampler in ("ipndm", "ipndm_v", "ipndm_vo"):          # src/samplers.h:688-940
                h_n = f32(s1 - s)
                o = order[i] = min(i, 3)
                coef[i, 0] = h_n
                if o == 0 or sampler == "ipndm" or (sampler == "ipndm_v" and o >= 2):     # forms that take h_n alone
                    continue
                h_n_1 = f32(s - sp)
                q = f32(h_n / h_n_1)
                if sampler == "ipndm_v":                                  # o == 1
                    coef[i, 1:3] = f32(two + q), q
                    continue
                c1 = f32(f32(two + q) / two)
                c2 = f32(f32(-q) / two)
                if o == 1:
                    coef[i, 1:3] = c1, c2
                    continue
                h_n_2 = f32(f32(sig[i - 1]) - f32(sig[i - 2]))
                hh = f32(h_n + h_n_1)
                temp = f32(f32(one - f32(f32(f32(h_n / f32(f32(3) * hh)) * f32(h_n * hh)) / f32(h_n_1 * f32(h_n_1 + h_n_2)))) / two)
                r12 = f32(one + f32(h_n_1 / h_n_2))
                if o == 2:
                    coef[i, 1:4] = f32(c1 + temp), f32(c2 - f32(r12 * temp)), f32(f32(temp * h_n_1) / h_n_2)
                    continue
                h_n_3 = f32(f32(sig[i - 2]) - f32(sig[i - 3]))
                hhh = f32(hh + h_n_2)
                p = f32(f32(f32(one - f32(h_n / f32(f32(3) * hh))) / two)
                        + f32(f32(f32(one - f32(h_n / f32(two * hh))) * h_n) / f32(f32(6) * hhh)))
                num = f32(f32(h_n * hh) * hhh)
                den = f32(f32(h_n_1 * f32(h_n_1 + h_n_2)) * f32(f32(h_n_1 + h_n_2) + h_n_3))
                temp2 = f32(f32(p * num) / den)
                g = f32(f32(h_n_1 * f32(h_n_1 + h_n_2)) / f32(h_n_2 * f32(h_n_2 + h_n_3)))
                q12 = f32(h_n_1 / h_n_2)
                coef[i, 1] = f32(f32(c1 + temp) + temp2)
                coef[i, 2] = f32(f32(c2 - f32(r12 * temp)) - f32(f32(f32(one + q12) + g) * temp2))
                coef[i, 3] = f32(f32(f32(temp * h_n_1) / h_n_2) + f32(f32(f32(q12 + f32(g * f32(one + f32(h_n_2 / h_n_3))))) * temp2))
                coef[i, 4] = f32(f32(f32(f32(-temp2) * g) * h_n_1) / h_n_2)
            elif sampler == "taylor3":                                    # src/samplers.h:942-987; sampler_history_dt = the previous dt
                dt = f32(s1 - s)
                o = order[i] = min(i, 2)
                coef[i, 0] = dt
                if o:                                                     # (at i = 0 the reference's 1 / dt_prev reads an unset float: unused)
                    dd = f32(dt * dt)
                    coef[i, 1:4] = f32(one / dt_prev), f32(dd / two), f32(f32(dd * dt) / f32(6))
                dt_prev = dt
            else:                                                         # ddim, src/samplers.h:1078-1100 and prescale_sample :27-59
                coef[i, 5] = self._prescale(s, i, steps, turbo)
                sn2 = float(f32(s1 * s1))
                alpha = 1.0 / (sn2 + 1.0)
                a = math.sqrt(1.0 - alpha) / float(s)
                dcoef[i] = a, math.sqrt(alpha) - a
        return MULTISTEP[sampler], order, coef, dcoef

    def stochastic_table(self, sig: np.ndarray, sampler: str, xl: bool = False, turbo: bool = False):
        """Per-step scalars of a sampler of STOCHASTIC, as the reference's process_sample computes them (src/samplers.h, ORIGINAL_SAMPLER_ALGORITHMS): the
        reference's expression tree in float, every operation rounded on its own, libm's float functions; its per-element std::log / std::exp /
        std::sqrt calls act on scalars and are hoisted here.  DDPM and LCM read the raw sigma[i + 1], DDIM-a and TCD sigma_reshaper_sharp, DPM++ 3M SDE
        the doubly averaged sigma_reshaper of :426-432.  xl (implied by turbo): the last step of DPM++ 3M SDE is the plain Euler step (src/sd.cpp:1711-1716).
        Returns (form [steps] int32 = the step's osg_stochastic_form, draws [steps] int32 = 1 where the step adds noise, coef [steps, 10] float32 =
        k0..k6, n0, n1 of the form and the prescale factor of x).  The drawing steps are a prefix of the image: the reference advances its noise seed on
        drawing steps only, so noise i of the application's walk belongs to step i."""
        if sampler not in STOCHASTIC:
            raise ValueError(f"{sampler!r} is not a stochastic sampler; those are: {', '.join(STOCHASTIC)}")
        steps = len(sig) - 1
        form = np.zeros(steps, np.int32)
        draws = np.zeros(steps, np.int32)
        coef = np.zeros((steps, 10), f32)
        coef[:, 8:] = 1
        zero, one, two = f32(0), f32(1), f32(2)
        xl = xl or turbo
        eta = f32(0.5 if sampler == "dpm++3msde_a" and turbo else STOCHASTIC[sampler])
        fmax = lambda a, b: b if a < b else a                             # std::max
        for i in range(steps):
            s, sn = f32(sig[i]), f32(sig[i + 1])
            with np.errstate(divide="ignore", invalid="ignore"):
                if sampler in ("ddpm", "ddpm_a"):                             # src/samplers.h:1039-1076
                    s2, sn2 = f32(s * s), f32(sn * sn)
                    scale_back, d = sqrtf(f32(s2 + one)), sqrtf(f32(sn2 + one))
                    variance = zero if eta <= 0 else f32(f32(f32(f32(eta * sqrtf(f32(s2 - sn2))) / d) * sn) / s)
                    form[i] = ST_LINEAR
                    coef[i, :2] = f32(f32(f32(sn2 / s2) * scale_back) / d), f32(f32(f32(s2 - sn2) / d) / s2)
                    if not variance <= 0:                                     # the reference's branch, :1053
                        draws[i], coef[i, 7] = 1, variance
                elif sampler == "lcm":                                        # :1406-1428
                    form[i] = ST_DEN
                    if sn > 0:
                        draws[i], coef[i, 7] = 1, sn
                elif sampler == "ddim_a":                                     # :1102-1158
                    si1 = sigma_reshaper_sharp(sn, i, steps, turbo)
                    a_t, a_prev = f32(one / f32(f32(s * s) + one)), f32(one / f32(f32(si1 * si1) + one))
                    b_t, b_prev = f32(one - a_t), f32(one - a_prev)
                    variance = f32(f32(b_prev / b_t) * f32(one - f32(a_t / a_prev)))
                    autozero = f32(variance * zero)
                    form[i], draws[i] = ST_DDIM_A, 1
                    coef[i, :5] = autozero, sqrtf(a_t), sqrtf(b_t), sqrtf(a_prev), sqrtf(f32(f32(one - a_prev) - f32(f32(variance * eta) * eta)))
                    coef[i, 7] = f32(eta * sqrtf(fmax(autozero, variance)))
                    coef[i, 9] = self._prescale(s, i, steps, turbo)
                elif sampler in ("tcd", "tcd_a"):                             # :1160-1223
                    si1 = sigma_reshaper_sharp(sn, i, steps, turbo)
                    si4 = f32(si1 * f32(one - eta))
                    si3 = f32(sig[int(f32(f32(f32(steps - i - 1) * eta) + f32(i)) + one)])      # float arithmetic, then truncation (:1174)
                    si2 = sqrtf(f32(sqrtf(f32(si3 * (f32(si3 * f32(si1 / sn)) if sn else si3))) * sqrtf(f32(si4 * sqrtf(f32(si3 * si4))))))
                    a_n, a_s, alpha = f32(one / f32(f32(si1 * si1) + one)), f32(one / f32(f32(si2 * si2) + one)), f32(one / f32(f32(s * s) + one))
                    beta, b_s = f32(one - alpha), f32(one - a_s)
                    form[i] = ST_TCD
                    coef[i, :3] = f32(sqrtf(beta) / sqrtf(alpha)), sqrtf(a_s), sqrtf(b_s)
                    if eta > 0 and i < steps - 1:
                        draws[i] = 1
                        coef[i, 8], coef[i, 7] = sqrtf(f32(a_n / a_s)), sqrtf(fmax(f32(s * zero), f32(one - f32(a_n / a_s))))
                    coef[i, 9] = self._prescale(s, i, steps, turbo)
                elif xl and i == steps - 1:                                   # dpm++3msde(_a): the sampler IS Euler for this step, :119-125
                    form[i] = ST_EULER
                    coef[i, 0] = f32(sigma_reshaper(sn, i, steps, turbo) - s)
                else:                                                         # dpm++3msde(_a), :412-541
                    rs = lambda v, j: sigma_reshaper(v, j, steps, turbo)
                    si1 = rs(sn, i)
                    si1 = f32(f32(si1 + rs(si1, i)) / two)                    # "it seems that single correction is not enough", :430-432
                    if not si1:
                        form[i] = ST_DEN
                        continue
                    h = f32(logf(s) - logf(si1))
                    h_eta = f32(h * f32(eta + one))
                    form[i] = (ST_SDE0, ST_SDE1, ST_SDE2)[min(i, 2)]
                    coef[i, :2] = expf(f32(-h_eta)), expm1f(f32(-h_eta))
                    if i:
                        si0 = rs(s, i - 1)
                        si0 = f32(f32(si0 + rs(si0, i - 1)) / two)
                        r = f32(f32(logf(f32(sig[i - 1])) - logf(si0)) / h)
                        phi_2 = f32(f32(expm1f(f32(-h_eta)) / h_eta) + one)
                        coef[i, 2:4] = r, phi_2
                    if i > 1:
                        sm1 = rs(f32(sig[i - 1]), i - 2)
                        sm1 = f32(f32(sm1 + rs(sm1, i - 2)) / two)
                        r2 = f32(f32(logf(f32(sig[i - 2])) - logf(sm1)) / h)
                        coef[i, 3:7] = r2, f32(r + r2), phi_2, f32(f32(phi_2 / h_eta) - f32(0.5))
                    if eta:
                        draws[i] = 1
                        coef[i, 7] = f32(si1 * sqrtf(fmax(f32(si1 * zero), f32(one - powf(f32(si1 / s), f32(two * eta))))))
        nd = int(draws.sum())
        assert draws[:nd].all() and not draws[nd:].any(), "the drawing steps must be a prefix of the image"
        return form, draws, coef

    @staticmethod
    def _prescale(s, i: int, steps: int, turbo: bool):
        """prescale_sample (src/samplers.h:27-59): the factor DDIM, DDIM-a and TCD scale x by before the denoiser sees it, softened after the first step
        in Turbo mode (:50-59)"""
        one = f32(1)
        root = sqrtf(f32(f32(s * s) + one))
        if turbo and i:                                           # "soften correction for Turbo model": pow(scale, 0.9925f - 2.5f / steps / steps)
            root = powf(root, f32(f32(0.9925) - f32(f32(f32(2.5) / f32(steps)) / f32(steps))))
        return f32(root / s) if i == 0 else root

    def sample_device(self, cond, uncond, steps: int = 20, seed: int = 42, latent_shape=(1, 4, 64, 64), guidance: float = 7.0,
                      init_latent: Optional[np.ndarray] = None, step_noise: Optional[Callable[[int], np.ndarray]] = None,
                      sampler: str = "euler_a", extra_cond=None, extra_uncond=None, xl: bool = False, turbo: bool = False) -> np.ndarray:
        """sample() with the whole loop enqueued on the GPU (HIP backend only): per step a scaling kernel fills the UNet's input staging,
        the captured pass is launched, and one kernel does eps -> denoised, the CFG combine and the Euler-Ancestral update -- no host
        round trip until the last step.  Same schedule, same random stream, same fp32 operation order as sample(): the two agree bit
        for bit.  The multistep samplers (MULTISTEP) run their update kernel (osg_sampler_cfg_multistep) with a history ring on the device, the
        samplers of STOCHASTIC theirs (osg_sampler_cfg_stochastic) with the ring and the pre-drawn noise of the steps that draw.  cond / uncond: one context each, or lists with one entry per prompt (latent_shape[0] prompts).
        extra_cond / extra_uncond, xl, turbo: as sample().  In Turbo mode the pass holds one sample per prompt and the guidance-free kernels
        (osg_sampler_*_single) run; the extras stay resident with the contexts and are refreshed with them when the plan is reused."""
        _check_sampler(sampler)
        if not self.batched:
            raise RuntimeError("sample_device needs the HIP backend (batched=True)")
        xl = xl or turbo
        n, P, B = self.names, latent_shape[0], 1 if turbo else 2
        conds, unconds = _per_prompt(cond, P), _per_prompt(uncond, P)
        extras = (_per_prompt(extra_cond, P), _per_prompt(extra_uncond, P))
        sig = sigma_schedule(steps, self.log_sigmas)
        rng = np.random.default_rng(seed)
        x0 = rng.standard_normal(latent_shape, dtype=f32) if init_latent is None else np.asarray(init_latent, f32).reshape(latent_shape)
        x = np.ascontiguousarray(x0 * f32(sig[0]), f32)
        c_in, c_out, ts, s_arr, d_sigma, s_up = self.loop_scalars(sig, "euler" if sampler in MULTISTEP or sampler in STOCHASTIC else sampler, turbo=turbo)
        if sampler in STOCHASTIC:
            form, draws, coef = self.stochastic_table(sig, sampler, xl=xl, turbo=turbo)
            noise = np.zeros((steps,) + tuple(latent_shape), f32) if draws.any() else None       # rows of the steps that draw nothing stay unread
            for i in np.flatnonzero(draws):
                noise[i] = rng.standard_normal(latent_shape, dtype=f32) if step_noise is None else np.asarray(step_noise(i), f32).reshape(latent_shape)
        elif sampler not in MULTISTEP:
            noise = np.empty((steps,) + tuple(latent_shape), f32)
            for i in range(steps):
                noise[i] = rng.standard_normal(latent_shape, dtype=f32) if step_noise is None else np.asarray(step_noise(i), f32).reshape(latent_shape)
        # a Model keeps one plan: the one of this batch (P prompts, B samples each) is resident iff no other was built since it was captured
        key = (id(self.unet), P) if B == 2 else (id(self.unet), P, B)
        if self._dev_ready.get(key) == self.unet.hip_plans_built():
            for p in range(P):      # plan + captured pass exist: only the contexts (and SDXL's extras) change between images
                for br, c in enumerate((conds[p], unconds[p])[:B]):
                    self.unet.hip_set_input(n["ctx"], B * p + br, c)
                    for name, v in (extras[br][p] or {}).items():
                        self.unet.hip_set_input(name, B * p + br, v)
        else:
            for _ in range(2):      # run() #1 plans and runs eagerly, #2 captures the pass; both leave the contexts resident
                if P > 1:
                    self.denoise(x, float(sig[0]), conds, unconds, guidance, extras[0], extras[1], turbo)
                else:
                    self.denoise(x, float(sig[0]), conds[0], unconds[0], guidance, extras[0][0], extras[1][0], turbo)
            self._dev_ready[key] = self.unet.hip_plans_built()
        io = (n["sample"], n["timestep"], n["out"], x)
        if sampler in MULTISTEP:
            loop, order, coef, dcoef = self.multistep_table(sig, sampler, xl=xl, turbo=turbo)
            if turbo:
                self.last_loop_ms = self.unet.hip_sampler_loop_multistep_single(*io, loop, c_in, c_out, ts, s_arr, order, coef, dcoef)
            else:
                self.last_loop_ms = self.unet.hip_sampler_loop_multistep(*io, loop, c_in, c_out, ts, s_arr, order, coef, dcoef, guidance)
        elif sampler in STOCHASTIC:
            if turbo:
                self.last_loop_ms = self.unet.hip_sampler_loop_stochastic_single(*io, c_in, c_out, ts, s_arr, form, draws, coef, noise)
            else:
                self.last_loop_ms = self.unet.hip_sampler_loop_stochastic(*io, c_in, c_out, ts, s_arr, form, draws, coef, noise, guidance)
        elif turbo:
            self.last_loop_ms = self.unet.hip_sampler_loop_single(*io, noise, c_in, c_out, ts, s_arr, d_sigma, s_up)
        else:
            self.last_loop_ms = self.unet.hip_sampler_loop(*io, noise, c_in, c_out, ts, s_arr, d_sigma, s_up, guidance)
        return x

    def decode(self, latents: np.ndarray, factor: float = 5.48998) -> np.ndarray:
        """decoder_solver: latents * 5.48998 -> VAE decoder -> (y + 1) * 127.5 (src/sd.cpp:1174-1256).  factor: the latent scaling (SDXL: 7.67754,
        src/sd.cpp:2359-2361).  The untiled case of blend_fold(); decode_device() computes the same bits on the device."""
        z = (latents * f32(factor)).astype(f32)
        ys = self._run(self.vae, [{self.names["vae_in"]: z[i:i + 1]} for i in range(z.shape[0])], self.names["vae_out"])
        return ((np.concatenate(ys) + f32(1.0)) * f32(127.5)).astype(f32)

    def decode_tiled(self, latents: np.ndarray, tile: int = 32, names=("latent_sample", "out_image"), factor: float = 5.48998) -> np.ndarray:
        """sd_tiled_decoder (src/sd.cpp:1258-1346): a VAE graph built for `tile` x `tile` latents is run over overlapping tiles
        (origins 0, 0.75*tile, ... and a last one flush with the border: 0/24/32 for 64-wide latents, tile_origins()) and the 8x upscaled tiles are
        blended with linear ramps over the first tile/2 * 8... = 64 output pixels of every non-border edge.  self.vae must be the
        tile-sized decoder.  With the HIP backend all tiles run as ONE batched pass.  factor: the latent scaling (SDXL: 7.67754, src/sd.cpp:2359-2361).
        One image per call.  blend_fold() states the same blend per output pixel; decode_device() computes the same bits on the device."""
        z = (latents * f32(factor)).astype(f32)
        _, _, H, W = z.shape
        ramp = tile * 2                                  # 64 output pixels for tile = 32
        oy, ox = tile_origins(H, tile), tile_origins(W, tile)
        pushes = [{names[0]: np.ascontiguousarray(z[:, :, y:y + tile, x:x + tile])} for y in oy for x in ox]
        outs = self._run(self.vae, pushes, names[1])
        up = outs[0].shape[-1] // tile                   # 8 for the SD decoders
        ramp = ramp * up // 8
        res = np.zeros((1, outs[0].shape[1], H * up, W * up), f32)
        T8 = tile * up
        yy = np.arange(T8, dtype=f32)[:, None]
        xx = np.arange(T8, dtype=f32)[None, :]
        k = 0
        for y in oy:
            for x in ox:
                f = np.ones((T8, T8), f32)
                if y:
                    f = f * np.where(yy < ramp, yy / f32(ramp), f32(1.0))
                if x:
                    f = f * np.where(xx < ramp, xx / f32(ramp), f32(1.0))
                d = res[:, :, y * up:y * up + T8, x * up:x * up + T8]
                res[:, :, y * up:y * up + T8, x * up:x * up + T8] = outs[k] * f + d * (f32(1.0) - f)
                k += 1
        return ((res + f32(1.0)) * f32(127.5)).astype(f32)

    def _declared_shape(self, name: str) -> List[int]:
        """the shape the decoder's model.txt declares for activation `name`: the tile size must be known before a plan exists, and the model_* C API has no
        shape query.  (vae_dir ends with a separator, as everywhere in this class: the constructor reads vae_dir + "model.txt".)"""
        import re
        with open(self._vae_dir + "model.txt") as fh:
            m = re.search(r"[:;]" + re.escape(Model.mangle_name(name)) + r"\(([0-9,]+)\)", fh.read())
        if not m:
            raise ValueError(f"decode_device: {name!r} has no declared shape in {self._vae_dir}model.txt")
        return [int(v) for v in m.group(1).split(",")]

    def decode_device(self, latents: np.ndarray, factor: float = 5.48998, names=None, want: str = "f32", tile: Optional[int] = None):
        """decode() / decode_tiled() with everything but one 16-64 KB upload per image on the GPU (HIP backend only): osg_decode_gather scales the latents
        and cuts the tiles straight into the decoder's input staging, the captured pass runs, osg_decode_blend folds the tiles, applies (y + 1) * 127.5
        and packs the 8-bit pixels; only what `want` names comes back.  latents: [images, 4, H, W]; names: (input, output) of the decoder graph
        (default: this object's vae_in / vae_out; the tiled decoders are fed as ("latent_sample", "out_image")); the tile size is the graph's own
        input size (model.txt) unless `tile` gives it -- equal to H and W it is the untiled decoder.  want: "f32" -> the image decode() / decode_tiled()
        return, bit for bit, [images, 3, u*H, u*W]; "u8" -> to_pixels() of it, [images, u*H, u*W, 3] uint8; "both" -> (image, pixels).
        The first call per (images, H, W) plans and captures with two ordinary batched runs; later calls are one model_hip_decode each."""
        if want not in ("f32", "u8", "both"):
            raise ValueError(f"unknown want {want!r}; valid: f32, u8, both")
        if not self.batched or self.vae is None:
            raise RuntimeError("decode_device needs the HIP backend (batched=True) and a VAE decoder")
        lat = np.ascontiguousarray(latents, f32)
        P, _, H, W = lat.shape
        in_name, out_name = names if names else (self.names["vae_in"], self.names["vae_out"])
        t = int(tile) if tile else self._declared_shape(in_name)[-1]
        oy, ox = tile_origins(H, t), tile_origins(W, t)
        key = (in_name, out_name, P, H, W, t)
        if not self._dec_ready or self._dec_ready[0] != key or self._dec_ready[2] != self.vae.hip_plans_built():
            z = (lat * f32(factor)).astype(f32)
            pushes = [{in_name: np.ascontiguousarray(z[p:p + 1, :, y:y + t, x:x + t])} for p in range(P) for y in oy for x in ox]
            for _ in range(2):          # run() #1 plans and runs eagerly, #2 captures the pass
                outs = self._run(self.vae, pushes, out_name)
            self._dec_ready = (key, outs[0].shape[-1] // t, self.vae.hip_plans_built())
        up = self._dec_ready[1]
        image = np.empty((P, 3, H * up, W * up), f32) if want != "u8" else None
        pixels = np.empty((P, H * up, W * up, 3), np.uint8) if want != "f32" else None
        self.last_decode_ms = self.vae.hip_decode(in_name, out_name, lat, factor, image, pixels)
        return (image, pixels) if want == "both" else image if want == "f32" else pixels

    def txt2img(self, cond: np.ndarray, uncond: np.ndarray, steps: int = 20, seed: int = 42, latent_shape=(1, 4, 64, 64), extra_cond=None,
                extra_uncond=None, xl: bool = False, turbo: bool = False) -> np.ndarray:
        return self.decode(self.sample(cond, uncond, steps, seed, latent_shape, extra_cond=extra_cond, extra_uncond=extra_uncond, xl=xl, turbo=turbo))

    def txt2img_device(self, cond, uncond, steps: int = 20, seed: int = 42, latent_shape=(1, 4, 64, 64), sampler: str = "euler_a",
                       factor: float = 5.48998, names=None, want: str = "f32", tile: Optional[int] = None, extra_cond=None, extra_uncond=None,
                       xl: bool = False, turbo: bool = False):
        """txt2img() on the device: sample_device() then decode_device() -- two host syncs per image batch"""
        lat = self.sample_device(cond, uncond, steps, seed, latent_shape, sampler=sampler, extra_cond=extra_cond, extra_uncond=extra_uncond, xl=xl,
                                 turbo=turbo)
        return self.decode_device(lat, factor, names, want, tile)
