"""ctypes binding over the ``model_*`` C API.

The product library (``onnxstream_amd/libonnxstream_amd.so``) exports the same ``extern "C"`` surface as the
reference's ``src/exports.cpp`` (model_new_2 :62, model_read_file :98, model_add_tensor :169, model_get_tensor :205,
model_run_2 :258, model_set_option :276, ...), so this class -- whose public API mirrors the reference's
``src/bindings.py`` ``Model`` (:62-330) -- drives either library unchanged.  That is the drop-in test: the very same
binding object is pointed at the reference oracle ``.so`` and at ours.

Additions over the reference binding (all optional, feature-probed with ``hasattr`` on the library):
``set_option_uint`` for non-bool options (attention parts), ``get_tensor_any`` for fp16/u8 read-back.
"""
import ctypes
import re
from typing import List

import numpy


class OnnxStreamError(Exception):
    pass


class _GetTensorReturnLayout(ctypes.Structure):
    _fields_ = [("dims_num", ctypes.c_size_t), ("dims", ctypes.c_void_p),
                ("data_num", ctypes.c_size_t), ("data", ctypes.c_void_p)]


_WP_NAMES = ("ram", "nocache", "prefetch", "ram+nocache", "ram+prefetch")


class SampleExt(ctypes.Structure):
    """model_hip_sample_ext (exports.cpp): the penalties, min-p and the token history of the three _ext calls"""
    _fields_ = [("repetition_penalty", ctypes.c_float), ("presence_penalty", ctypes.c_float), ("frequency_penalty", ctypes.c_float), ("min_p", ctypes.c_float),
                ("history", ctypes.POINTER(ctypes.c_longlong)), ("n_history", ctypes.c_longlong)]


def sample_ext(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0, history=None):
    """(SampleExt, the array that backs its history) when one of the five is set, else (None, None): the caller then takes the export without _ext"""
    import numpy as np
    if repetition_penalty == 1.0 and presence_penalty == 0.0 and frequency_penalty == 0.0 and min_p == 0.0 and history is None:
        return None, None
    hist = np.ascontiguousarray(np.asarray([] if history is None else history, np.int64).reshape(-1))
    ext = SampleExt(float(repetition_penalty), float(presence_penalty), float(frequency_penalty), float(min_p),
                    hist.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if hist.size else None, int(hist.size))
    return ext, hist


class Model:
    def __init__(self, library_path: str, threads_count: int = 0, weights_provider_name: str = "prefetch"):
        self._lib = ctypes.CDLL(library_path)
        self._proto()
        self.mangle_tensor_names = True
        if weights_provider_name not in _WP_NAMES:
            raise OnnxStreamError(f"Invalid weights provider name: {weights_provider_name}")
        self._h = self._lib.model_new_2(threads_count, weights_provider_name.encode())
        if not self._h:
            raise OnnxStreamError("Unable to create the native model object")

    def _proto(self):
        L, vp, cp = self._lib, ctypes.c_void_p, ctypes.c_char_p
        L.model_new_2.argtypes = [ctypes.c_int, cp]; L.model_new_2.restype = vp
        L.model_delete.argtypes = [vp]; L.model_delete.restype = None
        L.model_read_file.argtypes = [vp, cp]; L.model_read_file.restype = vp
        L.model_read_string.argtypes = [vp, cp]; L.model_read_string.restype = None
        L.model_run_2.argtypes = [vp]; L.model_run_2.restype = vp
        L.model_add_tensor.argtypes = [vp, cp, cp, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)]
        L.model_add_tensor.restype = vp
        L.model_get_tensor.argtypes = [vp, cp]; L.model_get_tensor.restype = vp
        L.model_get_all_tensor_names.argtypes = [vp]; L.model_get_all_tensor_names.restype = vp
        L.model_clear_tensors.argtypes = [vp]; L.model_clear_tensors.restype = None
        L.model_set_option.argtypes = [vp, cp, ctypes.c_uint]; L.model_set_option.restype = None
        L.model_add_extra_output.argtypes = [vp, cp]; L.model_add_extra_output.restype = None
        L.model_free_buffer.argtypes = [vp]; L.model_free_buffer.restype = None

    # -- lifetime ------------------------------------------------------------------------------
    def close(self):
        if self._h:
            self._lib.model_delete(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def lib(self):
        return self._lib

    def _err(self, p):
        if p:
            msg = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
            self._lib.model_free_buffer(p)
            raise OnnxStreamError(msg)

    # -- model / run ---------------------------------------------------------------------------
    def read_file(self, filename: str):
        self._err(self._lib.model_read_file(self._h, filename.encode()))

    def read_string(self, model_string: str):
        self._lib.model_read_string(self._h, model_string.encode())

    def run(self):
        self._err(self._lib.model_run_2(self._h))

    def _name(self, name):
        return (self.mangle_name(name) if self.mangle_tensor_names else name).encode()

    def add_tensor(self, name: str, data: "numpy.ndarray"):
        if data.dtype == numpy.float32:
            ty = b"float32"
        elif data.dtype == numpy.int64:
            ty = b"int64"
        else:
            raise OnnxStreamError(f"Unsupported data type: {data.dtype}")
        data = numpy.ascontiguousarray(data)
        dims = (ctypes.c_uint * data.ndim)(*data.shape)
        p = self._lib.model_add_tensor(self._h, ty, self._name(name), data.ndim, dims)
        ctypes.memmove(p, data.ctypes.data, data.nbytes)

    def get_tensor(self, name: str, index: int = 0):
        """index > 0: the result for the index-th extra sample pushed under the same input names (backend addition)."""
        if index:
            f = self._lib.model_hip_get_tensor_batch
            f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint]; f.restype = ctypes.c_void_p
            p = f(self._h, self._name(name), index)
        else:
            p = self._lib.model_get_tensor(self._h, self._name(name))
        if not p:
            return None
        r = ctypes.cast(p, ctypes.POINTER(_GetTensorReturnLayout)).contents
        dims = ctypes.cast(r.dims, ctypes.POINTER(ctypes.c_size_t))
        shape = [dims[i] for i in range(r.dims_num)]
        if r.data_num:
            arr = numpy.ctypeslib.as_array(ctypes.cast(r.data, ctypes.POINTER(ctypes.c_float)), shape=(r.data_num,)).copy()
        else:      # (a tensor without elements has no data to point to)
            arr = numpy.zeros(0, numpy.float32)
        self._lib.model_free_buffer(p)
        return arr.reshape(shape), shape

    def get_all_tensor_names(self) -> List[str]:
        p = self._lib.model_get_all_tensor_names(self._h)
        if not p:
            return []
        s = ctypes.cast(p, ctypes.c_char_p).value.decode()
        self._lib.model_free_buffer(p)
        names = s.split("|") if s else []
        return [self.demangle_name(n) for n in names] if self.mangle_tensor_names else names

    def clear_tensors(self):
        self._lib.model_clear_tensors(self._h)

    def add_extra_output(self, name: str):
        self._lib.model_add_extra_output(self._h, self._name(name))

    # -- options -------------------------------------------------------------------------------
    def _set_option(self, name: str, value):
        self._lib.model_set_option(self._h, name.encode(), int(value))

    def set_use_fp16_arithmetic(self, v): self._set_option("use_fp16_arithmetic", bool(v))
    def set_use_uint8_qdq(self, v): self._set_option("use_uint8_qdq", bool(v))
    def set_use_uint8_arithmetic(self, v): self._set_option("use_uint8_arithmetic", bool(v))
    def set_fuse_ops_in_attention(self, v): self._set_option("fuse_ops_in_attention", bool(v))
    def set_force_fp16_storage(self, v): self._set_option("force_fp16_storage", bool(v))
    def set_support_dynamic_shapes(self, v): self._set_option("support_dynamic_shapes", bool(v))
    def set_use_ops_cache(self, v): self._set_option("use_ops_cache", bool(v))
    def set_use_scaled_dp_attn_op(self, v): self._set_option("use_scaled_dp_attn_op", bool(v))
    def set_use_next_op_cache(self, v): self._set_option("use_next_op_cache", bool(v))
    def set_ops_printf(self, v): self._set_option("ops_printf", bool(v))
    def set_ops_times_printf(self, v): self._set_option("ops_times_printf", bool(v))
    def set_use_nchw_convs(self, v): self._set_option("use_nchw_convs", bool(v))

    # -- backend additions of libonnxstream_amd.so (absent from the reference library: feature-probed) -----------------
    def hip_replay(self, n: int, per_launch: bool = False):
        """Relaunch the captured pass n times on the inputs already resident in HBM.  Returns per-launch device ms
        (HIP events) when per_launch, else the mean ms over n back-to-back launches."""
        f = self._lib.model_hip_replay
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]; f.restype = ctypes.c_void_p
        if per_launch:
            buf = (ctypes.c_float * n)()
            self._err(f(self._h, n, buf))
            return list(buf)
        self._err(f(self._h, n, None))
        return self.hip_last_pass_ms()

    def hip_set_input(self, name: str, index: int, data):
        """Overwrite pushed sample `index` of a graph input that is resident from an earlier run() (no pass is executed)."""
        import numpy as np
        f = self._lib.model_hip_set_input
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_float), ctypes.c_ulonglong]
        f.restype = ctypes.c_void_p
        a = np.ascontiguousarray(data, np.float32)
        self._err(f(self._h, self._name(name), index, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size))

    def hip_sampler_schedule(self, t):
        """Name the timestep values the following sampler-loop calls walk: the first of them runs the timestep-only launches of the pass for each value
        ahead of step 0 and keeps the results, so that no step has to (option hip_loop_hoist).  A value the loops meet without having been named here is
        computed at its step and kept the same way."""
        import numpy as np
        f = self._lib.model_hip_sampler_schedule
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_ulonglong]; f.restype = ctypes.c_void_p
        a = np.ascontiguousarray(t, np.float32).ravel()
        self._err(f(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size))

    def hip_loop_hoist_stats(self) -> dict:
        """What the sampler loops of the current plan leave out of the step (all 0 before the first loop call, and with hip_loop_hoist off): launches of the
        per-step graph, hoisted prompt-only (p_steps) and timestep-only (t_steps) plan steps, device bytes added, timestep-table hits / misses of the last
        loop call, the input epoch and the filled table rows."""
        f = self._lib.model_hip_loop_hoist_stats
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]; f.restype = None
        out = (ctypes.c_ulonglong * 8)()
        f(self._h, out)
        return dict(zip(("step_launches", "p_steps", "t_steps", "extra_bytes", "t_hits", "t_misses", "epoch", "rows"), (int(v) for v in out)))

    def hip_loop_hoist_info(self) -> str:
        """The hoisted steps, the values they write and the table state of the current plan, as text (Plan::hoist_info)."""
        f = self._lib.model_hip_loop_hoist_info
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_void_p
        p = f(self._h)
        text = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        self._lib.model_free_buffer(p)
        if text.startswith("ERROR: "):
            raise OnnxStreamError(text[7:])
        return text

    # the three device sampler loops: one marshalling helper per family; guidance None = the *_single export, which has no such argument
    def _sampler_loop(self, fname: str, sample: str, timestep: str, out: str, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, guidance, clip):
        import numpy as np
        f = getattr(self._lib, "model_" + fname)
        fp = ctypes.POINTER(ctypes.c_float)
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, fp, fp, fp] + \
                     ([ctypes.c_float] if guidance is not None else []) + [fp, ctypes.POINTER(ctypes.c_double)]
        f.restype = ctypes.c_void_p
        assert x.dtype == np.float32 and x.flags.c_contiguous
        arrs = [np.ascontiguousarray(a, np.float32) for a in (c_in, c_out, t, sigma, d_sigma, sigma_up)]
        steps = len(arrs[0])
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float32)
            assert noise.size == steps * x.size
        if clip is not None:
            clip = np.ascontiguousarray(clip, np.float32)
            assert clip.size == steps
        ms = ctypes.c_double(0)
        self._err(f(self._h, self._name(sample), self._name(timestep), self._name(out), steps, x.shape[0], x.ctypes.data_as(fp),
                    noise.ctypes.data_as(fp) if noise is not None else None, *[a.ctypes.data_as(fp) for a in arrs],
                    *([guidance] if guidance is not None else []), clip.ctypes.data_as(fp) if clip is not None else None, ctypes.byref(ms)))
        return ms.value

    def hip_sampler_loop(self, sample: str, timestep: str, out: str, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, guidance: float = 7.0, clip=None) -> float:
        """The denoising loop (CFG combine + Euler-Ancestral update) enqueued on the device, one host sync at the end.
        x: float32 [prompts, ...] (updated IN PLACE); noise: float32 [steps, prompts, ...] or None; the per-step scalar arrays have
        `steps` float32 entries.  The plan must have been built by a run() with 2*prompts pushes.  Returns the loop's device ms."""
        return self._sampler_loop("hip_sampler_loop", sample, timestep, out, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, guidance, clip)

    def hip_sampler_loop_single(self, sample: str, timestep: str, out: str, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, clip=None) -> float:
        """hip_sampler_loop for a plan built by a run() with `prompts` pushes, ONE UNet sample per prompt (SDXL Turbo, src/sd.cpp:1537-1541):
        den = eps*c_out + x, no guidance pair.  The arguments of hip_sampler_loop without `guidance`."""
        return self._sampler_loop("hip_sampler_loop_single", sample, timestep, out, x, noise, c_in, c_out, t, sigma, d_sigma, sigma_up, None, clip)

    def _sampler_loop_multistep(self, fname: str, sample: str, timestep: str, out: str, x, sampler, c_in, c_out, t, sigma, order, coef, dcoef, guidance):
        import numpy as np
        f = getattr(self._lib, "model_" + fname)
        fp, dp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, ip,
                      fp, ctypes.c_ulonglong, dp, ctypes.c_ulonglong] + ([ctypes.c_float] if guidance is not None else []) + [ctypes.POINTER(ctypes.c_double)]
        f.restype = ctypes.c_void_p
        assert x.dtype == np.float32 and x.flags.c_contiguous
        arrs = [np.ascontiguousarray(a, np.float32) for a in (c_in, c_out, t, sigma)]
        steps = len(arrs[0])
        if any(len(a) != steps for a in arrs) or len(order) != steps:
            raise OnnxStreamError(f"{fname}: c_in, c_out, t, sigma and order need one entry per step")
        order = np.ascontiguousarray(order, np.int32)
        coef = np.ascontiguousarray(coef, np.float32)
        dcoef = np.ascontiguousarray(dcoef, np.float64)
        ms = ctypes.c_double(0)
        self._err(f(self._h, self._name(sample), self._name(timestep), self._name(out), steps, x.shape[0], int(sampler), x.ctypes.data_as(fp),
                    *[a.ctypes.data_as(fp) for a in arrs], order.ctypes.data_as(ip), coef.ctypes.data_as(fp), coef.size, dcoef.ctypes.data_as(dp),
                    dcoef.size, *([guidance] if guidance is not None else []), ctypes.byref(ms)))
        return ms.value

    def hip_sampler_loop_multistep(self, sample: str, timestep: str, out: str, x, sampler: int, c_in, c_out, t, sigma, order, coef, dcoef,
                                   guidance: float = 7.0) -> float:
        """The denoising loop with a one-evaluation multistep sampler (DPM++ 2M / 2M v2, iPNDM, iPNDM_v, iPNDM_vo, Taylor3, DDIM) on the device,
        one host sync at the end.  sampler: the loop form of model_hip_sampler_loop_multistep (pipeline.Txt2Img.multistep_table makes it and the
        tables); c_in, c_out, t, sigma: `steps` float32 entries; order: `steps` ints; coef: float32 [steps, 6]; dcoef: float64 [steps, 2].
        x: float32 [prompts, ...], updated IN PLACE.  Returns the loop's device ms."""
        return self._sampler_loop_multistep("hip_sampler_loop_multistep", sample, timestep, out, x, sampler, c_in, c_out, t, sigma, order, coef, dcoef,
                                            guidance)

    def hip_sampler_loop_multistep_single(self, sample: str, timestep: str, out: str, x, sampler: int, c_in, c_out, t, sigma, order, coef, dcoef) -> float:
        """hip_sampler_loop_multistep for a plan with ONE UNet sample per prompt (see hip_sampler_loop_single): the same arguments without `guidance`."""
        return self._sampler_loop_multistep("hip_sampler_loop_multistep_single", sample, timestep, out, x, sampler, c_in, c_out, t, sigma, order, coef,
                                            dcoef, None)

    def _sampler_loop_stochastic(self, fname: str, sample: str, timestep: str, out: str, x, c_in, c_out, t, sigma, form, draws, coef, noise, guidance):
        import numpy as np
        f = getattr(self._lib, "model_" + fname)
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, fp, fp, fp, fp, fp, ip, ip, fp,
                      ctypes.c_ulonglong, fp] + ([ctypes.c_float] if guidance is not None else []) + [ctypes.POINTER(ctypes.c_double)]
        f.restype = ctypes.c_void_p
        assert x.dtype == np.float32 and x.flags.c_contiguous
        arrs = [np.ascontiguousarray(a, np.float32) for a in (c_in, c_out, t, sigma)]
        steps = len(arrs[0])
        if any(len(a) != steps for a in arrs) or len(form) != steps or len(draws) != steps:
            raise OnnxStreamError(f"{fname}: c_in, c_out, t, sigma, form and draws need one entry per step")
        form, draws = np.ascontiguousarray(form, np.int32), np.ascontiguousarray(draws, np.int32)
        coef = np.ascontiguousarray(coef, np.float32)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float32)
            if noise.size != steps * x.size:
                raise OnnxStreamError(f"{fname}: noise must hold steps * x.size floats")
        ms = ctypes.c_double(0)
        self._err(f(self._h, self._name(sample), self._name(timestep), self._name(out), steps, x.shape[0], x.ctypes.data_as(fp),
                    *[a.ctypes.data_as(fp) for a in arrs], form.ctypes.data_as(ip), draws.ctypes.data_as(ip), coef.ctypes.data_as(fp), coef.size,
                    noise.ctypes.data_as(fp) if noise is not None else None, *([guidance] if guidance is not None else []), ctypes.byref(ms)))
        return ms.value

    def hip_sampler_loop_stochastic(self, sample: str, timestep: str, out: str, x, c_in, c_out, t, sigma, form, draws, coef, noise=None,
                                    guidance: float = 7.0) -> float:
        """The denoising loop with a one-evaluation sampler that adds fresh noise per step (DDPM(-a), DDIM-a, TCD(-a), LCM, DPM++ 3M SDE(-a)) on the
        device, one host sync at the end.  c_in, c_out, t, sigma: `steps` float32 entries; form: `steps` ints (osg_stochastic_form); draws: `steps`
        ints, != 0 where the step adds noise; coef: float32 [steps, 10] (pipeline.Txt2Img.stochastic_table makes the three); noise: float32
        [steps, prompts, ...] or None when no step draws.  x: float32 [prompts, ...], updated IN PLACE.  Returns the loop's device ms."""
        return self._sampler_loop_stochastic("hip_sampler_loop_stochastic", sample, timestep, out, x, c_in, c_out, t, sigma, form, draws, coef, noise,
                                             float(guidance))

    def hip_sampler_loop_stochastic_single(self, sample: str, timestep: str, out: str, x, c_in, c_out, t, sigma, form, draws, coef, noise=None) -> float:
        """hip_sampler_loop_stochastic for a plan with ONE UNet sample per prompt (see hip_sampler_loop_single): the same arguments without `guidance`."""
        return self._sampler_loop_stochastic("hip_sampler_loop_stochastic_single", sample, timestep, out, x, c_in, c_out, t, sigma, form, draws, coef,
                                             noise, None)

    def hip_decode(self, in_name: str, out_name: str, latents, factor: float, image=None, pixels=None) -> float:
        """Latents -> image on the device (model_hip_decode): the latents are uploaded, scaled by `factor` and cut into the decoder's tiles, the
        resident pass runs, the tiles are blended and (y + 1) * 127.5 applied -- one call, one host sync.  latents: float32 [images, 4, h, w].
        image: a C-contiguous float32 array [images, 3, u*h, u*w] to fill, or None; pixels: a C-contiguous uint8 array [images, u*h, u*w, 3] to
        fill, or None (what is None is neither made nor downloaded); a buffer of another size than the decode writes is refused.  The tile size and u are those of the resident plan, which must have been
        built by a run() with images * tiles pushes (pipeline.Txt2Img.decode_device does all of this).  Returns the device ms."""
        import numpy as np
        f = self._lib.model_hip_decode
        fp = ctypes.POINTER(ctypes.c_float)
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, fp, fp,
                      ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ubyte), ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_double)]
        f.restype = ctypes.c_void_p
        lat = np.ascontiguousarray(latents, np.float32)
        if lat.ndim != 4 or lat.shape[1] != 4:
            raise OnnxStreamError("hip_decode: latents must be [images, 4, h, w]")
        P, _, h, w = lat.shape
        for a, dt, what in ((image, np.float32, "image"), (pixels, np.uint8, "pixels")):      # (the library checks the sizes: u is the plan's to know)
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable):
                raise OnnxStreamError(f"hip_decode: {what} must be a writeable C-contiguous {np.dtype(dt).name} array of images * 3 * (u*h) * (u*w) elements")
        ms = ctypes.c_double(0)
        self._err(f(self._h, self._name(in_name), self._name(out_name), P, h, w, float(factor), lat.ctypes.data_as(fp),
                    image.ctypes.data_as(fp) if image is not None else None, image.size if image is not None else 0,
                    pixels.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if pixels is not None else None, pixels.size if pixels is not None else 0,
                    ctypes.byref(ms)))
        return ms.value

    def generate(self, max_new: int, n_caches: int, eos_id: int = -1, sync_every: int = 0, trace: bool = False, ids: str = "input_ids",
                 pos: str = "position_ids", mask: str = "attention_mask", logits: str = "logits", cache_in: str = "pkv", cache_out: str = "opkv",
                 temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, draw_base: int = 0, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, min_p: float = 0.0, history=None):
        """The LLM app's greedy token loop on the device (model_hip_generate): after a run() over the prompt has left `logits` (fp32) and the caches
        `cache_out`<i> (fp16, i < n_caches) in the Model, up to max_new tokens are picked (the app's argmax) and run through the resident T = 1 plan
        without a host round trip per token; the caches and the last logits are left as the host loop would leave them.  Returns
        (tokens int64 [n_tokens], stop, trace float32 [n_tokens, V] or None, device ms); stop: 0 budget spent, 1 eos_id picked, 2 invalid argmax.
        sync_every > 0: the stop code is read after every sync_every passes and the call ends early.
        temperature > 0 samples instead (model_hip_generate_sampled; the rule is stated in include/osgpu.h at osg_decode_sample): logits / temperature,
        the top_k largest (0 = off), the shortest prefix holding top_p of the mass (1 = off), a Philox draw keyed by the 64-bit `seed` at draw index
        draw_base + n_tokens; stop 2 then means a row without a finite maximum.  temperature == 0 is the greedy call, whatever the other four say.
        repetition_penalty (1 = off), presence_penalty, frequency_penalty (0 = off), min_p (0 = off; needs temperature > 0) and `history` (tokens the
        penalties count from the start; None = nothing, the prompt went through run() and is not known here) take the call through
        model_hip_generate_sampled_ext (steps 0 and 3b of the rule in include/osgpu.h); with temperature == 0 the pick then runs over the penalized
        logits.  The trace keeps the raw logits.  With all five at their defaults the call is the one it always was."""
        import numpy as np
        cp, ip = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)
        argtypes = [ctypes.c_void_p, cp, cp, cp, cp, cp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ip, ip,
                    ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
        rule = ()
        ext, _hist = sample_ext(repetition_penalty, presence_penalty, frequency_penalty, min_p, history)
        if temperature == 0 and ext is None:
            f = self._lib.model_hip_generate
        else:
            f = self._lib.model_hip_generate_sampled if ext is None else self._lib.model_hip_generate_sampled_ext
            argtypes += [ctypes.c_float, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_ulonglong]
            rule = (float(temperature), int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), int(draw_base) & (2 ** 64 - 1))
            if ext is not None:
                argtypes += [ctypes.POINTER(SampleExt)]
                rule += (ctypes.byref(ext),)
        f.argtypes = argtypes
        f.restype = ctypes.c_void_p
        toks = np.zeros(max(int(max_new), 1), np.int64)
        tr = None
        if trace:
            got = self.get_tensor(logits)          # (a copy: the Model keeps its tensor)
            if got is None:
                raise OnnxStreamError("Model::hip_generate: tensor not found: " + logits)
            tr = np.zeros((max(int(max_new), 1), got[1][-1]), np.float32)
        n, stop, ms = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
        self._err(f(self._h, self._name(ids), self._name(pos), self._name(mask), self._name(logits), self._name(cache_in), self._name(cache_out), int(n_caches),
                    int(max_new), int(eos_id), int(sync_every), toks.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ctypes.byref(n), ctypes.byref(stop),
                    tr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tr is not None else None, ctypes.byref(ms), *rule))
        return toks[:n.value].copy(), stop.value, (tr[:n.value].copy() if tr is not None else None), ms.value

    def generate_batch(self, n_seq: int, max_new: int, n_caches: int, seeds, temperature: float, top_k: int = 0, top_p: float = 1.0, draw_base: int = 0,
                       eos_id: int = -1, sync_every: int = 0, trace: bool = False, ids: str = "input_ids", pos: str = "position_ids",
                       mask: str = "attention_mask", logits: str = "logits", cache_in: str = "pkv", cache_out: str = "opkv", repetition_penalty: float = 1.0,
                       presence_penalty: float = 0.0, frequency_penalty: float = 0.0, min_p: float = 0.0, history=None):
        """n_seq sampled continuations of the one prompt in one call (model_hip_generate_batch): sequence s is `generate` with seed = seeds[s], on caches and
        a state of its own, and all of them share every pass of a decode plan of batch n_seq.  A sequence that stops, stops alone.  The Model's tensors are
        left as they were.  seeds: n_seq 64-bit integers (None: the call is refused).  Returns (tokens: list of n_seq int64 arrays [n_tokens[s]],
        stop int32 [n_seq], traces: list of n_seq float32 arrays [n_tokens[s], V] or None, device ms).
        repetition_penalty, presence_penalty, frequency_penalty, min_p, history: as `generate` (model_hip_generate_batch_ext); every sequence starts
        from the same history and counts its own tokens from there."""
        import numpy as np
        cp, ip = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)
        ext, _hist = sample_ext(repetition_penalty, presence_penalty, frequency_penalty, min_p, history)
        f = self._lib.model_hip_generate_batch if ext is None else self._lib.model_hip_generate_batch_ext
        f.argtypes = [ctypes.c_void_p, cp, cp, cp, cp, cp, cp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                      ctypes.POINTER(ctypes.c_longlong), ip, ip, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.c_float,
                      ctypes.c_longlong, ctypes.c_float, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_ulonglong] + ([ctypes.POINTER(SampleExt)] if ext is not None else [])
        f.restype = ctypes.c_void_p
        ns, mn = max(int(n_seq), 1), max(int(max_new), 1)
        sd = None
        if seeds is not None:
            sd = np.array([int(x) & (2 ** 64 - 1) for x in seeds], np.uint64)
            if int(n_seq) >= 1 and sd.size != ns:
                raise OnnxStreamError("Model::hip_generate_batch: one seed per sequence is needed.")
        toks = np.zeros((ns, mn), np.int64)
        tr = None
        if trace:
            got = self.get_tensor(logits)
            if got is None:
                raise OnnxStreamError("Model::hip_generate_batch: tensor not found: " + logits)
            tr = np.zeros((ns, mn, got[1][-1]), np.float32)
        n, stop, ms = np.zeros(ns, np.int32), np.zeros(ns, np.int32), ctypes.c_double(0)
        self._err(f(self._h, self._name(ids), self._name(pos), self._name(mask), self._name(logits), self._name(cache_in), self._name(cache_out), int(n_caches),
                    int(n_seq), int(max_new), int(eos_id), int(sync_every), toks.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), n.ctypes.data_as(ip),
                    stop.ctypes.data_as(ip), tr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tr is not None else None, ctypes.byref(ms),
                    float(temperature), int(top_k), float(top_p), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)) if sd is not None else None,
                    int(draw_base) & (2 ** 64 - 1), *([ctypes.byref(ext)] if ext is not None else [])))
        return ([toks[s, :n[s]].copy() for s in range(ns)], stop, [tr[s, :n[s]].copy() for s in range(ns)] if tr is not None else None, ms.value)

    def turn(self, prompt, max_new: int, n_caches: int, chunk: int = 32, capacity: int = 0, eos_id: int = -1, sync_every: int = 0, trace: bool = False,
             vocab: int = 0, ids: str = "input_ids", pos: str = "position_ids", mask: str = "attention_mask", logits: str = "logits", cache_in: str = "pkv",
             cache_out: str = "opkv", temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, draw_base: int = 0,
             repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0, min_p: float = 0.0, history=None):
        """One chat turn on the device (model_hip_turn): the prompt's tokens run in chunks of `chunk` rows over the conversation's caches (`cache_out`<i> as
        a run() or a turn left them, else `cache_in`<i> as pushed -- zero rows on the first turn), then up to max_new tokens are picked and run as `generate`
        does, the first from the prefill's own last logits row; nothing comes back to the host in between.  Leaves the caches of P + len(prompt) + n_tokens
        rows and `logits` [1, 1, V] of the last pass that ran.  capacity > 0 asks for capacity buffers of at least that many rows, so that later turns
        rebuild no plan.  trace needs `vocab` (the width of a logits row) unless a logits tensor is in the Model.  Returns what `generate` returns:
        (tokens, stop, trace or None, device ms of the whole turn).
        repetition_penalty, presence_penalty, frequency_penalty, min_p: as `generate` (model_hip_turn_ext).  history: the tokens the penalties count from
        the start; None = this turn's prompt (the export itself adds nothing: an earlier turn's tokens count only when the caller passes them)."""
        import numpy as np
        cp, ip = ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)
        pr = np.ascontiguousarray(np.asarray(prompt, np.int64).reshape(-1))
        ext, _hist = sample_ext(repetition_penalty, presence_penalty, frequency_penalty, min_p, history)
        if ext is not None and history is None:
            ext, _hist = sample_ext(repetition_penalty, presence_penalty, frequency_penalty, min_p, pr)
        f = self._lib.model_hip_turn if ext is None else self._lib.model_hip_turn_ext
        f.argtypes = [ctypes.c_void_p, cp, cp, cp, cp, cp, cp, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                      ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ip, ip, ctypes.POINTER(ctypes.c_float),
                      ctypes.POINTER(ctypes.c_double), ctypes.c_float, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_ulonglong] + (
                          [ctypes.POINTER(SampleExt)] if ext is not None else [])
        f.restype = ctypes.c_void_p
        toks = np.zeros(max(int(max_new), 1), np.int64)
        tr = None
        if trace:
            width = int(vocab)
            if width <= 0:
                got = self.get_tensor(logits)
                if got is None:
                    raise OnnxStreamError("Model::hip_turn: a logits trace needs `vocab` while no tensor '" + logits + "' is in the Model.")
                width = got[1][-1]
            tr = np.zeros((max(int(max_new), 1), width), np.float32)
        n, stop, ms = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
        self._err(f(self._h, self._name(ids), self._name(pos), self._name(mask), self._name(logits), self._name(cache_in), self._name(cache_out), int(n_caches),
                    pr.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if pr.size else None, int(pr.size), int(chunk), int(capacity), int(max_new), int(eos_id),
                    int(sync_every), toks.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ctypes.byref(n), ctypes.byref(stop),
                    tr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tr is not None else None, ctypes.byref(ms), float(temperature), int(top_k), float(top_p),
                    int(seed) & (2 ** 64 - 1), int(draw_base) & (2 ** 64 - 1), *([ctypes.byref(ext)] if ext is not None else [])))
        return toks[:n.value].copy(), stop.value, (tr[:n.value].copy() if tr is not None else None), ms.value

    def hip_prefill_plan_info(self) -> str:
        """The chunk plan `turn` built, as hip_plan_info gives a plan; its first line is "prefill chunk <C> capacity <rows>"."""
        f = self._lib.model_hip_prefill_plan_info
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_void_p
        p = f(self._h)
        text = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        self._lib.model_free_buffer(p)
        if text.startswith("ERROR: "):
            raise OnnxStreamError(text[7:])
        return text

    def get_tensor_f16(self, name: str):
        """The bits of a float16 tensor of Model::m_data (an output kept out of m_outputs_convert_set, e.g. a key/value cache of the LLM flow) as a
        numpy float16 array; a device-resident tensor is copied from where it lies and stays there (model_hip_get_tensor_f16)."""
        import numpy as np
        f = self._lib.model_hip_get_tensor_f16
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int)]
        f.restype = ctypes.c_void_p
        shape, rank = (ctypes.c_ulonglong * 8)(), ctypes.c_int(0)
        self._err(f(self._h, self._name(name), None, 0, shape, ctypes.byref(rank)))
        out = np.empty([int(shape[k]) for k in range(rank.value)], np.float16)
        self._err(f(self._h, self._name(name), out.ctypes.data, out.size, shape, ctypes.byref(rank)))
        return out

    def hip_decode_plan_info(self) -> str:
        """The decode plan `generate` built, as hip_plan_info gives a plan; its first line is "decode capacity <rows>"."""
        f = self._lib.model_hip_decode_plan_info
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_void_p
        p = f(self._h)
        text = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        self._lib.model_free_buffer(p)
        if text.startswith("ERROR: "):
            raise OnnxStreamError(text[7:])
        return text

    def set_upcast_substrings(self, subs):
        """Model::m_requires_upcast (a std::function in C++, src/llm.cpp:379-383): ops whose name contains one of `subs` run in fp32.  Works on
        libonnxstream_amd.so (model_hip_set_upcast_substrings) and on the oracle build of the reference (ref_set_upcast_substrings)."""
        text = "|".join(subs).encode()
        for sym in ("model_hip_set_upcast_substrings", "ref_set_upcast_substrings"):
            f = getattr(self._lib, sym, None)
            if f is not None:
                f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = None
                f(self._h, text)
                return
        raise OnnxStreamError("this library has no way to set m_requires_upcast through the C API")

    def add_outputs_convert(self, name: str):
        """Model::m_outputs_convert_set.insert(name): once the set is non-empty only its members are converted back to fp32 at the end of run()."""
        for sym in ("model_hip_add_outputs_convert", "ref_add_outputs_convert_exclusion"):
            f = getattr(self._lib, sym, None)
            if f is not None:
                f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = None
                f(self._h, self._name(name))
                return
        raise OnnxStreamError("this library has no way to reach m_outputs_convert_set through the C API")

    def drop_tensor(self, name: str) -> bool:
        """Remove one tensor from Model::m_data (what the LLM app's get_output does after reading a result, src/llm.cpp:342-353)."""
        for sym in ("model_hip_drop_tensor", "ref_drop_tensor"):
            f = getattr(self._lib, sym, None)
            if f is not None:
                f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = ctypes.c_int
                return bool(f(self._h, self._name(name)))
        raise OnnxStreamError("this library cannot drop tensors through the C API")

    def fetch_tensor(self, name: str) -> None:
        """Bring a device-resident tensor of Model::m_data (option hip_resident_outputs) to the host (backend addition)."""
        f = self._lib.model_hip_fetch_tensor
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = ctypes.c_void_p
        self._err(f(self._h, self._name(name)))

    def rename_tensor(self, src: str, dst: str) -> bool:
        """Rename a tensor of Model::m_data in place (the LLM app turns the opkv* outputs of one call into the pkv* inputs of the next this way)."""
        for sym in ("model_hip_rename_tensor", "ref_rename_tensor"):
            f = getattr(self._lib, sym, None)
            if f is not None:
                f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]; f.restype = ctypes.c_int
                return bool(f(self._h, self._name(src), self._name(dst)))
        raise OnnxStreamError("this library cannot rename tensors through the C API")

    def hip_set_vram_budget(self, nbytes: int):
        """CudaOptions.m_vram_to_use: weights (model order) stay resident until `nbytes` are spent, the rest stream every pass."""
        f = self._lib.model_hip_set_vram_budget
        f.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong]; f.restype = None
        f(self._h, int(nbytes))

    def hip_resident_weight_bytes(self) -> int:
        f = self._lib.model_hip_resident_weight_bytes
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_ulonglong
        return int(f(self._h))

    def hip_read_range_data(self, filename: str):
        f = self._lib.model_hip_read_range_data
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = ctypes.c_void_p
        self._err(f(self._h, filename.encode()))

    def hip_write_range_data(self, filename: str):
        f = self._lib.model_hip_write_range_data
        f.argtypes = [ctypes.c_void_p, ctypes.c_char_p]; f.restype = ctypes.c_void_p
        self._err(f(self._h, filename.encode()))

    def hip_plan_info(self) -> str:
        """Steps (reads / writes / side-stream marks) and arena placement of the current plan, as text (Plan::info)."""
        f = self._lib.model_hip_plan_info
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_void_p
        p = f(self._h)
        text = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        self._lib.model_free_buffer(p)
        if text.startswith("ERROR: "):
            raise OnnxStreamError(text[7:])
        return text

    def hip_profile(self, reps: int = 1):
        """Eager pass with HIP events around every step -> list of (ms, flops, bytes, what)."""
        f = self._lib.model_hip_profile
        f.argtypes = [ctypes.c_void_p, ctypes.c_int]; f.restype = ctypes.c_void_p
        p = f(self._h, reps)
        text = ctypes.cast(p, ctypes.c_char_p).value.decode("utf-8", "replace")
        self._lib.model_free_buffer(p)
        if text.startswith("ERROR: "):
            raise OnnxStreamError(text[7:])
        rows = []
        for line in text.splitlines():
            ms, fl, by, what = line.split("\t", 3)
            rows.append((float(ms), float(fl), float(by), what))
        return rows

    def hip_last_pass_ms(self) -> float:
        f = self._lib.model_hip_last_pass_ms
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_double
        return f(self._h)

    def hip_streamed_bytes(self) -> int:
        f = self._lib.model_hip_streamed_bytes
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_ulonglong
        return int(f(self._h))

    def hip_plans_built(self) -> int:
        f = self._lib.model_hip_plans_built
        f.restype = ctypes.c_ulonglong
        f.argtypes = [ctypes.c_void_p]
        return int(f(self._h))

    def hip_last_kernel_count(self) -> int:
        f = self._lib.model_hip_last_kernel_count
        f.argtypes = [ctypes.c_void_p]; f.restype = ctypes.c_ulonglong
        return int(f(self._h))

    # -- name mangling (reference bindings.py:310) ------------------------------------------------
    @staticmethod
    def mangle_name(name: str) -> str:
        return "".join(c if c.isalnum() else f"_{ord(c):X}_" for c in name)

    @staticmethod
    def demangle_name(name: str) -> str:
        def repl(m):
            try:
                return chr(int(m.group(1), 16))
            except (ValueError, TypeError):
                return m.group(0)
        return re.sub(r"_([0-9A-Fa-f]+)_", repl, name)
