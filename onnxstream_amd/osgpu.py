"""ctypes binding over the C ABI of ``libosgpu.so`` (include/osgpu.h) -- one method per exported entry point.

Only plumbing lives here: numpy <-> device buffers and argument marshalling.  There is deliberately NO CPU fallback:
if the HIP library is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OSGPU_LIB") or os.path.join(_HERE, "libosgpu.so")   # (OSGPU_LIB: A/B runs against another build, as the host library honours it)

U8, F16, F32, I64 = 1, 2, 3, 4
_NP2DT = {np.dtype(np.uint8): U8, np.dtype(np.float16): F16, np.dtype(np.float32): F32, np.dtype(np.int64): I64}
ACT_NONE, ACT_SILU, ACT_SIGMOID = 0, 1, 2
UN = dict(sigmoid=0, erf=1, sqrt=2, sin=3, cos=4, neg=5, pow=6, silu=7, gelu_erf=8)
BIN = dict(add=0, sub=1, mul=2, div=3)

EXPORTS = [
    "osg_device_count", "osg_init", "osg_destroy", "osg_last_error", "osg_device_name", "osg_stream", "osg_set_autotune", "osg_tune_misses",
    "osg_malloc", "osg_free", "osg_upload", "osg_upload_sync", "osg_host_register", "osg_host_unregister", "osg_upload_pinned", "osg_upload_pinned_async", "osg_copy_fence", "osg_download", "osg_copy", "osg_memset", "osg_sync",
    "osg_graph_begin", "osg_graph_end", "osg_graph_launch", "osg_graph_destroy", "osg_timer_start", "osg_timer_stop",
    "osg_conv2d_nhwc", "osg_conv2d_nhwc_rb", "osg_conv2d_nhwc_v", "osg_conv2d_nhwc_cat", "osg_conv3x3_cat_entries", "osg_gemm", "osg_gemm_ln", "osg_gemm_rowstats", "osg_last_route", "osg_last_epilogue", "osg_last_kernel", "osg_gemm_kernarg_check", "osg_attention_kernarg_check", "osg_gemm_w8", "osg_conv2d_nhwc_w8", "osg_gemm_w8_v", "osg_conv2d_nhwc_w8_v", "osg_transpose_kn_to_nk", "osg_attention", "osg_attention_strided", "osg_sdpa", "osg_rms_norm", "osg_rope",
    "osg_instance_norm", "osg_group_norm_nhwc", "osg_layer_norm", "osg_reduce_mean_last", "osg_softmax_last",
    "osg_unary", "osg_binary", "osg_geglu", "osg_transpose", "osg_copy_2d", "osg_concat2", "osg_resize_nearest", "osg_gather_rows",
    "osg_maxpool_nhwc", "osg_convert", "osg_sampler_prepare", "osg_sampler_cfg_euler_a", "osg_sampler_cfg_multistep", "osg_sampler_prepare_rescale",
    "osg_sampler_prepare_single", "osg_sampler_euler_a_single", "osg_sampler_multistep_single", "osg_sampler_cfg_stochastic", "osg_sampler_stochastic_single",
    "osg_decode_gather", "osg_decode_blend", "osg_decode_pick", "osg_decode_sample", "osg_kv_append_at", "osg_sdpa_len",
    "osg_decode_sample_batch", "osg_kv_append_at_batch", "osg_sdpa_len_batch", "osg_rope_batch",
    "osg_sdpa_chunk", "osg_kv_append_rows_at", "osg_prefill_stage",
    "osg_decode_count", "osg_decode_penalize", "osg_decode_pick_ext", "osg_decode_sample_ext", "osg_decode_sample_batch_ext",
    "osg_range_push", "osg_range_pop", "osg_marker_record", "osg_copy_wait_marker", "osg_timer_mark", "osg_timer_between", "osg_set_stat_sinks", "osg_group_norm_stats_nhwc", "osg_qu8_conv2d_nhwc", "osg_qu8_conv2d_nhwc_t", "osg_qu8_conv_tap_sums", "osg_qu8_gemm", "osg_qu8_lut", "osg_qu8_binary", "osg_qu8_instance_norm", "osg_qu8_instance_norm_nhwc", "osg_qu8_affine_act", "osg_qu8_norm_affine_act_nhwc", "osg_qu8_softmax_last", "osg_kdbg_read",
    "osg_tblock_tail_supported", "osg_tblock_tail", "osg_tblock_kv_pack_elems", "osg_tblock_kv_pack_jobs", "osg_tblock_pack_weight", 
]


class OsgError(RuntimeError):
    pass


class TBlockTailArgs(ctypes.Structure):
    """osg_tblock_tail_args of include/osgpu.h"""
    _vp, _cf, _ci, _cl = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_long
    _fields_ = [("a1", _vp), ("x0", _vp), ("wo1", _vp), ("bo1", _vp), ("g2", _vp), ("be2", _vp), ("eps2", _cf), ("wq2", _vp), ("bq2", _vp),
                ("kp", _vp), ("vtp", _vp), ("scale", _cf), ("Tk", _ci), ("wo2", _vp), ("bo2", _vp), ("g3", _vp), ("be3", _vp), ("eps3", _cf),
                ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("wpo", _vp), ("bpo", _vp), ("xin", _vp), ("out", _vp), ("out2", _vp),
                ("ldo", _cl), ("ldo2", _cl), ("M", _ci), ("rows_per_img", _ci), ("C", _ci), ("heads", _ci), ("dbg", _vp * 8), ("rows_per_block", _ci)]


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise OsgError(f"{path} not found: build it with `python -m onnxstream_amd.build` (hipcc, gfx950)")
    lib = ctypes.CDLL(path)
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    lib.osg_init.argtypes = [ci, ctypes.POINTER(vp)]
    lib.osg_destroy.argtypes = [vp]
    lib.osg_destroy.restype = None
    lib.osg_last_error.argtypes = [vp]
    lib.osg_last_error.restype = ctypes.c_char_p
    lib.osg_device_name.argtypes = [vp]
    lib.osg_device_name.restype = ctypes.c_char_p
    lib.osg_stream.argtypes = [vp]
    lib.osg_stream.restype = vp
    lib.osg_malloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    lib.osg_free.argtypes = [vp, vp]
    lib.osg_host_register.argtypes = [vp, vp, ctypes.c_size_t]
    lib.osg_host_unregister.argtypes = [vp, vp]
    for f in ("osg_upload", "osg_upload_sync", "osg_upload_pinned", "osg_upload_pinned_async", "osg_download", "osg_copy"):
        getattr(lib, f).argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.osg_memset.argtypes = [vp, vp, ci, ctypes.c_size_t]
    lib.osg_sync.argtypes = [vp]
    lib.osg_copy_fence.argtypes = [vp]
    lib.osg_graph_begin.argtypes = [vp]
    lib.osg_graph_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.osg_graph_launch.argtypes = [vp, vp]
    lib.osg_graph_destroy.argtypes = [vp]
    lib.osg_graph_destroy.restype = None
    lib.osg_timer_start.argtypes = [vp]
    lib.osg_timer_stop.argtypes = [vp, ctypes.POINTER(cf)]
    lib.osg_conv2d_nhwc.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp] + [ci] * 14
    lib.osg_conv2d_nhwc_rb.argtypes = [vp, ci, vp, vp, vp, ci, vp, cl, vp, vp] + [ci] * 14
    lib.osg_conv2d_nhwc_v.argtypes = [vp, ci, vp, vp, vp, ci, vp, cl, vp, vp, cl, vp, cl] + [ci] * 14
    lib.osg_conv2d_nhwc_cat.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp, cl, vp, cl] + [ci] * 6
    lib.osg_conv3x3_cat_entries.argtypes = []
    lib.osg_gemm_w8.argtypes = [vp, vp, vp, cf, ci, vp, ci, vp, vp, ci, ci, ci, ci]
    lib.osg_conv2d_nhwc_w8.argtypes = [vp, vp, vp, cf, ci, vp, ci, vp, cl, vp, vp] + [ci] * 14
    lib.osg_gemm_w8_v.argtypes = [vp, vp, vp, cf, ci, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci]
    lib.osg_conv2d_nhwc_w8_v.argtypes = [vp, vp, vp, cf, ci, vp, vp, vp, ci, vp, cl, vp, vp, cl, vp, cl] + [ci] * 14
    lib.osg_gemm.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp, vp, ci, ci, ci, ci, cl, cl, cl, ci]
    lib.osg_transpose_kn_to_nk.argtypes = [vp, ci, vp, vp, ci, ci]
    lib.osg_attention.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, cf, ci]
    lib.osg_attention_strided.argtypes = [vp, ci, vp, cl, cl, cl, vp, cl, cl, cl, vp, cl, cl, cl, vp, cl, cl, cl, ci, ci, ci, ci,
                                          ci, cf]
    lib.osg_sdpa.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf]
    lib.osg_rms_norm.argtypes = [vp, ci, vp, vp, vp, cl, ci, cf]
    lib.osg_rope.argtypes = [vp, ci, vp, vp, vp, vp, cl, cl, ci]
    lib.osg_instance_norm.argtypes = [vp, ci, vp, vp, vp, vp, ci, cl, ci, cf]
    lib.osg_group_norm_nhwc.argtypes = [vp, ci, vp, vp, vp, vp, ci, cl, ci, ci, cf, ci]
    lib.osg_layer_norm.argtypes = [vp, ci, vp, vp, vp, vp, cl, ci, cf]
    lib.osg_reduce_mean_last.argtypes = [vp, ci, vp, vp, cl, cl]
    lib.osg_softmax_last.argtypes = [vp, ci, vp, vp, cl, cl]
    lib.osg_unary.argtypes = [vp, ci, ci, vp, vp, cl, cf]
    lib.osg_binary.argtypes = [vp, ci, ci, vp, ctypes.POINTER(cl), vp, ctypes.POINTER(cl), vp, ci]
    lib.osg_geglu.argtypes = [vp, ci, vp, vp, cl, cl]
    lib.osg_transpose.argtypes = [vp, ci, vp, vp, ci, ctypes.POINTER(cl), ctypes.POINTER(ci)]
    lib.osg_copy_2d.argtypes = [vp, ci, vp, cl, cl, vp, cl, cl, cl, cl]
    lib.osg_resize_nearest.argtypes = [vp, ci, vp, vp] + [ci] * 7
    lib.osg_gather_rows.argtypes = [vp, ci, vp, vp, vp, cl, cl, cl]
    lib.osg_maxpool_nhwc.argtypes = [vp, ci, vp, vp] + [ci] * 12
    lib.osg_convert.argtypes = [vp, ci, ci, vp, vp, cl, cf, ci]
    lib.osg_concat2.argtypes = [vp, ci, vp, cl, vp, cl, vp, cl]
    lib.osg_gemm_ln.argtypes = [vp, vp, vp, vp, vp, cf, vp, vp, vp, ci, ci, ci, ci]
    lib.osg_gemm_rowstats.argtypes = [vp, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, vp]
    lib.osg_last_route.argtypes = [vp, ctypes.POINTER(ci)]
    lib.osg_last_kernel.argtypes = [vp, ctypes.POINTER(ci)]
    if hasattr(lib, "osg_last_epilogue"):          # (absent from a library of an older tree that OSGPU_LIB names in an A/B run)
        lib.osg_last_epilogue.argtypes = [vp, ctypes.POINTER(ci)]
    if hasattr(lib, "osg_gemm_kernarg_check"):     # (absent from a library of an older tree that OSGPU_LIB names in an A/B run)
        lib.osg_gemm_kernarg_check.argtypes = [vp, cl, ci]
        lib.osg_attention_kernarg_check.argtypes = [vp, cl, ci, ci]
    lib.osg_sampler_prepare.argtypes = [vp, vp, vp, vp, ci, cl, cf, cf, cl]
    lib.osg_sampler_cfg_euler_a.argtypes = [vp, vp, vp, vp, ci, cl, cf, cf, cf, cf, cf, cf]
    lib.osg_sampler_cfg_multistep.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, cl, cf, cf, cf, cf, cf, cf, cf, cf, ctypes.c_double, ctypes.c_double]
    lib.osg_sampler_prepare_rescale.argtypes = [vp, vp, vp, vp, ci, cl, cf, cf, cf, cl]
    lib.osg_sampler_prepare_single.argtypes = [vp, vp, vp, vp, ci, cl, cf, cf, cf, cl]
    lib.osg_sampler_euler_a_single.argtypes = [vp, vp, vp, vp, ci, cl, cf, cf, cf, cf, cf]
    lib.osg_sampler_multistep_single.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, cl, cf, cf, cf, cf, cf, cf, cf, ctypes.c_double, ctypes.c_double]
    lib.osg_sampler_cfg_stochastic.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, cl] + [cf] * 12
    lib.osg_sampler_stochastic_single.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, cl] + [cf] * 11
    lib.osg_decode_gather.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf]
    lib.osg_decode_blend.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci]
    if hasattr(lib, "osg_decode_pick"):            # (absent from a library of an older tree that OSGPU_LIB names in an A/B run)
        lib.osg_decode_pick.argtypes = [vp, vp, cl, cl, ctypes.c_longlong, vp, vp, vp, vp, cl]
        lib.osg_kv_append_at.argtypes = [vp, vp, vp, vp, ci, cl, ci]
        lib.osg_sdpa_len.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, cl, cl, cl, ci, ci, ci, ci, cf]
    if hasattr(lib, "osg_decode_sample"):
        lib.osg_decode_sample.argtypes = [vp, vp, cl, cl, ctypes.c_longlong, vp, vp, vp, vp, cl, cf, cl, cf, ctypes.c_ulonglong, ctypes.c_ulonglong]
    if hasattr(lib, "osg_decode_sample_batch"):
        lib.osg_decode_sample_batch.argtypes = [vp, vp, cl, ci, ctypes.c_longlong, vp, vp, vp, vp, cl, cf, cl, cf, vp, ctypes.c_ulonglong]
        lib.osg_kv_append_at_batch.argtypes = [vp, vp, vp, vp, ci, ci, cl, ci]
        lib.osg_sdpa_len_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, cl, cl, cl, cl, ci, ci, ci, ci, cf]
        lib.osg_rope_batch.argtypes = [vp, ci, vp, vp, vp, vp, cl, cl, cl, ci]
    if hasattr(lib, "osg_sdpa_chunk"):
        lib.osg_sdpa_chunk.argtypes = [vp, ci, vp, vp, vp, vp, vp, cf, cl, cl, cl, ci, ci, ci, ci, ci, cf]
        lib.osg_kv_append_rows_at.argtypes = [vp, vp, vp, vp, ci, ci, cl, ci]
        lib.osg_prefill_stage.argtypes = [vp, vp, cl, cl, cl, ci, vp, vp, vp]
    if hasattr(lib, "osg_decode_penalize"):
        lib.osg_decode_count.argtypes = [vp, vp, cl, vp, cl]
        lib.osg_decode_penalize.argtypes = [vp, vp, cl, cl, ci, vp, vp, cf, cf, cf, cf]
        lib.osg_decode_pick_ext.argtypes = [vp, vp, cl, cl, ctypes.c_longlong, vp, vp, vp, vp, cl, vp]
        lib.osg_decode_sample_ext.argtypes = [vp, vp, cl, cl, ctypes.c_longlong, vp, vp, vp, vp, cl, cf, cl, cf, ctypes.c_ulonglong, ctypes.c_ulonglong, cf, vp]
        lib.osg_decode_sample_batch_ext.argtypes = [vp, vp, cl, ci, ctypes.c_longlong, vp, vp, vp, vp, cl, cf, cl, cf, vp, ctypes.c_ulonglong, cf, vp]
    lib.osg_set_stat_sinks.argtypes = [vp, vp, ci, ci, ci, vp, ci, ci, ci, ci]
    lib.osg_group_norm_stats_nhwc.argtypes = [vp, vp, vp, vp, vp, ci, ctypes.c_long, ci, ci, cf, ci, vp]
    lib.osg_qu8_conv2d_nhwc.argtypes = [vp, vp, cf, ci, vp, cf, ci, vp, cf, ci, vp] + [ci] * 13
    lib.osg_qu8_conv2d_nhwc_t.argtypes = [vp, vp, cf, ci, vp, cf, ci, vp, cf, ci, vp] + [ci] * 13 + [vp]
    lib.osg_qu8_conv_tap_sums.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.osg_qu8_gemm.argtypes = [vp, vp, cl, cf, ci, vp, cf, ci, vp, cf, ci, vp, ci, ci, ci, ci, cl, cl, cl]
    lib.osg_qu8_lut.argtypes = [vp, vp, vp, cl, vp]
    lib.osg_qu8_binary.argtypes = [vp, ci, vp, ctypes.POINTER(cl), cf, ci, vp, ctypes.POINTER(cl), cf, ci, vp, cf, ci, ci]
    lib.osg_qu8_instance_norm.argtypes = [vp, vp, vp, ci, cl, ci, vp, vp, cf, cf, ci, cf, ci]
    lib.osg_qu8_affine_act.argtypes = [vp, vp, cf, ci, vp, cf, ci, cf, ci, vp, cf, ci, cf, ci, vp, cf, ci, cf, ci, vp, cl, ci, cl]
    lib.osg_qu8_instance_norm_nhwc.argtypes = [vp, vp, vp, cl, ci, ci, ci, vp, vp, cf, cf, ci, cf, ci]
    lib.osg_qu8_norm_affine_act_nhwc.argtypes = [vp, vp, cl, ci, ci, ci, vp, vp, cf, cf, ci, cf, ci, vp, cf, ci, cf, ci, vp, cf, ci, cf, ci, vp, cf, ci, cf, ci, vp]
    lib.osg_qu8_softmax_last.argtypes = [vp, vp, vp, cl, cl, vp]
    lib.osg_tblock_tail_supported.argtypes = [ci] * 5
    lib.osg_tblock_tail.argtypes = [vp, ctypes.POINTER(TBlockTailArgs)]
    lib.osg_tblock_kv_pack_elems.argtypes = [ci, ci, ci]
    lib.osg_tblock_kv_pack_elems.restype = ctypes.c_size_t
    lib.osg_tblock_kv_pack_jobs.argtypes = [vp, vp, cl, ci, ci, ci, ci, vp, vp]
    lib.osg_tblock_pack_weight.argtypes = [vp, vp, ci, ci, vp]
    return lib


class DevBuf:
    """A device allocation with numpy-side shape/dtype metadata."""

    def __init__(self, gpu: "Gpu", shape, dtype):
        self.gpu = gpu
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = ctypes.c_void_p()
        gpu._ck(gpu.lib.osg_malloc(gpu.ctx, max(self.nbytes, 16), ctypes.byref(p)))
        self.ptr = p.value

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            self.gpu._ck(self.gpu.lib.osg_download(self.gpu.ctx, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def read_rows(self, lo: int, hi: int) -> np.ndarray:
        """rows [lo, hi) of the buffer seen as [rows, shape[-1]] (NHWC: pixels), copied back without the rest of it"""
        row = self.shape[-1]
        assert 0 <= lo <= hi <= self.size // row, (lo, hi, self.shape)
        out = np.empty((hi - lo, row), self.dtype)
        if out.nbytes:
            self.gpu._ck(self.gpu.lib.osg_download(self.gpu.ctx, out.ctypes.data, self.ptr + lo * row * self.dtype.itemsize, out.nbytes))
        return out

    def view(self, offset: int, shape) -> "DevBuf":
        """`shape` elements of this buffer from element `offset` on, as a DevBuf that owns nothing (an out= between guard bands); valid while self is"""
        v = DevBuf.__new__(DevBuf)
        v.gpu, v.shape, v.dtype = self.gpu, tuple(int(s) for s in shape), self.dtype
        v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * self.dtype.itemsize
        assert 0 <= offset and offset * self.dtype.itemsize + v.nbytes <= self.nbytes, (offset, shape, self.shape)
        v.ptr, v.base = self.ptr + offset * self.dtype.itemsize, self
        return v

    def free(self):
        if self.ptr and getattr(self, "base", None) is None:
            self.gpu.lib.osg_free(self.gpu.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Gpu:
    def __init__(self, device: int = 0, lib_path: str = LIB_PATH):
        self.lib = load_library(lib_path)
        if self.lib.osg_device_count() <= 0:
            raise OsgError("no HIP device visible: the osgpu backend has no CPU fallback")
        c = ctypes.c_void_p()
        rc = self.lib.osg_init(device, ctypes.byref(c))
        if rc:
            raise OsgError(f"osg_init failed with code {rc}")
        self.ctx = c

    def close(self):
        if self.ctx:
            self.lib.osg_destroy(self.ctx)
            self.ctx = None

    def _ck(self, rc):
        if rc:
            raise OsgError(self.lib.osg_last_error(self.ctx).decode())

    @property
    def name(self):
        return self.lib.osg_device_name(self.ctx).decode()

    # ---- memory ----
    def empty(self, shape, dtype=np.float16) -> DevBuf:
        """a new buffer with every byte 0xFF (NaN in f16 and f32): an element that a kernel should write and does not shows up"""
        b = DevBuf(self, shape, dtype)
        if b.nbytes:
            self.memset(b, 0xFF)
        return b

    def last_route(self):
        """osg_last_route: (family, instantiation, k-slices, folded, reduce kernel) of the most recent contraction call"""
        r = (ctypes.c_int * 5)()
        self._ck(self.lib.osg_last_route(self.ctx, r))
        return tuple(r)

    def last_epilogue(self):
        """osg_last_epilogue: (lean instantiation or -1, EPI mask or -1) of the most recent gemm2_kernel launch"""
        r = (ctypes.c_int * 2)()
        self._ck(self.lib.osg_last_epilogue(self.ctx, r))
        return tuple(r)

    def last_kernel(self):
        """osg_last_kernel: what the most recent attention / GroupNorm / LayerNorm / InstanceNorm / transformer-block tail / uint8-arithmetic call launched (eight fields, include/osgpu.h)"""
        r = (ctypes.c_int * 8)()
        self._ck(self.lib.osg_last_kernel(self.ctx, r))
        return tuple(r)

    def to_dev(self, arr: np.ndarray, staged: bool = False) -> DevBuf:
        arr = np.ascontiguousarray(arr)
        b = DevBuf(self, arr.shape, arr.dtype)
        if arr.nbytes:
            fn = self.lib.osg_upload if staged else self.lib.osg_upload_sync
            self._ck(fn(self.ctx, b.ptr, arr.ctypes.data, arr.nbytes))
        return b

    def sync(self):
        self._ck(self.lib.osg_sync(self.ctx))

    def memset(self, b: DevBuf, byte: int):
        """every byte of b set to `byte` (on the compute stream, so ordered before the kernels launched after it)"""
        self._ck(self.lib.osg_memset(self.ctx, b.ptr, byte, b.nbytes))

    def _out(self, out: Optional[DevBuf], shape, dtype) -> DevBuf:
        """the caller's output buffer (checked against the shape / dtype the op produces), or a fresh one"""
        if out is None:
            return self.empty(shape, dtype)
        if out.size != int(np.prod(shape, dtype=np.int64)) or out.dtype != np.dtype(dtype):
            raise OsgError(f"out= holds {out.shape} {out.dtype}, the op writes {tuple(shape)} {np.dtype(dtype)}")
        return out

    def timer_start(self):
        self._ck(self.lib.osg_timer_start(self.ctx))

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        self._ck(self.lib.osg_timer_stop(self.ctx, ctypes.byref(ms)))
        return ms.value

    # ---- compute ----
    @staticmethod
    def _p(b: Optional[DevBuf]):
        return b.ptr if b is not None else None

    def conv2d_nhwc(self, x: DevBuf, w: DevBuf, bias: Optional[DevBuf], stride=1, pads=(1, 1, 1, 1), residual=None, act=ACT_NONE,
                    image_bias: Optional[DevBuf] = None):
        n, h, wd, cin = x.shape
        cout, kh, kw, cin2 = w.shape
        assert cin == cin2
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        pt, pl, pb, pr = pads
        ho, wo = (h + pt + pb - kh) // sh + 1, (wd + pl + pr - kw) // sw + 1
        y = self.empty((n, ho, wo, cout), x.dtype)
        bdt = _NP2DT[bias.dtype] if bias is not None else F16
        if image_bias is not None:   # [n, cout] f16, added per image (fused resnet time-embedding add)
            self._ck(self.lib.osg_conv2d_nhwc_rb(self.ctx, _NP2DT[x.dtype], x.ptr, w.ptr, self._p(bias), bdt, image_bias.ptr, cout,
                                                 self._p(residual), y.ptr, n, h, wd, cin, cout, kh, kw, sh, sw, pt, pl, pb, pr, act))
            return y
        self._ck(self.lib.osg_conv2d_nhwc(self.ctx, _NP2DT[x.dtype], x.ptr, w.ptr, self._p(bias), bdt, self._p(residual), y.ptr, n, h,
                                          wd, cin, cout, kh, kw, sh, sw, pt, pl, pb, pr, act))
        return y

    def conv2d_nhwc_view(self, x: DevBuf, w: DevBuf, bias: Optional[DevBuf], wide: DevBuf, col: int, dense: Optional[DevBuf] = None, stride=1,
                         pads=(1, 1, 1, 1), residual=None, act=ACT_NONE, image_bias: Optional[DevBuf] = None, swap=False):
        """osg_conv2d_nhwc_v: the result goes into columns [col, col + Cout) of the NHWC buffer `wide` (its last axis is the row pitch) and, when
        `dense` is given, a second time into that dense [n, ho, wo, Cout] tensor (swap: dense is the primary destination, the slice the second)."""
        n, h, wd, cin = x.shape
        cout, kh, kw, _ = w.shape
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        pt, pl, pb, pr = pads
        bdt = _NP2DT[bias.dtype] if bias is not None else F16
        es = x.dtype.itemsize
        v_ptr, v_ld = wide.ptr + col * es, wide.shape[-1]
        if dense is None:
            y, y_ld, y2, y2_ld = v_ptr, v_ld, None, 0
        elif swap:
            y, y_ld, y2, y2_ld = dense.ptr, 0, v_ptr, v_ld
        else:
            y, y_ld, y2, y2_ld = v_ptr, v_ld, dense.ptr, cout
        self._ck(self.lib.osg_conv2d_nhwc_v(self.ctx, _NP2DT[x.dtype], x.ptr, w.ptr, self._p(bias), bdt, self._p(image_bias), cout if image_bias is not None else 0,
                                            self._p(residual), y, y_ld, y2, y2_ld, n, h, wd, cin, cout, kh, kw, sh, sw, pt, pl, pb, pr, act))

    def gemm(self, a: DevBuf, b: DevBuf, bias=None, residual=None, b_is_nk=False, act=ACT_NONE):
        """a:[(batch,)M,K]; b:[(batch,)K,N] (or [(batch,)N,K] when b_is_nk)."""
        batch = a.shape[0] if len(a.shape) == 3 else 1
        m, k = a.shape[-2:]
        n = b.shape[-2] if b_is_nk else b.shape[-1]
        sb = 0 if len(b.shape) == 2 else k * n
        c = self.empty(a.shape[:-1] + (n,), a.dtype)
        bdt = _NP2DT[bias.dtype] if bias is not None else F16
        self._ck(self.lib.osg_gemm(self.ctx, _NP2DT[a.dtype], a.ptr, b.ptr, int(b_is_nk), self._p(bias), bdt, self._p(residual), c.ptr, m,
                                   n, k, batch, m * k if batch > 1 else 0, sb, m * n if batch > 1 else 0, act))
        return c

    def gemm_rowstats(self, a: DevBuf, b_nk: DevBuf, bias=None, residual=None, act=ACT_NONE):
        """osg_gemm_rowstats: returns (C, rowstats[M, N/32, 2])."""
        m, k = a.shape
        n = b_nk.shape[0]
        c = self.empty((m, n), a.dtype)
        rs = self.empty((m, n // 32, 2), np.dtype(np.float32))
        bdt = _NP2DT[bias.dtype] if bias is not None else F16
        self._ck(self.lib.osg_gemm_rowstats(self.ctx, a.ptr, b_nk.ptr, self._p(bias), bdt, self._p(residual), c.ptr, m, n, k, act, rs.ptr))
        return c, rs

    def gemm_ln(self, x: DevBuf, w_nk: np.ndarray, gamma: np.ndarray, beta: np.ndarray, bias=None, eps: float = 1e-5, residual=None, act=ACT_NONE,
                rowstats=None):
        """LayerNorm(x; gamma, beta, eps) . w_nk^T + bias through osg_gemm_ln: folds gamma into the [N,K] weight and builds c1 / c2 on the
        host exactly as the planner does (plan.cpp ln_fold_weight).  x:[M,K] device f16; w_nk, gamma, beta, bias: host f16 arrays."""
        m, k = x.shape
        n = w_nk.shape[0]
        wf = (gamma.astype(np.float32)[None, :] * w_nk.astype(np.float32)).astype(np.float16)
        c1 = wf.astype(np.float64).sum(axis=1).astype(np.float32)
        c2 = (w_nk.astype(np.float64) @ beta.astype(np.float64) + (bias.astype(np.float64) if bias is not None else 0.0)).astype(np.float32)
        dw, d1, d2 = self.to_dev(wf), self.to_dev(c1), self.to_dev(c2)
        y = self.empty((m, n // 2 if act == 3 else n), x.dtype)
        self._ck(self.lib.osg_gemm_ln(self.ctx, x.ptr, dw.ptr, d1.ptr, d2.ptr, eps, self._p(rowstats), self._p(residual), y.ptr, m, n, k, act))
        return y

    def transpose_kn_to_nk(self, w: DevBuf):
        k, n = w.shape
        o = self.empty((n, k), w.dtype)
        self._ck(self.lib.osg_transpose_kn_to_nk(self.ctx, _NP2DT[w.dtype], w.ptr, o.ptr, k, n))
        return o

    def attention(self, q: DevBuf, k: DevBuf, v: DevBuf, scale: float, k_is_dt: bool, out: Optional[DevBuf] = None):
        heads, tq, d = q.shape
        tkv = v.shape[1]
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_attention(self.ctx, _NP2DT[q.dtype], q.ptr, k.ptr, v.ptr, o.ptr, heads, tq, tkv, d, scale, int(k_is_dt)))
        return o

    def attention_tokens(self, q: DevBuf, k: DevBuf, v: DevBuf, heads: int, scale: float, out: Optional[DevBuf] = None):
        """q:[B,Tq,heads*D], k,v:[B,Tkv,heads*D] straight out of the projections -> o:[B,Tq,heads*D]."""
        bsz, tq, c = q.shape
        tkv = k.shape[1]
        d = c // heads
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_attention_strided(self.ctx, F16, q.ptr, c, d, tq * c, k.ptr, c, d, tkv * c, v.ptr, c, d, tkv * c, o.ptr, c, d,
                                                tq * c, bsz, heads, tq, tkv, d, scale))
        return o

    def attention_strided(self, q, k, v, o, batch: int, heads: int, tq: int, tkv: int, d: int, scale: float):
        """osg_attention_strided on raw operands: q, k, v, o = (device address, token stride, head stride, batch stride), strides in elements"""
        self._ck(self.lib.osg_attention_strided(self.ctx, F16, *q, *k, *v, *o, batch, heads, tq, tkv, d, scale))

    def tblock_kv_pack(self, k: DevBuf, v: DevBuf, heads: int):
        """k, v: [imgs, Tk, heads*D] -> (kp [imgs, heads, 80, DP], vtp [imgs, heads, DP, 80]) for tblock_tail.  Goes through the multi-job entry point the
        planner uses: K and V become two column ranges of one [imgs*Tk, 2C] matrix."""
        imgs, tk, c = k.shape
        d = c // heads
        dp = (d + 15) // 16 * 16
        n = self.lib.osg_tblock_kv_pack_elems(imgs, heads, d)
        assert n == imgs * heads * 80 * dp
        kv = self.to_dev(np.concatenate([k.numpy().reshape(imgs * tk, c), v.numpy().reshape(imgs * tk, c)], axis=1))
        jobs = self.to_dev(np.array([0, c, d, 0], np.int32))
        dst = self.empty((2 * n,), k.dtype)
        self._ck(self.lib.osg_tblock_kv_pack_jobs(self.ctx, kv.ptr, 2 * c, imgs, tk, heads, 1, jobs.ptr, dst.ptr))
        kp, vtp = self.empty((imgs, heads, 80, dp), k.dtype), self.empty((imgs, heads, dp, 80), k.dtype)
        self._ck(self.lib.osg_copy(self.ctx, kp.ptr, dst.ptr, n * 2))
        self._ck(self.lib.osg_copy(self.ctx, vtp.ptr, dst.ptr + n * 2, n * 2))
        return kp, vtp

    def tblock_kv_pack_jobs(self, base: DevBuf, ld: int, imgs: int, tk: int, heads: int, jobs, out: Optional[DevBuf] = None):
        """osg_tblock_kv_pack_jobs as the planner calls it: every job of `jobs` = (k_col, v_col, D) reads two column ranges of the one matrix `base`
        ([imgs * tk] rows, ld elements apart) in ONE launch.  Returns (dst, [element offset of each job's packs inside dst]): at an offset kp
        [imgs, heads, 80, DP], and osg_tblock_kv_pack_elems further on vtp [imgs, heads, DP, 80]."""
        offs, total = [], 0
        for _, _, d in jobs:
            offs.append(total)
            total += 2 * self.lib.osg_tblock_kv_pack_elems(imgs, heads, d)
        table = self.to_dev(np.array([[kc, vc, d, o] for (kc, vc, d), o in zip(jobs, offs)], np.int32))
        dst = self._out(out, (total,), base.dtype)
        self._ck(self.lib.osg_tblock_kv_pack_jobs(self.ctx, base.ptr, ld, imgs, tk, heads, len(offs), table.ptr, dst.ptr))
        self.sync()           # (the job table is read by the launch: it may go once the launch has run)
        table.free()
        return dst, offs

    TBLOCK_WEIGHTS = ("wo1", "wq2", "wo2", "w1", "w2", "wpo")

    def tblock_pack_weight(self, w_nk: DevBuf, out: Optional[DevBuf] = None) -> DevBuf:
        """[N, K] (k contiguous) -> the kn8 layout osg_tblock_tail streams, returned as a [K/8, N, 8] buffer"""
        n, k = w_nk.shape
        out = self._out(out, (k // 8, n, 8), w_nk.dtype)
        self._ck(self.lib.osg_tblock_pack_weight(self.ctx, w_nk.ptr, n, k, out.ptr))
        return out

    def tblock_weights(self, w: dict) -> dict:
        """host dict of a block's operands (weights [N, K]) -> device dict as tblock_tail wants it (weights packed)"""
        return {n: (self.tblock_pack_weight(self.to_dev(t)) if n in self.TBLOCK_WEIGHTS else self.to_dev(t)) for n, t in w.items()}

    def tblock_tail(self, a1: DevBuf, x0: DevBuf, w: dict, kp: DevBuf, vtp: DevBuf, tk: int, heads: int, scale: float, rows_per_img: int, eps: float = 1e-5,
                    xin: Optional[DevBuf] = None, out2: Optional[DevBuf] = None, out2_col: int = 0, debug: bool = False, out: Optional[DevBuf] = None, stamps: Optional[DevBuf] = None, rows_per_block: int = 0,
                    out_col: Optional[int] = None):
        """osg_tblock_tail.  w: dict of DevBuf -- wo1 [bo1] g2 be2 wq2 [bq2] wo2 [bo2] g3 be3 w1 [b1] w2 [b2] [wpo bpo]; weights in the kn8 layout (tblock_weights).
        out: a dense [m, c] buffer (the default: a fresh one) or, with out_col given, a wider [m, pitch] buffer whose columns [out_col, out_col + c) are
        written (a Concat slot, as out2 / out2_col).  Returns (out, [dumps])."""
        m, c = a1.shape
        a = TBlockTailArgs()
        a.a1, a.x0 = a1.ptr, x0.ptr
        for k_ in ("wo1", "bo1", "g2", "be2", "wq2", "wo2", "bo2", "g3", "be3", "w1", "b1", "w2", "b2", "wpo", "bpo", "bq2"):
            setattr(a, k_, w[k_].ptr if w.get(k_) is not None else None)
        a.kp, a.vtp, a.scale, a.Tk = kp.ptr, vtp.ptr, scale, tk
        a.eps2 = a.eps3 = eps
        a.xin = xin.ptr if xin is not None else None
        if out is None:
            out = self.empty((m, c), a1.dtype)
        if out_col is None:
            a.out, a.ldo = out.ptr, c
        else:
            a.out, a.ldo = out.ptr + out_col * 2, out.shape[-1]
        if out2 is not None:
            a.out2, a.ldo2 = out2.ptr + out2_col * 2, out2.shape[-1]
        a.M, a.rows_per_img, a.C, a.heads = m, rows_per_img, c, heads
        a.rows_per_block = rows_per_block
        dumps = []
        if debug:
            dumps = [self.empty((m, c), a1.dtype) for _ in range(7)]
            for i, dbuf in enumerate(dumps):
                a.dbg[i] = dbuf.ptr
        if stamps is not None:
            a.dbg[7] = stamps.ptr
        self._ck(self.lib.osg_tblock_tail(self.ctx, ctypes.byref(a)))
        return out, dumps

    def rms_norm(self, x: DevBuf, w: DevBuf, eps: float, out: Optional[DevBuf] = None):
        rows, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_rms_norm(self.ctx, _NP2DT[x.dtype], x.ptr, w.ptr, y.ptr, rows, c, eps))
        return y

    def rope(self, x: DevBuf, cos: DevBuf, sin: DevBuf):
        """x:[..., T, d], cos / sin:[T, d]"""
        t, d = x.shape[-2], x.shape[-1]
        y = self.empty(x.shape, x.dtype)
        self._ck(self.lib.osg_rope(self.ctx, _NP2DT[x.dtype], x.ptr, cos.ptr, sin.ptr, y.ptr, int(np.prod(x.shape[:-2])), t, d))
        return y

    def sdpa(self, q: DevBuf, k: DevBuf, v: DevBuf, mask: Optional[DevBuf], scale: float, out: Optional[DevBuf] = None):
        """q:[B,Hq,Tq,D], k,v:[B,Hkv,Tkv,D], mask:[Tq,Tkv] additive or None -> o:[B,Hq,Tq,D] (the reference's ScaledDotProductAttention op)."""
        bsz, hq, tq, d = q.shape
        hkv, tkv = k.shape[1], k.shape[2]
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_sdpa(self.ctx, _NP2DT[q.dtype], q.ptr, k.ptr, v.ptr, self._p(mask), o.ptr, bsz, hq, hkv, tq, tkv, d, scale))
        return o

    def sdpa_len(self, q: DevBuf, k: DevBuf, v: DevBuf, mask: DevBuf, state: DevBuf, scale: float, out: Optional[DevBuf] = None):
        """osg_sdpa_len: q:[B,Hq,1,D], k,v: capacity buffers [B,Hkv,CAP,D], mask:[CAP]; the number of keys is state[1] (device int32[4], osg_decode_pick's state)"""
        bsz, hq, tq, d = q.shape
        hkv, cap = k.shape[1], k.shape[2]
        assert tq == 1 and state.dtype == np.int32 and state.size >= 4
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_sdpa_len(self.ctx, _NP2DT[q.dtype], q.ptr, k.ptr, v.ptr, self._p(mask), o.ptr, state.ptr + 4, cap * d, cap * d * hkv, cap, bsz, hq, hkv,
                                       d, scale))
        return o

    def sdpa_chunk(self, q: DevBuf, k: DevBuf, v: DevBuf, base: DevBuf, masked: float, scale: float, out: Optional[DevBuf] = None):
        """osg_sdpa_chunk: q:[B,Hq,C,D], k,v: capacity buffers [B,Hkv,CAP,D]; query row i sees the keys 0 .. base[0] + i (base: device int32), a barred key
        gets the addend `masked`; None for `base` passes a null pointer (refused)"""
        bsz, hq, c, d = q.shape
        hkv, cap = k.shape[1], k.shape[2]
        assert base is None or base.dtype == np.int32
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_sdpa_chunk(self.ctx, _NP2DT[q.dtype], q.ptr, k.ptr, v.ptr, o.ptr, self._p(base), float(masked), cap * d, cap * d * hkv, cap, bsz, hq,
                                         hkv, c, d, scale))
        return o

    def kv_append_rows_at(self, src: DevBuf, cache: DevBuf, base: DevBuf):
        """osg_kv_append_rows_at: src f16 [Hkv, C, d] into cache [Hkv, CAP, d] from row base[0] on (device int32), in place"""
        hkv, cap, d = cache.shape
        assert src.shape[0] == hkv and src.shape[2] == d and base.dtype == np.int32
        self._ck(self.lib.osg_kv_append_rows_at(self.ctx, src.ptr, cache.ptr, base.ptr, hkv, src.shape[1], cap, d))

    def prefill_stage(self, prompt: DevBuf, first: int, pos0: int, ids: DevBuf, pos: DevBuf, base: DevBuf):
        """osg_prefill_stage: ids / pos int64 [C] from prompt int64 [n] at `first` and positions pos0 .., zeros behind the prompt's end; base[0] = pos0"""
        assert prompt.dtype == ids.dtype == pos.dtype == np.int64 and base.dtype == np.int32 and ids.size == pos.size
        self._ck(self.lib.osg_prefill_stage(self.ctx, prompt.ptr, prompt.size, int(first), int(pos0), ids.size, ids.ptr, pos.ptr, base.ptr))

    def kv_append_at(self, src: DevBuf, cache: DevBuf, state: DevBuf):
        """osg_kv_append_at: src f16 [Hkv, d] into cache [Hkv, CAP, d] at row state[0] (device int32[4]), in place"""
        hkv, cap, d = cache.shape
        assert src.size == hkv * d and state.dtype == np.int32 and state.size >= 4
        self._ck(self.lib.osg_kv_append_at(self.ctx, src.ptr, cache.ptr, state.ptr, hkv, cap, d))

    def decode_pick(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf):
        """osg_decode_pick over the last row of logits [T, V] fp32; state int32[4] = (row, len, n_tokens, stop); ids, pos int64 [1]; tokens int64 [max_tokens]"""
        t, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 and ids.dtype == pos.dtype == tokens.dtype == np.int64
        self._ck(self.lib.osg_decode_pick(self.ctx, logits.ptr, t, vv, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.size))

    def decode_sample(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf, temperature: float, top_k: int = 0,
                      top_p: float = 1.0, seed: int = 0, draw_base: int = 0):
        """osg_decode_sample: decode_pick's operands, then the sampling rule of include/osgpu.h (temperature > 0, top_k 0 = off, top_p 1 = off, a 64-bit seed;
        the draw index is draw_base + state[2])"""
        t, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 and ids.dtype == pos.dtype == tokens.dtype == np.int64
        self._ck(self.lib.osg_decode_sample(self.ctx, logits.ptr, t, vv, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.size, float(temperature),
                                            int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), int(draw_base) & (2 ** 64 - 1)))

    def decode_sample_batch(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf, seeds: DevBuf, temperature: float,
                            top_k: int = 0, top_p: float = 1.0, draw_base: int = 0):
        """osg_decode_sample_batch: logits fp32 [n_seq, V], state int32 [n_seq, 4], ids / pos int64 [n_seq], tokens int64 [n_seq, max_tokens], seeds uint64
        [n_seq] on the device; sequence s is decode_sample over row s with seeds[s]"""
        ns, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 * ns and ids.dtype == pos.dtype == tokens.dtype == np.int64
        assert ids.size >= ns and pos.size >= ns and tokens.shape[0] == ns and seeds.dtype == np.uint64 and seeds.size >= ns
        self._ck(self.lib.osg_decode_sample_batch(self.ctx, logits.ptr, vv, ns, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.shape[1],
                                                  float(temperature), int(top_k), float(top_p), seeds.ptr, int(draw_base) & (2 ** 64 - 1)))

    def decode_count(self, tokens: DevBuf, counts: DevBuf, n: Optional[int] = None):
        """osg_decode_count: counts int32 [V] += the occurrences of the first n (default: all) device tokens int64; tokens outside [0, V) are ignored"""
        assert tokens.dtype == np.int64 and counts.dtype == np.int32
        n = tokens.size if n is None else int(n)
        assert 0 <= n <= tokens.size
        self._ck(self.lib.osg_decode_count(self.ctx, tokens.ptr, n, counts.ptr, counts.size))

    def decode_penalize(self, logits: DevBuf, counts: DevBuf, repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0, row: int = 0,
                        n_seq: int = 1, out: Optional[DevBuf] = None) -> DevBuf:
        """osg_decode_penalize (step 0 of the rule, include/osgpu.h): rows row .. row + n_seq - 1 of logits fp32 [T, V] under counts int32 [n_seq, V]
        -> fp32 [n_seq, V]; inv_r = 1 / repetition is taken in fp32 here, as the host library takes it"""
        t, vv = logits.shape
        assert logits.dtype == np.float32 and counts.dtype == np.int32 and counts.size == n_seq * vv and 0 <= row and row + n_seq <= t
        o = self._out(out, (n_seq, vv), np.float32)
        r = np.float32(repetition)
        with np.errstate(all="ignore"):
            inv_r = np.float32(1.0) / r
        self._ck(self.lib.osg_decode_penalize(self.ctx, logits.ptr + 4 * row * vv, vv, vv, n_seq, counts.ptr, o.ptr, float(r), float(inv_r), float(presence),
                                              float(frequency)))
        return o

    def decode_pick_ext(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf, counts: Optional[DevBuf] = None):
        """osg_decode_pick_ext: decode_pick, and counts int32 [V] (or None) raised at the token it appends"""
        t, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 and ids.dtype == pos.dtype == tokens.dtype == np.int64
        assert counts is None or (counts.dtype == np.int32 and counts.size == vv)
        self._ck(self.lib.osg_decode_pick_ext(self.ctx, logits.ptr, t, vv, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.size, self._p(counts)))

    def decode_sample_ext(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf, temperature: float, top_k: int = 0,
                          top_p: float = 1.0, seed: int = 0, draw_base: int = 0, min_p: float = 0.0, counts: Optional[DevBuf] = None):
        """osg_decode_sample_ext: decode_sample plus min_p (0 = off) and counts int32 [V] (or None) raised at the token it appends"""
        t, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 and ids.dtype == pos.dtype == tokens.dtype == np.int64
        assert counts is None or (counts.dtype == np.int32 and counts.size == vv)
        self._ck(self.lib.osg_decode_sample_ext(self.ctx, logits.ptr, t, vv, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.size, float(temperature),
                                                int(top_k), float(top_p), int(seed) & (2 ** 64 - 1), int(draw_base) & (2 ** 64 - 1), float(min_p),
                                                self._p(counts)))

    def decode_sample_batch_ext(self, logits: DevBuf, eos_id: int, state: DevBuf, ids: DevBuf, pos: DevBuf, tokens: DevBuf, seeds: DevBuf, temperature: float,
                                top_k: int = 0, top_p: float = 1.0, draw_base: int = 0, min_p: float = 0.0, counts: Optional[DevBuf] = None):
        """osg_decode_sample_batch_ext: decode_sample_batch plus min_p and counts int32 [n_seq, V] (or None)"""
        ns, vv = logits.shape
        assert logits.dtype == np.float32 and state.dtype == np.int32 and state.size >= 4 * ns and ids.dtype == pos.dtype == tokens.dtype == np.int64
        assert ids.size >= ns and pos.size >= ns and tokens.shape[0] == ns and seeds.dtype == np.uint64 and seeds.size >= ns
        assert counts is None or (counts.dtype == np.int32 and counts.size == ns * vv)
        self._ck(self.lib.osg_decode_sample_batch_ext(self.ctx, logits.ptr, vv, ns, int(eos_id), state.ptr, ids.ptr, pos.ptr, tokens.ptr, tokens.shape[1],
                                                      float(temperature), int(top_k), float(top_p), seeds.ptr, int(draw_base) & (2 ** 64 - 1), float(min_p),
                                                      self._p(counts)))

    def kv_append_at_batch(self, src: DevBuf, cache: DevBuf, state: DevBuf):
        """osg_kv_append_at_batch: src f16 [B, Hkv, d] into cache [B, Hkv, CAP, d], batch b at row state[b, 0] (device int32 [B, 4]), in place"""
        bsz, hkv, cap, d = cache.shape
        assert src.size == bsz * hkv * d and state.dtype == np.int32 and state.size >= 4 * bsz
        self._ck(self.lib.osg_kv_append_at_batch(self.ctx, src.ptr, cache.ptr, state.ptr, bsz, hkv, cap, d))

    def sdpa_len_batch(self, q: DevBuf, k: DevBuf, v: DevBuf, mask: DevBuf, state: DevBuf, scale: float, out: Optional[DevBuf] = None):
        """osg_sdpa_len_batch: q:[B,Hq,1,D], k,v: capacity buffers [B,Hkv,CAP,D], mask:[CAP]; batch b reads state[b, 1] keys (device int32 [B, 4])"""
        bsz, hq, tq, d = q.shape
        hkv, cap = k.shape[1], k.shape[2]
        assert tq == 1 and state.dtype == np.int32 and state.size >= 4 * bsz
        o = self._out(out, q.shape, q.dtype)
        self._ck(self.lib.osg_sdpa_len_batch(self.ctx, _NP2DT[q.dtype], q.ptr, k.ptr, v.ptr, self._p(mask), o.ptr, state.ptr + 4, 4, cap * d, cap * d * hkv, cap,
                                             bsz, hq, hkv, d, scale))
        return o

    def rope_batch(self, x: DevBuf, cos: DevBuf, sin: DevBuf):
        """osg_rope_batch: x [B, H, T, d], cos / sin [B, T, d]"""
        bsz, h, t, d = x.shape
        y = self.empty(x.shape, x.dtype)
        self._ck(self.lib.osg_rope_batch(self.ctx, _NP2DT[x.dtype], x.ptr, cos.ptr, sin.ptr, y.ptr, bsz, h, t, d))
        return y

    def instance_norm(self, x: DevBuf, scale: Optional[DevBuf], bias: Optional[DevBuf], eps: float, out: Optional[DevBuf] = None):
        rows, L = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, x.dtype)
        ns = scale.size if scale is not None else bias.size if bias is not None else 1
        self._ck(self.lib.osg_instance_norm(self.ctx, _NP2DT[x.dtype], x.ptr, self._p(scale), self._p(bias), y.ptr, rows, L, ns, eps))
        return y

    def set_stat_sinks(self, rows_per_image: int, t0: Optional[DevBuf] = None, groups0=0, cpg0=0, off0=0, t1: Optional[DevBuf] = None, groups1=0, cpg1=0, off1=0):
        """osg_set_stat_sinks: arm the NEXT conv2d_nhwc / conv2d_nhwc_view launch (tables: int64 [N][groups][2], zeroed by the caller)."""
        self._ck(self.lib.osg_set_stat_sinks(self.ctx, self._p(t0), groups0, cpg0, off0, self._p(t1), groups1, cpg1, off1, rows_per_image))

    def group_norm_stats_nhwc(self, x: DevBuf, gamma: DevBuf, beta: DevBuf, groups: int, eps: float, table: DevBuf, act=ACT_NONE, out: Optional[DevBuf] = None):
        n, h, w, c = x.shape
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_group_norm_stats_nhwc(self.ctx, x.ptr, gamma.ptr, beta.ptr, y.ptr, n, h * w, c, groups, eps, act, table.ptr))
        return y

    def group_norm_nhwc(self, x: DevBuf, gamma: DevBuf, beta: DevBuf, groups: int, eps: float, act=ACT_NONE, out: Optional[DevBuf] = None):
        n, h, w, c = x.shape
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_group_norm_nhwc(self.ctx, _NP2DT[x.dtype], x.ptr, gamma.ptr, beta.ptr, y.ptr, n, h * w, c, groups, eps, act))
        return y

    def layer_norm(self, x: DevBuf, gamma: DevBuf, beta: DevBuf, eps: float, out: Optional[DevBuf] = None):
        rows, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_layer_norm(self.ctx, _NP2DT[x.dtype], x.ptr, gamma.ptr, beta.ptr, y.ptr, rows, c, eps))
        return y

    def reduce_mean_last(self, x: DevBuf, out: Optional[DevBuf] = None):
        rows, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape[:-1] + (1,), x.dtype)
        self._ck(self.lib.osg_reduce_mean_last(self.ctx, _NP2DT[x.dtype], x.ptr, y.ptr, rows, c))
        return y

    def softmax_last(self, x: DevBuf, out: Optional[DevBuf] = None):
        rows, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_softmax_last(self.ctx, _NP2DT[x.dtype], x.ptr, y.ptr, rows, c))
        return y

    def unary(self, kind: str, x: DevBuf, param: float = 0.0, out: Optional[DevBuf] = None):
        y = self._out(out, x.shape, x.dtype)
        self._ck(self.lib.osg_unary(self.ctx, _NP2DT[x.dtype], UN[kind], x.ptr, y.ptr, x.size, param))
        return y

    def binary(self, kind: str, a: DevBuf, b: DevBuf, out: Optional[DevBuf] = None):
        rank = max(len(a.shape), len(b.shape))
        ash = (1,) * (rank - len(a.shape)) + a.shape
        bsh = (1,) * (rank - len(b.shape)) + b.shape
        osh = tuple(np.broadcast_shapes(ash, bsh))
        y = self._out(out, osh, a.dtype)
        self.binary_at(kind, a.dtype, a.ptr, ash, b.ptr, bsh, y.ptr)
        return y

    def binary_at(self, kind: str, dtype, a_ptr: int, a_shape, b_ptr: int, b_shape, y_ptr: int):
        """osg_binary on raw device addresses (e.g. an offset into a DevBuf: the entry point's unaligned-operand path); shapes of equal rank"""
        rank = len(a_shape)
        assert len(b_shape) == rank
        A = (ctypes.c_long * rank)(*a_shape)
        B = (ctypes.c_long * rank)(*b_shape)
        self._ck(self.lib.osg_binary(self.ctx, _NP2DT[np.dtype(dtype)], BIN[kind], a_ptr, A, b_ptr, B, y_ptr, rank))

    def geglu(self, x: DevBuf):
        rows, c2 = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self.empty(x.shape[:-1] + (c2 // 2,), x.dtype)
        self._ck(self.lib.osg_geglu(self.ctx, _NP2DT[x.dtype], x.ptr, y.ptr, rows, c2 // 2))
        return y

    def transpose(self, x: DevBuf, perm: Sequence[int], out: Optional[DevBuf] = None):
        rank = len(x.shape)
        y = self._out(out, tuple(x.shape[p] for p in perm), x.dtype)
        S = (ctypes.c_long * rank)(*x.shape)
        P = (ctypes.c_int * rank)(*perm)
        self._ck(self.lib.osg_transpose(self.ctx, x.dtype.itemsize, x.ptr, y.ptr, rank, S, P))
        return y

    def copy_2d(self, src: DevBuf, src_pitch, src_off, dst: DevBuf, dst_pitch, dst_off, outer, inner):
        self._ck(self.lib.osg_copy_2d(self.ctx, src.dtype.itemsize, src.ptr, src_pitch, src_off, dst.ptr, dst_pitch, dst_off, outer, inner))

    def concat2(self, a: DevBuf, b: DevBuf, out: Optional[DevBuf] = None):
        """Concat of two dense tensors along the last axis in one launch."""
        outer = int(np.prod(a.shape[:-1]))
        y = self._out(out, a.shape[:-1] + (a.shape[-1] + b.shape[-1],), a.dtype)
        self._ck(self.lib.osg_concat2(self.ctx, a.dtype.itemsize, a.ptr, a.shape[-1], b.ptr, b.shape[-1], y.ptr, outer))
        return y

    def resize_nearest(self, x: DevBuf, ho: int, wo: int, nhwc: bool, out: Optional[DevBuf] = None):
        if nhwc:
            n, h, w, c = x.shape
            y = self._out(out, (n, ho, wo, c), x.dtype)
        else:
            n, c, h, w = x.shape
            y = self._out(out, (n, c, ho, wo), x.dtype)
        self._ck(self.lib.osg_resize_nearest(self.ctx, x.dtype.itemsize, x.ptr, y.ptr, n, c, h, w, ho, wo, int(nhwc)))
        return y

    def gather_rows(self, x: DevBuf, idx: DevBuf, out: Optional[DevBuf] = None):
        n_rows = x.shape[0]
        row = int(np.prod(x.shape[1:]))
        y = self._out(out, (idx.size,) + x.shape[1:], x.dtype)
        self._ck(self.lib.osg_gather_rows(self.ctx, x.dtype.itemsize, x.ptr, idx.ptr, y.ptr, idx.size, row, n_rows))
        return y

    def maxpool_nhwc(self, x: DevBuf, k, stride, pads, out: Optional[DevBuf] = None):
        n, h, w, c = x.shape
        pt, pl, pb, pr = pads
        ho, wo = (h + pt + pb - k[0]) // stride[0] + 1, (w + pl + pr - k[1]) // stride[1] + 1
        y = self._out(out, (n, ho, wo, c), x.dtype)
        self._ck(self.lib.osg_maxpool_nhwc(self.ctx, _NP2DT[x.dtype], x.ptr, y.ptr, n, h, w, c, k[0], k[1], stride[0], stride[1], pt, pl,
                                           pb, pr))
        return y

    def convert(self, x: DevBuf, dtype, scale: float = 1.0, zero_point: int = 0, out: Optional[DevBuf] = None):
        y = self._out(out, x.shape, dtype)
        self._ck(self.lib.osg_convert(self.ctx, _NP2DT[x.dtype], _NP2DT[np.dtype(dtype)], x.ptr, y.ptr, x.size, scale, zero_point))
        return y

    # ---- latents -> image around the VAE decoder pass ----
    @staticmethod
    def decode_tiles_along(n: int, tile: int) -> int:
        """number of tile origins along an axis of n latent pixels (0, 3*tile/4, ..., the last one flush with the border)"""
        step = tile * 3 // 4
        return 1 if n == tile else (n - tile + step - 1) // step + 1

    def decode_gather(self, latents: DevBuf, tile: int, factor: float, out: Optional[DevBuf] = None) -> DevBuf:
        """osg_decode_gather: latents [P,4,H,W] float32 -> the scaled tiles [P*T,4,tile,tile]"""
        P, c, H, W = latents.shape
        assert c == 4 and latents.dtype == np.float32
        T = self.decode_tiles_along(H, tile) * self.decode_tiles_along(W, tile)
        y = self._out(out, (P * T, 4, tile, tile), np.float32)
        self._ck(self.lib.osg_decode_gather(self.ctx, latents.ptr, y.ptr, P, H, W, tile, factor))
        return y

    def decode_blend(self, tiles: DevBuf, images: int, H: int, W: int, tile: int, want: str = "both", image: Optional[DevBuf] = None,
                     pixels: Optional[DevBuf] = None):
        """osg_decode_blend: decoder outputs [P*T,3,up*tile,up*tile] float32 -> (image [P,3,up*H,up*W] float32 or None, pixels [P,up*H,up*W,3]
        uint8 or None); want = "f32" | "u8" | "both" """
        assert want in ("f32", "u8", "both") and tiles.dtype == np.float32 and tiles.shape[1] == 3 and tiles.shape[2] % tile == 0
        up = tiles.shape[2] // tile
        T = self.decode_tiles_along(H, tile) * self.decode_tiles_along(W, tile)
        assert tiles.shape == (images * T, 3, up * tile, up * tile), (tiles.shape, images, T, up, tile)
        img = self._out(image, (images, 3, up * H, up * W), np.float32) if want != "u8" else None
        pix = self._out(pixels, (images, up * H, up * W, 3), np.uint8) if want != "f32" else None
        self._ck(self.lib.osg_decode_blend(self.ctx, tiles.ptr, self._p(img), self._p(pix), images, H, W, tile, up))
        return img, pix

    # ---- uint8 arithmetic (a uint8 tensor = codes DevBuf + (scale, zero_point)); out=: the caller's output buffer, as for the other ops ----
    def _table(self, t, dtype):
        """a 256-entry table: a DevBuf is used where it lies (owned by the caller), a host array is uploaded (owned here) -> (DevBuf, owned)"""
        if isinstance(t, DevBuf):
            if t.size != 256 or t.dtype != np.dtype(dtype):
                raise OsgError(f"a device table of 256 {np.dtype(dtype)} is wanted, not {t.shape} {t.dtype}")
            return t, False
        return self.to_dev(np.ascontiguousarray(t, dtype)), True

    def qu8_conv_tap_sums(self, w: DevBuf, out: Optional[DevBuf] = None) -> DevBuf:
        cout, kh, kw, cin = w.shape
        t = self._out(out, (cout, kh * kw), np.int32)
        self._ck(self.lib.osg_qu8_conv_tap_sums(self.ctx, w.ptr, cout, kh, kw, cin, t.ptr))
        return t

    def qu8_conv2d_nhwc(self, x: DevBuf, xq, w: DevBuf, wq, bias: Optional[DevBuf], oq, stride=1, pads=(1, 1, 1, 1), tap_sums: Optional[DevBuf] = None,
                        out: Optional[DevBuf] = None):
        n, h, wd, cin = x.shape
        cout, kh, kw, _ = w.shape
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        pt, pl, pb, pr = pads
        ho, wo = (h + pt + pb - kh) // sh + 1, (wd + pl + pr - kw) // sw + 1
        y = self._out(out, (n, ho, wo, cout), np.uint8)
        if tap_sums is not None:
            self._ck(self.lib.osg_qu8_conv2d_nhwc_t(self.ctx, x.ptr, float(xq[0]), int(xq[1]), w.ptr, float(wq[0]), int(wq[1]), self._p(bias), float(oq[0]), int(oq[1]),
                                                    y.ptr, n, h, wd, cin, cout, kh, kw, sh, sw, pt, pl, pb, pr, tap_sums.ptr))
            return y
        self._ck(self.lib.osg_qu8_conv2d_nhwc(self.ctx, x.ptr, float(xq[0]), int(xq[1]), w.ptr, float(wq[0]), int(wq[1]), self._p(bias), float(oq[0]), int(oq[1]),
                                              y.ptr, n, h, wd, cin, cout, kh, kw, sh, sw, pt, pl, pb, pr))
        return y

    def qu8_gemm(self, a: DevBuf, aq, b_nk: DevBuf, bq, bias: Optional[DevBuf], oq, out: Optional[DevBuf] = None, lda: Optional[int] = None,
                 stride_a: Optional[int] = None, stride_b: Optional[int] = None, stride_c: Optional[int] = None):
        """a:[(batch,)M,K], b_nk:[(batch,)N,K] codes.  lda: the row pitch of a (default K: dense) -- with lda > K or a batch stride beyond the dense one, `a`
        is the [(batch,)M,K] SHAPE of the operand and its buffer holds the pitched layout; stride_*: the batch strides in codes (defaults: dense, and 0 for a
        2-D b_nk).  With a stride_c of its own, out= is required and holds the strided layout (it is not checked against the dense shape)."""
        batch = a.shape[0] if len(a.shape) == 3 else 1
        m, k = a.shape[-2:]
        n = b_nk.shape[-2]
        lda = k if lda is None else int(lda)
        sa = (m * lda if batch > 1 else 0) if stride_a is None else int(stride_a)
        sb = (n * k if len(b_nk.shape) == 3 else 0) if stride_b is None else int(stride_b)
        if stride_c is None:
            sc = m * n if batch > 1 else 0
            c = self._out(out, a.shape[:-1] + (n,), np.uint8)
        else:
            sc = int(stride_c)
            if out is None or out.dtype != np.dtype(np.uint8) or out.size < (batch - 1) * sc + m * n:
                raise OsgError("qu8_gemm: a stride_c of its own needs an out= of at least (batch - 1) * stride_c + M * N codes")
            c = out
        self._ck(self.lib.osg_qu8_gemm(self.ctx, a.ptr, lda, float(aq[0]), int(aq[1]), b_nk.ptr, float(bq[0]), int(bq[1]), self._p(bias), float(oq[0]), int(oq[1]),
                                       c.ptr, m, n, k, batch, sa, sb, sc))
        return c

    def qu8_lut(self, x: DevBuf, lut, out: Optional[DevBuf] = None):
        """lut: 256 uint8 codes, a host array (uploaded for the call) or a DevBuf"""
        y = self._out(out, x.shape, np.uint8)
        t, owned = self._table(lut, np.uint8)
        self._ck(self.lib.osg_qu8_lut(self.ctx, x.ptr, y.ptr, x.size, t.ptr))
        if owned:
            self.sync()
            t.free()
        return y

    def qu8_binary(self, kind: str, a: DevBuf, aq, b: DevBuf, bq, oq, out: Optional[DevBuf] = None):
        rank = max(len(a.shape), len(b.shape))
        ash = (1,) * (rank - len(a.shape)) + a.shape
        bsh = (1,) * (rank - len(b.shape)) + b.shape
        y = self._out(out, tuple(np.broadcast_shapes(ash, bsh)), np.uint8)
        A = (ctypes.c_long * rank)(*ash)
        B = (ctypes.c_long * rank)(*bsh)
        self._ck(self.lib.osg_qu8_binary(self.ctx, BIN[kind], a.ptr, A, float(aq[0]), int(aq[1]), b.ptr, B, float(bq[0]), int(bq[1]), y.ptr, float(oq[0]), int(oq[1]), rank))
        return y

    def qu8_instance_norm(self, x: DevBuf, xq, scale: DevBuf, bias: DevBuf, eps: float, oq, out: Optional[DevBuf] = None):
        rows, L = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, np.uint8)
        self._ck(self.lib.osg_qu8_instance_norm(self.ctx, x.ptr, y.ptr, rows, L, scale.size, scale.ptr, bias.ptr, eps, float(xq[0]), int(xq[1]), float(oq[0]), int(oq[1])))
        return y

    def qu8_affine_act(self, x: DevBuf, xq, g: DevBuf, gq, mq, b: DevBuf, bq, aq, sig_lut: Optional[DevBuf], sq, oq, channels: int, inner: int = 1,
                       out: Optional[DevBuf] = None):
        """Mul(x, g[C]) -> Add(., b[C]) [-> Sigmoid -> Mul] in one pass; *q = (scale, zero point) of x, g, Mul out, b, Add out, Sigmoid out, final Mul out"""
        y = self._out(out, x.shape, np.uint8)
        self._ck(self.lib.osg_qu8_affine_act(self.ctx, x.ptr, float(xq[0]), int(xq[1]), g.ptr, float(gq[0]), int(gq[1]), float(mq[0]), int(mq[1]), b.ptr, float(bq[0]),
                                             int(bq[1]), float(aq[0]), int(aq[1]), self._p(sig_lut), float(sq[0]), int(sq[1]), float(oq[0]), int(oq[1]), y.ptr, x.size,
                                             channels, inner))
        return y

    def qu8_instance_norm_nhwc(self, x: DevBuf, groups: int, xq, scale: DevBuf, bias: DevBuf, eps: float, oq, out: Optional[DevBuf] = None):
        """x: [HW, C] codes (NHWC); rows of the normalisation = `groups` blocks of C/groups channels over every pixel"""
        hw, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, np.uint8)
        self._ck(self.lib.osg_qu8_instance_norm_nhwc(self.ctx, x.ptr, y.ptr, hw, c, groups, scale.size, scale.ptr, bias.ptr, eps, float(xq[0]), int(xq[1]), float(oq[0]), int(oq[1])))
        return y

    def qu8_norm_affine_act_nhwc(self, x: DevBuf, groups: int, xq, scale: DevBuf, bias: DevBuf, eps: float, nq, g: DevBuf, gq, mq, b: DevBuf, bq, aq, sig_lut: Optional[DevBuf], sq, oq,
                                 out: Optional[DevBuf] = None):
        """qu8_instance_norm_nhwc followed by qu8_affine_act, the normalisation's per-group table applied inside the affine pass"""
        hw, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, np.uint8)
        self._ck(self.lib.osg_qu8_norm_affine_act_nhwc(self.ctx, x.ptr, hw, c, groups, scale.size, scale.ptr, bias.ptr, eps, float(xq[0]), int(xq[1]), float(nq[0]), int(nq[1]),
                                                       g.ptr, float(gq[0]), int(gq[1]), float(mq[0]), int(mq[1]), b.ptr, float(bq[0]), int(bq[1]), float(aq[0]), int(aq[1]),
                                                       self._p(sig_lut), float(sq[0]), int(sq[1]), float(oq[0]), int(oq[1]), y.ptr))
        return y

    def qu8_softmax_last(self, x: DevBuf, lut_u32, out: Optional[DevBuf] = None):
        """lut_u32: the 256 uint32 entries of XNNPACK's exp table, a host array (uploaded for the call) or a DevBuf"""
        rows, c = int(np.prod(x.shape[:-1])), x.shape[-1]
        y = self._out(out, x.shape, np.uint8)
        t, owned = self._table(lut_u32, np.uint32)
        self._ck(self.lib.osg_qu8_softmax_last(self.ctx, x.ptr, y.ptr, rows, c, t.ptr))
        if owned:
            self.sync()
            t.free()
        return y
