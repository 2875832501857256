"""Python host binding of the C ABI (include/rspt_hip.h) in librspt_hip.so.

Mirrors the reference's operator interface for this path -- the i_signal_packer
factories and compress()/decompress() of lib_rspt/signal_packer.h:29-73 -- so
that tests read like the reference's own harness (lib_rspt_test/rspt_test.cpp:58-112).
torch is used only for device memory and streams in the batched, device-resident
calls; nothing here computes.  There is NO CPU fallback: if the HIP library or a
gfx950 device is missing every constructor raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

KIND_HZR, KIND_XDELTA_HZR, KIND_DCT, KIND_HADAMARD, KIND_BYTES = 0, 1, 2, 3, 4
KINDS = {"hzr": 0, "xdelta_hzr": 1, "dct": 2, "hadamard": 3, "bytes": 4}
DCT_FORCE_FFT = 0x100  # RSPT_HIP_DCT_FORCE_FFT (test hook, include/rspt_hip.h)

# every symbol include/rspt_hip.h declares (tests check the library exports them all)
C_ABI_SYMBOLS = [
    "rspt_hip_status_string", "rspt_hip_last_hip_error", "rspt_hip_device_count", "rspt_hip_packer_create",
    "rspt_hip_packer_destroy", "rspt_hip_compress", "rspt_hip_decompress", "rspt_hip_decompress_bounded", "rspt_hip_max_compressed_size",
    "rspt_hip_block_bytes", "rspt_hip_current_nb", "rspt_hip_set_nb", "rspt_hip_set_verify", "rspt_hip_reserve", "rspt_hip_compress_batch_dev",
    "rspt_hip_decompress_batch_dev", "rspt_hip_decompress_packed_dev", "rspt_hip_pack_bound", "rspt_hip_pack_batch_dev", "rspt_hip_stream", "rspt_hip_synchronize", "rspt_hip_set_profiling", "rspt_hip_stage_count",
    "rspt_hip_stage_name", "rspt_hip_stage_times", "rspt_hip_debug_read", "rspt_hip_iir_prefilter_batch_dev", "rspt_hip_fir_prefilter_batch_dev", "rspt_hip_median_filter_batch_dev", "rspt_hip_design_iir",
    "rspt_hip_iir_state_bytes", "rspt_hip_iir_prefilter_stream_dev", "rspt_hip_fir_state_bytes", "rspt_hip_fir_prefilter_stream_dev",
    "rspt_hip_iir_cascade_batch_dev", "rspt_hip_iir_cascade_state_bytes", "rspt_hip_iir_cascade_stream_dev",
    "rspt_hip_iir_zero_phase_work_bytes", "rspt_hip_iir_zero_phase_batch_dev",
    "rspt_hip_median_state_bytes", "rspt_hip_median_filter_stream_dev",
    "rspt_hip_peak_state_bytes", "rspt_hip_peak_detect_batch_dev", "rspt_hip_peak_offline_work_bytes", "rspt_hip_peak_detect_offline_batch_dev",
    "rspt_hip_prdn_batch_dev", "rspt_hip_native_to_i32_batch_dev", "rspt_hip_i32_to_native_batch_dev",
    "rspt_hip_set_byte_order", "rspt_hip_host_alloc", "rspt_hip_host_free",
    "rspt_hip_compress_many", "rspt_hip_decompress_many", "rspt_hip_gather_sizes", "rspt_hip_gather_payload", "rspt_hip_gather_containers",
    "rspt_hip_gather_post_sizes", "rspt_hip_gather_post_payload", "rspt_hip_gather_wait",
    "rspt_hip_hzr_max_compressed_size", "rspt_hip_hzr_verify_batch_dev",
    "rspt_hip_feed_begin", "rspt_hip_feed_push", "rspt_hip_feed_submit", "rspt_hip_feed_poll", "rspt_hip_feed_flush", "rspt_hip_feed_end",
]

_u8p = C.POINTER(C.c_uint8)
_szp = C.POINTER(C.c_size_t)
_lib = None


class RsptHipError(RuntimeError):
    def __init__(self, where, status, hip_error=0):
        self.status, self.hip_error = status, hip_error
        msg = lib().rspt_hip_status_string(status).decode() if _lib is not None else str(status)
        super().__init__("%s: %s (status %d, hipError %d)" % (where, msg, status, hip_error))


def lib():
    """Load librspt_hip.so.  A missing or stale library is rebuilt only where that is safe -- a single process with
    hipcc at hand; under a launcher (RANK set: the ranks of a torchrun job) a stale library is an error, never a
    concurrent compile.  Raises if the library cannot be had: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if os.environ.get("RSPT_HIP_LIB"):  # A/B timing of two builds in one session (tools/ab.sh); not a fallback
        path = os.environ["RSPT_HIP_LIB"]
    elif _build.stale():
        if "RANK" in os.environ:
            raise RuntimeError("rspt_amd: %s is missing or older than its sources; run `python __graft_entry__.py` (build()) "
                               "before launching ranks" % path)
        if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            path = _build.build()
        elif os.path.exists(path):  # built from other sources than the ones beside it, and no compiler to fix that: never run it silently
            raise RuntimeError("rspt_amd: %s does not match its sources (fingerprint %s) and there is no hipcc here to rebuild it"
                               % (path, _build.STAMP))
    if not os.path.exists(path):
        raise RuntimeError("rspt_amd: %s is missing and cannot be built here; there is no CPU fallback" % path)
    # One HIP runtime per process: torch ships its own libamdhip64 and the batch entry points take torch
    # tensors, so torch's copy has to be the one the loader binds first (a process that initialised
    # /opt/rocm's runtime before importing torch leaves torch without a visible device).
    import torch  # noqa: F401

    L = C.CDLL(path)
    L.rspt_hip_status_string.restype, L.rspt_hip_status_string.argtypes = C.c_char_p, [C.c_int]
    L.rspt_hip_last_hip_error.restype, L.rspt_hip_last_hip_error.argtypes = C.c_int, [C.c_void_p]
    L.rspt_hip_device_count.restype, L.rspt_hip_device_count.argtypes = C.c_int, []
    L.rspt_hip_packer_create.restype = C.c_int
    L.rspt_hip_packer_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    L.rspt_hip_packer_destroy.restype, L.rspt_hip_packer_destroy.argtypes = None, [C.c_void_p]
    L.rspt_hip_compress.restype, L.rspt_hip_compress.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_decompress.restype, L.rspt_hip_decompress.argtypes = C.c_int, [C.c_void_p, C.c_void_p, _szp, C.c_void_p]
    L.rspt_hip_decompress_bounded.restype, L.rspt_hip_decompress_bounded.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _szp, C.c_void_p]
    L.rspt_hip_compress_many.restype = C.c_int
    L.rspt_hip_compress_many.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_decompress_many.restype = C.c_int
    L.rspt_hip_decompress_many.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, _szp, C.c_size_t, C.c_void_p, _szp]
    L.rspt_hip_max_compressed_size.restype, L.rspt_hip_max_compressed_size.argtypes = C.c_size_t, [C.c_void_p]
    L.rspt_hip_block_bytes.restype, L.rspt_hip_block_bytes.argtypes = C.c_size_t, [C.c_void_p]
    L.rspt_hip_current_nb.restype, L.rspt_hip_current_nb.argtypes = C.c_uint, [C.c_void_p]
    L.rspt_hip_set_nb.restype, L.rspt_hip_set_nb.argtypes = C.c_int, [C.c_void_p, C.c_uint]
    L.rspt_hip_set_verify.restype, L.rspt_hip_set_verify.argtypes = C.c_int, [C.c_void_p, C.c_int]
    L.rspt_hip_reserve.restype, L.rspt_hip_reserve.argtypes = C.c_int, [C.c_void_p, C.c_size_t]
    L.rspt_hip_compress_batch_dev.restype = C.c_int
    L.rspt_hip_compress_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rspt_hip_decompress_batch_dev.restype = C.c_int
    L.rspt_hip_decompress_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_decompress_packed_dev.restype = C.c_int
    L.rspt_hip_decompress_packed_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_synchronize.restype, L.rspt_hip_synchronize.argtypes = C.c_int, [C.c_void_p]
    L.rspt_hip_stream.restype, L.rspt_hip_stream.argtypes = C.c_void_p, [C.c_void_p]
    L.rspt_hip_pack_bound.restype, L.rspt_hip_pack_bound.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t]
    L.rspt_hip_pack_batch_dev.restype = C.c_int
    L.rspt_hip_pack_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_set_profiling.restype, L.rspt_hip_set_profiling.argtypes = C.c_int, [C.c_void_p, C.c_int]
    L.rspt_hip_stage_count.restype, L.rspt_hip_stage_count.argtypes = C.c_int, [C.c_void_p]
    L.rspt_hip_stage_name.restype, L.rspt_hip_stage_name.argtypes = C.c_char_p, [C.c_void_p, C.c_int]
    L.rspt_hip_stage_times.restype, L.rspt_hip_stage_times.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    L.rspt_hip_debug_read.restype, L.rspt_hip_debug_read.argtypes = C.c_longlong, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.rspt_hip_set_byte_order.restype, L.rspt_hip_set_byte_order.argtypes = C.c_int, [C.c_void_p, C.c_int]
    L.rspt_hip_host_alloc.restype, L.rspt_hip_host_alloc.argtypes = C.c_void_p, [C.c_size_t]
    L.rspt_hip_host_free.restype, L.rspt_hip_host_free.argtypes = None, [C.c_void_p]
    L.rspt_hip_iir_prefilter_batch_dev.restype = C.c_int
    L.rspt_hip_iir_prefilter_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t, C.c_int,
                                                   C.c_int, C.c_void_p]
    L.rspt_hip_iir_state_bytes.restype, L.rspt_hip_iir_state_bytes.argtypes = C.c_int, [C.c_void_p, _szp]
    L.rspt_hip_iir_prefilter_stream_dev.restype = C.c_int
    L.rspt_hip_iir_prefilter_stream_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t, C.c_int,
                                                    C.c_void_p, C.c_void_p]
    _casc = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), _u8p]
    L.rspt_hip_iir_cascade_batch_dev.restype, L.rspt_hip_iir_cascade_batch_dev.argtypes = C.c_int, _casc + [C.c_void_p]
    L.rspt_hip_iir_cascade_state_bytes.restype, L.rspt_hip_iir_cascade_state_bytes.argtypes = C.c_int, [C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_iir_cascade_stream_dev.restype, L.rspt_hip_iir_cascade_stream_dev.argtypes = C.c_int, _casc + [C.c_void_p, C.c_void_p]
    L.rspt_hip_iir_zero_phase_work_bytes.restype, L.rspt_hip_iir_zero_phase_work_bytes.argtypes = C.c_int, [C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_iir_zero_phase_batch_dev.restype = C.c_int
    L.rspt_hip_iir_zero_phase_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.rspt_hip_fir_state_bytes.restype, L.rspt_hip_fir_state_bytes.argtypes = C.c_int, [C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_fir_prefilter_stream_dev.restype = C.c_int
    L.rspt_hip_fir_prefilter_stream_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.c_void_p, C.c_void_p]
    L.rspt_hip_fir_prefilter_batch_dev.restype = C.c_int
    L.rspt_hip_fir_prefilter_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_size_t, C.c_void_p]
    L.rspt_hip_median_filter_batch_dev.restype = C.c_int
    L.rspt_hip_median_filter_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.rspt_hip_median_state_bytes.restype, L.rspt_hip_median_state_bytes.argtypes = C.c_int, [C.c_void_p, C.c_size_t, _szp]
    L.rspt_hip_median_filter_stream_dev.restype = C.c_int
    L.rspt_hip_median_filter_stream_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rspt_hip_design_iir.restype = C.c_int
    L.rspt_hip_design_iir.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), _szp]
    L.rspt_hip_peak_state_bytes.restype, L.rspt_hip_peak_state_bytes.argtypes = C.c_int, [C.c_void_p, _szp]
    L.rspt_hip_peak_detect_batch_dev.restype = C.c_int
    L.rspt_hip_peak_detect_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_peak_offline_work_bytes.restype = C.c_int
    L.rspt_hip_peak_offline_work_bytes.argtypes = [C.c_void_p, C.c_size_t, C.c_int, _szp]
    L.rspt_hip_peak_detect_offline_batch_dev.restype = C.c_int
    L.rspt_hip_peak_detect_offline_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_prdn_batch_dev.restype = C.c_int
    L.rspt_hip_prdn_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rspt_hip_native_to_i32_batch_dev.restype = C.c_int
    L.rspt_hip_native_to_i32_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.rspt_hip_i32_to_native_batch_dev.restype = C.c_int
    L.rspt_hip_i32_to_native_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.rspt_hip_hzr_max_compressed_size.restype, L.rspt_hip_hzr_max_compressed_size.argtypes = C.c_size_t, [C.c_size_t]
    L.rspt_hip_hzr_verify_batch_dev.restype = C.c_int
    L.rspt_hip_hzr_verify_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rspt_hip_feed_begin.restype, L.rspt_hip_feed_begin.argtypes = C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t]
    L.rspt_hip_feed_push.restype, L.rspt_hip_feed_push.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rspt_hip_feed_submit.restype, L.rspt_hip_feed_submit.argtypes = C.c_int, [C.c_void_p]
    L.rspt_hip_feed_poll.restype, L.rspt_hip_feed_poll.argtypes = C.c_int, [C.c_void_p, _szp, _szp, C.POINTER(C.c_int)]
    L.rspt_hip_feed_flush.restype, L.rspt_hip_feed_flush.argtypes = C.c_int, [C.c_void_p]
    L.rspt_hip_feed_end.restype, L.rspt_hip_feed_end.argtypes = C.c_int, [C.c_void_p]
    # the C++ factories behind the same library (include/signal_packer.h), via their C shim
    L.rspt_cxx_new.restype, L.rspt_cxx_new.argtypes = C.c_void_p, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.rspt_cxx_delete.restype, L.rspt_cxx_delete.argtypes = None, [C.c_int, C.c_void_p]
    L.rspt_cxx_compress.restype, L.rspt_cxx_compress.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _szp]
    L.rspt_cxx_decompress.restype, L.rspt_cxx_decompress.argtypes = C.c_int, [C.c_void_p, C.c_void_p, _szp, C.c_void_p]
    L.rspt_cxx_set_device.restype, L.rspt_cxx_set_device.argtypes = C.c_int, [C.c_int]
    _lib = L
    return L


def _as_u8(buf):
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
    return np.ascontiguousarray(a)


class SignalPacker:
    """One i_signal_packer instance on one GPU."""

    def __init__(self, kind, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode=3, device=0):
        self._L = lib()
        kind_flags = KINDS[kind] if isinstance(kind, str) else int(kind)
        self.kind = kind_flags & 0xFF
        self.bps, self.nch, self.ns = bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel
        h = C.c_void_p()
        rc = self._L.rspt_hip_packer_create(C.byref(h), kind_flags, self.bps, self.nch, self.ns, nr_bytes_to_encode, device)
        if rc != 0:
            raise RsptHipError("rspt_hip_packer_create", rc)
        self._h = h
        self.block_bytes = self._L.rspt_hip_block_bytes(h)
        self.max_compressed_size = self._L.rspt_hip_max_compressed_size(h)

    def _check(self, where, rc):
        if rc != 0:
            raise RsptHipError(where, rc, self._L.rspt_hip_last_hip_error(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.rspt_hip_packer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- i_signal_packer::compress / decompress (host buffers) ----------------
    def compress(self, src, dst_max_len=None):
        a = _as_u8(src)
        assert a.size == self.block_bytes, (a.size, self.block_bytes)
        cap = dst_max_len if dst_max_len is not None else 2 * self.block_bytes + 4096
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._check("rspt_hip_compress", self._L.rspt_hip_compress(self._h, a.ctypes.data, out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].tobytes()

    def compress_into(self, src, out):
        """host buffers as they are (numpy uint8 arrays, e.g. from host_alloc): -> stream length"""
        n = C.c_size_t(0)
        self._check("rspt_hip_compress", self._L.rspt_hip_compress(self._h, src.ctypes.data, out.ctypes.data, out.size, C.byref(n)))
        return n.value

    def compress_many(self, src, out, raise_on_small=True):
        """a sequence of blocks from host memory through the upload | compress | download pipeline (rspt_hip_compress_many):
        src = uint8 array of n * block_bytes, out = uint8 array [n, stride] -> array of the n stream lengths"""
        n = src.size // self.block_bytes
        assert src.size == n * self.block_bytes and out.ndim == 2 and out.shape[0] == n
        lens = (C.c_size_t * n)()
        rc = self._L.rspt_hip_compress_many(self._h, src.ctypes.data, n, out.ctypes.data, out.strides[0], lens)
        if rc != -5 or raise_on_small:  # RSPT_HIP_ERR_DST_TOO_SMALL: the lengths say which streams
            self._check("rspt_hip_compress_many", rc)
        return np.array(lens[:], dtype=np.int64)

    # -- a feed of blocks that arrive over time (rspt_hip_feed_*): push when a block is there, poll for finished streams ----
    def feed_begin(self, blocks_per_launch=1, slots=3):
        self._check("rspt_hip_feed_begin", self._L.rspt_hip_feed_begin(self._h, blocks_per_launch, slots))

    def feed_push(self, src, dst):
        """queue one block (uint8 arrays that stay alive until the block is polled); False: the ring is full, poll first"""
        rc = self._L.rspt_hip_feed_push(self._h, src.ctypes.data, dst.ctypes.data, dst.size)
        if rc == -8:  # RSPT_HIP_ERR_BUSY
            return False
        self._check("rspt_hip_feed_push", rc)
        return True

    def feed_submit(self):
        self._check("rspt_hip_feed_submit", self._L.rspt_hip_feed_submit(self._h))

    def feed_poll(self):
        """-> (seq, length, status) of one finished block in push order, or None when none is ready (never waits)"""
        seq, n, st = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        rc = self._L.rspt_hip_feed_poll(self._h, C.byref(seq), C.byref(n), C.byref(st))
        if rc == 0:
            return None
        if rc != 1:
            self._check("rspt_hip_feed_poll", rc)
        return seq.value, n.value, st.value

    def feed_flush(self):
        self._check("rspt_hip_feed_flush", self._L.rspt_hip_feed_flush(self._h))

    def feed_end(self):
        self._check("rspt_hip_feed_end", self._L.rspt_hip_feed_end(self._h))

    def decompress_many(self, streams, out, lengths=None):
        """streams = uint8 array [n, stride] (one stream per row), out = uint8 array of n * block_bytes -> bytes consumed per stream
        (rspt_hip_decompress_many: upload | decode | download pipeline); lengths (optional): what to upload of each stream"""
        n = streams.shape[0]
        assert streams.ndim == 2 and out.size == n * self.block_bytes
        used = (C.c_size_t * n)()
        lens = (C.c_size_t * n)(*[int(v) for v in lengths]) if lengths is not None else None
        self._check("rspt_hip_decompress_many",
                    self._L.rspt_hip_decompress_many(self._h, streams.ctypes.data, streams.strides[0], lens, n, out.ctypes.data, used))
        return np.array(used[:], dtype=np.int64)

    def decompress_into(self, stream, out):
        n = C.c_size_t(0)
        self._check("rspt_hip_decompress", self._L.rspt_hip_decompress(self._h, stream.ctypes.data, C.byref(n), out.ctypes.data))
        return n.value

    def decompress(self, stream, bounded=False):
        """bounded: rspt_hip_decompress_bounded with the length of `stream` (for streams that may be damaged)"""
        s = _as_u8(stream)
        out = np.empty(self.block_bytes, dtype=np.uint8)
        n = C.c_size_t(0)
        if bounded:
            self._check("rspt_hip_decompress_bounded", self._L.rspt_hip_decompress_bounded(self._h, s.ctypes.data, s.size, C.byref(n), out.ctypes.data))
        else:
            self._check("rspt_hip_decompress", self._L.rspt_hip_decompress(self._h, s.ctypes.data, C.byref(n), out.ctypes.data))
        return out.tobytes(), n.value

    @property
    def nb(self):
        return self._L.rspt_hip_current_nb(self._h)

    def set_nb(self, nb):
        self._check("rspt_hip_set_nb", self._L.rspt_hip_set_nb(self._h, nb))

    def set_byte_order(self, big_endian=True):
        """samples arrive (compress) and leave (decompress) with their bytes reversed (utils.cpp reverse_byte_order branches)"""
        self._check("rspt_hip_set_byte_order", self._L.rspt_hip_set_byte_order(self._h, int(bool(big_endian))))

    def set_verify(self, on=True):
        """check every block's CRC-32C on decompress (hzr_verify's job in the reference); off by default"""
        self._check("rspt_hip_set_verify", self._L.rspt_hip_set_verify(self._h, int(bool(on))))

    # -- device-resident batches (torch tensors carry the memory) --------------
    def reserve(self, nblocks):
        self._check("rspt_hip_reserve", self._L.rspt_hip_reserve(self._h, nblocks))

    def compress_batch(self, d_src, d_dst=None, d_sizes=None, dst_stride=None, stream=None):
        """d_src: uint8 cuda tensor [nblocks, block_bytes].  Returns (d_dst, d_sizes);
        asynchronous on `stream` (default: torch's current stream)."""
        import torch

        assert d_src.is_cuda and d_src.dtype == torch.uint8 and d_src.is_contiguous()
        nblocks = d_src.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_src.numel()
        if dst_stride is None:
            dst_stride = (self.max_compressed_size + 255) // 256 * 256 if d_dst is None else d_dst.numel() // nblocks
        if d_dst is None:
            d_dst = torch.empty((nblocks, dst_stride), dtype=torch.uint8, device=d_src.device)
        if d_sizes is None:
            d_sizes = torch.empty(nblocks, dtype=torch.int64, device=d_src.device)
        st = stream if stream is not None else torch.cuda.current_stream(d_src.device).cuda_stream
        rc = self._L.rspt_hip_compress_batch_dev(self._h, d_src.data_ptr(), nblocks, d_dst.data_ptr(), dst_stride, d_sizes.data_ptr(), st)
        self._check("rspt_hip_compress_batch_dev", rc)
        return d_dst, d_sizes

    def decompress_batch(self, d_streams, nblocks, src_stride, d_out=None, d_consumed=None, stream=None):
        import torch

        if d_out is None:
            d_out = torch.empty((nblocks, self.block_bytes), dtype=torch.uint8, device=d_streams.device)
        if d_consumed is None:
            d_consumed = torch.empty(nblocks, dtype=torch.int64, device=d_streams.device)
        st = stream if stream is not None else torch.cuda.current_stream(d_streams.device).cuda_stream
        rc = self._L.rspt_hip_decompress_batch_dev(self._h, d_streams.data_ptr(), src_stride, nblocks, d_out.data_ptr(), d_consumed.data_ptr(), st)
        self._check("rspt_hip_decompress_batch_dev", rc)
        return d_out, d_consumed

    def decompress_packed(self, d_packed, d_out=None, d_consumed=None, stream=None, nbytes=None):
        """Decompress every stream of a container (what pack_batch / the multi-GPU gather produce) on the device.
        Each stream is decoded with the nb of its own index entry.  Reads the 32-byte header to the host for the block
        count (a synchronisation).  `nbytes`: container length if shorter than the tensor."""
        import torch

        head = d_packed[:32].cpu().numpy().view(np.uint64)
        if int(head[0]) != 0x4B43415054505352:
            raise ValueError("not an RSPTPACK container")
        nblocks = int(head[1])
        plen = int(nbytes) if nbytes is not None else d_packed.numel()
        if nblocks == 0 or nblocks > 65535 or plen < 32 or nblocks > (plen - 32) // 16:  # (nothing is sized from an untrusted count)
            raise RsptHipError("rspt_hip_decompress_packed_dev", -6 if 0 < nblocks <= 65535 else -1)
        if d_out is None:
            d_out = torch.empty((nblocks, self.block_bytes), dtype=torch.uint8, device=d_packed.device)
        if d_consumed is None:
            d_consumed = torch.empty(nblocks, dtype=torch.int64, device=d_packed.device)
        st = stream if stream is not None else torch.cuda.current_stream(d_packed.device).cuda_stream
        rc = self._L.rspt_hip_decompress_packed_dev(self._h, d_packed.data_ptr(), plen, nblocks, d_out.data_ptr(), d_consumed.data_ptr(), st)
        self._check("rspt_hip_decompress_packed_dev", rc)
        return d_out, d_consumed

    def hzr_verify_batch(self, d_streams, d_lengths, src_stride=None, d_decoded=None, stream=None):
        """hzr_verify of device-resident libhzr streams without decoding them (rspt_hip_hzr_verify_batch_dev; a `bytes` handle):
        d_streams = uint8 cuda tensor, stream b at b * src_stride (default: the row length of a 2-d tensor), d_lengths = int64 cuda
        tensor of their lengths -> d_decoded (int64: the size each master header names; negative = bit 63 = rejected)."""
        import torch

        nblocks = d_lengths.numel()
        if src_stride is None:
            src_stride = d_streams.numel() // nblocks
        assert d_streams.is_cuda and d_streams.dtype == torch.uint8 and d_streams.is_contiguous()
        assert d_lengths.is_cuda and d_lengths.dtype == torch.int64 and d_lengths.is_contiguous()
        if d_decoded is None:
            d_decoded = torch.empty(nblocks, dtype=torch.int64, device=d_streams.device)
        st = stream if stream is not None else torch.cuda.current_stream(d_streams.device).cuda_stream
        rc = self._L.rspt_hip_hzr_verify_batch_dev(self._h, d_streams.data_ptr(), src_stride, d_lengths.data_ptr(), nblocks, d_decoded.data_ptr(), st)
        self._check("rspt_hip_hzr_verify_batch_dev", rc)
        return d_decoded

    def pack_bound(self, nblocks):
        return self._L.rspt_hip_pack_bound(self._h, nblocks)

    def pack_batch(self, d_dst, d_sizes, d_packed=None, d_total=None, stream=None):
        """streams of a batch -> one container (layout: include/rspt_hip.h); asynchronous."""
        import torch

        nblocks = d_sizes.numel()
        stride = d_dst.numel() // nblocks
        if d_packed is None:
            d_packed = torch.empty(self.pack_bound(nblocks), dtype=torch.uint8, device=d_dst.device)
        if d_total is None:
            d_total = torch.zeros(1, dtype=torch.int64, device=d_dst.device)
        st = stream if stream is not None else torch.cuda.current_stream(d_dst.device).cuda_stream
        rc = self._L.rspt_hip_pack_batch_dev(self._h, d_dst.data_ptr(), stride, d_sizes.data_ptr(), nblocks, d_packed.data_ptr(), d_total.data_ptr(), st)
        self._check("rspt_hip_pack_batch_dev", rc)
        return d_packed, d_total

    def iir_state_bytes(self):
        n = C.c_size_t()
        self._check("rspt_hip_iir_state_bytes", self._L.rspt_hip_iir_state_bytes(self._h, C.byref(n)))
        return n.value

    def iir_state(self, device=None):
        """A zeroed state for iir_prefilter_batch(state=...): a fresh filter for every channel (uint8 device tensor)."""
        import torch

        return torch.zeros(self.iir_state_bytes(), dtype=torch.uint8, device=device if device is not None else "cuda")

    def fir_state_bytes(self, kernel_size):
        n = C.c_size_t()
        self._check("rspt_hip_fir_state_bytes", self._L.rspt_hip_fir_state_bytes(self._h, int(kernel_size), C.byref(n)))
        return n.value

    def fir_state(self, kernel_size, device=None):
        """A zeroed state for fir_prefilter_batch(state=...) with a kernel of kernel_size taps: a fresh filter for every channel."""
        import torch

        return torch.zeros(self.fir_state_bytes(kernel_size), dtype=torch.uint8, device=device if device is not None else "cuda")

    def iir_prefilter_batch(self, d_buf, n, d, init_nr_samples=2000, per_channel=False, stream=None, state=None):
        """The reference's pre-filter step (rspt_test.cpp:116-136) on device-resident blocks, in place; asynchronous.
        state: None, or an iir_state() tensor: the blocks are then consecutive pieces of one recording, one filter per channel
        running through them and on into the next call (rspt_hip_iir_prefilter_stream_dev); needs per_channel=True."""
        import torch

        assert d_buf.is_cuda and d_buf.dtype == torch.uint8 and d_buf.is_contiguous()
        nblocks = d_buf.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_buf.numel()
        nn, dd = np.ascontiguousarray(n, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        assert nn.size == dd.size
        st = stream if stream is not None else torch.cuda.current_stream(d_buf.device).cuda_stream
        if state is not None:
            if not per_channel:
                raise ValueError("iir_prefilter_batch: a carried state is one filter per channel (per_channel=True)")
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.iir_state_bytes()
            rc = self._L.rspt_hip_iir_prefilter_stream_dev(self._h, d_buf.data_ptr(), nblocks, nn.ctypes.data_as(C.POINTER(C.c_double)),
                                                           dd.ctypes.data_as(C.POINTER(C.c_double)), nn.size, init_nr_samples, state.data_ptr(), st)
            self._check("rspt_hip_iir_prefilter_stream_dev", rc)
            return d_buf
        rc = self._L.rspt_hip_iir_prefilter_batch_dev(self._h, d_buf.data_ptr(), nblocks, nn.ctypes.data_as(C.POINTER(C.c_double)),
                                                      dd.ctypes.data_as(C.POINTER(C.c_double)), nn.size, init_nr_samples, int(bool(per_channel)), st)
        self._check("rspt_hip_iir_prefilter_batch_dev", rc)
        return d_buf

    def iir_cascade_state_bytes(self, nsections):
        n = C.c_size_t()
        self._check("rspt_hip_iir_cascade_state_bytes", self._L.rspt_hip_iir_cascade_state_bytes(self._h, int(nsections), C.byref(n)))
        return n.value

    def iir_cascade_state(self, nsections, device=None):
        """A zeroed state for iir_cascade_batch(state=...) with nsections sections: a fresh chain for every channel."""
        import torch

        return torch.zeros(self.iir_cascade_state_bytes(nsections), dtype=torch.uint8, device=device if device is not None else "cuda")

    def iir_cascade_batch(self, d_buf, sections, stream=None, state=None):
        """1 to 4 reference IIR filters per channel, chained in double and truncated once (rspt_hip.h: rspt_hip_iir_cascade_batch_dev),
        on device-resident blocks, in place; asynchronous.  lp->filter_opt(hp->filter_opt(x)) is sections=[(hp_n, hp_d), (lp_n, lp_d, 0)].
        sections: a list of (n, d), (n, d, init_nr_samples) or (n, d, init_nr_samples, use_filter); init_nr_samples defaults to
        2000, use_filter (the section runs filter() instead of filter_opt()) to False.
        state: None (a fresh chain per block and channel), or an iir_cascade_state(len(sections)) tensor: the blocks are then
        consecutive pieces of one recording, one chain per channel running through them and on into the next call."""
        import torch

        assert d_buf.is_cuda and d_buf.dtype == torch.uint8 and d_buf.is_contiguous()
        nblocks = d_buf.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_buf.numel()
        S = len(sections)
        if not 1 <= S <= 4:
            raise ValueError("iir_cascade_batch: 1 to 4 sections")
        nn, dd = np.zeros((S, 5)), np.zeros((S, 5))
        nc, init, filt = np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.uint8)
        for k, sec in enumerate(sections):
            n, d = np.asarray(sec[0], dtype=np.float64).reshape(-1), np.asarray(sec[1], dtype=np.float64).reshape(-1)
            if n.size != d.size or not 2 <= n.size <= 5:
                raise ValueError("iir_cascade_batch: section %d needs 2 to 5 coefficients on each side" % k)
            nn[k, : n.size], dd[k, : d.size] = n, d
            nc[k], init[k], filt[k] = n.size, (sec[2] if len(sec) > 2 else 2000), bool(sec[3]) if len(sec) > 3 else False
        st = stream if stream is not None else torch.cuda.current_stream(d_buf.device).cuda_stream
        args = (self._h, d_buf.data_ptr(), nblocks, S, nn.ctypes.data_as(C.POINTER(C.c_double)), dd.ctypes.data_as(C.POINTER(C.c_double)),
                nc.ctypes.data_as(C.POINTER(C.c_uint32)), init.ctypes.data_as(C.POINTER(C.c_int32)), filt.ctypes.data_as(_u8p))
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.iir_cascade_state_bytes(S)
            self._check("rspt_hip_iir_cascade_stream_dev", self._L.rspt_hip_iir_cascade_stream_dev(*args, state.data_ptr(), st))
        else:
            self._check("rspt_hip_iir_cascade_batch_dev", self._L.rspt_hip_iir_cascade_batch_dev(*args, st))
        return d_buf

    def iir_zero_phase_work_bytes(self, nblocks):
        n = C.c_size_t()
        self._check("rspt_hip_iir_zero_phase_work_bytes", self._L.rspt_hip_iir_zero_phase_work_bytes(self._h, int(nblocks), C.byref(n)))
        return n.value

    def iir_zero_phase_batch(self, d_buf, n, d, init_nr_samples=2000, backward_init_nr_samples=0, work=None, stream=None):
        """Zero-phase (forward-backward) IIR filtering on device-resident blocks, in place; asynchronous.  One fresh reference
        filter per (block, channel) runs forward over the block and then, the same object, backward over its own untruncated
        output; the result is truncated once (rspt_hip.h: rspt_hip_iir_zero_phase_batch_dev).
        work: a device tensor of at least iir_zero_phase_work_bytes(nblocks) bytes, 8-byte aligned; None: allocated here."""
        import torch

        assert d_buf.is_cuda and d_buf.dtype == torch.uint8 and d_buf.is_contiguous()
        nblocks = d_buf.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_buf.numel()
        nn, dd = np.ascontiguousarray(n, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        assert nn.size == dd.size
        if work is None:
            work = torch.empty(max(1, (self.iir_zero_phase_work_bytes(max(nblocks, 1)) + 7) // 8), dtype=torch.float64, device=d_buf.device)
        assert work.is_cuda and work.is_contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(d_buf.device).cuda_stream
        rc = self._L.rspt_hip_iir_zero_phase_batch_dev(self._h, d_buf.data_ptr(), nblocks, nn.ctypes.data_as(C.POINTER(C.c_double)),
                                                       dd.ctypes.data_as(C.POINTER(C.c_double)), nn.size, int(init_nr_samples),
                                                       int(backward_init_nr_samples), work.data_ptr(), work.numel() * work.element_size(), st)
        self._check("rspt_hip_iir_zero_phase_batch_dev", rc)
        return d_buf

    def _window_call_buffers(self, d_src, d_dst, stream):
        """(nblocks, output, stream) of a windowed stage's call (fir_prefilter_batch, median_filter_batch): whole blocks of
        contiguous uint8 on the device, the output d_src itself when d_dst is None, the current stream when stream is None."""
        import torch

        assert d_src.is_cuda and d_src.dtype == torch.uint8 and d_src.is_contiguous()
        nblocks = d_src.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_src.numel()
        out = d_src if d_dst is None else d_dst
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == d_src.numel()
        st = stream if stream is not None else torch.cuda.current_stream(d_src.device).cuda_stream
        return nblocks, out, st

    def fir_prefilter_batch(self, d_src, kernel, d_dst=None, stream=None, state=None):
        """The reference's FIR pre-filter (i_filter::new_fir, init_history_values, filter_opt; rspt_hip.h) on device-resident
        blocks: in place when d_dst is None, else into d_dst (same size, not overlapping d_src); asynchronous.  Returns the output.
        state: None, or a fir_state(len(kernel)) tensor: the blocks are then consecutive pieces of one recording, one filter per
        channel running through them and on into the next call (rspt_hip_fir_prefilter_stream_dev)."""
        nblocks, out, st = self._window_call_buffers(d_src, d_dst, stream)
        k = np.ascontiguousarray(kernel, dtype=np.float64).reshape(-1)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.fir_state_bytes(k.size)
            rc = self._L.rspt_hip_fir_prefilter_stream_dev(self._h, d_src.data_ptr(), out.data_ptr(), nblocks, k.ctypes.data_as(C.POINTER(C.c_double)),
                                                           k.size, state.data_ptr(), st)
            self._check("rspt_hip_fir_prefilter_stream_dev", rc)
            return out
        rc = self._L.rspt_hip_fir_prefilter_batch_dev(self._h, d_src.data_ptr(), out.data_ptr(), nblocks, k.ctypes.data_as(C.POINTER(C.c_double)),
                                                      k.size, st)
        self._check("rspt_hip_fir_prefilter_batch_dev", rc)
        return out

    def median_state_bytes(self, window):
        n = C.c_size_t()
        self._check("rspt_hip_median_state_bytes", self._L.rspt_hip_median_state_bytes(self._h, int(window), C.byref(n)))
        return n.value

    def median_state(self, window, device=None):
        """A zeroed state for median_filter_batch(state=...) with this window: a fresh object for every channel."""
        import torch

        return torch.zeros(self.median_state_bytes(window), dtype=torch.uint8, device=device if device is not None else "cuda")

    def median_filter_batch(self, d_src, window, d_dst=None, stream=None, state=None):
        """The reference's rolling-window median (rolling_window_median<double>(window), one per channel; rspt_hip.h) on
        device-resident blocks: in place when d_dst is None, else into d_dst (same size, not overlapping d_src); asynchronous.
        Returns the output.
        state: None (a fresh object per channel of every block), or a median_state(window) tensor: the blocks are then
        consecutive pieces of one recording, one object per channel running through them and on into the next call
        (rspt_hip_median_filter_stream_dev); the window is then not clamped to ns."""
        nblocks, out, st = self._window_call_buffers(d_src, d_dst, stream)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.median_state_bytes(window)
            rc = self._L.rspt_hip_median_filter_stream_dev(self._h, d_src.data_ptr(), out.data_ptr(), nblocks, int(window), state.data_ptr(), st)
            self._check("rspt_hip_median_filter_stream_dev", rc)
            return out
        rc = self._L.rspt_hip_median_filter_batch_dev(self._h, d_src.data_ptr(), out.data_ptr(), nblocks, int(window), st)
        self._check("rspt_hip_median_filter_batch_dev", rc)
        return out

    def peak_state_bytes(self):
        n = C.c_size_t()
        self._check("rspt_hip_peak_state_bytes", self._L.rspt_hip_peak_state_bytes(self._h, C.byref(n)))
        return n.value

    def peak_state(self, device=None):
        """A zeroed state for peak_detect_batch(state=...): a fresh detector for every channel (uint8 device tensor)."""
        import torch

        return torch.zeros(self.peak_state_bytes(), dtype=torch.uint8, device=device if device is not None else "cuda")

    def _peak_call_buffers(self, d_src, max_peaks, state, traces, stream):
        """What both peak entries share: checks d_src (whole blocks of contiguous uint8 on the device) and state, allocates
        (count, index, value, sig, thr) -- sig and thr None without traces -- and picks the stream (the current one when None).
        -> (nblocks, outputs, stream, ptr); ptr(t): t's device pointer, None for None or an empty tensor."""
        import torch

        assert d_src.is_cuda and d_src.dtype == torch.uint8 and d_src.is_contiguous()
        nblocks = d_src.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_src.numel()
        dev = d_src.device
        count = torch.empty((nblocks, self.nch), dtype=torch.int32, device=dev)
        index = torch.empty((nblocks, self.nch, max_peaks), dtype=torch.int32, device=dev)
        value = torch.empty((nblocks, self.nch, max_peaks), dtype=torch.float64, device=dev)
        sig = thr = None
        if traces:
            sig = torch.empty((nblocks, self.ns, self.nch), dtype=torch.float64, device=dev)
            thr = torch.empty_like(sig)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.peak_state_bytes()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        return nblocks, (count, index, value, sig, thr), st, ptr

    def peak_detect_batch(self, d_src, variant="online", sampling_rate=None, marker_val=1.0, max_peaks=64, state=None, traces=False, stream=None):
        """The reference's R-peak detectors (peak_detector.h; rspt_hip.h: rspt_hip_peak_detect_batch_dev) on device-resident
        blocks, which are only read.  variant: "online" (peak_detector), "online_1st" (peak_detector_1st_order) or "offline_fw"
        (peak_detector_offline::detect_fw).  state: None for a fresh detector per (block, channel), or a peak_state() tensor that
        carries one detector per channel through the blocks and across calls (of one variant and sampling rate).  Asynchronous.
        Returns (count [nblocks, nch] int32, index [nblocks, nch, max_peaks] int32, value [nblocks, nch, max_peaks] float64) and,
        with traces, (sig, threshold) [nblocks, ns, nch] float64 as well."""
        if sampling_rate is None:
            raise ValueError("peak_detect_batch: sampling_rate is required")
        v = PEAK_VARIANTS[variant] if isinstance(variant, str) else int(variant)
        nblocks, out, st, ptr = self._peak_call_buffers(d_src, max_peaks, state, traces, stream)
        count, index, value, sig, thr = out
        rc = self._L.rspt_hip_peak_detect_batch_dev(self._h, d_src.data_ptr(), nblocks, v, float(sampling_rate), float(marker_val), ptr(state),
                                                    count.data_ptr(), ptr(index), ptr(value), max_peaks, ptr(sig), ptr(thr), st)
        self._check("rspt_hip_peak_detect_batch_dev", rc)
        return out if traces else out[:3]

    def peak_offline_work_bytes(self, nblocks, stateful=False):
        n = C.c_size_t()
        self._check("rspt_hip_peak_offline_work_bytes", self._L.rspt_hip_peak_offline_work_bytes(self._h, nblocks, int(bool(stateful)), C.byref(n)))
        return n.value

    def peak_detect_offline_batch(self, d_src, sampling_rate, marker_val=1.0, max_peaks=64, state=None, traces=False, stream=None):
        """The reference's zero-phase offline R-peak detector (peak_detector_offline::detect; rspt_hip.h:
        rspt_hip_peak_detect_offline_batch_dev) on device-resident blocks, which are only read.  state: None for a fresh object per
        (block, channel), or a peak_state() tensor carrying one object per channel through the blocks and across calls (it may
        alternate with peak_detect_batch(variant="offline_fw") calls at the same rate).  The workspace is allocated here.
        Asynchronous.  Returns what peak_detect_batch returns: (count, index, value) of the final peak_signal's non-zero entries
        and, with traces, (filt_signal, threshold_signal) [nblocks, ns, nch] float64 as well."""
        import torch

        nblocks, out, st, ptr = self._peak_call_buffers(d_src, max_peaks, state, traces, stream)
        count, index, value, sig, thr = out
        dev = d_src.device
        work = torch.empty(max(1, (self.peak_offline_work_bytes(max(nblocks, 1), state is not None) + 7) // 8), dtype=torch.float64, device=dev)
        rc = self._L.rspt_hip_peak_detect_offline_batch_dev(self._h, d_src.data_ptr(), nblocks, float(sampling_rate), float(marker_val), ptr(state),
                                                            work.data_ptr(), count.data_ptr(), ptr(index), ptr(value), max_peaks, ptr(sig), ptr(thr), st)
        self._check("rspt_hip_peak_detect_offline_batch_dev", rc)
        if stream is not None:  # (the workspace goes back to torch's pool only once the caller's stream is past this call)
            work.record_stream(torch.cuda.ExternalStream(stream, device=dev))
        return out if traces else out[:3]

    def prdn_batch(self, d_orig, d_dec, stream=None, parts=False):
        """The reference's quality figure PRDN[%] (rspt_test.cpp:98-111; rspt_hip.h: rspt_hip_prdn_batch_dev) of the decoded
        blocks d_dec against the originals d_orig, both device-resident in the native layout and only read; bit-identical with
        the reference.  Asynchronous.  Returns a float64 device tensor [nblocks]; with parts, (prdn, mse, ref, path): the two
        accumulators as the reference leaves them and, per block, 0 for the exact-integer path or 1 for the sequential one (int32)."""
        import torch

        for t in (d_orig, d_dec):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
        nblocks = d_orig.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_orig.numel() == d_dec.numel()
        dev = d_orig.device
        prdn = torch.empty(nblocks, dtype=torch.float64, device=dev)
        mse = ref = path = None
        if parts:
            mse, ref = torch.empty_like(prdn), torch.empty_like(prdn)
            path = torch.empty(nblocks, dtype=torch.int32, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        rc = self._L.rspt_hip_prdn_batch_dev(self._h, d_orig.data_ptr() if nblocks else None, d_dec.data_ptr() if nblocks else None, nblocks,
                                             prdn.data_ptr() if nblocks else None, ptr(mse), ptr(ref), ptr(path), st)
        self._check("rspt_hip_prdn_batch_dev", rc)
        return (prdn, mse, ref, path) if parts else prdn

    def to_planar_i32(self, d_src, d_out=None, stream=None):
        """The reference's convert_native_to_i32 (utils.cpp:123-191; rspt_hip.h: rspt_hip_native_to_i32_batch_dev) on
        device-resident blocks in the native layout (uint8, any alignment; the byte order of set_byte_order): every sample
        sign-extended from bps bytes.  Returns torch.int32 [nblocks, nch, ns].  Asynchronous."""
        import torch

        assert d_src.is_cuda and d_src.dtype == torch.uint8 and d_src.is_contiguous()
        nblocks = d_src.numel() // self.block_bytes
        assert nblocks * self.block_bytes == d_src.numel()
        if d_out is None:
            d_out = torch.empty((nblocks, self.nch, self.ns), dtype=torch.int32, device=d_src.device)
        assert d_out.is_cuda and d_out.dtype == torch.int32 and d_out.is_contiguous() and d_out.numel() == nblocks * self.nch * self.ns
        st = stream if stream is not None else torch.cuda.current_stream(d_src.device).cuda_stream
        rc = self._L.rspt_hip_native_to_i32_batch_dev(self._h, d_src.data_ptr() if nblocks else None, d_out.data_ptr() if nblocks else None, nblocks, st)
        self._check("rspt_hip_native_to_i32_batch_dev", rc)
        return d_out

    def from_planar_i32(self, d_planar, d_out=None, stream=None):
        """The reference's convert_i32_to_native (utils.cpp:51-121; rspt_hip.h: rspt_hip_i32_to_native_batch_dev): int32
        [nblocks, nch, ns] on the device -> the blocks in the native layout, the low bps bytes of every value kept (the byte order
        of set_byte_order).  Returns torch.uint8 [nblocks, block_bytes]; d_out may sit at any address.  Asynchronous."""
        import torch

        assert d_planar.is_cuda and d_planar.dtype == torch.int32 and d_planar.is_contiguous()
        nblocks = d_planar.numel() // (self.nch * self.ns)
        assert nblocks * self.nch * self.ns == d_planar.numel()
        if d_out is None:
            d_out = torch.empty((nblocks, self.block_bytes), dtype=torch.uint8, device=d_planar.device)
        assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() == nblocks * self.block_bytes
        st = stream if stream is not None else torch.cuda.current_stream(d_planar.device).cuda_stream
        rc = self._L.rspt_hip_i32_to_native_batch_dev(self._h, d_planar.data_ptr() if nblocks else None, d_out.data_ptr() if nblocks else None, nblocks, st)
        self._check("rspt_hip_i32_to_native_batch_dev", rc)
        return d_out

    def roundtrip_quality(self, d_src, stream=None):
        """The reference's test_packer_ (rspt_test.cpp:58-112) as one call: compress_batch -> decompress_batch -> prdn_batch on
        one stream with no host synchronisation in between.  Meant for the lossy kinds (dct, hadamard); works for any.  Returns
        (prdn, cr), float64 device tensors [nblocks]: PRDN[%] and the compression ratio block_bytes / compressed size as the
        reference prints it.  Asynchronous; a stream that did not decode shows in its cr (the consumed size carries bit 63)."""
        import torch

        nblocks = d_src.numel() // self.block_bytes
        d_dst, d_sizes = self.compress_batch(d_src, stream=stream)
        d_out, d_consumed = self.decompress_batch(d_dst, nblocks, d_dst.shape[1], stream=stream)
        prdn = self.prdn_batch(d_src.reshape(-1), d_out.reshape(-1), stream=stream)
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=d_src.device)) if stream is not None else None
        if ctx is not None:
            with ctx:
                cr = float(self.block_bytes) / d_consumed.to(torch.float64)
            for t in (d_dst, d_sizes, d_out, d_consumed):  # (back to torch's pool only once the caller's stream is past them)
                t.record_stream(torch.cuda.ExternalStream(stream, device=d_src.device))
        else:
            cr = float(self.block_bytes) / d_consumed.to(torch.float64)
        return prdn, cr

    def synchronize(self):
        self._check("rspt_hip_synchronize", self._L.rspt_hip_synchronize(self._h))

    @property
    def stream_ptr(self):
        """the handle's own hipStream_t (rspt_hip_stream): what the host-pointer entry points run on; a caller with several
        handles in flight can launch each handle's batches on it (torch.cuda.ExternalStream(pk.stream_ptr)) instead of making
        further streams -- the runtime maps streams onto few hardware queues (GPU_MAX_HW_QUEUES, default 4)"""
        return int(self._L.rspt_hip_stream(self._h) or 0)

    def debug_read(self, which, nbytes):
        """test hook: workspace buffer `which` of the last batch call (see rspt_hip.h)"""
        out = np.zeros(nbytes, dtype=np.uint8)
        n = self._L.rspt_hip_debug_read(self._h, which, out.ctypes.data, nbytes)
        if n < 0:
            raise RsptHipError("rspt_hip_debug_read", int(n))
        return out[:n]

    # -- measurement -------------------------------------------------------------
    def set_profiling(self, on=True):
        self._L.rspt_hip_set_profiling(self._h, int(on))

    def stage_times(self):
        n = self._L.rspt_hip_stage_count(self._h)
        ms = (C.c_float * n)()
        self._check("rspt_hip_stage_times", self._L.rspt_hip_stage_times(self._h, ms, n))
        return {self._L.rspt_hip_stage_name(self._h, i).decode(): float(ms[i]) for i in range(n)}


class HostBuffer:
    """page-locked host memory (rspt_hip_host_alloc) as a numpy uint8 array: `.a`"""

    def __init__(self, nbytes):
        self._L = lib()
        self._p = self._L.rspt_hip_host_alloc(nbytes)
        if not self._p:
            raise MemoryError("rspt_hip_host_alloc(%d)" % nbytes)
        self.a = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self._p))

    def close(self):
        if getattr(self, "_p", None):
            self.a = None
            self._L.rspt_hip_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# factory names of lib_rspt/signal_packer.h:59-69
FILTER_TYPES = {"high_pass": 0, "low_pass": 1, "band_pass": 2, "band_stop": 3}
PEAK_VARIANTS = {"online": 0, "online_1st": 1, "offline_fw": 2}


def design_iir(type, order, fs, lo, hi=0.0):
    """The reference's Butterworth designer (create_filter_iir; rspt_hip.h: rspt_hip_design_iir), bit-exact, on the host.
    type: "high_pass" / "low_pass" / "band_pass" / "band_stop" or 0..3; order 1 or 2; fs, lo, hi in Hz.  Returns (num, den)
    float64 arrays: num the feed-forward side, den (den[0] = 1) the feedback side.  Raises RsptHipError where the reference
    refuses the design.  To run the result as the IIR pre-filter, pass them crossed, as i_filter::new_iir(n, d) takes them:
        num, den = design_iir("band_pass", 2, 2000.0, 0.4, 200.0)
        packer.iir_prefilter_batch(buf, n=den, d=num)"""
    t = FILTER_TYPES[type] if isinstance(type, str) else int(type)
    num, den, n = np.zeros(5), np.zeros(5), C.c_size_t()
    rc = lib().rspt_hip_design_iir(t, int(order), float(fs), float(lo), float(hi), num.ctypes.data_as(C.POINTER(C.c_double)),
                                   den.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n))
    if rc != 0:
        raise RsptHipError("rspt_hip_design_iir", rc)
    return num[: n.value].copy(), den[: n.value].copy()


def new_xdelta_hzr(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode, device=0):
    return SignalPacker(KIND_XDELTA_HZR, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode, device)


def new_hzr(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0):
    return SignalPacker(KIND_HZR, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 4, device)


def new_dct(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0):
    return SignalPacker(KIND_DCT, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 2, device)


def new_bytes(nbytes, device=0):
    """libhzr on raw bytes (RSPT_HIP_KIND_BYTES): a handle for buffers of `nbytes` bytes; its streams are hzr_encode's"""
    return SignalPacker(KIND_BYTES, 1, 1, nbytes, 1, device)


def hzr_max_compressed_size(n):
    """hzr_max_compressed_size (host only: no device needed)"""
    return lib().rspt_hip_hzr_max_compressed_size(n)


def new_hadamard(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0):
    return SignalPacker(KIND_HADAMARD, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 3, device)


class CxxSignalPacker:
    """Drives the C++ i_signal_packer factories of include/signal_packer.h themselves
    (through the tiny C shim in signal_packer_hip.cpp) -- the reference-facing surface."""

    def __init__(self, kind, bps, nch, ns, nb=3):
        self._L = lib()
        self.kind = KINDS[kind] if isinstance(kind, str) else int(kind)
        self.block_bytes = bps * nch * ns
        self._p = self._L.rspt_cxx_new(self.kind, bps, nch, ns, nb)
        if not self._p:
            raise RuntimeError("i_signal_packer factory failed")

    def close(self):
        if getattr(self, "_p", None):
            self._L.rspt_cxx_delete(self.kind, self._p)
            self._p = None

    def compress(self, src):
        a = _as_u8(src)
        cap = 2 * self.block_bytes + 4096
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._L.rspt_cxx_compress(self._p, a.ctypes.data, out.ctypes.data, cap, C.byref(n))
        return out[: n.value].tobytes()

    def decompress(self, stream):
        s = _as_u8(stream)
        out = np.empty(self.block_bytes, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = self._L.rspt_cxx_decompress(self._p, s.ctypes.data, C.byref(n), out.ctypes.data)
        return out.tobytes(), n.value, rc
