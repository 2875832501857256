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

_p, _i, _u, _z, _d = C.c_void_p, C.c_int, C.c_uint, C.c_size_t, C.c_double
_dp, _u8p, _szp = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)
_casc = [_p, _p, _z, _z, _dp, _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), _u8p]  # what both cascade entries start with

# The C ABI, stated once: every function include/rspt_hip.h declares -> (restype, argtypes).  bind() applies it to a loaded
# library and tests/test_cabi.py holds it against the header's text.  A handle, a device pointer, a stream and a host buffer
# taken as an address are all c_void_p; the typed pointers are the ones callers hand ctypes arrays or byref() values to.
C_ABI = {
    "rspt_hip_status_string": (C.c_char_p, [_i]),
    "rspt_hip_last_hip_error": (_i, [_p]),
    "rspt_hip_device_count": (_i, []),
    "rspt_hip_packer_create": (_i, [C.POINTER(_p), _i, _z, _z, _z, _z, _i]),
    "rspt_hip_packer_destroy": (None, [_p]),
    "rspt_hip_compress": (_i, [_p, _p, _p, _z, _szp]),
    "rspt_hip_decompress": (_i, [_p, _p, _szp, _p]),
    "rspt_hip_decompress_bounded": (_i, [_p, _p, _z, _szp, _p]),
    "rspt_hip_max_compressed_size": (_z, [_p]),
    "rspt_hip_block_bytes": (_z, [_p]),
    "rspt_hip_hzr_max_compressed_size": (_z, [_z]),
    "rspt_hip_current_nb": (_u, [_p]),
    "rspt_hip_set_nb": (_i, [_p, _u]),
    "rspt_hip_set_quantizer": (_i, [_p, _d, _u]),
    "rspt_hip_get_quantizer": (_i, [_p, _dp, _p]),
    "rspt_hip_set_verify": (_i, [_p, _i]),
    "rspt_hip_set_byte_order": (_i, [_p, _i]),
    "rspt_hip_host_alloc": (_p, [_z]),
    "rspt_hip_host_free": (None, [_p]),
    "rspt_hip_compress_many": (_i, [_p, _p, _z, _p, _z, _szp]),
    "rspt_hip_decompress_many": (_i, [_p, _p, _z, _szp, _z, _p, _szp]),
    "rspt_hip_feed_begin": (_i, [_p, _z, _z]),
    "rspt_hip_feed_push": (_i, [_p, _p, _p, _z]),
    "rspt_hip_feed_submit": (_i, [_p]),
    "rspt_hip_feed_poll": (_i, [_p, _szp, _szp, C.POINTER(_i)]),
    "rspt_hip_feed_flush": (_i, [_p]),
    "rspt_hip_feed_end": (_i, [_p]),
    "rspt_hip_reserve": (_i, [_p, _z]),
    "rspt_hip_compress_batch_dev": (_i, [_p, _p, _z, _p, _z, _p, _p]),
    "rspt_hip_decompress_batch_dev": (_i, [_p, _p, _z, _z, _p, _p, _p]),
    "rspt_hip_compress_batch_ladder_dev": (_i, [_p, _p, _z, _dp, _z, _p, _p, _z, _p, _p]),
    "rspt_hip_decompress_batch_ladder_dev": (_i, [_p, _p, _z, _z, _dp, _z, _p, _p, _p, _p]),
    "rspt_hip_compress_target_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_target_batch_dev": (_i, [_p, _p, _z, _dp, _z, _d, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_debug_set_target_route": (_i, [_p, _i]),
    "rspt_hip_compress_budget_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_budget_batch_dev": (_i, [_p, _p, _z, _dp, _z, _z, _p, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_debug_set_budget_route": (_i, [_p, _i]),
    "rspt_hip_compress_total_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_total_batch_dev": (_i, [_p, _p, _z, _dp, _z, _z, _p, _z, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "rspt_hip_debug_set_total_route": (_i, [_p, _i]),
    "rspt_hip_compress_planar_batch_dev": (_i, [_p, _p, _z, _p, _z, _p, _p]),
    "rspt_hip_decompress_planar_batch_dev": (_i, [_p, _p, _z, _z, _p, _p, _p]),
    "rspt_hip_decompress_packed_planar_dev": (_i, [_p, _p, _z, _z, _p, _p, _p]),
    "rspt_hip_compress_planar_batch_ladder_dev": (_i, [_p, _p, _z, _dp, _z, _p, _p, _z, _p, _p]),
    "rspt_hip_decompress_planar_batch_ladder_dev": (_i, [_p, _p, _z, _z, _dp, _z, _p, _p, _p, _p]),
    "rspt_hip_compress_target_planar_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_target_planar_batch_dev": (_i, [_p, _p, _z, _dp, _z, _d, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_compress_budget_planar_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_budget_planar_batch_dev": (_i, [_p, _p, _z, _dp, _z, _z, _p, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_compress_total_planar_work_bytes": (_i, [_p, _z, _z, _szp]),
    "rspt_hip_compress_total_planar_batch_dev": (_i, [_p, _p, _z, _dp, _z, _z, _p, _z, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "rspt_hip_hzr_verify_batch_dev": (_i, [_p, _p, _z, _p, _z, _p, _p]),
    "rspt_hip_pack_bound": (_z, [_p, _z]),
    "rspt_hip_pack_batch_dev": (_i, [_p, _p, _z, _p, _z, _p, _p, _p]),
    "rspt_hip_decompress_packed_dev": (_i, [_p, _p, _z, _z, _p, _p, _p]),
    "rspt_hip_pack_batch_choice_dev": (_i, [_p, _p, _z, _p, _z, _p, _z, _p, _p, _p]),
    "rspt_hip_decompress_packed_ladder_dev": (_i, [_p, _p, _z, _z, _dp, _z, _p, _p, _p]),
    "rspt_hip_decompress_packed_planar_ladder_dev": (_i, [_p, _p, _z, _z, _dp, _z, _p, _p, _p]),
    "rspt_hip_gather_sizes": (_i, [_p, _p, _i, _p, _p, _p, _p]),
    "rspt_hip_gather_payload": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _z, _p]),
    "rspt_hip_gather_containers": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _z, _p, _p]),
    "rspt_hip_gather_post_sizes": (_i, [_p, _p, _i, _p, _i, _p]),
    "rspt_hip_gather_post_payload": (_i, [_p, _p, _i, _i, _i, _p, _i, _p, _z, _p]),
    "rspt_hip_gather_wait": (_i, [_p, _i, _p]),
    "rspt_hip_iir_prefilter_batch_dev": (_i, [_p, _p, _z, _dp, _dp, _z, _i, _i, _p]),
    "rspt_hip_iir_state_bytes": (_i, [_p, _szp]),
    "rspt_hip_iir_prefilter_stream_dev": (_i, [_p, _p, _z, _dp, _dp, _z, _i, _p, _p]),
    "rspt_hip_iir_cascade_batch_dev": (_i, _casc + [_p]),
    "rspt_hip_iir_cascade_state_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_iir_cascade_stream_dev": (_i, _casc + [_p, _p]),
    "rspt_hip_iir_prefilter_planar_batch_dev": (_i, [_p, _p, _z, _dp, _dp, _z, _i, _i, _p]),
    "rspt_hip_iir_prefilter_planar_stream_dev": (_i, [_p, _p, _z, _dp, _dp, _z, _i, _p, _p]),
    "rspt_hip_iir_cascade_planar_batch_dev": (_i, _casc + [_p]),
    "rspt_hip_iir_cascade_planar_stream_dev": (_i, _casc + [_p, _p]),
    "rspt_hip_iir_zero_phase_work_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_iir_zero_phase_batch_dev": (_i, [_p, _p, _z, _dp, _dp, _z, _i, _i, _p, _z, _p]),
    "rspt_hip_iir_zero_phase_planar_batch_dev": (_i, [_p, _p, _p, _z, _dp, _dp, _z, _i, _i, _p, _z, _p]),
    "rspt_hip_fir_prefilter_batch_dev": (_i, [_p, _p, _p, _z, _dp, _z, _p]),
    "rspt_hip_fir_state_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_fir_prefilter_stream_dev": (_i, [_p, _p, _p, _z, _dp, _z, _p, _p]),
    "rspt_hip_fir_prefilter_planar_batch_dev": (_i, [_p, _p, _p, _z, _dp, _z, _p]),
    "rspt_hip_fir_planar_state_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_fir_prefilter_planar_stream_dev": (_i, [_p, _p, _p, _z, _dp, _z, _p, _p]),
    "rspt_hip_median_filter_batch_dev": (_i, [_p, _p, _p, _z, _z, _p]),
    "rspt_hip_median_state_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_median_filter_stream_dev": (_i, [_p, _p, _p, _z, _z, _p, _p]),
    "rspt_hip_median_filter_planar_batch_dev": (_i, [_p, _p, _p, _z, _z, _p]),
    "rspt_hip_median_planar_state_bytes": (_i, [_p, _z, _szp]),
    "rspt_hip_median_filter_planar_stream_dev": (_i, [_p, _p, _p, _z, _z, _p, _p]),
    "rspt_hip_design_iir": (_i, [_i, _i, _d, _d, _d, _dp, _dp, _szp]),
    "rspt_hip_peak_state_bytes": (_i, [_p, _szp]),
    "rspt_hip_peak_detect_batch_dev": (_i, [_p, _p, _z, _i, _d, _d, _p, _p, _p, _p, _z, _p, _p, _p]),
    "rspt_hip_peak_offline_work_bytes": (_i, [_p, _z, _i, _szp]),
    "rspt_hip_peak_detect_offline_batch_dev": (_i, [_p, _p, _z, _d, _d, _p, _p, _p, _p, _p, _z, _p, _p, _p]),
    "rspt_hip_peak_detect_planar_batch_dev": (_i, [_p, _p, _z, _i, _d, _d, _p, _p, _p, _p, _z, _p, _p, _p]),
    "rspt_hip_peak_detect_offline_planar_batch_dev": (_i, [_p, _p, _z, _d, _d, _p, _p, _p, _p, _p, _z, _p, _p, _p]),
    "rspt_hip_prdn_batch_dev": (_i, [_p, _p, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_prdn_planar_batch_dev": (_i, [_p, _p, _p, _z, _p, _p, _p, _p, _p]),
    "rspt_hip_native_to_i32_batch_dev": (_i, [_p, _p, _p, _z, _p]),
    "rspt_hip_i32_to_native_batch_dev": (_i, [_p, _p, _p, _z, _p]),
    "rspt_hip_stream": (_p, [_p]),
    "rspt_hip_synchronize": (_i, [_p]),
    "rspt_hip_set_profiling": (_i, [_p, _i]),
    "rspt_hip_stage_count": (_i, [_p]),
    "rspt_hip_stage_name": (C.c_char_p, [_p, _i]),
    "rspt_hip_stage_times": (_i, [_p, C.POINTER(C.c_float), _i]),
    "rspt_hip_debug_read": (C.c_longlong, [_p, _i, _p, _z]),
}
# the C++ factories behind the same library (include/signal_packer.h), via their C shim in signal_packer_hip.cpp
CXX_SHIM = {
    "rspt_cxx_new": (_p, [_i, _z, _z, _z, _z]),
    "rspt_cxx_delete": (None, [_i, _p]),
    "rspt_cxx_compress": (None, [_p, _p, _p, _z, _szp]),
    "rspt_cxx_decompress": (_i, [_p, _p, _szp, _p]),
    "rspt_cxx_set_device": (_i, [_i]),
    "rspt_cxx_set_quantizer": (_i, [_p, _d, _u]),
}
C_ABI_SYMBOLS = list(C_ABI)  # every symbol include/rspt_hip.h declares (tests check the library exports them all)
_lib = None


def bind(L, missing_ok=False):
    """Give every function of the two tables its restype and argtypes on the loaded library L and return L.  missing_ok: skip
    what L does not export -- an older build loaded beside this one for A/B timing lacks the newer entries."""
    for table in (C_ABI, CXX_SHIM):
        for name, (restype, argtypes) in table.items():
            if missing_ok and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype, f.argtypes = restype, list(argtypes)
    return L


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

    _lib = bind(C.CDLL(path))
    return _lib


def _dptr(a):
    """the double* of a float64 numpy array"""
    return a.ctypes.data_as(_dp)


def _as_u8(buf):
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
    return np.ascontiguousarray(a)


class SignalPacker:
    """One i_signal_packer instance on one GPU."""

    def __init__(self, kind, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode=3, device=0, library=None):
        """library: another loaded and bound build of librspt_hip.so to run this handle on (A/B timing beside lib(), tools/planar_bench.py)"""
        self._L = library if library is not None else lib()
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

    # -- the frame of a device-batch call ---------------------------------------
    def _call(self, entry, *args):
        """entry(handle, *args); a status other than RSPT_HIP_OK raises RsptHipError under the entry's name"""
        self._check(entry, getattr(self._L, entry)(self._h, *args))

    def _nblocks(self, t, dtype=None, per_block=None):
        """the block count of t: a contiguous device tensor of whole blocks (uint8, block_bytes each, unless told otherwise)"""
        import torch

        per_block = self.block_bytes if per_block is None else per_block
        assert t.is_cuda and t.dtype == (torch.uint8 if dtype is None else dtype) and t.is_contiguous()
        nblocks = t.numel() // per_block
        assert nblocks * per_block == t.numel()
        return nblocks

    @staticmethod
    def _stream(stream, device):
        """the hipStream_t of a call: `stream`, or torch's current stream on `device` when it is None"""
        import torch

        return stream if stream is not None else torch.cuda.current_stream(device).cuda_stream

    def _bytes(self, entry, *args):
        """a *_state_bytes / *_work_bytes entry -> the byte count it writes through its size_t*"""
        n = C.c_size_t()
        self._call(entry, *args, C.byref(n))
        return n.value

    @staticmethod
    def _zero_state(nbytes, device):
        """a zeroed uint8 device tensor of nbytes: the fresh state of every carried-state stage"""
        import torch

        return torch.zeros(nbytes, dtype=torch.uint8, device=device if device is not None else "cuda")

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

    def quantizer(self):
        """(quality, nb) of a dct / hadamard handle (rspt_hip_get_quantizer)"""
        q, nb = C.c_double(), C.c_uint()
        self._call("rspt_hip_get_quantizer", C.byref(q), C.cast(C.byref(nb), C.c_void_p))
        return q.value, nb.value

    def set_quantizer(self, quality=None, nb=None):
        """The lossy packers' trade-off between size and distortion (rspt_hip.h: rspt_hip_set_quantizer): the reference's
        `quality` constant -- dct: larger is COARSER (128 in the reference); hadamard: larger is FINER (1 in the reference) --
        and nb, the low bytes of every stored value that reach the stream (dct 2, hadamard 3).  None keeps the current value.
        Neither is in the stream: the decoding handle needs the same setting.  Synchronises the device."""
        q0, nb0 = self.quantizer()
        self._call("rspt_hip_set_quantizer", float(q0 if quality is None else quality), int(nb0 if nb is None else nb))
        self.max_compressed_size = self._L.rspt_hip_max_compressed_size(self._h)  # (follows nb)

    def set_byte_order(self, big_endian=True):
        """samples arrive (compress) and leave (decompress) with their bytes reversed (utils.cpp reverse_byte_order branches)"""
        self._check("rspt_hip_set_byte_order", self._L.rspt_hip_set_byte_order(self._h, int(bool(big_endian))))

    def set_verify(self, on=True):
        """check every block's CRC-32C on decompress (hzr_verify's job in the reference); off by default"""
        self._check("rspt_hip_set_verify", self._L.rspt_hip_set_verify(self._h, int(bool(on))))

    # -- device-resident batches (torch tensors carry the memory) --------------
    def reserve(self, nblocks):
        self._check("rspt_hip_reserve", self._L.rspt_hip_reserve(self._h, nblocks))

    def _dst(self, nblocks, d_dst, dst_stride, device):
        """(d_dst, dst_stride) of a compress call: the caller's, or a stride that holds any stream -- max_compressed_size rounded up
        to 256 -- and a destination of nblocks of them, allocated here"""
        import torch

        if dst_stride is None:
            dst_stride = (self.max_compressed_size + 255) // 256 * 256 if d_dst is None else d_dst.numel() // nblocks
        if d_dst is None:
            d_dst = torch.empty((nblocks, dst_stride), dtype=torch.uint8, device=device)
        return d_dst, dst_stride

    def _rate_buffers(self, work_bytes, d_src, nblocks, ladder, work, d_dst, dst_stride):
        """what every rate-control call shares (compress_to_prdn, compress_to_budget, compress_to_total and their planar forms)
        -> (the ladder as a float64 array, the device, d_dst, dst_stride, d_sizes, d_choice, work); work: the caller's, or
        work_bytes(nblocks, nladder) bytes allocated here"""
        import torch

        lad = np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
        dev = d_src.device
        d_dst, dst_stride = self._dst(nblocks, d_dst, dst_stride, dev)
        d_sizes = torch.empty(nblocks, dtype=torch.int64, device=dev)
        d_choice = torch.empty(nblocks, dtype=torch.int32, device=dev)
        if work is None:
            work = torch.empty((work_bytes(nblocks, lad.size) + 7) // 8, dtype=torch.float64, device=dev)
        assert work.is_cuda and work.is_contiguous()
        return lad, dev, d_dst, dst_stride, d_sizes, d_choice, work

    def _ladder_args(self, ladder, choice, nblocks):
        """(double*, count, device pointer) of a ladder call: `ladder` a sequence of 1..8 qualities, `choice` a torch.int32 cuda
        tensor [nblocks] of indices into it (rspt_hip.h: rspt_hip_compress_batch_ladder_dev)"""
        import torch

        lad = np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
        assert choice.is_cuda and choice.dtype == torch.int32 and choice.is_contiguous() and choice.numel() == nblocks
        return lad, (_dptr(lad), lad.size, choice.data_ptr())

    def compress_batch(self, d_src, d_dst=None, d_sizes=None, dst_stride=None, stream=None, ladder=None, choice=None):
        """d_src: uint8 cuda tensor [nblocks, block_bytes].  Returns (d_dst, d_sizes);
        asynchronous on `stream` (default: torch's current stream).
        ladder, choice (both or neither; dct / hadamard): block b is compressed at quality ladder[choice[b]], whatever the
        handle's own -- choice a torch.int32 cuda tensor [nblocks]; an index outside the ladder sets bit 63 of d_sizes[b]."""
        import torch

        assert (ladder is None) == (choice is None)
        nblocks = self._nblocks(d_src)
        d_dst, dst_stride = self._dst(nblocks, d_dst, dst_stride, d_src.device)
        if d_sizes is None:
            d_sizes = torch.empty(nblocks, dtype=torch.int64, device=d_src.device)
        st = self._stream(stream, d_src.device)
        if ladder is not None:
            lad, largs = self._ladder_args(ladder, choice, nblocks)
            self._call("rspt_hip_compress_batch_ladder_dev", d_src.data_ptr(), nblocks, *largs, d_dst.data_ptr(), dst_stride, d_sizes.data_ptr(), st)
        else:
            self._call("rspt_hip_compress_batch_dev", d_src.data_ptr(), nblocks, d_dst.data_ptr(), dst_stride, d_sizes.data_ptr(), st)
        return d_dst, d_sizes

    def decompress_batch(self, d_streams, nblocks, src_stride, d_out=None, d_consumed=None, stream=None, ladder=None, choice=None):
        """ladder, choice: as compress_batch -- the decoder needs the choice the encoder had, it is not in the stream"""
        assert (ladder is None) == (choice is None)
        d_out, d_consumed = self._decode_buffers(nblocks, d_streams.device, d_out, d_consumed, False)
        st = self._stream(stream, d_streams.device)
        if ladder is not None:
            lad, largs = self._ladder_args(ladder, choice, nblocks)
            self._call("rspt_hip_decompress_batch_ladder_dev", d_streams.data_ptr(), src_stride, nblocks, *largs, d_out.data_ptr(),
                       d_consumed.data_ptr(), st)
        else:
            self._call("rspt_hip_decompress_batch_dev", d_streams.data_ptr(), src_stride, nblocks, d_out.data_ptr(), d_consumed.data_ptr(), st)
        return d_out, d_consumed

    def target_work_bytes(self, nblocks, nladder):
        return self._bytes("rspt_hip_compress_target_work_bytes", int(nblocks), int(nladder))

    def debug_set_target_route(self, route):
        """compress_to_prdn's route, for tests: 0 the host's choice, 1 general, 2 the fused probe (rspt_hip_debug_set_target_route)"""
        self._call("rspt_hip_debug_set_target_route", int(route))

    def compress_to_prdn(self, d_src, target, ladder, work=None, stream=None, d_dst=None, dst_stride=None):
        """The smallest stream of a quality ladder whose PRDN is at most `target` percent, block by block (rspt_hip.h:
        rspt_hip_compress_target_batch_dev): block b takes the first entry of `ladder` (ordered coarse to fine) whose round trip
        meets the target, and the last one if none does.  One asynchronous call; no hzr stage runs for a candidate.
        work: a device tensor of at least target_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here.
        Returns (d_dst, d_sizes, d_choice, d_prdn): streams and sizes as compress_batch(ladder=, choice=d_choice) writes them,
        the chosen indices (torch.int32; decompress_batch needs them) and the chosen entries' PRDN (float64)."""
        return self._compress_to_prdn("rspt_hip_compress_target_batch_dev", self.target_work_bytes, d_src, self._nblocks(d_src), target, ladder,
                                      work, stream, d_dst, dst_stride)

    def budget_work_bytes(self, nblocks, nladder):
        """bytes of compress_to_budget's work area, for the route a call would take now (debug_set_budget_route)"""
        return self._bytes("rspt_hip_compress_budget_work_bytes", int(nblocks), int(nladder))

    def debug_set_budget_route(self, route):
        """compress_to_budget's route, for tests: 0 the host's choice, 1 general, 2 batched (rspt_hip_debug_set_budget_route)"""
        self._call("rspt_hip_debug_set_budget_route", int(route))

    def compress_to_budget(self, d_src, budget, ladder, work=None, stream=None, d_dst=None, dst_stride=None, cand_sizes=False):
        """The finest entry of a quality ladder whose stream is at most `budget` bytes, block by block (rspt_hip.h:
        rspt_hip_compress_budget_batch_dev): block b takes the highest index of `ladder` (ordered coarse to fine) whose stream
        fits, and the smallest stream if none does (then d_sizes[b] > its budget).  One asynchronous call; no candidate's stream
        is written.  budget: an int for every block, or a torch.int64 cuda tensor [nblocks] (read as unsigned).
        work: a device tensor of at least budget_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here.
        Returns (d_dst, d_sizes, d_choice): streams and sizes as compress_batch(ladder=, choice=d_choice) writes them and the
        chosen indices (torch.int32; decompress_batch needs them); with cand_sizes also d_cand, torch.int64 [nladder, nblocks],
        every candidate's stream size."""
        return self._compress_to_budget("rspt_hip_compress_budget_batch_dev", self.budget_work_bytes, d_src, self._nblocks(d_src), budget, ladder,
                                        work, stream, d_dst, dst_stride, cand_sizes)

    def budget_planar_work_bytes(self, nblocks, nladder):
        """bytes of compress_to_budget_planar's work area: those of budget_work_bytes, on either route"""
        return self._bytes("rspt_hip_compress_budget_planar_work_bytes", int(nblocks), int(nladder))

    def compress_to_budget_planar(self, d_planar, budget, ladder, work=None, stream=None, d_dst=None, dst_stride=None, cand_sizes=False):
        """compress_to_budget for samples that already live in int32 (rspt_hip.h: rspt_hip_compress_budget_planar_batch_dev): d_planar
        is a contiguous torch.int32 cuda tensor [nblocks, nch, ns], only read; everything returned is what
        compress_to_budget(from_planar_i32(d_planar), ...) returns -- on a handle of bps < 4 only the low bps bytes of a value count.
        work: at least budget_planar_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        return self._compress_to_budget("rspt_hip_compress_budget_planar_batch_dev", self.budget_planar_work_bytes, d_planar, nblocks, budget,
                                        ladder, work, stream, d_dst, dst_stride, cand_sizes)

    def _compress_to_budget(self, entry, work_bytes, d_src, nblocks, budget, ladder, work, stream, d_dst, dst_stride, cand_sizes):
        import torch

        lad, dev, d_dst, dst_stride, d_sizes, d_choice, work = self._rate_buffers(work_bytes, d_src, nblocks, ladder, work, d_dst, dst_stride)
        d_cand = torch.empty((lad.size, nblocks), dtype=torch.int64, device=dev) if cand_sizes else None
        if isinstance(budget, torch.Tensor):
            assert budget.is_cuda and budget.dtype == torch.int64 and budget.is_contiguous() and budget.numel() == nblocks
            scalar, d_budget = 0, budget.data_ptr()
        else:
            scalar, d_budget = int(budget), None
            assert 0 <= scalar < 1 << 64
        self._call(entry, d_src.data_ptr(), nblocks, _dptr(lad), lad.size, scalar, d_budget, d_dst.data_ptr(), dst_stride, d_sizes.data_ptr(),
                   d_choice.data_ptr(), None if d_cand is None else d_cand.data_ptr(), work.data_ptr(), self._stream(stream, dev))
        return (d_dst, d_sizes, d_choice) + ((d_cand,) if cand_sizes else ())

    def total_work_bytes(self, nblocks, nladder):
        """bytes of compress_to_total's work area, for the route a call would take now (debug_set_total_route)"""
        return self._bytes("rspt_hip_compress_total_work_bytes", int(nblocks), int(nladder))

    def debug_set_total_route(self, route):
        """compress_to_total's route, for tests: 0 the host's choice, 1 general, 2 fused (rspt_hip_debug_set_total_route)"""
        self._call("rspt_hip_debug_set_total_route", int(route))

    def compress_to_total(self, d_src, total_bytes, ladder, work=None, stream=None, d_dst=None, dst_stride=None, tables=False):
        """The whole batch in at most `total_bytes` bytes at the lowest common PRDN level (rspt_hip.h:
        rspt_hip_compress_total_batch_dev): every block takes its smallest stream whose figure is at most the level T*, and T* is
        the lowest level at which those streams add up to at most total_bytes -- +inf if none does (then d_total > total_bytes is
        the miss).  One asynchronous call; no candidate's stream is written.  total_bytes: any int of 64 bits, unsigned.
        work: a device tensor of at least total_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here.
        Returns (d_dst, d_sizes, d_choice, d_level, d_total, d_prdn): streams and sizes as compress_batch(ladder=,
        choice=d_choice) writes them, the chosen indices (torch.int32; decompress_batch needs them), T* (float64 [1]), the sum
        of the chosen sizes (torch.int64 [1]) and the chosen entries' figures (float64); with tables also d_cand_sizes
        (torch.int64) and d_cand_figs (float64), both [nladder, nblocks]."""
        return self._compress_to_total("rspt_hip_compress_total_batch_dev", self.total_work_bytes, d_src, self._nblocks(d_src), total_bytes, ladder,
                                       work, stream, d_dst, dst_stride, tables)

    def total_planar_work_bytes(self, nblocks, nladder):
        """bytes of compress_to_total_planar's work area, for the route a call would take now (debug_set_total_route): fused those
        of total_work_bytes; general those less one planar copy of the batch at bps 4, and the same at bps < 4"""
        return self._bytes("rspt_hip_compress_total_planar_work_bytes", int(nblocks), int(nladder))

    def compress_to_total_planar(self, d_planar, total_bytes, ladder, work=None, stream=None, d_dst=None, dst_stride=None, tables=False):
        """compress_to_total for samples that already live in int32 (rspt_hip.h: rspt_hip_compress_total_planar_batch_dev): d_planar
        is a contiguous torch.int32 cuda tensor [nblocks, nch, ns], only read; everything returned is what
        compress_to_total(from_planar_i32(d_planar), ...) returns -- on a handle of bps < 4 only the low bps bytes of a value count.
        work: at least total_planar_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        return self._compress_to_total("rspt_hip_compress_total_planar_batch_dev", self.total_planar_work_bytes, d_planar, nblocks, total_bytes,
                                       ladder, work, stream, d_dst, dst_stride, tables)

    def _compress_to_total(self, entry, work_bytes, d_src, nblocks, total_bytes, ladder, work, stream, d_dst, dst_stride, tables):
        import torch

        lad, dev, d_dst, dst_stride, d_sizes, d_choice, work = self._rate_buffers(work_bytes, d_src, nblocks, ladder, work, d_dst, dst_stride)
        d_level = torch.empty(1, dtype=torch.float64, device=dev)
        d_total = torch.empty(1, dtype=torch.int64, device=dev)
        d_prdn = torch.empty(nblocks, dtype=torch.float64, device=dev)
        d_cand = torch.empty((lad.size, nblocks), dtype=torch.int64, device=dev) if tables else None
        d_figs = torch.empty((lad.size, nblocks), dtype=torch.float64, device=dev) if tables else None
        total_bytes = int(total_bytes)
        assert 0 <= total_bytes < 1 << 64
        self._call(entry, d_src.data_ptr(), nblocks, _dptr(lad), lad.size, total_bytes, d_dst.data_ptr(), dst_stride,
                   d_sizes.data_ptr(), d_choice.data_ptr(), d_level.data_ptr(), d_total.data_ptr(), d_prdn.data_ptr(),
                   None if d_cand is None else d_cand.data_ptr(), None if d_figs is None else d_figs.data_ptr(), work.data_ptr(), self._stream(stream, dev))
        return (d_dst, d_sizes, d_choice, d_level, d_total, d_prdn) + ((d_cand, d_figs) if tables else ())

    def target_planar_work_bytes(self, nblocks, nladder):
        """bytes of compress_to_prdn_planar's work area, for the route a call would take now (debug_set_target_route)"""
        return self._bytes("rspt_hip_compress_target_planar_work_bytes", int(nblocks), int(nladder))

    def compress_to_prdn_planar(self, d_planar, target, ladder, work=None, stream=None, d_dst=None, dst_stride=None):
        """compress_to_prdn for samples that already live in int32 (rspt_hip.h: rspt_hip_compress_target_planar_batch_dev): d_planar
        is a torch.int32 cuda tensor [nblocks, nch, ns], only read; everything returned is what
        compress_to_prdn(from_planar_i32(d_planar), ...) returns -- on a handle of bps < 4 the original is the matrix cut to the
        sample width.  work: at least target_planar_work_bytes(nblocks, len(ladder)) bytes, 16-byte aligned; None: allocated here."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        return self._compress_to_prdn("rspt_hip_compress_target_planar_batch_dev", self.target_planar_work_bytes, d_planar, nblocks, target,
                                      ladder, work, stream, d_dst, dst_stride)

    def _compress_to_prdn(self, entry, work_bytes, d_src, nblocks, target, ladder, work, stream, d_dst, dst_stride):
        import torch

        lad, dev, d_dst, dst_stride, d_sizes, d_choice, work = self._rate_buffers(work_bytes, d_src, nblocks, ladder, work, d_dst, dst_stride)
        d_prdn = torch.empty(nblocks, dtype=torch.float64, device=dev)
        self._call(entry, d_src.data_ptr(), nblocks, _dptr(lad), lad.size, float(target), d_dst.data_ptr(),
                   dst_stride, d_sizes.data_ptr(), d_choice.data_ptr(), d_prdn.data_ptr(), work.data_ptr(), self._stream(stream, dev))
        return d_dst, d_sizes, d_choice, d_prdn

    def _decode_buffers(self, nblocks, device, d_out, d_consumed, planar):
        """(d_out, d_consumed) of a decompress call, allocated where None: the native batch (uint8 [nblocks, block_bytes]) or,
        planar, the int32 matrix [nblocks, nch, ns]"""
        import torch

        if d_out is None:
            d_out = (torch.empty((nblocks, self.nch, self.ns), dtype=torch.int32, device=device) if planar
                     else torch.empty((nblocks, self.block_bytes), dtype=torch.uint8, device=device))
        if planar:
            assert d_out.is_cuda and d_out.dtype == torch.int32 and d_out.is_contiguous() and d_out.numel() == nblocks * self.nch * self.ns
        if d_consumed is None:
            d_consumed = torch.empty(nblocks, dtype=torch.int64, device=device)
        return d_out, d_consumed

    def compress_planar_batch(self, d_planar, d_dst=None, d_sizes=None, dst_stride=None, stream=None, ladder=None, choice=None):
        """compress_batch for samples that already live in int32 (rspt_hip.h: rspt_hip_compress_planar_batch_dev): d_planar is a
        torch.int32 cuda tensor [nblocks, nch, ns], only read; the streams are those of compress_batch(from_planar_i32(d_planar)).
        ladder, choice: as compress_batch (rspt_hip_compress_planar_batch_ladder_dev).  Returns (d_dst, d_sizes); asynchronous."""
        import torch

        assert (ladder is None) == (choice is None)
        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        d_dst, dst_stride = self._dst(nblocks, d_dst, dst_stride, d_planar.device)
        if d_sizes is None:
            d_sizes = torch.empty(nblocks, dtype=torch.int64, device=d_planar.device)
        st = self._stream(stream, d_planar.device)
        if ladder is not None:
            lad, largs = self._ladder_args(ladder, choice, nblocks)
            self._call("rspt_hip_compress_planar_batch_ladder_dev", d_planar.data_ptr(), nblocks, *largs, d_dst.data_ptr(), dst_stride,
                       d_sizes.data_ptr(), st)
        else:
            self._call("rspt_hip_compress_planar_batch_dev", d_planar.data_ptr(), nblocks, d_dst.data_ptr(), dst_stride, d_sizes.data_ptr(), st)
        return d_dst, d_sizes

    def decompress_planar_batch(self, d_streams, nblocks, src_stride, d_out=None, d_consumed=None, stream=None, ladder=None, choice=None):
        """decompress_batch into torch.int32 [nblocks, nch, ns] (rspt_hip.h: rspt_hip_decompress_planar_batch_dev): the values of
        to_planar_i32(decompress_batch(...)) on a little-endian handle.  ladder, choice: as decompress_batch
        (rspt_hip_decompress_planar_batch_ladder_dev).  Returns (d_out, d_consumed); asynchronous."""
        assert (ladder is None) == (choice is None)
        d_out, d_consumed = self._decode_buffers(nblocks, d_streams.device, d_out, d_consumed, True)
        st = self._stream(stream, d_streams.device)
        if ladder is not None:
            lad, largs = self._ladder_args(ladder, choice, nblocks)
            self._call("rspt_hip_decompress_planar_batch_ladder_dev", d_streams.data_ptr(), src_stride, nblocks, *largs, d_out.data_ptr(),
                       d_consumed.data_ptr(), st)
        else:
            self._call("rspt_hip_decompress_planar_batch_dev", d_streams.data_ptr(), src_stride, nblocks, d_out.data_ptr(), d_consumed.data_ptr(), st)
        return d_out, d_consumed

    def decompress_packed_planar(self, d_packed, d_out=None, d_consumed=None, stream=None, nbytes=None, ladder=None):
        """decompress_packed into torch.int32 [nblocks, nch, ns] (rspt_hip.h: rspt_hip_decompress_packed_planar_dev, with a ladder
        rspt_hip_decompress_packed_planar_ladder_dev)."""
        return self.decompress_packed(d_packed, d_out, d_consumed, stream, nbytes, planar=True, ladder=ladder)

    def decompress_packed(self, d_packed, d_out=None, d_consumed=None, stream=None, nbytes=None, planar=False, ladder=None):
        """Decompress every stream of a container (what pack_batch / the multi-GPU gather produce) on the device.
        Each stream is decoded with the nb of its own index entry.  Reads the 32-byte header to the host for the block
        count (a synchronisation).  `nbytes`: container length if shorter than the tensor.  planar: into an int32 matrix
        (decompress_packed_planar).  ladder: the container carries a choice per stream (pack_batch(choice=)) and every stream is
        decoded at ladder[its choice]; a stored choice outside the ladder flags its block and writes nothing for it."""
        entry = "rspt_hip_decompress_packed%s%s_dev" % ("_planar" if planar else "", "" if ladder is None else "_ladder")
        lad = None if ladder is None else np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
        largs = () if lad is None else (_dptr(lad), lad.size)
        head = d_packed[:32].cpu().numpy().view(np.uint64)
        if int(head[0]) != 0x4B43415054505352:
            raise ValueError("not an RSPTPACK container")
        nblocks = int(head[1])
        plen = int(nbytes) if nbytes is not None else d_packed.numel()
        if nblocks == 0 or nblocks > 65535 or plen < 32 or nblocks > (plen - 32) // 16:  # (nothing is sized from an untrusted count)
            raise RsptHipError(entry, -6 if 0 < nblocks <= 65535 else -1)
        d_out, d_consumed = self._decode_buffers(nblocks, d_packed.device, d_out, d_consumed, planar)
        st = self._stream(stream, d_packed.device)
        self._call(entry, d_packed.data_ptr(), plen, nblocks, *largs, d_out.data_ptr(), d_consumed.data_ptr(), st)
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
        st = self._stream(stream, d_streams.device)
        self._call("rspt_hip_hzr_verify_batch_dev", d_streams.data_ptr(), src_stride, d_lengths.data_ptr(), nblocks, d_decoded.data_ptr(), st)
        return d_decoded

    def pack_bound(self, nblocks):
        return self._L.rspt_hip_pack_bound(self._h, nblocks)

    def pack_batch(self, d_dst, d_sizes, d_packed=None, d_total=None, stream=None, choice=None, nladder=None):
        """streams of a batch -> one container (layout: include/rspt_hip.h); asynchronous.
        choice, nladder (both or neither; dct / hadamard): the torch.int32 cuda tensor [nblocks] a ladder or target compress call
        had or returned, and the length of its ladder -- each stream's choice travels in its index entry
        (rspt_hip_pack_batch_choice_dev) and decompress_packed(ladder=) needs nothing beside the container."""
        import torch

        assert (choice is None) == (nladder is None)
        nblocks = d_sizes.numel()
        stride = d_dst.numel() // nblocks
        if d_packed is None:
            d_packed = torch.empty(self.pack_bound(nblocks), dtype=torch.uint8, device=d_dst.device)
        if d_total is None:
            d_total = torch.zeros(1, dtype=torch.int64, device=d_dst.device)
        st = self._stream(stream, d_dst.device)
        if choice is not None:
            assert choice.is_cuda and choice.dtype == torch.int32 and choice.is_contiguous() and choice.numel() == nblocks
            self._call("rspt_hip_pack_batch_choice_dev", d_dst.data_ptr(), stride, d_sizes.data_ptr(), nblocks, choice.data_ptr(), int(nladder),
                       d_packed.data_ptr(), d_total.data_ptr(), st)
        else:
            self._call("rspt_hip_pack_batch_dev", d_dst.data_ptr(), stride, d_sizes.data_ptr(), nblocks, d_packed.data_ptr(), d_total.data_ptr(), st)
        return d_packed, d_total

    def iir_state_bytes(self):
        return self._bytes("rspt_hip_iir_state_bytes")

    def iir_state(self, device=None):
        """A zeroed state for iir_prefilter_batch(state=...): a fresh filter for every channel (uint8 device tensor)."""
        return self._zero_state(self.iir_state_bytes(), device)

    def fir_state_bytes(self, kernel_size):
        return self._bytes("rspt_hip_fir_state_bytes", int(kernel_size))

    def fir_state(self, kernel_size, device=None):
        """A zeroed state for fir_prefilter_batch(state=...) with a kernel of kernel_size taps: a fresh filter for every channel."""
        return self._zero_state(self.fir_state_bytes(kernel_size), device)

    def iir_prefilter_batch(self, d_buf, n, d, init_nr_samples=2000, per_channel=False, stream=None, state=None):
        """The reference's pre-filter step (rspt_test.cpp:116-136) on device-resident blocks, in place; asynchronous.
        state: None, or an iir_state() tensor: the blocks are then consecutive pieces of one recording, one filter per channel
        running through them and on into the next call (rspt_hip_iir_prefilter_stream_dev); needs per_channel=True."""
        return self._iir_prefilter("", d_buf, self._nblocks(d_buf), n, d, init_nr_samples, per_channel, stream, state)

    def iir_prefilter_planar_batch(self, d_planar, n, d, init_nr_samples=2000, per_channel=False, stream=None, state=None):
        """iir_prefilter_batch on samples that live in int32 (rspt_hip.h: rspt_hip_iir_prefilter_planar_batch_dev / _stream_dev):
        d_planar is a torch.int32 cuda tensor [nblocks, nch, ns], filtered in place; the whole int32 value is the sample and the
        result is stored whole, whatever the handle's bps.  n, d, init_nr_samples, per_channel and state as in iir_prefilter_batch."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        return self._iir_prefilter("planar_", d_planar, nblocks, n, d, init_nr_samples, per_channel, stream, state)

    def _iir_prefilter(self, form, d_buf, nblocks, n, d, init_nr_samples, per_channel, stream, state):
        """both layouts of the IIR pre-filter: form "" (native blocks) or "planar_" (the int32 matrix)"""
        nn, dd = np.ascontiguousarray(n, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        assert nn.size == dd.size
        st = self._stream(stream, d_buf.device)
        args = (d_buf.data_ptr(), nblocks, _dptr(nn), _dptr(dd), nn.size, init_nr_samples)
        if state is not None:
            if not per_channel:
                raise ValueError("iir_prefilter_%sbatch: a carried state is one filter per channel (per_channel=True)" % form)
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.iir_state_bytes()
            self._call("rspt_hip_iir_prefilter_%sstream_dev" % form, *args, state.data_ptr(), st)
        else:
            self._call("rspt_hip_iir_prefilter_%sbatch_dev" % form, *args, int(bool(per_channel)), st)
        return d_buf

    def iir_cascade_state_bytes(self, nsections):
        return self._bytes("rspt_hip_iir_cascade_state_bytes", int(nsections))

    def iir_cascade_state(self, nsections, device=None):
        """A zeroed state for iir_cascade_batch(state=...) with nsections sections: a fresh chain for every channel."""
        return self._zero_state(self.iir_cascade_state_bytes(nsections), device)

    def iir_cascade_batch(self, d_buf, sections, stream=None, state=None):
        """1 to 4 reference IIR filters per channel, chained in double and truncated once (rspt_hip.h: rspt_hip_iir_cascade_batch_dev),
        on device-resident blocks, in place; asynchronous.  lp->filter_opt(hp->filter_opt(x)) is sections=[(hp_n, hp_d), (lp_n, lp_d, 0)].
        sections: a list of (n, d), (n, d, init_nr_samples) or (n, d, init_nr_samples, use_filter); init_nr_samples defaults to
        2000, use_filter (the section runs filter() instead of filter_opt()) to False.
        state: None (a fresh chain per block and channel), or an iir_cascade_state(len(sections)) tensor: the blocks are then
        consecutive pieces of one recording, one chain per channel running through them and on into the next call."""
        return self._iir_cascade("", d_buf, self._nblocks(d_buf), sections, stream, state)

    def iir_cascade_planar_batch(self, d_planar, sections, stream=None, state=None):
        """iir_cascade_batch on samples that live in int32 (rspt_hip.h: rspt_hip_iir_cascade_planar_batch_dev / _stream_dev):
        d_planar is a torch.int32 cuda tensor [nblocks, nch, ns], filtered in place; the whole int32 value is the sample and the
        result is stored whole, whatever the handle's bps.  sections and state as in iir_cascade_batch."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        return self._iir_cascade("planar_", d_planar, nblocks, sections, stream, state)

    def _iir_cascade(self, form, d_buf, nblocks, sections, stream, state):
        """both layouts of the cascade: form "" (native blocks) or "planar_" (the int32 matrix)"""
        S = len(sections)
        if not 1 <= S <= 4:
            raise ValueError("iir_cascade_%sbatch: 1 to 4 sections" % form)
        nn, dd = np.zeros((S, 5)), np.zeros((S, 5))
        nc, init, filt = np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.uint8)
        for k, sec in enumerate(sections):
            n, d = np.asarray(sec[0], dtype=np.float64).reshape(-1), np.asarray(sec[1], dtype=np.float64).reshape(-1)
            if n.size != d.size or not 2 <= n.size <= 5:
                raise ValueError("iir_cascade_%sbatch: section %d needs 2 to 5 coefficients on each side" % (form, k))
            nn[k, : n.size], dd[k, : d.size] = n, d
            nc[k], init[k], filt[k] = n.size, (sec[2] if len(sec) > 2 else 2000), bool(sec[3]) if len(sec) > 3 else False
        st = self._stream(stream, d_buf.device)
        args = (d_buf.data_ptr(), nblocks, S, _dptr(nn), _dptr(dd),
                nc.ctypes.data_as(C.POINTER(C.c_uint32)), init.ctypes.data_as(C.POINTER(C.c_int32)), filt.ctypes.data_as(_u8p))
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.iir_cascade_state_bytes(S)
            self._call("rspt_hip_iir_cascade_%sstream_dev" % form, *args, state.data_ptr(), st)
        else:
            self._call("rspt_hip_iir_cascade_%sbatch_dev" % form, *args, st)
        return d_buf

    def iir_zero_phase_work_bytes(self, nblocks):
        return self._bytes("rspt_hip_iir_zero_phase_work_bytes", int(nblocks))

    def iir_zero_phase_batch(self, d_buf, n, d, init_nr_samples=2000, backward_init_nr_samples=0, work=None, stream=None):
        """Zero-phase (forward-backward) IIR filtering on device-resident blocks, in place; asynchronous.  One fresh reference
        filter per (block, channel) runs forward over the block and then, the same object, backward over its own untruncated
        output; the result is truncated once (rspt_hip.h: rspt_hip_iir_zero_phase_batch_dev).
        work: a device tensor of at least iir_zero_phase_work_bytes(nblocks) bytes, 8-byte aligned; None: allocated here."""
        return self._iir_zero_phase("", d_buf, d_buf, self._nblocks(d_buf), n, d, init_nr_samples, backward_init_nr_samples, work, stream)

    def iir_zero_phase_planar_batch(self, d_planar, n, d, init_nr_samples=2000, backward_init_nr_samples=0, out=None, work=None, stream=None):
        """iir_zero_phase_batch on samples that live in int32 (rspt_hip.h: rspt_hip_iir_zero_phase_planar_batch_dev): d_planar is a
        torch.int32 cuda tensor [nblocks, nch, ns]; in place when out is None, else into out (same shape, not overlapping
        d_planar, which is then only read).  The whole int32 value is the sample and the result is stored whole, whatever the
        handle's bps.  n, d, the history lengths and work as in iir_zero_phase_batch.  Returns the tensor that holds the result."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        if out is None:
            out = d_planar
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == d_planar.numel()
        return self._iir_zero_phase("planar_", d_planar, out, nblocks, n, d, init_nr_samples, backward_init_nr_samples, work, stream)

    def _iir_zero_phase(self, form, d_src, out, nblocks, n, d, init_nr_samples, backward_init_nr_samples, work, stream):
        """both layouts of the zero-phase stage: form "" (native blocks, out is d_src) or "planar_" (the int32 matrix)"""
        import torch

        nn, dd = np.ascontiguousarray(n, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        assert nn.size == dd.size
        if work is None:
            work = torch.empty(max(1, (self.iir_zero_phase_work_bytes(max(nblocks, 1)) + 7) // 8), dtype=torch.float64, device=d_src.device)
        assert work.is_cuda and work.is_contiguous()
        st = self._stream(stream, d_src.device)
        bufs = (d_src.data_ptr(), out.data_ptr()) if form else (d_src.data_ptr(),)
        self._call("rspt_hip_iir_zero_phase_%sbatch_dev" % form, *bufs, nblocks, _dptr(nn), _dptr(dd), nn.size, int(init_nr_samples),
                   int(backward_init_nr_samples), work.data_ptr(), work.numel() * work.element_size(), st)
        return out

    def _window_call_buffers(self, d_src, d_dst, stream):
        """(nblocks, output, stream) of a windowed stage's call (fir_prefilter_batch, median_filter_batch): whole blocks of
        contiguous uint8 on the device, the output d_src itself when d_dst is None, the current stream when stream is None."""
        import torch

        nblocks = self._nblocks(d_src)
        out = d_src if d_dst is None else d_dst
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == d_src.numel()
        return nblocks, out, self._stream(stream, d_src.device)

    def fir_prefilter_batch(self, d_src, kernel, d_dst=None, stream=None, state=None):
        """The reference's FIR pre-filter (i_filter::new_fir, init_history_values, filter_opt; rspt_hip.h) on device-resident
        blocks: in place when d_dst is None, else into d_dst (same size, not overlapping d_src); asynchronous.  Returns the output.
        state: None, or a fir_state(len(kernel)) tensor: the blocks are then consecutive pieces of one recording, one filter per
        channel running through them and on into the next call (rspt_hip_fir_prefilter_stream_dev)."""
        nblocks, out, st = self._window_call_buffers(d_src, d_dst, stream)
        k = np.ascontiguousarray(kernel, dtype=np.float64).reshape(-1)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.fir_state_bytes(k.size)
            self._call("rspt_hip_fir_prefilter_stream_dev", d_src.data_ptr(), out.data_ptr(), nblocks, _dptr(k), k.size, state.data_ptr(), st)
        else:
            self._call("rspt_hip_fir_prefilter_batch_dev", d_src.data_ptr(), out.data_ptr(), nblocks, _dptr(k), k.size, st)
        return out

    def fir_planar_state_bytes(self, kernel_size):
        return self._bytes("rspt_hip_fir_planar_state_bytes", int(kernel_size))

    def fir_planar_state(self, kernel_size, device=None):
        """A zeroed state for fir_prefilter_planar_batch(state=...) with a kernel of kernel_size taps: rows of nch int32, so the
        native fir_state() only where the handle's bps is 4."""
        return self._zero_state(self.fir_planar_state_bytes(kernel_size), device)

    def fir_prefilter_planar_batch(self, d_planar, kernel, d_out=None, stream=None, state=None):
        """fir_prefilter_batch on samples that live in int32 (rspt_hip.h: rspt_hip_fir_prefilter_planar_batch_dev / _stream_dev):
        d_planar is a torch.int32 cuda tensor [nblocks, nch, ns]; in place when d_out is None, else into d_out (same shape, not
        overlapping d_planar).  The whole int32 value is the sample and the result is stored whole, whatever the handle's bps.
        Returns the output.  state: None, or a fir_planar_state(len(kernel)) tensor, as in fir_prefilter_batch."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        out = d_planar if d_out is None else d_out
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == d_planar.numel()
        st = self._stream(stream, d_planar.device)
        k = np.ascontiguousarray(kernel, dtype=np.float64).reshape(-1)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.fir_planar_state_bytes(k.size)
            self._call("rspt_hip_fir_prefilter_planar_stream_dev", d_planar.data_ptr(), out.data_ptr(), nblocks, _dptr(k), k.size, state.data_ptr(), st)
        else:
            self._call("rspt_hip_fir_prefilter_planar_batch_dev", d_planar.data_ptr(), out.data_ptr(), nblocks, _dptr(k), k.size, st)
        return out

    def median_state_bytes(self, window):
        return self._bytes("rspt_hip_median_state_bytes", int(window))

    def median_state(self, window, device=None):
        """A zeroed state for median_filter_batch(state=...) with this window: a fresh object for every channel."""
        return self._zero_state(self.median_state_bytes(window), device)

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
            self._call("rspt_hip_median_filter_stream_dev", d_src.data_ptr(), out.data_ptr(), nblocks, int(window), state.data_ptr(), st)
        else:
            self._call("rspt_hip_median_filter_batch_dev", d_src.data_ptr(), out.data_ptr(), nblocks, int(window), st)
        return out

    def median_planar_state_bytes(self, window):
        return self._bytes("rspt_hip_median_planar_state_bytes", int(window))

    def median_planar_state(self, window, device=None):
        """A zeroed state for median_filter_planar_batch(state=...) with this window: rows of nch int32, so the native
        median_state() only where the handle's bps is 4."""
        return self._zero_state(self.median_planar_state_bytes(window), device)

    def median_filter_planar_batch(self, d_planar, window, d_out=None, stream=None, state=None):
        """median_filter_batch on samples that live in int32 (rspt_hip.h: rspt_hip_median_filter_planar_batch_dev / _stream_dev):
        d_planar is a torch.int32 cuda tensor [nblocks, nch, ns]; in place when d_out is None, else into d_out (same shape, not
        overlapping d_planar).  The whole int32 value is the sample and the result is stored whole, whatever the handle's bps.
        Returns the output.  state: None, or a median_planar_state(window) tensor, as in median_filter_batch."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        out = d_planar if d_out is None else d_out
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == d_planar.numel()
        st = self._stream(stream, d_planar.device)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.median_planar_state_bytes(window)
            self._call("rspt_hip_median_filter_planar_stream_dev", d_planar.data_ptr(), out.data_ptr(), nblocks, int(window), state.data_ptr(), st)
        else:
            self._call("rspt_hip_median_filter_planar_batch_dev", d_planar.data_ptr(), out.data_ptr(), nblocks, int(window), st)
        return out

    def peak_state_bytes(self):
        return self._bytes("rspt_hip_peak_state_bytes")

    def peak_state(self, device=None):
        """A zeroed state for peak_detect_batch(state=...): a fresh detector for every channel (uint8 device tensor)."""
        return self._zero_state(self.peak_state_bytes(), device)

    def _peak_call_buffers(self, d_src, max_peaks, state, traces, stream, planar=False):
        """What all peak entries share: checks d_src (whole blocks of contiguous uint8 on the device; planar: an int32 matrix
        [nblocks, nch, ns]) and state, allocates (count, index, value, sig, thr) -- sig and thr None without traces, and laid out
        as the samples are -- and picks the stream (the current one when None).
        -> (nblocks, outputs, stream, ptr); ptr(t): t's device pointer, None for None or an empty tensor."""
        import torch

        nblocks = self._nblocks(d_src, torch.int32, self.nch * self.ns) if planar else self._nblocks(d_src)
        dev = d_src.device
        count = torch.empty((nblocks, self.nch), dtype=torch.int32, device=dev)
        index = torch.empty((nblocks, self.nch, max_peaks), dtype=torch.int32, device=dev)
        value = torch.empty((nblocks, self.nch, max_peaks), dtype=torch.float64, device=dev)
        sig = thr = None
        if traces:
            sig = torch.empty((nblocks, self.nch, self.ns) if planar else (nblocks, self.ns, self.nch), dtype=torch.float64, device=dev)
            thr = torch.empty_like(sig)
        if state is not None:
            assert state.is_cuda and state.is_contiguous() and state.numel() * state.element_size() >= self.peak_state_bytes()
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        return nblocks, (count, index, value, sig, thr), self._stream(stream, dev), ptr

    def peak_detect_batch(self, d_src, variant="online", sampling_rate=None, marker_val=1.0, max_peaks=64, state=None, traces=False, stream=None):
        """The reference's R-peak detectors (peak_detector.h; rspt_hip.h: rspt_hip_peak_detect_batch_dev) on device-resident
        blocks, which are only read.  variant: "online" (peak_detector), "online_1st" (peak_detector_1st_order) or "offline_fw"
        (peak_detector_offline::detect_fw).  state: None for a fresh detector per (block, channel), or a peak_state() tensor that
        carries one detector per channel through the blocks and across calls (of one variant and sampling rate).  Asynchronous.
        Returns (count [nblocks, nch] int32, index [nblocks, nch, max_peaks] int32, value [nblocks, nch, max_peaks] float64) and,
        with traces, (sig, threshold) [nblocks, ns, nch] float64 as well."""
        return self._peak_detect("rspt_hip_peak_detect_batch_dev", False, d_src, variant, sampling_rate, marker_val, max_peaks, state, traces, stream)

    def peak_detect_planar_batch(self, d_planar, variant="online", sampling_rate=None, marker_val=1.0, max_peaks=64, state=None, traces=False,
                                 stream=None):
        """peak_detect_batch on samples that live in int32 (rspt_hip.h: rspt_hip_peak_detect_planar_batch_dev): d_planar is a
        torch.int32 cuda tensor [nblocks, nch, ns], only read; the whole int32 value is the sample, whatever the handle's bps.
        Returns what peak_detect_batch returns, the traces [nblocks, nch, ns].  state: a peak_state() tensor, which may
        alternate with native calls where the handle's bps is 4."""
        return self._peak_detect("rspt_hip_peak_detect_planar_batch_dev", True, d_planar, variant, sampling_rate, marker_val, max_peaks, state, traces,
                                 stream)

    def _peak_detect(self, entry, planar, d_src, variant, sampling_rate, marker_val, max_peaks, state, traces, stream):
        if sampling_rate is None:
            raise ValueError("peak_detect_batch: sampling_rate is required")
        v = PEAK_VARIANTS[variant] if isinstance(variant, str) else int(variant)
        nblocks, out, st, ptr = self._peak_call_buffers(d_src, max_peaks, state, traces, stream, planar)
        count, index, value, sig, thr = out
        self._call(entry, d_src.data_ptr(), nblocks, v, float(sampling_rate), float(marker_val), ptr(state),
                   count.data_ptr(), ptr(index), ptr(value), max_peaks, ptr(sig), ptr(thr), st)
        return out if traces else out[:3]

    def peak_offline_work_bytes(self, nblocks, stateful=False):
        return self._bytes("rspt_hip_peak_offline_work_bytes", nblocks, int(bool(stateful)))

    def peak_detect_offline_batch(self, d_src, sampling_rate, marker_val=1.0, max_peaks=64, state=None, traces=False, stream=None):
        """The reference's zero-phase offline R-peak detector (peak_detector_offline::detect; rspt_hip.h:
        rspt_hip_peak_detect_offline_batch_dev) on device-resident blocks, which are only read.  state: None for a fresh object per
        (block, channel), or a peak_state() tensor carrying one object per channel through the blocks and across calls (it may
        alternate with peak_detect_batch(variant="offline_fw") calls at the same rate).  The workspace is allocated here.
        Asynchronous.  Returns what peak_detect_batch returns: (count, index, value) of the final peak_signal's non-zero entries
        and, with traces, (filt_signal, threshold_signal) [nblocks, ns, nch] float64 as well."""
        return self._peak_detect_offline("rspt_hip_peak_detect_offline_batch_dev", False, d_src, sampling_rate, marker_val, max_peaks, state, traces,
                                         stream)

    def peak_detect_offline_planar_batch(self, d_planar, sampling_rate, marker_val=1.0, max_peaks=64, state=None, traces=False, stream=None):
        """peak_detect_offline_batch on samples that live in int32 (rspt_hip.h: rspt_hip_peak_detect_offline_planar_batch_dev):
        d_planar is a torch.int32 cuda tensor [nblocks, nch, ns], only read; the whole int32 value is the sample.  Returns what
        peak_detect_offline_batch returns, the traces [nblocks, nch, ns]."""
        return self._peak_detect_offline("rspt_hip_peak_detect_offline_planar_batch_dev", True, d_planar, sampling_rate, marker_val, max_peaks, state,
                                         traces, stream)

    def _peak_detect_offline(self, entry, planar, d_src, sampling_rate, marker_val, max_peaks, state, traces, stream):
        import torch

        nblocks, out, st, ptr = self._peak_call_buffers(d_src, max_peaks, state, traces, stream, planar)
        count, index, value, sig, thr = out
        dev = d_src.device
        work = torch.empty(max(1, (self.peak_offline_work_bytes(max(nblocks, 1), state is not None) + 7) // 8), dtype=torch.float64, device=dev)
        self._call(entry, d_src.data_ptr(), nblocks, float(sampling_rate), float(marker_val), ptr(state),
                   work.data_ptr(), count.data_ptr(), ptr(index), ptr(value), max_peaks, ptr(sig), ptr(thr), st)
        if stream is not None:  # (the workspace goes back to torch's pool only once the caller's stream is past this call)
            work.record_stream(torch.cuda.ExternalStream(stream, device=dev))
        return out if traces else out[:3]

    def prdn_batch(self, d_orig, d_dec, stream=None, parts=False):
        """The reference's quality figure PRDN[%] (rspt_test.cpp:98-111; rspt_hip.h: rspt_hip_prdn_batch_dev) of the decoded
        blocks d_dec against the originals d_orig, both device-resident in the native layout and only read; bit-identical with
        the reference.  Asynchronous.  Returns a float64 device tensor [nblocks]; with parts, (prdn, mse, ref, path): the two
        accumulators as the reference leaves them and, per block, 0 for the exact-integer path or 1 for the sequential one (int32)."""
        import torch

        nblocks = self._nblocks(d_orig)
        assert self._nblocks(d_dec) == nblocks
        return self._prdn("rspt_hip_prdn_batch_dev", d_orig, d_dec, nblocks, stream, parts)

    def _prdn(self, entry, d_orig, d_dec, nblocks, stream, parts):
        """both layouts of the PRDN stage: the outputs and the call"""
        import torch

        dev = d_orig.device
        prdn = torch.empty(nblocks, dtype=torch.float64, device=dev)
        mse = ref = path = None
        if parts:
            mse, ref = torch.empty_like(prdn), torch.empty_like(prdn)
            path = torch.empty(nblocks, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._call(entry, d_orig.data_ptr() if nblocks else None, d_dec.data_ptr() if nblocks else None, nblocks,
                   prdn.data_ptr() if nblocks else None, ptr(mse), ptr(ref), ptr(path), self._stream(stream, dev))
        return (prdn, mse, ref, path) if parts else prdn

    def prdn_planar_batch(self, d_orig, d_dec, stream=None, parts=False):
        """prdn_batch on samples that live in int32 (rspt_hip.h: rspt_hip_prdn_planar_batch_dev): d_orig and d_dec are torch.int32
        cuda tensors [nblocks, nch, ns], only read (they may be one tensor).  The whole int32 value is the sample, whatever the
        handle's bps and byte order: the figure is prdn_batch's on a little-endian bps = 4 handle of the same (nch, ns) given
        from_planar_i32 of the two.  No channel cap.  Asynchronous.  Returns what prdn_batch returns."""
        import torch

        nblocks = self._nblocks(d_orig, torch.int32, self.nch * self.ns)
        assert self._nblocks(d_dec, torch.int32, self.nch * self.ns) == nblocks
        return self._prdn("rspt_hip_prdn_planar_batch_dev", d_orig, d_dec, nblocks, stream, parts)

    def to_planar_i32(self, d_src, d_out=None, stream=None):
        """The reference's convert_native_to_i32 (utils.cpp:123-191; rspt_hip.h: rspt_hip_native_to_i32_batch_dev) on
        device-resident blocks in the native layout (uint8, any alignment; the byte order of set_byte_order): every sample
        sign-extended from bps bytes.  Returns torch.int32 [nblocks, nch, ns].  Asynchronous."""
        import torch

        nblocks = self._nblocks(d_src)
        if d_out is None:
            d_out = torch.empty((nblocks, self.nch, self.ns), dtype=torch.int32, device=d_src.device)
        assert d_out.is_cuda and d_out.dtype == torch.int32 and d_out.is_contiguous() and d_out.numel() == nblocks * self.nch * self.ns
        st = self._stream(stream, d_src.device)
        self._call("rspt_hip_native_to_i32_batch_dev", d_src.data_ptr() if nblocks else None, d_out.data_ptr() if nblocks else None, nblocks, st)
        return d_out

    def from_planar_i32(self, d_planar, d_out=None, stream=None):
        """The reference's convert_i32_to_native (utils.cpp:51-121; rspt_hip.h: rspt_hip_i32_to_native_batch_dev): int32
        [nblocks, nch, ns] on the device -> the blocks in the native layout, the low bps bytes of every value kept (the byte order
        of set_byte_order).  Returns torch.uint8 [nblocks, block_bytes]; d_out may sit at any address.  Asynchronous."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        if d_out is None:
            d_out = torch.empty((nblocks, self.block_bytes), dtype=torch.uint8, device=d_planar.device)
        assert d_out.is_cuda and d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() == nblocks * self.block_bytes
        st = self._stream(stream, d_planar.device)
        self._call("rspt_hip_i32_to_native_batch_dev", d_planar.data_ptr() if nblocks else None, d_out.data_ptr() if nblocks else None, nblocks, st)
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
        return prdn, self._cr_behind(d_src.device, stream, d_consumed, (d_dst, d_sizes, d_out, d_consumed))

    def _cr_behind(self, device, stream, d_consumed, temporaries):
        """block_bytes / consumed size on the call's stream; the round trip's temporaries go back to torch's pool only once the
        caller's stream is past them"""
        import torch

        if stream is None:
            return float(self.block_bytes) / d_consumed.to(torch.float64)
        ext = torch.cuda.ExternalStream(stream, device=device)
        with torch.cuda.stream(ext):
            cr = float(self.block_bytes) / d_consumed.to(torch.float64)
        for t in temporaries:
            t.record_stream(ext)
        return cr

    def roundtrip_quality_planar(self, d_planar, stream=None):
        """roundtrip_quality for samples that live in int32: compress_planar_batch -> decompress_planar_batch ->
        prdn_planar_batch on one stream with no host synchronisation in between; d_planar is a torch.int32 cuda tensor
        [nblocks, nch, ns], only read.  Returns (prdn, cr) as roundtrip_quality does.  PRDN is taken against the matrix AS GIVEN:
        on a handle of bps < 4, values outside the sample width are cut by the packer but not by PRDN, which reads the whole
        int32.  That differs from the reference's test_packer_, which converts from native first; for values inside the sample
        width it is test_packer_ exactly, and equals roundtrip_quality(from_planar_i32(d_planar))."""
        import torch

        nblocks = self._nblocks(d_planar, torch.int32, self.nch * self.ns)
        d_dst, d_sizes = self.compress_planar_batch(d_planar, stream=stream)
        d_out, d_consumed = self.decompress_planar_batch(d_dst, nblocks, d_dst.shape[1], stream=stream)
        prdn = self.prdn_planar_batch(d_planar, d_out, stream=stream)
        return prdn, self._cr_behind(d_planar.device, stream, d_consumed, (d_dst, d_sizes, d_out, d_consumed))

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
    rc = lib().rspt_hip_design_iir(t, int(order), float(fs), float(lo), float(hi), _dptr(num),
                                   _dptr(den), C.byref(n))
    if rc != 0:
        raise RsptHipError("rspt_hip_design_iir", rc)
    return num[: n.value].copy(), den[: n.value].copy()


def new_xdelta_hzr(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode, device=0):
    return SignalPacker(KIND_XDELTA_HZR, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, nr_bytes_to_encode, device)


def new_hzr(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0):
    return SignalPacker(KIND_HZR, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 4, device)


def _with_quantizer(pk, quality, nb):
    if quality is not None or nb is not None:
        try:
            pk.set_quantizer(quality, nb)
        except Exception:
            pk.close()
            raise
    return pk


def new_dct(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0, quality=None, nb=None):
    """quality, nb: SignalPacker.set_quantizer (None: the reference's 128 and 2)"""
    return _with_quantizer(SignalPacker(KIND_DCT, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 2, device), quality, nb)


def new_bytes(nbytes, device=0):
    """libhzr on raw bytes (RSPT_HIP_KIND_BYTES): a handle for buffers of `nbytes` bytes; its streams are hzr_encode's"""
    return SignalPacker(KIND_BYTES, 1, 1, nbytes, 1, device)


def hzr_max_compressed_size(n):
    """hzr_max_compressed_size (host only: no device needed)"""
    return lib().rspt_hip_hzr_max_compressed_size(n)


def new_hadamard(bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, device=0, quality=None, nb=None):
    """quality, nb: SignalPacker.set_quantizer (None: the reference's 1 and 3)"""
    return _with_quantizer(SignalPacker(KIND_HADAMARD, bytes_per_channel, nr_of_channels, nr_of_samples_in_each_channel, 3, device), quality, nb)


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

    def set_quantizer(self, quality, nb):
        """rspt_cxx_set_quantizer (include/signal_packer.h) on a dct / hadamard instance; raises RsptHipError where it is refused"""
        rc = self._L.rspt_cxx_set_quantizer(self._p, float(quality), int(nb))
        if rc != 0:
            raise RsptHipError("rspt_cxx_set_quantizer", rc)

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
