"""The hzr byte codec on both sides, for the tests that hold one against the other (tests/test_hzr_bytes.py,
tests/test_gpu_small_block_lists.py, tests/test_gpu_sparse_segments.py): libhzr's three calls -- the compiled reference where
oracle/_ref is there, else the oracle's restatement -- and a batch of buffers or streams through a device packer."""
import ctypes as C

import numpy as np

BAD = 1 << 63  # the flag in a block's size / consumed word


class Hzr:
    """hzr_encode / hzr_decode / hzr_verify of the reference (or of its restatement)"""

    def __init__(self, orc):
        from oracle import oracle

        self.orc = orc
        self.ref = oracle.Ref() if oracle.have_ref() else None
        self.enc = self.ref or orc

    def encode(self, data):
        return self.enc.hzr_encode(data)

    def decode(self, stream, n):
        """-> bytes, or None where hzr_decode fails (trailing bytes are not the decoder's business here: the restatement)"""
        try:
            return self.orc.hzr_decode(stream, n)[0]
        except RuntimeError:
            return None

    def verify(self, stream):
        """(ok, decoded size).  The reference checksums a block before it knows that the block ends inside the stream
        (hzr_decode.c:606-618): a block's length of zeros behind the stream keeps that read inside our memory."""
        s = np.frombuffer(bytes(stream), dtype=np.uint8)
        padded = np.zeros(s.size + 65536 + 16, dtype=np.uint8)
        padded[: s.size] = s
        n = C.c_size_t(0)
        f = self.ref.lib.ref_hzr_verify if self.ref else self.orc.lib.orc_hzr_verify
        ok = f(padded.ctypes.data_as(C.POINTER(C.c_uint8)), s.size, C.byref(n))
        return bool(ok), n.value


def gpu_encode(pk, bufs, dst_stride=None, fill=None):
    """-> (streams or None where flagged, raw d_dst as numpy [nb, stride], sizes)"""
    import torch

    d_src = torch.from_numpy(np.concatenate(bufs)).cuda()
    n = len(bufs)
    stride = dst_stride if dst_stride is not None else (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.full((n, stride), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
    d_dst, d_sizes = pk.compress_batch(d_src, d_dst=d_dst, dst_stride=stride)
    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().view(np.uint64)
    raw = d_dst.cpu().numpy()
    out = [None if int(s) & BAD else raw[i, : int(s)].tobytes() for i, s in enumerate(sizes)]
    return out, raw, sizes


def gpu_decode(pk, streams, n):
    """streams (bytes) through rspt_hip_decompress_batch_dev -> (outputs [len(streams), n], consumed as uint64)"""
    import torch

    stride = (max(len(s) for s in streams) + 15) // 16 * 16 + 16
    host = np.zeros((len(streams), stride), dtype=np.uint8)
    for i, s in enumerate(streams):
        host[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_out, d_used = pk.decompress_batch(torch.from_numpy(host).cuda(), len(streams), stride)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(len(streams), n), d_used.cpu().numpy().view(np.uint64)
