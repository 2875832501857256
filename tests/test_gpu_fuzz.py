"""Randomised GPU parity for the hzr kernels: byte streams of every density go through a 1-channel 8-bit `hzr` packer
(plane 0 of its stream IS hzr_encode(data), signal_packer_base.cpp:69-82) and must equal the oracle's encoding bit for
bit; the GPU decoder must give the bytes back.  The densities (tests/fuzz_cases.py) steer the encoder through all of its row
paths."""
import struct

import numpy as np
import pytest

from devframe import api  # noqa: F401
from fuzz_cases import KINDS, gen
from streamtools import describe_mismatch, parse_stream

pytestmark = pytest.mark.gpu


SIZES = [65536, 65536 * 3 + 1234, 4097, 200000, 16, 70000]
CASES = [(k, SIZES[(i + j) % len(SIZES)], 100 * i + j) for i, k in enumerate(KINDS) for j in range(3)]


@pytest.mark.parametrize("kind,n,seed", CASES)
def test_random_stream_bit_exact_and_back(api, orc, kind, n, seed):
    data = gen(seed, n, kind)
    pk = api.new_hzr(1, 1, n)
    got = pk.compress(data, dst_max_len=pk.max_compressed_size)
    p = parse_stream(got)
    o0 = p["planes"][0]["offset"]
    chunk0 = got[o0 + 4 : o0 + 4 + p["planes"][0]["len"]]
    want = orc.hzr_encode(data)
    assert chunk0 == want, "%s n=%d seed=%d: %s" % (
        kind, n, seed, describe_mismatch(b"\0" + struct.pack("<I", len(chunk0)) + chunk0, b"\0" + struct.pack("<I", len(want)) + want))
    ok, m = orc.hzr_verify(chunk0)
    assert ok and m == n
    dec, used = pk.decompress(got)
    assert used == len(got) and dec == data.tobytes()
    pk.close()


def test_random_batch_matches_single_calls(api, orc):
    """many different blocks in one launch (the work queues, the segment offsets and the side stream see a real mix)"""
    import torch

    n = 65536 * 2 + 777
    kinds = [KINDS[i % len(KINDS)] for i in range(24)]
    blocks = [gen(1000 + i, n, k) for i, k in enumerate(kinds)]
    pk = api.new_hzr(1, 1, n)
    d_src = torch.from_numpy(np.stack(blocks)).cuda()
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.zeros((len(blocks), stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(len(blocks), dtype=torch.int64, device="cuda")
    pk.compress_batch(d_src, d_dst, d_sizes, stride)
    torch.cuda.synchronize()
    po = orc.packer("hzr", 1, 1, n)
    for i, data in enumerate(blocks):
        got = d_dst[i, : int(d_sizes[i])].cpu().numpy().tobytes()
        want = po.compress(data)
        assert got == want, "block %d (%s): %s" % (i, kinds[i], describe_mismatch(got, want))
    out, used = pk.decompress_batch(d_dst, len(blocks), stride)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(np.stack(blocks))) and torch.equal(used, d_sizes)
    pk.close()


def test_blocks_with_one_populated_segment_every_launch(api, orc):
    """hzr blocks with a single non-zero 4 KiB segment that holds more tokens than the one-wave encoder takes: k_tree takes their
    histogram itself and k_encode counts each wave's tokens once more for the segment offsets (own_bits).  In that pass the
    sparse-row queue of wave 0 used to overlap the last bins of wave 15's histogram in LDS -- wave 15 counts the run that reaches
    the block end right there -- and about every second launch produced a damaged payload (found by tools/soak.py, round 4).
    A race: so the same batch many times over."""
    import torch

    r = np.random.default_rng(77)
    blocks = []
    for seg in (0, 0, 3, 15, 0, 7):
        x = np.zeros(65536 * 2 + 4096, dtype=np.uint8)
        for blk in range(3):
            n = 4096 if blk < 2 else 2048
            lo = blk * 65536 + (seg * 4096 if blk < 2 else 0)
            pos = lo + np.sort(r.choice(n, size=n // 6, replace=False))
            x[pos] = r.integers(1, 256, pos.size)
        blocks.append(x)
    n = blocks[0].size
    pk = api.new_hzr(1, 1, n)
    po = orc.packer("hzr", 1, 1, n)
    want = [po.compress(b) for b in blocks]
    d_src = torch.from_numpy(np.stack(blocks)).cuda()
    stride = (pk.max_compressed_size + 255) // 256 * 256
    for rep in range(40):
        d_dst = torch.zeros((len(blocks), stride), dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(len(blocks), dtype=torch.int64, device="cuda")
        pk.compress_batch(d_src, d_dst, d_sizes, stride)
        torch.cuda.synchronize()
        for i, w in enumerate(want):
            got = d_dst[i, : int(d_sizes[i])].cpu().numpy().tobytes()
            assert got == w, "launch %d block %d: %s" % (rep, i, describe_mismatch(got, w))
    pk.close()
