"""k_hist's compacted sparse segments (hist_segment_sparse: the non-zero granules of a 4 KiB segment in one row of lanes) and its
two-copy histogram, through the bare hzr codec: every stream byte for byte hzr_encode's, and decoded back.

The buffers are crafted granule by granule.  A segment is 4 rows of 64 granules of 16 bytes; a row stays sparse up to 48
non-zero granules; a segment is compacted up to 64 non-zero granules and 512 queue entries (its literals, and the run that
reaches the block end where the block ends in it) and goes row by row beyond either.  Every block has more than two non-zero
segments, so k_hist takes it, and the reference's block headers must say Huffman (mode 1) for every block of every case."""
import struct

import numpy as np
import pytest

import cases
from devframe import api  # noqa: F401
from hzr_dev import Hzr, gpu_decode, gpu_encode
from streamtools import describe_mismatch

pytestmark = pytest.mark.gpu

BLOCK = 65536
SEG = 4096
GRANULES = SEG // 16  # per segment


@pytest.fixture(scope="module")
def hzr(orc):
    return Hzr(orc)


# ---- crafted blocks ---------------------------------------------------------------------------------------------------------
def lit(pos, salt=0):
    """a non-zero byte value for position pos (a small alphabet: the block stays a Huffman block)"""
    return 1 + (pos * 2654435761 + salt * 40503 + (pos >> 7)) % 29


def put(buf, seg, granule, byte_idxs, salt=0):
    """literals at the given bytes of granule `granule` (0..255) of segment `seg`; positions past the buffer are left out"""
    for b in byte_idxs:
        pos = seg * SEG + granule * 16 + b
        if pos < buf.size:
            buf[pos] = lit(pos, salt)


def spread(count, avail=GRANULES):
    """`count` granule indices spread evenly over the first `avail` granules of a segment (each row gets its share)"""
    return [(i * avail) // count for i in range(count)]


def few_bytes(g, salt):
    """one to three byte positions of a granule, by hash"""
    h = (g * 0x9E3779B1 + salt * 0x85EBCA6B) & 0xFFFFFFFF
    return sorted({h % 16, (h >> 8) % 16, (h >> 16) % 16} if h % 3 == 2 else {h % 16, (h >> 8) % 16} if h % 3 == 1 else {h % 16})


def block_granule_counts(n, counts, salt=0):
    """a buffer of n bytes whose segment s holds counts[s % len(counts)] non-zero granules (as far as its valid bytes go: the last
    48 bytes of the buffer stay zero, so a cut buffer ends in a zero run)"""
    buf = np.zeros(n, dtype=np.uint8)
    for s in range((n + SEG - 1) // SEG):
        valid = min(SEG, n - s * SEG) - (48 if (s + 1) * SEG >= n else 0)
        avail = max(0, valid // 16)
        c = min(counts[s % len(counts)], avail)
        for g in (spread(c, avail) if c else []):
            put(buf, s, g, few_bytes(s * GRANULES + g, salt), salt)
    return buf


BOUNDARY_COUNTS = [1, 2, 63, 64, 65, 128, 0, 32]


def block_queue_boundary(lits_per_granule, last_segment_entries=None):
    """64 non-zero granules per segment (16 per row), `lits_per_granule` literals each; the last segment cut to
    `last_segment_entries` literals where given (it also queues the run that reaches the block end)"""
    buf = np.zeros(BLOCK, dtype=np.uint8)
    idxs = [0, 2, 4, 6, 8, 10, 12, 14, 15, 1][:lits_per_granule]
    for s in range(16):
        left = last_segment_entries if (s == 15 and last_segment_entries is not None) else 64 * lits_per_granule
        for g in spread(64):
            take = idxs[: max(0, min(len(idxs), left))]
            put(buf, s, g, take)
            left -= len(take)
    return buf


def block_positions():
    buf = np.zeros(BLOCK, dtype=np.uint8)
    for r in range(4):  # lane 0 and lane 63 of every row, first and last byte of the granule: the segment's first and last granule too
        put(buf, 0, 64 * r, [0, 15])
        put(buf, 0, 64 * r + 63, [0, 15])
    put(buf, 1, 5, [3])  # rows 1 and 2 all zero between occupied ones
    put(buf, 1, 3 * 64 + 40, [0, 1, 2])
    put(buf, 2, 255, [15])  # the segment's last byte; the run behind it starts in segment 3 ...
    put(buf, 4, 130, [7])  # ... and ends two segments on
    put(buf, 5, 0, [0])
    put(buf, 11, 200, [9])  # segments 6..10 zero: a run of more than 16662 that ends at a compacted literal
    put(buf, 12, 1, [0])
    put(buf, 12, 2, [15])
    put(buf, 14, 64, [15])
    put(buf, 14, 65, [0])  # neighbours across a granule seam: no zeros between them
    for g in spread(20):
        put(buf, 13, g, few_bytes(g, 7))
    put(buf, 15, 254, [14])  # the block ends in a run of 17 zeros
    assert buf[5 * SEG + 1 : 11 * SEG + 200 * 16 + 9].max() == 0 and 11 * SEG + 200 * 16 + 9 - (5 * SEG + 1) >= 16662
    return buf


def block_mixed_rows(salt=0):
    """segment s: row s % 4 dense (60 non-zero granules) while its three neighbours hold a few -- row by row -- except every
    third segment, which is sparse throughout and compacted"""
    buf = np.zeros(BLOCK, dtype=np.uint8)
    for s in range(16):
        for r in range(4):
            dense = s % 3 != 2 and r == s % 4
            for g in (range(2, 62) if dense else spread(5 + (s + r) % 7, 64)):
                put(buf, s, 64 * r + g, few_bytes(s * GRANULES + 64 * r + g, salt) if not dense else [1, 2, 5, 11], salt)
    return buf


def is_crafted_right(buf):
    """more than two non-zero segments in every block (so k_hist takes it)"""
    for b0 in range(0, buf.size, BLOCK):
        blk = buf[b0 : b0 + BLOCK]
        nz = sum(1 for s in range(0, blk.size, SEG) if blk[s : s + SEG].any())
        assert nz > 2, "block at %d has %d non-zero segments" % (b0, nz)


def block_modes(stream):
    n = struct.unpack_from("<I", stream, 0)[0]
    pos, modes = 4, []
    for _ in range((n + BLOCK - 1) // BLOCK):
        modes.append(stream[pos + 6])
        pos += 7 + struct.unpack_from("<H", stream, pos)[0] + 1
    return modes


def check(api, hzr, bufs, pk=None, crafted=None):
    """bufs (all of one size) as one batch: streams equal to the reference's, Huffman blocks throughout (for the crafted
    ones), and decoded back"""
    n = bufs[0].size
    own = pk is None
    pk = pk or api.new_bytes(n)
    want = [hzr.encode(b) for b in bufs]
    for i, b in enumerate(bufs):
        if crafted is None or crafted[i]:
            is_crafted_right(b)
            assert set(block_modes(want[i])) == {1}, ("buffer %d: the reference did not choose Huffman for every block" % i, block_modes(want[i]))
    got, _, _ = gpu_encode(pk, bufs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None, "buffer %d flagged" % i
        assert g == w, "buffer %d of %d bytes: %s" % (i, n, describe_mismatch(g, w))
    out, used = gpu_decode(pk, got, n)
    for i, b in enumerate(bufs):
        assert int(used[i]) == len(got[i]) and out[i].tobytes() == b.tobytes(), "buffer %d does not decode to its input" % i
    if own:
        pk.close()


# ---- the cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [BLOCK, 3 * SEG + 1007])
def test_granule_count_boundary(api, hzr, n):
    """1, 2, 63, 64, 65, 128, 0 and 32 non-zero granules per segment side by side: compacted, row by row and all-zero segments
    meet at segment seams; at the second size the block ends inside a segment (the virtual entry, a zero run to the end)"""
    rot = [BOUNDARY_COUNTS[(i + 2) % 8] for i in range(8)]  # (the short buffer's four segments: 63, 64, 65, 128)
    bufs = [block_granule_counts(n, BOUNDARY_COUNTS), block_granule_counts(n, rot, salt=1), block_granule_counts(n, [64, 65, 63], salt=2)]
    check(api, hzr, bufs)


@pytest.mark.parametrize("shape", ["t512", "t576", "last512"])
def test_queue_boundary(api, hzr, shape):
    """64 granules per segment: 8 literals each fill the queue exactly (512; the block's last segment, with the run that
    reaches the end, has 513 and goes row by row), 9 each are too many everywhere; and a last segment of 511 literals plus
    the end entry"""
    buf = {"t512": lambda: block_queue_boundary(8), "t576": lambda: block_queue_boundary(9), "last512": lambda: block_queue_boundary(8, 511)}[shape]()
    per_seg = [int(np.count_nonzero(buf[s * SEG : (s + 1) * SEG])) for s in range(16)]
    assert per_seg == {"t512": [512] * 16, "t576": [576] * 16, "last512": [512] * 15 + [511]}[shape]
    check(api, hzr, [buf])


def test_positions(api, hzr):
    """lanes 0 and 63, bytes 0 and 15, a segment's first and last granule, zero rows between occupied ones, a zero run past
    the 16662 cap that ends at a compacted literal, a run over a whole zero segment; also cut inside its last segment"""
    buf = block_positions()
    check(api, hzr, [buf])
    cut = buf[: 14 * SEG + 65 * 16 + 300].copy()  # ends in a zero run inside segment 14
    check(api, hzr, [cut])


def test_dense_row_beside_sparse_rows(api, hzr):
    check(api, hzr, [block_mixed_rows(0), block_mixed_rows(1)])


def test_queue_and_histogram_reuse_across_launches(api, hzr):
    """three launches on one handle, dense / crafted sparse / dense: what a launch leaves in the queues, the planes and the
    two histogram copies never shows in the next one"""
    n = 2 * BLOCK
    pk = api.new_bytes(n)
    sparse = [np.concatenate([block_granule_counts(BLOCK, BOUNDARY_COUNTS, salt=3), block_queue_boundary(8)]),
              np.concatenate([block_positions(), block_mixed_rows(2)])]
    for r in range(3):
        if r == 1:
            check(api, hzr, sparse, pk=pk)
        else:
            check(api, hzr, [cases.hash_bytes(n, 900 + 2 * r), cases.hash_bytes(n, 901 + 2 * r)], pk=pk, crafted=[False, False])
    pk.close()


def test_workgroups_with_several_blocks(api, hzr):
    """more blocks than k_hist has workgroups (two per CU), of alternating shape: consecutive blocks of one workgroup take the
    two histogram copies in turn"""
    shapes = [block_granule_counts(BLOCK, BOUNDARY_COUNTS, salt=4), block_queue_boundary(8), block_mixed_rows(3), block_positions(),
              block_granule_counts(BLOCK, [40, 64, 12], salt=5)]
    nblk = 1100
    buf = np.concatenate([shapes[i % len(shapes)] for i in range(nblk)])
    check(api, hzr, [buf])


@pytest.mark.parametrize("scale, nb0", [(1, 3), (5, 1)])
def test_xdelta_hzr_block_through_the_entry_lists(api, orc, scale, nb0):
    """8 ch x 65536 int32 of the synthetic signal: planes 1 and 2 are k_hist's medium blocks, encoded by k_encode from the
    lists the compacted segments left.  As the benchmark runs it (nb = 3 from the start), and five times the amplitude
    started at nb = 1, which escalates to nb = 3 inside the call"""
    from rspt_amd import synth

    src = synth.to_native(synth.synth_i32(8, 65536, 37) * scale).numpy()
    want = orc.packer("xdelta_hzr", 4, 8, 65536, nb0).compress(src)
    if nb0 == 1:  # (a packer that starts at 3 gives the same stream only if the escalation reaches 3, one that starts at 4 a longer one)
        assert want == orc.packer("xdelta_hzr", 4, 8, 65536, 3).compress(src) and want != orc.packer("xdelta_hzr", 4, 8, 65536, 4).compress(src)
    pk = api.new_xdelta_hzr(4, 8, 65536, nb0)
    got = pk.compress(src)
    assert got == want, describe_mismatch(got, want)
    pk.close()
