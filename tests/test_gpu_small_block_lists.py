"""Small hzr blocks through k_tree's one tokenization: the wave that takes a small block's histogram (at most two non-zero 4 KiB
segments) runs k_hist's compacted-row tokenizer once, keeps the entries as a list, and -- if the block is staged (Huffman, at
most 512 tokens, at most 3072 bytes of payload) -- encodes it from that list alone.  Every stream here is compared byte for
byte with hzr_encode's and decoded back; where a case is about the staged / not-staged boundary, BlockMeta::mode of the launch
is read back and must say which of the two encoders wrote the block.

The blocks are crafted byte by byte and go through the bare hzr codec (one buffer = one libhzr stream, 64 KiB per hzr block).
Two block sizes: a whole hzr block, and 3 x 4096 + 1007 bytes (a ragged last segment whose last granule holds 15 bytes).

The payload boundary.  A payload near 3072 bytes cannot be reached with 512 tokens: a payload is the tree (11 S - 1 bits for S <=
261 symbols), a code per token (the Huffman cost of 512 tokens over at most 261 symbols is at most 512 x 9 bits) and the extra
bits (at most 14 per token) -- 2870 + 4608 + 7168 bits = 1831 bytes at the very most.  So kSmallPayload never decides alone, and
the boundary is pinned as far as a block can reach it: from the token-rich side (two non-zero segments, payloads of 3071 / 3072 /
3073 bytes by the oracle's own block statistics, far more than 512 tokens: the workgroup encoder's), and by the staged block with
the longest codes this file could craft (255 distinct literal values and every run class within 512 tokens), whose payload the oracle
reports and the test prints."""

import numpy as np
import pytest

import cases
from devframe import api  # noqa: F401
from hzr_dev import Hzr, gpu_decode, gpu_encode
from streamtools import describe_mismatch

pytestmark = pytest.mark.gpu

BLOCK = 65536
SEG = 4096
RAGGED = 3 * SEG + 1007
CAP = 16662
MODE_COPY, MODE_HUFF, MODE_FILL, MODE_STAGED = 0, 1, 2, 4  # BlockMeta::mode (common.hpp); the stream's mode byte of a staged block is 1


@pytest.fixture(scope="module")
def hzr(orc):
    return Hzr(orc)


# ---- crafted blocks ---------------------------------------------------------------------------------------------------------
def val(pos, salt=0, alphabet=29):
    """a non-zero byte value for position pos (a small alphabet keeps a block a Huffman block)"""
    return 1 + (pos * 2654435761 + salt * 40503 + (pos >> 7)) % alphabet


def blk(n, positions, salt=0, alphabet=29):
    b = np.zeros(n, dtype=np.uint8)
    for p in positions:
        assert 0 <= p < n, p
        b[p] = val(p, salt, alphabet)
    return b


def nz_segments(b):
    return [s // SEG for s in range(0, b.size, SEG) if b[s : s + SEG].any()]


def facts(orc, b):
    """(class, tokens, payload bytes, non-zero segments) of one hzr block, from the oracle's block statistics"""
    hist, mode, plen = orc.hzr_block_stats(b)
    ntok, nseg = int(hist.sum()), len(nz_segments(b))
    if mode == MODE_FILL:
        return "fill", ntok, plen, nseg
    if mode == MODE_COPY:
        return "copy", ntok, plen, nseg
    if nseg > 2:
        return "hist", ntok, plen, nseg  # k_hist's block
    return ("staged" if ntok <= 512 and plen <= 3072 else "big"), ntok, plen, nseg


def run_case(api, hzr, orc, bufs, want_class=None, pk=None, decode=True):
    """bufs (one size, one hzr block or several each) as one launch: streams equal to the reference's; BlockMeta::mode of every
    hzr block says staged exactly where the oracle's statistics do; a staged block's plane bytes are zero afterwards"""
    n = bufs[0].size
    nblk = (n + BLOCK - 1) // BLOCK
    own = pk is None
    pk = pk or api.new_bytes(n)
    want = [hzr.encode(b) for b in bufs]
    got, _, _ = gpu_encode(pk, bufs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None, "buffer %d flagged" % i
        assert g == w, "buffer %d of %d bytes: %s" % (i, n, describe_mismatch(g, w))
    meta = pk.debug_read(4, len(bufs) * nblk * 16).view(np.uint32).reshape(-1, 4)
    classes = []
    for i, b in enumerate(bufs):
        for j in range(nblk):
            cls, ntok, plen, nseg = facts(orc, b[j * BLOCK : (j + 1) * BLOCK])
            classes.append(cls)
            mode = int(meta[i * nblk + j, 0])
            where = "buffer %d block %d (%s: %d tokens, %d payload bytes, %d non-zero segments)" % (i, j, cls, ntok, plen, nseg)
            if cls == "staged":
                assert mode == MODE_STAGED and int(meta[i * nblk + j, 1]) == plen, (where, meta[i * nblk + j].tolist())
            elif cls in ("big", "hist"):
                assert mode == MODE_HUFF, (where, meta[i * nblk + j].tolist())
    if want_class is not None:
        assert classes == list(want_class), classes
    if decode:
        out, used = gpu_decode(pk, got, n)
        for i, b in enumerate(bufs):
            assert int(used[i]) == len(got[i]) and out[i].tobytes() == b.tobytes(), "buffer %d does not decode to its input" % i
    if own:
        pk.close()
    return classes


# ---- segment counts, block sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [BLOCK, RAGGED])
def test_one_two_and_three_non_zero_segments(api, hzr, orc, n):
    """1 and 2 non-zero segments are k_tree's (staged), 3 are k_hist's; at the ragged size the last segment holds 1007 bytes and
    its last granule 15: once with a literal in the block's very last byte, once ending in a run"""
    last = (n - 1) // SEG
    one = blk(n, [last * SEG + p for p in range(3, min(SEG, n - last * SEG) - 40, 53)], 1)
    two = blk(n, list(range(7, SEG, 97)) + [last * SEG + p for p in range(5, n - last * SEG, 89)] + [n - 1], 2)
    two_adjacent = blk(n, [SEG + p for p in range(4000, SEG, 5)] + [2 * SEG + p for p in range(0, 200, 3)], 3)
    three = blk(n, list(range(0, SEG, 200)) + [SEG + p for p in range(0, SEG, 200)] + [last * SEG + p for p in range(0, n - last * SEG - 30, 150)], 4)
    assert two[n - 1] != 0 and one[n - 30 :].max() == 0
    assert [len(nz_segments(b)) for b in (one, two, two_adjacent, three)] == [1, 2, 2, 3]
    run_case(api, hzr, orc, [one, two, two_adjacent, three], want_class=["staged", "staged", "staged", "hist"])


# ---- token counts -----------------------------------------------------------------------------------------------------------
def packed(n, nlit, salt, at=0):
    return blk(n, range(at, at + nlit), salt)


def test_511_512_513_tokens(api, hzr, orc):
    """literals side by side from byte 0 and the zero run to the block end (three capped tokens and the remainder): 511 and 512
    tokens are staged, 513 are not -- and the same with the literals in two segments, and at the ragged size (one run token)"""
    bufs = [packed(BLOCK, t - 4, 10 + t) for t in (511, 512, 513)]
    for b, t in zip(bufs, (511, 512, 513)):
        assert facts(orc, b)[1] == t
    run_case(api, hzr, orc, bufs, want_class=["staged", "staged", "big"])
    two = []
    for t in (512, 513):
        nl = t - 4 - 1  # + the run between the two groups
        b = np.zeros(BLOCK, dtype=np.uint8)
        b[100 : 100 + nl // 2] = packed(nl // 2, nl // 2, 30 + t)
        b[8 * SEG : 8 * SEG + nl - nl // 2] = packed(nl - nl // 2, nl - nl // 2, 31 + t)
        two.append(b)
    toks = [facts(orc, b)[1] for b in two]
    run_case(api, hzr, orc, two, want_class=["staged" if t <= 512 else "big" for t in toks])
    assert 512 in toks and 513 in toks, toks
    rag = [packed(RAGGED, t - 1, 50 + t) for t in (511, 512, 513)]
    assert [facts(orc, b)[1] for b in rag] == [511, 512, 513]
    run_case(api, hzr, orc, rag, want_class=["staged", "staged", "big"])


@pytest.mark.parametrize("n, cls", [(512, "staged"), (513, "big")])
def test_a_block_of_literals_alone(api, hzr, orc, n, cls):
    """no zero byte at all: as many list entries as tokens, 512 of them fill the list to its last word (and no run reaches the
    block end); one more is neither listed nor staged"""
    b = blk(n, range(n), 60, alphabet=3)
    assert facts(orc, b)[:2] == (cls, n)
    run_case(api, hzr, orc, [b], want_class=[cls])


# ---- payload boundary -------------------------------------------------------------------------------------------------------
def two_segments_payload(orc, target, seed):
    """two non-zero segments (0 and 9) with so many literals that the payload is `target` bytes or the next reachable size"""
    for nl in range(2400, 3400):
        b = np.zeros(BLOCK, dtype=np.uint8)
        h = nl // 2
        b[:h] = cases.hash_bytes(h, seed, 1, 256)
        b[9 * SEG : 9 * SEG + nl - h] = cases.hash_bytes(nl - h, seed + 1, 1, 256)
        _, mode, plen = orc.hzr_block_stats(b)
        if mode == MODE_HUFF and plen >= target:
            return b, plen
    raise AssertionError("no literal count reaches a payload of %d bytes" % target)


def longest_codes_block():
    """255 distinct literal values, each once or twice, and runs of every class between them, in two segments: 512 tokens or fewer
    with codes as long as such a block has them (the module docstring: the payload stays far below 3072 bytes)"""
    b = np.zeros(BLOCK, dtype=np.uint8)
    gaps = [0, 1, 2, 3, 6, 7, 22, 23, 30]
    pos, v = 5, 1
    for i in range(128):
        b[pos] = v
        v += 1
        pos += 1 + gaps[i % len(gaps)]
    pos = 11 * SEG + 1
    for i in range(127):
        b[pos] = v
        v += 1
        pos += 1 + gaps[(i + 4) % len(gaps)]
    b[11 * SEG + SEG - 1] = 255
    assert v == 256 and len(set(b[b != 0].tolist())) == 255
    b[3] = 200  # (a second 200: the counts are not all equal)
    return b


def test_payload_boundary(api, hzr, orc):
    near = [two_segments_payload(orc, t, 40 + t) for t in (3071, 3072, 3073)]
    sizes = [p for _, p in near]
    assert min(sizes) <= 3072 < max(sizes), sizes  # (by the oracle's statistics of each block: on both sides of the bound)
    long_codes = longest_codes_block()
    cls, ntok, plen, nseg = facts(orc, long_codes)
    print("payload sizes from the token-rich side:", sizes, "-- longest-codes staged block:", ntok, "tokens,", plen, "payload bytes")
    assert cls == "staged" and nseg == 2 and ntok <= 512 and plen > 600
    run_case(api, hzr, orc, [b for b, _ in near] + [long_codes], want_class=["big", "big", "big", "staged"])


# ---- entry positions --------------------------------------------------------------------------------------------------------
def test_entry_positions(api, hzr, orc):
    """lane 0 and lane 63 of every row, byte 0 and byte 15 of a granule, a segment's first and last byte, neighbours across a
    granule seam and across the seam of two segments; the block's very last byte a literal, and the block ending in a run"""
    rows = [r * 1024 + g * 16 + by for r in range(4) for g in (0, 63) for by in (0, 15)]
    a = blk(BLOCK, [2 * SEG + p for p in rows] + [BLOCK - 1], 1)
    b = blk(BLOCK, [5 * SEG, 5 * SEG + 15, 5 * SEG + 16, 6 * SEG - 1, 6 * SEG, 6 * SEG + 1023, 6 * SEG + 1024], 2)  # ends in a run
    c = blk(BLOCK, [0, SEG - 1, 15 * SEG, BLOCK - 16, BLOCK - 1], 3)
    d = blk(RAGGED, [0, 15, 3 * SEG + 992, 3 * SEG + 1006], 4)  # the short last granule: its first and its last byte
    e = blk(RAGGED, [SEG - 1, 3 * SEG + 991], 5)                 # ends in a run of the whole short granule
    first = blk(BLOCK, [0], 6)
    run_case(api, hzr, orc, [a, b, c, first], want_class=["staged"] * 4)
    run_case(api, hzr, orc, [d, e], want_class=["staged", "staged"])


# ---- long runs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [CAP - 1, CAP, CAP + 1, 2 * CAP, 2 * CAP + 1])
def test_runs_around_the_cap_between_two_literals(api, hzr, orc, R):
    """a run of R zeros between the last byte of segment 0 and a literal: across all-zero segments, then the run that reaches the
    block end -- 44777 zeros and fewer, more than two capped tokens at the smaller R"""
    b = blk(BLOCK, [SEG - 1, SEG + R], R)
    assert b[SEG : SEG + R].max() == 0 and len(nz_segments(b)) == 2
    ends = blk(BLOCK, [BLOCK - 2 - R, BLOCK - 1], R + 1)  # the same run in front of a literal in the block's last byte
    assert ends[BLOCK - 1 - R : BLOCK - 1].max() == 0
    run_case(api, hzr, orc, [b, ends], want_class=["staged", "staged"])


RAGGED_LONG = 12 * SEG + 1007  # the ragged shape with room for three capped runs (the 3 x 4096 + 1007 block holds no run of 16661)


@pytest.mark.parametrize("R", [CAP - 1, CAP, CAP + 1, 2 * CAP, 2 * CAP + 1, 3 * CAP])
def test_runs_around_the_cap_that_end_the_block(api, hzr, orc, R):
    """the block's last literal has exactly R zeros behind it, up to the block end: at R = k x 16662 the run is capped tokens alone --
    the histogram counts symbol 260 only, the list's last entry emits no remainder token and no literal, and the payload ends on a
    capped token.  Alone in the block and behind a literal of another segment, at 65536 bytes and at a ragged size"""
    bufs = [blk(BLOCK, [BLOCK - 1 - R], R), blk(BLOCK, [5, BLOCK - 1 - R], R + 1)]
    rag = [blk(RAGGED_LONG, [RAGGED_LONG - 1 - R], R + 2), blk(RAGGED_LONG, [9, RAGGED_LONG - 1 - R], R + 3)]
    for b in bufs + rag:
        assert b[b.size - R :].max() == 0 and b[b.size - R - 1] != 0 and len(nz_segments(b)) <= 2
    run_case(api, hzr, orc, bufs, want_class=["staged", "staged"])
    run_case(api, hzr, orc, rag, want_class=["staged", "staged"])


def test_runs_of_more_than_two_caps(api, hzr, orc):
    """one literal and nothing else: runs of more than 3 x 16662 zeros in front of it, behind it, and on both sides"""
    bufs = [blk(BLOCK, [BLOCK - 1], 1), blk(BLOCK, [0], 2), blk(BLOCK, [100, BLOCK - 1], 3), blk(BLOCK, [2 * CAP + 5], 4), blk(BLOCK, [3 * CAP], 5),
            blk(BLOCK, [3 * CAP - 1, 3 * CAP + 1], 6)]
    run_case(api, hzr, orc, bufs, want_class=["staged"] * len(bufs))


# ---- tokenizer fall-backs ---------------------------------------------------------------------------------------------------
def granules(seg, count, per=1, salt=0, n=BLOCK):
    """`count` non-zero granules spread over segment `seg`, `per` literals each"""
    idx = [0, 15, 7, 3, 11, 1, 13, 5, 9, 2][:per]
    return [seg * SEG + ((i * 256) // count) * 16 + by for i in range(count) for by in idx]


def test_64_and_65_non_zero_granules(api, hzr, orc):
    """64 non-zero granules of a segment are compacted into one row of lanes, 65 go row by row: both lists are complete and both
    blocks staged; the same beside a second non-zero segment"""
    bufs = [blk(BLOCK, granules(3, 64), 1), blk(BLOCK, granules(3, 65), 2), blk(BLOCK, granules(3, 64, 2) + granules(12, 65), 3),
            blk(BLOCK, granules(0, 65) + granules(15, 64), 4)]
    run_case(api, hzr, orc, bufs, want_class=["staged"] * 4)


def test_more_than_512_entries_in_a_segment(api, hzr, orc):
    """a segment with more entries than a list holds, beside a second non-zero segment: 64 granules x 9 literals (compacted, too
    many entries for the queue), 260 granules x 2 (row by row, the list overflows in the fourth row), a row of 600 literals (more
    than the queue takes: every lane walks its own), and two whole segments of literals -- none staged, every stream right"""
    a = blk(BLOCK, granules(2, 64, 9) + granules(9, 5), 1)
    b = blk(BLOCK, [4 * SEG + g * 16 + by for g in range(256) for by in (2, 9)] + [4 * SEG + 4080, 4 * SEG + 4090] + granules(5, 3), 2)
    c = blk(BLOCK, [7 * SEG + 1024 + p for p in range(600)] + granules(8, 2), 3)
    d = blk(BLOCK, list(range(6 * SEG, 8 * SEG)), 4, alphabet=5)
    assert [int(np.count_nonzero(x[s * SEG : (s + 1) * SEG])) for x, s in ((a, 2), (b, 4), (c, 7))] == [576, 514, 600]
    run_case(api, hzr, orc, [a, b, c, d], want_class=["big"] * 4)


# ---- symbol counts ----------------------------------------------------------------------------------------------------------
def test_one_literal_value_and_256_of_them(api, hzr, orc):
    one = np.zeros(BLOCK, dtype=np.uint8)
    one[[9 * SEG + p for p in range(0, 2000, 37)]] = 7
    every = np.zeros(BLOCK, dtype=np.uint8)  # the 255 non-zero values, 100 of them twice, and the literal zero (a run of one) between those
    every[SEG : SEG + 255] = np.arange(1, 256)
    every[14 * SEG + 2 : 14 * SEG + 2 + 2 * 100 : 2] = np.arange(1, 101)
    cls, ntok, plen, nseg = facts(orc, every)
    hist = orc.hzr_block_stats(every)[0]
    assert int(np.count_nonzero(hist[:256])) == 256 and ntok <= 512, (int(np.count_nonzero(hist[:256])), ntok)
    run_case(api, hzr, orc, [one, every], want_class=["staged", "staged"])


# ---- clean-block invariant --------------------------------------------------------------------------------------------------
def test_dense_small_dense_small_launches_on_one_handle(api, hzr, orc):
    """a staged block leaves its plane bytes zero: the second small launch, with its literals at other places, shows no stale
    byte of the first, and the workspace plane reads all zero behind each small launch"""
    n = 2 * BLOCK
    pk = api.new_bytes(n)
    small1 = [np.concatenate([blk(BLOCK, granules(1, 40, 2) + granules(6, 64), 1), blk(BLOCK, [0, BLOCK - 1], 2)]),
              np.concatenate([blk(BLOCK, granules(15, 65), 3), packed(BLOCK, 500, 4, at=3 * SEG - 250)])]
    small2 = [np.concatenate([blk(BLOCK, granules(2, 30) + granules(7, 10, 3), 5), blk(BLOCK, [77], 6)]),
              np.concatenate([blk(BLOCK, granules(14, 3), 7), blk(BLOCK, granules(3, 20), 8)])]
    dense = lambda r: [cases.hash_bytes(n, 900 + 2 * r), cases.hash_bytes(n, 901 + 2 * r)]  # noqa: E731
    for r, bufs in enumerate([dense(0), small1, dense(1), small2, small1]):
        small = r in (1, 3, 4)
        run_case(api, hzr, orc, bufs, want_class=["staged"] * 4 if small else None, pk=pk, decode=False)
        if small:
            stride = (n + 255) // 256 * 256
            planes = pk.debug_read(0, 2 * stride)
            assert planes.size == 2 * stride and not planes.any(), "a staged block left %d non-zero plane bytes" % int(np.count_nonzero(planes))
    pk.close()


# ---- launch size ------------------------------------------------------------------------------------------------------------
def test_1100_blocks_in_one_launch(api, hzr, orc):
    """more than two small blocks per workgroup slot of k_tree's wave of a launch: staged blocks of several shapes, blocks whose
    list overflows, k_hist's blocks and all-zero blocks in turn"""
    shapes = [blk(BLOCK, granules(3, 64), 1), blk(BLOCK, [BLOCK - 1], 2), blk(BLOCK, granules(2, 64, 9) + granules(9, 5), 3), np.zeros(BLOCK, dtype=np.uint8),
              blk(BLOCK, granules(0, 65) + granules(15, 64), 4), blk(BLOCK, granules(1, 9) + granules(5, 9) + granules(11, 9), 5), packed(BLOCK, 508, 6)]
    want = ["staged", "staged", "big", "fill", "staged", "hist", "staged"]
    assert [facts(orc, s)[0] for s in shapes] == want
    nblk = 1100
    buf = np.concatenate([shapes[i % len(shapes)] for i in range(nblk)])
    pk = api.new_bytes(buf.size)
    got, _, _ = gpu_encode(pk, [buf])
    w = hzr.encode(buf)
    assert got[0] == w, describe_mismatch(got[0], w)
    meta = pk.debug_read(4, nblk * 16).view(np.uint32).reshape(-1, 4)
    modes = {"staged": MODE_STAGED, "big": MODE_HUFF, "hist": MODE_HUFF, "fill": MODE_FILL}
    assert meta[:, 0].tolist() == [modes[want[i % len(shapes)]] for i in range(nblk)]
    pk.close()


# ---- the benchmark's routes -------------------------------------------------------------------------------------------------
def test_xdelta_hzr_two_blocks_of_64_channels(api, orc):
    """the benchmark's shape: planes 1 and 2 of the synthetic signal are mostly small blocks"""
    import torch

    from rspt_amd import synth

    nch, ns, B = 64, 65536, 2
    pk = api.new_xdelta_hzr(4, nch, ns, 3)
    po = orc.packer("xdelta_hzr", 4, nch, ns, 3)
    d_src = synth.synth_batch_native(B, nch, ns, first_block=36, device="cuda")
    src = d_src.cpu().numpy()
    d_dst, d_sizes = pk.compress_batch(d_src)
    torch.cuda.synchronize()
    sizes, out = d_sizes.cpu().numpy(), d_dst.cpu().numpy()
    meta = pk.debug_read(4, B * 4 * 64 * 16).view(np.uint32).reshape(B, 4, 64, 4)
    assert int((meta[:, 1:3, :, 0] == MODE_STAGED).sum()) >= 40, "hardly any staged block: not the data this test is about"
    for b in range(B):
        w = po.compress(src[b])
        g = out[b, : sizes[b]].tobytes()
        assert g == w, "block %d: %s" % (b, describe_mismatch(g, w))
    pk.close()


def test_xdelta_hzr_escalating_from_one_plane(api, orc):
    """five times the amplitude, started at nb = 1: the call escalates to nb = 3, and the planes it adds bring small blocks"""
    from rspt_amd import synth

    src = synth.to_native(synth.synth_i32(8, 65536, 37) * 5).numpy()
    want = orc.packer("xdelta_hzr", 4, 8, 65536, 1).compress(src)
    assert want == orc.packer("xdelta_hzr", 4, 8, 65536, 3).compress(src)
    pk = api.new_xdelta_hzr(4, 8, 65536, 1)
    got = pk.compress(src)
    assert got == want, describe_mismatch(got, want)
    pk.close()
