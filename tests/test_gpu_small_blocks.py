"""Small hzr blocks (at most 2 non-zero 4 KiB segments, 512 tokens, 3 KiB of payload) are encoded by the wave of k_tree
that builds their code table, staged, and copied to their stream offset by k_encode.  These tests drive batches made
mostly of such blocks at every boundary of the class, against the oracle byte for byte.

The inputs are raw hzr blocks: plane 0 of a 1-channel 8-bit `hzr` packer is hzr_encode(data), 64 KiB per hzr block, so every
hzr block below is built byte by byte, and the oracle's own block statistics (tokens, mode, payload bytes) confirm that a
block sits where its name says.

A payload of 3 KiB cannot be reached with 512 tokens (a token is at most a 22-bit code word and 14 extra bits), so the
payload boundary is approached from the token-rich side: blocks of two non-zero segments whose payload is at, just under and
just over 3072 bytes have more than 512 tokens and belong to the workgroup encoder, next to the staged ones in one stream."""
import numpy as np
import pytest

import cases
from devframe import api  # noqa: F401
from streamtools import describe_mismatch

pytestmark = pytest.mark.gpu

HB = 65536
MODE_COPY, MODE_HUFF, MODE_FILL = 0, 1, 2


def _lits(n, seed, lo=1, hi=256):
    return cases.hash_bytes(n, seed, lo, hi)


def _blk_zero():
    return np.zeros(HB, dtype=np.uint8)


def _blk_packed(n, seed, at=0, size=HB):
    """n literals side by side from byte `at`: with at = 0 the tokens are n literals and the run to the block end"""
    b = np.zeros(size, dtype=np.uint8)
    b[at : at + n] = _lits(n, seed)
    return b


def _blk_scattered(positions, seed, size=HB):
    b = np.zeros(size, dtype=np.uint8)
    pos = np.asarray(positions)
    b[pos] = _lits(len(pos), seed)
    return b


def _blk_two_segments_payload(orc, target, seed):
    """two non-zero segments (0 and 9) filled with so many random literals that the payload is `target` bytes (or the nearest
    reachable size at or above it): far more than 512 tokens"""
    best = None
    for n in range(2400, 3400):
        b = np.zeros(HB, dtype=np.uint8)
        h = n // 2
        b[:h] = _lits(h, seed)
        b[9 * 4096 : 9 * 4096 + (n - h)] = _lits(n - h, seed + 1)
        _, mode, plen = orc.hzr_block_stats(b)
        if mode == MODE_HUFF and plen >= target:
            best = (b, plen)
            break
    assert best is not None, "no literal count reaches a payload of %d bytes" % target
    return best


def _small_block_cases(orc):
    """name -> (block, expected class); class: 'fill', 'copy', 'staged' (small), 'big' (Huffman, workgroup encoder)"""
    out = {}
    out["zero"] = (_blk_zero(), "fill")
    out["const_0x41"] = (np.full(HB, 0x41, dtype=np.uint8), "fill")
    out["plain_copy"] = (cases.hash_bytes(HB, 77), "copy")
    # one and two non-zero segments, few tokens
    out["one_seg_mid"] = (_blk_scattered(5 * 4096 + np.arange(0, 4096, 41), 3), "staged")
    out["two_seg_first_last"] = (_blk_scattered(np.concatenate([np.arange(7, 4096, 97), 15 * 4096 + np.arange(3, 4096, 89)]), 4), "staged")
    out["two_seg_adjacent"] = (_blk_scattered(np.concatenate([4096 * 3 + np.arange(4000, 4096, 5), 4096 * 4 + np.arange(0, 200, 3)]), 5), "staged")
    out["three_seg"] = (_blk_scattered(np.concatenate([np.arange(0, 4096, 200), 4096 * 6 + np.arange(0, 4096, 200), 4096 * 12 + np.arange(0, 4096, 200)]), 6), "big")
    # token boundary: n literals from byte 0 and the zero run to the block end (3 capped run tokens + the remainder)
    for want in (511, 512, 513):
        out["tokens_%d" % want] = (_blk_packed(want - 4, 10 + want), "staged" if want <= 512 else "big")
    # the same boundary with the literals in two segments
    for want in (512, 513):
        b = np.zeros(HB, dtype=np.uint8)
        n = want - 4 - 1  # + the run between the two groups
        b[100 : 100 + n // 2] = _lits(n // 2, 30 + want)
        b[8 * 4096 : 8 * 4096 + (n - n // 2)] = _lits(n - n // 2, 31 + want)
        out["tokens_%d_two_seg" % want] = (b, None)  # (class asserted from the oracle's token count below)
    # a literal in the very last byte: no run reaches the block end; and one in the first byte only
    out["last_byte"] = (_blk_scattered([HB - 1], 8), "staged")
    out["last_granule_full"] = (_blk_packed(16, 9, at=HB - 16), "staged")
    out["first_byte"] = (_blk_scattered([0], 9), "staged")
    out["segment_edges"] = (_blk_scattered([4095, 4096, 8191], 11), "staged")
    # runs of every token class between literals (1, 2, 3-6, 7-22, 23-278, >= 279) inside one segment
    out["run_classes"] = (_blk_scattered(2 * 4096 + np.cumsum([0, 2, 3, 4, 7, 8, 23, 24, 279, 280, 400, 700]), 12), "staged")
    # deep code table: Fibonacci counts
    fib = cases._fib_counts(12)
    b = np.zeros(HB, dtype=np.uint8)
    b[4096 : 4096 + fib.size] = fib
    out["fib_tree"] = (b, None)
    # payload boundary (3072 bytes) from the token-rich side
    for target in (3071, 3072, 3073):
        blk, plen = _blk_two_segments_payload(orc, target, 40 + target)
        out["payload_%d" % plen + ("" if plen == target else "_for_%d" % target)] = (blk, "big")
    return out


def _classify(orc, blk):
    hist, mode, plen = orc.hzr_block_stats(blk)
    if mode == MODE_FILL:
        return "fill"
    if mode == MODE_COPY:
        return "copy"
    nseg = sum(1 for s in range(0, blk.size, 4096) if blk[s : s + 4096].any())
    return "staged" if nseg <= 2 and int(hist.sum()) <= 512 and plen <= 3072 else "big"


def _sample_blocks(orc):
    """sample blocks (each a sequence of hzr blocks + a short last one) and the class of every hzr block"""
    named = _small_block_cases(orc)
    for name, (blk, want) in named.items():
        got = _classify(orc, blk)
        assert want is None or got == want, "case %s is %s, meant to be %s (tokens %d)" % (name, got, want, int(orc.hzr_block_stats(blk)[0].sum()))
    for want in (511, 512, 513):
        assert int(orc.hzr_block_stats(named["tokens_%d" % want][0])[0].sum()) == want
    assert _classify(orc, named["tokens_512_two_seg"][0]) == "staged" and _classify(orc, named["tokens_513_two_seg"][0]) == "big"
    order = list(named)
    tail = _blk_scattered([0, 17, 500, 999], 13, size=1000)  # the short last hzr block: small too
    # A: every case once, Fill and PlainCopy neighbours between the small ones
    a = [named[n][0] for n in order]
    # B: mostly small blocks, shuffled order
    rot = order[5:] + order[:5]
    b = [named[n][0] for n in rot if n != "plain_copy"] + [named["one_seg_mid"][0]]
    # C: the heavy one (several PlainCopy blocks): its stream is the longest
    c = [named["plain_copy"][0]] * 6 + [named[n][0] for n in order[: len(a) - 6]]
    assert len(a) == len(b) == len(c)
    blocks = [np.concatenate(x + [tail]) for x in (a, b, c)]
    return blocks, len(a)


def _run_batch(api_mod, pk, blocks, dst_stride=None):
    import torch

    d_src = torch.from_numpy(np.stack(blocks)).cuda()
    d_dst, d_sizes = pk.compress_batch(d_src, dst_stride=dst_stride)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy(), d_sizes.cpu().numpy()


def test_small_block_boundaries_bit_exact(api, orc):
    blocks, _ = _sample_blocks(orc)
    n = blocks[0].size
    po = orc.packer("hzr", 1, 1, n, 4)
    want = [po.compress(b) for b in blocks]
    pk = api.new_hzr(1, 1, n)
    out, sizes = _run_batch(api, pk, blocks)
    for i, w in enumerate(want):
        got = out[i, : sizes[i]].tobytes()
        assert got == w, "sample block %d: %s" % (i, describe_mismatch(got, w))
        dec, used, _ = po.decompress(got)
        assert dec == blocks[i].tobytes() and used == len(got)
    pk.close()


def test_second_launch_on_one_handle_is_identical(api, orc):
    """the clean-block wipe and the staging area carry nothing from one launch into the next"""
    blocks, _ = _sample_blocks(orc)
    n = blocks[0].size
    po = orc.packer("hzr", 1, 1, n, 4)
    want = [po.compress(b) for b in blocks]
    pk = api.new_hzr(1, 1, n)
    out1, sizes1 = _run_batch(api, pk, blocks)
    out2, sizes2 = _run_batch(api, pk, blocks)
    assert (sizes1 == sizes2).all()
    for i, w in enumerate(want):
        g1, g2 = out1[i, : sizes1[i]].tobytes(), out2[i, : sizes2[i]].tobytes()
        assert g1 == g2, "launch 2 differs from launch 1 in sample block %d: %s" % (i, describe_mismatch(g2, g1))
        assert g1 == w, describe_mismatch(g1, w)
    # other data in the same slots, then the first batch again: nothing of the batch in between shows
    other = [blocks[2], blocks[0], blocks[1]]
    out3, sizes3 = _run_batch(api, pk, other)
    for i, src in enumerate(other):
        assert out3[i, : sizes3[i]].tobytes() == po.compress(src)
    out4, sizes4 = _run_batch(api, pk, blocks)
    for i, w in enumerate(want):
        assert out4[i, : sizes4[i]].tobytes() == w
    pk.close()


def test_stream_that_does_not_fit_and_the_handle_afterwards(api, orc):
    blocks, _ = _sample_blocks(orc)
    n = blocks[0].size
    po = orc.packer("hzr", 1, 1, n, 4)
    want = [po.compress(b) for b in blocks]
    lens = [len(w) for w in want]
    assert lens[2] > max(lens[0], lens[1]) + 4096
    stride = (max(lens[0], lens[1]) + 255) // 256 * 256  # the first two fit, the heavy one does not
    pk = api.new_hzr(1, 1, n)
    import torch

    d_src = torch.from_numpy(np.stack(blocks)).cuda()
    d_dst = torch.full((3, stride), 0xA5, dtype=torch.uint8, device="cuda")
    d_dst, d_sizes = pk.compress_batch(d_src, d_dst=d_dst, dst_stride=stride)
    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy()
    out = d_dst.cpu().numpy()
    for i in (0, 1):
        assert out[i, : sizes[i]].tobytes() == want[i], describe_mismatch(out[i, : sizes[i]].tobytes(), want[i])
    assert sizes[2] < 0 and (int(sizes[2]) & ((1 << 63) - 1)) == lens[2]  # flagged, with the length it would have had
    assert (out[2] == 0xA5).all(), "nothing of a stream that does not fit is written"
    # the handle afterwards: the same batch with room for every stream, and once more
    for _ in range(2):
        out, sizes = _run_batch(api, pk, blocks)
        for i, w in enumerate(want):
            got = out[i, : sizes[i]].tobytes()
            assert got == w, "sample block %d after the too-small call: %s" % (i, describe_mismatch(got, w))
    pk.close()


def test_xdelta_batch_twice_on_one_handle(api, orc):
    """signal-shaped data (planes 1-2 are mostly small blocks) through the flagship packer, two launches on one handle"""
    import torch

    from rspt_amd import synth

    nch, ns, B = 16, 65536, 3
    pk = api.new_xdelta_hzr(4, nch, ns, 3)
    po = orc.packer("xdelta_hzr", 4, nch, ns, 3)
    d_src = synth.synth_batch_native(B, nch, ns, first_block=3, device="cuda")
    src = d_src.cpu().numpy()
    for launch in range(2):
        d_dst, d_sizes = pk.compress_batch(d_src)
        torch.cuda.synchronize()
        sizes = d_sizes.cpu().numpy()
        out = d_dst.cpu().numpy()
        for b in range(B):
            w = po.compress(src[b])
            got = out[b, : sizes[b]].tobytes()
            assert got == w, "launch %d, block %d: %s" % (launch, b, describe_mismatch(got, w))
    pk.close()
