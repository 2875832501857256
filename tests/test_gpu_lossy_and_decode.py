"""GPU parity, part 2: the hadamard and dct packers and the decompress path,
through the C ABI, against the oracle and the golden fixtures.

hadamard is all-integer -> bit-exact.  dct follows the reference's arithmetic
(float32 table from host libm, float products, sequential double sums, C
truncation), so the streams are expected to be identical too; the formal gate
SURVEY.md 8(d) asks for is PRDN within 0.05 percentage points and CR within 1 %."""
import zlib

import numpy as np
import pytest

import cases
from devframe import ERR_CORRUPT, api  # noqa: F401
from streamtools import describe_mismatch, parse_stream

pytestmark = pytest.mark.gpu

PRDN_TOL = 0.05  # percentage points
CR_TOL = 0.01


ALL = cases.packer_cases()
HAD = [c["name"] for c in ALL if c["kind"] == "hadamard"]
DCT = [c["name"] for c in ALL if c["kind"] == "dct"]
EVERY = [c["name"] for c in ALL]


@pytest.mark.parametrize("name", HAD)
def test_hadamard_stream_bit_exact(api, orc, golden, packer_cases, name):
    c, g = packer_cases[name], golden["packers"][name]
    pk = api.new_hadamard(c["bps"], c["nch"], c["ns"])
    got = pk.compress(c["data"])
    want = orc.packer("hadamard", c["bps"], c["nch"], c["ns"]).compress(c["data"])
    assert got == want, describe_mismatch(got, want, 3 * c["nch"])
    assert len(got) == g["size"] and orc.fnv1a(got) == g["fnv1a"]
    pk.close()


@pytest.mark.parametrize("name", DCT)
def test_dct_stream(api, orc, golden, packer_cases, name):
    c, g = packer_cases[name], golden["packers"][name]
    pk = api.new_dct(c["bps"], c["nch"], c["ns"])
    got = pk.compress(c["data"])
    po = orc.packer("dct", c["bps"], c["nch"], c["ns"])
    want = po.compress(c["data"])
    # formal gate: CR within 1 %, PRDN (decoded by the oracle) within 0.05 pp
    assert abs(len(got) / len(want) - 1) <= CR_TOL
    dec_g, used, _ = po.decompress(got)
    assert used == len(got)
    if g.get("prdn") is not None:
        assert abs(orc.prdn(c["data"], dec_g, c["ns"], c["nch"], c["bps"]) - g["prdn"]) <= PRDN_TOL
    # and, because the arithmetic is restated exactly, the stream itself
    assert got == want, describe_mismatch(got, want, 3 * c["nch"])
    assert orc.fnv1a(got) == g["fnv1a"]
    pk.close()


@pytest.mark.parametrize("name", EVERY)
def test_decompress_matches_reference_output(api, orc, golden, packer_cases, name):
    """GPU decompress of the reference's stream == the reference's own decode."""
    c, g = packer_cases[name], golden["packers"][name]
    po = orc.packer(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
    stream = po.compress(c["data"])
    assert orc.fnv1a(stream) == g["fnv1a"]
    pk = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
    if c["kind"] == "xdelta_hzr":
        pk.set_nb(g["final_nb"])  # nb is not in the stream (xdelta_hzr.cpp:39,66,77)
    dec, used = pk.decompress(stream + b"\xAA" * 37)  # trailing junk must not be consumed
    assert used == len(stream)
    assert zlib.crc32(dec) == g["decoded_crc32"], "decoded bytes differ from the reference's decode"
    if g["lossless"]:
        assert dec == c["data"].tobytes()
    pk.close()


def test_gpu_roundtrip_and_nb_follow_up(api, packer_cases):
    """compress then decompress on the same instance (escalated nb carried along)."""
    for name in ("esc_i32_big", "esc_i24_walk", "i8_nb4", "ragged_3x43691_xdelta", "ecg12x34199_xdelta_nb1", "tiny_3x1"):
        c = packer_cases[name]
        pk = api.new_xdelta_hzr(c["bps"], c["nch"], c["ns"], c["nb"])
        s = pk.compress(c["data"])
        dec, used = pk.decompress(s)
        assert used == len(s) and dec == c["data"].tobytes(), name
        pk.close()


def test_corrupt_stream_is_reported(api, orc, packer_cases):
    c = packer_cases["ecg12x8192_xdelta"]
    s = bytearray(orc.packer("xdelta_hzr", c["bps"], c["nch"], c["ns"], 3).compress(c["data"]))
    pk = api.new_xdelta_hzr(c["bps"], c["nch"], c["ns"], 3)
    bad = bytearray(s)
    bad[15] = 7  # first hzr block header starts at 9: [len-1:2][crc:4][mode:1] -> invalid encoding mode
    with pytest.raises(api.RsptHipError) as e:
        pk.decompress(bytes(bad))
    assert e.value.status == ERR_CORRUPT
    bad = bytearray(s)
    bad[5:9] = (123).to_bytes(4, "little")  # master header disagrees with the packer's N
    with pytest.raises(api.RsptHipError):
        pk.decompress(bytes(bad))
    dec, used = pk.decompress(bytes(s))  # the handle still works afterwards
    assert dec == c["data"].tobytes()
    pk.close()


def test_bit_flips_never_take_the_decoder_down(api, orc, packer_cases):
    """48 single-bit flips all over a stream (framing, block headers, tree descriptions, code bits, CRC fields): with
    block verification on, every one is either reported (RSPT_HIP_ERR_CORRUPT) or decodes to the original bytes (a flip in
    pad bits); none may hang or fault, and the handle decodes the pristine stream afterwards."""
    c = packer_cases["ecg12x8192_xdelta"]
    s = orc.packer("xdelta_hzr", c["bps"], c["nch"], c["ns"], 3).compress(c["data"])
    pk = api.new_xdelta_hzr(c["bps"], c["nch"], c["ns"], 3)
    pk.set_verify(True)
    rng = np.random.default_rng(20260406)
    reported = 0
    for pos in rng.integers(0, 8 * len(s), 48):
        bad = bytearray(s)
        bad[pos >> 3] ^= 1 << (pos & 7)
        try:
            dec, used = pk.decompress(bytes(bad) + bytes(64))
            assert dec == c["data"].tobytes(), "a damaged stream decoded to other bytes without being reported (bit %d)" % pos
        except api.RsptHipError as e:
            assert e.status == ERR_CORRUPT, (pos, e.status)
            reported += 1
    assert reported >= 40  # (nearly every bit of a stream matters)
    dec, used = pk.decompress(s)
    assert used == len(s) and dec == c["data"].tobytes()
    pk.close()


@pytest.mark.parametrize("n", [65536, 3000])
def test_tree_description_flips_with_long_codes(api, orc, n):
    """Flips inside the tree description of a block with ~100 prefixes that lead to codes longer than the decoder's table index
    (second-level slots, overflow walks; n = 65536: the parallel tree recovery, 3000: the one-wave parse).  Without block
    verification a damaged tree may decode to other bytes -- what is required is that every call returns (an error or n
    bytes) and that the handle still decodes the pristine stream."""
    from fuzz_cases import gen

    data = gen(4242, n, "wide")
    pk = api.new_hzr(1, 1, n)
    s = pk.compress(data, dst_max_len=pk.max_compressed_size)
    p = parse_stream(s)
    mode, plen, crc, off = p["planes"][0]["blocks"][0]
    assert plen > 300  # (a Huffman block: tree description + codes)
    rng = np.random.default_rng(n)
    outcomes = [0, 0]
    for bit in rng.integers(0, min(8 * plen, 2900), 64):
        bad = bytearray(s)
        bad[off + 7 + (int(bit) >> 3)] ^= 1 << (int(bit) & 7)
        try:
            dec, used = pk.decompress(bytes(bad) + bytes(64))
            assert len(dec) == n
            outcomes[0] += 1
        except api.RsptHipError as e:
            assert e.status == ERR_CORRUPT, (bit, e.status)
            outcomes[1] += 1
    assert outcomes[1] > 0  # (a flipped branch / leaf bit shifts the whole description: most of them cannot be a tree)
    dec, used = pk.decompress(s)
    assert used == len(s) and dec == data.tobytes()
    pk.close()


@pytest.mark.parametrize("kind,B", [("xdelta_hzr", 64), ("hzr", 24)])
def test_full_size_batch_round_trip(api, kind, B):
    """The bench's decompress workload as a test: B blocks of 64ch x 65536 int32 through compress_batch and decompress_batch,
    three times over, compared on the device.  Every persistent decoder workgroup takes dozens of hzr blocks here -- a hand-over
    race between two of them (a missing LDS wait in front of a barrier) showed at this size only, and not in every launch."""
    import torch

    from rspt_amd import synth

    nch, ns = 64, 65536
    d_src = synth.synth_batch_native(B, nch, ns, device="cuda")
    pk = api.new_xdelta_hzr(4, nch, ns, 3) if kind == "xdelta_hzr" else api.new_hzr(4, nch, ns)
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.empty(B, dtype=torch.int64, device="cuda")
    pk.compress_batch(d_src, d_dst, d_sizes, stride)
    for rep in range(3):
        d_out = torch.zeros_like(d_src)
        d_used = torch.empty(B, dtype=torch.int64, device="cuda")
        pk.decompress_batch(d_dst, B, stride, d_out, d_used)
        torch.cuda.synchronize()
        assert torch.equal(d_used, d_sizes), "rep %d: consumed lengths (or error flags) differ" % rep
        bad = (d_out.view(B, -1) != d_src.view(B, -1)).any(dim=1).nonzero().flatten().tolist()
        assert not bad, "rep %d: streams %s decoded to other samples" % (rep, bad[:8])
    pk.close()


def test_a_damaged_stream_in_a_batch_leaves_its_neighbours_alone(api):
    """One stream of a batch with a bit flipped in the tree description of a dense block, another truncated to a few bytes: both
    are flagged in `consumed` (bit 63), every other stream of the same launch decodes to its samples."""
    import torch

    from rspt_amd import synth

    B, nch, ns = 12, 64, 65536
    d_src = synth.synth_batch_native(B, nch, ns, device="cuda")
    pk = api.new_xdelta_hzr(4, nch, ns, 3)
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.empty(B, dtype=torch.int64, device="cuda")
    pk.compress_batch(d_src, d_dst, d_sizes, stride)
    torch.cuda.synchronize()
    s3 = bytes(d_dst[3, : int(d_sizes[3])].cpu().numpy())
    blk = parse_stream(s3)["planes"][0]["blocks"][5]  # a dense plane-0 block: (mode, payload length, crc, offset)
    d_dst[3, blk[3] + 7 + 4] ^= 0x04  # inside its tree description
    d_dst[8, 40:] = 0  # stream 8: framing gone after 40 bytes
    d_out = torch.zeros_like(d_src)
    d_used = torch.empty(B, dtype=torch.int64, device="cuda")
    pk.decompress_batch(d_dst, B, stride, d_out, d_used)
    torch.cuda.synchronize()
    used = d_used.cpu().numpy().astype(np.uint64)
    flagged = [int(i) for i in range(B) if int(used[i]) >> 63]
    assert 8 in flagged and set(flagged) <= {3, 8}, flagged  # (a flipped description bit nearly always breaks the tree; if it does not, the CRC-less decode may pass)
    for i in range(B):
        if i in (3, 8):
            continue
        assert int(used[i]) == int(d_sizes[i])
        assert torch.equal(d_out[i], d_src[i]), i
    pk.close()


def test_batched_decompress(api, orc):
    import torch

    nch, ns, bps, B = 5, 3000, 4, 6
    blocks = [cases._rand_native(nch, ns, bps, 700 + i, 2000, walk=True) for i in range(B)]
    po = orc.packer("xdelta_hzr", bps, nch, ns, 3)
    streams = [po.compress(b) for b in blocks]
    stride = (max(len(s) for s in streams) + 255) // 256 * 256
    buf = np.zeros((B, stride), dtype=np.uint8)
    for i, s in enumerate(streams):
        buf[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    pk = api.new_xdelta_hzr(bps, nch, ns, 3)
    pk.set_nb(orc.packer_nb(po))
    d_out, d_used = pk.decompress_batch(torch.from_numpy(buf).cuda(), B, stride)
    torch.cuda.synchronize()
    for i in range(B):
        assert int(d_used[i]) == len(streams[i])
        assert d_out[i].cpu().numpy().tobytes() == blocks[i].tobytes()
    pk.close()


@pytest.mark.parametrize("kind", ["xdelta_hzr", "hzr"])
@pytest.mark.parametrize("nch,ns", [(4, 256), (12, 8192), (16, 1280), (20, 512), (64, 768), (68, 256), (132, 1024)])
def test_batched_decompress_int32_direct_path(api, orc, kind, nch, ns):
    """int32 samples, ns % 256 == 0, nch % 4 == 0: the last inverse pass writes the interleaved block itself
    (k_inv_native: <= 16 channels per workgroup, 64, 64 + a partial group, several groups)."""
    import torch

    bps, B = 4, 3
    blocks = [cases._rand_native(nch, ns, bps, 900 + 7 * i + nch, 30000 if i else 3, walk=bool(i & 1)) for i in range(B)]
    po = orc.packer(kind, bps, nch, ns, 3)
    streams = [po.compress(b) for b in blocks]
    stride = (max(len(s) for s in streams) + 255) // 256 * 256
    buf = np.zeros((B, stride), dtype=np.uint8)
    for i, s in enumerate(streams):
        buf[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    pk = api.SignalPacker(kind, bps, nch, ns, 3)
    if kind == "xdelta_hzr":
        pk.set_nb(orc.packer_nb(po))
    d_out, d_used = pk.decompress_batch(torch.from_numpy(buf).cuda(), B, stride)
    torch.cuda.synchronize()
    for i in range(B):
        assert int(d_used[i]) == len(streams[i])
        want = po.decompress(streams[i])[0]
        assert d_out[i].cpu().numpy().tobytes() == bytes(want), (kind, nch, ns, i)
    if kind == "xdelta_hzr":  # big-endian samples out of the same path (byte swap behind it)
        pk.set_byte_order(True)
        d_be, _ = pk.decompress_batch(torch.from_numpy(buf).cuda(), B, stride)
        torch.cuda.synchronize()
        assert d_be[B - 1].cpu().numpy().view(">i4").astype("<i4").tobytes() == d_out[B - 1].cpu().numpy().tobytes()
    pk.close()


def test_verify_checks_block_crcs(api, orc, packer_cases):
    """rspt_hip_set_verify: what hzr_verify does in the reference (hzr_decode.c:569-624)"""
    c = packer_cases["ecg12_i32"] if "ecg12_i32" in packer_cases else next(v for v in packer_cases.values() if v["kind"] == "xdelta_hzr" and v["nch"] * v["ns"] > 100000)
    po = orc.packer(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
    stream = bytearray(po.compress(c["data"]))
    pk = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
    pk.set_nb(orc.packer_nb(po))
    pk.set_verify(True)
    dec, used = pk.decompress(bytes(stream))  # a sound stream passes, every block size and alignment included
    assert used == len(stream) and dec == c["data"].tobytes()
    # flip one bit of a stored CRC (first hzr block of plane 0: stream[9..] = u16 len, u32 crc): decoding would not notice
    bad = bytearray(stream)
    bad[9 + 2] ^= 0x10
    pk.set_verify(False)
    dec2, used2 = pk.decompress(bytes(bad))
    assert dec2 == c["data"].tobytes()
    pk.set_verify(True)
    with pytest.raises(api.RsptHipError):
        pk.decompress(bytes(bad))
    pk.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 4096, 4097, 65535, 65536, 70001])
def test_verify_all_payload_lengths(api, orc, n):
    """payload lengths around every boundary of the CRC's shift decomposition (incompressible data: PlainCopy, L = n)"""
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    pk = api.new_hzr(1, 1, n)
    pk.set_verify(True)
    got = pk.compress(data, dst_max_len=pk.max_compressed_size)
    dec, used = pk.decompress(got)
    assert used == len(got) and dec == data.tobytes()
    pk.close()


def test_decompress_straight_from_a_container(api, orc):
    """pack_batch -> decompress_packed: the consumer side of the multi-GPU gather, no host hop for the payload"""
    import torch

    from rspt_amd import synth

    nch, ns, B = 12, 8192, 5
    d_src = synth.synth_batch_native(B, nch, ns, first_block=40, device="cuda")
    pk = api.new_xdelta_hzr(4, nch, ns, 2)
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.empty((B, stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.empty(B, dtype=torch.int64, device="cuda")
    pk.compress_batch(d_src, d_dst, d_sizes, stride)
    packed, total = pk.pack_batch(d_dst, d_sizes)
    torch.cuda.synchronize()
    other = api.new_xdelta_hzr(4, nch, ns, 1)  # another instance: every stream's nb comes from its index entry
    out, used = other.decompress_packed(packed[: int(total.item())])
    torch.cuda.synchronize()
    assert torch.equal(out, d_src) and torch.equal(used, d_sizes)
    assert other.nb == 1  # the handle's own state is neither used nor changed
    pk.close()
    other.close()


@pytest.mark.parametrize("name", [c["name"] for c in cases.hadamard_big_cases()])
def test_hadamard_beyond_65536_points(api, orc, golden, name):
    """ns = 2^k > 65536 (two passes over the planar row: k_fwht_seg + k_fwht_cross; 2^22 takes two cross passes): the stream and
    the decoded block are the real reference's (fixtures from oracle/_ref), for int32 / int24 / int16 samples"""
    import zlib

    c = {x["name"]: x for x in cases.hadamard_big_cases()}[name]
    g = golden["hadamard_big"][name]
    pk = api.new_hadamard(c["bps"], c["nch"], c["ns"])
    got = pk.compress(c["data"])
    assert len(got) == g["size"] and orc.fnv1a(got) == g["fnv1a"] and zlib.crc32(got) == g["crc32"]
    dec = pk.decompress(got)
    dec = dec[0] if isinstance(dec, tuple) else dec
    assert zlib.crc32(bytes(dec)) == g["decoded_crc32"]
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bps,nch,ns,amp", [(4, 8, 2048, 1 << 29), (3, 4, 2048, 1 << 21), (4, 1, 3000, 1 << 29), (4, 3, 257, (1 << 31) - 1)])
def test_dct_decode_where_the_truncation_overflows(api, orc, bps, nch, ns, amp):
    """dct blocks far outside the packer's range (coefficients overflow their two planes): the decoded doubles pass 2^31, where C's
    `(int)x` is undefined and the reference's build (x86-64 cvttsd2si) returns 0x80000000 for every unrepresentable value -- the
    GPU's own conversion saturates, one count off for the positive ones (signal_packer_dct.cpp:98; found by tools/soak.py).
    Streams and decoded blocks equal the oracle's."""
    for seed in range(3):
        x = cases._rand_native(nch, ns, bps, 9100 + seed, amp, walk=bool(seed & 1))
        po = orc.packer("dct", bps, nch, ns)
        pk = api.SignalPacker("dct", bps, nch, ns)
        want = po.compress(x)
        got = pk.compress(x)
        assert got == want
        ref, used_ref, _ = po.decompress(want)
        dec, used = pk.decompress(got)
        assert used == len(got) and dec == ref
        pk.close()


@pytest.mark.gpu
def test_streams_shorter_than_their_own_header_are_flagged(api):
    """decompress_batch over buffers whose stride is smaller than the dct packer's means header (1 + 3 nch bytes): every stream is
    flagged, nothing is read past a stream's end (the last one ends with the allocation)."""
    import torch

    nch, ns = 700, 16
    pk = api.SignalPacker("dct", 4, nch, ns)
    stride = 64  # < 1 + 3 * 700
    B = 4
    d = torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
    d_out, d_used = pk.decompress_batch(d, B, stride)
    torch.cuda.synchronize()
    assert all(int(u) < 0 for u in d_used.cpu().tolist())  # bit 63: malformed
    pk.close()


@pytest.mark.gpu
def test_bounded_decompress_and_fill_block_verification(api, orc):
    """rspt_hip_decompress_bounded: truncated streams and damaged length fields are RSPT_HIP_ERR_CORRUPT without a byte read behind
    the buffer (the reference's own decompress, and rspt_hip_decompress, trust the stream's length fields).  And with verification on
    a Fill block's CRC is checked like any other block's (hzr_decode.c:569-624): a flipped fill value is an error, not other bytes.
    Both found by the damaged-stream leg of tests/soak.py."""
    n = 70000
    data = np.zeros(n, dtype=np.uint8)
    data[:3000] = np.arange(3000) % 251  # plane 0: a Huffman block and a Fill block (zeros); planes 1..3: Fill blocks
    s = orc.packer("hzr", 1, 1, n).compress(data)
    pk = api.new_hzr(1, 1, n)
    for cut in (1, 4, 5, 9, 100, len(s) // 2, len(s) - 1):
        with pytest.raises(api.RsptHipError) as e:
            pk.decompress(s[:cut], bounded=True)
        assert e.value.status == ERR_CORRUPT, cut
    big = bytearray(s)
    big[1:5] = (0x7FFFFFF0).to_bytes(4, "little")  # plane 0 claims 2 GiB
    with pytest.raises(api.RsptHipError) as e:
        pk.decompress(bytes(big), bounded=True)
    assert e.value.status == ERR_CORRUPT
    dec, used = pk.decompress(s, bounded=True)
    assert used == len(s) and dec == data.tobytes()
    # a Fill block's value flipped: reported with verification on
    p = parse_stream(s)
    fills = [(k, blk) for k, pl in enumerate(p["planes"]) for blk in pl["blocks"] if blk[0] == 2 and k == 0]  # (plane 0: the samples of an int8 block)
    assert fills
    off = fills[-1][1][3]
    bad = bytearray(s)
    bad[off + 7] ^= 0x40
    pk.set_verify(True)
    with pytest.raises(api.RsptHipError) as e:
        pk.decompress(bytes(bad), bounded=True)
    assert e.value.status == ERR_CORRUPT
    pk.set_verify(False)
    dec, used = pk.decompress(bytes(bad), bounded=True)  # (without verification the damaged value is simply what comes out)
    assert used == len(s) and dec != data.tobytes()
    pk.close()
