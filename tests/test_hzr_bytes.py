"""The raw hzr byte-buffer codec (RSPT_HIP_KIND_BYTES) against libhzr: every stream byte-for-byte hzr_encode's, every decode
hzr_decode's, every verdict hzr_verify's.  The reference is the compiled one where oracle/_ref is there, else the oracle's
restatement (the two are pinned to each other on the CPU: tests/test_oracle_golden.py)."""
import struct
import zlib

import numpy as np
import pytest

import cases
from devframe import ERR_ARG, ERR_CORRUPT, ERR_DST_TOO_SMALL, api  # noqa: F401
from hzr_dev import BAD, Hzr, gpu_decode, gpu_encode
from streamtools import describe_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hzr(orc):
    return Hzr(orc)


# ---- contents -------------------------------------------------------------------------------------------------------------
_XD = {}


def _xdelta_plane(orc, k):
    """plane k of the xdelta transform of a synthetic 64 x 65536 int32 block (4 MiB)"""
    if not _XD:
        from rspt_amd import synth

        native = synth.synth_native(64, 65536, 0).numpy()
        v = orc.xdelta_forward(orc.native_to_i32(native, 65536, 64, 4))
        b = v.view(np.uint8).reshape(-1, 4)
        for kk in range(4):
            _XD[kk] = np.ascontiguousarray(b[:, kk])
    return _XD[k]


def _sparse(n, seed):
    """one non-zero byte every 1000 .. 20000 bytes: zero runs across the 16662 cap and across hzr block ends"""
    out = np.zeros(n, dtype=np.uint8)
    gaps = 1000 + cases.hash_bytes(2 * (n // 1000 + 2), seed).astype(np.int64).reshape(-1, 2).dot([256, 1]) % 19001
    pos = np.cumsum(gaps)
    pos = pos[pos < n]
    out[pos] = 1 + (pos % 255).astype(np.uint8)
    return out


CONTENTS = ["zero", "fill", "random", "sparse", "fib", "xd0", "xd2"]


def content(orc, kind, n, seed=0):
    if kind == "zero":
        return np.zeros(n, dtype=np.uint8)
    if kind == "fill":
        return np.full(n, 0x5A + seed % 7, dtype=np.uint8)
    if kind == "random":
        return cases.hash_bytes(n, 100 + seed)
    if kind == "sparse":
        return _sparse(n, 200 + seed)
    if kind == "fib":
        return np.resize(cases._fib_counts(22), n)
    return np.resize(np.roll(_xdelta_plane(orc, 0 if kind == "xd0" else 2), -4099 * seed), n)


def check_streams(hzr, got, bufs):
    for i, (g, b) in enumerate(zip(got, bufs)):
        want = hzr.encode(b)
        assert g is not None, "buffer %d flagged" % i
        assert g == want, "buffer %d of %d bytes: %s" % (i, b.size, describe_mismatch(g, want))


# ---- encode ---------------------------------------------------------------------------------------------------------------
KATS = ["zeros100", "A10", "abracadabra", "mixed40", "xorshift300", "zeros140k_one7"]


@pytest.mark.parametrize("name", KATS)
def test_kat_stream_is_hzr_encode(api, hzr, golden, name):
    data = cases.hzr_kat_inputs()[name]
    pk = api.new_bytes(data.size)
    assert pk.block_bytes == data.size and pk.max_compressed_size == api.hzr_max_compressed_size(data.size) and pk.nb == 1
    want = hzr.encode(data)
    got = pk.compress(data)  # rspt_hip_compress
    assert got == want, describe_mismatch(got, want)
    g = golden["hzr"][name]
    assert len(got) == g["size"] and hzr.orc.fnv1a(got) == g["fnv1a"]
    (dev,), _, _ = gpu_encode(pk, [data])  # rspt_hip_compress_batch_dev
    assert dev == want
    dec, used = pk.decompress(got)
    assert dec == data.tobytes() and used == len(got)
    with pytest.raises(api.RsptHipError) as e:  # HZR_FAIL of a short buffer
        pk.compress(data, dst_max_len=len(want) - 1)
    assert e.value.status == ERR_DST_TOO_SMALL
    with pytest.raises(api.RsptHipError) as e:
        pk.set_nb(2)
    assert e.value.status == ERR_ARG
    pk.close()


SIZES = [1, 2, 15, 16, 17, 4095, 65535, 65536, 65537, 131072 + 5, 2**20 + 3, 2**24]


@pytest.mark.parametrize("n", SIZES)
def test_every_content_at_every_size(api, hzr, orc, n):
    """one batch of all contents per size: mixed contents, and for the odd sizes buffers at several alignments modulo 16.
    Encode, decode of our streams and of the reference's, d_consumed."""
    bufs = [content(orc, k, n) for k in CONTENTS]
    pk = api.new_bytes(n)
    got, _, _ = gpu_encode(pk, bufs)
    check_streams(hzr, got, bufs)
    out, used = gpu_decode(pk, got, n)
    for i, b in enumerate(bufs):
        assert int(used[i]) == len(got[i]), (i, int(used[i]), len(got[i]))
        assert out[i].tobytes() == b.tobytes(), "buffer %d does not decode to its input" % i
    pk.close()


@pytest.mark.parametrize("nbuf", [1, 3, 64])
def test_batches_with_mixed_contents_at_every_alignment(api, hzr, orc, nbuf):
    n = 4099 if nbuf == 64 else 70001  # odd: buffer b starts at b * n, every residue modulo 16 among 64 buffers
    bufs = [content(orc, CONTENTS[(3 * i + 1) % len(CONTENTS)], n, seed=i) for i in range(nbuf)]
    if nbuf == 64:
        assert len({(i * n) % 16 for i in range(nbuf)}) == 16
    pk = api.new_bytes(n)
    got, _, _ = gpu_encode(pk, bufs)
    check_streams(hzr, got, bufs)
    again, _, _ = gpu_encode(pk, bufs)  # the same call once more: identical bytes
    assert again == got
    out, used = gpu_decode(pk, got, n)
    assert [int(u) for u in used] == [len(s) for s in got]
    assert out.tobytes() == np.concatenate(bufs).tobytes()
    # the reference's own streams decode too (same bytes here, but through the decoder alone: no handle state from encoding)
    pk2 = api.new_bytes(n)
    out2, used2 = gpu_decode(pk2, [hzr.encode(b) for b in bufs], n)
    assert out2.tobytes() == np.concatenate(bufs).tobytes() and [int(u) for u in used2] == [len(s) for s in got]
    pk.close()
    pk2.close()


def test_dst_stride_one_byte_short_flags_that_buffer_only(api, hzr, orc):
    n = 70001
    bufs = [content(orc, "sparse", n), content(orc, "random", n), content(orc, "xd0", n)]
    want = [hzr.encode(b) for b in bufs]
    assert len(want[1]) > max(len(want[0]), len(want[2]))  # PlainCopy is the longest
    stride = len(want[1]) - 1
    pk = api.new_bytes(n)
    got, raw, sizes = gpu_encode(pk, bufs, dst_stride=stride, fill=0xEE)
    assert got[0] == want[0] and got[2] == want[2]
    assert int(sizes[1]) == (len(want[1]) | BAD)
    assert (raw[1] == 0xEE).all(), "bytes were written for the stream that does not fit"
    got, _, _ = gpu_encode(pk, bufs)  # and the handle is sound afterwards
    assert got == want
    pk.close()


def test_dense_sparse_dense_on_one_handle(api, hzr, orc):
    """the clean-block invariant: what a call leaves in the planes never shows in the next call's streams"""
    n = 3 * 65536 + 777
    pk = api.new_bytes(n)
    rounds = [["random", "xd0", "fib", "fill", "random"], ["sparse", "zero", "sparse", "xd2", "zero"], ["xd0", "random", "random", "fib", "xd0"],
              ["zero", "sparse", "zero", "zero", "sparse"]]
    for r, kinds in enumerate(rounds):
        bufs = [content(orc, k, n, seed=10 * r + i) for i, k in enumerate(kinds)]
        got, _, _ = gpu_encode(pk, bufs)
        check_streams(hzr, got, bufs)
        if r == 1:  # a decode in between leaves the planes in an unknown state: the next call must not trust them
            out, _ = gpu_decode(pk, got, n)
            assert out.tobytes() == np.concatenate(bufs).tobytes()
    pk.close()


# ---- decode ---------------------------------------------------------------------------------------------------------------
def test_host_bounded_and_container_forms(api, hzr, orc):
    import torch

    n = 140000 + 13
    bufs = [content(orc, k, n, seed=3) for k in ("xd0", "sparse", "random", "fib", "zero")]
    want = [hzr.encode(b) for b in bufs]
    pk = api.new_bytes(n)
    for b, w in zip(bufs, want):
        for bounded in (False, True):
            dec, used = pk.decompress(w, bounded=bounded)
            assert dec == b.tobytes() and used == len(w)
        with pytest.raises(api.RsptHipError) as e:  # a bound inside the stream: nothing behind it is read
            pk.decompress(w[:-1], bounded=True)
        assert e.value.status == ERR_CORRUPT
    # rspt_hip_compress_many / rspt_hip_decompress_many
    src = np.concatenate(bufs)
    out = np.zeros((len(bufs), (pk.max_compressed_size + 15) // 16 * 16), dtype=np.uint8)
    lens = pk.compress_many(src, out)
    assert [out[i, : int(lens[i])].tobytes() for i in range(len(bufs))] == want
    back = np.zeros(src.size, dtype=np.uint8)
    used = pk.decompress_many(out, back, lengths=lens)
    assert back.tobytes() == src.tobytes() and [int(u) for u in used] == [len(w) for w in want]
    # container: pack_batch -> decompress_packed, index entries with nb = 1
    d_src = torch.from_numpy(src).cuda()
    d_dst, d_sizes = pk.compress_batch(d_src)
    d_packed, d_total = pk.pack_batch(d_dst, d_sizes)
    torch.cuda.synchronize()
    total = int(d_total.item())
    head = d_packed[: 32 + 16 * len(bufs)].cpu().numpy().view(np.uint64)
    assert int(head[1]) == len(bufs) and int(head[3]) & 0xFFFFFFFF == 1
    for i, w in enumerate(want):
        assert int(head[4 + 2 * i + 1]) == (len(w) | (1 << 56))
    d_out, d_used = pk.decompress_packed(d_packed, nbytes=total)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == src.tobytes()
    assert [int(u) for u in d_used.cpu().numpy().view(np.uint64)] == [len(w) for w in want]
    pk.close()


def test_other_decoded_size_is_flagged(api, hzr, orc):
    n = 70001
    buf = content(orc, "xd0", n)
    s = hzr.encode(buf)
    pk = api.new_bytes(n)
    streams = [s, struct.pack("<I", n + 1) + s[4:], struct.pack("<I", n - 1) + s[4:], s]
    out, used = gpu_decode(pk, streams, n)
    assert int(used[0]) == len(s) and int(used[3]) == len(s) and out[0].tobytes() == buf.tobytes() and out[3].tobytes() == buf.tobytes()
    assert int(used[1]) & BAD and int(used[2]) & BAD
    with pytest.raises(api.RsptHipError) as e:
        pk.decompress(streams[1])
    assert e.value.status == ERR_CORRUPT
    pk.close()


# ---- verify ---------------------------------------------------------------------------------------------------------------
VERIFY_SIZES = [300, 70001, 140000]
DAMAGE = ["none", "payload", "crc", "mode", "length", "cut", "fill"]


def _blocks(stream):
    """offsets of the block headers of a sound stream"""
    n = struct.unpack_from("<I", stream, 0)[0]
    pos, out = 4, []
    for _ in range((n + 65535) // 65536):
        out.append(pos)
        pos += 7 + struct.unpack_from("<H", stream, pos)[0] + 1
    return out


def damaged_stream(hzr, orc, seed):
    """-> (size index, original buffer, stream, damage).  Seeds 0, 4, 8, ... and the fill seeds of streams without a Fill
    block are left whole."""
    h = zlib.crc32(struct.pack("<I", seed))
    si = seed % len(VERIFY_SIZES)
    n = VERIFY_SIZES[si]
    kind = ["xd0", "sparse", "random", "fib", "fill", "xd2", "zero"][(seed // 3) % 7]
    buf = content(orc, kind, n, seed=seed)
    s = bytearray(hzr.encode(buf))
    dmg = "none" if seed % 4 == 0 else DAMAGE[1 + (seed // 4) % 6]
    blocks = _blocks(s)
    b0 = blocks[h % len(blocks)]
    L = struct.unpack_from("<H", s, b0)[0] + 1
    bit = 1 << ((h >> 8) % 8)
    if dmg == "payload":
        s[b0 + 7 + (h >> 11) % L] ^= bit
    elif dmg == "crc":
        s[b0 + 2 + (h >> 11) % 4] ^= bit
    elif dmg == "mode":
        s[b0 + 6] ^= 1 << ((h >> 8) % 2) if (h >> 10) % 4 else bit
    elif dmg == "length":
        s[(b0 + (h >> 11) % 2) if (h >> 13) % 3 else (h >> 11) % 4] ^= bit  # a block's length, or the master header's
    elif dmg == "cut":
        s = s[: (h >> 8) % len(s)]
    elif dmg == "fill":
        fills = [b for b in blocks if s[b + 6] == 2]
        if fills:
            s[fills[h % len(fills)] + 7] ^= bit
        else:
            dmg = "none"
    return si, buf, bytes(s), dmg


def test_verify_matches_hzr_verify_on_200_streams(api, hzr, orc):
    import torch

    items = [damaged_stream(hzr, orc, seed) for seed in range(200)]
    verdicts = [hzr.verify(s) for _, _, s, _ in items]
    n_ok = sum(1 for ok, _ in verdicts if ok)
    assert 200 - n_ok >= 80 and n_ok >= 40, (n_ok, "the seeds must give 80 rejected and 40 accepted streams by the reference alone")
    assert {d for _, _, _, d in items} == set(DAMAGE)
    stride = max(len(s) for _, _, s, _ in items) + 1
    host = np.full((200, stride), 0xA5, dtype=np.uint8)  # what lies behind a stream is not zero: reading it would show
    for i, (_, _, s, _) in enumerate(items):
        host[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_len = torch.tensor([len(s) for _, _, s, _ in items], dtype=torch.int64, device="cuda")
    pk = api.new_bytes(16)  # any bytes handle: verify takes streams of any decoded size
    d_dec = pk.hzr_verify_batch(torch.from_numpy(host).cuda(), d_len, src_stride=stride)
    torch.cuda.synchronize()
    dec = d_dec.cpu().numpy().view(np.uint64)
    for i, ((ok, size), (_, _, s, dmg)) in enumerate(zip(verdicts, items)):
        print("stream %3d %-7s len %6d  reference %s  device %s" % (i, dmg, len(s), "ok" if ok else "FAIL", "FAIL" if int(dec[i]) & BAD else "ok"))
        assert bool(int(dec[i]) & BAD) == (not ok), (i, dmg)
        if ok:
            assert int(dec[i]) == size, (i, dmg)
    other = api.new_hzr(1, 1, 16)
    with pytest.raises(api.RsptHipError) as e:  # bytes handles only
        other.hzr_verify_batch(torch.from_numpy(host).cuda(), d_len, src_stride=stride)
    assert e.value.status == ERR_ARG
    other.close()
    pk.close()


def test_damaged_streams_decode_flagged_or_right(api, hzr, orc):
    """Each of the 200 streams once through decode with verify on: flagged, or the right bytes -- the buffer the stream was
    made from, or, for damage libhzr itself cannot see (a mode byte turned from one valid mode into another keeps every CRC),
    what hzr_decode makes of that stream."""
    items = [damaged_stream(hzr, orc, seed) for seed in range(200)]
    for si, n in enumerate(VERIFY_SIZES):
        mine = [(i, it) for i, it in enumerate(items) if it[0] == si]
        pk = api.new_bytes(n)
        pk.set_verify(True)
        out, used = gpu_decode(pk, [it[2] if len(it[2]) else b"\0" for _, it in mine], n)
        for r, (i, (_, buf, s, dmg)) in enumerate(mine):
            if int(used[r]) & BAD:
                assert dmg != "none", "sound stream %d flagged" % i
                continue
            ok, size = hzr.verify(s)
            ref = hzr.decode(s, n) if ok and size == n else None
            assert out[r].tobytes() in (buf.tobytes(), ref), "stream %d (%s): neither flagged nor right" % (i, dmg)
            if dmg == "none":
                assert int(used[r]) == len(s)
        pk.close()


# ---- the other kinds are untouched ----------------------------------------------------------------------------------------
def test_other_kinds_unchanged_beside_a_bytes_handle(api, orc, golden, packer_cases):
    pkb = api.new_bytes(70001)
    buf = content(orc, "xd0", 70001)
    first = pkb.compress(buf)
    for name in ("readme_sine_hzr", "readme_sine_xdelta_nb3", "sine4096_i32_dct", "readme_sine_hadamard"):
        c, g = packer_cases[name], golden["packers"][name]
        pk = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
        got = pk.compress(c["data"])
        assert len(got) == g["size"] and orc.fnv1a(got) == g["fnv1a"], name
        assert pkb.compress(buf) == first
        pk.close()
    pkb.close()
