"""GPU parity for the adjustable quantiser of the lossy packers (rspt_hip_set_quantizer): streams and decoded samples against
the reference rebuilt with the same `quality` / nr_bytes_to_compress_ constants (tests/golden/lossy_quantizer_record.json,
inputs and settings in tests/lossy_quantizer_cases.py) -- bit for bit on the hadamard kernels of every size class and the dense
dct, inside the gates of tests/test_gpu_dct_fft.py on the dct's FFT kernels -- through every kind of entry point, and the
setter's own contract."""
import ctypes as C

import numpy as np
import pytest

import cases
import devframe as df
import lossy_quantizer_cases as lq
from devframe import ERR_ARG, api  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in lq.all_cases()}
EXACT = [c["name"] for c in lq.all_cases() if c["fft"] is None]
FFT = [c["name"] for c in lq.all_cases() if c["fft"] is not None]


@pytest.fixture(scope="module")
def rec():
    return {e["name"]: e for e in df.golden("lossy_quantizer_record.json")["cases"]}


def _new(api, c, flags=0):
    pk = api.SignalPacker(lq.KIND_ID[c["kind"]] | flags, c["bps"], c["nch"], c["ns"], lq.DEFAULTS[c["kind"]][1])
    pk.set_quantizer(c["q"], c["nb"])
    return pk


def _blocks(c, rec):
    """(inputs, record entries) of a case, at least two blocks to a call (the 2^22 row stays single)"""
    data = [lq.block_data(c, i) for i in range(c["nblocks"])]
    want = list(rec[c["name"]]["blocks"])
    for d, w in zip(data, want):
        assert lq.crc(d) == w["in_crc32"], c["name"]
    if len(data) == 1 and c["ns"] < 1 << 22:
        data, want = data * 2, want * 2
    return data, want


def _same_stream(got, w):
    return got == lq.unpack(w["stream"]) if "stream" in w else (len(got) == w["size"] and lq.crc(got) == w["crc32"])


def _compress_batch(pk, data, planar=False):
    import torch

    d_src = torch.from_numpy(np.stack(data)).cuda()
    d_dst, d_sizes = pk.compress_planar_batch(pk.to_planar_i32(d_src)) if planar else pk.compress_batch(d_src)
    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy()
    return [d_dst[i, : int(sizes[i])].cpu().numpy().tobytes() for i in range(len(data))], d_dst, d_sizes


def _decompress_batch(pk, d_dst, nblocks, planar=False):
    import torch

    if planar:
        d_out, d_used = pk.decompress_planar_batch(d_dst, nblocks, d_dst.shape[1])
        d_out = pk.from_planar_i32(d_out)
    else:
        d_out, d_used = pk.decompress_batch(d_dst, nblocks, d_dst.shape[1])
    torch.cuda.synchronize()
    return [d_out[i].cpu().numpy().tobytes() for i in range(nblocks)], d_used.cpu().numpy()


@pytest.mark.parametrize("name", EXACT)
def test_native_batch_is_the_rebuilt_reference(api, rec, name):
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    assert pk.quantizer() == (c["q"], c["nb"]) and pk.nb == c["nb"]
    got, d_dst, _ = _compress_batch(pk, data)
    for i, w in enumerate(want):
        assert _same_stream(got[i], w), (name, i, len(got[i]), w["size"])
    dec, used = _decompress_batch(pk, d_dst, len(data))
    for i, w in enumerate(want):
        assert int(used[i]) == w["size"] and lq.crc(dec[i]) == w["dec_crc32"], (name, i)
        if "decoded" in w:
            assert dec[i] == lq.unpack(w["decoded"])
    pk.close()


# one case per kernel family: k_fwht_q, k_fwht64k_q, k_fwht_seg + k_fwht_cross_q, k_dct
PLANAR = ["had_5x1024_q7p3_nb3", "had_i24_2x64_q2_nb3", "had_2x65536_q3_nb3", "wave2x131072_q3_nb3", "dct_2x257_q0p37_nb3", "dct_i8_3x100_q8_nb1"]


@pytest.mark.parametrize("name", PLANAR)
def test_planar_batch_is_the_rebuilt_reference(api, rec, name):
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    got, d_dst, _ = _compress_batch(pk, data, planar=True)
    for i, w in enumerate(want):
        assert _same_stream(got[i], w), (name, i)
    dec, used = _decompress_batch(pk, d_dst, len(data), planar=True)
    for i, w in enumerate(want):
        assert int(used[i]) == w["size"] and lq.crc(dec[i]) == w["dec_crc32"], (name, i)
    pk.close()


RESTATED = {c["name"]: c for c in lq.hadamard_restated_cases()}


@pytest.mark.parametrize("name", list(RESTATED))
def test_long_hadamard_cross_widths_are_the_restatement(api, orc, name):
    """k_fwht_cross_q with m = 16, 32 and 64 as the last pass (2^19, 2^20, 2^21 points): the stored values, the header and the
    decoded block against the numpy restatement of the quantiser, two blocks to a call"""
    c = RESTATED[name]
    data = lq.block_data(c, 0)
    want, m32 = lq.restated_stored(c, data)
    assert (want != 0).mean() > 0.001  # (the quantised transform is not all zero)
    pk = _new(api, c)
    got, d_dst, _ = _compress_batch(pk, [data, data])
    assert got[0] == got[1]
    vals, means, used = lq.stream_values(orc, got[0], "hadamard", c["nch"], c["ns"], c["nb"])
    assert used == len(got[0])
    assert (means == ((m32.astype(np.int64) << 8).astype(np.int32) >> 8)).all()
    bad = np.nonzero(vals.reshape(-1) != want)[0]
    assert bad.size == 0, (name, bad.size, bad[:8], vals.reshape(-1)[bad[:8]], want[bad[:8]])
    dec, used = _decompress_batch(pk, d_dst, 2)
    back = lq.restated_decode(c, vals, means).tobytes()
    assert dec[0] == back and dec[1] == back and [int(u) for u in used] == [len(got[0])] * 2
    pk.close()


HOST = ["had_3x8_q7p3_nb1", "had_2x64_full_scale_q0p1_nb4", "had_2x32768_q3_nb3", "had_2x65536_q7p3_nb4", "wave3x262144_i24_q7p3_nb3",
        "dct_3x100_q1000_nb1", "dct_3x257_full_scale_q0p37_nb4"]


@pytest.mark.parametrize("name", HOST)
def test_host_pointer_calls_are_the_rebuilt_reference(api, rec, name):
    """compress / decompress / decompress_bounded, and the C++ factories with rspt_cxx_set_quantizer"""
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    cx = api.CxxSignalPacker(c["kind"], c["bps"], c["nch"], c["ns"])
    cx.set_quantizer(c["q"], c["nb"])
    for d, w in zip(data[:1] if c["ns"] > 65536 else data, want):
        got = pk.compress(d, dst_max_len=pk.max_compressed_size)
        assert _same_stream(got, w), name
        for dec, used in (pk.decompress(got), pk.decompress(got, bounded=True)):
            assert used == w["size"] and lq.crc(dec) == w["dec_crc32"], name
        if c["ns"] <= 65536:
            assert cx.compress(d) == got
            dec, used, rc = cx.decompress(got)
            assert (used, rc) == (len(got), 0) and lq.crc(dec) == w["dec_crc32"]
    cx.close()
    pk.close()


@pytest.mark.parametrize("name", ["had_5x1024_q0p1_nb4", "had_2x65536_q0p1_nb1", "dct_2x257_q8_nb4", "dct_3x100_q100_nb4"])
def test_container_entries_carry_the_plane_count(api, rec, name):
    """pack_batch + decompress_packed: the index nibble is the quantiser's nb, and a handle at another nb decodes the container by
    it (the quality has to be the writer's)"""
    import torch

    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    _, d_dst, d_sizes = _compress_batch(pk, data)
    d_packed, d_total = pk.pack_batch(d_dst, d_sizes)
    torch.cuda.synchronize()
    total = int(d_total.item())
    idx = d_packed[32: 32 + 16 * len(data)].cpu().numpy().view(np.uint64).reshape(-1, 2)
    assert [int(lw >> np.uint64(56)) & 0xF for lw in idx[:, 1]] == [c["nb"]] * len(data)
    other = _new(api, dict(c, nb=1 + c["nb"] % 4))
    for p in (pk, other):
        d_out, d_used = p.decompress_packed(d_packed, nbytes=total)
        torch.cuda.synchronize()
        for i, w in enumerate(want):
            assert int(d_used[i]) == w["size"] and lq.crc(d_out[i].cpu().numpy()) == w["dec_crc32"], (name, i)
    d_out, d_used = pk.decompress_packed_planar(d_packed, nbytes=total)
    d_nat = pk.from_planar_i32(d_out)
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        assert lq.crc(d_nat[i].cpu().numpy()) == w["dec_crc32"], (name, i)
    other.close()
    pk.close()


@pytest.mark.parametrize("name", ["had_i16_5x1024_q7p3_nb3", "had_i24_2x64_q2_nb3", "dct_i16_2x257_q100_nb2", "dct_i24_1x8_q1_nb3", "had_3x8_q3_nb4"])
def test_big_endian_samples(api, rec, name):
    """set_byte_order: the streams are those of the byte-reversed block, and the decoded samples leave reversed"""
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    pk.set_byte_order(True)
    got, d_dst, _ = _compress_batch(pk, [cases.reverse_samples(d, c["bps"]) for d in data])
    for i, w in enumerate(want):
        assert _same_stream(got[i], w), (name, i)
    dec, _ = _decompress_batch(pk, d_dst, len(data))
    for i, w in enumerate(want):
        back = cases.reverse_samples(np.frombuffer(dec[i], dtype=np.uint8), c["bps"])
        assert lq.crc(back) == w["dec_crc32"], (name, i)
    pk.close()


@pytest.mark.parametrize("name", ["had_5x1024_q3_nb2", "dct_3x100_q8_nb3"])
def test_the_many_pipeline_and_the_feed_follow_the_setting(api, rec, name):
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c)
    stride = (pk.max_compressed_size + 63) // 64 * 64
    out = np.zeros((len(data), stride), dtype=np.uint8)
    lens = pk.compress_many(np.concatenate(data), out)
    for i, w in enumerate(want):
        assert _same_stream(out[i, : lens[i]].tobytes(), w), (name, i)
    back = np.zeros(len(data) * pk.block_bytes, dtype=np.uint8)
    used = pk.decompress_many(out, back, lengths=lens)
    for i, w in enumerate(want):
        assert used[i] == w["size"] and lq.crc(back[i * pk.block_bytes: (i + 1) * pk.block_bytes]) == w["dec_crc32"]
    # the feed: open, the setter is refused and nothing changes; the blocks come out under the setting the handle has
    dst = [np.zeros(stride, dtype=np.uint8) for _ in data]
    pk.feed_begin(1, 3)
    with pytest.raises(api.RsptHipError) as e:
        pk.set_quantizer(c["q"] * 2, c["nb"])
    assert e.value.status == ERR_ARG
    for d, o in zip(data, dst):
        assert pk.feed_push(np.ascontiguousarray(d), o)
    pk.feed_flush()
    done = {}
    while len(done) < len(data):
        r = pk.feed_poll()
        assert r is not None
        done[r[0]] = r
    pk.feed_end()
    assert pk.quantizer() == (c["q"], c["nb"])
    first = min(done)
    for i, w in enumerate(want):
        seq, n, st = done[first + i]
        assert st == 0 and _same_stream(dst[i][:n].tobytes(), w), (name, i)
    pk.close()


@pytest.mark.parametrize("name", ["dct_3x100_q100_nb4", "had_5x1024_q0p1_nb4"])
def test_raising_nb_behind_the_many_pipeline(api, rec, name, packer_cases):
    """A handle that has run compress_many / decompress_many at the reference's constants and is then given more planes: the
    pipeline's staging, made for the smaller streams by the first call, is made again -- a stride taken from the new
    max_compressed_size is accepted and the streams are the rebuilt reference's (they were refused / came back too small)."""
    c = CASES[name]
    data, want = _blocks(c, rec)
    q0, nb0 = lq.DEFAULTS[c["kind"]]
    assert c["nb"] > nb0
    pk = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], nb0)

    def both_ways(blocks):
        stride = (pk.max_compressed_size + 63) // 64 * 64
        out = np.zeros((len(blocks), stride), dtype=np.uint8)
        lens = pk.compress_many(np.concatenate(blocks), out)
        back = np.zeros(len(blocks) * pk.block_bytes, dtype=np.uint8)
        used = pk.decompress_many(out, back, lengths=lens)
        return out, lens, back, used, stride

    _, lens, _, used, small = both_ways(data)  # at the defaults: the staging now exists, for streams of nb0 planes
    assert (used == lens).all()
    pk.set_quantizer(c["q"], c["nb"])
    out, lens, back, used, stride = both_ways(data)
    assert stride > small
    for i, w in enumerate(want):
        assert _same_stream(out[i, : lens[i]].tobytes(), w), (name, i)
        assert used[i] == w["size"] and lq.crc(back[i * pk.block_bytes: (i + 1) * pk.block_bytes]) == w["dec_crc32"], (name, i)
    pk.set_quantizer(q0, nb0)  # and back down
    _, lens, _, used, again = both_ways(data)
    assert again == small and (used == lens).all()
    pk.close()


def test_the_cxx_instance_prints_nothing_for_a_plane_count_that_was_set(api, rec, capfd):
    """'Compression needs one more byte to encode.' belongs to the xdelta packer's escalation; the reference rebuilt with another
    nr_bytes_to_compress_ never prints it for a lossy packer"""
    c = CASES["had_2x64_qn_nb4"]
    data, want = _blocks(c, rec)
    cx = api.CxxSignalPacker(c["kind"], c["bps"], c["nch"], c["ns"])
    cx.set_quantizer(c["q"], c["nb"])
    capfd.readouterr()
    got = cx.compress(data[0])
    assert _same_stream(got, want[0])
    cx.close()
    assert "one more byte" not in capfd.readouterr().out


def test_another_handle_with_the_same_setting_decodes_and_the_defaults_come_back(api, rec, golden, packer_cases):
    for name, gname in (("had_2x64_q7p3_nb2", "had_negmean_2x64"), ("dct_3x100_q0p37_nb2", "dct_negmean_3x100")):
        c = CASES[name]
        data, want = _blocks(c, rec)
        g, gc = golden["packers"][gname], packer_cases[gname]
        assert (gc["kind"], gc["bps"], gc["nch"], gc["ns"]) == (c["kind"], c["bps"], c["nch"], c["ns"])
        q0, nb0 = lq.DEFAULTS[c["kind"]]
        writer = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], nb0)
        assert writer.quantizer() == (q0, nb0)  # a fresh handle has the reference's constants
        size0 = writer.max_compressed_size
        assert writer.compress(gc["data"]) == bytes.fromhex(g["stream"])
        writer.set_quantizer(nb=c["nb"])  # None keeps the other value
        assert writer.quantizer() == (q0, c["nb"])
        writer.set_quantizer(quality=c["q"])
        assert writer.quantizer() == (c["q"], c["nb"])
        got = writer.compress(data[0], dst_max_len=writer.max_compressed_size)
        assert _same_stream(got, want[0])
        reader = (api.new_hadamard if c["kind"] == "hadamard" else api.new_dct)(c["bps"], c["nch"], c["ns"], quality=c["q"], nb=c["nb"])
        dec, used = reader.decompress(got)
        assert used == len(got) and lq.crc(dec) == want[0]["dec_crc32"]
        # back to the defaults: today's streams and decodes, and today's size bound
        writer.set_quantizer(q0, nb0)
        assert writer.max_compressed_size == size0
        s = writer.compress(gc["data"])
        assert s == bytes.fromhex(g["stream"])
        dec, used = writer.decompress(s)
        assert used == len(s) and lq.crc(dec) == g["decoded_crc32"]
        # four planes fit the bound of a handle set to four
        writer.set_quantizer(nb=4)
        hzr_max = 4 + c["nch"] * c["ns"] + 7 * ((c["nch"] * c["ns"] + 65535) // 65536)
        assert writer.max_compressed_size == 1 + 3 * c["nch"] + 4 * (4 + hzr_max)
        reader.close()
        writer.close()


def test_refusals(api):
    L = api.lib()
    had, dct = api.new_hadamard(4, 2, 64), api.new_dct(4, 2, 100)
    for pk, (q0, nb0) in ((had, lq.DEFAULTS["hadamard"]), (dct, lq.DEFAULTS["dct"])):
        for q, nb in ((1.0, 0), (1.0, 5), (0.0, 2), (-1.0, 2), (float("nan"), 2), (float("inf"), 2), (-float("inf"), 2)):
            assert L.rspt_hip_set_quantizer(pk._h, q, nb) == -1, (q, nb)
        assert L.rspt_hip_set_nb(pk._h, 2) == -1  # stays refused for these kinds
        assert pk.quantizer() == (q0, nb0)  # nothing changed
    # a quality that leaves n / q or a dct scale not finite or zero
    assert L.rspt_hip_set_quantizer(had._h, 5e-324, 3) == -1  # 64 / q overflows
    assert L.rspt_hip_set_quantizer(dct._h, 5e-324, 2) == -1  # ratio1 / q overflows
    one = api.new_dct(4, 1, 1)
    assert L.rspt_hip_set_quantizer(one._h, 1.5e308, 2) == -1  # sqrt(2 / 1) * q overflows
    assert one.quantizer() == lq.DEFAULTS["dct"]
    one.close()
    assert had.quantizer() == lq.DEFAULTS["hadamard"] and dct.quantizer() == lq.DEFAULTS["dct"]
    for pk in (api.new_hzr(4, 2, 64), api.new_xdelta_hzr(4, 2, 64, 3), api.new_bytes(100)):
        q, nb = C.c_double(), C.c_uint()
        assert L.rspt_hip_set_quantizer(pk._h, 1.0, 3) == -1
        assert L.rspt_hip_get_quantizer(pk._h, C.byref(q), C.cast(C.byref(nb), C.c_void_p)) == -1
        pk.close()
    cx = api.CxxSignalPacker("xdelta_hzr", 4, 2, 64, 3)
    with pytest.raises(api.RsptHipError):
        cx.set_quantizer(1.0, 3)
    cx.close()
    q, nb = C.c_double(), C.c_uint()
    assert L.rspt_hip_get_quantizer(had._h, None, C.cast(C.byref(nb), C.c_void_p)) == -1
    assert L.rspt_hip_get_quantizer(had._h, C.byref(q), None) == -1
    had.close()
    dct.close()


@pytest.mark.parametrize("name", FFT)
def test_dct_fft_kernels_inside_their_gates(api, rec, orc, name):
    """The FFT kernels (forced at small ns, natural at 16384) against the rebuilt reference's stream: coefficients equal except
    truncation-boundary flips of 1 on a share <= 2e-3, CR within 1 %, PRDN within 0.05 points -- the gates of
    tests/test_gpu_dct_fft.py.  Batch entries, native and planar."""
    c = CASES[name]
    data, want = _blocks(c, rec)
    pk = _new(api, c, api.DCT_FORCE_FFT if c["fft"] == "forced" else 0)
    for planar in (False, True):
        got, d_dst, _ = _compress_batch(pk, data, planar=planar)
        dec, used = _decompress_batch(pk, d_dst, len(data), planar=planar)
        for i, w in enumerate(want):
            ref_stream = lq.unpack(w["stream"])
            a, ma, _ = lq.stream_values(orc, got[i], "dct", c["nch"], c["ns"], c["nb"])
            b, mb, _ = lq.stream_values(orc, ref_stream, "dct", c["nch"], c["ns"], c["nb"])
            d = np.abs(a.astype(np.int64) - b.astype(np.int64))
            share, dmax = float((d != 0).mean()), int(d.max())
            print(name, "planar" if planar else "native", i, "share", share, "max", dmax, "size", len(got[i]), w["size"])
            assert (ma == mb).all() and dmax <= lq.FFT_MAX_DIFF and share <= lq.FFT_MAX_SHARE, (share, dmax)
            assert abs(len(got[i]) / w["size"] - 1) <= lq.CR_TOL
            assert int(used[i]) == len(got[i])
            p = orc.prdn(data[i], dec[i], c["ns"], c["nch"], c["bps"])
            print(name, i, "prdn", p, w["prdn"])
            assert abs(p - w["prdn"]) <= lq.PRDN_TOL
    # the FFT inverse on the reference's own stream
    for d, w in zip(data, want):
        dec, used = pk.decompress(lq.unpack(w["stream"]))
        assert used == w["size"] and abs(orc.prdn(d, dec, c["ns"], c["nch"], c["bps"]) - w["prdn"]) <= lq.PRDN_TOL
    pk.close()


def test_roundtrip_quality_moves_with_the_setting(api):
    """what the setting is for: on an ECG-like batch a coarser dct quality and a coarser hadamard quality both shrink the stream
    and raise PRDN -- in opposite directions of the number"""
    import torch

    from rspt_amd import synth

    d = synth.synth_batch_native(2, 4, 4096, device="cuda")
    out = {}
    for kind, new, ladder in (("dct", api.new_dct, (512.0, 128.0, 32.0)), ("hadamard", api.new_hadamard, (0.25, 1.0, 4.0))):
        pk = new(4, 4, 4096)
        for q in ladder:  # coarse -> fine
            pk.set_quantizer(quality=q)
            prdn, cr = pk.roundtrip_quality(d)
            torch.cuda.synchronize()
            out[kind, q] = (float(prdn.mean()), float(cr.mean()))
        pk.close()
        p, r = zip(*[out[kind, q] for q in ladder])
        assert p[0] > p[1] > p[2] and r[0] > r[1] > r[2], (kind, out)
