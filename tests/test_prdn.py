"""The PRDN stage: the quality figure the reference's test_packer_ prints behind a round trip
(lib_rspt_test/rspt_test.cpp:98-111), on the GPU: rspt_hip_prdn_batch_dev.

CPU: the record's inputs, what the record covers, the numpy restatement (tests/prdn_cases.py) and the oracle's orc_prdn against
the reference's printed figure (tests/golden/prdn_record.json) by bit pattern, the stored PRDN of the lossy fixtures, the C ABI.
GPU (-m gpu): bit-exact against the record and the oracle, on both paths, on real round trips, large batches, big-endian
samples, and stream-ordered behind a decompress."""
import ctypes as C
import re

import numpy as np
import pytest

import cases
import devframe as df
import prdn_cases as pc
from devframe import ERR_ARG, api  # noqa: F401

LOSSY = [c["name"] for c in pc.lossy_fixtures()]
SYNTH = [c["name"] for c in pc.synthetic_cases()]


@pytest.fixture(scope="module")
def record():
    return {r["name"]: r for r in df.golden("prdn_record.json")["cases"]}


@pytest.fixture(scope="module")
def pcases(orc):
    """every case of the record with its two blocks: the synthetic ones, the generated full-size one, the lossy fixtures as the
    oracle decodes them"""
    out = {c["name"]: c for c in pc.synthetic_cases()}
    out[pc.REF_SEQ["name"]] = pc.ref_seq_case()
    for f in pc.lossy_fixtures():
        out[f["name"]] = pc.lossy_case(f, pc.oracle_decoded(orc, f))
    return out


ALL = SYNTH + [pc.REF_SEQ["name"]] + LOSSY


# ---- CPU ----

def test_record_inputs_have_not_drifted(record, pcases):
    assert sorted(record) == sorted(pcases)
    for name, c in pcases.items():
        r = record[name]
        assert (c["bps"], c["nch"], c["ns"]) == (r["bps"], r["nch"], r["ns"]), name
        assert pc.crc(c["orig"]) == r["orig_crc32"], name
        assert pc.crc(c["dec"]) == r["dec_crc32"], name  # (lossy: the oracle decodes what the reference decoded)


def test_the_record_covers_what_it_must(record, pcases):
    rs = list(record.values())
    finite = lambda r: (int(r["prdn"], 16) >> 52) & 0x7FF != 0x7FF  # noqa: E731
    assert {r["bps"] for r in rs} == {1, 2, 3, 4}
    assert any(r["nch"] == 1 and r["ns"] == 1 for r in rs)
    assert any(r["ns"] & (r["ns"] - 1) == 0 and r["ns"] > 1 for r in rs) and any(r["ns"] & (r["ns"] - 1) for r in rs)
    # a negative channel sum at an ns that is not a power of two: the mean is garbage, and ref wraps or the figure is a NaN
    neg = [r for r in rs if r["group"] == "negsum"]
    assert neg and any(int(r["prdn"], 16) == pc.NAN_BITS for r in neg)
    for r in neg:
        c = pcases[r["name"]]
        o = pc.native_to_i32(c["orig"], c["bps"], c["nch"], c["ns"]).astype(np.int64)
        assert r["ns"] & (r["ns"] - 1) and (o.sum(axis=0) < 0).all()
        assert (pc.average_32(o.astype(np.int32)) != o.sum(axis=0) // r["ns"]).all(), r["name"]
    zero, inf = "0" * 16, "7ff0000000000000"
    assert any(r["group"] == "zero_over_zero" and int(r["prdn"], 16) == pc.NAN_BITS and r["mse"] == zero and r["ref"] == zero for r in rs)
    assert any(r["group"] == "inf" and r["prdn"] == inf and r["ref"] == zero and r["mse"] != zero for r in rs)
    assert any(r["group"] == "same" and r["prdn"] == zero and r["orig_crc32"] == r["dec_crc32"] for r in rs)
    for r in rs:
        if r["group"] == "wrap":  # some difference o - d leaves int32
            c = pcases[r["name"]]
            o, d = (pc.native_to_i32(c[k], c["bps"], c["nch"], c["ns"]).astype(np.int64) for k in ("orig", "dec"))
            assert (np.abs(o - d) >= 1 << 31).any(), r["name"]
    assert sum(r["group"] == "wrap" for r in rs) >= 1
    seq_mse = [r for r in rs if r["group"] == "seq_mse"]
    assert len(seq_mse) >= 2 and all(r["path"] == 1 and finite(r) for r in seq_mse)
    for r in seq_mse:
        assert pc.prdn_parts(**{k: pcases[r["name"]][k] for k in ("orig", "dec", "bps", "nch", "ns")})[4]["need_m"]
    assert record[pc.REF_SEQ["name"]]["path"] == 1  # sum |r| > 2^53 (test_restatement... checks that it is ref that needs it)
    assert {r["name"] for r in rs if r["group"] == "lossy"} == set(LOSSY) and len(LOSSY) >= 10
    # no case outside the ones built for it takes the sequential path
    assert {r["name"] for r in rs if r["path"] == 1} <= {r["name"] for r in rs if r["group"] in ("seq_mse", "seq_ref", "wrap")}


@pytest.mark.parametrize("name", ALL)
def test_restatement_and_oracle_equal_the_reference_bit_for_bit(orc, record, pcases, name):
    c, r = pcases[name], record[name]
    p, mse, ref, path, info = pc.prdn_parts(c["orig"], c["dec"], c["bps"], c["nch"], c["ns"])
    print(name, "restatement", pc.hexbits(p), "oracle", pc.hexbits(orc.prdn(c["orig"], c["dec"], c["ns"], c["nch"], c["bps"])), "record", r["prdn"])
    assert pc.hexbits(p) == r["prdn"]
    assert pc.hexbits(orc.prdn(c["orig"], c["dec"], c["ns"], c["nch"], c["bps"])) == r["prdn"]
    assert (pc.hexbits(mse), pc.hexbits(ref), path) == (r["mse"], r["ref"], r["path"])
    if name == pc.REF_SEQ["name"]:
        assert info["need_r"] and not info["need_m"] and info["sa"] > 1 << 53
    if r["nch"] * r["ns"] < 1 << 22:
        assert not info["need_r"]  # |r| <= 2^31: the ref condition always holds below 2^22 samples


@pytest.mark.parametrize("name", LOSSY)
def test_stored_prdn_of_the_lossy_fixtures_is_reproduced(golden, record, pcases, name):
    c, g = pcases[name], golden["packers"][name]
    assert pc.crc(c["dec"]) == g["decoded_crc32"]
    p = pc.prdn(c["orig"], c["dec"], c["bps"], c["nch"], c["ns"])
    if g.get("prdn") is None:  # (golden.json stores a NaN as null)
        assert p != p and int(record[name]["prdn"], 16) == pc.NAN_BITS
    else:
        assert abs(p - g["prdn"]) < 1e-9


SEQ_WIDTH = [c["name"] for c in pc.SEQ_WIDTH_CASES]


@pytest.mark.parametrize("name", SEQ_WIDTH)
def test_the_narrow_sequential_cases_are_flagged(name):
    """by the restatement alone: sum t^2 > 2^53 (so the chain computes mse), a finite figure; the int24 companion is not flagged"""
    c = pc.seq_width_case(name)
    p, mse, ref, path, info = pc.prdn_parts(c["orig"], c["dec"], c["bps"], c["nch"], c["ns"])
    print(name, pc.hexbits(p), "s2 / 2^53 =", info["s2"] / pc.EXACT_LIMIT)
    assert path == 1 and info["need_m"] and not info["need_r"] and np.isfinite(p) and p > 0
    assert c["bps"] < 4 and {c["bps"] for c in pc.SEQ_WIDTH_CASES} == {2, 3}
    if c["bps"] == 3:
        assert c["ns"] % 1024 == 1 and pc.prdn_parts(*c["calm"], 3, c["nch"], c["ns"])[3] == 0


def test_finish_follows_ieee():
    assert pc.bits(pc.finish(0.0, 0.0)) == pc.NAN_BITS and pc.bits(pc.finish(4.0, -1.0)) == pc.NAN_BITS
    assert pc.finish(4.0, 0.0) == float("inf") and pc.bits(pc.finish(0.0, 5.0)) == 0
    assert pc.bits(pc.finish(0.0, -5.0)) == 1 << 63  # sqrt(-0.0) * 100.0 = -0.0
    assert pc.finish(1.0, 4.0) == 50.0


def test_header_declares_the_entry_and_the_library_exports_it():
    hdr, out = df.header(flat=False), df.exported()
    df.check_entries([re.compile(r"int\s+rspt_hip_prdn_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+void\s*\*\s*d_orig\s*,\s*const\s+void\s*\*\s*d_dec\s*,"
                                 r"\s*size_t\s+nblocks\s*,\s*double\s*\*\s*d_prdn\s*,\s*double\s*\*\s*d_mse\s*,\s*double\s*\*\s*d_ref\s*,\s*uint32_t\s*\*\s*d_path\s*,"
                                 r"\s*void\s*\*\s*stream\s*\)")], ["rspt_hip_prdn_batch_dev"])
    for word in ("0xFFF8000000000000", "UNSIGNED", "WRAP", "2^53"):
        assert word in hdr
    declared = set(re.findall(r"\b(rspt_hip_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    defined = set(re.findall(r"\bT (rspt_hip_[a-z_0-9]+)$", out, re.M))
    assert declared == defined


def test_a_null_handle_is_refused_without_a_device():
    from rspt_amd import api

    buf = (C.c_double * 4)()
    assert api.lib().rspt_hip_prdn_batch_dev(None, buf, buf, 1, buf, None, None, None, None) == ERR_ARG


# ---- GPU ----

def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _orc_bits(orc, o, d, nblocks, bps, nch, ns):
    o, d = (np.ascontiguousarray(x).reshape(nblocks, -1) for x in (o, d))
    return np.array([pc.bits(orc.prdn(o[b], d[b], ns, nch, bps)) for b in range(nblocks)], dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_gpu_equals_the_record(api, record, pcases, name):
    import torch

    c, r = pcases[name], record[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    p, mse, ref, path = pk.prdn_batch(_dev(c["orig"]), _dev(c["dec"]), parts=True)
    torch.cuda.synchronize()
    got = ("%016x" % _u64(p)[0], "%016x" % _u64(mse)[0], "%016x" % _u64(ref)[0], int(path[0]))
    print(name, got)
    assert got == (r["prdn"], r["mse"], r["ref"], r["path"])
    pk.close()


@pytest.mark.gpu
def test_gpu_unaligned_buffers_and_one_buffer_for_both(api, record, pcases):
    """every load width: the same blocks at 16-, 4- and 1-byte alignment; and d_dec == d_orig"""
    import torch

    for name in ("rand7x1001_i8", "rand5x1000_i16", "rand3x777_i24", "rand5x333_i32", "negsum5x99_i32", "big_error3x50000_i32"):
        c, r = pcases[name], record[name]
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        for shift in (0, 4, 1):
            o = torch.zeros(c["orig"].size + 16, dtype=torch.uint8, device="cuda")
            d = torch.zeros_like(o)
            o[shift : shift + c["orig"].size] = _dev(c["orig"])
            d[shift : shift + c["dec"].size] = _dev(c["dec"])
            p, mse, ref, path = pk.prdn_batch(o[shift : shift + c["orig"].size], d[shift : shift + c["dec"].size], parts=True)
            torch.cuda.synchronize()
            assert ("%016x" % _u64(p)[0], "%016x" % _u64(mse)[0], "%016x" % _u64(ref)[0], int(path[0])) == (r["prdn"], r["mse"], r["ref"], r["path"]), (name, shift)
        o = _dev(c["orig"])
        p = pk.prdn_batch(o, o)
        torch.cuda.synchronize()
        assert int(_u64(p)[0]) == pc.bits(pc.prdn(c["orig"], c["orig"], c["bps"], c["nch"], c["ns"])), name
        pk.close()


@pytest.mark.gpu
def test_gpu_mixed_batch_takes_each_path_where_it_must(api, orc):
    """blocks of one shape in one call, some exact and some sequential: the flags are per block"""
    import torch

    nch, ns, nb = 2, 65536, 6
    o = np.stack([pc._i32(cases.hash_i32(nch * ns, 1800 + b, 40000)) for b in range(nb)])
    d = np.stack([pc._noisy(o[b], 4, nch, ns, 1850 + b, (1 << 28) if b % 2 else 50) for b in range(nb)])
    want = [pc.prdn_parts(o[b], d[b], 4, nch, ns) for b in range(nb)]
    assert [w[3] for w in want] == [0, 1, 0, 1, 0, 1]
    pk = api.new_hzr(4, nch, ns)
    p, mse, ref, path = pk.prdn_batch(_dev(o), _dev(d), parts=True)
    torch.cuda.synchronize()
    assert path.cpu().tolist() == [w[3] for w in want]
    for k, t in enumerate((p, mse, ref)):
        assert _u64(t).tolist() == [pc.bits(w[k]) for w in want], k
    assert _u64(p).tolist() == _orc_bits(orc, o, d, nb, 4, nch, ns).tolist()
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEQ_WIDTH)
def test_gpu_sequential_chain_at_every_width(api, orc, name):
    """k_q_seq at 2 and 3 bytes per sample (the record's sequential cases are all int32): as it is, big-endian, int24 also one byte
    off a 16-byte boundary (the chain's byte-wise fetch) and as the outer blocks of a batch around an unflagged block"""
    import torch

    c = pc.seq_width_case(name)
    bps, nch, ns, orig, dec = (c[k] for k in ("bps", "nch", "ns", "orig", "dec"))

    def want_of(o, d):
        w = pc.prdn_parts(o, d, bps, nch, ns)
        assert pc.bits(w[0]) == pc.bits(orc.prdn(o, d, ns, nch, bps))
        return pc.bits(w[0]), pc.bits(w[1]), pc.bits(w[2]), w[3]

    def run(o, d):
        p, mse, ref, path = pk.prdn_batch(o, d, parts=True)
        torch.cuda.synchronize()
        return list(zip(_u64(p).tolist(), _u64(mse).tolist(), _u64(ref).tolist(), path.cpu().tolist()))

    def off_by_one(a):
        buf = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[1 : 1 + a.size] = _dev(a)
        return buf[1 : 1 + a.size]

    want = want_of(orig, dec)
    assert want[3] == 1
    pk = api.new_hzr(bps, nch, ns)
    assert run(_dev(orig), _dev(dec)) == [want]
    if bps == 3:
        assert run(off_by_one(orig), off_by_one(dec)) == [want], "one byte off"
        calm = want_of(*c["calm"])
        assert calm[3] == 0
        got = run(_dev(np.concatenate([orig, c["calm"][0], orig])), _dev(np.concatenate([dec, c["calm"][1], dec])))
        assert got == [want, calm, want], "the flag is per block"
    pk.set_byte_order(True)
    assert run(_dev(cases.reverse_samples(orig, bps)), _dev(cases.reverse_samples(dec, bps))) == [want], "big-endian"
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOSSY)
def test_gpu_round_trip_quality(api, orc, packer_cases, name):
    """GPU compress -> GPU decompress -> GPU PRDN == orc.prdn of the same two buffers; roundtrip_quality adds the CR"""
    import torch

    c = packer_cases[name]
    mk = api.new_dct if c["kind"] == "dct" else api.new_hadamard
    pk = mk(c["bps"], c["nch"], c["ns"])
    src = _dev(c["data"]).reshape(1, -1)
    d_dst, d_sizes = pk.compress_batch(src)
    d_out, d_used = pk.decompress_batch(d_dst, 1, d_dst.shape[1])
    p = pk.prdn_batch(src.reshape(-1), d_out.reshape(-1))
    torch.cuda.synchronize()
    want = pc.bits(orc.prdn(c["data"], d_out.cpu().numpy().reshape(-1), c["ns"], c["nch"], c["bps"]))
    print(name, "%016x" % _u64(p)[0], "%016x" % want)
    assert int(_u64(p)[0]) == want
    q, cr = pk.roundtrip_quality(src)
    torch.cuda.synchronize()
    assert int(_u64(q)[0]) == want
    assert float(cr[0]) == float(c["data"].size) / int(d_used[0]) and int(d_used[0]) == int(d_sizes[0])
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", pc.BIG_BATCHES, ids=[b["name"] for b in pc.BIG_BATCHES])
def test_gpu_large_batches_equal_the_oracle_per_block(api, orc, shape):
    import torch

    from rspt_amd import synth

    nb, bps, nch, ns = shape["nblocks"], shape["bps"], shape["nch"], shape["ns"]
    src = synth.synth_batch_native(nb, nch, ns, device="cuda")
    pk = api.new_hadamard(bps, nch, ns)
    d_dst, _ = pk.compress_batch(src)
    d_out, _ = pk.decompress_batch(d_dst, nb, d_dst.shape[1])
    p, mse, ref, path = pk.prdn_batch(src.reshape(-1), d_out.reshape(-1), parts=True)
    torch.cuda.synchronize()
    assert int(path.sum()) == 0
    want = _orc_bits(orc, src.cpu().numpy(), d_out.cpu().numpy(), nb, bps, nch, ns)
    assert np.array_equal(_u64(p), want)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bps", [2, 3, 4])
def test_gpu_big_endian_batch(api, orc, bps):
    """the handle's byte-order flag: big-endian blocks give what the oracle gives on the byte-swapped input"""
    import torch

    nch, ns, nb = 5, 1200, 9
    o = np.stack([cases._rand_native(nch, ns, bps, 1900 + b, 1 << (8 * bps - 3)) for b in range(nb)])
    d = np.stack([pc._noisy(o[b], bps, nch, ns, 1950 + b, 6) for b in range(nb)])
    rev = lambda x: np.stack([cases.reverse_samples(x[b], bps) for b in range(nb)])  # noqa: E731
    pk = api.new_hzr(bps, nch, ns)
    pk.set_byte_order(True)
    p = pk.prdn_batch(_dev(rev(o)), _dev(rev(d)))
    torch.cuda.synchronize()
    assert _u64(p).tolist() == _orc_bits(orc, o, d, nb, bps, nch, ns).tolist()
    pk.close()


@pytest.mark.gpu
def test_gpu_stream_order_and_determinism(api, orc):
    """queued behind decompress_batch on one stream without a synchronisation; launched twice; launched after a call with another
    nblocks on the same handle: identical bytes each time"""
    import torch

    from rspt_amd import synth

    nb, nch, ns = 24, 12, 8192
    src = synth.synth_batch_native(nb, nch, ns, device="cuda")
    pk = api.new_dct(4, nch, ns)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_dst, _ = pk.compress_batch(src)
        d_out, _ = pk.decompress_batch(d_dst, nb, d_dst.shape[1])
        queued = pk.prdn_batch(src.reshape(-1), d_out.reshape(-1), parts=True)  # no synchronisation since the decompress
    s.synchronize()
    torch.cuda.synchronize()
    after = pk.prdn_batch(src.reshape(-1), d_out.reshape(-1), parts=True)
    torch.cuda.synchronize()
    small = pk.prdn_batch(src[:5].reshape(-1), src[:5].reshape(-1), parts=True)  # another nblocks, other values in the scratch
    again = pk.prdn_batch(src.reshape(-1), d_out.reshape(-1), parts=True)
    torch.cuda.synchronize()
    assert _u64(small[0]).tolist() == [0] * 5
    for a, b, c in zip(queued, after, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert np.array_equal(_u64(queued[0]), _orc_bits(orc, src.cpu().numpy(), d_out.cpu().numpy(), nb, 4, nch, ns))
    pk.close()


@pytest.mark.gpu
def test_gpu_abi_refusals(api):
    import torch

    pk = api.new_hzr(4, 3, 100)
    L, h = api.lib(), pk._h
    o = torch.zeros(pk.block_bytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    call = lambda *a: L.rspt_hip_prdn_batch_dev(h, *a, None, None, None, None)  # noqa: E731
    assert call(o.data_ptr(), o.data_ptr(), 0, out.data_ptr()) == ERR_ARG
    assert call(None, o.data_ptr(), 1, out.data_ptr()) == ERR_ARG
    assert call(o.data_ptr(), None, 1, out.data_ptr()) == ERR_ARG
    assert call(o.data_ptr(), o.data_ptr(), 1, None) == ERR_ARG
    assert call(o.data_ptr(), o.data_ptr(), (1 << 31) // 3 + 1, out.data_ptr()) == ERR_ARG  # nblocks * nch >= 2^31
    assert call(o.data_ptr(), o.data_ptr(), 1, out.data_ptr()) == 0
    torch.cuda.synchronize()
    pk.close()
