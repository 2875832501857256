"""The hzr decoder (k_dec_block, rspt_amd/csrc/decode.hip) on valid streams that neither encoder here writes: tests/hzr_craft.py
writes them in plain Python, the compiled reference's verdict on each is in tests/golden/hzr_craft_record.json
(tests/golden/make_hzr_craft_record.py).

Families: A single-leaf trees; B comb trees with codes of up to 31 bits (45 with a run's extra bits); C wide trees -- more ten-bit
prefixes that continue than the second level has slots, the full 521-node tree, duplicate and unused leaves; D fixed-length codes,
whose chunks never fall into step; E other tokenisations under an ordinary Huffman tree; F payload lengths around the output
size and at 65535 / 65536, pad bits set, crafted blocks between ordinary ones; G what the reference decodes and the GPU refuses
by contract (include/rspt_hip.h: codes of 32 bits and more, a leaf symbol above 260); H what the reference refuses too.

CPU: the record has not drifted, carries the verdicts the families stand for, and the restatement (oracle/rspt_oracle.c) gives the
same verdicts and bytes; what the case list covers is asserted over the list, with the decoder's constants read from decode.hip.
GPU (-m gpu): one test per family over its cases, grouped by decoded size (a bytes handle has one size): the device batch with
verification off and on between two ordinary streams, hzr_verify_batch, the container form, the bounded host call, and an
ordinary stream on the same handle afterwards; selected cases inside the planes of a sample packer's stream."""
import functools

import numpy as np
import pytest

import devframe as df
import hzr_craft as hc
from cases import digest
from devframe import ERR_CORRUPT, api  # noqa: F401
from hzr_dev import BAD

K = hc.decoder_constants()


@functools.lru_cache(maxsize=None)
def _record():
    return {r["name"]: r for r in df.golden("hzr_craft_record.json")["cases"]}


def _verdict(lib, c):
    """as tests/golden/make_hzr_craft_record.py records it"""
    try:
        out = lib.hzr_decode(c["stream"], c["n"])
        out, ok = (out[0] if isinstance(out, tuple) else out), True
    except RuntimeError:
        out, ok = b"", False
    v, size = lib.hzr_verify(c["stream"])
    return {"decode": ok, "digest": digest(out) if ok else None, "verify": v, "size": size}


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_record_has_not_drifted():
    rec = df.golden("hzr_craft_record.json")["cases"]
    C = hc.craft_cases()
    assert len(C) == len(rec) == len(_record())
    for c, r in zip(C, rec):
        assert (c["name"], c["crc32"], len(c["stream"]), c["ref_safe"]) == (r["name"], r["crc32"], r["len"], r["reference"]), c["name"]


@pytest.mark.parametrize("family", hc.FAMILIES)
def test_reference_verdicts(family):
    """A-F and G: the reference decodes every stream to the case's bytes; H: it refuses.  Every CRC is right, so hzr_verify
    passes all of them."""
    for c in hc.by_family(family):
        r = _record()[c["name"]]
        assert c["expect"] == {"G": "gpu_refuses", "H": "reject"}.get(family, "ok"), c["name"]
        if not c["ref_safe"]:
            assert "decode" not in r and family == "H", c["name"]
            continue
        assert r["verify"] and r["size"] == c["n"], c["name"]
        if family == "H":
            assert not r["decode"], c["name"]
        else:
            assert r["decode"] and r["digest"] == digest(c["data"]), c["name"]


def test_restatement_matches_reference(orc):
    for c in hc.craft_cases():
        v = _verdict(orc, c)
        if c["ref_safe"]:
            r = _record()[c["name"]]
            assert v == {k: r[k] for k in v}, c["name"]
        else:  # (recover_tree in oracle/rspt_oracle.c bounds its node array: count + 2 > 2 * 261 - 1 fails)
            assert v == {"decode": False, "digest": None, "verify": True, "size": c["n"]}, c["name"]


def test_the_writer_refuses_what_the_reference_cannot_take():
    tree = hc.complete_of([(1, 2) if i < 6 else 3 for i in range(256)])
    with pytest.raises(AssertionError):
        hc.huff_payload(tree, hc.Tokens([1, 2, 3]))
    with pytest.raises(AssertionError):
        hc.block(b"")
    with pytest.raises(AssertionError):
        hc.block(bytes(65537))
    for c in hc.craft_cases():
        if "tree" in c:
            assert c["tree"]["leaves"] <= hc.MAX_LEAVES or not c["ref_safe"], c["name"]
            assert 1 <= c["L"] <= hc.BLOCK


def test_decoder_constants_are_those_the_cases_were_sized_for():
    assert set(K) == {"kSerialTreePayload", "kLutBits", "kSubBits", "kSubSlots", "kDecMinChunkBits", "kDecThreads"}
    assert hc.N_SMALL < 8 * K["kSerialTreePayload"] and K["kLutBits"] + K["kSubBits"] == 15  # (the comb depths sit around both tables)
    assert hc.chunking(1) == (1, 1) and hc.chunking(K["kDecMinChunkBits"] + 1) == (2, K["kDecMinChunkBits"] // 2 + 1)
    assert hc.chunking(8 * hc.BLOCK)[0] == K["kDecThreads"]


def test_single_leaf_cases_cover_leaves_bits_and_both_recoveries():
    A = hc.by_family("A")
    T = K["kSerialTreePayload"]
    assert all(c["tree"]["nodes"] == 1 for c in A)
    assert {c["leaf"] for c in A} == {0x41, 0, 256, 257, 258, 259, 260}
    for leaf in (0x41, 0, 256, 257, 258):
        assert {(c["L"], c["leaf_bit"]) for c in A if c["leaf"] == leaf} >= {(L, b) for L in (2, T - 1, T) for b in (0, 1, "random")}
    for leaf in (259, 260):  # one token is more than two bytes of payload there
        assert {c["leaf_bit"] for c in A if c["leaf"] == leaf and c["ntok"] == 1} == {0, 1, "random"}
    assert any(c["n"] == hc.BLOCK and not c["data"].any() and c["leaf"] == 260 for c in A)  # zeros as run tokens only


def test_comb_cases_cover_depths_sides_deepest_leaves_and_both_recoveries():
    B = hc.by_family("B")
    want = {(D, side, sym, small) for D in (10, 11, 15, 16, 30, 31) for side in "ab" for sym in ("lit", 256, 257, 258, 259, 260) for small in (False, True)}
    assert {(c["depth"], c["side"], c["deepest"] if c["deepest"] > 255 else "lit", c["L"] < K["kSerialTreePayload"]) for c in B} == want
    for c in B:
        assert c["tree"]["depth"] == c["depth"] == max(c["used_lengths"]) and c["tree"]["leaves"] == c["depth"] + 1, c["name"]
        assert c["longest_token"] == c["depth"] + hc.RUN_EXTRA.get(c["deepest"], 0)
    assert max(c["longest_token"] for c in B) == 45
    al = [c for c in B if c["align16"]]
    assert {(c["longest_token"], c["side"], c["L"] < K["kSerialTreePayload"]) for c in al} == {(t, s, m) for t in (31, 45) for s in "ab" for m in (False, True)}


def test_wide_cases_cover_slots_lengths_and_the_full_tree():
    C = {c["name"]: c for c in hc.by_family("C")}
    for c in C.values():
        assert c["tree"]["long_prefixes"] >= 40 > K["kSubSlots"], c["name"]
        # codes that end in the second level (11 .. 15 bits) and codes that walk on (16 and more) in one tree
        assert any(K["kLutBits"] < ln <= K["kLutBits"] + K["kSubBits"] for ln in c["tree"]["lengths"])
        assert any(ln > K["kLutBits"] + K["kSubBits"] for ln in c["tree"]["lengths"])
    for name in ("C_wide_dup_small", "C_wide_dup_big", "C_full_big"):
        # every leaf is in use (but the ten unused ones): symbols under every prefix, whichever of them got a slot
        c = C[name]
        assert set(c["used_lengths"]) == set(c["tree"]["lengths"]), name
    assert C["C_wide_dup_small"]["tree"]["dup"] >= 80 and C["C_wide_dup_small"]["unused_leaves"] == 10
    assert C["C_wide_dup_small"]["L"] < K["kSerialTreePayload"] <= C["C_wide_dup_big"]["L"]
    for name in ("C_full_16bytes", "C_full_big"):
        assert C[name]["tree"]["leaves"] == 261 and C[name]["tree"]["nodes"] == 521 and C[name]["tree"]["dup"] == 0
    assert C["C_full_16bytes"]["n"] == 16 and C["C_full_16bytes"]["L"] > 20 * 16 and min(C["C_full_16bytes"]["used_lengths"]) > K["kLutBits"]
    assert C["C_full_big"]["L"] >= K["kSerialTreePayload"]


def test_fixed_length_cases_follow_the_chunk_rule():
    """nchunk = clamp(ceil(nbits / kDecMinChunkBits), 1, kDecThreads), S = ceil(nbits / nchunk), restated here"""
    D = {c["name"]: c for c in hc.by_family("D")}
    assert set(D) == {"D_fixed%d_%s" % (w, k) for w in (4, 8) for k in ("never", "aligned")}
    for c in D.values():
        w = c["width"]
        assert c["tree"]["lengths"] == [w] and c["tree"]["leaves"] == 1 << w
        nbits = 8 * c["L"] - ((1 << w) - 1 + 10 * (1 << w))
        nchunk = min(max((nbits + K["kDecMinChunkBits"] - 1) // K["kDecMinChunkBits"], 1), K["kDecThreads"])
        S = (nbits + nchunk - 1) // nchunk
        assert (nchunk, S) == c["chunks"] and nbits == c["code_bits"]
        if c["sync"] == "aligned":
            assert S % w == 0
        else:  # S is odd: chunk t starts t * S bits into the codes, in every phase of the code in turn
            assert S % 2 == 1 and {t * S % w for t in range(nchunk)} == set(range(w))
    assert D["D_fixed4_never"]["chunks"][0] == K["kDecThreads"]  # as many rounds as the decoder has chunks


def test_tokenisation_cases_cover_the_freedoms():
    E = {c["name"]: c for c in hc.by_family("E")}
    for tag in ("65536", "5000"):
        d = E["E_lit0_%s" % tag]["data"]
        assert E["E_lit0_%s" % tag]["lit0_only"] and E["E_lit0_%s" % tag]["ntok"] == d.size
        p = E["E_pairs_%s" % tag]
        assert p["pairs_only"] and p["ntok"] == int((p["data"] != 0).sum()) + int((p["data"] == 0).sum()) // 2
        assert E["E_split_%s" % tag]["run_pairs"] > 20 and E["E_consecutive_%s" % tag]["run_pairs"] > 100
        b = E["E_begin_end_run_%s" % tag]
        assert b["first_is_run"] and b["last_is_run"] and b["data"][0] == 0 and b["data"][-1] == 0
    z = E["E_zeros65536_4runs"]
    assert z["ntok"] == 4 and z["n"] == 65536 and z["tree"]["leaves"] == 2 and not z["data"].any()
    assert all(c["tree"]["leaves"] >= 2 for c in E.values())


def test_edge_cases_cover_payload_lengths_pads_and_positions():
    F = hc.by_family("F")
    assert {(c["out_minus_L"], c["pad"]) for c in F if "out_minus_L" in c} == {(d, p) for d in (1, 0, -1) for p in (0, 1)}
    assert {(c["L"], c["pad"]) for c in F if c["L"] >= 65535} == {(L, p) for L in (65535, 65536) for p in (0, 1)}
    for c in F:
        if "tree" in c:
            assert c["pad_bits"] > 0  # (there are pad bits to set)
    assert {c["position"] for c in F if "position" in c} == {"first", "middle", "last"}
    assert all(c["n"] > 2 * hc.BLOCK for c in F if "position" in c)


def test_beyond_and_reject_cases():
    G, H = hc.by_family("G"), hc.by_family("H")
    assert {(c["depth"], c["L"] < K["kSerialTreePayload"]) for c in G if "depth" in c} == {(D, m) for D in (32, 33, 40) for m in (False, True)}
    assert {c["L"] < K["kSerialTreePayload"] for c in G if c.get("bad_leaf") == 300} == {False, True}
    assert all(c["expect"] == "gpu_refuses" for c in G) and all(c["expect"] == "reject" for c in H)
    names = {c["name"] for c in H}
    assert names == {"H_run_overruns_by_one_small", "H_run_overruns_by_one_big", "H_used_symbol300_small", "H_used_symbol300_big", "H_description_cut",
                     "H_262_leaves_small", "H_262_leaves_big"}
    assert [c["name"] for c in H if not c["ref_safe"]] == ["H_262_leaves_small", "H_262_leaves_big"]
    assert all(c["tree"]["leaves"] == 262 for c in H if not c["ref_safe"])


def test_splice_replaces_one_block_of_one_plane(orc):
    n = 70000
    native = np.random.RandomState(3).randint(0, 50, 4 * n).astype(np.uint8)
    po = orc.packer("hzr", 4, 1, n)
    s0 = po.compress(native)
    planes = native.reshape(n, 4).T
    blk = hc.block(planes[2, 65536:].tobytes(), hc.MODE_COPY)
    s1 = hc.splice(s0, 2, 1, blk)
    assert s1 != s0 and hc.splice(s0, 2, 1, hc.blocks_of(orc.hzr_encode(planes[2]))[1]) == s0
    dec, used, rc = po.decompress(s1)
    assert dec == native.tobytes() and used == len(s1)
    po.close()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def _upload(streams, stride):
    """the streams `stride` bytes apart in one device buffer; what lies behind a stream is not zero: reading it would show"""
    import torch

    flat = np.full(len(streams) * stride + 64, 0xA5, dtype=np.uint8)
    for i, s in enumerate(streams):
        flat[i * stride: i * stride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return torch.from_numpy(flat).cuda()


def _check_batch(where, items, out, used):
    """items: (name, stream, the bytes it decodes to or None where it must be flagged, the record's digest or None)"""
    for i, (name, s, want, dg) in enumerate(items):
        u = int(used[i])
        if want is None:
            assert u & BAD, "%s: %s was not flagged (consumed %d of %d)" % (where, name, u, len(s))
            continue
        assert u == len(s), "%s: %s consumed %#x of %d" % (where, name, u, len(s))
        got = out[i].tobytes()
        if got != want:
            first = int(np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))[0])
            raise AssertionError("%s: %s decodes to other bytes, first at %d of %d" % (where, name, first, len(want)))
        assert dg is None or digest(got) == dg, (where, name)


def _run_group(api, orc, n, group, odd_stride=False):
    """the cases of one decoded size through every decode entry of one bytes handle, between two ordinary streams"""
    import torch

    rec = _record()
    (d0, s0), (d1, s1) = hc.ordinary(n, 1), hc.ordinary(n, 2)
    items = [("ordinary neighbour in front", s0, d0.tobytes(), None)]
    items += [(c["name"], c["stream"], c["data"].tobytes() if c["expect"] == "ok" else None, rec[c["name"]].get("digest")) for c in group]
    items += [("ordinary neighbour behind", s1, d1.tobytes(), None)]
    streams = [it[1] for it in items]
    nb = len(streams)
    stride = (max(len(s) for s in streams) + 15) // 16 * 16 + 16 + (1 if odd_stride else 0)
    d_src = _upload(streams, stride)
    pk = api.new_bytes(n)
    for verify in (False, True):
        pk.set_verify(verify)
        d_out, d_used = pk.decompress_batch(d_src, nb, stride)
        torch.cuda.synchronize()
        _check_batch("batch, verify %s" % verify, items, d_out.cpu().numpy().reshape(nb, n), d_used.cpu().numpy().view(np.uint64))
    pk.set_verify(False)
    # hzr_verify on the device agrees with hzr_verify: every CRC here is right
    d_len = torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")
    dec = pk.hzr_verify_batch(d_src, d_len, src_stride=stride).cpu().numpy().view(np.uint64)
    for i, c in enumerate(group, 1):
        ok, size = (rec[c["name"]]["verify"], rec[c["name"]]["size"]) if c["ref_safe"] else orc.hzr_verify(c["stream"])
        assert ok and int(dec[i]) == size == n, (c["name"], int(dec[i]))
    assert int(dec[0]) == n and int(dec[-1]) == n
    if not odd_stride:
        # the container form: the same streams behind an index
        d_packed, d_total = pk.pack_batch(d_src[: nb * stride], d_len)
        d_out, d_used = pk.decompress_packed(d_packed, nbytes=int(d_total.item()))
        torch.cuda.synchronize()
        _check_batch("container", items, d_out.cpu().numpy().reshape(nb, n), d_used.cpu().numpy().view(np.uint64))
        # the host call with the stream's length as its bound
        for name, s, want, _ in items:
            if want is None:
                with pytest.raises(api.RsptHipError) as e:
                    pk.decompress(s, bounded=True)
                assert e.value.status == ERR_CORRUPT, name
            else:
                got, used = pk.decompress(s, bounded=True)
                assert used == len(s) and got == want, "host: %s" % name
    # the handle decodes an ordinary stream afterwards
    got, used = pk.decompress(s1, bounded=True)
    assert used == len(s1) and got == d1.tobytes()
    pk.close()


def _run_family(api, orc, cases):
    for n in sorted({c["n"] for c in cases}):
        _run_group(api, orc, n, [c for c in cases if c["n"] == n])


@pytest.mark.gpu
def test_gpu_single_leaf_trees(api, orc):
    """(the workgroup-wide recovery gave the single leaf only the even table entries: a stream whose bit per symbol is 1 and whose
    payload has 4096 bytes or more was flagged, A_*_L4096_b1 and _brand)"""
    _run_family(api, orc, hc.by_family("A"))


@pytest.mark.gpu
def test_gpu_comb_trees(api, orc):
    _run_family(api, orc, hc.by_family("B"))


@pytest.mark.gpu
def test_gpu_longest_tokens_at_every_payload_alignment(api, orc):
    """16 copies of a stream 1 (mod 16) bytes apart: the payload of the 31-bit and of the 45-bit token at every byte alignment"""
    import torch

    al = [c for c in hc.by_family("B") if c["align16"]]
    for n in sorted({c["n"] for c in al}):
        group = [c for c in al if c["n"] == n]
        streams = [c["stream"] for c in group for _ in range(16)]
        stride = (max(len(s) for s in streams) + 15) // 16 * 16 + 17
        assert len({(i * stride) % 16 for i in range(16)}) == 16
        pk = api.new_bytes(n)
        d_out, d_used = pk.decompress_batch(_upload(streams, stride), len(streams), stride)
        torch.cuda.synchronize()
        items = [("%s, copy %d" % (c["name"], q), c["stream"], c["data"].tobytes(), None) for c in group for q in range(16)]
        _check_batch("alignments", items, d_out.cpu().numpy().reshape(len(streams), n), d_used.cpu().numpy().view(np.uint64))
        pk.close()
        _run_group(api, orc, n, group, odd_stride=True)


@pytest.mark.gpu
def test_gpu_wide_trees(api, orc):
    """(the host calls refused C_full_16bytes as malformed: their staging buffer ended at rspt_hip_max_compressed_size, less than a
    valid stream whose Huffman payload is longer than its output; D_fixed8_* and F_Lp1_* met the same)"""
    _run_family(api, orc, hc.by_family("C"))


@pytest.mark.gpu
def test_gpu_fixed_length_codes(api, orc):
    """the chunk rounds reach their bound (one round per chunk: the first wrong chunk is right after every round) and end.  The
    wall time of the never-synchronising block is printed beside an encoder-made block of the same size, for the record: no
    threshold.  (Measured on an MI355X: 12.1 ms for the 65536-byte block of 4-bit codes in 1024 chunks, 0.092 ms for the
    encoder-made one.)"""
    import torch

    D = hc.by_family("D")
    _run_family(api, orc, D)
    c = next(c for c in D if c["name"] == "D_fixed4_never")
    n = c["n"]
    r = np.random.RandomState(8)
    p = np.array([8, 7, 6, 5, 4, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1], dtype=np.float64)
    plain = (16 * r.choice(16, n, p=p / p.sum()) + 5).astype(np.uint8)  # sixteen literals as well, but a code that falls into step
    s_plain = orc.hzr_encode(plain)
    assert hc.blocks_of(s_plain)[0][6] == hc.MODE_HUFF
    pk = api.new_bytes(n)
    for name, s, want in (("never-synchronising block", c["stream"], c["data"]), ("encoder-made block", s_plain, plain)):
        stride = (len(s) + 31) // 16 * 16
        d_src = _upload([s], stride)
        times = []
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_out, d_used = pk.decompress_batch(d_src, 1, stride)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        assert int(d_used.cpu()[0]) == len(s) and d_out.cpu().numpy().tobytes() == want.tobytes()
        print("%s: %d bytes, payload %d, %d chunks: decode call %.3f ms (best of three after a warm-up; all: %s)" %
              (name, n, len(s) - 11, c["chunks"][0], min(times[1:]), ", ".join("%.3f" % t for t in times)))
    pk.close()


@pytest.mark.gpu
def test_gpu_tokenisations(api, orc):
    _run_family(api, orc, hc.by_family("E"))


@pytest.mark.gpu
def test_gpu_payload_edges(api, orc):
    _run_family(api, orc, hc.by_family("F"))


@pytest.mark.gpu
def test_gpu_refuses_long_codes_and_leaf_symbols_above_260(api, orc):
    """flagged by both tree recoveries alike (bit 63), never decoded to other bytes; neighbours and handle intact"""
    _run_family(api, orc, hc.by_family("G"))


@pytest.mark.gpu
def test_gpu_flags_what_the_reference_rejects(api, orc):
    _run_family(api, orc, hc.by_family("H"))


SPLICED = ["A_lit_L%d_b1" % K["kSerialTreePayload"], "A_r257_L%d_brand" % (K["kSerialTreePayload"] - 1), "B_comb31b_r260_small", "B_comb16a_lit_big",
           "C_full_16bytes", "C_wide_dup_big", "D_fixed8_never", "E_consecutive_5000", "F_L65536_pad1", "G_comb32a_lit_small", "H_run_overruns_by_one_small"]


@pytest.mark.gpu
def test_gpu_crafted_blocks_inside_a_sample_packer_stream(api, orc):
    """the crafted block as plane 0 and as a higher plane of an hzr sample packer's stream (int32 samples: plane k is byte k of
    every sample), alone and in a batch beside the stream as the oracle wrote it"""
    import torch

    by_name = {c["name"]: c for c in hc.craft_cases()}
    for i, name in enumerate(SPLICED):
        c = by_name[name]
        n = c["n"]
        assert n <= hc.BLOCK
        for k in (0, 1 + i % 3):
            planes = np.stack([hc.ordinary(n, 10 + q)[0] for q in range(4)])
            planes[k] = c["data"]
            native = np.ascontiguousarray(planes.T).reshape(-1)
            po = orc.packer("hzr", 4, 1, n)
            s0 = po.compress(native)
            s1 = hc.splice(s0, k, 0, hc.blocks_of(c["stream"])[0])
            po.close()
            pk = api.new_hzr(4, 1, n)
            stride = (max(len(s0), len(s1)) + 255) // 256 * 256
            d_src = _upload([s0, s1, s0], stride)
            for verify in (False, True):
                pk.set_verify(verify)
                d_out, d_used = pk.decompress_batch(d_src, 3, stride)
                torch.cuda.synchronize()
                items = [("as written", s0, native.tobytes(), None), ("%s in plane %d" % (name, k), s1, native.tobytes() if c["expect"] == "ok" else None, None),
                         ("as written", s0, native.tobytes(), None)]
                _check_batch("packer stream, verify %s" % verify, items, d_out.cpu().numpy().reshape(3, 4 * n), d_used.cpu().numpy().view(np.uint64))
            pk.set_verify(False)
            if c["expect"] == "ok":
                got, used = pk.decompress(s1, bounded=True)
                assert used == len(s1) and got == native.tobytes(), (name, k)
            else:
                with pytest.raises(api.RsptHipError) as e:
                    pk.decompress(s1, bounded=True)
                assert e.value.status == ERR_CORRUPT
            got, used = pk.decompress(s0, bounded=True)
            assert used == len(s0) and got == native.tobytes()
            pk.close()
