"""Pin the restatement against the compiled reference itself (oracle/_ref) on many seeded random inputs.  The reference's
answers are recorded in tests/golden/ref_record.json (tests/golden/make_ref_record.py), so this runs wherever the repo does."""
import zlib

import numpy as np
import pytest

import cases
from cases import digest


@pytest.mark.parametrize("chunk", range(8))
def test_hzr_encode_matches_reference(orc, ref_record, chunk):
    for seed in range(chunk * 40, chunk * 40 + 40):
        d = cases.hzr_soup_block(seed)
        in_crc32, want = ref_record["hzr_encode"][seed]
        assert zlib.crc32(d.tobytes()) == in_crc32, "test input drifted (seed %d)" % seed
        so = orc.hzr_encode(d)
        assert digest(so) == want, "seed %d n %d" % (seed, d.size)
        assert orc.hzr_decode(so, d.size)[0] == d.tobytes()


def test_hzr_payload_boundary(orc, ref_record):
    """Blocks whose Huffman payload lands at / next to in_size (PlainCopy edge,
    hzr_encode.c:377-382,463-469)."""
    rec = ref_record["hzr_payload_boundary"]
    hits = set()
    for n in cases.PAYLOAD_BOUNDARY_SIZES:
        blocks = [cases.payload_boundary_block(n, seed) for seed in range(cases.PAYLOAD_BOUNDARY_SEEDS)]
        assert zlib.crc32(np.concatenate(blocks).tobytes()) == rec["in_crc32"][str(n)], "test input drifted (n %d)" % n
        for seed, d in enumerate(blocks):
            so = orc.hzr_encode(d)
            assert digest(so) == rec["streams"][str(n)][seed], "n %d seed %d" % (n, seed)
            hist, mode, plen = orc.hzr_block_stats(d)
            assert mode == so[10] and (plen == len(so) - 11)
            if abs(plen - n) <= 1 and mode != 2:
                hits.add((mode, int(plen) - n))
    assert (1, 0) in hits and (0, 0) in hits  # exactly-fits Huffman and copy both seen


@pytest.mark.parametrize("seed", range(cases.RANDOM_PACKER_SEEDS))
def test_packers_match_reference(orc, ref_record, seed):
    c = cases.random_packer_case(seed)
    kind, bps, nch, ns, nb, amp = c["kind"], c["bps"], c["nch"], c["ns"], c["nb"], c["amp"]
    rec = ref_record["packers"][seed]
    assert zlib.crc32(c["data"].tobytes()) == rec["in_crc32"], "test input drifted"
    po = orc.packer(kind, bps, nch, ns, nb)
    for stream_want, decoded_want, used_want in rec["calls"]:  # second call exercises the persisted nb
        so = po.compress(c["data"])
        assert digest(so) == stream_want, (kind, bps, nch, ns, nb, amp)
        do, uo, _ = po.decompress(so)
        assert digest(do) == decoded_want and uo == used_want == len(so)
    po.close()


def test_needed_nb_matches_reference_escalation(orc, ref_record):
    """criterion (SURVEY 8 note a-3) == the reference's round-trip escalation (the chunk count of its stream)."""
    rec = ref_record["needed_nb"]
    for seed in range(cases.NEEDED_NB_SEEDS):
        c = cases.needed_nb_case(seed)
        bps, nch, ns, nb0, amp = c["bps"], c["nch"], c["ns"], c["nb"], c["amp"]
        assert zlib.crc32(c["data"].tobytes()) == rec["in_crc32"][seed], "test input drifted (seed %d)" % seed
        v = orc.xdelta_forward(orc.native_to_i32(c["data"], ns, nch, bps))
        assert orc.xdelta_needed_nb(v, bps, nb0) == rec["nb"][seed], (bps, nch, ns, nb0, amp)
