"""Every hadamard row length of the single-workgroup kernels, one case per k = log2(ns), k = 1 .. 16: the shapes, the ladder, the
inputs and the launch shape of the fused probes.

k_fwht_q, k_fwht_l (k_fwht_body.hpp) and tp_fwht (target.hip) take a row's transform three stages at a time and "the one or two
stages left" singly, so how the loop ends depends on k mod 3; around it the fused probes (k_target_probe, k_planar_target_probe,
k_budget_probe) launch nt = max(64, min(1024, ns / 8)) threads, so 1, 2, 4, 8 or 16 waves leave partial sums, lanes idle below
512 points, and the padded addressing first moves a word at 64.  The cases put every k on the device with the quantiser, the
ladder, the PRDN target and the byte budget, and tests/golden/hadamard_rows_record.json (make_hadamard_rows_record.py) holds what
the reference writes and decodes for every case, ladder entry and block.

A case is (kind, bps, nch, ns, nb), the shape of tests/budget_cases.py, and its blocks are budget_cases.batch_native(shape, 4):
random, walk, constant, full scale.  The ladder is tests/test_gpu_ladder.py's.  nb and bps are dealt round by round inside each
residue class of k mod 3 (iir_sweep_cases._Draw.cyc), so that every class meets every plane count and every sample width; the
order of the deal is chosen so that a case of nb < 4 has an entry whose values leave nb bytes (tests/test_hadamard_rows.py holds
the list to this and to the other conditions it exists for)."""
import functools

import numpy as np

import budget_cases as bc
import lossy_quantizer_cases as lq
import prdn_cases
import target_cases as tc
from iir_sweep_cases import _Draw
from test_gpu_ladder import CHOICE, HAD_LADDER  # noqa: F401

LADDER = list(HAD_LADDER)
KS = list(range(1, 17))
NBLOCKS = 4
FUSED_MAX_K = 13  # kTpMaxNs = 8192 of target.hip: the longest row of the fused probes
FUSED = [k for k in KS if k <= FUSED_MAX_K]
TP_PER = 8        # kTpPer of target.hip: samples a thread of a probe holds
NCH1_K = 2        # the one case of a single channel
# what the i-th case of residue class k mod 3 takes (the first case of class 1 is k = 1, of class 2 k = 2, of class 0 k = 3)
# -- the fifth and sixth take the first and second again.  Three planes stand where k <= 10 and int8 samples beside four planes:
# the largest stored value falls with the row length (about 2^31 q / n at full scale), and a row of 2^11 points and more no
# longer leaves three bytes, int8 samples from 2^8 points on not one
NB_DEAL = {1: [1, 2, 3, 4], 2: [2, 3, 1, 4], 0: [1, 3, 2, 4]}
BPS_DEAL = {1: [2, 4, 3, 1], 2: [3, 4, 2, 1], 0: [2, 4, 3, 1]}
# the workgroup size of the fused probes at each k where they run, written out: tests/test_hadamard_rows.py holds probe_threads()
# to it, and the five sizes to being there
PROBE_THREADS = {1: 64, 2: 64, 3: 64, 4: 64, 5: 64, 6: 64, 7: 64, 8: 64, 9: 64, 10: 128, 11: 256, 12: 512, 13: 1024}


def probe_threads(ns):
    """nt of host_rate.hip (probe_launch): std::max(64u, std::min(1024u, g.ns / kTpPer))"""
    return max(64, min(1024, ns // TP_PER))


@functools.lru_cache(maxsize=None)
def shapes():
    """{k: (kind, bps, nch, ns, nb)}"""
    g = _Draw(0)
    out = {}
    for k in KS:
        r = k % 3
        nb, bps = g.cyc(("nb", r), NB_DEAL[r]), g.cyc(("bps", r), BPS_DEAL[r])
        out[k] = ("hadamard", bps, 1 if k == NCH1_K else 3 if k <= 10 else 2, 1 << k, nb)
    return out


def case_id(k):
    return "k%d_%s" % (k, bc.shape_id(shapes()[k]))


def case_of(k, q=None):
    """the case as tests/lossy_quantizer_cases.py and tests/target_cases.py spell one"""
    kind, bps, nch, ns, nb = shapes()[k]
    c = dict(name=case_id(k), kind=kind, bps=bps, nch=nch, ns=ns, nb=nb)
    return c if q is None else dict(c, q=float(q))


@functools.lru_cache(maxsize=None)
def natives(k):
    """uint8 [NBLOCKS][block bytes] of case k, read-only and computed once per process"""
    a = bc.batch_native(shapes()[k], NBLOCKS)
    a.setflags(write=False)
    return a


def record_blocks(rec, k):
    """the record's entry of case k as [ladder entry][block] -> {in_crc32, size, crc32, dec_crc32[, stream, decoded]}"""
    e = rec[k]
    assert [e[f] for f in ("kind", "bps", "nch", "ns", "nb")] == list(shapes()[k]), k
    assert [float.fromhex(x["q_hex"]) for x in e["entries"]] == LADDER, k
    return [x["blocks"] for x in e["entries"]]


def record_table(rec, k):
    """the reference's stream sizes of case k, int64 [nladder][nblocks]"""
    return np.array([[b["size"] for b in row] for row in record_blocks(rec, k)], dtype=np.int64)


def same_stream(got, w):
    """got (bytes) is the record's stream w: byte for byte where the record keeps it, else by length and CRC-32"""
    return got == lq.unpack(w["stream"]) if "stream" in w else (len(got) == w["size"] and lq.crc(got) == w["crc32"])


@functools.lru_cache(maxsize=None)
def restated_figures(k):
    """the PRDN restatement of case k (k <= FUSED_MAX_K): [ladder entry][block] -> (prdn, mse, path)"""
    c = case_of(k)
    return [[(lambda p: (p[0], p[1], p[3]))(prdn_cases.prdn_parts(n, tc.candidate(c, n, q), c["bps"], c["nch"], c["ns"])) for n in natives(k)]
            for q in LADDER]


# ---- targets placed on the figures themselves -----------------------------------------------------------------------------------

def finite_cells(figs):
    """figs: [ladder entry][block] -> (prdn, mse, path).  The cells a target can sit on: path 0 and a finite PRDN above zero"""
    return [(e, b) for e, row in enumerate(figs) for b, (p, mse, path) in enumerate(row) if path == 0 and 0.0 < p < float("inf")]


def derive_targets(figs):
    """one list of targets for a case, from its own table as budget_cases.derive_budgets places budgets on sizes: per ladder entry
    one cell's figure exactly (its <= holds with equality) and the double just below it (it no longer holds), the cells taken from
    the blocks in turn; one target above every finite figure and one below every figure"""
    cells = finite_cells(figs)
    assert cells
    blocks = sorted({b for e, b in cells})
    out = []
    for e in range(len(figs)):
        mine = [b for ee, b in cells if ee == e]
        if mine:
            want = blocks[e % len(blocks)]
            p = figs[e][want if want in mine else mine[0]][0]
            out += [p, float(np.nextafter(p, 0.0))]
    ps = [figs[e][b][0] for e, b in cells]
    out += [max(ps) * 2.0, float(np.nextafter(min(ps), 0.0))]
    assert all(0.0 < t < float("inf") for t in out)
    return out
