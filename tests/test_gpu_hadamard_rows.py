"""Every hadamard row length 2^1 .. 2^16 on the device, against what the reference wrote and decoded at that length
(tests/golden/hadamard_rows_record.json; shapes, ladder and blocks in tests/hadamard_rows_cases.py) -- bit for bit, no tolerance:
(a) the quantiser: rspt_hip_set_quantizer + the plain batch entries, native and planar, per ladder entry (k_fwht_q, k_fwht64k_q);
(b) the ladder: one call with a mixed choice, compress and decompress, native and planar (k_fwht_l);
(c) compress to a PRDN target where the fused probes run (2^1 .. 2^13), the general and the fused route forced in turn, native and
    planar, with the targets placed ON the composed oracle's figures: exactly a figure, the double just below it, above every
    finite figure, below every figure.  The composed table is the numpy restatement's bit for bit (path and PRDN), the choice is
    target_cases.choose on it, the reported PRDN its figure, the streams the record's at the chosen quality;
(d) compress to a byte budget there, the general and the batched route forced in turn: the table of candidate sizes is the
    reference's, the budgets sit on those sizes (budget_cases.derive_budgets, scalar_budget), the choices are budget_cases.choose,
    the streams and the decoded blocks the record's at the chosen quality.
So the one- and two-stage tails of the transform loops, the 64- to 1024-thread launch shapes of the probes, their idle lanes and
their padded addressing all run, and a slip that the quantiser and the ladder kernel share at one row length cannot hide behind
a comparison of the device with the device."""
import numpy as np
import pytest

import budget_cases as bc
import devframe as df
import hadamard_rows_cases as hr
import lossy_dev as ld
import lossy_quantizer_cases as lq
import prdn_cases
import target_cases as tc
from devframe import api  # noqa: F401

pytestmark = pytest.mark.gpu

IDS = [hr.case_id(k) for k in hr.KS]
ROUTES = [(k, r) for k in hr.FUSED for r in (1, 2)]
TARGET_IDS = ["%s-%s" % (hr.case_id(k), {1: "general", 2: "fused"}[r]) for k, r in ROUTES]
BUDGET_IDS = ["%s-%s" % (hr.case_id(k), {1: "general", 2: "batched"}[r]) for k, r in ROUTES]


@pytest.fixture(scope="module")
def rec():
    return {e["k"]: e for e in df.golden("hadamard_rows_record.json")["cases"]}


@pytest.fixture(scope="module")
def runs(api):
    """per k, once: a handle at the case's nb, its four blocks on the device and the composed oracle of the ladder (with the PRDN
    figures where the probes run)"""
    import torch

    memo = {}

    def get(k):
        if k not in memo:
            kind, bps, nch, ns, nb = hr.shapes()[k]
            pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
            pk.set_quantizer(nb=nb)
            d_src = torch.from_numpy(hr.natives(k).copy()).cuda()
            memo[k] = (pk, d_src, ld.composed(pk, d_src, hr.LADDER, prdn=k in hr.FUSED))
        return memo[k]

    yield get
    for pk, _, _ in memo.values():
        pk.close()


def _first_difference(orc, k, q, b, stream):
    """what of a stream differs from the restatement: the first differing stored values, or that it does not parse"""
    kind, bps, nch, ns, nb = hr.shapes()[k]
    want, m32 = lq.restated_stored(hr.case_of(k, q), hr.natives(k)[b])
    try:
        vals, means, used = lq.stream_values(orc, stream, kind, nch, ns, nb)
    except Exception as ex:  # (a stream that is not one: say so instead of hiding the mismatch behind the parser's error)
        return "the stream does not parse: %r" % (ex,)
    bad = np.nonzero(vals.reshape(-1) != want)[0]
    return "%d of %d stored values differ, first at %s: got %s, restated %s; means %s, restated %s; %d of %d bytes parsed" % (
        bad.size, want.size, bad[:8].tolist(), vals.reshape(-1)[bad[:8]].tolist(), want[bad[:8]].tolist(), means.tolist(), tc.mean24(m32).tolist(),
        used, len(stream))


def _is_the_record(orc, k, e, b, w, stream, decoded, tag):
    """one block's stream and decoded bytes against the record's entry w of ladder entry e"""
    if not hr.same_stream(stream, w):
        raise AssertionError((tag, "stream", len(stream), w["size"], _first_difference(orc, k, hr.LADDER[e], b, stream)))
    assert lq.crc(decoded) == w["dec_crc32"], (tag, "decoded")
    if "decoded" in w:
        assert decoded == lq.unpack(w["decoded"]), (tag, "decoded")


@pytest.mark.parametrize("k", hr.KS, ids=IDS)
def test_the_quantiser_is_the_reference_at_every_row_length(rec, orc, runs, k):
    import torch

    pk, d_src, comp = runs(k)
    rows = hr.record_blocks(rec, k)
    own = pk.quantizer()
    d_planar = pk.to_planar_i32(d_src)
    for e, q in enumerate(hr.LADDER):
        o = comp[e]  # set_quantizer(q) + compress_batch + decompress_batch
        pk.set_quantizer(q)
        p_dst, p_sizes = pk.compress_planar_batch(d_planar)
        p_out, p_used = pk.decompress_planar_batch(p_dst, hr.NBLOCKS, p_dst.shape[1])
        p_nat = pk.from_planar_i32(p_out)
        torch.cuda.synchronize()
        p_dst, p_sizes, p_used, p_nat = p_dst.cpu().numpy(), p_sizes.cpu().numpy(), p_used.cpu().numpy(), p_nat.cpu().numpy()
        for b, w in enumerate(rows[e]):
            assert lq.crc(hr.natives(k)[b]) == w["in_crc32"]
            n = int(o["sizes"][b])
            _is_the_record(orc, k, e, b, w, o["dst"][b, :n].tobytes(), o["out"][b].tobytes(), (k, q, b, "native"))
            n = int(p_sizes[b])
            assert int(p_used[b]) == n, (k, q, b)
            _is_the_record(orc, k, e, b, w, p_dst[b, :n].tobytes(), p_nat[b].tobytes(), (k, q, b, "planar"))
    pk.set_quantizer(own[0])
    assert pk.quantizer() == own and ld.last_hip_error(pk) == 0


@pytest.mark.parametrize("k", hr.KS, ids=IDS)
def test_the_ladder_is_the_reference_at_every_row_length(rec, orc, runs, k):
    """five blocks -- the case's four and the first again -- with tests/test_gpu_ladder.py's choice: every entry, one of them twice"""
    import torch

    pk, d_src, _ = runs(k)
    rows = hr.record_blocks(rec, k)
    own = pk.quantizer()
    B = len(hr.CHOICE)
    d5 = torch.cat([d_src, d_src[: B - hr.NBLOCKS]])
    d_choice = torch.tensor(hr.CHOICE, dtype=torch.int32, device="cuda")
    d_dst, d_sizes = pk.compress_batch(d5, ladder=hr.LADDER, choice=d_choice)
    d_out, d_used = pk.decompress_batch(d_dst, B, d_dst.shape[1], ladder=hr.LADDER, choice=d_choice)
    p_dst, p_sizes = pk.compress_planar_batch(pk.to_planar_i32(d5), ladder=hr.LADDER, choice=d_choice)
    p_out, p_used = pk.decompress_planar_batch(p_dst, B, p_dst.shape[1], ladder=hr.LADDER, choice=d_choice)
    p_nat = pk.from_planar_i32(p_out)
    torch.cuda.synchronize()
    assert pk.quantizer() == own
    for form, dst, sizes, out, used in (("native", d_dst, d_sizes, d_out, d_used), ("planar", p_dst, p_sizes, p_nat, p_used)):
        dst, sizes, out, used = dst.cpu().numpy(), sizes.cpu().numpy(), out.cpu().numpy(), used.cpu().numpy()
        for i, e in enumerate(hr.CHOICE):
            b = i % hr.NBLOCKS
            n = int(sizes[i])
            assert 0 < n <= dst.shape[1] and int(used[i]) == n, (k, form, i, hex(n))
            _is_the_record(orc, k, e, b, rows[e][b], dst[i, :n].tobytes(), out[i].tobytes(), (k, form, i, e))
    assert ld.last_hip_error(pk) == 0


def _bits(figs):
    return [[(prdn_cases.bits(p), int(path)) for p, mse, path in row] for row in figs]


@pytest.mark.parametrize("k,route", ROUTES, ids=TARGET_IDS)
def test_a_prdn_target_on_the_figures_themselves(rec, orc, runs, k, route):
    pk, d_src, comp = runs(k)
    rows = hr.record_blocks(rec, k)
    figs = [[(float(o["prdn"][b]), float(o["mse"][b]), int(o["path"][b])) for b in range(hr.NBLOCKS)] for o in comp]
    restated = hr.restated_figures(k)
    assert _bits(figs) == _bits(restated), (k, "the composed table is not the restatement's", figs, restated)
    assert [[f[1] == 0.0 for f in row] for row in figs] == [[f[1] == 0.0 for f in row] for row in restated], k
    targets = hr.derive_targets(figs)
    d_planar = pk.to_planar_i32(d_src)
    pk.debug_set_target_route(route)
    try:
        for planar, src in ((False, d_src), (True, d_planar)):
            for t in targets:
                tag = (k, route, "planar" if planar else "native", float(t).hex())
                choice, prdn, sizes, dst = map(ld.rate_call(pk, "target", src, t, hr.LADDER, tag, planar=planar).get, ld.TARGET_FIELDS)
                for b in range(hr.NBLOCKS):
                    col = [row[b] for row in figs]
                    e, want = tc.choose(col, t)
                    assert int(choice[b]) == e, (tag, b, col, int(choice[b]))
                    assert prdn_cases.bits(prdn[b]) == prdn_cases.bits(want), (tag, b, prdn[b], want)
                    n = int(sizes[b])
                    assert n == rows[e][b]["size"], (tag, b, e, n)
                    if not hr.same_stream(dst[b, :n].tobytes(), rows[e][b]):
                        raise AssertionError((tag, b, e, "stream", _first_difference(orc, k, hr.LADDER[e], b, dst[b, :n].tobytes())))
    finally:
        pk.debug_set_target_route(0)


@pytest.mark.parametrize("k,route", ROUTES, ids=BUDGET_IDS)
def test_a_byte_budget_on_the_reference_s_sizes(rec, orc, runs, k, route):
    """eight blocks -- the case's four twice -- so that derive_budgets places every kind of budget: exactly at each entry's size,
    below the smallest, one byte below an entry"""
    import torch

    pk, d_src, _ = runs(k)
    rows = hr.record_blocks(rec, k)
    table = np.tile(hr.record_table(rec, k), (1, 2))
    d8 = torch.cat([d_src, d_src])
    pk.debug_set_budget_route(route)
    try:
        for budget, name in ((bc.derive_budgets(table), "per block"), (bc.scalar_budget(table), "one limit")):
            tag = (k, route, name)
            limits, choice, sizes, dst, out, cand = map(ld.rate_call(pk, "budget", d8, budget, hr.LADDER, tag).get, ld.BUDGET_FIELDS)
            assert np.array_equal(cand, table), (tag, "the table of candidate sizes", cand.tolist(), table.tolist())
            for i in range(2 * hr.NBLOCKS):
                b = i % hr.NBLOCKS
                e = bc.choose(table[:, i], limits[i])
                assert int(choice[i]) == e, (tag, i, table[:, i].tolist(), limits[i], int(choice[i]))
                n = int(sizes[i])
                assert n == int(table[e, i]), (tag, i, e)
                _is_the_record(orc, k, e, b, rows[e][b], dst[i, :n].tobytes(), out[i].tobytes(), (tag, i, e))
    finally:
        pk.debug_set_budget_route(0)
