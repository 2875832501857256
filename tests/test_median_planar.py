"""The rolling-window median on the planar int32 matrix (rspt_hip_median_filter_planar_batch_dev / _stream_dev,
rspt_hip_median_planar_state_bytes; tests/median_planar_cases.py).

CPU: the planar expectation of every case of the median records, cut to the case's sample width, is the compiled reference's
record; what the planar case lists cover; the C ABI; no new kernel uses scratch.
GPU (-m gpu): the record cases, row ends, several spans per row, values, both regimes, stream calls with their state, more than
one piece of keys, the cross identities with the native entries and with compress_planar_batch, ordering, refusals, a foreign
stream, a seeded sweep.  Every buffer and state sits between guards."""
import ctypes as C
import re

import numpy as np
import pytest

import devframe as df
import median_cases as mc
import median_planar_cases as pc
import median_stream_cases as msc
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_median_filter_planar_batch_dev", "rspt_hip_median_planar_state_bytes", "rspt_hip_median_filter_planar_stream_dev")


# ---- CPU ----

def test_planar_expectation_cut_to_the_sample_width_is_the_median_record():
    rec = df.golden("median_record.json")["cases"]
    Cs = mc.median_cases()
    assert len(Cs) == len(rec) == 27
    for c, r in zip(Cs, rec):
        assert c["name"] == r["name"]
        P = pc.record_planar(c)
        assert P.shape == (1, c["nch"], c["ns"]) and P.dtype == np.int32
        assert mc.crc(pc.cut(P, c["bps"])) == r["in_crc32"], c["name"]  # (the layout helpers are inverse to each other)
        y = pc.cut(pc.record_expected(c["name"]), c["bps"])
        assert digest(y) == r["digest"] and mc.crc(y) == r["crc32"], c["name"]


def test_planar_stream_expectation_cut_to_the_sample_width_is_the_stream_record():
    recs = {r["name"]: r for r in df.golden("median_stream_record.json")["cases"]}
    Cs = msc.stream_cases()
    assert len(Cs) == len(recs) == 45
    for c in Cs:
        r = recs[c["name"]]
        P = pc.record_planar(c, c["nblocks"])
        assert mc.crc(pc.cut(P, c["bps"])) == r["in_crc32"], c["name"]
        want, image = pc.stream_expected(P, c["W"])
        y = pc.cut(want, c["bps"])
        assert digest(y) == r["digest"] and mc.crc(y) == r["crc32"], c["name"]
        assert image.size == pc.state_bytes(c["W"], c["nch"])
        if c["bps"] == 4:  # the native state's layout at bps = 4
            assert np.array_equal(image, msc.state_after(c["data"], 4, c["nch"], c["W"])), c["name"]


def test_row_cases_cover_every_length_offset_bucket_edge_and_mode():
    Cs = pc.row_cases()
    assert (pc.R, pc.CHUNK, pc.MIN_LANES) == (32, 8192, 8)
    R, CH = pc.R, pc.CHUNK
    assert set(pc.ROW_NS) == {1, 2, R - 1, R, R + 1, 2 * R + 1, CH - 1, CH, CH + 1, 2 * CH + 5, 40}
    rows = [c for c in Cs if c["name"].startswith("row_")]
    assert {c["ns"] for c in rows} == set(pc.ROW_NS) and {c["nch"] for c in rows} >= set(pc.NCH)
    assert {(c["src_off"], c["dst_off"]) for c in rows if c["dst_off"] is not None} == {(s, d) for s in pc.OFFSETS for d in pc.OFFSETS}
    assert {c["src_off"] for c in rows if c["dst_off"] is None} == set(pc.OFFSETS) == {0, 4, 8, 12}
    for ns in pc.ROW_NS:
        assert {c["dst_off"] is None for c in rows if c["ns"] == ns} == {True, False}
    assert pc.geom(256, 2, 64, pc.MANY_ROWS_NS, 5)["rows_per_workgroup"] == 32  # many rows per workgroup
    assert {pc.geom(256, 2, 3, ns, 5)["lanes"] for ns in pc.ROW_NS} >= {8, 256}
    assert set(pc.BUCKET_WS) == {2, 3, 4, 5, 8, 9, 16, 17, 31, 32}
    for W in pc.BUCKET_WS:  # every bucket edge in both modes, on the wide path (16-byte aligned rows) as on the dword path, one chunk and more
        sel = [c for c in Cs if c["W"] == W and c["ns"] >= W]
        wide = [c for c in sel if c["src_off"] == 0 and c["dst_off"] in (None, 0) and c["ns"] % 4 == 0]
        narrow = [c for c in sel if c not in wide]
        assert {c["dst_off"] is None for c in wide} == {True, False} and {c["dst_off"] is None for c in narrow} == {True, False}, W
    assert any(c["ns"] > CH and c["src_off"] == 0 and c["dst_off"] in (None, 0) and c["ns"] % 4 == 0 for c in Cs)
    for ns, side in ((20, "short"), (50, "generic")):  # W = ns - 1, ns and above ns
        sel = [c for c in Cs if c["name"].startswith("window_ns%d_" % ns)]
        assert {c["W"] - ns for c in sel} >= {-1, 0} and any(c["W"] > ns for c in sel)
        assert all((min(c["W"], ns) <= pc.SHORT_MAX) == (side == "short") for c in sel)
    for c in Cs:  # at least two blocks; every channel its own samples
        P = c["planar"]
        assert P.dtype == np.int32 and c["nblocks"] >= 2
        assert c["ns"] < 8 or all(not np.array_equal(P[0, 0], P[0, ch]) for ch in range(1, c["nch"]))


def test_span_cases_are_split_whatever_the_cu_count():
    for cu in (8, 256, 304):
        for W in pc.SPAN_WS:
            g = pc.geom(cu, 1, 2, 40000, W)
            assert g["nsplit"] > 1 and g["span"] >= 4 * (W - 1) and g["span"] % pc.CHUNK == 0
    assert set(pc.SPAN_WS) == {3, 32}
    assert {c["W"] for c in pc.span_cases()} == set(pc.SPAN_WS) and all(c["dst_off"] is None and (c["nblocks"], c["nch"], c["ns"]) == (1, 2, 40000)
                                                                       for c in pc.span_cases())


def test_value_and_width_cases_hold_what_they_claim():
    V = {c["name"]: c for c in pc.value_cases()}
    full, neg, tern = V["full_scale_w4"]["planar"], V["negative_odd_w2"]["planar"], V["ternary_w6"]["planar"]
    assert set(np.unique(full)) == {mc.INT32_MIN, mc.INT32_MAX} and (full[0, 0, :70] == mc.INT32_MIN).all() and (full[0, 1, :70] == mc.INT32_MAX).all()
    pairs = neg[:, :, :-1].astype(np.int64) + neg[:, :, 1:]
    assert (neg < 0).all() and ((pairs % 2) != 0).sum() > 100
    assert set(np.unique(tern)) == {-1, 0, 1}
    for tag in ("full_scale", "negative_odd", "ternary"):
        sel = [c for c in V.values() if c["name"].startswith(tag)]
        assert {c["W"] <= pc.SHORT_MAX for c in sel} == {True, False} and {bool(c["calls"]) for c in sel} == {True, False}
    Wd = pc.width_cases()
    assert {c["bps"] for c in Wd} == {1, 2, 3} and {bool(c["calls"]) for c in Wd} == {True, False}
    for c in Wd:
        P, bps = c["planar"], c["bps"]
        assert (P == 1 << (8 * bps)).any() and (P == pc.FULL).any() and (P == -pc.FULL - 1).any()
        want = pc.expected(c)[0]
        lim = 1 << (8 * bps - 1)
        assert ((want >= lim) | (want < -lim)).mean() > 0.5, c["name"]  # cutting the output would show


def test_regime_and_stream_cases_cover_what_they_claim():
    Rg = pc.regime_cases()
    assert {(c["ns"], c["W"]) for c in Rg} == {(ns, W) for ns in pc.REGIME_NS for W in pc.REGIME_WS} and set(pc.REGIME_WS) == {32, 33}
    assert set(pc.REGIME_NS) == {1023, 1024, 1025, 4095, 4096, 4097, 8193}
    assert {c["dst_off"] is None for c in Rg if c["W"] == 33} == {True, False}
    S = pc.stream_cases()
    main = [c for c in S if c["name"].startswith("stream_ns")]
    assert {c["ns"] for c in main} == set(pc.STREAM_NS) and {c["calls"] for c in main} == set(pc.STREAM_CUTS)
    for ns in pc.STREAM_NS:
        below, blocks_back, past_call = pc.stream_windows(ns)
        assert 1 < below - 1 < ns and 2 * ns < blocks_back - 1 < 3 * ns and past_call - 1 > 5 * ns
        sel = [c for c in main if c["ns"] == ns]
        assert {c["W"] for c in sel} == {below, blocks_back, past_call}
        for W in (below, blocks_back, past_call):
            assert {c["dst_off"] is None for c in sel if c["W"] == W} == {True, False}, (ns, W)
    assert all(len(c["calls"]) == 3 and sum(c["calls"]) == c["nblocks"] for c in main)  # the first call on a fresh state, two on a started one
    assert {c["nch"] for c in main} >= {1, 3, 64, 65}
    for short in (True, False):  # on both sides of 32: W - 1 below ns, several blocks back, and above the first call's rows
        sel = [c for c in main if (c["W"] <= pc.SHORT_MAX) == short]
        assert any(c["W"] - 1 < c["ns"] for c in sel) and any(c["W"] - 1 > 2 * c["ns"] for c in sel)
        assert any(c["W"] - 1 > c["calls"][0] * c["ns"] for c in sel), short
    g = pc.by_name()[pc.GENERIC_STREAM]
    assert (g["nch"], g["ns"], g["W"], g["calls"][0], g["dst_off"]) == (2, 30000, 101, 3, None)
    assert -(-(3 * 30000) // ((1 << 16) - 100)) == 2  # segments of the first call
    assert {c["dst_off"] is None for c in S if c["W"] == 1} == {True, False}
    sp = pc.by_name()[pc.SPLIT_STREAM]  # a carried short call on split rows, out of place: one staged front per row, spans 1.. read d_src
    assert (sp["nch"], sp["ns"], sp["W"], sp["calls"]) == (2, 40000, 5, (1, 1)) and sp["dst_off"] is not None
    assert all(pc.geom(cu, 1, 2, 40000, 5)["nsplit"] > 1 for cu in (8, 256, 304))
    assert any(c["ns"] == 40000 and c["W"] == 5 and c["calls"] and c["dst_off"] is None for c in S)


def test_header_table_and_library_agree_on_the_planar_entries():
    df.check_entries(("int rspt_hip_median_filter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, "
                      "size_t window, void* stream);",
                      "int rspt_hip_median_planar_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes);",
                      "int rspt_hip_median_filter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, "
                      "size_t window, void* d_state, void* stream);"),
                     ENTRIES, native_of={n: n.replace("planar_", "") for n in ENTRIES},  # pointer types as the native siblings
                     methods=("median_filter_planar_batch", "median_planar_state_bytes", "median_planar_state"))


def test_argument_checks_that_need_no_device():
    from rspt_amd import api

    L = api.lib()
    buf = C.create_string_buffer(4096)
    sp = (C.addressof(buf) + 15) & ~15
    n = C.c_size_t(12345)
    assert L.rspt_hip_median_planar_state_bytes(None, 5, C.byref(n)) == ERR_ARG and n.value == 12345
    assert L.rspt_hip_median_filter_planar_batch_dev(None, sp, sp, 1, 3, None) == ERR_ARG
    assert L.rspt_hip_median_filter_planar_stream_dev(None, sp, sp, 1, 3, sp, None) == ERR_ARG
    assert bytes(buf.raw) == bytes(4096)


def test_no_new_kernel_uses_scratch(asm):
    """k_med_planar: four buckets, wide and dword; the gathering mover; the planar kernels of the sort and the walk"""
    short = [n for n in asm if re.search(r"\d+k_med_planarILj", n)]
    assert len(short) == 8, sorted(n for n in asm if "k_med" in n)
    names = short + [n for n in asm if re.search(r"\d+k_medp_save", n)] + [n for n in asm if re.search(r"\d+k_medp_(tile_sort|walk)E", n)]
    assert len(names) == 11, names
    df.uses_no_scratch(asm, names)
    wide = [n for n in short if re.search(r"global_load_dwordx4", "".join(asm[n])) and re.search(r"global_store_dwordx4", "".join(asm[n]))]
    assert len(wide) == 4  # the aligned instantiations


# ---- GPU ----

def _what(c):
    return df.what(c, hide=("planar",))


def _clean(api, pk):
    return api.lib().rspt_hip_last_hip_error(pk._h) == 0


def _check(api, c, want=None, image=None, calls="own", states=None):
    """c through the planar entry between guards (devframe.planar_window), against the restatement -> (output, state bytes)"""
    if want is None:
        want, image = pc.expected(c)
    W = c["W"]
    return df.planar_window(api, c, lambda pk, src, **kw: pk.median_filter_planar_batch(src, W, **kw), lambda pk: pk.median_planar_state_bytes(W),
                            pc.state_bytes(W, c["nch"]), want, image, calls, states)


@pytest.mark.gpu
def test_gpu_record_cases_as_a_matrix_in_place_and_out_of_place(api):
    for c in mc.median_cases():
        if c["ns"] > 30000:
            continue  # (ecg12x34199, several tiles and four merge passes: the next test, to keep each one short)
        P, want = pc.record_planar(c), pc.record_expected(c["name"])
        for do in (None, 4):
            _check(api, dict(name=c["name"], nch=c["nch"], ns=c["ns"], nblocks=1, planar=P, W=c["W"], src_off=0, dst_off=do, calls=None, bps=c["bps"]), want)


@pytest.mark.gpu
def test_gpu_record_cases_of_the_long_recording(api):
    for c in mc.median_cases():
        if c["ns"] > 30000:
            P, want = pc.record_planar(c), pc.record_expected(c["name"])
            for do in (None, 8):
                _check(api, dict(name=c["name"], nch=c["nch"], ns=c["ns"], nblocks=1, planar=P, W=c["W"], src_off=0, dst_off=do, calls=None, bps=c["bps"]), want)


@pytest.mark.gpu
def test_gpu_stateless_row_ends(api):
    for c in pc.row_cases():
        _check(api, c)


@pytest.mark.gpu
def test_gpu_several_spans_per_row_in_place(api):
    import torch

    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for c in pc.span_cases():
        assert pc.geom(cu, c["nblocks"], c["nch"], c["ns"], c["W"])["nsplit"] > 1
        _check(api, c)


@pytest.mark.gpu
def test_gpu_pads_ties_and_truncation_toward_zero(api):
    for c in pc.value_cases():
        _check(api, c)


@pytest.mark.gpu
def test_gpu_values_outside_the_sample_width_are_taken_whole_and_stored_uncut(api):
    for c in pc.width_cases():
        got, sbytes = _check(api, c)
        got4, sbytes4 = _check(api, dict(c, bps=4))  # the handle's bps has no effect
        assert np.array_equal(got, got4) and (sbytes is None or np.array_equal(sbytes, sbytes4)), _what(c)


@pytest.mark.gpu
def test_gpu_both_sides_of_the_regime_switch(api):
    for c in pc.regime_cases():
        _check(api, c)


@pytest.mark.gpu
def test_gpu_generic_window_on_the_longest_row_and_refused_beyond_it(api):
    import torch

    ns = pc.MAX_RANKS
    P = pc.block(1, 1, ns, 2950, 1 << 24)
    _check(api, dict(name="ranks_limit", nch=1, ns=ns, nblocks=1, planar=P, W=33, src_off=0, dst_off=None, calls=None, bps=4), pc.stateless_expected(P, 33))
    pk = api.new_hzr(4, 1, ns + 1)
    raw, view = df.guarded_matrix(np.zeros((1, 1, ns + 1), dtype=np.int32))
    before = raw.clone()
    st = torch.cuda.current_stream().cuda_stream
    assert api.lib().rspt_hip_median_filter_planar_batch_dev(pk._h, view.data_ptr(), view.data_ptr(), 1, 33, st) == ERR_UNSUPPORTED
    assert api.lib().rspt_hip_median_filter_planar_batch_dev(pk._h, view.data_ptr(), view.data_ptr(), 1, 32, st) == 0  # (short windows: any ns)
    torch.cuda.synchronize()
    assert torch.equal(raw, before) and _clean(api, pk)  # (the median of zeros)
    pk.close()


@pytest.mark.gpu
def test_gpu_stream_bit_exact_with_its_state_after_every_call(api):
    for c in pc.stream_cases():
        states = []
        want, image = pc.expected(c)
        _check(api, c, states=states)
        rows = pc.rows_of(c["planar"])
        for b0, sb, out in states:  # the state and the output after each call are the restatement's
            assert np.array_equal(sb, pc.state_image(rows[: b0 * c["ns"]], c["W"])), (b0, _what(c))
            assert np.array_equal(out, want[:b0]), (b0, _what(c))
        if c["W"] == 1:
            assert not image.any() and image.size == 8
        if c["calls"] == pc.STREAM_CUTS[0] or c["name"] == pc.GENERIC_STREAM:  # however it is cut: one call leaves the same bytes
            _check(api, c, calls=(c["nblocks"],))


@pytest.mark.gpu
def test_gpu_more_than_one_piece_of_keys_in_place_against_the_native_stream_entry(api):
    """the shape of median_stream_cases.PIECES as a matrix: 8 ch, 80 blocks of 65536, W = 101, in place, against the native stream
    entry on from_planar_i32 of the same values (bps = 4)"""
    import torch

    Pc = msc.PIECES
    nch, ns, nb, W = Pc["nch"], Pc["ns"], Pc["nblocks"], Pc["W"]
    assert nch * ns * nb > 1 << 25 and W > pc.SHORT_MAX
    x = torch.from_numpy(msc.pieces_data().view(np.int8).astype(np.int32).reshape(nb, ns, nch)).cuda()  # [block][row][channel]
    pk = api.new_hzr(4, nch, ns)
    native = x.contiguous().view(torch.uint8).reshape(nb, -1)
    P = pk.to_planar_i32(native)
    assert torch.equal(P, x.transpose(1, 2))
    sp, sn = pk.median_planar_state(W), pk.median_state(W)
    pk.median_filter_planar_batch(P, W, state=sp)
    pk.median_filter_batch(native, W, state=sn)
    torch.cuda.synchronize()
    assert torch.equal(pk.from_planar_i32(P).reshape(nb, -1), native) and torch.equal(sp, sn) and _clean(api, pk)
    pk.close()


CROSS = ("rand5x1000_i16_w3", "rand5x1000_i16_w33", "ternary7x1001_i8_w6", "ds3x20000_i24_w31", "full_scale6x3000_i32_w40", "rand3x200_i32_w207")


def _streams(d_dst, d_sizes):
    import torch

    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().astype(np.uint64)
    dst = d_dst.cpu().numpy()
    assert not any(int(s) >> 63 for s in sizes)
    return [dst[i, : int(s)].tobytes() for i, s in enumerate(sizes)]


@pytest.mark.gpu
def test_gpu_cross_identities_with_the_native_entry_and_the_planar_packer(api):
    """from_planar_i32(median_planar(to_planar_i32(X))) == median_filter_batch(X), stateless and carried, and
    compress_planar_batch(median_planar(to_planar_i32(X))) gives the streams of compress_batch(median_filter_batch(X))"""
    import torch

    by = {c["name"]: c for c in mc.median_cases()}
    assert {by[n]["bps"] for n in CROSS} == {1, 2, 3, 4}
    for name in CROSS:
        c = by[name]
        bps, nch, ns, W = c["bps"], c["nch"], c["ns"], c["W"]
        X = np.stack([c["data"], c["data"][::-1].copy()])  # two blocks
        pk = api.new_xdelta_hzr(bps, nch, ns, 3)
        for carried in (False, True):
            sn = pk.median_state(W) if carried else None
            sp = pk.median_planar_state(W) if carried else None
            native = pk.median_filter_batch(torch.from_numpy(X).cuda(), W, state=sn)
            P = pk.median_filter_planar_batch(pk.to_planar_i32(torch.from_numpy(X).cuda()), W, state=sp)
            back = pk.from_planar_i32(P)
            torch.cuda.synchronize()
            assert torch.equal(back.reshape(2, -1), native.reshape(2, -1)), (name, carried)
            if not carried:
                assert np.array_equal(native.cpu().numpy().reshape(2, -1), np.stack([mc.median_filter(X[b], bps, nch, ns, W) for b in range(2)])), name
            elif bps == 4:
                assert torch.equal(sn, sp), name
            assert _streams(*pk.compress_planar_batch(P)) == _streams(*pk.compress_batch(native)), (name, carried)
        pk.close()


@pytest.mark.gpu
def test_gpu_native_and_planar_calls_alternate_on_one_state(api):
    """bps = 4: one recording in three calls -- native, planar, native and the other way round -- gives the restatement's run and
    state, on both sides of 32; and the sizes: equal at bps = 4, rows of int32 on a 2-byte handle"""
    import torch

    nch, ns, cuts = 3, 40, (2, 3, 2)
    nb = sum(cuts)
    P = pc.block(nb, nch, ns, 2960, 1 << 26)
    pk = api.new_hzr(4, nch, ns)
    bb = pk.block_bytes
    p2 = api.new_hzr(2, nch, ns)
    assert p2.median_planar_state_bytes(101) == 8 + (100 * nch * 4 + 7) // 8 * 8 != p2.median_state_bytes(101)
    assert p2.median_planar_state_bytes(2) == 8 + 16 and p2.median_planar_state(2).numel() == 24 and p2.median_planar_state_bytes(1) == 8
    p2.close()
    for W in (31, 101):  # W - 1 = 100 rows: two and a half blocks
        assert pk.median_planar_state_bytes(W) == pk.median_state_bytes(W) == 8 + (W - 1) * nch * 4
        model, image = pc.stream_expected(P, W)
        for plan in (["native", "planar", "native"], ["planar", "native", "planar"]):
            rec = pc.native_of(P).reshape(nb, bb).copy()
            state = pk.median_state(W)
            b0 = 0
            for n, layout in zip(cuts, plan):
                if layout == "native":
                    buf = torch.from_numpy(rec[b0 : b0 + n]).cuda()
                    pk.median_filter_batch(buf, W, state=state)
                    torch.cuda.synchronize()
                    rec[b0 : b0 + n] = buf.cpu().numpy()
                else:
                    rows = rec[b0 : b0 + n].reshape(-1).view("<i4").reshape(n * ns, nch)
                    raw, view = df.guarded_matrix(pc.planar_of(rows, n, nch, ns), 4)
                    pk.median_filter_planar_batch(view, W, state=state)
                    torch.cuda.synchronize()
                    assert df.guards_untouched(raw, 4, view.numel() * 4)
                    rec[b0 : b0 + n] = pc.native_of(view.cpu().numpy()).reshape(n, bb)
                b0 += n
            assert np.array_equal(rec.reshape(-1), pc.native_of(model)) and np.array_equal(state.cpu().numpy(), image), (W, plan)
    pk.close()


@pytest.mark.gpu
def test_gpu_back_to_back_calls_without_host_sync_repeat_identically(api):
    """calls of different windows on one handle and one stream with no host synchronisation between them -- short, generic, a native
    median call in between, stream calls -- while the staged fronts, the head and the keys grow: the right bytes, twice"""
    import torch

    P = pc.block(2, 2, 40000, 2970)
    Ws = (3, 32, 101, 9)
    want = [pc.stateless_expected(P, W) for W in Ws]
    swant = [pc.stream_expected(P, W)[0] for W in (5, 101)]
    nat_in = pc.native_of(P).reshape(2, -1)
    nat_want = pc.native_of(pc.stateless_expected(P, 7)).reshape(2, -1)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert pc.geom(cu, 2, 2, 40000, 32)["nsplit"] > 1
    runs = []
    for rep in range(2):
        pk = api.new_hzr(4, 2, 40000)
        bufs = [torch.from_numpy(P.copy()).cuda() for _ in range(6)]
        nat = torch.from_numpy(nat_in.copy()).cuda()
        st = [pk.median_planar_state(5), pk.median_planar_state(101)]
        torch.cuda.synchronize()
        pk.median_filter_planar_batch(bufs[0], Ws[0])
        pk.median_filter_planar_batch(bufs[1], Ws[1])
        pk.median_filter_batch(nat, 7)
        pk.median_filter_planar_batch(bufs[2], Ws[2])
        pk.median_filter_planar_batch(bufs[3], Ws[3])
        pk.median_filter_planar_batch(bufs[4], 5, state=st[0])
        pk.median_filter_planar_batch(bufs[5], 101, state=st[1])
        torch.cuda.synchronize()
        got = [b.cpu().numpy() for b in bufs] + [nat.cpu().numpy()]
        for g, w, what in zip(got, want + swant + [nat_want], list(Ws) + ["stream 5", "stream 101", "native 7"]):
            assert np.array_equal(g, w), (rep, what)
        runs.append(b"".join(g.tobytes() for g in got))
        pk.close()
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_gpu_destroying_the_handle_with_a_call_in_flight_ends_cleanly(api):
    import torch

    P = pc.block(2, 2, 40000, 2980)
    for W, carried in ((32, False), (101, True)):
        pk = api.new_hzr(4, 2, 40000)
        buf = torch.from_numpy(P.copy()).cuda()
        state = pk.median_planar_state(W) if carried else None
        pk.median_filter_planar_batch(buf, W, state=state)
        pk.close()  # (no synchronisation in between)
        torch.cuda.synchronize()
        want = pc.stream_expected(P, W)[0] if carried else pc.stateless_expected(P, W)
        assert np.array_equal(buf.cpu().numpy(), want), W


@pytest.mark.gpu
def test_gpu_planar_entries_refuse_bad_arguments_and_write_nothing(api):
    import torch

    L = api.lib()
    nch, ns = 3, 100
    pk = api.new_hzr(2, nch, ns)
    P = pc.block(4, nch, ns, 2990)
    raw, view = df.guarded_matrix(P, 0)
    before = raw.clone()
    n = P.size * 4 // 2  # bytes of two blocks
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    straw, state = df.guarded(pk.median_planar_state_bytes((1 << 17) + 1), 8, fill=0)
    sbefore = straw.clone()
    base = view.data_ptr()

    def call(stream_form, handle=h, s=base, d=base, nblocks=2, W=5, state_ptr=state.data_ptr()):
        if stream_form:
            return L.rspt_hip_median_filter_planar_stream_dev(handle, s, d, nblocks, W, state_ptr, st)
        return L.rspt_hip_median_filter_planar_batch_dev(handle, s, d, nblocks, W, st)

    too_many = (1 << 31) // nch + 1  # nblocks * nch >= 2^31
    too_long = ((1 << 31) - (1 << 17)) // ns + 1  # a stream call of 2^31 - 2^17 rows and more
    for sf in (False, True):
        assert call(sf, handle=None) == ERR_ARG and call(sf, s=None) == ERR_ARG and call(sf, d=None) == ERR_ARG
        assert call(sf, nblocks=0) == ERR_ARG and call(sf, nblocks=too_many) == ERR_ARG and call(sf, W=0) == ERR_ARG
        for off in (1, 2, 3):  # off the 4-byte alignment, either buffer
            assert call(sf, s=base + off, d=base + off) == ERR_ARG and call(sf, s=base + off, d=base + n) == ERR_ARG and call(sf, d=base + n + off) == ERR_ARG
        assert call(sf, d=base + 16) == ERR_ARG and call(sf, d=base + n // 2) == ERR_ARG and call(sf, s=base + n // 2, d=base) == ERR_ARG  # partial overlap
        for W in (1, 33):  # (a copy and the generic path check as the short one does)
            assert call(sf, W=W, d=base + 16) == ERR_ARG and call(sf, W=W, s=base + 2, d=base + 2) == ERR_ARG
    assert call(True, state_ptr=None) == ERR_ARG and call(True, state_ptr=state.data_ptr() + 4) == ERR_ARG
    assert call(True, nblocks=too_long) == ERR_UNSUPPORTED and call(True, nblocks=too_long, W=101) == ERR_UNSUPPORTED
    assert call(True, W=(1 << 17) + 2) == ERR_UNSUPPORTED and call(True, W=1 << 40) == ERR_UNSUPPORTED  # W > 32 with W - 1 > 2^17
    nb = C.c_size_t(777)
    assert L.rspt_hip_median_planar_state_bytes(h, 3, None) == ERR_ARG and L.rspt_hip_median_planar_state_bytes(h, 0, C.byref(nb)) == ERR_ARG
    assert L.rspt_hip_median_planar_state_bytes(h, (1 << 17) + 2, C.byref(nb)) == ERR_UNSUPPORTED and nb.value == 777
    assert L.rspt_hip_median_planar_state_bytes(h, (1 << 17) + 1, C.byref(nb)) == 0 and nb.value == 8 + (1 << 17) * nch * 4
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.zeros(8192 * 4, dtype=torch.int32, device="cuda")
    wstate = torch.zeros(8 + 2 * 8192 * 4, dtype=torch.uint8, device="cuda")
    assert call(False, handle=wide._h, s=wbuf.data_ptr(), d=wbuf.data_ptr(), nblocks=1, W=3) == ERR_UNSUPPORTED
    assert call(True, handle=wide._h, s=wbuf.data_ptr(), d=wbuf.data_ptr(), nblocks=1, W=3, state_ptr=wstate.data_ptr()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(raw, before) and torch.equal(straw, sbefore) and int(wbuf.count_nonzero()) == 0 and int(wstate.count_nonzero()) == 0
    assert _clean(api, pk) and _clean(api, wide)
    wide.close()
    with pytest.raises(AssertionError):
        pk.median_filter_planar_batch(view.view(torch.uint8), 3)  # (not an int32 tensor)
    # accepted: the longest carried window, apart, on a handle whose bps is not 4; a stateless window far above ns
    assert call(True, W=(1 << 17) + 1, d=base + n) == 0 and call(False, W=1 << 40) == 0
    torch.cuda.synchronize()
    got = view.cpu().numpy()
    assert np.array_equal(got[2:], pc.stream_expected(P[:2], (1 << 17) + 1)[0]) and np.array_equal(got[:2], pc.stateless_expected(P[:2], 1 << 40))
    assert df.guards_untouched(raw, 0, P.size * 4) and df.guards_untouched(straw, 8, state.numel())
    pk.close()


@pytest.mark.gpu
def test_gpu_planar_entries_run_on_a_foreign_stream(api):
    import torch

    s = torch.cuda.Stream()
    picks = [next(c for c in pc.row_cases() if c["ns"] == pc.CHUNK + 1 and c["nch"] > 1), pc.span_cases()[0], pc.regime_cases()[-1],
             next(c for c in pc.stream_cases() if c["ns"] == 100 and c["dst_off"] is None),
             next(c for c in pc.stream_cases() if c["ns"] == 12 and c["dst_off"] is not None and c["W"] <= 32)]
    for c in picks:
        want = pc.expected(c)[0]
        pk = api.new_hzr(4, c["nch"], c["ns"])
        raw, src = df.guarded_matrix(c["planar"], c["src_off"])
        draw, dst = (raw, src) if c["dst_off"] is None else df.guarded_matrix(c["planar"], c["dst_off"], fill=0)
        state = pk.median_planar_state(c["W"]) if c["calls"] else None
        s.wait_stream(torch.cuda.current_stream())
        b0 = 0
        for k in c["calls"] or [c["nblocks"]]:
            pk.median_filter_planar_batch(src[b0 : b0 + k], c["W"], d_out=None if dst is src else dst[b0 : b0 + k], state=state, stream=s.cuda_stream)
            b0 += k
        s.synchronize()
        off = c["src_off"] if dst is src else c["dst_off"]
        assert np.array_equal(dst.cpu().numpy(), want) and df.guards_untouched(draw, off, dst.numel() * 4), _what(c)
        pk.close()


@pytest.mark.gpu
def test_gpu_random_sweep(api):
    """300 random small cases against the restatement: shapes, windows, offsets, in and out of place, stateless or cut into calls"""
    S = pc.sweep_cases()
    assert len(S) == 300 and {bool(c["calls"]) for c in S} == {True, False} and {c["dst_off"] is None for c in S} == {True, False}
    assert {c["W"] <= pc.SHORT_MAX for c in S} == {True, False}
    for c in S:
        want, image = pc.stream_expected(c["planar"], c["W"]) if c["calls"] else (pc.stateless_expected(c["planar"], c["W"]), None)
        _check(api, c, want, image)
