"""The rolling-window median with a carried state: one reference rolling_window_median<double> per channel over a
recording that arrives in blocks, on the GPU: rspt_hip_median_state_bytes, rspt_hip_median_filter_stream_dev.

CPU: the record's inputs, the numpy restatement (tests/median_stream_cases.py) against the reference's answers
(tests/golden/median_stream_record.json), what the record covers, the C ABI, the device ISA of the kernels, and the argument
checks that need no device.
GPU (-m gpu): every case bit-exact against the record and the restatement however the recording is cut into calls, in place and
out of place, the state's bytes, the equivalence with the stateless stage, that the state is used, and the statuses."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import devframe as df
import median_cases as mc
import median_stream_cases as msc
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_median_state_bytes", "rspt_hip_median_filter_stream_dev")

CASES = msc.stream_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def record():
    return {r["name"]: r for r in df.golden("median_stream_record.json")["cases"]}


@functools.lru_cache(maxsize=None)
def _want(name):
    return msc.filtered(BY_NAME[name])


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    assert len(CASES) == len(record) == len(set(NAMES))
    for c in CASES:
        r = record[c["name"]]
        assert (c["bps"], c["nch"], c["ns"], c["nblocks"], c["W"]) == (r["bps"], r["nch"], r["ns"], r["nblocks"], r["W"]), c["name"]
        assert msc.crc(c["data"]) == r["in_crc32"], c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(record, name):
    y = _want(name)
    assert digest(y) == record[name]["digest"] and msc.crc(y) == record[name]["crc32"]


def test_the_reference_own_sequence_in_blocks_of_four(record):
    """the 20 values of the reference's median test, 5 blocks of 4: the restatement truncates the doubles that test expects"""
    for W in (5, 6, 7):
        c = BY_NAME["ref20_4x5_w%d" % W]
        assert (c["ns"], c["nblocks"]) == (4, 5)
        got = mc.native_to_i32(_want(c["name"]), 4, 1, 20)[:, 0]
        assert got.tolist() == [int(v) for v in mc.REF20_EXPECTED[W]]


def test_the_record_covers_what_it_must(record):
    R = list(record.values())
    rows = lambda r: r["ns"] * r["nblocks"]  # noqa: E731
    assert {r["bps"] for r in R} == {1, 2, 3, 4}
    assert any(r["nch"] == 1 for r in R)
    assert any((r["nch"], r["ns"], r["nblocks"], r["bps"]) == (3, 1000, 20, 3) for r in R)
    assert any((r["nch"], r["ns"], r["nblocks"], r["bps"]) == (12, 2048, 16, 4) for r in R)
    assert any(r["ns"] < 64 for r in R) and any(r["ns"] > 64 and r["ns"] % 64 for r in R)
    assert {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 100, 101, 1500} <= {r["W"] for r in R}
    assert any(r["W"] == 4097 and r["ns"] == 700 for r in R)
    assert any(r["W"] == 65536 and (r["nch"], r["ns"]) == (2, 40) and 1 < r["nblocks"] and rows(r) < 65535 for r in R)
    long = [r for r in R if r["W"] > msc.SHORT_MAX and rows(r) > (1 << 18)]
    assert any(r["W"] <= 101 for r in long) and any(r["W"] == (1 << 17) + 1 for r in long) and len(long) >= 2
    assert any(r["W"] > msc.SHORT_MAX and r["ns"] > (1 << 18) for r in R)
    assert any(r["W"] - 1 > r["ns"] and r["nblocks"] > 1 for r in R)  # the per-block cut makes calls shorter than W - 1 rows
    for W in (5, 6, 7):
        assert (record["ref20_4x5_w%d" % W]["ns"], record["ref20_4x5_w%d" % W]["nblocks"]) == (4, 5)
    # ties
    assert any(r["bps"] == 1 and rows(r) >= 1000 for r in R)
    for prefix, distinct in (("constant", 1), ("alternating", 2)):
        group = [c for c in CASES if c["name"].startswith(prefix)]
        assert group and all(len(np.unique(mc.native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]))) == distinct for c in group)
        assert any(c["W"] <= msc.SHORT_MAX for c in group) and any(c["W"] > msc.SHORT_MAX for c in group)
    # negative pairs whose mean is no integer: truncation toward zero differs from the floor
    c = BY_NAME["negative2x100x4_i32_w2"]
    x = mc.native_to_i32(c["data"], 4, 2, 400).astype(np.int64)
    s = x[1:] + x[:-1]
    assert (x < 0).all() and ((s & 1) == 1).sum() > 50
    y = mc.native_to_i32(_want(c["name"]), 4, 2, 400).astype(np.int64)
    odd = (s & 1) == 1
    assert np.array_equal(y[1:][odd], (s[odd] + 1) // 2) and not np.array_equal(y[1:][odd], s[odd] // 2)


def test_state_layout_restatement():
    """fill, the valid rows last, zeros in front, 8-byte padding"""
    d = np.arange(1, 1 + 2 * 3 * 5, dtype=np.uint8)  # 5 rows of 3 ch int16
    s = msc.state_after(d, 2, 3, 8)
    assert s.size == 8 + 48 and int(s[:8].view(np.uint64)[0]) == 5
    assert not s[8 : 8 + 12].any() and np.array_equal(s[8 + 12 : 8 + 42], d) and not s[50:].any()
    s = msc.state_after(d, 2, 3, 3)
    assert int(s[:8].view(np.uint64)[0]) == 2 and np.array_equal(s[8:20], d[18:]) and s.size == 24
    assert msc.state_after(d, 2, 3, 1).size == 8 and not msc.state_after(d, 2, 3, 1).any()


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries((
        "int rspt_hip_median_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes);",
        "int rspt_hip_median_filter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, "
        "void* d_state, void* stream);",
    ), ENTRIES)


def test_the_stateless_entry_keeps_its_signature():
    hdr = df.header()
    assert "int rspt_hip_median_filter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* stream);" in hdr


def test_argument_checks_that_need_no_device():
    """a NULL handle and a NULL `bytes` are refused before anything touches a device"""
    from rspt_amd import api

    L = api.lib()
    n = C.c_size_t(12345)
    assert L.rspt_hip_median_state_bytes(None, 5, C.byref(n)) == ERR_ARG and n.value == 12345
    state = C.create_string_buffer(4096)
    sp = (C.addressof(state) + 7) & ~7
    assert L.rspt_hip_median_filter_stream_dev(None, sp, sp, 1, 5, sp, None) == ERR_ARG


FP = re.compile(r"^\s+(v_\w+_f(64|32|16)\w*|v_pk_\w+_f(32|16)\w*|v_mfma\w*|v_fma\w*|v_fmac\w*|v_mad\w*_f\w+|v_mac\w*_f\w+)\b")
# what the compiler makes of an integer division by a run-time value (u / g.nsplit, tid % g.cw, blockIdx.x / spans, ...): a
# reciprocal estimate in f32 and its correction.  The stateless kernels hold the same instructions for the same divisions.
INT_DIVISION = re.compile(r"^v_(cvt_f32_u32|cvt_u32_f32|rcp_iflag_f32|rcp_f32|mul_f32|trunc_f32|fmac_f32|fmamk_f32|fma_f32|mad_f32|madmk_f32|ldexp_f32)(_e32|_e64)?$")


def test_the_median_kernels_hold_no_floating_point(asm):
    """no f64, f16, packed or matrix instruction anywhere in the stage; the only f32 instructions are those of the compiler's
    integer-division expansion, no more of them in a carried-state instantiation than index arithmetic needs; and the movers,
    which divide nothing, hold no floating-point instruction at all"""
    names = [n for n in asm if re.search(r"\d+k_med_(short|tile_sort|merge|walk|carry)", n)]
    assert len(names) == 2 * (24 + 6 + 6) + 1 + 4, len(names)
    for n in names:
        fp = [FP.match(ln).group(1) for ln in asm[n] if FP.match(ln)]
        if "k_med_carry" in n:
            assert not fp, (n, fp)
        bad = [m for m in fp if not INT_DIVISION.match(m)]
        assert not bad, (n, bad)
        assert len(fp) <= 64, (n, len(fp))  # (a handful of divisions, 8 to 20 instructions each; sample arithmetic would be in the unrolled sweeps)


def test_the_kernel_instantiations(asm):
    """the stateless instantiations are still there, by count, beside as many with a head / in stream mode; the mover is a kernel
    of its own (no k_fir_carry in its name), in bytes and in words"""
    short = [n for n in asm if re.search(r"11k_med_shortIL", n)]
    sort = [n for n in asm if re.search(r"15k_med_tile_sortIL", n)]
    walk = [n for n in asm if re.search(r"10k_med_walkIL", n)]
    for group, per in ((short, 24), (sort, 6), (walk, 6)):  # (4 register buckets x) int8, int16 (+aligned), int24, int32 (+aligned)
        assert len([n for n in group if n.split("ELb")[-1].startswith("0")]) == per, sorted(group)
        assert len([n for n in group if n.split("ELb")[-1].startswith("1")]) == per, sorted(group)
    movers = [n for n in asm if "k_med_carry" in n]
    assert len(movers) == 4 and not [n for n in movers if "k_fir_carry" in n], movers


def test_the_widest_short_kernel_with_a_head_uses_no_scratch(asm):
    """k_med_short<32, ..., HEAD = true>: its 32-slot window stays in registers"""
    names = [n for n in asm if re.search(r"11k_med_shortILj32E", n) and n.split("ELb")[-1].startswith("1")]
    assert len(names) == 6, names
    df.uses_no_scratch(asm, names)


# ---- GPU ----

def _drive(pk, W, data, split, state, out_of_place=False, sync=False):
    """the recording through successive calls of split[i] blocks each; -> (filtered recording, source afterwards) as bytes"""
    import torch

    src = torch.from_numpy(np.asarray(data, dtype=np.uint8)).cuda()
    dst = torch.full_like(src, 0xA5) if out_of_place else None
    bb, b0 = pk.block_bytes, 0
    for k in split:
        lo, hi = b0 * bb, (b0 + k) * bb
        pk.median_filter_batch(src[lo:hi], W, d_dst=None if dst is None else dst[lo:hi], state=state)
        if sync:
            torch.cuda.synchronize()
        b0 += k
    assert b0 * bb == src.numel()
    torch.cuda.synchronize()
    return (dst if out_of_place else src).cpu().numpy(), src.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_stream_bit_exact_however_the_recording_is_cut(api, record, name):
    """one call, one call per block (calls shorter than W - 1 rows where ns < W - 1) and 1, 3, rest; in place and out of place;
    the state's bytes afterwards are the same for every cut and what the layout rules predict"""
    c = BY_NAME[name]
    want = _want(name)
    assert digest(want) == record[name]["digest"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    state_want = msc.state_after(c["data"], c["bps"], c["nch"], c["W"])
    for how, split in msc.splits(c["nblocks"]).items():
        for oop in (False, True):
            state = pk.median_state(c["W"])
            got, src_after = _drive(pk, c["W"], c["data"], split, state, out_of_place=oop)
            where = (how, "out of place" if oop else "in place")
            assert np.array_equal(got, want) and digest(got) == record[name]["digest"], where
            if oop:
                assert np.array_equal(src_after, c["data"]), where
            assert np.array_equal(state.cpu().numpy(), state_want), where
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ecg12x2048x16_i32_w31", "ecg12x2048x16_i32_w1500", "ds3x1000x20_i24_w101", "rand1x40x8_i8_w5",
                                  "rand3x700x4_i24_w4097", "walk1x65536x5_i32_w101", "synth5x300x10_i16_w100"])
def test_gpu_stream_on_a_fresh_state_equals_the_stateless_stage_on_one_long_block(api, name):
    import torch

    c = BY_NAME[name]
    rows = c["ns"] * c["nblocks"]
    if c["W"] > msc.SHORT_MAX and rows > (1 << 18):
        rows = 1 << 18  # the stateless entry's limit
        assert rows % c["ns"] == 0
    data = c["data"][: rows * c["nch"] * c["bps"]]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    got, _ = _drive(pk, c["W"], data, [rows // c["ns"]], pk.median_state(c["W"]))
    pk.close()
    one = api.new_hzr(c["bps"], c["nch"], rows)
    buf = torch.from_numpy(data).cuda()
    one.median_filter_batch(buf, c["W"])
    torch.cuda.synchronize()
    assert np.array_equal(got, buf.cpu().numpy())
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds3x1000x20_i24_w101", "ecg12x2048x16_i32_w31"])
def test_gpu_the_state_is_used(api, name):
    """block 1 behind block 0's state differs from the stateless output on block 1 in its first W - 1 rows and equals it after"""
    import torch

    c = BY_NAME[name]
    W, stride = c["W"], c["bps"] * c["nch"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    bb = pk.block_bytes
    state = pk.median_state(W)
    assert int(state.count_nonzero()) == 0
    _drive(pk, W, c["data"][:bb], [1], state)
    assert int(state.count_nonzero()) > 0
    carried, _ = _drive(pk, W, c["data"][bb : 2 * bb], [1], state)
    buf = torch.from_numpy(c["data"][bb : 2 * bb]).cuda()
    pk.median_filter_batch(buf, W)
    torch.cuda.synchronize()
    fresh = buf.cpu().numpy()
    assert np.array_equal(carried, _want(name)[bb : 2 * bb])
    cut = (W - 1) * stride
    assert not np.array_equal(carried[:cut], fresh[:cut]) and np.array_equal(carried[cut:], fresh[cut:])
    state.zero_()
    again, _ = _drive(pk, W, c["data"][bb : 2 * bb], [1], state)
    assert np.array_equal(again, fresh)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rand7x232x4_i32_w16", "synth5x300x10_i16_w101"])
def test_gpu_two_states_interleaved_on_one_handle(api, name):
    """two recordings of one shape, their blocks alternating on one handle and one stream, each with its own state; no host
    synchronisation between the calls"""
    import torch

    c = BY_NAME[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    rows = c["ns"] * c["nblocks"]
    other = dict(c, data=msc.cases._rand_native(c["nch"], rows, c["bps"], 4242, 1 << (8 * c["bps"] - 3)))
    bufs = [torch.from_numpy(x["data"]).cuda() for x in (c, other)]
    states = [pk.median_state(c["W"]), pk.median_state(c["W"])]
    bb = pk.block_bytes
    for b in range(c["nblocks"]):
        for buf, st in zip(bufs, states):
            pk.median_filter_batch(buf[b * bb : (b + 1) * bb], c["W"], state=st)
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0].cpu().numpy(), _want(name))
    assert np.array_equal(bufs[1].cpu().numpy(), msc.filtered(other))
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ds3x1000x20_i24_w1000", "rand5x100x6_i16_w31", "rand2x40x5_i32_w65536"])
def test_gpu_back_to_back_calls_equal_calls_with_a_host_synchronisation_between_them(api, name):
    c = BY_NAME[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for sync in (False, True):
        got, _ = _drive(pk, c["W"], c["data"], [1] * c["nblocks"], pk.median_state(c["W"]), sync=sync)
        assert np.array_equal(got, _want(name)), sync
    pk.close()


@pytest.mark.gpu
def test_gpu_in_place_generic_call_of_more_than_one_piece(api):
    """in place, W > 32, more than 2^25 samples in one call: the pieces overlap by W - 1 rows that an earlier piece's walk must not
    have overwritten.  Against the same recording filtered out of place block by block (every call one piece), and against the
    restatement on the rows around every segment edge and on the recording's first and last rows."""
    import torch

    P = msc.PIECES
    bps, nch, ns, nb, W = P["bps"], P["nch"], P["ns"], P["nblocks"], P["W"]
    assert W > msc.SHORT_MAX and nch * ns * nb > (1 << 25)
    data = msc.pieces_data()
    pk = api.new_hzr(bps, nch, ns)
    st_a, st_b = pk.median_state(W), pk.median_state(W)
    want, _ = _drive(pk, W, data, [1] * nb, st_a, out_of_place=True)
    src = torch.from_numpy(data).cuda()
    pk.median_filter_batch(src, W, state=st_b)
    torch.cuda.synchronize()
    got = src.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(st_a.cpu().numpy(), st_b.cpu().numpy())
    assert np.array_equal(st_b.cpu().numpy(), msc.state_after(data, bps, nch, W))
    x = mc.native_to_i32(data, bps, nch, ns * nb)
    y = mc.native_to_i32(got, bps, nch, ns * nb)
    rows = ns * nb
    assert np.array_equal(y[:5000], msc.median_stream_i32(x[:5000], W))
    L = 65536 - (W - 1)
    edges = list(range(L, rows, L)) + [rows - 1500]
    for e in edges:
        a, b = max(W - 1, e - 1500), min(rows, e + 1500)
        assert np.array_equal(y[a:b], msc.median_stream_i32(x[a - (W - 1) : b], W)[W - 1 :]), e
    pk.close()


@pytest.mark.gpu
def test_gpu_seeded_random_recordings(api):
    """120 fixed seeds: shape, width, W on both sides of 32, the cut, in place or out of place, against the restatement"""
    generic = 0
    for seed in range(120):
        c = msc.random_case(seed)
        generic += c["W"] > msc.SHORT_MAX
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        state = pk.median_state(c["W"])
        got, src_after = _drive(pk, c["W"], c["data"], c["cut"], state, out_of_place=c["out_of_place"])
        assert np.array_equal(got, msc.filtered(c)), (seed, {k: v for k, v in c.items() if k != "data"})
        assert np.array_equal(state.cpu().numpy(), msc.state_after(c["data"], c["bps"], c["nch"], c["W"])), seed
        if c["out_of_place"]:
            assert np.array_equal(src_after, c["data"]), seed
        pk.close()
    assert 20 < generic < 100


@pytest.mark.gpu
def test_gpu_state_sizes(api):
    for bps, nch, ns in ((4, 12, 2048), (3, 3, 1000), (1, 1, 40)):
        pk = api.new_hzr(bps, nch, ns)
        for W in (1, 2, 32, 33, 65536, (1 << 17) + 1):
            want = 8 + ((W - 1) * nch * bps + 7) // 8 * 8
            assert pk.median_state_bytes(W) == want
            st = pk.median_state(W)
            assert st.numel() == want and st.data_ptr() % 8 == 0 and int(st.count_nonzero()) == 0
        pk.close()


@pytest.mark.gpu
def test_gpu_window_one_copies_and_leaves_the_state_zero(api):
    c = BY_NAME["rand1x40x8_i8_w1"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for oop in (False, True):
        state = pk.median_state(1)
        assert state.numel() == 8
        got, _ = _drive(pk, 1, c["data"], [3, 5], state, out_of_place=oop)
        assert np.array_equal(got, c["data"]) and int(state.count_nonzero()) == 0
    pk.close()


@pytest.mark.gpu
def test_gpu_stream_entry_statuses(api):
    import torch

    L = api.lib()
    pk = api.new_hzr(4, 3, 100)
    bb = pk.block_bytes
    buf = torch.zeros(4 * bb, dtype=torch.uint8, device="cuda")
    src = buf[: 2 * bb]
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    state = torch.zeros(pk.median_state_bytes((1 << 17) + 1) + 8, dtype=torch.uint8, device="cuda")
    nb = C.c_size_t()
    assert L.rspt_hip_median_state_bytes(h, 5, None) == ERR_ARG
    assert L.rspt_hip_median_state_bytes(h, 0, C.byref(nb)) == ERR_ARG
    assert L.rspt_hip_median_state_bytes(h, (1 << 17) + 2, C.byref(nb)) == ERR_UNSUPPORTED

    def med(W=5, nblocks=2, state=state.data_ptr(), s=src.data_ptr(), d=src.data_ptr(), handle=h):
        return L.rspt_hip_median_filter_stream_dev(handle, s, d, nblocks, W, state, st)

    assert med(state=None) == ERR_ARG and med(state=state.data_ptr() + 4) == ERR_ARG  # NULL / misaligned state
    assert med(W=0) == ERR_ARG and med(nblocks=0) == ERR_ARG
    assert med(s=None) == ERR_ARG and med(d=None) == ERR_ARG
    assert med(d=buf[16 : 16 + 2 * bb].data_ptr()) == ERR_ARG and med(d=buf[bb : 3 * bb].data_ptr()) == ERR_ARG  # partial overlap
    assert med(nblocks=(1 << 31) // 3 + 1) == ERR_ARG  # nblocks * nch >= 2^31
    assert med(W=(1 << 17) + 2) == ERR_UNSUPPORTED and med(W=1 << 40) == ERR_UNSUPPORTED  # W > 32 with W - 1 > 2^17
    # the row limit, 2^31 - 2^17 rows: refused before anything is launched (no such buffer exists here)
    limit = (1 << 31) - (1 << 17)
    assert med(nblocks=(limit + 99) // 100) == ERR_UNSUPPORTED and med(W=101, nblocks=(limit + 99) // 100) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0 and int(state.count_nonzero()) == 0  # nothing ran
    # accepted: the extremes, apart
    assert med(W=(1 << 17) + 1, d=buf[2 * bb :].data_ptr()) == 0 and med(W=32) == 0 and med(W=33) == 0
    torch.cuda.synchronize()
    pk.close()
    # ns above 2^18 with a window above 32: the stateless entry refuses it, the stream entry takes it
    big = api.new_hzr(1, 1, (1 << 18) + 1)
    b = torch.zeros(big.block_bytes, dtype=torch.uint8, device="cuda")
    bstate = big.median_state(33)
    assert L.rspt_hip_median_filter_batch_dev(big._h, b.data_ptr(), b.data_ptr(), 1, 33, st) == ERR_UNSUPPORTED
    assert L.rspt_hip_median_filter_stream_dev(big._h, b.data_ptr(), b.data_ptr(), 1, 33, bstate.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(b.count_nonzero()) == 0
    big.close()
