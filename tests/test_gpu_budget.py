"""Compress to a byte budget (rspt_hip_compress_budget_batch_dev) against the composed oracle on the same device: per ladder entry
one plain rspt_hip_set_quantizer + compress_batch + decompress_batch.  The expected choices are tests/budget_cases.py's choose()
on THOSE sizes, and the budgets are placed on them at run time (exactly at a size, one byte below, below the smallest), per block
through d_budget and once as the call's one limit.  Held to the oracle: d_choice, d_sizes, the stream bytes, the whole table of
candidate sizes, the samples decoded with ladder= and choice=d_choice, and that the handle's quantiser is what it was.  Where
the batched route runs, the general and the batched route are forced in turn (rspt_hip_debug_set_budget_route) and both held to
the oracle, so to each other.  Around it: the batch shapes on either side of a wave and of the 65535-slot bound, ladders whose
sizes are not sorted or repeat, the handle's state behind a budget call, a stride the chosen stream does not fit, the refusals."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import cases
import devframe as df
import lossy_dev as ld
import lossy_quantizer_cases as lq
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
NBLOCKS = 5
ROUTE_NAMES = {0: "auto", 1: "general", 2: "batched"}
MID = ("hadamard", 2, 5, 1024, 3)  # the shape of the tests that are not about a shape


def _new(api, shape):
    kind, bps, nch, ns, nb = shape
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _composed(pk, d_src, ladder):
    """what a user does today, per ladder entry: (streams, sizes, decoded) on the host; the handle is left as it was"""
    return [(o["dst"], o["sizes"], o["out"]) for o in ld.composed(pk, d_src, ladder)]


def _table(oracle):
    t = np.stack([o[1] for o in oracle])
    assert t.min() > 0 and not (t.view(np.uint64) & np.uint64(BIT63)).any()
    return t


def _held_to_the_oracle(pk, d_src, ladder, oracle, budget, tag):
    """one budget call -- budget: an int, or one int per block -- checked in full; -> the choices"""
    B = d_src.shape[0]
    table = _table(oracle)
    # (the work area's guard, the handle's quantiser, the decoder's consumed bytes and the handle's HIP error: lossy_dev.rate_call)
    limits, choice, sizes, dst, out, cand = map(ld.rate_call(pk, "budget", d_src, budget, ladder, tag).get, ld.BUDGET_FIELDS)
    assert np.array_equal(cand, table), (tag, "the table of candidate sizes")
    for b in range(B):
        k = bc.choose(table[:, b], limits[b])
        assert int(choice[b]) == k, (tag, b, table[:, b].tolist(), limits[b], int(choice[b]))
        n = int(table[k, b])
        assert int(sizes[b]) == n, (tag, b, k)
        assert np.array_equal(dst[b, :n], oracle[k][0][b, :n]), (tag, b, k, "stream")
        assert np.array_equal(out[b], oracle[k][2][b]), (tag, b, k, "decoded")
    return choice


@pytest.fixture(scope="module")
def runs(api):
    """per shape, once: a handle, 5 blocks -- random, walk, constant, full scale, random -- and the composed oracle of its ladder"""
    import torch

    memo = {}

    def get(shape):
        if shape not in memo:
            pk = _new(api, shape)
            d_src = torch.from_numpy(bc.batch_native(shape, NBLOCKS)).cuda()
            memo[shape] = (pk, d_src, _composed(pk, d_src, bc.ladder_of(shape[0])))
        return memo[shape]

    yield get
    for pk, _, _ in memo.values():
        pk.close()


SHAPE_RUNS = [(s, 0) for s in bc.SHAPES] + [(s, r) for s in bc.SHAPES if bc.batched(s) for r in (1, 2)]


def test_the_batched_route_is_offered_where_the_header_says(api):
    for s in bc.SHAPES:
        pk = _new(api, s)
        L = api.lib()
        assert L.rspt_hip_debug_set_budget_route(pk._h, 2) == (0 if bc.batched(s) else ERR_UNSUPPORTED), s
        assert L.rspt_hip_debug_set_budget_route(pk._h, 1) == 0 and L.rspt_hip_debug_set_budget_route(pk._h, 0) == 0
        assert L.rspt_hip_debug_set_budget_route(pk._h, 3) == ERR_ARG and L.rspt_hip_debug_set_budget_route(pk._h, -1) == ERR_ARG
        pk.close()
    assert [bc.batched(s) for s in bc.HADAMARD_SHAPES] == [True] * 5 + [False] * 3 and not any(bc.batched(s) for s in bc.DCT_SHAPES)


@pytest.mark.parametrize("shape,route", SHAPE_RUNS, ids=["%s-%s" % (bc.shape_id(s), ROUTE_NAMES[r]) for s, r in SHAPE_RUNS])
def test_every_shape_against_the_composed_oracle(runs, shape, route):
    pk, d_src, oracle = runs(shape)
    ladder = bc.ladder_of(shape[0])
    table = _table(oracle)
    pk.debug_set_budget_route(route)
    tag = (bc.shape_id(shape), ROUTE_NAMES[route])
    _held_to_the_oracle(pk, d_src, ladder, oracle, bc.derive_budgets(table), tag + ("per block",))
    _held_to_the_oracle(pk, d_src, ladder, oracle, bc.scalar_budget(table), tag + ("one limit",))
    pk.debug_set_budget_route(0)


BATCH_RUNS = [(B, K, r) for B, K in ((1, 8), (9, 8), (3, 1)) for r in (0, 1, 2)]


@pytest.mark.parametrize("B,K,route", BATCH_RUNS, ids=["%dx%d-%s" % (B, K, ROUTE_NAMES[r]) for B, K, r in BATCH_RUNS])
def test_batch_shapes(api, B, K, route):
    """1 block with 8 entries, 9 with 8 (72 slots: past one wave), 3 with 1"""
    import torch

    ladder = bc.LADDER8[:K] if K > 1 else [1.0]
    pk = _new(api, MID)
    d_src = torch.from_numpy(bc.batch_native(MID, B)).cuda()
    oracle = _composed(pk, d_src, ladder)
    pk.debug_set_budget_route(route)
    _held_to_the_oracle(pk, d_src, ladder, oracle, bc.derive_budgets(_table(oracle)), (B, K, ROUTE_NAMES[route]))
    pk.close()


def test_65536_slots_take_the_general_route(api):
    """8192 blocks of (1 x 2) with 8 entries: one slot more than the batched route takes, so the host picks the general one --
    and a forced batched route refuses the call"""
    import torch

    shape, B = bc.HADAMARD_SHAPES[0], 8192
    assert shape[1:4] == (4, 1, 2) and B * len(bc.LADDER8) == bc.MAX_SLOTS + 1 and not bc.batched(shape, B, 8) and bc.batched(shape, B, 7)
    x = np.frombuffer(cases._rand_native(1, 2 * B, 4, 4242, 3000).tobytes(), dtype=np.int32).reshape(B, 2).copy()
    x[1::4] = np.frombuffer(cases._rand_native(1, 2 * (B // 4), 4, 4243, (1 << 31) - 1).tobytes(), dtype=np.int32).reshape(-1, 2)  # full scale
    x[2::4] = (np.arange(B // 4, dtype=np.int32) * 7 + 5)[:, None]  # constant blocks
    d_src = torch.from_numpy(x.view(np.uint8).reshape(B, 8)).cuda()
    pk = _new(api, shape)
    oracle = _composed(pk, d_src, bc.LADDER8)
    table = _table(oracle)
    _held_to_the_oracle(pk, d_src, bc.LADDER8, oracle, bc.derive_budgets(table), "65536 slots, per block")
    _held_to_the_oracle(pk, d_src, bc.LADDER8, oracle, bc.scalar_budget(table), "65536 slots, one limit")
    pk.debug_set_budget_route(2)
    n = C.c_size_t()
    assert api.lib().rspt_hip_compress_budget_work_bytes(pk._h, B, 8, C.byref(n)) == ERR_UNSUPPORTED
    assert api.lib().rspt_hip_compress_budget_work_bytes(pk._h, B, 7, C.byref(n)) == 0
    with pytest.raises(api.RsptHipError):
        pk.compress_to_budget(d_src, 100, bc.LADDER8)
    _held_to_the_oracle(pk, d_src[:64], bc.LADDER8, [tuple(a[:64] for a in o) for o in oracle], bc.derive_budgets(table[:, :64]), "64 x 8, batched")
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_ladders_whose_sizes_are_unsorted_or_repeat(api, route):
    import torch

    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    d_src = torch.from_numpy(bc.batch_native(MID, NBLOCKS, ("rand", "walk"))).cuda()
    for ladder in (bc.UNSORTED_LADDER, bc.REPEATED_LADDER):
        oracle = _composed(pk, d_src, ladder)
        table = _table(oracle)
        budgets = bc.derive_budgets(table)
        choice = _held_to_the_oracle(pk, d_src, ladder, oracle, budgets, (ROUTE_NAMES[route], ladder))
        if ladder is bc.UNSORTED_LADDER:
            assert any(table[j, b] > budgets[b] for b in range(NBLOCKS) for j in range(int(choice[b])) if table[choice[b], b] <= budgets[b])
        else:
            assert np.array_equal(table[1], table[2]) and int(choice[1]) == 2 and 1 not in choice.tolist()
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_any_uint64_is_a_budget(api, route):
    import torch

    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    ladder = bc.ladder_of("hadamard")
    d_src = torch.from_numpy(bc.batch_native(MID, NBLOCKS)).cuda()
    oracle = _composed(pk, d_src, ladder)
    table = _table(oracle)
    c0 = _held_to_the_oracle(pk, d_src, ladder, oracle, 0, "0")
    assert c0.tolist() == [int(np.argmin(table[:, b])) for b in range(NBLOCKS)]  # (np.argmin: the lowest index among equals)
    cmax = _held_to_the_oracle(pk, d_src, ladder, oracle, bc.U64_MAX, "2^64 - 1")
    assert cmax.tolist() == [len(ladder) - 1] * NBLOCKS
    _held_to_the_oracle(pk, d_src, ladder, oracle, [bc.U64_MAX, 0, BIT63, BIT63 - 1, int(table[1, 4])], "per block, to either end")
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_the_handle_behind_budget_calls(api, route):
    """a plain compress_batch right behind a budget call writes what it wrote before it; budget calls of 5, 2 and 9 blocks, then
    compress_to_prdn and a ladder call on the same handle, each still at its oracle"""
    import torch

    ladder = bc.ladder_of("hadamard")
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    d_all = torch.from_numpy(bc.batch_native(MID, 9)).cuda()
    oracle = _composed(pk, d_all, ladder)
    fresh = _new(api, MID)  # never sees a budget call
    want_prdn = [t.cpu().numpy() for t in fresh.compress_to_prdn(d_all[:5], 2.0, ladder)]
    fresh.close()
    plain_before, sizes_before = [t.cpu().numpy() for t in pk.compress_batch(d_all)]

    def part(lo, hi):
        return [tuple(a[lo:hi] for a in o) for o in oracle]

    for lo, hi in ((0, 5), (5, 7), (0, 9)):
        _held_to_the_oracle(pk, d_all[lo:hi], ladder, part(lo, hi), bc.derive_budgets(_table(part(lo, hi))), (ROUTE_NAMES[route], lo, hi))
        if hi == 5:
            plain, sizes = [t.cpu().numpy() for t in pk.compress_batch(d_all)]
            assert np.array_equal(sizes, sizes_before)
            for b in range(9):
                assert np.array_equal(plain[b, : int(sizes[b])], plain_before[b, : int(sizes[b])]), b
    got = [t.cpu().numpy() for t in pk.compress_to_prdn(d_all[:5], 2.0, ladder)]
    assert np.array_equal(got[2], want_prdn[2]) and np.array_equal(got[1], want_prdn[1]) and np.array_equal(got[3].view(np.uint64), want_prdn[3].view(np.uint64))
    for b in range(5):
        assert np.array_equal(got[0][b, : int(got[1][b])], want_prdn[0][b, : int(got[1][b])]), b
    pick = [3, 0, 2, 1, 3, 2, 0, 1, 2]
    d_dst, d_sizes = pk.compress_batch(d_all, ladder=ladder, choice=torch.tensor(pick, dtype=torch.int32, device="cuda"))
    dst, sizes = d_dst.cpu().numpy(), d_sizes.cpu().numpy()
    for b, k in enumerate(pick):
        n = int(oracle[k][1][b])
        assert int(sizes[b]) == n and np.array_equal(dst[b, :n], oracle[k][0][b, :n]), (b, k)
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_a_chosen_stream_that_does_not_fit_the_stride_is_flagged_as_the_ladder_call_flags_it(api, route):
    import torch

    ladder = bc.ladder_of("hadamard")
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    d_src = torch.from_numpy(bc.batch_native(MID, NBLOCKS)).cuda()
    table = _table(_composed(pk, d_src, ladder))
    budgets = bc.derive_budgets(table)
    want = [bc.choose(table[:, b], budgets[b]) for b in range(NBLOCKS)]
    chosen = sorted(int(table[k, b]) for b, k in enumerate(want))
    stride = (chosen[2] + 15) // 16 * 16  # holds some of the chosen streams and not others: the stride plays no part in the choice
    assert chosen[0] <= stride < chosen[-1]
    d_dst = torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda")
    d_dst, d_sizes, d_choice = pk.compress_to_budget(d_src, torch.tensor(budgets, dtype=torch.int64, device="cuda"), ladder, d_dst=d_dst)
    l_dst = torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda")
    l_dst, l_sizes = pk.compress_batch(d_src, d_dst=l_dst, ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    assert d_choice.cpu().tolist() == want
    sizes = d_sizes.cpu().numpy().view(np.uint64)
    assert np.array_equal(sizes, l_sizes.cpu().numpy().view(np.uint64)) and np.array_equal(d_dst.cpu().numpy(), l_dst.cpu().numpy())
    for b, k in enumerate(want):
        n = int(table[k, b])
        assert int(sizes[b]) == (n if n <= stride else n | BIT63), b
        if n > stride:
            assert (d_dst[b] == 0xC3).all(), (b, "nothing is written")
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    n = C.c_size_t()

    def status(pk, ladder, nblocks=2, off=None, budget_tensor=False, cand=False):
        """the entry's status; off: {argument: bytes off its boundary}.  A refused call launches nothing: the buffers stay as they were"""
        off = off or {}
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        d_src = torch.zeros(nblocks * pk.block_bytes + 16, dtype=torch.uint8, device="cuda")
        d_dst = torch.full((nblocks, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks + 4,), -1, dtype=torch.int32, device="cuda")
        d_budget = torch.full((nblocks + 2,), 1000, dtype=torch.int64, device="cuda")
        d_cand = torch.full((8 * nblocks + 2,), -1, dtype=torch.int64, device="cuda")
        work = torch.full((1 << 12,), -1, dtype=torch.int64, device="cuda")
        rc = L.rspt_hip_compress_budget_batch_dev(
            pk._h, d_src.data_ptr() + off.get("src", 0), nblocks, lp, lad.size, 1000,
            d_budget.data_ptr() + off.get("budget", 0) if budget_tensor or "budget" in off else None, d_dst.data_ptr(), 4096, d_sizes.data_ptr(),
            d_choice.data_ptr() + off.get("choice", 0), d_cand.data_ptr() + off.get("cand", 0) if cand or "cand" in off else None,
            work.data_ptr() + off.get("work", 0), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all() and (d_cand == -1).all() and (work == -1).all()
        return rc

    had = _new(api, ("hadamard", 4, 3, 8, 3))
    assert status(had, [1.0, 4.0]) == 0 and status(had, [1.0, 4.0], budget_tensor=True, cand=True) == 0
    assert status(had, []) == ERR_ARG and status(had, [1.0] * 9) == ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):
        assert status(had, [1.0, bad]) == ERR_ARG, bad
    for arg, by in (("src", 8), ("work", 8), ("choice", 2), ("budget", 4), ("cand", 4)):
        assert status(had, [1.0, 4.0], off={arg: by}) == ERR_ARG, arg
    assert status(had, [1.0, 4.0], off={"choice": 4, "budget": 8, "cand": 8, "work": 16}, budget_tensor=True, cand=True) == 0  # (their own boundaries are enough)
    assert L.rspt_hip_compress_budget_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_work_bytes(had._h, 65536, 1, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_work_bytes(had._h, 2, 2, None) == ERR_ARG
    assert had.budget_work_bytes(3, 8) >= 3 * 8 * 8 and had.budget_work_bytes(3, 8) < 3 * 8 * 8 + 256  # the size table, and nothing else
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0]) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_budget_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        assert L.rspt_hip_debug_set_budget_route(pk._h, 2) == ERR_UNSUPPORTED
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert status(dense, [128.0, 0.0]) == ERR_ARG and status(dense, [128.0, 16.0]) == 0
    assert L.rspt_hip_debug_set_budget_route(dense._h, 2) == ERR_UNSUPPORTED and L.rspt_hip_debug_set_budget_route(dense._h, 3) == ERR_ARG
    dense.close()
    long_rows = _new(api, ("hadamard", 4, 2, 16384, 3))
    assert L.rspt_hip_debug_set_budget_route(long_rows._h, 2) == ERR_UNSUPPORTED and L.rspt_hip_debug_set_budget_route(long_rows._h, -1) == ERR_ARG
    long_rows.close()


def test_header_library_and_binding_agree(api):
    df.check_entries(
        ["int rspt_hip_compress_budget_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);",
         "int rspt_hip_debug_set_budget_route(rspt_hip_packer* p, int route);",
         "size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, "
         "uint64_t* d_cand_sizes, void* d_work, void* stream);"],
        ["rspt_hip_compress_budget_work_bytes", "rspt_hip_compress_budget_batch_dev", "rspt_hip_debug_set_budget_route"],
        methods=("budget_work_bytes", "debug_set_budget_route", "compress_to_budget"))
