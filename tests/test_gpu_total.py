"""Compress a batch to one byte total (rspt_hip_compress_total_batch_dev) against the composed oracle on the same device: per ladder
entry one plain rspt_hip_set_quantizer + compress_batch + decompress_batch + prdn_batch.  Its sizes, PRDN, mse and path go through
tests/total_cases.py's choose_total, and the totals are placed on those tables at run time (at the cost of a level, one byte below,
below the cost of +inf, 0, 2^64 - 1).  Held to the oracle, exactly (tests/total_dev.py): d_choice, d_level's bit pattern, d_total,
d_prdn, both tables, d_sizes, the stream bytes and the samples decoded with ladder= and choice=d_choice; and that the handle's
quantiser is what it was and nothing is written behind the work area.  Where the fused route runs, the general and the fused route
are forced in turn (rspt_hip_debug_set_total_route) and both held to the oracle, so to each other.  Around it: batches on either
side of a wave, of the level kernel's workgroup and of the 65535-slot bound, ladders that are unsorted or repeat, duplicated and
unrated blocks, the handle's state behind a total call, a stride the chosen stream does not fit, the refusals, the route offer."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import cases
import devframe as df
import lossy_dev as ld
import lossy_quantizer_cases as lq
import target_cases as tc
import total_cases as tt
import total_dev as td
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
NBLOCKS = 5
ROUTE_NAMES = {0: "auto", 1: "general", 2: "fused"}
MID = ("hadamard", 2, 5, 1024, 3)  # the shape of the tests that are not about a shape
TINY = ("hadamard", 4, 3, 8, 2)  # the shape of the batch-size tests: small, and its candidates still differ in size
FUSED_MAX_NS, FUSED_MAX_N, MAX_SLOTS = 8192, 1 << 22, 65535

# (kind, bps, nch, ns, nb): every tp_fwht tail (log2(ns) mod 3) and every launch width from 64 to 1024 threads
HADAMARD_SHAPES = [("hadamard", 4, 1, 2, 1), ("hadamard", 4, 2, 4, 2), ("hadamard", 1, 3, 8, 2), ("hadamard", 4, 2, 512, 3), ("hadamard", 2, 5, 1024, 3),
                   ("hadamard", 4, 2, 2048, 3), ("hadamard", 4, 3, 4096, 3),
                   ("hadamard", 4, 12, 8192, 3),   # the longest fused row
                   ("hadamard", 4, 9, 8192, 3),    # a ragged last hzr block
                   ("hadamard", 4, 2, 16384, 3), ("hadamard", 4, 2, 65536, 3)]  # general route only
DCT_SHAPES = [("dct", 3, 3, 100, 2), ("dct", 4, 2, 257, 3)]
SHAPES = HADAMARD_SHAPES + DCT_SHAPES


def fused(shape, nblocks=1, nladder=1):
    """the fused route runs this call"""
    return shape[0] == "hadamard" and shape[3] <= FUSED_MAX_NS and shape[2] * shape[3] < FUSED_MAX_N and nblocks * nladder <= MAX_SLOTS


def _new(api, shape):
    kind, bps, nch, ns, nb = shape
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _totals(oracle, n=8):
    return td.some_totals(oracle, n=n)


def _part(oracle, lo, hi):
    return [{k: v[lo:hi] for k, v in o.items()} for o in oracle]


@pytest.fixture(scope="module")
def runs(api):
    """per shape, once: a handle, 5 blocks -- random, walk, constant, full scale, random -- and the composed oracle of its ladder"""
    import torch

    memo = {}

    def get(shape):
        if shape not in memo:
            pk = _new(api, shape)
            d_src = torch.from_numpy(bc.batch_native(shape, NBLOCKS)).cuda()
            memo[shape] = (pk, d_src, ld.composed(pk, d_src, bc.ladder_of(shape[0]), prdn=True))
        return memo[shape]

    yield get
    for pk, _, _ in memo.values():
        pk.close()


SHAPE_RUNS = [(s, 0) for s in SHAPES] + [(s, r) for s in SHAPES if fused(s) for r in (1, 2)]


def test_the_fused_route_is_offered_where_the_header_says(api):
    """asked of rspt_hip_debug_set_total_route alone: no kernel runs"""
    L = api.lib()
    for s in SHAPES + [("hadamard", 4, 511, 8192, 3), ("hadamard", 4, 512, 8192, 3)]:
        pk = _new(api, s)
        assert L.rspt_hip_debug_set_total_route(pk._h, 2) == (0 if fused(s) else ERR_UNSUPPORTED), s
        assert L.rspt_hip_debug_set_total_route(pk._h, 1) == 0 and L.rspt_hip_debug_set_total_route(pk._h, 0) == 0
        assert L.rspt_hip_debug_set_total_route(pk._h, 3) == ERR_ARG and L.rspt_hip_debug_set_total_route(pk._h, -1) == ERR_ARG
        pk.close()
    assert [fused(s) for s in HADAMARD_SHAPES] == [True] * 9 + [False] * 2 and not any(fused(s) for s in DCT_SHAPES)
    assert fused(("hadamard", 4, 511, 8192, 3)) and not fused(("hadamard", 4, 512, 8192, 3))


@pytest.mark.parametrize("shape,route", SHAPE_RUNS, ids=["%s-%s" % (bc.shape_id(s), ROUTE_NAMES[r]) for s, r in SHAPE_RUNS])
def test_every_shape_against_the_composed_oracle(runs, shape, route):
    pk, d_src, oracle = runs(shape)
    ladder = bc.ladder_of(shape[0])
    pk.debug_set_total_route(route)
    totals = _totals(oracle)
    assert 6 <= len(totals) <= 10
    levels = set()
    for total in totals:
        levels.add(td.held_to_the_oracle(pk, d_src, ladder, oracle, total, (bc.shape_id(shape), ROUTE_NAMES[route], total))[0])
    assert len(levels) >= 2, levels
    pk.debug_set_total_route(0)


def _tiny_batch(B, seed=4242):
    """B blocks of TINY: calm, full scale, constant and calm again, in turn"""
    n = TINY[2] * TINY[3]
    x = np.frombuffer(cases._rand_native(1, n * B, 4, seed, 3000).tobytes(), dtype=np.int32).reshape(B, n).copy()
    x[1::4] = np.frombuffer(cases._rand_native(1, n * len(x[1::4]), 4, seed + 1, (1 << 31) - 1).tobytes(), dtype=np.int32).reshape(-1, n)
    x[2::4] = (np.arange(len(x[2::4]), dtype=np.int32) * 7 + 5)[:, None]
    return x.view(np.uint8).reshape(B, 4 * n)


@pytest.fixture(scope="module")
def tiny(api):
    """65535 tiny blocks and their composed oracle at LADDER8, once: the batch-size tests take its first B blocks"""
    import torch

    assert TINY[1] == 4
    pk = _new(api, TINY)
    d_src = torch.from_numpy(_tiny_batch(65535)).cuda()
    oracle = ld.composed(pk, d_src, bc.LADDER8, prdn=True)
    yield pk, d_src, oracle
    pk.close()


BATCH_RUNS = [(B, r) for B in (1, 255, 256, 257, 1025) for r in (1, 2)]


@pytest.mark.parametrize("B,route", BATCH_RUNS, ids=["%dx8-%s" % (B, ROUTE_NAMES[r]) for B, r in BATCH_RUNS])
def test_batch_sizes(tiny, B, route):
    """either side of a wave and of k_total_pick's workgroup, and past the 1024 blocks k_total_level keeps in registers (the tests
    of 8192, 13107 and 65535 blocks take k_total_round)"""
    pk, d_all, oracle = tiny
    pk.debug_set_total_route(route)
    part = _part(oracle, 0, B)
    for total in _totals(part, n=4):
        td.held_to_the_oracle(pk, d_all[:B], bc.LADDER8, part, total, (B, ROUTE_NAMES[route], total), second="brute" if B == 1 else "bisect" if B <= 257 else None)
    pk.debug_set_total_route(0)


def test_65535_slots_take_the_fused_route(tiny):
    pk, d_all, oracle = tiny
    B, K = 13107, 5
    assert B * K == MAX_SLOTS and fused(TINY, B, K)
    part = _part(oracle[:K], 0, B)
    pk.debug_set_total_route(2)
    for total in _totals(part, n=2):
        td.held_to_the_oracle(pk, d_all[:B], bc.LADDER8[:K], part, total, ("65535 slots", total), second=None)
    pk.debug_set_total_route(0)


def test_65536_slots_take_the_general_route(api, tiny):
    """8192 tiny blocks with 8 entries: one slot more than the fused route takes, so the host picks the general one -- and a forced
    fused route refuses the call"""
    pk, d_all, oracle = tiny
    B = 8192
    assert B * 8 == MAX_SLOTS + 1 and not fused(TINY, B, 8) and fused(TINY, B, 7)
    part = _part(oracle, 0, B)
    general = pk.total_work_bytes(B, 8)
    for total in _totals(part, n=2):
        td.held_to_the_oracle(pk, d_all[:B], bc.LADDER8, part, total, ("65536 slots", total), second=None)
    pk.debug_set_total_route(2)
    n = C.c_size_t()
    assert api.lib().rspt_hip_compress_total_work_bytes(pk._h, B, 8, C.byref(n)) == ERR_UNSUPPORTED
    assert api.lib().rspt_hip_compress_total_work_bytes(pk._h, B, 7, C.byref(n)) == 0 and n.value < general
    with pytest.raises(api.RsptHipError):
        pk.compress_to_total(d_all[:B], 100, bc.LADDER8)
    pk.debug_set_total_route(0)


def test_65535_blocks_with_8_entries_against_the_vectorised_rule(tiny):
    pk, d_all, oracle = tiny
    sizes, prdn, mse, path = td.tables_of(oracle)
    at_inf = tt.choose_total_np(sizes, prdn, mse, path, 0)
    lowest = tt.choose_total_np(sizes, prdn, mse, path, tt.U64_MAX)
    assert at_inf[0] == tt.INF and lowest[0] < tt.INF and lowest[2] > at_inf[2]
    seen = set()
    for total in (tt.U64_MAX, (at_inf[2] + lowest[2]) // 2, at_inf[2], at_inf[2] - 1):
        seen.add(td.held_to_the_oracle(pk, d_all, bc.LADDER8, oracle, total, ("65535 x 8", total), second=None)[0])
    assert len(seen) == 4


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_ladders_that_are_unsorted_or_repeat_and_duplicated_blocks(api, route):
    import torch

    pk = _new(api, MID)
    pk.debug_set_total_route(route)
    x = bc.batch_native(MID, 6, ("rand", "walk"))
    x[2] = x[0]  # equal figures in two blocks: one level moves two picks
    d_src = torch.from_numpy(x).cuda()
    for ladder in (bc.HADAMARD_LADDER, bc.UNSORTED_LADDER, bc.REPEATED_LADDER):
        oracle = ld.composed(pk, d_src, ladder, prdn=True)
        sizes, prdn, mse, path = td.tables_of(oracle)
        assert np.array_equal(sizes[:, 0], sizes[:, 2]) and np.array_equal(prdn[:, 0].view(np.uint64), prdn[:, 2].view(np.uint64))
        picked = set()
        for total in _totals(oracle):
            level, choice, cost = td.held_to_the_oracle(pk, d_src, ladder, oracle, total, (ROUTE_NAMES[route], ladder, total))
            assert choice[0] == choice[2]
            picked |= set(choice.tolist())
            if ladder is bc.HADAMARD_LADDER and 0 < level < tt.INF:
                # the identity of the header: sizes ascend and figures descend strictly, so the choice is the target entry's at T*
                assert np.all(np.diff(sizes, axis=0) > 0) and np.all(np.diff(prdn, axis=0) < 0)
                t_choice = ld.rate_call(pk, "target", d_src, level, ladder, (ladder, total, "target"))["choice"]
                for b in range(6):
                    if any(tc.meets(prdn[k, b], mse[k, b], path[k, b], level) for k in range(4)):
                        assert int(t_choice[b]) == int(choice[b]), (total, b)
        if ladder is bc.REPEATED_LADDER:
            assert np.array_equal(sizes[1], sizes[2]) and 1 in picked and 2 not in picked  # equal size and figure: the lowest index
        else:
            assert picked == {0, 1, 2, 3}
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_unrated_blocks_take_their_smallest_stream_and_their_figures_never_count(api, route):
    """full-scale samples at nb = 1: every entry of blocks 0 and 2 has path 1"""
    import torch

    shape, ladder = ("hadamard", 4, 2, 64, 1), [1.0 / 4, 1.0, 64.0]
    pk = _new(api, shape)
    pk.debug_set_total_route(route)
    d_src = torch.from_numpy(bc.batch_native(shape, 3, ("full", "rand", "full"))).cuda()
    oracle = ld.composed(pk, d_src, ladder, prdn=True)
    sizes, prdn, mse, path = td.tables_of(oracle)
    assert (path[:, [0, 2]] == 1).all() and (path[:, 1] == 0).all()
    for total in _totals(oracle):
        level, choice, cost = td.held_to_the_oracle(pk, d_src, ladder, oracle, total, (ROUTE_NAMES[route], total))
        assert all(int(choice[b]) == int(np.argmin(sizes[:, b])) for b in (0, 2))
    both = torch.cat([d_src[0:1], d_src[2:3]])  # no rated block at all: the level is +0.0 whatever the total
    part = [{k: np.concatenate([v[0:1], v[2:3]]) for k, v in o.items()} for o in oracle]
    for total in (0, tt.U64_MAX):
        level, choice, cost = td.held_to_the_oracle(pk, both, ladder, part, total, (ROUTE_NAMES[route], "unrated alone", total))
        assert tt.bits(level) == 0 and cost > 0
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_the_handle_behind_total_calls(api, route):
    """plain, ladder, target and budget calls right behind a total call write what they wrote before it; total calls of 5, 2 and 9
    blocks in between, each at its oracle"""
    import torch

    ladder = bc.ladder_of("hadamard")
    pk = _new(api, MID)
    pk.debug_set_total_route(route)
    d_all = torch.from_numpy(bc.batch_native(MID, 9)).cuda()
    oracle = ld.composed(pk, d_all, ladder, prdn=True)
    pick = torch.tensor([3, 0, 2, 1, 3, 2, 0, 1, 2], dtype=torch.int32, device="cuda")

    def others():
        """(name, arrays, valid lengths per block or None) of a plain, a ladder, a target and a budget call"""
        out = []
        d_dst, d_sizes = pk.compress_batch(d_all)
        out.append(("plain", [d_dst.cpu().numpy()], d_sizes.cpu().numpy()))
        d_dst, d_sizes = pk.compress_batch(d_all, ladder=ladder, choice=pick)
        out.append(("ladder", [d_dst.cpu().numpy()], d_sizes.cpu().numpy()))
        d_dst, d_sizes, d_choice, d_prdn = pk.compress_to_prdn(d_all[:5], 2.0, ladder)
        out.append(("target", [d_dst.cpu().numpy(), d_choice.cpu().numpy(), d_prdn.cpu().numpy().view(np.uint64)], d_sizes.cpu().numpy()))
        d_dst, d_sizes, d_choice = pk.compress_to_budget(d_all, 6000, ladder)
        out.append(("budget", [d_dst.cpu().numpy(), d_choice.cpu().numpy()], d_sizes.cpu().numpy()))
        return out

    def same(a, b, tag):
        for (name, xs, n), (_, ys, m) in zip(a, b):
            assert np.array_equal(n, m), (tag, name, "sizes")
            cols = np.arange(xs[0].shape[1])[None, :]
            assert ((xs[0] == ys[0]) | (cols >= n[:, None])).all(), (tag, name, "streams")
            for x, y in zip(xs[1:], ys[1:]):
                assert np.array_equal(x, y), (tag, name)

    before = others()
    for lo, hi in ((0, 5), (5, 7), (0, 9)):
        part = _part(oracle, lo, hi)
        totals = _totals(part, n=3)
        td.held_to_the_oracle(pk, d_all[lo:hi], ladder, part, totals[len(totals) // 2], (ROUTE_NAMES[route], lo, hi))
        same(before, others(), (ROUTE_NAMES[route], lo, hi))
        td.held_to_the_oracle(pk, d_all[lo:hi], ladder, part, totals[-2], (ROUTE_NAMES[route], lo, hi, "behind the others"))
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_a_chosen_stream_that_does_not_fit_the_stride_is_flagged_as_the_ladder_call_flags_it(api, route):
    import torch

    ladder = bc.ladder_of("hadamard")
    pk = _new(api, MID)
    pk.debug_set_total_route(route)
    d_src = torch.from_numpy(bc.batch_native(MID, NBLOCKS)).cuda()
    oracle = ld.composed(pk, d_src, ladder, prdn=True)
    sizes = td.tables_of(oracle)[0]
    totals = _totals(oracle)
    total = totals[len(totals) // 2]
    level, want, cost = tt.choose_total(*td.as_lists(*td.tables_of(oracle)), total)
    chosen = sorted(int(sizes[k, b]) for b, k in enumerate(want))
    stride = (chosen[2] + 15) // 16 * 16  # holds some of the chosen streams and not others: the stride plays no part in the rule
    assert chosen[0] <= stride < chosen[-1]
    d_dst = torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda")
    got = ld.rate_call(pk, "total", d_src, total, ladder, "stride", d_dst=d_dst)
    l_dst = torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda")
    l_dst, l_sizes = pk.compress_batch(d_src, d_dst=l_dst, ladder=ladder, choice=torch.from_numpy(got["choice"]).cuda())
    torch.cuda.synchronize()
    assert got["choice"].tolist() == want and got["level"] == tt.bits(level) and got["total"] == cost
    out = got["sizes"].view(np.uint64)
    assert np.array_equal(out, l_sizes.cpu().numpy().view(np.uint64)) and np.array_equal(got["dst"], l_dst.cpu().numpy())
    for b, k in enumerate(want):
        n = int(sizes[k, b])
        assert int(out[b]) == (n if n <= stride else n | BIT63), b
        if n > stride:
            assert (got["dst"][b] == 0xC3).all(), (b, "nothing is written")
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    n = C.c_size_t()
    OPTIONAL = ("level", "total", "prdn", "cand", "figs")

    def status(pk, ladder, nblocks=2, off=None, optional=False, stride=4096, says=None):
        """the entry's status; off: {argument: bytes off its boundary}; says: the block count the call names, where it is not that
        of the buffers.  A refused call launches nothing: the buffers stay as they were"""
        off = off or {}
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        d_src = torch.zeros(nblocks * pk.block_bytes + 16, dtype=torch.uint8, device="cuda")
        d_dst = torch.full((nblocks, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks + 4,), -1, dtype=torch.int32, device="cuda")
        opt = {name: torch.full((8 * nblocks + 2,), -1, dtype=torch.int64, device="cuda") for name in OPTIONAL}
        work = torch.full((1 << 13,), -1, dtype=torch.int64, device="cuda")
        ptr = [opt[name].data_ptr() + off.get(name, 0) if optional or name in off else None for name in OPTIONAL]
        rc = L.rspt_hip_compress_total_batch_dev(pk._h, d_src.data_ptr() + off.get("src", 0), says or nblocks, lp, lad.size, 1000, d_dst.data_ptr(), stride,
                                                 d_sizes.data_ptr(), d_choice.data_ptr() + off.get("choice", 0), *ptr, work.data_ptr() + off.get("work", 0), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all() and (work == -1).all()
            assert all((t == -1).all() for t in opt.values())
        return rc

    had = _new(api, ("hadamard", 4, 3, 8, 3))
    assert status(had, [1.0, 4.0]) == 0 and status(had, [1.0, 4.0], optional=True) == 0
    assert status(had, []) == ERR_ARG and status(had, [1.0] * 9) == ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):
        assert status(had, [1.0, bad]) == ERR_ARG, bad
    for arg, by in (("src", 8), ("work", 8), ("choice", 2)) + tuple((name, 4) for name in OPTIONAL):
        assert status(had, [1.0, 4.0], off={arg: by}) == ERR_ARG, arg
    assert status(had, [1.0, 4.0], off=dict({name: 8 for name in OPTIONAL}, choice=4, work=16)) == 0  # (their own boundaries are enough)
    assert status(had, [1.0, 4.0], stride=1 << 32) == ERR_ARG  # (2^32 bytes per 65536 samples of a block)
    assert status(had, [1.0, 4.0], says=65536) == ERR_ARG
    assert L.rspt_hip_compress_total_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_work_bytes(had._h, 65536, 1, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_work_bytes(had._h, 2, 2, None) == ERR_ARG
    fused_bytes = had.total_work_bytes(3, 8)
    assert 3 * 8 * 72 + 1280 <= fused_bytes < 3 * 8 * 72 + 1280 + 8 * 256  # tables alone: 72 bytes per (entry, block); the result and the rounds' sums
    had.debug_set_total_route(1)
    assert had.total_work_bytes(3, 8) == 2 * 256 + 1280 + had.target_work_bytes(3, 8)  # the size table, the figures, the result; the target entry's area
    had.debug_set_total_route(0)
    assert status(had, [1.0, 4.0], nblocks=1) == 0
    had.feed_begin(1, 2)
    assert status(had, [1.0, 4.0]) == ERR_ARG  # an open feed owns the workspace
    had.feed_end()
    assert status(had, [1.0, 4.0]) == 0
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0]) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_total_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        assert L.rspt_hip_debug_set_total_route(pk._h, 2) == ERR_UNSUPPORTED
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert status(dense, [128.0, 0.0]) == ERR_ARG and status(dense, [128.0, 16.0]) == 0
    assert L.rspt_hip_debug_set_total_route(dense._h, 2) == ERR_UNSUPPORTED and L.rspt_hip_debug_set_total_route(dense._h, 3) == ERR_ARG
    dense.close()


def test_header_library_and_binding_agree(api):
    df.check_entries(
        ["int rspt_hip_compress_total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);",
         "int rspt_hip_debug_set_total_route(rspt_hip_packer* p, int route);",
         "size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level, uint64_t* d_total, "
         "double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream);"],
        ["rspt_hip_compress_total_work_bytes", "rspt_hip_compress_total_batch_dev", "rspt_hip_debug_set_total_route"],
        methods=("total_work_bytes", "debug_set_total_route", "compress_to_total"))
