"""Compress to a byte budget from the planar int32 matrix (rspt_hip_compress_budget_planar_batch_dev) on the matrices of
tests/budget_planar_cases.py, against two oracles that never involve the code under test:
(a) the native entry on from_planar_i32(P) on the same device -- rspt_hip_compress_budget_batch_dev, which tests/test_gpu_budget.py
    holds to the composed oracle: d_choice, d_sizes, the whole table of candidate sizes, the streams byte for byte, and the decode;
(b) the choices of budget_cases.restated for the rule cases.
The budgets are placed at run time on the oracle's own table: derive_budgets per block, scalar_budget as the call's one limit.
Every shape runs on the host's own route, the batched shapes on each route forced as well; the shapes below four bytes a sample also
with garbage above the sample width, with the same results; every matrix also from a base 4 bytes past a 16-byte boundary.  Around
it: a NaN guard band behind the work area, the matrix only read, the decode through the planar ladder decoder and through a
container, the batch shapes on either side of a wave and of the 65535-slot bound, any uint64 as a budget, the handle behind the
call, a stride the chosen stream does not fit, the refusals."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import budget_planar_cases as bp
import cases
import devframe as df
import lossy_dev as ld
import lossy_quantizer_cases as lq
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
ROUTE_NAMES = {0: "auto", 1: "general", 2: "batched"}
MID = ("hadamard", 2, 5, 1024, 3)  # the shape of the tests that are not about a shape


def _new(api, shape):
    kind, bps, nch, ns, nb = shape
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _native(pk, d_native, ladder, budget, shape, tag):
    """oracle (a): the native entry on the native blocks -> dict(choice, sizes, dst, cand, decoded) on the host, decoded as the
    planar matrix of the native decode.  A U64_MAX budget gives the table alone."""
    limits, choice, sizes, dst, out, cand = map(ld.rate_call(pk, "budget", d_native, budget, ladder, (tag, "native oracle")).get, ld.BUDGET_FIELDS)
    assert not (sizes.view(np.uint64) & np.uint64(BIT63)).any(), tag
    return dict(choice=choice, sizes=sizes, dst=dst, cand=cand, decoded=bp.to_matrix(out, shape), limits=limits)


def _equals(res, o, tag):
    """d_choice, d_sizes (bit 63 included), the table and the streams of a planar call against oracle (a)"""
    d_dst, d_sizes, d_choice, d_cand = res
    choice, sizes, dst, cand = d_choice.cpu().numpy(), d_sizes.cpu().numpy(), d_dst.cpu().numpy(), d_cand.cpu().numpy()
    assert np.array_equal(cand, o["cand"]), (tag, "the table of candidate sizes")
    assert np.array_equal(choice, o["choice"]), (tag, choice.tolist(), o["choice"].tolist())
    assert np.array_equal(sizes.view(np.uint64), o["sizes"].view(np.uint64)), (tag, sizes.tolist(), o["sizes"].tolist())
    for b in range(len(sizes)):
        n = int(o["sizes"][b])
        assert np.array_equal(dst[b, :n], o["dst"][b, :n]), (tag, b, "stream")


def _held(pk, P, off, ladder, budget, o, tag):
    """P from a base `off` bytes past a 16-byte boundary through one planar call, held to oracle (a); the matrix and its guards
    are untouched afterwards -> the call's device tensors"""
    sraw, src = df.guarded_matrix(P, off)
    res = ld.rate_call(pk, "budget", src, budget, ladder, tag, planar=True)["dev"]
    _equals(res, o, tag)
    assert np.array_equal(src.cpu().numpy(), P) and df.guards_untouched(sraw, off, P.size * 4), (tag, "d_planar is only read")
    return res


@pytest.fixture(scope="module")
def oracle(api):
    """per shape, once, on a handle of its own: oracle (a) for the per-block budgets and for the one limit, both placed on its table"""
    memo = {}

    def get(shape):
        import torch

        if shape not in memo:
            ladder = bc.ladder_of(shape[0])
            pk = _new(api, shape)
            d_native = pk.from_planar_i32(torch.from_numpy(bp.matrix(shape).copy()).cuda())
            assert np.array_equal(d_native.cpu().numpy(), bc.batch_native(shape, bp.NBLOCKS))
            table = _native(pk, d_native, ladder, bc.U64_MAX, shape, shape)["cand"]
            assert table.min() > 0
            memo[shape] = {"per block": _native(pk, d_native, ladder, bc.derive_budgets(table), shape, shape),
                           "one limit": _native(pk, d_native, ladder, bc.scalar_budget(table), shape, shape)}
            pk.close()
        return memo[shape]

    return get


SHAPE_RUNS = [(s, 0) for s in bp.SHAPES] + [(s, r) for s in bp.SHAPES if bc.batched(s) for r in (1, 2)]


@pytest.mark.parametrize("shape,route", SHAPE_RUNS, ids=["%s-%s" % (bc.shape_id(s), ROUTE_NAMES[r]) for s, r in SHAPE_RUNS])
def test_budget_planar_is_the_native_entry_on_the_converted_matrix(api, oracle, shape, route):
    ladder = bc.ladder_of(shape[0])
    pk = _new(api, shape)
    assert api.lib().rspt_hip_debug_set_budget_route(pk._h, 2) == (0 if bc.batched(shape) else ERR_UNSUPPORTED)
    pk.debug_set_budget_route(route)
    for kind, o in oracle(shape).items():
        budget = o["limits"] if kind == "per block" else o["limits"][0]
        for vtag, garbage in bp.variants(shape):
            for off in bp.OFFSETS:
                _held(pk, bp.matrix(shape, garbage), off, ladder, budget, o, (bc.shape_id(shape), ROUTE_NAMES[route], kind, vtag, off))
    pk.close()


@pytest.mark.parametrize("shape", bp.SHAPES, ids=[bc.shape_id(s) for s in bp.SHAPES])
def test_the_streams_decode_and_travel_in_a_container(api, oracle, shape):
    """decompress_planar_batch(ladder=, choice=d_choice) gives to_planar_i32 of the native decode and consumes d_sizes; and
    compress_to_budget_planar -> pack_batch(choice=, nladder=) -> decompress_packed_planar(ladder=) gives the same matrix"""
    import torch

    ladder = bc.ladder_of(shape[0])
    o = oracle(shape)["per block"]
    pk = _new(api, shape)
    garbage = bp.variants(shape)[-1][1]
    d_dst, d_sizes, d_choice, _ = _held(pk, bp.matrix(shape, garbage), 4, ladder, o["limits"], o, (bc.shape_id(shape), "decode"))
    d_out, d_used = pk.decompress_planar_batch(d_dst, bp.NBLOCKS, d_dst.shape[1], ladder=ladder, choice=d_choice)
    d_packed, d_total = pk.pack_batch(d_dst, d_sizes, choice=d_choice, nladder=len(ladder))
    torch.cuda.synchronize()
    assert np.array_equal(d_used.cpu().numpy(), o["sizes"])
    assert np.array_equal(d_out.cpu().numpy(), o["decoded"])
    d_back, d_used2 = pk.decompress_packed_planar(d_packed[: int(d_total.item())].clone(), ladder=ladder)
    torch.cuda.synchronize()
    assert np.array_equal(d_used2.cpu().numpy(), o["sizes"])
    assert np.array_equal(d_back.cpu().numpy(), o["decoded"])
    assert ld.last_hip_error(pk) == 0
    pk.close()


RULE_CASES = {c["name"]: c for c in bc.rule_cases()}


@pytest.mark.parametrize("name", list(RULE_CASES))
def test_rule_cases(api, name):
    """oracle (b): the choices of the CPU restatement, which oracle (a) must agree with, on every route the shape takes"""
    import torch

    c = RULE_CASES[name]
    natives, table, budgets, choices = bc.restated(c)
    P = bp.rule_matrix(c)
    ora = _new(api, c["shape"])
    o = _native(ora, ora.from_planar_i32(torch.from_numpy(P.copy()).cuda()), c["ladder"], budgets, c["shape"], name)
    ora.close()
    assert o["choice"].tolist() == choices and np.array_equal(o["cand"], table), (name, "the two oracles")
    pk = _new(api, c["shape"])
    for route in (0, 1, 2) if bc.batched(c["shape"]) else (0,):
        pk.debug_set_budget_route(route)
        res = _held(pk, P, 4, c["ladder"], budgets, o, (name, ROUTE_NAMES[route]))
        assert res[2].cpu().tolist() == choices, (name, ROUTE_NAMES[route])
    pk.close()


def _mid_matrix(B, contents=bc.CONTENTS, seed=4100):
    """(clean, garbage) matrices of B blocks of MID"""
    P = bp.to_matrix(bc.batch_native(MID, B, contents), MID)
    return P, bp.with_garbage(P, MID[1], seed + B)


def _mid_oracle(api, P, ladder, budget=None, slices=None):
    """oracle (a) on a handle of its own; budget None: derive_budgets on its table.  slices: one oracle per (lo, hi)"""
    import torch

    pk = _new(api, MID)
    d_native = pk.from_planar_i32(torch.from_numpy(np.ascontiguousarray(P)).cuda())
    out = []
    for lo, hi in slices or [(0, P.shape[0])]:
        d = d_native[lo:hi]
        lim = budget if budget is not None else bc.derive_budgets(_native(pk, d, ladder, bc.U64_MAX, MID, "table")["cand"])
        out.append(_native(pk, d, ladder, lim, MID, (lo, hi)))
    pk.close()
    return out if slices else out[0]


BATCH_RUNS = [(B, K, r) for B, K in ((1, 8), (9, 8), (3, 1)) for r in (0, 1, 2)]


@pytest.mark.parametrize("B,K,route", BATCH_RUNS, ids=["%dx%d-%s" % (B, K, ROUTE_NAMES[r]) for B, K, r in BATCH_RUNS])
def test_batch_shapes(api, B, K, route):
    """1 block with 8 entries, 9 with 8 (72 slots: past one wave), 3 with 1"""
    ladder = bc.LADDER8[:K] if K > 1 else [1.0]
    clean, dirty = _mid_matrix(B)
    o = _mid_oracle(api, clean, ladder)
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    _held(pk, clean, 0, ladder, o["limits"], o, (B, K, ROUTE_NAMES[route], "clean"))
    _held(pk, dirty, 4, ladder, o["limits"], o, (B, K, ROUTE_NAMES[route], "garbage"))
    pk.close()


def test_65536_slots_take_the_general_route(api):
    """8192 blocks of (1 x 2) with 8 entries: one slot more than the batched route takes, so the host picks the general one -- and
    a forced batched route is refused by both new entries; 7 entries are accepted"""
    import torch

    shape, B = bc.HADAMARD_SHAPES[0], 8192
    assert shape[1:4] == (4, 1, 2) and B * len(bc.LADDER8) == bc.MAX_SLOTS + 1 and not bc.batched(shape, B, 8) and bc.batched(shape, B, 7)
    x = np.frombuffer(cases._rand_native(1, 2 * B, 4, 4242, 3000).tobytes(), dtype=np.int32).reshape(B, 1, 2).copy()
    x[1::4] = np.frombuffer(cases._rand_native(1, 2 * (B // 4), 4, 4243, (1 << 31) - 1).tobytes(), dtype=np.int32).reshape(-1, 1, 2)  # full scale
    x[2::4] = (np.arange(B // 4, dtype=np.int32) * 7 + 5)[:, None, None]  # constant blocks
    ora = _new(api, shape)
    d_native = ora.from_planar_i32(torch.from_numpy(x).cuda())
    table = _native(ora, d_native, bc.LADDER8, bc.U64_MAX, shape, "table")["cand"]
    o8 = _native(ora, d_native, bc.LADDER8, bc.derive_budgets(table), shape, "65536 slots")
    o7 = _native(ora, d_native, bc.LADDER8[:7], bc.scalar_budget(table[:7]), shape, "57344 slots")
    ora.close()
    pk = _new(api, shape)
    _held(pk, x, 4, bc.LADDER8, o8["limits"], o8, "65536 slots, the host's route")
    pk.debug_set_budget_route(2)
    n = C.c_size_t()
    assert api.lib().rspt_hip_compress_budget_planar_work_bytes(pk._h, B, 8, C.byref(n)) == ERR_UNSUPPORTED
    assert api.lib().rspt_hip_compress_budget_planar_work_bytes(pk._h, B, 7, C.byref(n)) == 0 and n.value == pk.budget_work_bytes(B, 7)
    d_x = torch.from_numpy(x).cuda()
    work = torch.zeros(8 * B, dtype=torch.float64, device="cuda")
    with pytest.raises(api.RsptHipError):
        pk.compress_to_budget_planar(d_x, 100, bc.LADDER8, work=work)
    torch.cuda.synchronize()
    assert int(work.count_nonzero()) == 0
    _held(pk, x, 0, bc.LADDER8[:7], o7["limits"][0], o7, "57344 slots, batched")
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_any_uint64_is_a_budget(api, route):
    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(5)
    table = _mid_oracle(api, clean, ladder, bc.U64_MAX)["cand"]
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    for budget in (0, bc.U64_MAX, [bc.U64_MAX, 0, BIT63, BIT63 - 1, int(table[1, 4])]):
        o = _mid_oracle(api, clean, ladder, budget)
        want = [bc.choose(table[:, b], o["limits"][b]) for b in range(5)]
        assert o["choice"].tolist() == want
        res = _held(pk, dirty, 4, ladder, budget, o, (ROUTE_NAMES[route], budget))
        assert res[2].cpu().tolist() == want
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_the_handle_behind_budget_calls(api, route):
    """a plain compress_planar_batch and a plain compress_batch right behind a planar budget call write what they wrote before it;
    native and planar budget calls alternating on one handle with batches of 5, 2 and 9 blocks, each still at its oracle; then
    compress_to_prdn_planar gives what a fresh handle gives"""
    import torch

    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(9)
    slices = ((0, 5), (5, 7), (0, 9))
    oracles = _mid_oracle(api, clean, ladder, slices=slices)
    d_clean, d_dirty = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    fresh = _new(api, MID)  # never sees a budget call
    want_prdn = [t.cpu().numpy() for t in fresh.compress_to_prdn_planar(d_dirty[:5], 2.0, ladder)]
    fresh.close()
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    d_native = pk.from_planar_i32(d_clean)

    def plain():
        a = [t.cpu().numpy() for t in pk.compress_planar_batch(d_dirty)]
        b = [t.cpu().numpy() for t in pk.compress_batch(d_native)]
        return a, b

    before = plain()
    for (lo, hi), o in zip(slices, oracles):
        tag = (ROUTE_NAMES[route], lo, hi)
        _held(pk, dirty[lo:hi], 4, ladder, o["limits"], o, tag + ("planar",))
        if hi == 5:
            for (dst, sizes), (dst0, sizes0) in zip(plain(), before):
                assert np.array_equal(sizes, sizes0)
                for b in range(9):
                    assert np.array_equal(dst[b, : int(sizes[b])], dst0[b, : int(sizes[b])]), (tag, b)
        limits, choice, sizes, dst, out, cand = map(ld.rate_call(pk, "budget", d_native[lo:hi], o["limits"], ladder, tag + ("native",)).get, ld.BUDGET_FIELDS)
        assert np.array_equal(choice, o["choice"]) and np.array_equal(sizes, o["sizes"]) and np.array_equal(cand, o["cand"]), tag
        for b in range(hi - lo):
            assert np.array_equal(dst[b, : int(sizes[b])], o["dst"][b, : int(sizes[b])]), (tag, b)
        _held(pk, clean[lo:hi], 0, ladder, o["limits"], o, tag + ("planar again",))
    got = [t.cpu().numpy() for t in pk.compress_to_prdn_planar(d_dirty[:5], 2.0, ladder)]
    assert np.array_equal(got[2], want_prdn[2]) and np.array_equal(got[1], want_prdn[1]) and np.array_equal(got[3].view(np.uint64), want_prdn[3].view(np.uint64))
    for b in range(5):
        assert np.array_equal(got[0][b, : int(got[1][b])], want_prdn[0][b, : int(got[1][b])]), b
    assert ld.last_hip_error(pk) == 0
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "batched"])
def test_a_chosen_stream_that_does_not_fit_the_stride_is_flagged_as_the_planar_ladder_call_flags_it(api, route):
    import torch

    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(5)
    o = _mid_oracle(api, clean, ladder)
    table, budgets, want = o["cand"], o["limits"], o["choice"].tolist()
    chosen = sorted(int(table[k, b]) for b, k in enumerate(want))
    stride = (chosen[2] + 15) // 16 * 16  # holds some of the chosen streams and not others: the stride plays no part in the choice
    assert chosen[0] <= stride < chosen[-1]
    pk = _new(api, MID)
    pk.debug_set_budget_route(route)
    sraw, src = df.guarded_matrix(dirty, 4)
    d_dst = torch.full((5, stride), 0xC3, dtype=torch.uint8, device="cuda")
    d_dst, d_sizes, d_choice, d_cand = ld.rate_call(pk, "budget", src, budgets, ladder, ROUTE_NAMES[route], planar=True, d_dst=d_dst)["dev"]
    l_dst = torch.full((5, stride), 0xC3, dtype=torch.uint8, device="cuda")
    l_dst, l_sizes = pk.compress_planar_batch(src, d_dst=l_dst, ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    assert d_choice.cpu().tolist() == want and np.array_equal(d_cand.cpu().numpy(), table)
    sizes = d_sizes.cpu().numpy().view(np.uint64)
    assert np.array_equal(sizes, l_sizes.cpu().numpy().view(np.uint64)) and np.array_equal(d_dst.cpu().numpy(), l_dst.cpu().numpy())
    dst = d_dst.cpu().numpy()
    for b, k in enumerate(want):
        n = int(table[k, b])
        assert int(sizes[b]) == (n if n <= stride else n | BIT63), b
        if n > stride:
            assert (dst[b] == 0xC3).all(), (b, "nothing is written")
        else:
            assert np.array_equal(dst[b, :n], o["dst"][b, :n]), b
    assert np.array_equal(src.cpu().numpy(), dirty) and df.guards_untouched(sraw, 4, dirty.size * 4)
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    n = C.c_size_t()

    def status(pk, ladder, nblocks=2, off=None, budget_tensor=False, cand=False, feed=False):
        """the entry's status; off: {argument: bytes off its boundary}.  A refused call launches nothing: the buffers stay as they were"""
        off = off or {}
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        nsamp = getattr(pk, "nch", 1) * getattr(pk, "ns", 64)
        d_planar = torch.zeros(nblocks * nsamp + 4, dtype=torch.int32, device="cuda")
        d_dst = torch.full((nblocks, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks + 4,), -1, dtype=torch.int32, device="cuda")
        d_budget = torch.full((nblocks + 2,), 1000, dtype=torch.int64, device="cuda")
        d_cand = torch.full((8 * nblocks + 2,), -1, dtype=torch.int64, device="cuda")
        work = torch.full((1 << 12,), -1, dtype=torch.int64, device="cuda")
        rc = L.rspt_hip_compress_budget_planar_batch_dev(
            pk._h, d_planar.data_ptr() + off.get("planar", 0) if "null" not in off else None, nblocks, lp, lad.size, 1000,
            d_budget.data_ptr() + off.get("budget", 0) if budget_tensor or "budget" in off else None, d_dst.data_ptr(), off.get("stride", 4096),
            d_sizes.data_ptr(), d_choice.data_ptr() + off.get("choice", 0), d_cand.data_ptr() + off.get("cand", 0) if cand or "cand" in off else None,
            work.data_ptr() + off.get("work", 0), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all() and (d_cand == -1).all() and (work == -1).all()
            assert (d_planar == 0).all()
        return rc

    had = _new(api, ("hadamard", 4, 3, 8, 3))
    assert status(had, [1.0, 4.0]) == 0 and status(had, [1.0, 4.0], budget_tensor=True, cand=True) == 0
    assert status(had, [1.0, 4.0], off={"planar": 4}) == 0 and status(had, [1.0, 4.0], off={"planar": 12}) == 0  # any 4-byte alignment of the matrix
    assert status(had, []) == ERR_ARG and status(had, [1.0] * 9) == ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):
        assert status(had, [1.0, bad]) == ERR_ARG, bad
    for by in (1, 2, 3):
        assert status(had, [1.0, 4.0], off={"planar": by}) == ERR_ARG, by
    for arg, by in (("work", 8), ("choice", 2), ("budget", 4), ("cand", 4)):
        assert status(had, [1.0, 4.0], off={arg: by}) == ERR_ARG, arg
    assert status(had, [1.0, 4.0], off={"planar": 4, "choice": 4, "budget": 8, "cand": 8, "work": 16}, budget_tensor=True, cand=True) == 0  # (their own boundaries are enough)
    assert status(had, [1.0, 4.0], off={"null": 1}) == ERR_ARG and status(had, [1.0, 4.0], nblocks=0) == ERR_ARG
    assert status(had, [1.0, 4.0], off={"stride": 1 << 32}) == ERR_ARG  # (one hzr block per plane: 2^32 bytes of stride per block and more)
    # (65536 blocks are refused before any pointer is looked at: aligned numbers stand in for the buffers)
    assert L.rspt_hip_compress_budget_planar_batch_dev(had._h, 16, 65536, None, 1, 0, None, 16, 4096, 16, 16, None, 16, None) == ERR_ARG
    assert L.rspt_hip_compress_budget_planar_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_planar_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_planar_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_planar_work_bytes(had._h, 65536, 1, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_budget_planar_work_bytes(had._h, 2, 2, None) == ERR_ARG
    assert had.budget_planar_work_bytes(3, 8) == had.budget_work_bytes(3, 8) and 3 * 8 * 8 <= had.budget_planar_work_bytes(3, 8) < 3 * 8 * 8 + 256
    # an open feed owns the workspace
    assert L.rspt_hip_feed_begin(had._h, 2, 2) == 0
    assert status(had, [1.0, 4.0]) == ERR_ARG
    assert L.rspt_hip_feed_end(had._h) == 0
    assert status(had, [1.0, 4.0]) == 0
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0]) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_budget_planar_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert status(dense, [128.0, 0.0]) == ERR_ARG and status(dense, [128.0, 16.0]) == 0
    dense.close()


def test_byte_order_has_no_effect(api):
    """rspt_hip_set_byte_order changes nothing: there are no bytes to order"""
    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(3)
    o = _mid_oracle(api, clean, ladder)
    pk = _new(api, MID)
    pk.set_byte_order(True)
    _held(pk, dirty, 4, ladder, o["limits"], o, "big-endian handle")
    pk.close()


def test_header_library_and_binding_agree(api):
    native_of = {"rspt_hip_compress_budget_planar_work_bytes": "rspt_hip_compress_budget_work_bytes",
                 "rspt_hip_compress_budget_planar_batch_dev": "rspt_hip_compress_budget_batch_dev"}
    df.check_entries(
        ["int rspt_hip_compress_budget_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);",
         "int rspt_hip_compress_budget_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, "
         "size_t nladder, size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes, "
         "uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream);"],
        list(native_of), native_of=native_of, methods=("budget_planar_work_bytes", "compress_to_budget_planar"))
