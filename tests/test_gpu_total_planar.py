"""Compress a batch to one byte total from the planar int32 matrix (rspt_hip_compress_total_planar_batch_dev) on the matrices of
tests/total_planar_cases.py, against two oracles that never involve the code under test:
(a) the native entry on from_planar_i32(P) on the same device -- rspt_hip_compress_total_batch_dev, which tests/test_gpu_total.py
    holds to the composed oracle: d_choice, d_level's bit pattern, d_total, d_prdn's bit patterns, both tables, d_sizes with bit
    63, the streams byte for byte, and the decode;
(b) the rule of tests/total_cases.py (choose_total_np) on the composed oracle's tables (lossy_dev.composed, total_dev.tables_of).
The totals are placed at run time on the composed oracle's tables (total_dev.some_totals), never on the planar call's output.
Every shape runs on the host's own route, the fused shapes on each route forced as well; the shapes below four bytes a sample also
with garbage above the sample width, with the same results; every matrix also from a base 4 bytes past a 16-byte boundary.  Around
it: a NaN guard band behind the work area, the matrix only read, the work-area sizes the header names, the decode through the
planar ladder decoder and through a container, batches on either side of a wave, of the level kernel's workgroup, of the round
kernel's threshold and of the 65535-slot bound, unrated blocks, the handle behind the call, a stride some chosen streams do not
fit, the refusals."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import devframe as df
import lossy_dev as ld
import lossy_quantizer_cases as lq
import total_cases as tt
import total_dev as td
import total_planar_cases as tp
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401
from test_gpu_total import MID, TINY, _tiny_batch

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
ROUTE_NAMES = {0: "auto", 1: "general", 2: "fused"}


def _new(api, shape):
    kind, bps, nch, ns, nb = shape
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _pad(n):
    return (n + 255) // 256 * 256


class Ref:
    """Both oracles of one (native batch, ladder), on a handle of its own that never sees a planar total call: the composed
    oracle, its tables and the totals placed on them; per total, memoised, (a) the native entry's results and (b) the rule's."""

    def __init__(self, api, shape, P, ladder, n=8):
        import torch

        self.shape, self.ladder = shape, list(ladder)
        self.pk = _new(api, shape)
        self.d_native = self.pk.from_planar_i32(torch.from_numpy(np.array(P)).cuda())  # (a copy: P may be read-only)
        self.composed = ld.composed(self.pk, self.d_native, self.ladder, prdn=True)
        self.tables = td.tables_of(self.composed)
        self.totals = td.some_totals(self.composed, n=n)
        self._a, self._b = {}, {}

    def native(self, total):
        if total not in self._a:
            o = ld.rate_call(self.pk, "total", self.d_native, total, self.ladder, (self.shape, total, "native oracle"))
            o["decoded"] = None
            self._a[total] = o
        return self._a[total]

    def decoded(self, total):
        """the planar matrix of the native decode (small batches)"""
        o = self.native(total)
        if o["decoded"] is None:
            o["decoded"] = tp.to_matrix(o["out"], self.shape)
        return o["decoded"]

    def rule(self, total):
        if total not in self._b:
            self._b[total] = tt.choose_total_np(*self.tables, total)
        return self._b[total]

    def close(self):
        self.pk.close()


def _equals(got, ref, total, tag):
    """a planar call's results against oracle (a) in full and against oracle (b) -> the level of the rule"""
    o = ref.native(total)
    assert np.array_equal(got["cand"], o["cand"]), (tag, "the table of candidate sizes")
    assert np.array_equal(got["figs"].view(np.uint64), o["figs"].view(np.uint64)), (tag, "the table of figures")
    assert got["level"] == o["level"], (tag, tt.from_bits(got["level"]), tt.from_bits(o["level"]))
    assert np.array_equal(got["choice"], o["choice"]), (tag, np.flatnonzero(got["choice"] != o["choice"])[:8].tolist())
    assert got["total"] == o["total"], (tag, got["total"], o["total"])
    assert np.array_equal(got["prdn"].view(np.uint64), o["prdn"].view(np.uint64)), (tag, "d_prdn")
    assert np.array_equal(got["sizes"].view(np.uint64), o["sizes"].view(np.uint64)), (tag, "d_sizes")
    n = (o["sizes"].view(np.uint64) & np.uint64(BIT63 - 1)).astype(np.int64)
    assert not (o["sizes"].view(np.uint64) >> np.uint64(63)).any(), tag  # (the oracle's stride holds every stream)
    w = min(got["dst"].shape[1], o["dst"].shape[1])
    assert int(n.max()) <= w, tag
    cols = np.arange(w)[None, :]
    assert ((got["dst"][:, :w] == o["dst"][:, :w]) | (cols >= n[:, None])).all(), (tag, "streams")
    level, choice, cost = ref.rule(total)
    assert got["level"] == tt.bits(level), (tag, "the rule's level", tt.from_bits(got["level"]), level)
    assert np.array_equal(got["choice"], choice), (tag, "the rule's choice")
    assert got["total"] == cost, (tag, "the rule's cost", got["total"], cost)
    return level


def _held(pk, P, off, ref, total, tag, ladder=None):
    """P from a base `off` bytes past a 16-byte boundary through one planar call, held to both oracles; the matrix and its guards
    are untouched afterwards -> (the call's device tensors, the rule's level)"""
    sraw, src = df.guarded_matrix(P, off)
    got = ld.rate_call(pk, "total", src, total, ladder or ref.ladder, tag, planar=True)
    level = _equals(got, ref, total, tag)
    assert np.array_equal(src.cpu().numpy(), P) and df.guards_untouched(sraw, off, P.size * 4), (tag, "d_planar is only read")
    return got["dev"], level


@pytest.fixture(scope="module")
def refs(api):
    """per shape, once: the oracles of its clean matrix and ladder"""
    memo = {}

    def get(shape):
        if shape not in memo:
            memo[shape] = Ref(api, shape, tp.matrix(shape), bc.ladder_of(shape[0]))
            assert np.array_equal(memo[shape].d_native.cpu().numpy(), bc.batch_native(shape, tp.NBLOCKS))
        return memo[shape]

    yield get
    for r in memo.values():
        r.close()


SHAPE_RUNS = [(s, 0) for s in tp.SHAPES] + [(s, r) for s in tp.SHAPES if tp.FUSED[s] for r in (1, 2)]


@pytest.mark.parametrize("shape,route", SHAPE_RUNS, ids=["%s-%s" % (bc.shape_id(s), ROUTE_NAMES[r]) for s, r in SHAPE_RUNS])
def test_total_planar_is_the_native_entry_on_the_converted_matrix(api, refs, shape, route):
    ref = refs(shape)
    assert 6 <= len(ref.totals) <= 10
    assert len({tt.bits(ref.rule(t)[0]) for t in ref.totals}) >= 2, "the totals place at least two levels"
    pk = _new(api, shape)
    assert api.lib().rspt_hip_debug_set_total_route(pk._h, 2) == (0 if tp.FUSED[shape] else ERR_UNSUPPORTED)
    pk.debug_set_total_route(route)
    levels = set()
    for total in ref.totals:
        for vtag, garbage in tp.variants(shape):
            for off in tp.OFFSETS:
                levels.add(tt.bits(_held(pk, tp.matrix(shape, garbage), off, ref, total, (bc.shape_id(shape), ROUTE_NAMES[route], total, vtag, off))[1]))
    assert len(levels) >= 2, levels
    pk.close()


@pytest.mark.parametrize("shape", tp.SHAPES, ids=[bc.shape_id(s) for s in tp.SHAPES])
def test_the_work_area_is_what_the_header_names(api, shape):
    """fused: the native fused one's, tables alone; general at bps 4: the native general one less the 256-padded original; general
    at bps < 4: the native general one's.  No kernel runs."""
    kind, bps, nch, ns, nb = shape
    pk = _new(api, shape)
    for B, K in ((tp.NBLOCKS, len(bc.ladder_of(kind))), (1, 1), (3, 8)):
        for route in (0, 1, 2) if tp.FUSED[shape] else (0, 1):
            pk.debug_set_total_route(route)
            native, planar = pk.total_work_bytes(B, K), pk.total_planar_work_bytes(B, K)
            if (route == 0 and tp.FUSED[shape]) or route == 2:
                assert planar == native and K * B * 72 + 1280 <= planar < K * B * 72 + 1280 + 8 * 256, (shape, B, K, route)
            else:
                assert native == 2 * _pad(K * B * 8) + 1280 + pk.target_work_bytes(B, K), (shape, B, K, route)
                assert planar == native - (_pad(B * nch * ns * 4) if bps == 4 else 0), (shape, B, K, route)
    pk.close()


@pytest.mark.parametrize("shape", tp.SHAPES, ids=[bc.shape_id(s) for s in tp.SHAPES])
def test_the_streams_decode_and_travel_in_a_container(api, refs, shape):
    """decompress_planar_batch(ladder=, choice=d_choice) gives to_planar_i32 of the native decode and consumes d_sizes; and
    compress_to_total_planar -> pack_batch(choice=, nladder=) -> decompress_packed_planar(ladder=) gives the same matrix"""
    import torch

    ref = refs(shape)
    total = ref.totals[len(ref.totals) // 2]
    o = ref.native(total)
    pk = _new(api, shape)
    garbage = tp.variants(shape)[-1][1]
    res, _ = _held(pk, tp.matrix(shape, garbage), 4, ref, total, (bc.shape_id(shape), "decode"))
    d_dst, d_sizes, d_choice = res[:3]
    d_out, d_used = pk.decompress_planar_batch(d_dst, tp.NBLOCKS, d_dst.shape[1], ladder=ref.ladder, choice=d_choice)
    d_packed, d_total = pk.pack_batch(d_dst, d_sizes, choice=d_choice, nladder=len(ref.ladder))
    torch.cuda.synchronize()
    assert np.array_equal(d_used.cpu().numpy(), o["sizes"])
    assert np.array_equal(d_out.cpu().numpy(), ref.decoded(total))
    d_back, d_used2 = pk.decompress_packed_planar(d_packed[: int(d_total.item())].clone(), ladder=ref.ladder)
    torch.cuda.synchronize()
    assert np.array_equal(d_used2.cpu().numpy(), o["sizes"])
    assert np.array_equal(d_back.cpu().numpy(), ref.decoded(total))
    assert ld.last_hip_error(pk) == 0
    pk.close()


@pytest.fixture(scope="module")
def tiny():
    """8192 blocks of TINY as a matrix, once: the batch-size tests take its first B blocks"""
    assert TINY[1] == 4
    P = tp.to_matrix(_tiny_batch(8192), TINY)
    P.setflags(write=False)
    return P


BATCH_RUNS = [(B, r) for B in (1, 257, 1025) for r in (1, 2)]


@pytest.mark.parametrize("B,route", BATCH_RUNS, ids=["%dx8-%s" % (B, ROUTE_NAMES[r]) for B, r in BATCH_RUNS])
def test_batch_sizes(api, tiny, B, route):
    """one wave, past k_total_pick's workgroup, past the 1024 blocks k_total_level keeps in registers"""
    ref = Ref(api, TINY, tiny[:B], bc.LADDER8, n=4)
    pk = _new(api, TINY)
    pk.debug_set_total_route(route)
    for i, total in enumerate(ref.totals):
        _held(pk, tiny[:B], 4 * (i & 1), ref, total, (B, ROUTE_NAMES[route], total))
    pk.close()
    ref.close()


def test_65536_slots_take_the_general_route_and_57344_the_fused_one_behind_the_round_kernel(api, tiny):
    """8192 tiny blocks with 8 entries: one slot more than the fused route takes, so the host picks the general one -- and a forced
    fused route is refused by both new entries, d_work untouched; 7 entries are accepted, and with more than 4096 blocks
    k_total_round finds the level behind the planar probe"""
    import torch

    B = 8192
    assert B * 8 == tp.MAX_SLOTS + 1 and not tp.fused(TINY, B, 8) and tp.fused(TINY, B, 7) and B > 4096
    ref8 = Ref(api, TINY, tiny, bc.LADDER8, n=2)
    pk = _new(api, TINY)
    general = pk.total_planar_work_bytes(B, 8)
    assert general == pk.total_work_bytes(B, 8) - _pad(B * TINY[2] * TINY[3] * 4)
    for total in ref8.totals[1:3]:
        _held(pk, tiny, 4, ref8, total, ("65536 slots, the host's route", total))
    ref8.close()
    pk.debug_set_total_route(2)
    n = C.c_size_t()
    assert api.lib().rspt_hip_compress_total_planar_work_bytes(pk._h, B, 8, C.byref(n)) == ERR_UNSUPPORTED
    assert api.lib().rspt_hip_compress_total_planar_work_bytes(pk._h, B, 7, C.byref(n)) == 0 and n.value == pk.total_work_bytes(B, 7) < general
    d_x = torch.from_numpy(np.array(tiny)).cuda()
    work = torch.zeros(general // 8 + 1, dtype=torch.float64, device="cuda")
    with pytest.raises(api.RsptHipError):
        pk.compress_to_total_planar(d_x, 100, bc.LADDER8, work=work)
    torch.cuda.synchronize()
    assert int(work.count_nonzero()) == 0
    ref7 = Ref(api, TINY, tiny, bc.LADDER8[:7], n=2)
    seen = set()
    for total in ref7.totals[1:3] + [tt.U64_MAX]:  # (a miss, or a level above the lowest; and the lowest admissible level)
        seen.add(tt.bits(_held(pk, tiny, 0, ref7, total, ("57344 slots, fused", total))[1]))
    assert len(seen) >= 2
    ref7.close()
    pk.close()


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_unrated_blocks_take_their_smallest_stream_and_their_figures_never_count(api, route):
    """full-scale samples at nb = 1: every entry of blocks 0 and 2 has path 1"""
    shape, ladder = ("hadamard", 4, 2, 64, 1), [1.0 / 4, 1.0, 64.0]
    P = tp.to_matrix(bc.batch_native(shape, 3, ("full", "rand", "full")), shape)
    ref = Ref(api, shape, P, ladder)
    sizes, prdn, mse, path = ref.tables
    assert (path[:, [0, 2]] == 1).all() and (path[:, 1] == 0).all()
    pk = _new(api, shape)
    pk.debug_set_total_route(route)
    for total in ref.totals:
        res, _ = _held(pk, P, 4, ref, total, (ROUTE_NAMES[route], total))
        choice = res[2].cpu().numpy()
        assert all(int(choice[b]) == int(np.argmin(sizes[:, b])) for b in (0, 2))
    both = np.ascontiguousarray(P[[0, 2]])  # no rated block at all: the level is +0.0 whatever the total
    part = Ref(api, shape, both, ladder)
    for total in (0, tt.U64_MAX):
        res, level = _held(pk, both, 0, part, total, (ROUTE_NAMES[route], "unrated alone", total))
        assert tt.bits(level) == 0 and int(res[3].cpu().numpy().view(np.uint64)[0]) == 0 and int(res[4].item()) > 0
    part.close()
    ref.close()
    pk.close()


def _mid_matrix(B, seed=5200):
    """(clean, garbage) matrices of B blocks of MID"""
    P = tp.to_matrix(bc.batch_native(MID, B), MID)
    return P, tp.with_garbage(P, MID[1], seed + B)


def _same_streams(got, want, tag):
    """(d_dst, d_sizes, ...) of two calls: equal sizes, equal bytes up to them, everything else equal bit for bit"""
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    n = got[1].view(np.uint64)
    assert np.array_equal(n, want[1].view(np.uint64)) and not (n >> np.uint64(63)).any(), (tag, "sizes")
    cols = np.arange(got[0].shape[1])[None, :]
    assert ((got[0] == want[0]) | (cols >= n.astype(np.int64)[:, None])).all(), (tag, "streams")
    for x, y in zip(got[2:], want[2:]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), tag


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_the_handle_behind_total_planar_calls(api, route):
    """native and planar total calls alternating on one handle with batches of 5, 2 and 9 blocks, each at its oracle; and a plain
    compress_planar_batch, a plain compress_batch, compress_to_prdn_planar and compress_to_budget_planar right behind a planar
    total call write what a fresh handle writes"""
    import torch

    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(9)
    d_clean, d_dirty = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    slices = ((0, 5), (5, 7), (0, 9))
    parts = [Ref(api, MID, clean[lo:hi], ladder, n=3) for lo, hi in slices]

    def others(p, d_native):
        return [("plain planar", lambda: p.compress_planar_batch(d_dirty)), ("plain native", lambda: p.compress_batch(d_native)),
                ("target planar", lambda: p.compress_to_prdn_planar(d_dirty[:5], 2.0, ladder)),
                ("budget planar", lambda: p.compress_to_budget_planar(d_dirty, 6000, ladder))]

    fresh = _new(api, MID)  # never sees a total call
    want = [(name, call()) for name, call in others(fresh, fresh.from_planar_i32(d_clean))]
    torch.cuda.synchronize()
    pk = _new(api, MID)
    pk.debug_set_total_route(route)
    d_native = pk.from_planar_i32(d_clean)
    for (lo, hi), ref in zip(slices, parts):
        tag = (ROUTE_NAMES[route], lo, hi)
        mid = ref.totals[len(ref.totals) // 2]
        _held(pk, dirty[lo:hi], 4, ref, mid, tag + ("planar",))
        got = _host_native(pk, d_native[lo:hi], ladder, ref.totals[-2], tag + ("native",))
        _equals(got, ref, ref.totals[-2], tag + ("native",))
        _held(pk, clean[lo:hi], 0, ref, ref.totals[-2], tag + ("planar again",))
    ref = parts[2]
    for (name, call), (_, w) in zip(others(pk, d_native), want):
        _held(pk, dirty, 4, ref, ref.totals[len(ref.totals) // 2], (ROUTE_NAMES[route], "before", name))
        _same_streams(call(), w, (ROUTE_NAMES[route], name))
    assert ld.last_hip_error(pk) == 0
    for r in parts:
        r.close()
    fresh.close()
    pk.close()


def _host_native(pk, d_native, ladder, total, tag):
    """the native entry on this handle: what _equals compares of a planar call"""
    o = ld.rate_call(pk, "total", d_native, total, ladder, tag)
    return {k: o[k] for k in ("choice", "level", "total", "prdn", "sizes", "dst", "cand", "figs")}


@pytest.mark.parametrize("route", (1, 2), ids=["general", "fused"])
def test_a_chosen_stream_that_does_not_fit_the_stride_is_flagged_as_the_planar_ladder_call_flags_it(api, route):
    import torch

    ladder = bc.ladder_of("hadamard")
    clean, dirty = _mid_matrix(5)
    ref = Ref(api, MID, clean, ladder)
    sizes = ref.tables[0]
    total = ref.totals[len(ref.totals) // 2]
    level, want, cost = ref.rule(total)
    o = ref.native(total)
    chosen = sorted(int(sizes[k, b]) for b, k in enumerate(want))
    stride = (chosen[2] + 15) // 16 * 16  # holds some of the chosen streams and not others: the stride plays no part in the rule
    assert chosen[0] <= stride < chosen[-1]
    pk = _new(api, MID)
    pk.debug_set_total_route(route)
    sraw, src = df.guarded_matrix(dirty, 4)
    d_dst = torch.full((5, stride), 0xC3, dtype=torch.uint8, device="cuda")
    got = ld.rate_call(pk, "total", src, total, ladder, ROUTE_NAMES[route], planar=True, d_dst=d_dst)
    res = got["dev"]
    l_dst = torch.full((5, stride), 0xC3, dtype=torch.uint8, device="cuda")
    l_dst, l_sizes = pk.compress_planar_batch(src, d_dst=l_dst, ladder=ladder, choice=res[2])
    torch.cuda.synchronize()
    assert got["choice"].tolist() == want.tolist() == o["choice"].tolist() and got["level"] == tt.bits(level) == o["level"] and got["total"] == cost
    assert np.array_equal(got["cand"], o["cand"]) and np.array_equal(got["figs"].view(np.uint64), o["figs"].view(np.uint64))
    assert np.array_equal(got["prdn"].view(np.uint64), o["prdn"].view(np.uint64))
    out = got["sizes"].view(np.uint64)
    assert np.array_equal(out, l_sizes.cpu().numpy().view(np.uint64)) and np.array_equal(got["dst"], l_dst.cpu().numpy())
    for b, k in enumerate(want):
        n = int(sizes[k, b])
        assert int(out[b]) == (n if n <= stride else n | BIT63), b
        if n > stride:
            assert (got["dst"][b] == 0xC3).all(), (b, "nothing is written")
        else:
            assert np.array_equal(got["dst"][b, :n], o["dst"][b, :n]), b
    assert np.array_equal(src.cpu().numpy(), dirty) and df.guards_untouched(sraw, 4, dirty.size * 4)
    ref.close()
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    n = C.c_size_t()
    OPTIONAL = ("level", "total", "prdn", "cand", "figs")

    def status(pk, ladder, nblocks=2, off=None, optional=False, stride=4096, says=None):
        """the entry's status; off: {argument: bytes off its boundary}, "null": no matrix; says: the block count the call names,
        where it is not that of the buffers.  A refused call launches nothing: the buffers stay as they were"""
        off = off or {}
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        nsamp = getattr(pk, "nch", 1) * getattr(pk, "ns", 64)
        d_planar = torch.zeros(max(nblocks, 1) * nsamp + 4, dtype=torch.int32, device="cuda")
        d_dst = torch.full((max(nblocks, 1), 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks + 1,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks + 4,), -1, dtype=torch.int32, device="cuda")
        opt = {name: torch.full((8 * nblocks + 2,), -1, dtype=torch.int64, device="cuda") for name in OPTIONAL}
        work = torch.full((1 << 13,), -1, dtype=torch.int64, device="cuda")
        ptr = [opt[name].data_ptr() + off.get(name, 0) if optional or name in off else None for name in OPTIONAL]
        rc = L.rspt_hip_compress_total_planar_batch_dev(
            pk._h, d_planar.data_ptr() + off.get("planar", 0) if "null" not in off else None, nblocks if says is None else says, lp, lad.size, 1000,
            d_dst.data_ptr(), stride, d_sizes.data_ptr(), d_choice.data_ptr() + off.get("choice", 0), *ptr, work.data_ptr() + off.get("work", 0), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all() and (work == -1).all()
            assert all((t == -1).all() for t in opt.values()) and (d_planar == 0).all()
        return rc

    had = _new(api, ("hadamard", 4, 3, 8, 3))
    assert status(had, [1.0, 4.0]) == 0 and status(had, [1.0, 4.0], optional=True) == 0
    assert status(had, [1.0, 4.0], off={"planar": 4}) == 0 and status(had, [1.0, 4.0], off={"planar": 12}) == 0  # any 4-byte alignment of the matrix
    for by in (1, 2, 3):
        assert status(had, [1.0, 4.0], off={"planar": by}) == ERR_ARG, by
    assert status(had, []) == ERR_ARG and status(had, [1.0] * 9) == ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):
        assert status(had, [1.0, bad]) == ERR_ARG, bad
    for arg, by in (("work", 8), ("choice", 2)) + tuple((name, 4) for name in OPTIONAL):
        assert status(had, [1.0, 4.0], off={arg: by}) == ERR_ARG, arg
    assert status(had, [1.0, 4.0], off=dict({name: 8 for name in OPTIONAL}, planar=4, choice=4, work=16)) == 0  # (their own boundaries are enough)
    assert status(had, [1.0, 4.0], off={"null": 1}) == ERR_ARG
    assert status(had, [1.0, 4.0], says=0) == ERR_ARG and status(had, [1.0, 4.0], says=65536) == ERR_ARG
    assert status(had, [1.0, 4.0], stride=1 << 32) == ERR_ARG  # (2^32 bytes per 65536 samples of a block)
    assert L.rspt_hip_compress_total_planar_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_planar_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_planar_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_planar_work_bytes(had._h, 65536, 1, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_total_planar_work_bytes(had._h, 2, 2, None) == ERR_ARG
    assert status(had, [1.0, 4.0], nblocks=1) == 0
    had.feed_begin(1, 2)
    assert status(had, [1.0, 4.0]) == ERR_ARG  # an open feed owns the workspace
    had.feed_end()
    assert status(had, [1.0, 4.0]) == 0
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0]) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_total_planar_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert status(dense, [128.0, 0.0]) == ERR_ARG and status(dense, [128.0, 16.0]) == 0
    dense.close()


def test_byte_order_has_no_effect(api):
    """rspt_hip_set_byte_order changes nothing: there are no bytes to order"""
    clean, dirty = _mid_matrix(3)
    ref = Ref(api, MID, clean, bc.ladder_of("hadamard"), n=3)
    pk = _new(api, MID)
    pk.set_byte_order(True)
    for total in ref.totals[1:4]:
        _held(pk, dirty, 4, ref, total, ("big-endian handle", total))
    ref.close()
    pk.close()


def test_header_library_and_binding_agree(api):
    native_of = {"rspt_hip_compress_total_planar_work_bytes": "rspt_hip_compress_total_work_bytes",
                 "rspt_hip_compress_total_planar_batch_dev": "rspt_hip_compress_total_batch_dev"}
    df.check_entries(
        ["int rspt_hip_compress_total_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);",
         "int rspt_hip_compress_total_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, "
         "size_t nladder, size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level, "
         "uint64_t* d_total, double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream);"],
        list(native_of), native_of=native_of, methods=("total_planar_work_bytes", "compress_to_total_planar"))
