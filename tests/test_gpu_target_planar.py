"""Compress to a PRDN target from the planar int32 matrix (rspt_hip_compress_target_planar_batch_dev) on the matrices of
tests/target_planar_cases.py, against two oracles that never involve the code under test:
(a) the native entry on i32_to_native(P) -- rspt_hip_compress_target_batch_dev, which tests/test_gpu_target.py holds to the composed
    oracle: the choice, the PRDN bit for bit, the sizes, the streams byte for byte;
(b) the choices of the numpy restatement (target_cases.restated).
Every case runs on the host's own route, the fused shapes on each route forced as well; the cases below four bytes a sample also
with garbage above the sample width, with the same results; every matrix also from a base 4 bytes past a 16-byte boundary.
Around it: a NaN guard band behind the work area, the bounds on the work bytes, a second call writing the same bytes, the decode
through decompress_planar_batch(ladder=, choice=) to the reported PRDN, the matrix only read, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import devframe as df
import lossy_quantizer_cases as lq
import prdn_cases
import target_cases as tc
import target_planar_cases as tp
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in tc.all_cases()}
ROUTE_NAMES = {0: "auto", 1: "general", 2: "fused"}
# every case on the host's own choice; the fused shapes on each route forced as well
RUNS = [(n, 0) for n in CASES] + [(n, r) for n, c in CASES.items() if c["routes"] for r in (1, 2)]


def _new(api, c):
    pk = api.SignalPacker(lq.KIND_ID[c["kind"]], c["bps"], c["nch"], c["ns"], lq.DEFAULTS[c["kind"]][1])
    pk.set_quantizer(nb=c["nb"])
    return pk


def _bits(a):
    return [prdn_cases.bits(x) for x in np.asarray(a, dtype=np.float64)]


@pytest.fixture(scope="module")
def oracle(api):
    """per case, once: (choice, prdn, sizes, streams) of the native entry on i32_to_native(P), on the host's own route"""
    memo = {}

    def get(name):
        import torch

        if name not in memo:
            c = CASES[name]
            pk = _new(api, c)
            d_native = pk.from_planar_i32(torch.from_numpy(tp.matrix(c).copy()).cuda())
            d_dst, d_sizes, d_choice, d_prdn = pk.compress_to_prdn(d_native, c["target"], c["ladder"])
            torch.cuda.synchronize()
            memo[name] = (d_choice.cpu().numpy(), d_prdn.cpu().numpy(), d_sizes.cpu().numpy(), d_dst.cpu().numpy(), d_native)
            pk.close()
        return memo[name]

    return get


@pytest.mark.parametrize("name,route", RUNS, ids=["%s-%s" % (n, ROUTE_NAMES[r]) for n, r in RUNS])
def test_target_planar_is_the_native_entry_on_the_converted_matrix(api, oracle, name, route):
    import torch

    c = CASES[name]
    nblocks, K = c["nblocks"], len(c["ladder"])
    o_choice, o_prdn, o_sizes, o_dst, d_native = oracle(name)
    restated = tc.restated(c)
    for b in range(nblocks):  # oracle (b), and that the two oracles agree
        assert int(o_choice[b]) == restated[b][1][0] and prdn_cases.bits(o_prdn[b]) == prdn_cases.bits(restated[b][1][1]), (name, b)

    pk = _new(api, c)
    pk.debug_set_target_route(route)
    own = pk.quantizer()
    nwork = pk.target_planar_work_bytes(nblocks, K)
    # the bounds on the work bytes (include/rspt_hip.h)
    copy = nblocks * c["nch"] * c["ns"] * 4
    fused = route == 2 or (route == 0 and c["routes"])
    if c["bps"] == 4:
        assert nwork <= pk.target_work_bytes(nblocks, K) - copy, (name, nwork)
    else:  # (the cut original takes the place of the native entry's kept one: never more than that entry)
        assert nwork <= pk.target_work_bytes(nblocks, K), (name, nwork)
    if fused:  # the host's choice, and the forced fused route alike
        assert nwork < copy, (name, nwork, copy)

    first = None
    for vtag, garbage in tp.variants(c):
        P = tp.matrix(c, garbage)
        for off in tp.OFFSETS:
            tag = (name, ROUTE_NAMES[route], vtag, off)
            sraw, src = df.guarded_matrix(P, off)
            work = torch.full(((nwork + 7) // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
            d_dst, d_sizes, d_choice, d_prdn = pk.compress_to_prdn_planar(src, c["target"], c["ladder"], work=work[:-2])
            torch.cuda.synchronize()
            assert all(x != x for x in work[-2:].cpu().numpy()), tag  # (nothing behind the bytes the sizing call names)
            assert pk.quantizer() == own, tag
            choice, prdn, sizes, dst = d_choice.cpu().numpy(), d_prdn.cpu().numpy(), d_sizes.cpu().numpy(), d_dst.cpu().numpy()
            assert np.array_equal(choice, o_choice), (tag, choice, o_choice)
            assert _bits(prdn) == _bits(o_prdn), (tag, prdn, o_prdn)
            assert np.array_equal(sizes, o_sizes), tag
            for b in range(nblocks):
                n = int(o_sizes[b])
                assert np.array_equal(dst[b, :n], o_dst[b, :n]), (tag, b, "stream")
            assert np.array_equal(src.cpu().numpy(), P) and df.guards_untouched(sraw, off, P.size * 4), (tag, "d_planar is only read")
            if first is None:
                first = (src, work, d_dst, d_choice, choice, prdn, sizes, dst)

    # again on the same handle and work area: the same bytes
    src, work, d_dst, d_choice, choice, prdn, sizes, dst = first
    again = pk.compress_to_prdn_planar(src, c["target"], c["ladder"], work=work[:-2])
    torch.cuda.synchronize()
    assert np.array_equal(again[2].cpu().numpy(), choice) and _bits(again[3].cpu().numpy()) == _bits(prdn)
    assert np.array_equal(again[1].cpu().numpy(), sizes)
    for b in range(nblocks):
        assert np.array_equal(again[0][b, : int(sizes[b])].cpu().numpy(), dst[b, : int(sizes[b])]), (name, b)

    # the streams decode, through the planar ladder decoder, to a matrix whose PRDN against i32_to_native(P) is the reported one
    d_out, d_used = pk.decompress_planar_batch(d_dst, nblocks, d_dst.shape[1], ladder=c["ladder"], choice=d_choice)
    d_back = pk.from_planar_i32(d_out)
    p2, mse2, ref2, path2 = pk.prdn_batch(d_native.reshape(-1), d_back.reshape(-1), parts=True)
    torch.cuda.synchronize()
    assert np.array_equal(d_used.cpu().numpy(), sizes)
    for b in range(nblocks):
        if int(path2[b]) == 0:
            assert prdn_cases.bits(p2[b].item()) == prdn_cases.bits(prdn[b]), (name, b)
        else:
            assert prdn[b] == math.inf, (name, b)
    assert api.lib().rspt_hip_last_hip_error(pk._h) == 0
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()

    def status(pk, ladder, target, nblocks=2, planar_off=0, work_off=0, choice_off=0):
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        d_planar = torch.zeros((nblocks * pk.nch * pk.ns + 4,), dtype=torch.int32, device="cuda")
        d_dst = torch.full((nblocks, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks + 1,), -1, dtype=torch.int32, device="cuda")
        work = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        rc = L.rspt_hip_compress_target_planar_batch_dev(pk._h, d_planar.data_ptr() + planar_off, nblocks, lp, lad.size, float(target), d_dst.data_ptr(),
                                                         4096, d_sizes.data_ptr(), d_choice.data_ptr() + choice_off, None, work.data_ptr() + work_off, None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all() and (work == 0).all()
        return rc

    had = api.new_hadamard(4, 3, 8)
    assert status(had, [1.0, 4.0], 1.0) == 0
    assert status(had, [1.0, 4.0], 1.0, planar_off=4) == 0  # any 4-byte alignment of the matrix
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert status(had, [1.0, 4.0], bad) == ERR_ARG, bad
    assert status(had, [], 1.0) == ERR_ARG and status(had, [1.0] * 9, 1.0) == ERR_ARG and status(had, [1.0, 0.0], 1.0) == ERR_ARG
    for off in (1, 2, 3):
        assert status(had, [1.0, 4.0], 1.0, planar_off=off) == ERR_ARG, off
    assert status(had, [1.0, 4.0], 1.0, work_off=8) == ERR_ARG and status(had, [1.0, 4.0], 1.0, choice_off=2) == ERR_ARG
    n = C.c_size_t()
    assert L.rspt_hip_compress_target_planar_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_target_planar_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_target_planar_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_target_planar_work_bytes(had._h, 2, 2, None) == ERR_ARG
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0], 1.0) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_target_planar_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        pk.close()
