"""Compress to a PRDN target (rspt_hip_compress_target_batch_dev) on the cases of tests/target_cases.py, against two oracles:
(a) the composed one on the same device -- per ladder entry rspt_hip_set_quantizer, compress_batch, decompress_batch and
    prdn_batch, the rule applied on the host: the choice, the reported PRDN bit for bit, the streams byte for byte;
(b) the choices of the numpy restatement.
Where the fused probe runs (hadamard rows of up to 8192 points, nch * ns < 2^22) the general route and the fused one are forced in
turn (rspt_hip_debug_set_target_route) and held to the same oracles, so to each other bit for bit; a case on either side of the
2^22 bound shows the host switching routes.
And around it: the streams decode, through decompress_batch(ladder=, choice=), to samples whose PRDN is the reported one; a
second call on the same handle and work area writes the same bytes; the handle's own quantiser and its plain streams are what
they were before."""
import ctypes as C
import math

import numpy as np
import pytest

import lossy_dev as ld
import lossy_quantizer_cases as lq
import prdn_cases
import target_cases as tc
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in tc.all_cases()}


def _new(api, c):
    pk = api.SignalPacker(lq.KIND_ID[c["kind"]], c["bps"], c["nch"], c["ns"], lq.DEFAULTS[c["kind"]][1])
    pk.set_quantizer(nb=c["nb"])
    return pk


def _bits(a):
    """float64 array -> bit patterns, every NaN the canonical one"""
    return [prdn_cases.bits(x) for x in np.asarray(a, dtype=np.float64)]


def _composed(pk, d_src, c):
    """what a user does today, per ladder entry: (streams, sizes, prdn, mse, path) on the host; the handle is left as it was"""
    return [(o["dst"], o["sizes"], o["prdn"], o["mse"], o["path"]) for o in ld.composed(pk, d_src, c["ladder"], prdn=True)]


ROUTE_NAMES = {0: "auto", 1: "general", 2: "fused"}
# every case on the host's own choice; the fused shapes on each route forced as well
RUNS = [(n, 0) for n in CASES] + [(n, r) for n, c in CASES.items() if c["routes"] for r in (1, 2)]


def test_the_fused_probe_is_offered_where_the_header_says(api):
    for c in tc.all_cases():
        pk = _new(api, c)
        fused_ok = c["kind"] == "hadamard" and c["ns"] <= tc.FUSED_MAX_NS and c["nch"] * c["ns"] < 1 << 22
        assert fused_ok == c["routes"], c["name"]
        rc = api.lib().rspt_hip_debug_set_target_route(pk._h, 2)
        assert rc == (0 if fused_ok else ERR_UNSUPPORTED), c["name"]
        assert api.lib().rspt_hip_debug_set_target_route(pk._h, 3) == ERR_ARG and api.lib().rspt_hip_debug_set_target_route(pk._h, -1) == ERR_ARG
        pk.close()


@pytest.mark.parametrize("name,route", RUNS, ids=["%s-%s" % (n, ROUTE_NAMES[r]) for n, r in RUNS])
def test_target_against_the_composed_oracle_and_the_restatement(api, name, route):
    import torch

    c = CASES[name]
    nblocks, K = c["nblocks"], len(c["ladder"])
    pk = _new(api, c)
    d_src = torch.from_numpy(np.stack([tc.block_native(c, i) for i in range(nblocks)])).cuda()
    pk.debug_set_target_route(route)
    own = pk.quantizer()
    plain_before, plain_sizes = [t.cpu().numpy() for t in pk.compress_batch(d_src)]
    oracle = _composed(pk, d_src, c)

    work = ld.guarded_work(pk.target_work_bytes(nblocks, K))
    d_dst, d_sizes, d_choice, d_prdn = pk.compress_to_prdn(d_src, c["target"], c["ladder"], work=work[:-2])
    torch.cuda.synchronize()
    assert ld.work_guard_untouched(work)  # (nothing behind the bytes the sizing call names)
    assert pk.quantizer() == own
    choice, prdn, sizes, dst = d_choice.cpu().numpy(), d_prdn.cpu().numpy(), d_sizes.cpu().numpy(), d_dst.cpu().numpy()

    restated = tc.restated(c)
    for b in range(nblocks):
        figs = [(float(o[2][b]), float(o[3][b]), int(o[4][b])) for o in oracle]
        k, want = tc.choose(figs, c["target"])
        assert int(choice[b]) == k, (name, b, figs, "composed oracle")
        assert prdn_cases.bits(prdn[b]) == prdn_cases.bits(want), (name, b, prdn[b], want)
        n = int(oracle[k][1][b])
        assert int(sizes[b]) == n and np.array_equal(dst[b, :n], oracle[k][0][b, :n]), (name, b, "stream")
        rfigs, (rk, rp) = restated[b]
        assert int(choice[b]) == rk, (name, b, rfigs, figs, "restatement")
        assert [f[2] for f in figs] == [f[2] for f in rfigs] and prdn_cases.bits(want) == prdn_cases.bits(rp), (name, b, figs, rfigs)

    # the streams decode with the choice to samples of the reported PRDN
    d_out, d_used = pk.decompress_batch(d_dst, nblocks, d_dst.shape[1], ladder=c["ladder"], choice=d_choice)
    p2, mse2, ref2, path2 = pk.prdn_batch(d_src.reshape(-1), d_out.reshape(-1), parts=True)
    torch.cuda.synchronize()
    assert np.array_equal(d_used.cpu().numpy(), sizes)
    for b in range(nblocks):
        if int(path2[b]) == 0:
            assert prdn_cases.bits(p2[b].item()) == prdn_cases.bits(prdn[b]), (name, b)
        else:
            assert prdn[b] == math.inf, (name, b)

    # again on the same handle and work area: the same bytes
    again = pk.compress_to_prdn(d_src, c["target"], c["ladder"], work=work[:-2])
    torch.cuda.synchronize()
    assert np.array_equal(again[2].cpu().numpy(), choice) and _bits(again[3].cpu().numpy()) == _bits(prdn)
    assert np.array_equal(again[1].cpu().numpy(), sizes)
    for b in range(nblocks):
        assert np.array_equal(again[0][b, : int(sizes[b])].cpu().numpy(), dst[b, : int(sizes[b])]), (name, b)

    # the plain entries are what they were
    assert pk.quantizer() == own
    plain_after, sizes_after = [t.cpu().numpy() for t in pk.compress_batch(d_src)]
    assert np.array_equal(sizes_after, plain_sizes)
    for b in range(nblocks):
        assert np.array_equal(plain_after[b, : int(plain_sizes[b])], plain_before[b, : int(plain_sizes[b])]), (name, b)
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()

    def status(pk, ladder, target, nblocks=2):
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        d_src = torch.zeros((nblocks, pk.block_bytes), dtype=torch.uint8, device="cuda")
        d_dst = torch.full((nblocks, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        d_choice = torch.full((nblocks,), -1, dtype=torch.int32, device="cuda")
        work = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        rc = L.rspt_hip_compress_target_batch_dev(pk._h, d_src.data_ptr(), nblocks, lp, lad.size, float(target), d_dst.data_ptr(), 4096, d_sizes.data_ptr(),
                                                  d_choice.data_ptr(), None, work.data_ptr(), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_choice == -1).all()
        return rc

    had = api.new_hadamard(4, 3, 8)
    assert status(had, [1.0, 4.0], 1.0) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert status(had, [1.0, 4.0], bad) == ERR_ARG, bad
    assert status(had, [], 1.0) == ERR_ARG and status(had, [1.0] * 9, 1.0) == ERR_ARG and status(had, [1.0, 0.0], 1.0) == ERR_ARG
    n = C.c_size_t()
    assert L.rspt_hip_compress_target_work_bytes(had._h, 2, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_target_work_bytes(had._h, 0, 2, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_compress_target_work_bytes(had._h, 2, 9, C.byref(n)) == ERR_ARG
    assert had.target_work_bytes(3, 8) >= had.target_work_bytes(3, 1) >= 2 * 3 * had.nch * had.ns * 4
    had.close()
    for pk in (api.new_dct(4, 1, 16384), api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8),
               api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, [128.0], 1.0) == ERR_UNSUPPORTED, pk.kind
        assert L.rspt_hip_compress_target_work_bytes(pk._h, 2, 1, C.byref(n)) == ERR_UNSUPPORTED
        pk.close()
