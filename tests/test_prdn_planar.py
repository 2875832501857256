"""PRDN on the planar int32 matrix ("The planar form"): rspt_hip_prdn_planar_batch_dev,
SignalPacker.prdn_planar_batch and SignalPacker.roundtrip_quality_planar.

CPU: the C ABI, the planar restatement (tests/prdn_planar_cases.py) against the reference's record by bit pattern, the in-width
identity with the native restatement at bps 1 - 3, the shapes of the GPU tests against the host's thresholds, and that no new
kernel uses scratch.  GPU (-m gpu): bit-exact against the record, over the row-geometry grid at every offset of the two buffers,
on both sides of every threshold of the host's choice of form, on handles of every width, against the native entry on the device,
on real round trips, stream-ordered, and the refusals."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import cases
import devframe as df
import planar_cases as pl
import prdn_cases as pc
import prdn_planar_cases as pp
from devframe import ERR_ARG, ERR_UNSUPPORTED, ROOT, api, asm  # noqa: F401

ENTRY = "rspt_hip_prdn_planar_batch_dev"
SYNTH = [c["name"] for c in pc.synthetic_cases()]
LOSSY = [c["name"] for c in pc.lossy_fixtures()]
ALL = SYNTH + [pc.REF_SEQ["name"]] + LOSSY
NB_CTOR = {"hzr": 4, "xdelta_hzr": 3, "dct": 2, "hadamard": 3}


@pytest.fixture(scope="module")
def record():
    return {r["name"]: r for r in df.golden("prdn_record.json")["cases"]}


@pytest.fixture(scope="module")
def pcases(orc):
    """every case of the record with its two blocks (as tests/test_prdn.py makes them)"""
    out = {c["name"]: c for c in pc.synthetic_cases()}
    out[pc.REF_SEQ["name"]] = pc.ref_seq_case()
    for f in pc.lossy_fixtures():
        out[f["name"]] = pc.lossy_case(f, pc.oracle_decoded(orc, f))
    return out


# ---- CPU ----

def test_header_declares_the_entry_and_the_library_exports_it():
    hdr = df.header(flat=False)
    m = re.search(r"int\s+rspt_hip_prdn_planar_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+int32_t\s*\*\s*d_orig\s*,\s*const\s+int32_t\s*\*\s*d_dec\s*,"
                  r"\s*size_t\s+nblocks\s*,\s*double\s*\*\s*d_prdn\s*,\s*double\s*\*\s*d_mse\s*,\s*double\s*\*\s*d_ref\s*,\s*uint32_t\s*\*\s*d_path\s*,"
                  r"\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert m
    section = hdr[hdr.rindex("/* ----", 0, m.start()):m.start()]
    for word in ("whole int32", "bps = 4"):
        assert word in section, word
    df.check_entries((), (ENTRY,))


def test_a_null_handle_is_refused_without_a_device():
    from rspt_amd import api

    buf = (C.c_double * 4)()
    assert getattr(api.lib(), ENTRY)(None, buf, buf, 1, buf, None, None, None, None) == ERR_ARG


def test_the_python_entries_exist():
    from rspt_amd import api

    assert callable(api.SignalPacker.prdn_planar_batch) and callable(api.SignalPacker.roundtrip_quality_planar)
    doc = api.SignalPacker.roundtrip_quality_planar.__doc__
    assert "AS GIVEN" in doc and "test_packer_" in doc


@pytest.mark.parametrize("name", ALL)
def test_planar_restatement_equals_the_record(record, pcases, name):
    c, r = pcases[name], record[name]
    O, D = pp.planar_of(c)
    assert O.shape == D.shape == (c["nch"], c["ns"]) and O.dtype == np.int32
    p, mse, ref, path, _ = pp.prdn_parts_planar(O, D)
    assert (pc.hexbits(p), pc.hexbits(mse), pc.hexbits(ref), path) == (r["prdn"], r["mse"], r["ref"], r["path"])


INT32 = [c["name"] for c in pc.synthetic_cases() if c["bps"] == 4] + [pc.REF_SEQ["name"]] + [c["name"] for c in pc.lossy_fixtures() if c["bps"] == 4]


@pytest.mark.parametrize("name", INT32)
def test_in_width_identity_of_the_restatements(pcases, name):
    """the planar values cut to bps 1, 2, 3: the native restatement at that width == the planar restatement on the cut matrix"""
    c = pcases[name]
    O, D = pp.planar_of(c)
    for bps in (1, 2, 3):
        Oc, Dc = pp.cut(O, bps), pp.cut(D, bps)
        native = pc.prdn_parts(pl.cc.i32_to_native(Oc, bps), pl.cc.i32_to_native(Dc, bps), bps, c["nch"], c["ns"])
        planar = pp.prdn_parts_planar(Oc, Dc)
        assert [pc.bits(x) for x in native[:3]] + [native[3]] == [pc.bits(x) for x in planar[:3]] + [planar[3]], (name, bps)


def test_the_shapes_straddle_the_hosts_thresholds():
    pp.check_threshold_shapes()
    got = {(nch, ns, nb, a, b) for nch, ns, nb, a, b in _grid()}
    assert got == set(itertools.product(pp.GRID_NCH, pp.GRID_NS, pp.GRID_NBLOCKS, pp.OFFSETS, pp.OFFSETS)) and len(got) == 4 * 16 * 2 * 16
    host = open(os.path.join(ROOT, "rspt_amd", "csrc", "host_stages.hip")).read()
    body = host[host.index("int rspt_hip_prdn_planar_batch_dev"):]
    body = body[:body.index("\n}\n")]
    assert "kQpFusedMinUnits" in body and "kQpFusedMaxNs" in body and "kQpRowRegs" in body and "kQpWaveRow" in body
    assert not re.search(r"[<>=]=?\s*\d{3,}", body), "a threshold of the form choice is a literal"


def test_no_new_kernel_uses_scratch(asm):
    names = [n for n in asm if re.search(r"\d+k_qp_(sums|accum|rows|seq)", n)]
    kinds = {re.search(r"k_qp_[a-z]+", n).group(0) for n in names}
    assert {"k_qp_sums", "k_qp_accum", "k_qp_seq"} <= kinds, names
    df.uses_no_scratch(asm, names)


# ---- GPU ----

def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _at(P, off):
    """the matrix P on the device at `off` bytes behind a 16-byte boundary (torch's allocations are 256-byte aligned)"""
    import torch

    buf = torch.empty(P.size + 8, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off // 4: off // 4 + P.size].view(P.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(P)))
    assert v.data_ptr() % 16 == off
    return v


def _got(parts):
    """(prdn, mse, ref, path) of a call -> comparable tuples of lists, behind a synchronisation"""
    import torch

    torch.cuda.synchronize()
    p, mse, ref, path = parts
    return _u64(p).tolist(), _u64(mse).tolist(), _u64(ref).tolist(), path.cpu().tolist()


def _want(O, D):
    return tuple(x.tolist() for x in pp.want_bits(O, D))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_gpu_equals_the_record(api, record, pcases, name):
    c, r = pcases[name], record[name]
    O, D = pp.planar_of(c)
    pk = api.new_hzr(4, c["nch"], c["ns"])
    p, mse, ref, path = _got(pk.prdn_planar_batch(_t(O[None]), _t(D[None]), parts=True))
    got = ("%016x" % p[0], "%016x" % mse[0], "%016x" % ref[0], path[0])
    print(name, got)
    assert got == (r["prdn"], r["mse"], r["ref"], r["path"])
    pk.close()


def _grid():
    for nch in pp.GRID_NCH:
        for ns in pp.GRID_NS:
            for nb in pp.GRID_NBLOCKS:
                for a in pp.OFFSETS:
                    for b in pp.OFFSETS:
                        yield nch, ns, nb, a, b


@pytest.mark.gpu
@pytest.mark.parametrize("nch", pp.GRID_NCH)
def test_gpu_row_geometry(api, nch):
    """every ns and nblocks of the grid with d_orig and d_dec at every offset from a 16-byte boundary, independently"""
    import torch

    for ns in pp.GRID_NS:
        pk = api.new_hzr(4, nch, ns)
        for nb in pp.GRID_NBLOCKS:
            O, D = pp.values(nb, nch, ns, 7000 + 100 * nch + nb)
            want = _want(O, D)
            runs = []
            for a in pp.OFFSETS:
                dO = _at(O, a)
                for b in pp.OFFSETS:
                    runs.append((a, b, pk.prdn_planar_batch(dO, _at(D, b), parts=True)))
            for a, b, parts in runs:
                assert _got(parts) == want, (nch, ns, nb, a, b)
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", pp.THRESHOLD_SHAPES, ids=["%dx(%dx%d)" % s for s in pp.THRESHOLD_SHAPES])
def test_gpu_both_sides_of_every_threshold(api, shape):
    nb, nch, ns = shape
    O, D = pp.values(nb, nch, ns, 7700 + ns % 89)
    want = _want(O, D)
    pk = api.new_hzr(4, nch, ns)
    for a, b in pp.THRESHOLD_OFFSETS:
        assert _got(pk.prdn_planar_batch(_at(O, a), _at(D, b), parts=True)) == want, (shape, a, b)
    pk.close()


@pytest.mark.gpu
def test_gpu_width_independence(api):
    """the whole int32 is the sample: handles of bps 1 - 4, one of them big-endian, give the same bytes on values outside the
    narrow widths"""
    nb, nch, ns = 3, 5, 1201
    O, D = pl.noise(nb, nch, ns, 7801), pl.noise(nb, nch, ns, 7802)
    want = _want(O, D)
    dO, dD = _t(O), _t(D)
    for bps in (1, 2, 3, 4):
        pk = api.new_hzr(bps, nch, ns)
        pk.set_byte_order(bps == 3)
        assert _got(pk.prdn_planar_batch(dO, dD, parts=True)) == want, bps
        pk.close()


@pytest.mark.gpu
def test_gpu_one_buffer_for_both(api, pcases):
    for name in ("rand5x333_i32", "negsum5x99_i32", "const3x64_same_i32"):
        c = pcases[name]
        O, _ = pp.planar_of(c)
        want = pp.prdn_parts_planar(O, O)
        assert want[1] == 0.0
        dO = _t(O[None])
        pk = api.new_hzr(4, c["nch"], c["ns"])
        p, mse, ref, path = _got(pk.prdn_planar_batch(dO, dO, parts=True))
        assert (p[0], mse[0], ref[0], path[0]) == (pc.bits(want[0]), pc.bits(want[1]), pc.bits(want[2]), want[3]), name
        if name == "rand5x333_i32":
            assert p[0] == 0  # 0.0 on an ordinary block
        pk.close()


@pytest.mark.gpu
def test_gpu_mixed_batch_takes_each_path_where_it_must(api, orc):
    nch, ns, nb = 2, 65536, 6
    o = np.stack([pc._i32(cases.hash_i32(nch * ns, 1800 + b, 40000)) for b in range(nb)])
    d = np.stack([pc._noisy(o[b], 4, nch, ns, 1850 + b, (1 << 28) if b % 2 else 50) for b in range(nb)])
    O = np.stack([pl.cc.native_to_i32(o[b], 4, nch, ns) for b in range(nb)])
    D = np.stack([pl.cc.native_to_i32(d[b], 4, nch, ns) for b in range(nb)])
    want = _want(O, D)
    assert want[3] == [0, 1, 0, 1, 0, 1]
    pk = api.new_hzr(4, nch, ns)
    got = _got(pk.prdn_planar_batch(_t(O), _t(D), parts=True))
    assert got == want
    assert got[0] == [pc.bits(orc.prdn(o[b], d[b], ns, nch, 4)) for b in range(nb)]
    pk.close()


@pytest.mark.gpu
def test_gpu_wide_handle(api):
    """no channel cap: 8193 channels, which the native entry refuses"""
    import torch

    nb, nch, ns = 2, 8193, 16
    O, D = pp.values(nb, nch, ns, 7901)
    pk = api.new_hzr(4, nch, ns)
    assert _got(pk.prdn_planar_batch(_t(O), _t(D), parts=True)) == _want(O, D)
    nat = torch.zeros(nb * pk.block_bytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros(nb, dtype=torch.float64, device="cuda")
    assert api.lib().rspt_hip_prdn_batch_dev(pk._h, nat.data_ptr(), nat.data_ptr(), nb, out.data_ptr(), None, None, None, None) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch,ns", [(12, 512), (5, 4099), (64, 256)])
def test_gpu_identity_with_the_native_entry(api, nch, ns):
    nb = 3
    for bps in (2, 3, 4):
        O = pp.cut(pl.noise(nb, nch, ns, 8000 + bps), bps)
        D = pp.cut((O.astype(np.int64) + cases.hash_i32(O.size, 8010 + bps, 30).astype(np.int64).reshape(O.shape)).astype(np.int32), bps)
        pk = api.new_hzr(bps, nch, ns)
        dO, dD = _t(O), _t(D)
        planar = _got(pk.prdn_planar_batch(dO, dD, parts=True))
        native = _got(pk.prdn_batch(pk.from_planar_i32(dO).reshape(-1), pk.from_planar_i32(dD).reshape(-1), parts=True))
        assert planar == native, (nch, ns, bps)
        assert planar == _want(O, D)
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in pc.SEQ_WIDTH_CASES])
def test_gpu_identity_with_the_native_entry_on_flagged_blocks(api, name):
    """the narrow sequential cases (tests/prdn_cases.py) as int32 matrices, on and off a 16-byte boundary: k_qp_seq gives the four
    words k_q_seq gives at the case's own width, which are the restatement's"""
    import torch

    c = pc.seq_width_case(name)
    O, D = pp.planar_of(c)
    w = pc.prdn_parts(c["orig"], c["dec"], c["bps"], c["nch"], c["ns"])
    want = ([pc.bits(w[0])], [pc.bits(w[1])], [pc.bits(w[2])], [w[3]])
    assert w[3] == 1 and want == _want(O[None], D[None])
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    o, d = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("orig", "dec"))
    assert _got(pk.prdn_batch(o, d, parts=True)) == want
    for off in (0, 4):
        assert _got(pk.prdn_planar_batch(_at(O[None], off), _at(D[None], off), parts=True)) == want, off
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nch,ns", [("hadamard",) + s for s in pl.HADAMARD_SHAPES[:2]] + [("dct",) + s for s in pl.DCT_SHAPES[:3]])
def test_gpu_round_trip(api, orc, kind, nch, ns):
    import torch

    nb = 2
    for bps in (2, 3, 4):
        P = pl.walk(nb, nch, ns, bps, pl.seed_of(kind, bps, nch, ns))  # in width
        pk, pn = (api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind]) for _ in range(2))
        dP = _t(P)
        q, cr = pk.roundtrip_quality_planar(dP)
        qn, crn = pn.roundtrip_quality(pn.from_planar_i32(dP))
        torch.cuda.synchronize()
        assert torch.equal(dP, _t(P))
        assert _u64(q).tolist() == _u64(qn).tolist() and _u64(cr).tolist() == _u64(crn).tolist(), (kind, bps)
        po = orc.packer(kind, bps, nch, ns, NB_CTOR[kind])
        want, want_cr = [], []
        for b in range(nb):
            native = pl.cc.i32_to_native(P[b], bps)
            s = po.compress(native)
            dec, used, rc = po.decompress(s)
            assert rc == 0
            want.append(pc.bits(orc.prdn(native, np.frombuffer(dec, dtype=np.uint8), ns, nch, bps)))
            want_cr.append(float(native.size) / len(s))
        po.close()
        assert _u64(q).tolist() == want, (kind, bps)
        # (cr is torch's float64 division on the device: faithfully rounded, so within one ulp of the host's quotient)
        assert all(abs(g - w) <= 2.0 ** -52 * w for g, w in zip(cr.cpu().tolist(), want_cr)), (cr.cpu().tolist(), want_cr)
        pk.close()
        pn.close()


@pytest.mark.gpu
def test_gpu_stream_order_and_determinism(api, orc):
    """queued behind decompress_planar_batch on one stream without a synchronisation; launched again; after a call with another
    nblocks; after a native prdn_batch on the same handle (one scratch): identical bytes each time"""
    import torch

    from rspt_amd import synth

    nb, nch, ns = 24, 12, 8192
    src = synth.synth_batch_native(nb, nch, ns, device="cuda")
    pk = api.new_dct(4, nch, ns)
    P = pk.to_planar_i32(src)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_dst, _ = pk.compress_planar_batch(P)
        d_out, _ = pk.decompress_planar_batch(d_dst, nb, d_dst.shape[1])
        queued = pk.prdn_planar_batch(P, d_out, parts=True)  # no synchronisation since the decompress
    s.synchronize()
    torch.cuda.synchronize()
    after = pk.prdn_planar_batch(P, d_out, parts=True)
    torch.cuda.synchronize()
    small = pk.prdn_planar_batch(P[:5], P[:5], parts=True)  # another nblocks, other values in the scratch
    again = pk.prdn_planar_batch(P, d_out, parts=True)
    native = pk.prdn_batch(src.reshape(-1), pk.from_planar_i32(d_out).reshape(-1), parts=True)  # the same scratch
    shared = pk.prdn_planar_batch(P, d_out, parts=True)
    torch.cuda.synchronize()
    assert _u64(small[0]).tolist() == [0] * 5
    for a, b, c, d, e in zip(queued, after, again, native, shared):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and torch.equal(a, e)
    o, dd = src.cpu().numpy().reshape(nb, -1), pk.from_planar_i32(d_out).cpu().numpy().reshape(nb, -1)
    assert _u64(queued[0]).tolist() == [pc.bits(orc.prdn(o[b], dd[b], ns, nch, 4)) for b in range(nb)]
    pk.close()


@pytest.mark.gpu
def test_gpu_abi_refusals(api):
    import torch

    nch, ns = 3, 100
    pk, raw = api.new_hzr(4, nch, ns), api.new_bytes(4096)
    L, h = api.lib(), pk._h
    buf = torch.zeros(2 * nch * ns + 8, dtype=torch.int32, device="cuda")
    out = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    o, f = buf.data_ptr(), getattr(L, ENTRY)
    call = lambda hh, *a: f(hh, *a, None, None, None, None)  # noqa: E731
    assert call(None, o, o, 1, out.data_ptr()) == ERR_ARG
    assert call(h, o, o, 0, out.data_ptr()) == ERR_ARG
    assert call(h, None, o, 1, out.data_ptr()) == ERR_ARG
    assert call(h, o, None, 1, out.data_ptr()) == ERR_ARG
    assert call(h, o, o, 1, None) == ERR_ARG
    assert call(h, o, o, (1 << 31) // 3 + 1, out.data_ptr()) == ERR_ARG  # nblocks * nch >= 2^31
    assert call(h, o, o, 65536, out.data_ptr()) == ERR_ARG               # as rspt_hip_reserve
    assert call(h, o + 2, o, 1, out.data_ptr()) == ERR_ARG               # a misaligned d_orig
    assert call(h, o, o + 1, 1, out.data_ptr()) == ERR_ARG               # a misaligned d_dec
    assert call(raw._h, o, o, 1, out.data_ptr()) == ERR_ARG              # a byte buffer has no samples
    pk.feed_begin(1, 2)
    assert call(h, o, o, 1, out.data_ptr()) == ERR_ARG                   # an open feed owns the workspace
    pk.feed_end()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0, 7.0]  # a refused call writes nothing
    assert call(h, o + 4, o + 12, 2, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert _u64(out).tolist() == [pc.NAN_BITS] * 2  # zeros against zeros: 0 / 0
    pk.close()
    raw.close()
