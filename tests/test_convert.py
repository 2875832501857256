"""The native <-> int32 converter stages (rspt_hip_native_to_i32_batch_dev, rspt_hip_i32_to_native_batch_dev).

Without a GPU: the record of the compiled reference (tests/golden/convert_record.json) regenerates byte for byte where
oracle/_ref exists, the numpy model of tests/convert_cases.py equals it, the CPU oracle's streams of the wide blocks match the
recorded hashes, and a NULL handle is refused before a device is looked for.
On the GPU: both stages against the model (which the record pins to the reference) over narrow and wide handles, ragged ns,
every sample width and byte order, odd addresses, a foreign stream, the round trips, and every refusal.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cases
import convert_cases as cc
from devframe import ERR_ARG, ERR_UNSUPPORTED, ROOT

RECORD = os.path.join(ROOT, "tests", "golden", "convert_record.json")


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_record_regenerates_from_the_reference(orc):
    from oracle import oracle

    if not oracle.have_ref():
        pytest.skip("no oracle/_ref (the compiled reference) on this machine")
    ref = oracle.Ref()

    class Backend:
        native_to_i32 = staticmethod(lambda native, ns, nch, bps, rev: ref.native_to_i32(native, ns, nch, bps, rev))
        i32_to_native = staticmethod(lambda planar, bps, rev: ref.i32_to_native(planar, bps, rev))

        @staticmethod
        def pack(kind, bps, nch, ns, nb, data):
            pk = ref.packer(kind, bps, nch, ns, nb)
            s = pk.compress(data)
            pk.close()
            return s

    text = cc.dump_record(cc.record_cases(Backend, orc.fnv1a))
    with open(RECORD) as f:
        assert f.read() == text


def test_model_equals_the_record(orc, record):
    by_name = {e["name"]: e for e in record["cases"]}
    C_ = cc.converter_cases()
    assert len(C_) + len(cc.WIDE_PACKER_CASES) == len(record["cases"])
    for c in C_:
        e = by_name[c["name"]]
        y = cc.model_output(c, cc.case_input(c))
        assert (y.size, orc.fnv1a(y)) == (e["size"], e["fnv1a"]), c["name"]
        if "hex" in e:
            assert y.tobytes().hex() == e["hex"], c["name"]
            assert cc.fnv1a(y) == e["fnv1a"]  # (the oracle's hash is the plain 32-bit FNV-1a)


def test_model_round_trips():
    for nch, ns in ((3, 17), (12, 64)):
        for bps in (1, 2, 3, 4):
            for be in (False, True):
                x = cc.native_input(nch, ns, bps, 77)
                p = cc.native_to_i32(x, bps, nch, ns, be)
                assert np.array_equal(cc.i32_to_native(p, bps, be), x)
                y = cc.planar_input(nch, ns, 78)
                assert np.array_equal(cc.native_to_i32(cc.i32_to_native(y, bps, be), bps, nch, ns, be), cc.sign_extend(y, bps))
    # negative values at every width, and one-byte samples have no byte order
    assert cc.native_to_i32(np.array([0xFF, 0xFF, 0x7F], dtype=np.uint8), 3, 1, 1)[0, 0] == 0x7FFFFF
    assert cc.native_to_i32(np.array([0xFF, 0xFF, 0x7F], dtype=np.uint8), 3, 1, 1, True)[0, 0] == -129
    assert cc.native_to_i32(np.array([0x80], dtype=np.uint8), 1, 1, 1, True)[0, 0] == -128


def test_oracle_streams_of_wide_blocks_match_the_record(orc, record):
    by_name = {e["name"]: e for e in record["cases"]}
    for c in cc.WIDE_PACKER_CASES:
        pk = orc.packer(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
        data = cc.wide_packer_input(c)
        s = pk.compress(data)
        e = by_name[c["name"]]
        assert (len(s), orc.fnv1a(s)) == (e["size"], e["fnv1a"]), c["name"]
        if c["kind"] in ("hzr", "xdelta_hzr"):
            dec, used, rc = pk.decompress(s)
            assert rc == 0 and used == len(s) and dec == data.tobytes(), c["name"]
        pk.close()


def test_null_handle_is_refused_without_a_device():
    from rspt_amd import api

    L = api.lib()
    buf = np.zeros(64, dtype=np.uint8)
    assert L.rspt_hip_native_to_i32_batch_dev(None, buf.ctypes.data, buf.ctypes.data, 1, None) == ERR_ARG
    assert L.rspt_hip_i32_to_native_batch_dev(None, buf.ctypes.data, buf.ctypes.data, 1, None) == ERR_ARG


# ---- GPU ------------------------------------------------------------------------------------------------------------------
NCH = (1, 3, 12, 64, 1000, 8191, 8192, 8193, 20000, 65535)
NS = (1, 17, 63, 64, 65, 4097)
NUMPY_LIMIT = 1 << 21  # samples of a batch the numpy model checks; larger batches are checked by the torch restatement below


def t_native_to_i32(x, bps, nch, ns, be):
    """the model in torch (for the batches too large for numpy in a test): x uint8 [nblocks, ns * nch * bps]"""
    import torch

    a = x.reshape(-1, ns, nch, bps).to(torch.int32)
    if be and bps > 1:
        a = a.flip(-1)
    u = torch.zeros(a.shape[:-1], dtype=torch.int32, device=x.device)
    for k in range(bps):
        u |= a[..., k] << (8 * k)
    sh = 32 - 8 * bps
    return ((u << sh) >> sh).transpose(1, 2).contiguous()


def t_i32_to_native(p, bps, be):
    import torch

    u = p.transpose(1, 2).contiguous()  # [nblocks, ns, nch]
    b = torch.stack([((u >> (8 * k)) & 0xFF).to(torch.uint8) for k in range(bps)], dim=-1)
    if be and bps > 1:
        b = b.flip(-1)
    return b.reshape(p.shape[0], -1).contiguous()


def _rand_u8(n, seed, device="cuda"):
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device=device, generator=g)


def _rand_i32(n, seed, device="cuda"):
    return _rand_u8(4 * n, seed, device).view(__import__("torch").int32)


def _check_pair(pk, bps, nch, ns, be, nblocks, seed, off=0, stream=None):
    """both stages of one handle on a random batch against the model; off: the native buffers start off bytes past alignment"""
    import torch

    bb = bps * nch * ns
    small = nblocks * nch * ns <= NUMPY_LIMIT
    raw = _rand_u8(nblocks * bb + 16, seed)
    x = raw[off: off + nblocks * bb]
    got = pk.to_planar_i32(x, stream=stream)
    y = _rand_i32(nblocks * nch * ns, seed + 1).reshape(nblocks, nch, ns)
    out_raw = torch.full((nblocks * bb + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    back = pk.from_planar_i32(y, d_out=out_raw[off: off + nblocks * bb], stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    else:
        torch.cuda.current_stream().synchronize()
    assert got.shape == (nblocks, nch, ns) and got.dtype == torch.int32
    if small:
        xh, yh = x.cpu().numpy().reshape(nblocks, bb), y.cpu().numpy()
        want = np.stack([cc.native_to_i32(xh[b], bps, nch, ns, be) for b in range(nblocks)])
        assert np.array_equal(got.cpu().numpy(), want)
        wantn = np.stack([cc.i32_to_native(yh[b], bps, be) for b in range(nblocks)]).reshape(-1)
        assert np.array_equal(back.cpu().numpy().reshape(-1), wantn)
    else:
        assert torch.equal(got, t_native_to_i32(x.reshape(nblocks, bb), bps, nch, ns, be))
        assert torch.equal(back.reshape(nblocks, bb), t_i32_to_native(y, bps, be))
    # nothing outside the output is written
    assert bool((out_raw[:off] == 0xA5).all()) and bool((out_raw[off + nblocks * bb:] == 0xA5).all())


@pytest.mark.gpu
def test_torch_restatement_equals_the_numpy_model():
    import torch

    for bps in (1, 2, 3, 4):
        for be in (False, True):
            nch, ns, nb = 5, 19, 2
            x = _rand_u8(nb * bps * nch * ns, 9)
            xh = x.cpu().numpy().reshape(nb, -1)
            want = np.stack([cc.native_to_i32(xh[b], bps, nch, ns, be) for b in range(nb)])
            assert np.array_equal(t_native_to_i32(x.reshape(nb, -1), bps, nch, ns, be).cpu().numpy(), want)
            y = _rand_i32(nb * nch * ns, 10).reshape(nb, nch, ns)
            wantn = np.stack([cc.i32_to_native(y[b].cpu().numpy(), bps, be) for b in range(nb)])
            assert np.array_equal(t_i32_to_native(y, bps, be).cpu().numpy(), wantn)
    assert torch.cuda.is_available()


@pytest.mark.gpu
def test_record_cases_on_the_gpu(orc, record):
    """every converter case of the record: the GPU's bytes have the reference's size and hash"""
    import torch

    from rspt_amd import api

    by_name = {e["name"]: e for e in record["cases"]}
    for c in cc.converter_cases():
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        pk.set_byte_order(bool(c["be"]))
        x = cc.case_input(c)
        if c["dir"] == "n2i":
            y = pk.to_planar_i32(torch.from_numpy(x.copy()).cuda())
        else:
            y = pk.from_planar_i32(torch.from_numpy(x.copy()).cuda().reshape(1, c["nch"], c["ns"]))
        torch.cuda.synchronize()
        yb = y.cpu().numpy().view(np.uint8).reshape(-1)
        e = by_name[c["name"]]
        assert (yb.size, orc.fnv1a(yb)) == (e["size"], e["fnv1a"]), c["name"]
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch", NCH)
def test_converters_against_the_model(nch):
    from rspt_amd import api

    kinds = ("hzr", "xdelta_hzr", "dct", "hadamard")
    k = 0
    for ns in NS:
        for bps in (1, 2, 3, 4):  # the whole grid at every (nch, ns): batches beyond NUMPY_LIMIT are checked by the torch restatement
            for be in (False, True):
                k += 1
                kind = kinds[k % 4] if (ns & (ns - 1)) == 0 else kinds[k % 3]  # (hadamard needs ns = 2^k)
                pk = api.SignalPacker(kind, bps, nch, ns, 3)
                pk.set_byte_order(be)
                _check_pair(pk, bps, nch, ns, be, 2, 100 * k + nch % 89)
                pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch,ns", [(3, 65), (12, 64), (64, 4097), (1000, 17), (8193, 63), (20000, 5)])
def test_unaligned_native_buffers(nch, ns):
    from rspt_amd import api

    for bps in (1, 2, 3, 4):
        for off in (1, 2, 3):
            be = bool((off + bps) & 1)
            pk = api.new_xdelta_hzr(bps, nch, ns, 3)
            pk.set_byte_order(be)
            _check_pair(pk, bps, nch, ns, be, 3, 7000 + 10 * bps + off, off=off)
            pk.close()


@pytest.mark.gpu
def test_foreign_stream():
    import torch

    from rspt_amd import api

    s = torch.cuda.Stream()
    for bps, nch, ns in ((4, 12, 8192), (3, 8193, 65), (2, 64, 257)):
        pk = api.new_hzr(bps, nch, ns)
        torch.cuda.synchronize()
        _check_pair(pk, bps, nch, ns, False, 2, 8100 + nch, stream=s.cuda_stream)
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["xdelta_hzr", "hzr"])
def test_planar_view_of_a_decoded_batch(kind):
    """to_planar_i32(decompress_batch(compress_batch(x))) == to_planar_i32(x) for the lossless packers, narrow and wide"""
    import torch

    from rspt_amd import api

    for bps, nch, ns, be in ((4, 12, 8192, False), (3, 3, 1000, True), (2, 8193, 16, False), (4, 12000, 16, True)):
        pk = api.SignalPacker(kind, bps, nch, ns, 3)
        pk.set_byte_order(be)
        x = np.stack([cc.wide_block(bps, nch, ns, 40 + b) for b in range(3)])
        if be:
            x = np.stack([cases.reverse_samples(r, bps) for r in x])
        d = torch.from_numpy(x).cuda()
        d_dst, d_sizes = pk.compress_batch(d)
        d_out, d_used = pk.decompress_batch(d_dst, 3, d_dst.shape[1])
        a, b = pk.to_planar_i32(d_out), pk.to_planar_i32(d)
        torch.cuda.synchronize()
        assert torch.equal(d_used, d_sizes) and torch.equal(a, b)
        want = np.stack([cc.native_to_i32(r, bps, nch, ns, be) for r in x])
        assert np.array_equal(a.cpu().numpy(), want)
        pk.close()


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    import torch

    from rspt_amd import api

    L = api.lib()
    bps, nch, ns = 3, 12, 65
    pk = api.new_hzr(bps, nch, ns)
    nb = 2
    native = torch.full((nb * pk.block_bytes + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    planar = torch.full((nb * nch * ns + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n, p = native.data_ptr(), planar.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    fwd, inv = L.rspt_hip_native_to_i32_batch_dev, L.rspt_hip_i32_to_native_batch_dev
    h = pk._h
    calls = [
        (fwd, (h, None, p, nb, st)), (fwd, (h, n, None, nb, st)), (inv, (h, None, n, nb, st)), (inv, (h, p, None, nb, st)),
        (fwd, (h, n, p, 0, st)), (inv, (h, p, n, 0, st)),
        (fwd, (h, n, p + 1, nb, st)), (fwd, (h, n, p + 2, nb, st)), (inv, (h, p + 3, n, nb, st)),  # d_planar off its 4-byte alignment
        (fwd, (h, n, p, 65536, st)), (inv, (h, p, n, 65536, st)),  # more blocks than a grid holds
    ]
    for f, a in calls:
        assert f(*a) == ERR_ARG, a[1:4]
    # overlap: the planar matrix inside the native batch, and the other way round
    both = torch.full((nb * pk.block_bytes + nb * nch * ns * 4,), 0x5A, dtype=torch.uint8, device="cuda")
    b0 = both.data_ptr()
    assert b0 % 4 == 0
    assert fwd(h, b0, b0 + 4 * ((nb * pk.block_bytes) // 4 - 1), nb, st) == ERR_ARG
    assert inv(h, b0, b0 + 4 * nb * nch * ns - 1, nb, st) == ERR_ARG
    assert fwd(h, b0, b0, nb, st) == ERR_ARG and inv(h, b0, b0, nb, st) == ERR_ARG
    # nblocks * nch >= 2^31 on the widest handle
    wide = api.new_hzr(1, 65535, 1)
    assert fwd(wide._h, n, p, 32769, st) == ERR_ARG and inv(wide._h, p, n, 32769, st) == ERR_ARG
    wide.close()
    torch.cuda.synchronize()
    assert bool((native == 0x5A).all()) and bool((planar == 0x5A5A5A5A).all()) and bool((both == 0x5A).all())
    # and a valid call still works on the same handle
    _check_pair(pk, bps, nch, ns, False, nb, 1)
    pk.close()


@pytest.mark.gpu
def test_create_limit_is_the_references():
    from rspt_amd import api

    pk = api.new_hzr(1, 65535, 2)
    pk.close()
    with pytest.raises(api.RsptHipError) as e:
        api.new_hzr(1, 65536, 2)
    assert e.value.status == ERR_UNSUPPORTED
