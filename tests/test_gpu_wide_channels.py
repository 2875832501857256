"""Handles of more than 8192 channels: the four packers up to the reference's own limit of 65535 channels,
and the stages that stay behind at 8191.

k_planar_native keeps one row of all channels in LDS, which ended create at 8192 channels; decompress now ends in k_wide_native
there.  Every stream is compared byte for byte with the CPU oracle (which tests/test_convert.py pins to the compiled reference's
recorded hashes for these block generators), every decoded block with the oracle's.
"""

import numpy as np
import pytest

import cases
import convert_cases as cc
import devframe as df
from devframe import ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

KINDS = ("xdelta_hzr", "hzr", "dct", "hadamard")
NB = {"xdelta_hzr": 3, "hzr": 4, "dct": 2, "hadamard": 3}
NCH = (8192, 8193, 12000, 65535)


def _ns(nch):
    return 8 if nch == 65535 else 16


def _batch(bps, nch, ns, n, seed):
    return np.stack([cc.wide_block(bps, nch, ns, seed + b) for b in range(n)])


@pytest.mark.parametrize("nch", NCH)
@pytest.mark.parametrize("kind", KINDS)
def test_wide_packer_batches(orc, kind, nch):
    """compress_batch / decompress_batch, the container path and the host-pointer calls, bps 1 - 4, both byte orders"""
    import torch

    from rspt_amd import api

    ns, n = _ns(nch), 3
    for bps in (1, 2, 3, 4):
        x = _batch(bps, nch, ns, n, 300 + bps)
        po = orc.packer(kind, bps, nch, ns, NB[kind])
        want = [po.compress(x[b]) for b in range(n)]
        assert kind != "xdelta_hzr" or orc.packer_nb(po) == NB[kind]  # (these blocks never escalate: one nb for the whole batch)
        dec_want = []
        for b in range(n):
            dec, used, rc = po.decompress(want[b])
            assert rc == 0 and used == len(want[b])
            dec_want.append(dec)
        for be in (False, True):
            pk = api.SignalPacker(kind, bps, nch, ns, NB[kind])
            pk.set_byte_order(be)
            xin = np.stack([cases.reverse_samples(r, bps) for r in x]) if be and bps > 1 else x
            d = torch.from_numpy(xin).cuda()
            d_dst, d_sizes = pk.compress_batch(d)
            torch.cuda.synchronize()
            sizes = d_sizes.cpu().numpy()
            for b in range(n):
                got = d_dst[b, : int(sizes[b])].cpu().numpy().tobytes()
                assert got == want[b], (kind, nch, bps, be, b, len(got), len(want[b]))
            d_out, d_used = pk.decompress_batch(d_dst, n, d_dst.shape[1])
            # the container path
            d_packed, d_total = pk.pack_batch(d_dst, d_sizes)
            d_out2, d_used2 = pk.decompress_packed(d_packed)
            torch.cuda.synchronize()
            assert np.array_equal(d_used.cpu().numpy(), sizes) and np.array_equal(d_used2.cpu().numpy(), sizes)
            assert torch.equal(d_out, d_out2)
            for b in range(n):
                w = np.frombuffer(dec_want[b], dtype=np.uint8)
                if be and bps > 1:
                    w = cases.reverse_samples(w, bps)
                assert np.array_equal(d_out[b].cpu().numpy(), w), (kind, nch, bps, be, b)
            if kind in ("xdelta_hzr", "hzr"):
                assert torch.equal(d_out, d)
            pk.close()
        po.close()


@pytest.mark.parametrize("kind", KINDS)
def test_wide_host_pointer_calls(orc, kind):
    from rspt_amd import api

    for nch, bps, be in ((8193, 4, False), (8193, 3, True), (65535, 2, False), (12000, 1, False)):
        ns = _ns(nch)
        x = cc.wide_block(bps, nch, ns, 500 + bps)
        po = orc.packer(kind, bps, nch, ns, NB[kind])
        want = po.compress(x)
        dec_want, used_want, rc = po.decompress(want)
        assert rc == 0
        pk = api.SignalPacker(kind, bps, nch, ns, NB[kind])
        pk.set_byte_order(be)
        xin = cases.reverse_samples(x, bps) if be and bps > 1 else x
        got = pk.compress(xin)
        assert got == want, (kind, nch, bps, be, len(got), len(want))
        dec, used = pk.decompress(got)
        w = np.frombuffer(dec_want, dtype=np.uint8)
        if be and bps > 1:
            w = cases.reverse_samples(w, bps)
        assert used == used_want and np.array_equal(np.frombuffer(dec, dtype=np.uint8), w), (kind, nch, bps, be)
        pk.close()
        po.close()


def test_wide_streams_have_the_references_hashes(orc):
    """the recorded cases: size and FNV-1a of the compiled reference's own streams"""
    import torch

    from rspt_amd import api

    by_name = {e["name"]: e for e in df.golden("convert_record.json")["cases"]}
    for c in cc.WIDE_PACKER_CASES:
        pk = api.SignalPacker(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
        d = torch.from_numpy(cc.wide_packer_input(c)).cuda().reshape(1, -1)
        d_dst, d_sizes = pk.compress_batch(d)
        torch.cuda.synchronize()
        s = d_dst[0, : int(d_sizes[0])].cpu().numpy()
        e = by_name[c["name"]]
        assert (s.size, orc.fnv1a(s)) == (e["size"], e["fnv1a"]), c["name"]
        pk.close()


def test_longer_wide_blocks_round_trip(orc):
    """more than one tile along the time axis, ragged in both directions, every sample width: the inverse's tile edges"""
    import torch

    from rspt_amd import api

    for kind, bps, nch, ns, be in (("hzr", 1, 8193, 130, False), ("xdelta_hzr", 2, 9000, 65, True), ("hzr", 3, 8200, 127, True),
                                   ("xdelta_hzr", 4, 8193, 257, False), ("xdelta_hzr", 4, 8196, 256, True), ("hadamard", 3, 8193, 128, False)):
        x = _batch(bps, nch, ns, 2, 700 + bps)
        po = orc.packer(kind, bps, nch, ns, NB[kind])
        want = [po.compress(x[b]) for b in range(2)]
        dec_want = [po.decompress(s)[0] for s in want]
        pk = api.SignalPacker(kind, bps, nch, ns, NB[kind])
        pk.set_byte_order(be)
        xin = np.stack([cases.reverse_samples(r, bps) for r in x]) if be and bps > 1 else x
        d = torch.from_numpy(xin).cuda()
        d_dst, d_sizes = pk.compress_batch(d)
        d_out, d_used = pk.decompress_batch(d_dst, 2, d_dst.shape[1])
        torch.cuda.synchronize()
        for b in range(2):
            assert d_dst[b, : int(d_sizes[b])].cpu().numpy().tobytes() == want[b], (kind, bps, nch, ns, b)
            w = np.frombuffer(dec_want[b], dtype=np.uint8)
            if be and bps > 1:
                w = cases.reverse_samples(w, bps)
            assert np.array_equal(d_out[b].cpu().numpy(), w), (kind, bps, nch, ns, b)
        pk.close()
        po.close()


def test_stages_refuse_wide_handles():
    """IIR, FIR, median, both peak stages and PRDN are verified up to 8191 channels: beyond, RSPT_HIP_ERR_UNSUPPORTED and nothing runs"""
    import torch

    from rspt_amd import api

    for nch in (8192, 8193):
        pk = api.new_hzr(4, nch, 16)
        d = torch.full((pk.block_bytes,), 0x11, dtype=torch.uint8, device="cuda")
        out = torch.full((pk.block_bytes,), 0x22, dtype=torch.uint8, device="cuda")
        calls = [
            lambda: pk.iir_prefilter_batch(d, [1.0, -0.5], [0.5, 0.5], per_channel=True),
            lambda: pk.iir_prefilter_batch(d, [1.0, -0.5], [0.5, 0.5], per_channel=True, state=pk.iir_state()),
            lambda: pk.fir_prefilter_batch(d, [0.5, 0.5], d_dst=out),
            lambda: pk.fir_prefilter_batch(d, [0.5, 0.5], d_dst=out, state=pk.fir_state(2)),
            lambda: pk.median_filter_batch(d, 3, d_dst=out),
            lambda: pk.median_filter_batch(d, 3, d_dst=out, state=pk.median_state(3)),
            lambda: pk.peak_detect_batch(d, sampling_rate=500.0, max_peaks=4),
            lambda: pk.peak_detect_offline_batch(d, 500.0, max_peaks=4),
            lambda: pk.prdn_batch(d, out),
        ]
        for i, f in enumerate(calls):
            with pytest.raises(api.RsptHipError) as e:
                f()
            assert e.value.status == ERR_UNSUPPORTED, (nch, i, e.value.status)
        torch.cuda.synchronize()
        assert bool((d == 0x11).all()) and bool((out == 0x22).all())
        pk.close()
    # 8191 channels still run
    pk = api.new_hzr(4, 8191, 16)
    d = torch.zeros(pk.block_bytes, dtype=torch.uint8, device="cuda")
    pk.median_filter_batch(d, 3)
    pk.prdn_batch(d, d)
    torch.cuda.synchronize()
    pk.close()
