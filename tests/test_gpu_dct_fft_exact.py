"""The dct's FFT kernels (k_dctr_*, k_idctr_*, k_dctfft_*) held to exact values at every row length they take, 2^4 .. 2^22, in
both directions, and across more blocks than one pass over the FFT scratch holds.

The checker is the long-double reference of tests/dct_fft_cases.py: a coefficient (forward) or decoded sample (inverse) must be
the truncated reference value unless that value lies within 2^14 eps max|v| of a non-zero integer, where it may be one count off.
tests/test_dct_fft_exact_record.py shows on the CPU that the inputs put next to nothing there.  Every test prints, per block, how
many values lay inside the band and how many of those differed.

The host picks the FFT split from k = log2 ns (rspt_hip.hip, rspt_hip_packer_create): complex l1 = ceil(k/2), l2 = floor(k/2)
for k = 4..7 (odd k: a lone last radix-2 stage in both kernels), real lb = 6, la = k - 7 for k = 8..19 (lw = 12 - la down to 0
at k = 19), real la = 12, lb = k - 13 for k = 20..22 (the row-pair group of k_dctr_rows shrinks to R = 16, 8, 4)."""
import numpy as np
import pytest

import dct_fft_cases as dc
import lossy_quantizer_cases as lq
from devframe import api  # noqa: F401

pytestmark = pytest.mark.gpu

SWEEP = {c["name"]: c for c in dc.sweep_cases()}


@pytest.fixture(scope="module")
def compressed(api):
    """name -> the case's blocks through compress_batch, once for the forward and the inverse test"""
    import torch

    done = {}

    def run(name):
        if name not in done:
            c = SWEEP[name]
            xs = [dc.block_i32(c, i) for i in range(c["nblocks"])]
            d_src = torch.from_numpy(np.stack([dc.block_native(c, x) for x in xs])).cuda()
            pk = dc.new_packer(api, c)
            d_dst, d_sizes = pk.compress_batch(d_src)
            torch.cuda.synchronize()
            sizes = [int(n) for n in d_sizes.cpu()]
            streams = [d_dst[i, : sizes[i]].cpu().numpy().tobytes() for i in range(c["nblocks"])]
            done[name] = dict(c=c, pk=pk, xs=xs, d_dst=d_dst, d_sizes=d_sizes, sizes=sizes, streams=streams, coeffs={})
        return done[name]

    yield run
    for r in done.values():
        r["pk"].close()


def _coeffs(orc, r, i):
    if i not in r["coeffs"]:
        r["coeffs"][i] = dc.stream_coeffs(orc, r["streams"][i], r["c"])
    return r["coeffs"][i]


@pytest.mark.parametrize("name", list(SWEEP))
def test_forward_is_the_truncated_reference(api, orc, compressed, name):
    import torch

    r = compressed(name)
    c, pk = r["c"], r["pk"]
    for i, x in enumerate(r["xs"]):
        got, header = _coeffs(orc, r, i)
        v, means = dc.exact_forward(x, c["ns"], c["q"])
        assert header == dc.header_bytes(means), (name, i)
        stats = {}
        share = dc.check_exact(got, v, "%s block %d forward" % (name, i), stats)
        print(name, "forward block", i, stats)
        assert share <= dc.CAP
    if c["planar"]:  # the same blocks as a planar int32 matrix: the native entry's streams byte for byte
        d_planar = torch.from_numpy(np.stack(r["xs"])).cuda()
        d_dst, d_sizes = pk.compress_planar_batch(d_planar)
        torch.cuda.synchronize()
        assert torch.equal(d_sizes, r["d_sizes"])
        for i, n in enumerate(r["sizes"]):
            assert torch.equal(d_dst[i, :n], r["d_dst"][i, :n]), (name, i)


@pytest.mark.parametrize("name", [n for n, c in SWEEP.items() if c["inverse"]])
def test_inverse_is_the_truncated_reference(api, orc, compressed, name):
    """decompress_batch of the GPU's own streams against the long-double inverse of the coefficients those streams hold"""
    import torch

    r = compressed(name)
    c, pk = r["c"], r["pk"]
    d_out, d_used = pk.decompress_batch(r["d_dst"], c["nblocks"], r["d_dst"].shape[1])
    torch.cuda.synchronize()
    assert torch.equal(d_used, r["d_sizes"])
    for i in range(c["nblocks"]):
        coeffs, header = _coeffs(orc, r, i)
        m24 = lq.header_means(header)
        w = dc.exact_inverse(coeffs, m24, c["ns"], c["q"])
        dec = lq.native_to_i32(d_out[i].cpu().numpy(), c["bps"], c["nch"], c["ns"])
        stats = {}
        share = dc.check_exact(dc.decoded_minus_mean(dec, m24), w, "%s block %d inverse" % (name, i), stats)
        print(name, "inverse block", i, stats)
        assert share <= dc.CAP


def test_more_blocks_than_one_pass_over_the_fft_scratch(api, orc):
    """launch_dct_fft takes a batch fft_bpp blocks at a time (the scratch is bounded to 1 GiB); its kernels index the input and
    output by b0 + bl and the scratch by bl.  Six blocks of 16 ch x 2^20 are two passes (four blocks, then two): every stream and
    every decoded block is what a second handle makes of that block alone, from native and from planar, and block 4 -- the first
    of the second pass -- is the truncated reference."""
    import torch

    m = dc.MULTIPASS
    nch, ns, B = m["nch"], 1 << m["k"], m["nblocks"]
    assert B > (1 << 30) / (16 * nch * ns) and m["checked_block"] >= (1 << 30) // (16 * nch * ns)  # more than one pass, whatever the bound becomes
    c = dict(dc.multipass_case(), seed=m["seed"], nblocks=B)
    xs = [dc.block_i32(c, i) for i in range(B)]
    assert (xs[m["checked_block"]] == dc.block_i32(dc.multipass_case(), 0)).all()
    d_planar = torch.from_numpy(np.stack(xs)).cuda()
    many, one = dc.new_packer(api, c), dc.new_packer(api, c)
    d_src = many.from_planar_i32(d_planar)
    d_dst, d_sizes = many.compress_batch(d_src)
    torch.cuda.synchronize()
    sizes = [int(n) for n in d_sizes.cpu()]
    stride = d_dst.shape[1]
    alone = []
    for i in range(B):
        d1, s1 = one.compress_batch(d_src[i:i + 1])
        o1, u1 = one.decompress_batch(d1, 1, d1.shape[1])
        torch.cuda.synchronize()
        assert int(s1[0]) == sizes[i] == int(u1[0]) and torch.equal(d1[0, : sizes[i]], d_dst[i, : sizes[i]]), i
        alone.append(o1[0].clone())
    # block 4 against the long-double reference
    i = m["checked_block"]
    got, header = dc.stream_coeffs(orc, d_dst[i, : sizes[i]].cpu().numpy().tobytes(), c)
    v, means = dc.exact_forward(xs[i], ns, c["q"])
    stats = {}
    assert header == dc.header_bytes(means)
    assert dc.check_exact(got, v, "block %d of %d" % (i, B), stats) <= dc.CAP
    print("multi-pass forward block", i, stats)
    d_out, d_used = many.decompress_batch(d_dst, B, stride)
    torch.cuda.synchronize()
    assert torch.equal(d_used, d_sizes)
    for i in range(B):
        assert torch.equal(d_out[i], alone[i]), i
    # from and to planar
    d_dst2, d_sizes2 = many.compress_planar_batch(d_planar)
    torch.cuda.synchronize()
    assert torch.equal(d_sizes2, d_sizes)
    for i in range(B):
        assert torch.equal(d_dst2[i, : sizes[i]], d_dst[i, : sizes[i]]), i
    d_out2, d_used2 = many.decompress_planar_batch(d_dst2, B, stride)
    d_nat2 = many.from_planar_i32(d_out2)
    torch.cuda.synchronize()
    assert torch.equal(d_used2, d_sizes) and torch.equal(d_nat2, d_out)
    many.close()
    one.close()
