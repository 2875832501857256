"""The IIR pre-filter stage (filter.hip) at its edges: outputs past int32 range, infinities and NaN, and every kernel variant.

The reference truncates each double result with x86-64's conversion (every NaN, +-inf and every value whose truncation does not
fit becomes INT32_MIN) and stores the low bps bytes.  tests/iir_cases.py holds the inputs and a float64 restatement that keeps
the unrounded results; tests/golden/iir_record.json holds the compiled reference's answers in both drivings (one filter for
all channels of a block, one per channel).

CPU: the inputs against the record, the restatement and the oracle against the reference's answers, the claims of the
non-finite cases (class and onset), the variants the record covers, and the record's text reproduced byte for byte.
GPU (-m gpu): rspt_hip_iir_prefilter_batch_dev on every record case in both modes, on batches that spread the blocks over
more than one lane per workgroup, on misaligned bases, and twice back to back with other coefficients."""
import importlib.util
import json
import os

import numpy as np
import pytest

import iir_cases as ic
from cases import digest
from devframe import ROOT, api  # noqa: F401

RECORD = os.path.join(ROOT, "tests", "golden", "iir_record.json")
MODES = ("shared", "per_channel")


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return {r["name"]: r for r in json.load(f)["cases"]}


@pytest.fixture(scope="module")
def icases():
    return {c["name"]: c for c in ic.all_cases()}


NAMES = [c["name"] for c in ic.all_cases()]
EDGE_NAMES = [c["name"] for c in ic.iir_edge_cases()]


def _restated(c, mode):
    return ic.iir_double(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared=mode == "shared")[0]


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    cs = ic.all_cases()
    assert [c["name"] for c in cs] == list(record)
    for c in cs:
        r = record[c["name"]]
        assert (c["bps"], c["nch"], c["ns"], c["init"]) == (r["bps"], r["nch"], r["ns"], r["init"]), c["name"]
        assert ic.to_bits(c["n"]) == r["n"] and ic.to_bits(c["d"]) == r["d"], c["name"]
        assert ic.crc(c["data"]) == r["in_crc32"], c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_and_oracle_match_reference(orc, record, icases, name):
    c, r = icases[name], record[name]
    for mode in MODES:
        y = ic.iir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared=mode == "shared")
        assert digest(y) == r[mode], ("restatement", mode)
        o = orc.iir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared_state=mode == "shared")
        assert digest(o) == r[mode], ("oracle", mode)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_case_holds_the_class_and_onset_it_claims(icases, name):
    """a case whose blow-up has drifted (to all NaN, to all finite, to another chunk) fails here"""
    c = icases[name]
    assert c["claims"], "a non-finite case without a claim"
    ys = {m: ic.classify(_restated(c, m)) for m in MODES}
    for mode, cls, ch, region in c["claims"]:
        s = ic.onset(ys[mode][cls], ch)
        if region is None:
            assert s is None, (mode, cls, ch, s)
        else:
            assert s is not None and ic.in_region(region, s, c["ns"]), (mode, cls, ch, region, s)


def test_non_finite_cases_reach_every_class_in_every_width(icases):
    seen = set()
    for name in EDGE_NAMES:
        c = icases[name]
        for mode in MODES:
            cl = ic.classify(_restated(c, mode))
            seen |= {(c["bps"], k, mode) for k in ic.CLASSES if cl[k].any()}
    assert {(b, k, m) for b in (1, 2, 3, 4) for k in ic.CLASSES for m in MODES} <= seen
    # the int32 NaN onsets sit where the kernels differ: inside a full chunk of k_iir_pipe and in its last one, inside a
    # chunk of k_iir and in its tail -- each in a case that the launch routes to that kernel
    regions = {(ic.kernel_of(icases[n]["ns"], icases[n]["init"], len(icases[n]["n"])), r) for n in EDGE_NAMES for _, k, _, r in icases[n]["claims"]
               if k == "nan" and icases[n]["bps"] == 4}
    assert {("pipe", "pipe_full"), ("pipe", "pipe_tail"), ("iir", "iir_chunk"), ("iir", "iir_tail")} <= regions
    # non-finite coefficients: both NaN signs and both infinities, in n and in d, through both kernels
    coefs = {(n.split("_")[1], n.split("_")[2], n.split("_")[3][:4]) for n in EDGE_NAMES if n.startswith("coef_")}
    assert {(w, v, k) for w in ("n1", "d0", "dlast", "n0") for v in ("nan", "negnan", "inf", "neginf") for k in ("pipe", "iir3")} <= coefs
    neg = [icases[n] for n in EDGE_NAMES if "negnan" in n and not n.startswith("coef_n0")]
    assert neg and all(np.signbit(np.array(c["n"] + c["d"])[np.isnan(c["n"] + c["d"])]).all() for c in neg)


def test_the_record_covers_the_kernel_variants(icases):
    cs = list(icases.values())
    kern = {(len(c["n"]), ic.kernel_of(c["ns"], c["init"], len(c["n"]))) for c in cs}
    assert {(nc, k) for nc in (2, 3, 4, 5) for k in ("iir", "pipe")} <= kern
    # k_iir with a history initialisation (its step_const branch) at every order
    assert {len(c["n"]) for c in cs if ic.kernel_of(c["ns"], c["init"], len(c["n"])) == "iir" and 4 * c["init"] > len(c["n"]) - 1} == {2, 3, 4, 5}
    assert {(len(c["n"]), c["bps"]) for c in cs} >= {(nc, b) for nc in (2, 3, 4, 5) for b in (1, 2, 3, 4)}
    for nc in (2, 3, 4, 5):
        assert {1, nc - 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 232} <= {c["ns"] for c in cs if len(c["n"]) == nc}, nc
    assert {1, 63, 64, 65, 129} <= {c["nch"] for c in cs}
    # 232 = 3 * 64 + 40: the producer set that holds the last sample runs past the channel's end (load_set clamps it)
    assert 232 % ic.CHUNK_PIPE not in (0, 16, 32, 48)
    # full-scale int32 through k_iir_pipe: at every order, outputs past +2^31 inside full chunks (the chunk is redone
    # exactly) and past -2^31
    for nc in (2, 3, 4, 5):
        pos = neg = False
        for c in cs:
            if c["bps"] != 4 or len(c["n"]) != nc or ic.kernel_of(c["ns"], c["init"], nc) != "pipe" or c["name"].startswith(("onset", "ex3", "coef", "ff")):
                continue
            y = _restated(c, "per_channel")
            full = y[: c["ns"] // ic.CHUNK_PIPE * ic.CHUNK_PIPE]
            pos |= bool((np.isfinite(full) & (full >= 2.0 ** 31)).any())
            neg |= bool((np.isfinite(y) & (y <= -2.0 ** 31 - 1)).any())
        assert pos and neg, nc


def test_record_text_is_reproduced_byte_for_byte():
    """make_iir_record.py writes the record from the cases and a driving of the filter; with the restatement (pinned to the
    reference above) in place of the compiled reference it must give the committed file's bytes"""
    spec = importlib.util.spec_from_file_location("make_iir_record", os.path.join(ROOT, "tests", "golden", "make_iir_record.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    text = m.record_text(lambda native, bps, nch, ns, n, d, init: ic.iir_prefilter(native, bps, nch, ns, n, d, init).tobytes())
    with open(RECORD, "rb") as f:
        assert text.encode() == f.read()


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_iir_record_case(api, record, icases, name):
    """every case in both modes, two copies of the block per batch (each block has its own filter objects)"""
    import torch

    c, r = icases[name], record[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for mode in MODES:
        buf = torch.from_numpy(np.stack([c["data"]] * 2)).cuda()
        pk.iir_prefilter_batch(buf, c["n"], c["d"], c["init"], per_channel=mode == "per_channel")
        torch.cuda.synchronize()
        for b in range(2):
            assert digest(buf[b].cpu().numpy()) == r[mode], (mode, b)
    pk.close()


def _oracle_blocks(orc, data, bps, nch, ns, n, d, init, shared):
    bb = bps * nch * ns
    return b"".join(orc.iir_prefilter(data[i * bb : (i + 1) * bb], bps, nch, ns, n, d, init, shared_state=shared)
                    for i in range(data.size // bb))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes_per_wg", [1, 2, 3, 4])
def test_gpu_iir_shared_mode_lanes_per_workgroup(api, orc, lanes_per_wg):
    """shared mode puts ceil(nblocks / CUs) blocks on one workgroup of k_iir_pipe; the count is chosen to give 1 .. 4.  A
    full-scale batch (chunks redone for INT_MAX in some lanes only), then an unstable filter on a batch where one block in
    five blows up (NaN inside full chunks in those lanes only)"""
    import torch

    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nblocks = cu * (lanes_per_wg - 1) + 5
    assert -(-nblocks // cu) == lanes_per_wg
    bps, nch, ns = 4, 2, 256
    pk = api.new_hzr(bps, nch, ns)
    full = np.concatenate([ic.cases._rand_native(nch, ns, bps, 3000 + b, (1 << 31) - 1) for b in range(nblocks)])
    blow = np.concatenate([ic.onset_block(nch, ns, bps, 4000 + b, [None, 60 + b % 50] if b % 5 == 0 else [None, None], 1000) for b in range(nblocks)])
    for data, (n, d), init in ((full, ic.STABLE[2], 1), (blow, ic.unstable(1e3), 2)):
        buf = torch.from_numpy(data).cuda()
        pk.iir_prefilter_batch(buf, n, d, init)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == _oracle_blocks(orc, data, bps, nch, ns, n, d, init, True)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bps,misalign", [(2, 1), (4, 1), (4, 2), (3, 1)])
def test_gpu_iir_misaligned_base(api, orc, bps, misalign):
    """a base address off the sample width: the byte-wise instantiations of k_iir_pipe and k_iir's runtime check"""
    import torch

    for nch, ns, nc, init in ((3, 100, 5, 2), (5, 200, 4, 0), (2, 40, 3, 1)):
        n, d = ic.STABLE[nc]
        data = np.concatenate([ic.cases._rand_native(nch, ns, bps, 5000 + 10 * b + nc, 1 << (8 * bps - 1)) for b in range(3)])
        pk = api.new_hzr(bps, nch, ns)
        raw = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
        for shared in (True, False):
            buf = raw[misalign : misalign + data.size]
            buf.copy_(torch.from_numpy(data))
            pk.iir_prefilter_batch(buf, n, d, init, per_channel=not shared)
            torch.cuda.synchronize()
            assert buf.cpu().numpy().tobytes() == _oracle_blocks(orc, data, bps, nch, ns, n, d, init, shared), (nch, ns, nc, init, shared)
            assert not raw[:misalign].any() and not raw[misalign + data.size :].any()  # nothing written outside the blocks
        pk.close()


@pytest.mark.gpu
def test_gpu_iir_back_to_back_without_host_sync(api, orc):
    """two calls on one stream with other coefficients and no sync between them, the caller's arrays overwritten as soon as
    each call returns: each call filters with its own coefficients"""
    import torch

    bps, nch, ns = 4, 8, 4096
    data = np.concatenate([ic.cases._rand_native(nch, ns, bps, 6000 + b, 1 << 30) for b in range(16)])
    pk = api.new_hzr(bps, nch, ns)
    a = torch.from_numpy(data).cuda()
    b = torch.from_numpy(data[: 2 * bps * nch * ns].copy()).cuda()
    (n1, d1), (n2, d2) = [np.array(x, dtype=np.float64) for x in ic.STABLE[5]], [np.array(x, dtype=np.float64) for x in ic.STABLE[2]]
    want1 = _oracle_blocks(orc, data, bps, nch, ns, n1, d1, 100, True)
    want2 = _oracle_blocks(orc, data[: 2 * bps * nch * ns], bps, nch, ns, n2, d2, 1, False)
    pk.iir_prefilter_batch(a, n1, d1, 100)
    n1[:] = np.nan
    d1[:] = np.nan
    pk.iir_prefilter_batch(b, n2, d2, 1, per_channel=True)
    n2[:] = np.nan
    d2[:] = np.nan
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == want1
    assert b.cpu().numpy().tobytes() == want2
    pk.close()
