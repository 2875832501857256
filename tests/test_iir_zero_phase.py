"""The zero-phase IIR stage: one reference i_filter::new_iir object per (block, channel) run forward and then,
the same object, backward over its own untruncated output, truncated once, on the GPU: rspt_hip_iir_zero_phase_batch_dev.

CPU: the record's inputs, the numpy restatement (tests/iir_zero_phase_cases.py) against the reference's answers
(tests/golden/iir_zero_phase_record.json), what the record covers, that the answer is not two truncating passes of the single
stage, that the backward history counts, the C ABI, the device ISA of the new kernels, and the argument checks that need no
device.
GPU (-m gpu): every case bit-exact against the record and the restatement, base addresses off the sample width, a workspace full
of 0xFF bytes, a repeated call, both kernels on the same data, and the statuses.

These are hand-picked cases: their block lengths put the last sample into three of the pipelined kernel's four producer parts and
take five of the 64 residues mod its chunk.  Every residue, every (order, part, place of the last sample) and every backward
history with every order are covered by the seeded sweep, tests/test_iir_sweep.py (leg zero_phase of tests/iir_sweep_cases.py)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import devframe as df
import iir_cases as ic
import iir_zero_phase_cases as zc
from cases import IIR_BANDPASS, digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_iir_zero_phase_work_bytes", "rspt_hip_iir_zero_phase_batch_dev")
CHUNK = zc.CHUNK

CASES = zc.zero_phase_cases()
NAMES = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def _record():
    return df.golden("iir_zero_phase_record.json")


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case with the record's exact coefficients"""
    i = NAMES.index(name)
    r = _record()["cases"][i]
    assert r["name"] == name
    return zc.with_record_coefficients(CASES[i], r)


@functools.lru_cache(maxsize=None)
def _want(name):
    """the restatement's answer, computed once per process (read-only)"""
    y = zc.filtered(_case(name))
    y.setflags(write=False)
    return y


def _kernel(r):
    return zc.kernel_of(r["ns"], r["init"], len(r["n"]))


# ---- CPU ----

def test_record_inputs_have_not_drifted():
    rec = _record()["cases"]
    assert len(CASES) == len(rec)
    for c, r in zip(CASES, rec):
        assert (c["name"], c["bps"], c["nch"], c["ns"], c["nblocks"]) == (r["name"], r["bps"], r["nch"], r["ns"], r["nblocks"])
        assert zc.crc(c["data"]) == r["in_crc32"], c["name"]
        assert zc.to_record(c) == {k: r[k] for k in ("n", "d", "init", "backward_init")}, c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    c = _case(name)
    y = _want(name)
    assert digest(y) == c["rec"]["digest"] and zc.crc(y) == c["rec"]["crc32"]


def test_the_record_covers_what_it_must():
    rec = _record()["cases"]
    assert {r["ns"] for r in rec} >= {1, 2, 5, CHUNK - 1, CHUNK, CHUNK + 1, 103, 2 * CHUNK + 1, 200}
    assert {r["nch"] for r in rec} >= {1, 3, 64, 65, 130}
    assert {r["bps"] for r in rec} == {1, 2, 3, 4}
    assert {r["nblocks"] for r in rec} >= set(range(1, 8))
    assert {len(r["n"]) for r in rec} == {2, 3, 4, 5}
    assert {r["init"] for r in rec} >= {0, 1, 3, 2000} and {r["backward_init"] for r in rec} >= {0, 1, 2000}
    # every order and every backward history through both kernels; init 0 and 1 (nc >= 3) force the plain kernel at any length
    for kern in ("plain", "pipe"):
        assert {r["backward_init"] for r in rec if _kernel(r) == kern} >= {0, 1, 2000}, kern
    assert {len(r["n"]) for r in rec if _kernel(r) == "pipe"} == {2, 3, 4, 5}
    assert {len(r["n"]) for r in rec if _kernel(r) == "plain"} >= {3, 4, 5}
    assert any(r["ns"] >= CHUNK and r["init"] == 0 for r in rec) and any(r["ns"] >= CHUNK and r["init"] == 1 and len(r["n"]) >= 3 for r in rec)
    assert all(_kernel(r) == "plain" for r in rec if r["init"] == 0 or (r["init"] == 1 and len(r["n"]) >= 3))
    # a partial last chunk on both passes, and whole chunks only
    pipe = [r for r in rec if _kernel(r) == "pipe"]
    assert any(r["ns"] % CHUNK for r in pipe) and any(r["ns"] % CHUNK == 0 for r in pipe)
    # fewer backward steps than the ring is long on the pipelined kernel: forward inputs stay in the x ring behind w[ns-1]
    assert any(0 < 4 * r["backward_init"] < len(r["n"]) for r in pipe)
    # the README's band-pass on both recordings
    readme = [r for r in rec if r["n"] == ic.to_bits(IIR_BANDPASS[0]) and r["d"] == ic.to_bits(IIR_BANDPASS[1])]
    assert {(r["bps"], r["nch"], r["ns"], r["nblocks"]) for r in readme} == {(4, 12, 2048, 16), (3, 3, 1000, 20)}
    assert ic.to_bits(IIR_BANDPASS[0])[1] == ic.to_bits([-3.14332095199])[0]
    assert [r["name"] for r in readme] == list(zc.README_NAMES)
    assert {r["name"] for r in rec} >= set(zc.UNSTABLE_NAMES) | set(zc.SAME_DATA_PAIR)
    assert {_kernel(_case(n)["rec"]) for n in zc.UNSTABLE_NAMES} == {"plain", "pipe"}


@pytest.mark.parametrize("name", zc.UNSTABLE_NAMES)
def test_the_unstable_filter_poisons_the_rings_before_the_turn(name):
    """the forward pass passes 2^31, reaches +-inf and then NaN inside block 0; the backward pass starts from those rings, so
    every output of that channel is NaN (INT32_MIN); the channel that is never fed stays finite"""
    c = _case(name)
    back, fwd = zc.doubles(c)
    ns = c["ns"]
    f1, b1 = fwd[:ns, 1], back[:ns, 1]
    past = np.isfinite(f1) & (np.abs(f1) >= 2.0 ** 31)
    assert past.any() and np.isinf(f1).any() and np.isnan(f1).any()
    assert int(np.argmax(past)) < int(np.argmax(np.isinf(f1))) < int(np.argmax(np.isnan(f1))) < ns - 1
    assert np.isnan(f1[-1]) and np.isnan(b1).all()
    assert np.isfinite(back[:ns, 0]).all()
    got = zc.native_to_i32(_want(name), c["bps"], c["nch"], ns * c["nblocks"])
    assert (got[:ns, 1] == (-(1 << 31) if c["bps"] == 4 else 0)).all()  # the low bps bytes of INT32_MIN


@pytest.mark.parametrize("name", zc.README_NAMES)
def test_zero_phase_is_not_forward_reverse_forward_of_the_single_stage(name):
    """a forward pass, a reversal and another forward pass of the single stage truncate in between and start a fresh object"""
    c = _case(name)
    other = zc.forward_reverse_forward(c)
    assert other.shape == _want(name).shape and not np.array_equal(other, _want(name))


def test_the_backward_history_changes_the_answer():
    c = _case(zc.README_NAMES[1])
    assert c["binit"] == 0
    assert not np.array_equal(_want(c["name"]), zc.filtered(c, binit=1))
    a, b = _case(zc.SAME_DATA_PAIR[1]), _case("ns200_i32_3ch_x4_nc5_init2000_b2000")
    assert not np.array_equal(_want(a["name"]), zc.filtered(a, binit=0)) and not np.array_equal(_want(b["name"]), zc.filtered(b, binit=0))


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries((
        "int rspt_hip_iir_zero_phase_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t* bytes);",
        "int rspt_hip_iir_zero_phase_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients, "
        "int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes, void* stream);",
    ), ENTRIES, methods=("iir_zero_phase_work_bytes", "iir_zero_phase_batch"))


def test_the_zero_phase_kernels_hold_no_fused_multiply_add(asm):
    """k_iir_zp (sample width x order) and k_iir_zp_pipe ((int8, int16 (+aligned), int24, int32 (+aligned)) x order)"""
    plain = [n for n in asm if re.search(r"8k_iir_zpIL", n)]
    pipe = [n for n in asm if re.search(r"13k_iir_zp_pipeIL", n)]
    assert len(plain) == 16, sorted(plain)
    assert len(pipe) == 24, sorted(pipe)
    for n in plain + pipe:
        assert not [ln for ln in asm[n] if df.FUSED_F64_F32.match(ln)], n
        assert [ln for ln in asm[n] if re.match(r"^\s+v_mul_f64\b", ln)], n  # (the recurrence is in there, unfused)


def test_argument_checks_that_need_no_device():
    """a NULL handle and a NULL `bytes` are refused before anything touches a device"""
    from rspt_amd import api

    L = api.lib()
    n = C.c_size_t(12345)
    assert L.rspt_hip_iir_zero_phase_work_bytes(None, 2, C.byref(n)) == ERR_ARG and n.value == 12345
    k = (C.c_double * 3)(1.0, 0.5, 0.25)
    work = C.create_string_buffer(4096)
    wp = (C.addressof(work) + 7) & ~7
    assert L.rspt_hip_iir_zero_phase_batch_dev(None, wp, 1, k, k, 3, 0, 0, wp, 2048, None) == ERR_ARG


# ---- GPU ----

def _run(pk, c, buf=None, work=None):
    """the case's blocks through one call; -> the filtered bytes"""
    import torch

    if buf is None:
        buf = torch.from_numpy(np.array(c["data"], dtype=np.uint8)).cuda()
    pk.iir_zero_phase_batch(buf, c["n"], c["d"], init_nr_samples=c["init"], backward_init_nr_samples=c["binit"], work=work)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_bit_exact(api, name):
    c = _case(name)
    want = _want(name)
    assert digest(want) == c["rec"]["digest"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    got = _run(pk, c)
    assert np.array_equal(got, want) and digest(got) == c["rec"]["digest"]
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns64_i16_130ch_x2_nc2_init1_b1", "ns129_i32_130ch_x2_nc5_init2000_b1", "ns2_i16_65ch_x6_nc5_init3_b1"])
def test_gpu_base_address_off_the_sample_width(api, name):
    """the byte-wise instantiations of the widths that have a whole-sample one (int16 and int32 through the pipelined kernel, int16
    through the plain one): the blocks one byte off any 2- or 4-byte boundary"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    n = c["data"].size
    raw = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    buf = raw[1 : 1 + n]
    buf.copy_(torch.from_numpy(np.array(c["data"])))
    assert buf.data_ptr() % 2 == 1
    assert np.array_equal(_run(pk, c, buf=buf), _want(name))
    assert int(raw[0]) == 0 and int(raw[1 + n :].count_nonzero()) == 0
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns129_i32_130ch_x2_nc5_init2000_b1", "ns103_i32_3ch_x2_nc5_init3_b0_plain", zc.README_NAMES[1]])
def test_gpu_nothing_of_the_workspace_is_read_before_it_is_written(api, name):
    """a workspace of exactly the bound, full of 0xFF bytes (NaNs), gives the same output; the bytes behind it stay as they were"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    nb = pk.iir_zero_phase_work_bytes(c["nblocks"])
    assert nb == (c["nblocks"] * c["nch"] + 63) // 64 * 64 * c["ns"] * 8
    raw = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 8 == 0
    assert np.array_equal(_run(pk, c, work=raw[:nb]), _want(name))
    assert int((raw[nb:] != 0xFF).count_nonzero()) == 0
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns200_i32_3ch_x4_nc5_init2000_b2000", "ns5_i24_1ch_x5_nc4_init0_b2000"])
def test_gpu_a_repeated_call_gives_the_same_output(api, name):
    """the same handle and the same workspace, a fresh copy of the input: nothing of the first call is left for the second"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    work = torch.empty(pk.iir_zero_phase_work_bytes(c["nblocks"]) // 8, dtype=torch.float64, device="cuda")
    first = _run(pk, c, work=work)
    second = _run(pk, c, work=work)
    assert np.array_equal(first, _want(name)) and np.array_equal(second, first)
    pk.close()


@pytest.mark.gpu
def test_gpu_the_plain_and_the_pipelined_kernel_on_the_same_data(api):
    """init below nc - 1 selects the plain kernel, init = nc - 1 the pipelined one; each agrees with the record"""
    a, b = (_case(n) for n in zc.SAME_DATA_PAIR)
    assert np.array_equal(a["data"], b["data"]) and (a["n"], a["d"], a["binit"]) == (b["n"], b["d"], b["binit"])
    assert (_kernel(a["rec"]), _kernel(b["rec"])) == ("plain", "pipe")
    pk = api.new_hzr(a["bps"], a["nch"], a["ns"])
    for c in (a, b):
        got = _run(pk, c)
        assert digest(got) == c["rec"]["digest"] and np.array_equal(got, _want(c["name"])), c["name"]
    pk.close()


@pytest.mark.gpu
def test_gpu_entries_reject_bad_arguments(api):
    import torch

    L = api.lib()
    pk = api.new_hzr(4, 3, 100)
    bb = pk.block_bytes
    # samples that no filter leaves as they are, and a workspace of 0xFF bytes that any launch would overwrite with doubles
    data = torch.from_numpy(np.array(zc.cases._rand_native(3, 200, 4, 7200, 1 << 20), dtype=np.uint8)).cuda()
    buf = data.clone()
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    need = pk.iir_zero_phase_work_bytes(2)
    assert need == 64 * 100 * 8 and pk.iir_zero_phase_work_bytes(22) == 2 * 64 * 100 * 8
    work = torch.full((need + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    nb = C.c_size_t()
    assert L.rspt_hip_iir_zero_phase_work_bytes(h, 2, None) == ERR_ARG
    assert L.rspt_hip_iir_zero_phase_work_bytes(h, 0, C.byref(nb)) == ERR_ARG
    assert L.rspt_hip_iir_zero_phase_work_bytes(h, (1 << 31) // 3 + 1, C.byref(nb)) == ERR_ARG
    NULL = object()
    coef = np.array([1.0, -0.5, 0.1, 0.0, 0.0])
    dcoef = np.array([0.5, 0.25, 0.125, 0.0, 0.0])  # (not the feedback side's values: d = n would be the identity)
    cp, dp = coef.ctypes.data_as(C.POINTER(C.c_double)), dcoef.ctypes.data_as(C.POINTER(C.c_double))

    def call(hh=h, p=buf.data_ptr(), nblocks=2, n=cp, d=dp, nc=3, init=2, binit=0, w=work.data_ptr(), wb=need):
        return L.rspt_hip_iir_zero_phase_batch_dev(hh, p, nblocks, None if n is NULL else n, None if d is NULL else d, nc, init, binit, w, wb, st)

    # everything the single stage refuses
    assert call(p=None) == ERR_ARG and call(n=NULL) == ERR_ARG and call(d=NULL) == ERR_ARG
    assert call(nc=1) == ERR_ARG and call(nc=6) == ERR_ARG
    assert call(init=-1) == ERR_ARG and call(init=(1 << 28) + 1) == ERR_ARG
    assert call(nblocks=0) == ERR_ARG and call(nblocks=(1 << 31) // 3 + 1) == ERR_ARG  # nblocks * nch >= 2^31
    # the backward history and the workspace
    assert call(binit=-1) == ERR_ARG and call(binit=(1 << 28) + 1) == ERR_ARG
    assert call(w=None) == ERR_ARG and call(w=work.data_ptr() + 4) == ERR_ARG
    assert call(wb=need - 1) == ERR_ARG and call(wb=0) == ERR_ARG
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wdata = torch.from_numpy(np.array(zc.cases._rand_native(8192, 4, 1, 7201, 100), dtype=np.uint8)).cuda()
    wbuf = wdata.clone()
    wwork = torch.full((8192 * 4 * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    assert call(hh=wide._h, p=wbuf.data_ptr(), nblocks=1, w=wwork.data_ptr(), wb=wwork.numel()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    # nothing ran: a launch would have filtered the samples and written doubles over the 0xFF bytes
    assert torch.equal(buf, data) and torch.equal(wbuf, wdata)
    assert int((work != 0xFF).count_nonzero()) == 0 and int((wwork != 0xFF).count_nonzero()) == 0
    wide.close()
    # accepted: a workspace of exactly the bound, 8 bytes further on; both kernels; long histories
    assert call(nc=2, init=0, binit=0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, data) and int((work[:need] != 0xFF).count_nonzero()) > 0  # (and a call that runs does show)
    assert int((work[need:] != 0xFF).count_nonzero()) == 0
    assert call(nc=5, init=1 << 14, binit=1 << 14, w=work.data_ptr() + 8) == 0
    torch.cuda.synchronize()
    pk.close()
