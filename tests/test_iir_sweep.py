"""A seeded sweep of the IIR stages over random shapes, orders, histories and cuts (tests/iir_sweep_cases.py): the stateless and
the carried form of the IIR pre-filter and of the cascade, and the zero-phase stage, each through its plain and its pipelined
kernel (k_iir / k_iir_carry / k_iir_pipe, k_iir_cascade / k_iir_cascade_pipe, k_iir_zp / k_iir_zp_pipe).

CPU: the record's inputs (tests/golden/iir_sweep_record.json, the compiled reference's answers), the restatement and the oracle
against the record, and what the generated cases cover -- asserted over the list, so that an edit of the generator cannot hollow
the sweep out.
GPU (-m gpu): one test per leg that loops over its cases.  The output equals the record and the restatement, between two
untouched guards; the zero-phase workspace is exactly its bound, starts as NaNs and sits between guards too; a stream's state is
decoded by the layout rspt_hip.h documents and its rings equal the model's, and the same recording in one call gives the same
output and the same rings."""

import numpy as np
import pytest

import devframe as df
import iir_sweep_cases as sw
from cases import digest
from devframe import api  # noqa: F401
from iir_model import same_doubles, state_rings

PART = sw.PART


def _pipe_runs(leg, hands_on=False):
    """(case, run length) of every run of the leg that the launch routes to the pipelined kernel"""
    return [(c, L) for c in sw.sweep_cases()[leg] if not hands_on or sw.hands_on(c) for L, r in sw.runs(c) if r == "pipe"]


# ---- CPU ----

def test_record_inputs_have_not_drifted():
    rec = df.golden("iir_sweep_record.json")["cases"]
    C = sw.all_cases()
    assert len(C) == len(rec) == len(sw.record())
    for c, r in zip(C, rec):
        assert (c["name"], c["leg"], c["bps"], c["nch"], c["ns"], c["nblocks"]) == (r["name"], r["leg"], r["bps"], r["nch"], r["ns"], r["nblocks"])
        assert sw.crc(c["data"]) == r["in_crc32"], c["name"]


@pytest.mark.parametrize("leg", sw.LEGS)
def test_restatement_matches_reference(leg):
    for c in sw.sweep_cases()[leg]:
        y, r = sw.want(leg, c["name"])[0], sw.record()[c["name"]]
        assert digest(y) == r["digest"] and sw.crc(y) == r["crc32"], c["name"]


def test_single_leg_oracle_matches_reference(orc):
    for c in sw.sweep_cases()["single"]:
        bb = c["bps"] * c["nch"] * c["ns"]
        y = b"".join(orc.iir_prefilter(c["data"][b * bb : (b + 1) * bb], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared_state=c["shared"])
                     for b in range(c["nblocks"]))
        assert digest(np.frombuffer(y, dtype=np.uint8)) == sw.record()[c["name"]]["digest"], c["name"]


@pytest.mark.parametrize("leg", sw.LEGS)
def test_the_pipelined_runs_cover_every_residue_part_and_place(leg):
    """over run lengths, and for the stream legs over call lengths"""
    chunk = sw.CHUNK[leg]
    runs = _pipe_runs(leg)
    assert {L % chunk for _, L in runs} == set(range(chunk))
    # one chunk; three and a partial one (a stream's calls end at three chunks: there it is the recording in one call)
    whole = [c["rows"] for c in sw.sweep_cases()[leg]] if leg in sw.STREAM_LEGS else [L for _, L in runs]
    assert any(L == chunk for _, L in runs) and any(L > 3 * chunk and L % chunk for L in whole)
    assert any(L >= 2 * chunk and L % chunk == 0 for _, L in runs)  # whole chunks only, more than one
    pairs = {(nc, part) for nc in (2, 3, 4, 5) for part in range(chunk // PART)}
    assert {(sw.first_nc(c), (L - 1) % chunk // PART) for c, L in runs} == pairs
    assert {sw.first_nc(c) for c, L in runs if (L - 1) % PART < sw.first_nc(c) - 1} == {2, 3, 4, 5}
    if leg != "cascade":  # the same among the runs whose producers hand the last inputs on (the stateless cascade has no such run)
        hand = _pipe_runs(leg, hands_on=True)
        assert {(sw.first_nc(c), (L - 1) % chunk // PART) for c, L in hand} == pairs
        assert {sw.first_nc(c) for c, L in hand if (L - 1) % PART < sw.first_nc(c) - 1} == {2, 3, 4, 5}
    if leg.startswith("cascade"):  # fewer chunks than 2 S + 1: the pipeline never fills; and more: it does
        fill = [(L + chunk - 1) // chunk < 2 * len(c["sections"]) + 1 for c, L in runs]
        assert any(fill) and not all(fill)
        for S in (1, 2, 3, 4):
            assert any(len(c["sections"]) == S for c, _ in runs), S


@pytest.mark.parametrize("leg", sw.LEGS)
def test_the_cases_cover_routes_modes_histories_and_lane_edges(leg):
    C = sw.sweep_cases()[leg]
    # both routes for every (nc, bps); every draw of the common sets
    assert {(sw.first_nc(c), c["bps"], r) for c in C for _, r in sw.runs(c)} == {(nc, bps, r) for nc in (2, 3, 4, 5) for bps in (1, 2, 3, 4) for r in ("pipe", "plain")}
    assert {c["off"] for c in C} == {0, 1, 2, 3}
    assert {c["nch"] for c in C} >= set(sw.NCH)
    # init below, at and above nc - 1 for every nc
    secs = [s for c in C for s in (c["sections"] if "sections" in c else [(c["n"], c["d"], c["init"], False)])]
    for nc in (2, 3, 4, 5):
        got = {s[2] for s in secs if len(s[0]) == nc}
        assert any(v < nc - 1 for v in got) and nc - 1 in got and any(v > nc - 1 for v in got)
    if leg in ("single", "zero_phase"):  # a chunk and more on the plain route: the history is too short
        assert any(r == "plain" and L >= sw.CHUNK[leg] for c in C for L, r in sw.runs(c))
    if leg == "single":
        assert {c["shared"] for c in C} == {False, True}
        assert {c["nblocks"] for c in C if c["shared"]} >= set(sw.SHARED_NBLOCKS)
        assert all(c["nch"] == 2 for c in C if c["shared"] and c["nblocks"] >= 70)
    if leg == "zero_phase":
        assert {(len(c["n"]), c["binit"]) for c in C} == {(nc, b) for nc in (2, 3, 4, 5) for b in sw.BINIT}
        assert {(len(c["n"]), c["binit"]) for c in C if sw.route(c) == "pipe"} == {(nc, b) for nc in (2, 3, 4, 5) for b in sw.BINIT}
    if "cascade" in leg:  # both section modes in every section position, every section count
        assert {(k, s[3]) for c in C for k, s in enumerate(c["sections"])} == {(k, m) for k in range(4) for m in (False, True)}
        assert {len(c["sections"]) for c in C} == {1, 2, 3, 4}
    if leg in sw.STREAM_LEGS:
        assert {c["ns"] for c in C} == set(sw.HANDLE_NS)
        assert all(200 <= c["rows"] < 700 + 16 for c in C)
    else:  # nblocks * nch around a multiple of 64, and a wave whose lanes span two blocks
        per = [c for c in C if not c.get("shared")]
        assert {c["nblocks"] * c["nch"] % 64 for c in per} >= {0, 1, 63}
        assert any(c["nblocks"] > 1 and c["nch"] % 64 for c in per)
        assert {c["nblocks"] for c in per} >= set(range(1, 8))


@pytest.mark.parametrize("leg", sw.STREAM_LEGS)
def test_every_recording_is_cut_on_both_sides_of_the_chunk(leg):
    chunk, C = sw.CHUNK[leg], sw.sweep_cases()[leg]
    opens = []
    for c in C:
        calls = c["calls"]
        assert sum(calls) == c["rows"] == c["ns"] * c["nblocks"] and all(L > 0 and L % c["ns"] == 0 for L in calls), c["name"]
        assert min(calls) < chunk <= max(calls), c["name"]
        # a fresh channel starts in one kernel and continues in the other
        assert (calls[0] < chunk) != (calls[1] < chunk), c["name"]
        opens.append(calls[0] < chunk)
    assert abs(2 * sum(opens) - len(opens)) <= 2  # half open with a short call, half with a long one
    lengths = {L for c in C for L in c["calls"]}
    assert lengths >= {1, 2, 3, 4, 5, chunk - 1, chunk, chunk + 1}
    assert any(c["ns"] == 1 and len(c["calls"]) > 5 for c in C)  # a handle of one row: cut at any row


@pytest.mark.parametrize("leg", sw.LEGS)
def test_non_finite_values_travel_through_a_cut_or_the_turn(leg):
    """an unstable filter's +-inf and NaN start inside a run: in front of a later call of a stream, in front of the turn of the
    zero-phase stage; the milder one stays finite and passes 2^31"""
    C = [c for c in sw.sweep_cases()[leg] if c["grow"]]
    assert {c["grow"] for c in C} == set(sw.UNSTABLE_G)
    hits = past = 0
    for c in C:
        if leg in sw.STREAM_LEGS:
            y = sw.stream_doubles(c)[0]
            last_cut = c["rows"] - c["calls"][-1]
        elif leg == "zero_phase":
            y, last_cut = sw.zc.doubles(c)[1][: c["ns"]], c["ns"]  # the forward pass of block 0
        elif leg == "cascade":
            x = sw.native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]).astype(np.float64)[: c["ns"]]
            y, last_cut = sw.cc.chain_double(x, c["sections"])[0], c["ns"]
        else:
            y, last_cut = sw.ic.iir_double(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], c["shared"], c["nblocks"])[0], c["ns"]
        bad = ~np.isfinite(y)
        past += bool(c["grow"] == 1.5 and bad.sum() == 0 and (np.abs(y) >= 2.0 ** 31).any())
        for ch in range(c["nch"]):
            rows = np.flatnonzero(bad[:, ch])
            if rows.size and 0 < rows[0] < last_cut and np.isinf(y[:, ch]).any() and (np.isnan(y[:, ch]).any() or sw.first_nc(c) == 2):
                hits += 1
                break
    assert hits >= 1 and past >= 1


# ---- GPU ----

def _what(c):
    return df.what(c, hide=("data",))


def _call(pk, c, buf, state=None, work=None):
    leg = c["leg"]
    if leg == "single":
        pk.iir_prefilter_batch(buf, c["n"], c["d"], init_nr_samples=c["init"], per_channel=not c["shared"])
    elif leg == "single_stream":
        pk.iir_prefilter_batch(buf, c["n"], c["d"], init_nr_samples=c["init"], per_channel=True, state=state)
    elif leg == "zero_phase":
        pk.iir_zero_phase_batch(buf, c["n"], c["d"], init_nr_samples=c["init"], backward_init_nr_samples=c["binit"], work=work)
    else:
        pk.iir_cascade_batch(buf, c["sections"], state=state)


def _stateless_leg(api, leg):
    import torch

    for c in sw.sweep_cases()[leg]:
        want, rec = sw.want(leg, c["name"])[0], sw.record()[c["name"]]
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        n = c["data"].size
        raw, buf = df.guarded(n, c["off"], c["data"])
        assert buf.data_ptr() % 4 == c["off"]
        wraw = work = None
        if leg == "zero_phase":
            wn = pk.iir_zero_phase_work_bytes(c["nblocks"])
            assert wn == (c["nblocks"] * c["nch"] + 63) // 64 * 64 * c["ns"] * 8
            wraw, work = df.guarded(wn, 0, 0xFF)  # exactly the bound, NaNs throughout
            assert work.data_ptr() % 8 == 0
        _call(pk, c, buf, work=work)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert digest(got) == rec["digest"], ("record", _what(c))
        assert np.array_equal(got, want), ("restatement", _what(c))
        assert df.guards_untouched(raw, c["off"], n), ("guards", _what(c))
        if wraw is not None:
            assert df.guards_untouched(wraw, 0, work.numel()), ("workspace guards", _what(c))
        pk.close()


@pytest.mark.gpu
def test_gpu_single_sweep(api):
    _stateless_leg(api, "single")


@pytest.mark.gpu
def test_gpu_cascade_sweep(api):
    _stateless_leg(api, "cascade")


@pytest.mark.gpu
def test_gpu_zero_phase_sweep(api):
    _stateless_leg(api, "zero_phase")


def _stream_leg(api, leg):
    import torch

    for c in sw.sweep_cases()[leg]:
        (want, rings), rec = sw.want(leg, c["name"]), sw.record()[c["name"]]
        S = len(c["sections"])
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        n, row = c["data"].size, c["bps"] * c["nch"]
        new_state = pk.iir_state if leg == "single_stream" else lambda: pk.iir_cascade_state(S)
        seen = []
        for how, calls in (("cut", c["calls"]), ("one_call", [c["rows"]])):
            raw, buf = df.guarded(n, c["off"], c["data"])
            state = new_state()
            assert state.numel() == 88 * c["nch"] * S and int(state.count_nonzero()) == 0
            r0 = 0
            for L in calls:
                _call(pk, c, buf[r0 * row : (r0 + L) * row], state=state)
                r0 += L
            assert r0 == c["rows"]
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            assert digest(got) == rec["digest"], (how, "record", _what(c))
            assert np.array_equal(got, want), (how, "restatement", _what(c))
            assert df.guards_untouched(raw, c["off"], n), (how, "guards", _what(c))
            x, y, started = state_rings(state, c["nch"], S)
            assert (started == 1).all(), (how, "started", _what(c))
            for k, (mx, my) in enumerate(rings):  # the model's [nc][nch] against the state's first nc places
                nc = mx.shape[0]
                assert same_doubles(x[:, k, :nc].T, mx), (how, "x ring of section %d" % k, _what(c))
                assert same_doubles(y[:, k, :nc].T, my), (how, "y ring of section %d" % k, _what(c))
            seen.append((got, x, y))
        (g0, x0, y0), (g1, x1, y1) = seen  # however it is cut: the same output, the same first nc places
        assert np.array_equal(g0, g1), ("cut invariance", _what(c))
        for k, (mx, _) in enumerate(rings):
            nc = mx.shape[0]
            assert same_doubles(x0[:, k, :nc], x1[:, k, :nc]) and same_doubles(y0[:, k, :nc], y1[:, k, :nc]), ("cut invariance of the rings", k, _what(c))
        pk.close()


@pytest.mark.gpu
def test_gpu_single_stream_sweep(api):
    _stream_leg(api, "single_stream")


@pytest.mark.gpu
def test_gpu_cascade_stream_sweep(api):
    _stream_leg(api, "cascade_stream")
