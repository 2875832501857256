"""A seeded sweep of the IIR family (filter.hip, iir_cascade.hip, iir_zero_phase.hip) over shapes, orders, histories and cuts.

Five legs, each a list of dicts like the other case modules':
    single          iir_prefilter_batch, stateless, shared and per channel
    single_stream   iir_prefilter_batch(state=): one recording cut into calls of any length (a handle of 1 to 16 rows per block)
    cascade         iir_cascade_batch, stateless: 1..4 sections, each with its own order, history and filter() / filter_opt()
    cascade_stream  iir_cascade_batch(state=): the same, cut into calls
    zero_phase      iir_zero_phase_batch

The generator is deterministic (np.random.default_rng(SEED)) and stratified: where a quantity has to take every value of a small
set -- the run length's residue mod the pipelined kernel's chunk, with it the producer part and the place in it that hold the
last sample, the order, the sample width, the history length on either side of the route switch, the backward history, the
section modes -- case i takes value i mod the set's size (_Draw.cyc), and the rest is drawn.  tests/test_iir_sweep.py asserts what
the generated lists cover, so an edit here cannot hollow the sweep out unnoticed.

The drivers (expected, stream_expected) give the answers by tests/iir_model.py's IirModel, through iir_cases.iir_double,
iir_cascade_cases.chain_double and iir_zero_phase_cases.zero_phase_double: no second statement of the filter.  The compiled
reference's answers are tests/golden/iir_sweep_record.json (tests/golden/make_iir_sweep_record.py).

About one case in twelve takes an unstable filter behind an onset block, alternately iir_cases.unstable(1e3) and unstable(1.5):
within the few hundred rows of a run only the first reaches +-inf and NaN (1.5 ** 700 is 1e123), the second stays finite far
past 2^31.
"""
import functools
import json
import os

import numpy as np

import cases
import iir_cascade_cases as cc
import iir_cases as ic
import iir_zero_phase_cases as zc
from fir_cases import crc, i32_to_native, native_to_i32, trunc_i32  # noqa: F401

SEED = 20261018
LEGS = ("single", "single_stream", "cascade", "cascade_stream", "zero_phase")
STREAM_LEGS = ("single_stream", "cascade_stream")
CHUNK = {"single": ic.CHUNK_PIPE, "single_stream": ic.CHUNK_PIPE, "cascade": cc.CHUNK, "cascade_stream": cc.CHUNK, "zero_phase": zc.CHUNK}
PART = 16  # samples of a chunk per producer wave, in all three pipelined kernels

NCH = (1, 2, 3, 5, 12, 33, 63, 64, 65, 130)
HANDLE_NS = (1, 2, 3, 7, 16)
OFFSETS = (0, 0, 0, 1, 2, 3)  # bytes between a 256-byte boundary and the buffer
BINIT = (0, 1, 2, 50)
SHARED_NBLOCKS = (1, 3, 70, 300, 520, 800)  # 300, 520, 800: 2, 3, 4 blocks per workgroup on a part with 256 CUs
LANE_EDGES = ((64, 1), (65, 1), (63, 1), (64, 3), (1, 1), (33, 2))  # (nch, nblocks): nblocks * nch mod 64 in {0, 1, 63}, a wave over two blocks
MAX_SAMPLES = 120000  # per case, so that the restatement stays quick
COEFS = {2: (ic.STABLE[2],), 3: (ic.STABLE[3], cases.IIR_LOWPASS, cc.HP04), 4: (ic.STABLE[4],), 5: (ic.STABLE[5], cases.IIR_BANDPASS)}
UNSTABLE_G = (1e3, 1.5)


def inits(nc):
    """the history lengths a filter of nc coefficients takes: nc - 1 is the route switch of the single and zero-phase stages"""
    out = []
    for v in (0, 1, nc - 2, nc - 1, nc, 7, 50):
        if v not in out:
            out.append(v)
    return out


class _Draw:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.count = {}
        self.wanted = {}

    def cyc(self, key, seq):
        """value i mod len(seq) for the i-th asker under key"""
        i = self.count.get(key, 0)
        self.count[key] = i + 1
        return seq[i % len(seq)]

    def pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def int(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))


def _unstable(i):
    """the growth of case i's unstable filter, or None"""
    return UNSTABLE_G[(i // 12) % 2] if i % 12 == 5 else None


def _coef(g, leg, nc, grow):
    n, d = ic.unstable(grow, nc) if grow else g.cyc((leg, "coef", nc), COEFS[nc])
    return [float(v) for v in n], [float(v) for v in d]


def _data(g, bps, nch, rows, seed, grow):
    """native bytes of rows rows: full-scale, 1 << (8 bps - 4) or 3, random or a walk; an unstable filter's: channels fed from an
    early row on, from the first row on, never, in turn"""
    if grow:
        onset = g.int(1, 30)
        return ic.onset_block(nch, rows, bps, seed, [(onset, 0, None)[c % 3] for c in range(nch)], min(1000, (1 << (8 * bps - 1)) - 1))
    amp = g.pick(((1 << (8 * bps - 1)) - 1, 1 << (8 * bps - 4), 3))
    return cases._rand_native(nch, rows, bps, seed, amp, walk=bool(g.int(0, 1)))


def _lanes(g, leg, i, ns):
    """(nch, nblocks) of a stateless per-channel case"""
    nch, nb = g.cyc((leg, "edge"), LANE_EDGES) if i % 5 == 0 else (g.pick(NCH), g.int(1, 7))
    while nb > 1 and nch * nb * ns > MAX_SAMPLES:
        nb -= 1
    return nch, nb


def _slot(r, chunk):
    """the order and sample width of the pipelined run whose length is r mod chunk: the last sample's place in its producer part
    selects the order (place p: order 2 + p mod 4, so that it lies among the first nc - 1 places where p < 4), and every part and
    every order meets every width"""
    lastpos = (r - 1) % chunk
    return 2 + lastpos % 4, 1 + (lastpos // 4 + lastpos // PART) % 4


PIPE_EXTRA = (0, 0, 1, 63, 16, 32, 48, 15)  # residues once more, at two chunks and more (residue 0 of the first round is one chunk)


def _length(g, chunk, r, first_round, grow, qs):
    q = 1 if (r == 0 and first_round) else g.pick(qs)
    if grow:
        q = max(q, 256 // chunk)  # (room for 1e3 ** n to pass 1e308)
    return chunk * q + r if r else chunk * max(q, 1)


def _single(g):
    leg, C = "single", []
    slots = [(r, True) for r in range(64)] + [(r, False) for r in PIPE_EXTRA]
    for i in range(len(slots) + 16):
        grow = _unstable(i)
        # shared mode hands the last inputs on to the next channel: it takes every run whose last sample lies among its part's first four
        shared = bool(g.int(0, 1)) or (i < 64 and (i - 1) % 64 % PART < 4)
        big = 1
        if shared:
            big = g.cyc((leg, "shared"), SHARED_NBLOCKS[:2] if grow else SHARED_NBLOCKS)
        if i < len(slots):
            r, first = slots[i]
            nc, bps = _slot(r, 64)
            init = g.cyc((leg, "init_pipe", nc), [v for v in inits(nc) if v >= 1])
            ns = _length(g, 64, r, first, grow, (1,) if big >= 70 else (1, 1, 2, 3, 5, 9) if first else (2, 3, 4))
        else:
            k = i - len(slots)
            nc, bps = 2 + k % 4, 1 + k // 4
            if (k + k // 4) % 2 == 0:
                ns, init = g.int(1, 63), g.cyc((leg, "init_plain", nc), inits(nc))
            else:
                ns, init = 64 * g.pick((1,) if big >= 70 else (1, 2, 3)) + g.int(0, 63), 0  # a chunk and more, no history: the plain kernel
        if shared:
            nch, nb = 2 if big >= 70 else g.pick((2, 3, 5, 12)), big
        else:
            nch, nb = _lanes(g, leg, i, ns)
        n, d = _coef(g, leg, nc, grow)
        C.append(dict(leg=leg, bps=bps, nch=nch, ns=ns, nblocks=nb, n=n, d=d, init=init, shared=shared, off=g.pick(OFFSETS),
                      data=_data(g, bps, nch, ns * nb, 9000 + i, grow), grow=grow,
                      name="single%03d_i%d_%dch_ns%d_x%d_nc%d_init%d_%s" % (i, 8 * bps, nch, ns, nb, nc, init, "shared" if shared else "per_channel")))
    return C


def _zero_phase(g):
    leg, C = "zero_phase", []
    slots = [(r, True) for r in range(64)] + [(r, False) for r in PIPE_EXTRA]
    for i in range(len(slots) + 16):
        grow = _unstable(i)
        if i < len(slots):
            r, first = slots[i]
            nc, bps = _slot(r, 64)
            init = g.cyc((leg, "init_pipe", nc), [v for v in inits(nc) if v >= nc - 1])
            ns = _length(g, 64, r, first, grow, (1, 1, 2, 3, 5, 9) if first else (2, 3, 4))
        else:
            k = i - len(slots)
            nc, bps = 2 + k % 4, 1 + k // 4
            if (k + k // 4) % 2 == 0:
                ns, init = g.int(1, 63), g.cyc((leg, "init_plain", nc), inits(nc))
            else:  # a chunk and more with a history shorter than the ring's tail: the plain kernel
                ns, init = 64 * g.pick((1, 2, 3)) + g.int(0, 63), g.cyc((leg, "init_short", nc), [v for v in inits(nc) if v < nc - 1])
        binit = g.cyc((leg, "binit", nc), BINIT)
        nch, nb = _lanes(g, leg, i, ns)
        n, d = _coef(g, leg, nc, grow)
        C.append(dict(leg=leg, bps=bps, nch=nch, ns=ns, nblocks=nb, n=n, d=d, init=init, binit=binit, off=g.pick(OFFSETS),
                      data=_data(g, bps, nch, ns * nb, 11000 + i, grow), grow=grow,
                      name="zp%03d_i%d_%dch_ns%d_x%d_nc%d_init%d_b%d" % (i, 8 * bps, nch, ns, nb, nc, init, binit)))
    return C


def _sections(g, leg, nc0, modes, grow):
    """a chain whose section 0 has nc0 coefficients (an unstable filter's where grow), the others drawn"""
    secs = []
    for k, m in enumerate(modes):
        nc = nc0 if k == 0 else g.pick((2, 3, 4, 5))
        n, d = _coef(g, leg, nc, grow if k == 0 else None)
        secs.append((n, d, g.cyc((leg, "init", nc), inits(nc)), bool(m)))
    return secs


def _tag(secs):
    return "s%d_nc%s_%s" % (len(secs), "".join(str(len(s[0])) for s in secs), "".join("f" if s[3] else "o" for s in secs))


def _cascade(g):
    leg, C = "cascade", []
    combos = []
    for _ in range(2):  # per round of residues: every section count with every mode pattern of the sections behind the first
        c = [(S, pat) for S in (1, 2, 3, 4) for pat in range(8)]
        g.rng.shuffle(c)
        combos.append(c)
    for i in range(64 + 16):
        grow = _unstable(i)
        if i < 64:
            r, rnd = i % 32, i // 32
            nc0, bps = _slot(r, 32)
            bps = 1 + (bps - 1 + rnd) % 4
            S, pat = combos[rnd][r]
            modes = [rnd] + [(pat >> (k - 1)) & 1 for k in range(1, S)]  # round 0: section 0 runs filter_opt (the producers' hand-off)
            ns = _length(g, 32, r, rnd == 0, grow, (1, 1, 2, 3, 4, 6, 10, 20))
        else:
            k = i - 64
            nc0, bps = 2 + k % 4, 1 + k // 4
            modes = [g.int(0, 1) for _ in range(g.cyc((leg, "S"), (1, 2, 3, 4)))]
            ns = g.int(1, 31)
        secs = _sections(g, leg, nc0, modes, grow)
        nch, nb = _lanes(g, leg, i, ns)
        C.append(dict(leg=leg, bps=bps, nch=nch, ns=ns, nblocks=nb, sections=secs, off=g.pick(OFFSETS),
                      data=_data(g, bps, nch, ns * nb, 13000 + i, grow), grow=grow,
                      name="casc%03d_i%d_%dch_ns%d_x%d_%s" % (i, 8 * bps, nch, ns, nb, _tag(secs))))
    return C


def _cuts(g, leg, nc, hns, rows, open_short, hands_on):
    """the call lengths, in rows (multiples of the handle's hns), that a recording of `rows` rows is cut into: 1 to 5 rows;
    chunk - 1, chunk, chunk + 1; a uniform draw in [1, 3 chunk]; a residue mod the chunk that the leg still wants at one or two
    chunks and more; the remainder.  The first two calls lie on either side of the chunk"""
    chunk = CHUNK[leg]

    def fit(L):
        return max(hns, (L + hns - 1) // hns * hns)

    def long_call():
        # first the residues that put the last sample into each producer part, among its first nc - 1 places, for this order
        qs = (1, 2) if g.int(0, 3) else (2, 1)
        for key, fill in (((leg, nc), [(PART * p + nc - 2 + 1) % chunk for p in range(chunk // PART)]), (leg, list(range(chunk)))):
            if key != leg and not hands_on:
                continue
            if key not in g.wanted or (not g.wanted[key] and key == leg):
                g.wanted[key] = list(fill)
            for idx, r in enumerate(g.wanted[key]):
                for q in qs:
                    L = chunk * q + r
                    if L % hns == 0:
                        g.wanted[key].pop(idx)
                        return L
        return fit(chunk + g.int(0, 2 * chunk))

    def short():
        return fit(g.int(1, 5))

    kinds = {"short": short, "edge": lambda: fit(chunk + g.pick((-1, 0, 1))), "uniform": lambda: fit(g.int(1, 3 * chunk)), "long": long_call}
    calls, left = [], rows
    while left:
        if len(calls) < 2:
            kind = "short" if (len(calls) == 0) == open_short else "long"
        else:
            kind = g.pick(("short", "short", "edge", "uniform", "long", "long", "long", "long"))
        L = min(kinds[kind](), left)
        calls.append(L)
        left -= L
    assert sum(calls) == rows and all(L % hns == 0 for L in calls)
    return calls


def _stream(g, leg, count=60):
    C = []
    for i in range(count):
        grow = _unstable(i)
        nc0, bps, hns = 2 + i % 4, 1 + (i // 4) % 4, HANDLE_NS[i % 5]
        open_short = (i // 4 + i) % 2 == 0
        nch = g.pick(NCH)
        rows = (g.int(200, 700) + hns - 1) // hns * hns
        mode0 = leg == "cascade_stream" and (i // 16) % 4 == 3  # section 0 through filter(): the recurrence wave holds its x ring
        calls = _cuts(g, leg, nc0, hns, rows, open_short, not mode0)
        c = dict(leg=leg, bps=bps, nch=nch, ns=hns, nblocks=rows // hns, rows=rows, calls=calls, off=g.pick(OFFSETS), grow=grow)
        if leg == "single_stream":
            n, d = _coef(g, leg, nc0, grow)
            init = g.cyc((leg, "init", nc0), inits(nc0))
            c.update(n=n, d=d, init=init, sections=[(n, d, init, False)], name="sstream%03d_i%d_%dch_%dx%d_nc%d_init%d_%dcalls" % (i, 8 * bps, nch, hns, rows // hns, nc0, init, len(calls)))
        else:
            S = 1 + (i // 2) % 4
            modes = [int(mode0)] + [g.int(0, 1) for _ in range(S - 1)]
            secs = _sections(g, leg, nc0, modes, grow)
            c.update(sections=secs, name="cstream%03d_i%d_%dch_%dx%d_%s_%dcalls" % (i, 8 * bps, nch, hns, rows // hns, _tag(secs), len(calls)))
        c["data"] = _data(g, bps, nch, rows, (15000 if leg == "single_stream" else 17000) + i, grow)
        C.append(c)
    return C


@functools.lru_cache(maxsize=None)
def sweep_cases():
    """leg -> its cases.  Common keys: leg, name, bps, nch, ns, nblocks (the handle's shape and the block count), off (the base's
    offset in bytes), data (native bytes), grow (an unstable filter's growth, or None).  single, zero_phase: n, d, init (and shared /
    binit); the cascades: sections [(n, d, init, use_filter)]; the stream legs: rows, calls (their lengths in rows), sections"""
    g = _Draw(SEED)
    out = {"single": _single(g), "single_stream": _stream(g, "single_stream"), "cascade": _cascade(g),
           "cascade_stream": _stream(g, "cascade_stream"), "zero_phase": _zero_phase(g)}
    for leg, C in out.items():
        assert len({c["name"] for c in C}) == len(C), leg
        for c in C:
            c["data"] = np.ascontiguousarray(c["data"], dtype=np.uint8).reshape(-1)
            c["data"].setflags(write=False)
            assert c["data"].size == c["bps"] * c["nch"] * c["ns"] * c["nblocks"], c["name"]
    return out


def all_cases():
    S = sweep_cases()
    return [c for leg in LEGS for c in S[leg]]


# ---- what a case runs through ----

def route(c, rows=None):
    """'pipe' or 'plain': the kernel the launch routes a run of the case to (rows: a stream call's length)"""
    leg = c["leg"]
    if leg in STREAM_LEGS:
        return "pipe" if rows >= CHUNK[leg] else "plain"
    if leg == "single":
        return "pipe" if ic.kernel_of(c["ns"], c["init"], len(c["n"])) == "pipe" else "plain"
    if leg == "zero_phase":
        return zc.kernel_of(c["ns"], c["init"], len(c["n"]))
    return "pipe" if c["ns"] >= CHUNK[leg] else "plain"


def runs(c):
    """[(length in rows, route)] of the runs the case's launches see: one per stateless case, one per call of a stream"""
    if c["leg"] in STREAM_LEGS:
        return [(L, route(c, L)) for L in c["calls"]]
    return [(c["ns"], route(c))]


def first_nc(c):
    """the order of the filter whose inputs the producers hand on: the stage's own, or the cascade's section 0"""
    return len(c["sections"][0][0]) if "sections" in c else len(c["n"])


def hands_on(c):
    """whether a pipelined run of the case hands its last inputs on from a producer: shared mode, a carried state and the turn;
    a cascade's producers do it for a section 0 that runs filter_opt"""
    leg = c["leg"]
    if leg == "single":
        return c["shared"]
    if leg == "cascade":
        return False
    return leg != "cascade_stream" or not c["sections"][0][3]


# ---- the drivers ----

def expected(c):
    """the filtered blocks of a stateless case in the native sample width (bytes)"""
    leg = c["leg"]
    if leg == "single":
        return ic.iir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared=c["shared"], nblocks=c["nblocks"])
    if leg == "cascade":
        return cc.filtered(c, "stateless")
    if leg == "zero_phase":
        return zc.filtered(c)
    raise ValueError(leg)


def stream_doubles(c):
    """a stream case's untruncated outputs [rows][nch], and the filter objects of its sections (a lane per channel) as they
    stand behind the last row"""
    models = []
    x = native_to_i32(c["data"], c["bps"], c["nch"], c["rows"]).astype(np.float64)
    y, _ = cc.chain_double(x, c["sections"], models)
    return y, models


def stream_expected(c):
    """the filtered recording in the native sample width (bytes), and the rings the model holds behind the last row:
    per section (x, y), each [nc][nch] float64, newest first"""
    y, models = stream_doubles(c)
    rings = [(np.array(f.x, dtype=np.float64), np.array(f.y, dtype=np.float64)) for f in models]
    return i32_to_native(trunc_i32(y), c["bps"]), rings


# ---- the record and the answers, once per process ----

@functools.lru_cache(maxsize=None)
def record():
    """name -> the compiled reference's answer (tests/golden/iir_sweep_record.json)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iir_sweep_record.json")) as f:
        return {r["name"]: r for r in json.load(f)["cases"]}


@functools.lru_cache(maxsize=None)
def want(leg, name):
    """the restatement's answer (and, for a stream, the model's rings behind the last row), computed once per process (read-only)"""
    c = next(c for c in sweep_cases()[leg] if c["name"] == name)
    out = stream_expected(c) if leg in STREAM_LEGS else (expected(c), None)
    out[0].setflags(write=False)
    return out
