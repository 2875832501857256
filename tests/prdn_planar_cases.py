"""PRDN on the planar int32 matrix (rspt_hip_prdn_planar_batch_dev; DESIGN.md 4f, "The planar form"): the inputs and the CPU side
of every expectation of tests/test_prdn_planar.py.

The contract is one identity: prdn_planar(O, D) is the native entry's result on a little-endian bps = 4 handle given
i32_to_native(O) and i32_to_native(D).  The reference converts to int32 before its loop, so every case of
tests/golden/prdn_record.json is a planar case with the same answer (the planar input is native_to_i32(case).T), and the
restatement here is prdn_cases.prdn_parts at bps = 4 -- which the record pins to the reference.
"""
import os
import re

import numpy as np

import cases
import planar_cases as pl
import prdn_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planar_of(c):
    """a case of prdn_cases -> (O, D), each [nch][ns] int32"""
    return tuple(np.ascontiguousarray(pc.native_to_i32(c[k], c["bps"], c["nch"], c["ns"]).T) for k in ("orig", "dec"))


def prdn_parts_planar(O, D):
    """[nch][ns] int32 x 2 -> prdn_cases.prdn_parts of the two as bps = 4 native blocks"""
    nch, ns = O.shape
    return pc.prdn_parts(pc.i32_to_native(O.T, 4), pc.i32_to_native(D.T, 4), 4, nch, ns)


def want_bits(O, D):
    """[nblocks][nch][ns] x 2 -> (prdn, mse, ref) as uint64 bit patterns and path, one entry per block"""
    parts = [prdn_parts_planar(O[b], D[b]) for b in range(O.shape[0])]
    return tuple(np.array([pc.bits(w[k]) for w in parts], dtype=np.uint64) for k in range(3)) + (np.array([w[3] for w in parts], dtype=np.int32),)


def cut(P, bps):
    """the values of P inside a sample width of bps bytes (what from_planar_i32 keeps)"""
    return pl.cc.sign_extend(P, bps)


# ---- the host's choice of form, restated (rspt_amd/csrc/quality_planar.hip, host_stages.hip: quality_planar_geom) -------------------
WAVE = 64
THREADS = 256
WAVE_ROW = 1024          # kQpWaveRow: rows up to this take a wave each, four to a workgroup
U = 4                    # kQpU
SWEEP = THREADS * 4 * U  # kQpSweep
MIN_SWEEPS = 2           # kQpMinSweeps
UNITS = 4096             # kQpUnits
ROW_REGS = THREADS * 4 * U  # kQpRowRegs: whole rows up to this stay in registers
FUSED_MIN_UNITS = 1024   # kQpFusedMinUnits
FUSED_MAX_NS = 8192      # kQpFusedMaxNs


def source_constants():
    """the named constants of quality_planar.hip as the source states them"""
    text = open(os.path.join(ROOT, "rspt_amd", "csrc", "quality_planar.hip")).read()
    env = {"kWave": WAVE}
    for name, expr in re.findall(r"^constexpr uint32_t (kQp\w+) = ([^;]+);", text, re.M):
        env[name] = eval(expr, {}, env)  # (products of earlier constants and literals)
    return env


def form(nblocks, nch, ns):
    """what the host picks for a call: dict(fused, lanes, regs, nsplit)"""
    rows = nblocks * nch
    lanes = WAVE if ns <= WAVE_ROW else THREADS
    units = (rows + 3) // 4 if lanes == WAVE else rows
    if units >= FUSED_MIN_UNITS and ns <= FUSED_MAX_NS:
        return dict(fused=True, lanes=lanes, regs=ns <= (WAVE_ROW if lanes == WAVE else ROW_REGS), nsplit=1)
    nsplit = 1
    if lanes == THREADS:
        sweeps = (ns + SWEEP - 1) // SWEEP
        k = min(max(1, sweeps // MIN_SWEEPS), (UNITS + rows - 1) // rows)
        span = (sweeps + k - 1) // k * SWEEP
        if span < ns:
            nsplit = (ns + span - 1) // span
    return dict(fused=False, lanes=lanes, regs=False, nsplit=nsplit)


# ---- row geometry ---------------------------------------------------------------------------------------------------------------
GRID_NCH = (1, 2, 3, 5)
GRID_NS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
GRID_NBLOCKS = (1, 3)
OFFSETS = (0, 4, 8, 12)  # bytes from a 16-byte boundary, d_orig and d_dec independently

# (nblocks, nch, ns): both sides of every threshold of form(); offsets: a few, see THRESHOLD_OFFSETS
THRESHOLD_SHAPES = [
    (1, 2, SWEEP * (2 * MIN_SWEEPS - 1)), (1, 2, SWEEP * (2 * MIN_SWEEPS - 1) + 1),  # one span | the first ns that is cut into two
    (3, 1, 50001),                                                                 # an odd row cut into spans, blocks off the boundary
    (1, 4 * FUSED_MIN_UNITS - 4, 7), (1, 4 * FUSED_MIN_UNITS - 3, 7),                # a wave per row: split | whole rows
    (1, FUSED_MIN_UNITS - 1, WAVE_ROW + 1), (1, FUSED_MIN_UNITS, WAVE_ROW + 1),      # a workgroup per row: split | whole rows
    (2, FUSED_MIN_UNITS // 2, ROW_REGS), (2, FUSED_MIN_UNITS // 2, ROW_REGS + 1),    # whole rows: in registers | read twice
    (4, FUSED_MIN_UNITS, WAVE_ROW - 1), (4, FUSED_MIN_UNITS, WAVE_ROW),              # whole rows, a wave each, at the wave's capacity
    (1, FUSED_MIN_UNITS, FUSED_MAX_NS), (1, FUSED_MIN_UNITS, FUSED_MAX_NS + 1),      # the longest whole row | split again
]
THRESHOLD_OFFSETS = ((0, 0), (4, 12), (8, 8))


def check_threshold_shapes():
    """the shapes straddle the thresholds as the host has them"""
    k = source_constants()
    assert (k["kQpWaveRow"], k["kQpU"], k["kQpSweep"], k["kQpMinSweeps"], k["kQpUnits"], k["kQpRowRegs"], k["kQpFusedMinUnits"], k["kQpFusedMaxNs"]) == (
        WAVE_ROW, U, SWEEP, MIN_SWEEPS, UNITS, ROW_REGS, FUSED_MIN_UNITS, FUSED_MAX_NS)
    f = {s: form(*s) for s in THRESHOLD_SHAPES}
    t = THRESHOLD_SHAPES
    assert f[t[0]] == dict(fused=False, lanes=THREADS, regs=False, nsplit=1) and f[t[1]]["nsplit"] == 2 and f[t[2]]["nsplit"] > 2
    assert not f[t[3]]["fused"] and f[t[4]] == dict(fused=True, lanes=WAVE, regs=True, nsplit=1)
    assert not f[t[5]]["fused"] and f[t[6]] == dict(fused=True, lanes=THREADS, regs=True, nsplit=1)
    assert f[t[7]] == dict(fused=True, lanes=THREADS, regs=True, nsplit=1) and f[t[8]] == dict(fused=True, lanes=THREADS, regs=False, nsplit=1)
    assert f[t[9]]["lanes"] == f[t[10]]["lanes"] == WAVE and f[t[9]]["fused"] and f[t[10]]["regs"]
    assert f[t[11]] == dict(fused=True, lanes=THREADS, regs=False, nsplit=1) and not f[t[12]]["fused"]
    # rows-per-workgroup packing: both sides are in the grid
    assert WAVE_ROW in GRID_NS and WAVE_ROW + 1 in GRID_NS
    assert form(1, 1, WAVE_ROW)["lanes"] == WAVE and form(1, 1, WAVE_ROW + 1)["lanes"] == THREADS


def values(nblocks, nch, ns, seed):
    """(O, D) [nblocks][nch][ns]: block 0 full-range int32 noise against other noise where the shape's ns is odd, every other block
    a small walk against itself with a small error"""
    O = pl.walk(nblocks, nch, ns, 4, seed)
    D = (O.astype(np.int64) + cases.hash_i32(nblocks * nch * ns, seed + 1, 8).astype(np.int64).reshape(O.shape)).astype(np.int32)
    if ns % 2:
        O[0], D[0] = pl.noise(1, nch, ns, seed + 2)[0], pl.noise(1, nch, ns, seed + 3)[0]
    return O, D
