"""Compress to a byte budget (rspt_hip_compress_budget_batch_dev): shapes, ladders, inputs, the rule and a CPU restatement of a
candidate's stream size.

The rule (include/rspt_hip.h).  For block b and ladder entry k, size_k(b) is the length of the stream the ladder entry writes for
b at ladder[k] and the handle's nb.  budget(b) is the block's own limit or the one limit of the call; any uint64, 0 included.
The choice is the HIGHEST index k with size_k(b) <= budget(b) -- nothing assumes that the sizes are sorted in ladder order, and
<= is inclusive -- and, if no entry fits, the entry of the smallest size, the lowest index among equals.

The restated size is built on lossy_quantizer_cases' transforms and cuts, which give the byte planes, and on the oracle's
libhzr restatement, which gives each plane's stream: 1 + hdr_len + the sum over the nb planes of (4 + len(hzr stream)).
tests/test_budget_rule.py holds it to the reference's own streams (tests/golden/lossy_quantizer_record.json) and holds the
cases below to the conditions they exist for; tests/test_gpu_budget.py then holds the device to the composed oracle on the device.
"""
import functools

import numpy as np

import cases
import lossy_quantizer_cases as lq

HADAMARD_LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0]  # coarse to fine: a larger quality is finer
DCT_LADDER = [1024.0, 128.0, 16.0, 1.0]          # coarse to fine: a larger quality is coarser
LADDER8 = [1.0 / 64, 1.0 / 16, 1.0 / 4, 1.0 / 2, 1.0, 2.0, 4.0, 64.0]
UNSORTED_LADDER = [1.0, 1.0 / 16, 4.0, 1.0 / 4]  # sizes in ladder order: third, smallest, largest, second
REPEATED_LADDER = [1.0 / 4, 1.0, 1.0, 4.0]       # entries 1 and 2 write the same stream: the later index wins
BATCHED_MAX_NS = 8192      # kTpMaxNs of target.hip: the longest row of the batched route
MAX_SLOTS = 65535          # nladder * nblocks of the batched route (rspt_hip_reserve's bound)
U64_MAX = (1 << 64) - 1
CONTENTS = ("rand", "walk", "const", "full")

# (kind, bps, nch, ns, nb): the smallest shapes at which each piece can go wrong
HADAMARD_SHAPES = [("hadamard", 4, 1, 2, 1), ("hadamard", 1, 3, 8, 2), ("hadamard", 2, 5, 1024, 3),
                   ("hadamard", 4, 12, 8192, 3),   # the longest batched row
                   ("hadamard", 4, 9, 8192, 3),    # two hzr blocks per plane, the last one ragged
                   ("hadamard", 4, 2, 16384, 3), ("hadamard", 4, 2, 65536, 3), ("hadamard", 4, 2, 131072, 2)]  # general route only
DCT_SHAPES = [("dct", 3, 3, 100, 2), ("dct", 4, 2, 257, 3), ("dct", 2, 2, 4096, 1)]
SHAPES = HADAMARD_SHAPES + DCT_SHAPES


def shape_id(s):
    return "%s_i%d_%dx%d_nb%d" % (s[0], 8 * s[1], s[2], s[3], s[4])


def ladder_of(kind):
    return list(HADAMARD_LADDER if kind == "hadamard" else DCT_LADDER)


def batched(shape, nblocks=1, nladder=1):
    """the batched route runs this call"""
    return shape[0] == "hadamard" and shape[3] <= BATCHED_MAX_NS and nblocks * nladder <= MAX_SLOTS


def block_native(shape, content, i):
    """native bytes of block i: random samples, a random walk, one constant, or samples of the full range of the width"""
    kind, bps, nch, ns, nb = shape
    seed = 9500 + 17 * i + ns % 89 + nch
    if content == "const":
        return lq.i32_to_native(np.full((nch, ns), (777 + 5 * i) % (1 << (8 * bps - 2)), dtype=np.int32), bps)
    if content == "full":
        return cases._rand_native(nch, ns, bps, seed, (1 << (8 * bps - 1)) - 1, walk=False)
    return cases._rand_native(nch, ns, bps, seed, 100 if bps == 1 else 3000, walk=content == "walk")


def batch_native(shape, nblocks, contents=CONTENTS):
    return np.stack([block_native(shape, contents[i % len(contents)], i) for i in range(nblocks)])


# ---- the rule ----------------------------------------------------------------------------------------------------------------

def choose(sizes, budget):
    """sizes: size_k of one block in ladder order, budget: its limit -> the chosen index"""
    sizes = [int(s) for s in sizes]
    fit = [k for k, s in enumerate(sizes) if s <= int(budget)]
    return fit[-1] if fit else sizes.index(min(sizes))


def derive_budgets(table):
    """table: size_k(b) as [nladder][nblocks] -> one budget per block, placed on the sizes themselves: block b < nladder sits
    exactly at entry b's size, block nladder one byte below its smallest entry (nothing fits), and the blocks behind it one byte
    below the size of entry 0, 1, ... in turn"""
    t = np.asarray(table).astype(np.int64)
    K, B = t.shape
    out = []
    for b in range(B):
        s = [int(v) for v in t[:, b]]
        out.append(s[b] if b < K else min(s) - 1 if b == K else s[(b - K - 1) % K] - 1)
    return out


def scalar_budget(table):
    """one budget for every block: the median of all candidate sizes"""
    return int(np.sort(np.asarray(table).reshape(-1))[np.asarray(table).size // 2])


# ---- the restated size -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.oracle import Oracle

    return Oracle()


def planes_of(kind, bps, nch, ns, nb, native, q):
    """the nb byte planes the packer hands to libhzr for this block at quality q, plane 0 (the low bytes) first"""
    c = dict(kind=kind, bps=bps, nch=nch, ns=ns, nb=nb, q=float(q))
    v, _ = lq.restated_stored(c, np.asarray(native, dtype=np.uint8))
    b = np.ascontiguousarray(v.astype(np.int32)).view(np.uint8).reshape(-1, 4)
    return [np.ascontiguousarray(b[:, k]) for k in range(nb)]


def restated_size(kind, bps, nch, ns, nb, native, q):
    """method byte, 3 bytes of mean per channel, then per plane a u32 length and the plane's libhzr stream"""
    return 1 + 3 * nch + sum(4 + len(oracle().hzr_encode(p)) for p in planes_of(kind, bps, nch, ns, nb, native, q))


# ---- the cases of tests/test_budget_rule.py: small enough for the CPU, each with the condition it exists for ----

def _rule(name, shape, ladder, nblocks, contents=CONTENTS):
    return dict(name=name, shape=shape, ladder=list(ladder), nblocks=nblocks, contents=tuple(contents))


def rule_cases():
    had = ("hadamard", 2, 5, 1024, 3)
    return [
        _rule("every_index", had, HADAMARD_LADDER, 9, contents=("rand", "walk")),  # at every entry, nothing fits, one below every entry
        _rule("unsorted", had, UNSORTED_LADDER, 5, contents=("rand",)),
        _rule("repeated", had, REPEATED_LADDER, 5, contents=("walk",)),
        _rule("constant", ("hadamard", 4, 3, 8, 2), HADAMARD_LADDER, 6, contents=("const",)),
        _rule("stored", ("hadamard", 4, 2, 64, 3), [1.0 / 16, 1.0, 64.0], 5, contents=("rand",)),  # plane 1: Huffman, then PlainCopy
        _rule("dct", ("dct", 3, 3, 100, 2), DCT_LADDER, 6, contents=("rand", "walk", "const")),
    ]


@functools.lru_cache(maxsize=None)
def _restated(name):
    c = next(c for c in rule_cases() if c["name"] == name)
    natives = batch_native(c["shape"], c["nblocks"], c["contents"])
    table = np.array([[restated_size(*c["shape"], natives[b], q) for b in range(c["nblocks"])] for q in c["ladder"]], dtype=np.int64)
    budgets = derive_budgets(table)
    return natives, table, budgets, [choose(table[:, b], budgets[b]) for b in range(c["nblocks"])]


def restated(c):
    """(native blocks, size table [nladder][nblocks], budgets, choices) of a rule case, computed once per process"""
    return _restated(c["name"])
