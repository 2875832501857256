"""Compress a batch to one byte total (rspt_hip_compress_total_batch_dev): the rule, stated three times, and its CPU cases.

The rule (include/rspt_hip.h).  For block b and ladder entry k, size_k(b) is the budget entry's size and (prdn, mse, path) the
target entry's triple.  An entry is rated iff path == 0 and (mse == 0 or prdn is not a NaN); its figure is +0.0 where mse == 0,
else prdn.  At a level T the pick of a rated block is its rated entry of smallest size among those with a figure <= T, the
lowest index among equals; an unrated block takes its smallest stream.  T is admissible iff every rated block has a pick, cost(T)
is the sum of the picks' sizes, and T* is the smallest admissible T with cost(T) <= total -- +inf if there is none, +0.0 if no
block is rated.

choose_total is the brute force over every candidate level, choose_total_bisect an independent statement by bisection over the
bit patterns of the non-negative doubles, choose_total_np a vectorised form for large tables.  tests/test_total_rule.py holds the
three to each other and the cases below to the conditions they exist for; tests/test_gpu_total.py then holds the device to
choose_total on the composed oracle's tables.

The cases' tables come from budget_cases.restated_size and from target_cases.candidate + prdn_cases.prdn_parts, both held to the
reference's records.
"""
import functools
import math
import struct

import numpy as np

import budget_cases as bc
import prdn_cases
import target_cases as tc

INF = float("inf")
INF_BITS = 0x7FF0000000000000
NAN_BITS = 0x7FF8000000000000  # what the device reports for an unrated entry
U64_MAX = (1 << 64) - 1


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def rated(fig):
    prdn, mse, path = fig
    return path == 0 and (mse == 0.0 or prdn == prdn)


def figure(fig):
    """the figure of an entry: +0.0 where mse == 0, its PRDN where it is rated, a NaN where it is not"""
    return (0.0 if fig[1] == 0.0 else float(fig[0])) if rated(fig) else float("nan")


def reported(fig):
    """d_prdn of a chosen entry: its figure, or +inf where its path is 1"""
    return INF if fig[2] != 0 else figure(fig)


def _picks(sizes, figs, T):
    """(choice per block, or None where a rated block has no pick; cost) at level T"""
    K, B = len(sizes), len(sizes[0])
    choice, cost = [], 0
    for b in range(B):
        col = [k for k in range(K) if rated(figs[k][b])]
        if not col:
            k = min(range(K), key=lambda k: (int(sizes[k][b]), k))
        else:
            ok = [k for k in col if figure(figs[k][b]) <= T]
            if not ok:
                return None, None
            k = min(ok, key=lambda k: (int(sizes[k][b]), k))
        choice.append(k)
        cost += int(sizes[k][b])
    return choice, cost


def levels_of(figs):
    """every candidate level in ascending order: the rated figures, and +inf"""
    return sorted({figure(f) for row in figs for f in row if rated(f)} | {INF})


def cost_at(sizes, figs, T):
    """cost(T), or None where T is not admissible"""
    return _picks(sizes, figs, T)[1]


def choose_total(sizes, figs, total):
    """sizes: [K][B] ints, figs: [K][B] (prdn, mse, path), total: any uint64 -> (level, choice, cost): every candidate level in turn"""
    if not any(rated(f) for row in figs for f in row):
        choice, cost = _picks(sizes, figs, 0.0)
        return 0.0, choice, cost
    for T in levels_of(figs):
        choice, cost = _picks(sizes, figs, T)
        if choice is not None and (cost <= int(total) or T == INF):
            return T, choice, cost
    raise AssertionError("+inf is always admissible")


def choose_total_bisect(sizes, figs, total):
    """the same, by bisection over the patterns of [+0.0, +inf]: they order as the doubles do"""
    K, B = len(sizes), len(sizes[0])
    fb = [[bits(figure(figs[k][b])) if rated(figs[k][b]) else None for b in range(B)] for k in range(K)]

    def at(u):
        cost, choice = 0, []
        for b in range(B):
            have = [k for k in range(K) if fb[k][b] is not None]
            if have:
                have = [k for k in have if fb[k][b] <= u]
                if not have:
                    return None, None
            else:
                have = list(range(K))
            best = have[0]
            for k in have[1:]:
                if int(sizes[k][b]) < int(sizes[best][b]):
                    best = k
            choice.append(best)
            cost += int(sizes[best][b])
        return choice, cost

    if all(v is None for row in fb for v in row):
        choice, cost = at(0)
        return 0.0, choice, cost
    choice, cost = at(INF_BITS)
    if cost > int(total):
        return INF, choice, cost
    lo, hi = 0, INF_BITS
    while lo < hi:
        mid = (lo + hi) // 2
        c = at(mid)[1]
        if c is not None and c <= int(total):
            hi = mid
        else:
            lo = mid + 1
    choice, cost = at(hi)
    return from_bits(hi), choice, cost


def np_rule(sizes, prdn, mse, path):
    """for large tables -- sizes, prdn, mse, path: [K][B] arrays -> (the candidate levels in ascending order, any block rated,
    at(T) -> (choice array, cost) or (None, None)): every level's picks by masked minima over the ladder axis"""
    sizes = np.asarray(sizes).astype(np.int64)
    prdn, mse, path = np.asarray(prdn, dtype=np.float64), np.asarray(mse, dtype=np.float64), np.asarray(path)
    K, B = sizes.shape
    is_rated = (path == 0) & ((mse == 0.0) | ~np.isnan(prdn))
    fig = np.where(mse == 0.0, 0.0, prdn)
    block_rated = is_rated.any(axis=0)
    big = np.iinfo(np.int64).max

    def at(T):
        with np.errstate(invalid="ignore"):
            ok = np.where(block_rated[None, :], is_rated & (fig <= T), True)
        masked = np.where(ok, sizes, big)
        choice = masked.argmin(axis=0)  # (the lowest index among equals)
        best = masked[choice, np.arange(B)]
        if (best == big).any():
            return None, None
        return choice, sum(int(v) for v in best)

    return np.unique(np.concatenate([fig[is_rated], [INF]])), bool(block_rated.any()), at


def choose_total_np(sizes, prdn, mse, path, total):
    """the rule on np_rule's form: the level by a search of the sorted figures -> (level, choice array, cost)"""
    levels, any_rated, at = np_rule(sizes, prdn, mse, path)
    if not any_rated:
        choice, cost = at(0.0)
        return 0.0, choice, cost
    choice, cost = at(INF)
    if cost > int(total):
        return INF, choice, cost
    lo, hi = 0, len(levels) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        c = at(levels[mid])[1]
        if c is not None and c <= int(total):
            hi = mid
        else:
            lo = mid + 1
    choice, cost = at(levels[hi])
    return float(levels[hi]), choice, cost


def some_totals_np(sizes, prdn, mse, path, n=8):
    """some_totals for large tables: the costs of n levels spread over the admissible ones, some of them one byte lower, below
    cost(+inf), 0 and 2^64 - 1"""
    levels, any_rated, at = np_rule(sizes, prdn, mse, path)
    costs = [c for c in (at(levels[i * (len(levels) - 1) // max(1, n - 1)])[1] for i in range(n)) if c is not None]
    keep = {0, U64_MAX, at(INF)[1] - 1} | set(costs[::2]) | {c - 1 for c in costs[1::2]}
    return _at_least_six(keep, at(INF)[1])[: n + 2]


def derive_totals(sizes, figs):
    """totals placed on the table itself: cost(L) for every admissible level L and one byte below it, one byte below cost(+inf)
    and 0 (both misses), and 2^64 - 1 (the lowest admissible level)"""
    out = []
    for T in levels_of(figs):
        c = cost_at(sizes, figs, T)
        if c is not None:
            out += [c, c - 1]
    return sorted(set(out) | {0, U64_MAX})


def some_totals(sizes, figs, n=8):
    """at most n of derive_totals, spread over them, with both ends and the miss below cost(+inf)"""
    t = derive_totals(sizes, figs)
    keep = {0, U64_MAX, cost_at(sizes, figs, INF) - 1} | {t[i * (len(t) - 1) // (n - 1)] for i in range(n)}
    return _at_least_six(keep, cost_at(sizes, figs, INF))[: n + 2]


def _at_least_six(keep, least):
    """a table of few costs (a tiny shape, equal sizes) places few totals: fill up with totals beside the least cost"""
    for extra in (1, least + 1, U64_MAX - 1, least // 2):
        if len(keep) < 6:
            keep = keep | {extra}
    return sorted(keep)


# ---- the cases of tests/test_total_rule.py: small enough for the CPU, each with the condition it exists for ----

def _case(name, shape, ladder, nblocks, contents, copy=None):
    return dict(name=name, shape=shape, ladder=list(ladder), nblocks=nblocks, contents=tuple(contents), copy=copy)


def rule_cases():
    had = ("hadamard", 2, 5, 1024, 3)
    return [
        _case("sorted", had, bc.HADAMARD_LADDER, 6, ("rand", "walk")),
        _case("unsorted", had, bc.UNSORTED_LADDER, 6, ("rand", "walk")),
        _case("constant", ("hadamard", 4, 3, 8, 2), bc.HADAMARD_LADDER, 4, ("const", "rand")),
        _case("unrated", ("hadamard", 4, 2, 64, 1), [1.0 / 4, 1.0, 64.0], 3, ("full", "rand", "full")),
        _case("dct", ("dct", 3, 3, 100, 2), bc.DCT_LADDER, 3, ("rand", "walk", "const")),
        _case("twins", had, bc.HADAMARD_LADDER, 6, ("rand", "walk"), copy=(2, 0)),  # block 2 is a copy of block 0
    ]


def natives_of(c):
    x = bc.batch_native(c["shape"], c["nblocks"], c["contents"])
    if c["copy"]:
        x[c["copy"][0]] = x[c["copy"][1]]
    return x


@functools.lru_cache(maxsize=None)
def _block_tables(shape, ladder, native_bytes):
    kind, bps, nch, ns, nb = shape
    native = np.frombuffer(native_bytes, dtype=np.uint8)
    t = dict(kind=kind, bps=bps, nch=nch, ns=ns, nb=nb)
    sizes, figs = [], []
    for q in ladder:
        sizes.append(bc.restated_size(kind, bps, nch, ns, nb, native, q))
        p, mse, ref, path, info = prdn_cases.prdn_parts(native, tc.candidate(t, native, q), bps, nch, ns)
        figs.append((float(p), float(mse), int(path)))
    return sizes, figs


def restated(c):
    """(sizes [K][B], figs [K][B] of (prdn, mse, path)) of a rule case; a block's column is computed once per process"""
    cols = [_block_tables(c["shape"], tuple(c["ladder"]), n.tobytes()) for n in natives_of(c)]
    K = len(c["ladder"])
    return [[col[0][k] for col in cols] for k in range(K)], [[col[1][k] for col in cols] for k in range(K)]


def same_level(a, b):
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))
