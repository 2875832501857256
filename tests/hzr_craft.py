"""A libhzr stream writer in plain Python/numpy, and the crafted streams of tests/test_hzr_foreign.py: valid streams that neither
encoder here writes (and a few invalid ones), for the decoder alone.

The format (hzr_decode.c:263-567): a stream is a u32 decoded size and one block per 65536 bytes; a block is
u16 payload length - 1, u32 CRC-32C of the payload, u8 mode (0 copy, 1 Huffman + RLE, 2 fill) and the payload.  A Huffman payload
is the tree in pre-order -- `0` = branch (child_a, then child_b), `1` + 9-bit symbol = leaf --, then one code per token, the
root's decision first and child_a = bit 0, a run token (symbols 256..260: 2 / 3.. / 7.. / 23.. / 279.. zeros) followed by its
0 / 2 / 4 / 8 / 14 extra bits; bits are packed LSB first and the last byte is padded.  A tree of one leaf still spends one bit
per token, whose value the reference ignores (hzr_decode.c:290,489-496).

A tree is a nested pair structure: an int is a leaf (its symbol), a 2-tuple a branch (child_a, child_b).  A symbol may sit on
several leaves: the writer then rotates over them, occurrence by occurrence.  Tokens are two arrays (Tokens): the symbol, and for
a run symbol the value of its extra bits.

The constants that the cases follow are read from rspt_amd/csrc/decode.hip (decoder_constants), so the cases move with them.
"""
import functools
import heapq
import os
import re
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 65536
MAX_LEAVES = 261
RUN_BASE = {256: 2, 257: 3, 258: 7, 259: 23, 260: 279}
RUN_EXTRA = {256: 0, 257: 2, 258: 4, 259: 8, 260: 14}
_BASE = np.array([1] * 256 + [RUN_BASE[s] for s in range(256, 261)], dtype=np.int64)
_EXTRA = np.array([0] * 256 + [RUN_EXTRA[s] for s in range(256, 261)], dtype=np.int64)
MODE_COPY, MODE_HUFF, MODE_FILL = 0, 1, 2
FAMILIES = "ABCDEFGH"


def _eb(sym):
    """extra bits behind each symbol (none behind a symbol that the format does not have)"""
    return np.where(sym <= 260, _EXTRA[np.minimum(sym, 260)], 0)


@functools.lru_cache(maxsize=None)
def decoder_constants():
    """the constants of k_dec_block that decide which path a block takes, from the source"""
    with open(os.path.join(ROOT, "rspt_amd", "csrc", "decode.hip")) as f:
        text = f.read()
    out = {}
    for name in ("kSerialTreePayload", "kLutBits", "kSubBits", "kSubSlots", "kDecMinChunkBits", "kDecThreads"):
        m = re.search(r"constexpr uint32_t (?:\w+ = \d+, )*%s = (\d+)\s*[,;]" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


@functools.lru_cache(maxsize=None)
def _orc():
    from oracle.oracle import Oracle

    return Oracle()


# ---- trees --------------------------------------------------------------------------------------------------------------
def walk(tree):
    """pre-order -> (description as (value, width) pairs, leaves as (symbol, code, length), branches as (depth, code))"""
    desc, leaves, branches, stack = [], [], [], [(tree, 0, 0)]
    while stack:
        nd, code, depth = stack.pop()
        if isinstance(nd, tuple):
            assert len(nd) == 2
            desc.append((0, 1))
            branches.append((depth, code))
            stack.append((nd[1], code | (1 << depth), depth + 1))
            stack.append((nd[0], code, depth + 1))
        else:
            assert 0 <= int(nd) < 512
            desc.append((1 | (int(nd) << 1), 10))
            leaves.append((int(nd), code, depth))
    return desc, leaves, branches


def tree_stats(tree):
    K = decoder_constants()
    _, leaves, branches = walk(tree)
    return {"leaves": len(leaves), "nodes": len(leaves) + len(branches), "depth": max(d for _, _, d in leaves),
            "long_prefixes": sum(1 for d, _ in branches if d == K["kLutBits"]),
            "dup": len(leaves) - len({s for s, _, _ in leaves}), "lengths": sorted({d for _, _, d in leaves})}


def comb(depth, side, syms):
    """the maximally skewed tree: one leaf per level 1 .. depth - 1 and two at `depth`; syms[0] is the leaf at the end of the
    deep side -- all-zero code for side 'a', all-one for 'b' --, syms[1] its sibling, syms[2:] the leaves from the bottom up"""
    assert len(syms) == depth + 1 and side in "ab"
    t = (syms[0], syms[1]) if side == "a" else (syms[1], syms[0])
    for s in syms[2:]:
        t = (t, s) if side == "a" else (s, t)
    return t


def complete(syms):
    """a complete tree over 2^k symbols: a fixed-length code"""
    syms = list(syms)
    if len(syms) == 1:
        return syms[0]
    assert len(syms) % 2 == 0
    return (complete(syms[: len(syms) // 2]), complete(syms[len(syms) // 2:]))


def huffman(counts, unused=()):
    """an ordinary Huffman tree of {symbol: count > 0}, built with a heap as any writer would; `unused` symbols get a leaf of
    weight 0 each"""
    heap = [(c, i, s) for i, (s, c) in enumerate(sorted(counts.items()))]
    heap += [(0, len(heap) + i, s) for i, s in enumerate(unused)]
    heapq.heapify(heap)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, (a[2], b[2])))
        tick += 1
    return heap[0][2]


def wide_tree(sub_sizes, syms, top=5):
    """2^top subtrees under a complete top; subtree i < len(sub_sizes) / 2 is a chain down to depth kLutBits - 1 whose end has two
    branches at depth kLutBits, each the root of a side-'a' comb of sub_sizes[.] leaves (codes of kLutBits + 1 .. bits); the other
    subtrees are leaves.  The symbols are taken from `syms` in order."""
    lut = decoder_constants()["kLutBits"]
    it = iter(syms)

    def sub(size):
        s = [next(it) for _ in range(size)]
        return comb(size - 1, "a", s) if size > 2 else (s[0], s[1])

    tops = []
    for i in range(1 << top):
        if 2 * i < len(sub_sizes):
            t = (sub(sub_sizes[2 * i]), sub(sub_sizes[2 * i + 1]))
            for _ in range(lut - 1 - top):
                t = (next(it), t) if i % 2 else (t, next(it))
            tops.append(t)
        else:
            tops.append(next(it))
    return complete_of(tops)


def complete_of(subtrees):
    if len(subtrees) == 1:
        return subtrees[0]
    return (complete_of(subtrees[: len(subtrees) // 2]), complete_of(subtrees[len(subtrees) // 2:]))


# ---- tokens -------------------------------------------------------------------------------------------------------------
class Tokens:
    def __init__(self, sym, extra=None):
        self.sym = np.asarray(sym, dtype=np.int64).reshape(-1)
        self.extra = np.zeros_like(self.sym) if extra is None else np.asarray(extra, dtype=np.int64).reshape(-1)
        assert self.sym.shape == self.extra.shape

    @classmethod
    def of(cls, items):
        """a list of literals and of (run symbol, run length)"""
        sym = [t[0] if isinstance(t, tuple) else t for t in items]
        extra = [t[1] - RUN_BASE[t[0]] if isinstance(t, tuple) else 0 for t in items]
        return cls(sym, extra)

    def __len__(self):
        return self.sym.size

    def lengths(self):
        """output bytes per token (a symbol above 260 -- never valid -- counts as none)"""
        ok = self.sym <= 260
        return np.where(ok, _BASE[np.minimum(self.sym, 260)] + self.extra, 0)

    def expand(self):
        ln = self.lengths()
        out = np.zeros(int(ln.sum()), dtype=np.uint8)
        lit = self.sym < 256
        out[(np.cumsum(ln) - ln)[lit]] = self.sym[lit]
        return out

    def back_to_back_runs(self):
        r = self.sym >= 256
        return int((r[1:] & r[:-1]).sum())


def run_piece(length):
    """the one token of `length` zeros (1 <= length <= 16662)"""
    if length == 1:
        return 0
    for s in (260, 259, 258, 257, 256):
        if length >= RUN_BASE[s]:
            assert length - RUN_BASE[s] < (1 << RUN_EXTRA[s]) or s == 256
            return (s, length)


def greedy_pieces(length):
    """as the encoders cut a zero run: the longest token first"""
    out = []
    while length:
        p = min(length, 16662)
        out.append(p)
        length -= p
    return out


def tokenise(data, pieces=greedy_pieces):
    """data -> Tokens; pieces(run length) cuts a zero run into token lengths (1 = the literal 0, 2 = a pair, ...)"""
    data = np.asarray(data, dtype=np.uint8)
    nz = np.flatnonzero(data)
    edges = np.concatenate(([-1], nz, [data.size]))
    pos, sym, extra = [nz], [data[nz].astype(np.int64)], [np.zeros(nz.size, dtype=np.int64)]
    rp, rs, re_ = [], [], []
    for g in np.flatnonzero(np.diff(edges) > 1):
        p = int(edges[g]) + 1
        for ln in pieces(int(edges[g + 1]) - p):
            t = run_piece(ln)
            rp.append(p)
            rs.append(t[0] if isinstance(t, tuple) else 0)
            re_.append(ln - RUN_BASE[t[0]] if isinstance(t, tuple) else 0)
            p += ln
        assert p == int(edges[g + 1])
    pos.append(np.array(rp, dtype=np.int64))
    sym.append(np.array(rs, dtype=np.int64))
    extra.append(np.array(re_, dtype=np.int64))
    order = np.argsort(np.concatenate(pos), kind="stable")
    return Tokens(np.concatenate(sym)[order], np.concatenate(extra)[order])


# ---- the writer ---------------------------------------------------------------------------------------------------------
def _bits(vals, widths):
    """LSB-first bits of the values, `widths` bits each (up to 64), as one uint8 array of 0 / 1"""
    vals, widths = np.asarray(vals, dtype=np.uint64), np.asarray(widths, dtype=np.int64)
    total = int(widths.sum())
    idx = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(widths) - widths, widths)
    return ((np.repeat(vals, widths) >> idx.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def huff_payload(tree, toks, leaf_bit=0, pad=0, max_leaves=MAX_LEAVES, cut_bits=None, facts=None):
    """the payload of a Huffman block.  leaf_bit: the bit per token of a single-leaf tree (a value, or an array of one per token);
    pad: the value of the pad bits; cut_bits: keep only that many bits of the whole (for invalid streams); facts: a dict that
    receives the number of pad bits."""
    desc, leaves, _ = walk(tree)
    assert len(leaves) <= max_leaves, "the compiled reference does not bound its node array: never more than 261 leaves"
    by_sym = {}
    for s, code, ln in leaves:
        by_sym.setdefault(s, []).append((code, ln))
    code = np.zeros(len(toks), dtype=np.uint64)
    clen = np.zeros(len(toks), dtype=np.int64)
    for s in np.unique(toks.sym):
        at = np.flatnonzero(toks.sym == s)
        ls = by_sym[int(s)]  # (KeyError: a token whose symbol the tree does not hold)
        which = np.arange(at.size) % len(ls)
        code[at] = np.array([c for c, _ in ls], dtype=np.uint64)[which]
        clen[at] = np.array([ln for _, ln in ls], dtype=np.int64)[which]
    if len(leaves) == 1:
        code[:] = np.asarray(leaf_bit, dtype=np.uint64)
        clen[:] = 1
    eb = _eb(toks.sym)
    assert ((toks.extra >= 0) & (toks.extra < (1 << eb))).all() and int((clen + eb).max(initial=0)) <= 64
    vals = code | (toks.extra.astype(np.uint64) << clen.astype(np.uint64))
    bits = np.concatenate([_bits([v for v, _ in desc], [w for _, w in desc]), _bits(vals, clen + eb)])
    if cut_bits is not None:
        bits = bits[:cut_bits]
    if facts is not None:
        facts["pad_bits"] = -bits.size % 8
    bits = np.concatenate([bits, np.full(-bits.size % 8, pad, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").tobytes()


def block(payload, mode=MODE_HUFF):
    assert 1 <= len(payload) <= BLOCK, len(payload)
    return struct.pack("<HIB", len(payload) - 1, _orc().crc32c(payload), mode) + payload


def huff_block(tree, toks, **kw):
    return block(huff_payload(tree, toks, **kw))


def stream(n, blocks):
    """the bare framing (hzr_decode.c:626-674): u32 decoded size, then the blocks"""
    assert len(blocks) == (n + BLOCK - 1) // BLOCK
    return struct.pack("<I", n) + b"".join(blocks)


def blocks_of(s):
    """the blocks of a sound bare stream"""
    n, pos, out = struct.unpack_from("<I", s, 0)[0], 4, []
    for _ in range((n + BLOCK - 1) // BLOCK):
        ln = 7 + struct.unpack_from("<H", s, pos)[0] + 1
        out.append(s[pos: pos + ln])
        pos += ln
    assert pos == len(s)
    return out


def splice(packer_stream, k, j, blk, hdr_len=0):
    """a sample packer's stream with block j of plane k replaced by `blk` (the plane's length field follows)"""
    from streamtools import parse_stream

    ps = parse_stream(packer_stream, hdr_len)
    out = bytearray(packer_stream[: 1 + hdr_len])
    for kk, pl in enumerate(ps["planes"]):
        body = bytearray(struct.pack("<I", pl["in_size"]))
        for jj, (mode, plen, crc, off) in enumerate(pl["blocks"]):
            body += blk if (kk, jj) == (k, j) else packer_stream[off: off + 7 + plen]
        out += struct.pack("<I", len(body)) + body
    return bytes(out)


def chunking(nbits):
    """the decoder's chunk rule (decode.hip, "chunks"): -> (nchunk, bits per chunk)"""
    K = decoder_constants()
    nchunk = min(max(-(-nbits // K["kDecMinChunkBits"]), 1), K["kDecThreads"])
    return nchunk, -(-nbits // nchunk)


# ---- contents -----------------------------------------------------------------------------------------------------------
def ordinary(n, seed=0):
    """(data, stream as the oracle's encoder writes it): the neighbour of a crafted stream in a batch.  Sparse-ish bytes: literals,
    runs of every class."""
    r = np.random.RandomState(1000 + seed)
    data = (r.randint(0, 256, n) * (r.randint(0, 4, n) == 0)).astype(np.uint8)
    if n > 600:
        data[n // 3: n // 3 + min(n // 4, 20000)] = 0
    return data, _orc().hzr_encode(data)


def runs_data(n, seed, even=False, begin_run=False, end_run=False):
    """literals between zero runs of every token class (1, 2, 3-6, 7-22, 23-278, 279-16662 and one longer than 16662 where it
    fits); even: every run has an even length"""
    assert not (even and (begin_run or end_run))
    r = np.random.RandomState(seed)
    out, total, first = [], 0, True
    long_left = 1 if n >= 40000 else 0
    while total < n:
        if not (first and begin_run):
            lit = r.randint(1, 200, int(r.randint(1, 40))).astype(np.uint8)
            out.append(lit)
            total += lit.size
        first = False
        cls = int(r.randint(0, 7))
        ln = [1, 2, int(r.randint(3, 7)), int(r.randint(7, 23)), int(r.randint(23, 279)), int(r.randint(279, 600)), 1][cls]
        if cls == 6 and long_left and total > n // 4:
            ln, long_left = 16662 + int(r.randint(1, 400)), 0
        if even:
            ln += ln & 1
        if begin_run and not out:
            ln = max(ln, 3)
        out.append(np.zeros(ln, dtype=np.uint8))
        total += ln
    data = np.concatenate(out)[:n].copy()
    if end_run:  # exactly five zeros behind a literal
        data[n - 6], data[n - 5:] = 7, 0
    elif data[-1] == 0:
        data[-1] = 7
    if even:  # the cut may have left one odd run: mend it with a literal
        z = np.concatenate(([0], (data == 0).astype(np.int8), [0]))
        st, en = np.flatnonzero(np.diff(z) == 1), np.flatnonzero(np.diff(z) == -1)
        for s_, e_ in zip(st, en):
            if (e_ - s_) & 1:
                data[s_] = 9
    if begin_run:
        assert data[0] == 0
    return data


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _case(name, data, s, expect="ok", ref_safe=True, **info):
    """expect: 'ok' -- the reference and the GPU decode it; 'gpu_refuses' -- the reference decodes it, the GPU flags it (stricter
    than hzr_decode, documented in rspt_hip.h); 'reject' -- the reference refuses it too.  ref_safe: may be given to the
    compiled reference."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    data.setflags(write=False)
    return dict(name=name, family=name[0], data=data, n=struct.unpack_from("<I", s, 0)[0], stream=s, expect=expect, ref_safe=ref_safe,
                crc32=zlib.crc32(s), **info)


def _one_block(name, data, tree, toks, expect="ok", ref_safe=True, leaf_bit=0, pad=0, max_leaves=MAX_LEAVES, cut_bits=None, **info):
    """a stream of one crafted block; its facts for the coverage asserts"""
    data = np.asarray(data, dtype=np.uint8)
    if expect != "reject":
        assert toks.expand().tobytes() == data.tobytes(), name
    facts = {}
    pl = huff_payload(tree, toks, leaf_bit=leaf_bit, pad=pad, max_leaves=max_leaves, cut_bits=cut_bits, facts=facts)
    st = tree_stats(tree)
    desc, leaves, _ = walk(tree)
    by = {}
    for s_, _, ln in leaves:
        by.setdefault(s_, set()).add(ln)
    used = sorted({ln for s_ in np.unique(toks.sym) for ln in by.get(int(s_), ())})
    longest = 0
    for s_ in np.unique(toks.sym):
        if int(s_) in by:
            longest = max(longest, max(by[int(s_)]) + RUN_EXTRA.get(int(s_), 0))
    nbits = 8 * len(pl) - sum(w for _, w in desc)
    return _case(name, data, stream(data.size, [block(pl)]), expect, ref_safe, L=len(pl), tree=st, used_lengths=used,
                 longest_token=longest, pad=pad, pad_bits=facts["pad_bits"], leaf_bit=leaf_bit if np.isscalar(leaf_bit) else "random", ntok=len(toks),
                 code_bits=nbits, chunks=chunking(nbits), run_pairs=toks.back_to_back_runs(),
                 first_is_run=bool(len(toks) and toks.sym[0] >= 256), last_is_run=bool(len(toks) and toks.sym[-1] >= 256), **info)


N_SMALL, N_BIG = 26001, 64001  # decoded sizes of the comb cases: a payload well under / over kSerialTreePayload


def _single_leaf_cases():
    K = decoder_constants()
    T = K["kSerialTreePayload"]
    out = []
    for leaf, tag in ((0x41, "lit"), (0, "lit0"), (256, "r256"), (257, "r257"), (258, "r258"), (259, "r259"), (260, "r260")):
        per = 1 + RUN_EXTRA.get(leaf, 0)  # bits per token
        sizes = [("L2" if leaf <= 258 else "Lmin", max(1, (16 - 10) // per))]
        if leaf <= 258:  # (23 zeros and more per 9 bits: a block is full long before 4095 bytes of payload)
            sizes += [("L%d" % L, (8 * L - 10) // per) for L in (T - 1, T)]
        for stag, ntok in sizes:
            # (few values of the extra bits where the tokens are many: the block has to hold the zeros)
            extra = np.random.RandomState(leaf * 7 + ntok).randint(0, min(1 << RUN_EXTRA.get(leaf, 0), 4 if ntok > 6 else 256), ntok)
            toks = Tokens(np.full(ntok, leaf), extra)
            for btag, bit in (("b0", 0), ("b1", 1), ("brand", np.random.RandomState(ntok).randint(0, 2, ntok))):
                c = _one_block("A_%s_%s_%s" % (tag, stag, btag), toks.expand(), leaf, toks, leaf_bit=bit, leaf=leaf)
                assert c["L"] == {"L2": 2, "Lmin": c["L"], "L%d" % (T - 1): T - 1, "L%d" % T: T}[stag], (c["name"], c["L"])
                out.append(c)
    # a block of zeros as run tokens only, under a single leaf
    toks = Tokens.of([(260, 16662)] * 3 + [(260, 15550)])
    for btag, bit in (("b0", 0), ("b1", 1)):
        out.append(_one_block("A_zeros65536_r260_%s" % btag, np.zeros(BLOCK, dtype=np.uint8), 260, toks, leaf_bit=bit, leaf=260))
    return out


def _comb_tokens(n, syms, deepest, seed):
    """n output bytes under a comb: every leaf once or more, the deepest leaf at seeded places (its extra bits: all ones once, all
    zeros once, seeded otherwise), the rest the two shallowest literals"""
    r = np.random.RandomState(seed)
    special = [s for s in syms if s != deepest] + [deepest] * 6
    sym = np.array(special, dtype=np.int64)[r.permutation(len(special))]
    eb = RUN_EXTRA.get(deepest, 0)
    extra = np.zeros(sym.size, dtype=np.int64)
    at = np.flatnonzero(sym == deepest)
    cap = min((1 << eb) - 1, n // 20)  # (seeded runs stay short: the block has to hold them all)
    extra[at] = r.randint(0, cap + 1, at.size)
    extra[at[0]], extra[at[1]] = (1 << eb) - 1, 0
    body = Tokens(sym, extra)
    fill = n - int(body.lengths().sum())
    assert fill > sym.size
    # the shallow literals fill the block; the special tokens are spread among them at seeded places, two of them back to back
    shallow = np.where(r.randint(0, 8, fill) == 0, syms[-2], syms[-1])
    where = np.sort(r.choice(fill - 1, sym.size, replace=False))
    where[1] = where[0]
    out_s = np.insert(shallow, where, sym)
    out_e = np.insert(np.zeros(fill, dtype=np.int64), where, extra)
    return Tokens(out_s, out_e)


def _comb_cases(depths, fam, expect, kinds):
    K = decoder_constants()
    out = []
    for D in depths:
        for side in "ab":
            for deepest in kinds:
                # literals 1 .. D on the other leaves (mod 255: the 40-bit comb has no more than 41 leaves anyway)
                syms = [deepest] + [1 + i for i in range(D)]
                if deepest < 256:
                    syms[0] = 200 + D % 50
                tree = comb(D, side, syms)
                for stag, n in (("small", N_SMALL), ("big", N_BIG)):
                    toks = _comb_tokens(n, syms, syms[0], D * 1000 + ord(side) + syms[0])
                    c = _one_block("%s_comb%d%s_%s_%s" % (fam, D, side, "lit" if deepest < 256 else "r%d" % deepest, stag), toks.expand(), tree, toks,
                                   expect=expect, depth=D, side=side, deepest=syms[0], align16=(D == 31 and deepest in (0, 260)))
                    assert (c["L"] < K["kSerialTreePayload"]) == (stag == "small") and c["L"] != K["kSerialTreePayload"], (c["name"], c["L"])
                    assert c["longest_token"] == D + RUN_EXTRA.get(syms[0], 0)
                    out.append(c)
    return out


WIDE_SMALL, WIDE_BIG = 2500, 20000  # decoded sizes of the wide cases (their codes are long: ~ a byte of payload per byte)
_WIDE_SIZES = [2, 2, 3, 2, 6, 2, 2, 8] * 5  # leaves under each of 40 ten-bit prefixes: codes of 11 .. 17 bits


def _wide_syms(nleaves, seed, full):
    r = np.random.RandomState(seed)
    if full:
        return [int(v) for v in r.permutation(261)]
    # 120 literals and the run symbols, most on two leaves; ten literals that the data never uses
    base = [int(v) for v in r.permutation(np.concatenate([np.arange(0, 120), np.arange(256, 261)]))]
    unused = list(range(200, 210))
    syms = (base * 3)[: nleaves - len(unused)]
    for i, u in enumerate(unused):
        syms.insert(5 + 17 * i, u)
    return syms


def _tokens_over(syms_used, n, seed, per_leaf):
    """n output bytes of seeded tokens over the symbols, each at least per_leaf[s] times; the tail is filled with literals"""
    r = np.random.RandomState(seed)
    must = np.array([s for s in syms_used for _ in range(per_leaf.get(s, 1))], dtype=np.int64)
    lits = np.array([s for s in syms_used if 0 < s < 256], dtype=np.int64)
    sym, extra, total = [], [], 0
    pool = must[r.permutation(must.size)]
    while True:
        e = np.where(pool >= 256, r.randint(0, 1 << 14, pool.size) % np.minimum(1 << _EXTRA[pool], 64), 0)
        t = Tokens(pool, e)
        ln = int(t.lengths().sum())
        if total + ln > n:
            keep = int(np.searchsorted(np.cumsum(t.lengths()), n - total, side="right"))
            sym.append(pool[:keep])
            extra.append(e[:keep])
            total += int(t.lengths()[:keep].sum())
            break
        sym.append(pool)
        extra.append(e)
        total += ln
        pool = np.array(syms_used, dtype=np.int64)[r.randint(0, len(syms_used), 4096)]
    sym.append(lits[r.randint(0, lits.size, n - total)])
    extra.append(np.zeros(n - total, dtype=np.int64))
    return Tokens(np.concatenate(sym), np.concatenate(extra))


def _wide_cases():
    K = decoder_constants()
    out = []
    assert len(_WIDE_SIZES) > K["kSubSlots"]
    nleaves = sum(_WIDE_SIZES) + (len(_WIDE_SIZES) // 2) * (K["kLutBits"] - 1 - 5) + (32 - len(_WIDE_SIZES) // 2)
    # duplicate and unused leaves
    syms = _wide_syms(nleaves, 77, False)
    tree = wide_tree(_WIDE_SIZES, syms)
    count = {}
    for s in syms:
        count[s] = count.get(s, 0) + 1
    used = sorted(set(syms) - set(range(200, 210)))
    for stag, n in (("small", WIDE_SMALL), ("big", WIDE_BIG)):
        toks = _tokens_over(used, n, 5 + n, count)
        c = _one_block("C_wide_dup_%s" % stag, toks.expand(), tree, toks, unused_leaves=10)
        assert (c["L"] < K["kSerialTreePayload"]) == (stag == "small")
        out.append(c)
    # all 261 symbols once each: 521 nodes.  Grow the subtrees until the leaves are 261.
    sizes, i = list(_WIDE_SIZES), 0
    while nleaves + sum(sizes) - sum(_WIDE_SIZES) < 261:
        sizes[(7 * i) % len(sizes)] += 1
        i += 1
    syms = _wide_syms(261, 78, True)
    tree = wide_tree(sizes, syms)
    assert tree_stats(tree)["nodes"] == 2 * MAX_LEAVES - 1
    deep = [s for s, _, ln in walk(tree)[1] if ln > K["kLutBits"] and s < 256]
    toks = Tokens(deep[:16])
    out.append(_one_block("C_full_16bytes", toks.expand(), tree, toks))
    toks = _tokens_over(list(range(261)), WIDE_BIG, 99, {})
    c = _one_block("C_full_big", toks.expand(), tree, toks)
    assert c["L"] >= K["kSerialTreePayload"] and set(np.unique(toks.sym)) == set(range(261))
    out.append(c)
    return out


def _fixed_size(width, desc_bits, nchunk_want, kind):
    """the largest block size whose code bits are cut into nchunk_want chunks of S bits with S a multiple of the code length
    ('aligned': every chunk starts on a code boundary) or S odd ('never': the chunks' starts run through every phase of the code)"""
    for n in range(BLOCK, 0, -1):
        nchunk, S = chunking(8 * -(-(desc_bits + width * n) // 8) - desc_bits)
        if nchunk == nchunk_want and (S % width == 0 if kind == "aligned" else S % 2 == 1):
            return n
    raise AssertionError((width, nchunk_want, kind))


def _fixed_cases():
    """fixed-length codes: a decoder that starts inside a code never falls into step, so the chunk rounds reach their bound"""
    K = decoder_constants()
    out = []
    for width, nsym, nchunk_want in ((4, 16, K["kDecThreads"]), (8, 256, 8)):
        tree = complete(list(range(nsym)) if width == 8 else [16 * i + 5 for i in range(16)])
        desc_bits = sum(w for _, w in walk(tree)[0])
        syms = np.array([s for s, _, _ in walk(tree)[1]], dtype=np.int64)
        for kind in ("never", "aligned"):
            n = _fixed_size(width, desc_bits, nchunk_want, kind)
            toks = Tokens(syms[np.random.RandomState(n).randint(0, nsym, n)])
            c = _one_block("D_fixed%d_%s" % (width, kind), toks.expand(), tree, toks, width=width, sync=kind)
            nchunk, S = c["chunks"]
            assert nchunk == nchunk_want and (S % width == 0) == (kind == "aligned") and (kind == "aligned" or S % 2 == 1), (c["name"], nchunk, S)
            out.append(c)
    return out


def _split_pieces(r, consecutive=False):
    def pieces(length):
        out = []
        while length:
            p = min(length, 16662, int(r.randint(1, 1 + min(length, 600)))) if not consecutive else min(length, max(2, int(r.randint(2, 40))))
            if consecutive and length - p == 1:
                p += 1 if p < 16662 else -1
            out.append(p)
            length -= p
        return out

    return pieces


def _huff_case(name, data, toks, unused=(), **kw):
    counts = {}
    for s, c in zip(*np.unique(toks.sym, return_counts=True)):
        counts[int(s)] = int(c)
    return _one_block(name, data, huffman(counts, unused), toks, **kw)


def _tokenisation_cases(n, tag):
    out = []
    d = runs_data(n, 31)
    out.append(_huff_case("E_lit0_%s" % tag, d, tokenise(d, lambda ln: [1] * ln), lit0_only=True))
    de = runs_data(n, 32, even=True)
    out.append(_huff_case("E_pairs_%s" % tag, de, tokenise(de, lambda ln: [2] * (ln // 2)), pairs_only=True))
    out.append(_huff_case("E_split_%s" % tag, d, tokenise(d, _split_pieces(np.random.RandomState(33)))))
    out.append(_huff_case("E_consecutive_%s" % tag, d, tokenise(d, _split_pieces(np.random.RandomState(34), consecutive=True))))
    db = runs_data(n, 35, begin_run=True, end_run=True)
    out.append(_huff_case("E_begin_end_run_%s" % tag, db, tokenise(db)))
    return out


def _edge_cases():
    out = []
    # payload of out_size - 1, out_size, out_size + 1 bytes: a 15-level comb over 64 bytes, the code lengths chosen to the bit
    syms = list(range(1, 17))
    tree = comb(15, "a", syms)
    lens = {s: ln for s, _, ln in walk(tree)[1]}
    desc_bits = sum(w for _, w in walk(tree)[0])
    n = 64
    for tag, L in (("Lm1", n - 1), ("L0", n), ("Lp1", n + 1)):
        for pad in (0, 1):
            want = 8 * L - 3 - desc_bits  # three pad bits
            base = want // n
            by_len = {ln: s for s, ln in lens.items()}
            sym = [by_len[base + 1]] * (want - base * n) + [by_len[base]] * (n - (want - base * n))
            toks = Tokens(np.array(sym)[np.random.RandomState(L).permutation(n)])
            c = _one_block("F_%s_pad%d" % (tag, pad), toks.expand(), tree, toks, pad=pad, out_minus_L=n - L)
            assert c["L"] == L
            out.append(c)
    # 65535 and 65536 bytes of payload: the 8-bit code over 65183 and 65184 bytes
    tree = complete(list(range(256)))
    for n in (65183, 65184):
        for pad in (0, 1):
            toks = Tokens(np.random.RandomState(n).randint(0, 256, n))
            c = _one_block("F_L%d_pad%d" % (n + 352, pad), toks.expand(), tree, toks, pad=pad)
            assert c["L"] == n + 352 and c["L"] in (65535, 65536)
            out.append(c)
    return out


def _multi_block_cases(e_big, e_small):
    """the crafted block first, in the middle and last among blocks that the oracle's encoder wrote"""
    out = []
    n = 2 * BLOCK + e_small["n"]
    d0, s0 = ordinary(n, 5)
    ob = blocks_of(s0)
    cb, cs = blocks_of(e_big["stream"])[0], blocks_of(e_small["stream"])[0]
    for tag, j in (("first", 0), ("middle", 1), ("last", 2)):
        data, blks = d0.copy(), list(ob)
        lo = j * BLOCK
        src = e_small if j == 2 else e_big
        data[lo: lo + src["n"]] = src["data"]
        blks[j] = cs if j == 2 else cb
        out.append(_case("F_multi_%s" % tag, data, stream(n, blks), position=tag, L=src["L"], pad=0))
    return out


def _beyond_cases():
    """what the reference decodes and the GPU refuses"""
    out = _comb_cases((32, 33, 40), "G", "gpu_refuses", (0, 260))
    # a leaf with symbol 300 that no token uses, in an otherwise ordinary tree
    for stag, n in (("small", 3000), ("big", BLOCK)):
        d = runs_data(n, 41)
        toks = tokenise(d)
        out.append(_huff_case("G_unused_leaf300_%s" % stag, d, toks, unused=(300,), expect="gpu_refuses", bad_leaf=300))
        assert (out[-1]["L"] < decoder_constants()["kSerialTreePayload"]) == (stag == "small")
    return out


def _reject_cases():
    out = []
    for stag, n in (("small", 3000), ("big", BLOCK)):
        d = runs_data(n, 51, end_run=True)
        toks = tokenise(d)
        # the last run one byte longer than the block has room for
        over = Tokens(toks.sym.copy(), toks.extra.copy())
        assert over.sym[-1] in (257, 258)
        over.extra[-1] += 1
        out.append(_huff_case("H_run_overruns_by_one_%s" % stag, d, over, expect="reject"))
        # symbol 300 on a leaf and in use
        bad = Tokens(np.concatenate([toks.sym[: len(toks) // 2], [300], toks.sym[len(toks) // 2:]]),
                     np.concatenate([toks.extra[: len(toks) // 2], [0], toks.extra[len(toks) // 2:]]))
        out.append(_huff_case("H_used_symbol300_%s" % stag, d, bad, expect="reject"))
    # the payload ends inside the tree's description
    d = runs_data(300, 52)
    toks = tokenise(d)
    out.append(_huff_case("H_description_cut", d, toks, expect="reject", cut_bits=43))
    # 262 leaves: one more than the format has symbols for.  Never for the compiled reference, whose node count is not bounded.
    for stag, n in (("small", 600), ("big", 6000)):
        syms = list(range(256)) + [256, 257, 258, 259, 260, 0]
        tree = complete_of([(syms[2 * i], syms[2 * i + 1]) if i < 6 else syms[6 + i] for i in range(256)])
        assert tree_stats(tree)["leaves"] == 262
        toks = Tokens(np.random.RandomState(n).randint(1, 250, n))
        c = _one_block("H_262_leaves_%s" % stag, toks.expand(), tree, toks, expect="reject", ref_safe=False, max_leaves=262)
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def craft_cases():
    """every crafted stream, named, seeded and deterministic (read-only: the list is shared)"""
    out = _single_leaf_cases()
    out += _comb_cases((10, 11, 15, 16, 30, 31), "B", "ok", (0, 256, 257, 258, 259, 260))
    out += _wide_cases()
    out += _fixed_cases()
    e_big, e_small = _tokenisation_cases(BLOCK, "65536"), _tokenisation_cases(5000, "5000")
    toks = Tokens.of([(260, 16662)] * 3 + [(260, 15550)])
    e_big.append(_one_block("E_zeros65536_4runs", np.zeros(BLOCK, dtype=np.uint8), huffman({260: 4}, unused=(1,)), toks))
    out += e_big + e_small
    out += _edge_cases()
    out += _multi_block_cases(e_big[2], e_small[2])
    out += _beyond_cases()
    out += _reject_cases()
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def by_family(f):
    return [c for c in craft_cases() if c["family"] == f]
