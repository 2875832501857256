"""Seeded byte streams of every density for the hzr kernels (tests/test_gpu_fuzz.py, tests/soak.py).  The densities steer the
encoder through all of its row paths: dense quads, quads with long run tokens, register slots, the token queue of light blocks, the
one-wave small-block encoder, Fill and PlainCopy blocks, runs across the 16662 cap and across 64 KiB block edges."""
import numpy as np

KINDS = ["dense", "peaky", "medium", "sparse", "bursty", "noise", "const", "twos", "deep", "wide", "deeprun"]


def _geom(k, q):
    p = q ** np.arange(k)
    return p / p.sum()


def gen(seed, n, kind):
    r = np.random.default_rng(seed)
    if kind == "dense":  # almost no zeros, wide alphabet
        x = r.integers(1, 256, n, dtype=np.int64)
        z = r.random(n) < 0.03
        x[z] = 0
    elif kind == "peaky":  # a few very frequent symbols + rare ones (long codes), some zeros
        x = r.choice(np.arange(256), size=n, p=_geom(256, 0.35))
    elif kind == "medium":  # ~8 % tokens: literal followed by a short run
        x = np.zeros(n, dtype=np.int64)
        pos = np.cumsum(r.integers(2, 24, n // 8))
        pos = pos[pos < n]
        x[pos] = r.integers(1, 6, pos.size)
    elif kind == "sparse":  # long runs, some beyond the 16662 cap
        x = np.zeros(n, dtype=np.int64)
        pos = np.cumsum(r.integers(1, 40000, max(2, n // 9000)))
        pos = pos[pos < n]
        x[pos] = r.integers(1, 256, pos.size)
    elif kind == "bursty":  # dense stretches and empty stretches alternate (rows of both kinds inside one block)
        x = np.zeros(n, dtype=np.int64)
        p = 0
        while p < n:
            ln = int(r.integers(50, 6000))
            if r.random() < 0.5:
                x[p : p + ln] = r.integers(0, 256, min(ln, n - p))
            p += ln
    elif kind == "noise":  # incompressible: PlainCopy
        x = r.integers(0, 256, n, dtype=np.int64)
    elif kind == "const":
        x = np.full(n, int(r.integers(0, 256)), dtype=np.int64)
    elif kind == "twos":  # runs of exactly one and two zeros everywhere (symbols 0 and 256)
        x = r.integers(1, 40, n, dtype=np.int64)
        idx = r.integers(0, n - 3, n // 6)
        x[idx] = 0
        idx2 = r.integers(0, n - 3, n // 9)
        x[idx2] = 0
        x[idx2 + 1] = 0
    elif kind == "deep":  # Fibonacci counts: codes of up to ~21 bits in dense rows, the rarest symbols side by side (pairs of codes > 32 bits)
        fib = [1, 1]
        while sum(fib) + fib[-1] + fib[-2] <= n:
            fib.append(fib[-1] + fib[-2])
        vals = np.concatenate([np.full(c, 10 + i, dtype=np.int64) for i, c in enumerate(fib)])
        rest = n - vals.size
        x = np.concatenate([vals[:8], r.permutation(vals[8:]), np.full(rest, 10 + len(fib) - 1, dtype=np.int64)])  # rare ones first, in order
    elif kind == "deeprun":  # "deep" with one run of 300 zeros: the long-run symbol (14 extra bits) is the rarest, so its code is the
        # deepest -- code + extra bits reach past 32 stream bits (the decoder's 64-bit window branch)
        if n > 1000:
            y = gen(seed, n - 300, "deep").astype(np.int64)  # (inserted, not overwritten: the Fibonacci counts stay what they are)
            x = np.concatenate([y[: n // 2], np.zeros(300, dtype=np.int64), y[n // 2 :]])
        else:
            x = gen(seed, n, "deep").astype(np.int64)
    elif kind == "wide":  # five heavy symbols over 250 equally rare ones: ~100 ten-bit prefixes lead to longer codes (the decoder's
        # second-level table has 32 slots: the rest walk the tree) -- and the payload is long enough for the parallel tree recovery
        x = r.choice(np.arange(5, 255), size=n)
        u = r.random(n)
        for v, q in ((4, 0.92), (3, 0.84), (2, 0.72), (1, 0.52), (0, 0.28)):
            x[u < q] = v
    else:
        raise ValueError(kind)
    return x.astype(np.uint8)
