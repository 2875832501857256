"""Small helpers that every *_cases.py module shares: cutting and packing test inputs, the drivings of a recording as a stream,
and the text of a record file.  Nothing here knows a stage."""
import json
import zlib

import numpy as np


def _take(data, bps, nch, rows):
    """the first rows rows of native bytes, as a contiguous flat uint8 array"""
    d = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1)[: bps * nch * rows])
    assert d.size == bps * nch * rows
    return d


def _i32(a):
    """values -> the bytes of their int32s (native bytes at bps = 4), flat"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32)).view(np.uint8).reshape(-1)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def splits(nblocks, pattern):
    """the three drivings of a recording: all blocks in one call, one block per call, an uneven cut (the pattern's block counts,
    over and over)"""
    uneven, left, i = [], nblocks, 0
    while left:
        k = min(pattern[i % len(pattern)], left)
        uneven.append(k)
        left -= k
        i += 1
    return {"one_call": [nblocks], "per_block": [1] * nblocks, "uneven": uneven}


def record_text(out, per_line=("cases",)):
    """the text of a record file: a JSON object with one key per line and, for the keys of per_line (lists), one entry per line"""
    def value(key, v):
        return "[\n" + ",\n".join(json.dumps(e) for e in v) + "\n]" if key in per_line else json.dumps(v)

    return "{\n" + ",\n".join(json.dumps(key) + ": " + value(key, v) for key, v in out.items()) + "\n}\n"
