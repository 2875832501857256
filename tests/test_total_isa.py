"""The kernels of compress-a-batch-to-one-byte-total, as compiled for gfx950: none of them uses scratch memory -- the fused probe
keeps a row's transform and its round trip in LDS and indexes ladders that are kernel arguments, and the level kernel keeps its
thread's block, kMaxLadder (figure, size) cells, in registers."""
import re

import devframe as df
from devframe import asm  # noqa: F401

NEW = {"k_total_probe": 1, "k_total_figs": 1, "k_total_level": 1, "k_total_round": 1, "k_total_pick": 1}


def test_the_total_kernels_use_no_scratch(asm):
    names = []
    for stem, count in NEW.items():
        found = [n for n in asm if re.search(r"\d%s" % stem, n)]
        assert len(found) == count, (stem, found)
        names += found
    df.uses_no_scratch(asm, names)
