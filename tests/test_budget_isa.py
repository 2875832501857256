"""The kernels of compress-to-a-byte-budget, as compiled for gfx950: none of them uses scratch memory -- the batched route's probe
keeps a row's transform in LDS and indexes a ladder that is a kernel argument."""
import re

import devframe as df
from devframe import asm  # noqa: F401

NEW = {"k_budget_probe": 1, "k_budget_sizes": 1, "k_budget_select": 1}


def test_the_budget_kernels_use_no_scratch(asm):
    names = []
    for stem, count in NEW.items():
        found = [n for n in asm if re.search(r"\d%s" % stem, n)]
        assert len(found) == count, (stem, found)
        names += found
    df.uses_no_scratch(asm, names)
