"""The kernels of the quality ladder and of compress-to-a-PRDN-target, as compiled for gfx950: none of them uses scratch memory
-- the fused probe keeps a row's samples in registers beside the butterflies' values, and the ladder kernels index a table that
is a kernel argument."""
import re

import devframe as df
from devframe import asm  # noqa: F401

NEW = {"k_target_probe": 1, "k_target_select": 1, "k_fwht_lI": 2, "k_fwht64k_lI": 2, "k_fwht_cross_lI": 2, "k_dct_lI": 2, "k_wide_native_lI": 4,
       "k_ladder_refuse": 1, "k_ladder_flag": 1}


def test_the_ladder_and_target_kernels_use_no_scratch(asm):
    names = []
    for stem, count in NEW.items():
        found = [n for n in asm if re.search(r"\d%s" % stem, n)]
        assert len(found) == count, (stem, found)
        names += found
    df.uses_no_scratch(asm, names)
