"""The probe of compress-a-batch-to-one-byte-total on the planar matrix, as compiled for gfx950: there is exactly one, and it uses no
scratch memory -- like k_total_probe it keeps a row's transform and its round trip in LDS and indexes ladders that are kernel
arguments."""
import re

import devframe as df
from devframe import asm  # noqa: F401


def test_the_planar_total_probe_uses_no_scratch(asm):
    found = [n for n in asm if re.search(r"\dk_planar_total_probe", n)]
    assert len(found) == 1, found
    df.uses_no_scratch(asm, found)
