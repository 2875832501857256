"""The probe of compress-to-a-byte-budget on the planar matrix, as compiled for gfx950: there is exactly one, and it uses no scratch
memory -- like k_budget_probe it keeps a row's transform in LDS and indexes a ladder that is a kernel argument."""
import re

import devframe as df
from devframe import asm  # noqa: F401


def test_the_planar_budget_probe_uses_no_scratch(asm):
    found = [n for n in asm if re.search(r"\dk_planar_budget_probe", n)]
    assert len(found) == 1, found
    df.uses_no_scratch(asm, found)
