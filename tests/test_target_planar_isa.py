"""The kernels of the planar ladder and target entries and of the choice in the container index, as compiled for gfx950: none of
them uses scratch memory (the check of tests/test_target_isa.py)."""
import re

import devframe as df
from devframe import asm  # noqa: F401

NEW = {"k_planar_target_probe": 1, "k_planar_emit_l": 1, "k_pack_choice_sizes": 1, "k_pack_choice_bits": 1, "k_index_choices": 1}


def test_the_new_kernels_use_no_scratch(asm):
    names = []
    for stem, count in NEW.items():
        found = [n for n in asm if re.search(r"\d%sE" % stem, n)]
        assert len(found) == count, (stem, found)
        names += found
    df.uses_no_scratch(asm, names)
