"""The kernels of the quality ladder and of the rate-control entries -- compress to a PRDN target, to a byte budget, to one byte
total, each from native blocks and from the planar matrix -- as compiled for gfx950: each is there as often as stated, and none
uses scratch memory.  The probes keep a row's samples or its transform (and its round trip) in registers or LDS
and index ladders that are kernel arguments; the ladder kernels index a table that is a kernel argument; the level kernel keeps
its thread's block, kMaxLadder (figure, size) cells, in registers."""
import re

import pytest

import devframe as df
from devframe import asm  # noqa: F401

# group -> (what follows the stem in a mangled name, {stem: count})
KERNELS = {
    "ladder and target": ("", {"k_target_probe": 1, "k_target_select": 1, "k_fwht_lI": 2, "k_fwht64k_lI": 2, "k_fwht_cross_lI": 2, "k_dct_lI": 2,
                               "k_wide_native_lI": 4, "k_ladder_refuse": 1, "k_ladder_flag": 1}),
    "planar ladder, target and the choice in the index": ("E", {"k_planar_target_probe": 1, "k_planar_emit_l": 1, "k_pack_choice_sizes": 1,
                                                                "k_pack_choice_bits": 1, "k_index_choices": 1}),
    "budget": ("", {"k_budget_probe": 1, "k_budget_sizes": 1, "k_budget_select": 1}),
    "planar budget": ("", {"k_planar_budget_probe": 1}),
    "total": ("", {"k_total_probe": 1, "k_total_figs": 1, "k_total_level": 1, "k_total_round": 1, "k_total_pick": 1}),
    "planar total": ("", {"k_planar_total_probe": 1}),
}


@pytest.mark.parametrize("group", KERNELS, ids=lambda g: g.replace(" ", "_").replace(",", ""))
def test_the_kernels_use_no_scratch(asm, group):
    end, stems = KERNELS[group]
    names = []
    for stem, count in stems.items():
        found = [n for n in asm if re.search(r"\d%s%s" % (stem, end), n)]
        assert len(found) == count, (stem, found)
        names += found
    df.uses_no_scratch(asm, names)
