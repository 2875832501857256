"""The CRC-32C of a staged small block as one wave of k_tree computes it (tools/kernel_model.py: crc_wave_words -- words across the
64 lanes, counted from the end of X || payload, ceil(words / 64) Horner steps), against the oracle's CRC on the CPU.

The lengths: every payload length from 1 to 300 bytes -- one and two steps, every byte offset of the last word, the lanes that
hold no word, a missing and a partial top word -- and the lengths around the largest staged payload (3072 bytes, 13 steps)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_model as km  # noqa: E402

import cases

LENGTHS = list(range(1, 301)) + list(range(3069, 3077))


@pytest.fixture(scope="module")
def message():
    m = cases.hash_bytes(max(LENGTHS), 4242).tobytes()
    assert len(set(m)) > 200
    return m


def test_wave_crc_equals_the_oracles_for_every_length(orc, message):
    for n in LENGTHS:
        assert km.crc_wave_words(message[:n]) == orc.crc32c(message[:n]), n


def test_wave_crc_of_zeros_and_ones(orc):
    """the prefix X alone decides the CRC of a run of zero bytes; all-ones words exercise every bit of the shift constants"""
    for n in (1, 4, 252, 253, 256, 3072):
        for fill in (b"\x00", b"\xff"):
            assert km.crc_wave_words(fill * n) == orc.crc32c(fill * n), (n, fill)


def test_wave_crc_with_fewer_lanes_takes_more_steps(orc, message):
    """the same decomposition at 8 lanes: 300 bytes are then 10 steps, as 3072 are 13 at 64 lanes"""
    for n in (31, 32, 33, 299, 300):
        assert km.crc_wave_words(message[:n], lanes=8) == orc.crc32c(message[:n]), n
