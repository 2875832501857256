"""Host-side checks of the raw hzr byte-buffer codec (RSPT_HIP_KIND_BYTES): the size bound against the oracle's, and the
argument checks rspt_hip_packer_create makes before it touches a device.  No GPU needed."""
import ctypes as C
import random

from devframe import ERR_ARG


def test_hzr_max_compressed_size_is_the_oracles(orc):
    from rspt_amd import api

    ns = [0, 1, 65535, 65536, 65537, 2**31 - 1]
    rng = random.Random(20240)
    ns += [rng.randrange(0, 2**31) for _ in range(500)] + [rng.randrange(0, 1 << 20) for _ in range(500)]
    for n in ns:
        assert api.hzr_max_compressed_size(n) == orc.hzr_max_compressed_size(n), n
    assert api.hzr_max_compressed_size(0) == 4


def test_bytes_kind_arguments_are_checked_before_the_device():
    from rspt_amd import api

    L = api.lib()

    def create(kind, bps, nch, ns, nb):
        h = C.c_void_p()
        rc = L.rspt_hip_packer_create(C.byref(h), kind, bps, nch, ns, nb, 0)
        if rc == 0:
            L.rspt_hip_packer_destroy(h)
        return rc

    assert create(4, 2, 1, 16, 0) == ERR_ARG  # a byte buffer has bps = 1 ...
    assert create(4, 1, 2, 16, 0) == ERR_ARG  # ... and one channel
    assert create(4, 1, 1, 0, 0) == ERR_ARG  # in_size >= 1
    assert create(4, 1, 1, 2**31, 0) == ERR_ARG  # in_size < 2^31
    assert create(5, 1, 1, 16, 0) == ERR_ARG  # there is no kind 5
    # a valid shape gets past the argument checks (nb is ignored): the device decides the rest
    assert create(4, 1, 1, 16, 0) != ERR_ARG
    assert create(4, 1, 1, 2**31 - 1, 7) != ERR_ARG
    assert api.KINDS["bytes"] == api.KIND_BYTES == 4
