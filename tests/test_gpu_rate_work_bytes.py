"""The bytes the six sizing calls of the rate-control entries name (rspt_hip_compress_{target,budget,total}[_planar]_work_bytes),
pinned to the sizes stated here from the plain numbers of a call, on every route each handle takes.  The same statement holds
the layouts themselves on the CPU (tests/cxx/rate_work_layout.cpp).  Nothing is launched."""
import pytest

import lossy_quantizer_cases as lq
from devframe import ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

# (kind, bps, nch, ns); the routes beyond the general one: hadamard rows of up to 8192 points (and nch * ns < 2^22, here always)
HANDLES = [("hadamard", 4, 3, 8), ("hadamard", 2, 12, 1024), ("hadamard", 3, 2, 8192), ("hadamard", 4, 2, 16384), ("dct", 4, 3, 100)]
BATCHES = [1, 3, 300]
LADDERS = [1, 5, 8]


def pad(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("handle", HANDLES, ids=lambda h: "%s-%d-%d-%d" % h)
def test_the_sizing_calls_name_the_stated_bytes(api, handle):
    kind, bps, nch, ns = handle
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    N = nch * ns
    nblk = (N + 65535) // 65536
    fast = kind == "hadamard" and ns <= 8192
    setters = [getattr(pk, "debug_set_%s_route" % rule) for rule in ("target", "budget", "total")]
    for rule in ("target", "budget", "total"):  # the faster route is refused where the shape never takes it
        assert getattr(api.lib(), "rspt_hip_debug_set_%s_route" % rule)(pk._h, 2) == (0 if fast else ERR_UNSUPPORTED), (handle, rule)
    seen = 0
    for route in (0, 1, 2) if fast else (0, 1):
        for setter in setters:
            setter(route)
        fused = fast and route != 1
        for B in BATCHES:
            for K in LADDERS:
                c = K * B
                copy, nz = pad(B * N * 4), pad(B * 4 * nblk * 4)
                tables = 2 * pad(8 * c) + 2 * pad(4 * c) + pad(32 * c)
                head = 2 * pad(8 * c) + 1280
                cut = copy if bps < 4 else 0
                tag = (handle, route, B, K)
                assert pk.target_work_bytes(B, K) == 2 * copy + nz + tables, tag
                assert pk.target_planar_work_bytes(B, K) == (16 if fused else max(16, cut + copy + nz)), tag
                assert pk.budget_work_bytes(B, K) == pad(8 * c) and pk.budget_planar_work_bytes(B, K) == pad(8 * c), tag
                assert pk.total_work_bytes(B, K) == (head + tables if fused else head + 2 * copy + nz + tables), tag
                assert pk.total_planar_work_bytes(B, K) == (head + tables if fused else head + cut + copy + nz + tables), tag
                seen += 1
    assert seen == (3 if fast else 2) * 9
    pk.close()
