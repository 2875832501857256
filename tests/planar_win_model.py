"""The host's decomposition of a sliding-window stage on the planar int32 matrix (planar_win and win_split, host_stages.hip) and
the size of a carried state, restated once for the FIR and the median case lists (fir_planar_cases, median_planar_cases)."""


def geom(num_cu, nblocks, nch, ns, K, threads, run, min_lanes=1):
    """dict(lanes, rows_per_workgroup, chunk, span, nsplit) of a call with window K, as the host decides it: a lane holds `run`
    consecutive outputs, a workgroup `threads` lanes; a row takes the smallest power of two of lanes that covers it, at least
    min_lanes and at most threads; rows of more than one chunk are split into spans of whole chunks, each at least 4 (K - 1)
    samples, until there are about four workgroups per CU"""
    runs = (ns + run - 1) // run
    lanes = min_lanes
    while lanes < threads and lanes < runs:
        lanes *= 2
    rpw = threads // lanes
    C = lanes * run
    groups = (nblocks * nch + rpw - 1) // rpw
    want = 4 * num_cu
    nsplit = 1 if groups >= want else (want + groups - 1) // groups
    min_span = 4 * (K - 1) if K > 1 else 1
    nsplit = max(1, min(nsplit, ns // max(min_span, C)))
    span = ((ns + nsplit - 1) // nsplit + C - 1) // C * C
    return dict(lanes=lanes, rows_per_workgroup=rpw, chunk=C, span=span, nsplit=(ns + span - 1) // span)


def state_bytes(K, nch):
    """a uint64 header, then K - 1 rows of nch int32, to a multiple of 8"""
    return 8 + ((K - 1) * nch * 4 + 7) // 8 * 8
