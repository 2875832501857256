"""Compress to a PRDN target (rspt_hip_compress_target_batch_dev): inputs, ladders, targets and a numpy restatement of the rule.

The rule (include/rspt_hip.h).  For block b and ladder entry k: o is the native block, d_k what decompress(compress(o)) gives
at ladder[k] and the handle's nb, (prdn_k, mse_k, path_k) what the PRDN stage says of (o, d_k).  Entry k meets the target iff
path_k == 0 and (mse_k == 0 or prdn_k <= target); a NaN never does.  The choice is the first k in ladder order that meets it,
and the last entry if none does; the reported PRDN is the chosen entry's, +inf where its path is 1.

The restatement is built on lossy_quantizer_cases' transforms and cuts and on prdn_cases' restatement of the figure, both held
to the reference's records (tests/test_lossy_quantizer_record.py, tests/test_prdn.py): the hzr stage between the cut and the
way back changes no value and is left out here, as the device leaves it out for the candidates.

tests/test_target_rule.py holds the cases to the conditions they exist for, on the CPU: which entries get chosen, and that no
candidate's PRDN lies on a rounding edge of its target.
"""
import functools

import numpy as np

import cases
import lossy_quantizer_cases as lq
import prdn_cases

HADAMARD_LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0, 64.0]  # coarse to fine: a larger quality is finer
DCT_LADDER = [1024.0, 128.0, 16.0, 1.0]                  # coarse to fine: a larger quality is coarser
FUSED_MAX_NS = 8192  # kTpMaxNs of target.hip
EDGE = 1e-9  # no candidate's PRDN may lie this close (relative) to its case's target


def _case(name, kind, bps, nch, ns, nb, target, ladder=None, nblocks=3, amp=3000, seed=0, src="rand", special=None, routes=False):
    """special: {block index: "const" | "calm"} -- a constant block (ref == 0, the PRDN is a NaN: only mse == 0 can take an entry) or one of
    small samples in a case of full-scale ones (whose candidates' error sums leave 2^53: path 1).  routes: a hadamard shape both routes of the device run."""
    ladder = list(HADAMARD_LADDER if kind == "hadamard" else DCT_LADDER) if ladder is None else list(ladder)
    return dict(name=name, kind=kind, bps=bps, nch=nch, ns=ns, nb=nb, target=float(target), ladder=ladder, nblocks=nblocks, amp=amp, seed=seed,
                src=src, special=special or {}, routes=routes)


def all_cases():
    C = []
    # every hadamard shape of tests/test_gpu_target.py; the targets are placed by hand between the candidates' figures.  routes:
    # where the fused probe runs (rows of up to FUSED_MAX_NS points, nch * ns < 2^22); (12, 8192) is its longest row
    C.append(_case("had_3x8_nb3", "hadamard", 4, 3, 8, 3, 9.0, seed=1, nblocks=4, special={2: "const"}, routes=True))
    C.append(_case("had_i16_5x1024_nb2", "hadamard", 2, 5, 1024, 2, 1.5, seed=2, routes=True))
    C.append(_case("had_12x8192_nb3", "hadamard", 4, 12, 8192, 3, 1.0, seed=3, nblocks=2, src="synth", routes=True))
    C.append(_case("had_2x16384_nb3", "hadamard", 4, 2, 16384, 3, 1.0, seed=4, nblocks=2, src="synth"))  # above the fused bound
    C.append(_case("had_2x32768_nb2", "hadamard", 4, 2, 32768, 2, 2.0, seed=5, nblocks=2, src="synth"))
    # no entry meets it: the last one is taken
    C.append(_case("had_i8_3x8_nb1_none", "hadamard", 1, 3, 8, 1, 1e-3, ladder=[1.0 / 16, 1.0 / 4, 1.0], amp=100, seed=6, routes=True))
    # full-scale samples at nb = 1 (as had_2x64_full_scale_* of lossy_quantizer_cases): the coarse candidates' error sums leave
    # 2^53 and are passed over whatever the target; one calm block beside them
    C.append(_case("had_2x64_full_scale_nb1", "hadamard", 4, 2, 64, 1, 1e6, ladder=[1.0 / 4, 1.0, 64.0], amp=(1 << 31) - 1, seed=7,
                   special={1: "calm"}, routes=True))
    # nch * ns just below and at 2^22: where the host switches routes
    C.append(_case("had_511x8192_nb3", "hadamard", 4, 511, 8192, 3, 1.0, ladder=[1.0 / 4, 4.0], nblocks=1, seed=8, src="synth", routes=True))
    C.append(_case("had_512x8192_nb3", "hadamard", 4, 512, 8192, 3, 1.0, ladder=[1.0 / 4, 4.0], nblocks=1, seed=9, src="synth"))
    # dense dct
    C.append(_case("dct_3x100_nb2", "dct", 4, 3, 100, 2, 30.0, seed=10))
    C.append(_case("dct_i24_2x257_nb3", "dct", 3, 2, 257, 3, 1.0, amp=1 << 20, seed=11, special={1: "const"}))
    return C


def block_native(c, i):
    """native bytes of block i of case c"""
    kind = c["special"].get(i)
    if kind == "const":
        x = np.full((c["nch"], c["ns"]), 1234 % (1 << (8 * c["bps"] - 2)), dtype=np.int32)
        return lq.i32_to_native(x, c["bps"])
    if kind == "calm":
        return cases._rand_native(c["nch"], c["ns"], c["bps"], 9100 + 2 * c["seed"] + i, 3000, walk=False)
    if c["src"] == "synth":
        from rspt_amd import synth

        # blocks of different amplitude: the same ladder entry leaves them different PRDN
        x = synth.synth_native(c["nch"], c["ns"], block_index=c["seed"] + i, bps=4, ecg=True).numpy().reshape(-1).view(np.int32)
        x = (x.astype(np.int64) >> (6 * i)).astype(np.int32) if c["bps"] == 4 else x
        return np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return cases._rand_native(c["nch"], c["ns"], c["bps"], 9000 + 2 * c["seed"] + i, c["amp"] >> (3 * i), walk=False)


def mean24(m):
    """what the stream's header keeps of a mean: its low 24 bits, sign-extended (the decoder never sees more)"""
    return ((m.view(np.uint32) << np.uint32(8)).view(np.int32) >> 8).astype(np.int32)


def candidate(c, native, q):
    """the decoded native block of `native` at quality q and the case's nb"""
    x = lq.native_to_i32(native, c["bps"], c["nch"], c["ns"])
    if c["kind"] == "hadamard":
        y, m = lq.hadamard_forward(x, q)
        v = lq.cut_to_nb(y.reshape(-1), c["nb"]).reshape(x.shape)
        back = lq.hadamard_inverse(v, mean24(m), q)
    else:
        y, m = lq.dct_forward(x, q)
        v = lq.xdelta_inverse(lq.cut_to_nb(lq.xdelta_forward(y.reshape(-1)), c["nb"])).reshape(x.shape)
        back = lq.dct_inverse(v, mean24(m), q)
    return lq.i32_to_native(back, c["bps"])


def meets(prdn, mse, path, target):
    return path == 0 and (mse == 0.0 or prdn <= target)  # (a NaN compares false)


def choose(figs, target):
    """figs: [(prdn, mse, path)] in ladder order -> (choice, reported prdn)"""
    k = next((k for k, (p, m, path) in enumerate(figs) if meets(p, m, path, target)), len(figs) - 1)
    return k, (figs[k][0] if figs[k][2] == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def _restated(name):
    c = next(c for c in all_cases() if c["name"] == name)
    out = []
    for i in range(c["nblocks"]):
        native = block_native(c, i)
        figs = []
        for q in c["ladder"]:
            p, mse, ref, path, info = prdn_cases.prdn_parts(native, candidate(c, native, q), c["bps"], c["nch"], c["ns"])
            figs.append((p, mse, path))
        out.append((figs, choose(figs, c["target"])))
    return out


def restated(c):
    """per block: ([(prdn, mse, path) per ladder entry], (choice, reported prdn)), computed once per process"""
    return _restated(c["name"])
