"""Device runs that the ladder, target, budget and row-length tests of the lossy packers share (tests/test_gpu_target.py,
tests/test_gpu_budget.py, tests/test_gpu_total.py, their planar siblings, tests/test_gpu_hadamard_rows.py): the composed oracle --
what a user does today, one plain call per ladder entry -- and one call of any rate-control entry inside a work area of exactly
the bytes its sizing call names (rate_call).  Nothing here knows what a result is compared with.

torch is imported inside the functions, as in tests/devframe.py."""
import numpy as np

BIT63 = 1 << 63


def composed(pk, d_src, ladder, prdn=False):
    """per ladder entry rspt_hip_set_quantizer + compress_batch + decompress_batch (prdn: + prdn_batch with its parts) on the
    native batch d_src -> [dict(dst, sizes, out[, prdn, mse, path])] on the host; the handle is left as it was"""
    import torch

    own = pk.quantizer()
    res = []
    for q in ladder:
        pk.set_quantizer(q)
        d_dst, d_sizes = pk.compress_batch(d_src)
        d_out, _ = pk.decompress_batch(d_dst, d_src.shape[0], d_dst.shape[1])
        figs = pk.prdn_batch(d_src.reshape(-1), d_out.reshape(-1), parts=True) if prdn else None
        torch.cuda.synchronize()
        o = dict(dst=d_dst.cpu().numpy(), sizes=d_sizes.cpu().numpy(), out=d_out.cpu().numpy())
        if prdn:
            o.update(prdn=figs[0].cpu().numpy(), mse=figs[1].cpu().numpy(), path=figs[3].cpu().numpy())
        res.append(o)
    pk.set_quantizer(own[0])
    return res


def guarded_work(nbytes):
    """a float64 work area of nbytes (rounded up to 8) with two doubles behind it, every one a NaN: call with work[:-2]"""
    import torch

    return torch.full(((nbytes + 7) // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")


def work_guard_untouched(work):
    return all(x != x for x in work[-2:].cpu().numpy())


def last_hip_error(pk):
    from rspt_amd import api as a

    return a.lib().rspt_hip_last_hip_error(pk._h)


RATE = {"target": "compress_to_prdn", "budget": "compress_to_budget", "total": "compress_to_total"}  # rule -> the binding's method
RATE_TABLES = {"target": {}, "budget": dict(cand_sizes=True), "total": dict(tables=True)}
BUDGET_FIELDS = ("limits", "choice", "sizes", "dst", "out", "cand")  # of rate_call's dict, for callers that unpack
TARGET_FIELDS = ("choice", "prdn", "sizes", "dst")


def budget_arg(budget):
    """the binding's argument: an int stays one, one int per block (any uint64) becomes the int64 tensor that is read as unsigned"""
    import torch

    if isinstance(budget, int):
        return budget
    return torch.from_numpy(np.array([int(v) - (1 << 64) if int(v) >= BIT63 else int(v) for v in budget], dtype=np.int64)).cuda()


def rate_call(pk, rule, src, arg, ladder, tag, planar=False, **kw):
    """One call of a rate-control entry -- rule "target" (arg: the PRDN target), "budget" (arg: an int, or one int per block, any
    uint64) or "total" (arg: the total) -- with every table it can return, on native blocks or, planar, on the int32 matrix, inside
    a work area of exactly the bytes its sizing call names; then, where no stream is flagged, the decode of its streams with its
    choices.  Checked here: nothing is written behind the named bytes, the budget entry's are the table alone from either source,
    the handle's quantiser is what it was, the decoder consumed the sizes, no HIP error.
    -> dict on the host: choice, sizes, dst, out (the decoded native batch, None where a stream is flagged) and, by rule,
    prdn | limits, cand | level (its bit pattern), total, prdn, cand, figs; "dev": the device tensors as the binding returns them"""
    import torch

    B, K = src.shape[0], len(ladder)
    form = "_planar" if planar else ""
    own = pk.quantizer()
    nwork = getattr(pk, "%s%s_work_bytes" % (rule, form))(B, K)
    if rule == "budget":
        assert nwork == pk.budget_work_bytes(B, K) and K * B * 8 <= nwork < K * B * 8 + 256, tag
    work = guarded_work(nwork)
    res = getattr(pk, RATE[rule] + form)(src, budget_arg(arg) if rule == "budget" else arg, ladder, work=work[:-2], **RATE_TABLES[rule], **kw)
    d_dst, d_sizes, d_choice = res[:3]
    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy()
    d_out = None
    if not (sizes.view(np.uint64) >> np.uint64(63)).any():
        d_out, d_used = pk.decompress_batch(d_dst, B, d_dst.shape[1], ladder=ladder, choice=d_choice)
        torch.cuda.synchronize()
        assert np.array_equal(d_used.cpu().numpy(), sizes), tag
    assert work_guard_untouched(work), (tag, "written behind the bytes the sizing call names")
    assert pk.quantizer() == own, tag
    assert last_hip_error(pk) == 0, tag
    r = dict(dev=res, choice=d_choice.cpu().numpy(), sizes=sizes, dst=d_dst.cpu().numpy(), out=None if d_out is None else d_out.cpu().numpy())
    if rule == "target":
        r.update(prdn=res[3].cpu().numpy())
    elif rule == "budget":
        r.update(limits=[int(arg)] * B if isinstance(arg, int) else [int(v) for v in arg], cand=res[3].cpu().numpy())
    else:
        r.update(level=int(res[3].cpu().numpy().view(np.uint64)[0]), total=int(res[4].cpu().numpy().view(np.uint64)[0]), prdn=res[5].cpu().numpy(),
                 cand=res[6].cpu().numpy(), figs=res[7].cpu().numpy())
    return r
