"""Device runs that the ladder, target, budget and row-length tests of the lossy packers share (tests/test_gpu_target.py,
tests/test_gpu_budget.py, tests/test_gpu_hadamard_rows.py): the composed oracle -- what a user does today, one plain call per
ladder entry -- and a target or a budget call inside a work area of exactly the bytes its sizing call names.  Nothing here knows
what a result is compared with.

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


def budget_call(pk, d_src, ladder, budget, tag):
    """one rspt_hip_compress_budget_batch_dev with the table of candidate sizes -- budget: an int, or one int per block (any
    uint64) -- and the decode of its streams with its choices.  Checked here: nothing is written behind the bytes the sizing call
    names, the handle's quantiser is what it was, the decoder consumed the sizes, no HIP error.
    -> (limits per block, choice, sizes, dst, out, cand) on the host"""
    import torch

    B, K = d_src.shape[0], len(ladder)
    limits = [int(budget)] * B if isinstance(budget, int) else [int(v) for v in budget]
    arg = budget if isinstance(budget, int) else torch.from_numpy(np.array([v - (1 << 64) if v >= BIT63 else v for v in limits], dtype=np.int64)).cuda()
    own = pk.quantizer()
    work = guarded_work(pk.budget_work_bytes(B, K))
    d_dst, d_sizes, d_choice, d_cand = pk.compress_to_budget(d_src, arg, ladder, work=work[:-2], cand_sizes=True)
    d_out, d_used = pk.decompress_batch(d_dst, B, d_dst.shape[1], ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    assert work_guard_untouched(work), (tag, "written behind the bytes the sizing call names")
    assert pk.quantizer() == own, tag
    sizes = d_sizes.cpu().numpy()
    assert np.array_equal(d_used.cpu().numpy(), sizes), tag
    assert last_hip_error(pk) == 0, tag
    return limits, d_choice.cpu().numpy(), sizes, d_dst.cpu().numpy(), d_out.cpu().numpy(), d_cand.cpu().numpy()


def target_call(pk, d_src, target, ladder, tag, planar=False):
    """one rspt_hip_compress_target_batch_dev -- planar: rspt_hip_compress_target_planar_batch_dev, d_src the int32 matrix -- with
    the same checks -> (choice, prdn, sizes, dst) on the host"""
    import torch

    B, K = d_src.shape[0], len(ladder)
    own = pk.quantizer()
    work = guarded_work((pk.target_planar_work_bytes if planar else pk.target_work_bytes)(B, K))
    d_dst, d_sizes, d_choice, d_prdn = (pk.compress_to_prdn_planar if planar else pk.compress_to_prdn)(d_src, target, ladder, work=work[:-2])
    torch.cuda.synchronize()
    assert work_guard_untouched(work), (tag, "written behind the bytes the sizing call names")
    assert pk.quantizer() == own, tag
    assert last_hip_error(pk) == 0, tag
    return d_choice.cpu().numpy(), d_prdn.cpu().numpy(), d_sizes.cpu().numpy(), d_dst.cpu().numpy()
