"""The frame every test_*.py module stands in: the repository's root and the status codes, the `api` and `asm` fixtures, the
golden loader, device buffers between guards, the C ABI checks, the ISA checks and the run of a planar sliding-window stage.
Nothing here knows a stage.  A module takes the fixtures by name: `from devframe import api, asm  # noqa: F401`.

torch is imported inside the functions that need a device, so that the CPU suite does not."""
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import devasm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rspt_hip_status (include/rspt_hip.h; held against its text by tests/test_cabi.py)
OK, ERR_NO_DEVICE, ERR_ALLOC, ERR_LAUNCH, ERR_DST_TOO_SMALL, ERR_CORRUPT, ERR_BUSY = 0, -2, -3, -4, -5, -6, -8
ERR_ARG, ERR_UNSUPPORTED = -1, -7  # (what a refusal returns)
STATUS_NAMES = "OK ERR_ARG ERR_NO_DEVICE ERR_ALLOC ERR_LAUNCH ERR_DST_TOO_SMALL ERR_CORRUPT ERR_UNSUPPORTED ERR_BUSY".split()


# ---- fixtures ----

@pytest.fixture(scope="module")
def api():
    from rspt_amd import api as a

    assert a.lib().rspt_hip_device_count() > 0, "no gfx950 device visible: the HIP path cannot run (no CPU fallback)"
    return a


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(devasm.HIPCC):
        pytest.skip("hipcc not found")
    return devasm.functions()


def golden(name):
    """tests/golden/<name>, parsed"""
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


# ---- device buffers between guards ----

# bytes in front of and behind every buffer, and what they hold.  One size for all, so that what builds a buffer and what checks
# its guards cannot disagree
GUARD, FILL = 256, 0xA5


def guarded(nbytes, off=0, fill=FILL):
    """(raw, view): nbytes of uint8 on the device, `off` (< 16) bytes past a 16-byte boundary, between two guards of FILL.
    fill: what the view holds at first, one byte value for all of it or an array whose bytes are copied in."""
    import torch

    assert 0 <= off < 16
    raw = torch.full((GUARD + off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    view = raw[GUARD + off : GUARD + off + nbytes]
    assert raw.data_ptr() % 16 == 0 and (nbytes == 0 or view.data_ptr() % 16 == off)  # (an empty view has no address)
    if isinstance(fill, int):
        if fill != FILL:
            view.fill_(fill)
    else:
        view.copy_(torch.from_numpy(np.array(fill).view(np.uint8).reshape(-1)))
    return raw, view


def guarded_matrix(P, off=0, fill=None):
    """(raw, view): P on the device as int32 [nblocks][nch][ns], `off` bytes past a 16-byte boundary, between two guards.
    fill: as for guarded(), in place of P's values (a destination of P's shape)"""
    import torch

    raw, view = guarded(P.size * 4, off, np.asarray(P, dtype=np.int32) if fill is None else fill)
    return raw, view.view(torch.int32).reshape(P.shape)


def guards_untouched(raw, off, n):
    return int((raw[: GUARD + off] != FILL).count_nonzero()) == 0 and int((raw[GUARD + off + n :] != FILL).count_nonzero()) == 0


def what(c, hide=()):
    """the whole case but its name and the keys of `hide` (its samples), as text: a failure message shows a string in full"""
    return "%s: %r" % (c["name"], {k: v for k, v in c.items() if k != "name" and k not in hide})


# ---- the C ABI ----

@functools.lru_cache(maxsize=None)
def header(flat=True):
    """include/rspt_hip.h; flat: every run of white space one blank, so that a declaration is one line of text"""
    text = open(os.path.join(ROOT, "include", "rspt_hip.h")).read()
    return re.sub(r"\s+", " ", text) if flat else text


@functools.lru_cache(maxsize=None)
def exported():
    """`nm -D --defined-only` of the built library, once per process"""
    from rspt_amd import build

    return subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()


def check_entries(declarations, entries, native_of=None, methods=()):
    """Header, library and binding table agree on `entries`: every declaration (a text, or a compiled pattern) is in the flat
    header; every entry is exported as T, in api.C_ABI_SYMBOLS and an attribute of the loaded library; its C_ABI row equals that
    of native_of[entry] where one is named; every name of `methods` is a callable of SignalPacker."""
    from rspt_amd import api

    flat, out, L = header(), exported(), api.lib()
    for d in declarations:
        assert d.search(flat) if isinstance(d, re.Pattern) else d in flat, d
    for name in entries:
        assert re.search(r"\bT %s$" % name, out, re.M), name
        assert name in api.C_ABI_SYMBOLS and hasattr(L, name), name
        if native_of:
            assert api.C_ABI[name] == api.C_ABI[native_of[name]], name
    for m in methods:
        assert callable(getattr(api.SignalPacker, m)), m


# ---- the ISA ----

# a fused multiply-add (or an f64 MFMA) of either float width, packed ones included; and of f64 alone
FUSED_F64_F32 = re.compile(r"^\s+(v_fma\w*_f(64|32)|v_fmac\w*_f(64|32)|v_mad\w*_f(64|32)|v_mac\w*_f(64|32)|v_pk_fma\w*|v_mfma\w*f64)\b")
FUSED_F64 = re.compile(r"^\s+(v_fma\w*_f64|v_fmac\w*_f64|v_mad\w*_f64|v_mfma\w*f64)\b")


def rounds_separately(asm, name_regex, count, fused=FUSED_F64_F32):
    """`count` functions match name_regex; none holds a fused operation, each holds v_mul_f64 and v_add_f64 -> their names"""
    names = [n for n in asm if re.search(name_regex, n)]
    assert len(names) == count, (name_regex, sorted(names))
    for n in names:
        assert not [ln for ln in asm[n] if fused.match(ln)], n
        text = "".join(asm[n])
        assert re.search(r"^\s+v_mul_f64\b", text, re.M) and re.search(r"^\s+v_add_f64\b", text, re.M), n
    return names


def uses_no_scratch(asm, names):
    """every kernel of `names`: a private segment of 0 bytes in its descriptor and no scratch_ instruction in its body"""
    text = open(devasm.asm_path()).read()
    for n in names:
        m = re.search(r"^\s*\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(n), text, re.M | re.S)
        assert m, n
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", m.group(1)), n
        assert not re.search(r"^\s+scratch_", "".join(asm[n]), re.M), n


# ---- a planar sliding-window stage (FIR, median) ----

def planar_window(api, c, entry, state_bytes, want_state_bytes, want, image, calls="own", states=None, hide=("planar",)):
    """c through a planar window entry, every buffer between guards -> (output, state bytes or None).
    entry(pk, src, d_out=, state=) is the stage's call and state_bytes(pk) its sizing call; calls: None stateless, else blocks per
    call on a fresh state 8 bytes past a boundary ("own": the case's).  Checked: the destination returned, the state's size, the
    guards, that an out-of-place source is only read, that the handle recorded no HIP error, and the output and the state's
    bytes against want and image.  states: a list that receives (blocks so far, state bytes, output so far) after every call."""
    import torch

    P = c["planar"]
    calls = c["calls"] if calls == "own" else calls
    tag = what(c, hide)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    sraw, src = guarded_matrix(P, c["src_off"])
    draw, dst = (sraw, src) if c["dst_off"] is None else guarded_matrix(P, c["dst_off"], fill=0)
    state = None
    if calls is None:
        assert entry(pk, src, d_out=None if dst is src else dst, state=None) is dst
    else:
        nst = state_bytes(pk)
        assert nst == want_state_bytes
        straw, state = guarded(nst, 8, fill=0)
        b0 = 0
        for k in calls:
            entry(pk, src[b0 : b0 + k], d_out=None if dst is src else dst[b0 : b0 + k], state=state)
            b0 += k
            if states is not None:
                torch.cuda.synchronize()
                states.append((b0, state.cpu().numpy(), dst[:b0].cpu().numpy()))
        assert b0 == P.shape[0]
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert guards_untouched(sraw, c["src_off"], P.size * 4), ("source guards", tag)
    if dst is not src:
        assert guards_untouched(draw, c["dst_off"], P.size * 4), ("destination guards", tag)
        assert np.array_equal(src.cpu().numpy(), P), ("d_src is only read", tag)
    sbytes = None
    if state is not None:
        assert guards_untouched(straw, 8, nst), ("state guards", tag)
        sbytes = state.cpu().numpy()
    assert api.lib().rspt_hip_last_hip_error(pk._h) == 0, ("a HIP error on the handle", tag)
    pk.close()
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("output: %d differ, first at [block, channel, sample] %s" % (len(bad), bad[:1].tolist()), tag)
    if sbytes is not None:
        assert np.array_equal(sbytes, image), ("state", tag)
    return got, sbytes
