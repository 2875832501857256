"""CPU-side checks of the drop-in boundary: the library builds, loads, and exports
every symbol include/rspt_hip.h declares.  No compute calls without a GPU."""
import ctypes as C
import os
import re

import pytest

from devframe import ERR_ARG, ERR_NO_DEVICE, ROOT


def _declared():
    txt = open(os.path.join(ROOT, "include", "rspt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rspt_hip_[a-z_0-9]+)\s*\(", txt)))


def test_the_tests_status_names_are_the_headers_enum():
    """tests/devframe.py's OK, ERR_ARG, ... against the RSPT_HIP_* enumerators of rspt_hip_status, every one of them"""
    import devframe

    enum = dict(re.findall(r"\bRSPT_HIP_((?:OK|ERR_[A-Z_]+)) = (-?\d+)", open(os.path.join(ROOT, "include", "rspt_hip.h")).read()))
    assert {k: int(v) for k, v in enum.items()} == {k: getattr(devframe, k) for k in devframe.STATUS_NAMES} and len(enum) == 9


def test_library_exports_every_declared_symbol():
    from rspt_amd import api

    L = api.lib()
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), "librspt_hip.so does not export %s" % n
    assert sorted(api.C_ABI_SYMBOLS) == names, "rspt_amd/api.py binding list drifted from include/rspt_hip.h"


_C_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float,
              "long long": C.c_longlong, "void": None}
_C_POINTEES = {"double": C.c_double, "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int, "uint8_t": C.c_uint8,
               "uint32_t": C.c_uint32, "int32_t": C.c_int32}


def _header_signatures():
    """{name: (return type, [parameter types])} of every rspt_hip_* function include/rspt_hip.h declares; a type is
    (base, stars): ("void", 1) for `const void* p`, ("size_t", 0) for `size_t n`"""
    txt = open(os.path.join(ROOT, "include", "rspt_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in txt.split("\n") if not ln.lstrip().startswith("#"))

    def ctype(text, named):
        m = re.fullmatch(r"([A-Za-z_][\w ]*?)\s*(\**)\s*" + (r"\w+" if named else ""), re.sub(r"\bconst\b", " ", text).strip())
        assert m, "cannot read the C type %r" % text
        return " ".join(m.group(1).split()), len(m.group(2))

    sigs = {}
    for stmt in re.split(r"[;{}]", txt):
        stmt = " ".join(stmt.split())
        m = re.fullmatch(r"(.+?)\b(rspt_hip_[a-z_0-9]+) ?\((.*)\)", stmt)
        if not m or stmt.startswith("typedef"):
            continue
        params = [] if m.group(3).strip() == "void" else [ctype(q, True) for q in m.group(3).split(",")]
        assert m.group(2) not in sigs, m.group(2)
        sigs[m.group(2)] = (ctype(m.group(1), False), params)
    return sigs


def _type_matches(ctype, t):
    base, stars = ctype
    if stars == 0:
        return base in _C_SCALARS and t is _C_SCALARS[base]
    if stars == 2:
        return t is C.POINTER(C.c_void_p)
    return t is C.c_void_p or (base == "char" and t is C.c_char_p) or (base in _C_POINTEES and t is C.POINTER(_C_POINTEES[base]))


def _abi_mismatches(table, header):
    """{name: what is wrong} for every entry of table -- name -> (restype, argtypes) -- that differs from its declaration"""
    bad = {}
    for name in sorted(set(table) | set(header)):
        if name not in table or name not in header:
            bad[name] = "only in the %s" % ("header" if name in header else "table")
            continue
        (restype, argtypes), (c_ret, c_params) = table[name], header[name]
        if argtypes is None:
            bad[name] = "no argtypes"
        elif len(argtypes) != len(c_params):
            bad[name] = "%d parameters, the header declares %d" % (len(argtypes), len(c_params))
        elif not _type_matches(c_ret, restype):
            bad[name] = "returns %r, the header declares %r" % (restype, c_ret)
        else:
            wrong = [i for i, (c, t) in enumerate(zip(c_params, argtypes)) if not _type_matches(c, t)]
            if wrong:
                bad[name] = "; ".join("parameter %d is %r, the header declares %r" % (i, argtypes[i], c_params[i]) for i in wrong)
    return bad


def test_binding_table_matches_the_header():
    """Every rspt_hip_* declaration of include/rspt_hip.h against rspt_amd/api.py's table, and against what the loaded library's
    functions carry (a function bound outside the table cannot pass): the same names, parameter counts, scalars exactly, a C
    pointer as c_void_p, c_char_p (char*) or POINTER of its pointee, T** as POINTER(c_void_p).  No device needed."""
    from rspt_amd import api

    header = _header_signatures()
    assert sorted(header) == sorted(api.C_ABI_SYMBOLS) == _declared()
    assert _abi_mismatches(api.C_ABI, header) == {}
    L = api.lib()
    bound = {name: (getattr(L, name).restype, getattr(L, name).argtypes) for name in header}
    assert _abi_mismatches(bound, header) == {}


def test_the_header_check_reports_an_altered_entry_and_only_that_one():
    from rspt_amd import api

    header = _header_signatures()
    restype, argtypes = api.C_ABI["rspt_hip_reserve"]
    assert argtypes[1] is C.c_size_t
    narrowed = dict(api.C_ABI, rspt_hip_reserve=(restype, [argtypes[0], C.c_int]))  # a size_t made c_int
    assert list(_abi_mismatches(narrowed, header)) == ["rspt_hip_reserve"]
    restype, argtypes = api.C_ABI["rspt_hip_compress_batch_dev"]
    dropped = dict(api.C_ABI, rspt_hip_compress_batch_dev=(restype, argtypes[:-1]))  # one parameter dropped
    assert list(_abi_mismatches(dropped, header)) == ["rspt_hip_compress_batch_dev"]


def test_cxx_factories_are_exported():
    """include/signal_packer.h: the i_signal_packer statics must link from the .so."""
    import subprocess

    from rspt_amd import build

    out = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for f in ("new_xdelta_hzr", "delete_xdelta_hzr", "new_hzr", "delete_hzr", "new_dct", "delete_dct", "new_hadamard", "delete_hadamard"):
        assert re.search(r"_ZN15i_signal_packer\d+%sE" % f, out), f


def test_reference_style_program_compiles_against_our_header(tmp_path):
    """A program written like the reference's README example (README.md:49-83)
    compiles and links against include/signal_packer.h + librspt_hip.so."""
    import subprocess

    from rspt_amd import build

    src = tmp_path / "readme_example.cpp"
    src.write_text(
        """
#include <cstdint>
#include <cmath>
#include <iostream>
#include "signal_packer.h"
int main() {
    const int bytes_per_sample = 4, nr_samples = 8192, nr_channels = 1;
    static int32_t data_stream[nr_samples];
    for (int i = 0; i < nr_samples; ++i) data_stream[i] = sin(i / 100.0) * 1000.0;
    i_signal_packer* c = i_signal_packer::new_xdelta_hzr(bytes_per_sample, nr_channels, nr_samples, 3);
    size_t dst_max_len = nr_samples * nr_channels * bytes_per_sample * 2;
    static unsigned char dst[8192 * 4 * 2];
    size_t compressed_size = 0;
    c->compress((uint8_t*)data_stream, dst, dst_max_len, compressed_size);
    std::cout << "compressed_size: " << compressed_size << std::endl;
    i_signal_packer::delete_xdelta_hzr(c);
    return compressed_size == 2028 ? 0 : 1;
}
"""
    )
    exe = tmp_path / "readme_example"
    lib_dir = os.path.dirname(build.LIB)
    cmd = ["g++", "-std=c++11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + lib_dir, "-lrspt_hip",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    assert exe.exists()


def test_create_fails_loudly_without_device():
    from rspt_amd import api

    if api.lib().rspt_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.RsptHipError) as e:
        api.new_xdelta_hzr(4, 1, 8192, 3)
    assert e.value.status == ERR_NO_DEVICE  # no CPU fallback exists


def test_bad_arguments_are_rejected_before_touching_the_device():
    from rspt_amd import api

    import ctypes as C

    L = api.lib()
    h = C.c_void_p()
    for args in [(9, 4, 1, 16, 3), (1, 5, 1, 16, 3), (1, 4, 0, 16, 3), (1, 4, 1, 0, 3), (1, 4, 1, 16, 0), (1, 4, 1, 16, 5), (3, 4, 2, 100, 3)]:
        assert L.rspt_hip_packer_create(C.byref(h), *args, 0) == -1, args


@pytest.mark.gpu
def test_an_empty_batch_is_refused_under_the_name_of_its_entry():
    """The device-batch methods at nblocks == 0, which the library refuses (RSPT_HIP_ERR_ARG, include/rspt_hip.h): prdn_batch,
    to_planar_i32 and from_planar_i32 pass NULL pointers for their empty tensors, iir_zero_phase_batch and
    peak_detect_offline_batch size their workspace for one block; each error carries the name of the entry it came from."""
    import torch

    from rspt_amd import api

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device visible"
    pk = api.new_hzr(2, 3, 64)
    e8 = torch.empty(0, dtype=torch.uint8, device="cuda")
    e32 = torch.empty((0, 3, 64), dtype=torch.int32, device="cuda")
    calls = {
        "rspt_hip_prdn_batch_dev": lambda: pk.prdn_batch(e8, e8, parts=True),
        "rspt_hip_native_to_i32_batch_dev": lambda: pk.to_planar_i32(e8),
        "rspt_hip_i32_to_native_batch_dev": lambda: pk.from_planar_i32(e32),
        "rspt_hip_iir_zero_phase_batch_dev": lambda: pk.iir_zero_phase_batch(e8, [1.0, -0.5], [0.5, 0.5]),
        "rspt_hip_peak_detect_offline_batch_dev": lambda: pk.peak_detect_offline_batch(e8, 500.0),
    }
    for entry, call in calls.items():
        with pytest.raises(api.RsptHipError) as e:
            call()
        assert e.value.status == ERR_ARG and str(e.value).startswith(entry + ": "), (entry, str(e.value))
    pk.close()
