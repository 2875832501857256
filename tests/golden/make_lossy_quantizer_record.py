#!/usr/bin/env python3
"""Generate tests/golden/lossy_quantizer_record.json: what the reference's dct and hadamard packers write and decode when they
are rebuilt with other `quality` / nr_bytes_to_compress_ constants (signal_packer_dct.cpp:39,46, signal_packer_hadamard.cpp:37,44),
for the settings and inputs of tests/lossy_quantizer_cases.py.

The script copies the two packer sources into a temporary build directory outside the repository and substitutes each of the
four constants THERE by an expression that reads the value when a packer is constructed, asserting that every substitution
changes exactly one line; it compiles the reference library from the unpatched sources, the two patched copies and
tests/golden/lossy_quantizer_shim.cpp (gcc -O2 -std=c11 -DNDEBUG, g++ -O2 -std=gnu++11), runs the cases with the stack limit
lifted (fwht.c keeps two n-point arrays on the stack) and deletes the build.  Nothing of the patched text is kept: the record
holds results.  Per block of a case:
  in_crc32, size, crc32, dec_crc32, prdn   of the input, the stream, the decoded block; PRDN[%] by the oracle's restatement
  stream, decoded                          in full (base64) for the small cases and the cases the FFT kernels are held to
and per FFT case fft_share / fft_maxdiff: the share of coefficients by which a numpy fp64 FFT DCT (lossy_quantizer_cases.py:
fft_dct_coeffs) differs from the reference's stream and the largest difference -- the check, made here on the CPU, that the
chosen inputs stay inside the gates of tests/test_gpu_dct_fft.py.
"defaults" holds the cases of tests/golden/golden.json that the patched build must reproduce at the reference's own constants.

    python tests/golden/make_lossy_quantizer_record.py [--ref DIR]
"""
import ctypes as C
import glob
import os
import resource
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import refrecord

refrecord.repo_paths()

import cases  # noqa: E402
import lossy_quantizer_cases as lq  # noqa: E402

ENV = {("dct", "q"): "RSPT_LQ_DCT_QUALITY", ("dct", "nb"): "RSPT_LQ_DCT_NB", ("hadamard", "q"): "RSPT_LQ_HADAMARD_QUALITY",
       ("hadamard", "nb"): "RSPT_LQ_HADAMARD_NB"}
# file -> [(the constant's initialiser as the reference writes it, what stands there in the temporary copy)]
PATCHES = {
    "signal_packer_dct.cpp": [("quality = 128.0;", 'quality = strtod(getenv("%s"), 0);' % ENV["dct", "q"]),
                              ("nr_bytes_to_compress_ = 2;", 'nr_bytes_to_compress_ = (unsigned)strtol(getenv("%s"), 0, 10);' % ENV["dct", "nb"])],
    "signal_packer_hadamard.cpp": [("quality = 1;", 'quality = strtod(getenv("%s"), 0);' % ENV["hadamard", "q"]),
                                   ("nr_bytes_to_compress_ = 3;", 'nr_bytes_to_compress_ = (unsigned)strtol(getenv("%s"), 0, 10);' % ENV["hadamard", "nb"])],
}


def patched_copy(path, subs, tmp):
    text = open(path).read()
    for old, new in subs:
        before = text.split("\n")
        assert text.count(old) == 1, (path, old, text.count(old))
        text = text.replace(old, new)
        after = text.split("\n")
        assert len(after) == len(before) and sum(a != b for a, b in zip(before, after)) == 1, (path, old)
    out = os.path.join(tmp, os.path.basename(path))
    with open(out, "w") as f:
        f.write(text)
    return out


def build(ref, tmp):
    sp = os.path.join(ref, "lib_rspt", "lib_signalpacker")
    patched = [patched_copy(os.path.join(sp, f), subs, tmp) for f, subs in PATCHES.items()]
    cxx = [p for p in sorted(glob.glob(os.path.join(sp, "*.cpp"))) if os.path.basename(p) not in PATCHES]
    for d in ("lib_zaxtensor", "lib_filter"):
        cxx += sorted(glob.glob(os.path.join(ref, "lib_rspt", d, "*.cpp")))
    objs = []
    for f in sorted(glob.glob(os.path.join(ref, "lib_rspt", "lib_hzr", "*.c"))) + [os.path.join(ref, "lib_rspt", "lib_fwht", "fwht.c")]:
        objs.append(os.path.join(tmp, os.path.basename(f) + ".o"))
        subprocess.check_call(refrecord.CC + ["-c", f, "-o", objs[-1]])
    lib = os.path.join(tmp, "liblossy_quantizer_ref.so")
    subprocess.check_call(refrecord.CXX + ["-shared", "-include", "cstdlib", "-I" + os.path.join(ref, "lib_rspt"), "-I" + sp, "-o", lib] + cxx + patched
                          + [os.path.join(refrecord.HERE, "lossy_quantizer_shim.cpp")] + objs)
    L = C.CDLL(lib)
    L.lossy_quantizer_shim_roundtrip.restype = C.c_int
    L.lossy_quantizer_shim_roundtrip.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                 C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t)]
    return L


def roundtrip(L, kind, q, nb, data, bps, nch, ns):
    """-> (stream, decoded) of the reference built with (q, nb)"""
    os.environ[ENV[kind, "q"]] = repr(float(q))  # (repr round-trips a double; strtod rounds correctly)
    os.environ[ENV[kind, "nb"]] = str(int(nb))
    data = np.ascontiguousarray(data)
    cap = 1 + 3 * nch + 4 * (4 + nch * ns + 7 * ((nch * ns + 65535) // 65536 + 1)) + 64
    stream, dec = np.zeros(cap, dtype=np.uint8), np.zeros(data.size, dtype=np.uint8)
    n, used = C.c_size_t(0), C.c_size_t(0)
    rc = L.lossy_quantizer_shim_roundtrip(lq.KIND_ID[kind], data.ctypes.data, bps, nch, ns, stream.ctypes.data, cap, C.byref(n), dec.ctypes.data, C.byref(used))
    assert rc == 0 and used.value == n.value and 0 < n.value <= cap, (kind, q, nb, rc, used.value, n.value)
    return stream[: n.value].tobytes(), dec.tobytes()


def main():
    from oracle.oracle import Oracle

    orc = Oracle()
    ref = refrecord.ref_root()
    out = {"generator": "tests/golden/make_lossy_quantizer_record.py (the reference's packers with their quality / nr_bytes_to_compress_ "
                        "constants substituted in a temporary copy + tests/golden/lossy_quantizer_shim.cpp, g++ -O2 -std=gnu++11)",
           "prdn": "orc_prdn of the oracle (NaN: null)", "cases": [], "defaults": []}
    tmp = tempfile.mkdtemp(prefix="lossy_quantizer_ref_")
    try:
        L = build(ref, tmp)
        for c in lq.all_cases():
            e = {k: c[k] for k in ("name", "kind", "bps", "nch", "ns", "q", "nb")}
            e["q_hex"] = float(c["q"]).hex()
            e["blocks"] = []
            shares, maxdiff = [], 0
            for i in range(c["nblocks"]):
                data = lq.block_data(c, i)
                s, dec = roundtrip(L, c["kind"], c["q"], c["nb"], data, c["bps"], c["nch"], c["ns"])
                p = orc.prdn(data, dec, c["ns"], c["nch"], c["bps"])
                b = {"in_crc32": lq.crc(data), "size": len(s), "crc32": lq.crc(s), "dec_crc32": lq.crc(dec), "prdn": None if p != p else p}
                if c["full"]:
                    b["stream"] = lq.pack(s)
                    if c["fft"] is None:
                        b["decoded"] = lq.pack(dec)
                if c["fft"]:
                    want, _, _ = lq.stream_values(orc, s, c["kind"], c["nch"], c["ns"], c["nb"])
                    d = np.abs(lq.fft_dct_coeffs(data, c).astype(np.int64) - want.astype(np.int64))
                    shares.append(float((d != 0).mean()))
                    maxdiff = max(maxdiff, int(d.max()))
                e["blocks"].append(b)
            if c["fft"]:
                e["fft_share"], e["fft_maxdiff"] = shares, maxdiff
            out["cases"].append(e)
            print("%-36s q %-8g nb %d sizes %s prdn %s%s" % (c["name"], c["q"], c["nb"], [b["size"] for b in e["blocks"]],
                  ["%.4g" % b["prdn"] if b["prdn"] is not None else "nan" for b in e["blocks"]],
                  "  fft share %s maxdiff %d" % (shares, maxdiff) if c["fft"] else ""), flush=True)
        known = {c["name"]: c for c in cases.packer_cases()}
        for name in lq.default_cases():
            c = known[name]
            q, nb = lq.DEFAULTS[c["kind"]]
            s, dec = roundtrip(L, c["kind"], q, nb, c["data"], c["bps"], c["nch"], c["ns"])
            out["defaults"].append({"name": name, "size": len(s), "crc32": lq.crc(s), "decoded_crc32": lq.crc(dec)})
            print("%-36s default constants: size %d" % (name, len(s)), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    refrecord.write_record("lossy_quantizer_record.json", out, per_line=("cases", "defaults"))


def with_the_stack_limit_lifted(main):
    """main() in a fresh child process whose stack limit is the hard one (fwht.c keeps two n-point arrays on the stack)"""
    if os.environ.get("RSPT_LQ_STACK_LIFTED") != "1":
        hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
        resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=dict(os.environ, RSPT_LQ_STACK_LIFTED="1")))
    main()


if __name__ == "__main__":
    with_the_stack_limit_lifted(main)
