"""Build the gfx950 shared library in-tree: rspt_amd/librspt_hip.so.

hipcc cross-compiles without a GPU; the built .so is git-ignored but travels to
the GPU box with the gpurun snapshot.  Staleness is decided by a content
fingerprint of the sources (kept beside the library), not by mtimes -- a snapshot
copy need not preserve those.  Concurrent callers (the ranks of a torchrun job)
serialise on a file lock and the library is published with an atomic rename, so
nobody ever maps a half-written file.
"""
import fcntl
import glob
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librspt_hip.so")
STAMP = LIB + ".src-sha"
DIAG_LIB = os.path.join(HERE, "librspt_hip_diag.so")
SOURCES = ["rspt_hip.hip", "signal_packer_hip.cpp"]  # the translation units; everything else in csrc/ is included by them
INCLUDES = [os.path.join(os.path.dirname(HERE), "include", f) for f in ("rspt_hip.h", "signal_packer.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value"]


def _extra_flags():
    return os.environ.get("RSPT_EXTRA_FLAGS", "").split()


def fingerprint(salt="", extra=None):
    """Flags and every source file in csrc/ (whatever is added there is covered), plus the two public headers."""
    h = hashlib.sha256((salt + " ".join(FLAGS + sorted(_extra_flags() if extra is None else extra))).encode())
    deps = sorted(p for ext in ("hip", "hpp", "cpp") for p in glob.glob(os.path.join(CSRC, "*." + ext)))
    for p in deps + [p for p in INCLUDES if os.path.exists(p)]:
        h.update(os.path.basename(p).encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()


def stale(lib=LIB, fp=None):
    if not os.path.exists(lib) or not os.path.exists(lib + ".src-sha"):
        return True
    return open(lib + ".src-sha").read().strip() != (fp or fingerprint())


def _build(lib, flags, fp, force, verbose):
    """Lock, re-check, compile to a temporary, publish library and stamp by atomic rename."""
    if not force and not stale(lib, fp):
        return lib
    with open(lib + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if not force and not stale(lib, fp):  # another process built it while we waited
                return lib
            tmp = "%s.tmp.%d" % (lib, os.getpid())
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + flags + ["-o", tmp] + [os.path.join(CSRC, f) for f in SOURCES]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(tmp, lib)
            with open(lib + ".src-sha.tmp", "w") as f:
                f.write(fp + "\n")
            os.replace(lib + ".src-sha.tmp", lib + ".src-sha")
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return lib


def build(force=False, verbose=False):
    if "-DRSPT_DIAG" in _extra_flags():
        # the diagnostic library (timing probes that skip work) must never become what api.lib() loads
        raise RuntimeError("rspt_amd.build: -DRSPT_DIAG does not belong in RSPT_EXTRA_FLAGS; build the diagnostic library with "
                           "`python -m rspt_amd.build --diag` and load it through RSPT_HIP_LIB")
    return _build(LIB, _extra_flags(), fingerprint(), force, verbose)


def build_diag(verbose=False):
    """The diagnostic build (-DRSPT_DIAG: timing probes that skip work, tuning knobs from the environment) never replaces the
    product library: it goes to librspt_hip_diag.so, which is only ever loaded through RSPT_HIP_LIB."""
    flags = [f for f in _extra_flags() if f != "-DRSPT_DIAG"]
    return _build(DIAG_LIB, ["-DRSPT_DIAG"] + flags, fingerprint("diag ", flags), False, verbose)


if __name__ == "__main__":
    print(build_diag(verbose=True) if "--diag" in sys.argv else build(force="--force" in sys.argv, verbose=True))
