"""The work-area layouts of the rate-control entries (rspt_amd/csrc/rate_work.hpp: target, budget, total, either form and route),
swept on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cxx/rate_work_layout.cpp, a program of its own that
includes the header alone.  What it checks is stated there; the same sizes are held to the device's sizing calls by
tests/test_gpu_rate_work_bytes.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_holds_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rate_work_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "rate_work_layout.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.endswith("layouts hold\n") and int(out.stdout.split()[0]) > 100000, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
