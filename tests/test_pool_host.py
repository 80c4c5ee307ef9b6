"""CPU: the bookkeeping of the context's block pool and of its check mode (csrc/ics_pool.h), instantiated over malloc / memset /
memcpy by the stand-alone program tests/host/pool_selfcheck.cpp, built with the address and undefined-behaviour sanitizers and run as
a binary of its own (nothing is loaded into Python).  What the check mode finds on the device: tests/test_gpu_pool_check.py."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_bookkeeping_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # the sanitizer runtimes linked statically (clang's default): the binary runs the same whatever the environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(os.path.realpath(cxx)) else []
    exe = tmp_path / "pool_selfcheck"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "image-cases-studies_amd", "csrc"), os.path.join(ROOT, "tests", "host", "pool_selfcheck.cpp"),
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "pool_selfcheck OK" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    # the three scribbles the program plants are reported with the rounded size, the requested size and the first offending offset
    lines = [l for l in r.stderr.splitlines() if l.startswith("ics pool check:")]
    assert len(lines) == 3, lines
    assert "block of 73728 bytes (65536 requested)" in lines[0] and "offset 73727" in lines[0]
    assert "block of 65536 bytes (512 requested)" in lines[2] and "offset 512" in lines[2]
