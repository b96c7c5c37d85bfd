"""The claim / publish logic of the huge geometry's shared test-free tail (pda_amd/csrc/pda_tail_share.h) on the CPU: tests/tail_share_host.cpp,
a stand-alone program in which threads play the workgroups, is built around the header with -fsanitize=thread and with
-fsanitize=address,undefined, and run.  Every half-tile of every published range is claimed exactly once, nothing is claimed from an
unpublished or stale record, and every thread terminates (the program's own checks; the sanitizers find the races and the stray accesses)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tail_share_host.cpp")


def compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no C++ compiler")


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_threads_play_the_workgroups(tmp_path, sanitizer):
    exe = str(tmp_path / "tail_share_host")
    subprocess.run([compiler(), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pda_amd", "csrc"), SRC, "-o", exe], check=True, capture_output=True, text=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "150", "12"], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stderr[-2000:])
