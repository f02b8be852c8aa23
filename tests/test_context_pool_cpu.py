"""CPU: csrc/context_pool.hpp, the pool that hands the search and the fetch contexts of a handle to concurrent calls — no
more than 4 contexts are made or held at once, none by two threads, a make that fails leaves the pool usable, a release
runs its callable exactly once.  A stand-alone host program (context_pool_check.cpp) that includes only that header is
compiled with the host compiler, once plain, once under the address and undefined-behaviour sanitizers and once under
the thread sanitizer, and run directly; it prints one line per failed check."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", "-pthread", *flags, "-I", CSRC, os.path.join(HERE, "context_pool_check.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    return cc, (subprocess.run([exe], capture_output=True, text=True, timeout=300) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pool_bounds_and_leases(tmp_path):
    cc, run = _run(tmp_path, "context_pool_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pool_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "context_pool_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


def _tsan_works(tmp_path):
    """an empty program built with the thread sanitizer links and runs: asked before the check itself is built"""
    src, exe = tmp_path / "tsan_probe.cpp", str(tmp_path / "tsan_probe")
    src.write_text("int main() { return 0; }\n")
    cc = subprocess.run([CXX, "-pthread", "-fsanitize=thread", str(src), "-o", exe], capture_output=True, text=True)
    return cc.returncode == 0 and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pool_under_thread_sanitizer(tmp_path):
    """... and with ThreadSanitizer: what a release publishes and what a holder writes into its context are plain memory"""
    if not _tsan_works(tmp_path):
        pytest.skip("the host compiler does not link a thread sanitizer runtime that starts here")
    cc, run = _run(tmp_path, "context_pool_check_tsan", ["-g", "-O1", "-fsanitize=thread"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr
