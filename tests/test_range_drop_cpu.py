"""CPU: the ragged rules of csrc/self_drop.hpp by which a radius search by stored record takes the CSR result of a chunk's
search to the caller's CSR result — output length of a row and source index of an entry — against a brute-force "erase
per row, then concatenate".  A stand-alone host program (range_drop_check.cpp) that includes only that header is compiled
with the host compiler, once plain and once under the sanitizers, and run directly; it prints one line per failed check."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", *flags, "-I", CSRC, os.path.join(HERE, "range_drop_check.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    return cc, (subprocess.run([exe], capture_output=True, text=True) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_ragged_drop_matches_erase_then_concatenate(tmp_path):
    cc, run = _run(tmp_path, "range_drop_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_ragged_drop_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "range_drop_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


def test_the_program_includes_only_the_rules_header():
    text = open(os.path.join(HERE, "range_drop_check.cpp")).read()
    project = [l.split()[1] for l in text.splitlines() if l.startswith("#include") and '"' in l]
    assert project == ['"self_drop.hpp"'], project
    rules = open(os.path.join(CSRC, "self_drop.hpp")).read()
    assert "range_drop_len" in rules and "range_drop_src" in rules
