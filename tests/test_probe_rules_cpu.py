"""CPU: the rule of csrc/probe_rules.hpp by which adaptive probing shortens a probe row — the three counts, the clamp, the
closed-up candidate-order ranks — against a brute-force restatement on random and constructed rows: found 0 / 1 / 63 / 64
/ 65 / 200, d_0 == 0, all distances equal, a threshold exactly equal to a distance, a budget reached exactly at a list
boundary and never reached, min_probe > found, explicit counts 0 and > found, idempotence.  A stand-alone host program
(probe_rules_check.cpp) that includes only that header is compiled with the host compiler, once plain and once under the
sanitizers, and run directly; it prints one line per failed check."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", *flags, "-I", CSRC, os.path.join(HERE, "probe_rules_check.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    return cc, (subprocess.run([exe], capture_output=True, text=True) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_rule_agrees_with_its_brute_force_restatement(tmp_path):
    cc, run = _run(tmp_path, "probe_rules_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_rule_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "probe_rules_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


def test_the_program_includes_only_the_rules_header():
    text = open(os.path.join(HERE, "probe_rules_check.cpp")).read()
    project = [l.split()[1] for l in text.splitlines() if l.startswith("#include") and '"' in l]
    assert project == ['"probe_rules.hpp"'], project
    rules = open(os.path.join(CSRC, "probe_rules.hpp")).read()
    assert "probe_keep_count" in rules and "probe_threshold" in rules and "probe_closed_rank" in rules
    includes = [l.split()[1] for l in rules.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"], includes      # HIP-free: the host program runs the very functions the kernel calls
    kernel = open(os.path.join(CSRC, "probe_prune.hip")).read()
    assert '#include "probe_rules.hpp"' in kernel
    for fn in ("probe_threshold(", "probe_within_ratio(", "probe_budget_met(", "probe_keep_count(", "probe_closed_rank("):
        assert fn in kernel, fn
