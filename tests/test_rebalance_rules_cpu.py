"""CPU: the rules of csrc/rebalance_rules.hpp that vi_indexer_rebalance's kernels and host loop call — the plan over list
lengths (orderings, caps, a list that is donor and receiver), the farthest-member key (one unsigned maximum = largest
distance, lowest position; +0.0 against the smallest distances), the side and skip rules, the distance chain.  A
stand-alone host program (rebalance_rules_check.cpp) that includes only that header is compiled with the host compiler,
once plain and once under the sanitizers, and run directly; it prints one line per failed check."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def compile_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    # (-ffp-contract=off as the library is built: the distance chain is an unfused subtract, multiply, add)
    cmd = [CXX, "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, os.path.join(HERE, "rebalance_rules_check.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True), exe


def _run(tmp_path, name, flags):
    cc, exe = compile_check(tmp_path, name, flags)
    return cc, (subprocess.run([exe], capture_output=True, text=True) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_rules_hold(tmp_path):
    cc, run = _run(tmp_path, "rebalance_rules_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_rules_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "rebalance_rules_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


def test_the_program_includes_only_the_rules_header():
    text = open(os.path.join(HERE, "rebalance_rules_check.cpp")).read()
    project = [l.split()[1] for l in text.splitlines() if l.startswith("#include") and '"' in l]
    assert project == ['"rebalance_rules.hpp"'], project
    rules = open(os.path.join(CSRC, "rebalance_rules.hpp")).read()
    names = ("rebalance_plan", "rebalance_far_key", "rebalance_key_pos", "rebalance_skip", "rebalance_side", "rebalance_side_empty",
             "rebalance_dist_add")
    for name in names:
        assert name in rules, name
    includes = [l.split()[1] for l in rules.splitlines() if l.startswith("#include")]
    assert all(i.startswith("<") for i in includes) and not any("hip" in i for i in includes), includes   # HIP-free
    kernels = open(os.path.join(CSRC, "list_split.hip")).read()
    assert '#include "rebalance_rules.hpp"' in kernels
    for name in ("rebalance_far_key", "rebalance_key_pos", "rebalance_skip", "rebalance_side", "rebalance_side_empty",
                 "rebalance_dist_add", "refine_chain_add", "refine_mean", "refine_slot_of_ordinal"):
        assert name in kernels, name
    assert "rebalance_plan" in open(os.path.join(CSRC, "list_refine.hip")).read()
    # the two chains of the means kernel take no atomics: a side's sum is one sequential chain
    body = kernels.split("split_means_kernel(SplitArgs a) {")[1].split("\n}\n")[0]
    assert "atomic" not in body
    assert "list_split.o" in open(os.path.join(CSRC, "Makefile")).read()
