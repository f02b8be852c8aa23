"""CPU: the rules of csrc/cluster_rules.hpp by which a radius clustering unites records — the lock-free union-find by
index, the core test, the border choice — against a naive component labelling of random graphs, a chain of 200, a clique
of 70 and two stars with a bridge, edges in random order: every root must be its component's minimum.  A stand-alone host
program (cluster_rules_check.cpp) that includes only that header is compiled with the host compiler, once plain and once
under the sanitizers, and run directly; it prints one line per failed check.  And the plain-Python statement of the
definition that the GPU tests compare with (cluster_cases.cluster_reference) on hand-made graphs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cluster_cases import NOISE, cluster_reference, cluster_reference_csr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", *flags, "-I", CSRC, os.path.join(HERE, "cluster_rules_check.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    return cc, (subprocess.run([exe], capture_output=True, text=True) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_union_find_roots_are_component_minima(tmp_path):
    cc, run = _run(tmp_path, "cluster_rules_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_union_find_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "cluster_rules_check_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


def test_the_program_includes_only_the_rules_header():
    text = open(os.path.join(HERE, "cluster_rules_check.cpp")).read()
    project = [l.split()[1] for l in text.splitlines() if l.startswith("#include") and '"' in l]
    assert project == ['"cluster_rules.hpp"'], project
    rules = open(os.path.join(CSRC, "cluster_rules.hpp")).read()
    assert "cluster_find" in rules and "cluster_unite" in rules and "cluster_is_core" in rules
    includes = [l.split()[1] for l in rules.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"], includes      # HIP-free: the host program runs the very functions the kernels call
    kernels = open(os.path.join(CSRC, "cluster_radius.hip")).read()
    assert '#include "cluster_rules.hpp"' in kernels and "cluster_link<AgentAccess>" in kernels


# ---- the Python reference on hand-made graphs ----
def test_an_edge_present_in_one_direction_only_still_joins():
    rows = [[1], [], [3], [], []]           # 0 -> 1 and 2 -> 3, neither returned
    labels, degree, nc, counts = cluster_reference(rows, 5, 1)
    assert labels.tolist() == [0, 0, 2, 2, 4] and degree.tolist() == [1, 0, 1, 0, 0] and nc == 3
    assert counts == {"n_core": 5, "n_border": 0, "n_noise": 0, "hits": 2}
    # and for a border: only the core's row holds the pair
    rows = [[1, 2, 3], [0, 2], [0, 1], []]
    labels, degree, nc, _ = cluster_reference(rows, 4, 3)
    assert labels.tolist() == [0, 0, 0, 0] and degree.tolist() == [3, 2, 2, 0] and nc == 1
    # ... or only the border's row does
    rows = [[1, 2], [0, 2], [0, 1], [2]]
    labels, _, nc, counts = cluster_reference(rows, 4, 3)
    assert labels.tolist() == [0, 0, 0, 0] and counts["n_border"] == 1 and nc == 1


def test_a_border_with_cores_of_two_clusters_takes_the_lower_cores_cluster():
    # clusters {1, 2, 3, 4} and {6, 7, 8, 9} (cliques, degree 3); record 0 is adjacent to cores 6 and 4, record 10 to 9 and 2
    rows = [[6, 4], [2, 3, 4], [1, 3, 4], [1, 2, 4], [1, 2, 3], [], [7, 8, 9], [6, 8, 9], [6, 7, 9], [6, 7, 8], [9, 2]]
    labels, degree, nc, counts = cluster_reference(rows, 11, 4)
    assert degree.tolist() == [2, 3, 3, 3, 3, 0, 3, 3, 3, 3, 2]
    assert labels.tolist() == [1, 1, 1, 1, 1, NOISE, 6, 6, 6, 6, 1]     # 0: core 4 < core 6; 10: core 2 < core 9
    assert nc == 2 and counts == {"n_core": 8, "n_border": 2, "n_noise": 1, "hits": 28}
    # the border records do not join the two clusters
    assert labels[1] != labels[6]


def test_min_pts_0_and_1_give_the_same_result():
    rng = np.random.default_rng(3)
    n = 60
    rows = [rng.integers(0, n, size=rng.integers(0, 4)).tolist() for _ in range(n)]
    a, b = cluster_reference(rows, n, 0), cluster_reference(rows, n, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert (a[0] >= 0).all() and a[3]["n_core"] == n      # plain connected components: nobody is noise
    assert (a[0] <= np.arange(n)).all() and (a[0][a[0]] == a[0]).all()


def test_all_records_are_noise_when_min_pts_exceeds_n():
    rows = [[1, 2], [0, 2], [0, 1], [0]]
    labels, degree, nc, counts = cluster_reference(rows, 4, 5)
    assert labels.tolist() == [NOISE] * 4 and nc == 0 and degree.tolist() == [2, 2, 2, 1]
    assert counts == {"n_core": 0, "n_border": 0, "n_noise": 4, "hits": 7}


def test_the_numpy_form_of_the_reference_agrees_with_the_plain_one():
    """cluster_reference_csr (what the GPU tests use where rows hold millions of entries) against cluster_reference"""
    rng = np.random.default_rng(11)
    for trial in range(60):
        n = int(rng.integers(1, 120))
        part = rng.random(n) < 0.8 if trial % 3 == 0 else None
        ok = np.arange(n) if part is None else np.nonzero(part)[0]
        rows = []
        for j in range(n):
            m = int(rng.integers(0, 5)) if ok.size else 0
            rows.append(np.unique(rng.choice(ok, size=m)) if m else np.zeros(0, dtype=np.int64))     # (may hold j itself)
        if trial % 5 == 0:      # a long path in a shuffled numbering, one direction only
            path = rng.permutation(ok)
            for x, y in zip(path[:-1], path[1:]):
                rows[x] = np.union1d(rows[x], [y])
        lims = np.concatenate([[0], np.cumsum([r.size for r in rows])])
        cols = np.concatenate(rows) if n else np.zeros(0, dtype=np.int64)
        for min_pts in (0, 1, 2, 3, 4, 1000):
            want = cluster_reference(rows, n, min_pts, part)
            got = cluster_reference_csr(lims, cols, n, min_pts, part)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], (trial, min_pts)


def test_non_participants_are_ignored_and_get_noise():
    rows = [[1], [0, 2], [1, 3], [2]]       # a path; record 2 does not take part: its row is not read, nobody hits it
    part = np.array([True, True, False, True])
    filtered = [[1], [0], [99], []]
    labels, degree, nc, counts = cluster_reference(filtered, 4, 1, part)
    assert labels.tolist() == [0, 0, NOISE, 3] and degree.tolist() == [1, 1, 0, 0] and nc == 2
    assert counts["n_noise"] == 0 and counts["n_core"] == 3
    with pytest.raises(AssertionError):
        cluster_reference(rows, 4, 1, part)     # a hit that is no participant is an error of the caller's rows
