"""GPU parity on the worst-case inputs of margin_cases.py: inputs whose rank errors are coherent and reach 0.39 - 0.98 of
the margin 2E of DESIGN 2b (the proofs are checked in test_margin_cases_cpu.py), where the random suites stay one to two
orders below it.  A margin term that is too small by more than 1 / strength loses the victim of a case here.

Every comparison is exact and against the oracle on the same files: ids, distance bits, lims, probe rows, labels.  Each
list case runs on the forms that share the margin but not the records (f32 MFMA, bf16 x 3, 128-query groups, the
streaming kernel in both group sizes, int8 on / off) and on the generic engine as the control, the adversarial query
alone and at a ragged position among 70 ordinary ones; last_stats() must name the rank mode the case is about, so that
no case passes on an engine without a margin."""
import os
import re

import numpy as np
import pytest

import margin_cases as M
import oracle_lib as O
import vector_indexer_py as vip
from hiprt import Hip

pytestmark = pytest.mark.gpu

KNOBS = ("VI_FILTER", "VI_FILTER_BF16", "VI_FILTER_HI_ONLY", "VI_FILTER_GQ", "VI_RANK_STREAM", "VI_STREAM_GQ", "VI_RANK_I8",
         "VI_RANK_APPROX", "VI_CENTER", "VI_FORCE_GENERIC", "VI_COARSE_DIRECT", "VI_ASSIGN_CAND", "VI_DEBUG_APPROX")
FORMS = {
    "default": {},
    "f32": {"VI_FILTER_BF16": "0"},
    "bf16x3": {"VI_FILTER_HI_ONLY": "0"},
    "gq128": {"VI_FILTER_GQ": "128"},
    "stream128": {"VI_RANK_STREAM": "1", "VI_STREAM_GQ": "128"},
    "stream256": {"VI_RANK_STREAM": "1", "VI_STREAM_GQ": "256"},
    "i8on": {"VI_RANK_I8": "1"},
    "i8off": {"VI_RANK_I8": "0"},
    "generic": {"VI_FORCE_GENERIC": "1"},
}


def forms_of(name):
    return [f for f in FORMS if name[0] == "E" or not f.startswith("i8")]


def want_mode(case, form):
    """vi_search_stats::rank_mode of the case under the form (mfma_search.hip: rank_mode_code).
    The code is 4 (6) for VI_RANK_APPROX=1 and 2 alike and does not name the kernel, so for case B it does not show that
    the queries' lo plane was dropped: the block-synchronous kernel multiplies a non-zero lo plane under VI_RANK_APPROX=2
    too.  B is adversarial on the streaming kernel only — the stream128 / stream256 forms, and every hi-plane form at
    D = 128 — where the mutants of its terms fail it; B-D16 under default, gq128 and bf16x3 are controls."""
    centred = case["env"].get("VI_CENTER") == "1"
    if form == "generic":
        return 0
    if form == "f32":
        return 1 if case["D"] <= 128 else 0      # (the wide kernel ranks with bf16 x 3 only: the exact-order VALU engine)
    if case["D"] > 128 or form == "bf16x3" or case["arith"] == "bf16x3":
        return 5 if centred and case["D"] <= 128 else 2
    return 3 if case["arith"] == "int8" else 6 if centred else 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _knobs_as_the_case_sets_them(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    yield


class Loaded:
    """a case on disk, on both sides, with the oracle's answers to its two batches"""

    def __init__(self, case, root):
        self.case = case
        idx, sh = self.files = M.write_index(case, root)
        self.orc = O.OracleIndex.load(idx, sh)
        with pytest.MonkeyPatch.context() as mp:      # VI_CENTER is read when the index is loaded
            mp.setenv("VI_CENTER", case["env"]["VI_CENTER"])
            self.gpu = vip.load(idx, sh, case["D"])
        self.batches = [np.ascontiguousarray(case["q"][None]), case["Q"]]
        self.topk, self.radius = [], []
        for Q in self.batches:
            k = case["k"] if case["radius2"] is None else int((case["lists"] >= 0).sum())
            rc, Do, Io = self.orc.search_batch(Q, k, case["n_probe"])
            assert rc == O.ORC_OK
            if case["radius2"] is None:
                self.topk.append((Do, Io))
            else:
                hit = (Io >= 0) & (Do <= np.float32(case["radius2"]))
                lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.uint64)
                self.radius.append((lims, Do[hit], Io[hit]))


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    made = {}

    def get(name, case=None):
        if name not in made:
            made[name] = Loaded(case or M.list_case(name), tmp_path_factory.mktemp(name.replace("-", "_")))
        return made[name]
    yield get
    made.clear()


def check_case(L, what):
    case = L.case
    for b, Q in enumerate(L.batches):
        row = 0 if len(Q) == 1 else M.ADV_POS
        if case["radius2"] is None:
            Do, Io = L.topk[b]
            assert Io[row, 0] == case["victim"]
            Dg, Ig = L.gpu.search_sync(Q, case["k"], case["n_probe"])
            bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
            assert bad.size == 0, (f"{case['name']} {what} nq {len(Q)}: {bad.size} queries differ, first {bad[0]} (adversarial: {row}): "
                                   f"gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}")
        else:
            lims_e, De, Ie = L.radius[b]
            assert lims_e[row + 1] - lims_e[row] == 1 and Ie[int(lims_e[row])] == case["victim"]
            lims, D, I = L.gpu.range_search_sync(Q, case["radius2"], case["n_probe"])
            assert np.array_equal(lims, lims_e), f"{case['name']} {what} nq {len(Q)}: lims differ: {lims.tolist()} expected {lims_e.tolist()}"
            assert np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De)), f"{case['name']} {what} nq {len(Q)}: rows differ"
    return L.gpu.last_stats()


@pytest.mark.parametrize("name,form", [(n, f) for n in M.LIST_CASE_NAMES for f in forms_of(n)])
def test_adversarial_case_matches_the_oracle(name, form, loaded, monkeypatch):
    L = loaded(name)
    for key, value in {**{k: v for k, v in L.case["env"].items() if k != "VI_CENTER"}, **FORMS[form]}.items():
        monkeypatch.setenv(key, value)
    st = check_case(L, form)
    print(name, form, "rank_mode", st["rank_mode"], "group_queries", st["group_queries"], "rank_int8", st["rank_int8"])
    assert st["rank_mode"] == want_mode(L.case, form), st
    if st["rank_mode"] == 3:
        assert st["rank_int8"] == (0 if form == "i8off" else 1), st


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.close()


COARSE = {"default": {}, "f32 MFMA coarse": {"VI_FILTER_BF16": "0"}, "non-direct select": {"VI_COARSE_DIRECT": "0"}}


@pytest.mark.parametrize("form", list(COARSE))
@pytest.mark.parametrize("D", [4, 16])
def test_coarse_step_on_the_matrix_cores(D, form, loaded, hip, monkeypatch):
    """the adversarial pair among 1088 centroids, 256 queries (the MFMA coarse step runs from 256 queries and 1024 lists
    on): probe rows against the oracle's (distance, centroid index) order, then the search"""
    g = M.coarse_table(D)
    L = loaded(g["name"], g)
    for key, value in {"VI_RANK_APPROX": "0", **COARSE[form]}.items():
        monkeypatch.setenv(key, value)
    Q = g["Q"]
    nq = len(Q)
    want = np.array([L.orc.probe(q, 8)[1] for q in Q], dtype=np.int64)
    assert (want[g["adv_rows"], 0] == g["victim"]).all() and (want[g["adv_rows"], 1] == g["decoys"][0]).all()
    xq = hip.upload(Q)
    for n_probe in (1, 8):
        probes, order = hip.alloc(nq * n_probe * 4), hip.alloc(nq * n_probe * 4)
        assert L.gpu.probe_device(xq, nq, n_probe, probes, order) == n_probe
        got = hip.download(probes, (nq, n_probe), np.uint32).astype(np.int64)
        bad = np.nonzero((got != want[:, :n_probe]).any(axis=1))[0]
        assert bad.size == 0, (f"{g['name']} {form} n_probe {n_probe}: {bad.size} of {nq} probe rows differ ({np.isin(bad, g['adv_rows']).sum()} "
                               f"adversarial), first {bad[0]}: gpu {got[bad[0]].tolist()} oracle {want[bad[0], :n_probe].tolist()}")
        go = hip.download(order, (nq, n_probe), np.uint32).astype(np.int64)
        assert (np.sort(go, axis=1) == np.arange(n_probe)).all()
    for k, n_probe in [(1, 1), (10, 8)]:
        rc, Do, Io = L.orc.search_batch(Q, k, n_probe)
        assert rc == O.ORC_OK
        Dg, Ig = L.gpu.search_sync(Q, k, n_probe)
        bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
        assert bad.size == 0, f"{g['name']} {form} k {k} n_probe {n_probe}: {bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]]} oracle {Io[bad[0]]}"


ASSIGN_CASES = {"H-D4": lambda: M.assign_case(4), "H-D16": lambda: M.assign_case(16), "H-D4-n3600": lambda: M.assign_case(4, 3600, 2400),
                "H-D16-n3600": lambda: M.assign_case(16, 3600, 2400), "H-sweep-D16": M.assign_sweep_case}


def check_labels(h, labels, what):
    lab_o = O.assign(h["X"], h["centroids"], mode="brute")
    assert (lab_o[h["adv_rows"]] == h["victim"]).all()
    bad = np.nonzero(labels != lab_o)[0]
    assert bad.size == 0, (f"{h['name']} {what}: {bad.size} labels differ ({np.isin(bad, h['adv_rows']).sum()} adversarial), first "
                           f"{bad[0]}: gpu {labels[bad[0]]} oracle {lab_o[bad[0]]}")


@pytest.mark.parametrize("cand", ["1", "0"])
@pytest.mark.parametrize("name", list(ASSIGN_CASES))
def test_assign_tiers_on_nearly_equidistant_points(name, cand, hip, monkeypatch):
    """points whose rank prefers the second-nearest centroid: by 0.44 / 0.39 of the bf16 x 3 tier's margin (H-D4 / H-D16,
    1088 centroids), by 0.98 of the candidate sweep's (H-sweep, 8192 centroids: the sweep is the first tier;
    VI_ASSIGN_CAND=0 hands the same points to bf16 x 3).  The -n3600 variants leave 2400 points undecided, past the 2048 from
    which the f32 MFMA runs on the gathered rows before the exact scan.  Labels are the brute-force oracle's; the stats
    say that the MFMA tiers ran and left every adversarial point to the tiers behind."""
    from margin_assign_child import assign_with_stats
    monkeypatch.setenv("VI_ASSIGN_CAND", cand)
    h = ASSIGN_CASES[name]()
    labels, st = assign_with_stats(hip, h["X"], h["centroids"])
    print(name, "cand", cand, "tier1_rows", int(st.tier1_rows), "exact", int(st.ambiguous_rows))
    check_labels(h, labels, f"VI_ASSIGN_CAND={cand}")
    assert st.used_mfma == 1
    if not (name == "H-sweep-D16" and cand == "1"):       # (the sweep settles its listed candidates exactly itself)
        assert st.tier1_rows >= len(h["adv_rows"]), (int(st.tier1_rows), len(h["adv_rows"]))


def test_assign_f32_first_tier_in_a_fresh_process(tmp_path):
    """VI_ASSIGN_BF16=0: the f32 MFMA as the first tier (margins (d + 2) u').  The knob is read once per process, so the
    same cases run in a child started with it (margin_assign_child.py); the labels are compared here"""
    import subprocess
    import sys
    out = tmp_path / "labels.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "margin_assign_child.py")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["VI_ASSIGN_BF16"] = "0"
    subprocess.run([sys.executable, child, str(out)], check=True, timeout=240, env=env)
    got = np.load(out)
    for name, make in ASSIGN_CASES.items():
        used_mfma, tier1, exact = (int(x) for x in got[name + "/stats"])
        print(name, "VI_ASSIGN_BF16=0 tier1_rows", tier1, "exact", exact)
        check_labels(make(), got[name], "VI_ASSIGN_BF16=0")
        assert used_mfma == 1


@pytest.mark.parametrize("name", ["Ac-D16-K1", "Ac-D16-K10-near", "Cc-D16-K1"])
def test_the_centring_rule_picks_the_offset_unforced(name, loaded, monkeypatch):
    """the centred cases loaded with VI_CENTER unset: the halving rule centres them on its own (rank_mode 6 / 5) and the
    result on the adversarial query is the oracle's, as under VI_CENTER=1"""
    L = loaded(name)
    monkeypatch.setenv("VI_RANK_APPROX", L.case["env"]["VI_RANK_APPROX"])
    auto = vip.load(*L.files, L.case["D"])
    for (Do, Io), Q in zip(L.topk, L.batches):
        Dg, Ig = auto.search_sync(Q, L.case["k"], L.case["n_probe"])
        assert np.array_equal(Ig, Io) and np.array_equal(bits(Dg), bits(Do))
    assert auto.last_stats()["rank_mode"] == want_mode(L.case, "default") in (5, 6)


@pytest.mark.parametrize("name", ["A-D16-K1", "Ac-D16-K1"])
def test_load_time_statistics_are_maxima_over_all_slots(name, loaded, monkeypatch, capfd):
    """VI_DEBUG_APPROX=1 with the approximation on auto prints the vmax and rho the margins use (rank_approx_mode, %.4g):
    max|v| and max|v - hi(v)| over every stored vector, about the centre where centred.  Relative tolerance 1e-3: %.4g
    rounds within 5e-4 and the norms carry (D + 2) u' — the one figure here that is not compared bit for bit."""
    L = loaded(name)
    monkeypatch.setenv("VI_DEBUG_APPROX", "1")
    capfd.readouterr()
    L.gpu.search_sync(L.batches[0], 1, L.case["n_probe"])
    err = capfd.readouterr().err
    lines = re.findall(r"\[vi\] approx: centred (\d) qlen \S+ vmax (\S+) rho (\S+) ", err)
    assert lines, err
    centred, vmax, rho = int(lines[-1][0]), float(lines[-1][1]), float(lines[-1][2])
    want_vmax, want_rho = M.load_stats(L.case["X"], L.case["mu"])
    print(name, "vmax", vmax, want_vmax, "rho", rho, want_rho)
    assert centred == (1 if L.case["mu"] is not None else 0)
    assert abs(vmax - want_vmax) <= 1e-3 * want_vmax and abs(rho - want_rho) <= 1e-3 * want_rho
