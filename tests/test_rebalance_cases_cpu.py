"""CPU: every case of rebalance_cases.py can fail — its plan is not empty and is the one the case is made for, every
split that is done has two sides with records, records move, the balance ends below what the same number of plain refine
iterations reach, the tie and skip paths are really taken where a state is built for them — and the numpy plan agrees
with the C++ plan the library runs (rebalance_rules_check.cpp prints it for given lengths)."""
import subprocess

import numpy as np
import pytest

import rebalance_cases as B
from test_rebalance_rules_cpu import CXX, compile_check

_states = {}


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("rebalance_cases")


def state_of(name, root):
    if name not in _states:
        _states[name] = B.make_state(name, str(root / name))
    return _states[name]


@pytest.fixture(scope="module", params=list(B.CASES))
def outcome(request, root):
    case = B.CASES[request.param]
    idx, sh, st, info = state_of(case.state, root)
    return request.param, case, st, info, B.replay_rule(st, case.rule)


def test_the_plan_is_the_one_the_case_is_for(outcome):
    name, case, st, info, out = outcome
    assert out.rounds and all(len(r) > 0 for r in out.rounds), "an empty plan"
    assert len(out.rounds) == case.rule.split_rounds == out.iterations_run
    got = [[(p["donor"], p["receiver"]) for p in r] for r in out.rounds]
    assert got[0] == B.plan(st.lens(), case.rule)
    if name in B.NAMED_PAIRS:
        assert got == B.NAMED_PAIRS[name]
    if name in B.NAMED_PAIR_COUNTS:
        assert [len(r) for r in got] == B.NAMED_PAIR_COUNTS[name]
    lens = st.lens()
    for d, r in got[0]:
        assert lens[d] >= 2 and lens[d] > case.rule.split_factor * lens.sum() / len(lens) and lens[r] <= case.rule.receiver_max_len
    if name == "d128_real_long":
        assert lens[got[0][0][0]] == 4583            # more than 64 blocks, 72 LDS tiles
    if name == "d96_real_one_record":
        assert sorted(lens[r] for _, r in got[0]) == [0, 1]          # one receiver holds a record
    if name == "d128_real_long_three_rounds":
        first = {l for l in got[0][0]}
        assert any(d in first for r in got[1:] for d, _ in r), "a later round splits a list the first round made"


def test_every_done_split_has_two_sides(outcome):
    name, case, st, info, out = outcome
    for r in out.rounds:
        for p in r:
            if p["skipped"]:
                assert p["counts"] == []
                continue
            assert 1 <= len(p["counts"]) <= case.rule.split_iters
            assert all(a > 0 and b > 0 for a, b in p["counts"]), p["counts"]
            assert (B.bits(p["ca"]) != B.bits(p["cb"])).any()
    assert out.count("splits_done") >= 1
    assert out.count("pairs_planned") == out.count("splits_done") + out.count("splits_skipped")


def test_records_move_and_the_balance_beats_plain_iterations(outcome):
    name, case, st, info, out = outcome
    assert B.R.moved_between(st, out.state) > 0
    plain = B.replay_plain(st, case.rule.iters)
    assert B.imbalance(out.state.lens()) < B.imbalance(plain.lens()) and B.imbalance(out.state.lens()) < B.imbalance(st.lens())
    assert B.inertia(out.state) < B.inertia(plain)
    empty = int((out.state.lens() == 0).sum())
    assert empty == (1 if name == "copies" else 0)     # (the receiver of the skipped pair stays empty)
    # the receivers of the done splits hold records afterwards
    for p in out.rounds[-1]:
        if not p["skipped"]:
            assert out.state.lens()[p["receiver"]] > 0 and out.state.lens()[p["donor"]] > 0


def test_the_imbalance_factors_are_the_ones_reported(outcome):
    """the figures the change was proposed with, to two decimals"""
    name, case, st, info, out = outcome
    want = {"d3_tie": 4.75, "d96_real": 1.85, "d128_real_long": 4.68, "d128_u8": 1.91, "d160_real": 1.89,
            "d128_real_long_three_rounds": 1.49}
    if name in want:
        assert round(B.imbalance(out.state.lens()), 2) == want[name]


def test_the_tie_and_skip_paths_are_taken(root):
    for name in ("twins", "copies", "equidistant"):
        case = B.CASES[name]
        idx, sh, st, info = state_of(case.state, root)
        out = B.replay_rule(st, case.rule)
        pairs = out.rounds[0]
        if name == "twins":
            p = pairs[0]
            assert p["donor"] == info["donor"] and p["ties_a"] >= 2 and not p["skipped"]
            Xm = st.X[st.lab == p["donor"]]
            same = np.flatnonzero((Xm == Xm[p["a"]]).all(axis=1))
            assert p["a"] == same.min() and len(same) >= 3        # the lowest of the positions that hold the record
        elif name == "copies":
            skipped = [p for p in pairs if p["skipped"]]
            assert [p["donor"] for p in skipped] == [info["copies_list"]] and pairs[0]["skipped"]
            assert skipped[0]["ties_a"] == skipped[0]["ties_b"] == 401 and skipped[0]["a"] == skipped[0]["b"] == 0
            assert any(not p["skipped"] for p in pairs), "another pair of the round is split"
            assert out.count("splits_skipped") == 1 and out.count("splits_done") >= 1
            # both centroids of the skipped pair stay as step 1 left them
            C1, counts = B.O.update_centroids(st.X, st.lab.astype(np.uint64), st.k)
            d, r = skipped[0]["donor"], skipped[0]["receiver"]
            assert (B.bits(out.state.C[d]) == B.bits(C1[d])).all() and (B.bits(out.state.C[r]) == B.bits(st.C[r])).all()
        else:
            p = [q for q in pairs if q["donor"] == info["equidistant_list"]][0]
            assert p["side_ties"][0] >= 2 and not p["skipped"]
            assert len(p["counts"]) < case.rule.split_iters      # ... and it stops on unchanged centres, not on the cap


def test_split_rounds_zero_is_the_plain_replay(root):
    idx, sh, st, info = state_of("d96_real", root)
    out = B.replay_rule(st, B.Rule(iters=2, split_rounds=0))
    plain = B.replay_plain(st, 2)
    assert out.rounds == [] and (B.bits(out.state.C) == B.bits(plain.C)).all() and (out.state.ext == plain.ext).all()


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_numpy_plan_is_the_cpp_plan(root, tmp_path):
    cc, exe = compile_check(tmp_path, "rebalance_rules_check", ["-O1"])
    assert cc.returncode == 0, cc.stderr
    rng = np.random.default_rng(9)
    trials = []
    for name, case in B.CASES.items():
        trials.append((state_of(case.state, root)[2].lens().tolist(), case.rule))
    for _ in range(40):
        k = int(rng.integers(1, 40))
        lens = (rng.integers(0, 6, k) * rng.integers(0, 2, k) + (rng.random(k) < 0.2) * rng.integers(0, 400, k)).tolist()
        rule = B.Rule(split_factor=float(rng.choice([1.0, 1.5, 2.0, 3.25])), receiver_max_len=int(rng.choice([0, 1, 3, 1000])),
                      max_splits=int(rng.choice([0, 0, 1, 2])))
        trials.append((lens, rule))
    nonempty = 0
    for lens, rule in trials:
        if sum(lens) == 0:
            continue
        run = subprocess.run([exe, "plan", repr(rule.split_factor), str(rule.receiver_max_len), str(rule.max_splits)] + [str(v) for v in lens],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        got = [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]
        assert got == B.plan(lens, rule), (lens, rule)
        nonempty += bool(got)
    assert nonempty >= 15
