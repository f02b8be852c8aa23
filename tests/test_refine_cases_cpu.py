"""CPU: the cases of refine_cases.py can fail.  Everything here is the oracle's: the replay of one refine iteration moves
records, lowers the inertia, leaves lists of every length class, and its label rule is the reference's scalar chain with
the lowest index among equal distances.  These are conditions on the inputs, not measurements of the library."""
import numpy as np
import pytest

import oracle_lib as O
import refine_cases as R


_MADE = {}


def _make(name, tmp_path_factory):
    if name not in _MADE:
        idx, sh, st, info = R.make(name, str(tmp_path_factory.mktemp("refine_" + name)))
        after, moved = R.replay(st)
        _MADE[name] = dict(name=name, idx=idx, sh=sh, st=st, info=info, after=after, moved=moved)
    return _MADE[name]


@pytest.fixture(scope="module", params=list(R.CASES))
def made(request, tmp_path_factory):
    return _make(request.param, tmp_path_factory)


def test_the_directories_hold_the_state(made):
    st = made["st"]
    back, ids = R.read_state(made["idx"], made["sh"])
    assert (back.lab == st.lab).all() and (back.ext == st.ext).all() and (back.ts == st.ts).all()
    assert (back.X.view(np.uint32) == st.X.view(np.uint32)).all() and (back.C.view(np.uint32) == st.C.view(np.uint32)).all()
    assert len(np.unique(st.ext)) == len(st.ext) and len(st.lab) <= 8000
    assert (st.lens()[made["info"]["emptied"]]) == 0


def test_the_restated_chain_is_the_oracles(made):
    st = made["st"]
    rng = np.random.default_rng(3)
    rows, lists = rng.integers(0, len(st.X), 200), rng.integers(0, st.k, 200)
    D = R.pair_dist(st.X[rows], st.C)
    for i, (r, l) in enumerate(zip(rows, lists)):
        assert D[i, l].view(np.uint32) == O.l2sq_scalar(st.X[r], st.C[l]).view(np.uint32)
    orc = O.OracleIndex.load(made["idx"], made["sh"])
    lab = R.nearest(st.X[rows], st.C)
    for i, r in enumerate(rows):
        rc, p = orc.probe(st.X[r], 1)
        assert rc == O.ORC_OK and int(p[0]) == lab[i]
    # the added records went where the oracle's probe sends them
    added = np.flatnonzero(st.ext >= R.EXT0 + 1_000_000)
    for j in added[:: max(1, len(added) // 100)]:
        rc, p = orc.probe(st.X[j], 1)
        assert int(p[0]) == st.lab[j]


def test_the_drift_piles_into_a_few_lists(made):
    got = np.bincount(made["info"]["added_labels"], minlength=made["st"].k)
    top = np.sort(got)[::-1]
    assert top[:3].sum() >= 0.9 * got.sum() and top[0] < got.sum(), got


def test_an_iteration_moves_records_and_lowers_the_inertia(made):
    st, after = made["st"], made["after"]
    assert made["moved"] > 0 and R.moved_between(st, after) == made["moved"]
    recentred = R.State(st.X, st.lab, st.ext, st.ts, st.origin, after.C, st.c2s)
    assert R.inertia(after) <= R.inertia(recentred) <= R.inertia(st) and R.inertia(after) < R.inertia(st)
    assert R.imbalance(after.lens()) != R.imbalance(st.lens())


def test_list_lengths_of_every_class(made):
    lens = made["after"].lens()
    assert (lens == 0).any() and ((lens >= 1) & (lens <= 63)).any() and (lens > 64).any(), lens
    assert lens[made["info"]["emptied"]] == 0
    e = made["info"]["emptied"]
    assert (made["after"].C[e].view(np.uint32) == made["st"].C[e].view(np.uint32)).all()
    if made["name"].endswith("_long"):
        assert lens.max() > 4096 and made["st"].lens().max() > 4096


def test_the_stable_order(made):
    """records of a list keep the order of their previous positions"""
    after = made["after"]
    for l in range(after.k):
        o = after.origin[after.lab == l]
        assert (np.diff(o) > 0).all()


def test_the_tie(tmp_path_factory):
    made = _make("d3_tie", tmp_path_factory)
    st, after, info = made["st"], made["after"], made["info"]
    L, H = info["L"], info["H"]
    assert L < H
    assert (after.C[L] == info["want_L"]).all() and (after.C[H] == info["want_H"]).all()
    D = R.pair_dist(info["tie"], after.C)
    assert (D[:, L].view(np.uint32) == D[:, H].view(np.uint32)).all() and (D.min(axis=1) == D[:, L]).all()
    rows = [int(np.flatnonzero((after.X == t).all(axis=1))[0]) for t in info["tie"]]
    assert (after.lab[rows] == L).all()                              # the lowest index wins
    assert (np.argsort(D, axis=1, kind="stable")[:, 0] == L).all() and (D.shape[1] - 1 - np.argmin(D[:, ::-1], axis=1) == H).all()
    assert (after.X == np.rint(after.X)).all() and after.X.min() >= 0 and after.X.max() <= 255


def test_more_iterations_reach_a_fixed_point(made):
    st, n = made["after"], 1
    while n < 400:
        nxt, moved = R.replay(st)
        n += 1
        if moved == 0 and (nxt.C.view(np.uint32) == st.C.view(np.uint32)).all():
            break
        st = nxt
    print(made["name"], "fixed point found by iteration", n)
    assert n < 400, "no fixed point in 400 iterations"


def test_a_list_emptied_first_stays_empty_or_is_refilled(made):
    out = R.emptied_outcomes(made["st"])
    assert any(n == 0 for n, _, _ in out.values())
    assert any(n > 0 for n, _, _ in out.values()) == (made["name"] in R.REFILLED_CASES)
    for l, (n, cut, after) in out.items():
        if n == 0:
            assert (after.C[l].view(np.uint32) == made["st"].C[l].view(np.uint32)).all()
