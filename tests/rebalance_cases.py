"""Inputs and the expected outcome of vi_indexer_rebalance, made by the CPU oracle alone.

A plain module (no fixtures, no GPU): tests/test_rebalance_cases_cpu.py proves on the CPU that every case can fail (the
plan is not empty, both sides of a split hold records, records move, ties and skips happen where a case is made for
them), tests/test_rebalance_gpu.py runs the cases through the library.

The states are refine_cases' (20 lists, one emptied by a remove, drifted adds piled into two or three lists) and three
made from d3_tie with the same numpy-and-oracle's-writer steps.  replay_rule(state, rule) is the contract of
include/vi_amd.h as it reads: per iteration the centres from O.update_centroids (an empty list keeps its centroid),
in the first split_rounds iterations the plan and the splits — distances by refine_cases.pair_dist, the reference's scalar
chain; the two centres of an inner iteration by O.update_centroids over the donor's members labelled by side, so each
side's chain runs over its own members in list order — then labels by refine_cases.nearest and the stable regrouping.
"""
import os
from dataclasses import dataclass, field

import numpy as np

import oracle_lib as O
import refine_cases as R
from refine_cases import State, expected_files, imbalance, inertia, make, nearest, pair_dist, replay  # noqa: F401


@dataclass
class Rule:
    """vi_rebalance_rule, with vi_rebalance_rule_init's defaults"""
    iters: int = 1
    split_rounds: int = 1
    split_factor: float = 2.0
    receiver_max_len: int = 0
    max_splits: int = 0
    split_iters: int = 4

    def fields(self):
        return dict(iters=self.iters, split_rounds=self.split_rounds, split_factor=self.split_factor,
                    receiver_max_len=self.receiver_max_len, max_splits=self.max_splits, split_iters=self.split_iters)


@dataclass
class Case:
    state: str            # a state of refine_cases.CASES, or one of STATES below
    rule: Rule
    what: str


STATES = {  # name -> what the state made from d3_tie is for
    "twins": "the record farthest from the donor's centre sits in the list three times: seed a ties, the lowest position wins",
    "copies": "one list holds 401 equal records: its pair is skipped while the other pairs of the round are split",
    "equidistant": "three records of a donor are equidistant from ca and cb in the first inner iteration: they stay on side 0",
}

ONE_REC = Rule(receiver_max_len=1)
CASES = {
    "d3_tie": Case("d3_tie", Rule(), "D = 3: quad padding"),
    "d96_real": Case("d96_real", Rule(), "D = 96"),
    "d128_real_long": Case("d128_real_long", Rule(), "D = 128; a donor of more than 64 blocks and 72 LDS tiles"),
    "d128_u8": Case("d128_u8", Rule(), "D = 128, 8-bit values"),
    "d160_real": Case("d160_real", Rule(), "D = 160: three 64-column groups, the last partial"),
    "d96_real_one_record": Case("d96_real", ONE_REC, "two pairs in one round, one receiver holds a record"),
    "d128_real_long_three_rounds": Case("d128_real_long", Rule(iters=3, split_rounds=3, receiver_max_len=1),
                                        "rounds 2 and 3 split lists that exist only in the cur / seg order: the gather path"),
    "twins": Case("twins", Rule(), STATES["twins"]),
    "copies": Case("copies", ONE_REC, STATES["copies"]),
    "equidistant": Case("equidistant", ONE_REC, STATES["equidistant"]),
}
# what the plans must be, per round: (donor, receiver) list indices, or the number of pairs
NAMED_PAIRS = {"d96_real_one_record": [[(18, 3), (14, 5)]]}
NAMED_PAIR_COUNTS = {"d128_real_long_three_rounds": [1, 2, 2]}


def plan(lens, rule):
    """-> [(donor, receiver)]"""
    lens = [int(v) for v in lens]
    mean = float(sum(lens)) / len(lens)
    donors = [l for l in range(len(lens)) if lens[l] >= 2 and float(lens[l]) > rule.split_factor * mean]
    receivers = [l for l in range(len(lens)) if lens[l] <= rule.receiver_max_len and l not in donors]
    donors.sort(key=lambda l: (-lens[l], l))
    receivers.sort(key=lambda l: (lens[l], l))
    m = min(len(donors), len(receivers))
    if rule.max_splits:
        m = min(m, rule.max_splits)
    return list(zip(donors[:m], receivers[:m]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def split_members(Xm, c, split_iters):
    """the split of one donor (members Xm in list order, centre c) -> dict: skipped, ca, cb, seeds a and b, how many
    members share the largest distance at either seed, the members equidistant from ca and cb per inner iteration, the
    side counts of every inner iteration"""
    da = pair_dist(Xm, c[None])[:, 0]
    a = int(np.argmax(da))                        # (the first of equal maxima)
    db = pair_dist(Xm, Xm[a][None])[:, 0]
    b = int(np.argmax(db))
    out = dict(a=a, b=b, ties_a=int((da == da[a]).sum()), ties_b=int((db == db[b]).sum()), skipped=bool(db[b] == 0),
               side_ties=[], counts=[], ca=None, cb=None)
    if out["skipped"]:
        return out
    ca, cb = Xm[a].copy(), Xm[b].copy()
    for _ in range(split_iters):
        d0, d1 = pair_dist(Xm, ca[None])[:, 0], pair_dist(Xm, cb[None])[:, 0]
        side = d1 < d0                            # a tie goes to side 0
        out["side_ties"].append(int((d1 == d0).sum()))
        out["counts"].append((int((~side).sum()), int(side.sum())))
        if side.all() or not side.any():
            break
        C2, counts = O.update_centroids(Xm, side.astype(np.uint64), 2)
        assert counts[0] == (~side).sum() and counts[1] == side.sum()
        same = (bits(C2[0]) == bits(ca)).all() and (bits(C2[1]) == bits(cb)).all()
        ca, cb = C2[0].copy(), C2[1].copy()
        if same:
            break
    out["ca"], out["cb"] = ca, cb
    return out


def split(st, C1, pairs, split_iters):
    """step 1b on the centres C1 of step 1 -> (the table after it, the split_members record of every pair)"""
    C2 = C1.copy()
    done = []
    for d, r in pairs:
        s = split_members(st.X[st.lab == d], C1[d], split_iters)
        s.update(donor=d, receiver=r)
        if not s["skipped"]:
            C2[d], C2[r] = s["ca"], s["cb"]
        done.append(s)
    return C2, done


def replay_round(st, rule):
    """one iteration with its split step -> (the state after it, records it moved, the pairs' records)"""
    k = st.k
    C1, counts = O.update_centroids(st.X, st.lab.astype(np.uint64), k)
    C1[counts == 0] = st.C[counts == 0]
    pairs = plan(st.lens(), rule)
    C2, done = split(st, C1, pairs, rule.split_iters)
    lab2 = nearest(st.X, C2)
    o = np.argsort(lab2, kind="stable")
    moved = int((lab2 != st.lab).sum())
    return State(np.ascontiguousarray(st.X[o]), lab2[o], st.ext[o], st.ts[o], st.origin[o], C2, st.c2s), moved, done


@dataclass
class Outcome:
    state: State
    iterations_run: int = 0
    rounds: list = field(default_factory=list)    # per split round: the pairs' records

    def count(self, what):
        allp = [p for r in self.rounds for p in r]
        return {"pairs_planned": len(allp), "splits_skipped": sum(p["skipped"] for p in allp),
                "splits_done": sum(not p["skipped"] for p in allp)}[what]


def replay_rule(st, rule):
    """the whole call -> Outcome"""
    out = Outcome(st)
    for it in range(rule.iters):
        if it < rule.split_rounds:
            nxt, moved, done = replay_round(st, rule)
            out.rounds.append(done)
        else:
            nxt, moved = replay(st)
        fixed = moved == 0 and (bits(nxt.C) == bits(st.C)).all()
        st = nxt
        out.iterations_run = it + 1
        if fixed:
            break
    out.state = st
    return out


def replay_plain(st, iters):
    for _ in range(iters):
        st, _ = replay(st)
    return st


# ---- the states made from d3_tie ----
def _write(root, name, st, ids, base_idx, base_sh):
    idx, sh = os.path.join(root, name, "index"), os.path.join(root, name, "shards")
    os.makedirs(idx, exist_ok=True)
    with open(os.path.join(idx, "index.bin"), "wb") as f:
        f.write(open(os.path.join(base_idx, "index.bin"), "rb").read())
    R.write_state(st, ids, base_sh, sh)
    return idx, sh


def _single_lists(st, info, x):
    """lists of the lattice state that hold one record, a lattice point with first coordinate x, away from the lists the
    tie of d3_tie is built on"""
    lens = st.lens()
    avoid = (info["L"], info["H"], info["emptied"])
    yz = st.X[st.lab == info["L"]][0][1:]
    return [l for l in range(st.k) if lens[l] == 1 and l not in avoid and st.X[st.lab == l][0][0] == x
            and not (st.X[st.lab == l][0][1:] == yz).all()]


def make_state(name, root):
    """-> (index dir, shards dir, State, info), as refine_cases.make; `name` one of its cases or of STATES"""
    if name in R.CASES:
        return make(name, root)
    idx0, sh0, st0, info = make("d3_tie", root)
    base_idx, base_sh = os.path.join(root, "base", "index"), os.path.join(root, "base", "shards")
    st, ids = R.read_state(idx0, sh0)
    assert (bits(st.X) == bits(st0.X)).all() and (st.lab == st0.lab).all()
    ext0 = np.uint64(R.EXT0 + 2_000_000)

    def append(st, ids, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        m = len(rows)
        return R._append(st, ids, rows, ext0 + np.uint64(len(ids)) + np.arange(m, dtype=np.uint64), np.uint64(9500) + np.arange(m, dtype=np.uint64))

    info = dict(info)
    if name == "twins":
        # two more copies of the record that is farthest from the centre of the first donor; the centre moves with them,
        # so the copies are made of whichever record is farthest once they are in
        for _ in range(8):
            d = plan(st.lens(), Rule())[0][0]
            Xm = st.X[st.lab == d]
            C1, _ = O.update_centroids(st.X, st.lab.astype(np.uint64), st.k)
            dist = pair_dist(Xm, C1[d][None])[:, 0]
            if (dist == dist.max()).sum() >= 3:
                break
            far = Xm[int(np.argmax(dist))]
            st, ids, lab_n = append(st, ids, np.stack([far, far]))
            assert (lab_n == d).all(), "the copies join the donor"
        else:
            raise AssertionError("no state with a tie at seed a")
        info["donor"] = d
    elif name == "copies":
        l = _single_lists(st, info, 120)[0]
        row = st.X[st.lab == l][0]
        st, ids, lab_n = append(st, ids, np.repeat(row[None], 400, axis=0))
        assert (lab_n == l).all(), "the copies join the list of their row"
        info["copies_list"] = l
    elif name == "equidistant":
        l = _single_lists(st, info, 120)[0]
        P = st.X[st.lab == l][0]
        rng = np.random.default_rng(3)
        rows = [P + np.array([-40, 0, 0]), P + np.array([40, 0, 0]), P + np.array([0, 5, 0]), P + np.array([0, -5, 0])]
        for sx in (-30, 30):
            for _ in range(40):
                rows.append(P + np.array([sx + int(rng.integers(-3, 4)), int(rng.integers(-6, 7)), int(rng.integers(-6, 7))]))
        st, ids, lab_n = append(st, ids, np.stack(rows))
        assert (lab_n == l).all(), "the rows join the list of the lattice point"
        info["equidistant_list"] = l
    else:
        raise KeyError(name)
    idx, sh = _write(root, name, st, ids, base_idx, base_sh)
    return idx, sh, st, info
