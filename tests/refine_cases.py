"""Inputs and the expected outcome of vi_indexer_refine, made by the CPU oracle alone.

A plain module (no fixtures, no GPU): tests/test_refine_cases_cpu.py proves on the CPU that every case can fail (records
move, a list runs empty, ...), tests/test_refine_gpu.py runs the cases through the library.

A case is a pair of directories and the STATE of the index they hold: the records in list order (X, lab, ext, ts), the
table C and centroids_to_shard.  make(name, root) writes the base index with the oracle's build at nlist 20, reads its lists
back with the oracle's reader and then, in numpy and with the oracle's writer only, does what the update calls of the
library are tested elsewhere to do byte for byte: empties one list and shortens another (remove_ids), and appends records
drawn around a shifted centre to the list of their nearest centroid, so that they pile into two or three lists (add).

replay(state) is one iteration of the contract from the oracle's primitives: centres from O.update_centroids with the
empty lists restored to their old centroid, labels from nearest() — a numpy restatement of the reference's scalar chain
(per pair an f32 accumulate of (a - b) * (a - b) over d, separate multiply and add; the lowest index among equal
distances), which the CPU test holds to O.l2sq_scalar and the oracle's probe — and the stable regrouping.
"""
import os
from dataclasses import dataclass

import numpy as np

import oracle_lib as O
from add_cases import shard_bytes, shard_centroid_ids
from remove_cases import shard_files

NOW = 1_700_000_000
NLIST = 20
EXT0 = 5_000_000

CASES = {  # name -> (dimension, data kind, what the case is for)
    "d3_tie": (3, "lattice", "D = 3 (padding to dq), integer values 0..255; two records equidistant from two centroids after recentring"),
    "d96_real": (96, "real", "D = 96, real values"),
    "d128_real_long": (128, "real", "D = 128, real values; one list longer than 4096 records (more than 64 blocks)"),
    "d128_u8": (128, "u8", "D = 128, values 0..255: the int8 images of the rebuilt index"),
    "d160_real": (160, "real", "D = 160, real values: the wide rank path"),
}


@dataclass
class State:
    X: np.ndarray        # n x d f32, list order
    lab: np.ndarray      # n, non-decreasing
    ext: np.ndarray      # n u64
    ts: np.ndarray       # n u64
    origin: np.ndarray   # n: the record's position in the state the case was made with
    C: np.ndarray        # k x d f32
    c2s: np.ndarray      # k u64

    @property
    def k(self):
        return len(self.C)

    def lens(self):
        return np.bincount(self.lab.astype(np.int64), minlength=self.k)


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def pair_dist(A, B):
    """[len(A), len(B)] f32: the reference's scalar chain (src/utils.rs:28-30) for every pair"""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for j in range(A.shape[1]):
        t = A[:, j, None] - B[None, :, j]
        acc = acc + t * t   # (two f32 operations: numpy fuses nothing)
    return acc


def nearest(X, C):
    """the list the coarse step probes first for every row: lowest index among equal distances"""
    out = np.zeros(len(X), dtype=np.int64)
    for a in range(0, len(X), 2048):
        out[a:a + 2048] = np.argmin(pair_dist(X[a:a + 2048], C), axis=1)
    return out


def read_state(idx, sh):
    orc = O.OracleIndex.load(idx, sh)
    C, c2s = orc.centroids()
    parts = []
    for l in range(len(C)):
        rc, got = O.shard_get(sh, int(c2s[l]), [l])
        assert rc == O.ORC_OK
        parts.append((got[0][2], got[0][3]))
    metas = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 3), dtype=np.uint64)
    X = np.concatenate([p[1].reshape(-1, C.shape[1]) for p in parts]).astype(np.float32)
    lab = np.repeat(np.arange(len(C)), [len(p[0]) for p in parts]).astype(np.int64)
    return State(np.ascontiguousarray(X), lab, metas[:, 1].copy(), metas[:, 2].copy(), np.arange(len(lab)), C, c2s), metas[:, 0].copy()


def write_state(st, ids, base_sh, dst_sh):
    """every shard file of base_sh (its lists in their file order) holding the lists of st, by the oracle's writer; ids:
    VectorMeta.id of every record"""
    os.makedirs(dst_sh, exist_ok=True)
    d = st.X.shape[1]
    for f in shard_files(base_sh):
        s = int(f[len("shard_"):-len(".bin")])
        cids = shard_centroid_ids(base_sh, s)
        lists = []
        for c in cids:
            m = np.flatnonzero(st.lab == c)
            lists.append((ids[m], st.ext[m], st.ts[m], st.X[m].reshape(-1, d)))
        cents = st.C[np.asarray(cids, dtype=np.int64)] if cids else np.zeros((0, d), dtype=np.float32)
        assert O.shard_save(dst_sh, s, d, cids, cents, lists) == O.ORC_OK
    return {f: shard_bytes(dst_sh, int(f[len("shard_"):-len(".bin")])) for f in shard_files(dst_sh)}


def _lattice_points():
    g = np.array([[x, y, z] for x in (20, 120, 220) for y in (20, 120, 220) for z in (20, 120, 220)], dtype=np.float32)
    return g[:NLIST].copy()   # (x = 20 and 120 whole, two points of x = 220)


FAR_A, FAR_B = 30, 40   # records of the two far groups


def _clustered(rng, n, d, kind):
    """n rows around 12 centres, and behind them two small groups far from everything and from each other (k-means++ gives
    each a list of its own: make() checks it) -> (rows, the two far points)"""
    centres = rng.standard_normal((12, d)).astype(np.float32) * np.float32(4.0)
    X = centres[rng.integers(0, 12, n - FAR_A - FAR_B)] + rng.standard_normal((n - FAR_A - FAR_B, d)).astype(np.float32)
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    far = np.stack([9 * sign, -9 * sign]).astype(np.float32)
    far[1, : d // 2] *= -1
    groups = [far[i] + np.float32(0.3) * rng.standard_normal((m, d)).astype(np.float32) for i, m in enumerate((FAR_A, FAR_B))]
    X = np.concatenate([X] + groups)
    if kind == "u8":
        X, far = np.clip(np.rint(128 + 12 * X), 0, 255), 128 + 12 * far
    return np.ascontiguousarray(X, dtype=np.float32), far.astype(np.float32)


def _drop(st, ids, gone):
    keep = ~gone
    return State(st.X[keep], st.lab[keep], st.ext[keep], st.ts[keep], np.arange(int(keep.sum())), st.C, st.c2s), ids[keep]


def _append(st, ids, Xn, ext, ts):
    """add(): every row to the list of its nearest centroid, behind the list's records, internal ids n, n + 1, ..."""
    lab_n = nearest(Xn, st.C)
    X = np.concatenate([st.X, Xn.astype(np.float32)])
    lab = np.concatenate([st.lab, lab_n])
    o = np.argsort(lab, kind="stable")
    new_ids = np.concatenate([ids, len(ids) + np.arange(len(Xn), dtype=np.uint64)])
    out = State(np.ascontiguousarray(X[o]), lab[o], np.concatenate([st.ext, ext])[o], np.concatenate([st.ts, ts])[o],
                np.arange(len(lab)), st.C, st.c2s)
    return out, new_ids[o], lab_n


def make(name, root):
    """-> (index dir, shards dir, State, info): the directories hold the state"""
    d, kind, _ = CASES[name]
    rng = _rng(name)
    base_idx, base_sh = os.path.join(root, "base", "index"), os.path.join(root, "base", "shards")
    if kind == "lattice":
        X0 = _lattice_points()
    else:
        X0, far = _clustered(rng, 3000, d, kind)
    n0 = len(X0)
    O.OracleIndex.build(X0, base_idx, base_sh, ext_ids=np.uint64(EXT0) + np.arange(n0, dtype=np.uint64),
                        timestamps=np.uint64(1000) + (np.arange(n0, dtype=np.uint64) * np.uint64(7919)) % np.uint64(1000),
                        nlist=NLIST, now=NOW)
    st, ids = read_state(base_idx, base_sh)
    info = {}
    lens = st.lens()
    if kind == "lattice":
        # (the mini-batch run leaves centroids a few ulp off the points, and may merge two points into one list)
        single = [l for l in range(st.k) if lens[l] == 1]
        P = {l: st.X[st.lab == l][0] for l in single}               # the one record of each such list: a lattice point
        # L < H: two such lists whose points are 100 apart along x (120 and 220), the lower index first
        L, H = [(a, b) for a in single for b in single
                if a < b and {P[a][0], P[b][0]} == {120, 220} and (P[a][1:] == P[b][1:]).all()][0]
        u = np.array([np.sign(P[H][0] - P[L][0]), 0, 0], dtype=np.float32)
        y7 = np.array([0, 7, 0], dtype=np.float32)
        tie = np.stack([P[L] + 50 * u + y7, P[L] + 50 * u - y7])    # on the bisector of the two POINTS
        side = nearest(tie, st.C)                                   # where an add puts them: the centroids are a few ulp off
        assert set(side) <= {L, H}
        # the records beside them, such that the means come out as C'[L] = P[L] + 10 u and C'[H] = P[H] - 10 u, integers
        # both: the tie records are equidistant from the two centres AFTER the recentring, exactly
        extra = []
        for l, p, w in ((L, P[L], u), (H, P[H], -u)):
            mine = tie[side == l]
            ysum = (mine - (P[L] + 50 * u)).sum(axis=0)
            steps = {0: [20], 1: [-5, -5], 2: [-25, -25]}[len(mine)]
            rows = [p + a * w for a in steps]
            rows[0] = rows[0] - ysum
            extra += rows
        extra = np.stack(extra)
        # the drifted records: integer rows between three lattice points of the x = 20 face
        face = [l for l in single if P[l][0] == 20]
        centre = (P[face[0]] + P[face[1]] + P[face[3]]) / 3 + np.array([9, -4, 6], dtype=np.float32)
        cloud = np.clip(np.rint(centre + 28 * rng.standard_normal((400, 3))), 0, 255).astype(np.float32)
        Xn = np.concatenate([tie, extra, cloud])
        cand = [l for l in single if l not in (L, H) and P[l][0] != 20]
        emptied = max(cand, key=lambda l: float(((P[l] - centre) ** 2).sum()))    # the point farthest from the drift
        assert not (nearest(Xn, st.C) == emptied).any()
        info.update(L=L, H=H, tie=tie, emptied=emptied, want_L=P[L] + 10 * u, want_H=P[H] - 10 * u)
    else:
        # the drifted records: around a point between the two closest centroids, pushed off their line
        D = pair_dist(st.C, st.C).astype(np.float64) + np.eye(st.k) * 1e30
        a, b = np.unravel_index(np.argmin(D), D.shape)
        shift = rng.standard_normal(d).astype(np.float32)
        shift *= np.float32(0.6 * np.sqrt(D[a, b]) / np.linalg.norm(shift))
        centre = (st.C[a] + st.C[b]) / 2 + shift
        m = 4800 if name.endswith("_long") else 1500
        spread = (12.0 if kind == "u8" else 1.0) * 0.5
        Xn = centre + np.float32(spread) * rng.standard_normal((m, d)).astype(np.float32)
        if kind == "u8":
            Xn = np.clip(np.rint(Xn), 0, 255)
        # emptied: the list of the first far group; shortened to 10 records: the list of the second
        emptied, short = (int(l) for l in nearest(far, st.C))
        assert lens[emptied] == FAR_A and lens[short] == FAR_B, "each far group is one list"
        gone = (st.lab == short) & (np.cumsum(st.lab == short) > 10)
        st, ids = _drop(st, ids, gone)
        info.update(emptied=emptied, short=short)
    st, ids = _drop(st, ids, st.lab == info["emptied"])
    m = len(Xn)
    ts = np.uint64(9000) + np.arange(m, dtype=np.uint64)
    st, ids, lab_n = _append(st, ids, np.ascontiguousarray(Xn, dtype=np.float32), np.uint64(EXT0 + 1_000_000) + np.arange(m, dtype=np.uint64), ts)
    info["added_labels"] = lab_n
    idx, sh = os.path.join(root, "case", "index"), os.path.join(root, "case", "shards")
    os.makedirs(idx, exist_ok=True)
    with open(os.path.join(idx, "index.bin"), "wb") as f:       # (no update call touches the table)
        f.write(open(os.path.join(base_idx, "index.bin"), "rb").read())
    write_state(st, ids, base_sh, sh)
    return idx, sh, st, info


def replay(st):
    """one iteration -> (the state after it, records it moved)"""
    k = st.k
    C2, counts = O.update_centroids(st.X, st.lab.astype(np.uint64), k)
    C2[counts == 0] = st.C[counts == 0]            # an empty list keeps its centroid, bit for bit
    lab2 = nearest(st.X, C2)
    o = np.argsort(lab2, kind="stable")
    moved = int((lab2 != st.lab).sum())
    return State(np.ascontiguousarray(st.X[o]), lab2[o], st.ext[o], st.ts[o], st.origin[o], C2, st.c2s), moved


def moved_between(first, last):
    """records whose list in `last` differs from their list in `first` (the state their origin numbers)"""
    lab0 = np.empty(len(first.lab), dtype=np.int64)
    lab0[first.origin] = first.lab
    return int((last.lab != lab0[last.origin]).sum())


def expected_files(st, base_sh, dst_sh):
    """the shard files of the state as a refine leaves them: VectorMeta.id = position in list order"""
    return write_state(st, np.arange(len(st.lab), dtype=np.uint64), base_sh, dst_sh)


def inertia(st):
    """sum over the records of ||x - centroid of its list||^2, in f64"""
    diff = st.X.astype(np.float64) - st.C.astype(np.float64)[st.lab]
    return float((diff * diff).sum())


def imbalance(lens):
    lens = np.asarray(lens, dtype=np.float64)
    return float(len(lens) * (lens * lens).sum() / lens.sum() ** 2)


REFILLED_CASES = ("d3_tie", "d96_real")   # an emptied list of these receives records again (test_refine_cases_cpu proves it)


def emptied_outcomes(st):
    """what one iteration does after remove_ids has emptied one list: for the three shortest and the three longest lists
    with records, {list: (records it holds after the replay, the state without its records, that state replayed)}"""
    lens = st.lens()
    by_len = sorted((l for l in range(st.k) if lens[l] > 0), key=lambda l: (lens[l], l))
    out = {}
    for l in sorted(set(by_len[:3] + by_len[-3:])):
        keep = st.lab != l
        cut = State(st.X[keep], st.lab[keep], st.ext[keep], st.ts[keep], np.arange(int(keep.sum())), st.C, st.c2s)
        after, _ = replay(cut)
        out[l] = (int(after.lens()[l]), cut, after)
    return out
