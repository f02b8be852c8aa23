"""Shared by the upsert tests: the expected shard files of an upsert, made by the CPU oracle alone — the removal of
remove_cases.expected_remove followed by the append of add_cases.expected_append — the labels of new rows from the
oracle's coarse step, and the two calls of the block cases."""
import os

import numpy as np

import oracle_lib as O

import add_cases as A
import remove_cases as R
from remove_cases import all_bytes, shard_files

NEW_EXT0 = 70_000_000          # external ids no base record carries


def oracle_labels(orc, x):
    """list of every row: the first probe of the oracle's coarse step"""
    out = np.zeros(len(x), dtype=np.uint64)
    for i, v in enumerate(x):
        rc, p = orc.probe(v, 1)
        assert rc == O.ORC_OK and len(p) == 1
        out[i] = p[0]
    return out


def expected_upsert(src_dir, dst_dir, shard_id, removed_ext, cids, ids, ext, ts, vecs, dim):
    """shard_<id>.bin of src_dir without the records whose external id is in removed_ext, then with record i appended to
    list cids[i] (call order inside a list): the oracle's reader and writer, twice -> (its bytes, records removed)"""
    mid_dir = dst_dir + "_removed"
    raw, n_removed = R.expected_remove(src_dir, mid_dir, shard_id, removed_ext, dim)
    if len(cids):
        raw = A.expected_append(mid_dir, dst_dir, shard_id, cids, ids, ext, ts, vecs)
    return raw, n_removed


def expected_files(c2s, sh, exp_dir, labels, ids, ext, ts, x, dim):
    """every shard file after the upsert of rows x (external ids ext, internal ids ids, lists `labels`) ->
    ({name: bytes}, {name: records removed from it}, {name: records it received})"""
    want, removed, received = {}, {}, {}
    shard_of_row = np.asarray(c2s)[np.asarray(labels, dtype=np.int64)]
    for f in shard_files(sh):
        s = int(f[len("shard_"):-len(".bin")])
        pick = np.flatnonzero(shard_of_row == s)
        want[f], removed[f] = expected_upsert(sh, os.path.join(exp_dir, f"s{s}"), s, ext, labels[pick], ids[pick], ext[pick],
                                              ts[pick], x[pick], dim)
        received[f] = len(pick)
    return want, removed, received


def rows_near(cent, aims, rng, integer=False):
    """one row per entry of aims, next to the centroid of that list"""
    c = cent[np.asarray(aims, dtype=np.int64)]
    if integer:
        return np.rint(c).astype(np.float32)
    return (c + 1e-3 * rng.standard_normal(c.shape)).astype(np.float32)


def block_case_lists(lens):
    """the lists of the block cases: E the shortest, B and C ragged, A / D / G longer than a block"""
    order = np.argsort(lens, kind="stable")
    e = int(order[0])
    long = [int(l) for l in order if lens[l] > 64 and l != e]
    b, c = [l for l in long if lens[l] % 64 != 0][:2]
    a, d, g = [l for l in long if l not in (b, c)][:3]
    assert len({a, b, c, d, e, g}) == 6 and len(lens) - 6 >= 3
    return dict(A=a, B=b, C=c, D=d, E=e, G=g)


def block_case_calls(cent, lens, lists, rng):
    """-> (aim, [(ext ids, list aimed at per row), (…)]) for two calls, unsorted and with duplicates.
    call 1, one list each: A loses record 5 of its first block and receives 1 row (its length stays, every later position
    moves); B loses its tail down to a multiple of 64 and receives as many rows (the first lands in lane 0 of a new
    block); C loses its first 64 records and receives 70 (new rows span a block border, one block mixes kept and new
    lanes); D loses everything and receives 5; E loses everything and receives nothing; G loses nothing and receives the
    rows of D's and E's other ids and one more of A's id (named twice: added twice).  The other lists: nothing.
    call 2: E, now without a block, receives 70 rows; A's first three records are upserted again; ids nothing carries
    join G; and the id call 1 added twice, which two records carry now (in A and in G), loses both for one row in G."""
    aim = block_case_lists(lens)
    a, b, c, d, e, g = (aim[k] for k in "ABCDEG")
    L = lists
    tail = L[b][len(L[b]) - len(L[b]) % 64:]
    fresh = np.uint64(NEW_EXT0) + np.arange(6, dtype=np.uint64)
    ext1 = np.concatenate([L[a][5:6], tail, L[c][:64], fresh, L[d], L[e], L[a][5:6]])
    aim1 = np.concatenate([[a], [b] * len(tail), [c] * 70, [d] * 5, [g] * (len(L[d]) - 5), [g] * len(L[e]), [g]])
    p1 = rng.permutation(len(ext1))
    left_a = np.delete(L[a], 5)
    nobody = np.array([1, 2, (1 << 64) - 2], dtype=np.uint64)
    ext2 = np.concatenate([np.uint64(NEW_EXT0 + 100) + np.arange(70, dtype=np.uint64), left_a[:3], nobody, L[a][5:6]])
    aim2 = np.concatenate([[e] * 70, [a] * 3, [g] * 3, [g]])
    p2 = rng.permutation(len(ext2))
    return aim, [(ext1[p1], aim1[p1].astype(np.int64)), (ext2[p2], aim2[p2].astype(np.int64))]


__all__ = ["all_bytes", "block_case_calls", "block_case_lists", "expected_files", "expected_upsert", "oracle_labels", "rows_near"]
