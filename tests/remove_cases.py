"""Shared by the remove-records tests: the expected shard files of a removal, made by the CPU oracle alone (read the lists,
mask in numpy, save into a second directory), and small helpers around them."""
import os

import numpy as np

import oracle_lib as O

from add_cases import shard_bytes, shard_centroid_ids


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shard_files(sh):
    return sorted(f for f in os.listdir(sh) if f.startswith("shard_"))


def all_bytes(sh):
    return {f: open(os.path.join(sh, f), "rb").read() for f in shard_files(sh)}


def shard_lists(shards_dir, shard_id):
    """[(centroid id, centroid, metas[n x 3] = id / external id / timestamp, vecs[n x dim])] in file order"""
    rc, lists = O.shard_get(shards_dir, shard_id, shard_centroid_ids(shards_dir, shard_id))
    assert rc == O.ORC_OK
    return lists


def expected_remove(src_dir, dst_dir, shard_id, removed_ext, dim):
    """shard_<id>.bin of src_dir without the records whose external id is in removed_ext, written by the oracle into
    dst_dir; returns (its bytes, records removed)"""
    lists = shard_lists(src_dir, shard_id)
    gone = np.asarray(removed_ext, dtype=np.uint64)
    kept, n_removed = [], 0
    for cid, cent, metas, vecs in lists:
        stay = ~np.isin(metas[:, 1], gone)
        n_removed += int((~stay).sum())
        kept.append((metas[stay, 0], metas[stay, 1], metas[stay, 2], vecs[stay].reshape(-1, dim)))
    os.makedirs(dst_dir, exist_ok=True)
    cents = np.stack([l[1] for l in lists]) if lists else np.zeros((0, dim), dtype=np.float32)
    assert O.shard_save(dst_dir, shard_id, dim, [l[0] for l in lists], cents, kept) == O.ORC_OK
    return shard_bytes(dst_dir, shard_id), n_removed


def expected_files(sh, exp_dir, removed_ext, dim):
    """every shard file after the removal -> ({name: bytes}, {name: records removed from it})"""
    want, counts = {}, {}
    for f in shard_files(sh):
        s = int(f[len("shard_"):-len(".bin")])
        want[f], counts[f] = expected_remove(sh, exp_dir, s, removed_ext, dim)
    return want, counts


def assert_same(Dg, Ig, Do, Io, what):
    bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[0]}: got {Ig[bad[0]][:8]} {Dg[bad[0]][:8]} "
                           f"expected {Io[bad[0]][:8]} {Do[bad[0]][:8]}")
