"""Shared by the add-records tests: the expected shard files of an append, made by the CPU oracle alone (read the lists,
append in numpy, save into a second directory), and small helpers around them."""
import os
import struct

import numpy as np

import oracle_lib as O


def shard_centroid_ids(shards_dir, shard_id):
    """centroid ids of a shard file in file order (ShardHeader.num_centroids at byte 20, IndexEntry.centroid_id first of 32 bytes)"""
    raw = open(os.path.join(shards_dir, f"shard_{shard_id}.bin"), "rb").read()
    nl = struct.unpack_from("<I", raw, 20)[0]
    index_off = struct.unpack_from("<Q", raw, 24)[0]
    return [struct.unpack_from("<Q", raw, index_off + 32 * i)[0] for i in range(nl)]


def shard_bytes(shards_dir, shard_id):
    return open(os.path.join(shards_dir, f"shard_{shard_id}.bin"), "rb").read()


def expected_append(src_dir, dst_dir, shard_id, cids, ids, ext, ts, vecs):
    """shard_<id>.bin of src_dir with record i appended to list cids[i] (call order inside a list), written by the oracle
    into dst_dir; returns its bytes"""
    file_cids = shard_centroid_ids(src_dir, shard_id)
    rc, lists = O.shard_get(src_dir, shard_id, file_cids)
    assert rc == O.ORC_OK
    dim = lists[0][1].shape[0] if lists else np.asarray(vecs).shape[1]
    cids = np.asarray(cids, dtype=np.uint64)
    vecs = np.asarray(vecs, dtype=np.float32).reshape(len(cids), dim)
    merged = []
    for cid, cent, metas, old in lists:
        pick = np.flatnonzero(cids == cid)
        merged.append((np.concatenate([metas[:, 0], np.asarray(ids, dtype=np.uint64)[pick]]),
                       np.concatenate([metas[:, 1], np.asarray(ext, dtype=np.uint64)[pick]]),
                       np.concatenate([metas[:, 2], np.asarray(ts, dtype=np.uint64)[pick]]),
                       np.concatenate([old, vecs[pick]]).reshape(-1, dim)))
    os.makedirs(dst_dir, exist_ok=True)
    assert O.shard_save(dst_dir, shard_id, dim, file_cids, np.stack([l[1] for l in lists]), merged) == O.ORC_OK
    return shard_bytes(dst_dir, shard_id)
