// index_lifecycle.hpp — what makes and remakes the index of a handle: the build, the load, the updates of a built index
// (add, retain / remove, upsert) and its refine.  The extern "C" functions of api.cpp check their arguments and call these.
#pragma once
#include <memory>

#include "device_index.hpp"

namespace vi {

// mirrors VectorIndexer{cfg, index} — src/api.rs:96-99
struct Indexer {
  vi_config cfg{};
  std::string index_dir, shards_dir;
  IndexMeta meta;                       // IvfIndex{centroids, centroids_to_shard, dimension}
  std::unique_ptr<DeviceIndex> dev;     // HBM-resident lists (null until load/build)
  vi_build_stats build_stats{};         // phases of the last build on this handle
  vi_add_stats add_stats{};             // ... and of the last vi_indexer_add_records that added something
  vi_remove_stats remove_stats{};       // ... and of the last vi_indexer_retain / vi_indexer_remove_ids that removed something
  vi_upsert_stats upsert_stats{};       // ... and of the last vi_indexer_upsert_records with n > 0
  vi_refine_stats refine_stats{};       // ... and of the last vi_indexer_refine with iters > 0
  vi_rebalance_stats rebalance_stats{}; // ... and of the last vi_indexer_rebalance
};

// the resident index of this rank from the handle's files (a load; the build of a rank of a multi-GPU run)
vi_status attach_device(Indexer *ix);
// IvfIndex::fit_with_paths (src/ivf_index.rs:58-177) + save_to (:274-294): files and resident index from n host rows
vi_status fit_and_save(Indexer *ix, const float *X, const uint64_t *ext_ids, const uint64_t *timestamps, uint64_t n);
// the lengths of the resident lists, read back once per call
vi_status read_list_lengths(const DeviceIndex &ix, std::vector<uint32_t> *len);

// The entries of a built, unpartitioned index behind their argument checks; each succeeds or leaves handle and files as
// they were.  add: ext_ids null = the internal ids.  retain: `keep` is a filter of ix->dev.  refine: iters > 0.
vi_status add_records(Indexer *ix, const uint64_t *ext_ids, const float *X, const uint64_t *timestamps, uint64_t n);
vi_status retain_records(Indexer *ix, const SlotFilter &keep, uint64_t *removed_out);
vi_status upsert_records(Indexer *ix, const uint64_t *ext_ids, const float *X, const uint64_t *timestamps, uint64_t n,
                         uint64_t *replaced_out);
vi_status refine_records(Indexer *ix, uint64_t iters, uint64_t *moved_out, const SplitRule *rule = nullptr);

}  // namespace vi
