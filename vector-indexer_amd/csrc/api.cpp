// api.cpp — the extern "C" boundary declared in include/vi_amd.h, the host-side mirror of the reference's public surface
// (src/api.rs): the opaque handles, the argument checks, the guard against exceptions.  What builds, loads, updates or
// refines the index of a handle is index_lifecycle.cpp.
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>

#include "device_index.hpp"
#include "index_lifecycle.hpp"
#include "kmeans.hpp"
#include "probe_rules.hpp"
#include "record_fetch.hpp"
#include "refine_rules.hpp"
#include "rng.hpp"
#include "shards.hpp"
#include "slot_filter.hpp"

namespace vi {

std::string &last_error_ref() {
  static thread_local std::string msg;
  return msg;
}

// No C++ exception may unwind through the C ABI into a Rust / ctypes caller (std::vector growth, std::string, a
// corrupt length field...): every extern "C" entry point that returns a status runs its body in here.
template <typename F>
static vi_status guarded(F &&body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return fail(VI_ERR_OTHER, "out of host memory");
  } catch (const std::exception &e) {
    return fail(VI_ERR_OTHER, "internal error: %s", e.what());
  } catch (...) {
    return fail(VI_ERR_OTHER, "internal error");
  }
}

}  // namespace vi

using vi::fail;
using vi::Indexer;

struct vi_indexer {
  Indexer impl;
};

struct vi_filter {
  vi::SlotFilter impl;
};

struct vi_range_result {
  vi::RangeResult impl;
};

extern "C" {

const char *vi_last_error(void) { return vi::last_error_ref().c_str(); }
uint32_t vi_abi_version(void) { return VI_AMD_ABI_VERSION; }
int vi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// src/utils.rs:9-16
uint64_t vi_calculate_num_clusters(uint64_t n) {
  if (n < 10000) return (uint64_t)std::sqrt((double)n);
  if (n < 100000) return 2 * (uint64_t)std::ceil(std::sqrt((double)n));
  return 4 * (uint64_t)std::ceil(std::sqrt((double)n));
}
// src/utils.rs:18-26
uint64_t vi_calculate_max_iterations(uint64_t n) { return n < 10000 ? 300 : n < 100000 ? 100 : n < 1000000 ? 50 : 20; }
// src/kmeans.rs:83
uint64_t vi_minibatch_size(uint64_t n) {
  const uint64_t s = (uint64_t)std::sqrt((float)n);
  return s < 10 ? 10 : s > 256 ? 256 : s;
}

vi_status vi_l2sq_pairs(const float *a, const float *b, uint64_t n, uint32_t d, vi_sum_order order, float *out) {
  return vi::guarded([&]() -> vi_status {
  if ((n && (!a || !b || !out))) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  return vi::l2sq_pairs_device(a, b, n, d, (int)order, out);
  });
}

vi_status vi_assign(const float *X, uint64_t n, uint32_t d, const float *C, uint64_t k, uint64_t seed,
                    vi_assign_mode mode, uint64_t *labels, float *dist_out) {
  return vi::guarded([&]() -> vi_status {
  if (n == 0) return VI_OK;
  if (!X || !C || !labels || d == 0 || k == 0) return fail(VI_ERR_INVALID_INPUT, "bad arguments to vi_assign");
  vi::KMeansOptions opt;
  opt.mode = mode;
  return vi::assign_points(X, n, d, C, k, seed, opt, labels, dist_out);
  });
}

vi_status vi_assign_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, const float *C_dev, uint64_t k,
                           uint64_t seed, vi_assign_mode mode, uint32_t *labels_dev, vi_assign_stats *stats) {
  return vi::guarded([&]() -> vi_status {
  if (n == 0) return VI_OK;
  if (!X_dev || !C_dev || !labels_dev || d == 0 || k == 0) return fail(VI_ERR_INVALID_INPUT, "bad arguments to vi_assign_device");
  return vi::assign_points_device(device, X_dev, n, d, C_dev, k, seed, mode, labels_dev, stats);
  });
}

vi_status vi_kmeans_mini_batch(const float *X, uint64_t n, uint32_t d, uint64_t k, uint64_t max_iters, float thr,
                               uint64_t seed, vi_assign_mode mode, float *C, uint64_t *labels, uint64_t *iters) {
  return vi::guarded([&]() -> vi_status {
  vi::KMeansOptions opt;
  opt.mode = mode;
  return vi::kmeans_mini_batch(X, n, d, k, max_iters, thr, seed, opt, C, labels, iters);
  });
}

vi_status vi_kmeans_parallel(const float *X, uint64_t n, uint32_t d, uint64_t k, uint64_t max_iters, float thr,
                             uint64_t seed, vi_assign_mode mode, float *C, uint64_t *labels, uint64_t *iters) {
  return vi::guarded([&]() -> vi_status {
  vi::KMeansOptions opt;
  opt.mode = mode;
  return vi::kmeans_parallel(X, n, d, k, max_iters, thr, seed, opt, C, labels, iters);
  });
}

vi_status vi_kmeans_mini_batch_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, uint64_t k,
                                      uint64_t max_iters, float thr, uint64_t seed, vi_assign_mode mode, float *C_dev,
                                      uint32_t *labels_dev, uint64_t *iters) {
  return vi::guarded([&]() -> vi_status {
  return vi::kmeans_mini_batch_device(device, X_dev, n, d, k, max_iters, thr, seed, mode, C_dev, labels_dev, iters);
  });
}

vi_status vi_kmeans_parallel_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, uint64_t k,
                                    uint64_t max_iters, float thr, uint64_t seed, vi_assign_mode mode, float *C_dev,
                                    uint32_t *labels_dev, uint64_t *iters) {
  return vi::guarded([&]() -> vi_status {
  return vi::kmeans_parallel_device(device, X_dev, n, d, k, max_iters, thr, seed, mode, C_dev, labels_dev, iters);
  });
}

vi_status vi_kmeans_mini_batch_train(int32_t device, const vi_row_source *rows, uint64_t n, uint32_t d, uint64_t k,
                                     uint64_t max_iters, float thr, uint64_t seed, float *C_dev, uint64_t *iters) {
  return vi::guarded([&]() -> vi_status {
  if (!rows) return fail(VI_ERR_INVALID_INPUT, "null row source");
  return vi::kmeans_mini_batch_train(device, *rows, n, d, k, max_iters, thr, seed, C_dev, iters);
  });
}

vi_status vi_kmeans_pp_init(int32_t device, const vi_row_source *rows, uint64_t n, uint32_t d, uint64_t k, uint64_t seed,
                            float *C_dev) {
  return vi::guarded([&]() -> vi_status {
  if (!rows) return fail(VI_ERR_INVALID_INPUT, "null row source");
  return vi::kmeans_pp_init_rows_entry(device, *rows, n, d, k, seed, C_dev);
  });
}

vi_status vi_kmeans_partial_sums_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d,
                                        const uint32_t *labels_dev, uint64_t k, float *sums_dev, uint32_t *counts_dev) {
  return vi::guarded([&]() -> vi_status {
  return vi::kmeans_partial_sums_device(device, X_dev, n, d, labels_dev, k, sums_dev, counts_dev);
  });
}

vi_status vi_kmeans_finish_update_device(int32_t device, const float *sums_dev, const uint32_t *counts_dev, uint64_t k,
                                         uint32_t d, const float *C_prev_dev, float *C_new_dev, float *delta_out,
                                         uint32_t *empty_out, uint64_t *n_empty) {
  return vi::guarded([&]() -> vi_status {
  return vi::kmeans_finish_update_device(device, sums_dev, counts_dev, k, d, C_prev_dev, C_new_dev, delta_out, empty_out,
                                         n_empty);
  });
}

vi_status vi_kmeans_centroid_delta_device(int32_t device, const float *C_new_dev, const float *C_prev_dev, uint64_t k,
                                          uint32_t d, float *delta_out) {
  return vi::guarded([&]() -> vi_status {
  return vi::kmeans_centroid_delta(device, C_new_dev, C_prev_dev, k, d, delta_out);
  });
}

vi_rng *vi_rng_seed_from_u64(uint64_t seed) { return reinterpret_cast<vi_rng *>(new (std::nothrow) vi::StdRng(seed)); }
uint64_t vi_rng_gen_range(vi_rng *rng, uint64_t low, uint64_t high) {
  if (!rng || high <= low) return low;
  return reinterpret_cast<vi::StdRng *>(rng)->gen_range(low, high);
}
void vi_rng_free(vi_rng *rng) { delete reinterpret_cast<vi::StdRng *>(rng); }

vi_status vi_shard_save_to(const char *shards_dir, uint64_t shard_id, uint32_t dim, uint32_t num_lists,
                           const uint64_t *centroid_ids, const float *centroid_vecs, const uint64_t *list_off,
                           const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps,
                           const float *vecs) {
  return vi::guarded([&]() -> vi_status {
  if (!shards_dir || !list_off) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  return vi::shard_save_to(shards_dir, shard_id, dim, num_lists, centroid_ids, centroid_vecs, list_off, ids, ext_ids,
                           timestamps, vecs);
  });
}

vi_status vi_shard_get_centroid_vectors_from(const char *shards_dir, uint64_t shard_id, const uint64_t *centroid_ids,
                                             uint64_t n_req, uint32_t *dim_out, uint64_t *counts, float *centroid_out,
                                             uint64_t *metas_out, float *vecs_out) {
  return vi::guarded([&]() -> vi_status {
  if (!shards_dir) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  vi::ShardFile f;
  VI_TRY(f.open(shards_dir, shard_id));
  const uint32_t dim = f.dim();
  if (dim_out) *dim_out = dim;
  const uint64_t stride = vi::record_stride(dim);
  uint64_t vbase = 0;
  for (uint64_t r = 0; r < n_req; ++r) {
    const vi::ShardListView *lv = f.find(centroid_ids[r]);
    if (!lv) return fail(VI_ERR_NOT_FOUND, "Centroid %llu not found", (unsigned long long)centroid_ids[r]);
    if (counts) counts[r] = lv->num_vectors;
    if (centroid_out) std::memcpy(centroid_out + r * dim, lv->centroid, 4ull * dim);
    for (uint32_t v = 0; v < lv->num_vectors; ++v) {
      const uint8_t *rec = lv->records + (uint64_t)v * stride;
      if (metas_out) std::memcpy(metas_out + (vbase + v) * 3, rec, vi::kVectorMetaBytes);
      if (vecs_out) std::memcpy(vecs_out + (vbase + v) * dim, rec + vi::kVectorMetaBytes, 4ull * dim);
    }
    vbase += lv->num_vectors;
  }
  return VI_OK;
  });
}

vi_status vi_shard_append_to(const char *shards_dir, uint64_t shard_id, uint64_t n_add, const uint64_t *centroid_ids,
                             const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs) {
  return vi::guarded([&]() -> vi_status {
  if (!shards_dir) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (n_add && (!centroid_ids || !ids || !ext_ids || !timestamps || !vecs)) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  return vi::shard_append_to(shards_dir, shard_id, n_add, centroid_ids, ids, ext_ids, timestamps, vecs);
  });
}

void vi_config_init(vi_config *cfg, uint32_t dimension) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->dimension = dimension;
  cfg->default_k = 10;
  cfg->default_n_probe = 20;
  cfg->max_k = 10000;
  cfg->max_n_probe = 10000;
}

vi_status vi_indexer_new(const vi_config *cfg, vi_indexer **out) {
  return vi::guarded([&]() -> vi_status {
  if (!cfg || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  auto *h = new vi_indexer();
  h->impl.cfg = *cfg;
  h->impl.index_dir = cfg->index_dir ? cfg->index_dir : "index";
  h->impl.shards_dir = cfg->shards_dir ? cfg->shards_dir : "shards";
  h->impl.cfg.index_dir = nullptr;
  h->impl.cfg.shards_dir = nullptr;
  h->impl.meta.dimension = cfg->dimension;
  *out = h;
  return VI_OK;
  });
}

vi_status vi_indexer_load(const vi_config *cfg, vi_indexer **out) {
  return vi::guarded([&]() -> vi_status {
  vi_indexer *h = nullptr;
  VI_TRY(vi_indexer_new(cfg, &h));
  vi_status st = vi::index_meta_load(h->impl.index_dir, &h->impl.meta);
  if (st == VI_OK) st = vi::attach_device(&h->impl);
  if (st != VI_OK) { delete h; return st; }
  *out = h;
  return VI_OK;
  });
}

vi_status vi_indexer_build_from_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values,
                                        const uint64_t *timestamps, const uint32_t *dims, uint64_t n) {
  return vi::guarded([&]() -> vi_status {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (n == 0) return fail(VI_ERR_INVALID_INPUT, "no vectors provided");  // api.rs:116-118
  const uint32_t dim = ix->impl.cfg.dimension;
  if (dims)
    for (uint64_t i = 0; i < n; ++i)
      if (dims[i] != dim)  // api.rs:122-133
        return fail(VI_ERR_INVALID_INPUT, "vector dimension mismatch at index %llu: expected %u, got %u",
                    (unsigned long long)i, dim, dims[i]);
  if (!values) return fail(VI_ERR_INVALID_INPUT, "null values");
  return vi::fit_and_save(&ix->impl, values, ext_ids, timestamps, n);
  });
}

vi_status vi_indexer_build_from_vector_file(vi_indexer *ix, const char *vector_file) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !vector_file) return fail(VI_ERR_INVALID_INPUT, "invalid vector_file path");
  std::vector<vi::VectorFileRecord> recs;
  if (vi::read_vectors_from_file(vector_file, &recs) != VI_OK)
    return fail(VI_ERR_OTHER, "read_vectors_from_file: %s", vi::last_error_ref().c_str());  // api.rs:156
  if (recs.empty()) return fail(VI_ERR_INVALID_INPUT, "no vectors in vector_file");          // api.rs:158-163
  const uint32_t dim = ix->impl.cfg.dimension;
  for (size_t i = 0; i < recs.size(); ++i)
    if (recs[i].values.size() != dim)
      return fail(VI_ERR_INVALID_INPUT, "vector dimension mismatch at index %zu: expected %u, got %zu", i, dim,
                  recs[i].values.size());
  std::vector<float> X(recs.size() * (size_t)dim);
  std::vector<uint64_t> eid(recs.size()), ts(recs.size());
  for (size_t i = 0; i < recs.size(); ++i) {
    std::memcpy(&X[i * dim], recs[i].values.data(), dim * sizeof(float));
    eid[i] = recs[i].id;
    ts[i] = recs[i].meta;  // VectorStore::new(vectors): third field is the timestamp (api.rs:181)
  }
  return vi::fit_and_save(&ix->impl, X.data(), eid.data(), ts.data(), recs.size());
  });
}

vi_status vi_indexer_add_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values, const uint64_t *timestamps,
                                 uint64_t n) {
  return vi::guarded([&]() -> vi_status {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (n == 0) return VI_OK;  // nothing changes: no file, no index, no filter
  if (!values) return fail(VI_ERR_INVALID_INPUT, "null values");
  const uint32_t dim = ix->impl.cfg.dimension;
  if (dim && n > ~0ull / 4 / dim) return fail(VI_ERR_INVALID_INPUT, "more than 2^32 - 2 vectors");
  // a record is stored as it is and searched for ever: a NaN would poison every distance of its list
  for (uint64_t i = 0; i < n * (uint64_t)dim; ++i)
    if (!std::isfinite(values[i]))
      return fail(VI_ERR_INVALID_INPUT, "non-finite value at flat index %llu", (unsigned long long)i);
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1)
    return fail(VI_ERR_INVALID_INPUT, "records are added through an unpartitioned handle (world_size <= 1); ranks reload from its files");
  if (ix->impl.dev->nlists == 0) return fail(VI_ERR_INVALID_INPUT, "the index has no list to add to");
  if (n > 0xFFFFFFFEull || ix->impl.dev->nvec_resident + n > 0xFFFFFFFEull)
    return fail(VI_ERR_INVALID_INPUT, "more than 2^32 - 2 vectors");
  return vi::add_records(&ix->impl, ext_ids, values, timestamps, n);
  });
}

// the refusals vi_indexer_retain and vi_indexer_remove_ids share, before any file or device change
static vi_status remove_common(const vi_indexer *ix) {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1)
    return fail(VI_ERR_INVALID_INPUT, "records are removed through an unpartitioned handle (world_size <= 1); ranks reload from its files");
  return VI_OK;
}

vi_status vi_indexer_retain(vi_indexer *ix, const vi_filter *keep, uint64_t *removed_out) {
  return vi::guarded([&]() -> vi_status {
  if (removed_out) *removed_out = 0;
  VI_TRY(remove_common(ix));
  if (!keep) return fail(VI_ERR_INVALID_INPUT, "null filter");
  if (keep->impl.owner_serial != ix->impl.dev->serial)
    return fail(VI_ERR_INVALID_INPUT, "the filter was made from another indexer (or before this one was rebuilt)");
  return vi::retain_records(&ix->impl, keep->impl, removed_out);
  });
}

vi_status vi_indexer_remove_ids(vi_indexer *ix, const uint64_t *ext_ids, uint64_t n, uint64_t *removed_out) {
  return vi::guarded([&]() -> vi_status {
  if (removed_out) *removed_out = 0;
  VI_TRY(remove_common(ix));
  if (n && !ext_ids) return fail(VI_ERR_INVALID_INPUT, "null id set with n = %llu", (unsigned long long)n);
  if (n == 0) return VI_OK;  // nothing changes: no file, no index, no filter
  vi::SlotFilter keep;       // the records a VI_IDS_DENY filter of the set admits
  VI_TRY(vi::slot_filter_ids(*ix->impl.dev, ext_ids, n, false, true, &keep));
  return vi::retain_records(&ix->impl, keep, removed_out);
  });
}

vi_status vi_shard_remove_from(const char *shards_dir, uint64_t shard_id, const uint64_t *ext_ids, uint64_t n,
                               uint64_t *removed_out) {
  return vi::guarded([&]() -> vi_status {
  if (removed_out) *removed_out = 0;
  if (!shards_dir) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (n && !ext_ids) return fail(VI_ERR_INVALID_INPUT, "null id set with n = %llu", (unsigned long long)n);
  return vi::shard_remove_from(shards_dir, shard_id, ext_ids, n, removed_out);
  });
}

vi_status vi_indexer_upsert_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values, const uint64_t *timestamps,
                                    uint64_t n, uint64_t *replaced_out) {
  return vi::guarded([&]() -> vi_status {
  if (replaced_out) *replaced_out = 0;
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (n == 0) return VI_OK;  // nothing changes: no file, no index, no filter
  if (!ext_ids) return fail(VI_ERR_INVALID_INPUT, "null id set with n = %llu", (unsigned long long)n);
  if (!values) return fail(VI_ERR_INVALID_INPUT, "null values");
  const uint32_t dim = ix->impl.cfg.dimension;
  if (n > 0xFFFFFFFEull || (dim && n > ~0ull / 4 / dim)) return fail(VI_ERR_INVALID_INPUT, "more than 2^32 - 2 vectors");
  for (uint64_t i = 0; i < n * (uint64_t)dim; ++i)
    if (!std::isfinite(values[i]))
      return fail(VI_ERR_INVALID_INPUT, "non-finite value at flat index %llu", (unsigned long long)i);
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1)
    return fail(VI_ERR_INVALID_INPUT, "records are upserted through an unpartitioned handle (world_size <= 1); ranks reload from its files");
  if (ix->impl.dev->nlists == 0) return fail(VI_ERR_INVALID_INPUT, "the index has no list to add to");
  return vi::upsert_records(&ix->impl, ext_ids, values, timestamps, n, replaced_out);
  });
}

vi_status vi_indexer_refine(vi_indexer *ix, uint64_t iters, uint64_t *moved_out) {
  return vi::guarded([&]() -> vi_status {
  if (moved_out) *moved_out = 0;
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1)
    return fail(VI_ERR_INVALID_INPUT, "an index is refined through an unpartitioned handle (world_size <= 1); ranks reload from its files");
  if (ix->impl.dev->nlists == 0 || ix->impl.dev->nvec_resident == 0)
    return fail(VI_ERR_INVALID_INPUT, "the index holds no record to refine by");
  if (iters == 0) return VI_OK;  // nothing changes: no file, no index, no filter
  return vi::refine_records(&ix->impl, iters, moved_out);
  });
}

void vi_rebalance_rule_init(vi_rebalance_rule *r) {
  if (!r) return;
  *r = vi_rebalance_rule{};
  r->iters = 1;
  r->split_rounds = 1;
  r->split_factor = 2.0;
  r->split_iters = 4;
}

vi_status vi_indexer_rebalance(vi_indexer *ix, const vi_rebalance_rule *rule, uint64_t *moved_out) {
  return vi::guarded([&]() -> vi_status {
  if (moved_out) *moved_out = 0;
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (!rule) return fail(VI_ERR_INVALID_INPUT, "null rule");
  if (rule->iters == 0) return fail(VI_ERR_INVALID_INPUT, "a rebalance runs at least one iteration");
  if (rule->split_rounds > rule->iters) return fail(VI_ERR_INVALID_INPUT, "split_rounds exceeds iters");
  if (!std::isfinite(rule->split_factor) || rule->split_factor < 1.0) return fail(VI_ERR_INVALID_INPUT, "split_factor must be finite and at least 1");
  if (rule->split_iters < 1 || rule->split_iters > 64) return fail(VI_ERR_INVALID_INPUT, "split_iters must lie in 1..64");
  if (rule->reserved0 != 0) return fail(VI_ERR_INVALID_INPUT, "reserved0 must be 0");
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1)
    return fail(VI_ERR_INVALID_INPUT, "an index is rebalanced through an unpartitioned handle (world_size <= 1); ranks reload from its files");
  if (ix->impl.dev->nlists == 0 || ix->impl.dev->nvec_resident == 0)
    return fail(VI_ERR_INVALID_INPUT, "the index holds no record to rebalance by");
  vi::SplitRule sr;
  sr.split_rounds = rule->split_rounds;
  sr.split_factor = rule->split_factor;
  sr.receiver_max_len = rule->receiver_max_len;
  sr.max_splits = rule->max_splits;
  sr.split_iters = rule->split_iters;
  return vi::refine_records(&ix->impl, rule->iters, moved_out, &sr);
  });
}

vi_status vi_indexer_last_rebalance_stats(const vi_indexer *ix, vi_rebalance_stats *out) {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = ix->impl.rebalance_stats;
  return VI_OK;
}

vi_status vi_indexer_last_refine_stats(const vi_indexer *ix, vi_refine_stats *out) {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = ix->impl.refine_stats;
  return VI_OK;
}

vi_status vi_indexer_list_stats(const vi_indexer *ix, vi_list_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = vi_list_stats{};
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  std::vector<uint32_t> len;
  VI_HIP(hipSetDevice(ix->impl.dev->device));
  VI_TRY(vi::read_list_lengths(*ix->impl.dev, &len));
  out->lists = len.size();
  if (len.empty()) return VI_OK;
  uint64_t total = 0;
  out->min_len = len[0];
  for (const uint32_t v : len) {
    out->empty_lists += v == 0;
    out->min_len = std::min<uint64_t>(out->min_len, v);
    out->max_len = std::max<uint64_t>(out->max_len, v);
    total += v;
  }
  out->mean_len = (double)total / (double)len.size();
  out->imbalance = vi::refine_imbalance(len.data(), len.size());
  return VI_OK;
  });
}

vi_status vi_shard_upsert_to(const char *shards_dir, uint64_t shard_id, uint64_t n, const uint64_t *centroid_ids,
                             const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs,
                             uint64_t *removed_out) {
  return vi::guarded([&]() -> vi_status {
  if (removed_out) *removed_out = 0;
  if (!shards_dir) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (n && (!centroid_ids || !ids || !ext_ids || !timestamps || !vecs)) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  return vi::shard_upsert_to(shards_dir, shard_id, n, centroid_ids, ids, ext_ids, timestamps, vecs, removed_out);
  });
}

// ---- reading records back (record_fetch.hip) ----
static vi_status get_records_common(const vi_indexer *ix, const uint64_t *ids, uint64_t n, bool on_device, uint32_t *count,
                                    float *values, uint64_t *timestamps, uint64_t *where) {
  return vi::guarded([&]() -> vi_status {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (n && !ids) return fail(VI_ERR_INVALID_INPUT, "null id set with n = %llu", (unsigned long long)n);
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (n > (1ull << 40)) return fail(VI_ERR_INVALID_INPUT, "id set of %llu ids is too large", (unsigned long long)n);
  if (n == 0) return VI_OK;  // nothing is read or written
  return vi::fetch_records_by_id(*ix->impl.dev, ids, n, on_device, count, values, timestamps, where);
  });
}

vi_status vi_indexer_get_records(const vi_indexer *ix, const uint64_t *ext_ids, uint64_t n, uint32_t *count_out,
                                 float *values_out, uint64_t *timestamps_out, uint64_t *where_out) {
  return get_records_common(ix, ext_ids, n, false, count_out, values_out, timestamps_out, where_out);
}

vi_status vi_indexer_get_records_device(const vi_indexer *ix, const uint64_t *ext_ids_dev, uint64_t n, uint32_t *count_dev,
                                        float *values_dev, uint64_t *timestamps_dev, uint64_t *where_dev) {
  return get_records_common(ix, ext_ids_dev, n, true, count_dev, values_dev, timestamps_dev, where_dev);
}

// records [first, first + count) of the list order exist: what every entry that takes such a range checks
static vi_status record_range_check(uint64_t first, uint64_t count, uint64_t nvec) {
  if (first > nvec || count > nvec - first)
    return fail(VI_ERR_INVALID_INPUT, "records [%llu, %llu + %llu) of %llu resident records", (unsigned long long)first,
                (unsigned long long)first, (unsigned long long)count, (unsigned long long)nvec);
  return VI_OK;
}

static vi_status export_records_common(const vi_indexer *ix, uint64_t first, uint64_t count, bool on_device, uint64_t *ext_ids,
                                       float *values, uint64_t *timestamps, uint64_t *where) {
  return vi::guarded([&]() -> vi_status {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  VI_TRY(record_range_check(first, count, ix->impl.dev->nvec_resident));
  if (count == 0) return VI_OK;
  return vi::export_records(*ix->impl.dev, first, count, on_device, ext_ids, values, timestamps, where);
  });
}

vi_status vi_indexer_export_records(const vi_indexer *ix, uint64_t first, uint64_t count, uint64_t *ext_ids_out,
                                    float *values_out, uint64_t *timestamps_out, uint64_t *where_out) {
  return export_records_common(ix, first, count, false, ext_ids_out, values_out, timestamps_out, where_out);
}

vi_status vi_indexer_export_records_device(const vi_indexer *ix, uint64_t first, uint64_t count, uint64_t *ext_ids_dev,
                                           float *values_dev, uint64_t *timestamps_dev, uint64_t *where_dev) {
  return export_records_common(ix, first, count, true, ext_ids_dev, values_dev, timestamps_dev, where_dev);
}

vi_status vi_indexer_last_fetch_stats(const vi_indexer *ix, vi_fetch_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out || !ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "no stats");
  ix->impl.dev->fetch.pool.locked([&] { *out = ix->impl.dev->fetch.last; });
  return VI_OK;
  });
}

static vi_status search_common(const vi_indexer *ix, uint64_t *k, uint64_t *n_probe) {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  const vi_config &c = ix->impl.cfg;
  if (*k > c.max_k) *k = c.max_k;                    // api.rs:189
  if (*n_probe > c.max_n_probe) *n_probe = c.max_n_probe;  // api.rs:190
  return VI_OK;
}

// the filter of a search entry: null (unfiltered), or one made from this handle's resident index
static vi_status filter_common(const vi_indexer *ix, const vi_filter *f, const vi::SlotFilter **out) {
  *out = nullptr;
  if (!f) return VI_OK;
  if (!ix->impl.dev || f->impl.owner_serial != ix->impl.dev->serial)
    return fail(VI_ERR_INVALID_INPUT, "the filter was made from another indexer (or before this one was rebuilt)");
  *out = &f->impl;
  return VI_OK;
}

vi_status vi_indexer_search_filtered(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq,
                                     uint32_t query_dim, uint64_t k, uint64_t n_probe, float *D, int64_t *I, float *V,
                                     uint64_t *counts, uint64_t *k_out) {
  return vi::guarded([&]() -> vi_status {
  VI_TRY(search_common(ix, &k, &n_probe));
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(filter_common(ix, f, &flt));
  if (k_out) *k_out = k;
  if (query_dim != ix->impl.cfg.dimension)  // api.rs:192-201
    return fail(VI_ERR_INVALID_INPUT, "query dimension mismatch: expected %u, got %u", ix->impl.cfg.dimension,
                query_dim);
  if (k == 0 || n_probe == 0)  // ivf_index.rs:197-202
    return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  if (nq == 0) return VI_OK;
  if (!queries || !D || !I) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  // NaN/Inf in a query makes partial_cmp().unwrap() panic in the reference (ivf_index.rs:215)
  for (uint64_t i = 0; i < nq * (uint64_t)query_dim; ++i)
    if (!std::isfinite(queries[i])) return fail(VI_ERR_PANIC, "non-finite query value at flat index %llu",
                                                (unsigned long long)i);
  vi::SearchIO io;
  io.queries = queries; io.nq = nq; io.k = k; io.n_probe = n_probe;
  io.D = D; io.I = I; io.V = V; io.counts = counts;
  io.filter = flt;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search(const vi_indexer *ix, const float *queries, uint64_t nq, uint32_t query_dim, uint64_t k,
                            uint64_t n_probe, float *D, int64_t *I, float *V, uint64_t *counts, uint64_t *k_out) {
  return vi_indexer_search_filtered(ix, nullptr, queries, nq, query_dim, k, n_probe, D, I, V, counts, k_out);
}

vi_status vi_indexer_search_filtered_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev, uint64_t nq,
                                            uint64_t k, uint64_t n_probe, float *D_dev, int64_t *I_dev, uint64_t *tie_dev) {
  return vi::guarded([&]() -> vi_status {
  VI_TRY(search_common(ix, &k, &n_probe));
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(filter_common(ix, f, &flt));
  if (k == 0 || n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  if (nq == 0) return VI_OK;
  if (!queries_dev || !D_dev || !I_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  vi::SearchIO io;
  io.queries = queries_dev; io.on_device = true; io.nq = nq; io.k = k; io.n_probe = n_probe;
  io.D = D_dev; io.I = I_dev; io.tie = tie_dev;
  io.filter = flt;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t k,
                                   uint64_t n_probe, float *D_dev, int64_t *I_dev, uint64_t *tie_dev) {
  return vi_indexer_search_filtered_device(ix, nullptr, queries_dev, nq, k, n_probe, D_dev, I_dev, tie_dev);
}

vi_status vi_indexer_probe_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t n_probe,
                                  uint32_t *probes_dev, uint32_t *order_dev, uint64_t *n_probe_eff) {
  return vi::guarded([&]() -> vi_status {
  uint64_t k = 1;
  VI_TRY(search_common(ix, &k, &n_probe));
  if (n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  const uint64_t p_eff = std::min<uint64_t>(n_probe, ix->impl.meta.k());
  if (n_probe_eff) *n_probe_eff = p_eff;
  if (nq == 0 || p_eff == 0) return VI_OK;
  if (!queries_dev || !probes_dev || !order_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  vi::SearchIO io;
  io.queries = queries_dev; io.on_device = true; io.nq = nq; io.k = 1; io.n_probe = n_probe;
  io.probes_out = probes_dev; io.order_out = order_dev;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search_probed_filtered_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev,
                                                   uint64_t nq, uint64_t k, uint64_t n_probe_eff, const uint32_t *probes_dev,
                                                   const uint32_t *order_dev, float *D_dev, int64_t *I_dev,
                                                   uint64_t *tie_dev) {
  return vi::guarded([&]() -> vi_status {
  uint64_t n_probe = n_probe_eff;
  VI_TRY(search_common(ix, &k, &n_probe));
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(filter_common(ix, f, &flt));
  if (k == 0 || n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  if (nq == 0) return VI_OK;
  if (!queries_dev || !D_dev || !I_dev || !probes_dev || !order_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  if (n_probe_eff != std::min<uint64_t>(n_probe, ix->impl.meta.k()))
    return fail(VI_ERR_INVALID_INPUT, "n_probe_eff does not match this index (use the value vi_indexer_probe_device returned)");
  vi::SearchIO io;
  io.queries = queries_dev; io.on_device = true; io.nq = nq; io.k = k; io.n_probe = n_probe;
  io.D = D_dev; io.I = I_dev; io.tie = tie_dev;
  io.probes_in = probes_dev; io.order_in = order_dev;
  io.filter = flt;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search_probed_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t k,
                                          uint64_t n_probe_eff, const uint32_t *probes_dev,
                                          const uint32_t *order_dev, float *D_dev, int64_t *I_dev,
                                          uint64_t *tie_dev) {
  return vi_indexer_search_probed_filtered_device(ix, nullptr, queries_dev, nq, k, n_probe_eff, probes_dev, order_dev, D_dev,
                                                  I_dev, tie_dev);
}

// ---- adaptive probing (probe_prune.hip) ----
// The checks the three entries share, all before any device work; on VI_OK *k and *n_probe are clamped, *flt is set and
// *pr carries the rule.
// query_dim: of the entry that takes one, else null.
static vi_status adaptive_common(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule, const uint32_t *query_dim,
                                 uint64_t *k, uint64_t *n_probe, const vi::SlotFilter **flt, vi::ProbePrune *pr) {
  vi::prune_reset_stats();  // (vi_prune_last_stats reads zeros after a call that failed or pruned nothing)
  VI_TRY(search_common(ix, k, n_probe));
  if (!rule) return fail(VI_ERR_INVALID_INPUT, "null probe rule");
  if (!vi::probe_ratio_legal(rule->ratio2)) return fail(VI_ERR_INVALID_INPUT, "ratio2 must be 0 (off) or finite and >= 1");
  if (*k == 0 || *n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  if (query_dim && *query_dim != ix->impl.cfg.dimension)
    return fail(VI_ERR_INVALID_INPUT, "query dimension mismatch: expected %u, got %u", ix->impl.cfg.dimension, *query_dim);
  if (rule->max_codes != 0 && (ix->impl.cfg.world_size > 1 || (ix->impl.dev && ix->impl.dev->stripe_world > 1)))
    return fail(VI_ERR_INVALID_INPUT, "max_codes needs the whole index on one handle: a partitioned handle knows the resident "
                "lengths of its lists only (the ratio and the per-query counts work on every rank)");
  VI_TRY(filter_common(ix, f, flt));
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  pr->min_probe = rule->min_probe; pr->ratio2 = rule->ratio2; pr->max_codes = rule->max_codes; pr->n_probe_q = rule->n_probe_q;
  return VI_OK;
}

vi_status vi_indexer_prune_probes_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t n_probe_eff,
                                         uint32_t *probes_dev, uint32_t *order_dev, const vi_probe_rule *rule,
                                         uint32_t *n_kept_dev) {
  return vi::guarded([&]() -> vi_status {
  uint64_t k = 1, n_probe = n_probe_eff;
  const vi::SlotFilter *flt = nullptr;
  vi::ProbePrune pr;
  VI_TRY(adaptive_common(ix, nullptr, rule, nullptr, &k, &n_probe, &flt, &pr));
  if (n_probe_eff != std::min<uint64_t>(n_probe, ix->impl.meta.k()))
    return fail(VI_ERR_INVALID_INPUT, "n_probe_eff does not match this index (use the value vi_indexer_probe_device returned)");
  if (nq == 0) return VI_OK;
  if (!queries_dev || !probes_dev || !order_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  pr.n_kept = n_kept_dev;
  return vi::device_index_prune_probes(*ix->impl.dev, queries_dev, nq, (uint32_t)n_probe_eff, probes_dev, order_dev, pr);
  });
}

vi_status vi_indexer_search_adaptive(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule, const float *queries,
                                     uint64_t nq, uint32_t query_dim, uint64_t k, uint64_t n_probe, float *D, int64_t *I,
                                     float *V, uint64_t *counts, uint32_t *n_probed, uint64_t *k_out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  vi::ProbePrune pr;
  VI_TRY(adaptive_common(ix, f, rule, &query_dim, &k, &n_probe, &flt, &pr));
  if (k_out) *k_out = k;
  if (nq == 0) return VI_OK;
  if (!queries || !D || !I) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  for (uint64_t i = 0; i < nq * (uint64_t)query_dim; ++i)  // (as vi_indexer_search_filtered)
    if (!std::isfinite(queries[i])) return fail(VI_ERR_PANIC, "non-finite query value at flat index %llu", (unsigned long long)i);
  pr.n_kept = n_probed;
  vi::SearchIO io;
  io.queries = queries; io.nq = nq; io.k = k; io.n_probe = n_probe;
  io.D = D; io.I = I; io.V = V; io.counts = counts;
  io.filter = flt; io.prune = &pr;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search_adaptive_device(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule,
                                            const float *queries_dev, uint64_t nq, uint64_t k, uint64_t n_probe,
                                            float *D_dev, int64_t *I_dev, uint64_t *tie_dev, uint32_t *n_probed_dev) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  vi::ProbePrune pr;
  VI_TRY(adaptive_common(ix, f, rule, nullptr, &k, &n_probe, &flt, &pr));
  if (nq == 0) return VI_OK;
  if (!queries_dev || !D_dev || !I_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  pr.n_kept = n_probed_dev;
  vi::SearchIO io;
  io.queries = queries_dev; io.on_device = true; io.nq = nq; io.k = k; io.n_probe = n_probe;
  io.D = D_dev; io.I = I_dev; io.tie = tie_dev;
  io.filter = flt; io.prune = &pr;
  return vi::device_index_search(*ix->impl.dev, io);
  });
}

vi_status vi_prune_last_stats(uint64_t *probes_in, uint64_t *probes_kept, float *ms_prune) {
  return vi::guarded([&]() -> vi_status {
  if (!probes_in && !probes_kept && !ms_prune) return fail(VI_ERR_INVALID_INPUT, "null pointer: no output asked for");
  const vi::PruneStats s = vi::prune_last_stats();
  if (probes_in) *probes_in = s.probes_in;
  if (probes_kept) *probes_kept = s.probes_kept;
  if (ms_prune) *ms_prune = s.ms_prune;
  return VI_OK;
  });
}

// ---- the entries whose queries are stored records (similar_search.hip, cluster_radius.hip) ----
// The checks they share, all before any device work; on VI_OK *n_probe is clamped and *flt is set.  radius2: 0 where the
// entry has none.  own: the entry's own argument error, or null; it is reported where the entry always reported it,
// behind the row checks.  advice: what the entry tells the caller of a partitioned handle to do instead.
static vi_status stored_record_common(const vi_indexer *ix, const vi_filter *f, uint64_t nq, bool null_ids, uint64_t *n_probe,
                                      float radius2, const char *own, const char *advice, const vi::SlotFilter **flt) {
  uint64_t k = 1;
  VI_TRY(search_common(ix, &k, n_probe));
  if (*n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "n_probe must be greater than 0");
  if (std::isnan(radius2)) return fail(VI_ERR_INVALID_INPUT, "radius2 is NaN");
  if (nq > (1ull << 40)) return fail(VI_ERR_INVALID_INPUT, "%llu rows are too many for one call", (unsigned long long)nq);
  if (nq && null_ids) return fail(VI_ERR_INVALID_INPUT, "null id array with nq = %llu", (unsigned long long)nq);
  if (own) return fail(VI_ERR_INVALID_INPUT, "%s", own);
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  if (ix->impl.cfg.world_size > 1 || ix->impl.dev->stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "%s", advice);
  return filter_common(ix, f, flt);
}

// search by stored record: the four entries; on VI_OK *k is clamped as well
static vi_status similar_common(const vi_indexer *ix, const vi_filter *f, uint64_t nq, bool null_ids, bool null_rows, uint64_t *k,
                                uint64_t *n_probe, const vi::SlotFilter **flt) {
  VI_TRY(search_common(ix, k, n_probe));  // (the clamps; the shared checks find them made)
  if (*k == 0 || *n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "k and n_probe must be greater than 0");
  return stored_record_common(
      ix, f, nq, null_ids, n_probe, 0.0f, nq && null_rows ? "null pointer: D and I are required" : nullptr,
      "search by stored record needs the whole index on one handle; on a partitioned handle call "
      "vi_indexer_get_records_device on every rank, take the record with the lowest `where`, and search its vector "
      "with vi_indexer_probe_device / vi_indexer_search_probed_device (the record itself is then not excluded)",
      flt);
}

static vi_status search_by_ids_common(const vi_indexer *ix, const vi_filter *f, const uint64_t *ids, uint64_t nq, uint64_t k,
                                      uint64_t n_probe, uint32_t exclude_self, bool on_device, float *D, int64_t *I, uint64_t *tie,
                                      float *V, uint64_t *counts, uint32_t *found, uint64_t *k_out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(similar_common(ix, f, nq, !ids, !D || !I, &k, &n_probe, &flt));
  if (nq == 0) return VI_OK;  // nothing is read or written
  if (k_out) *k_out = k;
  vi::SimilarIO io;
  io.rows.ids = ids; io.rows.on_device = on_device; io.rows.nq = nq; io.k = k; io.n_probe = n_probe; io.exclude_self = exclude_self != 0;
  io.filter = flt; io.D = D; io.I = I; io.tie = tie; io.V = V; io.counts = counts; io.found = found;
  return vi::device_index_search_similar(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq,
                                   uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, float *V,
                                   uint64_t *counts, uint32_t *found, uint64_t *k_out) {
  return search_by_ids_common(ix, f, ext_ids, nq, k, n_probe, exclude_self, false, D, I, nullptr, V, counts, found, k_out);
}

vi_status vi_indexer_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq,
                                          uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev,
                                          uint64_t *tie_dev, uint32_t *found_dev) {
  return search_by_ids_common(ix, f, ext_ids_dev, nq, k, n_probe, exclude_self, true, D_dev, I_dev, tie_dev, nullptr, nullptr,
                              found_dev, nullptr);
}

static vi_status knn_graph_common(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k,
                                  uint64_t n_probe, uint32_t exclude_self, bool on_device, float *D, int64_t *I, uint64_t *tie,
                                  uint64_t *counts, uint64_t *k_out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(similar_common(ix, f, count, false, !D || !I, &k, &n_probe, &flt));
  VI_TRY(record_range_check(first, count, ix->impl.dev->nvec_resident));
  if (count == 0) return VI_OK;  // nothing is read or written
  if (k_out) *k_out = k;
  vi::SimilarIO io;
  io.rows.first = first; io.rows.on_device = on_device; io.rows.nq = count; io.k = k; io.n_probe = n_probe; io.exclude_self = exclude_self != 0;
  io.filter = flt; io.D = D; io.I = I; io.tie = tie; io.counts = counts;
  return vi::device_index_search_similar(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_knn_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k,
                               uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, uint64_t *counts, uint64_t *k_out) {
  return knn_graph_common(ix, f, first, count, k, n_probe, exclude_self, false, D, I, nullptr, counts, k_out);
}

vi_status vi_indexer_knn_graph_device(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k,
                                      uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev, uint64_t *tie_dev) {
  return knn_graph_common(ix, f, first, count, k, n_probe, exclude_self, true, D_dev, I_dev, tie_dev, nullptr, nullptr);
}

vi_status vi_similar_last_times(float *ms_resolve, float *ms_search, float *ms_drop, uint64_t *drop_bytes, uint64_t *chunk_rows) {
  return vi::guarded([&]() -> vi_status {
  const vi::SimilarTimes t = vi::similar_last_times();
  if (ms_resolve) *ms_resolve = t.ms_resolve;
  if (ms_search) *ms_search = t.ms_search;
  if (ms_drop) *ms_drop = t.ms_drop;
  if (drop_bytes) *drop_bytes = t.drop_bytes;
  if (chunk_rows) *chunk_rows = t.chunk_rows;
  return VI_OK;
  });
}

vi_status vi_indexer_filter_timestamps(const vi_indexer *ix, uint64_t ts_min, uint64_t ts_max, vi_filter **out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (ts_min > ts_max) return fail(VI_ERR_INVALID_INPUT, "timestamp window: ts_min > ts_max");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  auto f = std::make_unique<vi_filter>();
  VI_TRY(vi::slot_filter_timestamps(*ix->impl.dev, ts_min, ts_max, &f->impl));
  *out = f.release();
  return VI_OK;
  });
}

static vi_status filter_ids_common(const vi_indexer *ix, const uint64_t *ids, uint64_t n, vi_id_mode mode, bool on_device,
                                   vi_filter **out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (n && !ids) return fail(VI_ERR_INVALID_INPUT, "null id set with n = %llu", (unsigned long long)n);
  if ((int)mode != VI_IDS_ALLOW && (int)mode != VI_IDS_DENY)
    return fail(VI_ERR_INVALID_INPUT, "id filter mode %d (VI_IDS_ALLOW = 0 or VI_IDS_DENY = 1)", (int)mode);
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  auto f = std::make_unique<vi_filter>();
  VI_TRY(vi::slot_filter_ids(*ix->impl.dev, ids, n, on_device, (int)mode == VI_IDS_DENY, &f->impl));
  *out = f.release();
  return VI_OK;
  });
}

vi_status vi_indexer_filter_ids(const vi_indexer *ix, const uint64_t *ids, uint64_t n, vi_id_mode mode, vi_filter **out) {
  return filter_ids_common(ix, ids, n, mode, false, out);
}

vi_status vi_indexer_filter_ids_device(const vi_indexer *ix, const uint64_t *ids_dev, uint64_t n, vi_id_mode mode,
                                       vi_filter **out) {
  return filter_ids_common(ix, ids_dev, n, mode, true, out);
}

vi_status vi_filter_intersect(const vi_indexer *ix, const vi_filter *a, const vi_filter *b, vi_filter **out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out || !a || !b) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  const vi::SlotFilter *fa = nullptr, *fb = nullptr;
  VI_TRY(filter_common(ix, a, &fa));
  VI_TRY(filter_common(ix, b, &fb));
  auto f = std::make_unique<vi_filter>();
  VI_TRY(vi::slot_filter_intersect(*ix->impl.dev, *fa, *fb, &f->impl));
  *out = f.release();
  return VI_OK;
  });
}

// Every check of a composed filter that does not need the resident arrays (those are slot_filter_compose's, which still
// come before any device work); then one launch.  With `reuse` the filter is written in place and *out = reuse.
vi_status vi_indexer_filter_compose(const vi_indexer *ix, vi_filter_join join, const vi_filter_term *terms, uint32_t n_terms,
                                    vi_filter *reuse, vi_filter **out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !terms || !out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if ((int)join != VI_JOIN_AND && (int)join != VI_JOIN_OR)
    return fail(VI_ERR_INVALID_INPUT, "filter join %d (VI_JOIN_AND = 0 or VI_JOIN_OR = 1)", (int)join);
  if (n_terms < 1 || n_terms > VI_FILTER_MAX_TERMS)
    return fail(VI_ERR_INVALID_INPUT, "%u terms (1 to %d)", n_terms, VI_FILTER_MAX_TERMS);
  if (!ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "the indexer holds no index (build or load it first)");
  const vi::SlotFilter *operands[VI_FILTER_MAX_TERMS] = {};
  for (uint32_t i = 0; i < n_terms; ++i) {
    const vi_filter_term &t = terms[i];
    if (t.negate > 1) return fail(VI_ERR_INVALID_INPUT, "term %u: negate %u (0 or 1)", i, t.negate);
    switch (t.kind) {
      case VI_TERM_TIMESTAMPS:
      case VI_TERM_ID_RANGE:
        if (t.lo > t.hi) return fail(VI_ERR_INVALID_INPUT, "term %u: lo > hi", i);
        break;
      case VI_TERM_IDS:
      case VI_TERM_IDS_DEVICE:
      case VI_TERM_MASK:
      case VI_TERM_MASK_DEVICE:
        if (t.n && !t.data) return fail(VI_ERR_INVALID_INPUT, "term %u: null data with n = %llu", i, (unsigned long long)t.n);
        break;
      case VI_TERM_FILTER:
        if (!t.filter) return fail(VI_ERR_INVALID_INPUT, "term %u: null filter", i);
        VI_TRY(filter_common(ix, t.filter, &operands[i]));
        if (t.filter == reuse)
          return fail(VI_ERR_INVALID_INPUT, "term %u: the filter to overwrite is an operand of the expression", i);
        break;
      default:
        return fail(VI_ERR_INVALID_INPUT, "term %u: kind %u (vi_term_kind: 0 to 6)", i, t.kind);
    }
  }
  const vi::SlotFilter *checked = nullptr;
  VI_TRY(filter_common(ix, reuse, &checked));
  std::unique_ptr<vi_filter> fresh;
  if (!reuse) fresh = std::make_unique<vi_filter>();
  vi_filter *f = reuse ? reuse : fresh.get();
  VI_TRY(vi::slot_filter_compose(*ix->impl.dev, (int)join == VI_JOIN_OR, terms, n_terms, operands, &f->impl));
  fresh.release();
  *out = f;
  return VI_OK;
  });
}

static vi_filter_term filter_term(const vi_filter *f, uint32_t negate) {
  vi_filter_term t{};
  t.kind = VI_TERM_FILTER; t.negate = negate; t.filter = f;
  return t;
}

vi_status vi_filter_union(const vi_indexer *ix, const vi_filter *a, const vi_filter *b, vi_filter **out) {
  const vi_filter_term t[2] = {filter_term(a, 0), filter_term(b, 0)};
  return vi_indexer_filter_compose(ix, VI_JOIN_OR, t, 2, nullptr, out);
}

vi_status vi_filter_complement(const vi_indexer *ix, const vi_filter *a, vi_filter **out) {
  const vi_filter_term t = filter_term(a, 1);
  return vi_indexer_filter_compose(ix, VI_JOIN_AND, &t, 1, nullptr, out);
}

vi_status vi_indexer_filter_id_range(const vi_indexer *ix, uint64_t id_min, uint64_t id_max, vi_filter **out) {
  vi_filter_term t{};
  t.kind = VI_TERM_ID_RANGE; t.lo = id_min; t.hi = id_max;
  return vi_indexer_filter_compose(ix, VI_JOIN_AND, &t, 1, nullptr, out);
}

static vi_status filter_mask_common(const vi_indexer *ix, const uint8_t *mask, uint64_t n, bool on_device, vi_filter **out) {
  vi_filter_term t{};
  t.kind = on_device ? VI_TERM_MASK_DEVICE : VI_TERM_MASK; t.data = mask; t.n = n;
  return vi_indexer_filter_compose(ix, VI_JOIN_AND, &t, 1, nullptr, out);
}

vi_status vi_indexer_filter_mask(const vi_indexer *ix, const uint8_t *mask, uint64_t n, vi_filter **out) {
  return filter_mask_common(ix, mask, n, false, out);
}

vi_status vi_indexer_filter_mask_device(const vi_indexer *ix, const uint8_t *mask_dev, uint64_t n, vi_filter **out) {
  return filter_mask_common(ix, mask_dev, n, true, out);
}

uint64_t vi_filter_num_allowed(const vi_filter *f) { return f ? f->impl.num_allowed : 0; }

void vi_filter_free(vi_filter *f) { delete f; }

// the checks the radius entries share; *done: nothing to search (an empty result was made)
static vi_status range_common(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq, float radius2,
                              uint64_t *n_probe, vi_range_result **out, const vi::SlotFilter **flt) {
  uint64_t k = 1;
  VI_TRY(search_common(ix, &k, n_probe));
  if (!out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = nullptr;
  VI_TRY(filter_common(ix, f, flt));
  if (*n_probe == 0) return fail(VI_ERR_INVALID_INPUT, "n_probe must be greater than 0");
  if (std::isnan(radius2)) return fail(VI_ERR_INVALID_INPUT, "radius2 is NaN");
  if (nq && !queries) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  if (!ix->impl.dev) return fail(VI_ERR_DEVICE, "index is not resident on a GPU (build or load it first)");
  return VI_OK;
}

// *out = the result run(&result) fills, or nothing: a failed call leaves no result
static vi_status range_run(vi_range_result **out, const std::function<vi_status(vi::RangeResult *)> &run) {
  auto r = std::make_unique<vi_range_result>();
  VI_TRY(run(&r->impl));
  *out = r.release();
  return VI_OK;
}

vi_status vi_indexer_range_search(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq, uint32_t query_dim,
                                  float radius2, uint64_t n_probe, vi_range_result **out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(range_common(ix, f, queries, nq, radius2, &n_probe, out, &flt));
  if (query_dim != ix->impl.cfg.dimension)
    return fail(VI_ERR_INVALID_INPUT, "query dimension mismatch: expected %u, got %u", ix->impl.cfg.dimension, query_dim);
  // NaN/Inf in a query makes partial_cmp().unwrap() panic in the reference (ivf_index.rs:215)
  for (uint64_t i = 0; i < nq * (uint64_t)query_dim; ++i)
    if (!std::isfinite(queries[i])) return fail(VI_ERR_PANIC, "non-finite query value at flat index %llu", (unsigned long long)i);
  vi::RangeIO io;
  io.queries = queries; io.nq = nq; io.n_probe = n_probe; io.radius2 = radius2; io.filter = flt;
  return range_run(out, [&](vi::RangeResult *r) { return vi::device_index_range_search(*ix->impl.dev, io, r); });
  });
}

vi_status vi_indexer_range_search_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev, uint64_t nq,
                                         float radius2, uint64_t n_probe, vi_range_result **out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(range_common(ix, f, queries_dev, nq, radius2, &n_probe, out, &flt));
  vi::RangeIO io;
  io.queries = queries_dev; io.on_device = true; io.nq = nq; io.n_probe = n_probe; io.radius2 = radius2; io.filter = flt;
  return range_run(out, [&](vi::RangeResult *r) { return vi::device_index_range_search(*ix->impl.dev, io, r); });
  });
}

// ---- radius search by stored record (similar_search.hip) ----
// The checks of the three entries, all before any device work; on VI_OK *out is NULL, *n_probe clamped, *flt set.
static vi_status range_similar_common(const vi_indexer *ix, const vi_filter *f, uint64_t nq, bool null_ids, float radius2,
                                      uint64_t *n_probe, vi_range_result **out, const vi::SlotFilter **flt) {
  if (!out) return fail(VI_ERR_INVALID_INPUT, "null pointer: out is required");
  *out = nullptr;
  return stored_record_common(
      ix, f, nq, null_ids, n_probe, radius2, nullptr,
      "radius search by stored record needs the whole index on one handle; on a partitioned handle call "
      "vi_indexer_get_records_device on every rank, take the record with the lowest `where`, search its vector "
      "with vi_indexer_range_search_device on every rank and merge with vi_range_merge_device (the record itself "
      "is then not excluded)",
      flt);
}

static vi_status range_by_ids_common(const vi_indexer *ix, const vi_filter *f, const uint64_t *ids, uint64_t nq, float radius2,
                                     uint64_t n_probe, uint32_t exclude_self, bool on_device, uint32_t *found,
                                     vi_range_result **out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(range_similar_common(ix, f, nq, !ids, radius2, &n_probe, out, &flt));
  vi::RangeSimilarIO io;
  io.rows.ids = ids; io.rows.on_device = on_device; io.rows.nq = nq; io.n_probe = n_probe; io.radius2 = radius2;
  io.exclude_self = exclude_self != 0; io.filter = flt; io.found = found;
  return range_run(out, [&](vi::RangeResult *r) { return vi::device_index_range_similar(*ix->impl.dev, io, r); });
  });
}

vi_status vi_indexer_range_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq,
                                         float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found,
                                         vi_range_result **out) {
  return range_by_ids_common(ix, f, ext_ids, nq, radius2, n_probe, exclude_self, false, found, out);
}

vi_status vi_indexer_range_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq,
                                                float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found_dev,
                                                vi_range_result **out) {
  return range_by_ids_common(ix, f, ext_ids_dev, nq, radius2, n_probe, exclude_self, true, found_dev, out);
}

vi_status vi_indexer_radius_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, float radius2,
                                  uint64_t n_probe, uint32_t exclude_self, vi_range_result **out) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(range_similar_common(ix, f, count, false, radius2, &n_probe, out, &flt));
  VI_TRY(record_range_check(first, count, ix->impl.dev->nvec_resident));
  vi::RangeSimilarIO io;
  io.rows.first = first; io.rows.nq = count; io.n_probe = n_probe; io.radius2 = radius2; io.exclude_self = exclude_self != 0;
  io.filter = flt;
  return range_run(out, [&](vi::RangeResult *r) { return vi::device_index_range_similar(*ix->impl.dev, io, r); });
  });
}

// ---- clustering the stored records by radius (cluster_radius.hip) ----
static vi_status cluster_radius_common(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe, uint32_t min_pts,
                                       bool on_device, int64_t *labels, uint32_t *degree, uint64_t *n_clusters) {
  return vi::guarded([&]() -> vi_status {
  const vi::SlotFilter *flt = nullptr;
  VI_TRY(stored_record_common(
      ix, f, 0, false, &n_probe, radius2,
      !labels && !degree && !n_clusters ? "null pointer: one of labels, degree and n_clusters_out is required" : nullptr,
      "clustering by radius needs the whole index on one handle: a partitioned handle (world_size > 1) holds "
      "only its part of every neighbourhood",
      &flt));
  vi::ClusterIO io;
  io.on_device = on_device; io.n_probe = n_probe; io.radius2 = radius2; io.min_pts = min_pts; io.filter = flt;
  io.labels = labels; io.degree = degree; io.n_clusters = n_clusters;
  return vi::device_index_cluster_radius(*ix->impl.dev, io);
  });
}

vi_status vi_indexer_cluster_radius(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe,
                                    uint32_t min_pts, int64_t *labels_out, uint32_t *degree_out, uint64_t *n_clusters_out) {
  return cluster_radius_common(ix, f, radius2, n_probe, min_pts, false, labels_out, degree_out, n_clusters_out);
}

vi_status vi_indexer_cluster_radius_device(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe,
                                           uint32_t min_pts, int64_t *labels_dev, uint32_t *degree_dev, uint64_t *n_clusters_out) {
  return cluster_radius_common(ix, f, radius2, n_probe, min_pts, true, labels_dev, degree_dev, n_clusters_out);
}

vi_status vi_cluster_last_stats(vi_cluster_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = vi::cluster_last_stats();
  return VI_OK;
  });
}

uint64_t vi_range_result_total(const vi_range_result *r) { return r ? r->impl.total : 0; }

vi_status vi_range_result_copy(const vi_range_result *r, uint64_t *lims, float *D, int64_t *I, float *V) {
  return vi::guarded([&]() -> vi_status {
  if (!r) return fail(VI_ERR_INVALID_INPUT, "null range result");
  return vi::range_result_copy(r->impl, lims, D, I, V);
  });
}

vi_status vi_range_result_device(const vi_range_result *r, const uint64_t **lims_dev, const float **D_dev, const int64_t **I_dev,
                                 const uint64_t **tie_dev) {
  return vi::guarded([&]() -> vi_status {
  if (!r) return fail(VI_ERR_INVALID_INPUT, "null range result");
  if (lims_dev) *lims_dev = r->impl.lims.p;
  if (D_dev) *D_dev = r->impl.D.p;
  if (I_dev) *I_dev = r->impl.I.p;
  if (tie_dev) *tie_dev = r->impl.tie.p;
  return VI_OK;
  });
}

vi_status vi_range_result_copy_device(const vi_range_result *r, uint64_t *lims_dev, float *D_dev, int64_t *I_dev,
                                      uint64_t *tie_dev) {
  return vi::guarded([&]() -> vi_status {
  if (!r) return fail(VI_ERR_INVALID_INPUT, "null range result");
  const vi::RangeResult &x = r->impl;
  VI_HIP(hipSetDevice(x.device));
  if (lims_dev) VI_HIP(hipMemcpyAsync(lims_dev, x.lims.p, (x.nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr));
  if (D_dev && x.total) VI_HIP(hipMemcpyAsync(D_dev, x.D.p, x.total * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
  if (I_dev && x.total) VI_HIP(hipMemcpyAsync(I_dev, x.I.p, x.total * sizeof(int64_t), hipMemcpyDeviceToDevice, nullptr));
  if (tie_dev && x.total) VI_HIP(hipMemcpyAsync(tie_dev, x.tie.p, x.total * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr));
  VI_HIP(hipStreamSynchronize(nullptr));
  return VI_OK;
  });
}

void vi_range_result_free(vi_range_result *r) { delete r; }

vi_status vi_range_merge_device(int32_t device, uint64_t nq, uint32_t parts, const uint64_t *const *lims_dev, const float *const *D_dev,
                                const int64_t *const *I_dev, const uint64_t *const *tie_dev, vi_range_result **out) {
  return vi::guarded([&]() -> vi_status {
  if (!out) return fail(VI_ERR_INVALID_INPUT, "null pointer");
  *out = nullptr;
  if (!lims_dev || !D_dev || !I_dev || !tie_dev) return fail(VI_ERR_INVALID_INPUT, "null pointer array");
  if (parts == 0 || parts > vi::kRangeMergeMaxParts) return fail(VI_ERR_INVALID_INPUT, "parts must be 1..64, got %u", parts);
  for (uint32_t p = 0; p < parts; ++p) {
    if (!lims_dev[p]) return fail(VI_ERR_INVALID_INPUT, "part %u: null lims pointer", p);
    // (a part without entries still has buffers: every vi_range_result does)
    if (!D_dev[p] || !I_dev[p] || !tie_dev[p]) return fail(VI_ERR_INVALID_INPUT, "part %u: null D / I / tie pointer", p);
  }
  auto r = std::make_unique<vi_range_result>();
  VI_TRY(vi::range_merge_device(device, nq, parts, lims_dev, D_dev, I_dev, tie_dev, &r->impl));  // (all or nothing)
  *out = r.release();
  return VI_OK;
  });
}

vi_status vi_range_merge_last_times(float *ms_lims, float *ms_alloc, float *ms_place) {
  return vi::guarded([&]() -> vi_status {
  const vi::RangeMergeTimes t = vi::range_merge_last_times();
  if (ms_lims) *ms_lims = t.ms_lims;
  if (ms_alloc) *ms_alloc = t.ms_alloc;
  if (ms_place) *ms_place = t.ms_place;
  return VI_OK;
  });
}

vi_status vi_merge_partials_device(int32_t device, uint64_t nq, uint64_t k, uint32_t parts, const float *D_parts,
                                   const int64_t *I_parts, const uint64_t *tie_parts, float *D_out, int64_t *I_out) {
  return vi::guarded([&]() -> vi_status {
  return vi::merge_partials_device(device, nq, k, parts, D_parts, I_parts, tie_parts, D_out, I_out);
  });
}

vi_status vi_merge_partials_packed_device(int32_t device, uint64_t nq, uint64_t k, uint32_t parts, const void *packed_dev,
                                          float *D_out, int64_t *I_out) {
  return vi::guarded([&]() -> vi_status {
  return vi::merge_partials_packed_device(device, nq, k, parts, packed_dev, D_out, I_out);
  });
}

uint64_t vi_packed_result_bytes(uint64_t nq, uint64_t k) { return (nq * k * 4 + 7) / 8 * 8 + 2 * nq * k * 8; }

uint32_t vi_indexer_dimension(const vi_indexer *ix) { return ix ? ix->impl.meta.dimension : 0; }
uint64_t vi_indexer_num_centroids(const vi_indexer *ix) { return ix ? ix->impl.meta.k() : 0; }
uint64_t vi_indexer_num_vectors(const vi_indexer *ix) { return ix && ix->impl.dev ? ix->impl.dev->nvec_resident : 0; }
uint64_t vi_indexer_num_shards(const vi_indexer *ix) { return ix && ix->impl.dev ? ix->impl.dev->nshards : 0; }

vi_status vi_indexer_centroids(const vi_indexer *ix, float *centroids_out, uint64_t *c2s_out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix) return fail(VI_ERR_INVALID_INPUT, "null indexer");
  const vi::IndexMeta &m = ix->impl.meta;
  if (centroids_out && !m.centroids.empty()) std::memcpy(centroids_out, m.centroids.data(), m.centroids.size() * 4);
  if (c2s_out && !m.c2s.empty()) std::memcpy(c2s_out, m.c2s.data(), m.c2s.size() * 8);
  return VI_OK;
  });
}

void vi_indexer_free(vi_indexer *ix) { delete ix; }

vi_status vi_indexer_last_stats(const vi_indexer *ix, vi_search_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out || !ix->impl.dev) return fail(VI_ERR_INVALID_INPUT, "no stats");
  ix->impl.dev->search_contexts.locked([&] { *out = ix->impl.dev->last_stats; });
  return VI_OK;
  });
}

vi_status vi_indexer_last_build_stats(const vi_indexer *ix, vi_build_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "no stats");
  *out = ix->impl.build_stats;
  return VI_OK;
  });
}

vi_status vi_indexer_last_add_stats(const vi_indexer *ix, vi_add_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "no stats");
  *out = ix->impl.add_stats;
  return VI_OK;
  });
}

vi_status vi_indexer_last_remove_stats(const vi_indexer *ix, vi_remove_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "no stats");
  *out = ix->impl.remove_stats;
  return VI_OK;
  });
}

vi_status vi_indexer_last_upsert_stats(const vi_indexer *ix, vi_upsert_stats *out) {
  return vi::guarded([&]() -> vi_status {
  if (!ix || !out) return fail(VI_ERR_INVALID_INPUT, "no stats");
  *out = ix->impl.upsert_stats;
  return VI_OK;
  });
}

void vi_indexer_enable_timing(vi_indexer *ix, int enable) {
  if (ix && ix->impl.dev) ix->impl.dev->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
}

}  // extern "C"
