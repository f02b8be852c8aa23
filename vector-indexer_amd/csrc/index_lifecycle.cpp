// index_lifecycle.cpp — the build of an index and the rewrites of a built one, between the argument checks of api.cpp
// and the device routes of device_index.hpp.
//
// A rewrite (add, retain / remove, upsert: update_records; refine: refine_records) runs in one order of events: a plan,
// the files under temporary names (ShardRewriteSet, shards.hpp) and the new resident index beside the old one — an update
// writes its files first, from the old files and the caller's rows, a refine after the index, from it — then the renames,
// then the swap.  Everything before the renames can fail without a trace: the temporary files are removed, the handle
// keeps its index.
#include <sys/time.h>

#include <cmath>
#include <cstring>
#include <map>

#include "index_lifecycle.hpp"
#include "kmeans.hpp"
#include "list_layout.hpp"
#include "slot_filter.hpp"

namespace vi {

static uint64_t unix_timestamp_secs() {  // src/utils.rs:109-114
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return (uint64_t)tv.tv_sec;
}

// the timestamp of a record that brings none (vector_store.rs:36-40): the handle's fixed clock, or the clock
static uint64_t now_secs(const Indexer &ix) { return ix.cfg.now_secs ? ix.cfg.now_secs : unix_timestamp_secs(); }

vi_status attach_device(Indexer *ix) {
  auto dev = std::make_unique<DeviceIndex>();
  VI_TRY(device_index_load(ix->meta, ix->shards_dir, ix->cfg.device, ix->cfg.rank, ix->cfg.world_size, ix->cfg.placement,
                           dev.get()));
  ix->dev = std::move(dev);
  return VI_OK;
}

// IvfIndex::fit_with_paths (src/ivf_index.rs:58-177) + save_to (:274-294).  The points go to the GPU once and stay:
// k-means, the grouping of ids by list, the blocks of the resident index and the records of the shard files all come
// from that one device copy (list_build.hip, shard_export.hip); only the shard images travel back, to be written.
vi_status fit_and_save(Indexer *ix, const float *X, const uint64_t *ext_ids, const uint64_t *timestamps, uint64_t n) {
  const uint32_t dim = ix->cfg.dimension;
  const uint64_t seed = ix->cfg.seed ? ix->cfg.seed : 42;  // api.rs:143
  const uint64_t k = ix->cfg.nlist_override ? ix->cfg.nlist_override : vi_calculate_num_clusters(n);
  const uint64_t max_iters = vi_calculate_max_iterations(n);
  const uint64_t now = now_secs(*ix);
  vi_build_stats &bs = ix->build_stats;
  bs = vi_build_stats{};
  bs.n = n; bs.nlist = k;
  const double t0 = now_ms();
  if (n > 0xFFFFFFFEull) return fail(VI_ERR_INVALID_INPUT, "more than 2^32 - 2 vectors");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VI_ERR_DEVICE, "no HIP device visible: libvi_amd never falls back to the CPU");
  if (ix->cfg.device < 0 || ix->cfg.device >= ndev) return fail(VI_ERR_DEVICE, "device %d out of range (%d visible)", ix->cfg.device, ndev);
  VI_HIP(hipSetDevice(ix->cfg.device));
  hipStream_t st = nullptr;
  VI_HIP(hipStreamCreateWithFlags(&st, hipStreamDefault));
  struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } guard{st};
  DevBuf<float> Xd, Cd;
  DevBuf<uint32_t> lab, order;
  DevBuf<uint64_t> ext_dev, ts_dev;
  VI_TRY(Xd.reserve(n * dim));
  VI_HIP(hipMemcpyAsync(Xd.p, X, n * dim * sizeof(float), hipMemcpyHostToDevice, st));
  if (ext_ids) { VI_TRY(ext_dev.reserve(n)); VI_HIP(hipMemcpyAsync(ext_dev.p, ext_ids, n * 8, hipMemcpyHostToDevice, st)); }
  if (timestamps) { VI_TRY(ts_dev.reserve(n)); VI_HIP(hipMemcpyAsync(ts_dev.p, timestamps, n * 8, hipMemcpyHostToDevice, st)); }
  VI_HIP(hipStreamSynchronize(st));
  const double t1 = now_ms();
  bs.ms_upload = (float)(t1 - t0);
  VI_TRY(Cd.reserve(k * dim));
  VI_TRY(lab.reserve(n));
  if (kmeans_mini_batch_device(ix->cfg.device, Xd.p, n, dim, k, max_iters, -1.0f, seed, (vi_assign_mode)ix->cfg.assign_mode,
                               Cd.p, lab.p, nullptr) != VI_OK)
    return fail(VI_ERR_PANIC, "Failed to run KMeans: %s", last_error_ref().c_str());  // .expect (ivf_index.rs:71)
  std::vector<float> C(k * dim);
  VI_HIP(hipMemcpy(C.data(), Cd.p, k * dim * sizeof(float), hipMemcpyDeviceToHost));
  const double t2 = now_ms();
  bs.ms_kmeans = (float)(t2 - t1);
  // IVF lists in ascending internal id (:94-101): ids grouped by label on the device
  std::vector<uint64_t> off;
  DevBuf<uint32_t> seg_dev;
  VI_TRY(group_ids_by_label_device(lab.p, n, k, order, seg_dev, &off, st));
  const double t3 = now_ms();
  bs.ms_group = (float)(t3 - t2);
  // super-centroids => shard of every list (:104-109)
  const uint64_t num_shards = (uint64_t)std::ceil(std::sqrt((float)k));
  const uint64_t super_seed = seed * 31ULL + 7ULL;
  std::vector<float> SC(num_shards * dim);
  std::vector<uint64_t> slab(k);
  KMeansOptions opt;
  opt.device = ix->cfg.device;
  opt.mode = (vi_assign_mode)ix->cfg.assign_mode;
  if (kmeans_mini_batch(C.data(), k, dim, num_shards, 100, -1.0f, super_seed, opt, SC.data(), slab.data(), nullptr) !=
      VI_OK)
    return fail(VI_ERR_PANIC, "Failed to run kmeans: %s", last_error_ref().c_str());
  const double t4 = now_ms();
  bs.ms_super = (float)(t4 - t3);
  // drop empty lists and renumber (:123-164)
  std::vector<uint64_t> newid(k, ~0ull);
  uint64_t kk = 0;
  for (uint64_t c = 0; c < k; ++c)
    if (off[c + 1] > off[c]) newid[c] = kk++;
  ix->meta.dimension = dim;
  ix->meta.centroids.assign(kk * dim, 0.0f);
  ix->meta.c2s.assign(kk, 0);
  std::vector<uint64_t> src_off(kk);
  std::vector<uint32_t> len(kk), lshard(kk);
  std::vector<std::vector<uint32_t>> of_shard(num_shards);  // kept lists of every shard, ascending
  for (uint64_t c = 0; c < k; ++c)
    if (newid[c] != ~0ull) {
      const uint64_t l = newid[c];
      std::memcpy(&ix->meta.centroids[l * dim], &C[c * dim], dim * sizeof(float));
      ix->meta.c2s[l] = slab[c];
      src_off[l] = off[c];
      len[l] = (uint32_t)(off[c + 1] - off[c]);
      lshard[l] = (uint32_t)slab[c];
      of_shard[slab[c]].push_back((uint32_t)l);
    }
  // every shard is written, also the ones that received no list (:118-120,166-171)
  {
    ShardExportWs ws;
    std::vector<uint64_t> cids, soff;
    std::vector<uint32_t> slen;
    std::vector<float> cvec;
    for (uint64_t s = 0; s < num_shards; ++s) {
      cids.clear(); soff.clear(); slen.clear(); cvec.clear();
      for (uint32_t l : of_shard[s]) {
        cids.push_back(l);
        soff.push_back(src_off[l]);
        slen.push_back(len[l]);
        cvec.insert(cvec.end(), &ix->meta.centroids[(uint64_t)l * dim], &ix->meta.centroids[(uint64_t)l * dim] + dim);
        bs.shard_bytes += (uint64_t)len[l] * record_stride(dim);
      }
      // a failed shard write is only reported, never fatal (ivf_index.rs:168-170)
      if (shard_export_device(ix->shards_dir, s, dim, cids, cvec.data(), soff, slen, Xd.p, order.p,
                              ext_ids ? ext_dev.p : nullptr, timestamps ? ts_dev.p : nullptr, now, ws, st) != VI_OK)
        fprintf(stderr, "Failed to write shard %llu to disk: %s\n", (unsigned long long)s, last_error_ref().c_str());
    }
  }
  VI_TRY(index_meta_save(ix->meta, ix->index_dir));
  const double t5 = now_ms();
  bs.ms_export = (float)(t5 - t4);
  // the resident index: straight from the device copy (a rank of a multi-GPU run keeps only its stripes: from the files)
  vi_status rc;
  if (ix->cfg.world_size > 1) {
    rc = attach_device(ix);
  } else {
    auto dev = std::make_unique<DeviceIndex>();
    rc = device_index_from_order(ix->cfg.device, dim, ix->meta.centroids.data(), kk, Xd.p, order.p, src_off, len, lshard,
                                 ext_ids ? ext_dev.p : nullptr, timestamps ? ts_dev.p : nullptr, now, dev.get());
    if (rc == VI_OK) ix->dev = std::move(dev);
  }
  const double t6 = now_ms();
  bs.ms_index = (float)(t6 - t5);
  bs.ms_total = (float)(t6 - t0);
  bs.lists = kk;
  bs.shards = num_shards;
  return rc;
}

vi_status read_list_lengths(const DeviceIndex &ix, std::vector<uint32_t> *len) {
  len->resize(ix.nlists);
  if (ix.nlists) VI_HIP(hipMemcpy(len->data(), ix.list_len.p, ix.nlists * 4, hipMemcpyDeviceToHost));
  return VI_OK;
}

// ---- what update_records and refine_records share ----

// touched lists of every touched shard, ascending; touched(l) is asked once per list, in list order
typedef std::map<uint64_t, std::vector<uint32_t>> ListsOfShard;
template <typename F>
static ListsOfShard touched_lists_by_shard(const IndexMeta &meta, uint64_t nlists, F touched) {
  ListsOfShard lists_of_shard;
  for (uint64_t l = 0; l < nlists; ++l)
    if (touched(l)) lists_of_shard[meta.c2s[l]].push_back((uint32_t)l);
  return lists_of_shard;
}

// Every touched shard once: its file must hold every touched list at its resident length old_len[l] (else InvalidData);
// write(s, f, lists, views, &bytes) then writes files.temporary(s) — views[i]: where f has lists[i] — and it is registered.
template <typename W>
static vi_status rewrite_shards(ShardRewriteSet &files, uint32_t dim, const ListsOfShard &lists_of_shard,
                                const std::vector<uint32_t> &old_len, W write) {
  std::vector<const ShardListView *> views;
  for (const auto &kv : lists_of_shard) {
    const uint64_t s = kv.first;
    ShardFile f;
    VI_TRY(files.open(s, dim, &f));
    views.clear();
    for (const uint32_t l : kv.second) {
      const ShardListView *lv;
      VI_TRY(files.find(f, s, l, old_len[l], &lv));
      views.push_back(lv);
    }
    uint64_t bytes = 0;
    VI_TRY(write(s, f, kv.second, views, &bytes));
    files.add(s, bytes);
  }
  return VI_OK;
}

// the renames in the order registered, then the swap: the handle holds the new index only once its files are in place
static vi_status commit_and_swap(Indexer *ix, ShardRewriteSet &files, std::unique_ptr<DeviceIndex> dev) {
  VI_TRY(files.commit());
  ix->dev = std::move(dev);
  return VI_OK;
}

// ---- updates of a built index: add_records, retain_records and upsert_records, all through update_records ----
// What goes is a keep filter of ix->dev, what joins is a set of uploaded rows; either may be absent.

// the rows an add or an upsert brings: the caller's host arrays, the stored timestamps, the device copies and their stream
struct NewRows {
  const float *X = nullptr;
  const uint64_t *ext = nullptr;
  uint64_t n = 0;
  std::vector<uint64_t> ts;
  hipStream_t st = nullptr;
  DevBuf<float> Xd;
  DevBuf<uint64_t> ext_dev, ts_dev;
  ~NewRows() { if (st) (void)hipStreamDestroy(st); }
};

static vi_status upload_rows(const Indexer *ix, const uint64_t *ext, const float *X, const uint64_t *timestamps, uint64_t n, NewRows *r) {
  const uint32_t dim = ix->cfg.dimension;
  const uint64_t now = now_secs(*ix);
  r->X = X; r->ext = ext; r->n = n;
  r->ts.resize(n);
  for (uint64_t i = 0; i < n; ++i) r->ts[i] = timestamps && timestamps[i] ? timestamps[i] : now;
  VI_HIP(hipSetDevice(ix->dev->device));
  VI_HIP(hipStreamCreateWithFlags(&r->st, hipStreamDefault));
  VI_TRY(r->Xd.reserve(n * dim));
  VI_TRY(r->ext_dev.reserve(n));
  VI_TRY(r->ts_dev.reserve(n));
  VI_HIP(hipMemcpyAsync(r->Xd.p, X, n * dim * sizeof(float), hipMemcpyHostToDevice, r->st));
  VI_HIP(hipMemcpyAsync(r->ext_dev.p, ext, n * 8, hipMemcpyHostToDevice, r->st));
  VI_HIP(hipMemcpyAsync(r->ts_dev.p, r->ts.data(), n * 8, hipMemcpyHostToDevice, r->st));
  VI_HIP(hipStreamSynchronize(r->st));
  return VI_OK;
}

struct UpdateStats {
  uint64_t lists_touched = 0, lists_emptied = 0, shards_rewritten = 0, bytes_written = 0, kernel_bytes = 0;
  float ms_plan = 0, ms_files = 0, ms_index = 0, ms_kernel = 0, ms_total = 0;
};
// the fields vi_add_stats, vi_remove_stats and vi_upsert_stats have in common
template <typename S>
static S common_stats(const UpdateStats &us) {
  S s{};
  s.lists_touched = us.lists_touched; s.shards_rewritten = us.shards_rewritten; s.bytes_written = us.bytes_written;
  s.kernel_bytes = us.kernel_bytes;
  s.ms_files = us.ms_files; s.ms_index = us.ms_index; s.ms_kernel = us.ms_kernel; s.ms_total = us.ms_total;
  return s;
}

// keep (or null: nothing goes): a filter of ix->dev, its allow words say which positions of which lists stay (position p
// of list l: bit p % 64 of word first[l] + p / 64).  rows (or null: nothing joins): the label of every row, from the old
// index, says where it goes; row r gets internal id (records kept) + r.  t0: when the call began.  On success the handle
// holds the new index and *us the figures; on failure nothing has changed.
static vi_status update_records(Indexer *ix, const SlotFilter *keep, const NewRows *rows, double t0, UpdateStats *us) {
  const DeviceIndex &old = *ix->dev;
  const uint32_t dim = ix->cfg.dimension;
  const uint64_t nlists = old.nlists, n = rows ? rows->n : 0, n_kept = keep ? keep->num_allowed : old.nvec_resident;
  VI_HIP(hipSetDevice(old.device));
  // ---- plan ----
  DevBuf<uint32_t> lab, order, seg_dev;
  std::vector<uint64_t> seg(nlists + 1, 0);
  std::vector<uint32_t> h_order(n), h_first, h_len;
  std::vector<uint64_t> h_allow;
  if (rows) {
    VI_TRY(lab.reserve(n));
    VI_TRY(device_index_label_rows(old, rows->Xd.p, n, lab.p));
    VI_TRY(group_ids_by_label_device(lab.p, n, nlists, order, seg_dev, &seg, rows->st));
    if (seg.size() != nlists + 1 || seg[nlists] != n) return fail(VI_ERR_OTHER, "update: a record was assigned to no list");
    VI_HIP(hipMemcpy(h_order.data(), order.p, n * 4, hipMemcpyDeviceToHost));
  }
  VI_TRY(read_list_lengths(old, &h_len));
  std::vector<uint64_t> kept(h_len.begin(), h_len.end()), full_len(nlists);
  if (keep) {
    h_allow.resize(old.lists.nblocks);
    h_first.resize(nlists);
    if (old.lists.nblocks) VI_HIP(hipMemcpy(h_allow.data(), keep->allow.p, old.lists.nblocks * 8, hipMemcpyDeviceToHost));
    VI_HIP(hipMemcpy(h_first.data(), old.list_first_block.p, nlists * 4, hipMemcpyDeviceToHost));
    for (uint64_t l = 0; l < nlists; ++l) {
      kept[l] = 0;
      for (uint32_t b = 0; b < (h_len[l] + 63u) / 64u; ++b) kept[l] += (uint64_t)__builtin_popcountll(h_allow[h_first[l] + b]);
    }
  }
  for (uint64_t l = 0; l < nlists; ++l) full_len[l] = kept[l] + (seg[l + 1] - seg[l]);
  {  // the slot limit of the new layout, before anything is written
    ListLayout lay;
    if (plan_list_layout(full_len.data(), nlists, 1, 0, &lay) != LayoutError::none)
      return fail(VI_ERR_INVALID_INPUT, "index too large for 32-bit slot ids");
  }
  const auto lists_of_shard = touched_lists_by_shard(ix->meta, nlists, [&](uint64_t l) {
    if (kept[l] == h_len[l] && seg[l + 1] == seg[l]) return false;  // lost nothing, received nothing
    ++us->lists_touched;
    us->lists_emptied += h_len[l] != 0 && full_len[l] == 0;
    return true;
  });
  const double t1 = now_ms();
  us->ms_plan = (float)(t1 - t0);

  // ---- files: from the old file's records and the caller's rows ----
  ShardRewriteSet files(ix->shards_dir);
  {
    std::vector<uint64_t> s_cid, s_id, s_ext, s_ts;
    std::vector<float> s_vec;
    std::vector<const uint64_t *> keep_of;  // (left empty without a filter: nothing goes)
    VI_TRY(rewrite_shards(files, dim, lists_of_shard, h_len,
                          [&](uint64_t s, const ShardFile &f, const std::vector<uint32_t> &lists, const std::vector<const ShardListView *> &views,
                              uint64_t *bytes) -> vi_status {
      if (keep) keep_of.assign(f.num_lists(), nullptr);
      s_cid.clear(); s_id.clear(); s_ext.clear(); s_ts.clear(); s_vec.clear();
      for (size_t i = 0; i < lists.size(); ++i) {
        const uint32_t l = lists[i];
        if (kept[l] != h_len[l]) keep_of[views[i] - &f.list(0)] = h_allow.data() + h_first[l];
        for (uint64_t e = seg[l]; e < seg[l + 1]; ++e) {
          const uint32_t r = h_order[e];
          s_cid.push_back(l); s_id.push_back(n_kept + r); s_ext.push_back(rows->ext[r]); s_ts.push_back(rows->ts[r]);
          s_vec.insert(s_vec.end(), rows->X + (uint64_t)r * dim, rows->X + (uint64_t)r * dim + dim);
        }
      }
      return shard_update_write(f, s, keep_of, s_cid.size(), s_cid.data(), s_id.data(), s_ext.data(), s_ts.data(), s_vec.data(),
                                files.temporary(s), bytes, nullptr, nullptr);
    }));
  }
  const double t2 = now_ms();

  // ---- the new resident index, beside the old one ----
  auto dev = std::make_unique<DeviceIndex>();
  VI_TRY(device_index_update(old, keep, rows ? rows->Xd.p : nullptr, n, order.p, seg_dev.p, seg, rows ? rows->ext_dev.p : nullptr,
                             rows ? rows->ts_dev.p : nullptr, h_len, dev.get(), &us->ms_kernel, &us->kernel_bytes));
  const double t3 = now_ms();
  us->ms_index = (float)(t3 - t2);

  VI_TRY(commit_and_swap(ix, files, std::move(dev)));
  const double t4 = now_ms();
  us->bytes_written = files.bytes();
  us->shards_rewritten = files.files();
  us->ms_files = (float)((t2 - t1) + (t4 - t3));
  us->ms_total = (float)(t4 - t0);
  return VI_OK;
}

// rows, no filter
vi_status add_records(Indexer *ix, const uint64_t *ext_ids, const float *X, const uint64_t *timestamps, uint64_t n) {
  const double t0 = now_ms();
  const uint64_t n_before = ix->dev->nvec_resident;
  std::vector<uint64_t> own_ext;  // no external ids: the internal ones
  if (!ext_ids) {
    own_ext.resize(n);
    for (uint64_t i = 0; i < n; ++i) own_ext[i] = n_before + i;
    ext_ids = own_ext.data();
  }
  NewRows rows;
  UpdateStats us;
  VI_TRY(upload_rows(ix, ext_ids, X, timestamps, n, &rows));
  VI_TRY(update_records(ix, nullptr, &rows, t0, &us));
  vi_add_stats as = common_stats<vi_add_stats>(us);
  as.n = n;
  as.ms_assign = us.ms_plan;
  ix->add_stats = as;
  return VI_OK;
}

// `keep`, and no rows (so no stream, no upload, no labelling)
vi_status retain_records(Indexer *ix, const SlotFilter &keep, uint64_t *removed_out) {
  const uint64_t n_before = ix->dev->nvec_resident;
  if (removed_out) *removed_out = 0;
  if (keep.num_allowed > n_before) return fail(VI_ERR_OTHER, "retain: the filter admits more records than the index holds");
  const uint64_t n_removed = n_before - keep.num_allowed;
  if (n_removed == 0) return VI_OK;  // nothing changes: no file, no index, no filter
  if (keep.num_allowed == 0)
    return fail(VI_ERR_INVALID_INPUT, "the removal would leave the index without a record (an index keeps at least one; to drop it, delete its directories)");
  const double t0 = now_ms();
  UpdateStats us;
  VI_TRY(update_records(ix, &keep, nullptr, t0, &us));
  vi_remove_stats rs = common_stats<vi_remove_stats>(us);
  rs.n_removed = n_removed;
  rs.lists_emptied = us.lists_emptied;
  rs.ms_plan = us.ms_plan;
  ix->remove_stats = rs;
  if (removed_out) *removed_out = n_removed;
  return VI_OK;
}

// rows, and the filter that denies their external ids
vi_status upsert_records(Indexer *ix, const uint64_t *ext_ids, const float *X, const uint64_t *timestamps, uint64_t n,
                         uint64_t *replaced_out) {
  const double t0 = now_ms();
  const uint64_t n_before = ix->dev->nvec_resident;
  NewRows rows;
  UpdateStats us;
  VI_TRY(upload_rows(ix, ext_ids, X, timestamps, n, &rows));
  SlotFilter keep;  // the records a VI_IDS_DENY filter of the set admits (the ids are read from the upload)
  VI_TRY(slot_filter_ids(*ix->dev, rows.ext_dev.p, n, true, true, &keep));
  if (keep.num_allowed > n_before) return fail(VI_ERR_OTHER, "upsert: the filter admits more records than the index holds");
  const uint64_t n_replaced = n_before - keep.num_allowed;
  if (keep.num_allowed + n > 0xFFFFFFFEull) return fail(VI_ERR_INVALID_INPUT, "more than 2^32 - 2 vectors");
  VI_TRY(update_records(ix, &keep, &rows, t0, &us));
  vi_upsert_stats st = common_stats<vi_upsert_stats>(us);
  st.n = n;
  st.n_replaced = n_replaced;
  st.lists_emptied = us.lists_emptied;
  st.ms_plan = us.ms_plan;
  ix->upsert_stats = st;
  if (replaced_out) *replaced_out = n_replaced;
  return VI_OK;
}

// ---- refine: every list touched, the new resident index first (device_index_refine: it decides what the files hold),
// then every shard file that holds a list, and index.bin behind them, written from it ----
// rule (a rebalance): the split steps of the first iterations, and the counts go to rebalance_stats instead
vi_status refine_records(Indexer *ix, uint64_t iters, uint64_t *moved_out, const SplitRule *rule) {
  const double t0 = now_ms();
  const DeviceIndex &old = *ix->dev;
  const uint32_t dim = ix->cfg.dimension;
  const uint64_t nlists = old.nlists;
  if (ix->meta.k() != nlists || ix->meta.centroids.size() != nlists * dim)
    return fail(VI_ERR_OTHER, "refine: the table of the handle does not match its index");
  VI_HIP(hipSetDevice(old.device));
  auto dev = std::make_unique<DeviceIndex>();
  RefineResult rr;
  SplitStats ss;
  VI_TRY(device_index_refine(old, ix->meta.centroids.data(), iters, dev.get(), &rr, rule, rule ? &ss : nullptr));
  const double t1 = now_ms();

  // ---- files: every shard that holds a list, its lists in the order the file has them; then index.bin ----
  IndexMeta meta = ix->meta;
  meta.centroids = rr.table;
  ShardRewriteSet files(ix->shards_dir);
  {
    ShardExportWs ws;
    std::vector<uint64_t> cids;
    std::vector<float> cvec;
    VI_TRY(rewrite_shards(files, dim, touched_lists_by_shard(ix->meta, nlists, [](uint64_t) { return true; }), rr.old_len,
                          [&](uint64_t s, const ShardFile &f, const std::vector<uint32_t> &lists, const std::vector<const ShardListView *> &,
                              uint64_t *bytes) -> vi_status {
      // every resident list of the shard is in the file; the file holds no other
      if (f.num_lists() != lists.size())
        return fail(VI_ERR_INVALID_DATA, "shard %llu holds %u lists, the index %zu of it", (unsigned long long)s, f.num_lists(), lists.size());
      cids.clear(); cvec.clear();
      for (uint32_t i = 0; i < f.num_lists(); ++i) {
        const uint64_t l = f.list(i).centroid_id;
        if (l >= nlists || ix->meta.c2s[l] != s)
          return fail(VI_ERR_INVALID_DATA, "shard %llu holds a list the index keeps elsewhere", (unsigned long long)s);
        cids.push_back(l);
        cvec.insert(cvec.end(), &meta.centroids[l * dim], &meta.centroids[l * dim] + dim);
      }
      return shard_export_blocks(*dev, files.temporary(s), s, cids, cvec.data(), ws, bytes);
    }));
    VI_TRY(index_meta_replace(meta, ix->index_dir, &files));
  }

  VI_TRY(commit_and_swap(ix, files, std::move(dev)));
  ix->meta.centroids.swap(meta.centroids);
  const double t2 = now_ms();
  vi_refine_stats rs{};
  rs.iterations_run = rr.iterations_run; rs.moved = rr.moved; rs.lists_emptied = rr.lists_emptied;
  rs.shards_rewritten = files.files(); rs.bytes_written = files.bytes();
  rs.means_bytes = rr.means_bytes; rs.rehome_bytes = rr.rehome_bytes;
  rs.ms_total = (float)(t2 - t0);
  rs.ms_means = rr.ms_means; rs.ms_label = rr.ms_label; rs.ms_rehome = rr.ms_rehome; rs.ms_images = rr.ms_images;
  rs.ms_files = (float)(t2 - t1);
  rs.ms_means_kernel = rr.ms_means_kernel; rs.ms_rehome_kernel = rr.ms_rehome_kernel;
  if (rule) {
    vi_rebalance_stats bs{};
    bs.iterations_run = rs.iterations_run; bs.moved = rs.moved; bs.lists_emptied = rs.lists_emptied;
    bs.shards_rewritten = rs.shards_rewritten; bs.bytes_written = rs.bytes_written;
    bs.means_bytes = rs.means_bytes; bs.rehome_bytes = rs.rehome_bytes;
    bs.ms_total = rs.ms_total; bs.ms_means = rs.ms_means; bs.ms_label = rs.ms_label; bs.ms_rehome = rs.ms_rehome;
    bs.ms_images = rs.ms_images; bs.ms_files = rs.ms_files;
    bs.ms_means_kernel = rs.ms_means_kernel; bs.ms_rehome_kernel = rs.ms_rehome_kernel;
    bs.pairs_planned = ss.pairs_planned; bs.splits_done = ss.splits_done; bs.splits_skipped = ss.splits_skipped;
    bs.inner_iterations = ss.inner_iterations; bs.split_bytes = ss.split_bytes;
    bs.ms_split = ss.ms; bs.ms_split_kernels = ss.ms_kernels;
    ix->rebalance_stats = bs;
  } else {
    ix->refine_stats = rs;
  }
  if (moved_out) *moved_out = rr.moved;
  return VI_OK;
}

}  // namespace vi
