// shards.hpp — shard_<id>.bin on-disk format (byte-identical to the reference writer,
// src/shards.rs:22-51,68-177) and index/index.bin (src/ivf_index.rs:274-316).
//
// The reference re-opens and re-reads shard files with io_uring on every query
// (shards.rs:188-349).  Here files are only touched at build/load time: lists are
// repacked into the lane-interleaved HBM layout (device_index.hpp) and stay resident.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

namespace vi {

// Layout constants of the repr(C) structs (shards.rs:22-51).
constexpr uint64_t kShardHeaderBytes = 40;  // the reference's "// 48 bytes" comment is wrong
constexpr uint64_t kIndexEntryBytes = 32;
constexpr uint64_t kVectorMetaBytes = 24;

inline uint64_t pad8(uint64_t vec_bytes) { return (8 - (vec_bytes % 8)) % 8; }
// bytes of one stored record: VectorMeta + D*f32 + pad (shards.rs:106-114)
inline uint64_t record_stride(uint32_t dim) { return kVectorMetaBytes + 4ull * dim + pad8(4ull * dim); }

struct ShardListView {       // one inverted list inside a mapped shard file
  uint64_t centroid_id = 0;
  uint32_t num_vectors = 0;
  const uint8_t *centroid = nullptr;  // dim f32
  const uint8_t *records = nullptr;   // num_vectors records of record_stride(dim) bytes
};

// Read-only memory map of one shard file with a validated index.
class ShardFile {
 public:
  ShardFile() = default;
  ~ShardFile();
  ShardFile(const ShardFile &) = delete;
  ShardFile &operator=(const ShardFile &) = delete;

  // Errors follow get_centroid_vectors_from (shards.rs:193-231): open failure => Other,
  // short/invalid header or shard-id mismatch => InvalidData.
  vi_status open(const std::string &shards_dir, uint64_t shard_id);
  uint32_t dim() const { return dim_; }
  uint32_t num_lists() const { return (uint32_t)lists_.size(); }
  const ShardListView &list(uint32_t i) const { return lists_[i]; }
  // linear find, as the reference does (shards.rs:257-265); nullptr => NotFound
  const ShardListView *find(uint64_t centroid_id) const;

 private:
  void *map_ = nullptr;
  size_t len_ = 0;
  uint32_t dim_ = 0;
  std::vector<ShardListView> lists_;
};

// Where everything of a shard image lies, from dim and the record count of every list in file order: header, index
// entries, then list after list its centroid vector, the pad to 8 bytes and its records (shards.rs:68-177).
struct ShardPlan {
  uint32_t dim;
  uint64_t vsz, pad, stride, data_off, total;  // bytes of a vector, its pad, a record; first block; the whole image
  std::vector<uint64_t> count, off, size;      // per list: records, byte offset and bytes of its block
  ShardPlan(uint32_t dim, std::vector<uint64_t> counts);
  uint64_t records(uint32_t i) const { return off[i] + vsz + pad; }  // byte offset of list i's first record
};
// Header, index entries and centroid vectors (pad zeroed) of the image at p, pl.total bytes; the records are the
// caller's.  cids[i] / cvecs[i]: centroid id and vector (dim f32) of list i.  The one place these bytes are laid down.
void shard_frame_write(uint8_t *p, const ShardPlan &pl, uint64_t shard_id, const uint64_t *cids, const void *const *cvecs);
// The image to the file `path` (created or truncated).  unlink_on_failure: a file left short by a failed write is removed.
vi_status shard_image_write(const std::string &path, const uint8_t *p, uint64_t total, bool unlink_on_failure);
std::string shard_file_path(const std::string &shards_dir, uint64_t shard_id);  // the one place a shard file is named

vi_status shard_save_to(const std::string &shards_dir, uint64_t shard_id, uint32_t dim,
                        uint32_t num_lists, const uint64_t *centroid_ids, const float *centroid_vecs,
                        const uint64_t *list_off, const uint64_t *ids, const uint64_t *ext_ids,
                        const uint64_t *timestamps, const float *vecs);

// Remove records from lists of an open shard file and append records to them, in one image.
//   keep: what goes.  Either empty — nothing goes, the same as num_lists() null entries — or one entry per list entry of
//     the file, in file order: null = every record of the list stays, else record p stays iff bit p % 64 of word p / 64
//     is set (ceil(num_vectors / 64) words: the allow words of a SlotFilter over the list's blocks).
//   n_add records: what joins; 0 = nothing is appended and none of the five arrays is read.  Added record i goes to the FIRST
//     list of the file that carries centroid_ids[i], behind the list's kept records and behind the added records named
//     before it.  A centroid id the file does not hold: NotFound, nothing written.
// The file is written to out_path — byte-identical to shard_save_to of the resulting lists: lists keep their file order,
// centroid vectors and kept records are copied verbatim, in runs (VectorMeta.id included), a list that keeps nothing and
// receives nothing stays as an entry with num_vectors == 0 — and f's own file is left alone: the caller renames out_path
// over it when every file of its batch is complete (index_lifecycle.cpp: update_records).  bytes_out / removed_out / lists_out
// (optional): size of the file written, records removed, lists that lost or received a record.
vi_status shard_update_write(const ShardFile &f, uint64_t shard_id, const std::vector<const uint64_t *> &keep, uint64_t n_add,
                             const uint64_t *centroid_ids, const uint64_t *ids, const uint64_t *ext_ids,
                             const uint64_t *timestamps, const float *vecs, const std::string &out_path, uint64_t *bytes_out,
                             uint64_t *removed_out, uint64_t *lists_out);
// The same for one shard file on its own: open, write beside it under a temporary name, rename.
// shard_append_to: nothing goes.  n_add == 0: the file is opened (the reader's errors) and left as it is.
vi_status shard_append_to(const std::string &shards_dir, uint64_t shard_id, uint64_t n_add, const uint64_t *centroid_ids,
                          const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs);
// shard_remove_from: nothing joins; every record whose external id is one of ext_ids[0..n) goes (any order, duplicates
// allowed, unknown ids ignored; of entries that repeat a centroid id only the first, the one a reader finds, is looked
// at).  Nothing matches: the file is opened and left as it is.
vi_status shard_remove_from(const std::string &shards_dir, uint64_t shard_id, const uint64_t *ext_ids, uint64_t n,
                            uint64_t *removed_out);
// shard_upsert_to: both, the ids that go being those of the records that join.  n == 0: the file is opened and left as it is.
vi_status shard_upsert_to(const std::string &shards_dir, uint64_t shard_id, uint64_t n, const uint64_t *centroid_ids,
                          const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs,
                          uint64_t *removed_out);

// The files one call rewrites: every file is written beside the old one under a temporary name and registered; commit()
// renames them over the old files in the order registered.  Whatever is registered and not renamed when the set goes
// away is unlinked: a call can fail anywhere before commit() without a trace.  The shard files of a call, and behind
// them its index.bin if the call changes the table (index_meta_replace).  Host only.
class ShardRewriteSet {
 public:
  explicit ShardRewriteSet(std::string shards_dir) : dir_(std::move(shards_dir)) {}
  ~ShardRewriteSet() { drop(); }
  ShardRewriteSet(const ShardRewriteSet &) = delete;
  ShardRewriteSet &operator=(const ShardRewriteSet &) = delete;

  // shard_<s>.bin of the directory, which must hold vectors of `dim` dimensions (else InvalidData)
  vi_status open(uint64_t s, uint32_t dim, ShardFile *f) const;
  // resident list l in f (= shard s), which must hold `len` records there (else InvalidData)
  vi_status find(const ShardFile &f, uint64_t s, uint32_t l, uint32_t len, const ShardListView **out) const;
  std::string temporary(uint64_t s) const { return shard_file_path(dir_, s) + ".tmp"; }
  void add(uint64_t s, uint64_t bytes);  // temporary(s) is written, `bytes` long
  // any other pair: `temporary` is written, `bytes` long, and becomes `final_path` (counted by bytes(), not by files())
  void add_pair(std::string temporary, std::string final_path, uint64_t bytes);
  // Renames in order.  The first failure unlinks the temporaries not yet renamed: VI_ERR_IO (the files renamed before it
  // stay in place, and the message says so).  Close every ShardFile of the set's files first.
  vi_status commit();
  uint64_t files() const { return shard_files_; }  // shard files registered
  uint64_t bytes() const { return bytes_; }        // of every pair

 private:
  void drop();
  std::string dir_;
  std::vector<std::pair<std::string, std::string>> pairs_;  // (temporary, final)
  size_t done_ = 0;                                         // pairs renamed or unlinked
  uint64_t shard_files_ = 0, bytes_ = 0;
};

// index/index.bin: IvfIndex{centroids, centroids_to_shard, dimension} through bincode 2
// `config::standard()` + ndarray serde.  PARITY UNPINNED (no cargo here to confirm bytes).
struct IndexMeta {
  uint32_t dimension = 0;
  std::vector<float> centroids;      // k' x dimension
  std::vector<uint64_t> c2s;         // k'
  uint64_t k() const { return c2s.size(); }
};
vi_status index_meta_save(const IndexMeta &m, const std::string &index_dir);
vi_status index_meta_load(const std::string &index_dir, IndexMeta *out);
// the same bytes to any path (bytes_out, optional: how many)
vi_status index_meta_write(const IndexMeta &m, const std::string &path, uint64_t *bytes_out);
// index.bin as one more file of a rewrite set: written to index.bin.tmp beside it and registered as the set's last pair
// so far (a temporary left short by a failed write is removed, nothing is registered)
vi_status index_meta_replace(const IndexMeta &m, const std::string &index_dir, ShardRewriteSet *set);

// batched vector file of read_vectors_from_file (src/utils.rs:82-107): concatenated
// bincode Vec<(u64, Vec<f32>, u64)> batches.  Decoding stops silently at the first
// undecodable batch (utils.rs:102), as the reference does.
struct VectorFileRecord { uint64_t id; std::vector<float> values; uint64_t meta; };
vi_status read_vectors_from_file(const std::string &path, std::vector<VectorFileRecord> *out);

vi_status make_dirs(const std::string &path);

}  // namespace vi
