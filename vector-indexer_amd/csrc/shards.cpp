// shards.cpp — see shards.hpp.
#include "shards.hpp"

#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

namespace vi {

namespace {
template <typename T>
T load_le(const uint8_t *p) {
  T v;
  std::memcpy(&v, p, sizeof(T));
  return v;
}
void put_record(uint8_t *o, uint64_t id, uint64_t ext_id, uint64_t timestamp, const float *vec, uint64_t vsz) {
  const uint64_t meta[3] = {id, ext_id, timestamp};  // VectorMeta (shards.rs:45-51)
  std::memcpy(o, meta, kVectorMetaBytes);
  std::memcpy(o + kVectorMetaBytes, vec, vsz);
}
}  // namespace

std::string shard_file_path(const std::string &shards_dir, uint64_t shard_id) {
  return shards_dir + "/shard_" + std::to_string(shard_id) + ".bin";
}

vi_status make_dirs(const std::string &path) {
  if (path.empty()) return fail(VI_ERR_IO, "empty directory path");
  std::string cur;
  size_t i = 0;
  while (i <= path.size()) {
    if (i == path.size() || path[i] == '/') {
      if (!cur.empty() && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST)
        return fail(VI_ERR_IO, "create_dir_all(%s): %s", cur.c_str(), strerror(errno));
    }
    if (i < path.size()) cur.push_back(path[i]);
    ++i;
  }
  return VI_OK;
}

ShardFile::~ShardFile() {
  if (map_ && len_) munmap(map_, len_);
}

vi_status ShardFile::open(const std::string &shards_dir, uint64_t shard_id) {
  const std::string path = shard_file_path(shards_dir, shard_id);
  int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0)
    return fail(VI_ERR_OTHER, "Failed to open shard_%llu.bin file: %s", (unsigned long long)shard_id,
                strerror(errno));
  struct stat st;
  if (fstat(fd, &st) != 0) {
    ::close(fd);
    return fail(VI_ERR_OTHER, "Failed to read header of shard_%llu.bin file", (unsigned long long)shard_id);
  }
  len_ = (size_t)st.st_size;
  if (len_ < kShardHeaderBytes) {
    ::close(fd);
    len_ = 0;
    return fail(VI_ERR_INVALID_DATA, "Invalid shard header, reading shard_%llu.bin.", (unsigned long long)shard_id);
  }
  map_ = mmap(nullptr, len_, PROT_READ, MAP_PRIVATE, fd, 0);
  ::close(fd);
  if (map_ == MAP_FAILED) {
    map_ = nullptr;
    len_ = 0;
    return fail(VI_ERR_OTHER, "mmap shard_%llu.bin: %s", (unsigned long long)shard_id, strerror(errno));
  }
  const uint8_t *base = (const uint8_t *)map_;
  const uint64_t file_shard = load_le<uint64_t>(base + 0);
  if (file_shard != shard_id)  // shards.rs:223-231
    return fail(VI_ERR_INVALID_DATA, "Shard ID mismatch: expected %llu, found %llu in file",
                (unsigned long long)shard_id, (unsigned long long)file_shard);
  dim_ = load_le<uint32_t>(base + 16);
  const uint32_t nc = load_le<uint32_t>(base + 20);
  const uint64_t index_off = load_le<uint64_t>(base + 24);
  if (index_off > len_ || (uint64_t)nc * kIndexEntryBytes > len_ - index_off)
    return fail(VI_ERR_INVALID_DATA, "Failed to read index in shard_%llu", (unsigned long long)shard_id);
  const uint64_t vsz = 4ull * dim_, cpad = pad8(vsz), stride = record_stride(dim_);
  lists_.resize(nc);
  for (uint32_t i = 0; i < nc; ++i) {
    const uint8_t *e = base + index_off + (uint64_t)i * kIndexEntryBytes;
    ShardListView &lv = lists_[i];
    lv.centroid_id = load_le<uint64_t>(e + 0);
    lv.num_vectors = load_le<uint32_t>(e + 8);
    const uint64_t off = load_le<uint64_t>(e + 16), size = load_le<uint64_t>(e + 24);
    if (off > len_ || size > len_ - off || size < vsz)
      return fail(VI_ERR_OTHER, "Failed to read cluster: block out of file bounds");
    // bounds check of every record (shards.rs:310-316)
    const uint64_t need = vsz + cpad + (uint64_t)lv.num_vectors * stride - (lv.num_vectors ? cpad : 0);
    if (need > size)
      return fail(VI_ERR_INVALID_DATA, "Not enough bytes for vector metadata in centroid %llu block",
                  (unsigned long long)lv.centroid_id);
    lv.centroid = base + off;
    lv.records = base + off + vsz + cpad;
  }
  return VI_OK;
}

const ShardListView *ShardFile::find(uint64_t centroid_id) const {
  for (const ShardListView &l : lists_)
    if (l.centroid_id == centroid_id) return &l;
  return nullptr;
}

// ---- the frame every writer shares ---------------------------------------------------------
ShardPlan::ShardPlan(uint32_t dim_, std::vector<uint64_t> counts)
    : dim(dim_), vsz(4ull * dim_), pad(pad8(vsz)), stride(record_stride(dim_)),
      data_off(kShardHeaderBytes + kIndexEntryBytes * (uint64_t)counts.size()), total(data_off), count(std::move(counts)) {
  for (uint64_t nv : count) {
    off.push_back(total);
    size.push_back(vsz + pad + nv * stride);
    total += size.back();
  }
}

void shard_frame_write(uint8_t *p, const ShardPlan &pl, uint64_t shard_id, const uint64_t *cids, const void *const *cvecs) {
  auto put64 = [&](uint64_t off, uint64_t v) { std::memcpy(p + off, &v, 8); };
  auto put32 = [&](uint64_t off, uint32_t v) { std::memcpy(p + off, &v, 4); };
  const uint32_t nl = (uint32_t)pl.count.size();
  put64(0, shard_id); put64(8, 1); put32(16, pl.dim); put32(20, nl);
  put64(24, kShardHeaderBytes); put64(32, pl.data_off);
  for (uint32_t i = 0; i < nl; ++i) {
    const uint64_t e = kShardHeaderBytes + (uint64_t)i * kIndexEntryBytes;
    put64(e, cids[i]); put32(e + 8, (uint32_t)pl.count[i]); put32(e + 12, 0);
    put64(e + 16, pl.off[i]); put64(e + 24, pl.size[i]);
    std::memcpy(p + pl.off[i], cvecs[i], pl.vsz);
    std::memset(p + pl.off[i] + pl.vsz, 0, pl.pad);
  }
}

vi_status shard_image_write(const std::string &path, const uint8_t *p, uint64_t total, bool unlink_on_failure) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return fail(VI_ERR_IO, "File::create(%s): %s", path.c_str(), strerror(errno));
  const bool ok = total == 0 || fwrite(p, 1, total, f) == total;
  if (fclose(f) != 0 || !ok) {
    if (unlink_on_failure) ::unlink(path.c_str());
    return fail(VI_ERR_IO, "write(%s) failed", path.c_str());
  }
  return VI_OK;
}

namespace {
// the zeroed image of f's lists with other record counts, its frame written: what shard_update_write starts from
ShardPlan image_of_file(const ShardFile &f, uint64_t shard_id, std::vector<uint64_t> counts, std::vector<uint8_t> *img) {
  const uint32_t nl = f.num_lists();
  std::vector<uint64_t> cids(nl);
  std::vector<const void *> cvecs(nl);
  for (uint32_t i = 0; i < nl; ++i) { cids[i] = f.list(i).centroid_id; cvecs[i] = f.list(i).centroid; }
  ShardPlan pl(f.dim(), std::move(counts));
  img->assign(pl.total, 0);
  shard_frame_write(img->data(), pl, shard_id, cids.data(), cvecs.data());
  return pl;
}
}  // namespace

vi_status shard_save_to(const std::string &shards_dir, uint64_t shard_id, uint32_t dim,
                        uint32_t num_lists, const uint64_t *centroid_ids, const float *centroid_vecs,
                        const uint64_t *list_off, const uint64_t *ids, const uint64_t *ext_ids,
                        const uint64_t *timestamps, const float *vecs) {
  VI_TRY(make_dirs(shards_dir));
  const std::string path = shard_file_path(shards_dir, shard_id);
  ::unlink(path.c_str());  // shards.rs:73
  std::vector<uint64_t> counts(num_lists);
  std::vector<const void *> cvecs(num_lists);
  for (uint32_t i = 0; i < num_lists; ++i) { counts[i] = list_off[i + 1] - list_off[i]; cvecs[i] = centroid_vecs + (uint64_t)i * dim; }
  const ShardPlan pl(dim, std::move(counts));
  std::vector<uint8_t> img(pl.total, 0);  // the whole image assembled once, written with a single call
  shard_frame_write(img.data(), pl, shard_id, centroid_ids, cvecs.data());
  for (uint32_t i = 0; i < num_lists; ++i) {
    uint8_t *o = img.data() + pl.records(i);
    for (uint64_t v = list_off[i]; v < list_off[i + 1]; ++v, o += pl.stride)
      put_record(o, ids[v], ext_ids[v], timestamps[v], vecs + v * dim, pl.vsz);
  }
  return shard_image_write(path, img.data(), pl.total, false);
}

vi_status shard_update_write(const ShardFile &f, uint64_t shard_id, const std::vector<const uint64_t *> &keep, uint64_t n_add,
                             const uint64_t *centroid_ids, const uint64_t *ids, const uint64_t *ext_ids,
                             const uint64_t *timestamps, const float *vecs, const std::string &out_path, uint64_t *bytes_out,
                             uint64_t *removed_out, uint64_t *lists_out) {
  const uint32_t dim = f.dim(), nl = f.num_lists();
  if (!keep.empty() && keep.size() != nl) return fail(VI_ERR_OTHER, "update: %zu keep entries for %u lists", keep.size(), nl);
  auto words_of = [&](uint32_t i) { return keep.empty() ? nullptr : keep[i]; };  // (an empty keep: nothing goes)
  auto stays = [](const uint64_t *w, uint32_t p) { return ((w[p >> 6] >> (p & 63u)) & 1ull) != 0; };
  // the list of every added record: the first entry with its centroid id, as the reader finds it (shards.rs:257-265)
  std::unordered_map<uint64_t, uint32_t> entry_of;
  for (uint32_t i = nl; i-- > 0;) entry_of[f.list(i).centroid_id] = i;
  std::vector<uint32_t> entry(n_add);
  std::vector<uint64_t> kept(nl), received(nl, 0);
  for (uint64_t i = 0; i < n_add; ++i) {
    const auto it = entry_of.find(centroid_ids[i]);
    if (it == entry_of.end()) return fail(VI_ERR_NOT_FOUND, "Centroid %llu not found", (unsigned long long)centroid_ids[i]);
    entry[i] = it->second;
    ++received[it->second];
  }
  uint64_t removed = 0, touched = 0;
  std::vector<uint64_t> counts(nl);
  for (uint32_t i = 0; i < nl; ++i) {
    const uint32_t nv = f.list(i).num_vectors;
    kept[i] = nv;
    if (const uint64_t *w = words_of(i)) {
      kept[i] = 0;
      for (uint32_t p = 0; p < nv; ++p) kept[i] += stays(w, p);
    }
    counts[i] = kept[i] + received[i];
    if (counts[i] > 0xFFFFFFFFull) return fail(VI_ERR_INVALID_INPUT, "list %llu would pass 2^32 - 1 records", (unsigned long long)f.list(i).centroid_id);
    removed += nv - kept[i];
    touched += kept[i] != nv || received[i] != 0;
  }
  std::vector<uint8_t> img;
  const ShardPlan pl = image_of_file(f, shard_id, std::move(counts), &img);
  std::vector<uint64_t> next(nl);  // where the next added record of a list goes: behind its kept records
  for (uint32_t i = 0; i < nl; ++i) {
    const ShardListView &lv = f.list(i);
    uint8_t *o = img.data() + pl.records(i);
    next[i] = pl.records(i) + kept[i] * pl.stride;
    if (kept[i] == lv.num_vectors) {  // nothing lost: verbatim
      if (lv.num_vectors) std::memcpy(o, lv.records, (uint64_t)lv.num_vectors * pl.stride);
      continue;
    }
    const uint64_t *w = words_of(i);  // (not null: the list lost a record)
    for (uint32_t v = 0; v < lv.num_vectors;) {  // runs of kept records
      if (!stays(w, v)) { ++v; continue; }
      uint32_t end = v + 1;
      while (end < lv.num_vectors && stays(w, end)) ++end;
      std::memcpy(o, lv.records + (uint64_t)v * pl.stride, (uint64_t)(end - v) * pl.stride);
      o += (uint64_t)(end - v) * pl.stride;
      v = end;
    }
  }
  for (uint64_t i = 0; i < n_add; ++i) {
    put_record(img.data() + next[entry[i]], ids[i], ext_ids[i], timestamps[i], vecs + i * dim, pl.vsz);
    next[entry[i]] += pl.stride;
  }
  VI_TRY(shard_image_write(out_path, img.data(), pl.total, true));
  if (bytes_out) *bytes_out = pl.total;
  if (removed_out) *removed_out = removed;
  if (lists_out) *lists_out = touched;
  return VI_OK;
}

namespace {
// The allow words of a file by external id: keep[i] of every first entry of f that carries one of ext_ids[0..n) (null: the
// entry loses nothing); `words` owns them.  -> whether any record goes
bool deny_words_of_file(const ShardFile &f, const uint64_t *ext_ids, uint64_t n, std::vector<std::vector<uint64_t>> *words,
                        std::vector<const uint64_t *> *keep) {
  const std::unordered_set<uint64_t> gone(ext_ids, ext_ids + n);
  const uint32_t nl = f.num_lists();
  const uint64_t stride = record_stride(f.dim());
  words->assign(nl, {});
  keep->assign(nl, nullptr);
  bool any = false;
  for (uint32_t i = 0; i < nl; ++i) {
    const ShardListView &lv = f.list(i);
    if (f.find(lv.centroid_id) != &lv) continue;  // (a later entry of a repeated centroid id: no reader sees it)
    (*words)[i].assign(((uint64_t)lv.num_vectors + 63) / 64, 0);
    for (uint32_t v = 0; v < lv.num_vectors; ++v) {
      uint64_t ext;
      std::memcpy(&ext, lv.records + (uint64_t)v * stride + 8, 8);  // VectorMeta.external_id
      if (gone.count(ext)) (*keep)[i] = (*words)[i].data();
      else (*words)[i][v >> 6] |= 1ull << (v & 63u);
    }
    any = any || (*keep)[i];
  }
  return any;
}

// One shard file on its own: the records that carry one of gone_ext[0..n_gone) go, n_add records join; open, write beside
// the file under a temporary name, rename.  Nothing to go and nothing to join: the file is opened and left as it is.
vi_status update_one_file(const std::string &shards_dir, uint64_t shard_id, const uint64_t *gone_ext, uint64_t n_gone, uint64_t n_add,
                          const uint64_t *centroid_ids, const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps,
                          const float *vecs, uint64_t *removed_out) {
  if (removed_out) *removed_out = 0;
  ShardRewriteSet set(shards_dir);
  uint64_t removed = 0;
  {
    ShardFile f;
    VI_TRY(f.open(shards_dir, shard_id));
    std::vector<std::vector<uint64_t>> words;
    std::vector<const uint64_t *> keep;  // (stays empty where no id is given: nothing goes)
    const bool any_goes = n_gone && deny_words_of_file(f, gone_ext, n_gone, &words, &keep);
    if (!any_goes && n_add == 0) return VI_OK;
    uint64_t bytes = 0;
    VI_TRY(shard_update_write(f, shard_id, keep, n_add, centroid_ids, ids, ext_ids, timestamps, vecs, set.temporary(shard_id), &bytes,
                              &removed, nullptr));
    set.add(shard_id, bytes);
  }  // (unmapped before the rename)
  VI_TRY(set.commit());
  if (removed_out) *removed_out = removed;
  return VI_OK;
}
}  // namespace

vi_status shard_append_to(const std::string &shards_dir, uint64_t shard_id, uint64_t n_add, const uint64_t *centroid_ids,
                          const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs) {
  return update_one_file(shards_dir, shard_id, nullptr, 0, n_add, centroid_ids, ids, ext_ids, timestamps, vecs, nullptr);
}

vi_status shard_remove_from(const std::string &shards_dir, uint64_t shard_id, const uint64_t *ext_ids, uint64_t n,
                            uint64_t *removed_out) {
  return update_one_file(shards_dir, shard_id, ext_ids, n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, removed_out);
}

vi_status shard_upsert_to(const std::string &shards_dir, uint64_t shard_id, uint64_t n, const uint64_t *centroid_ids,
                          const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs,
                          uint64_t *removed_out) {
  return update_one_file(shards_dir, shard_id, ext_ids, n, n, centroid_ids, ids, ext_ids, timestamps, vecs, removed_out);
}

// ---- the rewrite set ------------------------------------------------------------------------
vi_status ShardRewriteSet::open(uint64_t s, uint32_t dim, ShardFile *f) const {
  VI_TRY(f->open(dir_, s));
  if (f->dim() != dim) return fail(VI_ERR_INVALID_DATA, "shard_%llu.bin holds dimension %u", (unsigned long long)s, f->dim());
  return VI_OK;
}

vi_status ShardRewriteSet::find(const ShardFile &f, uint64_t s, uint32_t l, uint32_t len, const ShardListView **out) const {
  *out = f.find(l);
  if (!*out || (*out)->num_vectors != len)  // (the resident blocks are what the file's records are taken to be)
    return fail(VI_ERR_INVALID_DATA, "shard_%llu.bin no longer matches the resident list %u", (unsigned long long)s, l);
  return VI_OK;
}

void ShardRewriteSet::add(uint64_t s, uint64_t bytes) {
  add_pair(temporary(s), shard_file_path(dir_, s), bytes);
  ++shard_files_;
}

void ShardRewriteSet::add_pair(std::string temporary, std::string final_path, uint64_t bytes) {
  pairs_.emplace_back(std::move(temporary), std::move(final_path));
  bytes_ += bytes;
}

void ShardRewriteSet::drop() {
  for (; done_ < pairs_.size(); ++done_) ::unlink(pairs_[done_].first.c_str());
}

vi_status ShardRewriteSet::commit() {
  for (; done_ < pairs_.size(); ++done_)
    if (::rename(pairs_[done_].first.c_str(), pairs_[done_].second.c_str()) != 0) {
      const int e = errno;
      const size_t i = done_;
      drop();
      return fail(VI_ERR_IO, "rename(%s): %s%s", pairs_[i].first.c_str(), strerror(e),
                  i ? " (earlier shard files of this call are already in place: reload the index)" : "");
    }
  return VI_OK;
}

// ---- bincode 2 "standard" varint ----------------------------------------------------------
namespace {
void put_varint(std::vector<uint8_t> &b, uint64_t v) {
  auto raw = [&](int n) { for (int i = 0; i < n; ++i) b.push_back((uint8_t)(v >> (8 * i))); };
  if (v < 251) b.push_back((uint8_t)v);
  else if (v <= 0xFFFF) { b.push_back(251); raw(2); }
  else if (v <= 0xFFFFFFFFull) { b.push_back(252); raw(4); }
  else { b.push_back(253); raw(8); }
}
struct Reader {
  const uint8_t *p; size_t len, off = 0;
  bool varint(uint64_t *v) {
    if (off >= len) return false;
    const uint8_t t = p[off++];
    int nb;
    if (t < 251) { *v = t; return true; }
    if (t == 251) nb = 2; else if (t == 252) nb = 4; else if (t == 253) nb = 8; else return false;
    if (off + nb > len) return false;
    uint64_t x = 0;
    for (int i = 0; i < nb; ++i) x |= (uint64_t)p[off + i] << (8 * i);
    off += nb;
    *v = x;
    return true;
  }
  bool byte(uint8_t *v) { if (off >= len) return false; *v = p[off++]; return true; }
  bool floats(float *dst, uint64_t n) {
    if (n > (len - off) / 4) return false;
    std::memcpy(dst, p + off, n * 4);
    off += n * 4;
    return true;
  }
};
vi_status slurp(const std::string &path, std::vector<uint8_t> *out, vi_status not_found) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return fail(errno == ENOENT ? not_found : VI_ERR_IO, "open(%s): %s", path.c_str(), strerror(errno));
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize(sz > 0 ? (size_t)sz : 0);
  const bool ok = out->empty() || fread(out->data(), 1, out->size(), f) == out->size();
  fclose(f);
  return ok ? VI_OK : fail(VI_ERR_IO, "read(%s) failed", path.c_str());
}
}  // namespace

vi_status index_meta_save(const IndexMeta &m, const std::string &index_dir) {
  VI_TRY(make_dirs(index_dir));
  return index_meta_write(m, index_dir + "/index.bin", nullptr);
}

vi_status index_meta_write(const IndexMeta &m, const std::string &path, uint64_t *bytes_out) {
  std::vector<uint8_t> b;
  const uint64_t k = m.k(), d = m.dimension;
  b.reserve(k * (d * 4 + 12) + 64);
  b.push_back(1); put_varint(b, k); put_varint(b, k);       // ndarray: version, dim, data len
  for (uint64_t c = 0; c < k; ++c) {
    put_varint(b, c); put_varint(b, d);                       // Centroid{id, vector}
    const uint8_t *src = (const uint8_t *)(m.centroids.data() + c * d);
    b.insert(b.end(), src, src + d * 4);
  }
  b.push_back(1); put_varint(b, k); put_varint(b, k);
  for (uint64_t c = 0; c < k; ++c) put_varint(b, m.c2s[c]);
  put_varint(b, d);
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return fail(VI_ERR_IO, "File::create(%s): %s", path.c_str(), strerror(errno));
  const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
  if (fclose(f) != 0 || !ok) return fail(VI_ERR_IO, "write(%s) failed", path.c_str());
  if (bytes_out) *bytes_out = b.size();
  return VI_OK;
}

vi_status index_meta_replace(const IndexMeta &m, const std::string &index_dir, ShardRewriteSet *set) {
  const std::string path = index_dir + "/index.bin", tmp = path + ".tmp";
  uint64_t bytes = 0;
  const vi_status s = index_meta_write(m, tmp, &bytes);
  if (s != VI_OK) ::remove(tmp.c_str());
  else set->add_pair(tmp, path, bytes);
  return s;
}

vi_status index_meta_load(const std::string &index_dir, IndexMeta *out) {
  std::vector<uint8_t> raw;
  VI_TRY(slurp(index_dir + "/index.bin", &raw, VI_ERR_NOT_FOUND));
  Reader r{raw.data(), raw.size()};
  auto bad = [] { return fail(VI_ERR_OTHER, "Bincode decoding error: malformed index.bin"); };
  uint8_t ver;
  uint64_t k, k2, v;
  if (!r.byte(&ver) || ver != 1 || !r.varint(&k) || !r.varint(&k2) || k != k2) return bad();
  uint64_t d0 = 0;
  out->centroids.clear();
  for (uint64_t c = 0; c < k; ++c) {
    uint64_t id, dl;
    if (!r.varint(&id) || !r.varint(&dl)) return bad();
    if (c == 0) { d0 = dl; if (dl && k > (raw.size() / 4) / dl + 1) return bad(); out->centroids.resize(k * dl); }
    if (dl != d0 || !r.floats(out->centroids.data() + c * d0, dl)) return bad();
  }
  if (!r.byte(&ver) || ver != 1 || !r.varint(&v) || v != k || !r.varint(&v) || v != k) return bad();
  out->c2s.resize(k);
  for (uint64_t c = 0; c < k; ++c)
    if (!r.varint(&out->c2s[c])) return bad();
  if (!r.varint(&v)) return bad();
  out->dimension = (uint32_t)v;
  if (k > 0 && d0 != out->dimension) return bad();
  return VI_OK;
}

vi_status read_vectors_from_file(const std::string &path, std::vector<VectorFileRecord> *out) {
  std::vector<uint8_t> raw;
  VI_TRY(slurp(path, &raw, VI_ERR_OTHER));  // api.rs:156 wraps every failure as Other
  Reader r{raw.data(), raw.size()};
  out->clear();
  while (r.off < r.len) {
    const size_t batch_start_count = out->size();
    uint64_t cnt;
    bool ok = r.varint(&cnt) && cnt <= r.len - r.off;  // every record takes at least three bytes
    for (uint64_t i = 0; ok && i < cnt; ++i) {
      VectorFileRecord rec;
      uint64_t vl;
      ok = r.varint(&rec.id) && r.varint(&vl) && vl <= (r.len - r.off) / 4;  // (vl * 4 would wrap for vl >= 2^62)
      if (ok) { rec.values.resize(vl); ok = r.floats(rec.values.data(), vl) && r.varint(&rec.meta); }
      if (ok) out->push_back(std::move(rec));
    }
    if (!ok) { out->resize(batch_start_count); break; }  // Err(_) => break (utils.rs:102)
  }
  return VI_OK;
}

}  // namespace vi
