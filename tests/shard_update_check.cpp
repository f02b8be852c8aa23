// shard_update_check.cpp — host checks of the shard frame and the rewrite set of csrc/shards.cpp (compiled together with
// it and run by test_shard_update_cpu.py, in the scratch directory given as argv[1]): prints one line per failed check
// and exits non-zero if there was one.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "shards.hpp"

namespace vi {
std::string &last_error_ref() {
  static thread_local std::string msg;
  return msg;
}
}  // namespace vi

using namespace vi;

static int failures = 0;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static bool exists(const std::string &path) {
  struct stat st;
  return ::stat(path.c_str(), &st) == 0;
}

static Bytes slurp(const std::string &path) {
  Bytes b;
  if (FILE *f = fopen(path.c_str(), "rb")) {
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + n);
    fclose(f);
  }
  return b;
}

static void spill(const std::string &path, const std::string &text) {
  CHECK(shard_image_write(path, (const uint8_t *)text.data(), text.size(), false) == VI_OK, "%s", path.c_str());
}

template <typename T>
static T load(const Bytes &b, uint64_t off) {
  T v{};
  if (off + sizeof(T) <= b.size()) std::memcpy(&v, b.data() + off, sizeof(T));
  return v;
}

// the lists the issue names: 5, 70, 0, 1 and 130 records, centroid ids 20..24; record v carries id v, external id
// 1000 + v, timestamp 5000 + v and the vector (v, v + 0.5, ...)
struct Lists {
  uint32_t dim;
  std::vector<uint64_t> cids{20, 21, 22, 23, 24}, off{0, 5, 75, 75, 76, 206}, ids, ext, ts;
  std::vector<float> cvecs, vecs;
  explicit Lists(uint32_t d) : dim(d) {
    for (uint64_t v = 0; v < off.back(); ++v) {
      ids.push_back(v); ext.push_back(1000 + v); ts.push_back(5000 + v);
      for (uint32_t e = 0; e < d; ++e) vecs.push_back((float)v + 0.5f * (float)e);
    }
    for (uint64_t c = 0; c < cids.size(); ++c)
      for (uint32_t e = 0; e < d; ++e) cvecs.push_back(-(float)(c * d + e));
  }
  vi_status save(const std::string &dir, uint64_t shard) const {
    return shard_save_to(dir, shard, dim, (uint32_t)cids.size(), cids.data(), cvecs.data(), off.data(), ids.data(), ext.data(),
                         ts.data(), vecs.data());
  }
};

static void check_frame(const std::string &work, uint32_t dim) {
  const std::string dir = work + "/frame_" + std::to_string(dim);
  const Lists L(dim);
  CHECK(L.save(dir, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
  std::vector<uint64_t> counts;
  for (size_t i = 0; i + 1 < L.off.size(); ++i) counts.push_back(L.off[i + 1] - L.off[i]);
  const ShardPlan pl(dim, counts);
  CHECK(pl.pad == (dim == 3 ? 4u : 0u), "D %u: pad %llu", dim, (unsigned long long)pl.pad);
  CHECK(pl.data_off == 40 + 32 * 5, "D %u: data_off %llu", dim, (unsigned long long)pl.data_off);
  const Bytes raw = slurp(shard_file_path(dir, 3));
  CHECK(raw.size() == pl.total, "D %u: file of %zu bytes, plan %llu", dim, raw.size(), (unsigned long long)pl.total);
  CHECK(load<uint64_t>(raw, 0) == 3 && load<uint64_t>(raw, 8) == 1 && load<uint32_t>(raw, 16) == dim && load<uint32_t>(raw, 20) == 5 &&
            load<uint64_t>(raw, 24) == 40 && load<uint64_t>(raw, 32) == pl.data_off, "D %u: header", dim);
  ShardFile f;
  CHECK(f.open(dir, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
  CHECK(f.dim() == dim && f.num_lists() == 5, "D %u: dim %u, %u lists", dim, f.dim(), f.num_lists());
  uint64_t next = pl.data_off;
  for (uint32_t i = 0; i < f.num_lists() && i < 5; ++i) {
    const uint64_t e = 40 + 32ull * i, off = load<uint64_t>(raw, e + 16), size = load<uint64_t>(raw, e + 24);
    const ShardListView &lv = f.list(i);
    CHECK(load<uint64_t>(raw, e) == L.cids[i] && lv.centroid_id == L.cids[i], "D %u list %u: centroid id", dim, i);
    CHECK(load<uint32_t>(raw, e + 8) == counts[i] && lv.num_vectors == counts[i] && load<uint32_t>(raw, e + 12) == 0,
          "D %u list %u: count %u", dim, i, lv.num_vectors);
    CHECK(off == next && off == pl.off[i], "D %u list %u: offset %llu, want %llu", dim, i, (unsigned long long)off, (unsigned long long)next);
    CHECK(size == 4ull * dim + pl.pad + counts[i] * record_stride(dim) && size == pl.size[i], "D %u list %u: size %llu", dim, i,
          (unsigned long long)size);
    CHECK(lv.centroid == f.list(0).centroid + (off - pl.data_off) && lv.records == lv.centroid + 4ull * dim + pl.pad,
          "D %u list %u: the reader's view of the block", dim, i);
    CHECK(std::memcmp(lv.centroid, &L.cvecs[(uint64_t)i * dim], 4ull * dim) == 0, "D %u list %u: centroid vector", dim, i);
    for (uint64_t p = 0; p < pl.pad && off + 4ull * dim + p < raw.size(); ++p)
      CHECK(raw[off + 4ull * dim + p] == 0, "D %u list %u: pad byte %llu", dim, i, (unsigned long long)p);
    for (uint64_t v = 0; v < lv.num_vectors; ++v) {
      const uint8_t *r = lv.records + v * record_stride(dim);
      const uint64_t g = L.off[i] + v, want[3] = {L.ids[g], L.ext[g], L.ts[g]};
      CHECK(std::memcmp(r, want, 24) == 0 && std::memcmp(r + 24, &L.vecs[g * dim], 4ull * dim) == 0, "D %u list %u record %llu", dim,
            i, (unsigned long long)v);
    }
    next = off + size;
  }
  CHECK(next == raw.size(), "D %u: blocks end at %llu of %zu", dim, (unsigned long long)next, raw.size());
}

// append 3 records to the list of 70 and 2 to the empty list, retain everything but those five: the first file again
static void check_round_trip(const std::string &work, uint32_t dim) {
  const std::string a = work + "/trip_a_" + std::to_string(dim), b = work + "/trip_b_" + std::to_string(dim);
  const Lists L(dim);
  CHECK(L.save(a, 3) == VI_OK && make_dirs(b) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
  const Bytes first = slurp(shard_file_path(a, 3));
  const std::vector<uint64_t> cid{21, 22, 21, 22, 21}, id{300, 301, 302, 303, 304}, ext{9, 8, 7, 6, 5}, ts{1, 2, 3, 4, 5};
  const std::vector<float> vec(5 * dim, 2.25f);
  uint64_t bytes = 0, lists = 0, removed = 0;
  {
    ShardFile f;
    CHECK(f.open(a, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    CHECK(shard_update_write(f, 3, {}, 5, cid.data(), id.data(), ext.data(), ts.data(), vec.data(), shard_file_path(b, 3), &bytes, nullptr,
                             &lists) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());  // (no keep: nothing goes)
  }
  CHECK(lists == 2 && bytes == first.size() + 5 * record_stride(dim), "D %u: %llu lists, %llu bytes", dim, (unsigned long long)lists,
        (unsigned long long)bytes);
  CHECK(slurp(shard_file_path(a, 3)) == first, "D %u: the append changed its source file", dim);
  const std::string back = work + "/trip_back_" + std::to_string(dim) + ".bin";
  {
    ShardFile f;
    CHECK(f.open(b, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    CHECK(f.num_lists() == 5 && f.list(1).num_vectors == 73 && f.list(2).num_vectors == 2, "D %u: appended counts", dim);
    const uint64_t keep70[2] = {~0ull, (1ull << 6) - 1}, keep_none[1] = {0};  // positions 0..69 of 73; neither of 2
    const std::vector<const uint64_t *> keep{nullptr, keep70, keep_none, nullptr, nullptr};
    CHECK(shard_update_write(f, 3, keep, 0, nullptr, nullptr, nullptr, nullptr, nullptr, back, &bytes, &removed, nullptr) == VI_OK,
          "D %u: %s", dim, last_error_ref().c_str());  // (no rows: nothing joins)
  }
  CHECK(removed == 5 && bytes == first.size(), "D %u: %llu removed, %llu bytes", dim, (unsigned long long)removed, (unsigned long long)bytes);
  CHECK(slurp(back) == first, "D %u: append then retain does not give the first file back", dim);
}

static bool ends_with(const std::string &s, const std::string &tail) {
  return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0;
}

static const char *kInPlace = " (earlier shard files of this call are already in place: reload the index)";

// a directory with shard_0.bin and shard_1.bin ("old0", "old1"; blocked: that one is a non-empty directory instead) and
// both temporaries written ("new0", "new1") and registered
static void stage(const std::string &dir, int blocked, ShardRewriteSet *set) {
  CHECK(make_dirs(dir) == VI_OK, "%s", last_error_ref().c_str());
  for (int s = 0; s < 2; ++s) {
    const std::string path = shard_file_path(dir, s);
    if (s == blocked) {
      CHECK(make_dirs(path) == VI_OK, "%s", last_error_ref().c_str());
      spill(path + "/in_the_way", "x");
    } else {
      spill(path, "old" + std::to_string(s));
    }
    spill(set->temporary(s), "new" + std::to_string(s));
    set->add(s, 4);
  }
}

static std::string text(const std::string &path) {
  const Bytes b = slurp(path);
  return std::string(b.begin(), b.end());
}

static void check_rewrite_set(const std::string &work) {
  const auto no_temporaries = [](const std::string &dir) { return !exists(dir + "/shard_0.bin.tmp") && !exists(dir + "/shard_1.bin.tmp"); };
  {  // destroyed without commit
    const std::string dir = work + "/set_dropped";
    {
      ShardRewriteSet set(dir);
      stage(dir, -1, &set);
      CHECK(set.files() == 2 && set.bytes() == 8 && exists(set.temporary(0)) && exists(set.temporary(1)), "dropped: staged");
    }
    CHECK(no_temporaries(dir), "dropped: a temporary is left");
    CHECK(text(dir + "/shard_0.bin") == "old0" && text(dir + "/shard_1.bin") == "old1", "dropped: a final file changed");
  }
  {  // committed
    const std::string dir = work + "/set_committed";
    ShardRewriteSet set(dir);
    stage(dir, -1, &set);
    CHECK(set.commit() == VI_OK, "committed: %s", last_error_ref().c_str());
    CHECK(no_temporaries(dir), "committed: a temporary is left");
    CHECK(text(dir + "/shard_0.bin") == "new0" && text(dir + "/shard_1.bin") == "new1", "committed: a final file was not replaced");
  }
  {  // the second rename fails
    const std::string dir = work + "/set_second_fails";
    ShardRewriteSet set(dir);
    stage(dir, 1, &set);
    CHECK(set.commit() == VI_ERR_IO, "second fails: status");
    CHECK(ends_with(last_error_ref(), kInPlace) && last_error_ref().find("rename(" + dir + "/shard_1.bin.tmp): ") == 0,
          "second fails: text '%s'", last_error_ref().c_str());
    CHECK(text(dir + "/shard_0.bin") == "new0", "second fails: the first final file was not replaced");
    CHECK(no_temporaries(dir) && exists(dir + "/shard_1.bin/in_the_way"), "second fails: a temporary is left");
  }
  {  // the first rename fails
    const std::string dir = work + "/set_first_fails";
    ShardRewriteSet set(dir);
    stage(dir, 0, &set);
    CHECK(set.commit() == VI_ERR_IO, "first fails: status");
    CHECK(!ends_with(last_error_ref(), kInPlace) && last_error_ref().find("rename(" + dir + "/shard_0.bin.tmp): ") == 0,
          "first fails: text '%s'", last_error_ref().c_str());
    CHECK(text(dir + "/shard_1.bin") == "old1", "first fails: the second final file changed");
    CHECK(no_temporaries(dir), "first fails: a temporary is left");
  }
  {  // what a call checks of a file before it rewrites it
    const std::string dir = work + "/set_open";
    CHECK(Lists(3).save(dir, 0) == VI_OK, "%s", last_error_ref().c_str());
    const ShardRewriteSet set(dir);
    ShardFile f, g;
    const ShardListView *lv = nullptr;
    CHECK(set.open(0, 16, &g) == VI_ERR_INVALID_DATA && last_error_ref() == "shard_0.bin holds dimension 3", "open: '%s'",
          last_error_ref().c_str());
    CHECK(set.open(0, 3, &f) == VI_OK, "open: %s", last_error_ref().c_str());
    CHECK(set.find(f, 0, 21, 70, &lv) == VI_OK && lv == &f.list(1), "find: %s", last_error_ref().c_str());
    CHECK(set.find(f, 0, 21, 71, &lv) == VI_ERR_INVALID_DATA && last_error_ref() == "shard_0.bin no longer matches the resident list 21",
          "find, other length: '%s'", last_error_ref().c_str());
    CHECK(set.find(f, 0, 25, 0, &lv) == VI_ERR_INVALID_DATA, "find, absent list");
  }
}

// index.bin as the last pair of a set behind two shard pairs (a refine): `old_meta` is in place (blocked: a non-empty
// directory instead), `new_meta` is written beside it and registered
static void check_index_pair(const std::string &work) {
  IndexMeta old_meta, new_meta;
  old_meta.dimension = new_meta.dimension = 2;
  old_meta.centroids = {1.0f, 2.0f, 3.0f, 4.0f};
  new_meta.centroids = {1.5f, 2.5f, 3.5f, 4.5f};
  old_meta.c2s = new_meta.c2s = {0, 1};
  const auto stage_index = [&](const std::string &dir, bool blocked, ShardRewriteSet *set) {
    stage(dir, -1, set);
    if (blocked) {
      CHECK(make_dirs(dir + "/index.bin") == VI_OK, "%s", last_error_ref().c_str());
      spill(dir + "/index.bin/in_the_way", "x");
    } else {
      CHECK(index_meta_save(old_meta, dir) == VI_OK, "%s", last_error_ref().c_str());
    }
    CHECK(index_meta_replace(new_meta, dir, set) == VI_OK, "%s", last_error_ref().c_str());
  };
  const auto no_temporaries = [](const std::string &dir) {
    return !exists(dir + "/shard_0.bin.tmp") && !exists(dir + "/shard_1.bin.tmp") && !exists(dir + "/index.bin.tmp");
  };
  const auto table_in_place = [](const std::string &dir) {
    IndexMeta m;
    return index_meta_load(dir, &m) == VI_OK ? m.centroids : std::vector<float>();
  };
  {  // committed: shards in registered order, then index.bin
    const std::string dir = work + "/index_committed";
    ShardRewriteSet set(dir);
    stage_index(dir, false, &set);
    const uint64_t index_bytes = slurp(dir + "/index.bin.tmp").size();
    CHECK(set.files() == 2 && index_bytes > 0 && set.bytes() == 8 + index_bytes, "index committed: %llu files, %llu bytes",
          (unsigned long long)set.files(), (unsigned long long)set.bytes());
    CHECK(table_in_place(dir) == old_meta.centroids, "index committed: index.bin changed before the commit");
    CHECK(set.commit() == VI_OK, "index committed: %s", last_error_ref().c_str());
    CHECK(no_temporaries(dir), "index committed: a temporary is left");
    CHECK(text(dir + "/shard_0.bin") == "new0" && text(dir + "/shard_1.bin") == "new1", "index committed: a shard file was not replaced");
    CHECK(table_in_place(dir) == new_meta.centroids, "index committed: index.bin was not replaced");
  }
  {  // the rename of index.bin fails: it comes last, both shard files are in place by then and the message says so
    const std::string dir = work + "/index_rename_fails";
    ShardRewriteSet set(dir);
    stage_index(dir, true, &set);
    CHECK(set.commit() == VI_ERR_IO, "index rename fails: status");
    CHECK(ends_with(last_error_ref(), kInPlace) && last_error_ref().find("rename(" + dir + "/index.bin.tmp): ") == 0,
          "index rename fails: text '%s'", last_error_ref().c_str());
    CHECK(text(dir + "/shard_0.bin") == "new0" && text(dir + "/shard_1.bin") == "new1", "index rename fails: a shard file was not replaced");
    CHECK(no_temporaries(dir) && exists(dir + "/index.bin/in_the_way"), "index rename fails: a temporary is left");
  }
  {  // a shard rename in front of it fails: index.bin is not reached
    const std::string dir = work + "/index_not_reached";
    ShardRewriteSet set(dir);
    stage(dir, 1, &set);
    CHECK(index_meta_save(old_meta, dir) == VI_OK && index_meta_replace(new_meta, dir, &set) == VI_OK, "%s", last_error_ref().c_str());
    CHECK(set.commit() == VI_ERR_IO, "index not reached: status");
    CHECK(text(dir + "/shard_0.bin") == "new0" && table_in_place(dir) == old_meta.centroids, "index not reached: order of the renames");
    CHECK(no_temporaries(dir), "index not reached: a temporary is left");
  }
  {  // destroyed without commit
    const std::string dir = work + "/index_dropped";
    {
      ShardRewriteSet set(dir);
      stage_index(dir, false, &set);
      CHECK(exists(dir + "/index.bin.tmp"), "index dropped: staged");
    }
    CHECK(no_temporaries(dir), "index dropped: a temporary is left");
    CHECK(text(dir + "/shard_0.bin") == "old0" && text(dir + "/shard_1.bin") == "old1" && table_in_place(dir) == old_meta.centroids,
          "index dropped: a final file changed");
  }
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: shard_update_check <scratch directory>\n");
    return 2;
  }
  const std::string work = argv[1];
  for (uint32_t dim : {3u, 16u}) {
    check_frame(work, dim);
    check_round_trip(work, dim);
  }
  check_rewrite_set(work);
  check_index_pair(work);
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
