// shard_upsert_check.cpp — host checks of shard_update_write of csrc/shards.cpp, the writer that drops and appends in one
// image, with both halves, with either alone and with "nothing goes" said both ways (compiled together with shards.cpp and run by test_shard_upsert_cpu.py, in the scratch directory given as
// argv[1]): prints one line per failed check and exits non-zero if there was one.
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

// lists of 5, 70, 0, 1 and 130 records, centroid ids 20..24; record v carries id v, external id 1000 + v, timestamp
// 5000 + v and the vector (v, v + 0.5, ...)
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

// The call of every check.  List 20: untouched.  21 (70 records): loses position 5, receives 1: its length stays, every
// later record moves.  22 (empty): receives 3: all new.  23 (1 record): loses it, receives nothing: emptied.  24 (130):
// loses its first 64, receives 2.
struct Call {
  uint64_t keep21[2] = {~0ull & ~(1ull << 5), (1ull << 6) - 1}, keep23[1] = {0}, keep24[3] = {0, ~0ull, 3};
  std::vector<const uint64_t *> keep{nullptr, keep21, nullptr, keep23, keep24};
  std::vector<uint64_t> cid{22, 24, 21, 22, 24, 22}, id{300, 301, 302, 303, 304, 305}, ext{9, 8, 7, 6, 5, 4}, ts{1, 2, 3, 4, 5, 6};
  std::vector<float> vec;
  explicit Call(uint32_t dim) {
    for (uint64_t i = 0; i < cid.size() * dim; ++i) vec.push_back(2.25f + (float)i);
  }
  vi_status write(const ShardFile &f, const std::string &out, uint64_t *bytes, uint64_t *removed, uint64_t *lists) const {
    return shard_update_write(f, 3, keep, cid.size(), cid.data(), id.data(), ext.data(), ts.data(), vec.data(), out, bytes, removed, lists);
  }
};

static uint64_t meta_word(const ShardListView &lv, uint32_t dim, uint32_t v, int word) {
  uint64_t x;
  std::memcpy(&x, lv.records + (uint64_t)v * record_stride(dim) + 8 * word, 8);
  return x;
}

static void check_update(const std::string &work, uint32_t dim) {
  const std::string a = work + "/upd_a_" + std::to_string(dim), mid = work + "/upd_mid_" + std::to_string(dim),
                    pair = work + "/upd_pair_" + std::to_string(dim), one = work + "/upd_one_" + std::to_string(dim);
  const Lists L(dim);
  const Call c(dim);
  CHECK(L.save(a, 3) == VI_OK && make_dirs(mid) == VI_OK && make_dirs(pair) == VI_OK && make_dirs(one) == VI_OK, "D %u: %s", dim,
        last_error_ref().c_str());
  const Bytes first = slurp(shard_file_path(a, 3));
  uint64_t bytes = 0, removed = 0, lists = 0;
  {  // two executions, one after the other: drop only (no rows), then append only (no keep) to the file that left
    ShardFile f, g;
    CHECK(f.open(a, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    CHECK(shard_update_write(f, 3, c.keep, 0, nullptr, nullptr, nullptr, nullptr, nullptr, shard_file_path(mid, 3), nullptr, &removed,
                             nullptr) == VI_OK && removed == 1 + 1 + 64, "D %u: retain: %s", dim, last_error_ref().c_str());
    CHECK(g.open(mid, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    CHECK(shard_update_write(g, 3, {}, c.cid.size(), c.cid.data(), c.id.data(), c.ext.data(), c.ts.data(), c.vec.data(),
                             shard_file_path(pair, 3), nullptr, nullptr, nullptr) == VI_OK, "D %u: append: %s", dim, last_error_ref().c_str());
  }
  {  // ... and the one that does both
    ShardFile f;
    CHECK(f.open(a, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    removed = 0;
    CHECK(c.write(f, shard_file_path(one, 3), &bytes, &removed, &lists) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
    CHECK(c.write(f, shard_file_path(one, 3) + ".again", nullptr, nullptr, nullptr) == VI_OK, "D %u: optional outputs: %s", dim,
          last_error_ref().c_str());
  }
  const Bytes got = slurp(shard_file_path(one, 3));
  CHECK(got == slurp(shard_file_path(pair, 3)), "D %u: update differs from retain followed by append", dim);
  CHECK(got == slurp(shard_file_path(one, 3) + ".again"), "D %u: two equal calls differ", dim);
  CHECK(removed == 66 && lists == 4 && bytes == got.size() && bytes == first.size() + (6 - 66) * record_stride(dim),
        "D %u: %llu removed, %llu lists, %llu bytes", dim, (unsigned long long)removed, (unsigned long long)lists, (unsigned long long)bytes);
  CHECK(slurp(shard_file_path(a, 3)) == first, "D %u: the update changed its source file", dim);
  ShardFile f;
  CHECK(f.open(one, 3) == VI_OK && f.num_lists() == 5, "D %u: %s", dim, last_error_ref().c_str());
  if (f.num_lists() != 5) return;
  const uint32_t want[5] = {5, 70, 3, 0, 68};
  for (uint32_t i = 0; i < 5; ++i)
    CHECK(f.list(i).num_vectors == want[i] && f.list(i).centroid_id == L.cids[i], "D %u list %u: %u records", dim, i, f.list(i).num_vectors);
  if (f.list(1).num_vectors != 70 || f.list(2).num_vectors != 3 || f.list(4).num_vectors != 68) return;
  // unchanged length: positions 0..4 as they were, 5..68 one further on, the new record last
  for (uint32_t v = 0; v < 69; ++v)
    CHECK(meta_word(f.list(1), dim, v, 0) == 5 + v + (v >= 5), "D %u list 21 position %u: id %llu", dim, v,
          (unsigned long long)meta_word(f.list(1), dim, v, 0));
  CHECK(meta_word(f.list(1), dim, 69, 0) == 302 && meta_word(f.list(1), dim, 69, 1) == 7 && meta_word(f.list(1), dim, 69, 2) == 3,
        "D %u list 21: the new record", dim);
  CHECK(std::memcmp(f.list(1).records + 69 * record_stride(dim) + 24, &c.vec[2 * dim], 4ull * dim) == 0, "D %u list 21: the new vector", dim);
  // all new: call order
  CHECK(meta_word(f.list(2), dim, 0, 0) == 300 && meta_word(f.list(2), dim, 1, 0) == 303 && meta_word(f.list(2), dim, 2, 0) == 305,
        "D %u list 22: call order", dim);
  // kept run, then the new records
  CHECK(meta_word(f.list(4), dim, 0, 0) == 76 + 64 && meta_word(f.list(4), dim, 65, 0) == 76 + 129 && meta_word(f.list(4), dim, 66, 0) == 301 &&
            meta_word(f.list(4), dim, 67, 0) == 304, "D %u list 24: kept records, then new ones", dim);
}

// "nothing goes" said both ways: an empty keep, and num_lists() null entries
static void check_no_keep(const std::string &work, uint32_t dim) {
  const std::string a = work + "/nokeep_a_" + std::to_string(dim), out = work + "/nokeep_" + std::to_string(dim);
  const Lists L(dim);
  const Call c(dim);
  CHECK(L.save(a, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
  const Bytes first = slurp(shard_file_path(a, 3));
  ShardFile f;
  CHECK(f.open(a, 3) == VI_OK, "D %u: %s", dim, last_error_ref().c_str());
  const std::vector<const uint64_t *> empty, nulls(f.num_lists(), nullptr);
  uint64_t bytes[2] = {0, 0}, removed[2] = {7, 7}, lists[2] = {0, 0};
  CHECK(shard_update_write(f, 3, empty, c.cid.size(), c.cid.data(), c.id.data(), c.ext.data(), c.ts.data(), c.vec.data(), out + ".empty",
                           &bytes[0], &removed[0], &lists[0]) == VI_OK, "D %u: empty keep: %s", dim, last_error_ref().c_str());
  CHECK(shard_update_write(f, 3, nulls, c.cid.size(), c.cid.data(), c.id.data(), c.ext.data(), c.ts.data(), c.vec.data(), out + ".nulls",
                           &bytes[1], &removed[1], &lists[1]) == VI_OK, "D %u: null keep entries: %s", dim, last_error_ref().c_str());
  const Bytes got = slurp(out + ".empty");
  CHECK(got.size() == first.size() + 6 * record_stride(dim) && got == slurp(out + ".nulls"), "D %u: an empty keep and null entries differ", dim);
  for (int i = 0; i < 2; ++i)
    CHECK(removed[i] == 0 && lists[i] == 3 && bytes[i] == got.size(), "D %u: %llu removed, %llu lists, %llu bytes", dim,
          (unsigned long long)removed[i], (unsigned long long)lists[i], (unsigned long long)bytes[i]);
  // ... and with nothing to join either: the file again
  CHECK(shard_update_write(f, 3, empty, 0, nullptr, nullptr, nullptr, nullptr, nullptr, out + ".same", nullptr, nullptr, &lists[0]) == VI_OK &&
            lists[0] == 0 && slurp(out + ".same") == first, "D %u: nothing goes, nothing joins: %s", dim, last_error_ref().c_str());
}

static void check_failures(const std::string &work) {
  const uint32_t dim = 3;
  const std::string a = work + "/fail_a", blocked = work + "/fail_blocked";
  const Lists L(dim);
  Call c(dim);
  CHECK(L.save(a, 3) == VI_OK && make_dirs(shard_file_path(blocked, 3)) == VI_OK, "%s", last_error_ref().c_str());
  CHECK(shard_image_write(shard_file_path(blocked, 3) + "/in_the_way", (const uint8_t *)"x", 1, false) == VI_OK, "%s", last_error_ref().c_str());
  const Bytes first = slurp(shard_file_path(a, 3));
  ShardFile f;
  CHECK(f.open(a, 3) == VI_OK, "%s", last_error_ref().c_str());
  {  // the rename fails: the temporary goes, what is in the way stays
    ShardRewriteSet set(blocked);
    uint64_t bytes = 0;
    CHECK(c.write(f, set.temporary(3), &bytes, nullptr, nullptr) == VI_OK && exists(set.temporary(3)), "%s", last_error_ref().c_str());
    set.add(3, bytes);
    CHECK(set.commit() == VI_ERR_IO && last_error_ref().find("rename(" + blocked + "/shard_3.bin.tmp): ") == 0, "rename: '%s'",
          last_error_ref().c_str());
    CHECK(!exists(set.temporary(3)) && exists(shard_file_path(blocked, 3) + "/in_the_way"), "rename: a temporary is left");
  }
  {  // a failure before the renames: a set that is dropped takes its temporary along
    const std::string dir = work + "/fail_dropped";
    CHECK(make_dirs(dir) == VI_OK, "%s", last_error_ref().c_str());
    {
      ShardRewriteSet set(dir);
      uint64_t bytes = 0;
      CHECK(c.write(f, set.temporary(3), &bytes, nullptr, nullptr) == VI_OK && exists(set.temporary(3)), "%s", last_error_ref().c_str());
      set.add(3, bytes);
    }
    CHECK(!exists(dir + "/shard_3.bin.tmp") && !exists(dir + "/shard_3.bin"), "dropped: a file is left");
  }
  {  // refusals write nothing
    const std::string out = work + "/fail_out.bin";
    uint64_t removed = 7;
    c.cid[3] = 99;
    CHECK(c.write(f, out, nullptr, &removed, nullptr) == VI_ERR_NOT_FOUND && last_error_ref() == "Centroid 99 not found" && !exists(out),
          "unknown centroid: '%s'", last_error_ref().c_str());
    c.cid[3] = 22;
    c.keep.pop_back();
    CHECK(c.write(f, out, nullptr, nullptr, nullptr) == VI_ERR_OTHER && !exists(out), "keep entries: '%s'", last_error_ref().c_str());
  }
  CHECK(slurp(shard_file_path(a, 3)) == first, "a failed update changed its source file");
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: shard_upsert_check <scratch directory>\n");
    return 2;
  }
  const std::string work = argv[1];
  for (uint32_t dim : {3u, 16u}) check_update(work, dim);
  for (uint32_t dim : {3u, 16u}) check_no_keep(work, dim);
  check_failures(work);
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
