// slot_filter.hip — builds a SlotFilter (slot_filter.hpp): from the resident timestamps of an index, from a set of
// external ids, as the intersection of two filters of one index, or from a composed expression: the AND / OR of up to
// eight terms — windows, id ranges, id sets, caller-kept masks, other filters — each negated or not.  One writer, four
// predicates.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_index.hpp"
#include "id_table.hpp"
#include "list_layout.hpp"
#include "rank_stream.hpp"
#include "record_fetch.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;

// what every filter is made of: the index's norm arrays, the filter's masked copies of them, its allow words, its count
struct FilterOut {
  const float *xnorm, *xnorm_img;
  const int *i8_norm_img;  // or null
  uint64_t *allow;
  float *xnorm_out, *xnorm_img_out;
  int *i8_out;
  unsigned long long *count;
};

// The one writer of a filter, called by a whole wave for 64-vector block `block` with lane = vector of the block and
// ok = "this slot is allowed" (false on every pad slot): lane 0 stores the wave's ballot as the block's allow word; the
// masked norms: natural order as they are, image order through image_column — the one definition of that permutation —
// with kBig / kI8PadNorm on the slots that are not allowed.  Returns the number of allowed slots of the block.
__device__ __forceinline__ uint32_t write_filter_block(const FilterOut &o, uint32_t block, uint32_t lane, bool ok) {
  const size_t base = (size_t)block * kWave;
  const uint32_t col = image_column(lane);
  const uint64_t word = __ballot(ok);
  if (lane == 0) o.allow[block] = word;
  o.xnorm_out[base + lane] = ok ? o.xnorm[base + lane] : kBig;
  o.xnorm_img_out[base + col] = ok ? o.xnorm_img[base + col] : kBig;
  if (o.i8_norm_img) o.i8_out[base + col] = ok ? o.i8_norm_img[base + col] : kI8PadNorm;
  return (uint32_t)__popcll(word);
}

// allow = stored timestamp within [ts_min, ts_max]
struct TimestampPred {
  const uint64_t *timestamps;
  uint64_t ts_min, ts_max;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) const {
    const uint64_t ts = timestamps[(size_t)block * kWave + lane];
    return resident && ts >= ts_min && ts <= ts_max;
  }
};

// allow = (external id is in the table, id_table.hpp) != exclude; the table is complete (the insert kernel ran before on the stream)
struct IdPred {
  const uint64_t *ext_ids;
  IdTable t;
  bool exclude;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) const {
    const bool member = id_table_find(t, ext_ids[(size_t)block * kWave + lane]) != kNoEntry;
    return resident && member != exclude;  // (resident first in both modes: a deny filter never allows a pad slot)
  }
};

// allow = a.allow & b.allow
struct IntersectPred {
  const uint64_t *a, *b;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) const {
    return resident && (((a[block] & b[block]) >> lane) & 1ull) != 0;
  }
};

// One term of a composed filter, as the kernel reads it: the seven kinds of vi_term_kind are four ways to look
enum : uint32_t {
  kLookRange = 0,  // lo <= p[slot] <= hi, p = the index's timestamps or external ids
  kLookTable = 1,  // the slot's external id is in t
  kLookMask = 2,   // p[ordinal] != 0, p = one byte per resident record in list order
  kLookAllow = 3,  // bit `lane` of p[block], p = the allow words of another filter
};
struct ComposeTerm {
  uint32_t look, flip;  // flip 0 / 1: negate
  uint64_t lo, hi;
  const void *p;
  IdTable t;
};

// allow = AND / OR over n terms, each flipped first where it says so.  The terms travel by value in the kernel arguments;
// n, `any` and every term's look are the same for all lanes, so the loop and its switch are wave-uniform.  A mask byte is
// read for resident slots only: the ordinal of a pad slot belongs to the next list, or lies past the mask.
struct ComposePred {
  const uint64_t *ext_ids;  // of the index (kLookTable)
  const uint64_t *prefix;   // [nlists] records before each list in list order (kLookMask), FetchState::prefix
  uint32_t n, any;
  ComposeTerm term[VI_FILTER_MAX_TERMS];
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident, uint32_t list, uint32_t b) const {
    const size_t slot = (size_t)block * kWave + lane;
    bool acc = any == 0;
    for (uint32_t i = 0; i < n; ++i) {
      const ComposeTerm &c = term[i];
      bool v;
      switch (c.look) {
        case kLookRange: {
          const uint64_t x = static_cast<const uint64_t *>(c.p)[slot];
          v = x >= c.lo && x <= c.hi;
          break;
        }
        case kLookTable:
          v = id_table_find(c.t, ext_ids[slot]) != kNoEntry;
          break;
        case kLookMask:
          v = resident && static_cast<const uint8_t *>(c.p)[prefix[list] + (uint64_t)b * kWave + lane] != 0;
          break;
        default:
          v = ((static_cast<const uint64_t *>(c.p)[block] >> lane) & 1ull) != 0;
          break;
      }
      v = v != (c.flip != 0);
      acc = any ? (acc || v) : (acc && v);
    }
    return resident && acc;  // (resident last and always: no expression admits a pad slot)
  }
};

// The walk of list_layout.hpp: a slot's allow bit is the predicate AND `position below the list length`.
template <class Pred>
__global__ void __launch_bounds__(256) slot_filter_kernel(ResidentLists L, FilterOut o, Pred pred) {
  uint32_t n = 0;
  for_each_resident_block(L, [&](uint32_t block, uint32_t lane, bool resident, uint32_t list, uint32_t b) {
    n += write_filter_block(o, block, lane, pred(block, lane, resident, list, b));
  });
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(o.count, (unsigned long long)n);
}

// The part every filter shares: the buffers of *f, the zeroed count, one launch of the kernel with `pred`, the count.
// The index's own statistics — xmax2, rho2_max, the centring mu, mean_* — are left as they are and keep setting the rank
// margins and the rank mode of a filtered search: a filter only removes candidates, it never widens a bound, so the
// margins of the full index remain valid upper bounds for every subset of it — whatever predicate chose the subset.
// (*f may be a finished filter of ix: DevBuf::reserve keeps a buffer that is large enough, so writing it again allocates
// nothing.  nflags id tables: the two flag words of each, flags_dev[i], come back into flags_host[i] with the count.)
struct TableFlags { uint32_t w[2]; };
template <class Pred>
vi_status build_filter(const DeviceIndex &ix, const Pred &pred, SlotFilter *f, const uint32_t *const *flags_dev = nullptr,
                       TableFlags *flags_host = nullptr, uint32_t nflags = 0) {
  const uint64_t nb = ix.lists.nblocks, nslots = nb * kWave;
  f->owner_serial = ix.serial;
  VI_TRY(f->allow.reserve(std::max<uint64_t>(1, nb)));
  VI_TRY(f->xnorm.reserve(std::max<uint64_t>(1, nslots)));
  VI_TRY(f->xnorm_img.reserve(std::max<uint64_t>(1, nslots)));
  if (ix.i8_norm_img.p) VI_TRY(f->i8_norm_img.reserve(std::max<uint64_t>(1, nslots)));
  DevBuf<unsigned long long> &cnt = f->count;
  VI_TRY(cnt.reserve(1));
  hipStream_t st = ix.stream;
  VI_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), st));
  VI_HIP(hipMemsetAsync(f->allow.p, 0, std::max<uint64_t>(1, nb) * sizeof(uint64_t), st));
  if (nb && ix.nlists) {
    ResidentLists L{ix.list_first_block.p, ix.list_len.p, (uint32_t)ix.nlists};
    FilterOut o{ix.xnorm.p, ix.xnorm_img.p, ix.i8_norm_img.p, f->allow.p, f->xnorm.p, f->xnorm_img.p, f->i8_norm_img.p, cnt.p};
    hipLaunchKernelGGL(slot_filter_kernel<Pred>, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, L, o, pred);
    VI_HIP(hipGetLastError());
  }
  unsigned long long n = 0;
  VI_HIP(hipMemcpyAsync(&n, cnt.p, sizeof(n), hipMemcpyDeviceToHost, st));
  for (uint32_t i = 0; i < nflags; ++i)
    VI_HIP(hipMemcpyAsync(flags_host[i].w, flags_dev[i], sizeof(TableFlags), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  f->num_allowed = n;
  return VI_OK;
}

}  // namespace

vi_status slot_filter_timestamps(const DeviceIndex &ix, uint64_t ts_min, uint64_t ts_max, SlotFilter *f) {
  if (!ix.timestamps.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no timestamps");
  VI_HIP(hipSetDevice(ix.device));
  return build_filter(ix, TimestampPred{ix.timestamps.p, ts_min, ts_max}, f);
}

vi_status slot_filter_ids(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, bool exclude,
                          SlotFilter *f) {
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  if (n > (1ull << 40)) return fail(VI_ERR_INVALID_INPUT, "id set of %llu ids is too large", (unsigned long long)n);
  VI_HIP(hipSetDevice(ix.device));
  IdSetBuffers set;  // lives until this function returns
  IdTable t;
  VI_TRY(id_set_build(set, ids, n, ids_on_device, 0, ix.stream, &t));
  TableFlags fl{{0, 0}};
  const uint32_t *fl_dev = set.flags.p;
  VI_TRY(build_filter(ix, IdPred{ix.ext_ids.p, t, exclude}, f, &fl_dev, &fl, 1));
  return id_set_check(fl.w, t, n, "id filter");
}

vi_status slot_filter_intersect(const DeviceIndex &ix, const SlotFilter &a, const SlotFilter &b, SlotFilter *f) {
  if (a.owner_serial != ix.serial || b.owner_serial != ix.serial)
    return fail(VI_ERR_INVALID_INPUT, "the filter was made from another indexer (or before this one was rebuilt)");
  VI_HIP(hipSetDevice(ix.device));
  return build_filter(ix, IntersectPred{a.allow.p, b.allow.p}, f);
}

vi_status slot_filter_compose(const DeviceIndex &ix, bool any, const vi_filter_term *terms, uint32_t n,
                              const SlotFilter *const *filters, SlotFilter *f) {
  // ---- what depends on the index, before any device work ----
  for (uint32_t i = 0; i < n; ++i) {
    const vi_filter_term &t = terms[i];
    const bool ids = t.kind == VI_TERM_IDS || t.kind == VI_TERM_IDS_DEVICE;
    if (t.kind == VI_TERM_TIMESTAMPS && !ix.timestamps.p)
      return fail(VI_ERR_INVALID_INPUT, "term %u: this index keeps no timestamps", i);
    if ((ids || t.kind == VI_TERM_ID_RANGE) && !ix.ext_ids.p)
      return fail(VI_ERR_INVALID_INPUT, "term %u: this index keeps no external ids", i);
    if (ids && t.n > (1ull << 40))
      return fail(VI_ERR_INVALID_INPUT, "term %u: id set of %llu ids is too large", i, (unsigned long long)t.n);
    if ((t.kind == VI_TERM_MASK || t.kind == VI_TERM_MASK_DEVICE) && t.n != ix.nvec_resident)
      return fail(VI_ERR_INVALID_INPUT, "term %u: a mask of %llu bytes for %llu resident records", i, (unsigned long long)t.n,
                  (unsigned long long)ix.nvec_resident);
  }
  VI_HIP(hipSetDevice(ix.device));
  hipStream_t st = ix.stream;
  // ---- the terms as the kernel reads them; tables and uploads live until this function returns ----
  IdSetBuffers sets[VI_FILTER_MAX_TERMS];
  DevBuf<uint8_t> masks[VI_FILTER_MAX_TERMS];
  const uint32_t *flags_dev[VI_FILTER_MAX_TERMS];
  TableFlags flags_host[VI_FILTER_MAX_TERMS] = {};
  uint32_t table_term[VI_FILTER_MAX_TERMS], ntables = 0;
  ComposePred pred{};
  pred.ext_ids = ix.ext_ids.p;
  pred.n = n;
  pred.any = any ? 1u : 0u;
  for (uint32_t i = 0; i < n; ++i) {
    const vi_filter_term &t = terms[i];
    ComposeTerm &c = pred.term[i];
    c.flip = t.negate;
    switch (t.kind) {
      case VI_TERM_TIMESTAMPS:
      case VI_TERM_ID_RANGE:
        c.look = kLookRange;
        c.p = t.kind == VI_TERM_TIMESTAMPS ? ix.timestamps.p : ix.ext_ids.p;
        c.lo = t.lo;
        c.hi = t.hi;
        break;
      case VI_TERM_IDS:
      case VI_TERM_IDS_DEVICE:
        c.look = kLookTable;
        VI_TRY(id_set_build(sets[ntables], static_cast<const uint64_t *>(t.data), t.n, t.kind == VI_TERM_IDS_DEVICE, 0, st, &c.t));
        flags_dev[ntables] = sets[ntables].flags.p;
        table_term[ntables++] = i;
        break;
      case VI_TERM_MASK:
      case VI_TERM_MASK_DEVICE:
        c.look = kLookMask;
        c.p = t.data;
        if (t.kind == VI_TERM_MASK && t.n) {
          VI_TRY(masks[i].reserve(t.n));
          VI_HIP(hipMemcpyAsync(masks[i].p, t.data, t.n, hipMemcpyHostToDevice, st));
          c.p = masks[i].p;
        }
        if (!pred.prefix) {
          VI_TRY(ensure_fetch_layout(ix, st));
          pred.prefix = ix.fetch.prefix.p;
        }
        break;
      default:  // VI_TERM_FILTER
        c.look = kLookAllow;
        c.p = filters[i]->allow.p;
        break;
    }
  }
  VI_TRY(build_filter(ix, pred, f, flags_dev, flags_host, ntables));
  for (uint32_t j = 0; j < ntables; ++j)
    VI_TRY(id_set_check(flags_host[j].w, pred.term[table_term[j]].t, terms[table_term[j]].n, "composed filter"));
  return VI_OK;
}

}  // namespace vi
