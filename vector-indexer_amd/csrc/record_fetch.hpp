// record_fetch.hpp — reading records back from a resident index (record_fetch.hip): by external id, or a range of all of
// them in list order.  The contract is vi_indexer_get_records / vi_indexer_export_records in include/vi_amd.h.
//
// List order is the order the slots already lie in: lists back to back in list order, positions ascending inside a list,
// pad slots skipped.  So "the first record in list order" is the lowest slot, on a striped rank too (full_position,
// list_layout.hpp, is monotone in the local position).
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;

// Both are const on the index: they hold a FetchContext of it (device_index.hpp), never ix.stream.  on_device: the ids
// and every output are device pointers; otherwise host pointers, staged through the context.  Any output may be null.
// Arguments are checked by the caller (api.cpp); n > 0 / count > 0.
vi_status fetch_records_by_id(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool on_device, uint32_t *count,
                              float *values, uint64_t *timestamps, uint64_t *where);
vi_status export_records(const DeviceIndex &ix, uint64_t first, uint64_t count, bool on_device, uint64_t *ext_ids,
                         float *values, uint64_t *timestamps, uint64_t *where);

// The same two reads as a search by stored record needs them (similar_search.hip): every output a device pointer, the
// stored rows written straight into the search's query buffer (an absent id: a row of zeros, count 0), and with them the
// SLOT of every row — the record `where` names, 0xFFFFFFFF for an absent id.  ids_on_device: host ids are uploaded once.
// They hold a FetchContext for their duration like the public two, and leave the handle's fetch stats as they are.
vi_status resolve_records_by_id(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, uint32_t *count_dev,
                                float *values_dev, uint32_t *slot_dev);
vi_status resolve_records_by_range(const DeviceIndex &ix, uint64_t first, uint64_t count, float *values_dev, uint32_t *slot_dev);

// Makes ix.fetch's layout (device_index.hpp: FetchState) if no call has yet: the host copies of first block and length
// and the exclusive prefix of the lengths — the list-order ordinal of every list's first record — on the host and the
// device.  Synchronises st on the first call of an index, does nothing afterwards.  The one prefix of an index: exports
// and mask filters (slot_filter.hip) read ix.fetch.prefix.
vi_status ensure_fetch_layout(const DeviceIndex &ix, hipStream_t st);

}  // namespace vi
