// select.hpp — the select phase of the MFMA engine (select.hip, range_select.hip) as mfma_search.hip's pipelines launch it
// on their SearchBatch (search_internal.hpp), and the constants both sides must agree on.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_index.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {

constexpr int kGroupQ = 128;            // queries per work item: 4 waves x one MFMA column tile of 32
constexpr uint32_t kDirectBlocks = 256;  // coarse tables up to here (16 384 centroids): direct records (coarse_select_direct_kernel)
constexpr uint32_t kPosBits = 26;        // candidate key = (probe rank << 26) | position in list
constexpr uint32_t kPosMask = (1u << kPosBits) - 1u;

// how the list phase was ranked, as far as the select must know
struct SelectFrame {
  uint32_t gq;      // queries per rank work item (a record tile holds 2 * gq pair records)
  bool wave_order;  // pair records in the streaming kernel's wave order (scan.hpp: seg_records), else pair order
  int approx;       // real-valued lists ranked from their hi planes: 1 queries hi + lo, 2 queries' hi plane only; 0 otherwise
  bool rank_i8;     // ranked with int8 products in the frame shifted by 127 (rank_stream.hpp)
};
// list select: one wave per query, the top-k of its probed lists in the reference's stable order.  Chooses among the
// four select_kernel instantiations (k <= 64 or <= 128; with or without the allow words of b.flt).
vi_status launch_list_select(SearchBatch &b, uint64_t k, const SelectFrame &f, const SelectOutputs &out);

// radius select (range_select.hip): one wave per query, every probed vector whose reference distance is <= radius2, in
// the reference's stable order, appended to res query chunk by query chunk (search_internal.hpp: range_result_place)
vi_status launch_range_select(SearchBatch &b, float radius2, const SelectFrame &f, RangeResult *res);

// coarse select: from the table's records (segments of segb blocks, recs group records per query; direct: the direct
// records of a table of <= kDirectBlocks blocks) to ws.probes / gorder, the per-list histogram with ws.pair_rank —
// recorded in the batch as b.pair_rank_valid — and the list phase's record offsets (ws.pair_rel / qtot)
vi_status launch_coarse_select(SearchBatch &b, uint32_t segb, uint32_t recs, bool direct);

}  // namespace vi
