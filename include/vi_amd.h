/*
 * vi_amd.h — C ABI of libvi_amd.so, the MI355X-native (gfx950) implementation of the
 * distance hot path of NirajNair/vector-indexer.
 *
 * The reference is a pure-Rust crate with no FFI seam; the entry points below are the
 * calls its Rust host code (src/api.rs, src/ivf_index.rs, src/kmeans.rs) would bind
 * through `extern "C"` to move that path onto the GPU.  Each declaration cites the
 * reference interface it replaces (file:line relative to the reference repo).  The Rust
 * and Python bindings a maintainer would add are shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + sizes, caller-allocated outputs, no exceptions/panics cross the ABI
 *   - every function returns a vi_status; vi_last_error() gives the thread-local message
 *   - vi_status mirrors the std::io::ErrorKind values the reference returns
 *   - all arrays are row-major contiguous, f32 / u64 / i64 little-endian host memory unless a
 *     parameter says "device"
 *   - entry points taking DEVICE pointers run on a library-owned stream created with
 *     hipStreamDefault, i.e. ordered after work already queued on the legacy null stream (where
 *     PyTorch-ROCm launches by default); callers using other streams must synchronise first.
 *     Every entry point returns only after its device work has completed.
 *   - a vi_indexer handle may be shared by several host threads: up to 4 searches run concurrently on one handle (each
 *     call holds its own stream and workspace; further callers wait), as the reference's &self search does
 *     (ivf_index_tests.rs:768-807)
 */
#ifndef VI_AMD_H
#define VI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VI_AMD_ABI_VERSION 2

typedef enum vi_status {
  VI_OK = 0,
  VI_ERR_INVALID_INPUT = 1, /* io::ErrorKind::InvalidInput (api.rs:116-134,192-201; ivf_index.rs:197-202) */
  VI_ERR_NOT_FOUND = 2,     /* io::ErrorKind::NotFound (missing index.bin; shards.rs:257-265) */
  VI_ERR_INVALID_DATA = 3,  /* io::ErrorKind::InvalidData (shards.rs:215-231,310-316) */
  VI_ERR_OTHER = 4,         /* io::ErrorKind::Other (bincode wrap ivf_index.rs:280,312; shards.rs:193-213) */
  VI_ERR_IO = 5,            /* any other raw std::fs error */
  VI_ERR_PANIC = 6,         /* the reference would panic here (NaN in partial_cmp().unwrap(), ivf_index.rs:215,265) */
  VI_ERR_DEVICE = 7         /* no MI355X / HIP failure: the product never falls back to the CPU */
} vi_status;

/* Thread-local, NUL-terminated description of the last failure on this thread. */
const char *vi_last_error(void);
uint32_t vi_abi_version(void);
/* Number of visible HIP devices (0 on a CPU-only box; never an error). */
int vi_device_count(void);

/* ---- heuristics ------------------------------------------------------------------- */
/* replaces calculate_num_clusters — src/utils.rs:9-16 */
uint64_t vi_calculate_num_clusters(uint64_t num_vectors);
/* replaces calculate_max_iterations — src/utils.rs:18-26 */
uint64_t vi_calculate_max_iterations(uint64_t num_vectors);
/* mini-batch size rule — src/kmeans.rs:83 */
uint64_t vi_minibatch_size(uint64_t num_vectors);

/* ---- distance kernels ------------------------------------------------------------- */
typedef enum vi_sum_order {
  VI_ORDER_SCALAR = 0, /* euclidean_distance_squared — src/utils.rs:28-30 (search path) */
  VI_ORDER_LANES = 1   /* compute_distance_simd — src/kmeans.rs:377-419 (k-means path) */
} vi_sum_order;

/* out[i] = squared L2 between a[i,:] and b[i,:], n pairs of dimension d, computed on the
 * GPU with the reference's exact f32 summation order (bit-identical results). */
vi_status vi_l2sq_pairs(const float *a, const float *b, uint64_t n, uint32_t d, vi_sum_order order,
                        float *out);

/* ---- k-means ---------------------------------------------------------------------- */
typedef enum vi_assign_mode {
  /* reference behaviour: k <= 100 brute force, k > 100 hierarchical (approximate)
   * — assign_points_simd_parallel, src/kmeans.rs:445-459 */
  VI_ASSIGN_REFERENCE = 0,
  /* extension: exact nearest centroid for every k (MFMA -2·X·Cᵀ+‖c‖² filter + exact-order
   * re-check); equals assign_points_brute_force (src/kmeans.rs:462-470) bit for bit */
  VI_ASSIGN_EXACT = 1
} vi_assign_mode;

/* replaces assign_points_simd_parallel(&X,&C,&mut labels,seed) — src/kmeans.rs:445-450.
 * labels: n u64 (Rust usize).  dist_out (optional, n f32): lane-order distance to the label. */
vi_status vi_assign(const float *X, uint64_t n, uint32_t d, const float *C, uint64_t k, uint64_t seed,
                    vi_assign_mode mode, uint64_t *labels, float *dist_out);

/* Same assignment with DEVICE pointers (X_dev n x d, C_dev k x d, labels_dev n u32) on HIP device
 * `device`: nothing crosses PCIe.  stats (optional; zero-initialise it: it carries one optional input) reports the MFMA
 * filter's kernel time and how many rows needed the exact-order re-check. */
typedef struct vi_assign_stats {
  uint64_t n, k;
  uint64_t ambiguous_rows; /* rows re-evaluated exactly (VI_ASSIGN_EXACT / brute-force path) */
  uint32_t used_mfma;      /* 1 when the MFMA tiers ran (bf16 x 3, then f32 on the rows that one leaves ambiguous),
                              0 for the exact-order scan kernel alone */
  float ms_total;          /* wall time of the call incl. the exact re-check */
  float ms_filter;         /* HIP-event time of the first-tier MFMA kernel alone */
  uint64_t tier1_rows;     /* rows the first (bf16 x 3) tier left undecided; ambiguous_rows of them also failed the f32 tier */
  /* in (optional, zero = off): device buffer of ambiguous_cap u32 that receives the row indices counted in tier1_rows
   * (a superset of the rows re-evaluated exactly) — lets a test check exactly the rows the margins did not decide */
  uint32_t *ambiguous_rows_dev;
  uint64_t ambiguous_cap;
} vi_assign_stats;
vi_status vi_assign_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, const float *C_dev,
                           uint64_t k, uint64_t seed, vi_assign_mode mode, uint32_t *labels_dev,
                           vi_assign_stats *stats);

/* replaces run_kmeans_mini_batch(&data,k,max_iters,early_stop_threshold,seed)
 * — src/kmeans.rs:64-70.  early_stop_threshold < 0 means None (=> 1e-4).
 * centroids_out: k x d, labels_out: n.  iters_run optional.
 * Empty input => VI_ERR_INVALID_INPUT (kmeans.rs:72-77). */
vi_status vi_kmeans_mini_batch(const float *X, uint64_t n, uint32_t d, uint64_t k, uint64_t max_iters,
                               float early_stop_threshold, uint64_t seed, vi_assign_mode mode,
                               float *centroids_out, uint64_t *labels_out, uint64_t *iters_run);

/* replaces run_kmeans_parallel(...) — src/kmeans.rs:15-21 (same shape as above). */
vi_status vi_kmeans_parallel(const float *X, uint64_t n, uint32_t d, uint64_t k, uint64_t max_iters,
                             float early_stop_threshold, uint64_t seed, vi_assign_mode mode,
                             float *centroids_out, uint64_t *labels_out, uint64_t *iters_run);

/* The same two entry points with DEVICE pointers on HIP device `device` (X_dev n x d, centroids_dev k x d, labels_dev n
 * u32; labels_dev may be NULL for vi_kmeans_mini_batch_device to skip the final assignment): the points never cross PCIe
 * — config C3's 5 GB would take longer to upload than to assign. */
vi_status vi_kmeans_mini_batch_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, uint64_t k,
                                      uint64_t max_iters, float early_stop_threshold, uint64_t seed, vi_assign_mode mode,
                                      float *centroids_dev, uint32_t *labels_dev, uint64_t *iters_run);
vi_status vi_kmeans_parallel_device(int32_t device, const float *X_dev, uint64_t n, uint32_t d, uint64_t k,
                                    uint64_t max_iters, float early_stop_threshold, uint64_t seed, vi_assign_mode mode,
                                    float *centroids_dev, uint32_t *labels_dev, uint64_t *iters_run);

/* ---- k-means with the points SHARDED over the GPUs of a node (one process per GPU; extension: the reference has no
 *      distributed mode).  The collectives stay in the caller (RCCL through torch.distributed, as for search):
 *
 *   training   k-means++ seeding, the mini-batches and the empty-cluster re-seeds read only the rows the rand stream
 *              names (50 000 + k + iterations x (batch + empty clusters) of them).  vi_kmeans_mini_batch_train /
 *              vi_kmeans_pp_init run that loop over a vi_row_source: the caller's fetch_rows gathers the named rows
 *              from their owner ranks (a collective every rank enters with the same row list: every rank replays the
 *              same rand 0.8.5 stream; rank 0's centroids are broadcast afterwards, which pins them bit for bit).
 *   assignment vi_assign_device on every rank's own points (labels stay local) — the O(N k D) part.
 *   Lloyd      per iteration: vi_assign_device, vi_kmeans_partial_sums_device (this rank's sums k x d and counts k),
 *              all-reduce(sum) of both, vi_kmeans_finish_update_device (means, RMS movement, empty clusters);
 *              empty clusters are re-seeded with rows drawn from a vi_rng stream every rank replays (same seed, same
 *              draws) and fetched like the training rows.
 *              Sums combined over ranks associate differently from the reference's single pass: centroids agree
 *              to rounding (compare with a tolerance), labels of the first iteration exactly. */
typedef struct vi_row_source {
  void *ctx;
  /* out_dev[i, 0..d) = data row global_rows[i] for i < n_rows, complete on return; 0 = ok */
  int (*fetch_rows)(void *ctx, const uint64_t *global_rows, uint64_t n_rows, float *out_dev);
} vi_row_source;
/* the loop of run_kmeans_mini_batch (src/kmeans.rs:64-142) without its final assignment; centroids_dev k x d */
vi_status vi_kmeans_mini_batch_train(int32_t device, const vi_row_source *rows, uint64_t n_global, uint32_t d, uint64_t k,
                                     uint64_t max_iters, float early_stop_threshold, uint64_t seed,
                                     float *centroids_dev, uint64_t *iters_run);
/* kmeans_plus_plus_init (src/kmeans.rs:154-310) alone (the start of run_kmeans_parallel) */
vi_status vi_kmeans_pp_init(int32_t device, const vi_row_source *rows, uint64_t n_global, uint32_t d, uint64_t k,
                            uint64_t seed, float *centroids_dev);
/* update_centroids_parallel (src/kmeans.rs:674-719), this rank's share: sums_dev k x d f32, counts_dev k u32 */
vi_status vi_kmeans_partial_sums_device(int32_t device, const float *X_dev, uint64_t n_local, uint32_t d,
                                        const uint32_t *labels_dev, uint64_t k, float *sums_dev, uint32_t *counts_dev);
/* ... and what follows the all-reduce: C_new = sums / counts (zero rows for empty clusters), *delta_out =
 * compute_centroid_delta(C_new, C_prev) (src/kmeans.rs:334-351), empty_out (optional, host, k u32) / *n_empty = the
 * clusters handle_empty_clusters (src/kmeans.rs:313-331) re-seeds, ascending */
vi_status vi_kmeans_finish_update_device(int32_t device, const float *sums_dev, const uint32_t *counts_dev, uint64_t k,
                                         uint32_t d, const float *C_prev_dev, float *C_new_dev, float *delta_out,
                                         uint32_t *empty_out, uint64_t *n_empty);
/* compute_centroid_delta (src/kmeans.rs:334-351) of two device tables (after the re-seed, as the reference orders it) */
vi_status vi_kmeans_centroid_delta_device(int32_t device, const float *C_new_dev, const float *C_prev_dev, uint64_t k,
                                          uint32_t d, float *delta_out);
/* rand 0.8.5 StdRng::seed_from_u64(seed) and Rng::gen_range(low..high) on usize — the stream the reference draws
 * re-seed rows from (src/kmeans.rs:31,325) */
typedef struct vi_rng vi_rng;
vi_rng *vi_rng_seed_from_u64(uint64_t seed);
uint64_t vi_rng_gen_range(vi_rng *rng, uint64_t low, uint64_t high);
void vi_rng_free(vi_rng *rng);

/* ---- shard files ------------------------------------------------------------------ */
/* replaces Shard::save_to(&self, shards_dir) — src/shards.rs:68-177.  Lists flattened:
 * list i owns vectors [list_off[i], list_off[i+1]).  Byte-identical file layout. */
vi_status vi_shard_save_to(const char *shards_dir, uint64_t shard_id, uint32_t dim, uint32_t num_lists,
                           const uint64_t *centroid_ids, const float *centroid_vecs,
                           const uint64_t *list_off, const uint64_t *ids, const uint64_t *ext_ids,
                           const uint64_t *timestamps, const float *vecs);

/* replaces Shard::get_centroid_vectors_from(shards_dir, shard_id, &centroid_ids)
 * — src/shards.rs:188-349.  Call once with the output buffers NULL to get counts[i]
 * (vectors in requested list i) and *dim_out, then again with buffers:
 * centroid_out n_req x dim; metas_out 3 u64 {id, external_id, timestamp} per vector;
 * vecs_out dim f32 per vector, in request order. */
vi_status vi_shard_get_centroid_vectors_from(const char *shards_dir, uint64_t shard_id,
                                             const uint64_t *centroid_ids, uint64_t n_req,
                                             uint32_t *dim_out, uint64_t *counts, float *centroid_out,
                                             uint64_t *metas_out, float *vecs_out);

/* extension: append n_add records to lists of an existing shard file (the file half of vi_indexer_add_records on its own;
 * needs no GPU).  Record i — internal id ids[i], external id ext_ids[i], stored timestamp timestamps[i], vector
 * vecs[i, 0..dim) with dim read from the file — goes to the list of centroid_ids[i], behind the list's old records and
 * behind the records of this call named before it.  The result is byte-identical to vi_shard_save_to of the merged lists;
 * old records are copied verbatim.  The new file is written beside the old one under a temporary name and renamed over it
 * when complete.  A centroid id the shard does not hold: VI_ERR_NOT_FOUND, and the file is untouched.  A file that cannot
 * be read: the errors of vi_shard_get_centroid_vectors_from.  n_add == 0 leaves the file as it is. */
vi_status vi_shard_append_to(const char *shards_dir, uint64_t shard_id, uint64_t n_add, const uint64_t *centroid_ids,
                             const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps,
                             const float *vecs);

/* ---- VectorIndexer (src/api.rs) ---------------------------------------------------- */
/* mirrors VectorIndexerConfig — src/api.rs:8-54 — plus clearly marked extensions */
typedef struct vi_config {
  uint32_t dimension;
  const char *index_dir;    /* NULL => "index"  (api.rs:36) */
  const char *shards_dir;   /* NULL => "shards" (api.rs:37) */
  uint64_t default_k;       /* 10      (api.rs:38) */
  uint64_t default_n_probe; /* 20      (api.rs:39) */
  uint64_t max_k;           /* 10 000  (api.rs:40) */
  uint64_t max_n_probe;     /* 10 000  (api.rs:41) */
  /* --- extensions (all zero = reference behaviour) --- */
  uint64_t nlist_override;  /* 0 => calculate_num_clusters(N) (ivf_index.rs:59) */
  uint64_t seed;            /* 0 => 42 (api.rs:143,183) */
  int32_t assign_mode;      /* vi_assign_mode for the build's final assignment */
  int32_t device;           /* HIP device ordinal */
  /* multi-GPU partition: this process keeps a stripe of every inverted list resident (block b of 64 vectors
   * lives on rank b % world_size; coarse table replicated).  world_size 0/1 => everything. */
  int32_t rank;
  int32_t world_size;
  uint64_t now_secs;        /* 0 => wall clock; else value used for timestamp==0 records
                               (vector_store.rs:36-40) */
  /* multi-GPU partition rule: 0 = stripes (above; balances whatever the skew); 1 = shard placement: whole shard
   * files — the reference's super-centroid grouping of lists, src/ivf_index.rs:104-164 — are dealt to the ranks greedily
   * by bytes (largest first to the least loaded rank), a list is scanned by the one rank that holds its shard */
  int32_t placement;
  int32_t reserved0;
} vi_config;

/* VectorIndexerConfig::new(dimension) — src/api.rs:33-43 */
void vi_config_init(vi_config *cfg, uint32_t dimension);

typedef struct vi_indexer vi_indexer;

/* VectorIndexer::new(cfg) — src/api.rs:103-106 */
vi_status vi_indexer_new(const vi_config *cfg, vi_indexer **out);
/* VectorIndexer::load(cfg) — src/api.rs:109-112 (+ uploads the lists to HBM) */
vi_status vi_indexer_load(const vi_config *cfg, vi_indexer **out);
/* VectorIndexer::build_from_records(self, records) — src/api.rs:115-146.
 * values: n x dimension; ext_ids: n (NULL => 0..n-1); timestamps: n (NULL or 0 => now).
 * dims (optional, n): per-record length, to reproduce the "vector dimension mismatch at
 * index {i}" error (api.rs:122-133); NULL => all equal cfg.dimension.
 * Device memory: the build keeps the uploaded points (4 n D bytes, + 16 n for ids and timestamps when given) resident
 * until the searchable index built from them (another 4 n D for the blocks + 4 n D of bf16 images, + 1 n D for 8-bit data)
 * is complete: its peak is about twice what vi_indexer_load of the same index needs; the grouping sort adds 16 n bytes
 * and the largest shard's staging image transiently.  The resident index keeps 16 bytes per stored vector beside its
 * images: the external id and the timestamp (vi_indexer_filter_timestamps); a built or a loaded index alike.  A data set that fills more than ~40 % of HBM should be built in
 * parts or loaded from shard files written elsewhere. */
vi_status vi_indexer_build_from_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values,
                                        const uint64_t *timestamps, const uint32_t *dims, uint64_t n);
/* VectorIndexer::build_from_vector_file(self, path) — src/api.rs:149-186 */
vi_status vi_indexer_build_from_vector_file(vi_indexer *ix, const char *vector_file);

/* extension (the reference has no add, api.rs:101-237): append n records to a built or loaded index.  Afterwards the index
 * is the one the reference would search if each new record had been appended to the inverted list of its nearest kept
 * centroid: "nearest" is the first probe of the reference's coarse step (ivf_index.rs:205-220: smallest
 * euclidean_distance_squared in scalar order, ties to the lower centroid index).  The coarse table, index.bin and
 * centroids_to_shard do not change and nothing is retrained, so the balance of the lists degrades as adds accumulate.
 *   - order inside a list: old records keep their positions; new records follow in call order (ascending i); a second
 *     call goes behind the first
 *   - VectorMeta.id of new record i is N_before + i, N_before = vi_indexer_num_vectors before the call
 *   - values: n x dimension; ext_ids: n (NULL => N_before + i); timestamps: n (NULL or 0 => cfg.now_secs, else wall clock);
 *     duplicate external ids are not checked, as in a build
 *   - files: every touched shard file is rewritten, byte-identical to vi_shard_save_to of the merged lists (old records
 *     copied verbatim): all new files are written beside the old ones under temporary names, then renamed, and only then
 *     is the resident index swapped; a failure before the renames leaves files and handle unchanged.  A later
 *     vi_indexer_load of the directories gives the same index.  Cost: the touched shard files, plus one rebuild of the
 *     resident images.
 *   - resident index: rebuilt ON THE GPU from the old resident blocks and the new rows, not re-read from the files.  It
 *     is a replaced index: every vi_filter made before the call is VI_ERR_INVALID_INPUT afterwards (free it), and
 *     vi_range_results must be freed or copied before the call.  The call must not overlap searches on the handle, as for
 *     a rebuild; this is not enforced.
 *   - errors, all before any file or device change (VI_ERR_INVALID_INPUT): a null ix, values == NULL with n > 0, a
 *     non-finite value, a handle with no index, a partitioned handle (world_size > 1: ranks reload from the files an
 *     unpartitioned handle wrote), a total past 2^32 - 2 records or the 32-bit slot limit.  Files that no longer match the
 *     resident lists: VI_ERR_INVALID_DATA.
 *   - n == 0: VI_OK, nothing at all changes (old filters stay valid)
 * Device memory: the old and the new resident index coexist until the swap (about twice what vi_indexer_load of the new
 * index needs), beside the n uploaded rows (4 n D + 28 n bytes). */
vi_status vi_indexer_add_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values, const uint64_t *timestamps,
                                 uint64_t n);

/* VectorIndexer::search(&self, SearchRequest) — src/api.rs:188-222 — batched over nq queries
 * (extension: the reference takes one query per call; bindings/python/src/lib.rs:74-97 loops).
 * k and n_probe are clamped to max_k / max_n_probe first (api.rs:189-190), then k==0 or
 * n_probe==0 => VI_ERR_INVALID_INPUT (ivf_index.rs:197-202); query_dim != dimension =>
 * VI_ERR_INVALID_INPUT (api.rs:192-201).
 * Outputs (row stride = clamped k, which is returned in *k_out if non-NULL):
 *   D  nq x k f32 squared-L2, padded +inf     (lib.rs:179-187)
 *   I  nq x k i64 external ids, padded -1
 *   V  optional nq x k x dimension f32 (include_vectors; api.rs:213-217), zero padded
 *   counts optional nq: results actually found per query */
vi_status vi_indexer_search(const vi_indexer *ix, const float *queries, uint64_t nq, uint32_t query_dim,
                            uint64_t k, uint64_t n_probe, float *D, int64_t *I, float *V,
                            uint64_t *counts, uint64_t *k_out);

/* Same search, but queries/D/I are DEVICE pointers on the indexer's GPU and nothing is copied
 * to the host; tie (optional, nq x k u64) receives the reference candidate-order key
 * ((shard-visit-order<<32)|position) needed to merge per-GPU partial results exactly.
 * Used by the multi-GPU path (all-gather of per-rank top-k over RCCL). */
vi_status vi_indexer_search_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq,
                                   uint64_t k, uint64_t n_probe, float *D_dev, int64_t *I_dev,
                                   uint64_t *tie_dev);

/* Multi-GPU: the two halves of vi_indexer_search_device as separate calls, so that the coarse step — identical on
 * every rank, since the centroid table is replicated — can be SPLIT over the ranks by query instead of repeated:
 *   vi_indexer_probe_device          ivf_index.rs:205-220 for a slice of the batch: the n_probe_eff = min(n_probe,
 *                                    #centroids) nearest lists of each query in (distance, centroid index) order,
 *                                    and order[q][r] = rank of probe r in the reference's candidate order (shard
 *                                    visiting order, ivf_index.rs:223-262) — what the tie keys are built from;
 *   (all-gather of probes / order over the ranks)
 *   vi_indexer_search_probed_device  ivf_index.rs:223-274 for the whole batch against this rank's stripes with the
 *                                    given probe lists; outputs as vi_indexer_search_device.  Each row must hold its
 *                                    found real probes (list ids < #centroids) first, then only empty markers
 *                                    0xFFFFFFFF (whose order is not read), and the orders of the real probes must be
 *                                    a permutation of 0 .. found-1; anything else is VI_ERR_INVALID_INPUT.
 * Both return with their outputs complete; all pointers are device pointers.  Any k and n_probe the single-GPU entry
 * accepts (k > 128 or n_probe > 64 take the sort-everything path there and here). */
vi_status vi_indexer_probe_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t n_probe,
                                  uint32_t *probes_dev, uint32_t *order_dev, uint64_t *n_probe_eff);
vi_status vi_indexer_search_probed_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t k,
                                          uint64_t n_probe_eff, const uint32_t *probes_dev,
                                          const uint32_t *order_dev, float *D_dev, int64_t *I_dev,
                                          uint64_t *tie_dev);

/* ---- timestamp-window filtered search (extension: the reference stores VectorMeta.timestamp, shards.rs:45-51, but never
 * filters on it) ----
 * The filtered result of a query is what the reference's search would return if the candidates whose STORED timestamp
 * (the value in the shard file: a record built with timestamp 0 carries the build's `now`) lies outside
 * [ts_min, ts_max] — both inclusive — were deleted from its candidate sequence before the stable sort.  The coarse step
 * does not look at the filter (the probed lists are those of the unfiltered search), so a query may find fewer than k
 * results: padded +inf / -1 / zero vectors and reported in counts, as always.  Distances and tie keys are the unfiltered
 * ones, so per-rank partial results merge exactly through vi_merge_partials*_device when every rank filters by the same
 * window.  A window that admits everything returns bit for bit what the unfiltered entry returns; one that admits
 * nothing returns VI_OK with zero results; ts_min > ts_max is VI_ERR_INVALID_INPUT.
 * A vi_filter belongs to the resident index of ONE handle (another handle's, or one made before the handle was rebuilt,
 * is VI_ERR_INVALID_INPUT), is immutable (the one exception: `reuse` of vi_indexer_filter_compose, below), and may be
 * shared by the concurrent searches a handle allows.  It holds 12 bytes
 * of device memory per resident slot (16 for 8-bit descriptor data) and must be freed before its indexer.
 * f == NULL: the unfiltered entry. */
typedef struct vi_filter vi_filter;
vi_status vi_indexer_filter_timestamps(const vi_indexer *ix, uint64_t ts_min, uint64_t ts_max, vi_filter **out);
uint64_t vi_filter_num_allowed(const vi_filter *f); /* resident vectors inside the window */
void vi_filter_free(vi_filter *f);                  /* NULL ok */
/* vi_indexer_search / _search_device / _search_probed_device with a filter: the same arguments after it, the same
 * clamping and validation of k / n_probe / query_dim */
vi_status vi_indexer_search_filtered(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq,
                                     uint32_t query_dim, uint64_t k, uint64_t n_probe, float *D, int64_t *I, float *V,
                                     uint64_t *counts, uint64_t *k_out);
vi_status vi_indexer_search_filtered_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev,
                                            uint64_t nq, uint64_t k, uint64_t n_probe, float *D_dev, int64_t *I_dev,
                                            uint64_t *tie_dev);
vi_status vi_indexer_search_probed_filtered_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev,
                                                   uint64_t nq, uint64_t k, uint64_t n_probe_eff,
                                                   const uint32_t *probes_dev, const uint32_t *order_dev, float *D_dev,
                                                   int64_t *I_dev, uint64_t *tie_dev);

/* ---- filters by external id: allow and deny sets, and the intersection of two filters (extension; what Faiss calls
 * IDSelectorBatch / IDSelectorNot) ----
 * The filtered result of a query is the reference's candidate sequence with some candidates deleted before the stable
 * sort: VI_IDS_ALLOW deletes the candidates whose external id is NOT in the set, VI_IDS_DENY those whose external id IS
 * in it (a deny set hides records for one search; vi_indexer_remove_ids removes them).  The coarse step, distances, tie keys,
 * padding and counts are exactly as for the timestamp filter above, so per-rank partial results merge exactly when every
 * rank filters by the same set.
 *   - the set needs no order; duplicates are allowed; ids that no resident vector carries are ignored
 *   - any u64 is a legal id, 0 and UINT64_MAX included
 *   - n == 0 (ids may be NULL): ALLOW admits nothing (VI_OK, zero results); DENY admits everything and returns bit for
 *     bit what the unfiltered entry returns
 *   - a null ix or out, ids == NULL with n > 0, or a mode other than 0 / 1: VI_ERR_INVALID_INPUT, before any device work
 *   - _device: the n ids are read in place from device memory; the host entry uploads them once
 *   - on a partitioned handle (world_size > 1) the filter covers the resident slots
 * vi_filter_intersect: the vectors both a and b admit (for example "this tenant's ids" and "last week").  A null filter,
 * or a filter of another handle or of a replaced index, is VI_ERR_INVALID_INPUT; a and b stay valid and independent.
 * The resulting vi_filter is a vi_filter like any other: the three *_filtered* search entries and both radius entries
 * take it, vi_filter_num_allowed and vi_filter_free apply, and it holds the same device memory as a timestamp filter (the
 * id set itself is not kept). */
typedef enum vi_id_mode { VI_IDS_ALLOW = 0, VI_IDS_DENY = 1 } vi_id_mode;
vi_status vi_indexer_filter_ids(const vi_indexer *ix, const uint64_t *ids, uint64_t n, vi_id_mode mode, vi_filter **out);
vi_status vi_indexer_filter_ids_device(const vi_indexer *ix, const uint64_t *ids_dev, uint64_t n, vi_id_mode mode,
                                       vi_filter **out);
vi_status vi_filter_intersect(const vi_indexer *ix, const vi_filter *a, const vi_filter *b, vi_filter **out);

/* ---- compound filters: union, complement, id ranges, masks, and one call for a whole expression (extension; Faiss's
 * IDSelectorRange / IDSelectorOr / IDSelectorNot / IDSelectorBitmap) ----
 * vi_indexer_filter_compose makes ONE filter from the AND (VI_JOIN_AND) or the OR (VI_JOIN_OR) of n_terms = 1 ..
 * VI_FILTER_MAX_TERMS terms, in one kernel launch with one synchronisation.  A resident record is admitted when the join
 * of the terms holds; `negate` = 1 flips a term before the join.  Negation is relative to the resident records: no
 * expression admits a pad slot, as with a deny set.  Deeper expressions nest through VI_TERM_FILTER.  The result is a
 * vi_filter like any other (searches, radius searches, vi_indexer_retain, the per-rank merges), and the filtered result
 * of a query is, as above, the reference's candidate sequence less the candidates the filter does not admit.
 * Fields a kind does not use are ignored.  Per kind:
 *   VI_TERM_TIMESTAMPS   lo <= stored timestamp <= hi   } both inclusive; any u64 is a legal bound, (0, UINT64_MAX) holds
 *   VI_TERM_ID_RANGE     lo <= external id <= hi        } everywhere; lo > hi is VI_ERR_INVALID_INPUT
 *   VI_TERM_IDS          the external id is one of data[0 .. n) (u64, host memory): the rules of vi_indexer_filter_ids —
 *   VI_TERM_IDS_DEVICE     no order, duplicates allowed, absent ids ignored, UINT64_MAX legal; n == 0 (data may be NULL)
 *                          holds nowhere.  _DEVICE: the ids are read in place from device memory.  Every id term of a
 *                          call gets a table of its own; all are freed before the call returns.
 *   VI_TERM_MASK         data[i] != 0 (n bytes, host memory; _DEVICE: device memory, read in place), i = the record's
 *   VI_TERM_MASK_DEVICE    ordinal in LIST ORDER: byte i belongs to the record vi_indexer_export_records returns as row i
 *                          — an attribute the caller keeps beside an export.  n must equal vi_indexer_num_vectors(ix).  On
 *                          a partitioned handle this is the rank's own list order, as for an export: a mask is per rank.
 *   VI_TERM_FILTER       `filter` admits the record: a filter of this handle's index (another handle's, or one made
 *                          before an update: VI_ERR_INVALID_INPUT)
 * reuse (or NULL): a filter of this handle's index that the call OVERWRITES in place; *out is then `reuse`, and no filter
 * buffer is allocated.  This is the one exception to "a vi_filter is immutable": THE CALLER GUARANTEES THAT NO SEARCH IS
 * USING `reuse` DURING THE CALL.  `reuse` passes the same validity check as an operand (one made before an update is
 * rejected) and must not be one of the call's own VI_TERM_FILTER operands (the writer clears the allow words first):
 * VI_ERR_INVALID_INPUT before any device work, `reuse` untouched.  On an error after validation the content of `reuse`
 * is unspecified; it stays freeable.
 * Errors, all VI_ERR_INVALID_INPUT before any device work (*out untouched): a null ix, terms or out; n_terms outside
 * 1 .. 8; an unknown kind or join; negate other than 0 / 1; data == NULL with n > 0; a null `filter` of a FILTER term; a
 * handle with no index; a timestamp term on an index that keeps no timestamps; an id or id-range term on an index that
 * keeps no external ids; an id set of more than 2^40 ids; a mask of the wrong length.
 * The five entries below it are thin calls into it: a | b, the complement of a within the resident records, one id range,
 * one mask. */
#define VI_FILTER_MAX_TERMS 8
typedef enum vi_term_kind { VI_TERM_TIMESTAMPS = 0, VI_TERM_ID_RANGE = 1, VI_TERM_IDS = 2, VI_TERM_IDS_DEVICE = 3,
                            VI_TERM_MASK = 4, VI_TERM_MASK_DEVICE = 5, VI_TERM_FILTER = 6 } vi_term_kind;
typedef enum vi_filter_join { VI_JOIN_AND = 0, VI_JOIN_OR = 1 } vi_filter_join;
typedef struct vi_filter_term {
  uint32_t kind;            /* vi_term_kind */
  uint32_t negate;          /* 0 / 1 */
  uint64_t lo, hi;          /* TIMESTAMPS, ID_RANGE: both inclusive */
  const void *data;         /* IDS*: n u64 ids;  MASK*: n bytes, non-zero admits */
  uint64_t n;
  const vi_filter *filter;  /* FILTER */
} vi_filter_term;
vi_status vi_indexer_filter_compose(const vi_indexer *ix, vi_filter_join join, const vi_filter_term *terms,
                                    uint32_t n_terms, vi_filter *reuse, vi_filter **out);
vi_status vi_filter_union(const vi_indexer *ix, const vi_filter *a, const vi_filter *b, vi_filter **out);
vi_status vi_filter_complement(const vi_indexer *ix, const vi_filter *a, vi_filter **out);
vi_status vi_indexer_filter_id_range(const vi_indexer *ix, uint64_t id_min, uint64_t id_max, vi_filter **out);
vi_status vi_indexer_filter_mask(const vi_indexer *ix, const uint8_t *mask, uint64_t n, vi_filter **out);
vi_status vi_indexer_filter_mask_device(const vi_indexer *ix, const uint8_t *mask_dev, uint64_t n, vi_filter **out);

/* ---- extension (the reference has no remove, api.rs:101-237): remove records from a built or loaded index ----
 * Afterwards the index is the one the reference would search if the removed records had been deleted from their inverted
 * lists: the remaining records of each list close up in their old order.  The coarse table, index.bin, centroids_to_shard
 * and the centroid vectors in the shard files do not change and nothing is retrained.  A list that loses every record
 * stays in its shard file as an entry with num_vectors == 0, stays in the coarse table and is still probed (it yields no
 * candidate).  Every search afterwards returns, in ids and distance bits, what the same search returned before through a
 * filter admitting exactly the kept records; tie keys differ, because positions move.
 *   vi_indexer_retain      keeps exactly the resident records `keep` admits (any vi_filter of this handle's index: a
 *                          timestamp window, an id set, an intersection)
 *   vi_indexer_remove_ids  Faiss's remove_ids: removes every record whose external id is in the set, by the rules of a
 *                          VI_IDS_DENY set (any order, duplicates allowed, unknown ids ignored, any u64 is an id); it is
 *                          vi_indexer_retain of that deny filter
 *   *removed_out (optional): records removed (0 on an error)
 *   - files: only shard files that hold a removed record are rewritten, WHOLE, byte-identical to vi_shard_save_to of the
 *     remaining lists (lists in file order, centroid vectors and kept records copied verbatim, VectorMeta.id unchanged).
 *     All new files are written beside the old ones as shard_<id>.bin.tmp, then renamed, and only then is the resident
 *     index swapped; a failure before the renames removes the temporaries and leaves files and handle unchanged.  A later
 *     vi_indexer_load of the directories gives the same index.
 *   - resident index: rebuilt ON THE GPU from the old resident blocks, not re-read from the files.  It is a replaced
 *     index: every vi_filter made before the call is VI_ERR_INVALID_INPUT afterwards, `keep` included (free them), and
 *     vi_range_results must be freed or copied before the call.  The call must not overlap searches on the handle; this
 *     is not enforced.
 *   - nothing to remove (`keep` admits everything, n == 0, no id matches): VI_OK, *removed_out = 0, no file is touched,
 *     no index is replaced, old filters stay valid
 *   - errors, all VI_ERR_INVALID_INPUT before any file or device change: a null ix, a null keep, ext_ids == NULL with
 *     n > 0, a handle with no index, a filter of another handle or of a replaced index, a partitioned handle
 *     (world_size > 1: ranks reload from the files an unpartitioned handle wrote), a removal that would leave the index
 *     with no record at all (an index keeps at least one record; to drop an index, delete its directories).  A shard
 *     file whose list no longer has its resident length: VI_ERR_INVALID_DATA.
 *   - vi_indexer_add_records afterwards still numbers VectorMeta.id from vi_indexer_num_vectors, so after a remove a
 *     later add can repeat an internal id that is still in the files.  Nothing in the search path reads VectorMeta.id:
 *     results carry external ids.
 * Device memory: the old and the new resident index coexist until the swap, beside one filter (vi_indexer_remove_ids
 * makes its own).
 * vi_shard_remove_from: the file half alone, no GPU: the same removal, by external id, from one shard file (written
 * beside it under a temporary name, renamed when complete).  A file that cannot be read: the errors of
 * vi_shard_get_centroid_vectors_from.  No record matches: the file is left as it is. */
vi_status vi_indexer_retain(vi_indexer *ix, const vi_filter *keep, uint64_t *removed_out);
vi_status vi_indexer_remove_ids(vi_indexer *ix, const uint64_t *ext_ids, uint64_t n, uint64_t *removed_out);
vi_status vi_shard_remove_from(const char *shards_dir, uint64_t shard_id, const uint64_t *ext_ids, uint64_t n,
                               uint64_t *removed_out);

/* ---- extension (the reference has no update, api.rs:101-237): upsert records in a built or loaded index; what Faiss's IVF
 * calls update_vectors ----
 * "This id has a new vector."  Afterwards the index is the one these two calls leave, in this order on the same handle:
 *   vi_indexer_remove_ids(ix, ext_ids, n, &r);  vi_indexer_add_records(ix, ext_ids, values, timestamps, n);
 * with byte-identical shard files, an untouched index.bin / coarse table / centroids_to_shard, and the same ids, distance
 * bits, counts, padding and tie keys from every search — but every touched shard file is written ONCE, the resident
 * index is rebuilt ONCE (one pass of update_blocks_kernel over the new blocks, one set of ranking images) and swapped
 * ONCE, and the record is never absent from the files or the handle in between.
 *   - what goes: every stored record whose external id is in ext_ids, by the rules of a VI_IDS_DENY set (any order,
 *     duplicates allowed, ids nothing carries are ignored, any u64 is an id; an id several stored records carry removes
 *     them all).  The kept records of a list close up in their old order.
 *   - where new records go: record i goes behind the kept records of the list of its nearest centroid ("nearest": the
 *     first probe of the reference's coarse step, ivf_index.rs:205-220, on the old index; the table does not change),
 *     new records in call order.  An id named twice in one call is added twice, as vi_indexer_add_records does; nothing
 *     is de-duplicated.
 *   - VectorMeta.id of new record i is N_before - replaced + i; timestamps: NULL or 0 => cfg.now_secs, else wall clock
 *   - *replaced_out (optional): records removed (0 on an error)
 *   - no id matches: a plain add with those ids.  n == 0: VI_OK, nothing at all changes (old filters stay valid).
 *   - one deliberate difference from the two calls: a call may replace EVERY record of the index (the two-call form stops
 *     at "an index keeps at least one record"); the result holds n >= 1 records.  Lists that receive nothing become empty
 *     entries (num_vectors == 0, still in the coarse table, still probed).
 *   - files: a shard file is rewritten, whole, if a list in it lost or received a record; all new files are written
 *     beside the old ones as shard_<id>.bin.tmp, then renamed, and only then is the resident index swapped; a failure
 *     before the renames removes the temporaries and leaves files and handle unchanged
 *   - resident index: a replaced index, as after an add or a remove: every vi_filter made before the call is
 *     VI_ERR_INVALID_INPUT afterwards (free it), vi_range_results must be freed or copied before the call, and the call
 *     must not overlap searches on the handle; this is not enforced
 *   - errors, all VI_ERR_INVALID_INPUT before any file or device change: a null ix, ext_ids == NULL or values == NULL
 *     with n > 0, a non-finite value, a handle with no index, a partitioned handle (world_size > 1),
 *     N_before - replaced + n past 2^32 - 2, the 32-bit slot limit of the planned layout.  A shard file whose list no
 *     longer has its resident length: VI_ERR_INVALID_DATA.
 * Device memory: the old and the new resident index coexist until the swap, beside one filter and the n uploaded rows
 * (4 n D + 28 n bytes).
 * vi_shard_upsert_to: the file half alone, no GPU: from one shard file every record whose external id is in ext_ids goes
 * (the rules of vi_shard_remove_from), then record i joins the list of centroid_ids[i] (the arguments and rules of
 * vi_shard_append_to); one image, one temporary file, one rename.  A centroid id the shard does not hold:
 * VI_ERR_NOT_FOUND, and the file is untouched.  n == 0 leaves the file as it is.  *removed_out (optional): records removed. */
vi_status vi_indexer_upsert_records(vi_indexer *ix, const uint64_t *ext_ids, const float *values, const uint64_t *timestamps,
                                    uint64_t n, uint64_t *replaced_out);
vi_status vi_shard_upsert_to(const char *shards_dir, uint64_t shard_id, uint64_t n, const uint64_t *centroid_ids,
                             const uint64_t *ids, const uint64_t *ext_ids, const uint64_t *timestamps, const float *vecs,
                             uint64_t *removed_out);

/* ---- extension (the reference never retrains, api.rs:101-237): refine a built or loaded index — recentre the lists and
 * re-home the records, on the GPU; Lloyd iterations warm-started from the table the index has ----
 * The index holds n records in list order (the order vi_indexer_export_records returns): record i is row X[i] in list
 * lab[i]; the table C has k lists, the empty ones included.  ONE ITERATION:
 *   1. centres.  For each list l with at least one record, C'[l] is what the reference's update_centroids_parallel
 *      (kmeans.rs:674-719) gives for cluster l of (X, lab): per column one sequential f32 chain from +0.0 over the list's
 *      records in list order, then that function's division by the count.  A list WITHOUT a record keeps C[l] bit for
 *      bit.  (A deliberate deviation: the reference writes zeros there, and a zero centroid would attract records.)
 *   2. labels.  lab'[i] is the list the reference's search would probe first for X[i] on the table C': the coarse step of
 *      ivf_index.rs:205-220 at n_probe = 1, scalar summation order, the lowest list index among equal distances — the
 *      rule of vi_indexer_add_records, so afterwards every record sits where an add would put it.
 *   3. lists.  List l holds the records with lab' == l in ascending order of their position before the iteration (stable).
 *      List ids, centroids_to_shard and the number of lists do not change; a list may end empty and stays as an entry
 *      with no records (num_vectors == 0, still in the coarse table, still probed), as after vi_indexer_remove_ids.
 * `iters` iterations run one after another; the call stops early after an iteration that moved no record and whose C'
 * equals its C bit for bit (every further iteration would be the identity), which shows in iterations_run alone.
 *   - *moved_out (optional): records whose list after the call differs from their list before it (0 on an error)
 *   - iters == 0: VI_OK and nothing at all changes — no file is touched, the resident index stays, old filters stay valid
 *   - files afterwards: index.bin holds the new table; every shard file that holds a list equals, byte for byte, the
 *     reference's writer over the new lists: lists keep their file order, external ids and stored timestamps are carried
 *     verbatim, and VectorMeta.id is renumbered to the record's position in the NEW list order, 0..n-1 (so refine(3)
 *     equals three refine(1), and the repeated internal ids earlier updates may have left are gone; a later add continues
 *     from n).  Shard files without a list are left alone.
 *   - crash behaviour: every file is written under a temporary name first (shard_<id>.bin.tmp, index.bin.tmp); a failure
 *     before the first rename removes them and leaves files and handle unchanged.  Then the renames: shards first,
 *     index.bin last, then the resident index is swapped.  A crash between the first and the last rename leaves a
 *     directory that mixes old and new files — the limit vi_indexer_upsert_records has.
 *   - resident index: a replaced index: every vi_filter made before a call that ran an iteration is
 *     VI_ERR_INVALID_INPUT afterwards (free it), vi_range_results must be freed or copied before the call, and the call
 *     must not overlap searches on the handle; this is not enforced (the rules of vi_indexer_add_records)
 *   - errors, all VI_ERR_INVALID_INPUT before any file or device change: a null ix, a handle with no index, a partitioned
 *     handle (world_size > 1), an index without a record.  A shard file whose lists are no longer the resident ones:
 *     VI_ERR_INVALID_DATA.
 * Device memory: the old and the new resident index coexist until the swap, beside 32 bytes per record of labels and
 * orders, the grouping's scratch, one chunk of stored rows and two tables; no N x D row-major copy is made anywhere. */
vi_status vi_indexer_refine(vi_indexer *ix, uint64_t iters, uint64_t *moved_out);
/* the most recent vi_indexer_refine on this handle with iters > 0 (wall-clock ms unless said otherwise) */
typedef struct vi_refine_stats {
  uint64_t iterations_run;   /* iterations run, the one that found the fixed point included */
  uint64_t moved;            /* records whose list changed over the call */
  uint64_t lists_emptied;    /* lists that held records before the call and hold none after it */
  uint64_t shards_rewritten; /* shard files rewritten, each once */
  uint64_t bytes_written;    /* bytes of those files and of index.bin */
  uint64_t means_bytes;      /* bytes list_means_kernel read and wrote, summed over the iterations ... */
  uint64_t rehome_bytes;     /* ... and rehome_blocks_kernel */
  float ms_total;
  float ms_means;            /* the centres of every iteration: list_means_kernel, the table read back and compared */
  float ms_label;            /* the labels of every iteration: coarse table, walk over the stored rows, grouping */
  float ms_rehome;           /* the new layout, rehome_blocks_kernel, the new coarse table */
  float ms_images;           /* norms and ranking images of the new index */
  float ms_files;            /* new files written and renamed */
  float ms_means_kernel;     /* HIP-event time of list_means_kernel alone, summed over the iterations (part of ms_means) */
  float ms_rehome_kernel;    /* HIP-event time of rehome_blocks_kernel alone (part of ms_rehome) */
} vi_refine_stats;
vi_status vi_indexer_last_refine_stats(const vi_indexer *ix, vi_refine_stats *out);

/* ---- extension: rebalance a built or loaded index — a refine whose first iterations split overfull lists into the empty
 * ones (the cure Faiss's k-means applies to an empty cluster).  A refine is warm-started, so it never moves a centroid
 * across the data: a list many adds piled into stays one list, a list vi_indexer_remove_ids emptied stays empty.  Here an
 * empty (or nearly empty) list takes over one half of an overfull one.  The number of lists, the list ids and
 * centroids_to_shard do not change ----
 * The call runs rule->iters iterations of vi_indexer_refine's contract; each of the first rule->split_rounds of them is
 * that contract's steps 1, 1b, 2, 3 over the records in the current list order (1, 2 and 3 verbatim):
 *  1b. PLAN, from the list lengths len[] at the start of the iteration, mean = n / lists in double:
 *        donors     the lists with len >= 2 and (double)len > split_factor * mean, by (len descending, index ascending)
 *        receivers  the lists with len <= receiver_max_len, by (len ascending, index ascending); a list that qualifies
 *                   as both is a donor only
 *        pair i = (donor i, receiver i) for i < min(#donors, #receivers, max_splits or no cap)
 *      SPLIT of pair (d, r) over the members x_0 .. x_{m-1} of d in list order, c = C'[d] from step 1.  Every distance is
 *      the reference's euclidean_distance_squared scalar chain (utils.rs:28-30): an unfused (a - b) * (a - b) accumulated
 *      in column order, the arithmetic of the coarse step.
 *        seeds   a = the position with the largest d(x_i, c), b = the position with the largest d(x_i, x_a), each the
 *                lowest position among equals.  d(x_b, x_a) == 0 (all members equal): the pair is SKIPPED — both
 *                centroids stay as step 1 left them.  Otherwise ca = x_a, cb = x_b.
 *        inner iteration, at most split_iters times: side_i = 1 if d(x_i, cb) < d(x_i, ca), else 0 (a tie goes to side
 *                0).  Either side empty: stop, keep ca and cb.  Otherwise ca' / cb' = the centre of the side-0 / side-1
 *                members: step 1's chain per column over THAT side's members in list order, then its one divide.  Stop
 *                after an inner iteration that left every bit of ca and cb unchanged.
 *        result  C'[d] = ca, C'[r] = cb.  A receiver that still holds records loses them to step 2 like any other record;
 *                the split itself touches no record.
 * Step 2 labels against the table after 1b, and the fixed-point test compares THAT table with the iteration's input
 * table: an iteration whose plan is empty or wholly skipped is a plain refine iteration and may end the call early.
 *   - split_rounds == 0: the call IS vi_indexer_refine(iters), file for file
 *   - files, crash behaviour, resident index and filters, device memory: as vi_indexer_refine (beside its memory: one
 *     byte per member of the donors, two centres and a few words per pair)
 *   - errors, all VI_ERR_INVALID_INPUT before any file or device change: a null rule, iters == 0, split_rounds > iters, a
 *     split_factor that is not finite or below 1, split_iters outside 1..64, a non-zero reserved0, and everything
 *     vi_indexer_refine refuses (a null ix, no index, a partitioned handle, no record) */
typedef struct vi_rebalance_rule {
  uint64_t iters;            /* iterations of vi_indexer_refine's contract, >= 1 */
  uint64_t split_rounds;     /* the first split_rounds iterations carry a split step; <= iters; 0: the call IS vi_indexer_refine(iters) */
  double   split_factor;     /* a donor is longer than split_factor * (n / lists); finite, >= 1.0 */
  uint64_t receiver_max_len; /* a receiver holds at most this many records; 0 = empty lists only */
  uint64_t max_splits;       /* pairs per round at most; 0 = no cap */
  uint32_t split_iters;      /* inner two-means iterations of a split, 1..64 */
  uint32_t reserved0;
} vi_rebalance_rule;
void vi_rebalance_rule_init(vi_rebalance_rule *r);   /* 1, 1, 2.0, 0, 0, 4 */
vi_status vi_indexer_rebalance(vi_indexer *ix, const vi_rebalance_rule *rule, uint64_t *moved_out);
/* the most recent vi_indexer_rebalance on this handle that ran: the fields of vi_refine_stats, then the split steps */
typedef struct vi_rebalance_stats {
  uint64_t iterations_run, moved, lists_emptied, shards_rewritten, bytes_written, means_bytes, rehome_bytes;
  float ms_total, ms_means, ms_label, ms_rehome, ms_images, ms_files, ms_means_kernel, ms_rehome_kernel;
  uint64_t pairs_planned;    /* pairs of every round's plan */
  uint64_t splits_done;      /* ... whose two centres went into the table */
  uint64_t splits_skipped;   /* ... whose members were all equal */
  uint64_t inner_iterations; /* inner iterations, summed over the pairs */
  uint64_t split_bytes;      /* bytes the three split kernels read and wrote */
  float ms_split;            /* plans and splits of every round, the table written back (wall clock; in none of the phases above) */
  float ms_split_kernels;    /* HIP-event time of the split kernels alone (part of ms_split) */
} vi_rebalance_stats;
vi_status vi_indexer_last_rebalance_stats(const vi_indexer *ix, vi_rebalance_stats *out);
/* the balance of the resident lists, from their lengths (on a rank of a partitioned index: the rank's part of every list):
 * when imbalance grows after many adds, a refine is due */
typedef struct vi_list_stats {
  uint64_t lists;            /* entries of the coarse table */
  uint64_t empty_lists;      /* ... without a record */
  uint64_t min_len, max_len; /* shortest (the empty ones count) and longest list */
  double mean_len;
  double imbalance;          /* Faiss's imbalance factor, lists * sum(len^2) / sum(len)^2: 1 = equal lengths, lists = one
                                list holds everything; 0 for an index without a record */
} vi_list_stats;
vi_status vi_indexer_list_stats(const vi_indexer *ix, vi_list_stats *out);

/* ---- extension (the reference reads a stored vector only through include_vectors, api.rs:213-217): read records back from
 * a built or loaded index: by external id, or a range of all of them in list order ----
 * LIST ORDER: the resident records ordered by list index ascending (the row of vi_indexer_centroids = the centroid_id of
 * the shard files), then by position in the list ascending (the record's place in its list in the shard file, which is
 * the reference's candidate order inside a list).  where = (list index << 32) | position in the FULL list.
 * vi_indexer_get_records, per requested id i:
 *   - count_out[i]: the resident records whose external id equals ext_ids[i]; 0: absent
 *   - values_out[i, 0..dim) (the stored f32 bits), timestamps_out[i], where_out[i]: the FIRST such record in list order
 *   - an absent id: a zero-filled row, timestamp 0, where VI_WHERE_NONE, and the call still returns VI_OK
 *   - the request needs no order and may repeat ids; every row is filled, a repeated id's included; any u64 is an id
 *   - any of the four outputs may be NULL, which skips that work: with values_out == NULL nothing is gathered and the call
 *     is "contains / how many"
 *   - n == 0: VI_OK, nothing is read or written
 * vi_indexer_export_records: records [first, first + count) of the list order; row j of every output is record first + j.
 *   first + count > vi_indexer_num_vectors: VI_ERR_INVALID_INPUT; count == 0: VI_OK; outputs may be NULL, as above.
 * The _device forms take and fill device pointers (ids, counts u32, values f32 row-major n x dim, timestamps, where).
 *   - on a partitioned handle (world_size > 1, both placements) both calls cover the resident records of this rank in
 *     its local list order; where still carries the position in the full list (a stripe's local position p is
 *     ((p / 64) * world + rank) * 64 + p % 64 there), so per-rank answers combine by the lowest where and the sum of counts
 *   - VectorMeta.id (the internal id) is not resident and is not returned
 *   - the result is the caller's memory: it stays valid across later updates of the handle
 *   - threads: the contract of a search: const on the handle, any number of gets, exports and searches at once (each
 *     holds a stream of its own), none of them overlapping an update (add / remove / upsert / build)
 *   - cost: there is no persistent id -> slot map: every get reads the 8-byte external id of every resident slot once
 *     (a hash table of the REQUESTED ids is probed with them), then gathers n rows; an export reads each block once
 *   - errors, all VI_ERR_INVALID_INPUT before any device work: a null ix, ext_ids == NULL with n > 0, a handle with no
 *     index, n past 2^40.  Any other failure is VI_ERR_DEVICE, the outputs unspecified. */
#define VI_WHERE_NONE UINT64_MAX
vi_status vi_indexer_get_records(const vi_indexer *ix, const uint64_t *ext_ids, uint64_t n, uint32_t *count_out,
                                 float *values_out, uint64_t *timestamps_out, uint64_t *where_out);
vi_status vi_indexer_get_records_device(const vi_indexer *ix, const uint64_t *ext_ids_dev, uint64_t n, uint32_t *count_dev,
                                        float *values_dev, uint64_t *timestamps_dev, uint64_t *where_dev);
vi_status vi_indexer_export_records(const vi_indexer *ix, uint64_t first, uint64_t count, uint64_t *ext_ids_out,
                                    float *values_out, uint64_t *timestamps_out, uint64_t *where_out);
vi_status vi_indexer_export_records_device(const vi_indexer *ix, uint64_t first, uint64_t count, uint64_t *ext_ids_dev,
                                           float *values_dev, uint64_t *timestamps_dev, uint64_t *where_dev);

/* ---- extension: search by stored record ("what is similar to the record I already hold?") --------------------------
 * The query of a row is the stored f32 bits of a resident record r; the row is the reference's candidate sequence for
 * that query (probed lists in shard visiting order, probe rank, list position), less what the filter does not admit,
 * less — with exclude_self != 0 — the ONE candidate that is r itself (the same list and position: a record with the
 * same external id, or with the same bits under another id, stays), stably sorted, take(k).  Coarse step, distances,
 * tie keys, padding (+inf / -1 / tie UINT64_MAX / zero vectors) and counts are exactly those of
 * vi_indexer_search_filtered* with a deny of that one slot; exclude_self == 0 gives bit for bit what vi_indexer_search*
 * returns for the stored bits as the query.  If r's own list is not among the probed ones nothing is deleted.
 *   by ids:    an id names the first record in list order that carries it (the record vi_indexer_get_records returns);
 *              found[i] = resident records carrying it (the get's count_out).  An absent id is no error: its row is all
 *              padding, counts[i] = 0, found[i] = 0.  Ids may repeat, in any order; any u64 is an id.
 *   knn_graph: rows = records [first, first + count) of LIST ORDER (row j is the record vi_indexer_export_records returns
 *              as row j); first + count > vi_indexer_num_vectors is VI_ERR_INVALID_INPUT.  The range is processed in
 *              chunks of VI_GRAPH_CHUNK rows (environment, default 65536) through one search context.
 * k and n_probe are clamped to max_k / max_n_probe first; the row stride is the clamped k (*k_out).  The one extra
 * candidate exclusion needs internally is not subject to max_k.  COST: an excluding call searches k + 1 wide, so k = 64
 * (VALU engine) and k = 128 (MFMA engine) fall to the engine that sorts every candidate; results are the same bits.
 * f == NULL: no filter; a row exists for every named record whether or not the filter admits that record.  D / I /
 * tie / found of the *_device entries are device pointers; tie and found may be NULL, as V, counts, found, k_out of the
 * host entries.  nq == 0 / count == 0: VI_OK, nothing touched.  Partitioned handles (world_size > 1) are
 * VI_ERR_INVALID_INPUT.  Threads: the contract of a search.  vi_indexer_last_stats afterwards reads as after the
 * underlying search (of the last chunk), k as the caller's clamped k. */
/* queries named by external id */
vi_status vi_indexer_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq,
                                   uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, float *V,
                                   uint64_t *counts, uint32_t *found, uint64_t *k_out);
vi_status vi_indexer_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq,
                                          uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev,
                                          uint64_t *tie_dev, uint32_t *found_dev);
/* rows = records [first, first + count) of LIST ORDER (row j is the record vi_indexer_export_records returns as row j) */
vi_status vi_indexer_knn_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k,
                               uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, uint64_t *counts, uint64_t *k_out);
vi_status vi_indexer_knn_graph_device(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k,
                                      uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev, uint64_t *tie_dev);
/* Of the calling thread's last of the four (or of the three radius forms below), summed over its chunks, taken only while the environment variable
 * VI_SIMILAR_TIMING is set (and not "0"); zeros otherwise.  ms_resolve / ms_search: host clock around the gather of the
 * queries and around the search; ms_drop: HIP events around self_drop_kernel.  Reported with or without the variable:
 * drop_bytes, the bytes that kernel moved, and chunk_rows, the rows per chunk used.  Any pointer may be NULL. */
vi_status vi_similar_last_times(float *ms_resolve, float *ms_search, float *ms_drop, uint64_t *drop_bytes, uint64_t *chunk_rows);

/* ---- extension: radius (range) search -----------------------------------------------------------------------------
 * Every candidate of the probed lists whose squared distance is at most radius2.  The result of a query is the
 * reference's candidate sequence (probed lists in shard visiting order, then probe rank, then list position) after the
 * reference's stable sort by distance, cut at the first candidate with d > radius2: take_while(d <= radius2) where a
 * search has take(k).  d is the reference's f32 scalar-order sum and the comparison is made in f32, so d == radius2 is
 * inside.  Ids, distance bits, order and per-query counts are exact on every engine.
 *   - the coarse step is the unfiltered, unradiused one: the result covers the n_probe probed lists only; n_probe is
 *     clamped to max_n_probe; n_probe == 0 or a query_dim mismatch is VI_ERR_INVALID_INPUT
 *   - radius2 NaN: VI_ERR_INVALID_INPUT; negative: VI_OK with zero results; +inf: everything probed, sorted
 *   - a NaN / Inf query value: VI_ERR_PANIC (host entry), as for a search
 *   - f: candidates outside the filter's window are deleted from the sequence first (NULL: no filter)
 *   - on a partitioned handle (world_size > 1) the result covers the resident part, with the tie keys
 *     vi_indexer_search_device gives (stripe correction included): per-rank results merge by (distance, tie) — vi_range_merge_device
 *   - a batch is all or nothing: when scratch or result memory cannot be had the call fails (VI_ERR_DEVICE, or
 *     VI_ERR_INVALID_INPUT "split nq") and *out stays NULL
 * The result is an opaque object in CSR layout, as Faiss's RangeSearchResult: query q owns entries [lims[q], lims[q+1])
 * of D / I / tie.  It owns its device buffers, stays valid through later searches of the handle, and must be freed
 * before its indexer.  vi_indexer_last_stats after a radius search reads as after a search, with k = 0. */
typedef struct vi_range_result vi_range_result;
vi_status vi_indexer_range_search(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq,
                                  uint32_t query_dim, float radius2, uint64_t n_probe, vi_range_result **out);
vi_status vi_indexer_range_search_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev, uint64_t nq,
                                         float radius2, uint64_t n_probe, vi_range_result **out);
uint64_t vi_range_result_total(const vi_range_result *r); /* lims[nq]; NULL: 0 */
/* host buffers: lims nq + 1, D and I `total` each, V (optional) total x dim: the stored vectors of the hits */
vi_status vi_range_result_copy(const vi_range_result *r, uint64_t *lims, float *D, int64_t *I, float *V);
/* the result's own device buffers (any of the four may be NULL); tie = (candidate-order rank << 32) | list position */
vi_status vi_range_result_device(const vi_range_result *r, const uint64_t **lims_dev, const float **D_dev,
                                 const int64_t **I_dev, const uint64_t **tie_dev);
/* the same four arrays copied into DEVICE buffers of the caller on the result's GPU (lims nq + 1, the rest `total` each;
 * any may be NULL), e.g. tensors of a framework that is to own them; complete on return */
vi_status vi_range_result_copy_device(const vi_range_result *r, uint64_t *lims_dev, float *D_dev, int64_t *I_dev,
                                      uint64_t *tie_dev);
void vi_range_result_free(vi_range_result *r); /* NULL ok */

/* ---- extension: radius search by stored record ("which records are within eps of the one I hold?") ------------------
 * The row of a stored record r is the reference's candidate sequence for the query "r's stored f32 bits" (probed lists in
 * shard visiting order, probe rank, list position), less what the filter does not admit, less — with exclude_self != 0 —
 * the ONE candidate that is r itself (the same list and position, i.e. the same slot: a record with the same external
 * id, or with the same bits under another id, stays), stably sorted, take_while(d <= radius2) in f32, inclusive, on the
 * reference's scalar-order sum.  exclude_self == 0 gives bit for bit what vi_indexer_range_search_device returns for the
 * stored bits as queries: lims, D, I and tie.  If r's own list is not among the probed ones nothing is deleted.  A row
 * exists for every named record whether or not the filter admits that record (f == NULL: no filter).
 *   by ids:       an id names the first record in list order that carries it (the record vi_indexer_get_records returns);
 *                 found[i] = resident records carrying it (the get's count_out).  An absent id is no error: its row is
 *                 empty (lims[i + 1] == lims[i]) and found[i] = 0.  Ids may repeat, in any order; any u64 is an id.
 *                 ext_ids_dev / found_dev of the *_device entry are device pointers; found / found_dev may be NULL.
 *   radius_graph: rows = records [first, first + count) of LIST ORDER (row j is the record vi_indexer_export_records
 *                 returns as row j); first + count > vi_indexer_num_vectors is VI_ERR_INVALID_INPUT.  One entry point:
 *                 the result lives on the device either way.
 * radius2 NaN: VI_ERR_INVALID_INPUT; negative: VI_OK, nq empty rows, found still filled; +inf: everything probed less
 * what is deleted; radius2 = 0 with exclusion: exactly the OTHER records whose distance bits are 0.  n_probe is clamped
 * to max_n_probe; 0 is VI_ERR_INVALID_INPUT.  Partitioned handles (world_size > 1) are VI_ERR_INVALID_INPUT.  nq == 0 /
 * count == 0: what vi_indexer_range_search gives for nq == 0, a result of no rows.  The rows are processed in chunks of
 * VI_GRAPH_CHUNK (environment, default 65536) through one search context; the result is allocated at its true total
 * and at least doubles when a further chunk outgrows it.  The call is all or nothing: on any error — a result larger
 * than device memory is VI_ERR_DEVICE — *out stays NULL, found is not written, and the handle stays usable.
 * The result is an ordinary vi_range_result of the index: vi_range_result_total / _copy (V included) / _device /
 * _copy_device / _free and vi_range_merge_device take it unchanged.  Threads: the contract of a search.
 * vi_indexer_last_stats afterwards reads as after a radius search (of the last chunk), k = 0.  vi_similar_last_times
 * reports these calls too: ms_drop / drop_bytes then cover range_find_kernel and range_move_kernel. */
vi_status vi_indexer_range_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq,
                                         float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found,
                                         vi_range_result **out);
vi_status vi_indexer_range_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq,
                                                float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found_dev,
                                                vi_range_result **out);
vi_status vi_indexer_radius_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, float radius2,
                                  uint64_t n_probe, uint32_t exclude_self, vi_range_result **out);

/* ---- extension: clustering the stored records by radius ("which records are copies of each other, which form groups?") --
 * Connected components and DBSCAN labels of the index's own radius graph, without the graph ever leaving the device or
 * being held whole: one label and one degree per record.  labels and degree have N = vi_indexer_num_vectors(ix) entries
 * in LIST ORDER: entry j belongs to the record vi_indexer_export_records returns as row j.  The results are exact.
 *   Participants: the resident records f admits (f == NULL: all of them).
 *   Row R(j) of participant j: row j of vi_indexer_radius_graph(ix, f, 0, N, radius2, n_probe, exclude_self = 1), read as
 *              a set of records (slots) — the reference's candidate sequence for j's stored bits, less what the filter
 *              does not admit, less j's own slot, cut at d <= radius2 in f32, inclusive.  Rows of non-participants are
 *              ignored, and no non-participant is a hit: the filter deletes them.
 *   degree[j]  = |R(j)| for a participant, 0 otherwise.
 *   Adjacent:  a ~ b iff b is in R(a) or a is in R(b).  The probed lists make rows one-directional in places (a record
 *              whose own list is not probed is one example); the union closes that.
 *   Core:      a participant with degree + 1 >= min_pts.  min_pts 0 or 1: every participant.
 *   Clusters:  the connected components of the core records under ~ restricted to core-core pairs.  The label of a core
 *              record is the list-order ordinal of the lowest-ordinal record of its component, so labels[j] == j exactly
 *              for the representatives.
 *   Border:    a non-core participant adjacent to at least one core record; its label is the label of its adjacent core
 *              record with the lowest list-order ordinal (classic DBSCAN leaves this to the visiting order; here it is fixed).
 *   Noise:     every other participant.  Noise and every non-participant get VI_LABEL_NOISE.
 *   *n_clusters_out = the number of distinct labels >= 0.  It is a host pointer in both forms.
 * min_pts <= 1 is plain connected components, and radius2 = 0 then gives the groups of exact copies; min_pts >= 2 is
 * DBSCAN over the index's own approximate neighbourhoods.  labels == 0 .. N-1 elementwise is a vi_indexer_filter_mask;
 * vi_indexer_retain of it removes every duplicate but one.
 *   - n_probe is clamped to max_n_probe; 0 is VI_ERR_INVALID_INPUT.  radius2 NaN: VI_ERR_INVALID_INPUT; negative: VI_OK
 *     with no edges (min_pts <= 1: every participant its own cluster; otherwise all noise); +inf: everything probed is adjacent.
 *   - any output may be NULL; all three NULL is VI_ERR_INVALID_INPUT
 *   - VI_ERR_INVALID_INPUT before any device work, the outputs untouched: a null ix, a handle with no index, a filter of
 *     another handle or of a replaced index, a partitioned handle (world_size > 1)
 *   - all or nothing: on any later failure the outputs are not written and the handle stays usable; host outputs are
 *     staged on the device until every chunk has succeeded
 *   - threads: the contract of a search — the call is const on the handle, holds one search context for the whole call,
 *     and must not overlap an update.  Labels refer to the list order at call time: an update invalidates them.
 *   - the rows run in chunks of VI_GRAPH_CHUNK (environment, default 65536) as the graph calls do; no chunk's result
 *     outlives its chunk.  Beside one chunk's result the call holds 12 bytes and one bit per slot, freed on return.
 * Cost: every pass searches all N rows.  min_pts <= 1: one pass over the radius graph.  min_pts >= 2 with labels or
 * n_clusters_out asked for: two passes, degrees first and links second (whether a hit is core is not known until its own
 * row has been searched).  Only degree_out asked for: one pass.  The edges of the first pass are not kept to save the
 * second, and the rows of a selective filter are not compacted: all N rows are searched and the rows of non-participants
 * are skipped in the link step. */
#define VI_LABEL_NOISE (-1)
vi_status vi_indexer_cluster_radius(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe,
                                    uint32_t min_pts, int64_t *labels_out, uint32_t *degree_out, uint64_t *n_clusters_out);
vi_status vi_indexer_cluster_radius_device(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe,
                                           uint32_t min_pts, int64_t *labels_dev, uint32_t *degree_dev, uint64_t *n_clusters_out);
/* Of the calling thread's last vi_indexer_cluster_radius (either form); zeros after a failed one.  rows: N; hits: the sum
 * of the degrees; passes: 1 or 2 as above; n_core + n_border + n_noise = the participants; chunk_rows: rows per chunk
 * used; link_bytes: bytes the degree / link kernels read of the chunks' results, all passes.  With only degree_out asked
 * for nothing is clustered: n_core, n_border, n_noise and n_clusters are 0.  The ms_* are taken only while the
 * environment variable VI_SIMILAR_TIMING is set (and not "0"), summed over chunks and passes: host clock around the
 * gather of the queries (ms_resolve) and the radius search (ms_search), HIP events around cluster_degree_kernel /
 * cluster_link_kernel (ms_link) and cluster_label_kernel (ms_label). */
typedef struct vi_cluster_stats {
  uint64_t rows, hits, passes;
  uint64_t n_core, n_border, n_noise, n_clusters;
  uint64_t chunk_rows, link_bytes;
  float ms_resolve, ms_search, ms_link, ms_label;
} vi_cluster_stats;
vi_status vi_cluster_last_stats(vi_cluster_stats *out);

/* ---- extension: adaptive probing — per-query probe counts by distance ratio, code budget or list ---------------------
 * Every search entry above takes one n_probe for the whole batch.  Here n_probe is the UPPER bound and a rule decides,
 * per query, how many of its probes are searched: a prefix of its probe row.  For a row with `found` real probes in
 * coarse order, their exact coarse distances d_r (euclidean_distance_squared of the query and the centroid, the bits
 * the coarse step sorts by) and the full lengths of their lists, the number of probes kept is
 *
 *     p_q = clamp(min(p_ratio, p_codes, p_explicit),  lo = min(max(min_probe, 1), found),  hi = found)
 *
 *   p_ratio    = #{ r < found : d_r <= t },  t = fl32(ratio2 * d_0): one rounded f32 multiply, compared in f32.
 *                ratio2 == 0: off.  d_0 == 0 keeps exactly the centroids at distance bits 0.
 *   p_codes    = the smallest p >= 1 whose first p lists hold >= max_codes vectors together — the list that crosses the
 *                budget is still searched (Faiss's IndexIVF.max_codes) — or `found` if they never do.  max_codes == 0: off.
 *   p_explicit = n_probe_q[q].  NULL: off.
 *
 * Exactness is the library's: the pruned search of query q is, bit for bit, the search of q alone with n_probe = p_q —
 * ids, distance bits, counts, padding and tie keys.  (The reference sorts centroids by (distance, index), so a prefix of
 * a probe row is the probe row of a smaller n_probe, and its shard visiting order restricted to a prefix is the prefix's
 * own: the candidate-order ranks of the kept probes are the old ranks closed up.)  A zero-initialised rule prunes
 * nothing, and pruning is idempotent: a row that already carries markers is pruned over its real probes.
 *
 *   vi_indexer_prune_probes_device   in place, between vi_indexer_probe_device and vi_indexer_search_probed_device (the
 *                                    multi-GPU seam): probes r >= p_q of a row and their order words become the marker
 *                                    0xFFFFFFFF, the orders of the kept probes are closed up.  queries_dev: the nq
 *                                    queries the rows belong to; rows as vi_indexer_search_probed_device takes them
 *                                    (anything else is VI_ERR_INVALID_INPUT); n_kept_dev (optional, nq u32): p_q.
 *   vi_indexer_search_adaptive       one call: the coarse step ONCE, the prune, the list phase over the pruned rows, all
 *   vi_indexer_search_adaptive_device  on the device.  Outputs as vi_indexer_search_filtered / _filtered_device, plus
 *                                    n_probed (optional, nq u32: p_q).  f == NULL: no filter.
 *   - n_probe is clamped to max_n_probe and k to max_k, as always (k_out); a zero rule returns bit for bit what
 *     vi_indexer_search_filtered* returns: D, I, tie, counts and V
 *   - VI_ERR_INVALID_INPUT before any device work, outputs untouched: a null ix or rule; a handle with no index; ratio2
 *     NaN, infinite, negative or in (0, 1); n_probe == 0 or k == 0; a query_dim mismatch; a foreign or stale filter;
 *     max_codes != 0 on a partitioned handle (its lists hold resident lengths only).  The ratio and the explicit rule
 *     work on partitioned handles: the coarse table is replicated, every rank prunes alike
 *   - vi_indexer_last_stats afterwards reads as after the underlying search; its scanned_vectors is where the saving shows
 *   - threads: the contract of a search
 *   - n_probe_q: host memory for vi_indexer_search_adaptive, device memory for the two _device entries
 * Out of scope: radius search, the calls whose queries are stored records, and clustering take no rule.
 * vi_prune_last_stats: of the calling thread's last call of the three — the real probes its rows held, the probes kept,
 * and, only while the environment variable VI_PRUNE_TIMING is set (and not "0"), the HIP-event time of
 * probe_prune_kernel (zero otherwise).  Zeros after a call that failed or pruned nothing (nq == 0, an empty index: its
 * n_probed is all zero).  Any of the three pointers may be NULL, not all. */
typedef struct vi_probe_rule {
  uint32_t min_probe;        /* 0 => 1 */
  float    ratio2;           /* 0 = off; else finite and >= 1 */
  uint64_t max_codes;        /* 0 = off */
  const uint32_t *n_probe_q; /* NULL = off; nq entries, host memory for the host entry, device for _device */
} vi_probe_rule;
vi_status vi_indexer_prune_probes_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t n_probe_eff,
                                         uint32_t *probes_dev, uint32_t *order_dev, const vi_probe_rule *rule,
                                         uint32_t *n_kept_dev);
vi_status vi_indexer_search_adaptive(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule, const float *queries,
                                     uint64_t nq, uint32_t query_dim, uint64_t k, uint64_t n_probe, float *D, int64_t *I,
                                     float *V, uint64_t *counts, uint32_t *n_probed, uint64_t *k_out);
vi_status vi_indexer_search_adaptive_device(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule,
                                            const float *queries_dev, uint64_t nq, uint64_t k, uint64_t n_probe,
                                            float *D_dev, int64_t *I_dev, uint64_t *tie_dev, uint32_t *n_probed_dev);
vi_status vi_prune_last_stats(uint64_t *probes_in, uint64_t *probes_kept, float *ms_prune);

/* Merge `parts` per-rank partial results (each nq x k, device pointers laid out
 * [part][nq][k]) into the global top-k with the reference's stable order. */
vi_status vi_merge_partials_device(int32_t device, uint64_t nq, uint64_t k, uint32_t parts,
                                   const float *D_parts, const int64_t *I_parts,
                                   const uint64_t *tie_parts, float *D_out, int64_t *I_out);

/* The same merge for results PACKED per rank as [D f32 nq*k | pad to 8 B | I i64 nq*k | tie u64 nq*k]
 * (vi_packed_result_bytes(nq, k) bytes; point vi_indexer_search*_device's D / I / tie outputs into one such buffer):
 * the ranks then exchange their partial results with ONE all-gather instead of three. */
uint64_t vi_packed_result_bytes(uint64_t nq, uint64_t k);
vi_status vi_merge_partials_packed_device(int32_t device, uint64_t nq, uint64_t k, uint32_t parts,
                                          const void *packed_dev, float *D_out, int64_t *I_out);

/* ---- extension: merging per-rank radius results ---------------------------------------------------------------------
 * The radius results of the ranks of a partitioned index, for the same nq queries, merged into the result the
 * unpartitioned index gives: ids, distance bits, tie keys, order and per-query counts.  Every part is CSR (lims nq + 1;
 * D / I / tie of lims[nq] entries) with each row sorted by (distance bits, tie), which is how
 * vi_indexer_range_search_device leaves it; the output row of query q is the parts' rows q merged on that key and
 * lims[q] is the sum of the parts' lims[q].
 *   - the pointer arrays serve both uses: in-process ranks pass what vi_range_result_device returned; after an
 *     all-gather into one buffer the pointers are base + r * stride
 *   - the result is an ordinary vi_range_result that belongs to no index: _total, _device (tie included), _free and
 *     _copy with V == NULL work as for any result; _copy with V != NULL is VI_ERR_INVALID_INPUT (the stored vectors
 *     live on the ranks).  It owns its buffers and stays valid after the parts and their indexers are freed
 *   - parts == 1 is a copy; a part or a row without entries is legal; no entry at all is VI_OK with lims all zero;
 *     nq == 0 is VI_OK with the one lims entry 0, as a radius search of no query
 *   - sortedness is NOT checked: parts whose rows are not sorted give an unspecified order inside each row, never an
 *     access outside the buffers (lims must be non-decreasing CSR offsets).  Equal keys in two parts (the same rank
 *     passed twice) come out lower part first
 *   - errors, all VI_ERR_INVALID_INPUT before any device work: out == NULL, a NULL array, parts == 0 or > 64, a NULL
 *     lims pointer, a NULL D / I / tie pointer of a part.  Then: no device, or an ordinal out of range, is
 *     VI_ERR_DEVICE; there is no CPU fallback.  All or nothing: on any failure *out stays NULL
 *   - one stream, one host synchronisation before the output is allocated (the total sizes it), complete on return
 * lims_dev / D_dev / I_dev / tie_dev: HOST arrays of `parts` DEVICE pointers (part p: lims nq+1, the rest lims_p[nq] each). */
vi_status vi_range_merge_device(int32_t device, uint64_t nq, uint32_t parts,
                                const uint64_t *const *lims_dev, const float *const *D_dev,
                                const int64_t *const *I_dev, const uint64_t *const *tie_dev,
                                vi_range_result **out);
/* HIP-event times of the calling thread's last vi_range_merge_device, taken only while the environment variable
 * VI_RANGE_MERGE_TIMING is set (and not "0"); zeros otherwise.  ms_alloc: between the two kernels — the read-back of
 * lims, the synchronisation, the allocations.  Any pointer may be NULL. */
vi_status vi_range_merge_last_times(float *ms_lims, float *ms_alloc, float *ms_place);

/* accessors */
uint32_t vi_indexer_dimension(const vi_indexer *ix);
uint64_t vi_indexer_num_centroids(const vi_indexer *ix);
uint64_t vi_indexer_num_vectors(const vi_indexer *ix); /* resident on this rank */
uint64_t vi_indexer_num_shards(const vi_indexer *ix);
/* centroids (k' x dim) and centroids_to_shard (k') of the loaded index */
vi_status vi_indexer_centroids(const vi_indexer *ix, float *centroids_out, uint64_t *c2s_out);
void vi_indexer_free(vi_indexer *ix);

/* ---- instrumentation (bench.py / profiling) ---------------------------------------- */
typedef struct vi_search_stats {
  uint64_t nq, k, n_probe_eff;
  uint64_t coarse_candidates;  /* nq * k' */
  uint64_t scanned_vectors;    /* Σ over queries of Σ len(probed lists resident here) */
  uint64_t scan_items;         /* (list, query-group) work items of the list-scan kernel */
  float ms_total, ms_coarse, ms_group, ms_scan, ms_merge; /* HIP-event times on the search stream */
  uint64_t fallback_queries;   /* always 0 (kept for ABI stability: the MFMA path has no fallback) */
  uint64_t filter_tile_blocks; /* MFMA path: (128-query group, 64-vector block) tiles ranked; 0 on the VALU engine */
  uint64_t filter_rechecked;   /* VI_FILTER_STATS=1: (query, vector) pairs re-evaluated in exact order */
  uint64_t filter_accepted;    /* VI_FILTER_STATS=1: block records consulted */
  uint64_t rank_mode;          /* list scan of the last search: 0 exact-order VALU engine, 1 f32 MFMA,
                                  2 bf16 x 3 MFMA, 3 bf16 MFMA on hi planes only (bf16-exact stored values),
                                  4 bf16 MFMA on the hi planes of real-valued lists (wider margin, more exact re-evaluations),
                                  5 / 6 = 2 / 4 with the images taken about the mean of the stored vectors (real-valued
                                  lists far from the origin: the margins scale with the spread, not the offset) */
  uint64_t group_queries;      /* MFMA path: queries per rank work item (128, or 32 when lists are probed by few) */
  uint64_t rank_int8;          /* 1: the list rank multiplied int8 images (8-bit descriptors, integer queries in 0..254; rank_mode 3) */
} vi_search_stats;
/* phases of the most recent build on this handle (wall-clock ms): the points are uploaded once; k-means, the grouping of
 * ids by list, the shard export and the resident index all work from that device copy */
typedef struct vi_build_stats {
  uint64_t n, nlist, lists, shards;  /* points, requested lists, non-empty lists, shard files */
  uint64_t shard_bytes;              /* record bytes written to the shard files */
  float ms_total, ms_upload, ms_kmeans, ms_group, ms_super, ms_export, ms_index;
} vi_build_stats;
vi_status vi_indexer_last_build_stats(const vi_indexer *ix, vi_build_stats *out);
/* the most recent vi_indexer_add_records on this handle that added something (wall-clock ms unless said otherwise) */
typedef struct vi_add_stats {
  uint64_t n;                /* records added */
  uint64_t lists_touched;    /* lists that received records */
  uint64_t shards_rewritten; /* shard files rewritten */
  uint64_t bytes_written;    /* bytes of those files */
  float ms_total;
  float ms_assign;           /* upload, labels (coarse step), grouping by list */
  float ms_files;            /* new shard files written and renamed */
  float ms_index;            /* new resident index: update_blocks_kernel + the ranking images */
  float ms_kernel;           /* HIP-event time of update_blocks_kernel alone (part of ms_index) ... */
  uint64_t kernel_bytes;     /* ... and the bytes it read and wrote */
} vi_add_stats;
vi_status vi_indexer_last_add_stats(const vi_indexer *ix, vi_add_stats *out);
/* the most recent vi_indexer_retain / vi_indexer_remove_ids on this handle that removed something (wall-clock ms unless
 * said otherwise) */
typedef struct vi_remove_stats {
  uint64_t n_removed;        /* records removed */
  uint64_t lists_touched;    /* lists that lost records ... */
  uint64_t lists_emptied;    /* ... and of them, lists that lost their last */
  uint64_t shards_rewritten; /* shard files rewritten */
  uint64_t bytes_written;    /* bytes of those files */
  float ms_total;
  float ms_plan;             /* the allow words read back, the touched lists and shards found */
  float ms_files;            /* new shard files written and renamed */
  float ms_index;            /* new resident index: kept_count_kernel, update_blocks_kernel + the ranking images */
  float ms_kernel;           /* HIP-event time of update_blocks_kernel alone (part of ms_index) ... */
  uint64_t kernel_bytes;     /* ... and the bytes it read and wrote */
} vi_remove_stats;
vi_status vi_indexer_last_remove_stats(const vi_indexer *ix, vi_remove_stats *out);
/* the most recent vi_indexer_upsert_records on this handle with n > 0 (wall-clock ms unless said otherwise) */
typedef struct vi_upsert_stats {
  uint64_t n;                /* records added */
  uint64_t n_replaced;       /* records removed */
  uint64_t lists_touched;    /* lists that lost or received records ... */
  uint64_t lists_emptied;    /* ... and of them, lists that lost their last and received none */
  uint64_t shards_rewritten; /* shard files rewritten, each once */
  uint64_t bytes_written;    /* bytes of those files */
  float ms_total;
  float ms_plan;             /* upload, deny filter, labels (coarse step), grouping, allow words read back */
  float ms_files;            /* new shard files written and renamed */
  float ms_index;            /* new resident index: kept_count_kernel, update_blocks_kernel + the ranking images */
  float ms_kernel;           /* HIP-event time of update_blocks_kernel alone (part of ms_index) ... */
  uint64_t kernel_bytes;     /* ... and the bytes it read and wrote */
} vi_upsert_stats;
vi_status vi_indexer_last_upsert_stats(const vi_indexer *ix, vi_upsert_stats *out);
/* the most recent vi_indexer_get_records* / vi_indexer_export_records* on this handle (n > 0 / count > 0).  The ms_* are
 * HIP-event times on the call's stream, non-zero only under vi_indexer_enable_timing; an export has no table and no match */
typedef struct vi_fetch_stats {
  uint64_t n;             /* ids requested / records exported */
  uint64_t n_found;       /* requested ids (repeats counted) that a resident record carries / records exported */
  uint64_t slots_scanned; /* get: resident records whose external id was probed; export: slots of the blocks read */
  uint64_t bytes_moved;   /* device bytes the kernels read and wrote (the request, the scan, the rows in and out) */
  float ms_total;
  float ms_table;         /* get: clearing the id table and inserting the request */
  float ms_match;         /* get: fetch_match_kernel, the scan of the resident external ids */
  float ms_gather;        /* get: fetch_resolve_gather_kernel; export: export_blocks_kernel */
} vi_fetch_stats;
vi_status vi_indexer_last_fetch_stats(const vi_indexer *ix, vi_fetch_stats *out);

/* stats of the most recent search on this handle (timing collected only if enabled) */
vi_status vi_indexer_last_stats(const vi_indexer *ix, vi_search_stats *out);
/* enable: 0 off; 1 HIP events at every phase boundary of a search (ms_total / ms_coarse / ms_group / ms_scan / ms_merge);
 * 2 around the list-rank kernel only (ms_scan; the others read 0) — every event record is a barrier packet on the search
 * stream, five of them cost about 0.01 ms per search */
void vi_indexer_enable_timing(vi_indexer *ix, int enable);

#ifdef __cplusplus
}
#endif
#endif /* VI_AMD_H */
