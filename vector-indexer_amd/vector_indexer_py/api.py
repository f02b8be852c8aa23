"""Mirror of the reference's public Rust API (src/api.rs) on top of the C ABI.

    VectorIndexerConfig.new(dimension).with_index_dir(..).with_shards_dir(..)      api.rs:32-54
    VectorRecord(external_id, values, timestamp=None)                              api.rs:57-62
    SearchRequest(query, include_vectors, k, n_probe) + with_*                     api.rs:64-87
    SearchResult(external_id, distance, vector)                                    api.rs:89-94
    VectorIndexer.new(cfg) / .load(cfg) / .build_from_records / .build_from_vector_file /
    .search(req) / .search_request(query) / .config()                             api.rs:101-237
    .range_search(query, radius2, ...)                                            extension: everything within a radius
    .add_records(records)                                                         extension: append to a built index
    .remove_records(external_ids) -> int                                          extension: remove from a built index
    .upsert_records(records) -> int                                               extension: replace by external id
    .refine_lists(iters=1) -> int                                                 extension: recentre lists, re-home records
    .rebalance_lists(rule=None, **fields) -> int                                  extension: ... and split overfull lists into empty ones
    .get_records(external_ids) -> [VectorRecord or None]                          extension: read back by external id
    .search_similar(external_id, k, n_probe, ...) -> [SearchResult] or None       extension: neighbours of a stored record
    .range_search_similar(external_id, radius2, ...) -> [SearchResult] or None    extension: ... within a radius of it
    .duplicate_groups(radius2=0.0, n_probe, min_size=2) -> [[external_id]]        extension: groups of (near-)copies
    SearchRequest.with_timestamp_range / .with_allowed_ids / .with_excluded_ids   extension: filtered search
    SearchRequest.with_probe_ratio(ratio2, min_probe=1) / .with_max_codes(n)      extension: adaptive probing

Errors are ViError (a RuntimeError) whose .kind is the io::ErrorKind name the reference returns.
"""
import ctypes as C
import hashlib
from dataclasses import dataclass, field, replace
from typing import List, Optional, Tuple

import numpy as np

from . import _native
from ._native import ViError, lib


@dataclass
class VectorIndexerConfig:
    dimension: int
    index_dir: str = "index"
    shards_dir: str = "shards"
    default_k: int = 10
    default_n_probe: int = 20
    max_k: int = 10_000
    max_n_probe: int = 10_000
    # extensions (zero = reference behaviour)
    nlist_override: int = 0
    seed: int = 0
    assign_mode: int = 0
    device: int = 0
    rank: int = 0
    world_size: int = 0
    now_secs: int = 0

    @staticmethod
    def new(dimension: int) -> "VectorIndexerConfig":
        return VectorIndexerConfig(dimension)

    def with_index_dir(self, index_dir) -> "VectorIndexerConfig":
        return replace(self, index_dir=str(index_dir))

    def with_shards_dir(self, shards_dir) -> "VectorIndexerConfig":
        return replace(self, shards_dir=str(shards_dir))


@dataclass
class VectorRecord:
    external_id: int
    values: List[float]
    timestamp: Optional[int] = None


@dataclass(frozen=True, eq=False)
class IdSelector:
    """a set of external ids a search is restricted to (exclude=False) or kept away from (exclude=True): the ids sorted,
    unique, uint64 and read-only; `key` names the set in the indexer's filter cache"""
    ids: np.ndarray
    exclude: bool
    digest: str

    @staticmethod
    def of(ids, exclude: bool) -> "IdSelector":
        a = np.unique(_native.id_array(ids))
        a.setflags(write=False)
        return IdSelector(a, bool(exclude), hashlib.sha256(a.tobytes()).hexdigest())

    @property
    def key(self):
        return ("ids", self.exclude, int(self.ids.size), self.digest)


@dataclass
class SearchRequest:
    query: List[float]
    include_vectors: bool = False
    k: int = 10
    n_probe: int = 20
    # extension: only records whose stored timestamp lies in [lo, hi], both inclusive (None: all, the reference's search)
    timestamp_range: Optional[Tuple[int, int]] = None
    # extension: only records whose external id is in a set / is not in a set (None: all); with timestamp_range: both
    id_selector: Optional[IdSelector] = None
    # extension: adaptive probing — n_probe is the upper bound; the probes whose centroid distance exceeds probe_ratio2 x
    # the nearest one's are dropped (0.0: off), and probing stops once the probed lists hold max_codes vectors (0: off)
    probe_ratio2: float = 0.0
    min_probe: int = 1
    max_codes: int = 0

    def with_probe_ratio(self, ratio2, min_probe=1):
        return replace(self, probe_ratio2=float(ratio2), min_probe=int(min_probe))

    def with_max_codes(self, n):
        return replace(self, max_codes=int(n))

    def with_k(self, k):
        return replace(self, k=k)

    def with_n_probe(self, n_probe):
        return replace(self, n_probe=n_probe)

    def with_include_vectors(self, include_vectors):
        return replace(self, include_vectors=include_vectors)

    def with_timestamp_range(self, lo, hi):
        return replace(self, timestamp_range=(int(lo), int(hi)))

    def with_allowed_ids(self, ids):
        return replace(self, id_selector=IdSelector.of(ids, False))

    def with_excluded_ids(self, ids):
        return replace(self, id_selector=IdSelector.of(ids, True))


@dataclass
class SearchResult:
    external_id: int
    distance: float
    vector: Optional[List[float]] = field(default=None)


class VectorIndexer:
    def __init__(self, cfg: VectorIndexerConfig, handle):
        self._cfg = cfg
        self._h = handle
        self._filters = {}  # (lo, hi) / IdSelector.key / (both) -> native filter of the resident index

    def _drop_filters(self):
        filters, self._filters = getattr(self, "_filters", {}), {}
        for f in filters.values():
            lib().vi_filter_free(f)

    def __del__(self):
        self._drop_filters()  # (before their indexer)
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().vi_indexer_free(h)

    def _filter(self, rng, selector: Optional[IdSelector] = None):
        """the native filter of a timestamp window, an id selector, or both (their intersection); None: no filter"""
        tkey = None if rng is None else (int(rng[0]), int(rng[1]))
        ikey = None if selector is None else selector.key
        if tkey is None or ikey is None:
            key = tkey if ikey is None else ikey
            if key is None:
                return None
        else:
            key = (tkey, ikey)
        if key in self._filters:
            return self._filters[key]
        missing = [k for k in {tkey, ikey, key} if k is not None and k not in self._filters]
        if len(self._filters) + len(missing) > 16:  # (a filter holds device memory in proportion to the index)
            self._drop_filters()
        if tkey is not None and tkey not in self._filters:
            f = C.c_void_p()
            _native.check(lib().vi_indexer_filter_timestamps(self._h, tkey[0], tkey[1], C.byref(f)))
            self._filters[tkey] = f
        if ikey is not None and ikey not in self._filters:
            f, ids = C.c_void_p(), selector.ids
            _native.check(lib().vi_indexer_filter_ids(self._h, _native.ptr(ids) if ids.size else None, ids.size,
                                                      _native.VI_IDS_DENY if selector.exclude else _native.VI_IDS_ALLOW,
                                                      C.byref(f)))
            self._filters[ikey] = f
        if key not in self._filters:
            f = C.c_void_p()
            _native.check(lib().vi_filter_intersect(self._h, self._filters[tkey], self._filters[ikey], C.byref(f)))
            self._filters[key] = f
        return self._filters[key]

    @staticmethod
    def _native_cfg(cfg: VectorIndexerConfig):
        c = _native.Config()
        lib().vi_config_init(C.byref(c), int(cfg.dimension))
        keep = (cfg.index_dir.encode(), cfg.shards_dir.encode())
        c.index_dir, c.shards_dir = keep
        for f in ("default_k", "default_n_probe", "max_k", "max_n_probe", "nlist_override", "seed", "assign_mode",
                  "device", "rank", "world_size", "now_secs"):
            setattr(c, f, int(getattr(cfg, f)))
        return c, keep

    @staticmethod
    def new(cfg: VectorIndexerConfig) -> "VectorIndexer":
        c, keep = VectorIndexer._native_cfg(cfg)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_new(C.byref(c), C.byref(h)))
        return VectorIndexer(cfg, h)

    @staticmethod
    def load(cfg: VectorIndexerConfig) -> "VectorIndexer":
        c, keep = VectorIndexer._native_cfg(cfg)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_load(C.byref(c), C.byref(h)))
        return VectorIndexer(cfg, h)

    def build_from_records(self, records: List[VectorRecord]) -> "VectorIndexer":
        self._drop_filters()  # (they describe the index this build replaces)
        n = len(records)
        dim = self._cfg.dimension
        dims = np.array([len(r.values) for r in records], dtype=np.uint32)
        vals = np.zeros((n, dim), dtype=np.float32)
        for i, r in enumerate(records):
            if len(r.values) == dim:
                vals[i] = np.asarray(r.values, dtype=np.float32)
        ext = np.array([r.external_id for r in records], dtype=np.uint64)
        ts = np.array([r.timestamp or 0 for r in records], dtype=np.uint64)  # unwrap_or(0), api.rs:138
        _native.check(lib().vi_indexer_build_from_records(self._h, _native.ptr(ext), _native.ptr(vals), _native.ptr(ts),
                                                          _native.ptr(dims), n))
        return self

    def add_records(self, records: List[VectorRecord]) -> "VectorIndexer":
        """extension: append records to the built or loaded index, each to the list of its nearest centroid (files and
        resident index; nothing is retrained).  An empty list changes nothing."""
        n = len(records)
        dim = self._cfg.dimension
        for i, r in enumerate(records):
            if len(r.values) != dim:  # (the message of build_from_records, api.rs:122-133)
                raise ViError(_native.VI_ERR_INVALID_INPUT,
                              f"vector dimension mismatch at index {i}: expected {dim}, got {len(r.values)}")
        if n == 0:
            return self
        vals = np.ascontiguousarray([r.values for r in records], dtype=np.float32).reshape(n, dim)
        ext = np.array([r.external_id for r in records], dtype=np.uint64)
        ts = np.array([r.timestamp or 0 for r in records], dtype=np.uint64)
        self._drop_filters()  # (cached filters describe the index this call replaces)
        _native.check(lib().vi_indexer_add_records(self._h, _native.ptr(ext), _native.ptr(vals), _native.ptr(ts), n))
        return self

    def remove_records(self, external_ids) -> int:
        """extension: remove every record whose external id is in external_ids from the built or loaded index (files and
        resident index; unknown ids are ignored) -> records removed.  An empty set changes nothing."""
        ids = _native.id_array(external_ids)
        removed = C.c_uint64(0)
        self._drop_filters()  # (cached filters describe the index this call replaces)
        _native.check(lib().vi_indexer_remove_ids(self._h, _native.ptr(ids) if ids.size else None, ids.size, C.byref(removed)))
        return int(removed.value)

    def upsert_records(self, records: List[VectorRecord]) -> int:
        """extension: replace the stored records that carry the records' external ids by the records (files and resident
        index, one rewrite; ids nothing carries are added) -> records replaced.  An empty list changes nothing."""
        n = len(records)
        dim = self._cfg.dimension
        for i, r in enumerate(records):
            if len(r.values) != dim:  # (the message of build_from_records, api.rs:122-133)
                raise ViError(_native.VI_ERR_INVALID_INPUT,
                              f"vector dimension mismatch at index {i}: expected {dim}, got {len(r.values)}")
        if n == 0:
            return 0
        vals = np.ascontiguousarray([r.values for r in records], dtype=np.float32).reshape(n, dim)
        ext = np.array([r.external_id for r in records], dtype=np.uint64)
        ts = np.array([r.timestamp or 0 for r in records], dtype=np.uint64)
        replaced = C.c_uint64(0)
        self._drop_filters()  # (cached filters describe the index this call replaces)
        _native.check(lib().vi_indexer_upsert_records(self._h, _native.ptr(ext), _native.ptr(vals), _native.ptr(ts), n,
                                                      C.byref(replaced)))
        return int(replaced.value)

    def refine_lists(self, iters: int = 1) -> int:
        """extension: recentre the lists of the built or loaded index on the records they hold and re-home every record
        to its nearest centroid, `iters` times (files and resident index, one rewrite) -> records whose list changed.
        iters == 0 changes nothing."""
        moved = C.c_uint64(0)
        if int(iters) > 0:
            self._drop_filters()  # (cached filters describe the index this call replaces)
        _native.check(lib().vi_indexer_refine(self._h, int(iters), C.byref(moved)))
        return int(moved.value)

    def rebalance_lists(self, rule=None, **fields) -> int:
        """extension: refine_lists whose first iterations split overfull lists into the empty ones (a RebalanceRule of
        vector_indexer_py, or its fields) -> records whose list changed"""
        from . import RebalanceRule
        if rule is None:
            rule = RebalanceRule(**fields)
        elif fields:
            raise TypeError("give a rule or its fields, not both")
        moved = C.c_uint64(0)
        r = rule._native_rule()
        self._drop_filters()  # (cached filters describe the index this call replaces)
        _native.check(lib().vi_indexer_rebalance(self._h, C.byref(r), C.byref(moved)))
        return int(moved.value)

    def get_records(self, external_ids) -> List[Optional[VectorRecord]]:
        """extension: the stored record of every id, in request order: its vector and timestamp as they are stored (of the
        first record in list order where several carry the id); None for an id nothing carries"""
        ids = _native.id_array(external_ids)
        n, dim = ids.size, self._cfg.dimension
        cnt, ts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        vals = np.zeros((n, dim), dtype=np.float32)
        _native.check(lib().vi_indexer_get_records(self._h, _native.ptr(ids) if n else None, n, _native.ptr(cnt),
                                                   _native.ptr(vals), _native.ptr(ts), None))
        return [VectorRecord(int(ids[i]), vals[i].tolist(), int(ts[i])) if cnt[i] else None for i in range(n)]

    def build_from_vector_file(self, path) -> "VectorIndexer":
        self._drop_filters()
        _native.check(lib().vi_indexer_build_from_vector_file(self._h, str(path).encode()))
        return self

    def search(self, req: SearchRequest) -> List[SearchResult]:
        q = np.ascontiguousarray(np.asarray(req.query, dtype=np.float32).reshape(1, -1))
        k = max(int(req.k), 0)
        kcap = min(k, self._cfg.max_k)
        D = np.full((1, max(kcap, 1)), np.inf, dtype=np.float32)
        I = np.full((1, max(kcap, 1)), -1, dtype=np.int64)
        V = np.zeros((1, max(kcap, 1), self._cfg.dimension), dtype=np.float32) if req.include_vectors else None
        cnt = np.zeros(1, dtype=np.uint64)
        kout = C.c_uint64(0)
        flt = self._filter(req.timestamp_range, req.id_selector)
        if req.probe_ratio2 != 0.0 or req.max_codes != 0:  # adaptive probing
            rule = _native.ProbeRuleC(int(req.min_probe), float(req.probe_ratio2), int(req.max_codes), None)
            _native.check(lib().vi_indexer_search_adaptive(self._h, flt, C.byref(rule), _native.ptr(q), 1, q.shape[1], k,
                                                           int(req.n_probe), _native.ptr(D), _native.ptr(I), _native.ptr(V),
                                                           _native.ptr(cnt), None, C.byref(kout)))
        else:
            _native.check(lib().vi_indexer_search_filtered(self._h, flt, _native.ptr(q), 1,
                                                           q.shape[1], k, int(req.n_probe), _native.ptr(D), _native.ptr(I),
                                                           _native.ptr(V), _native.ptr(cnt), C.byref(kout)))
        return [SearchResult(int(I[0, j]), float(D[0, j]), V[0, j].tolist() if V is not None else None)
                for j in range(int(cnt[0]))]

    def range_search(self, query, radius2: float, n_probe: Optional[int] = None, include_vectors: bool = False,
                     timestamp_range: Optional[Tuple[int, int]] = None, allowed_ids=None,
                     excluded_ids=None) -> List[SearchResult]:
        """extension: every record of the probed lists within squared distance radius2 of the query, nearest first (the
        reference's stable order); n_probe None: the config's default_n_probe"""
        if allowed_ids is not None and excluded_ids is not None:
            raise ValueError("give allowed_ids or excluded_ids, not both")
        selector = (IdSelector.of(allowed_ids, False) if allowed_ids is not None
                    else IdSelector.of(excluded_ids, True) if excluded_ids is not None else None)
        q = np.ascontiguousarray(np.asarray(query, dtype=np.float32).reshape(1, -1))
        p = self._cfg.default_n_probe if n_probe is None else int(n_probe)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search(self._h, self._filter(timestamp_range, selector), _native.ptr(q), 1, q.shape[1],
                                                    float(radius2), p, C.byref(h)))
        try:
            n = int(lib().vi_range_result_total(h))
            lims = np.zeros(2, dtype=np.uint64)
            D, I = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64)
            V = np.zeros((n, self._cfg.dimension), dtype=np.float32) if include_vectors else None
            _native.check(lib().vi_range_result_copy(h, _native.ptr(lims), _native.ptr(D), _native.ptr(I), _native.ptr(V)))
        finally:
            lib().vi_range_result_free(h)
        return [SearchResult(int(I[j]), float(D[j]), V[j].tolist() if V is not None else None) for j in range(n)]

    def search_similar(self, external_id: int, k: Optional[int] = None, n_probe: Optional[int] = None,
                       include_vectors: bool = False, exclude_self: bool = True,
                       timestamp_range: Optional[Tuple[int, int]] = None, allowed_ids=None,
                       excluded_ids=None) -> Optional[List[SearchResult]]:
        """extension: the neighbours of the stored record that carries external_id (the first in list order where several
        do: the record get_records returns), nearest first; exclude_self drops that one record — not other records with
        its id or its vector — from its own result.  None for an id nothing carries.  k / n_probe None: the config's
        defaults.  The filters restrict the neighbours, not the record asked about."""
        if allowed_ids is not None and excluded_ids is not None:
            raise ValueError("give allowed_ids or excluded_ids, not both")
        selector = (IdSelector.of(allowed_ids, False) if allowed_ids is not None
                    else IdSelector.of(excluded_ids, True) if excluded_ids is not None else None)
        ids = _native.id_array([external_id])
        k = max(int(self._cfg.default_k if k is None else k), 0)
        p = self._cfg.default_n_probe if n_probe is None else int(n_probe)
        kcap = max(min(k, self._cfg.max_k), 1)
        D = np.full((1, kcap), np.inf, dtype=np.float32)
        I = np.full((1, kcap), -1, dtype=np.int64)
        V = np.zeros((1, kcap, self._cfg.dimension), dtype=np.float32) if include_vectors else None
        cnt, found = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
        kout = C.c_uint64(0)
        _native.check(lib().vi_indexer_search_by_ids(self._h, self._filter(timestamp_range, selector), _native.ptr(ids), 1, k, p,
                                                     1 if exclude_self else 0, _native.ptr(D), _native.ptr(I), _native.ptr(V),
                                                     _native.ptr(cnt), _native.ptr(found), C.byref(kout)))
        if not found[0]:
            return None
        return [SearchResult(int(I[0, j]), float(D[0, j]), V[0, j].tolist() if V is not None else None)
                for j in range(int(cnt[0]))]

    def range_search_similar(self, external_id: int, radius2: float, n_probe: Optional[int] = None,
                             include_vectors: bool = False, exclude_self: bool = True) -> Optional[List[SearchResult]]:
        """extension: every record of the probed lists within squared distance radius2 of the stored record that carries
        external_id (the first in list order where several do), nearest first; exclude_self drops that one record — not
        other records with its id or its vector — from its own result.  None for an id nothing carries.  n_probe None:
        the config's default_n_probe."""
        ids = _native.id_array([external_id])
        p = self._cfg.default_n_probe if n_probe is None else int(n_probe)
        found = np.zeros(1, dtype=np.uint32)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search_by_ids(self._h, None, _native.ptr(ids), 1, float(radius2), p,
                                                           1 if exclude_self else 0, _native.ptr(found), C.byref(h)))
        try:
            n = int(lib().vi_range_result_total(h))
            lims = np.zeros(2, dtype=np.uint64)
            D, I = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64)
            V = np.zeros((n, self._cfg.dimension), dtype=np.float32) if include_vectors else None
            _native.check(lib().vi_range_result_copy(h, _native.ptr(lims), _native.ptr(D), _native.ptr(I), _native.ptr(V)))
        finally:
            lib().vi_range_result_free(h)
        if not found[0]:
            return None
        return [SearchResult(int(I[j]), float(D[j]), V[j].tolist() if V is not None else None) for j in range(n)]

    def duplicate_groups(self, radius2: float = 0.0, n_probe: Optional[int] = None, min_size: int = 2) -> List[List[int]]:
        """extension: the clusters of stored records chained by squared distance <= radius2 (0.0: exact copies) that have
        at least min_size members, as lists of external ids — members in list order, groups ordered by their first
        member.  The connected components of the index's radius graph over the probed lists, made on the GPU; only one
        label per record comes back.  n_probe None: the config's default_n_probe."""
        p = self._cfg.default_n_probe if n_probe is None else int(n_probe)
        n = int(lib().vi_indexer_num_vectors(self._h))
        labels, ids = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.uint64)
        _native.check(lib().vi_indexer_cluster_radius(self._h, None, float(radius2), p, 1, _native.ptr(labels), None, None))
        if n:
            _native.check(lib().vi_indexer_export_records(self._h, 0, n, _native.ptr(ids), None, None, None))
        order = np.argsort(labels, kind="stable")          # by representative, list order inside a group
        reps, start, size = np.unique(labels[order], return_index=True, return_counts=True)
        return [[int(e) for e in ids[order[s:s + c]]] for r, s, c in zip(reps, start, size) if r >= 0 and c >= max(int(min_size), 1)]

    def search_request(self, query) -> SearchRequest:
        return SearchRequest(list(query), False, self._cfg.default_k, self._cfg.default_n_probe)

    def config(self) -> VectorIndexerConfig:
        return self._cfg
