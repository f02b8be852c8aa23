"""vector_indexer_py — ctypes mirror of the reference's Python module, on top of libvi_amd.so.

Reference contract (bindings/python/src/lib.rs:120-325 and
bindings/python/python/vector_indexer_py/__init__.py):

    build(xb, work_dir=None) -> VectorIndex       external_id = row index, dirs <work_dir>/{index,shards}
    load(index_dir, shards_dir, dimension) -> VectorIndex
    suggest_nlist(n) -> int
    VectorIndex.search(xq, k, n_probe)   (coroutine) -> (D f32[nq,k], I i64[nq,k])   +inf / -1 padded
    VectorIndex.search_sync(xq, k, n_probe)
    VectorIndex.dimension
    VectorIndex.add(xb, ext_ids=None, timestamps=None)      extension: append records to a built or loaded index
    VectorIndex.remove_ids(ids) / .retain(filter) -> int    extension: remove records from it (by id / all a filter excludes)
    VectorIndex.upsert(xb, ext_ids, timestamps=None) -> int extension: replace the records that carry ext_ids, in one rewrite
    VectorIndex.refine(iters=1) -> int / .list_stats()      extension: recentre the lists and re-home the records / list balance
    VectorIndex.rebalance(rule=None, **fields) -> int       extension: a refine whose first iterations split overfull lists
                                                            into the empty ones (RebalanceRule)
    VectorIndex.get(ids) / .export(first, count)            extension: read records back, by id / a range in list order
    VectorIndex.filter_timestamps / _ids / _id_range / _mask / _compose(terms)   extension: filters for `filter=`; of two
                                                            filters a & b, a | b, a - b and ~a are filters too
    VectorIndex.search_adaptive_sync(xq, k, n_probe, rule)  extension: n_probe as an upper bound, a ProbeRule deciding each
                                                            query's own probe count (distance ratio, code budget, per query)
    merge_range_results(device, parts) -> RangeResult       extension: the radius results of the ranks of a partitioned
                                                            index merged on the device into the unpartitioned result

Errors surface as RuntimeError, as PyO3's PyRuntimeError does.  There is NO CPU fallback: if
libvi_amd.so is missing or no MI355X is visible, build/load/search raise.
"""
import asyncio
import ctypes as C
import os
import tempfile
from typing import Optional, Tuple, Union

import numpy as np

from . import _native
from ._native import (ViError, lib, VI_ASSIGN_EXACT, VI_ASSIGN_REFERENCE, VI_ORDER_LANES, VI_ORDER_SCALAR)

__all__ = ["build", "load", "suggest_nlist", "VectorIndex", "ProbeRule", "RebalanceRule", "TimestampFilter", "IdFilter", "FilterIntersection", "ComposedFilter", "Term", "AnyFilter", "RangeResult", "merge_range_results", "merge_range_results_device", "ViError", "kmeans_mini_batch", "kmeans_parallel",
           "assign", "l2sq_pairs", "VI_ASSIGN_EXACT", "VI_ASSIGN_REFERENCE", "VI_ORDER_LANES", "VI_ORDER_SCALAR"]


def suggest_nlist(n: int) -> int:
    """lib.rs:308-315 (mirrors src/utils.rs:9-16)."""
    return int(lib().vi_calculate_num_clusters(int(n)))


class Term:
    """One term of VectorIndex.filter_compose: Term.timestamps(lo, hi), .id_range(lo, hi), .ids(ids), .ids_device(ptr, n),
    .mask(a), .mask_device(ptr, n), .filter(f); `~term` is the term negated.  Ids are kept as a flat uint64 array, a mask
    as a flat uint8 array (bool or uint8 in, non-zero admits); a term keeps what it points at alive."""

    __slots__ = ("kind", "negate", "lo", "hi", "data", "ptr", "n", "flt")

    def __init__(self, kind, negate=False, lo=0, hi=0, data=None, ptr=0, n=0, flt=None):
        self.kind, self.negate, self.lo, self.hi = int(kind), bool(negate), int(lo), int(hi)
        self.data, self.ptr, self.n, self.flt = data, int(ptr or 0), int(n), flt

    def __invert__(self):
        return Term(self.kind, not self.negate, self.lo, self.hi, self.data, self.ptr, self.n, self.flt)

    @classmethod
    def timestamps(cls, lo: int, hi: int):
        return cls(_native.VI_TERM_TIMESTAMPS, lo=lo, hi=hi)

    @classmethod
    def id_range(cls, lo: int, hi: int):
        return cls(_native.VI_TERM_ID_RANGE, lo=lo, hi=hi)

    @classmethod
    def ids(cls, ids):
        a = _native.id_array(ids)
        return cls(_native.VI_TERM_IDS, data=a, n=a.size)

    @classmethod
    def ids_device(cls, ids_ptr: int, n: int):
        return cls(_native.VI_TERM_IDS_DEVICE, ptr=ids_ptr, n=n)

    @classmethod
    def mask(cls, mask):
        a = _native.mask_array(mask)
        return cls(_native.VI_TERM_MASK, data=a, n=a.size)

    @classmethod
    def mask_device(cls, mask_ptr: int, n: int):
        return cls(_native.VI_TERM_MASK_DEVICE, ptr=mask_ptr, n=n)

    @classmethod
    def filter(cls, f):
        if not isinstance(f, _Filter):
            raise TypeError("Term.filter takes a filter of the index")
        return cls(_native.VI_TERM_FILTER, flt=f)

    def _native_term(self) -> "_native.FilterTerm":
        t = _native.FilterTerm()
        t.kind, t.negate, t.lo, t.hi, t.n = self.kind, int(self.negate), self.lo, self.hi, self.n
        if self.data is not None:
            t.data = self.data.ctypes.data if self.data.size else None
        elif self.ptr:
            t.data = self.ptr
        if self.flt is not None:
            t.filter = self.flt._h
        return t


def _compose(index, terms, any=False, reuse=None):
    """vi_indexer_filter_compose over Term objects -> the native handle (reuse's own when reuse is given)"""
    terms = list(terms)
    if not all(isinstance(t, Term) for t in terms):
        raise TypeError("filter_compose takes Term objects")
    arr = (_native.FilterTerm * max(len(terms), 1))(*[t._native_term() for t in terms])
    h = C.c_void_p()
    _native.check(lib().vi_indexer_filter_compose(index._h, _native.VI_JOIN_OR if any else _native.VI_JOIN_AND, arr, len(terms),
                                                  reuse._h if reuse is not None else None, C.byref(h)))
    return h


class _Filter:
    """A subset of the resident vectors of one VectorIndex.  Immutable (but for VectorIndex.filter_compose(reuse=));
    pass it as `filter=` to that index's searches.  Keeps its index alive and frees itself.  Of two filters of one index:
    `a & b` the vectors both admit, `a | b` those either admits, `a - b` those a admits and b does not; `~a` the resident
    vectors a does not admit.  Each is a filter of its own, made by one call."""

    def __init__(self, index, handle):
        self._index = index  # (the native filter must be freed before its indexer)
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib().vi_filter_free(h)
            except Exception:
                pass

    @property
    def num_allowed(self) -> int:
        """resident vectors the filter admits"""
        return int(lib().vi_filter_num_allowed(self._h))

    def __and__(self, other):
        if not isinstance(other, _Filter):
            return NotImplemented
        h = C.c_void_p()
        _native.check(lib().vi_filter_intersect(self._index._h, self._h, other._h, C.byref(h)))
        return FilterIntersection(self._index, h, (self, other))

    def __or__(self, other):
        if not isinstance(other, _Filter):
            return NotImplemented
        h = C.c_void_p()
        _native.check(lib().vi_filter_union(self._index._h, self._h, other._h, C.byref(h)))
        return ComposedFilter(self._index, h, (self, other))

    def __sub__(self, other):
        if not isinstance(other, _Filter):
            return NotImplemented
        return ComposedFilter(self._index, _compose(self._index, [Term.filter(self), ~Term.filter(other)]), (self, other))

    def __invert__(self):
        h = C.c_void_p()
        _native.check(lib().vi_filter_complement(self._index._h, self._h, C.byref(h)))
        return ComposedFilter(self._index, h, (self,))


class TimestampFilter(_Filter):
    """The vectors of one VectorIndex whose stored timestamp lies in [ts_min, ts_max] (VectorIndex.filter_timestamps)."""

    def __init__(self, index, handle, ts_min, ts_max):
        super().__init__(index, handle)
        self.ts_min, self.ts_max = int(ts_min), int(ts_max)


class IdFilter(_Filter):
    """The vectors of one VectorIndex whose external id is in a set (exclude=False), or is not in it (exclude=True)
    (VectorIndex.filter_ids, .filter_ids_device).  The set itself is not kept."""

    def __init__(self, index, handle, num_ids, exclude):
        super().__init__(index, handle)
        self.num_ids, self.exclude = int(num_ids), bool(exclude)


class FilterIntersection(_Filter):
    """`a & b`: a filter of its own (the operands may go away); keeps the index of both operands alive."""

    def __init__(self, index, handle, operands):
        super().__init__(index, handle)
        self._indexes = tuple(o._index for o in operands)


class ComposedFilter(_Filter):
    """A union, a complement, a difference, an id range, a mask or a whole expression (VectorIndex.filter_compose): a filter
    of its own (operands, id sets and masks may go away); keeps the index of its operands alive."""

    def __init__(self, index, handle, operands=()):
        super().__init__(index, handle)
        self._indexes = tuple(o._index for o in operands)


AnyFilter = Union[TimestampFilter, IdFilter, FilterIntersection, ComposedFilter]


class RangeResult:
    """A radius search's result left on the device (VectorIndex.range_search_device), CSR like Faiss's RangeSearchResult:
    query q owns entries [lims[q], lims[q + 1]) of D / I / tie.  The four pointers are device addresses of buffers this
    object owns; they stay valid through later searches of the index, until free() (or the object's end).  Keeps its
    index alive.  index None: a merged result (merge_range_results), which belongs to no index — it outlives its parts,
    and the stored vectors of its hits stay on the ranks."""

    def __init__(self, index, handle, nq):
        self._index = index  # (the native result must be freed before its indexer; None: a merged result)
        self._h = handle
        self.nq = int(nq)
        self.total = int(lib().vi_range_result_total(handle))
        p = [C.c_void_p() for _ in range(4)]
        _native.check(lib().vi_range_result_device(handle, *[C.byref(x) for x in p]))
        self.lims_ptr, self.D_ptr, self.I_ptr, self.tie_ptr = [x.value or 0 for x in p]

    def copy(self, include_vectors=False):
        """(lims u64[nq + 1], D f32[total], I i64[total][, V f32[total, dim]]) on the host"""
        if include_vectors and self._index is None:
            raise ViError(_native.VI_ERR_INVALID_INPUT, "a merged result has no stored vectors: they live on the ranks")
        lims = np.zeros(self.nq + 1, dtype=np.uint64)
        D, I = np.zeros(self.total, dtype=np.float32), np.zeros(self.total, dtype=np.int64)
        V = np.zeros((self.total, self._index.dimension), dtype=np.float32) if include_vectors else None
        _native.check(lib().vi_range_result_copy(self._h, _native.ptr(lims), _native.ptr(D), _native.ptr(I), _native.ptr(V)))
        return (lims, D, I, V) if include_vectors else (lims, D, I)

    def copy_device(self, lims_ptr: int = 0, D_ptr: int = 0, I_ptr: int = 0, tie_ptr: int = 0):
        """the same arrays (tie included) copied into device buffers of the caller's on the result's GPU — lims nq + 1,
        the rest `total` entries each; a pointer of 0 skips that array.  Complete on return."""
        _native.check(lib().vi_range_result_copy_device(self._h, *[C.c_void_p(p) if p else None
                                                                   for p in (lims_ptr, D_ptr, I_ptr, tie_ptr)]))

    def free(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib().vi_range_result_free(h)
            except Exception:
                pass
        self.lims_ptr = self.D_ptr = self.I_ptr = self.tie_ptr = 0

    __del__ = free


def merge_range_results_device(device: int, nq: int, lims_ptrs, D_ptrs, I_ptrs, tie_ptrs) -> RangeResult:
    """extension: the radius results of the ranks of a partitioned index, for the same nq queries, merged on `device` into
    the unpartitioned result (vi_range_merge_device).  Part p is CSR in device memory: lims_ptrs[p] -> u64[nq + 1],
    D / I / tie_ptrs[p] -> f32 / i64 / u64 of lims[nq] entries, every row sorted by (distance bits, tie) as
    range_search_device leaves it.  Complete on return; the parts may go afterwards."""
    cols = [list(map(int, c)) for c in (lims_ptrs, D_ptrs, I_ptrs, tie_ptrs)]
    parts = len(cols[0])
    if any(len(c) != parts for c in cols):
        raise ViError(_native.VI_ERR_INVALID_INPUT, "one lims, D, I and tie pointer per part")
    arrays = [(C.c_void_p * max(parts, 1))(*c) for c in cols]
    h = C.c_void_p()
    _native.check(lib().vi_range_merge_device(int(device), int(nq), parts, *arrays, C.byref(h)))
    return RangeResult(None, h, nq)


def merge_range_results(device: int, parts) -> RangeResult:
    """... for RangeResults that live on `device` (in-process ranks)"""
    parts = list(parts)
    if not parts:
        raise ViError(_native.VI_ERR_INVALID_INPUT, "parts must be 1..64")
    if any(p.nq != parts[0].nq for p in parts):
        raise ViError(_native.VI_ERR_INVALID_INPUT, "the parts answer different numbers of queries")
    return merge_range_results_device(device, parts[0].nq, [p.lims_ptr for p in parts], [p.D_ptr for p in parts],
                                      [p.I_ptr for p in parts], [p.tie_ptr for p in parts])


def _filter_handle(f):
    return f._h if f is not None else None


class ProbeRule:
    """extension: adaptive probing — how many of its n_probe probes each query of a search keeps (vi_probe_rule).  The
    probes kept are a prefix of the query's probe row: those whose centroid distance is <= ratio2 * the nearest one's
    (squared distances, f32; 0.0: off), no more than it takes for their lists to hold max_codes vectors (the list that
    crosses the budget included: Faiss's max_codes; 0: off), no more than n_probe_q[q] (None: off), never fewer than
    min_probe.  The result of a query is exactly the search of that query alone with its own probe count.  n_probe_q: an
    integer array-like with one entry per query for the host calls, a device address (int) of nq u32 for the device
    calls.  ProbeRule() prunes nothing."""

    __slots__ = ("min_probe", "ratio2", "max_codes", "n_probe_q")

    def __init__(self, min_probe: int = 1, ratio2: float = 0.0, max_codes: int = 0, n_probe_q=None):
        self.min_probe, self.ratio2, self.max_codes, self.n_probe_q = int(min_probe), float(ratio2), int(max_codes), n_probe_q

    def _native_rule(self, nq: int, device: bool):
        """(vi_probe_rule, what it points at)"""
        r = _native.ProbeRuleC()
        r.min_probe, r.ratio2, r.max_codes = self.min_probe, self.ratio2, self.max_codes
        keep = None
        if self.n_probe_q is not None:
            if device:
                if not isinstance(self.n_probe_q, (int, np.integer)):
                    raise TypeError("a device call takes n_probe_q as a device address")
                r.n_probe_q = int(self.n_probe_q)
            else:
                keep = np.ascontiguousarray(np.asarray(self.n_probe_q).reshape(-1), dtype=np.uint32)
                if keep.size != nq:
                    raise RuntimeError("n_probe_q must have one entry per query")
                r.n_probe_q = keep.ctypes.data if keep.size else None
        return r, keep


class RebalanceRule:
    """extension: the rule of VectorIndex.rebalance (vi_rebalance_rule): `iters` iterations of refine()'s contract, the
    first `split_rounds` of which split overfull lists: a list longer than split_factor * (n / lists) gives one half of
    its records (two-means from its two farthest members, at most split_iters inner iterations) to a list that holds at
    most receiver_max_len records (0: empty lists only), longest donor to shortest receiver, at most max_splits pairs a
    round (0: no cap).  split_rounds == 0: refine(iters) itself."""

    __slots__ = ("iters", "split_rounds", "split_factor", "receiver_max_len", "max_splits", "split_iters")

    def __init__(self, iters: int = 1, split_rounds: int = 1, split_factor: float = 2.0, receiver_max_len: int = 0,
                 max_splits: int = 0, split_iters: int = 4):
        self.iters, self.split_rounds, self.split_factor = int(iters), int(split_rounds), float(split_factor)
        self.receiver_max_len, self.max_splits, self.split_iters = int(receiver_max_len), int(max_splits), int(split_iters)

    def _native_rule(self):
        r = _native.RebalanceRuleC()
        lib().vi_rebalance_rule_init(C.byref(r))
        for f in self.__slots__:
            setattr(r, f, getattr(self, f))
        return r


class VectorIndex:
    """Index handle (PyVectorIndex + the async wrapper of the reference)."""

    def __init__(self, handle, dimension, keep=None):
        self._h = handle
        self._dimension = int(dimension)
        self._keep = keep

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # (module globals are already torn down at interpreter exit)
            try:
                lib().vi_indexer_free(h)
            except Exception:
                pass

    @property
    def dimension(self) -> int:
        return self._dimension

    @property
    def num_centroids(self) -> int:
        return int(lib().vi_indexer_num_centroids(self._h))

    @property
    def num_vectors(self) -> int:
        return int(lib().vi_indexer_num_vectors(self._h))

    @property
    def num_shards(self) -> int:
        return int(lib().vi_indexer_num_shards(self._h))

    def centroids(self):
        k, d = self.num_centroids, self._dimension
        cent = np.zeros((k, d), dtype=np.float32)
        c2s = np.zeros(k, dtype=np.uint64)
        _native.check(lib().vi_indexer_centroids(self._h, _native.ptr(cent), _native.ptr(c2s)))
        return cent, c2s

    # PyVectorIndex.search_blocking (lib.rs:123-203)
    def filter_timestamps(self, ts_min: int, ts_max: int) -> TimestampFilter:
        """extension: the searches of this index restricted to stored timestamps in [ts_min, ts_max], both inclusive"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_timestamps(self._h, int(ts_min), int(ts_max), C.byref(h)))
        return TimestampFilter(self, h, ts_min, ts_max)

    def filter_ids(self, ids, exclude: bool = False) -> IdFilter:
        """extension: the searches of this index restricted to the records whose external id is in `ids` (any integer
        array-like; no order needed, duplicates allowed), or — exclude=True — to the records whose id is NOT in it"""
        a = _native.id_array(ids)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_ids(self._h, _native.ptr(a) if a.size else None, a.size,
                                                  _native.VI_IDS_DENY if exclude else _native.VI_IDS_ALLOW, C.byref(h)))
        return IdFilter(self, h, a.size, exclude)

    def filter_ids_device(self, ids_ptr: int, n: int, exclude: bool = False) -> IdFilter:
        """... for n u64 ids in device memory, read in place"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_ids_device(self._h, C.c_void_p(ids_ptr) if ids_ptr else None, int(n),
                                                         _native.VI_IDS_DENY if exclude else _native.VI_IDS_ALLOW,
                                                         C.byref(h)))
        return IdFilter(self, h, n, exclude)

    def filter_id_range(self, lo: int, hi: int) -> ComposedFilter:
        """extension: the records whose external id lies in [lo, hi], both inclusive (Faiss's IDSelectorRange)"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_id_range(self._h, int(lo), int(hi), C.byref(h)))
        return ComposedFilter(self, h)

    def filter_mask(self, mask) -> ComposedFilter:
        """extension: the records whose entry of `mask` is non-zero: a bool or uint8 array of num_vectors entries in LIST
        ORDER — entry i belongs to the record export() returns as row i, so an attribute kept beside an export filters
        directly.  On a rank of a partitioned index: the rank's own list order (a mask is per rank)."""
        a = _native.mask_array(mask)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_mask(self._h, _native.ptr(a) if a.size else None, a.size, C.byref(h)))
        return ComposedFilter(self, h)

    def filter_mask_device(self, mask_ptr: int, n: int) -> ComposedFilter:
        """... for n mask bytes in device memory, read in place"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_filter_mask_device(self._h, C.c_void_p(mask_ptr) if mask_ptr else None, int(n),
                                                          C.byref(h)))
        return ComposedFilter(self, h)

    def filter_compose(self, terms, any: bool = False, reuse: Optional[AnyFilter] = None) -> AnyFilter:
        """extension: ONE filter from the AND (any=False) or the OR (any=True) of 1 to 8 Term objects, `~term` negated, in
        one launch: Term.timestamps / .id_range / .ids / .ids_device / .mask / .mask_device / .filter (which nests).
        reuse=f: f, a filter of this index that is no operand of the expression, is overwritten in place and returned —
        nothing is allocated for it, and f.num_allowed reflects the new content; no search may be using f meanwhile."""
        terms = list(terms)
        h = _compose(self, terms, any, reuse)
        operands = tuple(t.flt for t in terms if isinstance(t, Term) and t.flt is not None)
        if reuse is not None:
            return reuse   # (its handle is h; the operands are filters of reuse's own index)
        return ComposedFilter(self, h, operands)

    def search_sync(self, xq, k: int, n_probe: int, include_vectors: bool = False, filter: Optional[AnyFilter] = None):
        xq = np.asarray(xq)
        if xq.ndim != 2:
            raise RuntimeError("Query array must be 2-dimensional")
        if xq.shape[1] != self._dimension:  # lib.rs:133-138
            raise RuntimeError(f"Query dimension {xq.shape[1]} doesn't match index dimension {self._dimension}")
        xq = np.ascontiguousarray(xq, dtype=np.float32)
        nq = xq.shape[0]
        k = int(k)
        D = np.full((nq, max(k, 0)), np.inf, dtype=np.float32)
        I = np.full((nq, max(k, 0)), -1, dtype=np.int64)
        V = np.zeros((nq, k, self._dimension), dtype=np.float32) if include_vectors else None
        kout = C.c_uint64(0)
        _native.check(lib().vi_indexer_search_filtered(self._h, _filter_handle(filter), _native.ptr(xq), nq, xq.shape[1], k,
                                                       int(n_probe), _native.ptr(D), _native.ptr(I), _native.ptr(V), None,
                                                       C.byref(kout)))
        if kout.value != k:  # k was clamped to max_k (api.rs:189): results occupy the first kout columns
            kk = kout.value
            D2 = np.full((nq, k), np.inf, dtype=np.float32)
            I2 = np.full((nq, k), -1, dtype=np.int64)
            D2[:, :kk] = D.reshape(-1)[: nq * kk].reshape(nq, kk)
            I2[:, :kk] = I.reshape(-1)[: nq * kk].reshape(nq, kk)
            D, I = D2, I2
        return (D, I, V) if include_vectors else (D, I)

    def range_search_sync(self, xq, radius2: float, n_probe: int, include_vectors: bool = False,
                          filter: Optional[AnyFilter] = None):
        """extension: every probed candidate with squared distance <= radius2, per query in the reference's stable order ->
        (lims u64[nq + 1], D f32[total], I i64[total][, V f32[total, dim]]); query q owns [lims[q], lims[q + 1])"""
        xq = np.asarray(xq)
        if xq.ndim != 2:
            raise RuntimeError("Query array must be 2-dimensional")
        xq = np.ascontiguousarray(xq, dtype=np.float32)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search(self._h, _filter_handle(filter), _native.ptr(xq), xq.shape[0], xq.shape[1],
                                                    float(radius2), int(n_probe), C.byref(h)))
        res = RangeResult(self, h, xq.shape[0])
        try:
            return res.copy(include_vectors)
        finally:
            res.free()

    def range_search_device(self, xq_ptr: int, nq: int, radius2: float, n_probe: int,
                            filter: Optional[AnyFilter] = None) -> RangeResult:
        """... for nq queries in device memory; the result stays there (RangeResult)"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search_device(self._h, _filter_handle(filter), C.c_void_p(xq_ptr), int(nq),
                                                           float(radius2), int(n_probe), C.byref(h)))
        return RangeResult(self, h, nq)

    async def search(self, xq, k: int, n_probe: int) -> Tuple[np.ndarray, np.ndarray]:
        loop = asyncio.get_event_loop()
        return await loop.run_in_executor(None, self.search_sync, xq, k, n_probe)

    def enable_timing(self, on=True):
        """True / 1: HIP events at every phase boundary; 2: around the list-rank kernel only (ms_scan); False / 0: none"""
        lib().vi_indexer_enable_timing(self._h, 2 if on == 2 and on is not True else (1 if on else 0))

    def last_stats(self) -> dict:
        st = _native.SearchStats()
        _native.check(lib().vi_indexer_last_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def last_stat(self, field: str):
        """one field of last_stats() without building the dict (a timed loop reads ms_scan after every step)"""
        st = self.__dict__.get("_stat_buf")
        if st is None:
            st = self.__dict__["_stat_buf"] = _native.SearchStats()
        _native.check(lib().vi_indexer_last_stats(self._h, C.byref(st)))
        return getattr(st, field)

    def add(self, xb, ext_ids=None, timestamps=None) -> None:
        """extension: append the rows of xb to the index, each to the list of its nearest centroid (nothing is retrained),
        in the shard files and on the GPU.  ext_ids None: num_vectors + i; timestamps None or 0: now.  Unpartitioned
        indexes only.  Filters made before the call are rejected afterwards; RangeResults must be copied or freed before it;
        the call must not overlap searches of this index."""
        xb = np.asarray(xb)
        if xb.ndim != 2:
            raise RuntimeError("Array must be 2-dimensional")
        if xb.shape[1] != self._dimension:
            raise RuntimeError(f"Vector dimension {xb.shape[1]} doesn't match index dimension {self._dimension}")
        xb = np.ascontiguousarray(xb, dtype=np.float32)
        n = xb.shape[0]
        e = None if ext_ids is None else _native.id_array(ext_ids)
        t = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64).reshape(-1)
        if (e is not None and e.size != n) or (t is not None and t.size != n):
            raise RuntimeError("ext_ids and timestamps must have one entry per row")
        _native.check(lib().vi_indexer_add_records(self._h, _native.ptr(e), _native.ptr(xb), _native.ptr(t), n),
                      prefix="Failed to add records: ")

    def add_stats(self) -> dict:
        """phases of the most recent add() that added something"""
        st = _native.AddStats()
        _native.check(lib().vi_indexer_last_add_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def retain(self, filter: AnyFilter) -> int:
        """extension: keep exactly the records `filter` (a filter of this index) admits, in the shard files and on the
        GPU; the kept records of every list close up in their old order, nothing is retrained -> records removed.
        Unpartitioned indexes only; at least one record must stay.  Unless nothing was removed, filters made before the
        call — `filter` included — are rejected afterwards; RangeResults must be copied or freed before it; the call must
        not overlap searches of this index."""
        if filter is None:
            raise ViError(_native.VI_ERR_INVALID_INPUT, "null filter")
        removed = C.c_uint64(0)
        _native.check(lib().vi_indexer_retain(self._h, filter._h, C.byref(removed)), prefix="Failed to remove records: ")
        return int(removed.value)

    def remove_ids(self, ids) -> int:
        """extension: remove every record whose external id is in `ids` (any integer array-like; no order needed,
        duplicates allowed, unknown ids ignored) -> records removed.  The limits of retain() apply."""
        a = _native.id_array(ids)
        removed = C.c_uint64(0)
        _native.check(lib().vi_indexer_remove_ids(self._h, _native.ptr(a) if a.size else None, a.size, C.byref(removed)),
                      prefix="Failed to remove records: ")
        return int(removed.value)

    def remove_stats(self) -> dict:
        """phases of the most recent retain() / remove_ids() that removed something"""
        st = _native.RemoveStats()
        _native.check(lib().vi_indexer_last_remove_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def upsert(self, xb, ext_ids, timestamps=None) -> int:
        """extension: "these ids have new vectors": every stored record whose external id is in ext_ids goes (the rules
        of remove_ids()), then row i of xb joins the list of its nearest centroid with id ext_ids[i] (the rules of add())
        -> records replaced.  The index afterwards is the one remove_ids(ext_ids) followed by add(xb, ext_ids, timestamps)
        leaves, from one rewrite of every touched shard file and one rebuild of the resident index; unlike that pair, a
        call may replace every record.  Ids nothing carries are simply added; an id named twice is added twice.
        Unpartitioned indexes only.  Filters made before the call are rejected afterwards; RangeResults must be copied or
        freed before it; the call must not overlap searches of this index."""
        xb = np.asarray(xb)
        if xb.ndim != 2:
            raise RuntimeError("Array must be 2-dimensional")
        if xb.shape[1] != self._dimension:
            raise RuntimeError(f"Vector dimension {xb.shape[1]} doesn't match index dimension {self._dimension}")
        xb = np.ascontiguousarray(xb, dtype=np.float32)
        n = xb.shape[0]
        e = _native.id_array(ext_ids)
        t = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64).reshape(-1)
        if e.size != n or (t is not None and t.size != n):
            raise RuntimeError("ext_ids and timestamps must have one entry per row")
        replaced = C.c_uint64(0)
        _native.check(lib().vi_indexer_upsert_records(self._h, _native.ptr(e) if n else None, _native.ptr(xb), _native.ptr(t), n,
                                                      C.byref(replaced)), prefix="Failed to upsert records: ")
        return int(replaced.value)

    def upsert_stats(self) -> dict:
        """phases of the most recent upsert() of at least one row"""
        st = _native.UpsertStats()
        _native.check(lib().vi_indexer_last_upsert_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def refine(self, iters: int = 1) -> int:
        """extension: `iters` Lloyd iterations warm-started from the table the index has, on the GPU: every list with a
        record gets the mean of its records as its centroid (an empty list keeps its own), every record goes to the list
        of its now-nearest centroid (the rule of add()), in its previous order -> records whose list changed.  Stops early
        at a fixed point.  index.bin and every shard file with a list are rewritten once (internal ids become the new list
        order, 0..n-1), the resident index is swapped once; iters == 0 changes nothing.  Unpartitioned indexes only.
        Filters made before a call that ran an iteration are rejected afterwards; RangeResults must be copied or freed
        before it; the call must not overlap searches of this index."""
        moved = C.c_uint64(0)
        _native.check(lib().vi_indexer_refine(self._h, int(iters), C.byref(moved)), prefix="Failed to refine the index: ")
        return int(moved.value)

    def refine_stats(self) -> dict:
        """counts and phases of the most recent refine() with iters > 0"""
        st = _native.RefineStats()
        _native.check(lib().vi_indexer_last_refine_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def rebalance(self, rule: Optional[RebalanceRule] = None, **fields) -> int:
        """extension: refine() with a split step in its first iterations (RebalanceRule; `fields` are its fields, given
        instead of a rule): an overfull list gives one half of its records to an empty one, which a warm-started refine
        never does -> records whose list changed.  The number of lists, the list ids and the shard of every list stay.
        Files, resident index, filters and overlap with searches: as refine()."""
        if rule is None:
            rule = RebalanceRule(**fields)
        elif fields:
            raise TypeError("give a rule or its fields, not both")
        if not isinstance(rule, RebalanceRule):
            raise TypeError("rule must be a RebalanceRule")
        moved = C.c_uint64(0)
        r = rule._native_rule()
        _native.check(lib().vi_indexer_rebalance(self._h, C.byref(r), C.byref(moved)), prefix="Failed to rebalance the index: ")
        return int(moved.value)

    def rebalance_stats(self) -> dict:
        """counts and phases of the most recent rebalance(): the fields of refine_stats(), then pairs_planned, splits_done,
        splits_skipped, inner_iterations, split_bytes, ms_split and ms_split_kernels"""
        st = _native.RebalanceStats()
        _native.check(lib().vi_indexer_last_rebalance_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def list_stats(self) -> dict:
        """the balance of the resident lists: lists, empty_lists, min_len, max_len, mean_len and Faiss's imbalance factor
        (1 = equal lengths); on a rank of a partitioned index, of the rank's part"""
        st = _native.ListStats()
        _native.check(lib().vi_indexer_list_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def get(self, ids, *, vectors: bool = True):
        """extension: read records back by external id (any integer array-like; no order needed, ids may repeat) ->
        (counts u32[n], X f32[n, dim] or None, timestamps u64[n], where u64[n]).  counts[i]: resident records that carry
        ids[i] (0: absent — a zero row, timestamp 0, where 2^64 - 1); the rest describes the first of them in list order:
        the stored f32 bits, the stored timestamp, where = (list << 32) | position in the full list.  vectors=False:
        nothing is gathered ("contains / how many").  May run beside searches, not beside an update."""
        a = _native.id_array(ids)
        n = a.size
        counts, ts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        where = np.full(n, _native.WHERE_NONE, dtype=np.uint64)
        X = np.zeros((n, self._dimension), dtype=np.float32) if vectors else None
        _native.check(lib().vi_indexer_get_records(self._h, _native.ptr(a) if n else None, n, _native.ptr(counts), _native.ptr(X),
                                                   _native.ptr(ts), _native.ptr(where)), prefix="Failed to get records: ")
        return counts, X, ts, where

    def get_device(self, ids_ptr: int, n: int, count_ptr: int = 0, values_ptr: int = 0, ts_ptr: int = 0, where_ptr: int = 0):
        """... for n u64 ids in device memory, into device memory: counts u32[n], values f32[n, dim], timestamps and where
        u64[n]; a pointer of 0 skips that output"""
        _native.check(lib().vi_indexer_get_records_device(self._h, C.c_void_p(ids_ptr) if ids_ptr else None, int(n),
                                                          *[C.c_void_p(p) if p else None
                                                            for p in (count_ptr, values_ptr, ts_ptr, where_ptr)]),
                      prefix="Failed to get records: ")

    def export(self, first: int = 0, count: Optional[int] = None):
        """extension: records [first, first + count) of the list order (lists ascending, positions ascending; count None:
        to the end) -> (ext_ids u64[count], X f32[count, dim], timestamps u64[count], where u64[count]).  On a rank of a
        partitioned index: the rank's resident records, where carrying full-list positions."""
        first = int(first)
        count = max(self.num_vectors - first, 0) if count is None else int(count)
        ext, ts, where = (np.zeros(count, dtype=np.uint64) for _ in range(3))
        X = np.zeros((count, self._dimension), dtype=np.float32)
        _native.check(lib().vi_indexer_export_records(self._h, first, count, _native.ptr(ext), _native.ptr(X), _native.ptr(ts),
                                                      _native.ptr(where)), prefix="Failed to export records: ")
        return ext, X, ts, where

    def export_device(self, first: int, count: int, ids_ptr: int = 0, values_ptr: int = 0, ts_ptr: int = 0, where_ptr: int = 0):
        """... into device memory: ext_ids u64[count], values f32[count, dim] row-major, timestamps and where u64[count];
        a pointer of 0 skips that output"""
        _native.check(lib().vi_indexer_export_records_device(self._h, int(first), int(count),
                                                             *[C.c_void_p(p) if p else None
                                                               for p in (ids_ptr, values_ptr, ts_ptr, where_ptr)]),
                      prefix="Failed to export records: ")

    def search_by_ids(self, ids, k: int, n_probe: int, exclude_self: bool = True, include_vectors: bool = False,
                      filter: Optional[AnyFilter] = None):
        """extension: "what is similar to the record I hold?" -> (D f32[n, k'], I i64[n, k'][, V f32[n, k', dim]], found
        u32[n]), k' = k clamped to max_k.  Row i is the top-k of the stored vector of the first record in list order that
        carries ids[i] (the record get() describes), that ONE record deleted from its candidates if exclude_self — records
        with the same id or the same bits stay.  found[i]: resident records carrying ids[i]; 0: an absent id, a row of
        padding (inf / -1 / zero vectors), no error.  Ids may repeat.  An excluding call searches k + 1 wide: k = 64 and
        k = 128 are served by a slower engine (same bits).  Unpartitioned handles only."""
        a = _native.id_array(ids)
        n, k = a.size, int(k)
        D = np.full((n, max(k, 0)), np.inf, dtype=np.float32)
        I = np.full((n, max(k, 0)), -1, dtype=np.int64)
        V = np.zeros((n, max(k, 0), self._dimension), dtype=np.float32) if include_vectors else None
        found = np.zeros(n, dtype=np.uint32)
        kout = C.c_uint64(k)
        _native.check(lib().vi_indexer_search_by_ids(self._h, _filter_handle(filter), _native.ptr(a) if n else None, n, k,
                                                     int(n_probe), 1 if exclude_self else 0, _native.ptr(D), _native.ptr(I),
                                                     _native.ptr(V), None, _native.ptr(found), C.byref(kout)),
                      prefix="Failed to search by ids: ")
        kk = int(kout.value)
        if kk != k:  # k was clamped to max_k: the rows are kk wide
            D = D.reshape(-1)[: n * kk].reshape(n, kk).copy()
            I = I.reshape(-1)[: n * kk].reshape(n, kk).copy()
            if V is not None:
                V = V.reshape(-1)[: n * kk * self._dimension].reshape(n, kk, self._dimension).copy()
        return (D, I, V, found) if include_vectors else (D, I, found)

    def search_by_ids_device(self, ids_ptr: int, nq: int, k: int, n_probe: int, D_ptr: int, I_ptr: int, tie_ptr: int = 0,
                             found_ptr: int = 0, exclude_self: bool = True, filter: Optional[AnyFilter] = None):
        """... for nq u64 ids in device memory, into device memory: D f32 / I i64 / tie u64 [nq, k'], found u32[nq]; a
        pointer of 0 skips tie / found"""
        _native.check(lib().vi_indexer_search_by_ids_device(self._h, _filter_handle(filter), C.c_void_p(ids_ptr) if ids_ptr else None,
                                                            int(nq), int(k), int(n_probe), 1 if exclude_self else 0,
                                                            C.c_void_p(D_ptr) if D_ptr else None, C.c_void_p(I_ptr) if I_ptr else None,
                                                            C.c_void_p(tie_ptr) if tie_ptr else None,
                                                            C.c_void_p(found_ptr) if found_ptr else None),
                      prefix="Failed to search by ids: ")

    def knn_graph(self, k: int, n_probe: int, first: int = 0, count: Optional[int] = None, exclude_self: bool = True,
                  filter: Optional[AnyFilter] = None):
        """extension: the k-NN graph of records [first, first + count) of the list order (count None: to the end) -> (D
        f32[count, k'], I i64[count, k']); row j belongs to the record export() returns as row j, and is what
        search_by_ids gives for it.  Processed in chunks of VI_GRAPH_CHUNK rows (environment; default 65536)."""
        first, k = int(first), int(k)
        count = max(self.num_vectors - first, 0) if count is None else int(count)
        D = np.full((count, max(k, 0)), np.inf, dtype=np.float32)
        I = np.full((count, max(k, 0)), -1, dtype=np.int64)
        kout = C.c_uint64(k)
        _native.check(lib().vi_indexer_knn_graph(self._h, _filter_handle(filter), first, count, k, int(n_probe),
                                                 1 if exclude_self else 0, _native.ptr(D), _native.ptr(I), None, C.byref(kout)),
                      prefix="Failed to build the k-NN graph: ")
        kk = int(kout.value)
        if kk != k:
            D = D.reshape(-1)[: count * kk].reshape(count, kk).copy()
            I = I.reshape(-1)[: count * kk].reshape(count, kk).copy()
        return D, I

    def knn_graph_device(self, first: int, count: int, k: int, n_probe: int, D_ptr: int, I_ptr: int, tie_ptr: int = 0,
                         exclude_self: bool = True, filter: Optional[AnyFilter] = None):
        """... into device memory: D f32 / I i64 / tie u64 [count, k']; a tie pointer of 0 skips it"""
        _native.check(lib().vi_indexer_knn_graph_device(self._h, _filter_handle(filter), int(first), int(count), int(k),
                                                        int(n_probe), 1 if exclude_self else 0,
                                                        C.c_void_p(D_ptr) if D_ptr else None, C.c_void_p(I_ptr) if I_ptr else None,
                                                        C.c_void_p(tie_ptr) if tie_ptr else None),
                      prefix="Failed to build the k-NN graph: ")

    def range_search_by_ids(self, ids, radius2: float, n_probe: int, exclude_self: bool = True, include_vectors: bool = False,
                            filter: Optional[AnyFilter] = None):
        """extension: "which records are within radius2 of the record I hold?" -> (lims u64[n + 1], D f32[total], I
        i64[total][, V f32[total, dim]], found u32[n]); row i owns [lims[i], lims[i + 1]) and is the radius search of the
        stored vector of the first record in list order that carries ids[i], that ONE record deleted if exclude_self —
        records with the same id or the same bits stay.  found[i]: resident records carrying ids[i]; 0: an absent id, an
        empty row, no error.  Ids may repeat.  Unpartitioned handles only."""
        a = _native.id_array(ids)
        n = a.size
        found = np.zeros(n, dtype=np.uint32)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search_by_ids(self._h, _filter_handle(filter), _native.ptr(a) if n else None, n,
                                                           float(radius2), int(n_probe), 1 if exclude_self else 0,
                                                           _native.ptr(found), C.byref(h)),
                      prefix="Failed to range-search by ids: ")
        res = RangeResult(self, h, n)
        try:
            return (*res.copy(include_vectors), found)
        finally:
            res.free()

    def range_search_by_ids_device(self, ids_ptr: int, nq: int, radius2: float, n_probe: int, exclude_self: bool = True,
                                   found_ptr: int = 0, filter: Optional[AnyFilter] = None) -> RangeResult:
        """... for nq u64 ids in device memory; the result stays there (RangeResult), found u32[nq] is written to
        found_ptr (0 skips it)"""
        h = C.c_void_p()
        _native.check(lib().vi_indexer_range_search_by_ids_device(self._h, _filter_handle(filter),
                                                                  C.c_void_p(ids_ptr) if ids_ptr else None, int(nq), float(radius2),
                                                                  int(n_probe), 1 if exclude_self else 0,
                                                                  C.c_void_p(found_ptr) if found_ptr else None, C.byref(h)),
                      prefix="Failed to range-search by ids: ")
        return RangeResult(self, h, nq)

    def radius_graph(self, radius2: float, n_probe: int, first: int = 0, count: Optional[int] = None, exclude_self: bool = True,
                     filter: Optional[AnyFilter] = None) -> RangeResult:
        """extension: the radius graph of records [first, first + count) of the list order (count None: to the end), left on
        the device (RangeResult); row j belongs to the record export() returns as row j, and is what range_search_by_ids
        gives for it.  Processed in chunks of VI_GRAPH_CHUNK rows (environment; default 65536)."""
        first = int(first)
        count = max(self.num_vectors - first, 0) if count is None else int(count)
        h = C.c_void_p()
        _native.check(lib().vi_indexer_radius_graph(self._h, _filter_handle(filter), first, count, float(radius2), int(n_probe),
                                                    1 if exclude_self else 0, C.byref(h)),
                      prefix="Failed to build the radius graph: ")
        return RangeResult(self, h, count)

    def cluster_radius(self, radius2: float, n_probe: int, min_pts: int = 1, filter: Optional[AnyFilter] = None,
                       with_degree: bool = False):
        """extension: cluster the stored records by radius -> labels i64[n] (or (labels, degree u32[n])) in LIST ORDER:
        entry j belongs to the record export() returns as row j.  min_pts <= 1: the connected components of the radius
        graph (radius2 = 0: the groups of exact copies); min_pts >= 2: DBSCAN over it.  A label is the list-order ordinal
        of its cluster's first record, so `labels == np.arange(n)` marks one representative per cluster — a filter_mask
        whose retain() removes every duplicate but one; -1: noise, or a record the filter does not admit.  degree: other
        records within the radius.  The graph is consumed on the device chunk by chunk and never held whole.
        cluster_stats()["n_clusters"] has the number of clusters.  Unpartitioned handles only."""
        n = self.num_vectors
        labels = np.full(n, -1, dtype=np.int64)
        degree = np.zeros(n, dtype=np.uint32) if with_degree else None
        nc = C.c_uint64(0)
        _native.check(lib().vi_indexer_cluster_radius(self._h, _filter_handle(filter), float(radius2), int(n_probe), int(min_pts),
                                                      _native.ptr(labels), _native.ptr(degree), C.byref(nc)),
                      prefix="Failed to cluster by radius: ")
        return (labels, degree) if with_degree else labels

    def cluster_radius_device(self, labels_ptr: int, degree_ptr: int = 0, radius2: float = 0.0, n_probe: int = 1, min_pts: int = 1,
                              filter: Optional[AnyFilter] = None) -> int:
        """... into device memory: labels i64[num_vectors] / degree u32[num_vectors]; a pointer of 0 skips that output.
        Returns the number of clusters."""
        nc = C.c_uint64(0)
        _native.check(lib().vi_indexer_cluster_radius_device(self._h, _filter_handle(filter), float(radius2), int(n_probe),
                                                             int(min_pts), C.c_void_p(labels_ptr) if labels_ptr else None,
                                                             C.c_void_p(degree_ptr) if degree_ptr else None, C.byref(nc)),
                      prefix="Failed to cluster by radius: ")
        return int(nc.value)

    def cluster_stats(self) -> dict:
        """this thread's last cluster_radius (either form): rows, hits (the sum of the degrees), passes over the graph,
        n_core / n_border / n_noise / n_clusters, chunk_rows, link_bytes; the ms_* only under VI_SIMILAR_TIMING"""
        st = _native.ClusterStats()
        _native.check(lib().vi_cluster_last_stats(C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def similar_times(self) -> dict:
        """this thread's last search_by_ids / knn_graph / range_search_by_ids / radius_graph (any form) under
        VI_SIMILAR_TIMING: host ms around the gather of the queries and the search, HIP-event ms and bytes of the drop
        kernels (self_drop_kernel; range_find_kernel + range_move_kernel), rows per chunk; zeros otherwise"""
        r, s, d = C.c_float(0), C.c_float(0), C.c_float(0)
        b, c = C.c_uint64(0), C.c_uint64(0)
        _native.check(lib().vi_similar_last_times(C.byref(r), C.byref(s), C.byref(d), C.byref(b), C.byref(c)))
        return {"ms_resolve": r.value, "ms_search": s.value, "ms_drop": d.value, "drop_bytes": int(b.value), "chunk_rows": int(c.value)}

    def fetch_stats(self) -> dict:
        """figures of the most recent get() / export() (either form); the ms_* only under enable_timing()"""
        st = _native.FetchStats()
        _native.check(lib().vi_indexer_last_fetch_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def build_stats(self) -> dict:
        st = _native.BuildStats()
        _native.check(lib().vi_indexer_last_build_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    # device-pointer search used by the multi-GPU path (torch tensors on this GPU)
    def search_device(self, xq_ptr: int, nq: int, k: int, n_probe: int, D_ptr: int, I_ptr: int, tie_ptr: int = 0,
                      filter: Optional[AnyFilter] = None):
        _native.check(lib().vi_indexer_search_filtered_device(self._h, _filter_handle(filter), C.c_void_p(xq_ptr), nq, k,
                                                              n_probe, C.c_void_p(D_ptr), C.c_void_p(I_ptr),
                                                              C.c_void_p(tie_ptr) if tie_ptr else None))


    def probe_device(self, xq_ptr: int, nq: int, n_probe: int, probes_ptr: int, order_ptr: int) -> int:
        """coarse step only (ivf_index.rs:205-220) -> n_probe_eff; probes / order are u32[nq][n_probe_eff] on the device"""
        p_eff = C.c_uint64(0)
        _native.check(lib().vi_indexer_probe_device(self._h, C.c_void_p(xq_ptr), nq, n_probe, C.c_void_p(probes_ptr),
                                                    C.c_void_p(order_ptr), C.byref(p_eff)))
        return int(p_eff.value)

    def search_probed_device(self, xq_ptr: int, nq: int, k: int, n_probe_eff: int, probes_ptr: int, order_ptr: int,
                             D_ptr: int, I_ptr: int, tie_ptr: int = 0, filter: Optional[AnyFilter] = None):
        """list scan + top-k (ivf_index.rs:223-274) with probe lists computed elsewhere"""
        _native.check(lib().vi_indexer_search_probed_filtered_device(self._h, _filter_handle(filter), C.c_void_p(xq_ptr), nq,
                                                                     k, n_probe_eff, C.c_void_p(probes_ptr),
                                                                     C.c_void_p(order_ptr), C.c_void_p(D_ptr),
                                                                     C.c_void_p(I_ptr),
                                                                     C.c_void_p(tie_ptr) if tie_ptr else None))


    # ---- adaptive probing (vi_probe_rule) ----
    def search_adaptive_sync(self, xq, k: int, n_probe: int, rule: ProbeRule, filter: Optional[AnyFilter] = None,
                             include_vectors: bool = False, return_probed: bool = False):
        """extension: search_sync with n_probe as the upper bound and `rule` deciding each query's own probe count ->
        (D, I[, V][, n_probed u32[nq]]).  One coarse step, the prune and the list phase, all on the device; the rows of a
        query are what search_sync gives for it alone at n_probe = n_probed[q].  ProbeRule(): search_sync itself."""
        if not isinstance(rule, ProbeRule):
            raise TypeError("rule must be a ProbeRule")
        xq = np.asarray(xq)
        if xq.ndim != 2:
            raise RuntimeError("Query array must be 2-dimensional")
        if xq.shape[1] != self._dimension:
            raise RuntimeError(f"Query dimension {xq.shape[1]} doesn't match index dimension {self._dimension}")
        xq = np.ascontiguousarray(xq, dtype=np.float32)
        nq, k = xq.shape[0], int(k)
        D = np.full((nq, max(k, 0)), np.inf, dtype=np.float32)
        I = np.full((nq, max(k, 0)), -1, dtype=np.int64)
        V = np.zeros((nq, max(k, 0), self._dimension), dtype=np.float32) if include_vectors else None
        probed = np.zeros(nq, dtype=np.uint32)
        r, keep = rule._native_rule(nq, device=False)
        kout = C.c_uint64(k)
        _native.check(lib().vi_indexer_search_adaptive(self._h, _filter_handle(filter), C.byref(r), _native.ptr(xq), nq, xq.shape[1],
                                                       k, int(n_probe), _native.ptr(D), _native.ptr(I), _native.ptr(V), None,
                                                       _native.ptr(probed), C.byref(kout)))
        del keep
        kk = int(kout.value)
        if kk != k:  # k was clamped to max_k: results occupy the first kk columns
            D2 = np.full((nq, k), np.inf, dtype=np.float32)
            I2 = np.full((nq, k), -1, dtype=np.int64)
            D2[:, :kk] = D.reshape(-1)[: nq * kk].reshape(nq, kk)
            I2[:, :kk] = I.reshape(-1)[: nq * kk].reshape(nq, kk)
            D, I = D2, I2
            if V is not None:
                V2 = np.zeros((nq, k, self._dimension), dtype=np.float32)
                V2[:, :kk] = V.reshape(-1)[: nq * kk * self._dimension].reshape(nq, kk, self._dimension)
                V = V2
        return (D, I) + ((V,) if include_vectors else ()) + ((probed,) if return_probed else ())

    def search_adaptive_device(self, xq_ptr: int, nq: int, k: int, n_probe: int, rule: ProbeRule, D_ptr: int, I_ptr: int,
                               tie_ptr: int = 0, n_probed_ptr: int = 0, filter: Optional[AnyFilter] = None):
        """... for nq queries in device memory, into device memory as search_device; n_probed u32[nq] is written to
        n_probed_ptr (0 skips it); rule.n_probe_q is a device address"""
        r, _ = rule._native_rule(nq, device=True)
        _native.check(lib().vi_indexer_search_adaptive_device(self._h, _filter_handle(filter), C.byref(r), C.c_void_p(xq_ptr),
                                                              int(nq), int(k), int(n_probe), C.c_void_p(D_ptr), C.c_void_p(I_ptr),
                                                              C.c_void_p(tie_ptr) if tie_ptr else None,
                                                              C.c_void_p(n_probed_ptr) if n_probed_ptr else None))

    def prune_probes_device(self, xq_ptr: int, nq: int, n_probe_eff: int, probes_ptr: int, order_ptr: int, rule: ProbeRule,
                            n_kept_ptr: int = 0):
        """the prune alone, in place on the rows probe_device left (of the same nq queries), before search_probed_device:
        the multi-GPU seam.  Probes past a query's count and their orders become 0xFFFFFFFF, the kept orders close up."""
        r, _ = rule._native_rule(nq, device=True)
        _native.check(lib().vi_indexer_prune_probes_device(self._h, C.c_void_p(xq_ptr), int(nq), int(n_probe_eff),
                                                           C.c_void_p(probes_ptr), C.c_void_p(order_ptr), C.byref(r),
                                                           C.c_void_p(n_kept_ptr) if n_kept_ptr else None))

    def prune_stats(self) -> dict:
        """this thread's last search_adaptive_* / prune_probes_device: real probes in, probes kept, and under
        VI_PRUNE_TIMING the HIP-event ms of the prune kernel (0.0 otherwise)"""
        a, b, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
        _native.check(lib().vi_prune_last_stats(C.byref(a), C.byref(b), C.byref(ms)))
        return {"probes_in": int(a.value), "probes_kept": int(b.value), "ms_prune": float(ms.value)}


def _config(dimension, index_dir, shards_dir, **ext):
    cfg = _native.Config()
    lib().vi_config_init(C.byref(cfg), int(dimension))
    keep = (index_dir.encode(), shards_dir.encode())
    cfg.index_dir, cfg.shards_dir = keep
    for key, val in ext.items():
        if val is not None:
            setattr(cfg, key, val)
    return cfg, keep


def build(xb, work_dir: Optional[str] = None, *, nlist: int = 0, seed: int = 0, assign_mode: int = 0,
          device: int = 0, rank: int = 0, world_size: int = 0, now_secs: int = 0, ext_ids=None,
          timestamps=None) -> VectorIndex:
    """build(xb, work_dir=None) — lib.rs:220-280.  Keyword arguments are extensions."""
    xb = np.asarray(xb)
    if xb.ndim != 2:
        raise RuntimeError("Array must be 2-dimensional")
    n, d = xb.shape
    if n == 0:
        raise RuntimeError("Cannot build index from empty array")  # lib.rs:225-227
    xb = np.ascontiguousarray(xb, dtype=np.float32)
    work = work_dir if work_dir is not None else os.path.join(tempfile.gettempdir(), "vector_indexer_bench")
    index_dir, shards_dir = os.path.join(work, "index"), os.path.join(work, "shards")
    os.makedirs(index_dir, exist_ok=True)
    os.makedirs(shards_dir, exist_ok=True)
    cfg, keep = _config(d, index_dir, shards_dir, nlist_override=nlist, seed=seed, assign_mode=assign_mode,
                        device=device, rank=rank, world_size=world_size, now_secs=now_secs)
    h = C.c_void_p()
    _native.check(lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    e = None if ext_ids is None else np.ascontiguousarray(ext_ids, dtype=np.uint64)
    t = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64)
    try:
        _native.check(lib().vi_indexer_build_from_records(h, _native.ptr(e), _native.ptr(xb), _native.ptr(t), None, n),
                      prefix="Failed to build index: ")
    except Exception:
        lib().vi_indexer_free(h)
        raise
    return VectorIndex(h, d, keep)


def load(index_dir: str, shards_dir: str, dimension: int, *, device: int = 0, rank: int = 0,
         world_size: int = 0, placement: int = 0, now_secs: int = 0) -> VectorIndex:
    """load(index_dir, shards_dir, dimension) — lib.rs:291-304.  now_secs: the timestamp add() gives records without one
    (0: wall clock)."""
    cfg, keep = _config(dimension, index_dir, shards_dir, device=device, rank=rank, world_size=world_size,
                        placement=placement, now_secs=now_secs)
    h = C.c_void_p()
    _native.check(lib().vi_indexer_load(C.byref(cfg), C.byref(h)), prefix="Failed to load index: ")
    return VectorIndex(h, dimension, keep)


# ---- k-means seams (src/kmeans.rs public functions) --------------------------------------------
def _kmeans(fn, X, k, max_iters, thr, seed, mode):
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2:
        X = X.reshape(0, 0)
    X = np.ascontiguousarray(X)
    n, d = X.shape
    cent = np.zeros((int(k), d), dtype=np.float32)
    labels = np.zeros(n, dtype=np.uint64)
    iters = C.c_uint64(0)
    _native.check(fn(_native.ptr(X), n, d, int(k), int(max_iters), -1.0 if thr is None else float(thr), int(seed),
                     int(mode), _native.ptr(cent), _native.ptr(labels), C.byref(iters)))
    return cent, labels, iters.value


def kmeans_mini_batch(X, k, max_iters, early_stop_threshold=None, seed=42, mode=VI_ASSIGN_REFERENCE):
    """run_kmeans_mini_batch — src/kmeans.rs:64-70 -> (centroids, labels, iterations_run)"""
    return _kmeans(lib().vi_kmeans_mini_batch, X, k, max_iters, early_stop_threshold, seed, mode)


def kmeans_parallel(X, k, max_iters, early_stop_threshold=None, seed=42, mode=VI_ASSIGN_REFERENCE):
    """run_kmeans_parallel — src/kmeans.rs:15-21"""
    return _kmeans(lib().vi_kmeans_parallel, X, k, max_iters, early_stop_threshold, seed, mode)


def assign(X, centroids, seed=42, mode=VI_ASSIGN_REFERENCE, return_dist=False):
    """assign_points_simd_parallel — src/kmeans.rs:445-459"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    cent = np.ascontiguousarray(centroids, dtype=np.float32)
    n, d = X.shape
    labels = np.zeros(n, dtype=np.uint64)
    dist = np.zeros(n, dtype=np.float32) if return_dist else None
    _native.check(lib().vi_assign(_native.ptr(X), n, d, _native.ptr(cent), cent.shape[0], int(seed), int(mode),
                                  _native.ptr(labels), _native.ptr(dist)))
    return (labels, dist) if return_dist else labels


def l2sq_pairs(a, b, order=VI_ORDER_SCALAR):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    n, d = a.shape
    out = np.zeros(n, dtype=np.float32)
    _native.check(lib().vi_l2sq_pairs(_native.ptr(a), _native.ptr(b), n, d, int(order), _native.ptr(out)))
    return out
