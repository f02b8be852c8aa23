"""Multi-GPU search: one process per GPU, every inverted list striped over the ranks, ONE all-gather.

Rank r keeps block b (64 vectors) of every list iff b % world == r (vi_config.rank/world_size); the
coarse table is replicated so every rank derives the same probe list and the same candidate-order
keys.  Per query each rank returns its local top-k (D, I, tie); the three arrays are exchanged with
torch.distributed.all_gather (backend "nccl" == RCCL over xGMI on the GPU box, "gloo" in the CPU
protocol tests) and merged on (dist, tie), which reproduces the single-GPU stable order exactly.

A radius search returns ragged rows, so its exchange is two all-gathers: every rank's lims (nq + 1 u64: fixed size, and
they tell every rank every total), then one byte buffer per rank padded to the largest total (range_part_layout).  The
merge by the same key runs on the device, parallel over entries (vi_range_merge_device).  A filter belongs to one handle:
every rank makes its own from the same predicate and passes it as `filter=`.  A mask (VectorIndex.filter_mask, Term.mask)
is per rank: its bytes follow the rank's own list order, so every rank builds it from its own export().

The reference has no distributed mode (its "two-level sharding" only groups files,
src/ivf_index.rs:104-164); this is the MI355X-native extension BASELINE.json's north_star asks for.
"""
import numpy as np


def block_owner(block: int, world: int) -> int:
    """placement rule shared by vi_indexer_load (csrc/device_index.hip, csrc/list_layout.hpp) and the oracle's protocol checker: block b
    (vectors 64b .. 64b+63) of EVERY list lives on rank b % world.  Stripes, not whole lists or shard files: the scan
    work is concentrated in a few huge lists (two lists carry half of it on the bench index), which no placement of
    whole lists can balance."""
    return int(block) % max(int(world), 1)


def range_part_layout(cap: int):
    """one rank's radius result padded to `cap` entries, as the second all-gather of ShardedSearcher.range_search carries
    it: [D f32 cap | pad to 8 B | I i64 cap | tie u64 cap] (the layout idea of vi_packed_result_bytes) ->
    (byte offset of I, byte offset of tie, bytes in all).  Every block starts 8-byte aligned."""
    cap = int(cap)
    off_I = (cap * 4 + 7) // 8 * 8
    off_tie = off_I + cap * 8
    return off_I, off_tie, off_tie + cap * 8


def pack_range_part(cap: int, D, I, tie):
    """(D f32[n], I i64[n], tie i64[n] — the u64 bit pattern) tensors, n <= cap -> a uint8 tensor of
    range_part_layout(cap) bytes on their device; the padding is zero"""
    import torch
    off_I, off_tie, nbytes = range_part_layout(cap)
    n = int(D.shape[0])
    if n > cap or I.shape[0] != n or tie.shape[0] != n:
        raise ValueError("a part holds n entries of D, I and tie each, n <= cap")
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=D.device)
    if n:
        buf[:4 * n].view(torch.float32).copy_(D)
        buf[off_I:off_I + 8 * n].view(torch.int64).copy_(I)
        buf[off_tie:off_tie + 8 * n].view(torch.int64).copy_(tie)
    return buf


def unpack_range_part(buf, cap: int, n: int):
    """the first n entries of a packed part -> (D, I, tie) views of buf"""
    import torch
    off_I, off_tie, nbytes = range_part_layout(cap)
    if buf.numel() != nbytes or n > cap:
        raise ValueError("not a part packed for this cap")
    n = int(n)
    return (buf[:4 * n].view(torch.float32), buf[off_I:off_I + 8 * n].view(torch.int64),
            buf[off_tie:off_tie + 8 * n].view(torch.int64))


class ShardedSearcher:
    """local_search(xq, k, n_probe[, filter=]) -> (D, I, tie) tensors on this rank's device;
    merge(D_all, I_all, T_all) -> (D, I) with *_all shaped [world, nq, k].

    Radius search (both optional; range_search needs them):
    local_range_search(xq, radius2, n_probe[, filter=]) -> (lims i64[nq + 1], D f32[n], I i64[n], tie i64[n]) tensors on
    this rank's device, CSR, n = lims[nq], every row sorted by (distance bits, tie) (lims and tie: u64 bit patterns);
    merge_range(lims_all i64[world, nq + 1], packed u8[world, range_part_layout(cap)[2]], cap) -> the merged
    (lims, D, I, tie), rank r's part being unpack_range_part(packed[r], cap, lims_all[r, nq])."""

    def __init__(self, local_search, merge, group=None, local_range_search=None, merge_range=None):
        import torch.distributed as dist
        self._dist = dist
        self._local_search = local_search
        self._merge = merge
        self._group = group
        self.local_range_search = local_range_search
        self.merge_range = merge_range
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1

    def range_search(self, xq, radius2, n_probe, filter=None):
        """every probed candidate within radius2 over all ranks -> (lims, D, I, tie) as local_range_search gives them,
        equal to the unpartitioned index's result; world 1: the local result.  filter: this rank's own filter object
        (every rank makes its own from the same predicate).  Two all-gathers: the ranks' lims (which tell every rank
        every total), then one byte buffer per rank padded to the largest total (range_part_layout); the second and the
        merge are skipped when no rank found anything."""
        import torch
        if self.local_range_search is None or self.merge_range is None:
            raise RuntimeError("this ShardedSearcher was made without local_range_search / merge_range")
        kw = {} if filter is None else {"filter": filter}
        lims, D, I, T = self.local_range_search(xq, radius2, n_probe, **kw)
        if self.world == 1:
            return lims, D, I, T
        n1 = lims.shape[0]
        lims_all = torch.empty((self.world * n1,), dtype=lims.dtype, device=lims.device)
        self._dist.all_gather_into_tensor(lims_all, lims.contiguous(), group=self._group)
        lims_all = lims_all.view(self.world, n1)
        cap = int(lims_all[:, -1].max().item())
        if cap == 0:
            return lims, D, I, T       # (every rank's result is the empty one)
        mine = pack_range_part(cap, D, I, T)
        packed = torch.empty((self.world * mine.numel(),), dtype=torch.uint8, device=mine.device)
        self._dist.all_gather_into_tensor(packed, mine, group=self._group)
        return self.merge_range(lims_all, packed.view(self.world, mine.numel()), cap)

    def search(self, xq, k, n_probe, filter=None, rule=None):
        """filter: this rank's own filter object (every rank makes its own from the same predicate); it reaches
        local_search as the keyword `filter`, and only when given.  rule: a ProbeRule (ratio2 / n_probe_q; the same on
        every rank) — adaptive probing; it reaches local_search as the keyword `rule`, and only when given: the coarse
        step, the prune of its rows, then the list phase of this rank over the pruned rows"""
        import torch
        kw = {}
        if filter is not None:
            kw["filter"] = filter
        if rule is not None:
            kw["rule"] = rule
        D, I, T = self._local_search(xq, k, n_probe, **kw)
        if self.world == 1:
            return D, I
        nq, k = D.shape
        # concatenated output form (world*nq, k): accepted by both the RCCL and the gloo backend
        Dg = torch.empty((self.world * nq, k), dtype=D.dtype, device=D.device)
        Ig = torch.empty((self.world * nq, k), dtype=I.dtype, device=I.device)
        Tg = torch.empty((self.world * nq, k), dtype=T.dtype, device=T.device)
        self._dist.all_gather_into_tensor(Dg, D.contiguous(), group=self._group)
        self._dist.all_gather_into_tensor(Ig, I.contiguous(), group=self._group)
        self._dist.all_gather_into_tensor(Tg, T.contiguous(), group=self._group)
        shape = (self.world, nq, k)
        return self._merge(Dg.view(shape), Ig.view(shape), Tg.view(shape))


def gpu_searcher(index, device_index: int, group=None) -> ShardedSearcher:
    """ShardedSearcher over a vector_indexer_py.VectorIndex loaded with rank/world_size."""
    import torch
    from . import _native

    dev = torch.device("cuda", device_index)

    def gathered_probes(xq, n_probe):
        """the coarse step split over the ranks by query and all-gathered (the table is replicated: every rank computes
        the same rows), or run whole on this rank where the batch does not divide -> (probes, order, n_probe_eff)"""
        import torch.distributed as dist
        nq, dim = xq.shape
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        p_eff = min(int(n_probe), index.num_centroids)
        probes = torch.empty((nq, p_eff), dtype=torch.int32, device=dev)  # u32 bit patterns
        order = torch.empty((nq, p_eff), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # (xq may come from torch's stream)
        if world == 1 or nq % world:
            index.probe_device(xq.data_ptr(), nq, n_probe, probes.data_ptr(), order.data_ptr())
            return probes, order, p_eff
        per, r = nq // world, dist.get_rank(group)
        mine_p = torch.empty((per, p_eff), dtype=torch.int32, device=dev)
        mine_o = torch.empty((per, p_eff), dtype=torch.int32, device=dev)
        index.probe_device(xq.data_ptr() + r * per * dim * 4, per, n_probe, mine_p.data_ptr(), mine_o.data_ptr())
        dist.all_gather_into_tensor(probes, mine_p, group=group)
        dist.all_gather_into_tensor(order, mine_o, group=group)
        torch.cuda.synchronize(dev)
        return probes, order, p_eff

    def local_search(xq, k, n_probe, filter=None, rule=None):
        nq = xq.shape[0]
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        T = torch.empty((nq, k), dtype=torch.int64, device=dev)  # u64 bit pattern
        if rule is None:
            index.search_device(xq.data_ptr(), nq, k, n_probe, D.data_ptr(), I.data_ptr(), T.data_ptr(), filter=filter)
            return D, I, T
        # adaptive probing: the prune between the gathered probe step and this rank's list phase
        probes, order, p_eff = gathered_probes(xq, n_probe)
        index.prune_probes_device(xq.data_ptr(), nq, p_eff, probes.data_ptr(), order.data_ptr(), rule)
        index.search_probed_device(xq.data_ptr(), nq, k, p_eff, probes.data_ptr(), order.data_ptr(), D.data_ptr(), I.data_ptr(),
                                   T.data_ptr(), filter=filter)
        return D, I, T

    def to_tensors(res):
        """a native RangeResult's arrays copied into torch tensors (the exchange works on tensors), the result freed"""
        n, nq = res.total, res.nq
        out = (torch.empty(nq + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
        torch.cuda.synchronize(dev)
        res.copy_device(*[t.data_ptr() if t.numel() else 0 for t in out])
        res.free()
        return out

    def local_range_search(xq, radius2, n_probe, filter=None):
        torch.cuda.synchronize(dev)  # (xq may come from torch's stream)
        return to_tensors(index.range_search_device(xq.data_ptr(), xq.shape[0], radius2, n_probe, filter=filter))

    def merge_range(lims_all, packed, cap):
        from . import merge_range_results_device
        world, n1 = lims_all.shape
        off_I, off_tie, stride = range_part_layout(cap)
        lims_all, packed = lims_all.contiguous(), packed.contiguous()
        torch.cuda.synchronize(dev)  # (the all-gathers ran on torch's stream)
        base = [packed.data_ptr() + r * stride for r in range(world)]
        return to_tensors(merge_range_results_device(device_index, n1 - 1, [lims_all.data_ptr() + r * n1 * 8 for r in range(world)],
                                                     base, [b + off_I for b in base], [b + off_tie for b in base]))

    def merge(Dg, Ig, Tg):
        world, nq, k = Dg.shape
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        _native.check(_native.lib().vi_merge_partials_device(device_index, nq, k, world, Dg.data_ptr(), Ig.data_ptr(),
                                                             Tg.data_ptr(), D.data_ptr(), I.data_ptr()))
        return D, I

    return ShardedSearcher(local_search, merge, group, local_range_search, merge_range)


def merge_range_reference(parts):
    """numpy statement of the radius merge rule (used by the CPU protocol tests): parts = [(lims, D, I, tie), ...], CSR
    results of the same queries -> (lims u64, D, I, tie u64): per query the union of the parts' rows ordered by
    (distance bits, tie) — distances are >= +0 — and, for equal keys, by part"""
    parts = [(np.asarray(l).astype(np.uint64), np.asarray(d, dtype=np.float32), np.asarray(i, dtype=np.int64),
              np.asarray(t).view(np.uint64) if np.asarray(t).dtype == np.int64 else np.asarray(t, dtype=np.uint64))
             for l, d, i, t in parts]
    nq = parts[0][0].size - 1
    lims = np.zeros(nq + 1, dtype=np.uint64)
    for l, _, _, _ in parts:
        lims += l
    D, I, T = np.zeros(int(lims[-1]), np.float32), np.zeros(int(lims[-1]), np.int64), np.zeros(int(lims[-1]), np.uint64)
    for q in range(nq):
        rows = [(d[int(l[q]):int(l[q + 1])], i[int(l[q]):int(l[q + 1])], t[int(l[q]):int(l[q + 1])]) for l, d, i, t in parts]
        d, i, t = (np.concatenate([r[c] for r in rows]) for c in range(3))
        order = np.lexsort((t, d.view(np.uint32)))  # (stable: equal keys stay in part order)
        a, b = int(lims[q]), int(lims[q + 1])
        D[a:b], I[a:b], T[a:b] = d[order], i[order], t[order]
    return lims, D, I, T


def merge_partials_reference(Dg, Ig, Tg):
    """numpy statement of the merge rule (used by the CPU protocol tests)."""
    Dg, Ig = np.asarray(Dg), np.asarray(Ig)
    Tg = np.asarray(Tg).view(np.uint64) if np.asarray(Tg).dtype == np.int64 else np.asarray(Tg)
    world, nq, k = Dg.shape
    D = np.full((nq, k), np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        d, i, t = Dg[:, q].reshape(-1), Ig[:, q].reshape(-1), Tg[:, q].reshape(-1)
        live = i >= 0
        order = np.lexsort((t[live], d[live].view(np.uint32)))  # (dist bits, tie): dists are >= +0
        m = min(k, order.size)
        D[q, :m], I[q, :m] = d[live][order[:m]], i[live][order[:m]]
    return D, I


# =====================================================================================================================
# k-means with the points sharded over the GPUs of a node (X split N/world per GPU, centroids replicated)
# =====================================================================================================================
# The reference's k-means (src/kmeans.rs) is a single-process loop; what follows is the data-parallel form of it:
#
#   * the training loop of run_kmeans_mini_batch (k-means++ seeding, mini-batches, empty-cluster re-seeds) reads only
#     the rows its rand stream names; every rank replays that stream through vi_kmeans_mini_batch_train and the
#     named rows are exchanged by `comm.fetch_rows` (owners contribute their rows' bit patterns to an integer
#     all-reduce, which reproduces them exactly).  Rank 0's centroids are broadcast (RCCL broadcast of k x d f32),
#     then every rank assigns its own points: the O(N k D) part shards perfectly, labels never leave their rank.
#   * run_kmeans_parallel (Lloyd): per iteration local assign -> per-rank sums / counts -> all-reduce(sum) of
#     k x d f32 + k u32 -> means, re-seed of empty clusters (rows drawn from the replayed rand stream, fetched from
#     their owners), RMS movement, early stop — identical on every rank since all of it derives from all-reduced data.
#
# The arithmetic runs through the C ABI (`GpuKMeansEngine`); the collectives through a communicator object
# (`TorchComm`: torch.distributed — backend "nccl" is RCCL over xGMI on the GPU box, "gloo" in the CPU protocol test).
# Both are passed in, so the tests drive the same loops with N in-process ranks on one GPU and with a CPU engine.


class ShardedPoints:
    """this rank's slice of the points: rows [row_begin, row_begin + n_local) of the n_global x d f32 matrix, resident
    at device pointer `ptr` (`tensor` keeps a torch tensor alive / lets TorchComm index it)"""

    def __init__(self, ptr, n_local, d, row_begin, n_global, tensor=None):
        self.ptr, self.n_local, self.d = int(ptr), int(n_local), int(d)
        self.row_begin, self.n_global, self.tensor = int(row_begin), int(n_global), tensor


class GpuKMeansEngine:
    """the per-rank arithmetic of the sharded k-means, through the C ABI (raw device pointers)"""

    def __init__(self, device=0):
        from . import _native
        self.N, self.device = _native, int(device)

    def _source(self, fetch):
        N = self.N

        def cb(_ctx, rows_p, n_rows, out_dev):
            try:
                rows = np.ctypeslib.as_array(rows_p, shape=(int(n_rows),)).copy()
                fetch(rows, int(out_dev))
                return 0
            except Exception:  # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        fn = N.FETCH_ROWS_FN(cb)
        return N.RowSource(None, fn), fn

    def mini_batch_train(self, fetch, n_global, d, k, max_iters, thr, seed, C_ptr):
        import ctypes as C
        src, keep = self._source(fetch)
        it = C.c_uint64(0)
        self.N.check(self.N.lib().vi_kmeans_mini_batch_train(self.device, C.byref(src), n_global, d, k, max_iters,
                                                             -1.0 if thr is None else float(thr), seed, C_ptr, C.byref(it)))
        return int(it.value)

    def pp_init(self, fetch, n_global, d, k, seed, C_ptr):
        import ctypes as C
        src, keep = self._source(fetch)
        self.N.check(self.N.lib().vi_kmeans_pp_init(self.device, C.byref(src), n_global, d, k, seed, C_ptr))

    def assign(self, X_ptr, n_local, d, C_ptr, k, seed, mode, labels_ptr):
        self.N.check(self.N.lib().vi_assign_device(self.device, X_ptr, n_local, d, C_ptr, k, seed, mode, labels_ptr, None))

    def partial_sums(self, X_ptr, n_local, d, labels_ptr, k, sums_ptr, counts_ptr):
        self.N.check(self.N.lib().vi_kmeans_partial_sums_device(self.device, X_ptr, n_local, d, labels_ptr, k, sums_ptr,
                                                                counts_ptr))

    def finish_update(self, sums_ptr, counts_ptr, k, d, C_prev_ptr, C_new_ptr):
        import ctypes as C
        empties = np.zeros(k, dtype=np.uint32)
        ne = C.c_uint64(0)
        self.N.check(self.N.lib().vi_kmeans_finish_update_device(self.device, sums_ptr, counts_ptr, k, d, C_prev_ptr,
                                                                 C_new_ptr, None, empties.ctypes.data, C.byref(ne)))
        return empties[:ne.value]

    def centroid_delta(self, C_new_ptr, C_prev_ptr, k, d):
        import ctypes as C
        delta = C.c_float(0)
        self.N.check(self.N.lib().vi_kmeans_centroid_delta_device(self.device, C_new_ptr, C_prev_ptr, k, d, C.byref(delta)))
        return float(delta.value)

    def rng(self, seed):
        lib = self.N.lib()

        class _Rng:
            def __init__(s):
                s.h = lib.vi_rng_seed_from_u64(seed)

            def gen_range(s, lo, hi):
                return int(lib.vi_rng_gen_range(s.h, lo, hi))

            def __del__(s):
                if s.h:
                    lib.vi_rng_free(s.h)
                    s.h = None
        return _Rng()


class TorchComm:
    """collectives of the sharded k-means over torch.distributed.  Buffers are torch tensors on `device` ("cpu" with the
    gloo backend); the C library's own device buffers (fetch_rows' destination) are reached through the HIP runtime
    torch has loaded."""

    def __init__(self, device="cpu", group=None):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.group = torch, dist, group
        self.device = torch.device(device)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self._hip = None

    class Buf:
        def __init__(self, t):
            self.t, self.ptr = t, t.data_ptr()

    def alloc(self, nbytes):
        return TorchComm.Buf(self.torch.zeros(max(int(nbytes), 8) // 4 + 1, dtype=self.torch.int32, device=self.device))

    def all_reduce_sum(self, buf, count, kind):
        t = buf.t[:count] if kind == "u32" else buf.t[:count].view(self.torch.float32)
        self.dist.all_reduce(t, group=self.group)

    def broadcast(self, buf, nbytes, root=0):
        self.dist.broadcast(buf.t[:(nbytes + 3) // 4], src=root, group=self.group)

    def copy(self, dst_ptr, src_ptr, nbytes):
        import ctypes as C
        if self.device.type == "cpu":
            C.memmove(dst_ptr, src_ptr, nbytes)
            return
        if self._hip is None:
            self._hip = C.CDLL("libamdhip64.so")
            self._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.torch.cuda.synchronize(self.device)
        if self._hip.hipMemcpy(dst_ptr, src_ptr, nbytes, 3) != 0:
            raise RuntimeError("hipMemcpy (device to device) failed")

    def fetch_rows(self, pts, rows, out_ptr):
        """out[i] = data row rows[i]: every rank enters with the same rows; the owner of a row contributes its bit
        pattern, every other rank zeros, and the int32 sum over the ranks is the row, exactly"""
        torch = self.torch
        idx = torch.from_numpy(rows.astype(np.int64)).to(self.device)
        mine = (idx >= pts.row_begin) & (idx < pts.row_begin + pts.n_local)
        buf = torch.zeros((idx.numel(), pts.d), dtype=torch.int32, device=self.device)
        if pts.n_local:
            buf[mine] = pts.tensor.view(torch.int32)[idx[mine] - pts.row_begin]
        if self.world > 1:
            self.dist.all_reduce(buf, group=self.group)
        self.copy(out_ptr, buf.data_ptr(), buf.numel() * 4)


def kmeans_mini_batch_sharded(engine, comm, pts, k, max_iters, thr=None, seed=42, mode=0):
    """run_kmeans_mini_batch (src/kmeans.rs:64-150) over sharded points -> (centroids buffer k x d, labels buffer
    n_local u32, iterations).  Centroids are bit-identical to the single-GPU run (the training loop sees the same rows);
    labels are each rank's slice of the single-GPU labels."""
    d = pts.d
    Cb = comm.alloc(k * d * 4)
    iters = engine.mini_batch_train(lambda rows, out: comm.fetch_rows(pts, rows, out), pts.n_global, d, k, max_iters, thr,
                                    seed, Cb.ptr)
    comm.broadcast(Cb, k * d * 4, 0)  # every rank replayed the same stream; rank 0's copy pins the bits
    Lb = comm.alloc(max(pts.n_local, 1) * 4)
    if pts.n_local:
        engine.assign(pts.ptr, pts.n_local, d, Cb.ptr, k, seed, mode, Lb.ptr)
    return Cb, Lb, iters


def kmeans_parallel_sharded(engine, comm, pts, k, max_iters, thr=None, seed=42, mode=0):
    """run_kmeans_parallel (src/kmeans.rs:15-60) over sharded points: all-reduce of the per-rank sums / counts each
    iteration -> (centroids buffer, labels buffer, iterations)"""
    d, n = pts.d, pts.n_global
    thr = 1e-4 if thr is None else thr
    fetch = lambda rows, out: comm.fetch_rows(pts, rows, out)  # noqa: E731
    Cb, Cn = comm.alloc(k * d * 4), comm.alloc(k * d * 4)
    Sb, Nb = comm.alloc(k * d * 4), comm.alloc(k * 4)
    Lb = comm.alloc(max(pts.n_local, 1) * 4)
    engine.pp_init(fetch, n, d, k, seed, Cb.ptr)
    comm.broadcast(Cb, k * d * 4, 0)
    rng = engine.rng(seed)  # handle_empty_clusters draws from a stream of its own (kmeans.rs:31)
    it = 0
    while it < max_iters:
        if pts.n_local:  # (a rank without points — world > n, or an uneven split — contributes zero sums)
            engine.assign(pts.ptr, pts.n_local, d, Cb.ptr, k, seed, mode, Lb.ptr)
        engine.partial_sums(pts.ptr, pts.n_local, d, Lb.ptr, k, Sb.ptr, Nb.ptr)
        comm.all_reduce_sum(Sb, k * d, "f32")
        comm.all_reduce_sum(Nb, k, "u32")
        empties = engine.finish_update(Sb.ptr, Nb.ptr, k, d, Cb.ptr, Cn.ptr)
        if len(empties):  # kmeans.rs:313-331: a random data row for every cluster that received no point
            rows = np.array([rng.gen_range(0, n) for _ in empties], dtype=np.uint64)
            Rb = comm.alloc(len(rows) * d * 4)
            comm.fetch_rows(pts, rows, Rb.ptr)
            for i, c in enumerate(empties):
                comm.copy(Cn.ptr + int(c) * d * 4, Rb.ptr + i * d * 4, d * 4)
        delta = engine.centroid_delta(Cn.ptr, Cb.ptr, k, d)
        Cb, Cn = Cn, Cb
        it += 1
        if delta < thr:
            break
    return Cb, Lb, it
