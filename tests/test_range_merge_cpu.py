"""CPU: the multi-GPU radius search without a GPU — vi_range_merge_device's ABI and argument checks, the numpy statement of
the merge rule against the oracle on the tie fixture, the exchange of ShardedSearcher.range_search over gloo (world 2) with
the oracle as every rank's searcher, the packed part layout, and range_merge.hip compiled to gfx950 assembly."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import range_merge_cases as RC
from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32
PROTOTYPE = (C.c_int, [i32, u64, u32, vp, vp, vp, vp, C.POINTER(vp)])


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_the_symbol_resolves_with_the_documented_prototype():
    fn = N.lib().vi_range_merge_device      # AttributeError: not exported
    assert fn.restype == PROTOTYPE[0] and list(fn.argtypes) == PROTOTYPE[1]
    assert N.SIGNATURES["vi_range_merge_device"] == PROTOTYPE


def test_the_header_declares_it_and_the_abi_version_is_2():
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().split())
    assert ("vi_status vi_range_merge_device(int32_t device, uint64_t nq, uint32_t parts, const uint64_t *const *lims_dev, "
            "const float *const *D_dev, const int64_t *const *I_dev, const uint64_t *const *tie_dev, vi_range_result **out);") in flat
    assert "#define VI_AMD_ABI_VERSION 2" in flat
    assert N.lib().vi_abi_version() == 2


def _arrays(parts, null=None):
    """four host arrays of `parts` made-up non-null device pointers (never followed: the checks come first); null = (array
    number, part) to zero"""
    cols = [(vp * max(parts, 1))(*[0x1000 * (a + 1) + 0x100 * p for p in range(parts)]) for a in range(4)]
    if null is not None:
        cols[null[0]][null[1]] = None
    return cols


def test_bad_arguments_are_invalid_input_before_any_device_work():
    L = N.lib()
    out = vp(0xdead)

    def call(parts, cols, outp=None):
        return L.vi_range_merge_device(0, 5, parts, *cols, C.byref(out) if outp is None else outp)

    assert L.vi_range_merge_device(0, 5, 2, *_arrays(2), None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()   # null out
    for a in range(4):                                                                                             # a null array
        cols = _arrays(2)
        cols[a] = None
        out.value = 0xdead
        assert call(2, cols) == N.VI_ERR_INVALID_INPUT and L.vi_last_error() and not out.value, a
    for parts in (0, 65, 1 << 31):                                                                                 # parts
        cols = _arrays(min(parts, 65))
        assert call(parts, cols) == N.VI_ERR_INVALID_INPUT and L.vi_last_error(), parts
        assert b"parts" in L.vi_last_error()
    for a in range(4):                                                                   # a null lims / D / I / tie pointer
        for p in (0, 63):
            out.value = 0xdead
            assert call(64, _arrays(64, null=(a, p))) == N.VI_ERR_INVALID_INPUT and not out.value, (a, p)
            assert ("part %d" % p).encode() in L.vi_last_error()


def test_a_well_formed_call_without_its_device_is_a_device_error():
    """no device at all (device 0 where none is visible), or an ordinal out of range (anywhere): never a CPU fallback"""
    L = N.lib()
    for device in [10_000, -1] + ([0] if L.vi_device_count() <= 0 else []):
        out = vp(0xdead)
        assert L.vi_range_merge_device(device, 5, 2, *_arrays(2), C.byref(out)) == N.VI_ERR_DEVICE, device
        assert L.vi_last_error() and not out.value


# ---- the merge rule in numpy against the oracle ---------------------------------------------------------------------------
class Tie:
    """the tie fixture built by the oracle; per n_probe the oracle's full sorted sequences and, per world, every rank's"""

    def __init__(self, root):
        import oracle_lib as O
        self.X, self.Q = RC.tie_data()
        self.n = self.X.shape[0]
        self.idx, self.sh = os.path.join(root, "index"), os.path.join(root, "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, nlist=RC.NLIST)
        self._full, self._part = {}, {}

    def full(self, p):
        if p not in self._full:
            rc, D, I = self.orc.search_batch(self.Q, self.n, p)
            assert rc == 0
            self._full[p] = (D, I)
        return self._full[p]

    def partial(self, p, rank, world):
        if (p, rank, world) not in self._part:
            self._part[p, rank, world] = self.orc.search_partial_batch(self.Q, self.n, p, rank, world)
        return self._part[p, rank, world]


@pytest.fixture(scope="module")
def tie(tmp_path_factory):
    return Tie(str(tmp_path_factory.mktemp("tie")))


def test_the_fixture_is_what_the_tests_need(tie):
    assert tie.orc.num_shards == 3
    lens = [int(tie.orc.list_len(c)) for c in range(tie.orc.num_centroids)]
    assert len(lens) == RC.NLIST and min(lens) > 8 * 64, lens      # more than 8 blocks: every rank of 8 holds a stripe of every list


@pytest.mark.parametrize("world", RC.WORLDS)
@pytest.mark.parametrize("n_probe", RC.PROBES)
def test_merge_range_reference_gives_the_oracles_full_sequence(tie, n_probe, world):
    from vector_indexer_py.distributed import merge_range_reference
    D, I = tie.full(n_probe)
    for name, r in RC.radii(D, I).items():
        want = RC.cut(r, D, I)
        parts = [RC.cut(r, *tie.partial(n_probe, rank, world)) for rank in range(world)]
        assert all(int(p[0][-1]) > 0 for p in parts), (name, [int(p[0][-1]) for p in parts])    # every rank holds part of the answer
        if name == "r10" and world >= 4:
            assert RC.empty_rows(parts) > 0
        assert RC.queries_with_cross_rank_ties(parts) >= len(tie.Q) // 2
        got = merge_range_reference(parts)
        assert got[0].dtype == np.uint64 and got[3].dtype == np.uint64
        RC.same(got, want, tie=False)
        assert int(got[0][-1]) == sum(int(p[0][-1]) for p in parts)


def test_merge_range_reference_puts_equal_keys_in_part_order():
    from vector_indexer_py.distributed import merge_range_reference
    a = (np.array([0, 2], np.uint64), np.array([1.0, 2.0], np.float32), np.array([10, 11]), np.array([5, 5], np.uint64))
    b = (np.array([0, 2], np.uint64), np.array([1.0, 2.0], np.float32), np.array([20, 21]), np.array([5, 5], np.uint64))
    lims, D, I, T = merge_range_reference([a, b])
    assert lims.tolist() == [0, 4] and I.tolist() == [10, 20, 11, 21] and D.tolist() == [1.0, 1.0, 2.0, 2.0]


# ---- the exchange over gloo -------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, work):
    import torch
    import torch.distributed as dist
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "vector-indexer_amd")]
    import oracle_lib as O
    import range_merge_cases as RC
    from vector_indexer_py import distributed as VD

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    orc = O.OracleIndex.load(os.path.join(work, "index"), os.path.join(work, "shards"))
    Q = np.load(os.path.join(work, "q.npy"))
    n = int(np.load(os.path.join(work, "n.npy")))
    calls = []

    def local_search(*args, **kw):
        calls.append((args, kw))
        xq, k, n_probe = args
        D, I, T = orc.search_partial_batch(xq.numpy(), k, n_probe, rank, world)
        return torch.from_numpy(D), torch.from_numpy(I), torch.from_numpy(T.view(np.int64))

    def merge(Dg, Ig, Tg):
        D, I = VD.merge_partials_reference(Dg.numpy(), Ig.numpy(), Tg.numpy())
        return torch.from_numpy(D), torch.from_numpy(I)

    def local_range_search(xq, radius2, n_probe):
        lims, D, I, T = RC.cut(radius2, *orc.search_partial_batch(xq.numpy(), n, n_probe, rank, world))
        return (torch.from_numpy(lims.view(np.int64)), torch.from_numpy(D), torch.from_numpy(I), torch.from_numpy(T.view(np.int64)))

    merges = []

    def merge_range(lims_all, packed, cap):
        merges.append(cap)
        assert lims_all.shape == (world, Q.shape[0] + 1) and packed.shape == (world, VD.range_part_layout(cap)[2])
        assert cap == int(lims_all[:, -1].max())
        parts = []
        for r in range(world):
            D, I, T = VD.unpack_range_part(packed[r], cap, int(lims_all[r, -1]))
            parts.append((lims_all[r].numpy().view(np.uint64), D.numpy(), I.numpy(), T.numpy()))
        return tuple(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a) for a in VD.merge_range_reference(parts))

    s = VD.ShardedSearcher(local_search, merge, None, local_range_search, merge_range)
    assert s.world == world
    res = {}
    for name, r in [("r10", float(np.load(os.path.join(work, "r10.npy")))), ("inf", RC.INF), ("neg", -1.0)]:
        before = len(merges)
        lims, D, I, T = s.range_search(torch.from_numpy(Q), r, 3)
        assert (len(merges) == before) == (name == "neg")       # nothing found anywhere: no second gather, no merge
        res[f"lims_{name}"], res[f"D_{name}"], res[f"I_{name}"] = lims.numpy(), D.numpy(), I.numpy()
    # a filter reaches local_search as a keyword, and only when given
    tok = object()
    s.search(torch.from_numpy(Q), 5, 3)
    assert len(calls[-1][0]) == 3 and calls[-1][1] == {}
    s.search(torch.from_numpy(Q), 5, 3, filter=tok)
    assert len(calls[-1][0]) == 3 and list(calls[-1][1]) == ["filter"] and calls[-1][1]["filter"] is tok
    np.savez(os.path.join(work, f"out_{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_range_search_protocol_gloo_world2(tie):
    import torch.multiprocessing as mp
    work = os.path.dirname(tie.idx)
    D, I = tie.full(3)
    r10 = RC.radii(D, I)["r10"]
    np.save(os.path.join(work, "q.npy"), tie.Q)
    np.save(os.path.join(work, "n.npy"), np.array(tie.n))
    np.save(os.path.join(work, "r10.npy"), np.array(r10))
    mp.spawn(_worker, args=(2, _free_port(), work), nprocs=2, join=True)
    for rank in range(2):          # every rank holds the merged result
        got = np.load(os.path.join(work, f"out_{rank}.npz"))
        for name, r in [("r10", r10), ("inf", RC.INF), ("neg", -1.0)]:
            want = RC.cut(r, D, I)
            assert (int(want[0][-1]) == 0) == (name == "neg")
            RC.same((got[f"lims_{name}"].view(np.uint64), got[f"D_{name}"], got[f"I_{name}"]), want, tie=False)


def test_three_argument_callers_keep_working_and_range_search_needs_its_closures():
    import torch
    from vector_indexer_py.distributed import ShardedSearcher
    seen = []
    s = ShardedSearcher(lambda xq, k, p: seen.append((xq, k, p)) or (torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, 2)),
                        lambda *a: None)
    assert s.world == 1 and len(s.search(torch.zeros(1, 3), 2, 1)) == 2 and seen[0][1:] == (2, 1)
    with pytest.raises(RuntimeError):
        s.range_search(torch.zeros(1, 3), 1.0, 1)
    local = (torch.zeros(2, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    s = ShardedSearcher(None, None, None, lambda xq, r, p, **kw: seen.append(kw) or local, lambda *a: None)
    got = s.range_search(torch.zeros(1, 3), 1.0, 1, filter="f")
    assert all(a is b for a, b in zip(got, local)) and seen[-1] == {"filter": "f"}       # world 1: the local result
    s.range_search(torch.zeros(1, 3), 1.0, 1)
    assert seen[-1] == {}


# ---- the packed part ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1, 7, 1001])
def test_range_part_layout_round_trip(cap):
    import torch
    from vector_indexer_py.distributed import pack_range_part, range_part_layout, unpack_range_part
    off_I, off_tie, nbytes = range_part_layout(cap)
    assert off_I % 8 == 0 and off_tie % 8 == 0 and nbytes % 8 == 0
    assert off_I >= 4 * cap and off_tie == off_I + 8 * cap and nbytes == off_tie + 8 * cap and off_I - 4 * cap < 8
    rng = np.random.default_rng(cap)
    for n in sorted({0, cap // 2, cap}):
        D = rng.standard_normal(n).astype(np.float32)
        I = rng.integers(0, 1 << 63, size=n, dtype=np.uint64).view(np.int64) * 2 + 1      # ids past 2^63 as i64 bit patterns
        T = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        buf = pack_range_part(cap, torch.from_numpy(D), torch.from_numpy(I), torch.from_numpy(T.view(np.int64)))
        assert buf.dtype == torch.uint8 and buf.shape == (nbytes,)
        raw = buf.numpy()
        assert np.array_equal(raw[:4 * n].view(np.uint32), D.view(np.uint32))              # the layout itself, not only the round trip
        assert np.array_equal(raw[off_I:off_I + 8 * n].view(np.int64), I) and np.array_equal(raw[off_tie:off_tie + 8 * n].view(np.uint64), T)
        assert not raw[4 * n:off_I].any() and not raw[off_I + 8 * n:off_tie].any() and not raw[off_tie + 8 * n:].any()
        d, i, t = unpack_range_part(buf, cap, n)
        assert np.array_equal(d.numpy().view(np.uint32), D.view(np.uint32)) and np.array_equal(i.numpy(), I)
        assert np.array_equal(t.numpy().view(np.uint64), T)
    with pytest.raises(ValueError):
        pack_range_part(cap, torch.zeros(cap + 1), torch.zeros(cap + 1, dtype=torch.int64), torch.zeros(cap + 1, dtype=torch.int64))


# ---- range_merge.hip compiled to gfx950 assembly (no GPU needed) ---------------------------------------------------------------
SRC = os.path.join(ROOT, "vector-indexer_amd", "csrc", "range_merge.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("range_merge_lims_kernel", "range_merge_place_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> (kernel descriptor, resource-usage comment block); only the metadata is read"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "range_merge.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
    subprocess.check_call([HIPCC, *flags, "--cuda-device-only", "-S", "-o", out, SRC], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_ZN2vi\w*?(?:%s)\w*):[^\n]*\n.*?\n\.Lfunc_end" % "|".join(KERNELS), text, re.S | re.M):
        name = m.group(1)
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        found[name] = (meta, text[m.end():].split("\n_ZN", 1)[0])
    return found


def test_both_kernels_are_there_without_scratch_or_spills(kernels):
    for k in KERNELS:
        assert sum(k in name for name in kernels) == 1, (k, sorted(kernels))
    for name, (meta, usage) in kernels.items():
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert re.search(r";\s*ScratchSize:\s*\d+", usage), f"{name}: no resource usage found"
        for what in ("ScratchSize", "SGPRSpill", "VGPRSpill", r"\.sgpr_spill_count", r"\.vgpr_spill_count"):
            for m in re.finditer(r"%s:\s*(\d+)" % what, usage):
                assert int(m.group(1)) == 0, f"{name}: {what} {m.group(1)}"
