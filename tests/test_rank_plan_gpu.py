"""Which rank kernel a search takes (mfma_search.hip: the rank plan), pinned route by route: for every way through the
plan the triple (rank_mode, group_queries, rank_int8) of `last_stats()` is the one listed here, and the result is the
oracle's, ids and distance bits.  Three small indexes, built once: 8-bit descriptors (hi planes only, streaming kernel,
int8 products for integer batches), real-valued lists (bf16 x 3 or, asked for, their hi planes; about the origin or about
their mean: VI_CENTER is read when the index is loaded), and wide vectors (the GEMM-shaped kernel, always groups of 128)."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip

pytestmark = pytest.mark.gpu

KNOBS = ("VI_FILTER", "VI_FILTER_BF16", "VI_FILTER_HI_ONLY", "VI_FILTER_GQ", "VI_RANK_STREAM", "VI_STREAM_GQ", "VI_RANK_I8",
         "VI_RANK_APPROX", "VI_CENTER", "VI_FORCE_GENERIC", "VI_STREAM_PROF")
K, N_PROBE = 10, 8


@pytest.fixture(autouse=True)
def _no_knobs_from_outside():
    if any(name in os.environ for name in KNOBS):
        pytest.skip("the engine knobs are set in the environment: the plan is not the one pinned here")
    yield


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    """an index on both sides and the oracle's answer to each of its query batches, computed once"""

    def __init__(self, root, X, batches, centre=("",)):
        idx, sh = str(root / "index"), str(root / "shards")
        self.orc = O.OracleIndex.build(X, idx, sh, nlist=0, seed=42)
        self.gpu = {}
        for c in centre:   # VI_CENTER is a load-time option
            with pytest.MonkeyPatch.context() as mp:
                if c:
                    mp.setenv("VI_CENTER", c)
                self.gpu[c] = vip.load(idx, sh, X.shape[1])
        self.batches = {}
        for name, Q in batches.items():
            rc, Do, Io = self.orc.search_batch(Q, K, N_PROBE)
            assert rc == O.ORC_OK
            self.batches[name] = (Q, Do, Io)

    def search(self, batch, centre=""):
        """one search, compared as test_search_gpu.check_parity compares; returns the stats of that search"""
        Q, Do, Io = self.batches[batch]
        gpu = self.gpu[centre]
        Dg, Ig = gpu.search_sync(Q, K, N_PROBE)
        assert Ig.shape == (Q.shape[0], K) and Dg.dtype == np.float32 and Ig.dtype == np.int64
        bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}"
        return gpu.last_stats()


@pytest.fixture(scope="module")
def bytes_index(tmp_path_factory):
    rng = np.random.default_rng(128)
    X = rng.integers(0, 201, size=(6000, 128)).astype(np.float32)
    Qi = np.ascontiguousarray(X[rng.integers(0, 6000, 300)] + rng.integers(-3, 4, size=(300, 128)), dtype=np.float32).clip(0, 200)
    Qf = np.ascontiguousarray(Qi[:100] + rng.random((100, 128), dtype=np.float32) * 0.37, dtype=np.float32)
    return Case(tmp_path_factory.mktemp("bytes"), X, {"integer": Qi, "non-integer": Qf})


@pytest.fixture(scope="module")
def real_index(tmp_path_factory):
    rng = np.random.default_rng(32)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    Q = np.concatenate([rng.standard_normal((120, 32)).astype(np.float32), X[:8]])
    return Case(tmp_path_factory.mktemp("real"), X, {"real": np.ascontiguousarray(Q)}, centre=("0", "1"))


@pytest.fixture(scope="module")
def wide_index(tmp_path_factory):
    rng = np.random.default_rng(144)
    X = rng.standard_normal((3000, 144)).astype(np.float32)
    Q = np.concatenate([rng.standard_normal((60, 144)).astype(np.float32), X[:4]])
    return Case(tmp_path_factory.mktemp("wide"), X, {"wide": np.ascontiguousarray(Q)})


def triple(st, group_queries=True, rank_int8=True):
    return (st["rank_mode"], st["group_queries"] if group_queries else None, st["rank_int8"] if rank_int8 else None)


@pytest.mark.parametrize("knobs,batch,want", [
    ({}, "integer", (3, 128, 1)),                                        # streaming kernel, int8 products
    ({}, "non-integer", (3, 128, 0)),                                    # streaming kernel, bf16 (queries hi + lo)
    ({"VI_RANK_I8": "0"}, "integer", (3, 128, 0)),
    ({"VI_RANK_STREAM": "0", "VI_FILTER_GQ": "32"}, "integer", (3, 32, 0)),    # block-synchronous kernel, one wave per item
    ({"VI_RANK_STREAM": "0", "VI_FILTER_GQ": "128"}, "integer", (3, 128, 0)),
    ({"VI_FILTER_HI_ONLY": "0"}, "integer", (2, None, 0)),               # bf16 x 3
    ({"VI_FILTER_BF16": "0"}, "integer", (1, None, 0)),                  # f32 MFMA
    ({"VI_FILTER": "0"}, "integer", (0, None, 0)),                       # exact-order VALU engine
], ids=lambda v: "+".join(f"{k}={x}" for k, x in v.items()) or "default" if isinstance(v, dict) else None)
def test_routes_of_8_bit_descriptors(knobs, batch, want, bytes_index, monkeypatch):
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    st = bytes_index.search(batch)
    got = triple(st, group_queries=want[1] is not None)
    print("plan", knobs, batch, triple(st))
    assert got == want, st


def test_groups_of_256_from_the_second_integer_batch(bytes_index, monkeypatch):
    """VI_STREAM_GQ=256: groups of 256 once the handle has seen a batch of bf16-exact queries"""
    monkeypatch.setenv("VI_STREAM_GQ", "256")
    bytes_index.search("integer")
    st = bytes_index.search("integer")
    print("plan", "VI_STREAM_GQ=256", triple(st))
    assert triple(st) == (3, 256, 1), st


def test_streaming_kernel_profile_is_printed_and_the_search_unchanged(bytes_index, monkeypatch, capfd):
    """VI_STREAM_PROF=1: the streaming bf16 kernel counts into its profile block and the pipeline prints it behind the
    kernel (rank_stream.hip: print_rank_stream_profile); route and result stay what they are without it"""
    monkeypatch.setenv("VI_STREAM_PROF", "1")
    st = bytes_index.search("non-integer")
    err = capfd.readouterr().err
    print("plan", "VI_STREAM_PROF=1", triple(st))
    assert triple(st) == (3, 128, 0), st
    assert any(line.startswith("rank_stream wave-0 ticks") for line in err.splitlines()), err


@pytest.mark.parametrize("centre,approx,mode", [("0", "0", 2), ("0", "1", 4), ("1", "0", 5), ("1", "2", 6)])
def test_routes_of_real_valued_lists(centre, approx, mode, real_index, monkeypatch):
    monkeypatch.setenv("VI_RANK_APPROX", approx)
    st = real_index.search("real", centre)
    print("plan", centre, approx, triple(st))
    assert st["rank_mode"] == mode, st


def test_wide_vectors_always_rank_in_groups_of_128(wide_index, monkeypatch):
    monkeypatch.setenv("VI_FILTER_GQ", "32")
    st = wide_index.search("wide")
    print("plan", "wide", triple(st))
    assert triple(st, rank_int8=False) == (2, 128, None), st
