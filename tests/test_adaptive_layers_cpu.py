"""CPU: the Python layers above the adaptive-probing entries hand the rule down and leave a call without a rule exactly as
it was: SearchRequest.with_probe_ratio / .with_max_codes, FaissStyleAdapter.max_codes / .probe_ratio2,
ShardedSearcher.search(rule=) and ProbeRule's own conversion.  (No GPU: the index below is a recorder.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import vector_indexer_py as vip
from vector_indexer_py.api import SearchRequest
from vector_indexer_py.harness import FaissStyleAdapter


class Recorder:
    """stands in for a VectorIndex: remembers how it was searched"""
    dimension = 4

    def __init__(self):
        self.calls = []

    def search_sync(self, xq, k, n_probe, **kw):
        self.calls.append(("plain", k, n_probe, kw))
        return np.zeros((len(xq), k), np.float32), np.zeros((len(xq), k), np.int64)

    def search_adaptive_sync(self, xq, k, n_probe, rule, **kw):
        self.calls.append(("adaptive", k, n_probe, rule, kw))
        return np.zeros((len(xq), k), np.float32), np.zeros((len(xq), k), np.int64)


def test_search_request_carries_the_rule_and_defaults_to_none():
    req = SearchRequest([0.0] * 4)
    assert (req.probe_ratio2, req.min_probe, req.max_codes) == (0.0, 1, 0)
    r2 = req.with_probe_ratio(1.5, min_probe=3).with_max_codes(5000).with_k(7)
    assert (r2.probe_ratio2, r2.min_probe, r2.max_codes, r2.k) == (1.5, 3, 5000, 7)
    assert (req.probe_ratio2, req.min_probe, req.max_codes) == (0.0, 1, 0)      # a request is not changed in place
    assert req.with_probe_ratio(2.0).min_probe == 1


def test_adapter_reads_its_two_attributes_at_every_search():
    idx = Recorder()
    ad = FaissStyleAdapter(idx)
    assert (ad.max_codes, ad.probe_ratio2) == (0, 0.0)
    ad.nprobe = 16
    xq = np.zeros((3, 4), np.float32)
    ad.search(xq, 5)
    assert idx.calls[-1] == ("plain", 5, 16, {})
    ad.max_codes = 4000
    ad.search(xq, 5)
    kind, k, n_probe, rule, kw = idx.calls[-1]
    assert (kind, k, n_probe, kw) == ("adaptive", 5, 16, {"filter": None})
    assert (rule.min_probe, rule.ratio2, rule.max_codes, rule.n_probe_q) == (1, 0.0, 4000, None)
    ad.max_codes, ad.probe_ratio2 = 0, 1.25
    ad.search(xq, 5)
    assert idx.calls[-1][0] == "adaptive" and idx.calls[-1][3].ratio2 == 1.25 and idx.calls[-1][3].max_codes == 0
    ad.probe_ratio2 = 0.0
    ad.search(xq, 5)
    assert idx.calls[-1] == ("plain", 5, 16, {})


SHARDED = """
import vector_indexer_py as vip
from vector_indexer_py.distributed import ShardedSearcher
seen = []
def local_search(xq, k, n_probe, **kw):
    seen.append(kw)
    return "D", "I", "T"
s = ShardedSearcher(local_search, merge=None)
assert s.world == 1
rule = vip.ProbeRule(ratio2=1.5)
assert s.search(None, 5, 8) == ("D", "I") and seen[-1] == {}
assert s.search(None, 5, 8, rule=rule) == ("D", "I") and seen[-1] == {"rule": rule}
s.search(None, 5, 8, filter="f", rule=rule)
assert seen[-1] == {"filter": "f", "rule": rule}
s.search(None, 5, 8, filter="f")
assert seen[-1] == {"filter": "f"}
print("ok")
"""


def test_sharded_searcher_hands_the_rule_to_the_local_search_only_when_given():
    """in a process of its own: ShardedSearcher imports torch, whose HIP runtime must not be the test process's first"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    run = subprocess.run([sys.executable, "-c", SHARDED], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_probe_rule_conversion():
    r, keep = vip.ProbeRule()._native_rule(4, device=False)
    assert (r.min_probe, r.ratio2, r.max_codes, r.n_probe_q, keep) == (1, 0.0, 0, None, None)
    r, keep = vip.ProbeRule(n_probe_q=np.array([4, 0, 9], dtype=np.int64))._native_rule(3, device=False)
    assert keep.dtype == np.uint32 and keep.tolist() == [4, 0, 9] and r.n_probe_q == keep.ctypes.data
    with pytest.raises(RuntimeError):
        vip.ProbeRule(n_probe_q=[1, 2])._native_rule(3, device=False)       # one count per query
    r, keep = vip.ProbeRule(n_probe_q=0x7F0000001000)._native_rule(3, device=True)
    assert r.n_probe_q == 0x7F0000001000 and keep is None
    with pytest.raises(TypeError):
        vip.ProbeRule(n_probe_q=[1, 2, 3])._native_rule(3, device=True)     # a device call takes an address
