"""Build-time gate for the int8 form of the streaming rank kernel (rank_stream.hip: rank_stream_i8_kernel).

Compiled to gfx950 assembly (no GPU needed): every instantiation multiplies with v_mfma_i32_32x32x32_i8 and never
touches scratch memory, and a step of the tile loop multiplies WITHOUT waiting for the tile it has just requested (no
`s_waitcnt vmcnt(0)` between a step's prefetch and its last MFMA: the hand-placed tile_landed_i8 touch keeps the wait in
front of the prefetch)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "vector-indexer_amd", "csrc", "rank_stream.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def i8_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa_i8") / "rank_stream.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
    subprocess.check_call([HIPCC, *flags, "--cuda-device-only", "-S", "-o", out, SRC], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"^(_ZN2vi12_GLOBAL__N_121rank_stream_i8_kernelILi(\d+)ELi(\d+)EEEvNS_16RankStreamI8ArgsE):[^\n]*\n(.*?)\n\.Lfunc_end",
                         text, re.S | re.M):
        name, nc, nu, body = m.groups()
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        ks[name] = dict(body=body, meta=meta, nc=int(nc), nu=int(nu))
    return ks


def test_int8_rank_kernels_use_the_int8_matrix_op_and_do_not_spill(i8_kernels):
    assert len(i8_kernels) == 8   # 1..4 chunks of 32 dimensions x {groups of 128, 256}
    for name, k in i8_kernels.items():
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", k["meta"]).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert not re.search(r"\bscratch_(load|store)|buffer_(load|store)", k["body"]), name
        mfmas = re.findall(r"v_mfma_\w+", k["body"])
        assert mfmas and set(mfmas) == {"v_mfma_i32_32x32x32_i8"}, f"{name}: {sorted(set(mfmas))}"


def test_int8_rank_kernel_multiplies_while_the_next_tile_loads(i8_kernels):
    checked = 0
    for name, k in i8_kernels.items():
        if k["nu"] != 4:
            continue
        lines = k["body"].split("\n")
        tile_loads = [i for i, l in enumerate(lines) if "global_load_dwordx4" in l]
        mfmas = [i for i, l in enumerate(lines) if "v_mfma_i32_32x32x32_i8" in l]
        steps = 0
        for i in tile_loads:
            nxt = [m for m in mfmas if m > i]
            if not nxt or any(i < t < nxt[0] for t in tile_loads):
                continue   # not the last load of its run
            chain = [m for m in nxt if m < i + 600][: k["nc"] * 4]
            if len(chain) < k["nc"]:
                continue
            between = "\n".join(lines[i + 1:chain[-1]])
            if "s_barrier" in between:
                continue   # (the run in front of the item loop)
            assert not re.search(r"s_waitcnt[^\n]*vmcnt\(0\)", between), f"{name}: a step drains vector memory after its prefetch"
            steps += 1
        assert steps >= 2, name   # the two halves of the unrolled tile loop
        checked += 1
    assert checked == 4
